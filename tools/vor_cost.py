#!/usr/bin/env python3
"""What transdimensional Voronoi-cell models cost: needs a GPU.

  raster   the raster kernel alone at the headline shape (C3: 1024 chains x
           32 768 cells), every model holding k = 16, 128 and 512 nuclei, timed
           with device events: a warm-up, then --launches rasters of every
           model back to back (Sampler.vor_rasterize; no FSM in the timed
           window).  Prints ms per raster, the bytes moved (per model 12 B per
           cell written -- v and both slowness rows; a Voronoi step's own raster
           writes 8 -- and 8 B per nucleus read by each of its cell tiles),
           bytes/s against the 8 TB/s of the project's roofline, the nucleus-
           cell pairs compared per second, and the share of one C3 step.
  step     a Voronoi step against a single-cell step at 40 x 40 x 24 and 64^3
           nodes (8 stations, 16 events, cells of 4 x 4 x 4 nodes, fp32) with 8
           and 64 chains: a host clock around each `run(1)` that ends in a
           device synchronise, after a warm-up, the median.  Each measurement
           is a process of its own; with --parent DIR (a built checkout of the
           parent commit) the single-cell step is the parent's, and the two
           alternate for --rounds rounds.  Without it the single-cell step is
           this tree's with the models off.  (A single-cell sampler of these
           sizes may run multi-step launches; `multi_step` is reported.)  The
           device time of the FSM launches and the sweep iterations per step
           are reported beside it: a rastered model is piecewise constant with
           sharp contrasts, and what its forward costs is part of the answer.

One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_BYTES_S = 8e12                     # the roofline's HBM figure (bench.py)
C3_STEP_MS = 1565.0                     # BENCH_r06.json rank_step_ms
TILE = 1024                             # cells per raster workgroup (csrc/vor.h VOR_TILE)


def problem(mcmc, shape, nstat, nev):
    nx, ny, nz = shape
    p = mcmc.make_problem("C2", n=nx, nstat=nstat, nev=nev)
    if (ny, nz) != (nx, nx):
        p.ny, p.nz = ny, nz
        p.sz[:] = (nz - 1) * p.h
        p.ez = np.clip(p.ez, p.h, (nz - 2) * p.h)
        p.v_true = mcmc.cell_velocity(p)
    return p


def raster_cost(args):
    import torch
    from mceik_amd import mcmc
    p = mcmc.make_problem(args.config, picks="analytic")
    nch = args.chains or mcmc.CONFIGS[args.config]["nchains"]
    smp = mcmc.Sampler(p, nchains=nch)
    stream = torch.cuda.current_stream()
    smp.set_stream(stream.cuda_stream)
    nph, ncell = max(1, p.nphase), p.ncell
    g = np.random.default_rng(1)
    for k in (16, 128, 512):
        cells = np.zeros((nch, nph, 512), np.int32)
        for c in range(nch):
            for ph in range(nph):
                cells[c, ph, :k] = g.choice(ncell, k, replace=False)
        vals = g.integers(p.vmin, p.vmax + 1, cells.shape).astype(np.int32)
        smp.vor_enable(kmin=1, kmax=512, nuclei=(cells, vals, np.full((nch, nph), k, np.int32)))
        for _ in range(args.warmup):
            smp.vor_rasterize()
        smp.sync()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(args.launches):
            smp.vor_rasterize()
        ev1.record(stream)
        ev1.synchronize()
        ms = ev0.elapsed_time(ev1) / args.launches
        rows, tiles = nch * nph, -(-ncell // TILE)
        nbytes = rows * (12 * ncell + 8 * k * tiles)
        print(json.dumps({"what": "raster", "config": args.config, "chains": nch, "ncell": ncell, "k": k,
                          "launches": args.launches, "ms_per_raster": round(ms, 4), "bytes_per_raster": int(nbytes),
                          "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                          "frac_of_8TBs": round(nbytes / (ms * 1e-3) / PEAK_BYTES_S, 4),
                          "pairs_per_s": round(rows * ncell * k / (ms * 1e-3), 0),
                          "share_of_c3_step": round(ms / C3_STEP_MS, 6)}), flush=True)
    smp.close()


def one_step_cost(args):
    """The child process of `step`: one sampler of --root's library, one kind of step."""
    sys.path.insert(0, os.path.abspath(args.root))
    from mceik_amd import mcmc
    shape = tuple(int(x) for x in args.shape.split("x"))
    p = problem(mcmc, shape, args.nstat, args.nev)
    smp = mcmc.Sampler(p, nchains=args.chains)
    if args.kind == "voronoi":
        smp.vor_enable(kmin=1, kmax=args.kmax, k0=args.k0)
    smp.run(args.warmup)
    smp.sync()
    smp.fsm_stats(reset=True)
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        smp.run(1)
        smp.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    info = smp.info()
    fsm_ms, nlaunch, iters, visits = smp.fsm_stats()
    out = {"what": "step", "kind": args.kind, "root": os.path.abspath(args.root), "grid": list(shape),
           "ncell": int(p.ncell), "chains": args.chains, "npipe": info["npipe"], "multi_step": info["multi_step"],
           "ms_step": round(float(np.median(ms)), 3), "ms_all": [round(x, 3) for x in ms],
           # the forward's share: device time of the FSM launches and sweep iterations, per step (means)
           "ms_fsm_per_step": round(fsm_ms / args.steps, 3), "fsm_launches": int(nlaunch),
           "sweep_iterations_per_step": round(int(iters) / args.steps, 1),
           "brick_visits_per_step": round(int(visits[0]) / args.steps, 1),
           "segments_updated_per_step": round(int(visits[1]) / args.steps, 1)}
    if args.kind == "voronoi":
        st = smp.vor_stats()
        out["k0"], out["kmax"] = args.k0, args.kmax
        out["acceptance"] = {t: round(st[t]["accepts"] / max(st[t]["attempts"], 1), 3) for t in st}
        out["k_mean"] = round(float(smp.vor_get()[2].mean()), 2)
    smp.close()
    print(json.dumps(out), flush=True)


def step_cost(args):
    me = os.path.abspath(__file__)
    base = [sys.executable, me, "_one", "--nstat", str(args.nstat), "--nev", str(args.nev), "--steps", str(args.steps),
            "--warmup", str(args.warmup), "--k0", str(args.k0), "--kmax", str(args.kmax)]
    for shape in ("40x40x24", "64x64x64"):
        for nch in (8, 64):
            med = {"voronoi": [], "single": []}
            for _ in range(args.rounds):
                for kind, root in (("single", args.parent or ROOT), ("voronoi", ROOT)):
                    r = subprocess.run(base + ["--kind", kind, "--root", root, "--shape", shape, "--chains", str(nch)],
                                       capture_output=True, text=True, timeout=600)
                    if r.returncode != 0:
                        sys.exit(f"vor_cost.py: the {kind} measurement failed ({r.returncode}):\n{r.stderr[-2000:]}")
                    line = r.stdout.strip().splitlines()[-1]
                    print(line, flush=True)
                    d = json.loads(line)
                    med[kind].append((d["ms_step"], d["ms_fsm_per_step"], d["sweep_iterations_per_step"],
                                      d["segments_updated_per_step"]))
            v, s = (np.median(np.array(med[k]), axis=0) for k in ("voronoi", "single"))
            print(json.dumps({"what": "step_ratio", "grid": shape, "chains": nch, "single_cell_of": args.parent or ROOT,
                              "ms_voronoi_step": round(float(v[0]), 3), "ms_single_cell_step": round(float(s[0]), 3),
                              "voronoi_in_single_cell_steps": round(float(v[0] / s[0]), 3),
                              "ms_fsm_voronoi": round(float(v[1]), 3), "ms_fsm_single_cell": round(float(s[1]), 3),
                              "sweep_iterations_voronoi": float(v[2]), "sweep_iterations_single_cell": float(s[2]),
                              "segments_updated_voronoi": float(v[3]), "segments_updated_single_cell": float(s[3])}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("raster", "step", "_one"))
    ap.add_argument("--config", default="C3")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=12, help="timed steps of a `step` measurement")
    ap.add_argument("--rounds", type=int, default=2, help="`step`: rounds of one single-cell and one Voronoi process")
    ap.add_argument("--parent", default=None, help="`step`: a built checkout whose single-cell step is the yardstick")
    ap.add_argument("--nstat", type=int, default=8)
    ap.add_argument("--nev", type=int, default=16)
    ap.add_argument("--k0", type=int, default=16)
    ap.add_argument("--kmax", type=int, default=64)
    ap.add_argument("--kind", default="voronoi", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--shape", default="40x40x24", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.what == "_one":
        return one_step_cost(args)
    if args.what == "step":             # (this process starts the measurements and never opens the GPU itself)
        return step_cost(args)
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("vor_cost.py: no GPU (a timing needs one)")
    raster_cost(args)


if __name__ == "__main__":
    main()
