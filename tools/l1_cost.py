#!/usr/bin/env python3
"""What the L1 (Laplace) likelihood costs: needs a GPU.  It
measures only and asserts nothing.

  grid     the L1 grid search beside the L2 one, device arrays, timed with
           device events (a warm-up, then --launches launches back to back):
           mceik_relocate_l1 against mceik_relocate (fp32) at locate.c's own
           shape (145 x 145 x 45 points, one event of 20 picks) and at C3's
           relocation shape (32 events x 128^3 points x 32 picks, 32 table
           rows).  Prints ms, the (k, j) pairs of the median per second, and
           the L1 / L2 ratio (expected about n-fold: the median is n^2 per
           point).  With --dropin also locate_l1_gridSearch__double64 against
           locate_l2_gridSearch__double64 at locate.c's shape: host arrays, a
           host clock around the whole call (allocation and copies included).
  step     an L1 velocity step against an L2 per-step step at 40 x 40 x 24 and
           64^3 nodes (8 stations, 16 events, cells of 4 x 4 x 4 nodes, fp32)
           with 8 and 64 chains: a host clock around each `run(1)` that ends in
           a device synchronise, after a warm-up, the median.  Each measurement
           is a process of its own; with --parent DIR (a built checkout of the
           parent commit) the L2 step is the parent's, and the two alternate for
           --rounds rounds.  Both run one launch per step (MCEIK_PERSIST=0).
           The device time of the FSM launches per step is reported beside it
           (summed over the pipes, so two overlapping launches count twice).

One JSON line per measurement on stdout.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"locate": dict(ngrd=145 * 145 * 45, nev=1, npick=20, nrows=20),
          "c3": dict(ngrd=128 ** 3, nev=32, npick=32, nrows=32)}


def grid_cost(args):
    import torch
    from mceik_amd import _lib
    from mceik_amd.eikonal import aligned_empty, locate_l1_gridsearch, locate_l2_gridsearch
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    g = np.random.default_rng(4042)
    for name in args.shapes.split(","):
        s = SHAPES[name]
        ngrd, nev, n, nrows = s["ngrd"], s["nev"], s["npick"], s["nrows"]
        ld = (ngrd + 15) // 16 * 16
        tab = torch.rand((nrows, ld), dtype=torch.float32, device=dev) * 3.0 + 0.2
        ptr = torch.arange(0, (nev + 1) * n, n, dtype=torch.int32, device=dev)
        rows = torch.tensor(np.concatenate([g.permutation(nrows)[:n] for _ in range(nev)]).astype(np.int32), device=dev)
        tc = torch.tensor(g.uniform(0.5, 3.5, nev * n).astype(np.float32), device=dev)
        wt = torch.tensor((1.0 / g.uniform(0.01, 0.2, nev * n)).astype(np.float32), device=dev)
        xn = torch.stack([wt[e * n:(e + 1) * n].sum() for e in range(nev)])
        out = torch.empty((nev, ld), dtype=torch.float32, device=dev)
        t0 = torch.empty((nev, ld), dtype=torch.float32, device=dev)
        b = _lib.RelocateBatch()
        b.ldgrd, b.ngrd, b.nev, b.iwantOT, b.t0use = ld, ngrd, nev, 1, 0.0
        b.tables, b.ev_ptr, b.obs_row = tab.data_ptr(), ptr.data_ptr(), rows.data_ptr()
        b.tc, b.wt, b.xnorm, b.t0, b.out, b.log_pdf = tc.data_ptr(), wt.data_ptr(), xn.data_ptr(), t0.data_ptr(), \
            out.data_ptr(), 1
        b.nrows, b.nobs = nrows, nev * n
        stream = torch.cuda.current_stream()
        ms = {}
        for norm, f in ((2, L.mceik_relocate), (1, L.mceik_relocate_l1)):
            for _ in range(args.warmup):
                f(C.byref(b), C.c_void_p(stream.cuda_stream))
            torch.cuda.synchronize(dev)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            for _ in range(args.launches):
                f(C.byref(b), C.c_void_p(stream.cuda_stream))
            ev1.record(stream)
            ev1.synchronize()
            ms[norm] = ev0.elapsed_time(ev1) / args.launches
        pairs = float(nev) * ngrd * n * n
        print(json.dumps({"what": "grid", "shape": name, "precision": 32, "ngrd": ngrd, "events": nev, "picks": n,
                          "launches": args.launches, "ms_l1": round(ms[1], 4), "ms_l2": round(ms[2], 4),
                          "l1_over_l2": round(ms[1] / ms[2], 2), "pairs": pairs,
                          "pairs_per_s": round(pairs / (ms[1] * 1e-3), 0),
                          "table_bytes": int(nrows) * ngrd * 4}), flush=True)
    if args.dropin:
        s = SHAPES["locate"]
        ngrd, n = s["ngrd"], s["npick"]
        ld = (ngrd + 7) // 8 * 8
        test = aligned_empty(n * ld)
        test[:] = g.uniform(0.2, 3.0, n * ld)
        tobs, var, mask = g.uniform(0.5, 3.5, n), g.uniform(0.01, 0.2, n), np.zeros(n, np.int32)
        t0, obj = aligned_empty(ld), aligned_empty(ld)
        ms = {}
        for norm in (2, 1, 2, 1):
            t = time.perf_counter()
            if norm == 1:
                locate_l1_gridsearch(ld, ngrd, n, 1, 0.0, mask, tobs, var, test, t0, obj)
            else:
                locate_l2_gridsearch(ld, ngrd, n, 1, 0.0, mask, tobs, None, var, test, t0, obj)
            ms[norm] = 1e3 * (time.perf_counter() - t)       # (the second call of each: allocations are warm)
        print(json.dumps({"what": "dropin", "shape": "locate", "precision": 64, "ngrd": ngrd, "picks": n,
                          "ms_call_l1": round(ms[1], 2), "ms_call_l2": round(ms[2], 2),
                          "note": "host clock around the whole call: allocation and 151 MB of copies included"}),
              flush=True)


def problem(mcmc, shape, nstat, nev):
    nx, ny, nz = shape
    p = mcmc.make_problem("C2", n=nx, nstat=nstat, nev=nev)
    if (ny, nz) != (nx, nx):
        p.ny, p.nz = ny, nz
        p.sz[:] = (nz - 1) * p.h
        p.ez = np.clip(p.ez, p.h, (nz - 2) * p.h)
        p.v_true = mcmc.cell_velocity(p)
    return p


def one_step_cost(args):
    """The child process of `step`: one sampler of --root's library, one norm."""
    os.environ["MCEIK_PERSIST"] = "0"
    sys.path.insert(0, os.path.abspath(args.root))
    from mceik_amd import mcmc
    shape = tuple(int(x) for x in args.shape.split("x"))
    p = problem(mcmc, shape, args.nstat, args.nev)
    smp = mcmc.Sampler(p, nchains=args.chains)
    if args.norm == 1:
        smp.likelihood_set(1)
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
    fsm_ms = smp.fsm_stats()[0]
    acc = int(smp.state()[2].sum())
    smp.close()
    print(json.dumps({"what": "step", "norm": args.norm, "root": os.path.abspath(args.root), "grid": list(shape),
                      "chains": args.chains, "events": args.nev, "stations": args.nstat, "npipe": info["npipe"],
                      "multi_step": info["multi_step"], "ms_step": round(float(np.median(ms)), 3),
                      "ms_all": [round(x, 3) for x in ms], "ms_fsm_per_step": round(fsm_ms / args.steps, 3),
                      "accepted": acc}), flush=True)


def step_cost(args):
    me = os.path.abspath(__file__)
    base = [sys.executable, me, "_one", "--nstat", str(args.nstat), "--nev", str(args.nev), "--steps", str(args.steps),
            "--warmup", str(args.warmup)]
    for shape in ("40x40x24", "64x64x64"):
        for nch in (8, 64):
            med = {1: [], 2: []}
            for _ in range(args.rounds):
                for norm, root in ((2, args.parent or ROOT), (1, ROOT)):
                    r = subprocess.run(base + ["--norm", str(norm), "--root", root, "--shape", shape, "--chains", str(nch)],
                                       capture_output=True, text=True, timeout=600)
                    if r.returncode != 0:
                        sys.exit(f"l1_cost.py: the norm {norm} measurement failed ({r.returncode}):\n{r.stderr[-2000:]}")
                    line = r.stdout.strip().splitlines()[-1]
                    print(line, flush=True)
                    d = json.loads(line)
                    med[norm].append((d["ms_step"], d["ms_fsm_per_step"]))
            a, b = (np.median(np.array(med[k]), axis=0) for k in (1, 2))
            print(json.dumps({"what": "step_ratio", "grid": shape, "chains": nch, "l2_step_of": args.parent or ROOT,
                              "ms_l1_step": round(float(a[0]), 3), "ms_l2_step": round(float(b[0]), 3),
                              "l1_over_l2": round(float(a[0] / b[0]), 3), "ms_fsm_l1": round(float(a[1]), 3),
                              "ms_fsm_l2": round(float(b[1]), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("grid", "step", "_one"))
    ap.add_argument("--shapes", default="locate,c3", help="`grid`: of " + ", ".join(SHAPES))
    ap.add_argument("--dropin", action="store_true", help="`grid`: also the fp64 drop-ins on host arrays")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--steps", type=int, default=12, help="timed steps of a `step` measurement")
    ap.add_argument("--rounds", type=int, default=2, help="`step`: rounds of one L2 and one L1 process")
    ap.add_argument("--parent", default=None, help="`step`: a built checkout whose L2 step is the yardstick")
    ap.add_argument("--nstat", type=int, default=8)
    ap.add_argument("--nev", type=int, default=16)
    ap.add_argument("--norm", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--chains", type=int, default=8, help=argparse.SUPPRESS)
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
        sys.exit("l1_cost.py: no GPU (a timing needs one)")
    grid_cost(args)


if __name__ == "__main__":
    main()
