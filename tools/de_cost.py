#!/usr/bin/env python3
"""What a differential-evolution step costs: needs a GPU.

One sampler with `de_enable(every=2)`, so that DE steps and single-cell steps
alternate: a host clock around each `run(1)` that ends in a device synchronise,
after a warm-up, the median per kind.  Grids 40 x 40 x 24 and 64^3 (the sizes
of DESIGN.md s.18), 8 stations, 16 events, inversion cells of 4 x 4 x 4 nodes,
fp32, with 8 and with 64 chains.  A DE step solves for half the chains, so
about half a single-cell step is expected; what the pipes' join and fork around
the proposal add shows in the difference between the two chain counts.  Also
reports the acceptance, the out-of-box share and the cells moved per accepted
move of the timed DE steps.  One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem(mcmc, shape, nstat, nev):
    nx, ny, nz = shape
    p = mcmc.make_problem("C2", n=nx, nstat=nstat, nev=nev)
    if (ny, nz) != (nx, nx):
        p.ny, p.nz = ny, nz
        p.sz[:] = (nz - 1) * p.h
        p.ez = np.clip(p.ez, p.h, (nz - 2) * p.h)
        p.v_true = mcmc.cell_velocity(p)
    return p


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=12, help="timed steps (half of them DE steps)")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--nstat", type=int, default=8)
    ap.add_argument("--nev", type=int, default=16)
    ap.add_argument("--gamma", type=float, default=None)
    ap.add_argument("--cr", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("de_cost.py: no GPU (a timing needs one)")
    from mceik_amd import mcmc
    for shape in ((40, 40, 24), (64, 64, 64)):
        p = problem(mcmc, shape, args.nstat, args.nev)
        for nch in (8, 64):
            smp = mcmc.Sampler(p, nchains=nch)
            smp.de_enable(2, gamma=args.gamma, cr=args.cr)
            smp.run(args.warmup)
            smp.sync()
            smp.de_stats(reset=True)
            ms = {0: [], 1: []}
            for gs in range(args.warmup, args.warmup + args.steps):
                t0 = time.perf_counter()
                smp.run(1)
                smp.sync()
                ms[gs % 2].append(1e3 * (time.perf_counter() - t0))
            st, info, o = smp.de_stats(), smp.info(), smp.de_options()
            smp.close()
            de, sc = float(np.median(ms[0])), float(np.median(ms[1]))
            print(json.dumps({"what": "de_cost", "grid": list(shape), "ncell": int(p.ncell), "chains": nch,
                              "npipe": info["npipe"], "gamma": round(o["gamma"], 5), "cr": o["cr"],
                              "ms_de_step": round(de, 3), "ms_single_cell_step": round(sc, 3),
                              "de_in_single_cell_steps": round(de / sc, 3),
                              "ms_de_all": [round(x, 3) for x in ms[0]], "ms_single_cell_all": [round(x, 3) for x in ms[1]],
                              "attempts": st["attempts"], "accepts": st["accepts"], "outbox": st["outbox"],
                              "failed": st["failed"],
                              "cells_moved_per_accept": round(st["moved"] / st["accepts"], 1) if st["accepts"] else None}),
                  flush=True)


if __name__ == "__main__":
    main()
