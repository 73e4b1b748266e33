#!/usr/bin/env python3
"""Which move pays: effective sample size per second of the plain single-cell
sampler, of block proposals, of discrete Langevin moves and of
differential-evolution moves on one problem, the same seed and the same
wall-clock budget each: needs a GPU.

Problem: tests/_adjoint.ps_problem (24 x 24 x 16, P+S, 144 cells per model), 8
chains.  Per configuration: --burn steps of burn-in, then steps in chunks of
--chunk until --seconds of wall clock (a device synchronise ends every chunk)
with the batch-means sums on (keepK = 1); then `ess_summary` at the level it
picks and at the largest level that still closed --batches batches per chain.
Reports the median tau over the cells at every level (a plateau means the
batches have outgrown the correlation; tau_l = 2^l means a cell hardly moves
within a batch and tau is only bounded from below), and at both levels the
median and the minimum ESS over the cells that moved and the same per second.
One JSON line per configuration on stdout.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {
    "single-cell": lambda smp: None,
    "block": lambda smp: smp.block_enable(),
    "langevin": lambda smp: smp.lang_enable(every=4, sigma=4),
    "de": lambda smp: smp.de_enable(every=2),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--burn", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--nlevels", type=int, default=12)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--only", choices=list(CONFIGS), default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ess_compare.py: no GPU (a rate needs one)")
    import _adjoint as A
    from mceik_amd import mcmc
    p = A.ps_problem()
    p.nburn, p.keepk = args.burn, 1
    for name, enable in CONFIGS.items():
        if args.only and name != args.only:
            continue
        smp = mcmc.Sampler(p, nchains=args.chains)
        enable(smp)
        smp.ess_enable(args.nlevels)
        smp.run(args.burn)
        smp.sync()
        steps, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < args.seconds:
            smp.run(args.chunk)
            smp.sync()
            steps += args.chunk
        dt = time.perf_counter() - t0
        s = mcmc.ess_summary(smp)
        top = max(l for l in range(args.nlevels) if (steps >> l) >= args.batches or l == 0)
        st = mcmc.ess_summary(smp, level=top)
        nacc = int(smp.state()[2].sum())
        de = smp.de_stats() if smp._de is not None else None      # (burn-in included)
        smp.close()
        ess, tau = s.ess[np.isfinite(s.ess)], s.tau[np.isfinite(s.tau)]
        ess_t = st.ess[np.isfinite(st.ess)]
        tl = s.tau_levels.reshape(args.nlevels, -1)
        print(json.dumps({"what": "ess_compare", "config": name, "chains": args.chains, "seconds": round(dt, 2),
                          "steps": steps, "ms_per_step": round(1e3 * dt / steps, 3), "accepts": nacc,
                          "count": s.count, "level": s.level, "cells_moved": int(ess.size), "cells": int(s.ess.size),
                          "tau_median": round(float(np.median(tau)), 2), "tau_max": round(float(tau.max()), 2),
                          "ess_median": round(float(np.median(ess)), 1), "ess_min": round(float(ess.min()), 1),
                          "ess_median_per_s": round(float(np.median(ess)) / dt, 2),
                          "ess_min_per_s": round(float(ess.min()) / dt, 3),
                          "tau_levels_median": [round(float(np.nanmedian(r)), 2) if np.isfinite(r).any() else None for r in tl],
                          "top_level": top, "top_ess_median": round(float(np.median(ess_t)), 1),
                          "top_ess_min": round(float(ess_t.min()), 1),
                          "top_ess_median_per_s": round(float(np.median(ess_t)) / dt, 3),
                          "top_ess_min_per_s": round(float(ess_t.min()) / dt, 3), "de": de}), flush=True)
        assert s.count == steps and s.nchains == args.chains


if __name__ == "__main__":
    main()
