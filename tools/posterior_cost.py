#!/usr/bin/env python3
"""What the streaming posterior costs: needs a GPU.

  accumulate  the accumulate launch alone, timed with device events at the
              headline shape (C3: 1024 chains x 32 768 entries), models set via
              restore (no FSM in the timed window), a warm-up, then --launches
              launches back to back; every mode.  Prints ms, bytes/s for
              36 B per chain and entry (4 B v read, 16 B sum/sumsq read, 16 B
              written; pooled mode moves 4 B) against the 8 TB/s of the
              project's roofline, and the share of one C3 step.
  chunking    C2 (multi-step launches by default): proposals/s with the
              posterior off and on at keepK = 8 and 1.

One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_S = 8e12                     # the roofline's HBM figure (bench.py)
C3_STEP_MS = 1565.0                     # BENCH_r06.json rank_step_ms


def accumulate_cost(args):
    import torch
    from mceik_amd import mcmc
    p = mcmc.make_problem(args.config, picks="analytic")
    nch = args.chains or mcmc.CONFIGS[args.config]["nchains"]
    smp = mcmc.Sampler(p, nchains=nch)
    stream = torch.cuda.current_stream()
    smp.set_stream(stream.cuda_stream)
    ck = smp.checkpoint()
    rng = np.random.default_rng(3)
    ck["v"] = rng.integers(p.vmin, p.vmax + 1, smp.model_shape).astype(np.int32)
    smp.restore(ck)                     # logl given: no forward
    ncm = p.nphase * p.ncell
    for per_chain, nbins in ((True, args.nbins), (True, 0), (False, args.nbins), (False, 0)):
        smp.posterior_enable(per_chain=per_chain, nbins=nbins)
        for _ in range(args.warmup):
            smp.posterior_accumulate()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(args.launches):
            smp.posterior_accumulate()
        ev1.record(stream)
        ev1.synchronize()
        ms = ev0.elapsed_time(ev1) / args.launches
        nbytes = nch * ncm * (36 if per_chain else 4)
        print(json.dumps({"what": "accumulate", "config": args.config, "chains": nch, "ncm": ncm,
                          "per_chain": per_chain, "nbins": nbins, "launches": args.launches,
                          "ms_per_launch": round(ms, 4), "bytes": nbytes,
                          "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                          "frac_of_8TBs": round(nbytes / (ms * 1e-3) / PEAK_BYTES_S, 3),
                          "share_of_c3_step": round(ms / C3_STEP_MS, 6)}), flush=True)
        assert smp.posterior_raw()["n"] == args.warmup + args.launches
    smp.close()


def chunking_cost(args):
    from mceik_amd import mcmc
    p = mcmc.make_problem("C2", picks="analytic")
    mcmc.bench_picks(p)
    nch = mcmc.CONFIGS["C2"]["nchains"]
    for label, keepk in (("off", 1), ("keepK=8", 8), ("keepK=1", 1), ("off", 1)):
        p.nburn, p.keepk = 0, keepk
        smp = mcmc.Sampler(p, nchains=nch)
        if label != "off":
            smp.posterior_enable(per_chain=True, nbins=args.nbins)
        multi = smp.info()["multi_step"]
        smp.run(args.chunk_warmup)
        smp.sync()
        _, nl0, _, _ = smp.fsm_stats()
        t0 = time.perf_counter()
        smp.run(args.chunk_steps)
        smp.sync()
        dt = time.perf_counter() - t0
        _, nl1, _, _ = smp.fsm_stats()
        print(json.dumps({"what": "chunking", "config": "C2", "chains": nch, "posterior": label, "multi_step": multi,
                          "steps": args.chunk_steps, "launches": nl1 - nl0, "seconds": round(dt, 4),
                          "proposals_per_s": round(nch * args.chunk_steps / dt, 1)}), flush=True)
        smp.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("accumulate", "chunking", "all"))
    ap.add_argument("--config", default="C3")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--chunk-warmup", type=int, default=64)
    ap.add_argument("--chunk-steps", type=int, default=128)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("posterior_cost.py: no GPU (a timing needs one)")
    if args.what in ("accumulate", "all"):
        accumulate_cost(args)
    if args.what in ("chunking", "all"):
        chunking_cost(args)


if __name__ == "__main__":
    main()
