#!/usr/bin/env python3
"""What parallel tempering costs: needs a GPU.

  exchange    the swap round alone (decide + exchange kernels), timed with
              device events at the headline shape (C3: 1024 chains x 32 768
              entries), 8 rungs on an all-ones ladder so that every attempted
              pair swaps; no FSM in the timed window.  A warm-up, then
              --launches rounds back to back, parities alternating (parity 0
              has 4 rung pairs, parity 1 has 3).  Prints ms per round, the bytes
              moved (per swapped pair 3 rows of 4-byte entries, read and
              written, for both chains: 48 B per entry), bytes/s against the
              8 TB/s of the project's roofline, and the share of one C3 step.
  chunking    C2 (multi-step launches by default): proposals/s with tempering
              off and on at swap_every = 8 and 1 (a launch ends before the next
              swap step).

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


def exchange_cost(args):
    import torch
    from mceik_amd import mcmc
    p = mcmc.make_problem(args.config, picks="analytic")
    nch = args.chains or mcmc.CONFIGS[args.config]["nchains"]
    smp = mcmc.Sampler(p, nchains=nch)
    stream = torch.cuda.current_stream()
    smp.set_stream(stream.cuda_stream)
    nt = args.ntemps
    G = nch // nt
    ncm = p.nphase * p.ncell
    smp.temper_enable(betas=np.ones(nt), swap_every=0)
    for i in range(args.warmup):
        smp.temper_swap(i & 1)
    smp.sync()
    smp.temper_stats(reset=True)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    for i in range(args.launches):
        smp.temper_swap(i & 1)
    ev1.record(stream)
    ev1.synchronize()
    att, acc = smp.temper_stats()
    assert att.tolist() == acc.tolist() and int(att.sum()) > 0      # all-ones ladder: every pair swapped
    pairs = int(acc.sum())
    ms = ev0.elapsed_time(ev1) / args.launches
    nbytes = pairs * ncm * 48 / args.launches
    print(json.dumps({"what": "exchange", "config": args.config, "chains": nch, "ncm": ncm, "ntemps": nt, "G": G,
                      "launches": args.launches, "pairs_per_round": round(pairs / args.launches, 1),
                      "ms_per_round": round(ms, 4), "bytes_per_round": int(nbytes),
                      "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                      "frac_of_8TBs": round(nbytes / (ms * 1e-3) / PEAK_BYTES_S, 3),
                      "share_of_c3_step": round(ms / C3_STEP_MS, 6)}), flush=True)
    smp.close()


def chunking_cost(args):
    from mceik_amd import mcmc
    p = mcmc.make_problem("C2", picks="analytic")
    mcmc.bench_picks(p)
    nch = mcmc.CONFIGS["C2"]["nchains"]
    for label, k in (("off", 0), ("swap_every=8", 8), ("swap_every=1", 1), ("off", 0)):
        smp = mcmc.Sampler(p, nchains=nch)
        if label != "off":
            smp.temper_enable(ntemps=args.ntemps, tmax=args.tmax, swap_every=k)
        multi = smp.info()["multi_step"]
        smp.run(args.chunk_warmup)
        smp.sync()
        _, nl0, _, _ = smp.fsm_stats()
        t0 = time.perf_counter()
        smp.run(args.chunk_steps)
        smp.sync()
        dt = time.perf_counter() - t0
        _, nl1, _, _ = smp.fsm_stats()
        out = {"what": "chunking", "config": "C2", "chains": nch, "tempering": label, "multi_step": multi,
               "steps": args.chunk_steps, "launches": nl1 - nl0, "seconds": round(dt, 4),
               "proposals_per_s": round(nch * args.chunk_steps / dt, 1)}
        if label != "off":
            att, acc = smp.temper_stats()
            out["swap_attempts"], out["swap_accepts"] = att.tolist(), acc.tolist()
        print(json.dumps(out), flush=True)
        smp.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("exchange", "chunking", "all"))
    ap.add_argument("--config", default="C3")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--ntemps", type=int, default=8)
    ap.add_argument("--tmax", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--chunk-warmup", type=int, default=64)
    ap.add_argument("--chunk-steps", type=int, default=128)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("temper_cost.py: no GPU (a timing needs one)")
    if args.what in ("exchange", "all"):
        exchange_cost(args)
    if args.what in ("chunking", "all"):
        chunking_cost(args)


if __name__ == "__main__":
    main()
