#!/usr/bin/env python3
"""What the probe-to-cell covariances cost: needs a GPU.

  accumulate  the gather + accumulate launches alone, timed with device events
              at the headline shape (C3: 1024 chains x 32 768 entries), models
              set via restore (no FSM in the timed window), a warm-up, then
              --launches pairs back to back; np in {1, 16, 64}, `within` off and
              on.  Prints ms, the share of one C3 velocity step (--step-ms: take
              it from the same visit's bench.py line), and the bytes moved
              against the 8 TB/s of the project's roofline: 4 B of v per chain
              and entry and probe group of 16 (the v row is re-read per group),
              8 B per flushed atomic word (one per (p + 2, j) and chain slice of
              64), and with `within` 16 B of S_c per chain and entry.
  reduce      the within-chain reduce of `cov_partials`, timed once per np
              (wall clock around the call, copies to the host included).

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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--step-ms", type=float, default=0.0, help="one C3 velocity step (bench.py rank_step_ms of this visit)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cov_cost.py: no GPU (a timing needs one)")
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
    entries = rng.permutation(ncm)
    for nprobe in args.probes:
        for within in (False, True):
            smp.cov_clear()
            smp.cov_enable([("model", int(e)) for e in entries[:nprobe]], within=within)
            for _ in range(args.warmup):
                smp.cov_accumulate()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            for _ in range(args.launches):
                smp.cov_accumulate()
            ev1.record(stream)
            ev1.synchronize()
            ms = ev0.elapsed_time(ev1) / args.launches
            groups, slices = -(-nprobe // 16), -(-nch // 64)
            nbytes = nch * ncm * 4 * groups + (nprobe + 2) * ncm * slices * 8 + (nch * ncm * 16 if within else 0)
            out = {"what": "accumulate", "config": args.config, "chains": nch, "ncm": ncm, "np": nprobe,
                   "within": within, "launches": args.launches, "ms_per_state": round(ms, 4), "bytes": nbytes,
                   "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                   "frac_of_8TBs": round(nbytes / (ms * 1e-3) / PEAK_BYTES_S, 4),
                   "mad_per_ns": round(nch * ncm * nprobe / (ms * 1e6), 1)}
            if args.step_ms > 0:
                out["share_of_c3_step"] = round(ms / args.step_ms, 6)
            print(json.dumps(out), flush=True)
            assert smp.cov_raw()["n"] == args.warmup + args.launches
            if within:
                smp.sync()
                t0 = time.perf_counter()
                parts = smp.cov_partials()
                dt = time.perf_counter() - t0
                assert parts.nkept == args.warmup + args.launches
                print(json.dumps({"what": "reduce", "config": args.config, "chains": nch, "ncm": ncm, "np": nprobe,
                                  "ms_partials_call": round(dt * 1e3, 3)}), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
