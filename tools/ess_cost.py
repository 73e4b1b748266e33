#!/usr/bin/env python3
"""What the batch-means accumulate launch costs: needs a GPU.

The launch alone at the headline shape (C3: 1024 chains x 32 768 entries),
models set via restore (no FSM in the timed window), tools/posterior_cost.py's
method: device events, a warm-up, then --launches launches.  The cost of a
launch depends on k, the trailing zero bits of the state's number t: a pair
of events around every launch, and the launches grouped by k.  Bytes per chain
and entry: 4 (v) + 16 (Sc read and written) + 4 k (pend[0 .. k - 1] read) + 4
(pend[k] written, while k <= nlevels - 2).  The posterior's per-chain launch
(36 B per chain and entry) is timed the same way on the same box.

One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_S = 8e12                     # the roofline's HBM figure (bench.py)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--nlevels", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ess_cost.py: no GPU (a timing needs one)")
    from mceik_amd import mcmc
    p = mcmc.make_problem(args.config, picks="analytic")
    nch = args.chains or mcmc.CONFIGS[args.config]["nchains"]
    smp = mcmc.Sampler(p, nchains=nch)
    stream = torch.cuda.current_stream()
    smp.set_stream(stream.cuda_stream)
    ck = smp.checkpoint()
    ck["v"] = np.random.default_rng(3).integers(p.vmin, p.vmax + 1, smp.model_shape).astype(np.int32)
    smp.restore(ck)                     # logl given: no forward
    ncm, L = p.nphase * p.ncell, args.nlevels

    def timed(launch, n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record(stream)
            launch()
            b.record(stream)
        ev[-1][1].synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    def line(what, k, ms, per_entry):
        nbytes = nch * ncm * per_entry
        med = float(np.median(ms))
        print(json.dumps({"what": what, "config": args.config, "chains": nch, "ncm": ncm, "nlevels": L, "k": k,
                          "launches": len(ms), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                          "bytes_per_chain_entry": per_entry, "bytes": nbytes,
                          "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3),
                          "frac_of_8TBs": round(nbytes / (med * 1e-3) / PEAK_BYTES_S, 3)}), flush=True)

    smp.posterior_enable(per_chain=True, nbins=0)
    timed(smp.posterior_accumulate, args.warmup)
    line("posterior_accumulate", None, timed(smp.posterior_accumulate, args.launches), 36)
    smp.posterior_disable()

    smp.ess_enable(L)
    warm = max(args.warmup, 8)          # t = 1 .. 8: every instance up to four closing levels has run
    timed(smp.ess_accumulate, warm)
    ms = timed(smp.ess_accumulate, args.launches)
    by_k = {}
    for i, m in enumerate(ms):
        t = warm + 1 + i
        by_k.setdefault((t & -t).bit_length() - 1, []).append(m)
    for k in sorted(by_k):
        kk = min(k, L - 1)
        line("ess_accumulate", k, by_k[k], 20 + 4 * kk + (4 if k <= L - 2 else 0))
    line("ess_accumulate", "all", ms, 0)
    assert smp.ess_raw()["n"] == warm + args.launches
    smp.close()


if __name__ == "__main__":
    main()
