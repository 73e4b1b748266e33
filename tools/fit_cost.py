#!/usr/bin/env python3
"""What the streaming data-fit sums cost: needs a GPU.

Steps per second of one sampler of a BASELINE configuration (C2 and C3 by
default), one- and two-model, with the sums off and on.  keepK = 1 and no
burn-in, so every step is a kept step: the worst case.  One process, one
sampler per (configuration, phases): a warm-up, then --blocks rounds, each a
timed block of --steps steps with the sums off and one with them on (the
order alternates from round to round), every block ended by a synchronise and
timed on the host.  Reported: steps/s of every block, the medians, the spread
of the off blocks (max - min over the median: what a difference has to exceed
to mean anything), the cost of the sums as 1 - on / off, and the time of the
two accumulate kernels on an otherwise idle GPU (--launches of them between
two synchronises).

Two costs are in that figure.  The accumulate launches: two kernels per kept
step and pipe.  And, for a one-model sampler, leaving the multi-step
launches: while the sums are on every step is one launch of each kernel
(info()["multi_step"] is reported for both modes).

--modes off measures the first half alone, and --root DIR imports mceik_amd
from another checkout (say, the parent commit's, built): the off-cost of this
change is the difference between the two trees' off figures, to be read
against their spreads.  One JSON line per (configuration, phases) on stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time


def measure(mcmc, args, config, phases):
    p = mcmc.make_problem(config, phases=phases, picks="analytic")
    p.nburn, p.keepk = 0, args.keepk
    nch = args.chains or mcmc.CONFIGS[config]["nchains"]
    smp = mcmc.Sampler(p, nchains=nch)
    modes = args.modes.split(",")
    info = {}

    def switch(mode):
        if "on" in modes:
            (smp.fit_enable if mode == "on" else smp.fit_disable)()
        if mode not in info:
            i = smp.info()
            info[mode] = {"multi_step": i["multi_step"], "npipe": i["npipe"]}

    for mode in modes:                      # every kernel of both modes has run before a timed block
        switch(mode)
        smp.run(args.warmup)
        smp.sync()
    rate = {m: [] for m in modes}
    for b in range(args.blocks):
        for mode in (modes if b % 2 == 0 else modes[::-1]):
            switch(mode)
            smp.sync()
            t = time.perf_counter()
            smp.run(args.steps)
            smp.sync()
            rate[mode].append(args.steps / (time.perf_counter() - t))
    out = {"what": "steps/s with the data-fit sums off / on", "config": config, "phases": phases, "chains": nch,
           "nstat": p.nstat, "nev": p.nevents, "nobs": int(p.obs_ptr[-1]), "keepk": args.keepk,
           "steps_per_block": args.steps, "blocks": args.blocks, "kernel": smp.info()["kernel"]}
    for m in modes:
        med = statistics.median(rate[m])
        out[m] = {"steps_per_s": [round(r, 4) for r in rate[m]], "median": round(med, 4),
                  "spread": round((max(rate[m]) - min(rate[m])) / med, 5), **info[m]}
    if "on" in modes and "off" in modes:
        out["cost_of_on"] = round(1.0 - out["on"]["median"] / out["off"]["median"], 5)
        out["states_in_sums"] = smp.fit_raw()["n"]
        # the two accumulate kernels alone, nothing else on the GPU: --launches of them between two synchronises
        smp.fit_enable()
        smp.fit_accumulate()
        smp.sync()
        t = time.perf_counter()
        for _ in range(args.launches):
            smp.fit_accumulate()
        smp.sync()
        out["accumulate_alone_ms"] = round((time.perf_counter() - t) * 1e3 / args.launches, 4)
    smp.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C2,C3", help="BASELINE configurations (mcmc.CONFIGS)")
    ap.add_argument("--phases", default="P,PS")
    ap.add_argument("--chains", type=int, default=0, help="0: the configuration's")
    ap.add_argument("--keepk", type=int, default=1, help="1: every step is a kept step")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps of each mode")
    ap.add_argument("--steps", type=int, default=4, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=4, help="rounds of one off block and one on block")
    ap.add_argument("--launches", type=int, default=50, help="accumulate launches timed on their own")
    ap.add_argument("--modes", default="off,on", help="off,on or off")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout mceik_amd is imported from (default: this one)")
    args = ap.parse_args()
    if args.modes not in ("off,on", "off"):
        sys.exit("fit_cost.py: --modes off,on or off")
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        sys.exit("fit_cost.py: no GPU (a timing needs one)")
    from mceik_amd import mcmc
    for config in args.configs.split(","):
        for phases in args.phases.split(","):
            measure(mcmc, args, config, phases)


if __name__ == "__main__":
    main()
