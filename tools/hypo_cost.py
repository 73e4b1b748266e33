#!/usr/bin/env python3
"""What a hypocentre step costs: needs a GPU.

A sampler of a BASELINE configuration (C2 by default) with hypocentre moves on
and every = 2, so velocity steps and hypocentre steps alternate in one run of
one sampler.  Every step is run and synchronised on its own and timed on the
host; the two kinds are reported by their medians, with their ratio.  From the
code a hypocentre step of a P-only sampler is one velocity step's solves with
2 nev gathers per solve instead of nev, and of a P+S sampler twice the solves
(both phases are solved, a velocity step solves the proposal's phase).

While hypocentre moves are on every step is one launch of each kernel, so the
velocity steps timed here are per-step launches on the sampler's pipes, not
the multi-step launches a C2 sampler otherwise runs.  One JSON line per phase
set on stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(mcmc, args, phases):
    p = mcmc.make_problem(args.config, phases=phases, picks="analytic")
    p.dvmax = 50
    nch = args.chains or mcmc.CONFIGS[args.config]["nchains"]
    smp = mcmc.Sampler(p, nchains=nch)
    smp.hypo_enable(2, dmax=(args.dmax,) * 3)
    info = smp.info()
    smp.run(2 * args.warmup)
    smp.sync()
    ms = {0: [], 1: []}                     # step parity: 0 velocity, 1 hypocentre
    step = smp.state()[3]
    for _ in range(2 * args.steps):
        t = time.perf_counter()
        smp.run(1)
        smp.sync()
        ms[step % 2].append((time.perf_counter() - t) * 1e3)
        step += 1
    att, acc = smp.hypo_stats()
    moved = int((smp.hypo_positions() != smp.hypo_positions()[:1]).any(-1).sum())
    smp.close()
    vel, hyp = statistics.median(ms[0]), statistics.median(ms[1])
    print(json.dumps({"what": "hypocentre step against velocity step", "config": args.config, "phases": phases,
                      "chains": nch, "nstat": p.nstat, "nev": p.nevents, "npipe": info["npipe"],
                      "kernel": info["kernel"], "steps_each": args.steps,
                      "velocity_step_ms": round(vel, 3), "hypo_step_ms": round(hyp, 3),
                      "ratio": round(hyp / vel, 4),
                      "velocity_min_max_ms": [round(min(ms[0]), 3), round(max(ms[0]), 3)],
                      "hypo_min_max_ms": [round(min(ms[1]), 3), round(max(ms[1]), 3)],
                      "move_accept_rate": round(float(acc.sum()) / max(int(att.sum()), 1), 4),
                      "events_off_chain0": moved}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C2", help="BASELINE configuration (mcmc.CONFIGS)")
    ap.add_argument("--chains", type=int, default=0, help="0: the configuration's")
    ap.add_argument("--dmax", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2, help="pairs of steps before the timed ones")
    ap.add_argument("--steps", type=int, default=8, help="timed steps of each kind")
    ap.add_argument("--phases", default="P,PS")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("hypo_cost.py: no GPU (a timing needs one)")
    from mceik_amd import mcmc
    for phases in args.phases.split(","):
        measure(mcmc, args, phases)


if __name__ == "__main__":
    main()
