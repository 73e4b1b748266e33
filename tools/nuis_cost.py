#!/usr/bin/env python3
"""What a nuisance step costs: needs a GPU.

A sampler of a BASELINE configuration (C2 by default) with the noise-scale and
station-static moves on, every = 2 and nsub = 64, so velocity steps and
nuisance steps alternate in one run of one sampler.  Every step is run and
synchronised on its own and timed on the host; the two kinds are reported by
their medians, with their ratio.  From the code a nuisance step is one launch
of one wave per chain doing nsub x 3 passes over the chain's nobs
observations, and no eikonal solve.

While the values are held every step is one launch of each kernel, so the
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
    smp.nuis_enable(2, offset=1, nsub=args.nsub, ladder=mcmc.nuis_ladder(args.nk, None, args.lam_max), dk=2,
                    statics_dt=args.dt, dc=2, kcmax=args.kcmax)
    info = smp.info()
    solves0 = smp.fsm_solves()
    smp.run(2 * args.warmup)
    smp.sync()
    ms = {0: [], 1: []}                     # step parity: 0 velocity, 1 nuisance
    step = smp.state()[3]
    for _ in range(2 * args.steps):
        t = time.perf_counter()
        smp.run(1)
        smp.sync()
        ms[step % 2].append((time.perf_counter() - t) * 1e3)
        step += 1
    att, acc = smp.nuis_stats()
    solves = smp.fsm_solves() - solves0
    smp.close()
    vel, nui = statistics.median(ms[0]), statistics.median(ms[1])
    print(json.dumps({"what": "nuisance step against velocity step", "config": args.config, "phases": phases,
                      "chains": nch, "nstat": p.nstat, "nev": p.nevents, "nobs": int(p.obs_ptr[-1]),
                      "npipe": info["npipe"], "kernel": info["kernel"], "nsub": args.nsub, "steps_each": args.steps,
                      "velocity_step_ms": round(vel, 3), "nuis_step_ms": round(nui, 3),
                      "ratio": round(nui / vel, 6),
                      "velocity_min_max_ms": [round(min(ms[0]), 3), round(max(ms[0]), 3)],
                      "nuis_min_max_ms": [round(min(ms[1]), 3), round(max(ms[1]), 3)],
                      "solves_per_velocity_step": solves / (args.warmup + args.steps),
                      "noise_accept_rate": round(float(acc[:p.nphase].sum()) / max(int(att[:p.nphase].sum()), 1), 4),
                      "statics_accept_rate": round(float(acc[p.nphase:].sum()) / max(int(att[p.nphase:].sum()), 1), 4)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C2", help="BASELINE configuration (mcmc.CONFIGS)")
    ap.add_argument("--chains", type=int, default=0, help="0: the configuration's")
    ap.add_argument("--nsub", type=int, default=64, help="sub-moves per chain and nuisance step")
    ap.add_argument("--nk", type=int, default=41, help="ladder entries (odd)")
    ap.add_argument("--lam-max", type=float, default=10.0)
    ap.add_argument("--dt", type=float, default=1e-3, help="seconds per unit of a static")
    ap.add_argument("--kcmax", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2, help="pairs of steps before the timed ones")
    ap.add_argument("--steps", type=int, default=8, help="timed steps of each kind")
    ap.add_argument("--phases", default="P,PS")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("nuis_cost.py: no GPU (a timing needs one)")
    from mceik_amd import mcmc
    for phases in args.phases.split(","):
        measure(mcmc, args, phases)


if __name__ == "__main__":
    main()
