#!/usr/bin/env python3
"""What block proposals cost: needs a GPU.

Times the two kernels of a block step alone -- block_propose_kernel then
block_accept_kernel (csrc/block.hip), no FSM launch between them -- with device
events at the headline shape (C3: 1024 chains x 32 768 cells, 32 stations x 32
events), for rmin = 0 and rmax = 0, 2 and 8, beside the single-cell
propose_kernel + accept_kernel (csrc/mcmc_kernels.hip) in the same run.  With
--baseline-lib the single-cell pair comes from another build of the library
(the parent commit's), so the two builds alternate inside one process.

The kernels are reached through the library's internal launchers (mcmc_propose,
mcmc_accept, block_propose, block_accept; C++ symbols of libmceik_hip.so) on a
chain state built here from device tensors: ctypes mirrors of McmcDev
(csrc/mcmc_common.h) and BlockDev (csrc/block.h), which must follow those
structs.  Models sit mid-prior, the proposal tables are random, and the start
logL makes every second chain accept (its footprint is committed) and the
others reject (reverted), launch after launch.  Every observation is used, so
the accept kernels pay the full misfit (3 passes over 1024 observations per
chain, fp64).

A warm-up, then --launches pairs back to back with the step counter running.
One JSON line per measurement on stdout; share_of_c3_step is against one C3
step (1565 ms, README).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C3_STEP_MS = 1565.0                     # BENCH_r06.json rank_step_ms
_P = C.c_void_p


class McmcDev(C.Structure):
    """csrc/mcmc_common.h McmcDev."""
    _fields_ = [(n, C.c_int) for n in ("nchains", "chain_offset", "ncell", "nstat", "nev", "nphase", "ncm",
                                       "vmin", "vmax", "dvmax", "vsmin", "vsmax")] + [("seed", C.c_uint32)] + \
               [(n, _P) for n in ("v", "slow_cur", "slow_prop", "logl", "naccept", "prop_cell", "prop_v",
                                  "prop_inprior", "prop_phase", "prop_logu", "accept", "ttab", "ttab_cur",
                                  "obs_ptr", "obs_stat", "obs_mask", "obs_phase", "tobs", "tcorr", "var",
                                  "keep_v", "keep_logl")] + [("keep_stride", C.c_int), ("beta", _P)]


class BlockDev(C.Structure):
    """csrc/block.h BlockDev."""
    _fields_ = [(n, C.c_int) for n in ("ncx", "ncy", "ncz", "rmin", "rmax")] + \
               [(n, _P) for n in ("prop_amp", "prop_rad", "attempts", "accepts")]


_SYMS = {"mcmc_propose": ("_Z12mcmc_proposeRK7McmcDevmP12ihipStream_t", [_P, C.c_uint64, _P]),
         "mcmc_accept": ("_Z11mcmc_acceptRK7McmcDeviP12ihipStream_t", [_P, C.c_int, _P]),
         "block_propose": ("_Z13block_proposeRK7McmcDevRK8BlockDevmP12ihipStream_t", [_P, _P, C.c_uint64, _P]),
         "block_accept": ("_Z12block_acceptRK7McmcDevRK8BlockDeviP12ihipStream_t", [_P, _P, C.c_int, _P])}


def launcher(lib, name):
    sym, argtypes = _SYMS[name]
    f = getattr(lib, sym)
    f.restype = C.c_int
    f.argtypes = argtypes
    return f


class State:
    """A sampler's device state without a sampler: tensors and the two structs."""

    def __init__(self, torch, nch, nc, nstat, nev, seed=2016):
        dev = torch.device("cuda", 0)
        g = torch.Generator(device="cpu").manual_seed(seed)
        ncell = nc ** 3
        nobs = nstat * nev
        t = self.t = {}
        t["v"] = torch.full((nch, ncell), 5000, dtype=torch.int32, device=dev)
        t["slow_cur"] = (1.0 / t["v"].float()).contiguous()
        t["slow_prop"] = t["slow_cur"].clone()
        # tables around 1 s against picks around 1 s: a finite logL per chain
        t["ttab"] = (1.0 + 0.1 * torch.rand((nch, nstat, nev), generator=g)).float().to(dev)
        t["tobs"] = (1.0 + 0.1 * torch.rand(nobs, generator=g, dtype=torch.float64)).to(dev)
        t["tcorr"] = torch.zeros(nobs, dtype=torch.float64, device=dev)
        t["var"] = torch.full((nobs,), 0.25, dtype=torch.float64, device=dev)
        t["obs_ptr"] = (torch.arange(nev + 1, dtype=torch.int32) * nstat).to(dev)
        t["obs_stat"] = torch.arange(nstat, dtype=torch.int32).repeat(nev).to(dev)
        t["obs_mask"] = torch.zeros(nobs, dtype=torch.int32, device=dev)
        # logL <= 0: chains starting at -1e300 accept (and from then on tie, which accepts);
        # chains starting at 0 never do
        logl = torch.zeros(nch, dtype=torch.float64)
        logl[::2] = -1e300
        t["logl"] = logl.to(dev)
        t["naccept"] = torch.zeros(nch, dtype=torch.int64, device=dev)
        for n in ("prop_cell", "prop_v", "prop_inprior", "prop_phase", "prop_amp", "prop_rad"):
            t[n] = torch.zeros(nch, dtype=torch.int32, device=dev)
        t["prop_logu"] = torch.zeros(nch, dtype=torch.float64, device=dev)
        t["accept"] = torch.zeros(nch, dtype=torch.uint8, device=dev)
        t["cnt"] = torch.zeros(2 * 9, dtype=torch.int64, device=dev)
        D = self.D = McmcDev()
        D.nchains, D.chain_offset, D.ncell, D.nstat, D.nev, D.nphase, D.ncm = nch, 0, ncell, nstat, nev, 1, ncell
        D.vmin, D.vmax, D.dvmax, D.vsmin, D.vsmax, D.seed = 1500, 9000, 50, 0, 0, seed
        for n in ("v", "slow_cur", "slow_prop", "logl", "naccept", "prop_cell", "prop_v", "prop_inprior",
                  "prop_phase", "prop_logu", "accept", "ttab", "obs_ptr", "obs_stat", "obs_mask", "tobs",
                  "tcorr", "var"):
            setattr(D, n, t[n].data_ptr())
        D.keep_stride = nch
        B = self.B = BlockDev()
        B.ncx = B.ncy = B.ncz = nc
        B.prop_amp, B.prop_rad = t["prop_amp"].data_ptr(), t["prop_rad"].data_ptr()
        B.attempts, B.accepts = t["cnt"].data_ptr(), t["cnt"].data_ptr() + 9 * 8
        self.nch = nch


def measure(torch, label, propose, accept, args, radii=None):
    st = State(torch, args.chains, args.cells, args.nstat, args.nev)
    stream = torch.cuda.current_stream()
    sp = _P(stream.cuda_stream)
    if radii is not None:
        st.B.rmin, st.B.rmax = radii
        extra = (C.byref(st.B),)
    else:
        extra = ()

    def pair(step):
        if propose(C.byref(st.D), *extra, step, sp) != 0 or accept(C.byref(st.D), *extra, -1, sp) != 0:
            sys.exit(f"block_cost.py: a launch of {label} failed")

    for i in range(args.warmup):
        pair(i)
    torch.cuda.synchronize()
    n0 = int(st.t["naccept"].sum())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record(stream)
    for i in range(args.launches):
        pair(args.warmup + i)
    ev[1].record(stream)
    # each kernel alone: the proposals, then (one more proposal pending) the accepts
    step = args.warmup + args.launches
    ev[2].record(stream)
    for i in range(args.launches):
        propose(C.byref(st.D), *extra, step + i, sp)
    ev[3].record(stream)
    torch.cuda.synchronize()
    ms_pair = ev[0].elapsed_time(ev[1]) / args.launches
    ms_prop = ev[2].elapsed_time(ev[3]) / args.launches
    acc = (int(st.t["naccept"].sum()) - n0) / (args.launches * st.nch)
    v = st.t["v"]
    assert int(v.min()) >= 1500 and int(v.max()) <= 9000
    out = {"what": label, "chains": st.nch, "cells": args.cells ** 3, "nstat": args.nstat, "nev": args.nev,
           "launches": args.launches, "ms_per_pair": round(ms_pair, 4), "ms_propose_alone": round(ms_prop, 4),
           "accept_share": round(acc, 3), "share_of_c3_step": round(ms_pair / C3_STEP_MS, 7)}
    if radii is not None:
        att = st.t["cnt"][:9].cpu().numpy()
        assert int(att.sum()) == (args.warmup + args.launches) * st.nch and not att[radii[1] + 1:].any()
        out["rmin"], out["rmax"] = radii
        out["attempts_by_radius"] = att[:radii[1] + 1].tolist()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--cells", type=int, default=32, help="inversion cells per axis (C3: 128 / nref 4)")
    ap.add_argument("--nstat", type=int, default=32)
    ap.add_argument("--nev", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2, help="the whole set of measurements, repeated")
    ap.add_argument("--baseline-lib", default=None, help="another libmceik_hip.so for the single-cell pair")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("block_cost.py: no GPU (a timing needs one)")
    from mceik_amd import _lib
    mine = C.CDLL(_lib.LIB_PATH)
    base = C.CDLL(os.path.abspath(args.baseline_lib)) if args.baseline_lib else None
    for _ in range(args.rounds):
        if base is not None:
            measure(torch, "single-cell (baseline lib)", launcher(base, "mcmc_propose"), launcher(base, "mcmc_accept"),
                    args)
        measure(torch, "single-cell", launcher(mine, "mcmc_propose"), launcher(mine, "mcmc_accept"), args)
        for rmax in (0, 2, 8):
            measure(torch, "block", launcher(mine, "block_propose"), launcher(mine, "block_accept"), args,
                    radii=(0, rmax))


if __name__ == "__main__":
    main()
