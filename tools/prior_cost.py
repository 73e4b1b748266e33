#!/usr/bin/env python3
"""What the smoothness / reference-model prior costs: needs a GPU.

Times the prior's two kernels alone (csrc/prior.hip), with device events at the
headline shape (C3: 1024 chains x 32 768 cells):

* prior_fold_kernel, the one kernel a step gains, on pending block proposals
  of radii [0, rmax] for rmax = 0, 2 and 8 (and every proposal at radius 8, the
  largest footprint: 18^3 lower cells per chain), with a reference model, so
  both energies are evaluated;
* prior_energy_kernel, the on-demand full sum, with the bytes it has to read
  (every chain's model once and the reference model) against 8 TB/s.

The kernels are reached through the library's internal launchers (block_propose,
prior_fold, prior_energy; C++ symbols of libmceik_hip.so) on the chain state of
tools/block_cost.py plus a ctypes mirror of PriorDev (csrc/prior.h), which must
follow that struct.  One block_propose makes the pending proposals; the fold is
then launched --launches times on them (it rewrites prop_logu each time, which
costs the same).  A warm-up first.  One JSON line per measurement on stdout;
share_of_c3_step is against one C3 step (1565 ms, README).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import block_cost as bc  # noqa: E402

_P = C.c_void_p
HBM_TBS = 8.0


class PriorDev(C.Structure):
    """csrc/prior.h PriorDev."""
    _fields_ = [(n, C.c_double) for n in ("ws0", "ws1", "wd0", "wd1")] + [("vref", _P), ("dE", _P)]


_SYMS = {"prior_fold": ("_Z10prior_foldRK7McmcDevRK8BlockDevRK8PriorDevbP12ihipStream_t", [_P, _P, _P, C.c_bool, _P]),
         "prior_energy": ("_Z12prior_energyRK7McmcDevRK8BlockDevRK8PriorDevPyS8_P12ihipStream_t",
                          [_P, _P, _P, _P, _P, _P])}


def launcher(lib, name):
    sym, argtypes = _SYMS[name]
    f = getattr(lib, sym)
    f.restype = C.c_int
    f.argtypes = argtypes
    return f


def prior_state(torch, st, ncell):
    """The prior's device arrays beside a block_cost State; models with structure, so no energy is trivially 0."""
    dev = st.t["v"].device
    g = torch.Generator(device="cpu").manual_seed(7)
    st.t["v"].copy_(torch.randint(4000, 6001, st.t["v"].shape, generator=g, dtype=torch.int32).to(dev))
    st.t["vref"] = torch.full((ncell,), 5000, dtype=torch.int32, device=dev)
    st.t["dE"] = torch.zeros((st.nch, 2), dtype=torch.int64, device=dev)
    st.t["E"] = torch.zeros((2, st.nch), dtype=torch.int64, device=dev)
    P = PriorDev()
    P.ws0 = P.ws1 = 1.0 / (2.0 * 200.0 * 200.0)
    P.wd0 = P.wd1 = 1.0 / (2.0 * 500.0 * 500.0)
    P.vref, P.dE = st.t["vref"].data_ptr(), st.t["dE"].data_ptr()
    return P


def timed(torch, stream, n, launch):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    for _ in range(n):
        launch()
    ev[1].record(stream)
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


def measure_fold(torch, lib, args, radii):
    st = bc.State(torch, args.chains, args.cells, args.nstat, args.nev)
    P = prior_state(torch, st, args.cells ** 3)
    st.B.rmin, st.B.rmax = radii
    stream = torch.cuda.current_stream()
    sp = _P(stream.cuda_stream)
    propose, fold = bc.launcher(lib, "block_propose"), launcher(lib, "prior_fold")
    if propose(C.byref(st.D), C.byref(st.B), 3, sp) != 0:
        sys.exit("prior_cost.py: block_propose failed")

    def one():
        if fold(C.byref(st.D), C.byref(st.B), C.byref(P), True, sp) != 0:
            sys.exit("prior_cost.py: prior_fold failed")

    for _ in range(args.warmup):
        one()
    ms = timed(torch, stream, args.launches, one)
    de = st.t["dE"].cpu().numpy()
    inp = st.t["prop_inprior"].cpu().numpy()
    assert inp.all() and de[:, 0].any() and de[:, 1].any()          # models mid-box: every proposal is evaluated
    print(json.dumps({"what": "prior_fold", "chains": st.nch, "cells": args.cells ** 3, "rmin": radii[0],
                      "rmax": radii[1], "launches": args.launches, "ms_per_launch": round(ms, 5),
                      "share_of_c3_step": round(ms / bc.C3_STEP_MS, 8)}), flush=True)


def measure_energy(torch, lib, args):
    st = bc.State(torch, args.chains, args.cells, args.nstat, args.nev)
    ncell = args.cells ** 3
    P = prior_state(torch, st, ncell)
    stream = torch.cuda.current_stream()
    sp = _P(stream.cuda_stream)
    energy = launcher(lib, "prior_energy")
    E = st.t["E"]

    def one():
        E.zero_()
        if energy(C.byref(st.D), C.byref(st.B), C.byref(P), E[0].data_ptr(), E[1].data_ptr(), sp) != 0:
            sys.exit("prior_cost.py: prior_energy failed")

    for _ in range(args.warmup):
        one()
    ms = timed(torch, stream, args.launches, one)
    v = st.t["v"][0].cpu().numpy().astype("int64").reshape(args.cells, args.cells, args.cells)
    want = sum(int((np.diff(v, axis=ax) ** 2).sum()) for ax in range(3))
    assert int(E[0, 0]) == want and int(E[1, 0]) == int(((v - 5000) ** 2).sum())
    nbytes = st.nch * ncell * 4 + ncell * 4
    print(json.dumps({"what": "prior_energy (with the memset of its 2 x nchains sums)", "chains": st.nch, "cells": ncell,
                      "launches": args.launches, "ms_per_launch": round(ms, 5), "bytes_read": nbytes,
                      "GBps": round(nbytes / ms * 1e-6, 1), "share_of_8TBps": round(nbytes / ms * 1e-9 / HBM_TBS, 4),
                      "share_of_c3_step": round(ms / bc.C3_STEP_MS, 8)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--cells", type=int, default=32, help="inversion cells per axis (C3: 128 / nref 4)")
    ap.add_argument("--nstat", type=int, default=32)
    ap.add_argument("--nev", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2, help="the whole set of measurements, repeated")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("prior_cost.py: no GPU (a timing needs one)")
    from mceik_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for _ in range(args.rounds):
        for radii in ((0, 0), (0, 2), (0, 8), (8, 8)):
            measure_fold(torch, lib, args, radii)
        measure_energy(torch, lib, args)


if __name__ == "__main__":
    main()
