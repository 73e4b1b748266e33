"""Hypocentre moves on the GPU (csrc/hypo.hip, include/mceik.h mceik_mcmc_hypo_*,
mceik_eikonal.h mceik_fsm_batch.ev_stride), the rule restated
here in Python and compared bit for bit.

Every chain carries a node (ix, iy, iz) per event.  With every = K global step
gs is a hypocentre step iff gs % K == K - 1; event e of chain c (global id gid)
draws Philox4x32-10 with counter {gs lo, gs hi, 2, e} and key {gid, seed}:

    d[a] = ((r[a] * (2 dmax[a] + 1)) >> 32) - dmax[a];  log u = det_log((r[3] + 0.5) / 2^32)
    candidate = current + d, inside iff lo <= candidate <= hi on every axis
    accept iff inside and log u < beta * (obj_cur - obj_cand)      (beta only with tempering)
    logL = 0; logL = logL - obj_sel[e] in event order

The tables of the chain's models at [current | candidate] are the oracle's CPU
forward on a copy of the problem with nevents = 2 nev, one event's objfn the
oracle's logL on a one-event view (nevents = 1, obs_ptr + e, the event's
column).  Every other step is the oracle's velocity step at the chain's own
nodes; the swap rule is tests/test_gpu_temper.py's, with the positions
travelling with the models.

The picks are analytic, so the whole restatement runs without a GPU: seeds,
dmax and the narrowed box of _CASES were chosen that way, and every restated
test asserts the events it is there for.  Launch paths and grids as
tests/test_gpu_prior.py: per-step 24^3, two pipes 40^3, a multi-step-built
sampler 32^3.
"""
import ctypes as C
import dataclasses
import functools
import types

import numpy as np
import pytest

import _oracle as O
import _refinement as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_PROBLEMS = {}
LADDER3 = np.array([1.0, 0.1, 1e-3])

_PATHS = {
    "per_step": dict(env={"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, n=24),
    "two_pipes": dict(env={"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}, n=40),
    "multi_step": dict(env={"MCEIK_PERSIST": "1"}, n=32),
}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _set_path(path, monkeypatch):
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in _PATHS[path]["env"].items():
        monkeypatch.setenv(k, val)
    return _PATHS[path]["n"]


def _problem(phases="P", n=24, seed=7, nburn=0, keepk=1):
    """4 stations, 6 events, analytic picks.  varObs = 0.005 s^2: one node (100 m) moves a travel time by about
    25 ms and a weighted residual by about 3.5, so hypocentre moves and velocity proposals are both accepted and
    rejected, and log u decides some of the hypocentre moves."""
    from mceik_amd import mcmc
    key = (phases, n)
    if key not in _PROBLEMS:
        p = mcmc.make_problem("C2", n=n, nstat=4, nev=6, seed=7, phases=phases, picks="analytic")
        p.dvmax = 300
        p.var[:] = 0.005
        _PROBLEMS[key] = p
    return dataclasses.replace(_PROBLEMS[key], seed=seed, nburn=nburn, keepk=keepk, _keep=[])


def _same(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i)
        else:
            assert x == y, (what, i)


# --- the restatement ---
class _View:
    """A problem with other event nodes (and CSR rows): what tests/_oracle.make_problem reads, overridden."""

    def __init__(self, p, **kw):
        self._p = p
        self.__dict__.update(kw)

    def __getattr__(self, name):
        return getattr(self._p, name)


def _nodes(p, xyz):
    xyz = np.asarray(xyz, np.int64)
    return ((xyz[..., 2] * p.ny + xyz[..., 1]) * p.nx + xyz[..., 0]).astype(np.int32)


def _catalogue_xyz(p, nch):
    n = p.ev_node.astype(np.int64)
    xyz = np.stack([n % p.nx, n // p.nx % p.ny, n // (p.nx * p.ny)], 1).astype(np.int32)
    return np.repeat(xyz[None], nch, 0).copy()


def _bounding_box(p):
    """The smallest box that holds the catalogue's nodes: events on its faces draw candidates outside it."""
    xyz = _catalogue_xyz(p, 1)[0]
    return tuple(int(x) for x in xyz.min(0)), tuple(int(x) for x in xyz.max(0))


def _hdraw(seed, gid, gs, e, dmax):
    r = [int(x) for x in O.philox([gs & 0xFFFFFFFF, gs >> 32, 2, e], [gid, seed])]
    d = [((r[a] * (2 * dmax[a] + 1)) >> 32) - dmax[a] for a in range(3)]
    return np.array(d, np.int32), O.lib().oracle_det_log((float(r[3]) + 0.5) * (1.0 / 4294967296.0))


def _swap_logu(seed, gs, gid):
    out = O.philox([gs & 0xFFFFFFFF, gs >> 32, 1, 0], [gid, seed])
    return O.lib().oracle_det_log((float(out[0]) + 0.5) * (1.0 / 4294967296.0))


def _at(p, nodes, prec=32):
    """The oracle's problem with the events at `nodes` (len(nodes) events)."""
    return O.make_problem(_View(p, ev_node=np.ascontiguousarray(nodes, np.int32), nevents=len(nodes)), prec)


def _logl_at(p, v, xyz, prec=32):
    P = _at(p, _nodes(p, xyz), prec)
    return O.loglik(P, O.forward_all_f32(P, v))


def _start(p, nch, off, prec=32):
    """The chains' start state without a GPU: the sampler's start models, the catalogue's nodes."""
    from mceik_amd import mcmc
    v0 = mcmc.initial_models(p, range(off, off + nch))
    xyz0 = _catalogue_xyz(p, nch)
    l0 = np.array([_logl_at(p, v0[c].ravel(), xyz0[c], prec) for c in range(nch)])
    return v0, xyz0, l0


def _restate(p, v0, xyz0, logl0, off, nsteps, hyp, betas=None, swap_every=0, step0=0, prec=32):
    """Runs the chains on the CPU.  hyp: None (velocity steps only, at the chains' positions) or (every, dmax, lo,
    hi).  Returns a namespace: v, xyz, logl, naccept, accept [nsteps, nch], hsteps {step index: (cand, acc, obj)},
    hatt / hacc [nev], the moments n / sum / sq, swap_att / swap_acc, events (one record per hypocentre draw),
    vsteps (one per velocity proposal) and swaps (accepted pairs whose positions differed)."""
    nch, nev, nph = len(v0), p.nevents, p.nphase
    v = v0.reshape(nch, -1).copy()
    xyz = np.asarray(xyz0, np.int32).copy()
    logl = logl0.copy()
    nacc = np.zeros(nch, np.int64)
    nt = len(betas) if betas is not None else 1
    G = nch // nt
    satt, sacc = np.zeros(max(nt - 1, 0), np.int64), np.zeros(max(nt - 1, 0), np.int64)
    flags = np.zeros((nsteps, nch), np.uint8)
    hatt, hacc = np.zeros(nev, np.int64), np.zeros(nev, np.int64)
    mom = types.SimpleNamespace(n=0, sum=np.zeros((nev, 3), np.int64), sq=np.zeros((nev, 6), np.int64))
    one = [O.make_problem(_View(p, nevents=1, obs_ptr=np.ascontiguousarray(p.obs_ptr[e:e + 2]),
                                ev_node=np.zeros(1, np.int32)), prec) for e in range(nev)]
    hsteps, events, vsteps, swaps = {}, [], [], []
    moved = np.zeros(nch, bool)
    for i, gs in enumerate(range(step0, step0 + nsteps)):
        if nt > 1 and swap_every > 0 and gs > 0 and gs % swap_every == 0:
            for r in range((gs // swap_every) & 1, nt - 1, 2):
                for g in range(G):
                    a, b = r * G + g, (r + 1) * G + g
                    satt[r] += 1
                    if _swap_logu(p.seed, gs, off + a) < (betas[r] - betas[r + 1]) * (logl[b] - logl[a]):
                        if (xyz[a] != xyz[b]).any():
                            swaps.append((i, a, b))
                        v[[a, b]] = v[[b, a]]
                        xyz[[a, b]] = xyz[[b, a]]
                        logl[[a, b]] = logl[[b, a]]
                        moved[[a, b]] = moved[[b, a]]
                        sacc[r] += 1
        if hyp is not None and hyp[0] > 0 and gs % hyp[0] == hyp[0] - 1:
            every, dmax, lo, hi = hyp
            cand, acc, obj = np.zeros((nch, nev, 3), np.int32), np.zeros((nch, nev), np.uint8), np.zeros((nch, nev, 2))
            for c in range(nch):
                logu, inside = np.zeros(nev), np.zeros(nev, bool)
                for e in range(nev):
                    d, logu[e] = _hdraw(p.seed, off + c, gs, e, dmax)
                    cand[c, e] = xyz[c, e] + d
                    inside[e] = all(lo[a] <= cand[c, e, a] <= hi[a] for a in range(3))
                cur = _nodes(p, xyz[c])
                P2 = _at(p, np.concatenate([cur, np.where(inside, _nodes(p, cand[c]), cur)]), prec)
                tt = O.forward_all_f32(P2, v[c])                        # [nphase][nstat][2 nev]
                ln = 0.0
                for e in range(nev):
                    oc = 0.0 - O.loglik(one[e], tt[:, :, e:e + 1])
                    od = 0.0 - O.loglik(one[e], tt[:, :, nev + e:nev + e + 1])
                    obj[c, e] = oc, od
                    a = bool(inside[e]) and (logu[e] < betas[c // G] * (oc - od) if nt > 1 else logu[e] < oc - od)
                    acc[c, e] = a
                    ln = ln - (od if a else oc)
                    hatt[e] += 1
                    hacc[e] += a
                    events.append(types.SimpleNamespace(step=i, chain=c, e=e, inside=bool(inside[e]), acc=a,
                                                        moved=a and bool((cand[c, e] != xyz[c, e]).any()),
                                                        by_logu=bool(inside[e]) and (oc - od < 0.0) and a))
                    if a:
                        moved[c] |= bool((cand[c, e] != xyz[c, e]).any())
                        xyz[c, e] = cand[c, e]
                logl[c] = ln
            hsteps[i] = (cand, acc, obj)
        else:
            for c in range(nch):
                P = _at(p, _nodes(p, xyz[c]), prec)
                cell, vn, inp, logu = O.propose(P, off + c, gs, v[c])
                a = False
                if inp:
                    vp = v[c].copy()
                    vp[cell] = vn
                    ln = O.loglik(P, O.forward_all_f32(P, vp))
                    dl = ln - logl[c]
                    a = bool(logu < betas[c // G] * dl) if nt > 1 else bool(logu < dl)
                    if a:
                        v[c], logl[c], nacc[c] = vp, ln, nacc[c] + 1
                flags[i, c] = a
                vsteps.append(types.SimpleNamespace(step=i, chain=c, inp=inp, acc=a, moved=bool(moved[c]),
                                                    ph=cell // p.ncell))
        if hyp is not None and gs >= p.nburn and (gs - p.nburn) % p.keepk == 0:
            q = xyz[:G].astype(np.int64)
            mom.n += G
            mom.sum += q.sum(0)
            for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
                mom.sq[:, k] += (q[:, :, a] * q[:, :, b]).sum(0)
    return types.SimpleNamespace(v=v.reshape(v0.shape), xyz=xyz, logl=logl, naccept=nacc, accept=flags, hsteps=hsteps,
                                 hatt=hatt, hacc=hacc, mom=mom, swap_att=satt, swap_acc=sacc, events=events,
                                 vsteps=vsteps, swaps=swaps)


def _assert_events(r):
    ev = r.events
    assert any(e.moved for e in ev), "no accepted move that changes a node"
    assert any(e.inside and not e.acc for e in ev), "no rejection inside the box"
    out = [e for e in ev if not e.inside]
    assert out and not any(e.acc for e in out), "no candidate outside the box"
    # a velocity step of a chain whose events have moved, accepted and rejected: logL at the new nodes
    assert any(s.moved and s.acc for s in r.vsteps) and any(s.moved and s.inp and not s.acc for s in r.vsteps)


def _moments(smp):
    m = smp.hypo_moments()
    return m["n"], m["sum"], m["sq"]


def _recomputed_logl(smp):
    """logL after restore(..., recompute_logl=True): one full forward at the chains' models and positions."""
    ck = smp.checkpoint()
    smp.restore(ck, recompute_logl=True)
    return ck["logl"], smp.state()[1]


# --- 1. per-model event lists of a batch ---
H = 100.0
_N4 = (21, 20, 27)             # no axis a multiple of the 8-node tile; four 8-z bricks, which the 16-z instance needs
# one case per row of tests/_refinement.py (the row's first instance, on the row's geometry), an fp64 and a
# forced 8-z instance, and at nref 4 on a ragged grid the fixed-layout 16-z instance with its 8-z and fp64 twins
_BATCH = [(rid, geo, nref) + cells[0] for rid, geo, nref, cells in R._ROWS] + [
    ("n664", R.G, (6, 6, 4), 64, True, 0, R.Z4_KB64), ("n664", R.G, (6, 6, 4), 32, True, 8, R.Z4_KB32),
    ("n4", _N4, (4, 4, 4), 32, True, 0, R.FSM16_FT), ("n4", _N4, (4, 4, 4), 32, True, 8, R.Z4_KB32),
    ("n4", _N4, (4, 4, 4), 64, True, 0, R.Z4_KB64)]
_BATCH_IDS = ["%s-f%d%s" % (c[0], c[3], "-z8" if c[5] else "") for c in _BATCH]
NMODEL, NSTAT, NEV = 3, 2, 5


@functools.lru_cache(maxsize=None)
def _batch_inputs(geo, nref):
    nx, ny, nz = geo
    ncx, ncy, ncz = [-(-a // r) for a, r in zip(geo, nref)]
    rng = np.random.default_rng([43, nx, ny, nz, *nref])
    v = rng.integers(2500, 6501, (NMODEL, ncz, ncy, ncx)).astype(np.int32)
    scell = (1.0 / v.astype(np.float32)).astype(np.float32)
    src = np.array([[[0.0, 1234.5, 987.6, (nz - 1) * H]], [[0.1, 1500.0, 1200.0, 700.0]]])
    # every model its own nodes: the grid's last node among them, the lists pairwise different
    ev = rng.integers(0, nx * ny * nz, (NMODEL, NEV)).astype(np.int32)
    ev[NMODEL - 1, NEV - 1] = nx * ny * nz - 1
    assert len({tuple(r) for r in ev}) == NMODEL
    return scell, src, ev


@functools.lru_cache(maxsize=None)
def _batch_twin(geo, nref, precision):
    """The twin's fields [NMODEL * NSTAT][n] on the expanded node fields (callers do not modify them)."""
    scell, src, _ = _batch_inputs(geo, nref)
    nx, ny, nz = geo
    dt = np.float32 if precision == 32 else np.float64
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    out = []
    for m in range(NMODEL):
        sfield = scell[m][k // nref[2], j // nref[1], i // nref[0]].ravel().astype(dt)
        for s in range(NSTAT):
            out.append(O.eikonal_solve(*geo, sfield, H, src[s], dtype=dt)[0])
    return out


def _batch_solve(case, ev, ev_frac=None, max_waves=0):
    from mceik_amd import _lib
    from mceik_amd.eikonal import BatchSolver
    _, geo, nref, precision, fast, step_z, want = case
    dev = _dev()
    scell, src, _ = _batch_inputs(geo, nref)
    bs = BatchSolver(*geo, H, 0.0, 0.0, 0.0, 50, 1e-8, precision, nref=nref, fast_sqrt=fast)
    kname = _lib.lib().mceik_fsm_kernel_name(C.byref(bs.describe(NMODEL, NSTAT, 1, 1, nev=NEV, step_z=step_z))).decode()
    assert kname == want, kname
    out = bs.solve(torch.tensor(src), torch.tensor(scell.reshape(NMODEL, -1), device=dev), ev_node=torch.tensor(ev),
                   step_z=step_z, ev_frac=ev_frac, max_waves=max_waves)
    torch.cuda.synchronize(dev)
    return out["ttab"].cpu().numpy()


@pytest.mark.parametrize("case", _BATCH, ids=_BATCH_IDS)
def test_batch_per_model_event_lists(case):
    """3 models x 2 stations, 5 events per model at different nodes: ttab[m * nstat + s][e] is the twin's field
    of solve (m, s) at model m's node e; the shared list repeated per model gives the shared list's tables."""
    _, geo, nref, precision, _, _, _ = case
    _, _, ev = _batch_inputs(geo, nref)
    tt = _batch_solve(case, ev)
    twin = _batch_twin(geo, nref, precision)
    want = np.stack([twin[q][ev[q // NSTAT]].astype(np.float32) for q in range(NMODEL * NSTAT)])
    assert tt.shape == (NMODEL * NSTAT, NEV) and tt.tobytes() == want.tobytes()
    # not vacuous: with model 0's list for everyone the other models' rows would differ
    shared = np.stack([twin[q][ev[0]].astype(np.float32) for q in range(NMODEL * NSTAT)])
    assert (shared[NSTAT:] != want[NSTAT:]).any()
    assert _batch_solve(case, ev[0]).tobytes() == shared.tobytes()                  # ev_stride = 0: today's shared list
    assert _batch_solve(case, np.repeat(ev[:1], NMODEL, 0)).tobytes() == shared.tobytes()
    # one wave takes the six solves in turn: the row offset follows the solve, not the wave
    assert _batch_solve(case, ev, max_waves=1).tobytes() == want.tobytes()


def test_batch_per_model_event_lists_trilinear():
    """ev_frac with per-model lists: fractions [nmodel][nev][3] beside the corner nodes."""
    case = _BATCH[_BATCH_IDS.index("n4-f32")]
    _, geo, nref, precision, _, _, _ = case
    nx, ny, nz = geo
    rng = np.random.default_rng(5)
    ix, iy, iz = (rng.integers(0, n - 1, (NMODEL, NEV)) for n in geo)
    ev = ((iz * ny + iy) * nx + ix).astype(np.int32)
    w = rng.random((NMODEL, NEV, 3)).astype(np.float32)
    w[0, 0] = 0.0, 1.0, 0.5
    tt = _batch_solve(case, ev, ev_frac=w)
    twin = _batch_twin(geo, nref, precision)
    want = np.array([[O.event_time(twin[q], nx, ny, nz, ev[q // NSTAT, e], w[q // NSTAT, e]) for e in range(NEV)]
                     for q in range(NMODEL * NSTAT)], np.float32)
    assert tt.tobytes() == want.tobytes()
    other = np.array([[O.event_time(twin[q], nx, ny, nz, ev[q // NSTAT, e], w[0, e]) for e in range(NEV)]
                      for q in range(NMODEL * NSTAT)], np.float32)
    assert (other[NSTAT:] != want[NSTAT:]).any()                                   # the fractions are per model too


# --- 2., 3., 11. the restated run ---
# seed and dmax chosen on the CPU (the restatement alone) so that every event _assert_events names happens within
# the steps; the box is the catalogue's bounding box, so events on its faces draw candidates outside it
_CASES = {
    "P-per_step": dict(phases="P", path="per_step", seed=7, nch=4, nsteps=12, dmax=(1, 1, 1), precision=32),
    "PS-two_pipes": dict(phases="PS", path="two_pipes", seed=8, nch=4, nsteps=8, dmax=(1, 2, 1), precision=32),
    "P-per_step-f64": dict(phases="P", path="per_step", seed=7, nch=4, nsteps=4, dmax=(1, 1, 1), precision=64),
}
EVERY, OFF = 2, 5


@pytest.mark.parametrize("case", list(_CASES))
def test_restated_run(case, monkeypatch):
    """Positions, candidates, per-event flags, both objfn, logL, v and the velocity accept sequence, step by
    step; with two models the kept S / P tables after accepted moves show in the next velocity step's logL."""
    _dev()
    cfg = _CASES[case]
    from mceik_amd import mcmc
    p = _problem(cfg["phases"], n=_set_path(cfg["path"], monkeypatch), seed=cfg["seed"])
    nch, nsteps, prec = cfg["nch"], cfg["nsteps"], cfg["precision"]
    lo, hi = _bounding_box(p)
    smp = mcmc.Sampler(p, nchains=nch, chain_offset=OFF, precision=prec)
    smp.hypo_enable(EVERY, dmax=cfg["dmax"], box=(lo, hi))
    info = smp.info()
    assert not info["multi_step"] and info["npipe"] == (2 if cfg["path"] == "two_pipes" else 1), info
    v0, l0, _, _ = smp.state()
    xyz0 = smp.hypo_positions()
    w0 = _start(p, nch, OFF, prec)
    _same((v0, xyz0, l0), w0, case + ": start")
    r = _restate(p, v0, xyz0, l0, OFF, nsteps, (EVERY, cfg["dmax"], lo, hi), prec=prec)
    if prec == 32:
        _assert_events(r)
    else:
        assert any(e.moved for e in r.events) and any(e.inside and not e.acc for e in r.events)
    for i in range(nsteps):
        smp.run(1)
        acc = smp.last()[2]
        _same((acc,), (r.accept[i],), case + f": accept flags of step {i}")
        if i in r.hsteps:
            assert not acc.any()
            _same(smp.hypo_last(), r.hsteps[i], case + f": hypocentre step {i}")
    v, logl, nacc, step = smp.state()
    assert step == nsteps
    _same((v, smp.hypo_positions(), logl, nacc), (r.v, r.xyz, r.logl, r.naccept), case)
    _same(smp.hypo_stats(), (r.hatt, r.hacc), case + ": counters")
    _same(_moments(smp), (r.mom.n, r.mom.sum, r.mom.sq), case + ": moments")
    assert r.naccept.sum() > 0 and (r.xyz != xyz0).any()
    # 5. logL is what a full forward at the chains' models and positions gives
    kept, fresh = _recomputed_logl(smp)
    smp.close()
    assert kept.tobytes() == fresh.tobytes() == r.logl.tobytes()


# --- 4. a multi-step-built sampler ---
def test_multi_step_built(monkeypatch):
    _dev()
    from mceik_amd import mcmc
    p = _problem("P", n=_set_path("multi_step", monkeypatch), seed=7)
    nch, n1, n2 = 4, 6, 4
    lo, hi = _bounding_box(p)
    smp = mcmc.Sampler(p, nchains=nch, chain_offset=OFF)
    assert smp.info()["multi_step"]
    smp.hypo_enable(EVERY, dmax=(1, 1, 1), box=(lo, hi))
    assert not smp.info()["multi_step"]
    v0, l0, _, _ = smp.state()
    xyz0 = smp.hypo_positions()
    r1 = _restate(p, v0, xyz0, l0, OFF, n1, (EVERY, (1, 1, 1), lo, hi))
    assert any(e.moved for e in r1.events) and len({r1.xyz[c].tobytes() for c in range(nch)}) > 1
    smp.run(n1)
    _same(smp.state()[:3] + (smp.hypo_positions(),), (r1.v, r1.logl, r1.naccept, r1.xyz), "enabled")
    smp.hypo_disable()
    assert smp.info()["multi_step"]
    # multi-step launches with every chain's own nodes (ev_stride = nev), velocity steps only
    r2 = _restate(p, r1.v, r1.xyz, r1.logl, OFF, n2, None, step0=n1)
    assert r2.naccept.sum() > 0 and any(s.inp and not s.acc for s in r2.vsteps)
    smp.run(n2)
    v, logl, nacc, step = smp.state()
    assert step == n1 + n2
    _same((v, logl, nacc - r1.naccept, smp.last()[2], smp.hypo_positions()),
          (r2.v, r2.logl, r2.naccept, r2.accept[-1], r1.xyz), "after disable")
    kept, fresh = _recomputed_logl(smp)
    smp.close()
    assert kept.tobytes() == fresh.tobytes()


# --- 6. enabled, no hypocentre step within the run ---
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_enabled_without_a_hypocentre_step_is_the_plain_sampler(phases, monkeypatch):
    _dev()
    from mceik_amd import mcmc
    p = _problem(phases, n=_set_path("per_step", monkeypatch), seed=8)
    nsteps = 6

    def run(enable):
        s = mcmc.Sampler(p, nchains=4, chain_offset=OFF, max_samples=nsteps)
        if enable:
            s.hypo_enable(1000)
        flags = []
        for _ in range(nsteps):
            s.run(1)
            flags.append(s.last()[2])
        out = s.state() + (np.stack(flags),) + s.samples()
        xyz = s.hypo_positions() if enable else None
        s.close()
        return out, xyz

    plain, _ = run(False)
    on, xyz = run(True)
    _same(plain, on, "every past the run")
    assert plain[2].sum() > 0 and xyz.tobytes() == _catalogue_xyz(p, 4).tobytes()


# --- 7. tempering ---
def test_with_tempering(monkeypatch):
    """A 3-rung ladder: swaps carry the positions, the moments see the cold chains only."""
    _dev()
    from mceik_amd import mcmc
    p = _problem("P", n=_set_path("per_step", monkeypatch), seed=7)
    nch, nsteps = 6, 8                                   # G = 2
    lo, hi = _bounding_box(p)
    smp = mcmc.Sampler(p, nchains=nch, chain_offset=OFF)
    smp.temper_enable(betas=LADDER3, swap_every=1)
    smp.hypo_enable(EVERY, dmax=(1, 1, 1), box=(lo, hi))
    v0, l0, _, _ = smp.state()
    xyz0 = smp.hypo_positions()
    r = _restate(p, v0, xyz0, l0, OFF, nsteps, (EVERY, (1, 1, 1), lo, hi), betas=LADDER3, swap_every=1)
    # accepted swaps between chains at different positions: one that reaches a cold chain, one between hot rungs
    assert any(a < 2 for _, a, _ in r.swaps) and any(a >= 2 for _, a, _ in r.swaps), r.swaps
    assert any(e.moved for e in r.events) and any(e.inside and not e.acc for e in r.events)
    assert r.mom.n == 2 * nsteps
    smp.run(nsteps)
    v, logl, nacc, _ = smp.state()
    _same((v, smp.hypo_positions(), logl, nacc), (r.v, r.xyz, r.logl, r.naccept), "tempered")
    _same(smp.temper_stats(), (r.swap_att, r.swap_acc), "swap counters")
    _same(smp.hypo_stats(), (r.hatt, r.hacc), "counters")
    _same(_moments(smp), (r.mom.n, r.mom.sum, r.mom.sq), "moments of the cold chains")
    kept, fresh = _recomputed_logl(smp)
    smp.close()
    assert kept.tobytes() == fresh.tobytes()


# --- 8. checkpoint / restore ---
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_checkpoint(phases, monkeypatch):
    """6 steps = 3 + checkpoint + restore + 3.  One model: hypo_set, restore with the saved logL, moments_set.
    Two models: the restore runs its forward, as every two-model resume does (the current tables of both models
    come from it); its logL is the saved one."""
    _dev()
    from mceik_amd import mcmc
    p = _problem(phases, n=_set_path("per_step", monkeypatch), seed=8)
    nch = 4
    lo, hi = _bounding_box(p)
    opts = dict(dmax=(1, 2, 1), box=(lo, hi))

    def done(s):
        out = s.state() + (s.hypo_positions(),) + s.hypo_stats() + _moments(s) + s.hypo_last()
        s.close()
        return out

    a = mcmc.Sampler(p, nchains=nch, chain_offset=OFF)
    a.hypo_enable(EVERY, **opts)
    a.run(6)
    ra = done(a)
    b = mcmc.Sampler(p, nchains=nch, chain_offset=OFF)
    b.hypo_enable(EVERY, **opts)
    b.run(3)
    ck = b.checkpoint()
    b.close()
    assert ck["step"] == 3 and ck["hypo"]["n"] == 3 * nch and ck["hypo"]["attempts"].sum() == nch * p.nevents
    assert (ck["hypo"]["xyz"] != _catalogue_xyz(p, nch)).any()
    for bad in (dict(opts, dmax=(1, 1, 1)), None):
        c = mcmc.Sampler(p, nchains=nch, chain_offset=OFF)
        if bad is not None:
            c.hypo_enable(EVERY, **bad)
        with pytest.raises(ValueError):
            c.restore(ck)
        c.close()
    d = mcmc.Sampler(p, nchains=nch, chain_offset=OFF)
    d.hypo_enable(EVERY, **opts)
    d.restore(ck, recompute_logl=phases == "PS")
    assert d.hypo_positions().tobytes() == ck["hypo"]["xyz"].tobytes()
    assert d.state()[1].tobytes() == ck["logl"].tobytes()
    d.run(3)
    _same(ra, done(d), "3 + checkpoint + restore + 3")
    if phases == "P":                                   # the restore's own forward gives the saved logL too
        e = mcmc.Sampler(p, nchains=nch, chain_offset=OFF)
        e.hypo_enable(EVERY, **opts)
        e.restore(ck, recompute_logl=True)
        assert e.state()[1].tobytes() == ck["logl"].tobytes()
        e.run(3)
        _same(ra, done(e), "3 + checkpoint + restore with a forward + 3")
    assert ra[2].sum() > 0 and ra[5].sum() > 0


# --- 9. the moments ---
def test_moments(monkeypatch):
    """nburn 3, keepK 2: exact int64 sums over the restated kept states, and the summary in metres."""
    _dev()
    from mceik_amd import mcmc
    p = _problem("P", n=_set_path("per_step", monkeypatch), seed=7, nburn=3, keepk=2)
    nch, nsteps = 4, 10
    lo, hi = _bounding_box(p)
    smp = mcmc.Sampler(p, nchains=nch, chain_offset=OFF)
    smp.hypo_enable(EVERY, dmax=(1, 1, 1), box=(lo, hi))
    v0, l0, _, _ = smp.state()
    xyz0 = smp.hypo_positions()
    r = _restate(p, v0, xyz0, l0, OFF, nsteps, (EVERY, (1, 1, 1), lo, hi))
    assert r.mom.n == 4 * nch                           # steps 3, 5, 7, 9
    smp.run(nsteps)
    n, sm, sq = _moments(smp)
    _same((n, sm, sq), (r.mom.n, r.mom.sum, r.mom.sq), "moments")
    mean, cov = smp.hypo_summary()
    mu = sm / n
    assert np.array_equal(mean, np.array([p.x0, p.y0, p.z0]) + p.h * mu)
    assert np.allclose(cov[:, 0, 1], (sq[:, 3] / n - mu[:, 0] * mu[:, 1]) * p.h ** 2, rtol=0, atol=1e-6)
    assert np.array_equal(cov, cov.transpose(0, 2, 1)) and (np.einsum("eii->ei", cov) >= -1e-6).all()
    assert (np.einsum("eii->ei", cov) > 0).any()        # some event's kept positions differ
    smp.hypo_enable(EVERY, dmax=(1, 1, 1), box=(lo, hi))
    assert _moments(smp)[0] == 0 and not _moments(smp)[1].any() and not smp.hypo_stats()[0].any()   # enable resets
    smp.close()


# --- 10. refusals ---
def test_refusals(monkeypatch):
    from mceik_amd import _lib, mcmc
    _dev()
    n = _set_path("per_step", monkeypatch)
    p = _problem("P")
    s = mcmc.Sampler(p, nchains=4)
    L = _lib.lib()
    lo, hi = _bounding_box(p)

    def opts(every=2, dmax=(1, 1, 1), lo=(0, 0, 0), hi=(n - 1, n - 1, n - 1)):
        o = _lib.HypoOpts()
        o.every = every
        for a in range(3):
            o.dmax[a], o.lo[a], o.hi[a] = dmax[a], lo[a], hi[a]
        return o

    xyz = np.zeros((4, p.nevents, 3), np.int32)
    ptr = xyz.ctypes.data_as(C.c_void_p)
    # before the first enable
    assert L.mceik_mcmc_hypo_get(s._h, None, ptr) == 1 and L.mceik_mcmc_hypo_set(s._h, ptr) == 1
    assert L.mceik_mcmc_hypo_stats(s._h, None, None, 0) == 1 and L.mceik_mcmc_hypo_last(s._h, None, None, None) == 1
    assert L.mceik_mcmc_hypo_moments_get(s._h, None, None, None) == 1
    assert L.mceik_mcmc_hypo_disable(s._h) == 0 and L.mceik_mcmc_hypo_disable(None) == 1
    assert L.mceik_mcmc_hypo_enable(s._h, None) == 1 and L.mceik_mcmc_hypo_enable(None, C.byref(opts())) == 1
    for bad in (opts(every=-1), opts(dmax=(1, -1, 1)), opts(lo=(5, 0, 0), hi=(4, n - 1, n - 1)),
                opts(lo=(-1, 0, 0)), opts(hi=(n - 1, n, n - 1)),
                opts(lo=lo, hi=(hi[0] - 1, hi[1], hi[2])),            # an event of the catalogue outside the box
                opts(lo=(lo[0], lo[1] + 1, lo[2]), hi=hi)):
        assert L.mceik_mcmc_hypo_enable(s._h, C.byref(bad)) == 1
    assert L.mceik_mcmc_hypo_get(s._h, None, ptr) == 1                 # still off, nothing allocated
    with pytest.raises(ValueError):
        s.hypo_enable(2, dmax=(1, 1))
    # an enabled posterior that holds states refuses, as tempering and the prior do
    s.posterior_enable(per_chain=True, nbins=0)
    s.run(1)
    with pytest.raises(ValueError):
        s.hypo_enable(2)
    s.posterior_disable()
    s.hypo_enable(2, box=(lo, hi))
    o = _lib.HypoOpts()
    assert L.mceik_mcmc_hypo_get(s._h, C.byref(o), ptr) == 0
    assert (o.every, tuple(o.dmax), tuple(o.lo), tuple(o.hi)) == (2, (1, 1, 1), lo, hi)
    assert xyz.tobytes() == _catalogue_xyz(p, 4).tobytes()
    # hypo_set: outside the box while enabled, outside the grid after disable
    out = xyz.copy()
    out[3, 5, 0] = hi[0] + 1
    with pytest.raises(ValueError):
        s.hypo_set(out)
    with pytest.raises(ValueError):
        s.hypo_set(xyz[:3])
    s.hypo_disable()
    assert L.mceik_mcmc_hypo_get(s._h, C.byref(o), None) == 0 and o.every == 0
    if hi[0] + 1 < n:
        s.hypo_set(out)                                 # inside the grid: fine once the box is off
        assert s.hypo_positions().tobytes() == out.tobytes()
        with pytest.raises(ValueError):
            s.hypo_enable(2, box=(lo, hi))              # a chain's current position outside the box
    out[3, 5, 0] = n
    with pytest.raises(ValueError):
        s.hypo_set(out)
    assert L.mceik_mcmc_hypo_moments_set(s._h, -1, ptr, ptr) == 1
    s.close()
    # trilinear mode: integer node moves with fixed fractions have no meaning
    pt = dataclasses.replace(_problem("P"), tt_interp=1, _keep=[])
    t = mcmc.Sampler(pt, nchains=2)
    with pytest.raises(ValueError):
        t.hypo_enable(2)
    t.close()


def test_hypo_set_recomputes_logl(monkeypatch):
    """hypo_set's forward: logL at arbitrary per-chain positions == the oracle's, one and two models."""
    _dev()
    from mceik_amd import mcmc
    for phases in ("P", "PS"):
        p = _problem(phases, n=_set_path("per_step", monkeypatch), seed=8)
        s = mcmc.Sampler(p, nchains=3, chain_offset=OFF)
        s.hypo_enable(0)
        rng = np.random.default_rng(3)
        xyz = rng.integers(0, p.nx, (3, p.nevents, 3)).astype(np.int32)
        s.hypo_set(xyz)
        v, logl, _, _ = s.state()
        s.close()
        want = np.array([_logl_at(p, v[c].ravel(), xyz[c]) for c in range(3)])
        assert logl.tobytes() == want.tobytes(), phases
