"""Block proposals on the GPU (csrc/block.hip, include/mceik.h
mceik_mcmc_block_*), every rule restated here in Python and
compared bit for bit.

A step of chain c (global id gid) draws Philox4x32-10 with counter {step lo,
step hi, 0, 0} and key {gid, seed}: centre cell = (r0 * ncm) >> 32, mag = 1 +
((r1 * dvmax) >> 32), minus = r2 & 1, R = rmin + (((r2 >> 1) * (rmax - rmin +
1)) >> 31), logu = det_log((r3 + 0.5) / 2^32).  The footprint
(mcmc.block_footprint, pinned by test_block_host.py) moves the cells of the
centre's model; the proposal is inside the prior iff every touched entry is;
accept iff inside && logu < beta * (ln - logl).  The forward is the oracle's
CPU solver, the logL the oracle's.

The picks are analytic (no GPU forward), so the whole restatement runs without
a GPU: the seeds and the narrowed priors of _CASES were chosen that way, and
every restated test asserts the events it is there for.

Launch paths and grids as tests/test_gpu_temper.py: per-step 24^3, multi-step
32^3, two pipes 40^3 (nref 4: 6^3, 8^3, 10^3 cells).
"""
import dataclasses
import types

import numpy as np
import pytest

import _oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_PROBLEMS = {}
_BIG = types.SimpleNamespace(ncx=17, ncy=17, ncz=17)     # no face within 8 cells of its centre
_BIG_CENTRE = (8 * 17 + 8) * 17 + 8
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


def _check_path(smp, path, block=False):
    info = smp.info()
    assert bool(info["multi_step"]) == (path == "multi_step" and not block), info
    if path != "multi_step":
        assert info["npipe"] == (2 if path == "two_pipes" else 1), info


def _problem(phases="P", n=24, seed=7, prior=None, nburn=0, keepk=1):
    """4 stations, 6 events, analytic picks; `prior` = (vmin, vmax, vsmin, vsmax) narrows the prior (the start
    models are clipped to it), `seed` is the sampler's and the start models'."""
    from mceik_amd import mcmc
    key = (phases, n)
    if key not in _PROBLEMS:
        p = mcmc.make_problem("C2", n=n, nstat=4, nev=6, seed=7, phases=phases, picks="analytic")
        p.dvmax = 300
        p.var[:] = 1e-5
        _PROBLEMS[key] = p
    p = dataclasses.replace(_PROBLEMS[key], seed=seed, nburn=nburn, keepk=keepk, _keep=[])
    if prior is not None:
        p.vmin, p.vmax, p.vsmin, p.vsmax = prior
    return p


def _sampler(p, nchains, block=None, **kw):
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=nchains, **kw)
    if block is not None:
        smp.block_enable(*block)
    return smp


def _same(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i)
        else:
            assert x == y, (what, i)


# --- the restatement ---
def _draw(p, gid, step, rmin, rmax):
    r = [int(x) for x in O.philox([step & 0xFFFFFFFF, step >> 32, 0, 0], [gid, p.seed])]
    ncm = p.nphase * p.ncell
    cell = (r[0] * ncm) >> 32
    mag = 1 + ((r[1] * p.dvmax) >> 32)
    R = rmin + (((r[2] >> 1) * (rmax - rmin + 1)) >> 31)
    logu = O.lib().oracle_det_log((float(r[3]) + 0.5) * (1.0 / 4294967296.0))
    return cell, (-mag if r[2] & 1 else mag), R, logu


def _swap_logu(seed, gs, gid):
    out = O.philox([gs & 0xFFFFFFFF, gs >> 32, 1, 0], [gid, seed])
    return O.lib().oracle_det_log((float(out[0]) + 0.5) * (1.0 / 4294967296.0))


def _restate(p, v0, logl0, off, nsteps, rmin, rmax, precision=32, betas=None, swap_every=0, step0=0):
    """Runs the chains on the CPU.  Returns a namespace: v, logl, naccept, accept (last step's flags), ttab /
    phase (last step's proposal tables [nch, nstat, nev] and models), attempts / accepts [rmax + 1], swap_att /
    swap_acc, and events: one record per proposal."""
    from mceik_amd import mcmc
    P = O.make_problem(p, precision)
    nch, ncell = len(v0), p.ncell
    v = v0.reshape(nch, -1).copy()
    logl = logl0.copy()
    nacc = np.zeros(nch, np.int64)
    att, acc_r = np.zeros(rmax + 1, np.int64), np.zeros(rmax + 1, np.int64)
    nt = len(betas) if betas is not None else 1
    G = nch // nt
    satt, sacc = np.zeros(max(nt - 1, 0), np.int64), np.zeros(max(nt - 1, 0), np.int64)
    flags = np.zeros(nch, np.uint8)
    ttab = np.zeros((nch, p.nstat, p.nevents), np.float32)
    phase = np.zeros(nch, np.int32)
    bounds = [(p.vmin, p.vmax), (p.vsmin, p.vsmax)]
    events = []
    for gs in range(step0, step0 + nsteps):
        if nt > 1 and swap_every > 0 and gs > 0 and gs % swap_every == 0:
            for r in range((gs // swap_every) & 1, nt - 1, 2):
                for g in range(G):
                    a, b = r * G + g, (r + 1) * G + g
                    satt[r] += 1
                    if _swap_logu(p.seed, gs, off + a) < (betas[r] - betas[r + 1]) * (logl[b] - logl[a]):
                        v[[a, b]] = v[[b, a]]
                        logl[[a, b]] = logl[[b, a]]
                        sacc[r] += 1
        for c in range(nch):
            cell, amp, R, logu = _draw(p, off + c, gs, rmin, rmax)
            ph, cc = divmod(cell, ncell)
            cells, dv = mcmc.block_footprint(p, cc, R, amp)
            full = len(mcmc.block_footprint(_BIG, _BIG_CENTRE, R, amp)[0])
            idx = ph * ncell + cells.astype(np.int64)
            vp = v[c].copy()
            vp[idx] += dv
            lo, hi = bounds[ph]
            inside = (vp[idx] >= lo) & (vp[idx] <= hi)
            inp = bool(inside.all())
            # outside the prior the forward still runs, on the unchanged model
            tt = O.forward_all_f32(P, vp if inp else v[c])
            a = False
            if inp:
                ln = O.loglik(P, tt)
                d = ln - logl[c]
                a = bool(logu < betas[c // G] * d) if nt > 1 else bool(logu < d)
                if a:
                    v[c], logl[c], nacc[c] = vp, ln, nacc[c] + 1
                    acc_r[R] += 1
            att[R] += 1
            flags[c], ttab[c], phase[c] = a, tt[ph], ph
            cz = cells // (p.ncx * p.ncy)
            events.append(types.SimpleNamespace(
                R=R, ph=ph, inp=inp, acc=a, clipped=len(cells) < full, ntouched=len(cells),
                z_face=bool((cz == 0).any() or (cz == p.ncz - 1).any()),
                centre_in=bool(lo <= vp[cell] <= hi)))
    return types.SimpleNamespace(v=v.reshape(v0.shape), logl=logl, naccept=nacc, accept=flags, ttab=ttab,
                                 phase=phase, attempts=att, accepts=acc_r, swap_att=satt, swap_acc=sacc,
                                 events=events)


def _run_gpu(p, nch, off, nsteps, block, precision=32, betas=None, swap_every=0, path=None, order="block_first"):
    """order: block_enable before temper_enable ("block_first") or after it ("temper_first")."""
    assert order in ("block_first", "temper_first")
    smp = _sampler(p, nch, block=block if order == "block_first" else None, chain_offset=off, precision=precision)
    if betas is not None:
        smp.temper_enable(betas=betas, swap_every=swap_every)
    if order == "temper_first":
        smp.block_enable(*block)
    if path is not None:
        _check_path(smp, path, block=True)
    v0, l0, _, _ = smp.state()
    smp.run(nsteps)
    out = types.SimpleNamespace()
    out.v0, out.l0 = v0, l0
    out.v, out.logl, out.naccept, out.step = smp.state()
    out.ttab, _, out.accept = smp.last()
    out.phase = smp.last_phase()
    out.attempts, out.accepts = smp.block_stats()
    if betas is not None:
        out.swap_att, out.swap_acc = smp.temper_stats()
    smp.close()
    return out


def _compare(g, r, nsteps, what):
    assert g.step == nsteps
    _same((g.v, g.logl, g.naccept, g.accept), (r.v, r.logl, r.naccept, r.accept), what + ": state")
    _same((g.attempts, g.accepts), (r.attempts, r.accepts), what + ": counters")
    _same((g.phase, g.ttab), (r.phase, r.ttab), what + ": proposal tables")


# --- 1. radius 0 is the plain sampler ---
@pytest.mark.parametrize("phases", ["P", "PS"])
@pytest.mark.parametrize("path", ["per_step", "multi_step", "two_pipes"])
def test_radius_zero_is_the_plain_sampler(path, phases, monkeypatch):
    _dev()
    p = _problem(phases, n=_set_path(path, monkeypatch))
    nch = 6

    def done(s):
        out = s.state() + (s.last()[2],)
        s.close()
        return out

    a = _sampler(p, nch, chain_offset=5)
    _check_path(a, path)
    a.run(6)
    ra = done(a)
    b = _sampler(p, nch, block=(0, 0), chain_offset=5)
    _check_path(b, path, block=True)
    b.run(6)
    att, acc = b.block_stats()
    rb = done(b)
    _same(ra, rb, "block(0, 0)")
    assert ra[3] == 6 and ra[2].sum() > 0
    assert att.tolist() == [6 * nch] and acc.tolist() == [int(ra[2].sum())]
    if path == "multi_step":
        c = _sampler(p, nch, chain_offset=5)
        assert c.info()["multi_step"]
        c.block_enable(0, 0)
        assert not c.info()["multi_step"]
        c.run(3)
        c.block_disable()
        assert c.info()["multi_step"]
        c.run(3)
        _same(ra, done(c), "enable, 3, disable, 3")


# --- 2. the restated run ---
# seed and prior (vmin, vmax, vsmin, vsmax): chosen on the CPU (the restatement alone) so that every
# event asserted below happens within the 8 steps; the start models are clipped to the narrowed prior, so
# many cells sit on its lower bound and a downward block move next to them leaves it at a neighbour first.
# The other restated tests (default seed 7, full prior) assert their events the same way.
_PRIOR = (3600, 9000, 2100, 5500)
_CASES = {
    "P-per_step": dict(phases="P", path="per_step", nch=8, seed=7, prior=_PRIOR),
    "PS-per_step": dict(phases="PS", path="per_step", nch=8, seed=8, prior=_PRIOR),
    "P-two_pipes": dict(phases="P", path="two_pipes", nch=7, seed=7, prior=_PRIOR),      # pipes of 3 and 4 chains
    "PS-two_pipes": dict(phases="PS", path="two_pipes", nch=6, seed=8, prior=_PRIOR),
}


def _assert_events(r, phases):
    ev = r.events
    assert any(e.acc and e.R >= 1 for e in ev), "no accepted proposal with R >= 1"
    assert any(e.inp and not e.acc for e in ev), "no in-prior rejection"
    assert any(e.clipped for e in ev), "no clipped footprint"
    assert any(e.centre_in and not e.inp for e in ev), "no proposal whose centre stays inside while a neighbour leaves"
    if phases == "PS":
        assert any(e.ph == 1 and e.R >= 1 and e.z_face for e in ev), "no S proposal reaching a z face"
        assert any(e.ph == 0 for e in ev)


@pytest.mark.parametrize("case", list(_CASES))
def test_restated_run(case, monkeypatch):
    _dev()
    cfg = _CASES[case]
    p = _problem(cfg["phases"], n=_set_path(cfg["path"], monkeypatch), seed=cfg["seed"], prior=cfg["prior"])
    nch, off, nsteps = cfg["nch"], 5, 8
    g = _run_gpu(p, nch, off, nsteps, (0, 2), path=cfg["path"])
    r = _restate(p, g.v0, g.l0, off, nsteps, 0, 2)
    _assert_events(r, cfg["phases"])
    _compare(g, r, nsteps, case)
    assert r.attempts.sum() == nch * nsteps and (r.attempts > 0).all()


# --- 3. a footprint that covers the model ---
def test_covering_footprint(monkeypatch):
    _dev()
    p = _problem("PS", n=_set_path("per_step", monkeypatch))
    nch, off, nsteps = 6, 5, 2
    g = _run_gpu(p, nch, off, nsteps, (8, 8))
    r = _restate(p, g.v0, g.l0, off, nsteps, 8, 8)
    assert all(e.R == 8 and e.clipped for e in r.events) and any(e.ntouched == p.ncell for e in r.events)
    assert any(e.acc for e in r.events) and any(e.inp and not e.acc for e in r.events)
    _compare(g, r, nsteps, "R = 8")
    assert g.attempts.tolist() == [0] * 8 + [nch * nsteps]


# --- 4. precision 64 ---
def test_precision_64(monkeypatch):
    _dev()
    p = _problem("PS", n=_set_path("per_step", monkeypatch))
    nch, off, nsteps = 6, 5, 3
    g = _run_gpu(p, nch, off, nsteps, (0, 2), precision=64)
    r = _restate(p, g.v0, g.l0, off, nsteps, 0, 2, precision=64)
    assert any(e.acc and e.R >= 1 for e in r.events) and any(e.inp and not e.acc for e in r.events)
    _compare(g, r, nsteps, "fp64")


# --- 5. tempering with block proposals ---
# 9 chains, 3 rungs: G = 3, and two pipes split at chain 4, inside a replica group.  Either order of the two
# enables must leave every pipe's view with both the block arrays and beta.
_TEMPERED = {}          # path -> (v0, l0, restatement): the start state does not depend on the order


@pytest.mark.parametrize("order", ["block_first", "temper_first"])
@pytest.mark.parametrize("path", ["per_step", "two_pipes"])
def test_tempering_with_block_proposals(path, order, monkeypatch):
    _dev()
    p = _problem("P", n=_set_path(path, monkeypatch))
    nch, off, nsteps = 9, 5, 5
    g = _run_gpu(p, nch, off, nsteps, (0, 2), betas=LADDER3, swap_every=2, path=path, order=order)
    if path not in _TEMPERED:
        _TEMPERED[path] = (g.v0, g.l0, _restate(p, g.v0, g.l0, off, nsteps, 0, 2, betas=LADDER3, swap_every=2))
    v0, l0, r = _TEMPERED[path]
    _same((g.v0, g.l0), (v0, l0), "start state")
    # rounds at gs = 2 (parity 1) and 4 (parity 0): a swap after rejected and accepted block steps moves
    # slow_prop rows that must equal slow_cur, or the next forward solves a stale model
    assert r.swap_att.tolist() == [3, 3] and r.swap_acc.sum() > 0
    assert any(e.acc and e.R >= 1 for e in r.events) and any(e.inp and not e.acc and e.R >= 1 for e in r.events)
    _compare(g, r, nsteps, "tempered")
    _same((g.swap_att, g.swap_acc), (r.swap_att, r.swap_acc), "swap counters")


def test_tempering_and_blocks_switched_off_two_pipes_is_one_pipe(monkeypatch):
    """Block proposals and tempering on, 2 steps, tempering off, 2 steps, block proposals off, 2 steps: two pipes
    and one pipe give the same words (every pipe's view follows each switch)."""
    _dev()
    p = _problem("P", n=_set_path("two_pipes", monkeypatch))
    nch, off = 9, 5

    def run(npipe):
        monkeypatch.setenv("MCEIK_PIPES", str(npipe))
        s = _sampler(p, nch, block=(0, 2), chain_offset=off, max_samples=8)
        assert s.info()["npipe"] == npipe and not s.info()["multi_step"], s.info()
        s.temper_enable(betas=LADDER3, swap_every=2)
        s.run(2)
        s.temper_disable()
        s.run(2)
        s.block_disable()
        s.run(2)
        out = s.state() + s.samples()
        s.close()
        return out

    two, one = run(2), run(1)
    _same(two, one, "two pipes against one")
    v, logl, nacc, step, kv, kl = two
    assert step == 6 and nacc.sum() > 0 and len(kv) == 6
    _same((kv[-1], kl[-1]), (v, logl), "the last kept state is the state after step 5")


# --- 6. the streaming posterior sees block steps ---
def test_posterior_with_block_proposals(monkeypatch):
    _dev()
    p = _problem("PS", n=_set_path("two_pipes", monkeypatch), nburn=1, keepk=2)
    nch, nsteps = 7, 6
    s = _sampler(p, nch, block=(0, 2), max_samples=8)
    _check_path(s, "two_pipes", block=True)
    s.posterior_enable(per_chain=True, nbins=0)
    s.run(nsteps)
    raw = s.posterior_raw()
    kv, kl = s.samples()
    v, logl, nacc, _ = s.state()
    s.close()
    assert len(kv) == 3 and raw["n"] == 3 and nacc.sum() > 0          # kept steps 1, 3, 5
    k64 = kv.astype(np.int64)
    assert np.array_equal(raw["sum"], k64.sum(0)) and np.array_equal(raw["sumsq"], (k64 ** 2).sum(0))
    _same((kv[-1], kl[-1]), (v, logl), "the last kept state is the state after step 5")
    assert (kv[0] != kv[-1]).any()


# --- 7. sharding ---
def test_sharding(monkeypatch):
    _dev()
    p = _problem("PS", n=_set_path("per_step", monkeypatch))

    def run(nch, off):
        s = _sampler(p, nch, block=(0, 2), chain_offset=off)
        s.run(4)
        out = s.state()[:3] + (s.last()[2],) + s.block_stats()
        s.close()
        return out

    whole, a, b = run(12, 3), run(5, 3), run(7, 8)
    _same(whole[:4], tuple(np.concatenate([x, y]) for x, y in zip(a[:4], b[:4])), "5 + 7 chains")
    _same(whole[4:], (a[4] + b[4], a[5] + b[5]), "counters add up")
    assert whole[2].sum() > 0 and whole[4].sum() == 48


# --- 8. checkpoint ---
def test_checkpoint(monkeypatch):
    _dev()
    p = _problem("PS", n=_set_path("per_step", monkeypatch))
    nch = 6

    def done(s):
        out = s.state() + s.block_stats()
        s.close()
        return out

    a = _sampler(p, nch, block=(1, 3), chain_offset=5)
    a.run(6)
    ra = done(a)
    b = _sampler(p, nch, block=(1, 3), chain_offset=5)
    b.run(3)
    ck = b.checkpoint()
    b.close()
    assert ck["step"] == 3 and ck["block"]["rmin"] == 1 and ck["block"]["rmax"] == 3
    assert ck["block"]["attempts"].sum() == 3 * nch and ck["block"]["attempts"][0] == 0
    for other in ((0, 3), (1, 2), None):
        c = _sampler(p, nch, block=other, chain_offset=5)
        with pytest.raises(ValueError):
            c.restore(ck)
        c.close()
    d = _sampler(p, nch, block=(1, 3), chain_offset=5)
    d.restore(ck, recompute_logl=True)                 # the tables of the current models (two models)
    assert d.state()[1].tobytes() == ck["logl"].tobytes()
    _same(d.block_stats(), (ck["block"]["attempts"], ck["block"]["accepts"]), "counters carried over")
    d.run(3)
    _same(ra, done(d), "3 + checkpoint + 3")
    assert ra[4].sum() == 6 * nch and ra[5].sum() == ra[2].sum() > 0
    # a checkpoint without the entry restores anywhere
    plain = {k: val for k, val in ck.items() if k != "block"}
    e = _sampler(p, nch, block=(0, 1), chain_offset=5)
    e.restore(plain, recompute_logl=True)
    e.close()


# --- 9. arguments ---
def test_arguments(monkeypatch):
    import ctypes as C
    from mceik_amd import _lib
    _dev()
    _set_path("per_step", monkeypatch)
    p = _problem("P")
    s = _sampler(p, 6)
    L = _lib.lib()
    a, b = C.c_int(-1), C.c_int(-1)
    assert L.mceik_mcmc_block_stats(s._h, None, None, 0) == 1
    assert L.mceik_mcmc_block_get(s._h, C.byref(a), C.byref(b)) == 1
    with pytest.raises(RuntimeError):
        s.block_stats()
    assert L.mceik_mcmc_block_enable(s._h, None) == 1
    assert L.mceik_mcmc_block_enable(None, C.byref(_lib.BlockOpts(0, 2))) == 1
    for rmin, rmax in ((-1, 2), (3, 2), (0, 9), (9, 9)):
        assert L.mceik_mcmc_block_enable(s._h, C.byref(_lib.BlockOpts(rmin, rmax))) == 1
        with pytest.raises(ValueError):
            s.block_enable(rmin, rmax)
    assert L.mceik_mcmc_block_get(s._h, None, None) == 1          # still off
    assert L.mceik_mcmc_block_disable(s._h) == 0 and L.mceik_mcmc_block_disable(None) == 1
    s.block_enable(1, 8)
    assert L.mceik_mcmc_block_get(s._h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (1, 8)
    assert L.mceik_mcmc_block_get(s._h, None, None) == 0
    s.run(2)
    att, acc = s.block_stats()
    assert att.sum() == 12 and att[0] == 0 and len(att) == 9 and (acc <= att).all()
    s.block_enable(0, 2)                                          # enable resets the counters
    att, acc = s.block_stats()
    assert att.tolist() == [0, 0, 0] and acc.tolist() == [0, 0, 0]
    s.run(1)
    assert s.block_stats(reset=True)[0].sum() == 6
    assert s.block_stats()[0].sum() == 0
    s.block_disable()
    assert L.mceik_mcmc_block_stats(s._h, None, None, 0) == 1
    s.close()
