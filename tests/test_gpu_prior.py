"""The smoothness / reference-model prior on the GPU (csrc/prior.hip,
include/mceik.h mceik_mcmc_prior_*), the rule restated here in
Python and compared bit for bit.

A step of chain c (global id gid) draws Philox4x32-10 as tests/test_gpu_block.py
restates it (centre cell, mag, sign, radius, logu); with block proposals off the
radius is 0.  For a proposal inside the box that touches phase ph, dEs and dEd
are E(v') - E(v) by numpy int64 on the whole model (the footprint through
mcmc.block_footprint), and

    dlp = -(ws[ph] * float(dEs) + wd[ph] * float(dEd));  thr = logu - dlp
    accept iff thr < beta * (ln - logl)

in Python floats (IEEE double, nothing contracted).  A proposal outside the box
is rejected with dE = 0.  The forward is the oracle's CPU solver, the logL the
oracle's, the swap rule tests/test_gpu_temper.py's, unchanged.

The picks are analytic, so the whole restatement runs without a GPU: seeds,
sigmas and the narrowed box of _CASES were chosen that way, and every restated
test asserts the events it is there for.

Launch paths and grids as tests/test_gpu_block.py: per-step 24^3, two pipes
40^3, a multi-step-built sampler 32^3 (nref 4: 6^3, 10^3, 8^3 cells).
"""
import dataclasses
import types

import numpy as np
import pytest

import _oracle as O

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


def _check_path(smp, path, per_launch=False):
    info = smp.info()
    assert bool(info["multi_step"]) == (path == "multi_step" and not per_launch), info
    if path != "multi_step":
        assert info["npipe"] == (2 if path == "two_pipes" else 1), info


def _problem(phases="P", n=24, seed=7, box=None, nburn=0, keepk=1):
    """4 stations, 6 events, analytic picks; `box` = (vmin, vmax, vsmin, vsmax) narrows the uniform prior (the
    start models are clipped to it), `seed` is the sampler's and the start models'."""
    from mceik_amd import mcmc
    key = (phases, n)
    if key not in _PROBLEMS:
        p = mcmc.make_problem("C2", n=n, nstat=4, nev=6, seed=7, phases=phases, picks="analytic")
        p.dvmax = 300
        p.var[:] = 1e-5
        _PROBLEMS[key] = p
    p = dataclasses.replace(_PROBLEMS[key], seed=seed, nburn=nburn, keepk=keepk, _keep=[])
    if box is not None:
        p.vmin, p.vmax, p.vsmin, p.vsmax = box
    return p


def _vref(p):
    """The reference model: the model the picks were made in, clipped to the box (prior_enable refuses a
    reference model outside it)."""
    vp = np.clip(p.v_true, p.vmin, p.vmax).astype(np.int32)
    return vp if p.nphase == 1 else np.stack([vp, np.clip(p.vs_true, p.vsmin, p.vsmax)]).astype(np.int32)


def _same(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i)
        else:
            assert x == y, (what, i)


# --- the restatement ---
def _energy(p, v, vref=None):
    """(Es, Ed) of one phase model by numpy int64 on the whole model."""
    a = np.asarray(v, np.int64).reshape(p.ncz, p.ncy, p.ncx)
    es = sum(int((np.diff(a, axis=ax) ** 2).sum()) for ax in range(3))
    ed = 0 if vref is None else int(((a.ravel() - np.asarray(vref, np.int64).ravel()) ** 2).sum())
    return es, ed


def _energies(p, v, vref):
    """(Es, Ed) int64 [nchains, nphase] of chain models v."""
    nch = len(v)
    vv = v.reshape(nch, p.nphase, p.ncell)
    rr = None if vref is None else vref.reshape(p.nphase, p.ncell)
    es, ed = np.zeros((nch, p.nphase), np.int64), np.zeros((nch, p.nphase), np.int64)
    for c in range(nch):
        for ph in range(p.nphase):
            es[c, ph], ed[c, ph] = _energy(p, vv[c, ph], None if rr is None else rr[ph])
    return es, ed


def _draw(p, gid, step, block):
    r = [int(x) for x in O.philox([step & 0xFFFFFFFF, step >> 32, 0, 0], [gid, p.seed])]
    cell = (r[0] * p.nphase * p.ncell) >> 32
    mag = 1 + ((r[1] * p.dvmax) >> 32)
    R = 0 if block is None else block[0] + (((r[2] >> 1) * (block[1] - block[0] + 1)) >> 31)
    logu = O.lib().oracle_det_log((float(r[3]) + 0.5) * (1.0 / 4294967296.0))
    return cell, (-mag if r[2] & 1 else mag), R, logu


def _swap_logu(seed, gs, gid):
    out = O.philox([gs & 0xFFFFFFFF, gs >> 32, 1, 0], [gid, seed])
    return O.lib().oracle_det_log((float(out[0]) + 0.5) * (1.0 / 4294967296.0))


def _start(p, nch, off):
    """The chains' start state without a GPU (the sampler's own, tests/test_gpu_mcmc.py)."""
    from mceik_amd import mcmc
    P = O.make_problem(p)
    v0 = mcmc.initial_models(p, range(off, off + nch))
    l0 = np.array([O.loglik(P, O.forward_all_f32(P, v0[c].ravel())) for c in range(nch)])
    return v0, l0


def _restate(p, v0, logl0, off, nsteps, block, ws, wd, vref, betas=None, swap_every=0, step0=0):
    """Runs the chains on the CPU.  ws, wd: the weights per phase; vref [nphase * ncell] or None.  Returns a
    namespace: v, logl, naccept, accept [nsteps, nch], dE [nsteps, nch, 2], swap_att / swap_acc, and events: one
    record per proposal."""
    from mceik_amd import mcmc
    P = O.make_problem(p)
    nch, ncell = len(v0), p.ncell
    v = v0.reshape(nch, -1).copy()
    logl = logl0.copy()
    nacc = np.zeros(nch, np.int64)
    nt = len(betas) if betas is not None else 1
    G = nch // nt
    satt, sacc = np.zeros(max(nt - 1, 0), np.int64), np.zeros(max(nt - 1, 0), np.int64)
    flags = np.zeros((nsteps, nch), np.uint8)
    dE = np.zeros((nsteps, nch, 2), np.int64)
    rr = None if vref is None else np.asarray(vref).reshape(p.nphase, ncell)
    bounds = [(p.vmin, p.vmax), (p.vsmin, p.vsmax)]
    rmax = 0 if block is None else block[1]
    events = []
    for i, gs in enumerate(range(step0, step0 + nsteps)):
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
            cell, amp, R, logu = _draw(p, off + c, gs, block)
            ph, cc = divmod(cell, ncell)
            cells, dv = mcmc.block_footprint(p, cc, R, amp)
            idx = ph * ncell + cells.astype(np.int64)
            vp = v[c].copy()
            vp[idx] += dv
            lo, hi = bounds[ph]
            inp = bool(((vp[idx] >= lo) & (vp[idx] <= hi)).all())
            a, plain = False, False
            if inp:
                sl = slice(ph * ncell, (ph + 1) * ncell)
                e0 = _energy(p, v[c][sl], None if rr is None else rr[ph])
                e1 = _energy(p, vp[sl], None if rr is None else rr[ph])
                dEs, dEd = e1[0] - e0[0], e1[1] - e0[1]
                dlp = -(ws[ph] * float(dEs) + wd[ph] * float(dEd))
                thr = logu - dlp
                ln = O.loglik(P, O.forward_all_f32(P, vp))
                d = ln - logl[c]
                beta = betas[c // G] if nt > 1 else None
                a = bool(thr < beta * d) if nt > 1 else bool(thr < d)
                plain = bool(logu < beta * d) if nt > 1 else bool(logu < d)
                dE[i, c] = dEs, dEd
                if a:
                    v[c], logl[c], nacc[c] = vp, ln, nacc[c] + 1
            flags[i, c] = a
            events.append(types.SimpleNamespace(step=i, chain=c, R=R, ph=ph, inp=inp, acc=a, flipped=a != plain,
                                                rmax=R == rmax, clipped=len(cells) < (2 * R + 1) ** 3))
    return types.SimpleNamespace(v=v.reshape(v0.shape), logl=logl, naccept=nacc, accept=flags, dE=dE,
                                 swap_att=satt, swap_acc=sacc, events=events)


def _sampler(p, nchains, block=None, prior=None, **kw):
    """prior: None or dict(sigma_smooth, sigma_damp, vref) for Sampler.prior_enable."""
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=nchains, **kw)
    if block is not None:
        smp.block_enable(*block)
    if prior is not None:
        smp.prior_enable(**prior)
    return smp


def _weights(prior):
    from mceik_amd import mcmc
    return mcmc.prior_weight(prior.get("sigma_smooth")), mcmc.prior_weight(prior.get("sigma_damp"))


# --- 1. the energy kernel ---
@pytest.mark.parametrize("with_vref", [False, True])
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_energy_kernel(phases, with_vref, monkeypatch):
    _dev()
    from mceik_amd import mcmc
    # 40^3: 1000 cells, one tile with a partial last wave; 5 chains: not a multiple of the 4 chains per block
    p = _problem(phases, n=_set_path("two_pipes", monkeypatch))
    vref = _vref(p) if with_vref else None
    smp = _sampler(p, 5, prior=dict(sigma_smooth=200.0, sigma_damp=300.0 if with_vref else None, vref=vref),
                   chain_offset=3)
    v = smp.state()[0]
    es, ed = smp.prior_energy()
    smp.close()
    wes, wed = _energies(p, v, vref)
    assert es.dtype == np.int64 and es.shape == (5, p.nphase)
    _same((es, ed), (wes, wed), "energies")
    assert (es > 0).all() and (ed > 0).all() == with_vref and (with_vref or not ed.any())
    # the host entry point agrees (one arithmetic)
    vv = v.reshape(5, p.nphase, p.ncell)
    assert mcmc.prior_energy(p, vv[4, p.nphase - 1])[0] == es[4, p.nphase - 1]


def test_energy_kernel_many_tiles(monkeypatch):
    """A model of more cells than one block covers in one pass (tiles > 1, the grid-stride loop): 16^3 cells."""
    _dev()
    from mceik_amd import mcmc
    _set_path("per_step", monkeypatch)
    p = mcmc.make_problem("C2", n=32, nstat=2, nev=2, seed=7, phases="PS", picks="analytic", nref=(2, 2, 2))
    assert p.ncell == 4096
    vref = _vref(p)
    smp = _sampler(p, 3, prior=dict(sigma_smooth=200.0, sigma_damp=300.0, vref=vref))
    v = smp.state()[0]
    es, ed = smp.prior_energy()
    smp.close()
    _same((es, ed), _energies(p, v, vref), "energies")


# --- 2. zero weights are the plain sampler ---
@pytest.mark.parametrize("block", [None, (0, 2)], ids=["single", "block02"])
@pytest.mark.parametrize("path", ["per_step", "two_pipes", "multi_step"])
def test_zero_weights_are_the_plain_sampler(path, block, monkeypatch):
    _dev()
    p = _problem("PS", n=_set_path(path, monkeypatch))
    nch, nsteps = 6, 8

    def done(s):
        out = s.state() + (s.last()[2],) + s.samples()
        s.close()
        return out

    a = _sampler(p, nch, block=block, chain_offset=5, max_samples=8)
    _check_path(a, path, per_launch=block is not None)
    a.run(nsteps)
    ra = done(a)
    # a reference model with weight 0: both terms are evaluated and multiplied by zero
    b = _sampler(p, nch, block=block, prior=dict(vref=_vref(p)), chain_offset=5, max_samples=8)
    _check_path(b, path, per_launch=True)
    assert not b.info()["multi_step"]
    b.run(nsteps)
    de = b.prior_last()
    rb = done(b)
    _same(ra, rb, "zero weights")
    assert ra[3] == nsteps and ra[2].sum() > 0 and len(ra[5]) == nsteps
    assert de.any()                                      # the fold ran: the energies did change
    # enable, 4 steps, disable, 4 steps: multi_step comes back, the chains are still the plain ones
    c = _sampler(p, nch, block=block, chain_offset=5, max_samples=8)
    before = c.info()["multi_step"]
    c.prior_enable()
    assert not c.info()["multi_step"]
    c.run(4)
    c.prior_disable()
    assert c.info()["multi_step"] == before == (path == "multi_step" and block is None)
    with pytest.raises(RuntimeError):
        c.prior_last()
    c.run(4)
    _same(ra, done(c), "enable, 4, disable, 4")


# --- 3. the restated run ---
# seed, box (vmin, vmax, vsmin, vsmax) and sigmas: chosen on the CPU (the restatement alone) so that every event
# asserted below happens within the 8 steps.  The start models are clipped to the narrowed box, so many cells
# sit on its lower bound and downward moves leave it.
_BOX = (3600, 9000, 2100, 5500)
_PRIOR = dict(sigma_smooth=(60.0, 40.0), sigma_damp=(90.0, 60.0))
_CASES = {
    "P-per_step": dict(phases="P", path="per_step", block=None, seed=7),
    "PS-per_step": dict(phases="PS", path="per_step", block=None, seed=8),
    "P-two_pipes": dict(phases="P", path="two_pipes", block=None, seed=7),
    "PS-two_pipes": dict(phases="PS", path="two_pipes", block=None, seed=8),
    "P-multi_step": dict(phases="P", path="multi_step", block=None, seed=7),
    "PS-multi_step": dict(phases="PS", path="multi_step", block=None, seed=8),
    "P-block08": dict(phases="P", path="per_step", block=(0, 8), seed=7),
    "PS-block08": dict(phases="PS", path="per_step", block=(0, 8), seed=8),
}


def _assert_events(r, phases, block):
    ev = r.events
    assert any(e.acc for e in ev), "no accept"
    assert any(e.inp and not e.acc for e in ev), "no rejection inside the box"
    assert any(e.flipped for e in ev), "no decision differs from the run without the prior"
    out = [e for e in ev if not e.inp]
    assert out and all(not r.dE[e.step, e.chain].any() and not e.acc for e in out), "no proposal outside the box"
    assert any(r.dE[e.step, e.chain, 0] != 0 and r.dE[e.step, e.chain, 1] != 0 for e in ev if e.inp)
    if block is not None:
        assert any(e.R == 0 for e in ev) and any(e.rmax for e in ev), "R = 0 and R = rmax"
        assert all(e.clipped for e in ev if e.rmax)       # 6^3 cells: radius 8 is clipped at every face
    if phases == "PS":
        assert any(e.ph == 0 and e.inp for e in ev) and any(e.ph == 1 and e.inp for e in ev), "both phases"


@pytest.mark.parametrize("case", list(_CASES))
def test_restated_run(case, monkeypatch):
    _dev()
    cfg = _CASES[case]
    p = _problem(cfg["phases"], n=_set_path(cfg["path"], monkeypatch), seed=cfg["seed"], box=_BOX)
    nch, off, nsteps = 6, 5, 8
    vref = _vref(p)
    prior = dict(_PRIOR, vref=vref)
    ws, wd = _weights(prior)
    smp = _sampler(p, nch, block=cfg["block"], prior=prior, chain_offset=off)
    _check_path(smp, cfg["path"], per_launch=True)
    v0, l0, _, _ = smp.state()
    r = _restate(p, v0, l0, off, nsteps, cfg["block"], ws, wd, vref)
    _assert_events(r, cfg["phases"], cfg["block"])
    # stop once after a step with a proposal outside the box: its dE is there to be read
    k = next(e.step for e in r.events if not e.inp)
    smp.run(k + 1)
    _same((smp.prior_last(), smp.last()[2]), (r.dE[k], r.accept[k]), case + f": step {k}")
    smp.run(nsteps - k - 1)
    v, logl, nacc, step = smp.state()
    acc, de = smp.last()[2], smp.prior_last()
    smp.close()
    assert step == nsteps
    _same((v, logl, nacc, acc, de), (r.v, r.logl, r.naccept, r.accept[-1], r.dE[-1]), case)


# --- 4. the fold against the energy kernel ---
@pytest.mark.parametrize("block", [None, (0, 8)], ids=["single", "block08"])
def test_fold_against_energy(block, monkeypatch):
    _dev()
    p = _problem("PS", n=_set_path("per_step", monkeypatch), seed=8)
    nch = 6
    smp = _sampler(p, nch, block=block, prior=dict(_PRIOR, vref=_vref(p)), chain_offset=5)
    seen = np.zeros(2, np.int64)
    for _ in range(5):
        es0, ed0 = smp.prior_energy()
        smp.run(1)
        es1, ed1 = smp.prior_energy()
        de, acc, ph = smp.prior_last(), smp.last()[2], smp.last_phase()
        want_s, want_d = np.zeros_like(es0), np.zeros_like(ed0)
        for c in range(nch):
            if acc[c]:
                want_s[c, ph[c]], want_d[c, ph[c]] = de[c]
        _same((es1 - es0, ed1 - ed0), (want_s, want_d), "energy after - before")
        seen += np.bincount(acc, minlength=2)
    smp.close()
    assert seen[0] > 0 and seen[1] > 0, seen


# --- 5. with tempering ---
@pytest.mark.parametrize("path", ["per_step", "two_pipes"])
def test_with_tempering(path, monkeypatch):
    _dev()
    p = _problem("P", n=_set_path(path, monkeypatch))
    nch, off, nsteps = 9, 5, 5                          # G = 3; two pipes split at chain 4, inside a replica group
    vref = _vref(p)
    prior = dict(_PRIOR, vref=vref)
    ws, wd = _weights(prior)
    smp = _sampler(p, nch, prior=prior, chain_offset=off)
    smp.temper_enable(betas=LADDER3, swap_every=2)
    _check_path(smp, path, per_launch=True)
    v0, l0, _, _ = smp.state()
    smp.run(nsteps)
    v, logl, nacc, step = smp.state()
    acc, de = smp.last()[2], smp.prior_last()
    satt, sacc = smp.temper_stats()
    smp.close()
    r = _restate(p, v0, l0, off, nsteps, None, ws, wd, vref, betas=LADDER3, swap_every=2)
    assert r.swap_att.tolist() == [3, 3] and r.swap_acc.sum() > 0          # rounds at gs = 2 and 4
    assert any(e.acc for e in r.events) and any(e.inp and not e.acc for e in r.events)
    assert any(e.flipped for e in r.events)
    _same((v, logl, nacc, acc, de), (r.v, r.logl, r.naccept, r.accept[-1], r.dE[-1]), "tempered")
    _same((satt, sacc), (r.swap_att, r.swap_acc), "swap counters")


# --- 6. checkpoint ---
def test_checkpoint(monkeypatch):
    _dev()
    p = _problem("PS", n=_set_path("per_step", monkeypatch), seed=8)
    nch = 6
    vref = _vref(p)
    prior = dict(_PRIOR, vref=vref)

    def done(s):
        out = s.state() + (s.prior_last(),)
        s.close()
        return out

    a = _sampler(p, nch, block=(0, 2), prior=prior, chain_offset=5)
    a.run(6)
    ra = done(a)
    b = _sampler(p, nch, block=(0, 2), prior=prior, chain_offset=5)
    b.run(3)
    ck = b.checkpoint()
    b.close()
    ws, wd = _weights(prior)
    assert ck["step"] == 3 and ck["prior"]["w_smooth"] == ws and ck["prior"]["w_damp"] == wd
    assert len(ck["prior"]["vref_sha256"]) == 64
    other = vref.copy()
    other[0, 0] += 1
    for bad in (dict(prior, sigma_smooth=(60.0, 41.0)), dict(prior, sigma_damp=None), dict(prior, vref=other),
                dict(sigma_smooth=_PRIOR["sigma_smooth"]), None):
        c = _sampler(p, nch, block=(0, 2), prior=bad, chain_offset=5)
        with pytest.raises(ValueError):
            c.restore(ck)
        c.close()
    d = _sampler(p, nch, block=(0, 2), prior=prior, chain_offset=5)
    d.restore(ck, recompute_logl=True)                  # the tables of the current models (two models)
    assert d.state()[1].tobytes() == ck["logl"].tobytes()
    d.run(3)
    _same(ra, done(d), "3 + checkpoint + 3")
    assert ra[2].sum() > 0
    # a checkpoint without the entry restores anywhere
    plain = {k: val for k, val in ck.items() if k != "prior"}
    e = _sampler(p, nch, block=(0, 2), prior=dict(sigma_smooth=10.0), chain_offset=5)
    e.restore(plain, recompute_logl=True)
    e.close()


# --- 7. arguments ---
def test_arguments(monkeypatch):
    import ctypes as C
    from mceik_amd import _lib
    _dev()
    _set_path("per_step", monkeypatch)
    p = _problem("P", nburn=0)
    s = _sampler(p, 6, max_samples=0)
    L = _lib.lib()
    de = np.zeros((6, 2), np.int64)
    o = _lib.PriorOpts()
    assert L.mceik_mcmc_prior_last(s._h, de.ctypes.data_as(C.c_void_p)) == 1           # not enabled
    assert L.mceik_mcmc_prior_energy(s._h, None, None) == 1
    assert L.mceik_mcmc_prior_get(s._h, C.byref(o), None) == 1
    assert L.mceik_mcmc_prior_disable(s._h) == 0 and L.mceik_mcmc_prior_disable(None) == 1
    assert L.mceik_mcmc_prior_enable(s._h, None) == 1 and L.mceik_mcmc_prior_enable(None, C.byref(o)) == 1
    for bad in (-1.0, float("inf"), float("nan")):
        for field, ph in (("w_smooth", 0), ("w_smooth", 1), ("w_damp", 0), ("w_damp", 1)):
            o = _lib.PriorOpts()
            getattr(o, field)[ph] = bad
            assert L.mceik_mcmc_prior_enable(s._h, C.byref(o)) == 1, (bad, field, ph)
    with pytest.raises(RuntimeError):
        s.prior_energy()
    with pytest.raises(ValueError):
        s.prior_enable(sigma_damp=100.0)                 # damping without a reference model
    with pytest.raises(ValueError):
        s.prior_enable(sigma_smooth=-5.0)
    with pytest.raises(ValueError):
        s.prior_enable(vref=_vref(p)[:-1])
    outside = _vref(p)
    outside[3] = p.vmax + 1
    with pytest.raises(ValueError):
        s.prior_enable(sigma_damp=100.0, vref=outside)
    assert L.mceik_mcmc_prior_get(s._h, None, None) == 1                               # still off
    vref = _vref(p)
    s.prior_enable(sigma_smooth=(100.0, None), sigma_damp=50.0, vref=vref)
    back = np.zeros_like(vref)
    assert L.mceik_mcmc_prior_get(s._h, C.byref(o), back.ctypes.data_as(C.c_void_p)) == 0
    assert (o.w_smooth[0], o.w_smooth[1]) == (1.0 / (2.0 * 100.0 * 100.0), 0.0)
    assert (o.w_damp[0], o.w_damp[1]) == (1.0 / (2.0 * 50.0 * 50.0),) * 2
    assert back.tobytes() == vref.tobytes() and o.vref == back.ctypes.data
    s.prior_enable(sigma_smooth=100.0)                   # replaces: no reference model any more
    assert L.mceik_mcmc_prior_get(s._h, C.byref(o), back.ctypes.data_as(C.c_void_p)) == 0 and not o.vref
    assert not s.prior_energy()[1].any()
    # an enabled posterior that holds states refuses both switches, as tempering's
    s.posterior_enable(per_chain=True, nbins=0)
    s.run(1)
    with pytest.raises(ValueError):
        s.prior_disable()
    with pytest.raises(ValueError):
        s.prior_enable(sigma_smooth=50.0)
    s.posterior_disable()
    s.prior_disable()
    s.close()
    # 3 ncell (hi - lo + 2 dvmax)^2 >= 2^53: 216 cells and a box of 4 000 000 m/s
    wide = _problem("P", box=(1500, 4_001_500, 800, 5500))
    assert 3 * wide.ncell * (4_000_000 + 600) ** 2 >= 2 ** 53
    w = _sampler(wide, 2)
    with pytest.raises(ValueError):
        w.prior_enable(sigma_smooth=100.0)
    w.close()
    fits = _problem("P", box=(1500, 3_001_500, 800, 5500))
    assert 3 * fits.ncell * (3_000_000 + 600) ** 2 < 2 ** 53
    f = _sampler(fits, 2)
    f.prior_enable(sigma_smooth=100.0)
    f.close()
