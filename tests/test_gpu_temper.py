"""Parallel tempering on the GPU (csrc/temper.hip, include/mceik.h
mceik_mcmc_temper_*), every rule restated here in Python and compared bit for
bit.

Layout: nchains chains, ntemps rungs, G = nchains // ntemps groups; rung r of
group g is local chain r * G + g, the cold chains are [0, G).  Accept:
inprior && logu < beta_c * (ln - logl_c).  Swap round of step gs: pairs a = r *
G + g, b = a + G for r % 2 == parity; Philox4x32-10 counter {gs lo, gs hi, 1,
0}, key {chain_offset + a, seed}; logu = det_log((out[0] + 0.5) / 2^32); swap
iff logu < (beta[r] - beta[r+1]) * (logl[b] - logl[a]).

The multi-step launch path needs the 16-z FSM kernel, which a 24^3 grid does
not get (fewer than four z-blocks): those cases run on a 32^3 grid and assert
info()["multi_step"].  Two pipes need the 40^3 grid of test_gpu_posterior.py.
"""
import numpy as np
import pytest

import _oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_PROBLEMS = {}
LADDER4 = np.array([1.0, 0.1, 1e-3, 1e-6])
LADDER3 = np.array([1.0, 0.1, 1e-3])


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _problem(phases="P", n=24, nstat=4, nev=6, nburn=0, keepk=1):
    """test_gpu_posterior.py's _problem; the picks (one GPU forward) are made once per shape."""
    from mceik_amd import mcmc
    key = (phases, n, nstat, nev)
    if key not in _PROBLEMS:
        p = mcmc.make_problem("C2", n=n, nstat=nstat, nev=nev, seed=7, phases=phases, picks=mcmc.picks_from_forward(0))
        p.dvmax = 300
        p.var[:] = 1e-5
        _PROBLEMS[key] = p
    p = _PROBLEMS[key]
    p.nburn, p.keepk = nburn, keepk
    return p


# launch paths: environment (read when the sampler is built) and the grid that gets the path
_PATHS = {
    "per_step": dict(env={"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, n=24),
    "two_pipes": dict(env={"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}, n=40),
    "multi_step": dict(env={"MCEIK_PERSIST": "1"}, n=32),
}


def _set_path(path, monkeypatch):
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in _PATHS[path]["env"].items():
        monkeypatch.setenv(k, val)
    return _PATHS[path]["n"]


def _check_path(smp, path):
    info = smp.info()
    assert bool(info["multi_step"]) == (path == "multi_step"), info
    if path != "multi_step":
        assert info["npipe"] == (2 if path == "two_pipes" else 1), info


def _sampler(p, nchains, betas=None, swap_every=0, **kw):
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=nchains, **kw)
    if betas is not None:
        smp.temper_enable(betas=betas, swap_every=swap_every)
    return smp


def _same(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i)
        else:
            assert x == y, (what, i)


def _swap_logu(seed, gs, gid):
    out = O.philox([gs & 0xFFFFFFFF, gs >> 32, 1, 0], [gid, seed])
    return O.lib().oracle_det_log((float(out[0]) + 0.5) * (1.0 / 4294967296.0))


def _swap_round(betas, nch, logl, parity, gs, seed, off=0):
    """The round restated: (perm, logl after, attempts, accepts); chain i holds
    afterwards the state chain perm[i] held before."""
    nt = len(betas)
    G = nch // nt
    perm = np.arange(nch)
    logl = logl.copy()
    att, acc = np.zeros(nt - 1, np.int64), np.zeros(nt - 1, np.int64)
    for r in range(parity, nt - 1, 2):
        for g in range(G):
            a, b = r * G + g, (r + 1) * G + g
            att[r] += 1
            if _swap_logu(seed, gs, off + a) < (betas[r] - betas[r + 1]) * (logl[b] - logl[a]):
                perm[a], perm[b] = perm[b], perm[a]
                logl[a], logl[b] = logl[b], logl[a]
                acc[r] += 1
    return perm, logl, att, acc


# --- 1. off is off ---
@pytest.mark.parametrize("path", ["per_step", "multi_step"])
def test_one_rung_is_the_plain_sampler(path, monkeypatch):
    _dev()
    p = _problem("P", n=_set_path(path, monkeypatch))
    a = _sampler(p, 6, chain_offset=5)
    b = _sampler(p, 6, betas=[1.0], swap_every=1, chain_offset=5)
    _check_path(a, path)
    _check_path(b, path)
    assert list(b.cold_chains) == list(range(6)) and list(a.cold_chains) == list(range(6))
    a.run(6)
    b.run(6)
    sa, sb = a.state(), b.state()
    att, acc = b.temper_stats()
    a.close()
    b.close()
    _same(sa, sb)
    assert sa[2].sum() > 0 and sa[3] == 6 and len(att) == 0 and len(acc) == 0


@pytest.mark.parametrize("path", ["per_step", "multi_step"])
def test_cold_chains_without_swaps_are_plain_chains(path, monkeypatch):
    _dev()
    p = _problem("P", n=_set_path(path, monkeypatch))
    a = _sampler(p, 3, chain_offset=5)
    b = _sampler(p, 12, betas=LADDER4, swap_every=0, chain_offset=5)
    _check_path(b, path)
    assert list(b.cold_chains) == [0, 1, 2]
    a.run(6)
    b.run(6)
    (va, la, na, _), (vb, lb, nb, _) = a.state(), b.state()
    att, acc = b.temper_stats()
    a.close()
    b.close()
    _same((va, la, na), (vb[:3], lb[:3], nb[:3]))
    assert na.sum() > 0 and not att.any() and not acc.any()


# --- 2. the tempered accept rule ---
@pytest.mark.parametrize("phases", ["P", "PS"])
@pytest.mark.parametrize("path", ["per_step", "multi_step"])
def test_tempered_accept_exact(path, phases, monkeypatch):
    _dev()
    p = _problem(phases, n=_set_path(path, monkeypatch))
    nch, off, betas = 12, 5, LADDER4
    G = nch // len(betas)
    t = _sampler(p, nch, betas=betas, swap_every=0, chain_offset=off)
    _check_path(t, path)
    t.run(3)
    v0, l0, n0, step = t.state()
    assert step == 3
    # the proposals' logL from a twin that accepts every in-prior proposal
    twin = _sampler(p, nch, chain_offset=off)
    ck = {"v": v0, "logl": l0, "naccept": n0, "step": step, "nkept": 0}
    if phases == "PS":
        twin.restore(ck, recompute_logl=True)        # the tables of the current models
    twin.restore({**ck, "logl": np.full(nch, -1e300)})
    twin.run(1)
    _, ln, _, _ = twin.state()
    acc_twin = twin.last()[2]
    twin.close()
    t.run(1)
    v1, l1, n1, _ = t.state()
    acc = t.last()[2]
    t.close()
    P = O.make_problem(p)
    ev, el, en = v0.copy(), l0.copy(), n0.copy()
    flat = ev.reshape(nch, -1)
    want = np.zeros(nch, np.uint8)
    cold_rejects = np.zeros(nch, bool)
    for c in range(nch):
        cell, vn, inp, logu = O.propose(P, off + c, step, v0[c])
        assert bool(acc_twin[c]) == inp
        if not inp:
            continue
        d = ln[c] - l0[c]
        want[c] = logu < betas[c // G] * d
        cold_rejects[c] = not (logu < d)
        if want[c]:
            flat[c, cell], el[c], en[c] = vn, ln[c], en[c] + 1
    _same((acc, v1, l1, n1), (want, ev, el, en))
    hot = np.arange(nch) >= G
    assert (hot & (want == 1) & cold_rejects).any(), "no hot chain accepted what beta = 1 rejects"
    assert (hot & (want == 0)).any(), "no hot chain rejected"


# --- 3. the swap kernels ---
_SWAP_CASES = {
    "P-4": dict(phases="P", betas=LADDER4, nch=12, n=24, nstat=4, nev=6),
    "PS-4": dict(phases="PS", betas=LADDER4, nch=12, n=24, nstat=4, nev=6),
    "P-3": dict(phases="P", betas=LADDER3, nch=9, n=24, nstat=4, nev=6),
    "PS-3": dict(phases="PS", betas=LADDER3, nch=9, n=24, nstat=4, nev=6),
    # 125 cells: every row but each fourth starts off a 16-byte boundary
    "P-4-odd": dict(phases="P", betas=LADDER4, nch=12, n=20, nstat=3, nev=5),
    # 17^3 = 4913 cells, 9826 entries per chain: three row tiles, rows of even chains aligned with a
    # two-dword tail, rows of odd chains not aligned; table rows of 30 floats
    "PS-3-odd-tiles": dict(phases="PS", betas=LADDER3, nch=12, n=68, nstat=3, nev=5),
    # every attempted pair must swap
    "P-4-ones": dict(phases="P", betas=np.ones(4), nch=12, n=24, nstat=4, nev=6),
    "PS-3-ones": dict(phases="PS", betas=np.ones(3), nch=9, n=20, nstat=3, nev=5),
}


@pytest.mark.parametrize("case", list(_SWAP_CASES))
def test_swap_round_exact(case, monkeypatch):
    _dev()
    cfg = _SWAP_CASES[case]
    _set_path("per_step", monkeypatch)
    p = _problem(cfg["phases"], n=cfg["n"], nstat=cfg["nstat"], nev=cfg["nev"])
    nch, betas, off = cfg["nch"], cfg["betas"], 5
    t = _sampler(p, nch, betas=betas, swap_every=0, chain_offset=off)
    t.run(3)
    v0, l0, n0, step = t.state()
    t.temper_swap(0)
    t.temper_swap(1)
    v1, l1, n1, step1 = t.state()
    att, acc = t.temper_stats()
    pa, la, att_a, acc_a = _swap_round(betas, nch, l0, 0, step, p.seed, off)
    pb, lb, att_b, acc_b = _swap_round(betas, nch, la, 1, step, p.seed, off)
    perm = pa[pb]
    _same((v1, l1, n1, step1), (v0[perm], lb, n0, step), "state after the rounds")
    assert lb.tobytes() == l0[perm].tobytes()
    _same((att, acc), (att_a + att_b, acc_a + acc_b), "counters")
    G = nch // len(betas)
    assert att.tolist() == [G] * (len(betas) - 1)
    if case.endswith("ones"):
        assert acc.tolist() == att.tolist()
    else:
        assert 0 < acc.sum() < att.sum(), (att, acc)
    # the hidden state moved with the models: a fresh sampler restored from the expected state runs on alike
    f = _sampler(p, nch, betas=betas, swap_every=0, chain_offset=off)
    ck = {"v": v0[perm], "logl": lb, "naccept": n0, "step": step, "nkept": 0}
    if cfg["phases"] == "PS":
        f.restore(ck, recompute_logl=True)
        assert f.state()[1].tobytes() == lb.tobytes()
    else:
        f.restore(ck)
    t.run(3)
    f.run(3)
    st, sf = t.state(), f.state()
    t.close()
    f.close()
    _same(st, sf, "three steps after the rounds")
    assert st[3] == step + 3 and (st[2] - n0).sum() > 0


# --- 4. the schedule ---
_SCHEDULE = {
    "multi_step": dict(path="multi_step", nch=12, betas=LADDER4, precision=32),
    "per_step": dict(path="per_step", nch=12, betas=LADDER4, precision=32),
    # pipes of 4 and 5 chains: the split falls inside rung 1 (chains 3..5)
    "two_pipes": dict(path="two_pipes", nch=9, betas=LADDER3, precision=32),
    "fp64": dict(path="per_step", nch=12, betas=LADDER4, precision=64),
}


@pytest.mark.parametrize("case", list(_SCHEDULE))
def test_schedule(case, monkeypatch):
    _dev()
    cfg = _SCHEDULE[case]
    p = _problem("P", n=_set_path(cfg["path"], monkeypatch))
    nch, betas, off = cfg["nch"], cfg["betas"], 5
    kw = dict(chain_offset=off, precision=cfg["precision"])

    def done(s):
        out = s.state() + s.temper_stats()
        s.close()
        return out

    a = _sampler(p, nch, betas=betas, swap_every=2, **kw)
    _check_path(a, cfg["path"])
    a.run(7)
    ra = done(a)
    b = _sampler(p, nch, betas=betas, swap_every=0, **kw)
    for gs in range(7):
        if gs > 0 and gs % 2 == 0:
            b.temper_swap((gs // 2) & 1)
        b.run(1)
    _same(ra, done(b), "by hand")
    c = _sampler(p, nch, betas=betas, swap_every=2, **kw)
    c.run(3)
    c.run(4)
    _same(ra, done(c), "run(3); run(4)")
    d = _sampler(p, nch, betas=betas, swap_every=2, **kw)
    d.run(4)
    ck = d.checkpoint()
    d.close()
    assert ck["step"] == 4 and ck["temper"]["swap_every"] == 2 and ck["temper"]["betas"].tolist() == list(betas)
    e = _sampler(p, nch, betas=betas, swap_every=2, **kw)
    e.restore(ck)
    e.run(3)
    _same(ra, done(e), "checkpoint at step 4")
    # rounds at gs = 2, 4, 6: parities 1, 0, 1
    G, nt = nch // len(betas), len(betas)
    want = [G * sum(1 for par in (1, 0, 1) if r % 2 == par) for r in range(nt - 1)]
    att, acc = ra[4], ra[5]
    assert ra[3] == 7 and att.tolist() == want and acc.sum() > 0 and ra[2].sum() > 0


# --- 5. the posterior sees the cold chains ---
def _hist(p, states, nbins):
    ncm = p.nphase * p.ncell
    v = states.reshape(-1, p.nphase, p.ncell).astype(np.int64)
    lo = np.array([p.vmin, p.vsmin][:p.nphase], np.int64)[:, None]
    hi = np.array([p.vmax, p.vsmax][:p.nphase], np.int64)[:, None]
    b = np.clip((v - lo) * nbins // (hi - lo + 1), 0, nbins - 1).reshape(-1, ncm)
    flat = (np.arange(ncm)[None, :] * nbins + b).ravel()
    return np.bincount(flat, minlength=ncm * nbins).reshape(ncm, nbins)


@pytest.mark.parametrize("per_chain", [True, False])
@pytest.mark.parametrize("path", ["per_step", "multi_step"])
def test_posterior_sees_the_cold_chains(path, per_chain, monkeypatch):
    _dev()
    p = _problem("P", n=_set_path(path, monkeypatch), nburn=0, keepk=1)
    nch, G, nsteps = 12, 4, 6
    s = _sampler(p, nch, betas=LADDER3, swap_every=2, max_samples=8)
    _check_path(s, path)
    s.posterior_enable(per_chain=per_chain, nbins=7)
    s.run(nsteps)
    raw, parts = s.posterior_raw(), s.posterior_partials()
    kv, _ = s.samples()
    with pytest.raises(ValueError):                  # states are held: the ladder stays
        s.temper_enable(betas=LADDER3, swap_every=2)
    with pytest.raises(ValueError):
        s.temper_disable()
    s.posterior_enable(per_chain=per_chain, nbins=7)   # reset: n = 0
    s.temper_disable()
    s.close()
    assert len(kv) == nsteps and raw["n"] == nsteps
    cold = kv[:, :G].astype(np.int64)
    if per_chain:
        assert np.array_equal(raw["sum"][:G], cold.sum(0)) and np.array_equal(raw["sumsq"][:G], (cold ** 2).sum(0))
        assert not raw["sum"][G:].any() and not raw["sumsq"][G:].any()
    else:
        assert np.array_equal(raw["sum"], cold.sum((0, 1))) and np.array_equal(raw["sumsq"], (cold ** 2).sum((0, 1)))
    hist = raw["hist"].reshape(p.ncell, 7).astype(np.int64)
    assert (hist.sum(1) == G * nsteps).all()
    assert np.array_equal(hist, _hist(p, kv[:, :G], 7))
    assert parts.nchains == G and parts.nkept == nsteps
    assert np.array_equal(parts.S, cold.sum((0, 1)).ravel())
    assert np.array_equal(parts.hist.astype(np.int64), hist)


# --- 6. errors ---
def test_errors(monkeypatch):
    import ctypes as C
    from mceik_amd import _lib
    _dev()
    _set_path("per_step", monkeypatch)
    p = _problem("P")
    s = _sampler(p, 12)
    with pytest.raises(RuntimeError):
        s.temper_swap(0)
    with pytest.raises(RuntimeError):
        s.temper_stats()
    L = _lib.lib()
    assert L.mceik_mcmc_temper_swap(s._h, 0) == 1
    assert L.mceik_mcmc_temper_stats(s._h, None, None, 0) == 1
    assert L.mceik_mcmc_temper_get(s._h, None, None, None) == 1
    assert L.mceik_mcmc_temper_enable(s._h, None) == 1
    assert L.mceik_mcmc_temper_enable(s._h, C.byref(_lib.TemperOpts(4, 1, None))) == 1
    assert L.mceik_mcmc_temper_disable(s._h) == 0
    for bad in ([1.0, 0.5, 0.25, 0.1, 0.01],         # 12 % 5 != 0
                [0.9, 0.5, 0.1],                     # beta[0] != 1
                [1.0, 0.5, 0.7],                     # increasing
                [1.0, 0.5, 0.0],                     # beta <= 0
                [1.0, 0.5, -0.1],
                [1.0, float("nan"), 0.1]):
        with pytest.raises(ValueError):
            s.temper_enable(betas=bad)
    with pytest.raises(ValueError):
        s.temper_enable()
    with pytest.raises(ValueError):
        s.temper_enable(betas=[1.0, 0.5], ntemps=2, tmax=2.0)
    with pytest.raises(ValueError):
        s.temper_enable(betas=[1.0, 0.5], swap_every=-1)
    with pytest.raises(RuntimeError):
        s.temper_stats()                             # still off
    s.temper_enable(ntemps=4, tmax=50.0, swap_every=3)
    from mceik_amd import mcmc
    nt, k, beta = C.c_int(0), C.c_int(0), np.zeros(4)
    assert L.mceik_mcmc_temper_get(s._h, C.byref(nt), C.byref(k), beta.ctypes.data_as(C.c_void_p)) == 0
    assert (nt.value, k.value) == (4, 3) and beta.tobytes() == mcmc.temper_ladder(4, 50.0).tobytes()
    assert list(s.cold_chains) == [0, 1, 2]
    with pytest.raises(ValueError):
        s.temper_swap(2)
    with pytest.raises(ValueError):
        s.temper_swap(-1)
    ck = s.checkpoint()
    s.close()
    other = _sampler(p, 12, betas=[1.0, 0.5, 0.25, 0.125], swap_every=3)
    with pytest.raises(ValueError):
        other.restore(ck)                            # another ladder
    other.temper_enable(ntemps=4, tmax=50.0, swap_every=2)
    with pytest.raises(ValueError):
        other.restore(ck)                            # another swap_every
    other.temper_disable()
    with pytest.raises(ValueError):
        other.restore(ck)                            # not tempered
    other.temper_enable(ntemps=4, tmax=50.0, swap_every=3)
    other.restore(ck)
    other.close()
