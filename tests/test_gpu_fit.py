"""Streaming pick residuals, origin times and data-fit checks on the GPU
(csrc/fit.hip) against the restatement tests/_fit.py word for
word: the run path on one- and two-model samplers, with every other feature
on, at ticks where the 128-bit sums carry and where the words saturate, over
a checkpoint, over shards; the chains with and without it; refusals and the
one-model sampler's held tables.

24^3 nodes, 4 stations, 6 events, nburn 2, keepK 2, 24 steps: kept steps 2, 4,
..., 22 (11 states)."""
import numpy as np
import pytest

import _fit
import test_gpu_hypo as TH
import test_gpu_nuis as TN
import test_gpu_posterior as TP

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NCH, NSTEPS, NKEPT = 4, 24, 11
# The problem's varObs is 1e-5, so a residual of 1 ms is z = 100: with the default zmax = 8 every z lands in an
# edge bin.  The restated run spreads the bins over +-512 instead; the other tests keep the defaults.
ZMAX = 512.0
ENVS = {"per_step": {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, "default": {}, "multi_step": {"MCEIK_PERSIST": "1"},
        "two_pipes": {"MCEIK_PIPES": "2"}}


def _env(name, monkeypatch):
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in ENVS[name].items():
        monkeypatch.setenv(k, val)


def _problem(phases, n=24):
    return TP._problem(phases, n=n, nburn=2, keepk=2)


def _states(smp):
    """The kept ring as the restatement's states (the catalogue's observations and nodes)."""
    return [{"v": v} for v in smp.samples()[0]]


def _run(p, fit, nch=NCH, nsteps=NSTEPS, **kw):
    """A run with the sums on: (fit_raw, fit_last, states, info)."""
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=nch, max_samples=16, **kw)
    try:
        smp.fit_enable(**fit)
        info = smp.info()
        smp.run(nsteps)
        return smp.fit_raw(), smp.fit_last(), _states(smp), info
    finally:
        smp.close()


def _assert_last(last, want, p):
    q, zq, tq = last
    for c, (wq, wzq, _, wtq, _) in enumerate(want):
        assert np.array_equal(q[c], wq) and np.array_equal(zq[c], wzq) and np.array_equal(tq[c], wtq), c
    assert not q[len(want):].any() and not tq[len(want):].any()


# --- 1. the restated run ---
@pytest.mark.parametrize("env", ["per_step", "default"])
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_restated_run(phases, env, monkeypatch):
    TP._dev()
    _env(env, monkeypatch)
    p = _problem(phases)
    fit = dict(tick=2.0 ** -20, nbins=64, zmax=ZMAX)
    raw, last, states, info = _run(p, fit)
    assert len(states) == NKEPT and raw["n"] == NKEPT
    f, wlast = _fit.restate(p, states, **fit)
    want = f.raw()
    assert want["hist"].sum() == NKEPT * NCH * int((p.obs_mask == 0).sum()) and want["sat"].tolist() == [0, 0, 0]
    assert np.count_nonzero(want["hist"].sum((0, 1))) > 2, "every z in one or two bins: the histogram shows nothing"
    _fit.assert_raw_equal(raw, want, (phases, env))
    _assert_last(last, wlast, p)
    assert (raw["tick"], raw["nbins"], raw["zmax"]) == (2.0 ** -20, 64, ZMAX) and not raw["t0_ref"].any()


def test_summary_and_t0_ref(monkeypatch):
    """t0_ref moves the words of the origin times and nothing else, and the summary adds it back."""
    from mceik_amd import mcmc
    TP._dev()
    _env("per_step", monkeypatch)
    p = _problem("PS")
    ref = np.linspace(-0.01, 0.01, p.nevents)
    out = []
    for t0_ref in (None, ref):
        smp = mcmc.Sampler(p, nchains=NCH, max_samples=16)
        try:
            smp.fit_enable(nbins=32, zmax=ZMAX, t0_ref=t0_ref)
            smp.run(NSTEPS)
            out.append((smp.fit_raw(), mcmc.fit_summary(smp), _states(smp)))
        finally:
            smp.close()
    (ra, sa, states), (rb, sb, _) = out
    for k in ("sq", "szq", "sq2", "szq2", "hist", "sat"):
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert ra["stq"].tobytes() != rb["stq"].tobytes()
    _fit.assert_raw_equal(rb, _fit.restate(p, states, tick=2.0 ** -20, nbins=32, zmax=ZMAX, t0_ref=ref)[0].raw(), "t0_ref")
    assert np.allclose(sa.t0_mean, sb.t0_mean, rtol=0, atol=2.0 ** -20) and np.allclose(sa.t0_sd, sb.t0_sd, rtol=1e-3)
    assert not p.obs_mask.any() and sa.count == NKEPT and sa.nchains == NCH and sa.hist.sum() == NKEPT * NCH * len(p.tobs)
    assert np.isfinite(sa.pick_mean).all() and (sa.pick_zrms > 0).all() and np.isfinite(sa.ev_misfit).all()
    # the mean residual of a pick is what the states' residuals average to (r within half a tick of q tick)
    r = np.array([[np.concatenate([t[3] for t in mcmc._pick_terms(p, _fit.oracle_tables(p, st["v"][c]), None, None)])
                   for c in range(NCH)] for st in states])
    assert np.allclose(sa.pick_mean, r.mean((0, 1)), rtol=0, atol=2.0 ** -21)


# --- 2. the chains are untouched ---
@pytest.mark.parametrize("phases,env,n", [("P", "per_step", 24), ("P", "multi_step", 32), ("PS", "multi_step", 32),
                                          ("PS", "default", 24)])
def test_chains_untouched(phases, env, n, monkeypatch):
    from mceik_amd import mcmc
    TP._dev()
    _env(env, monkeypatch)
    p = _problem(phases, n=n)
    res = []
    for on in (False, True):
        smp = mcmc.Sampler(p, nchains=NCH, max_samples=16)
        try:
            before = smp.info()
            if on:
                smp.fit_enable()
            info = smp.info()
            smp.run(NSTEPS)
            res.append((smp.state(), smp.samples(), before, info, smp.fit_raw()["n"] if on else None))
        finally:
            smp.close()
    (sa, ka, ba, ia, _), (sb, kb, bb, ib, nb) = res
    TH._same(sa, sb, "state")
    TH._same(ka, kb, "samples")
    assert nb == NKEPT and ba == bb == ia
    if env == "multi_step":
        assert ia["multi_step"], ia
    if phases == "P":                    # a one-model sampler leaves the multi-step launches: this pins the two branches
        assert not ib["multi_step"]
    else:                                # a two-model sampler keeps them
        assert ib["multi_step"] == ia["multi_step"]


# --- 3. everything on: the cold-chain boundary inside a pipe ---
def _everything(env, monkeypatch, stepwise):
    from mceik_amd import mcmc
    _env(env, monkeypatch)
    p = _problem("P")
    smp = mcmc.Sampler(p, nchains=9, max_samples=16)
    try:
        smp.temper_enable(betas=TH.LADDER3, swap_every=2)
        smp.hypo_enable(3, dmax=(1, 1, 1))
        TN._enable(smp, TN._nu(p, every=3, offset=1))
        smp.posterior_enable(per_chain=True, nbins=16)
        probes = [("model", 100), ("hypo", 0, 2), ("static", 0, 1), ("noise", 0)]
        smp.cov_enable(probes, within=True)
        smp.ess_enable(3, probes=probes)
        smp.fit_enable()
        info, states = smp.info(), []
        if stepwise:
            for gs in range(NSTEPS):
                smp.run(1)
                if gs >= p.nburn and (gs - p.nburn) % p.keepk == 0:
                    li = mcmc.logl_inputs(smp)
                    states.append({"v": smp.state()[0].copy(), "hyp": li["hyp"], "var": li["var"], "tcorr": li["tcorr"]})
        else:
            smp.run(NSTEPS)
        return p, info, smp.fit_raw(), smp.fit_partials(), smp.fit_last(), states, smp.state()
    finally:
        smp.close()


def test_everything_on(monkeypatch):
    TP._dev()
    p, i1, raw1, parts1, last1, states, st1 = _everything("per_step", monkeypatch, True)
    _, i2, raw2, parts2, last2, _, st2 = _everything("two_pipes", monkeypatch, False)
    assert i1["npipe"] == 1 and i2["npipe"] == 2 and i2["chains"] == [4, 5], (i1, i2)
    TH._same(st1, st2, "state")
    _fit.assert_raw_equal(raw1, raw2, "one pipe stepwise vs two pipes")
    TH._same(last1, last2, "fit_last")
    assert raw2["n"] == NKEPT == len(states) and parts2.nchains == 3 and parts2.nkept == NKEPT
    assert any(not np.array_equal(s["hyp"][:3], states[0]["hyp"][:3]) for s in states), "no hypocentre moved"
    assert any(not np.array_equal(s["var"][:3], states[0]["var"][:3]) for s in states), "no noise scale moved"
    f, wlast = _fit.restate(p, states, ncold=3)
    _fit.assert_raw_equal(raw2, f.raw(), "restatement")
    _assert_last(last2, wlast, p)
    assert raw2["hist"].sum() == NKEPT * 3 * len(p.tobs)


# --- 4. carries and saturation ---
def test_carry_and_saturation(monkeypatch):
    TP._dev()
    _env("per_step", monkeypatch)
    p = _problem("P")
    for tick in (2.0 ** -34, 2.0 ** -40):
        fit = dict(tick=tick, nbins=64, zmax=8.0)
        raw, last, states, _ = _run(p, fit)
        f, wlast = _fit.restate(p, states, **fit)
        want = f.raw()
        r = np.abs(np.array(f.sq, dtype=np.float64)) * tick / (NKEPT * NCH)
        print(f"tick 2^{int(np.log2(tick))}: largest |mean residual| {r.max():.3e} s, hi words "
              f"{want['sq2'][:, 1].tolist()}, saturated {want['sat'].tolist()}")
        if tick == 2.0 ** -34:
            assert want["sq2"][:, 1].any(), "no sum of squares crossed 2^64"
        else:
            assert want["sat"][0] > 0
            nsat = sum(int((np.abs(st_q) == 2 ** 31 - 1).sum()) for st_q in [w[0] for w in wlast])
            assert nsat > 0 and np.abs(last[0]).max() == 2 ** 31 - 1
        _fit.assert_raw_equal(raw, want, tick)
        _assert_last(last, wlast, p)


# --- 5. checkpoint ---
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_checkpoint(phases, monkeypatch):
    from mceik_amd import mcmc
    TP._dev()
    _env("per_step", monkeypatch)
    p = _problem(phases)
    straight = _run(p, {})[0]
    a = mcmc.Sampler(p, nchains=NCH, max_samples=16)
    b = mcmc.Sampler(p, nchains=NCH, max_samples=16)
    try:
        a.fit_enable()
        a.run(12)
        ck = a.checkpoint()
        assert ck["fit"]["n"] == 5                   # kept steps 2, 4, 6, 8, 10
        b.fit_enable()
        b.restore(ck, recompute_logl=(phases == "PS"))      # (two models: the forward makes both models' current tables)
        TH._same((b.state()[1],), (ck["logl"],), "logL after restore")
        b.run(12)
        _fit.assert_raw_equal(b.fit_raw(), straight, "12 + 12")
        b.fit_clear()
        b.fit_enable(nbins=32)
        with pytest.raises(ValueError):
            b.restore(ck)
    finally:
        a.close()
        b.close()


# --- 6. shards ---
def test_shards(monkeypatch):
    from mceik_amd import mcmc
    TP._dev()
    _env("per_step", monkeypatch)
    p = _problem("PS")
    parts = []
    for nch, off in ((4, 0), (2, 0), (2, 2)):
        smp = mcmc.Sampler(p, nchains=nch, chain_offset=off)
        try:
            smp.fit_enable()
            smp.run(NSTEPS)
            parts.append(smp.fit_partials())
        finally:
            smp.close()
    whole, a, b = parts
    a.merge(b)
    assert (a.nchains, a.nkept) == (whole.nchains, whole.nkept) == (4, NKEPT)
    for k in _fit.ARRAYS + ("obs_ptr", "obs_stat", "obs_phase", "obs_mask", "t0_ref"):
        x, y = getattr(a, k), getattr(whole, k)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    assert np.array_equal(whole.obs_ptr, p.obs_ptr) and np.array_equal(whole.obs_mask, p.obs_mask)
    assert np.array_equal(whole.obs_phase, p.obs_phase) and whole.sq2.any()


# --- 7. refusals and the one-model sampler's held tables ---
def test_refusals_and_table_holding(monkeypatch):
    from mceik_amd import mcmc
    TP._dev()
    _env("per_step", monkeypatch)
    p = _problem("P")
    smp = mcmc.Sampler(p, nchains=NCH)
    try:
        for bad in (dict(tick=1e-6), dict(tick=0.0), dict(tick=3 * 2.0 ** -20), dict(nbins=63), dict(nbins=0),
                    dict(nbins=258), dict(zmax=0.0), dict(zmax=-1.0), dict(zmax=float("nan")), dict(zmax=float("inf")),
                    dict(t0_ref=np.full(p.nevents, np.nan))):
            with pytest.raises(ValueError):
                smp.fit_enable(**bad)
        with pytest.raises(ValueError):
            smp.fit_enable(t0_ref=np.zeros(p.nevents + 1))
        with pytest.raises(RuntimeError):
            smp.fit_raw()
        l0 = smp.state()[1]
        smp.fit_enable()
        TH._same((smp.state()[1],), (l0,), "enable leaves logL")
        smp.fit_enable(nbins=32)                    # no states held yet: other options replace the empty sums
        assert smp.fit_raw()["hist"].shape[-1] == 32
        smp.run(6)
        assert smp.fit_raw()["n"] == 2               # steps 0 .. 5: kept 2, 4
        for other in (dict(nbins=64), dict(nbins=32, tick=2.0 ** -21), dict(nbins=32, zmax=7.0),
                      dict(nbins=32, t0_ref=np.ones(p.nevents))):
            with pytest.raises(ValueError):
                smp.fit_enable(**other)
        smp.fit_disable()
        smp.run(2)                                   # kept step 6 passes unseen
        smp.fit_enable(nbins=32)                     # the held options: the sums go on
        smp.run(2)
        assert smp.fit_raw()["n"] == 3               # steps 8, 9: kept 8
        held, again = TN._recomputed_logl(smp)
        TH._same((held,), (again,), "logL, fit on")
        # nuisance state comes and goes while the sums are on: the tables stay
        TN._enable(smp, TN._nu(p, every=2, offset=1))
        smp.run(4)
        held, again = TN._recomputed_logl(smp)
        TH._same((held,), (again,), "logL with nuisance state")
        smp.nuis_clear()
        smp.run(3)
        n = smp.fit_raw()["n"]
        assert n == 3 + 2 + 2                        # steps 10 .. 16: kept 10, 12 | 14, 16
        held, again = TN._recomputed_logl(smp)
        TH._same((held,), (again,), "logL after nuis_clear")
        # ... and the other way round: the sums go while nuisance state is held
        TN._enable(smp, TN._nu(p, every=2, offset=1))
        smp.run(2)
        smp.fit_clear()
        with pytest.raises(RuntimeError):
            smp.fit_partials()
        smp.run(3)
        held, again = TN._recomputed_logl(smp)
        TH._same((held,), (again,), "logL after fit_clear")
        smp.nuis_clear()
        smp.run(2)
        held, again = TN._recomputed_logl(smp)
        TH._same((held,), (again,), "logL, the plain sampler again")
    finally:
        smp.close()
