"""Batch-means effective sample sizes on the GPU (csrc/ess.hip): the accumulate
kernel against the restatement tests/_ess.py word for word, the run path
against the kept ring on every launch path, shards, checkpoints, tempering,
probes against the chains' own state step by step, errors."""
import numpy as np
import pytest

import _ess
import test_gpu_hypo as TH
import test_gpu_nuis as TN
import test_gpu_posterior as TP
from test_posterior_host import check_close

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _restate(states, nlevels):
    """states [n][M][ne] -> the restatement after adding them in order."""
    e = _ess.Ess(states.shape[1], states.shape[2], nlevels)
    for s in states:
        e.add(s)
    return e


def _words(a):
    """uint64 [..., 2] (lo, hi) -> Python integers modulo 2^128, flat."""
    a = np.asarray(a).reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in a]


def _check_raw(raw, e, sel=None, nchains=None):
    """Sc, pend, A, Q, P of `ess_raw` against the restatement, word for word, on
    the entries `sel` (all); rows of chains past the restatement's (hot ones) are zero."""
    L, M = e.L, e.M
    sel = np.arange(raw["Sc"].shape[1]) if sel is None else np.asarray(sel)
    assert raw["n"] == e.n and raw["nlevels"] == L
    assert raw["Sc"].shape[0] == (M if nchains is None else nchains) and raw["pend"].shape[0] == L - 1
    assert raw["Sc"][:M][:, sel].tolist() == e.Sc.tolist(), "Sc"
    assert raw["pend"][:, :M][:, :, sel].tolist() == e.pend.tolist(), "pend"
    assert not raw["Sc"][M:].any() and not raw["pend"][:, M:].any()
    assert raw["A"][:, sel].tolist() == e.A.tolist(), "A"
    m128 = (1 << 128) - 1
    assert _words(raw["Q"][:, sel]) == [int(x) & m128 for x in e.Q.ravel()], "Q"
    assert _words(raw["P"][:, sel]) == [int(x) & m128 for x in e.P.ravel()], "P"


def _accumulate_by_hand(p, nchains, v, nlevels, level=None):
    """The hand-state pattern of tests/test_gpu_posterior.py: restore a state with logl given, then accumulate."""
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=nchains)
    try:
        smp.ess_enable(nlevels)
        ck = smp.checkpoint()
        assert ck["ess"]["n"] == 0 and not ck["ess"]["Sc"].any() and not ck["ess"]["Q"].any()
        del ck["ess"]
        for t in range(len(v)):
            ck["v"] = v[t].reshape(smp.model_shape)
            smp.restore(ck)              # logl given: no forward runs
            smp.ess_accumulate()
        return smp.ess_raw(), smp.ess_partials(), mcmc.ess_summary(smp, level=level), smp.model_shape
    finally:
        smp.close()


# --- 1. the kernel against the restatement ---
@pytest.mark.parametrize("nlevels,nstates", [(4, 19), (1, 3), (16, 3)])
def test_kernel_against_restatement(nlevels, nstates):
    """PS at 24^3: 432 entries = 6 tiles + 48, the phase boundary inside a tile; 67 chains = a slice of 64 +
    3.  L = 4 and 19 states: t = 8 has k = L - 1, t = 16 has k > L - 1, 19 is a multiple of no batch size
    above 1.  Entry 0 is constant everywhere, entry 1 constant per chain, entries at vmin and vmax.
    L = 1 has no pend; L = 16 with 3 states closes nothing above level 1."""
    TP._dev()
    p = TP._problem("PS")
    nch, ncm = 67, p.nphase * p.ncell
    v = TP._hand_states(p, nch, nstates)
    assert v.shape == (nstates, nch, ncm) and (v == p.vmin).any() and (v == p.vmax).any()
    raw, parts, summ, shape = _accumulate_by_hand(p, nch, v, nlevels)
    e = _restate(v, nlevels)
    _check_raw(raw, e)
    assert (parts.ncm, parts.np, parts.nlevels, parts.nchains, parts.nkept) == (ncm, 0, nlevels, nch, nstates)
    assert parts.A.tolist() == e.A.tolist() and _words(parts.Q) == [int(x) for x in e.Q.ravel()]
    assert _words(parts.P) == [int(x) for x in e.P.ravel()]
    et, ee, em, el = _ess.expected(e.Q, e.P, nch, nstates, nlevels)
    assert summ.level == el == _ess.lstar(nlevels, nstates) and summ.count == nstates and summ.nchains == nch
    assert summ.tau_levels.shape == (nlevels,) + shape[1:] and summ.ess.shape == shape[1:]
    check_close(summ.tau_levels.reshape(nlevels, ncm).ravel(), et.ravel(), "tau")
    check_close(summ.ess.ravel(), ee, "ess")
    check_close(summ.mcse.ravel(), em, "mcse")
    # not vacuous: the constant entries are NaN (R-hat's rule), the others are not
    assert np.isnan(ee[:2]).all() and np.isfinite(ee[2:]).all() and np.isfinite(et[0, 2:]).all()
    if nlevels == 4:
        assert summ.level == 2 and np.isfinite(et[:, 2:]).all() and raw["pend"].any()


def test_kernel_many_levels():
    """The instances that close more than four levels at once: L = 10 and 260 states (t = 16 closes 5,
    t = 256 closes 9), P at 24^3 (216 entries = 3 tiles + 24), 5 chains (wave 0 takes two of them)."""
    TP._dev()
    p = TP._problem("P")
    nch, ncm, n, L = 5, p.ncell, 260, 10
    rng = np.random.default_rng(17)
    v = rng.integers(p.vmin, p.vmax + 1, (n, nch, ncm)).astype(np.int32)
    v[:, :, 3] = p.vmax
    raw, parts, summ, _ = _accumulate_by_hand(p, nch, v, L, level=7)
    e = _restate(v, L)
    _check_raw(raw, e)
    et, ee, em, el = _ess.expected(e.Q, e.P, nch, n, L, 7)
    assert summ.level == 7 and np.isnan(et[8:]).all() and np.isfinite(et[:8, 4:]).all()
    check_close(summ.tau_levels.reshape(L, ncm).ravel(), et.ravel(), "tau")
    check_close(summ.ess.ravel(), ee, "ess")


# --- 2. the run path: every launch path equals the kept ring, the chains do not change ---
def _run_path(path, monkeypatch, ess, max_samples=32, nsteps=40):
    from mceik_amd import mcmc
    cfg = TP._PATHS[path]
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in cfg["env"].items():
        monkeypatch.setenv(k, val)
    p = TP._problem("P", cfg["n"], cfg["nstat"], cfg["nev"], nburn=3, keepk=2)
    smp = mcmc.Sampler(p, nchains=cfg["nchains"], chain_offset=11, max_samples=max_samples)
    try:
        if ess:
            smp.ess_enable(4)
        info = smp.info()
        smp.run(nsteps)
        return {"info": info, "state": smp.state(), "kept": smp.samples(), "raw": smp.ess_raw() if ess else None}
    finally:
        smp.close()


@pytest.mark.parametrize("path", list(TP._PATHS))
def test_run_equals_kept_ring(path, monkeypatch):
    """nburn 3, keepk 2, 40 steps: 19 kept states (steps 3, 5, ..., 39), all in the 32-slot ring; the
    accumulators are the restatement's fed from the ring, and v, logL and naccept are those of a twin
    sampler without the feature.  Large models: the 128-bit words on every 37th entry and the last tile,
    Sc in full."""
    TP._dev()
    a = _run_path(path, monkeypatch, True)
    b = _run_path(path, monkeypatch, False)
    info = a["info"]
    if path == "multi_step":
        assert info["multi_step"]
    else:
        assert not info["multi_step"] and info["npipe"] == (2 if path == "two_pipes" else 1)
    kv, _ = a["kept"]
    assert len(kv) == 19 and (kv != kv[:1]).any()
    ncm = kv.shape[2]
    sel = np.arange(ncm) if ncm <= 512 else np.unique(np.r_[np.arange(0, ncm, 37), np.arange(ncm - 64, ncm)])
    _check_raw(a["raw"], _restate(kv[:, :, sel], 4), sel)
    assert np.array_equal(a["raw"]["Sc"], kv.astype(np.int64).sum(0))
    assert np.array_equal(a["raw"]["A"][0], kv.astype(np.int64).sum((0, 1)))
    assert 0 < a["state"][2].sum()
    for x, y in zip(a["state"] + a["kept"], b["state"] + b["kept"]):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
        else:
            assert x == y


# --- 3. shards, checkpoints, tempering ---
def test_shards_merge_exactly(monkeypatch):
    from mceik_amd import mcmc
    TP._dev()
    monkeypatch.setenv("MCEIK_PERSIST", "0")
    p = TP._problem("P", nburn=0, keepk=2)

    def run(nchains, off):
        smp = mcmc.Sampler(p, nchains=nchains, chain_offset=off)
        try:
            smp.ess_enable(3)
            smp.run(20)
            return smp.ess_partials()
        finally:
            smp.close()

    whole, a, b = run(12, 0), run(5, 0), run(7, 5)
    assert whole.nkept == 10 and a.nchains == 5 and b.nchains == 7
    a.merge(b)
    assert a.nchains == 12 and a.nkept == 10
    for k in ("A", "Q", "P"):
        assert getattr(a, k).tobytes() == getattr(whole, k).tobytes(), k
    assert whole.A.all() and whole.Q.any() and whole.P.any()
    sa, sw = mcmc.EssSummary(a), mcmc.EssSummary(whole)
    for k in ("tau_levels", "tau", "ess", "mcse"):
        assert getattr(sa, k).tobytes() == getattr(sw, k).tobytes(), k
    assert sw.level == 1 and np.isfinite(sw.ess).any()


def test_checkpoint_carries_the_open_batches(monkeypatch):
    """nburn 2, keepk 3: 9 steps keep 3 states (steps 2, 5, 8), an odd count, so pend[0] and pend[1] are
    live in the checkpoint; a fresh sampler continues to the words of the uninterrupted run."""
    from mceik_amd import mcmc
    TP._dev()
    monkeypatch.setenv("MCEIK_PERSIST", "0")
    p = TP._problem("P", nburn=2, keepk=3)
    keys = ("Sc", "pend", "A", "Q", "P")
    s1 = mcmc.Sampler(p, nchains=6)
    s1.ess_enable(4)
    s1.run(24)
    want = s1.ess_raw()
    s1.close()
    s2 = mcmc.Sampler(p, nchains=6)
    s2.ess_enable(4)
    s2.run(9)
    ck = s2.checkpoint()
    s2.close()
    assert ck["ess"]["n"] == 3 and ck["ess"]["pend"][0].any() and ck["ess"]["pend"][1].any()
    s3 = mcmc.Sampler(p, nchains=6)
    s3.ess_enable(4)
    s3.restore(ck)
    s3.run(15)
    got = s3.ess_raw()
    s3.close()
    assert got["n"] == want["n"] == 8
    for k in keys:
        assert got[k].tobytes() == want[k].tobytes(), k
    # another hierarchy is refused; a sampler without the sums ignores the entry; a checkpoint without it is as before
    s4 = mcmc.Sampler(p, nchains=6)
    s4.ess_enable(5)
    with pytest.raises(ValueError):
        s4.restore(ck)
    s4.ess_clear()
    s4.restore(ck)
    assert "ess" not in s4.checkpoint()
    s4.ess_enable(4)
    del ck["ess"]
    s4.restore(ck)
    assert s4.ess_raw()["n"] == 0
    s4.close()


def test_tempering_counts_cold_chains(monkeypatch):
    TH._set_path("per_step", monkeypatch)
    TP._dev()
    from mceik_amd import mcmc
    p = TP._problem("P", nburn=2, keepk=2)
    nch, G = 6, 3
    smp = mcmc.Sampler(p, nchains=nch, max_samples=16)
    try:
        smp.temper_enable(betas=[1.0, 0.5], swap_every=2)
        smp.ess_enable(3)
        smp.run(24)
        raw, parts = smp.ess_raw(), smp.ess_partials()
        kv, _ = smp.samples()
        att, _ = smp.temper_stats()
    finally:
        smp.close()
    assert len(kv) == 11 and att.sum() > 0           # kept steps 2, 4, ..., 22; swap rounds ran
    _check_raw(raw, _restate(kv[:, :G], 3), nchains=nch)
    assert raw["Sc"][:G].all() and parts.nchains == G and parts.nkept == 11


# --- 4. probes, one step at a time ---
def test_probes_against_the_chains_state(monkeypatch):
    """Steps 0..11 with keepK = 1: nuisance steps 1, 4, 7, 10, hypocentre steps 2, 5, 8, 11, velocity steps
    between; after every step the chains' own state is read back and fed to the restatement: the cells,
    then one hypocentre axis and the statics of every station of phase 0 (pair moves: some go negative)."""
    TH._set_path("per_step", monkeypatch)
    TH._dev()
    from mceik_amd import mcmc
    p = TH._problem("PS", seed=11)
    nch, ncm, L = 4, 2 * p.ncell, 3
    smp = mcmc.Sampler(p, nchains=nch)
    try:
        TN._enable(smp, TN._nu(p, every=3, offset=1))
        smp.hypo_enable(3, dmax=(1, 1, 1))
        probes = [("hypo", 0, 2)] + [("static", 0, k) for k in range(p.nstat)]
        smp.ess_enable(L, probes=probes)
        states = []
        for _ in range(12):
            smp.run(1)
            v = smp.checkpoint()["v"].reshape(nch, ncm)
            xyz, (kn, kc) = smp.hypo_positions(), smp.nuis_get()
            states.append(np.concatenate([v, xyz[:, 0, 2:3], kc[:, 0, :]], 1))
        raw, summ = smp.ess_raw(), mcmc.ess_summary(smp)
        with pytest.raises(ValueError):
            smp.nuis_clear()             # a registered probe reads the values
    finally:
        smp.close()
    s = np.array(states).astype(np.int64)
    assert raw["probes"] == [(1, 2)] + [(2, k) for k in range(p.nstat)]
    assert (s[:, :, ncm + 1:] < 0).any() and (s[:, :, ncm] != s[:1, :, ncm]).any(), "a static below zero, a hypocentre that moved"
    e = _restate(s, L)
    _check_raw(raw, e)
    et, ee, em, _ = _ess.expected(e.Q, e.P, nch, 12, L)
    assert summ.probe_ess.shape == (1 + p.nstat,) and summ.level == 1 and summ.probes == raw["probes"]
    check_close(summ.probe_tau_levels.ravel(), et[:, ncm:].ravel(), "probe tau")
    check_close(summ.probe_ess, ee[ncm:], "probe ess")
    check_close(summ.probe_mcse, em[ncm:], "probe mcse")
    check_close(summ.ess.ravel(), ee[:ncm], "ess")


# --- 5. errors ---
def test_errors():
    from mceik_amd import mcmc
    TP._dev()
    p = TP._problem("P")
    smp = mcmc.Sampler(p, nchains=3)
    try:
        for call in (smp.ess_raw, smp.ess_accumulate, smp.ess_partials):
            with pytest.raises(RuntimeError):
                call()
        for bad in (0, 17, -1):
            with pytest.raises(ValueError):
                smp.ess_enable(bad)
        with pytest.raises(ValueError):
            smp.ess_enable(4, probes=[("hypo", 0, 0)])       # no hypocentre state is held
        with pytest.raises(RuntimeError):
            smp.ess_raw()
        smp.ess_enable(4)
        smp.ess_accumulate()
        assert smp.ess_raw()["n"] == 1 and smp.ess_raw()["Sc"].all()
        with pytest.raises(ValueError):
            smp.ess_enable(5)            # the sums hold a state of another hierarchy
        smp.ess_disable()
        with pytest.raises(RuntimeError):
            smp.ess_accumulate()
        smp.ess_enable(4)                # the held sums go on
        smp.ess_accumulate()
        assert smp.ess_raw()["n"] == 2
        smp.ess_clear()
        with pytest.raises(RuntimeError):
            smp.ess_raw()
        smp.ess_enable(5)
        assert smp.ess_raw()["n"] == 0 and not smp.ess_raw()["A"].any()
    finally:
        smp.close()
    # the int32 bound of a half batch: vmax 2^(L - 2) >= 2^31 is refused, one level less is not
    import copy
    q = copy.copy(p)
    q.vmax = 200000
    assert not mcmc.ess_check(16, q.vmax) and mcmc.ess_check(15, q.vmax)
    smp = mcmc.Sampler(q, nchains=2, v0=mcmc.initial_models(p, range(2)))
    try:
        with pytest.raises(ValueError):
            smp.ess_enable(16)
        smp.ess_enable(15)
        smp.ess_accumulate()
        assert smp.ess_raw()["n"] == 1
    finally:
        smp.close()
