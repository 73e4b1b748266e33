"""Probe-to-cell covariances on the GPU (csrc/cov.hip): the gather, accumulate
and reduce kernels against numpy / Python integers word for word, mixed probe
kinds against the chains' own state step by step, the run path against the
kept ring on every launch path, tempering, shards, checkpoints, refusals."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_hypo as TH
import test_gpu_nuis as TN
import test_gpu_posterior as TP
from test_cov_host import check_summary, expected, part_words, want_words

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KEYS = ("A", "G", "S", "Q", "C", "Ac", "Sc")


def _np_sums(x, v, nchains=None):
    """x [n][M][np], v [n][M][ncm] -> the accumulators in int64 numpy (the values
    here are far from 2^63); rows of chains past M (hot chains) stay zero."""
    x, v = x.astype(np.int64), v.astype(np.int64)
    n, M = x.shape[:2]
    nch = M if nchains is None else nchains
    out = {"n": n, "M": M, "A": x.sum((0, 1)), "G": np.einsum("tcp,tcq->pq", x, x), "S": v.sum((0, 1)),
           "Q": (v * v).sum((0, 1)), "C": np.einsum("tcp,tcj->pj", x, v)}
    out["Ac"], out["Sc"] = np.zeros((nch, x.shape[2]), np.int64), np.zeros((nch, v.shape[2]), np.int64)
    out["Ac"][:M], out["Sc"][:M] = x.sum(0), v.sum(0)
    return out


def _reduced(s):
    """PA, P, T of the per-chain sums (products below 2^63 here, asserted) as Python integers."""
    Ac, Sc = s["Ac"], s["Sc"]
    assert float(np.abs(Ac).max()) * float(np.abs(Sc).max()) * len(Ac) < 2.0 ** 62
    return {"PA": (Ac.T @ Ac).tolist(), "P": (Sc * Sc).sum(0).tolist(), "T": (Ac.T @ Sc).tolist()}


def _check_raw(raw, want, within=True):
    assert raw["n"] == want["n"]
    for k in KEYS[:5] + (KEYS[5:] if within else ()):
        assert raw[k].shape == want[k].shape and np.array_equal(raw[k], want[k]), k
    assert within or ("Ac" not in raw and "Sc" not in raw)


def _check_parts(parts, want, within=True):
    assert (parts.nchains, parts.nkept, parts.within) == (want["M"], want["n"], within)
    assert np.array_equal(parts.A, want["A"]) and np.array_equal(parts.S, want["S"])
    for k in ("G", "Q", "C"):
        assert part_words(getattr(parts, k)) == want_words(want[k].tolist()), k
    red = _reduced(want) if within else None
    for k in ("PA", "P", "T"):
        assert part_words(getattr(parts, k)) == (want_words(red[k]) if within else [(0, 0)] * (getattr(parts, k).size // 2)), k
    return red


def _model_probes(p, count):
    """`count` model probes: the tile edges, the phase boundary, the last entry, one duplicate, then others."""
    ncm = p.nphase * p.ncell
    head = [63, 0, 64, p.ncell - 1, p.ncell if p.nphase > 1 else p.ncell - 2, ncm - 1, 63, 1, 5]
    rest = [int(e) for e in np.random.default_rng(3).permutation(ncm) if e not in head]
    return [("model", e) for e in (head + rest)[:count]]


# --- 1. the kernels against numpy / Python integers ---
@pytest.mark.parametrize("within", [False, True])
@pytest.mark.parametrize("nprobe", [1, 33, 64])
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_kernels_against_numpy(phases, nprobe, within):
    """216 cells = 3 tiles + 24 entries (PS: 432, the phase boundary inside a
    tile), 67 chains = a slice of 64 + 3, 5 hand-made states; 33 probes = two
    full groups of 16 + 1."""
    TP._dev()
    from mceik_amd import mcmc
    p = TP._problem(phases)
    nch, ncm = 67, p.nphase * p.ncell
    v = TP._hand_states(p, nch)
    probes = _model_probes(p, nprobe)
    idx = [e for _, e in probes]
    smp = mcmc.Sampler(p, nchains=nch)
    smp.cov_enable(probes, within=within)
    ck = smp.checkpoint()
    assert ck["cov"]["n"] == 0 and not ck["cov"]["C"].any() and ck["cov"]["probes"] == [(0, e) for e in idx]
    del ck["cov"]
    for t in range(len(v)):
        ck["v"] = v[t].reshape(smp.model_shape)
        smp.restore(ck)                  # logl given: no forward runs
        smp.cov_accumulate()
    raw, parts, summ = smp.cov_raw(), smp.cov_partials(), mcmc.cov_summary(smp)
    shape = smp.model_shape
    smp.close()
    want = _np_sums(v[:, :, idx], v)
    _check_raw(raw, want, within)
    red = _check_parts(parts, want, within)
    assert (parts.np, parts.ncm, parts.probes) == (nprobe, ncm, [(0, e) for e in idx])
    # the summary against exact rationals, for the first probes (the named ones) and every entry
    k = min(nprobe, 7)
    sub = {"n": 5, "M": nch, "A": want["A"][:k].tolist(), "S": want["S"].tolist(), "Q": want["Q"].tolist(),
           "G": want["G"][:k, :k].tolist(), "C": want["C"][:k].tolist()}
    if within:
        sub.update(PA=[r[:k] for r in red["PA"][:k]], P=red["P"], T=red["T"][:k])
    ex = expected(sub, within=within)
    got = {"cov": summ.cov, "corr": summ.corr, "cov_within": summ.cov_within, "corr_within": summ.corr_within}
    assert summ.cov.shape == (nprobe,) + shape[1:] and summ.count == 5 and summ.nchains == nch
    check_summary({kk: a.reshape(nprobe, ncm)[:k] for kk, a in got.items()},
                  {kk: ex[kk] for kk in got})
    check_summary({"probe_mean": summ.probe_mean[:k], "probe_cov": summ.probe_cov[:k, :k],
                   "probe_corr": summ.probe_corr[:k, :k], "probe_corr_within": summ.probe_corr_within[:k, :k]},
                  {kk: ex[kk] for kk in ("probe_mean", "probe_cov", "probe_corr", "probe_corr_within")})
    # not vacuous: entry 0 is constant (no correlation, as a column and as a probe), entry 1 is constant per chain
    # (no within-chain correlation), the others correlate weakly, a probe with itself fully
    corr, corrw = summ.corr.reshape(nprobe, ncm), summ.corr_within.reshape(nprobe, ncm)
    e = np.array(idx)
    assert np.isnan(corr[:, 0]).all() and np.isnan(corr[e == 0]).all() and np.isfinite(corr[e != 0][:, 1:]).all()
    assert ((np.abs(corr[e != 0][:, 2:]) > 0) & (np.abs(corr[e != 0][:, 2:]) < 1 - 1e-9)).any()
    assert abs(corr[0, idx[0]] - 1.0) <= 1e-14
    if within:
        assert np.isnan(corrw[:, :2]).all() and np.isnan(corrw[e < 2]).all() and np.isfinite(corrw[e >= 2][:, 2:]).all()
        assert abs(corrw[0, idx[0]] - 1.0) <= 1e-14
    else:
        assert np.isnan(corrw).all() and np.isnan(summ.cov_within).all()
    if nprobe >= 7:
        assert np.array_equal(raw["C"][0], raw["C"][6]) and raw["G"][0, 6] == raw["G"][0, 0]      # the duplicate


# --- 2. mixed probe kinds, one step at a time ---
def test_mixed_probe_kinds(monkeypatch):
    """Steps 0..11 with keepK = 1: nuisance steps 1, 4, 7, 10, hypocentre steps 2, 5, 8, 11, velocity steps
    between; after every step the chains' own state is read back and accumulated in numpy."""
    TH._set_path("per_step", monkeypatch)
    TH._dev()
    from mceik_amd import mcmc
    p = TH._problem("PS", seed=11)
    nch, ncm = 4, 2 * p.ncell

    def sampler():
        smp = mcmc.Sampler(p, nchains=nch)
        TN._enable(smp, TN._nu(p, every=3, offset=1))
        smp.hypo_enable(3, dmax=(1, 1, 1))
        return smp
    # a twin without the feature finds model entries that the velocity steps 3, 6 and 9 change
    # (the chains do not depend on the feature)
    twin = sampler()
    try:
        twin.run(1)                      # (the first kept state is the one after step 0)
        v0 = twin.state()[0].reshape(nch, ncm)
        twin.run(11)
        changed = np.flatnonzero((twin.state()[0].reshape(nch, ncm) != v0).any(0))
    finally:
        twin.close()
    assert len(changed) >= 1
    cells = [int(changed[0]), int(changed[-1]), 7]
    smp = sampler()
    try:
        probes = [("hypo", 0, 2), ("hypo", 3, 0), ("static", 0, 1), ("static", 1, 2), ("noise", 0), ("noise", 1)] + \
                 [("model", e // p.ncell, e % p.ncell) for e in cells]
        smp.cov_enable(probes, within=True)
        xs, vs = [], []
        for _ in range(12):
            smp.run(1)
            v = smp.checkpoint()["v"].reshape(nch, ncm)
            xyz, (kn, kc) = smp.hypo_positions(), smp.nuis_get()
            xs.append(np.stack([xyz[:, 0, 2], xyz[:, 3, 0], kc[:, 0, 1], kc[:, 1, 2], kn[:, 0], kn[:, 1]] +
                               [v[:, e] for e in cells], 1))
            vs.append(v)
        raw, parts = smp.cov_raw(), smp.cov_partials()
    finally:
        smp.close()
    x, v = np.array(xs), np.array(vs)
    assert raw["probes"] == [(1, 2), (1, 9), (2, 1), (2, p.nstat + 2), (3, 0), (3, 1)] + [(0, e) for e in cells]
    want = _np_sums(x, v)
    _check_raw(raw, want)
    _check_parts(parts, want)
    moved = (x != x[:1]).any((0, 1))
    assert moved[0:2].any() and moved[2:4].any() and moved[4:6].any() and moved[6:9].any(), moved
    assert (x[:, :, 2:4] < 0).any() or (x[:, :, 2:4] > 0).any()


# --- 3. the run path: every launch path equals the kept ring, the chains do not change ---
def _run_path(path, monkeypatch, cov, probes=None, max_samples=16, nsteps=40):
    from mceik_amd import mcmc
    cfg = TP._PATHS[path]
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in cfg["env"].items():
        monkeypatch.setenv(k, val)
    p = TP._problem("P", cfg["n"], cfg["nstat"], cfg["nev"], nburn=5, keepk=3)
    smp = mcmc.Sampler(p, nchains=cfg["nchains"], chain_offset=11, max_samples=max_samples)
    if cov:
        smp.cov_enable(probes, within=True)
    info = smp.info()
    smp.run(nsteps)
    out = {"info": info, "state": smp.state(), "kept": smp.samples(), "raw": smp.cov_raw() if cov else None, "p": p}
    smp.close()
    return out


@pytest.mark.parametrize("path", list(TP._PATHS))
def test_run_equals_kept_ring(path, monkeypatch):
    """nburn 5, keepk 3, 40 steps: 12 kept states (steps 5, 8, ..., 38), all in
    the 16-slot ring; the accumulators are the ring's sums and v, logL and
    naccept are those of a twin sampler without the feature."""
    TP._dev()
    cfg = TP._PATHS[path]
    ncell = -(-cfg["n"] // 4) ** 3
    probes = [("model", e) for e in (0, 63, 64, ncell - 1, 70, 0)]
    a = _run_path(path, monkeypatch, True, probes)
    b = _run_path(path, monkeypatch, False)
    info = a["info"]
    if path == "multi_step":
        assert info["multi_step"]
    else:
        assert not info["multi_step"] and info["npipe"] == (2 if path == "two_pipes" else 1)
    kv, _ = a["kept"]
    assert len(kv) == 12 and a["p"].ncell == ncell
    want = _np_sums(kv[:, :, [e for _, e in probes]], kv)
    _check_raw(a["raw"], want)
    assert 0 < a["state"][2].sum() and (kv != kv[:1]).any()
    for x, y in zip(a["state"] + a["kept"], b["state"] + b["kept"]):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
        else:
            assert x == y


# --- 4. tempering: the cold chains only ---
def test_tempering_counts_cold_chains(monkeypatch):
    TH._set_path("per_step", monkeypatch)
    TP._dev()
    from mceik_amd import mcmc
    p = TP._problem("P", nburn=2, keepk=2)
    nch, G = 9, 3
    smp = mcmc.Sampler(p, nchains=nch, max_samples=16)
    smp.temper_enable(betas=TH.LADDER3, swap_every=2)
    probes = [("model", 0), ("model", 100), ("model", p.ncell - 1)]
    smp.cov_enable(probes, within=True)
    smp.run(24)
    raw, parts = smp.cov_raw(), smp.cov_partials()
    kv, _ = smp.samples()
    att, acc = smp.temper_stats()
    smp.close()
    assert len(kv) == 11 and att.sum() > 0           # kept steps 2, 4, ..., 22; swap rounds ran
    want = _np_sums(kv[:, :G][:, :, [e for _, e in probes]], kv[:, :G], nchains=nch)
    _check_raw(raw, want)
    assert not raw["Ac"][G:].any() and not raw["Sc"][G:].any() and raw["Sc"][:G].all()
    want_cold = dict(want, Ac=want["Ac"][:G], Sc=want["Sc"][:G])
    _check_parts(parts, want_cold)
    assert parts.nchains == G


# --- 5. shards merge to the whole ---
def test_shards_merge_exactly(monkeypatch):
    from mceik_amd import mcmc
    TP._dev()
    monkeypatch.setenv("MCEIK_PERSIST", "0")
    p = TP._problem("P", nburn=0, keepk=2)
    probes = [("model", 3), ("model", 64), ("model", p.ncell - 1)]

    def run(nchains, off):
        smp = mcmc.Sampler(p, nchains=nchains, chain_offset=off)
        smp.cov_enable(probes, within=True)
        smp.run(20)
        parts = smp.cov_partials()
        smp.close()
        return parts

    whole, a, b = run(12, 0), run(5, 0), run(7, 5)
    assert whole.nkept == 10 and a.nchains == 5 and b.nchains == 7
    a.merge(b)
    assert a.nchains == 12 and a.nkept == 10
    for k in ("A", "S", "G", "Q", "C", "PA", "P", "T"):
        assert getattr(a, k).tobytes() == getattr(whole, k).tobytes(), k
    assert whole.T.any() and whole.PA.any() and whole.C.any()
    sa, sw = mcmc.CovSummary(a), mcmc.CovSummary(whole)
    for k in ("cov", "corr", "cov_within", "corr_within", "probe_cov", "probe_corr_within"):
        assert getattr(sa, k).tobytes() == getattr(sw, k).tobytes(), k
    assert np.isfinite(sw.cov).all()


# --- 6. checkpoints carry the sums and the probe list ---
def test_checkpoint_carries_the_sums(monkeypatch):
    from mceik_amd import mcmc
    TP._dev()
    monkeypatch.setenv("MCEIK_PERSIST", "0")
    p = TP._problem("P", nburn=0, keepk=1)
    probes = [("model", 3), ("model", 64)]
    s1 = mcmc.Sampler(p, nchains=6)
    s1.cov_enable(probes, within=True)
    s1.run(6)
    want, state = s1.cov_raw(), s1.state()
    s1.close()
    s2 = mcmc.Sampler(p, nchains=6)
    s2.cov_enable(probes, within=True)
    s2.run(3)
    ck = s2.checkpoint()
    s2.close()
    assert ck["cov"]["n"] == 3 and ck["cov"]["probes"] == [(0, 3), (0, 64)] and ck["cov"]["within"]
    s3 = mcmc.Sampler(p, nchains=6)
    s3.cov_enable(probes, within=True)
    s3.restore(ck)
    s3.run(3)
    got, state3 = s3.cov_raw(), s3.state()
    s3.close()
    assert got["n"] == want["n"] == 6 and want["C"].any()
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k
    TH._same(state3, state)
    # another list or another `within` is refused; a sampler without the sums ignores the entry
    for other, within in (([("model", 3), ("model", 65)], True), (probes[:1], True), (probes, False)):
        s4 = mcmc.Sampler(p, nchains=6)
        s4.cov_enable(other, within=within)
        with pytest.raises(ValueError):
            s4.restore(ck)
        s4.close()
    s5 = mcmc.Sampler(p, nchains=6)
    s5.restore(ck)
    assert "cov" not in s5.checkpoint()
    s5.close()


# --- 7. refusals ---
def test_refusals(monkeypatch):
    TH._set_path("per_step", monkeypatch)
    TH._dev()
    from mceik_amd import _lib, mcmc
    L = _lib.lib()
    p = TH._problem("PS", seed=11)
    ncm = 2 * p.ncell
    smp = mcmc.Sampler(p, nchains=4)
    try:
        def rc(probes, within=0):
            o = _lib.CovOpts()
            o.np, o.within = len(probes), within
            for k, (kind, idx) in enumerate(probes[:64]):
                o.kind[k], o.index[k] = kind, idx
            return L.mceik_mcmc_cov_enable(smp._h, C.byref(o))
        assert L.mceik_mcmc_cov_enable(smp._h, None) == 1 and L.mceik_mcmc_cov_accumulate(smp._h) == 1
        with pytest.raises(RuntimeError):
            smp.cov_raw()
        assert rc([]) == 1 and rc([(0, 0)] * 65) == 1                       # np outside [1, 64]
        assert rc([(4, 0)]) == 1 and rc([(-1, 0)]) == 1                     # an unknown kind
        assert rc([(0, -1)]) == 1 and rc([(0, ncm)]) == 1                   # an index out of range
        assert rc([(1, 0)]) == 1 and rc([(2, 0)]) == 1 and rc([(3, 0)]) == 1   # state that is not held
        with pytest.raises(ValueError):
            smp.cov_enable([("hypo", 0, 3)])
        with pytest.raises(ValueError):
            smp.cov_enable([("cell", 0)])
        with pytest.raises(ValueError):
            smp.cov_enable([])
        TN._enable(smp, TN._nu(p, every=3, offset=1, noise=False))          # statics only
        assert rc([(3, 0)]) == 1 and rc([(2, 2 * p.nstat)]) == 1 and rc([(2, -1)]) == 1
        smp.nuis_clear()
        TN._enable(smp, TN._nu(p, every=3, offset=1))
        assert rc([(3, 2)]) == 1 and rc([(1, 0)]) == 1
        smp.hypo_enable(3, dmax=(1, 1, 1))
        smp.hypo_disable()                                                  # the positions stay held
        assert rc([(1, 3 * p.nevents)]) == 1 and rc([(1, -1)]) == 1
        with pytest.raises(RuntimeError):
            smp.cov_raw()                                                   # no refused enable left anything behind
        # held sums: only their own list and `within` may be enabled again
        probes = [("hypo", 1, 2), ("static", 1, 0), ("noise", 1), ("model", 1, 5), ("static", 1, 0)]
        smp.cov_enable(probes)
        smp.cov_enable(probes[:2])                                          # no states yet: another list replaces it
        smp.cov_enable(probes)
        smp.cov_accumulate()
        for bad, within in ((probes[:4], False), (probes[::-1], False), (probes, True)):
            with pytest.raises(ValueError):
                smp.cov_enable(bad, within=within)
        with pytest.raises(ValueError):
            smp.nuis_clear()                                                # a static probe is registered
        smp.cov_disable()
        with pytest.raises(RuntimeError):
            smp.cov_accumulate()                                            # disabled: the sums stay
        assert smp.cov_raw()["n"] == 1
        smp.cov_enable(probes)                                              # the same list resumes them
        smp.cov_accumulate()
        raw = smp.cov_raw()
        assert raw["n"] == 2 and np.array_equal(raw["C"][1], raw["C"][4]) and raw["S"].all()
        smp.cov_disable()
        smp.nuis_clear()                                                    # not while disabled
        with pytest.raises(ValueError):
            smp.cov_enable(probes)                                          # its static and noise probes lost their state
        smp.cov_clear()
        with pytest.raises(RuntimeError):
            smp.cov_raw()
        smp.cov_enable(probes[:1] + probes[3:4], within=True)
        assert smp.cov_raw()["n"] == 0 and not smp.cov_raw()["Sc"].any()
    finally:
        smp.close()
