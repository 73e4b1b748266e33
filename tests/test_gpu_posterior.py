"""Streaming posterior on the GPU (csrc/posterior.hip): the accumulate and
reduce kernels against numpy / Python integers bit for bit, the run path
against the kept ring on every launch path, shards, checkpoints, errors."""
import numpy as np
import pytest
import torch

from test_posterior_host import check_close, expected, words

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _problem(phases="P", n=24, nstat=4, nev=6, nburn=0, keepk=1):
    """Like tests/test_gpu_mcmc.py::_problem; the picks (one GPU forward) are made once per shape."""
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


def _bins(p, v, nbins):
    """Bin of every value of v [..., nphase, ncell] (or [..., ncell]): the header's integer formula."""
    v = v.reshape(v.shape[:-1 if p.nphase == 1 else -2] + (p.nphase, p.ncell)).astype(np.int64)
    lo = np.array([p.vmin, p.vsmin][:p.nphase], np.int64)[:, None]
    hi = np.array([p.vmax, p.vsmax][:p.nphase], np.int64)[:, None]
    return np.clip((v - lo) * nbins // (hi - lo + 1), 0, nbins - 1)


def _hist(p, states, nbins):
    """[ncm][nbins] counts over every leading axis of states [..., (nphase,) ncell]."""
    ncm = p.nphase * p.ncell
    b = _bins(p, states, nbins).reshape(-1, ncm)
    flat = (np.arange(ncm)[None, :] * nbins + b).ravel()
    return np.bincount(flat, minlength=ncm * nbins).reshape(ncm, nbins)


def _hand_states(p, nchains, nstates=5):
    """Random models inside the prior: entry 0 the same for all chains of a
    state, entry 1 constant per chain, some entries exactly vmin / vmax."""
    rng = np.random.default_rng(11)
    ncm = p.nphase * p.ncell
    lo = np.repeat(np.array([p.vmin, p.vsmin][:p.nphase]), p.ncell)
    hi = np.repeat(np.array([p.vmax, p.vsmax][:p.nphase]), p.ncell)
    v = rng.integers(lo, hi + 1, (nstates, nchains, ncm)).astype(np.int32)
    v[:, :, 0] = 2500
    v[:, :, 1] = rng.integers(p.vmin, p.vmax + 1, nchains)[None, :]
    v[:, ::3, 5] = p.vmin
    v[:, 1::3, 5] = p.vmax
    v[:, ::2, ncm - 1] = hi[-1]          # the last entries (the tail tile): the last phase's bounds
    v[:, 1::2, ncm - 2] = lo[-1]
    v[0, :, 64] = hi[64]                 # first lane of the second tile
    return v


def _accumulate_by_hand(p, nchains, v, per_chain, nbins):
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=nchains)
    smp.posterior_enable(per_chain=per_chain, nbins=nbins)
    ck = smp.checkpoint()
    assert ck["posterior"]["n"] == 0 and not ck["posterior"]["sum"].any()
    del ck["posterior"]
    for t in range(len(v)):
        ck["v"] = v[t].reshape(smp.model_shape)
        smp.restore(ck)                  # logl given: no forward runs
        smp.posterior_accumulate()
    raw, parts, summ = smp.posterior_raw(), smp.posterior_partials(), mcmc.posterior_summary(smp)
    shape = smp.model_shape
    smp.close()
    return raw, parts, summ, shape


@pytest.mark.parametrize("nbins", [0, 7, 128])
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_kernels_against_numpy(phases, nbins):
    """216 cells = 3 tiles + 24 entries (PS: 432 = 6 tiles + 48, the phase
    boundary inside a tile), 67 chains = a slice of 64 + 3."""
    _dev()
    p = _problem(phases)
    nch, ncm = 67, p.nphase * p.ncell
    v = _hand_states(p, nch)
    raw, parts, summ, shape = _accumulate_by_hand(p, nch, v, True, nbins)
    v64 = v.astype(np.int64)
    assert raw["n"] == 5 and raw["sum"].shape == shape and raw["hist"].shape == shape[1:] + (nbins,)
    assert np.array_equal(raw["sum"].reshape(nch, ncm), v64.sum(0))
    assert np.array_equal(raw["sumsq"].reshape(nch, ncm), (v64 ** 2).sum(0))
    want_hist = _hist(p, v.reshape((5, nch) + shape[1:]), nbins) if nbins else np.zeros((ncm, 0), np.int64)
    assert np.array_equal(raw["hist"].reshape(ncm, nbins).astype(np.int64), want_hist)
    if nbins:
        assert (want_hist.sum(1) == 5 * nch).all() and want_hist[:, 0].any() and want_hist[:, -1].any()
    # partials: Python integers, word for word
    sums = [[int(x) for x in row] for row in v64.sum(0)]
    S = [sum(r[i] for r in sums) for i in range(ncm)]
    Q = [int(x) for x in (v64 ** 2).sum((0, 1))]
    P = [sum(r[i] ** 2 for r in sums) for i in range(ncm)]
    assert (parts.ncm, parts.nbins, parts.per_chain, parts.nchains, parts.nkept) == (ncm, nbins, True, nch, 5)
    assert [int(x) for x in parts.S] == S
    assert [(int(a), int(b)) for a, b in parts.Q] == words(Q)
    assert [(int(a), int(b)) for a, b in parts.P] == words(P)
    assert np.array_equal(parts.hist.astype(np.int64), want_hist)
    # summary against exact rationals
    em, ev, er = expected(S, Q, P, nch, 5)
    assert np.isnan(er[0]) and np.isnan(er[1]) and np.isfinite(er[2:]).all()      # not vacuous
    check_close(summ.mean.ravel(), em, "mean")
    check_close(summ.var.ravel(), ev, "var")
    check_close(summ.rhat.ravel(), er, "rhat")
    assert summ.count == 5 and summ.nchains == nch and summ.mean.shape == shape[1:]
    if nbins == 128:
        # 5 * 67 = 335 values per entry: the median is the 168th, which lies in the bin
        # where the cumulative count reaches 167.5, so the two agree within a bin width
        width = (p.vmax - p.vmin + 1) / nbins
        med = summ.quantile(0.5).ravel()[:p.ncell]
        ref = np.quantile(v64.reshape(-1, ncm)[:, :p.ncell], 0.5, axis=0)
        assert np.all(np.abs(med - ref) <= width)
        assert np.all(summ.quantile(0.0) <= summ.quantile(1.0))


def test_pooled_mode():
    _dev()
    p = _problem("PS")
    nch, ncm = 67, p.nphase * p.ncell
    v = _hand_states(p, nch)
    raw, parts, summ, shape = _accumulate_by_hand(p, nch, v, False, 7)
    v64 = v.astype(np.int64)
    assert raw["sum"].shape == shape[1:]
    assert np.array_equal(raw["sum"].ravel(), v64.sum((0, 1)))
    assert np.array_equal(raw["sumsq"].ravel(), (v64 ** 2).sum((0, 1)))
    assert np.array_equal(raw["hist"].reshape(ncm, 7).astype(np.int64), _hist(p, v.reshape((5, nch) + shape[1:]), 7))
    assert np.array_equal(parts.S, v64.sum((0, 1))) and not parts.P.any() and not parts.per_chain
    assert np.isnan(summ.rhat).all() and np.isfinite(summ.var).all()
    check_close(summ.mean.ravel(), v64.sum((0, 1)) / (5.0 * nch), "mean")


# --- the run path: launch paths, max_samples = 0 ---
_PATHS = {
    "one_pipe": dict(env={"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, n=24, nstat=4, nev=6, nchains=6),
    "two_pipes": dict(env={"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}, n=40, nstat=4, nev=6, nchains=5),
    "multi_step": dict(env={"MCEIK_PERSIST": "1"}, n=64, nstat=8, nev=8, nchains=64),
}


def _run_path(path, monkeypatch, posterior, max_samples=16, nsteps=40):
    from mceik_amd import mcmc
    cfg = _PATHS[path]
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in cfg["env"].items():
        monkeypatch.setenv(k, val)
    p = _problem("P", cfg["n"], cfg["nstat"], cfg["nev"], nburn=5, keepk=3)
    smp = mcmc.Sampler(p, nchains=cfg["nchains"], chain_offset=11, max_samples=max_samples)
    if posterior:
        smp.posterior_enable(per_chain=True, nbins=16)
    info = smp.info()
    smp.run(nsteps)
    out = {"info": info, "state": smp.state(), "kept": smp.samples() if max_samples else None,
           "raw": smp.posterior_raw() if posterior else None, "p": p}
    smp.close()
    return out


@pytest.mark.parametrize("path", list(_PATHS))
def test_run_equals_kept_ring(path, monkeypatch):
    """nburn 5, keepk 3, 40 steps: 12 kept states (steps 5, 8, ..., 38), all in
    the 16-slot ring; the accumulators are the ring's sums and the chains are
    those of a run without the posterior.  max_samples = 0 gives the same
    accumulators."""
    _dev()
    a = _run_path(path, monkeypatch, True)
    b = _run_path(path, monkeypatch, False)
    c = _run_path(path, monkeypatch, True, max_samples=0)
    info, p = a["info"], a["p"]
    if path == "multi_step":
        assert info["multi_step"]
    else:
        assert not info["multi_step"] and info["npipe"] == (2 if path == "two_pipes" else 1)
    kv, kl = a["kept"]
    raw = a["raw"]
    assert len(kv) == 12 and raw["n"] == 12
    k64 = kv.astype(np.int64)
    assert np.array_equal(raw["sum"], k64.sum(0))
    assert np.array_equal(raw["sumsq"], (k64 ** 2).sum(0))
    assert np.array_equal(raw["hist"].astype(np.int64), _hist(p, kv, 16))
    assert 0 < a["state"][2].sum()
    for x, y in zip(a["state"] + a["kept"], b["state"] + b["kept"]):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
        else:
            assert x == y
    assert c["raw"]["n"] == 12
    for k in ("sum", "sumsq", "hist"):
        assert c["raw"][k].tobytes() == raw[k].tobytes(), k


def test_shards_merge_exactly(monkeypatch):
    from mceik_amd import mcmc
    _dev()
    monkeypatch.setenv("MCEIK_PERSIST", "0")
    p = _problem("P", nburn=0, keepk=2)

    def run(nchains, off):
        smp = mcmc.Sampler(p, nchains=nchains, chain_offset=off)
        smp.posterior_enable(per_chain=True, nbins=16)
        smp.run(20)
        parts = smp.posterior_partials()
        smp.close()
        return parts

    whole, a, b = run(12, 0), run(5, 0), run(7, 5)
    assert whole.nkept == 10 and a.nchains == 5 and b.nchains == 7
    a.merge(b)
    assert a.nchains == 12 and a.nkept == 10
    for k in ("S", "Q", "P", "hist"):
        assert getattr(a, k).tobytes() == getattr(whole, k).tobytes(), k
    assert whole.S.any() and whole.hist.sum() == 12 * 10 * p.ncell
    sa, sw = mcmc.PosteriorSummary(a), mcmc.PosteriorSummary(whole)
    for k in ("mean", "var", "rhat", "hist"):
        assert getattr(sa, k).tobytes() == getattr(sw, k).tobytes(), k
    assert np.isfinite(sw.mean).all()


def test_checkpoint_carries_the_posterior(monkeypatch):
    from mceik_amd import mcmc
    _dev()
    monkeypatch.setenv("MCEIK_PERSIST", "0")
    p = _problem("P", nburn=2, keepk=3)
    s1 = mcmc.Sampler(p, nchains=6)
    s1.posterior_enable(per_chain=True, nbins=16)
    s1.run(24)
    want = s1.posterior_raw()
    s1.close()
    s2 = mcmc.Sampler(p, nchains=6)
    s2.posterior_enable(per_chain=True, nbins=16)
    s2.run(12)
    ck = s2.checkpoint()
    s2.close()
    assert 0 < ck["posterior"]["n"] < want["n"]
    s3 = mcmc.Sampler(p, nchains=6)
    s3.posterior_enable(per_chain=True, nbins=16)
    s3.restore(ck)
    s3.run(12)
    got = s3.posterior_raw()
    s3.close()
    assert got["n"] == want["n"] == 8
    for k in ("sum", "sumsq", "hist"):
        assert got[k].tobytes() == want[k].tobytes(), k
    # a sampler without the posterior ignores the entry; a checkpoint without it is as before
    s4 = mcmc.Sampler(p, nchains=6)
    s4.restore(ck)
    assert "posterior" not in s4.checkpoint()
    s4.close()


def test_errors():
    from mceik_amd import mcmc
    _dev()
    p = _problem("P")
    smp = mcmc.Sampler(p, nchains=3)
    with pytest.raises(RuntimeError):
        smp.posterior_raw()
    with pytest.raises(RuntimeError):
        smp.posterior_accumulate()
    with pytest.raises(ValueError):
        smp.posterior_enable(nbins=129)
    with pytest.raises(RuntimeError):
        smp.posterior_raw()
    smp.posterior_enable(nbins=4)
    smp.posterior_accumulate()
    assert smp.posterior_raw()["n"] == 1 and smp.posterior_raw()["sum"].any()
    smp.posterior_enable(nbins=4)
    raw = smp.posterior_raw()
    assert raw["n"] == 0 and not raw["sum"].any() and not raw["hist"].any()
    smp.posterior_disable()
    with pytest.raises(RuntimeError):
        smp.posterior_raw()
    smp.close()
