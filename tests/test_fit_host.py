"""Host side of the streaming data-fit sums (include/mceik.h mceik_fit_*): the
ABI of the two structs, check / merge / finish on synthetic integer partials
against Python integers and plain numpy, and the restatement tests/_fit.py
against mcmc._pick_terms on a hand-made event.  No GPU call."""
import numpy as np
import pytest

import _fit
from test_posterior_host import _offsets_c

MASK = (1 << 64) - 1


@pytest.mark.parametrize("ctype,pyname", [("mceik_fit_opts", "FitOpts"), ("mceik_fit_partials", "FitPartials")])
def test_ctypes_mirrors_match_header(ctype, pyname):
    import ctypes as C
    from mceik_amd import _lib
    cls = getattr(_lib, pyname)
    names = [f[0] for f in cls._fields_]
    c = _offsets_c(ctype, names)
    assert C.sizeof(cls) == c["sizeof"]
    for n in names:
        assert getattr(cls, n).offset == c[n], n


def test_fit_check():
    from mceik_amd import mcmc
    t = 2.0 ** -20
    assert mcmc.fit_check(t, 0.0) and mcmc.fit_check(t, 2047.0) and mcmc.fit_check(t, (2 ** 31 - 1) * t)
    assert not mcmc.fit_check(t, 2048.0) and not mcmc.fit_check(t, 1e9)
    assert mcmc.fit_check(2.0 ** -34, 0.124) and not mcmc.fit_check(2.0 ** -34, 0.126)      # 2^31 2^-34 = 0.125
    assert mcmc.fit_check(1.0, 2e9) and mcmc.fit_check(2.0 ** -64, 1e-10) and mcmc.fit_check(2.0 ** 64, 1e20)
    for bad in (1e-6, 3.0 * t, 0.0, -t, float("inf"), float("nan"), 2.0 ** -65, 2.0 ** 65):
        assert not mcmc.fit_check(bad, 1.0), bad
    assert not mcmc.fit_check(t, -1.0) and not mcmc.fit_check(t, float("nan"))


# --- a small catalogue: 3 events, 2 phases, 3 stations, one masked pick, one event with a single used pick ---
NEV, NPH, NST, NB = 3, 2, 3, 8
PTR = np.array([0, 4, 7, 9], np.int32)
STAT = np.array([0, 1, 2, 0, 1, 2, 0, 1, 1], np.int32)
PHASE = np.array([0, 0, 0, 1, 0, 1, 0, 0, 1], np.int32)
OMASK = np.array([0, 0, 0, 0, 0, 0, 0, 1, 0], np.int32)        # event 2: pick 7 masked, pick 8 alone
T0REF = np.array([10.0, -3.5, 1e9])


def _parts(nchains, nkept, tick=2.0 ** -20, zmax=4.0):
    from mceik_amd import mcmc
    p = mcmc.FitPartials(len(STAT), NEV, NPH, NST, NB, tick, zmax, nchains=nchains, nkept=nkept)
    p.obs_ptr[:], p.obs_stat[:], p.obs_phase[:], p.obs_mask[:], p.t0_ref[:] = PTR, STAT, PHASE, OMASK, T0REF
    return p


def _fill(p, f):
    """The Python integers of a _fit.Fit-like namespace into the partials' words."""
    raw = f if isinstance(f, dict) else f.raw()
    for k in _fit.ARRAYS:
        getattr(p, k)[...] = raw[k]
    return p


def _values(rng, M, n, qscale, used=None):
    """q, zq [n, M, nobs] and tq [n, M, nev] integers; masked picks 0."""
    used = (OMASK == 0) if used is None else used
    q = rng.integers(-qscale, qscale + 1, (n, M, len(STAT))) * used
    zq = rng.integers(-5000, 5001, (n, M, len(STAT))) * used
    tq = rng.integers(-qscale, qscale + 1, (n, M, NEV))
    return q.astype(object), zq.astype(object), tq.astype(object)


def _sums(q, zq, tq, rng=None):
    """The words of _fit.Fit.raw() from integer arrays (Python integers: no overflow)."""
    s64 = lambda xs: np.array([int(x) & MASK for x in xs], np.uint64).view(np.int64)
    w = lambda xs: np.array([_fit.words128(x) for x in xs], np.uint64).reshape(len(xs), 2)
    hist = np.zeros((NPH, NST, NB), np.int64)
    if rng is not None:
        hist[...] = rng.integers(0, 50, hist.shape)
    tot = lambda x: x.reshape(-1, x.shape[-1]).sum(0)            # (object arrays reduce one axis at a time)
    return {"sq": s64(tot(q)), "szq": s64(tot(zq)), "sq2": w(tot(q ** 2)), "szq2": w(tot(zq ** 2)),
            "stq": s64(tot(tq)), "stq2": w(tot(tq ** 2)),
            "hist": hist, "sat": np.array([1, 2, 3], np.int64), "n": q.shape[0]}


def test_merge_is_addition_with_carries():
    """Two shards of 3 and 4 chains at |q| near 2^31: every sum of squares crosses 2^64, and the low words of the
    two shards add past 2^64 (a carry out of the lo word in the merge itself)."""
    rng = np.random.default_rng(5)
    n = 9
    q, zq, tq = _values(rng, 7, n, 2 ** 31 - 1)
    q[:, :, 0] = 2 ** 31 - 1                             # 63 (2^31 - 1)^2 = 2^67.9
    q[:, :, 1] = -(2 ** 31 - 1)
    whole = _sums(q, zq, tq, rng)
    a, b = _sums(q[:, :3], zq[:, :3], tq[:, :3]), _sums(q[:, 3:], zq[:, 3:], tq[:, 3:])
    b["hist"] = whole["hist"] - a["hist"]
    a["sat"], b["sat"] = np.array([1, 0, 2], np.int64), np.array([0, 2, 1], np.int64)
    lo = lambda x, j: int(x["sq2"][j, 0])
    assert any(lo(a, j) + lo(b, j) > MASK for j in range(len(STAT))), "no carry out of a lo word"
    assert whole["sq2"][OMASK == 0, 1].all() and int(whole["sq"][1]) < 0
    pa, pb = _fill(_parts(3, n), a), _fill(_parts(4, n), b)
    pa.merge(pb)
    assert (pa.nchains, pa.nkept) == (7, n)
    _fit.assert_raw_equal({**{k: getattr(pa, k) for k in _fit.ARRAYS}, "n": n}, whole, "merge")
    # partials of another run do not merge
    for kw, attr in ((dict(nkept=n + 1), None), (dict(tick=2.0 ** -19), None), (dict(zmax=5.0), None),
                     ({}, "obs_mask"), ({}, "t0_ref"), ({}, "obs_stat")):
        other = _fill(_parts(4, **{"nkept": n, **kw}), b)
        if attr:
            getattr(other, attr)[0] += 1
        with pytest.raises(ValueError):
            _fill(_parts(3, n), a).merge(other)


def _finish_by_numpy(q, zq, tq, tick):
    """Straightforward numpy on the integer values as float64."""
    n, M, nobs = q.shape
    N = n * M
    used = OMASK == 0
    r = q.astype(np.float64) * tick
    z = zq.astype(np.float64) / 1024.0
    t = tq.astype(np.float64) * tick
    nan = lambda a, ok: np.where(ok, a, np.nan)
    out = {"pick_mean": nan(r.mean((0, 1)), used), "pick_sd": nan(r.std((0, 1), ddof=1), used),
           "pick_zmean": nan(z.mean((0, 1)), used), "pick_zrms": nan(np.sqrt((z ** 2).mean((0, 1))), used)}
    nused = np.array([used[PTR[e]:PTR[e + 1]].sum() for e in range(NEV)])
    out["t0_mean"] = t.mean((0, 1)) + T0REF
    out["t0_sd"] = t.std((0, 1), ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["ev_misfit"] = np.array([np.where(nused[e] >= 2, (z[:, :, PTR[e]:PTR[e + 1]] ** 2).sum(2).mean() /
                                              (nused[e] - 1.0), np.nan) for e in range(NEV)])
    sm, sz, pz = np.full((NPH, NST), np.nan), np.full((NPH, NST), np.nan), np.full(NPH, np.nan)
    for ph in range(NPH):
        for k in range(NST):
            sel = used & (PHASE == ph) & (STAT == k)
            if sel.any():
                sm[ph, k] = r[:, :, sel].mean()
                sz[ph, k] = np.sqrt((z[:, :, sel] ** 2).mean())
        pz[ph] = np.sqrt((z[:, :, used & (PHASE == ph)] ** 2).mean())
    out.update({"sta_mean": sm, "sta_zrms": sz, "phase_zrms": pz})
    return out


@pytest.mark.parametrize("qscale,tick", [(3000, 2.0 ** -20), (2 ** 31 - 1, 2.0 ** -34)])
def test_finish_against_numpy(qscale, tick):
    """Both sides are a handful of fp64 operations on the same exact integers: 1e-12 relative.  (numpy's std
    subtracts the mean first, so its error is relative to the spread, not to the mean: the values are drawn
    about zero, where the two are of one size.)"""
    from mceik_amd import mcmc
    rng = np.random.default_rng(8)
    M, n = 5, 7
    q, zq, tq = _values(rng, M, n, qscale)
    parts = _fill(_parts(M, n, tick=tick), _sums(q, zq, tq, rng))
    got, want = parts.finish(), _finish_by_numpy(q, zq, tq, tick)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (k, got[k], want[k])
        ok = ~np.isnan(want[k])
        assert np.allclose(got[k][ok], want[k][ok], rtol=1e-12, atol=0.0), (k, got[k], want[k])
    # masked pick 7: NaN; event 2 has one used pick: an origin time, no reduced misfit; row (S, station 0): a pick
    assert np.isnan(got["pick_mean"][7]) and np.isnan(got["pick_sd"][7]) and np.isnan(got["pick_zrms"][7])
    assert np.isfinite(got["t0_mean"]).all() and np.isnan(got["ev_misfit"][2]) and np.isfinite(got["ev_misfit"][:2]).all()
    assert np.isnan(got["sta_mean"][1, 2]) == (not ((PHASE == 1) & (STAT == 2) & (OMASK == 0)).any())
    s = mcmc.FitSummary(parts)
    assert s.saturated == (1, 2, 3) and s.count == n and s.nchains == M and s.hist.shape == (NPH, NST, NB)
    assert s.bin_edges[0] == -4.0 and s.bin_edges[-1] == 4.0 and len(s.bin_edges) == NB + 1
    # fewer than two states: everything NaN
    one = _fill(_parts(M, 1, tick=tick), _sums(q[:1], zq[:1], tq[:1]))
    assert all(np.isnan(v).all() for v in one.finish().values())


def _hand_problem(tc, var=(0.5, 1.0, 1.0), luse=(1, 1, 1)):
    """One event, picks at stations 0, 1, 2 with weights 1 / var = (2, 1, 1): xnorm = 4, the shares 1/2, 1/4, 1/4
    are exact, so t0 and every residual of a dyadic tc are exact."""
    from mceik_amd import mcmc
    k = len(tc)
    return mcmc.Problem(nx=8, ny=8, nz=8, h=100.0, sx=np.zeros(3), sy=np.zeros(3), sz=np.zeros(3), pcorr=np.zeros(3),
                        ex=np.zeros(1), ey=np.zeros(1), ez=np.zeros(1), obs_ptr=np.array([0, k], np.int32),
                        obs_stat=np.arange(k, dtype=np.int32) % 3, pick_type=np.full(k, mcmc.P_PRIMARY_PICK, np.int32),
                        luse=np.array(luse, np.int32), tobs=np.array(tc, np.float64), var=np.array(var, np.float64))


def test_restatement_on_a_hand_made_event():
    from mceik_amd import mcmc
    tick = 2.0 ** -4
    tt = np.zeros((1, 3, 1), np.float32)
    p = _hand_problem([0.0, 0.0, 2 * tick])
    (js, w, xnorm, res, obj, t0), = mcmc._pick_terms(p, tt, None, None, with_t0=True)
    assert len(mcmc._pick_terms(p, tt, None, None)[0]) == 5               # the existing return values stay
    assert (js, w, xnorm, t0) == ([0, 1, 2], [2.0, 1.0, 1.0], 4.0, tick / 2)
    assert res == [-tick / 2, -tick / 2, 3 * tick / 2]                     # r / tick = -0.5, -0.5, 1.5: all half-way
    q, zq, b, tq, sat = _fit.state_words(p, tt, None, None, tick, 8, 4.0)
    assert q.tolist() == [0, 0, 2] and sat == [0, 0, 0]                    # round-half-even: -0.5 -> -0, 1.5 -> 2
    assert q.tolist() == [int(np.rint(r / tick)) for r in res]
    assert zq.tolist() == [-64, -32, 96]                                   # z = w r = -1/16, -1/32, 3/32
    assert tq.tolist() == [0]                                              # t0 / tick = 0.5 -> 0
    assert b.tolist() == [3, 3, 4]                                         # floor(z + 4)
    assert _fit.state_words(p, tt, None, None, tick, 8, 4.0, t0_ref=[-tick])[3].tolist() == [2]   # 1.5 -> 2
    # 2.5 -> 2 and -2.5 -> -2 (away from zero would give 3): residuals -5/2, -5/2, 15/2 ticks at tc = (0, 0, 10 tick)
    assert _fit.state_words(_hand_problem([0.0, 0.0, 10 * tick]), tt, None, None, tick, 8, 4.0)[0].tolist() == [-2, -2, 8]
    # saturation: r = -1/4, -1/4, 3/4 s at tick 2^-40 is +-2^38, 3 2^38 ticks
    q, zq, b, tq, sat = _fit.state_words(_hand_problem([0.0, 0.0, 1.0]), tt, None, None, 2.0 ** -40, 8, 4.0)
    assert q.tolist() == [-(2 ** 31 - 1)] * 2 + [2 ** 31 - 1] and sat == [3, 0, 1] and tq.tolist() == [2 ** 31 - 1]
    assert zq.tolist() == [-512, -256, 768]
    # z beyond +-zmax lands in the edge bins; a masked pick has no words
    p4 = _hand_problem([0.0, 0.0, 64.0, 5.0], var=(0.5, 1.0, 1.0, 1.0), luse=(1, 1, 1, 0))
    q, zq, b, tq, sat = _fit.state_words(p4, tt, None, None, tick, 8, 4.0)
    assert b.tolist() == [0, 0, 7, -1] and q[3] == 0 and zq[3] == 0
    f = _fit.Fit(p4, tick, 8, 4.0)
    f.add(tt)
    f.add(tt)
    f.counted()
    raw = f.raw()
    assert raw["hist"][0, :, :].sum() == 6 and raw["hist"][0, 2, 7] == 2 and raw["sq"][3] == 0 and raw["n"] == 1
    assert raw["sq2"][2].tolist() == [2 * int(q[2]) ** 2, 0]
