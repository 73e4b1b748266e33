"""The L1 likelihood's host side (csrc/l1.h; no GPU):
weightedMedian__double -- the symbol the reference declares (locate.c:73) and
never defines -- mcmc.weighted_median / l1_event / logl_picks(norm=1), against
the textbook example, exact rational arithmetic and the restatement
tests/_l1.py, bit for bit."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import _l1


def _wmed(x, w, perm=None):
    """weightedMedian__double through ctypes: (median, perm, lsort, ierr)."""
    from mceik_amd import _lib
    L = _lib.lib()
    x = None if x is None else np.ascontiguousarray(x, np.float64)
    w = None if w is None else np.ascontiguousarray(w, np.float64)
    n = 0 if x is None else len(x)
    pm = np.arange(n, dtype=np.int32) if perm is None else np.ascontiguousarray(perm, np.int32).copy()
    lsort, ierr = C.c_bool(False), C.c_int(-1)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    t = L.weightedMedian__double(n, ptr(x), ptr(w), ptr(pm), C.byref(lsort), C.byref(ierr))
    return t, pm, bool(lsort.value), ierr.value


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_textbook_example():
    """locate.c:226-237, the reference's own (unlinkable) check: values = weights give 0.2, unit weights 0.1."""
    from mceik_amd import mcmc
    xs = [0.1, 0.35, 0.05, 0.1, 0.15, 0.05, 0.2]
    for w, want in ((xs, 0.2), ([1.0] * 7, 0.1)):
        t, pm, lsort, ierr = _wmed(xs, w)
        assert (t, ierr) == (want, 0)
        assert pm.tolist() == [2, 5, 0, 3, 4, 6, 1] and lsort
        assert mcmc.weighted_median(xs, w) == want
        assert float(_l1.median(xs, w)) == want
        assert mcmc.l1_event(xs, w)[0] == want


def _exact_minimisers(x, w, mask):
    """Exact rational arithmetic: the objective sum w |x - t| at every used t = x_k."""
    js = [j for j in range(len(x)) if not mask[j]]
    f = {k: sum(Fraction(w[j]) * abs(Fraction(x[j]) - Fraction(x[k])) for j in js) for k in js}
    return js, f


EXACT = {
    "n1": ([3.0], [2.0], [0]),
    "n2": ([5.0, -1.0], [1.0, 1.0], [0, 0]),
    "n2_heavy_upper": ([5.0, -1.0], [3.0, 1.0], [0, 0]),
    "even_equal_weights": ([4.0, 1.0, 3.0, 2.0], [1.0] * 4, [0] * 4),
    "even_equal_weights_6": ([6.0, 1.0, 5.0, 2.0, 4.0, 3.0], [0.5] * 6, [0] * 6),
    "all_equal": ([2.0] * 5, [1.0, 2.0, 3.0, 1.0, 1.0], [0] * 5),
    "duplicates": ([1.0, 3.0, 1.0, 3.0, 2.0, 3.0], [1.0, 1.0, 2.0, 1.0, 1.0, 2.0], [0] * 6),
    "signed_zeros": ([0.0, -0.0, 1.0, -1.0, -0.0], [1.0] * 5, [0] * 5),
    "negative_zero_first": ([-0.0, 0.0], [1.0, 1.0], [0, 0]),
    "more_than_half": ([1.0, 9.0, 2.0, 3.0], [1.0, 8.0, 1.0, 1.0], [0] * 4),
    "exactly_half": ([1.0, 9.0, 2.0, 3.0], [1.0, 3.0, 1.0, 1.0], [0] * 4),
    "masked": ([7.0, 1.0, 100.0, 3.0, 2.0, -50.0], [1.0, 1.0, 9.0, 1.0, 1.0, 9.0], [0, 0, 1, 0, 0, 1]),
    "masked_first_and_last": ([9.0, 1.0, 2.0, 9.0], [5.0, 1.0, 1.0, 5.0], [1, 0, 0, 1]),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_median_minimises_exactly(name):
    """t0 is one of the x_k, it minimises sum w |x - t| over them, and it is the lower one of the minimisers."""
    from mceik_amd import mcmc
    x, w, mask = EXACT[name]
    js, f = _exact_minimisers(x, w, mask)
    fmin = min(f.values())
    lowest = min(Fraction(x[k]) for k in js if f[k] == fmin)
    t0, obj = mcmc.l1_event(x, w, mask)
    assert any(_bits(t0) == _bits(x[k]) for k in js), "t0 is not one of the residuals"
    assert Fraction(t0) == lowest and Fraction(obj) == fmin
    # among equal values (signed zeros) the bits are those of the first k in catalogue order whose s_k reaches half
    half = sum(Fraction(w[j]) for j in js) / 2
    s = lambda k: sum(Fraction(w[j]) for j in js if x[j] < x[k] or (x[j] == x[k] and j <= k))
    first = min(k for k in js if Fraction(x[k]) == lowest and s(k) >= half)
    assert _bits(t0) == _bits(x[first])
    r0, robj = _l1.event(x, w, mask)
    assert _bits(t0) == _bits(r0) and _bits(obj) == _bits(robj)
    if not any(mask):
        t, _, _, ierr = _wmed(x, w)
        assert ierr == 0 and _bits(t) == _bits(t0)
        assert _bits(mcmc.weighted_median(x, w)) == _bits(t0)


def test_nothing_used_and_argument_errors():
    from mceik_amd import mcmc
    assert mcmc.l1_event([], []) == (0.0, 0.0)
    assert mcmc.l1_event([1.0, 2.0], [1.0, 1.0], [1, 1]) == (0.0, 0.0)
    assert _l1.event(np.zeros(0), np.zeros(0)) == (0.0, 0.0)
    t, _, _, ierr = _wmed(None, None)
    assert (t, ierr) == (0.0, 1)
    x = np.ones(3)
    from mceik_amd import _lib
    L = _lib.lib()
    for n, xp, wp in ((0, x, x), (-1, x, x), (3, None, x), (3, x, None)):
        ierr = C.c_int(-1)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        assert L.weightedMedian__double(n, p(xp), p(wp), None, None, C.byref(ierr)) == 0.0 and ierr.value == 1
    with pytest.raises(ValueError):
        mcmc.weighted_median([], [])
    with pytest.raises(ValueError):
        mcmc.weighted_median([1.0], [1.0, 2.0])
    with pytest.raises(ValueError):
        mcmc.l1_event([1.0], [1.0], [0, 0])


def test_library_equals_restatement_on_random_inputs():
    from mceik_amd import mcmc
    g = np.random.default_rng(23)
    for trial in range(200):
        n = int(g.integers(1, 40))
        x = g.normal(0.0, 1.0, n)
        if trial % 3 == 0:                             # ties
            x = np.round(x * 2.0) / 2.0
        w = g.uniform(0.05, 4.0, n) if trial % 4 else np.full(n, 0.1)
        mask = (g.random(n) < 0.2).astype(np.int32) if trial % 2 else np.zeros(n, np.int32)
        t0, obj = mcmc.l1_event(x, w, mask)
        r0, robj = _l1.event(x, w, mask)
        assert _bits(t0) == _bits(r0) and _bits(obj) == _bits(robj), trial
        start = g.permutation(n).astype(np.int32) if trial % 5 else _l1.perm(x)
        t, pm, lsort, ierr = _wmed(x, w, start)
        assert ierr == 0 and _bits(t) == _bits(_l1.median(x, w)), trial
        assert np.array_equal(pm, _l1.perm(x)) and lsort == (not np.array_equal(start, _l1.perm(x))), trial
        assert _bits(mcmc.weighted_median(x, w)) == _bits(t)


def test_one_gross_outlier_moves_l2_but_not_l1():
    """One pick late by 1000 var: the L2 origin time moves by w_j / sum w of it, the L1 origin time by no more
    than the gap to the neighbouring residual."""
    from mceik_amd import mcmc
    g = np.random.default_rng(5)
    n = 9
    x = g.normal(0.0, 0.02, n)
    var = np.full(n, 0.02)             # equal weights: the median moves by one neighbour at the most
    w = 1.0 / var
    t1 = mcmc.weighted_median(x, w)
    t2 = float((w * x).sum() / w.sum())
    for j in range(n):
        y = x.copy()
        y[j] += 1000.0 * var[j]
        u1 = mcmc.weighted_median(y, w)
        u2 = float((w * y).sum() / w.sum())
        assert abs((u2 - t2) - (w[j] / w.sum()) * 1000.0 * var[j]) < 1e-9
        assert u2 - t2 > 0.5
        above = np.sort(x[x > t1])
        gap = (above[0] - t1) if len(above) else 0.0
        assert 0.0 <= u1 - t1 <= gap, (j, u1 - t1, gap)
        assert any(_bits(u1) == _bits(v) for v in x), "the L1 origin time is still one of the clean residuals"


@pytest.mark.parametrize("phases", ["P", "PS"])
def test_logl_picks_norm1_against_restatement(phases):
    from mceik_amd import mcmc
    p = mcmc.make_problem("C2", n=16, nstat=4, nev=6, phases=phases)
    p.luse[[1, 7]] = 0
    p.luse[p.obs_ptr[3]:p.obs_ptr[4]] = 0              # an event without a used pick
    p.tobs[5] += 250.0 * p.var[5]                      # a gross outlier
    g = np.random.default_rng(11)
    nph = max(1, p.nphase)
    tt = (g.uniform(0.1, 2.0, (nph, p.nstat, p.nevents))).astype(np.float32)
    var = p.var * g.uniform(0.5, 2.0, len(p.var))
    tcorr = g.normal(0.0, 0.01, len(p.var))
    for v, tc in ((None, None), (var, tcorr)):
        got = mcmc.logl_picks(p, tt, v, tc, norm=1)
        assert _bits(got) == _bits(_l1.logl(p, tt, v, tc))
        terms = mcmc._pick_terms(p, tt, v, tc, with_t0=True, norm=1)
        want = _l1.pick_terms(p, tt, v, tc)
        assert len(terms) == len(want) == p.nevents
        for (js, w, wsum, res, obj, t0), (wjs, wt0, wobj, wres) in zip(terms, want):
            assert js == wjs and _bits(t0) == _bits(wt0) and _bits(obj) == _bits(wobj)
            assert np.array_equal(_bits(res), _bits(wres))
        assert terms[3][0] == [] and terms[3][4] == 0.0 and terms[3][5] == 0.0
    # the default norm is the L2 misfit, unchanged
    assert _bits(mcmc.logl_picks(p, tt)) == _bits(mcmc.logl_picks(p, tt, norm=2))
    assert _bits(mcmc.logl_picks(p, tt)) != _bits(mcmc.logl_picks(p, tt, norm=1))
    with pytest.raises(ValueError):
        mcmc.logl_picks(p, tt, norm=3)
