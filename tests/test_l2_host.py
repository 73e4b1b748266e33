"""The numpy restatement of the L2 grid searches (tests/_l2.py) pinned on the
CPU, before tests/test_gpu_l2.py holds the kernels against it: bit for bit the
compiled reference's golden vectors and the C oracle on every drop-in case of
the GPU sweep, within a derived rounding bound of a long-double evaluation of
the formulas, and the known answer of gridsearch.f90's own driver.  The sweep's
cases are defined here, once, for both files."""
import itertools
import os
import types

import numpy as np
import pytest

import _l2
import _oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (ngrd, ldgrd): around the 64-lane wave and the 256-thread block, ngrd < ldgrd included
SHAPES = [(1, 8), (63, 64), (64, 64), (65, 80), (255, 256), (256, 256), (257, 320)]
PICKS = (1, 2, 3, 4, 5, 12, 33)
MASKS = ("none", "ends", "one")                 # none; first and last masked; all but one masked
T0USE = 0.25


def ld_for(ldgrd, mult):
    """ldgrd under an entry point's alignment rule: a multiple of 8 (fp64 locate.c, 64 bytes), 16 (fp32 locate.c) or
    64 (gridsearch.f90, both precisions)."""
    return -(-ldgrd // mult) * mult


def mask_of(kind, nobs):
    m = np.zeros(nobs, np.int32)
    if kind == "ends":
        m[0] = m[nobs - 1] = 1                   # (1 or 2 picks: nothing is left)
    elif kind == "one":
        m[:] = 1
        m[nobs // 2] = 0
    elif kind == "two":                          # gridsearch.f90 only: the value 2 is not 1, hence used
        m[0], m[nobs - 1] = 1, 2
    return m


def case(ngrd, ldgrd, nobs, seed=0, dtype=np.float64, test_scale=1.0, var_scale=1.0):
    """Inputs of one grid search from default_rng([ngrd, ldgrd, nobs, seed]); test is 64-byte aligned."""
    g = np.random.default_rng([ngrd, ldgrd, nobs, seed])
    raw = np.zeros(nobs * ldgrd + 16, dtype)
    off = (-raw.ctypes.data % 64) // raw.itemsize
    test = raw[off:off + nobs * ldgrd]
    test[:] = g.uniform(0.2, 3.0, nobs * ldgrd) * test_scale
    tobs = (g.uniform(0.5, 3.5, nobs) * test_scale).astype(dtype)
    varobs = (g.uniform(0.01, 0.2, nobs) * var_scale).astype(dtype)
    tcorr = g.normal(0.0, 0.01, nobs).astype(dtype)
    return types.SimpleNamespace(ngrd=ngrd, ldgrd=ldgrd, nobs=nobs, test=test, tobs=tobs, varobs=varobs, tcorr=tcorr,
                                 dtype=dtype)


def sweep(ngrd, ldgrd, dtype, mult, masks=MASKS):
    """Every (case, mask, iwantOT) of one shape of the drop-in sweep."""
    for nobs in PICKS:
        c = case(ngrd, ld_for(ldgrd, mult), nobs, dtype=dtype)
        for kind, iwantOT in itertools.product(masks, (1, 0)):
            yield c, mask_of(kind, nobs), iwantOT


# fp32 edges.  3 picks: gridsearch.f90's var_i * sum(var) stays below FLT_MAX.
def subnormal_case(ld=80):
    """Variances near 1e19, residuals of order 1: (sqrt(1/2) / var * residual)^2 ~ 1e-39 < FLT_MIN."""
    return case(65, ld, 3, seed=19, dtype=np.float32, var_scale=5.0e19)


def overflow_case(ld=80):
    """Tables and picks near 1e20: the squared residuals pass FLT_MAX."""
    return case(65, ld, 3, seed=20, dtype=np.float32, test_scale=1.0e20)


def edge_events(c):
    """The edge case as a relocation batch: its three picks, and a second event that repeats a row."""
    return [dict(rows=[0, 1, 2], tobs=c.tobs, varobs=c.varobs),
            dict(rows=[2, 2, 0, 1], tobs=c.tobs[[1, 2, 0, 0]], varobs=c.varobs[[0, 1, 2, 1]], mask=[0, 0, 1, 0])]


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want, what=""):
    """Bit for bit; where the reference is NaN, NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions")
    bad = np.flatnonzero((_u(got) != _u(want)).ravel() & ~nan.ravel())
    assert bad.size == 0, (what, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


# ---------------------------------------------------------------------------
# golden vectors of the compiled reference

@pytest.mark.parametrize("name,dtype", [("locate_l2", np.float64), ("locate_l2_f32", np.float32)])
def test_gridsearch_equals_the_compiled_locate_c(name, dtype):
    g = dict(np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False))
    ld, ng, no = int(g["ldgrd"]), int(g["ngrd"]), int(g["nobs"])
    assert g["test"].dtype == dtype
    t0, obj = _l2.gridsearch(ld, ng, 1, 0.0, g["mask"], g["tobs"], g["tcorr"], g["varobs"], g["test"], dtype)
    same(t0, g["ot_t0"], "t0")
    same(obj, g["ot_objfn"], "objfn")
    t0, obj = _l2.gridsearch(ld, ng, 0, 4.0, np.zeros(no, np.int32), g["tobs"], None, g["varobs"], g["test"], dtype)
    same(t0, g["fixed_t0"], "fixed t0")
    same(obj, g["fixed_objfn"], "fixed objfn")


@pytest.mark.parametrize("prec,dtype", [(64, np.float64), (32, np.float32)])
def test_gridsearch_f90_equals_the_compiled_gridsearch_f90(prec, dtype):
    g = dict(np.load(os.path.join(GOLD, "gridsearch_f90.npz"), allow_pickle=False))
    ld, ng = int(g["ldgrd"]), int(g["ngrd"])
    assert 2 in g["mask"] and 1 in g["mask"]
    for iw in (1, 0):
        lp, _ = _l2.gridsearch_f90(ld, ng, iw, g["mask"], g["tobs"], g["varobs"], g["test"], dtype)
        same(lp, g[f"logpdf{prec}_ot{iw}"], iw)


# ---------------------------------------------------------------------------
# the C oracle on the GPU sweep's cases

@pytest.mark.parametrize("ngrd,ldgrd", SHAPES)
def test_restatement_equals_the_oracle_on_the_sweep(ngrd, ldgrd):
    n = 0
    for dtype, mult, orc in ((np.float64, 8, O.locate_l2), (np.float32, 16, O.locate_l2_f32)):
        for c, mask, iwantOT in sweep(ngrd, ldgrd, dtype, mult):
            for tcorr in (c.tcorr, None):
                ierr, wt0, wobj = orc(c.ldgrd, ngrd, c.nobs, iwantOT, T0USE, mask, c.tobs, tcorr, c.varobs, c.test)
                t0, obj = _l2.gridsearch(c.ldgrd, ngrd, iwantOT, T0USE, mask, c.tobs, tcorr, c.varobs, c.test, dtype)
                what = (dtype.__name__, c.nobs, mask.tolist(), iwantOT, tcorr is None)
                assert ierr == 0
                same(t0, wt0, what)
                same(obj, wobj, what)
                if mask.all():                   # nothing used: today t0 = 0 or t0use, objfn = 0
                    assert not obj.any() and (t0 == (0.0 if iwantOT else dtype(T0USE))).all()
                n += 1
    for c, mask, iwantOT in sweep(ngrd, ldgrd, np.float64, 64, MASKS + ("two",)):
        if mask.sum() == c.nobs:                 # gridsearch.f90:415 refuses these (the oracle does not model ierr)
            continue
        _, _, wlp = O.gridsearch_f90(c.ldgrd, ngrd, c.nobs, iwantOT, mask, c.tobs, c.varobs, c.test)
        lp, _ = _l2.gridsearch_f90(c.ldgrd, ngrd, iwantOT, mask, c.tobs, c.varobs, c.test)
        same(lp, wlp, (c.nobs, mask.tolist(), iwantOT))
        n += 1
    assert n > 2 * len(PICKS) * len(MASKS) * 2 * 2


def test_restatement_equals_the_oracle_on_the_fp32_edges():
    for c in (subnormal_case(), overflow_case()):
        for iwantOT in (1, 0):
            ierr, wt0, wobj = O.locate_l2_f32(c.ldgrd, c.ngrd, c.nobs, iwantOT, T0USE, np.zeros(3), c.tobs, None, c.varobs,
                                              c.test)
            t0, obj = _l2.gridsearch(c.ldgrd, c.ngrd, iwantOT, T0USE, np.zeros(3), c.tobs, None, c.varobs, c.test,
                                     np.float32)
            same(t0, wt0)
            same(obj, wobj)
            ev = edge_events(c)
            out, rt0 = _l2.relocate(c.test.reshape(3, c.ldgrd), ev, c.ngrd, iwantOT, T0USE, log_pdf=False)
            same(out[0], wobj, "relocate")
            same(rt0[0], wt0, "relocate")


# ---------------------------------------------------------------------------
# a long-double evaluation of the formulas

def _gamma(k, dtype):
    u = np.longdouble(np.finfo(dtype).eps) / 2
    return k * u / (1 - k * u)


def _check_against_longdouble(w0, w1, tc, rows, t0, obj, dtype, iwantOT, what):
    """t0 = sum_j w0_j (tc_j - te_j) and obj = 1/2 sum_j (w1_j (tc_j - (te_j + t0)))^2 in long double from the exact
    weights w0, w1 (long double) and the inputs tc, te (dtype), against the restatement's t0, obj (dtype)."""
    L = np.longdouble
    n = len(tc)
    rows = [r.astype(L) for r in rows]
    if iwantOT == 1:
        terms = [w0[j] * (L(tc[j]) - rows[j]) for j in range(n)]
        exact = sum(terms, np.zeros_like(t0, L))
        bound = _gamma(3 * n + 5, dtype) * sum((np.abs(t) for t in terms), np.zeros_like(t0, L))
        err = np.abs(t0.astype(L) - exact)
        assert (err <= bound).all(), (what, "t0", float((err - bound).max()))
    t = t0.astype(L)                             # the origin time as computed: an input of the second formula
    exact = sum(((w1[j] * (L(tc[j]) - (rows[j] + t))) ** 2 for j in range(n)), np.zeros_like(t, L)) / 2
    a2 = sum(((w1[j] * (abs(L(tc[j])) + np.abs(rows[j] + t))) ** 2 for j in range(n)), np.zeros_like(t, L)) / 2
    err = np.abs(obj.astype(L) - exact)
    bound = _gamma(n + 16, dtype) * a2
    assert (err <= bound).all(), (what, "objfn", float((err - bound).max()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_within_the_rounding_bound_of_a_long_double_evaluation(dtype):
    """The restatement against the same formulas in np.longdouble (u_ld = 2^-64 on x86-64), so that restatement,
    oracle and kernel cannot share one wrong formula.  u = eps/2 of dtype, gamma_k = k u / (1 - k u), <k> a product
    of k factors (1 + d)^(+-1), |d| <= u, |<k> - 1| <= gamma_k (Higham, Accuracy and Stability, 3.1, 3.4), n used picks.

    Origin time, t0 = sum_j w0_j (tc_j - te_j), tc_j as computed (tobs - tcorr is one operation, the same on both
    sides).  locate.c: w0_j = (1/var_j) / X, X = sum 1/var.  Computed 1/var_j = (1/var_j)<1>; X by n - 1 additions
    of positive terms, Xc = X (1 + h), |h| <= gamma_n, so 1/Xc = (1/X)(1 + h'), |h'| <= gamma_n / (1 - gamma_n) <=
    gamma_2n; the division <1>; the subtraction <1>; the product <1>; the term then passes through at most n
    additions <n>.  k = 1 + 2n + 1 + 1 + 1 + n = 3n + 4.  gridsearch.f90: w0_i = 1 / (var_i X), X = sum var: 2n for
    X as above, the product <1>, the division <1>, then as before: 3n + 4 again.  One more for the long double's own
    rounding (3n + 4 operations at 2^-64 are below one at 2^-53): k = 3n + 5, and
        |t0 - exact| <= gamma_(3n+5) sum_j |w0_j (tc_j - te_j)|.

    Objective at the computed t0 (taken as an input): half the weighted squared residuals, obj = 1/2 sum_j r_j^2,
    r_j = w1_j (tc_j - (te_j + t0)), w1_j = 1/var_j; the code folds the half into the weight as sqrt(1/2).  Its
    weight carries 4 roundings (1/var; the constant, within one ulp = 2u of sqrt(1/2) -- locate.c's literal is not
    the nearest double; the product; f90: sqrt, 1/sqrt, /var = 3), te_j + t0 one, relative to |te_j + t0|, the
    subtraction and the product one each: with a_j = w1_j (|tc_j| + |te_j + t0|) >= |r_j| the computed
    sqrt(1/2) r_j is sqrt(1/2) (r_j + e_j), |e_j| <= gamma_7 a_j.  The square differs from r_j^2 / 2 by at most
    (2 |r_j| |e_j| + e_j^2) / 2 <= (2 gamma_7 + gamma_7^2) a_j^2 / 2 <= gamma_15 a_j^2 / 2; the squaring rounds once
    and the n additions n times:
        |obj - exact| <= gamma_(n+16) 1/2 sum_j a_j^2.
    Small cases only: the first four shapes of the sweep."""
    L = np.longdouble
    mult = 8 if dtype == np.float64 else 16
    cases = [(c, m, iw) for ngrd, ldgrd in SHAPES[:4] for c, m, iw in sweep(ngrd, ldgrd, dtype, mult) if not m.all()]
    for c, mask, iwantOT in cases:
        use = np.flatnonzero(mask == 0)
        n = len(use)
        rows = [c.test.reshape(c.nobs, c.ldgrd)[j, :c.ngrd] for j in use]
        t0, obj = _l2.gridsearch(c.ldgrd, c.ngrd, iwantOT, T0USE, mask, c.tobs, c.tcorr, c.varobs, c.test, dtype)
        tc = [dtype(c.tobs[j] - c.tcorr[j]) for j in use]
        X = sum(1 / L(c.varobs[j]) for j in use)
        w0 = [1 / L(c.varobs[j]) / X for j in use]
        w1 = [1 / L(c.varobs[j]) for j in use]
        _check_against_longdouble(w0, w1, tc, rows, t0, obj, dtype, iwantOT, (c.ngrd, n, iwantOT))
    for c, mask, iwantOT in ((c, m, iw) for ngrd, ldgrd in SHAPES[:4]
                             for c, m, iw in sweep(ngrd, ldgrd, dtype, 64, MASKS + ("two",)) if m.sum() != c.nobs):
        use = np.flatnonzero(mask != 1)
        n = len(use)
        rows = [c.test.reshape(c.nobs, c.ldgrd)[j, :c.ngrd] for j in use]
        lp, t0 = _l2.gridsearch_f90(c.ldgrd, c.ngrd, iwantOT, mask, c.tobs, c.varobs, c.test, dtype)
        X = sum(L(c.varobs[j]) for j in use)
        w0 = [1 / (L(c.varobs[j]) * X) for j in use]
        w1 = [1 / L(c.varobs[j]) for j in use]
        _check_against_longdouble(w0, w1, [c.tobs[j] for j in use], rows, t0, lp, dtype, iwantOT,
                                  ("f90", c.ngrd, n, iwantOT))


# ---------------------------------------------------------------------------
# known answer

def test_noise_free_picks_shifted_by_4_s_locate_the_true_node():
    """gridsearch.f90:38-116 on a smaller grid: straight-ray times at 5 km/s, picks = the true node's times + 4 s.
    The misfit is smallest at the true node and the origin time there is 4 s to rounding: locate.c's weights sum to
    1 whatever the variances; gridsearch.f90's 1 / (var_i sum var) do so for unit variances, as its driver sets."""
    nx, ny, nz, nobs, dx = 13, 11, 5, 8, 1.0e3
    isrc = (7, 4, 2)
    node = (isrc[2] * ny + isrc[1]) * nx + isrc[0]
    rng = np.random.default_rng(5)
    rec = rng.random((nobs, 3)) * (np.array([nx, ny, nz]) - 1) * dx
    ngrd = nx * ny * nz
    ldgrd = ld_for(ngrd, 64)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), k.ravel()], 1) * dx
    test = np.zeros((nobs, ldgrd))
    for o in range(nobs):
        test[o, :ngrd] = np.sqrt(((pts - rec[o]) ** 2).sum(1)) / 5.0e3
    tobs = test[:, node] + 4.0
    var = rng.uniform(0.01, 0.2, nobs)
    none = np.zeros(nobs, np.int32)
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-5)):
        t0, obj = _l2.gridsearch(ldgrd, ngrd, 1, 0.0, none, tobs, None, var, test.ravel(), dtype)
        assert int(np.argmin(obj)) == node and abs(float(t0[node]) - 4.0) < tol and obj[node] < tol
        lp, t0 = _l2.gridsearch_f90(ldgrd, ngrd, 1, none, tobs, np.ones(nobs), test.ravel(), dtype)
        assert int(np.argmin(lp)) == node and abs(float(t0[node]) - 4.0) < 10 * tol
    ev = [dict(rows=list(range(nobs)), tobs=tobs, varobs=var),
          dict(rows=list(range(nobs))[::-1], tobs=tobs[::-1] - 1.5, varobs=var[::-1])]
    out, t0 = _l2.relocate(test, ev, ngrd)
    for e, shift in enumerate((4.0, 2.5)):
        assert int(np.argmax(out[e])) == node and abs(float(t0[e, node]) - shift) < 1e-5


# ---------------------------------------------------------------------------
# the fp32 edge inputs do what they are for

def test_the_subnormal_inputs_give_subnormal_results():
    tiny = np.finfo(np.float32).tiny
    c = subnormal_case()
    for iwantOT in (1, 0):
        _, obj = _l2.gridsearch(c.ldgrd, c.ngrd, iwantOT, T0USE, np.zeros(3), c.tobs, None, c.varobs, c.test, np.float32)
        assert ((obj > 0) & (obj < tiny)).any() and np.isfinite(obj).all()
        out, _ = _l2.relocate(c.test.reshape(3, c.ldgrd), edge_events(c), c.ngrd, iwantOT, T0USE)
        assert ((out < 0) & (out > -tiny)).any()
    f = subnormal_case(128)
    for iwantOT in (1, 0):
        lp, _ = _l2.gridsearch_f90(f.ldgrd, f.ngrd, iwantOT, np.zeros(3), f.tobs, f.varobs, f.test, np.float32)
        assert ((lp > 0) & (lp < tiny)).any() and np.isfinite(lp).all()


def test_the_overflow_inputs_give_inf():
    c = overflow_case()
    for iwantOT in (1, 0):
        t0, obj = _l2.gridsearch(c.ldgrd, c.ngrd, iwantOT, T0USE, np.zeros(3), c.tobs, None, c.varobs, c.test, np.float32)
        assert np.isposinf(obj).any() and np.isfinite(t0).all() and not np.isnan(obj).any()
        out, _ = _l2.relocate(c.test.reshape(3, c.ldgrd), edge_events(c), c.ngrd, iwantOT, T0USE)
        assert np.isneginf(out).any()
    f = overflow_case(128)
    for iwantOT in (1, 0):
        lp, _ = _l2.gridsearch_f90(f.ldgrd, f.ngrd, iwantOT, np.zeros(3), f.tobs, f.varobs, f.test, np.float32)
        assert np.isposinf(lp).any()
