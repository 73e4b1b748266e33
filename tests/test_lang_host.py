"""Discrete Langevin moves, host side (no GPU): the deterministic exp
(mceik_det_exp), the per-cell proposal (mceik_lang_cell; the arithmetic the
kernels of csrc/lang.hip run) against the transcription in
tests/_lang.py, detailed balance of the whole move by enumeration, and the
refusals of the C-ABI."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import _lang as LG

# observed on the CPU, asserted at 4 x (DESIGN.md s.8c's convention; s.18's table)
OBS_DET_EXP_REL = 2.3e-16           # max |det_exp - exp| / exp over the two ranges below
OBS_BALANCE = 2.8e-17               # max |pi_a P_ab - pi_b P_ba| and |pi P - pi| over the two targets


def _lib():
    from mceik_amd import _lib
    return _lib.lib()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _points():
    rng = np.random.default_rng(18)
    return np.concatenate([rng.uniform(-40.0, 40.0, 200000), rng.uniform(-708.0, 0.0, 200000)])


def test_det_exp_is_the_transcription_bitwise():
    L = _lib()
    xs = _points()
    for x in np.concatenate([xs[:5000], xs[-5000:]]):
        assert _bits(L.mceik_det_exp(float(x))) == _bits(LG.det_exp(x)), x
    for x in (0.0, -0.0, 709.0, -708.0, 709.5, -708.5, 1e-300, 0.34657359027997264, -0.34657359027997264):
        assert _bits(L.mceik_det_exp(x)) == _bits(LG.det_exp(x)), x


def test_det_exp_accuracy_edges_and_monotonicity():
    L = _lib()
    worst = 0.0
    for x in _points():
        e = math.exp(x)
        worst = max(worst, abs(L.mceik_det_exp(float(x)) - e) / e)
    print(f"det_exp: max relative deviation from math.exp {worst:.3e}")
    assert worst <= 4 * OBS_DET_EXP_REL
    assert L.mceik_det_exp(0.0) == 1.0 and L.mceik_det_exp(-709.0) == 0.0 and L.mceik_det_exp(710.0) == math.inf
    assert math.isnan(L.mceik_det_exp(math.nan))
    grid = np.linspace(-708.0, 709.0, 28341)
    y = np.array([L.mceik_det_exp(float(x)) for x in grid])
    assert (np.diff(y) > 0.0).all()
    fine = np.linspace(-1.0, 1.0, 20001)                   # across the k = -1, 0, 1 joints
    y = np.array([L.mceik_det_exp(float(x)) for x in fine])
    assert (np.diff(y) >= 0.0).all()


def _cell(seed, g, gs, i, d, v, vlo, vhi, sigma, dmax):
    from mceik_amd import mcmc
    return mcmc.lang_cell(seed, g, gs, i, d, v, vlo, vhi, sigma, dmax)


def test_cell_normalised_clipped_and_symmetric():
    for d, v, sigma, dmax in ((0.3, 4000, 5.0, 12), (-2.0, 1500, 3.0, 8), (0.0, 9000, 10.0, 32), (4.0, 8997, 2.0, 6),
                              (-0.7, 1502, 6.0, 5), (50.0, 3000, 1.0, 4)):
        delta, lo, lq = _cell(3, 1, 7, 5, d, v, 1500, 9000, sigma, dmax)
        assert abs(sum(math.exp(x) for x in lq) - 1.0) <= 1e-14
        assert lo == max(-dmax, 1500 - v) and lo + len(lq) - 1 == min(dmax, 9000 - v)
        assert lo <= delta <= lo + len(lq) - 1
    # both box edges at once, and dmax alone
    _, lo, lq = _cell(3, 1, 7, 5, 0.1, 1502, 1500, 1505, 4.0, 8)
    assert lo == -2 and len(lq) == 6
    assert len(_cell(3, 1, 7, 5, 0.1, 4000, 1500, 9000, 4.0, 8)[2]) == 17
    # zero drift: q(delta) == q(-delta) bit for bit
    _, lo, lq = _cell(3, 1, 7, 5, 0.0, 4000, 1500, 9000, 5.0, 9)
    assert lo == -9 and np.array_equal(_bits(lq), _bits(lq[::-1]))


def test_cell_is_the_transcription_bitwise():
    rng = np.random.default_rng(5)
    for k in range(400):
        d = float(rng.normal() * (0.05 if k % 2 else 3.0))
        v = int(rng.integers(1500, 9001)) if k % 5 else int(rng.choice([1500, 1501, 8999, 9000]))
        sigma, dmax = float(rng.uniform(0.5, 12.0)), int(rng.integers(1, 33))
        a = LG.cell(11, k % 7, 1000 * k, 3 * k, d, v, 1500, 9000, sigma, dmax)
        b = _cell(11, k % 7, 1000 * k, 3 * k, d, v, 1500, 9000, sigma, dmax)
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(_bits(a[2]), _bits(b[2])), k
    # a step counter above 2^32 reaches the second counter word
    draws = {gs: _cell(11, 2, gs, 4, 0.2, 4000, 1500, 9000, 4.0, 8)[0] for gs in [(k << 32) + 9 for k in range(12)]}
    assert all(LG.cell(11, 2, gs, 4, 0.2, 4000, 1500, 9000, 4.0, 8)[0] == dl for gs, dl in draws.items())
    assert len(set(draws.values())) > 1


def test_cell_frequencies_follow_q():
    L = _lib()
    N, d, v, sigma, dmax = 200000, 0.4, 1503, 3.0, 6
    _, lo, lq = _cell(2016, 0, 0, 0, d, v, 1500, 9000, sigma, dmax)
    q = np.exp(lq)
    cnt = np.zeros(len(q), np.int64)
    dl = C.c_int(0)
    for gs in range(N):
        assert L.mceik_lang_cell(2016, 0, gs, 0, d, v, 1500, 9000, sigma, dmax, C.byref(dl), None, None, None) == 0
        cnt[dl.value - lo] += 1
    f = cnt / N
    assert lo == -3 and len(q) == 10
    assert (np.abs(f - q) <= 5.0 * np.sqrt(q * (1.0 - q) / N)).all(), (f, q)


def _kernel(logpi, grad, sigma, dmax, lo=1500, nv=5, fold=None):
    """The 25 x 25 transition matrix of one Langevin move on 2 cells x nv
    velocities: the library's exact q (mceik_lang_cell's logq with drift
    grad(v)) and min(1, ratio) with ratio as the sampler forms it."""
    states = list(itertools.product(range(lo, lo + nv), repeat=2))
    n = len(states)
    lq = {}
    for s in states:
        d = grad(s)
        lq[s] = [_cell(1, 0, 0, i, d[i], s[i], lo, lo + nv - 1, sigma, dmax) for i in range(2)]

    def logq(a, b):
        t = 0.0
        for i in range(2):
            _, l0, q = lq[a][i]
            t = t + float(q[b[i] - a[i] - l0])
        return t

    P = np.zeros((n, n))
    for ia, a in enumerate(states):
        for ib, b in enumerate(states):
            if ia == ib:
                continue
            lqf, lqr = logq(a, b), logq(b, a)
            dlp = 0.0 if fold is None else fold(b) - fold(a)
            P[ia, ib] = math.exp(lqf) * min(1.0, math.exp((logpi(b) - logpi(a)) + dlp + (lqr - lqf)))
        P[ia, ia] = 1.0 - P[ia].sum()
    pi = np.array([math.exp(logpi(s) + (0.0 if fold is None else fold(s))) for s in states])
    return pi / pi.sum(), P


def test_detailed_balance_by_enumeration():
    c = (1502.3, 1500.8)

    def logl(s):
        return -0.35 * (s[0] - c[0]) ** 2 - 0.2 * (s[1] - c[1]) ** 2 + 0.15 * (s[0] - c[0]) * (s[1] - c[1])

    def glogl(s):
        return (-0.7 * (s[0] - c[0]) + 0.15 * (s[1] - c[1]), -0.4 * (s[1] - c[1]) + 0.15 * (s[0] - c[0]))

    # a prior-like integer term: -(ws (v0 - v1)^2 + wd ((v0 - r0)^2 + (v1 - r1)^2)), its gradient in the drift
    ws, wd, r = 0.125, 0.0625, (1501, 1503)

    def lprior(s):
        return -(ws * float((s[0] - s[1]) ** 2) + wd * float((s[0] - r[0]) ** 2 + (s[1] - r[1]) ** 2))

    def gpost(s):
        g = glogl(s)
        return (g[0] + -(ws * float(2 * (s[0] - s[1])) + wd * float(2 * (s[0] - r[0]))),
                g[1] + -(ws * float(2 * (s[1] - s[0])) + wd * float(2 * (s[1] - r[1]))))

    worst = 0.0
    for grad, fold in ((glogl, None), (gpost, lprior)):
        pi, P = _kernel(logl, grad, 1.5, 4, fold=fold)
        assert (P >= 0.0).all() and np.abs(P.sum(1) - 1.0).max() <= 1e-15
        F = pi[:, None] * P
        worst = max(worst, np.abs(F - F.T).max(), np.abs(pi @ P - pi).max())
    print(f"detailed balance: max residual {worst:.3e}")
    assert worst <= 4 * OBS_BALANCE


def test_failed_step_is_a_rejection_in_the_restatement():
    from mceik_amd import mcmc
    import _oracle as O
    p = mcmc.make_problem("C2", n=16, nstat=2, nev=3)
    p.var[:] = 2e-3
    v0 = mcmc.initial_models(p, range(1))[0]
    P = O.make_problem(p)
    l0 = O.loglik(P, O.forward_all_f32(P, v0))
    ok = LG.step(p, 0, 0, v0, l0, 4.0, 8)
    bad = LG.step(p, 0, 0, v0, l0, 4.0, 8, failed=True)
    assert bad["accept"] == 0 and bad["status"] == 1 and np.array_equal(bad["v"].ravel(), v0) and bad["logl"] == l0
    assert np.array_equal(bad["delta"], ok["delta"]) and bad["lqf"] == ok["lqf"] and bad["lqr"] == ok["lqr"]
    assert (ok["delta"] != 0).any() and ok["status"] == 0


def test_abi_refusals_without_a_sampler():
    from mceik_amd import _lib, mcmc
    L = _lib.lib()
    good = _lib.LangOpts(2, 0, 4.0, 8, 0)
    assert L.mceik_mcmc_lang_enable(None, C.byref(good)) == 1
    assert L.mceik_mcmc_lang_enable(None, None) == 1
    for every, offset, sigma, dmax, mem in ((0, 0, 4.0, 8, 0), (-1, 0, 4.0, 8, 0), (2, 2, 4.0, 8, 0), (2, -1, 4.0, 8, 0),
                                           (2, 0, 0.0, 8, 0), (2, 0, -1.0, 8, 0), (2, 0, math.nan, 8, 0), (2, 0, 4.0, 0, 0),
                                           (2, 0, 4.0, _lib.LANG_DMAX_CAP + 1, 0), (2, 0, 4.0, 8, 1)):
        o = _lib.LangOpts(every, offset, sigma, dmax, mem)
        assert L.mceik_mcmc_lang_enable(None, C.byref(o)) == 1
    assert L.mceik_mcmc_lang_disable(None) == 1
    assert L.mceik_mcmc_lang_get(None, None, None) == 1
    assert L.mceik_mcmc_lang_stats(None, None, None, None, None, 0) == 1
    assert L.mceik_mcmc_lang_last(None, None, None, None, None, None, None, None) == 1
    assert _lib.LANG_DMAX_CAP == 32
    for bad in (dict(sigma=0.0), dict(dmax=0), dict(dmax=33), dict(v=1499), dict(v=9001), dict(cell=-1)):
        kw = dict(cell=0, d=0.1, v=4000, sigma=4.0, dmax=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            mcmc.lang_cell(1, 0, 0, kw["cell"], kw["d"], kw["v"], 1500, 9000, kw["sigma"], kw["dmax"])
