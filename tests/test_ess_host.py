"""Host side of the batch-means effective sample sizes (include/mceik.h
mceik_ess_*): the ABI of the two structs, the restatement tests/_ess.py against
the definitions, and finish / merge / check / lstar on synthetic integer data
against Python integers and fractions.Fraction.  No GPU call."""
import numpy as np
import pytest

import _ess
from test_posterior_host import _offsets_c, check_close

MASK = (1 << 64) - 1


@pytest.mark.parametrize("ctype,pyname", [("mceik_ess_opts", "EssOpts"), ("mceik_ess_partials", "EssPartials")])
def test_ctypes_mirrors_match_header(ctype, pyname):
    import ctypes as C
    from mceik_amd import _lib
    cls = getattr(_lib, pyname)
    names = [f[0] for f in cls._fields_]
    c = _offsets_c(ctype, names)
    assert C.sizeof(cls) == c["sizeof"]
    for n in names:
        assert getattr(cls, n).offset == c[n], n


def fill(parts, A, Q, P, nchains, nkept):
    """A, Q, P [L][ne] Python integers (P, A two's complement where negative) into an `EssPartials`."""
    parts.nchains, parts.nkept = nchains, nkept
    for l in range(parts.nlevels):
        for j in range(parts.ncm + parts.np):
            parts.A[l, j] = int(A[l][j])
            parts.Q[l, j] = (int(Q[l][j]) & MASK, (int(Q[l][j]) >> 64) & MASK)
            parts.P[l, j] = (int(P[l][j]) & MASK, (int(P[l][j]) >> 64) & MASK)
    return parts


def _states(n=19, M=5, ne=12, seed=3):
    """Entry 0 constant everywhere, entry 1 constant per chain, entry 2 negative-going (a static)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(1500, 9001, (n, M, ne)).astype(np.int64)
    v[:, :, 0] = 4321
    v[:, :, 1] = rng.integers(1500, 9001, M)[None, :]
    v[:, :, 2] = rng.integers(-40, 41, (n, M))
    return v


@pytest.mark.parametrize("n,L", [(19, 4), (16, 4), (3, 16), (7, 1), (64, 5)])
def test_restatement_matches_the_definitions(n, L):
    """The recurrence gives Q_l = sum of squared batch sums, P_l = sum_c S_c(nb 2^l)^2 and A_l word for
    word, also where n is no multiple of 2^l, where t has more trailing zeros than levels, and with one level."""
    v = _states(n)
    e = _ess.Ess(v.shape[1], v.shape[2], L)
    for t in range(n):
        e.add(v[t])
    A, Q, P = _ess.direct(v, L)
    assert e.n == n
    for name, want in (("A", A), ("Q", Q), ("P", P)):
        got = getattr(e, name)
        assert [[int(x) for x in r] for r in got] == [[int(x) for x in r] for r in want], name
    assert [int(x) for x in e.Sc.ravel()] == [int(x) for x in v.sum(0).ravel()]
    # pend[l]: the level-l batch sum that waits for its second half, where one is open
    for l in range(L - 1):
        done = (n >> (l + 1)) << (l + 1)
        if n - done >= 1 << l:
            want = v[done:done + (1 << l)].sum(0)
            assert [int(x) for x in e.pend[l].ravel()] == [int(x) for x in want.ravel()], l


def test_finish_matches_fractions_and_nan_rules():
    from mceik_amd import mcmc
    v = _states(19)
    n, M, ne = v.shape
    L = 4
    A, Q, P = _ess.direct(v, L)
    parts = fill(mcmc.EssPartials(ne, L), A, Q, P, M, n)
    for level in (None, 0, 1, 3):
        tau, ess, mcse, used = parts.finish(level)
        et, ee, em, el = _ess.expected(Q, P, M, n, L, level)
        assert used == el == (2 if level is None else level)
        check_close(tau.ravel(), et.ravel(), "tau")
        check_close(ess, ee, "ess")
        check_close(mcse, em, "mcse")
    tau, ess, mcse, used = parts.finish()
    # an entry that never moved within a chain (0: constant; 1: constant per chain) is NaN, R-hat's rule
    assert np.isnan(tau[:, :2]).all() and np.isnan(ess[:2]).all() and np.isnan(mcse[:2]).all()
    assert np.isfinite(tau[:, 2:]).all() and np.isfinite(ess[2:]).all() and (mcse[2:] > 0).all()
    assert np.all(tau[0, 2:] == 1.0)
    # nb_l < 2: n = 19 closes 2 batches of 8 (level 3) but one of 16
    A5, Q5, P5 = _ess.direct(v, 5)
    p5 = fill(mcmc.EssPartials(ne, 5), A5, Q5, P5, M, n)
    t5 = p5.finish()[0]
    assert np.isnan(t5[4]).all() and np.isfinite(t5[3, 2:]).all()
    _, e4, m4, _ = p5.finish(4)
    assert np.isnan(e4).all() and np.isnan(m4).all()
    with pytest.raises(ValueError):
        p5.finish(5)
    # one state, no state, no chain
    for nn, MM in ((1, M), (0, M), (n, 0)):
        An, Qn, Pn = _ess.direct(v[:nn], L)
        pn = fill(mcmc.EssPartials(ne, L), An, Qn, Pn, MM, nn)
        t, e, m, used = pn.finish()
        assert np.isnan(t).all() and np.isnan(e).all() and np.isnan(m).all() and (used == 0 or nn == n)


def test_merge_carries_and_refuses_mismatches():
    from mceik_amd import mcmc
    # hand-made words: low words that wrap, a negative (two's complement) P and A
    a = mcmc.EssPartials(2, 2, nchains=3, nkept=8)
    b = mcmc.EssPartials(2, 2, nchains=4, nkept=8)
    qa, qb = (1 << 64) - 5, 9                        # lo wraps into hi
    pa, pb = -7, 3 - (1 << 64)                       # negative sums: hi words all ones, lo wraps
    for parts, q, p, s in ((a, qa, pa, -11), (b, qb, pb, 4)):
        fill(parts, [[s, s], [s, s]], [[q, q << 20], [q, q]], [[p, p], [p, p]], parts.nchains, 8)
    a.merge(b)
    assert a.nchains == 7 and a.nkept == 8
    assert (int(a.Q[0, 0, 0]), int(a.Q[0, 0, 1])) == ((qa + qb) & MASK, (qa + qb) >> 64) == (4, 1)
    assert (int(a.Q[0, 1, 0]), int(a.Q[0, 1, 1])) == ((((qa + qb) << 20) & MASK), ((qa + qb) << 20) >> 64)
    sp = (pa + pb) & ((1 << 128) - 1)
    assert (int(a.P[1, 1, 0]), int(a.P[1, 1, 1])) == (sp & MASK, sp >> 64)
    assert int(a.A[1, 0]) == -7
    for kw in (dict(nkept=9), dict(ncm=3), dict(nlevels=3), dict(probes=[(1, 0)])):
        args = dict(ncm=2, nlevels=2, nkept=8, probes=[])
        args.update(kw)
        c = mcmc.EssPartials(args["ncm"], args["nlevels"], probes=args["probes"], nchains=1, nkept=args["nkept"])
        before = a.Q.copy()
        with pytest.raises(ValueError):
            a.merge(c)
        assert np.array_equal(a.Q, before) and a.nchains == 7


def test_merged_shards_finish_like_the_whole():
    from mceik_amd import mcmc
    v = _states(19, M=7)
    whole = fill(mcmc.EssPartials(12, 4), *_ess.direct(v, 4), 7, 19)
    a = fill(mcmc.EssPartials(12, 4), *_ess.direct(v[:, :3], 4), 3, 19)
    b = fill(mcmc.EssPartials(12, 4), *_ess.direct(v[:, 3:], 4), 4, 19)
    a.merge(b)
    for k in ("A", "Q", "P"):
        assert getattr(a, k).tobytes() == getattr(whole, k).tobytes(), k
    for x, y in zip(a.finish(), whole.finish()):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_level_bound():
    """pend is int32: max value x 2^(nlevels - 2) must stay below 2^31."""
    from mceik_amd import mcmc
    assert mcmc.ess_check(16, 9000) and mcmc.ess_check(1, 2 ** 31 - 1) and mcmc.ess_check(2, 2 ** 31 - 1)
    assert not mcmc.ess_check(2, 2 ** 31) and mcmc.ess_check(3, 2 ** 30 - 1) and not mcmc.ess_check(3, 2 ** 30)
    assert mcmc.ess_check(16, 2 ** 17 - 1) and not mcmc.ess_check(16, 2 ** 17)
    assert not mcmc.ess_check(0, 1) and not mcmc.ess_check(17, 1)


def test_lstar():
    from mceik_amd import mcmc
    for n, want in ((1, 0), (3, 0), (4, 1), (15, 1), (16, 2), (2 ** 20, 10)):
        assert mcmc.ess_lstar(16, n) == want == _ess.lstar(16, n), n
    assert mcmc.ess_lstar(8, 2 ** 20) == 7 and mcmc.ess_lstar(1, 2 ** 20) == 0 and mcmc.ess_lstar(8, 0) == 0


# rho: (tau = (1 + rho) / (1 - rho), tau observed at level 6 on the chains below, asserted band = 4 x |observed - tau|)
_AR1 = {0.0: (1.0, 1.0034, 0.014), 0.5: (3.0, 2.8376, 0.65), 0.9: (19.0, 16.4169, 10.4)}


def _ar1_chains():
    """64 chains x 4096 states of integer-rounded AR(1), one entry per rho: v = round(5000 + 300 x),
    x_t = rho x_(t-1) + sqrt(1 - rho^2) e_t from the stationary start, seed 2024."""
    rng = np.random.default_rng(2024)
    n, M = 4096, 64
    out = np.empty((n, M, len(_AR1)), np.int64)
    for j, rho in enumerate(_AR1):
        e = rng.standard_normal((n, M))
        x = e[0].copy()
        for t in range(n):
            if t:
                x = rho * x + np.sqrt(1.0 - rho * rho) * e[t]
            out[t, :, j] = np.rint(5000.0 + 300.0 * x)
    return out


def test_estimator_against_ar1():
    """Not merely self-consistent: tau at lstar = 6 (batches of 64) against (1 + rho) / (1 - rho).
    Batch means are biased low at strong correlation: 64 states are 3.4 tau at rho = 0.9."""
    from mceik_amd import mcmc
    v = _ar1_chains()
    n, M, ne = v.shape
    L = 8
    e = _ess.Ess(M, ne, L)
    for t in range(n):
        e.add(v[t])
    parts = fill(mcmc.EssPartials(ne, L), e.A, e.Q, e.P, M, n)
    s = mcmc.EssSummary(parts)
    assert s.level == 6 and s.count == n and s.nchains == M
    et, ee, em, _ = _ess.expected(e.Q, e.P, M, n, L)
    check_close(s.tau_levels.ravel(), et.ravel(), "tau")
    check_close(s.ess, ee, "ess")
    for j, (rho, (tau, seen, band)) in enumerate(_AR1.items()):
        print(f"rho {rho}: tau {tau} observed {s.tau[j]:.4f} levels {np.round(s.tau_levels[:, j], 3)}")
    for j, (rho, (tau, seen, band)) in enumerate(_AR1.items()):
        assert abs(s.tau[j] - tau) <= band, (rho, s.tau[j])
        assert abs(s.ess[j] * s.tau[j] - M * n) <= 1e-9 * M * n
