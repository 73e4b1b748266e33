"""Host side of the streaming posterior (include/mceik.h mceik_posterior_*): the
ABI of the two structs, and merge / finish on synthetic integer data against
Python integers and fractions.Fraction.  No GPU call."""
import ctypes as C
import math
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
MASK = (1 << 64) - 1


def _offsets_c(ctype, fields):
    body = "".join(f'  printf("{f} %zu\\n", offsetof({ctype}, {f}));\n' for f in fields)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mceik.h"\n'
           f'int main(void) {{\n  printf("sizeof %zu\\n", sizeof({ctype}));\n{body}  return 0;\n}}\n')
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "o.c")
        open(p, "w").write(src)
        exe = os.path.join(td, "o")
        subprocess.run(["gcc", "-I", INC, p, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(out[0::2], map(int, out[1::2])))


@pytest.mark.parametrize("ctype,pyname", [("mceik_posterior_opts", "PosteriorOpts"),
                                          ("mceik_posterior_partials", "PosteriorPartials")])
def test_ctypes_mirrors_match_header(ctype, pyname):
    from mceik_amd import _lib
    cls = getattr(_lib, pyname)
    names = [f[0] for f in cls._fields_]
    c = _offsets_c(ctype, names)
    assert C.sizeof(cls) == c["sizeof"]
    for n in names:
        assert getattr(cls, n).offset == c[n], n


# --- partials and expected values in Python integers / Fractions ---
def py_partials(sums, sumsqs):
    """sums, sumsqs: [M][ncm] Python ints per chain -> (S, Q, P) lists of Python ints."""
    ncm = len(sums[0])
    S = [sum(row[i] for row in sums) for i in range(ncm)]
    Q = [sum(row[i] for row in sumsqs) for i in range(ncm)]
    P = [sum(row[i] ** 2 for row in sums) for i in range(ncm)]
    return S, Q, P


def fill(parts, S, Q, P, nchains, nkept):
    parts.nchains, parts.nkept = nchains, nkept
    for i in range(parts.ncm):
        parts.S[i] = S[i]
        parts.Q[i] = (Q[i] & MASK, Q[i] >> 64)
        parts.P[i] = (P[i] & MASK, P[i] >> 64)
    return parts


def words(x):
    return [(int(v) & MASK, int(v) >> 64) for v in x]


def expected(S, Q, P, M, n, per_chain=True):
    """mean, var, rhat of the header's formulas in exact rationals, rounded once."""
    N = M * n
    mean, var, rhat = [], [], []
    for s, q, p in zip(S, Q, P):
        mean.append(float(Fraction(s, N)))
        var.append(float(Fraction(N * q - s * s, N * (N - 1))) if N >= 2 else math.nan)
        wnum = n * q - p
        if not per_chain or M < 2 or n < 2 or wnum == 0:
            rhat.append(math.nan)
            continue
        W = Fraction(wnum, M * n * (n - 1))
        Bn = Fraction(M * p - s * s, M * (M - 1) * n * n)
        r2 = (Fraction(n - 1, n) * W + Bn) / W
        # sqrt of the exact rational, correctly rounded: integer sqrt at 2^200 scaling
        k = 200
        root = math.isqrt((r2.numerator << (2 * k)) // r2.denominator)
        rhat.append(float(Fraction(root, 1 << k)))
    return np.array(mean), np.array(var), np.array(rhat)


def check_close(got, want, what):
    """Relative 1e-14: the numerators are exact integers converted once, then at
    most ~10 correctly rounded fp64 operations (2^-53 each), no cancellation."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    assert np.all(err <= 1e-14 * np.abs(want[ok])), (what, float((err / np.maximum(np.abs(want[ok]), 1e-300)).max()))


def _states():
    """M = 7 chains, n = 5 states, 40 entries in [1500, 9000]; entry 0 constant
    everywhere, entry 1 constant per chain, entry 2 at vmax in one chain."""
    rng = np.random.default_rng(5)
    v = rng.integers(1500, 9001, (7, 5, 40)).astype(np.int64)
    v[:, :, 0] = 4321
    v[:, :, 1] = rng.integers(1500, 9001, 7)[:, None]
    v[3, :, 2] = 9000
    return v


def _chain_moments(v):
    sums = [[int(x) for x in row] for row in v.sum(1)]
    sumsqs = [[int(x) for x in row] for row in (v ** 2).sum(1)]
    return sums, sumsqs


def test_finish_matches_fractions():
    from mceik_amd import mcmc
    v = _states()
    sums, sumsqs = _chain_moments(v)
    S, Q, P = py_partials(sums, sumsqs)
    parts = fill(mcmc.PosteriorPartials(40, 0, True), S, Q, P, 7, 5)
    mean, var, rhat = parts.finish()
    em, ev, er = expected(S, Q, P, 7, 5)
    assert np.isnan(er[0]) and np.isnan(er[1]) and np.isfinite(er[2:]).all()
    check_close(mean, em, "mean")
    check_close(var, ev, "var")
    check_close(rhat, er, "rhat")
    assert var[0] == 0.0 and np.isnan(rhat[0]) and np.isnan(rhat[1]) and var[1] > 0.0
    # the documented NaN conventions: pooled mode, one chain, one state
    pooled = fill(mcmc.PosteriorPartials(40, 0, False), S, Q, [0] * 40, 7, 5)
    m2, v2, r2 = pooled.finish()
    assert np.array_equal(m2, mean) and np.array_equal(v2, var) and np.isnan(r2).all()
    one = fill(mcmc.PosteriorPartials(40, 0, True), sums[0], sumsqs[0], [x * x for x in sums[0]], 1, 5)
    assert np.isnan(one.finish()[2]).all()
    single = fill(mcmc.PosteriorPartials(40, 0, True), [int(x) for x in v[0, 0]], [int(x) ** 2 for x in v[0, 0]],
                  [int(x) ** 2 for x in v[0, 0]], 1, 1)
    ms, vs, rs = single.finish()
    assert np.array_equal(ms, v[0, 0].astype(np.float64)) and np.isnan(vs).all() and np.isnan(rs).all()


def test_merge_is_exact_and_refuses_mismatches():
    from mceik_amd import mcmc
    v = _states()
    sums, sumsqs = _chain_moments(v)
    rng = np.random.default_rng(6)
    hists = rng.integers(0, 2 ** 40, (2, 40, 3)).astype(np.uint64)
    full = py_partials(sums, sumsqs)
    a = fill(mcmc.PosteriorPartials(40, 3, True), *py_partials(sums[:3], sumsqs[:3]), 3, 5)
    b = fill(mcmc.PosteriorPartials(40, 3, True), *py_partials(sums[3:], sumsqs[3:]), 4, 5)
    a.hist[:], b.hist[:] = hists[0], hists[1]
    a.merge(b)
    assert a.nchains == 7 and a.nkept == 5
    assert [int(x) for x in a.S] == full[0]
    assert [(int(l), int(h)) for l, h in a.Q] == words(full[1])
    assert [(int(l), int(h)) for l, h in a.P] == words(full[2])
    assert np.array_equal(a.hist, hists[0] + hists[1])
    for kw in (dict(nkept=6), dict(ncm=39), dict(nbins=2), dict(per_chain=False)):
        args = dict(ncm=40, nbins=3, per_chain=True, nkept=5)
        args.update(kw)
        c = mcmc.PosteriorPartials(args["ncm"], args["nbins"], args["per_chain"], nchains=1, nkept=args["nkept"])
        before = a.S.copy()
        with pytest.raises(ValueError):
            a.merge(c)
        assert np.array_equal(a.S, before) and a.nchains == 7


@pytest.mark.parametrize("pair,p_carries", [((2_500_000_000, 2_400_000_000), False),
                                            ((3_100_000_000, 3_000_000_000), True)])
def test_128_bit_carry(pair, p_carries):
    """M = 2, n = 3, chain sums of a few 1e9; sumsq_c = ceil(sum_c^2 / n) + a
    small spread keeps n Q - P >= 0.  With (2.5e9, 2.4e9) P = sum_c sum_c^2 =
    1.201e19 stays just under 2^64 = 1.845e19 but n Q, M P and S^2 pass it; with
    (3.1e9, 3.0e9) P itself carries into its high word."""
    from mceik_amd import mcmc
    sums = [[pair[0]], [pair[1]]]
    sumsqs = [[-(-s[0] ** 2 // 3) + d] for s, d in zip(sums, (17, 40))]
    S, Q, P = py_partials(sums, sumsqs)
    assert 3 * Q[0] - P[0] > 0 and 2 * P[0] >= 1 << 64 and S[0] ** 2 >= 1 << 64
    parts = fill(mcmc.PosteriorPartials(1, 0, True), S, Q, P, 2, 3)
    assert (P[0] >= 1 << 64) == p_carries and (int(parts.P[0, 1]) >= 1) == p_carries
    mean, var, rhat = parts.finish()
    em, ev, er = expected(S, Q, P, 2, 3)
    assert np.isfinite(er).all()
    check_close(mean, em, "mean")
    check_close(var, ev, "var")
    check_close(rhat, er, "rhat")
    # split 1 + 1 and merged: the carry into the high word survives the merge
    a = fill(mcmc.PosteriorPartials(1, 0, True), *py_partials(sums[:1], sumsqs[:1]), 1, 3)
    b = fill(mcmc.PosteriorPartials(1, 0, True), *py_partials(sums[1:], sumsqs[1:]), 1, 3)
    a.merge(b)
    assert [(int(l), int(h)) for l, h in a.P] == words(P) and [(int(l), int(h)) for l, h in a.Q] == words(Q)
