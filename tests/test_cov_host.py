"""Host side of the probe-to-cell covariances (include/mceik.h mceik_cov_*): the
ABI of the two structs, and merge / finish on synthetic integer data against
Python integers and fractions.Fraction, in one process and over two gloo
ranks.  No GPU call."""
import ctypes as C
import math
import os
import socket
from fractions import Fraction

import numpy as np
import pytest

from test_posterior_host import _offsets_c, check_close

MASK = (1 << 64) - 1


@pytest.mark.parametrize("ctype,pyname", [("mceik_cov_opts", "CovOpts"), ("mceik_cov_partials", "CovPartials")])
def test_ctypes_mirrors_match_header(ctype, pyname):
    from mceik_amd import _lib
    cls = getattr(_lib, pyname)
    names = [f[0] for f in cls._fields_]
    c = _offsets_c(ctype, names)
    assert C.sizeof(cls) == c["sizeof"]
    for n in names:
        assert getattr(cls, n).offset == c[n], n
    assert _lib.COV_MAX_PROBES == 64 and cls.kind.size == 64 * C.sizeof(C.c_int)


# --- sums and expected values in Python integers / Fractions (tests/test_gpu_cov.py uses them too) ---
def words128(x):
    """(lo, hi) uint64 words of the 128-bit two's complement of Python int x."""
    x = int(x) & ((1 << 128) - 1)
    return (x & MASK, x >> 64)


def py_sums(x, v):
    """x [n][M][np], v [n][M][ncm] integer arrays (states, chains) -> dict of
    Python-int lists: A, G, S, Q, C and the per-chain Ac, Sc with their chain
    reductions PA, P, T."""
    x, v = np.asarray(x, dtype=object), np.asarray(v, dtype=object)
    n, M, npr = x.shape
    ncm = v.shape[2]
    Ac = [[sum(int(x[t, c, p]) for t in range(n)) for p in range(npr)] for c in range(M)]
    Sc = [[sum(int(v[t, c, j]) for t in range(n)) for j in range(ncm)] for c in range(M)]
    xs = [[int(a) for a in row] for row in x.reshape(n * M, npr)]
    vs = [[int(a) for a in row] for row in v.reshape(n * M, ncm)]
    out = {"n": n, "M": M, "Ac": Ac, "Sc": Sc}
    out["A"] = [sum(r[p] for r in Ac) for p in range(npr)]
    out["S"] = [sum(r[j] for r in Sc) for j in range(ncm)]
    out["G"] = [[sum(r[p] * r[q] for r in xs) for q in range(npr)] for p in range(npr)]
    out["Q"] = [sum(r[j] ** 2 for r in vs) for j in range(ncm)]
    out["C"] = [[sum(a[p] * b[j] for a, b in zip(xs, vs)) for j in range(ncm)] for p in range(npr)]
    out["PA"] = [[sum(r[p] * r[q] for r in Ac) for q in range(npr)] for p in range(npr)]
    out["P"] = [sum(r[j] ** 2 for r in Sc) for j in range(ncm)]
    out["T"] = [[sum(a[p] * b[j] for a, b in zip(Ac, Sc)) for j in range(ncm)] for p in range(npr)]
    return out


def fill(parts, s, within=True):
    """Python-int sums (py_sums) into a mcmc.CovPartials."""
    parts.nchains, parts.nkept = s["M"], s["n"]
    parts.A[:], parts.S[:] = s["A"], s["S"]
    for name in ("G", "Q", "C") + (("PA", "P", "T") if within else ()):
        a = getattr(parts, name)
        flat = np.asarray(s[name], dtype=object).ravel()
        a.reshape(-1, 2)[:] = [words128(t) for t in flat]
    return parts


def part_words(a):
    return [(int(lo), int(hi)) for lo, hi in np.asarray(a).reshape(-1, 2)]


def want_words(x):
    return [words128(t) for t in np.asarray(x, dtype=object).ravel()]


def _ratio(num, den2):
    """sign(num) sqrt(num^2 / den2) of exact rationals, correctly rounded: integer sqrt at 2^200 scaling."""
    if num == 0:
        return 0.0
    r2 = Fraction(num * num) / den2
    k = 200
    root = math.isqrt((r2.numerator << (2 * k)) // r2.denominator)
    return math.copysign(float(Fraction(root, 1 << k)), num)


def expected(s, within=True):
    """The header's formulas in exact rationals, rounded once: dict like CovPartials.finish()."""
    n, M = s["n"], s["M"]
    N = M * n
    npr, ncm = len(s["A"]), len(s["S"])
    nan = math.nan
    pooled, win = N >= 2, within and n >= 2 and M >= 1
    dp, dw = (N * (N - 1)) if pooled else 1, (M * n * (n - 1)) if win else 1
    nx = [N * s["G"][p][p] - s["A"][p] ** 2 for p in range(npr)]
    nv = [N * s["Q"][j] - s["S"][j] ** 2 for j in range(ncm)]
    wx = [n * s["G"][p][p] - s["PA"][p][p] for p in range(npr)] if win else [0] * npr
    wv = [n * s["Q"][j] - s["P"][j] for j in range(ncm)] if win else [0] * ncm

    def table(second, first_a, first_b, red, va, vb, wa, wb):
        rows, cols = len(first_a), len(first_b)
        cov, corr, covw, corrw = (np.full((rows, cols), nan) for _ in range(4))
        for a in range(rows):
            for b in range(cols):
                if pooled:
                    num = N * second[a][b] - first_a[a] * first_b[b]
                    cov[a, b] = float(Fraction(num, dp))
                    if va[a] != 0 and vb[b] != 0:
                        corr[a, b] = _ratio(Fraction(num), Fraction(va[a] * vb[b]))
                if win:
                    num = n * second[a][b] - red[a][b]
                    covw[a, b] = float(Fraction(num, dw))
                    if wa[a] != 0 and wb[b] != 0:
                        corrw[a, b] = _ratio(Fraction(num), Fraction(wa[a] * wb[b]))
        return cov, corr, covw, corrw
    out = {}
    out["cov"], out["corr"], out["cov_within"], out["corr_within"] = table(s["C"], s["A"], s["S"], s.get("T"), nx, nv, wx, wv)
    out["probe_cov"], out["probe_corr"], out["probe_cov_within"], out["probe_corr_within"] = \
        table(s["G"], s["A"], s["A"], s.get("PA"), nx, nx, wx, wx)
    out["probe_mean"] = np.array([float(Fraction(a, N)) if N > 0 else nan for a in s["A"]])
    return out


def check_summary(got, want):
    for k, w in want.items():
        check_close(np.asarray(got[k], np.float64).ravel(), np.asarray(w, np.float64).ravel(), k)


def _states():
    """n = 4 states, M = 3 chains, ncm = 5, np = 2: entry 0 constant everywhere,
    entry 1 constant per chain, probe 0 entry 2 itself, probe 1 signed (a static)."""
    rng = np.random.default_rng(21)
    v = rng.integers(1500, 9001, (4, 3, 5)).astype(np.int64)
    v[:, :, 0] = 4321
    v[:, :, 1] = rng.integers(1500, 9001, 3)[None, :]
    x = np.empty((4, 3, 2), np.int64)
    x[:, :, 0] = v[:, :, 2]
    x[:, :, 1] = rng.integers(-40, 41, (4, 3))
    return x, v


PROBES = [(0, 2), (2, 1)]


def test_finish_matches_fractions():
    from mceik_amd import mcmc
    x, v = _states()
    s = py_sums(x, v)
    got = fill(mcmc.CovPartials(PROBES, 5, True), s).finish()
    want = expected(s)
    check_summary(got, want)
    # not vacuous, and the rules: a constant entry has no correlation; one that is constant per chain has a pooled one only
    assert np.isnan(got["corr"][:, 0]).all() and np.isnan(got["corr_within"][:, 0]).all() and (got["cov"][:, 0] == 0).all()
    assert np.isfinite(got["corr"][:, 1]).all() and np.isnan(got["corr_within"][:, 1]).all()
    assert np.isfinite(got["corr"][:, 2:]).all() and np.isfinite(got["corr_within"][:, 2:]).all()
    assert 0 < abs(got["corr"][1, 3]) < 1
    # probe 0 is entry 2 itself: perfectly correlated, pooled and within the chains
    for k in ("corr", "corr_within"):
        assert abs(got[k][0, 2] - 1.0) <= 1e-14, (k, got[k][0, 2])
    assert abs(got["probe_corr"][0, 0] - 1.0) <= 1e-14 and abs(got["probe_corr_within"][1, 1] - 1.0) <= 1e-14
    assert got["cov"][0, 2] == got["probe_cov"][0, 0]


def test_finish_nan_rules():
    from mceik_amd import mcmc
    x, v = _states()
    keys_p = ("cov", "corr", "probe_cov", "probe_corr")
    keys_w = ("cov_within", "corr_within", "probe_cov_within", "probe_corr_within")
    # within = 0: no within-chain quantity; the pooled ones are those of within = 1
    s = py_sums(x, v)
    got = fill(mcmc.CovPartials(PROBES, 5, False), s, within=False).finish()
    check_summary(got, expected(s, within=False))
    assert all(np.isnan(got[k]).all() for k in keys_w) and np.isfinite(got["cov"]).all()
    # n = 1 state per chain: no within-chain quantity, pooled ones over M = 3 values
    s = py_sums(x[:1], v[:1])
    got = fill(mcmc.CovPartials(PROBES, 5, True), s).finish()
    check_summary(got, expected(s))
    assert all(np.isnan(got[k]).all() for k in keys_w) and np.isfinite(got["cov"]).all()
    # N = 1: nothing but the mean
    s = py_sums(x[:1, :1], v[:1, :1])
    got = fill(mcmc.CovPartials(PROBES, 5, True), s).finish()
    assert all(np.isnan(got[k]).all() for k in keys_p + keys_w)
    assert np.array_equal(got["probe_mean"], x[0, 0].astype(np.float64))
    # N = 0
    empty = mcmc.CovPartials(PROBES, 5, True)
    got = empty.finish()
    assert all(np.isnan(got[k]).all() for k in keys_p + keys_w + ("probe_mean",))


def _split(x, v, cut):
    return py_sums(x[:, :cut], v[:, :cut]), py_sums(x[:, cut:], v[:, cut:])


def test_merge_is_exact_and_refuses_mismatches():
    from mceik_amd import mcmc
    x, v = _states()
    full = py_sums(x, v)
    sa, sb = _split(x, v, 1)
    a, b = fill(mcmc.CovPartials(PROBES, 5, True), sa), fill(mcmc.CovPartials(PROBES, 5, True), sb)
    a.merge(b)
    assert a.nchains == 3 and a.nkept == 4
    assert [int(t) for t in a.A] == full["A"] and [int(t) for t in a.S] == full["S"]
    for name in ("G", "Q", "C", "PA", "P", "T"):
        assert part_words(getattr(a, name)) == want_words(full[name]), name
    for kw in (dict(probes=[(0, 2)]), dict(probes=[(0, 2), (2, 0)]), dict(probes=[(0, 2), (3, 1)]), dict(ncm=4),
               dict(within=False), dict(nkept=5)):
        args = dict(probes=PROBES, ncm=5, within=True, nkept=4)
        args.update(kw)
        c = mcmc.CovPartials(args["probes"], args["ncm"], args["within"], nchains=1, nkept=args["nkept"])
        before = (a.S.copy(), a.C.copy())
        with pytest.raises(ValueError):
            a.merge(c)
        assert np.array_equal(a.S, before[0]) and np.array_equal(a.C, before[1]) and a.nchains == 3


def test_merge_carries_across_the_word_boundary():
    """Hand-made words: a low word that overflows (2^64 - 5 + 9 carries 1 into
    the high word), a negative plus a positive value that crosses zero, and two
    negative values; every 128-bit array takes the same path."""
    from mceik_amd import mcmc
    vals_a = [(1 << 64) - 5, -7, -(1 << 70) - 3, (1 << 100) + (1 << 63), 0]
    vals_b = [9, 12, -(1 << 64) + 2, (1 << 63), -1]
    a, b = mcmc.CovPartials([(0, 0)], 5, True, nchains=2, nkept=3), mcmc.CovPartials([(0, 0)], 5, True, nchains=1, nkept=3)
    for name in ("Q", "P"):
        getattr(a, name)[:] = [words128(t) for t in vals_a]
        getattr(b, name)[:] = [words128(t) for t in vals_b]
    for name in ("C", "T"):
        getattr(a, name)[0, :] = [words128(t) for t in vals_a]
        getattr(b, name)[0, :] = [words128(t) for t in vals_b]
    a.G[0, 0], b.G[0, 0] = words128(vals_a[0]), words128(vals_b[0])
    a.PA[0, 0], b.PA[0, 0] = words128(vals_a[2]), words128(vals_b[2])
    a.A[0], b.A[0], a.S[:], b.S[:] = -5, 3, [1, -2, 3, -4, 5], [10, 20, 30, 40, -50]
    assert int(a.Q[0, 0]) + int(b.Q[0, 0]) >= 1 << 64                 # the low word overflows
    a.merge(b)
    want = [x + y for x, y in zip(vals_a, vals_b)]
    for name in ("Q", "P", "C", "T"):
        assert part_words(getattr(a, name)) == want_words(want), name
    assert part_words(a.Q)[0] == (4, 1)
    assert part_words(a.G) == [words128(want[0])] and part_words(a.PA) == [words128(want[2])]
    assert int(a.A[0]) == -2 and [int(t) for t in a.S] == [11, 18, 33, 36, -45] and a.nchains == 3


# --- two ranks (gloo): synthetic partials merged on rank 0 ---
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_states():
    """n = 4, M = 5 chains (rank 0: chains 0..1, rank 1: 2..4), ncm = 6, np = 3; values of a few 1e9 so that the
    products pass 2^64."""
    rng = np.random.default_rng(33)
    v = rng.integers(2_000_000_000, 2_100_000_000, (4, 5, 6)).astype(np.int64)
    x = rng.integers(-2_000_000_000, 2_000_000_000, (4, 5, 3)).astype(np.int64)
    return x, v


RANK_PROBES = [(0, 1), (1, 4), (2, 0)]


def _worker(rank, world, port, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here); sys.path.insert(0, os.path.dirname(here))
    import torch.distributed as dist
    from mceik_amd import mcmc
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    x, v = _rank_states()
    lo, hi = mcmc.shard(5, rank, world)

    class Fake:                          # what cov_summary needs of a sampler
        def cov_partials(self):
            return fill(mcmc.CovPartials(RANK_PROBES, 6, True), py_sums(x[:, lo:hi], v[:, lo:hi]))
    parts = Fake().cov_partials()
    every = [None] * world if rank == 0 else None
    dist.gather_object(parts, every, dst=0)
    summ = mcmc.cov_summary(Fake(), group=dist.group.WORLD, dst=0)
    if rank == 0:
        merged = every[0]
        for other in every[1:]:
            merged.merge(other)
        q.put(({k: getattr(merged, k) for k in ("A", "S", "G", "Q", "C", "PA", "P", "T", "nchains", "nkept")},
               {k: getattr(summ, k) for k in ("cov", "corr", "cov_within", "corr_within", "probe_mean", "nchains")}))
    else:
        assert summ is None
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_merge_equals_single_process():
    torch = pytest.importorskip("torch")
    import torch.multiprocessing as tmp
    from mceik_amd import mcmc
    ctx = tmp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got, summ = q.get(timeout=300)
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    x, v = _rank_states()
    full = py_sums(x, v)
    assert got["nchains"] == 5 and got["nkept"] == 4
    assert [int(t) for t in got["A"]] == full["A"] and [int(t) for t in got["S"]] == full["S"]
    for name in ("G", "Q", "C", "PA", "P", "T"):
        assert part_words(got[name]) == want_words(full[name]), name
    assert min(full["Q"]) >= 1 << 64 and min(full["P"]) >= 1 << 64          # the high words are in use
    one = mcmc.CovSummary(fill(mcmc.CovPartials(RANK_PROBES, 6, True), full))
    for k in ("cov", "corr", "cov_within", "corr_within", "probe_mean"):
        assert np.asarray(summ[k]).tobytes() == getattr(one, k).tobytes(), k
    assert summ["nchains"] == 5 and np.isfinite(one.corr).all()
