"""The streaming data-fit sums (csrc/fit.hip) restated with
numpy and Python integers: from a chain state's travel-time tables and
effective observations the integers q, zq, tq and the histogram bin of every
pick (mcmc._pick_terms gives t0, r and the weights), and from a list of kept
states every accumulator word.  The tables of a model come from the CPU oracle
(tests/_oracle.py), as in test_gpu_nuis.py."""
import math

import numpy as np

QMAX = 2 ** 31 - 1
MASK = (1 << 64) - 1
ZSCALE = 1024.0


def sat32(x):
    """(rint(x) clamped to +-(2^31 - 1), 1 if it was clamped): fp64 round-half-even; a NaN clamps upwards."""
    r = float(np.rint(np.float64(x)))
    if not (r <= QMAX):
        return QMAX, 1
    if r < -QMAX:
        return -QMAX, 1
    return int(r), 0


def state_words(p, ttab, var, tcorr, tick, nbins, zmax, t0_ref=None):
    """One chain state: (q, zq, bin int64 [nobs] (bin -1: a masked pick), tq int64 [nev], sat [3])."""
    from mceik_amd import mcmc
    nobs, nev = len(p.tobs), p.nevents
    inv, hs, half = 1.0 / tick, nbins / (2.0 * zmax), float(nbins // 2)
    ref = np.zeros(nev) if t0_ref is None else np.asarray(t0_ref, np.float64)
    q, zq, b = np.zeros(nobs, np.int64), np.zeros(nobs, np.int64), np.full(nobs, -1, np.int64)
    tq, sat = np.zeros(nev, np.int64), [0, 0, 0]
    for e, (js, w, _, res, _, t0) in enumerate(mcmc._pick_terms(p, ttab, var, tcorr, with_t0=True)):
        for j, wj, r in zip(js, w, res):
            z = wj * r
            q[j], s = sat32(r * inv)
            sat[0] += s
            zq[j], s = sat32(z * ZSCALE)
            sat[1] += s
            f = z * hs + half
            b[j] = 0 if not (f >= 0.0) else min(nbins - 1, int(math.floor(min(f, 1e9))))
        if js:
            tq[e], s = sat32((t0 - float(ref[e])) * inv)
            sat[2] += s
    return q, zq, b, tq, sat


def words128(x):
    return (int(x) & MASK, (int(x) >> 64) & MASK)


class Fit:
    """The accumulators as Python integers."""

    def __init__(self, p, tick=2.0 ** -20, nbins=64, zmax=8.0, t0_ref=None):
        self.p, self.tick, self.nbins, self.zmax = p, tick, nbins, zmax
        self.t0_ref = np.zeros(p.nevents) if t0_ref is None else np.asarray(t0_ref, np.float64)
        nobs, nev = len(p.tobs), p.nevents
        self.sq, self.szq, self.sq2, self.szq2 = ([0] * nobs for _ in range(4))
        self.stq, self.stq2 = [0] * nev, [0] * nev
        self.hist = np.zeros((max(1, p.nphase), p.nstat, nbins), np.int64)
        self.sat = [0, 0, 0]
        self.n = 0

    def add_words(self, q, zq, b, tq, sat):
        """One chain's state."""
        p = self.p
        for j in range(len(q)):
            if b[j] < 0:
                continue
            self.sq[j] += int(q[j])
            self.szq[j] += int(zq[j])
            self.sq2[j] += int(q[j]) ** 2
            self.szq2[j] += int(zq[j]) ** 2
            self.hist[int(p.obs_phase[j]), int(p.obs_stat[j]), int(b[j])] += 1
        for e in range(len(tq)):
            self.stq[e] += int(tq[e])
            self.stq2[e] += int(tq[e]) ** 2
        for k in range(3):
            self.sat[k] += sat[k]

    def add(self, ttab, var=None, tcorr=None):
        w = state_words(self.p, ttab, var, tcorr, self.tick, self.nbins, self.zmax, self.t0_ref)
        self.add_words(*w)
        return w

    def counted(self):
        """Every chain of a kept step is added."""
        self.n += 1

    def raw(self):
        """The words as Sampler.fit_raw() holds them."""
        s64 = lambda xs: np.array([x & MASK for x in xs], np.uint64).view(np.int64)
        w = lambda xs: np.array([words128(x) for x in xs], np.uint64).reshape(len(xs), 2)
        return {"sq": s64(self.sq), "szq": s64(self.szq), "sq2": w(self.sq2), "szq2": w(self.szq2),
                "stq": s64(self.stq), "stq2": w(self.stq2), "hist": self.hist.copy(),
                "sat": np.array(self.sat, np.int64), "n": self.n}


ARRAYS = ("sq", "szq", "sq2", "szq2", "stq", "stq2", "hist", "sat")


def assert_raw_equal(got, want, what=""):
    assert got["n"] == want["n"], (what, "n", got["n"], want["n"])
    for k in ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, k, np.argwhere(a != b)[:4])


class _View:
    """A problem with other event nodes: what tests/_oracle.make_problem reads, overridden."""

    def __init__(self, p, **kw):
        self._p = p
        self.__dict__.update(kw)

    def __getattr__(self, name):
        return getattr(self._p, name)


def oracle_tables(p, v, hyp=None, prec=32):
    """The CPU oracle's tables [nphase, nstat, nev] of one chain's models v at the chain's event nodes (hyp int
    [nev, 3] grid positions; None: the catalogue's)."""
    import _oracle as O
    if hyp is None:
        nodes = p.ev_node
    else:
        xyz = np.asarray(hyp, np.int64)
        nodes = (xyz[:, 2] * p.ny + xyz[:, 1]) * p.nx + xyz[:, 0]
    P = O.make_problem(_View(p, ev_node=np.ascontiguousarray(nodes, np.int32), nevents=len(nodes)), prec)
    tt = O.forward_all_f32(P, np.ascontiguousarray(v, np.int32).ravel())
    return np.asarray(tt, np.float32).reshape(max(1, p.nphase), p.nstat, p.nevents)


def restate(p, states, ncold=None, **opts):
    """states: one dict per kept step with "v" [nchains, ...] and optionally "hyp" [nchains, nev, 3], "var",
    "tcorr" [nchains, nobs].  Returns (Fit, the words of the last kept step per cold chain)."""
    f = Fit(p, **opts)
    last = []
    for st in states:
        v = np.asarray(st["v"])
        n = v.shape[0] if ncold is None else ncold
        last = []
        for c in range(n):
            hyp = None if st.get("hyp") is None else st["hyp"][c]
            var = None if st.get("var") is None else st["var"][c]
            tcorr = None if st.get("tcorr") is None else st["tcorr"][c]
            last.append(f.add(oracle_tables(p, v[c], hyp), var, tcorr))
        f.counted()
    return f, last
