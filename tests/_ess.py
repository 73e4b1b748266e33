"""Restatement of the batch-means accumulators of csrc/ess.hip
in Python integers, and the estimates they give in exact rationals.

`Ess` holds, for M chains and ne entries, Sc [M][ne], pend [L - 1][M][ne] and
the pooled A, Q, P [L][ne] as numpy object arrays of Python integers, and adds
one state of every chain at a time by the recurrence of include/mceik.h.
`expected` forms tau, ESS and the Monte-Carlo standard error from A, Q, P with
fractions.Fraction; only the last square root is floating point."""
import math
from fractions import Fraction

import numpy as np

MASK64 = (1 << 64) - 1


class Ess:
    def __init__(self, nchains, ne, nlevels):
        self.M, self.ne, self.L, self.n = nchains, ne, nlevels, 0
        self.Sc = np.zeros((nchains, ne), object)
        self.pend = np.zeros((max(nlevels - 1, 0), nchains, ne), object)
        self.A, self.Q, self.P = (np.zeros((nlevels, ne), object) for _ in range(3))

    def add(self, v):
        """State number t = n + 1 of every chain: v [M][ne] integers."""
        v = np.asarray(v).astype(object).reshape(self.M, self.ne)
        t = self.n + 1
        k = (t & -t).bit_length() - 1            # trailing zero bits of t
        kk = min(k, self.L - 1)
        b = v.copy()
        self.Sc = self.Sc + v
        for l in range(kk + 1):
            self.A[l] += b.sum(0)
            self.Q[l] += (b * b).sum(0)
            self.P[l] += (b * (2 * self.Sc - b)).sum(0)
            if l == k and l <= self.L - 2:
                self.pend[l] = b
                break
            if l < kk:
                b = self.pend[l] + b
        self.n = t
        return self

    def words(self, name):
        """A as signed Python integers [L][ne]; Q, P as (lo, hi) words of 128-bit two's complement [L][ne][2]."""
        a = getattr(self, name)
        if name == "A":
            return [[int(x) for x in row] for row in a]
        return [[(int(x) & MASK64, (int(x) >> 64) & MASK64) for x in row] for row in a]


def direct(states, nlevels):
    """A, Q, P [L][ne] straight from their definitions, states [n][M][ne]: the
    closed level-l batches of every chain are the first n >> l blocks of 2^l
    states."""
    s = np.asarray(states).astype(object)
    n, M, ne = s.shape
    A, Q, P = (np.zeros((nlevels, ne), object) for _ in range(3))
    for l in range(nlevels):
        nb, m = n >> l, 1 << l
        for b in range(nb):
            B = s[b * m:(b + 1) * m].sum(0)          # [M][ne]
            A[l] += B.sum(0)
            Q[l] += (B * B).sum(0)
        if nb:
            S = s[:nb * m].sum(0)
            P[l] += (S * S).sum(0)
    return A, Q, P


def lstar(nlevels, n):
    lg = n.bit_length() - 1 if n >= 1 else 0         # floor(log2 n)
    return min(nlevels - 1, lg // 2)


def expected(Q, P, M, n, nlevels, level=None):
    """(tau [L][ne], ess [ne], mcse [ne], level) as floats of exact rationals (NaN by the header's rules)."""
    ne = len(Q[0])
    ls = lstar(nlevels, n) if level is None else level
    nan = float("nan")
    tau = np.full((nlevels, ne), nan)
    ess, mcse = np.full(ne, nan), np.full(ne, nan)
    for j in range(ne):
        s2 = []
        for l in range(nlevels):
            nb = n >> l
            N = nb * int(Q[l][j]) - int(P[l][j])
            if l == 0 and N == 0:
                s2 = None
                break
            s2.append(Fraction(N, M * nb * (nb - 1)) if nb >= 2 and M >= 1 else None)
        if s2 is None or M < 1:
            continue
        for l in range(nlevels):
            if s2[l] is not None and s2[0] is not None:
                tau[l, j] = float(s2[l] / ((1 << l) * s2[0]))
        if s2[ls] is not None and s2[0] is not None:
            t = s2[ls] / ((1 << ls) * s2[0])
            ess[j] = float(Fraction(M * n) / t) if t != 0 else math.inf
            mcse[j] = math.sqrt(s2[ls] / (1 << ls) / (M * n))
    return tau, ess, mcse, ls
