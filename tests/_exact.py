"""Exactly enumerated posteriors of toy problems, and the harness that compares
the GPU sampler's chain states with them (imported only by tests/).

A toy is small enough to enumerate: every state s gets log pi(s) from the
DEFINITION of the target alone -- the oracle's forward and logL (tests/_oracle.py;
the L1 logL through mcmc.logl_picks), the prior energies (mcmc.prior_energy with
mcmc.prior_weight), a rung's beta and the noise normalisation -- in fp64 on the
CPU.  No accept rule, draw or restated move is imported here: the move rules play
no part in the reference, which is what lets these tests see a rule that is
executed faithfully and samples the wrong distribution.

Targets (by section):
  s.4   uniform box times L                      s.11/13  prior * L^beta per rung (prior, boxes untempered)
  s.14  uniform over the nodes of the box        s.15     uniform over the ladder index; statics uniform on the
  s.21  the product over the population                   zero-sum lattice |kc| <= kcmax; logL carries -norm ln lam
  s.22  uniform on k, on sets of k cells and on values    s.23     the L1 logL

Two runs per case through mcmc.Sampler's public API: *invariance* starts N chains
from exact draws of pi (Philox is keyed by the global chain, so the N final states
are N independent draws of pi if the step leaves pi invariant) and *mixing* starts
every chain in one corner state.  The final-state counts are compared with N pi by
Pearson's X^2 (states with N pi < 8 pooled, the pooled mass at most 1 % -- a
condition on the toy), p = Q(dof / 2, X^2 / 2) >= 1e-6; the same counts must
reject wrong targets (pi^0.9, the uniform distribution, and per feature the
target without that feature's term) at p <= 1e-12.

EXACT_SELFTEST=1 (read here) swaps in a wrong reference for the tempering and the
noise cases, which must then fail: a check of the harness's own sensitivity.
"""
import itertools
import math
import os
import time
import types

import numpy as np
import torch

import _oracle as O
from test_gpu_hypo import _View
from test_gpu_nuis import _eff

MIN_EXPECTED = 8.0          # states with N pi below this are pooled into one bin
POOL_CAP = 0.01             # ... whose mass may not exceed this (a condition on the toy)
P_PASS = 1e-6               # a correct sampler fails one assertion at the committed seed with this chance
P_REJECT = 1e-12            # every wrong target must be rejected at least this strongly
N_FLOOR = 65536             # chains per histogram
SELFTEST = os.environ.get("EXACT_SELFTEST") == "1"


# --- the statistic ---
def pool_bins(expected):
    """(bin of every state, number of bins, pooled share): states whose expected
    count is below MIN_EXPECTED share one last bin."""
    expected = np.asarray(expected, np.float64)
    small = expected < MIN_EXPECTED
    bins = np.cumsum(~small) - 1
    nb = int((~small).sum())
    if small.any():
        bins = np.where(small, nb, bins)
        nb += 1
    tot = float(expected.sum())
    return bins.astype(np.int64), nb, (float(expected[small].sum()) / tot if tot > 0 else 0.0)


def upper_gamma_q(a, x):
    """Q(a, x), the regularised upper incomplete gamma function, in float64."""
    return float(torch.special.gammaincc(torch.tensor(float(a), dtype=torch.float64),
                                         torch.tensor(float(x), dtype=torch.float64)))


def chi2_test(counts, q):
    """Pearson's X^2 of the state counts against sum(counts) * q (q normalised).
    Returns a namespace: x2, dof, p, pooled (share of q in the pooled bin), nbins."""
    counts = np.asarray(counts, np.float64)
    q = np.asarray(q, np.float64)
    assert counts.shape == q.shape and abs(q.sum() - 1.0) < 1e-9, (counts.shape, q.shape, q.sum())
    n = counts.sum()
    bins, nb, pooled = pool_bins(n * q)
    obs = np.bincount(bins, weights=counts, minlength=nb)
    exp = np.bincount(bins, weights=n * q, minlength=nb)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(exp > 0, (obs - exp) ** 2 / exp, np.where(obs > 0, np.inf, 0.0))
    x2 = float(terms.sum())
    dof = nb - 1
    p = upper_gamma_q(dof / 2.0, x2 / 2.0) if dof > 0 and math.isfinite(x2) else (0.0 if dof > 0 else 1.0)
    return types.SimpleNamespace(x2=x2, dof=dof, p=p, pooled=pooled, nbins=nb)


def normalise(logw):
    """exp(logw) / sum, by log-sum-exp in fp64."""
    logw = np.asarray(logw, np.float64)
    m = logw.max()
    return np.exp(logw - (m + math.log(np.exp(logw - m).sum())))


def properties(pi, n=N_FLOOR):
    """What the toys are chosen by: states, pooled share at n chains, effective
    states exp(entropy), max / min."""
    pi = np.asarray(pi, np.float64)
    nz = pi[pi > 0]
    return types.SimpleNamespace(states=pi.size, pooled=pool_bins(n * pi)[2],
                                 effective=float(np.exp(-(nz * np.log(nz)).sum())), ratio=float(pi.max() / pi.min()))


# --- toy problems ---
def toy_problem(nxyz=(8, 8, 8), nref=(8, 8, 4), nstat=3, nev=3, phases="P", var=1e-5, box=(4000, 4007),
                sbox=(2300, 2307), dvmax=3, v_true=None, vs_true=None, ev_nodes=None, seed=11, prec=32):
    """Stations on the top face, events inside, every station picks every event
    (P, or P and S); the picks are the oracle's forward of an interior model of
    the box plus N(0, var) noise.  `ev_nodes` [nev, 3] puts the events on nodes."""
    from mceik_amd import mcmc
    nx, ny, nz = nxyz
    h = 100.0
    rng = np.random.default_rng(seed)
    nph = 2 if phases == "PS" else 1
    p = mcmc.Problem(nx=nx, ny=ny, nz=nz, h=h, nref=tuple(nref), seed=seed)
    ex, ey, ez = (nx - 1) * h, (ny - 1) * h, (nz - 1) * h
    p.sx, p.sy, p.sz = rng.uniform(2 * h, ex - 2 * h, nstat), rng.uniform(2 * h, ey - 2 * h, nstat), np.full(nstat, ez)
    p.pcorr, p.scorr = np.zeros(nstat), np.zeros(nstat)
    if ev_nodes is None:
        p.ex, p.ey, p.ez = rng.uniform(h, ex - h, nev), rng.uniform(h, ey - h, nev), rng.uniform(h, ez - h, nev)
    else:
        en = np.asarray(ev_nodes, np.float64).reshape(nev, 3)
        p.ex, p.ey, p.ez = en[:, 0] * h, en[:, 1] * h, en[:, 2] * h
    p.nphase = nph
    p.vmin, p.vmax, p.dvmax = int(box[0]), int(box[1]), int(dvmax)
    p.vsmin, p.vsmax = int(sbox[0]), int(sbox[1])
    mid = lambda b: (int(b[0]) + int(b[1]) + 1) // 2  # noqa: E731
    p.v_true = np.full(p.ncell, mid(box), np.int32) if v_true is None else np.asarray(v_true, np.int32)
    if nph == 2:
        p.vs_true = np.full(p.ncell, mid(sbox), np.int32) if vs_true is None else np.asarray(vs_true, np.int32)
    per = nstat * nph
    p.obs_ptr = (np.arange(nev + 1) * per).astype(np.int32)
    p.obs_stat = np.tile(np.repeat(np.arange(nstat, dtype=np.int32), nph), nev)
    p.pick_type = np.tile(np.arange(1, nph + 1, dtype=np.int32), nev * nstat)
    p.luse = np.ones(nev * per, np.int32)
    p.var = np.full(nev * per, float(var))
    p.tobs = np.zeros(nev * per)
    P = O.make_problem(p, prec)
    vt = p.v_true if nph == 1 else np.concatenate([p.v_true, p.vs_true])
    tt = O.forward_all_f32(P, vt).astype(np.float64)                 # [nph][nstat][nev]
    # observation (e, k, ph) at e * per + k * nph + ph
    p.tobs = tt.transpose(2, 1, 0).ravel() + rng.normal(0.0, float(var), nev * per)
    return p


def _node_index(p, xyz):
    xyz = np.asarray(xyz, np.int64)
    return ((xyz[..., 2] * p.ny + xyz[..., 1]) * p.nx + xyz[..., 0]).astype(np.int32)


def statics_lattice(nstat, kcmax):
    """Every zero-sum vector of nstat integers with |kc| <= kcmax: what the
    zero-sum pair moves reach from 0."""
    out = [k for k in itertools.product(range(-kcmax, kcmax + 1), repeat=nstat) if sum(k) == 0]
    return np.array(out, np.int32)


class Toy:
    """One enumerated target.  The state is (velocity models, hypocentres, noise
    indices and statics); a feature that is off contributes one state.

    vbox     per entry of a chain's [nphase * ncell] model the admissible values (a range)
    hyp      None or (lo, hi): the node box every event moves in
    nuis     None or a namespace (lam, lnlam, dt, norm [nphase], noise, statics, kcmax)
    prior    None or (sigma_smooth, sigma_damp, vref [nphase * ncell])
    norm     the likelihood's norm: 2, or 1
    """

    def __init__(self, p, vbox=None, hyp=None, nuis=None, prior=None, prec=32, norm=2):
        from mceik_amd import mcmc
        self.p, self.prec, self.norm, self.hyp, self.nuis, self.prior = p, prec, norm, hyp, nuis, prior
        nph, ncell, nev = p.nphase, p.ncell, p.nevents
        if vbox is None:
            vbox = [range(p.vmin, p.vmax + 1)] * ncell + ([range(p.vsmin, p.vsmax + 1)] * ncell if nph == 2 else [])
        assert len(vbox) == nph * ncell
        self.vstates = np.array(list(itertools.product(*vbox)), np.int32)                 # [nV][nph * ncell]
        cat = np.stack([p.ev_node % p.nx, (p.ev_node // p.nx) % p.ny, p.ev_node // (p.nx * p.ny)], 1).astype(np.int32)
        if hyp is None:
            nodes = cat
            self.hstates = cat[None].copy()                                               # [1][nev][3]
            hsel = np.arange(nev)[None]
        else:
            lo, hi = hyp
            nodes = np.array([(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1)
                              for x in range(lo[0], hi[0] + 1)], np.int32)
            hsel = np.array(list(itertools.product(range(len(nodes)), repeat=nev)), np.int64)   # [nH][nev]
            self.hstates = nodes[hsel]
        self.hsel, self.nbox = hsel, len(nodes)
        if nuis is None:
            self.ustates = [(np.zeros(nph, np.int32), np.zeros((nph, p.nstat), np.int32))]
        else:
            kns = range(len(nuis.lam)) if nuis.noise else [len(nuis.lam) // 2]
            kcs = statics_lattice(p.nstat, nuis.kcmax) if nuis.statics else np.zeros((1, p.nstat), np.int32)
            per = [(kn, kc) for kn in kns for kc in kcs]
            self.ustates = [(np.array([a[0] for a in c], np.int32), np.array([a[1] for a in c], np.int32))
                            for c in itertools.product(per, repeat=nph)]
        nV, nH, nU = len(self.vstates), len(self.hstates), len(self.ustates)
        # tables of every model at every node the events can sit on: [nV][nph][nstat][nnodes]
        Pall = O.make_problem(_View(p, ev_node=_node_index(p, nodes), nevents=len(nodes)), prec)
        tall = np.stack([O.forward_all_f32(Pall, v) for v in self.vstates])
        self.data = np.zeros((nV, nH, nU))          # the data misfit part of logL
        self.noise = np.zeros(nU)                   # - sum_ph norm[ph] * lnlam[kn[ph]]
        for iu, (kn, kc) in enumerate(self.ustates):
            if nuis is None:
                ve, tce = np.asarray(p.var, np.float64), np.asarray(p.tcorr, np.float64)
            else:
                ve, tce = _eff(p, nuis, kn, kc)
                self.noise[iu] = -sum(float(nuis.norm[q]) * float(nuis.lnlam[kn[q]]) for q in range(nph))
            Pu = O.make_problem(_View(p, var=ve, tcorr=tce), prec)
            for ih in range(nH):
                for iv in range(nV):
                    tt = np.ascontiguousarray(tall[iv][:, :, hsel[ih]])
                    self.data[iv, ih, iu] = O.loglik(Pu, tt) if norm == 2 else mcmc.logl_picks(p, tt, ve, tce, norm=1)
        self.logprior = np.zeros(nV)
        if prior is not None:
            ss, sd, vref = prior
            ws, wd = mcmc.prior_weight(ss), mcmc.prior_weight(sd)
            for iv, v in enumerate(self.vstates):
                for q in range(nph):
                    es, ed = mcmc.prior_energy(p, v[q * ncell:(q + 1) * ncell],
                                               None if vref is None else np.asarray(vref).ravel()[q * ncell:(q + 1) * ncell])
                    self.logprior[iv] -= ws[q] * es + wd[q] * ed
        self.shape = (nV, nH, nU)
        self.nstates = nV * nH * nU
        self._vkey = {v.tobytes(): i for i, v in enumerate(self.vstates)}
        self._hkey = {h.tobytes(): i for i, h in enumerate(self.hstates)}
        self._ukey = {kn.tobytes() + kc.tobytes(): i for i, (kn, kc) in enumerate(self.ustates)}

    def log_target(self, beta=1.0, prior=True, noise=True, temper_prior=False, swap_events=None):
        """Unnormalised log pi of every state, flat over (V, H, U).  The keywords
        other than beta build the WRONG targets of the power controls."""
        data = self.data
        if swap_events is not None:                 # two events' marginals exchanged: pi'(.., a, .., b, ..) = pi(.., b, .., a, ..)
            a, b = swap_events
            sel = self.hsel.copy()
            sel[:, [a, b]] = sel[:, [b, a]]
            data = data[:, np.ravel_multi_index(tuple(sel.T), (self.nbox,) * sel.shape[1]), :]
        logl = data + (self.noise[None, None, :] if noise else 0.0)
        lp = self.logprior[:, None, None] if prior else 0.0
        return ((beta * (logl + lp)) if temper_prior else (beta * logl + lp)).ravel()

    def target(self, **kw):
        return normalise(self.log_target(**kw))

    def index(self, v, xyz=None, kn=None, kc=None):
        """Flat state index of every chain: v [n][...], xyz [n][nev][3], kn [n][nph], kc [n][nph][nstat]."""
        n = len(v)
        v = np.ascontiguousarray(v, np.int32).reshape(n, -1)
        iv = np.array([self._vkey[r.tobytes()] for r in v])
        ih = np.zeros(n, np.int64) if xyz is None else \
            np.array([self._hkey[np.ascontiguousarray(r, np.int32).tobytes()] for r in xyz])
        iu = np.zeros(n, np.int64) if kn is None else \
            np.array([self._ukey[np.ascontiguousarray(a, np.int32).tobytes() + np.ascontiguousarray(b, np.int32).tobytes()]
                      for a, b in zip(kn, kc)])
        return (iv * self.shape[1] + ih) * self.shape[2] + iu

    def states(self, idx):
        """(v [n][nph * ncell], xyz [n][nev][3], kn [n][nph], kc [n][nph][nstat]) of flat indices."""
        iv, ih, iu = np.unravel_index(np.asarray(idx, np.int64), self.shape)
        return (self.vstates[iv], self.hstates[ih], np.stack([self.ustates[i][0] for i in iu]),
                np.stack([self.ustates[i][1] for i in iu]))


class VorToy:
    """Voronoi-cell models of one phase: a state is a set of
    kmin <= k <= kmax (cell, value) pairs in distinct cells, pi = L(raster) /
    (K C(ncell, k) nv^k)."""

    def __init__(self, p, kmin, kmax, metric=(1, 1, 1)):
        from mceik_amd import mcmc
        assert p.nphase == 1
        self.p, self.kmin, self.kmax = p, kmin, kmax
        vals = range(p.vmin, p.vmax + 1)
        self.sets = []
        for k in range(kmin, kmax + 1):
            for cells in itertools.combinations(range(p.ncell), k):
                for w in itertools.product(vals, repeat=k):
                    self.sets.append((cells, w))
        self._key = {s: i for i, s in enumerate(self.sets)}
        P = O.make_problem(p)
        self.data = np.array([O.loglik(P, O.forward_all_f32(P, mcmc.vor_raster(p, c, w, metric))) for c, w in self.sets])
        nv = len(vals)
        self.logcomb = np.array([-math.log(math.comb(p.ncell, len(c))) for c, _ in self.sets])
        self.logvals = np.array([-len(c) * math.log(nv) for c, _ in self.sets])
        self.nstates = len(self.sets)
        self.shape = (self.nstates,)

    def log_target(self, beta=1.0, comb=True, **_):
        return beta * self.data + self.logvals + (self.logcomb if comb else 0.0)

    def target(self, **kw):
        return normalise(self.log_target(**kw))

    def index(self, cells, vals, counts):
        out = []
        for c, w, k in zip(cells.reshape(len(cells), -1), vals.reshape(len(vals), -1), counts.ravel()):
            o = np.argsort(c[:k])
            out.append(self._key[(tuple(int(x) for x in c[:k][o]), tuple(int(x) for x in w[:k][o]))])
        return np.array(out)

    def nuclei(self, idx):
        """(cells, vals [n][1][kmax], counts [n][1]) of flat indices; unused slots hold a free cell and vmin."""
        n = len(idx)
        c, w, k = np.zeros((n, 1, self.kmax), np.int32), np.full((n, 1, self.kmax), self.p.vmin, np.int32), \
            np.zeros((n, 1), np.int32)
        for r, i in enumerate(idx):
            cells, vals = self.sets[int(i)]
            k[r, 0] = len(cells)
            rest = [x for x in range(self.p.ncell) if x not in cells]
            c[r, 0] = (list(cells) + rest)[:self.kmax]
            w[r, 0, :len(vals)] = vals
        return c, w, k


# --- the cases ---
_PATHS = {"per_step": {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, "two_pipes": {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"},
          "multi_step": {"MCEIK_PERSIST": "1"}}


def _ladder(nk, lam_max):
    from mceik_amd import mcmc
    return mcmc.nuis_ladder(nk, 1.0 / lam_max, lam_max)


def _nu(p, nk, lam_max, dt, kcmax, every, offset=0, nsub=4, noise=True, statics=True):
    lam, lnlam = _ladder(nk, lam_max) if noise else (np.ones(1), np.zeros(1))
    used = p.obs_mask == 0
    norm = np.array([float((used & (p.obs_phase == q)).sum()) for q in range(p.nphase)])
    return types.SimpleNamespace(lam=lam, lnlam=lnlam, dt=dt if statics else 0.0, kcmax=kcmax if statics else 0,
                                 norm=norm, noise=noise, statics=statics, every=every, offset=offset, nsub=nsub)


def _case(toy, path="per_step", K=0, K_first=0, K_inv=None, N=N_FLOOR, kernel=None, betas=None, **kw):
    """K_first: the smallest K (by doubling from 4) at which the corner start
    first passed on an MI355X.  The mixing run takes K = 4 K_first steps; where
    that would run past about 10 s it takes 2 K_first, and K_first itself in the
    two cases whose step costs most (joint: three rungs of three kinds of step;
    lang: two forwards and two adjoint batches a step).  The invariance run needs
    no mixing and takes K_inv <= K_first (DESIGN.md s.24's table has every number)."""
    return types.SimpleNamespace(toy=toy, path=path, K=K, K_first=K_first, K_inv=K_first if K_inv is None else K_inv,
                                 N=N, kernel=kernel, betas=betas,
                                 block=kw.pop("block", None), lang=kw.pop("lang", None), de=kw.pop("de", None),
                                 vor=kw.pop("vor", None), hyp_every=kw.pop("hyp_every", 0),
                                 hyp_dmax=kw.pop("hyp_dmax", (1, 1, 1)), **kw)


HYP_BOX = ((0, 2, 3), (2, 4, 4))            # 3 x 3 x 2 nodes; x = 0 is the grid's edge


def _single(dvmax=3, **kw):
    return Toy(toy_problem(dvmax=dvmax), **kw)


def _build(name):
    # K_first, K (mixing) and K_inv as measured on an MI355X: `_case`; var, the ladders and dt were chosen on the CPU
    # for the properties tests/test_exact_host.py asserts (a flat toy has no power, a sharp one pools too much)
    if name == "single":                      # 1: single cell, P, fp32, one launch per step
        return _case(_single(), "per_step", K=128, K_first=32)
    if name == "single_wide":                  # 1: dvmax 10 > the box's width 7: 13 of 20 proposals leave the box
        return _case(_single(dvmax=10), "per_step", K=256, K_first=64)
    if name == "multi_step":                   # 2: the multi-step launch needs the 16-z kernel: nz >= 25, nrz = 4
        p = toy_problem(nxyz=(8, 8, 25), nref=(8, 8, 4), box=(4000, 4001), dvmax=1, var=1e-6, seed=12)
        return _case(Toy(p), "multi_step", K=128, K_first=64, K_inv=32, kernel="fsm16_solve_kernel")
    if name == "ps":                           # 3: P and S, two pipes, 2 + 2 cells x 3 values
        p = toy_problem(phases="PS", box=(4000, 4002), sbox=(2300, 2302), dvmax=3, var=1.2e-4, seed=13)
        return _case(Toy(p), "two_pipes", K=256, K_first=64)
    if name == "fp64":                         # 4: precision 64, the target from the fp64 forward
        return _case(Toy(toy_problem(prec=64), prec=64), "per_step", K=128, K_first=32)
    if name == "block_prior":                  # 5: radii 0..1, both prior terms, 2 x 2 x 1 cells x 4 values
        p = toy_problem(nref=(4, 4, 8), box=(4000, 4003), dvmax=2, var=2e-5, seed=15)
        prior = (3.0, 4.0, np.array([4001, 4002, 4001, 4002], np.int32))
        return _case(Toy(p, prior=prior), "per_step", K=128, K_first=64, K_inv=32, block=(0, 1))
    if name == "temper":                       # 6: 3 rungs, swaps before every step, prior on
        p = toy_problem(dvmax=5)
        prior = (3.0, 4.0, np.array([4003, 4004], np.int32))
        return _case(Toy(p, prior=prior), "per_step", K=64, K_first=32, N=3 * N_FLOOR, betas=np.array([1.0, 0.5, 0.2]))
    if name in ("hypo", "hypo_l1"):            # 7 (10: under L1): 2 events, 3 x 3 x 2 nodes, one velocity value
        p = toy_problem(nref=(8, 8, 8), nev=2, box=(4000, 4000), dvmax=1, var=4e-3,
                        ev_nodes=[(1, 3, 3), (2, 2, 4)], seed=17)
        return _case(Toy(p, hyp=HYP_BOX, norm=1 if name == "hypo_l1" else 2), "per_step", K=128, K_first=32, hyp_every=1)
    if name == "nuis":                         # 8: PS, ladder of 5, statics |kc| <= 1, every step a nuisance step
        p = toy_problem(nref=(8, 8, 8), phases="PS", box=(4000, 4000), sbox=(2300, 2300), dvmax=1, var=1e-3, seed=18)
        return _case(Toy(p, nuis=_nu(p, 5, 1.3, 3e-4, 1, every=1)), "per_step", K=64, K_first=32, K_inv=16, N=4 * N_FLOOR)
    if name == "joint":                        # 9: velocity, hypocentre and nuisance steps in turn, 3 rungs
        p = toy_problem(nref=(8, 8, 8), nev=1, box=(4000, 4002), dvmax=2, var=5e-3, ev_nodes=[(1, 1, 3)], seed=19)
        nu = _nu(p, 3, 1.6, 4e-3, 1, every=3, offset=1)
        return _case(Toy(p, hyp=((0, 0, 3), (1, 1, 4)), nuis=nu), "per_step", K=64, K_first=64, K_inv=16, N=3 * N_FLOOR,
                     betas=np.array([1.0, 0.75, 0.55]), hyp_every=3)
    if name == "single_l1":                    # 10: case 1 under the Laplace likelihood
        return _case(_single(norm=1), "per_step", K=128, K_first=32)
    if name == "lang":                         # 11: Langevin and single-cell steps in turn, 2 cells x 5 values
        p = toy_problem(box=(4000, 4004), dvmax=2, var=7e-6, seed=21)
        return _case(Toy(p), "per_step", K=16, K_first=16, K_inv=4, lang=dict(every=2, offset=1, sigma=2.0, dmax=4))
    if name == "de":                           # 11: DE and single-cell steps in turn, the chains one population
        return _case(_single(), "per_step", K=256, K_first=64, de=dict(every=2, offset=1, gamma=1.0, cr=1.0))
    if name == "vor":                          # 11: 4 cells, 1 <= k <= 2, 3 values: 66 states
        p = toy_problem(nref=(4, 4, 8), box=(4000, 4002), dvmax=2, var=2e-5, seed=23)
        return _case(VorToy(p, 1, 2), "per_step", K=128, K_first=64, K_inv=32, vor=dict(kmin=1, kmax=2, dv=2, dmax=(1, 1, 1)))
    raise KeyError(name)


CASES = ("single", "single_wide", "multi_step", "ps", "fp64", "block_prior", "temper", "hypo", "nuis", "joint",
         "single_l1", "hypo_l1", "lang", "de", "vor")
_BUILT = {}


def case(name):
    if name not in _BUILT:
        _BUILT[name] = _build(name)
    return _BUILT[name]


def rung_targets(cs):
    """The exact target of every rung ([1] without tempering)."""
    return [cs.toy.target(beta=float(b)) for b in (cs.betas if cs.betas is not None else [1.0])]


def controls(cs, rung=0):
    """{name: wrong target} that the histogram of `rung` must reject."""
    toy = cs.toy
    beta = float(cs.betas[rung]) if cs.betas is not None else 1.0
    pi = toy.target(beta=beta)
    out = {"pi^0.9": normalise(0.9 * np.log(pi)), "uniform": np.full(pi.size, 1.0 / pi.size)}
    if getattr(toy, "prior", None) is not None:
        out["no prior"] = toy.target(beta=beta, prior=False)
    if cs.betas is not None:
        for r in (rung - 1, rung + 1):
            if 0 <= r < len(cs.betas):
                out[f"rung {r}"] = toy.target(beta=float(cs.betas[r]))
        if getattr(toy, "prior", None) is not None and beta != 1.0:
            out["prior tempered"] = toy.target(beta=beta, temper_prior=True)
    if getattr(toy, "nuis", None) is not None and toy.nuis.noise:
        out["no noise term"] = toy.target(beta=beta, noise=False)
    if getattr(toy, "hyp", None) is not None and toy.p.nevents >= 2:
        out["events exchanged"] = toy.target(beta=beta, swap_events=(0, 1))
    if isinstance(toy, VorToy):
        out["no 1/C(ncell,k)"] = toy.target(beta=beta, comb=False)
    return out


def reference(cs, name, rung=0):
    """The target a rung's histogram is held against: the exact one, unless
    EXACT_SELFTEST=1 asks for a wrong one where the tests must then fail."""
    if SELFTEST and name == "temper" and rung == 1:
        return cs.toy.target(beta=float(cs.betas[0]))
    if SELFTEST and name == "nuis":
        return cs.toy.target(noise=False)
    return rung_targets(cs)[rung]


def draw_states(pi, n, seed):
    return np.random.default_rng(seed).choice(pi.size, size=n, p=pi)


def check(name, cs, counts_by_rung, what):
    """Asserts the statistic and the power controls on every rung's counts;
    prints every figure first.  Returns the lines printed."""
    lines = []
    fails = []
    for r, counts in enumerate(counts_by_rung):
        pi = reference(cs, name, r)
        exact = rung_targets(cs)[r]
        t = chi2_test(counts, pi)
        cap = pool_bins(counts.sum() * exact)[2]
        lines.append(f"{name} {what} rung {r}: N {int(counts.sum())} K {cs.K_inv if what == 'invariance' else cs.K} "
                     f"(first pass {cs.K_first}) states {pi.size} "
                     f"X2 {t.x2:.1f} dof {t.dof} p {t.p:.3e} pooled {cap:.2e}")
        if cap > POOL_CAP:
            fails.append(f"rung {r}: pooled mass {cap:.3e} > {POOL_CAP}")
        if not t.p >= P_PASS:
            fails.append(f"rung {r}: p {t.p:.3e} < {P_PASS} against the exact target")
        for cname, q in controls(cs, r).items():
            tc = chi2_test(counts, q)
            lines.append(f"    control {cname}: X2 {tc.x2:.1f} dof {tc.dof} p {tc.p:.3e}")
            if not tc.p <= P_REJECT:
                fails.append(f"rung {r}: control '{cname}' not rejected, p {tc.p:.3e}")
    print("\n".join(lines))
    assert not fails, (name, what, fails)
    return lines


# --- the GPU run ---
def set_path(cs, monkeypatch):
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in _PATHS[cs.path].items():
        monkeypatch.setenv(k, val)


def run_gpu(name, cs, mode, chain_offset=0, K=None, max_chains=1 << 18):
    """The final-state counts per rung of one run of the real sampler, and the
    accept counters {move: array}.  mode: 'invariance' (starts drawn from every
    rung's exact target) or 'mixing' (every chain in the corner state 0).  A
    sampler takes at most max_chains; more run as several with disjoint global
    chain ids."""
    from mceik_amd import mcmc
    toy, p = cs.toy, cs.toy.p
    if K is None:
        K = cs.K_inv if mode == "invariance" else cs.K
    if mode == "mixing":
        chain_offset += cs.N                 # other global chains than the invariance run's: two independent tests
    nt = len(cs.betas) if cs.betas is not None else 1
    G = cs.N // nt
    targets = rung_targets(cs)
    counts = [np.zeros(toy.nstates, np.int64) for _ in range(nt)]
    stats = {}

    def add(key, a):
        stats[key] = stats.get(key, 0) + np.asarray(a, np.int64)

    parts = max(1, -(-cs.N // max_chains))
    g = G // parts
    assert g * parts == G, (G, parts)
    wall = 0.0
    for part in range(parts):
        off = chain_offset + part * g * nt
        if mode == "invariance":
            idx = np.concatenate([draw_states(targets[r], g, [20261021, off, r]) for r in range(nt)])
        else:
            idx = np.zeros(g * nt, np.int64)
        vor = isinstance(toy, VorToy)
        if vor:
            nuc = toy.nuclei(idx)
            v0 = np.stack([mcmc.vor_raster(p, toy.sets[int(i)][0], toy.sets[int(i)][1]) for i in np.unique(idx)])
            v0 = v0[np.searchsorted(np.unique(idx), idx)]
        else:
            v0, xyz0, kn0, kc0 = toy.states(idx)
        v0 = np.ascontiguousarray(v0, np.int32).reshape((g * nt,) + ((p.nphase, p.ncell) if p.nphase > 1 else (p.ncell,)))
        smp = mcmc.Sampler(p, g * nt, chain_offset=off, v0=v0, precision=toy.prec if not vor else 32)
        try:
            if cs.betas is not None:
                smp.temper_enable(betas=cs.betas, swap_every=1)
            if not vor and toy.prior is not None:
                ss, sd, vref = toy.prior
                smp.prior_enable(sigma_smooth=ss, sigma_damp=sd,
                                 vref=np.asarray(vref, np.int32).reshape(smp.model_shape[1:]))
            if cs.block is not None:
                smp.block_enable(*cs.block)
            if not vor and toy.norm == 1:
                smp.likelihood_set(1)
            if not vor and toy.hyp is not None:
                smp.hypo_enable(cs.hyp_every, dmax=cs.hyp_dmax, box=toy.hyp)
                smp.hypo_set(xyz0)
            if not vor and toy.nuis is not None:
                nu = toy.nuis
                smp.nuis_enable(nu.every, offset=nu.offset, nsub=nu.nsub, ladder=(nu.lam, nu.lnlam) if nu.noise else None,
                                statics_dt=nu.dt if nu.statics else None, kcmax=nu.kcmax)
                smp.nuis_set(kn0, kc0)
            if cs.lang is not None:
                smp.lang_enable(**cs.lang)
            if cs.de is not None:
                smp.de_enable(**cs.de)
            if vor:
                smp.vor_enable(nuclei=nuc, **cs.vor)
            info = smp.info()
            # every feature but tempering makes each step a launch of its own
            plain = not (cs.block or cs.lang or cs.de or vor) and toy.prior is None and toy.hyp is None and \
                toy.nuis is None and toy.norm == 2
            assert bool(info["multi_step"]) == (cs.path == "multi_step" and plain), info
            if cs.path != "multi_step":
                assert info["npipe"] == (2 if cs.path == "two_pipes" else 1), info
            if cs.kernel is not None:
                assert cs.kernel in info["kernel"], info
            smp.sync()
            t0 = time.perf_counter()
            smp.run(K)
            smp.sync()
            wall += time.perf_counter() - t0
            v, _, nacc, step = smp.state()
            assert step == K, step
            if vor:
                fin = toy.index(*smp.vor_get())
                st = smp.vor_stats()
                for t in mcmc.VOR_TYPES:
                    add("vor " + t, [st[t]["accepts"]])
            else:
                fin = toy.index(v, smp.hypo_positions() if toy.hyp is not None else None,
                                *(smp.nuis_get() if toy.nuis is not None else (None, None)))
                if len(toy.vstates) > 1:
                    add("velocity", [nacc.sum()])
            if cs.betas is not None:
                add("swap", smp.temper_stats()[1])
            if cs.block is not None:
                add("block", smp.block_stats()[1])
            if not vor and toy.hyp is not None:
                add("hypo", smp.hypo_stats()[1])
            if not vor and toy.nuis is not None:
                add("nuis", smp.nuis_stats()[1])
            if cs.lang is not None:
                add("lang", [smp.lang_stats()["accepts"]])
            if cs.de is not None:
                add("de", [smp.de_stats()["accepts"]])
        finally:
            smp.close()
        for r in range(nt):
            counts[r] += np.bincount(fin[r * g:(r + 1) * g], minlength=toy.nstates)
    return counts, stats, wall
