"""Noise-scale and station-static moves on the GPU (csrc/nuis.hip, include/mceik.h
mceik_mcmc_nuis_*), the rule restated here in Python and compared
bit for bit.

Every chain carries a ladder index kn[ph] per phase and a static kc[ph][station]
in units of dt.  Its effective observations and logL are

    var_eff[j]   = var[j] * lam[kn[ph(j)]]
    tcorr_eff[j] = tcorr[j] + float(kc[ph(j)][stat(j)]) * dt
    logL         = (((0 - obj_0) - obj_1) ...) - norm[0] * lnlam[kn[0]] (- norm[1] * lnlam[kn[1]])

with the obj sum the oracle's logL on a view of the problem whose var / tcorr are
the effective arrays, on the oracle's CPU tables of the chain's models.  Global
step gs is a nuisance step iff gs % every == offset (and it is no hypocentre
step): nsub sub-moves per chain, sub-move `sub` of global chain gid drawing
Philox4x32-10 with counter {gs lo, gs hi, 3, sub} and key {gid, seed} as
tests/test_nuis_host.py restates it.  Every other step is the velocity step of
tests/test_gpu_prior.py (block footprint, prior threshold; both off: the plain
single-cell step) or the hypocentre step of tests/test_gpu_hypo.py, with logL
by the three lines above; the swap rule is tests/test_gpu_temper.py's, the
values travelling with the models.

The picks are analytic, so the restatement runs without a GPU: seeds, nsub, dt
and the ladder were chosen that way, and every restated test asserts on the
restatement the events it is there for.
"""
import types

import numpy as np
import pytest

import _oracle as O
import test_gpu_hypo as TH
import test_gpu_prior as TP
from test_nuis_host import restated_draw

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LADDER3 = TH.LADDER3
NCH = 4


def _nu(p, every=2, offset=1, nsub=6, nk=9, lam_max=4.0, dk=2, dt=0.004, dc=3, kcmax=5, noise=True, statics=True,
        norm=None):
    """The options of one case, with what the restatement derives from them."""
    from mceik_amd import mcmc
    lam, lnlam = mcmc.nuis_ladder(nk, 1.0 / lam_max, lam_max) if noise else (np.ones(1), np.zeros(1))
    act = mcmc.nuis_active(p)
    used = p.obs_mask == 0
    nm = np.array([float((used & (p.obs_phase == q)).sum()) for q in range(p.nphase)]) if norm is None \
        else np.asarray(norm, np.float64)
    return types.SimpleNamespace(every=every, offset=offset, nsub=nsub, lam=lam, lnlam=lnlam, dk=dk, dc=dc,
                                 kcmax=kcmax if statics else 0, dt=dt if statics else 0.0, noise=noise, statics=statics,
                                 norm=nm, norm_opt=norm, act=act,
                                 nact=[len(a) if statics and len(a) >= 2 else 0 for a in act])


def _enable(smp, nu, **kw):
    o = dict(every=nu.every, offset=nu.offset, nsub=nu.nsub, dk=nu.dk, dc=nu.dc, kcmax=nu.kcmax, norm=nu.norm_opt,
             ladder=(nu.lam, nu.lnlam) if nu.noise else None, statics_dt=nu.dt if nu.statics else None)
    o.update(kw)
    smp.nuis_enable(**o)


def _eff(p, nu, kn, kc):
    ph, st = p.obs_phase, np.where(p.obs_mask == 0, p.obs_stat, 0)
    return (np.asarray(p.var, np.float64) * nu.lam[kn[ph]],
            np.asarray(p.tcorr, np.float64) + kc[ph, st].astype(np.float64) * nu.dt)


def _norm(p, nu, kn, ln):
    ln = ln - nu.norm[0] * nu.lnlam[kn[0]]
    if p.nphase > 1:
        ln = ln - nu.norm[1] * nu.lnlam[kn[1]]
    return ln


def _view(p, nu, kn, kc, nodes, prec):
    ve, tce = _eff(p, nu, kn, kc)
    return O.make_problem(TH._View(p, var=ve, tcorr=tce, ev_node=np.ascontiguousarray(nodes, np.int32)), prec)


def _logl(p, nu, kn, kc, tt, nodes, prec=32):
    return _norm(p, nu, kn, O.loglik(_view(p, nu, kn, kc, nodes, prec), tt))


def _start(p, nch, off, prec=32):
    """Start models and logL without a GPU (the start values leave every logL the plain sampler's)."""
    return TH._start(p, nch, off, prec)


def _restate(p, nu, v0, logl0, off, nsteps, hyp=None, block=None, prior=None, betas=None, swap_every=0, step0=0,
             prec=32, kn0=None, kc0=None, xyz0=None):
    """Runs the chains on the CPU.  nu: _nu(...) or a namespace with every = 0 (the values held, no nuisance
    steps).  hyp: None or (every, dmax, lo, hi); block: None or (rmin, rmax); prior: None or (ws, wd).  Returns a
    namespace: v, logl, kn, kc, xyz, naccept, accept [nsteps, nch], nsteps_rec {step index: (rec, rlogl)}, att /
    acc per parameter, the moments, subs (one record per sub-move) and vsteps (one per velocity proposal)."""
    from mceik_amd import mcmc
    nch, nev, nph, nst, ncell = len(v0), p.nevents, p.nphase, p.nstat, p.ncell
    v = v0.reshape(nch, -1).copy()
    logl = logl0.copy()
    kn = np.full((nch, nph), len(nu.lam) // 2, np.int32) if kn0 is None else kn0.copy()
    kc = np.zeros((nch, nph, nst), np.int32) if kc0 is None else kc0.copy()
    xyz = TH._catalogue_xyz(p, nch) if xyz0 is None else np.asarray(xyz0, np.int32).copy()
    nacc = np.zeros(nch, np.int64)
    nt = len(betas) if betas is not None else 1
    G = nch // nt
    flags = np.zeros((nsteps, nch), np.uint8)
    npar = nph * (1 + nst)
    att, acc = np.zeros(npar, np.int64), np.zeros(npar, np.int64)
    mom = types.SimpleNamespace(n=0, ksum=np.zeros((nph, 2), np.int64), hist=np.zeros((nph, len(nu.lam)), np.int64),
                                csum=np.zeros((nph, nst, 2), np.int64))
    ws, wd = prior if prior is not None else ((0.0, 0.0), (0.0, 0.0))
    bounds = [(p.vmin, p.vmax), (p.vsmin, p.vsmax)]
    nnoise = nph if nu.noise else 0
    recs, subs, vsteps, swaps = {}, [], [], []
    changed = np.zeros(nch, bool)             # the chain's values differ from the start values
    for i, gs in enumerate(range(step0, step0 + nsteps)):
        if nt > 1 and swap_every > 0 and gs > 0 and gs % swap_every == 0:
            for r in range((gs // swap_every) & 1, nt - 1, 2):
                for g in range(G):
                    a, b = r * G + g, (r + 1) * G + g
                    if TH._swap_logu(p.seed, gs, off + a) < (betas[r] - betas[r + 1]) * (logl[b] - logl[a]):
                        if (kn[a] != kn[b]).any() or (kc[a] != kc[b]).any():
                            swaps.append((i, a, b))
                        for arr in (v, logl, kn, kc, xyz, changed):
                            arr[[a, b]] = arr[[b, a]]
        beta = (lambda c: betas[c // G]) if nt > 1 else (lambda c: None)
        hstep = hyp is not None and hyp[0] > 0 and gs % hyp[0] == hyp[0] - 1
        if hstep:
            _, dmax, lo, hi = hyp
            for c in range(nch):
                ve, tce = _eff(p, nu, kn[c], kc[c])
                one = [O.make_problem(TH._View(p, nevents=1, obs_ptr=np.ascontiguousarray(p.obs_ptr[e:e + 2]),
                                               ev_node=np.zeros(1, np.int32), var=ve, tcorr=tce), prec)
                       for e in range(nev)]
                cand, logu, inside = np.zeros((nev, 3), np.int32), np.zeros(nev), np.zeros(nev, bool)
                for e in range(nev):
                    d, logu[e] = TH._hdraw(p.seed, off + c, gs, e, dmax)
                    cand[e] = xyz[c, e] + d
                    inside[e] = all(lo[a] <= cand[e, a] <= hi[a] for a in range(3))
                cur = TH._nodes(p, xyz[c])
                P2 = TH._at(p, np.concatenate([cur, np.where(inside, TH._nodes(p, cand), cur)]), prec)
                tt = O.forward_all_f32(P2, v[c])
                ln = 0.0
                for e in range(nev):
                    oc = 0.0 - O.loglik(one[e], tt[:, :, e:e + 1])
                    od = 0.0 - O.loglik(one[e], tt[:, :, nev + e:nev + e + 1])
                    a = bool(inside[e]) and (logu[e] < beta(c) * (oc - od) if nt > 1 else logu[e] < oc - od)
                    ln = ln - (od if a else oc)
                    if a:
                        xyz[c, e] = cand[e]
                logl[c] = _norm(p, nu, kn[c], ln)
        elif nu.every > 0 and gs % nu.every == nu.offset:
            rec, rl = np.zeros((nch, nu.nsub, 4), np.int32), np.zeros((nch, nu.nsub, 2))
            for c in range(nch):
                nodes = TH._nodes(p, xyz[c])
                tt = O.forward_all_f32(TH._at(p, nodes, prec), v[c])          # the chain's current tables
                for sub in range(nu.nsub):
                    (kind, ph, a, b, delta), logu = restated_draw(p.seed, off + c, gs, sub, nnoise, nu.nact, nu.dk, nu.dc)
                    ckn, ckc = kn[c].copy(), kc[c].copy()
                    if kind == 0:
                        ckn[ph] += delta
                        inside = 0 <= ckn[ph] < len(nu.lam)
                        par, partner, cand = ph, -1, int(ckn[ph])
                    else:
                        sa, sb = int(nu.act[ph][a]), int(nu.act[ph][b])
                        ckc[ph, sa] += delta
                        ckc[ph, sb] -= delta
                        inside = abs(int(ckc[ph, sa])) <= nu.kcmax and abs(int(ckc[ph, sb])) <= nu.kcmax
                        par, partner, cand = nph + ph * nst + sa, nph + ph * nst + sb, int(ckc[ph, sa])
                    ln, ok = logl[c], False
                    if inside:
                        ln = _logl(p, nu, ckn, ckc, tt, nodes, prec)
                        d = ln - logl[c]
                        ok = bool(logu < beta(c) * d) if nt > 1 else bool(logu < d)
                    rec[c, sub] = par, partner, cand, ok
                    rl[c, sub] = logl[c], ln
                    for q in (par,) + ((partner,) if partner >= 0 else ()):
                        att[q] += 1
                        acc[q] += ok
                    subs.append(types.SimpleNamespace(step=i, chain=c, kind=kind, inside=inside, acc=ok,
                                                      by_logu=ok and ln - logl[c] < 0.0))
                    if ok:
                        kn[c], kc[c], logl[c] = ckn, ckc, ln
                        changed[c] = True
            recs[i] = (rec, rl)
        else:
            for c in range(nch):
                nodes = TH._nodes(p, xyz[c])
                cell, amp, R, logu = TP._draw(p, off + c, gs, block)
                ph, cc = divmod(cell, ncell)
                cells, dv = mcmc.block_footprint(p, cc, R, amp)
                idx = ph * ncell + cells.astype(np.int64)
                vp = v[c].copy()
                vp[idx] += dv
                inp = bool(((vp[idx] >= bounds[ph][0]) & (vp[idx] <= bounds[ph][1])).all())
                a = False
                if inp:
                    thr = logu
                    if prior is not None:
                        sl = slice(ph * ncell, (ph + 1) * ncell)
                        e0, e1 = TP._energy(p, v[c][sl]), TP._energy(p, vp[sl])
                        thr = logu - (-(ws[ph] * float(e1[0] - e0[0]) + wd[ph] * float(e1[1] - e0[1])))
                    ln = _logl(p, nu, kn[c], kc[c], O.forward_all_f32(TH._at(p, nodes, prec), vp), nodes, prec)
                    d = ln - logl[c]
                    a = bool(thr < beta(c) * d) if nt > 1 else bool(thr < d)
                    if a:
                        v[c], logl[c], nacc[c] = vp, ln, nacc[c] + 1
                flags[i, c] = a
                vsteps.append(types.SimpleNamespace(step=i, chain=c, inp=inp, acc=a, changed=bool(changed[c])))
        if nu.every > 0 and gs >= p.nburn and (gs - p.nburn) % p.keepk == 0:
            mom.n += G
            k = kn[:G].astype(np.int64)
            mom.ksum[:, 0] += k.sum(0)
            mom.ksum[:, 1] += (k * k).sum(0)
            for ph in range(nph):
                mom.hist[ph] += np.bincount(k[:, ph], minlength=len(nu.lam))
            q = kc[:G].astype(np.int64)
            mom.csum[..., 0] += q.sum(0)
            mom.csum[..., 1] += (q * q).sum(0)
    return types.SimpleNamespace(v=v.reshape(v0.shape), logl=logl, kn=kn, kc=kc, xyz=xyz, naccept=nacc, accept=flags,
                                 recs=recs, att=att, acc=acc, mom=mom, subs=subs, vsteps=vsteps, swaps=swaps)


def _assert_events(r, nu):
    """An accepted and a rejected sub-move of each kind, and a velocity step accepted after a value changed."""
    for kind, on in ((0, nu.noise), (1, nu.statics)):
        if on:
            s = [x for x in r.subs if x.kind == kind]
            assert any(x.acc for x in s), ("no accepted sub-move of kind", kind)
            assert any(x.inside and not x.acc for x in s), ("no rejected sub-move of kind", kind)
    assert any(s.changed and s.acc for s in r.vsteps), "no velocity step accepted after a nuisance value changed"


def _run_gpu(smp, nsteps):
    """Steps one by one: the accept flags and the record of every nuisance step."""
    flags, recs = [], {}
    for i in range(nsteps):
        step = smp.state()[3]
        smp.run(1)
        flags.append(smp.last()[2].copy())
        if smp._nuis and smp._nuis["every"] and step % smp._nuis["every"] == smp._nuis["offset"]:
            recs[i] = smp.nuis_last()
    return np.array(flags), recs


def _compare(smp, r, flags, recs, what):
    v, l, nacc, _ = smp.state()
    kn, kc = smp.nuis_get()
    TH._same((v, l, nacc, kn, kc, flags), (r.v, r.logl, r.naccept, r.kn, r.kc, r.accept), what)
    assert sorted(recs) == sorted(r.recs), what
    for i in recs:
        TH._same(recs[i], r.recs[i], (what, "nuis_last", i))
    att, acc = smp.nuis_stats()
    TH._same((att, acc), (r.att, r.acc), (what, "stats"))


def _moments(smp):
    m = smp.nuis_moments()
    return m["n"], m["ksum"], m["hist"], m["csum"]


def _recomputed_logl(smp):
    ck = smp.checkpoint()
    smp.restore(ck, recompute_logl=True)
    return ck["logl"], smp.state()[1]


# --- 1. the restated run ---
_CASES = {
    "P-per_step": dict(path="per_step", phases="P", precision=32),
    "PS-two_pipes": dict(path="two_pipes", phases="PS", precision=32),
    "P-fp64": dict(path="per_step", phases="P", precision=64),
    # the same run with the travel times read from the tables at every use, not staged in LDS (8 nev + 4 nstat
    # = 64 B fit the 100 B this allows, the 96 B of the 24 observations' times do not)
    "P-no_lds": dict(path="per_step", phases="P", precision=32, lds="100"),
}
NSTEPS = 8


@pytest.mark.parametrize("case", list(_CASES))
def test_restated_run(case, monkeypatch):
    k = _CASES[case]
    n = TH._set_path(k["path"], monkeypatch)
    monkeypatch.delenv("MCEIK_NUIS_LDS", raising=False)
    if "lds" in k:
        monkeypatch.setenv("MCEIK_NUIS_LDS", k["lds"])
    p = TH._problem(k["phases"], n=n, seed=11)
    assert int(p.obs_ptr[-1]) == 24 * p.nphase
    nu = _nu(p)
    v0, _, l0 = _start(p, NCH, 0, k["precision"])
    r = _restate(p, nu, v0, l0, 0, NSTEPS, prec=k["precision"])
    _assert_events(r, nu)
    assert any(not s.inside for s in r.subs), "no candidate outside a box"
    TH._dev()
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=NCH, precision=k["precision"])
    try:
        assert smp.info()["npipe"] == (2 if k["path"] == "two_pipes" else 1)
        TH._same((smp.state()[1],), (l0,), "start")
        _enable(smp, nu)
        TH._same((smp.state()[1],), (l0,), "enable leaves logL")
        flags, recs = _run_gpu(smp, NSTEPS)
        _compare(smp, r, flags, recs, case)
    finally:
        smp.close()


# --- 2. a nuisance step runs no eikonal solve ---
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_no_solve(phases, monkeypatch):
    TH._set_path("per_step", monkeypatch)
    TH._dev()
    from mceik_amd import mcmc
    p = TH._problem(phases, seed=11)
    smp = mcmc.Sampler(p, nchains=NCH)
    try:
        s0 = smp.fsm_solves()
        _enable(smp, _nu(p))
        assert smp.fsm_solves() == s0                 # the enable's forward is not counted
        smp.run(1)                                      # step 0: velocity
        s1 = smp.fsm_solves()
        assert s1 - s0 == NCH * p.nstat
        l1 = smp.state()[1]
        smp.run(1)                                      # step 1: nuisance
        assert smp.fsm_solves() == s1
        assert (smp.state()[1] != l1).any() and not smp.last()[2].any()
        smp.run(1)
        assert smp.fsm_solves() - s1 == NCH * p.nstat
    finally:
        smp.close()


# --- 3. logL is the logL of a full forward at the chain's models, positions and values ---
@pytest.mark.parametrize("case", ["P", "PS", "P-hypo"])
def test_logl_invariant(case, monkeypatch):
    TH._set_path("per_step", monkeypatch)
    TH._dev()
    from mceik_amd import mcmc
    p = TH._problem(case.split("-")[0], seed=11)
    smp = mcmc.Sampler(p, nchains=NCH)
    try:
        _enable(smp, _nu(p, every=3, offset=1))
        if case.endswith("hypo"):
            smp.hypo_enable(3, dmax=(1, 1, 1))          # steps 2, 5, 8
        smp.run(9)
        kn, kc = smp.nuis_get()
        assert (kn != 4).any() and (kc != 0).any() and smp.state()[2].sum() > 0
        if case.endswith("hypo"):
            assert (smp.hypo_positions() != smp.hypo_positions()[:1]).any() or smp.hypo_stats()[1].sum() > 0
        saved, again = _recomputed_logl(smp)
        TH._same((again,), (saved,), case)
        smp.run(3)                                      # and the tables it left serve the next nuisance step
        saved, again = _recomputed_logl(smp)
        TH._same((again,), (saved,), case + " after restore")
    finally:
        smp.close()


# --- 4. enabled, but no nuisance step in the run: the plain sampler ---
@pytest.mark.parametrize("path,phases", [("per_step", "P"), ("two_pipes", "PS")])
def test_enabled_but_never_stepping(path, phases, monkeypatch):
    n = TH._set_path(path, monkeypatch)
    TH._dev()
    from mceik_amd import mcmc
    p = TH._problem(phases, n=n, seed=11)
    out = []
    for on in (False, True):
        smp = mcmc.Sampler(p, nchains=NCH, max_samples=8)
        try:
            if on:
                _enable(smp, _nu(p, every=1000, offset=999))
            flags = []
            for _ in range(5):
                smp.run(1)
                flags.append(smp.last()[2].copy())
            v, l, nacc, _ = smp.state()
            kv, kl = smp.samples()
            out.append((v, l, nacc, np.array(flags), kv, kl))
        finally:
            smp.close()
    assert out[0][2].sum() > 0
    TH._same(out[1], out[0], path)


# --- 5. a sampler built for multi-step launches ---
def test_multi_step_sampler(monkeypatch):
    n = TH._set_path("multi_step", monkeypatch)
    TH._dev()
    from mceik_amd import mcmc
    p = TH._problem("P", n=n, seed=11)
    nu = _nu(p)
    v0, _, l0 = _start(p, NCH, 0)
    r = _restate(p, nu, v0, l0, 0, 4)
    off = types.SimpleNamespace(**{**vars(nu), "every": 0})
    r2 = _restate(p, off, r.v, r.logl, 0, 2, step0=4, kn0=r.kn, kc0=r.kc)        # disabled: the values still count
    assert (r.kn != 4).any() or (r.kc != 0).any()
    smp = mcmc.Sampler(p, nchains=NCH)
    plain = mcmc.Sampler(p, nchains=NCH)
    try:
        assert smp.info()["multi_step"]
        _enable(smp, nu)
        assert not smp.info()["multi_step"]
        smp.run(4)
        TH._same(smp.state()[:2] + smp.nuis_get(), (r.v, r.logl, r.kn, r.kc), "enabled")
        smp.nuis_disable()
        assert not smp.info()["multi_step"]
        smp.run(2)
        TH._same(smp.state()[:2] + smp.nuis_get(), (r2.v, r2.logl, r2.kn, r2.kc), "disabled")
        smp.nuis_clear()
        assert smp.info()["multi_step"]
        with pytest.raises(RuntimeError):
            smp.nuis_get()
        ck = smp.checkpoint()
        plain.restore(ck, recompute_logl=True)
        TH._same((smp.state()[1],), (plain.state()[1],), "clear recomputes the plain logL")
        smp.run(5)
        plain.run(5)
        TH._same(smp.state(), plain.state(), "after clear")
    finally:
        smp.close()
        plain.close()


# --- 6. tempering: the values travel with the models ---
def test_tempering(monkeypatch):
    TH._set_path("per_step", monkeypatch)
    p = TH._problem("P", seed=11)
    nu = _nu(p)
    nch = 6
    v0, _, l0 = _start(p, nch, 0)
    r = _restate(p, nu, v0, l0, 0, NSTEPS, betas=LADDER3, swap_every=2)
    assert r.swaps, "no accepted swap between chains whose values differ"
    assert any(s.acc for s in r.subs if s.chain >= 2) and any(s.changed and s.acc for s in r.vsteps)
    TH._dev()
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=nch)
    try:
        smp.temper_enable(LADDER3, swap_every=2)
        _enable(smp, nu)
        flags, recs = _run_gpu(smp, NSTEPS)
        _compare(smp, r, flags, recs, "tempered")
        saved, again = _recomputed_logl(smp)            # the effective rows and current tables travelled too
        TH._same((again,), (saved,), "tempered, recomputed")
    finally:
        smp.close()


# --- 7. block proposals and the prior act on the velocity steps, with the effective arrays ---
def test_block_and_prior(monkeypatch):
    TH._set_path("per_step", monkeypatch)
    from mceik_amd import mcmc
    p = TH._problem("PS", seed=11)
    nu = _nu(p)
    block, sig = (0, 2), dict(sigma_smooth=(400.0, 300.0))
    ws, wd = mcmc.prior_weight(sig["sigma_smooth"]), (0.0, 0.0)
    v0, _, l0 = _start(p, NCH, 0)
    r = _restate(p, nu, v0, l0, 0, NSTEPS, block=block, prior=(ws, wd))
    assert any(s.changed and s.acc for s in r.vsteps) and any(s.changed and s.inp and not s.acc for s in r.vsteps)
    TH._dev()
    smp = mcmc.Sampler(p, nchains=NCH)
    try:
        smp.block_enable(*block)
        smp.prior_enable(**sig)
        _enable(smp, nu)
        flags, recs = _run_gpu(smp, NSTEPS)
        _compare(smp, r, flags, recs, "block and prior")
    finally:
        smp.close()


# --- 8. checkpoint, moments ---
def test_checkpoint_and_moments(monkeypatch):
    TH._set_path("per_step", monkeypatch)
    p = TH._problem("P", seed=11, nburn=1, keepk=2)
    nu = _nu(p)
    v0, _, l0 = _start(p, NCH, 0)
    r = _restate(p, nu, v0, l0, 0, 6)
    assert r.mom.n == 3 * NCH and (r.mom.hist.sum(1) == r.mom.n).all() and (r.mom.hist[:, 4] != r.mom.n).any()
    TH._dev()
    from mceik_amd import mcmc
    one, a, b = (mcmc.Sampler(p, nchains=NCH) for _ in range(3))
    try:
        for s in (one, a, b):
            _enable(s, nu)
        one.run(6)
        TH._same(_moments(one), (r.mom.n, r.mom.ksum, r.mom.hist, r.mom.csum), "moments against the restatement")
        TH._same(one.state()[:2] + one.nuis_get(), (r.v, r.logl, r.kn, r.kc), "6 steps")
        a.run(3)
        ck = a.checkpoint()
        b.restore(ck)
        b.run(3)
        TH._same(b.state() + b.nuis_get() + _moments(b) + b.nuis_stats(),
                 one.state() + one.nuis_get() + _moments(one) + one.nuis_stats(), "3 + checkpoint + restore + 3")
        # ranks merge by addition: the first three steps' moments plus what a run without them adds
        m3 = a.nuis_moments()
        b.nuis_moments_set({"n": 0, "ksum": 0 * m3["ksum"], "hist": 0 * m3["hist"], "csum": 0 * m3["csum"]})
        assert b.nuis_moments()["n"] == 0
        a.run(3)
        b.restore(ck)
        b.nuis_moments_set({"n": 0, "ksum": 0 * m3["ksum"], "hist": 0 * m3["hist"], "csum": 0 * m3["csum"]})
        b.run(3)
        mb = b.nuis_moments()
        TH._same(tuple(m3[k] + mb[k] for k in ("n", "ksum", "hist", "csum")), _moments(one), "merge by addition")
        sm = one.nuis_summary()
        w = r.mom.hist / r.mom.n
        assert np.allclose(sm["lnlam_mean"], w @ nu.lnlam) and sm["static_std"].shape == (1, p.nstat)
        assert np.allclose(sm["static_mean"], r.mom.csum[..., 0] / r.mom.n * nu.dt)
        other = mcmc.Sampler(p, nchains=NCH)
        try:
            _enable(other, nu, dk=nu.dk + 1)
            with pytest.raises(ValueError):
                other.restore(ck)
        finally:
            other.close()
    finally:
        for s in (one, a, b):
            s.close()


# --- 9. nuis_set ---
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_set_values(phases, monkeypatch):
    TH._set_path("per_step", monkeypatch)
    p = TH._problem(phases, seed=11)
    nu = _nu(p)
    rng = np.random.default_rng(5)
    kn = rng.integers(0, 9, (NCH, p.nphase)).astype(np.int32)
    kc = rng.integers(-nu.kcmax, nu.kcmax + 1, (NCH, p.nphase, p.nstat)).astype(np.int32)
    v0, _, _ = _start(p, NCH, 0)
    nodes = p.ev_node
    want = np.array([_logl(p, nu, kn[c], kc[c], O.forward_all_f32(TH._at(p, nodes), v0[c].ravel()), nodes)
                     for c in range(NCH)])
    TH._dev()
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=NCH)
    try:
        _enable(smp, nu)
        smp.run(2)
        smp.restore({"v": v0, "logl": None, "naccept": np.zeros(NCH, np.int64), "step": 0}, recompute_logl=True)
        s0 = smp.fsm_solves()
        smp.nuis_set(kn, kc)
        assert smp.fsm_solves() == s0
        TH._same(smp.nuis_get() + (smp.state()[1],), (kn, kc, want), "set")
        saved, again = _recomputed_logl(smp)
        TH._same((again,), (saved,), "set against a recompute")
        with pytest.raises(ValueError):
            smp.nuis_set(kn + 9, kc)
        with pytest.raises(ValueError):
            smp.nuis_set(kn, kc + 2 * nu.kcmax + 1)
    finally:
        smp.close()


# --- 10. refusals ---
def test_refusals(monkeypatch):
    TH._set_path("per_step", monkeypatch)
    TH._dev()
    from mceik_amd import mcmc
    p = TH._problem("P", seed=11)
    nu = _nu(p)
    lam, lnlam = nu.lam, nu.lnlam
    smp = mcmc.Sampler(p, nchains=NCH)
    try:
        for f in (smp.nuis_get, smp.nuis_stats, smp.nuis_last, smp.nuis_moments):
            with pytest.raises(RuntimeError):
                f()
        bad = [dict(ladder=None, statics_dt=None), dict(every=0), dict(every=-1), dict(offset=2), dict(offset=-1),
               dict(nsub=0), dict(ladder=(lam[:8], lnlam[:8])), dict(ladder=(lam * 1.5, lnlam)),
               dict(ladder=(lam, lnlam + 0.25)), dict(dk=-1), dict(dc=-1), dict(kcmax=-1), dict(statics_dt=0.0),
               dict(statics_dt=-0.004)]
        for kw in bad:
            with pytest.raises(ValueError):
                _enable(smp, nu, **kw)
            with pytest.raises(RuntimeError):             # a refused enable leaves no state
                smp.nuis_get()
        smp.posterior_enable()
        smp.run(1)
        with pytest.raises(ValueError):                   # an enabled posterior that holds states
            _enable(smp, nu)
        smp.posterior_disable()
        _enable(smp, nu)
        with pytest.raises(ValueError):                   # held values index a ladder of 9
            _enable(smp, nu, ladder=mcmc.nuis_ladder(11, 0.25, 4.0))
        smp.run(2)
    finally:
        smp.close()
    # tt_interp = 1 is allowed: nothing here depends on nodes
    import dataclasses
    q = dataclasses.replace(p, tt_interp=1, _keep=[])
    smp = mcmc.Sampler(q, nchains=2)
    try:
        _enable(smp, nu)
        smp.run(2)
        saved, again = _recomputed_logl(smp)
        TH._same((again,), (saved,), "tt_interp")
    finally:
        smp.close()
