"""The L1 (Laplace) likelihood and the L1 grid searches on the GPU (csrc/l1.h,
csrc/l1.hip) against the restatement tests/_l1.py, bit for bit.

Drop-ins: locate_l1_gridSearch__double64 and mceik_relocate_l1 against the
restated grid search, through the LDS-staged path and the fallback (more picks
than the 16 KiB residual tile holds: 32 in fp64, 64 in fp32).

Sampler: every logL the sampler reports under norm = 1 is restated from the
GPU's own travel-time tables (Sampler.last()), and every accept decision from
those tables and the step's log u; hypocentre steps from the CPU oracle's tables
at the current and candidate nodes.  C2 at n = 16 (64 cells), 4 stations, 6
events, var = 2e-3, two picks masked, one pick late by 1000 var."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

import _de as DE
import _fit
import _l1
import _oracle as O
import test_gpu_block as TB
import test_gpu_hypo as TH
import test_gpu_nuis as TN
import test_gpu_temper as TT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_PROBLEMS = {}
STAGE_CAP64, STAGE_CAP32 = 32, 64      # picks per event the kernels stage in LDS (l1.hip L1_LDS_BYTES / (64 sizeof))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------
# drop-ins

def _gs_case(ngrd, ldgrd, nobs, seed, mask=None, var=None, ties=False):
    from mceik_amd.eikonal import aligned_empty
    g = np.random.default_rng([ngrd, ldgrd, nobs, seed])
    test = aligned_empty(nobs * ldgrd)
    test[:] = g.uniform(0.2, 3.0, nobs * ldgrd)
    tobs = g.uniform(0.5, 3.5, nobs)
    varobs = g.uniform(0.01, 0.2, nobs) if var is None else np.asarray(var, np.float64)
    if ties:
        # residuals on a coarse lattice (equal residuals at many points) and two equal tables with equal picks
        t = test.reshape(nobs, ldgrd)
        t[:] = np.round(t * 4.0) / 4.0
        tobs = np.round(tobs * 4.0) / 4.0
        if nobs > 1:
            t[1], tobs[1] = t[0], tobs[0]
    m = np.zeros(nobs, np.int32) if mask is None else np.asarray(mask, np.int32)
    return types.SimpleNamespace(ngrd=ngrd, ldgrd=ldgrd, nobs=nobs, test=test, tobs=tobs, varobs=varobs, mask=m)


def _gs_check(c, iwantOT, t0use=0.25):
    from mceik_amd.eikonal import aligned_empty, locate_l1_gridsearch
    t0, obj = aligned_empty(c.ldgrd), aligned_empty(c.ldgrd)
    t0[:], obj[:] = -7.0, -7.0
    assert locate_l1_gridsearch(c.ldgrd, c.ngrd, c.nobs, iwantOT, t0use, c.mask, c.tobs, c.varobs, c.test, t0, obj) == 0
    wt0, wobj = _l1.gridsearch(c.ldgrd, c.ngrd, iwantOT, t0use, c.mask, c.tobs, c.varobs, c.test)
    what = (c.ngrd, c.ldgrd, c.nobs, iwantOT)
    assert np.array_equal(_bits(t0[:c.ngrd]), _bits(wt0)), what
    assert np.array_equal(_bits(obj[:c.ngrd]), _bits(wobj)), what
    assert (t0[c.ngrd:] == -7.0).all() and (obj[c.ngrd:] == -7.0).all(), "written past ngrd"
    return t0[:c.ngrd].copy(), obj[:c.ngrd].copy()


@pytest.mark.parametrize("ngrd,ldgrd", [(1, 8), (63, 64), (130, 136), (63, 80)])
def test_locate_l1_gridsearch(ngrd, ldgrd):
    _dev()
    for nobs in (1, 2, 7, 20, STAGE_CAP64, STAGE_CAP64 + 1, 65):
        g = np.random.default_rng([nobs, ngrd])
        masks = [None]
        if nobs >= 7:
            m = (g.random(nobs) < 0.3).astype(np.int32)
            m[0], m[nobs - 1], m[2] = 1, 1, 0            # the first and the last are masked, one is surely used
            masks.append(m)
        for k, mask in enumerate(masks):
            c = _gs_case(ngrd, ldgrd, nobs, k, mask=mask)
            for iwantOT in (1, 0):
                t0, obj = _gs_check(c, iwantOT)
                used = int((c.mask == 0).sum())
                if iwantOT == 1:                          # the median is one of the residuals
                    x = c.tobs[:, None] - c.test.reshape(nobs, ldgrd)[:, :ngrd]
                    assert all(t0[i] in x[c.mask == 0, i] for i in range(ngrd))
                else:
                    assert (t0 == 0.25).all()
                assert (obj >= 0.0).all() and (used < 2 or obj.any())


def test_locate_l1_gridsearch_special_inputs():
    _dev()
    ngrd, ldgrd = 130, 136
    # all masked: t0 = 0 (or t0use), objfn = 0
    c = _gs_case(ngrd, ldgrd, 7, 0, mask=np.ones(7, np.int32))
    for iwantOT in (1, 0):
        t0, obj = _gs_check(c, iwantOT)
        assert not obj.any() and (t0 == (0.0 if iwantOT else 0.25)).all()
    # weights that already sum to 1 (the 1e-14 branch: not scaled), exactly and within rounding
    for nobs, var in ((4, np.full(4, 4.0)), (7, np.full(7, 7.0)), (20, 1.0 / np.full(20, 0.05))):
        w = 1.0 / var
        s = 0.0
        for x in w:
            s = s + float(x)
        assert abs(s - 1.0) <= 1e-14
        _gs_check(_gs_case(ngrd, ldgrd, nobs, 1, var=var), 1)
    # ties: equal residuals at many points, two equal tables; equal and unequal weights
    for nobs in (2, 7, 20, STAGE_CAP64 + 1):
        for var in (None, np.full(nobs, 0.05)):
            c = _gs_case(ngrd, ldgrd, nobs, 2, var=var, ties=True)
            x = c.tobs[:, None] - c.test.reshape(nobs, ldgrd)[:, :ngrd]
            assert nobs < 7 or any(len(set(x[:, i])) < nobs - 1 for i in range(ngrd)), "no tie beyond the equal tables"
            _gs_check(c, 1)
            m = np.zeros(nobs, np.int32)
            m[0] = 1                                      # the first of the two equal tables is masked
            _gs_check(_gs_case(ngrd, ldgrd, nobs, 2, mask=m, var=var, ties=True), 1)


def test_locate_l1_gridsearch_argument_errors(capfd):
    """Argument checks, messages and return codes are the L2 drop-in's."""
    _dev()
    from mceik_amd.eikonal import aligned_empty, locate_l1_gridsearch, locate_l2_gridsearch
    c = _gs_case(16, 16, 3, 0)
    t0, obj = aligned_empty(16), aligned_empty(16)
    ok = dict(ldgrd=16, ngrd=16, nobs=3, mask=c.mask, tobs=c.tobs, varobs=c.varobs, test=c.test, t0=t0, objfn=obj)
    off = aligned_empty(24)[1:17]                         # 8 bytes past a 64-byte boundary
    bad = [dict(ldgrd=12, ngrd=12), dict(ngrd=17), dict(nobs=0), dict(mask=None), dict(tobs=None), dict(varobs=None),
           dict(test=None), dict(t0=None), dict(objfn=None), dict(t0=off), dict(objfn=off)]
    libc = C.CDLL(None)

    def said():                                           # (the library prints through C stdio: flush it first)
        libc.fflush(None)
        return capfd.readouterr().out
    for kw in bad:
        a = dict(ok, **kw)
        said()
        r1 = locate_l1_gridsearch(a["ldgrd"], a["ngrd"], a["nobs"], 1, 0.0, a["mask"], a["tobs"], a["varobs"], a["test"],
                                  a["t0"], a["objfn"])
        m1 = said()
        assert r1 == 1, kw
        if all(a[k] is not None for k in ("mask", "tobs", "varobs", "test", "t0", "objfn")):
            r2 = locate_l2_gridsearch(a["ldgrd"], a["ngrd"], a["nobs"], 1, 0.0, a["mask"], a["tobs"], None, a["varobs"],
                                      a["test"], a["t0"], a["objfn"])
            assert r2 == 1 and m1.replace("locate_l1_gridSearch", "locate_l2_gridSearch") == said(), kw
        else:
            assert "is null" in m1, kw
    assert locate_l1_gridsearch(16, 16, 3, 1, 0.0, c.mask, c.tobs, c.varobs, c.test, t0, obj) == 0


def _reloc_events():
    g = np.random.default_rng(77)
    n2 = STAGE_CAP32 + 2                                  # more picks than the fp32 tile holds: the fallback
    return [
        {"rows": [3, 0, 3], "tobs": g.uniform(1.0, 3.0, 3), "varobs": g.uniform(0.01, 0.1, 3)},
        {"rows": [], "tobs": np.zeros(0), "varobs": np.zeros(0)},
        {"rows": g.integers(0, 5, n2).tolist(), "tobs": np.round(g.uniform(1.0, 3.0, n2) * 8.0) / 8.0,
         "varobs": g.uniform(0.01, 0.1, n2), "tcorr": g.normal(0.0, 0.01, n2)},
        {"rows": [1, 2, 4, 0, 1, 2, 4], "tobs": g.uniform(1.0, 3.0, 7), "varobs": np.full(7, 0.05),
         "mask": [0, 1, 0, 0, 0, 0, 1]},
    ]


@pytest.mark.parametrize("single_pass", [True, False])
@pytest.mark.parametrize("want_t0", [True, False])
@pytest.mark.parametrize("log_pdf", [True, False])
def test_relocate_l1(log_pdf, want_t0, single_pass):
    """mceik_relocate_l1 (relocate(norm=1)): 5 table rows, ngrd = 130, events of 3, 0, 66 and 5 used picks."""
    dev = _dev()
    from mceik_amd.eikonal import relocate
    ld = None                                             # (relocate: ngrd = ldgrd = the tables' 130 columns)
    g = np.random.default_rng(3)
    tab = np.round(g.uniform(0.2, 3.0, (5, 130)) * 16.0).astype(np.float32) / np.float32(16.0)
    ev = _reloc_events()
    assert len(ev[2]["rows"]) > STAGE_CAP32 and ev[2].get("mask") is None
    out, t0 = relocate(torch.tensor(tab, device=dev), ev, ldgrd=ld, log_pdf=log_pdf, want_t0=want_t0,
                       single_pass=single_pass, norm=1)
    torch.cuda.synchronize(dev)
    assert tuple(out.shape) == (len(ev), 130)
    ld = 130
    wout, wt0 = _l1.relocate(tab, ev, ld, log_pdf=log_pdf)
    assert np.array_equal(_bits32(out.cpu().numpy()), _bits32(wout))
    assert (t0 is None) == (not want_t0)
    if want_t0:
        assert np.array_equal(_bits32(t0.cpu().numpy()), _bits32(wt0))
    assert not wout[1].any() and wout[0].any() and wout[2].any()
    # a fixed origin time: the objective alone
    out0, t00 = relocate(torch.tensor(tab, device=dev), ev, ldgrd=ld, log_pdf=log_pdf, single_pass=single_pass, iwantOT=0,
                         t0use=0.125, norm=1)
    w0, wt00 = _l1.relocate(tab, ev, ld, iwantOT=0, t0use=0.125, log_pdf=log_pdf)
    assert np.array_equal(_bits32(out0.cpu().numpy()), _bits32(w0)) and np.array_equal(_bits32(t00.cpu().numpy()), _bits32(wt00))
    # L2 is what it was: another objective
    out2, _ = relocate(torch.tensor(tab, device=dev), ev, ldgrd=ld, log_pdf=log_pdf, single_pass=single_pass)
    assert not np.array_equal(out2.cpu().numpy()[0], wout[0])


def test_relocate_l1_row_outside_the_tables():
    dev = _dev()
    from mceik_amd.eikonal import relocate
    tab = np.random.default_rng(4).uniform(0.2, 3.0, (5, 72)).astype(np.float32)
    ev = [{"rows": [0, 1], "tobs": [1.0, 2.0], "varobs": [0.1, 0.1]}, {"rows": [2, 5], "tobs": [1.0, 2.0], "varobs": [0.1, 0.1]}]
    out, t0 = relocate(torch.tensor(tab, device=dev), ev, ldgrd=72, norm=1)
    out, t0 = out.cpu().numpy(), t0.cpu().numpy()
    assert np.isfinite(out[0]).all() and np.isnan(out[1]).all() and np.isnan(t0[1]).all()
    with pytest.raises(ValueError):
        relocate(torch.tensor(tab, device=dev), ev[:1], ldgrd=72, norm=3)


# ---------------------------------------------------------------------------
# sampler

def _problem(phases, seed=7, n=16, **kw):
    from mceik_amd import mcmc
    key = (phases, n)
    if key not in _PROBLEMS:
        p = mcmc.make_problem("C2", n=n, nstat=4, nev=6, phases=phases)
        p.dvmax = 300
        p.var[:] = 2e-3
        per = 4 * (2 if phases == "PS" else 1)
        p.luse[[2, per + 1]] = 0                          # two picks masked
        p.tobs[2 * per + 3] += 1000.0 * p.var[2 * per + 3]    # one gross outlier: late by 1000 var
        _PROBLEMS[key] = p
    return dataclasses.replace(_PROBLEMS[key], seed=seed, _keep=[], **kw)


def _env(monkeypatch, **env):
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)


def _beta(smp):
    if smp._temper is not None and len(smp._temper[0]) > 1:
        return np.repeat(np.asarray(smp._temper[0], np.float64), smp.nchains // len(smp._temper[0]))
    return np.ones(smp.nchains)


def _restated(smp, tables, c, li=None):
    """Chain c's logL from its tables [nphase, nstat, nev] and the effective observations the sampler holds."""
    from mceik_amd import mcmc
    li = mcmc.logl_inputs(smp) if li is None else li
    terms = li["norm"][c] if smp._nuis is not None else ()
    return _l1.logl(smp.p, tables, li["var"][c], li["tcorr"][c], terms)


def _full_tables(smp):
    p = smp.p
    tt = smp.last()[0]
    assert tt.shape == (smp.nchains,) + ((p.nphase,) if p.nphase > 1 else ()) + (p.nstat, p.nevents)
    return tt.reshape(smp.nchains, max(1, p.nphase), p.nstat, p.nevents).copy()


def _sync(smp, what=""):
    """One full forward at the state the sampler holds: the logL it held is the logL of that forward, and both are
    the restatement's on the GPU's tables.  Returns the chains' current tables."""
    ck = smp.checkpoint()
    smp.restore(ck, recompute_logl=True)
    cur = _full_tables(smp)
    l = smp.state()[1]
    assert np.array_equal(_bits(l), _bits(ck["logl"])), (what, "held logL vs a full forward")
    from mceik_amd import mcmc
    li = mcmc.logl_inputs(smp)
    for c in range(smp.nchains):
        assert _bits(l[c]) == _bits(_restated(smp, cur[c], c, li)), (what, c)
    return cur


def _velocity_step(smp, cur, draw):
    """Runs the next step, a velocity step of any kind.  draw(c, gs, v0[c]) -> (reaches the accept test, log u) or
    None where the kind reports them itself.  Updates cur; returns (accept flags, logL' per chain or None)."""
    p, nch = smp.p, smp.nchains
    beta = _beta(smp)
    v0, l0, na0, gs = smp.state()
    smp.run(1)
    tt, _, acc = smp.last()
    ph = smp.last_phase()
    v1, l1, na1, _ = smp.state()
    lprop = [None] * nch
    for c in range(nch):
        tabs = cur[c].copy()
        tabs[ph[c]] = tt[c]
        d = draw(c, int(gs), v0[c])
        if d is not None:
            reaches, logu = d
            a = False
            if reaches:
                lprop[c] = _restated(smp, tabs, c)
                a = bool(logu < beta[c] * (lprop[c] - l0[c]))
            print(f"step {gs} chain {c} phase {ph[c]}: logL {l0[c]:.6f} -> {lprop[c]}, log u {logu:.4f}, accept {acc[c]}")
            assert bool(acc[c]) == a, (gs, c)
        if acc[c]:
            ln = _restated(smp, tabs, c) if lprop[c] is None else lprop[c]
            lprop[c] = ln
            assert _bits(l1[c]) == _bits(ln), (gs, c, "logL of an accepted step")
            assert (v1[c] != v0[c]).any() and na1[c] == na0[c] + 1
            cur[c] = tabs
        else:
            assert _bits(l1[c]) == _bits(l0[c]) and np.array_equal(v1[c], v0[c]) and na1[c] == na0[c], (gs, c)
    return acc, lprop


def _single_cell_draw(smp):
    P = O.make_problem(smp.p, smp.precision)

    def draw(c, gs, v):
        cell, vn, inp, logu = O.propose(P, smp.chain_offset + c, gs, np.ascontiguousarray(v, np.int32).ravel())
        return bool(inp), logu
    return draw


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_velocity_moves_under_l1(phases, prec, monkeypatch):
    """likelihood_set(1), then single-cell, block, DE and Voronoi steps; likelihood_set(2) gives the L2 logL back."""
    _dev()
    _env(monkeypatch, MCEIK_PERSIST="0", MCEIK_PIPES="1")
    from mceik_amd import mcmc
    p = _problem(phases)
    nch, nph = 8, max(1, p.nphase)
    smp = mcmc.Sampler(p, nchains=nch, precision=prec)
    try:
        assert smp.likelihood == 2
        v0, l2, _, _ = smp.state()
        smp.likelihood_set(1)
        assert smp.likelihood == 1 and not smp.info()["multi_step"]
        va, l1, na, step = smp.state()
        assert np.array_equal(va, v0) and step == 0 and not na.any()
        cur = _full_tables(smp)
        for c in range(nch):
            assert _bits(l1[c]) == _bits(_l1.logl(p, cur[c])) and _bits(l1[c]) != _bits(l2[c]), c
            assert _bits(l2[c]) == _bits(mcmc.logl_picks(p, cur[c])), c
        # single-cell steps, accepted and rejected
        seen = set()
        draw = _single_cell_draw(smp)
        for _ in range(6):
            acc, _ = _velocity_step(smp, cur, draw)
            seen |= {int(a) for a in acc}
        assert seen == {0, 1}, "single-cell steps: not both accepted and rejected"
        # a block step
        smp.block_enable(0, 2)

        def block_draw(c, gs, v):
            cell, amp, R, logu = TB._draw(p, smp.chain_offset + c, gs, 0, 2)
            ph, cc = divmod(cell, p.ncell)
            cells, dv = mcmc.block_footprint(p, cc, R, amp)
            vp = np.asarray(v, np.int64).reshape(nph, -1)[ph][cells] + dv
            lo, hi = ((p.vsmin, p.vsmax) if ph else (p.vmin, p.vmax))
            return bool(((vp >= lo) & (vp <= hi)).all()), logu
        for _ in range(2):
            _velocity_step(smp, cur, block_draw)
        smp.block_disable()
        # DE steps of both parities: logL' as the step reports it, and the decision from its log u
        smp.de_enable(1, gamma=0.3)
        for _ in range(2):
            gs = smp.state()[3]
            k, par, dph = DE.plan(int(gs), 1, 0, nph)
            movers, partners = mcmc.de_movers(nch, 1, k)
            l0 = smp.state()[1]

            def de_draw(c, gs, v):
                return None
            acc, lprop = _velocity_step(smp, cur, de_draw)
            last = smp.de_last()
            assert sorted(movers) == np.flatnonzero(last["mover"]).tolist()
            for c in movers:
                if not last["inbox"][c] or last["status"][c]:
                    assert not acc[c]
                    continue
                tabs = cur[c].copy()
                if not acc[c]:
                    tabs[dph] = smp.last()[0][c]
                ln = _restated(smp, tabs, c)
                assert _bits(last["logl_prop"][c]) == _bits(ln), (gs, c)
                logu = DE.draw(p.seed, smp.chain_offset + c, int(gs), len(partners[c]))[2]
                assert bool(acc[c]) == bool(logu < ln - l0[c]), (gs, c)
        smp.de_disable()
        cur = _sync(smp, "after the DE steps")
        # Voronoi steps: logL' and log u as the step reports them
        smp.vor_enable(kmin=1, kmax=6, k0=3)
        cur = _sync(smp, "vor_enable")
        for _ in range(3):
            l0 = smp.state()[1]
            acc, _ = _velocity_step(smp, cur, lambda c, gs, v: None)
            last = smp.vor_last()
            tt = smp.last()[0]
            for c in range(nch):
                if last["reason"][c]:
                    assert not acc[c]
                    continue
                tabs = cur[c].copy()
                if not acc[c]:
                    tabs[last["phase"]] = tt[c]
                ln = _restated(smp, tabs, c)
                assert _bits(last["logl_prop"][c]) == _bits(ln), c
                assert bool(acc[c]) == bool(last["logu"][c] < ln - l0[c]), c
        smp.vor_disable()
        _sync(smp, "after the Voronoi steps")
        # back to L2: bit for bit the logL of a sampler that never left it, at the same models
        vb = smp.state()[0]
        smp.likelihood_set(2)
        assert smp.likelihood == 2
        twin = mcmc.Sampler(p, nchains=nch, precision=prec, v0=vb)
        try:
            assert np.array_equal(_bits(smp.state()[1]), _bits(twin.state()[1]))
        finally:
            twin.close()
    finally:
        smp.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("phases", ["P", "PS"])
def test_hypocentre_and_nuisance_steps_under_l1(phases, prec, monkeypatch):
    _dev()
    _env(monkeypatch, MCEIK_PERSIST="0", MCEIK_PIPES="1")
    from mceik_amd import mcmc
    p = _problem(phases)
    nch, nph, nev, nst = 6, max(1, p.nphase), p.nevents, p.nstat
    smp = mcmc.Sampler(p, nchains=nch, precision=prec)
    try:
        smp.likelihood_set(1)
        smp.run(2)
        # --- a hypocentre step: per-event objectives of both sides, the decisions, the chain's logL
        smp.hypo_enable(1, dmax=(1, 1, 1))
        every, dmax, lo, hi = smp._hypo
        v0, _, _, gs = smp.state()
        xyz = smp.hypo_positions()
        smp.run(1)
        cand, acc, obj = smp.hypo_last()
        l1 = smp.state()[1]
        moved = rejected = 0
        for c in range(nch):
            inside = np.zeros(nev, bool)
            for e in range(nev):
                d, _ = TH._hdraw(p.seed, smp.chain_offset + c, int(gs), e, dmax)
                assert np.array_equal(cand[c, e], xyz[c, e] + d)
                inside[e] = all(lo[a] <= cand[c, e, a] <= hi[a] for a in range(3))
            nodes = TH._nodes(p, xyz[c])
            P2 = TH._at(p, np.concatenate([nodes, np.where(inside, TH._nodes(p, cand[c]), nodes)]), prec)
            tt = np.asarray(O.forward_all_f32(P2, np.ascontiguousarray(v0[c], np.int32).ravel()), np.float32)
            tt = tt.reshape(nph, nst, 2 * nev)
            oc, od = _l1.event_objs(p, tt[:, :, :nev]), _l1.event_objs(p, tt[:, :, nev:])
            ln = 0.0
            for e in range(nev):
                assert _bits(obj[c, e, 0]) == _bits(oc[e]) and _bits(obj[c, e, 1]) == _bits(od[e]), (c, e)
                logu = TH._hdraw(p.seed, smp.chain_offset + c, int(gs), e, dmax)[1]
                a = bool(inside[e]) and bool(logu < oc[e] - od[e])
                assert bool(acc[c, e]) == a, (c, e)
                ln = ln - (od[e] if a else oc[e])
                moved += a and bool((cand[c, e] != xyz[c, e]).any())
                rejected += bool(inside[e]) and not a
            assert _bits(l1[c]) == _bits(ln), c
        assert moved and rejected, "hypocentre step: not both an accepted move and a rejection"
        smp.hypo_disable()
        cur = _sync(smp, "after the hypocentre step")
        # --- a nuisance step: logL and logL' of every sub-move from the current tables
        TN._enable(smp, TN._nu(p, every=1, offset=0, nsub=6))
        assert not smp.info()["multi_step"]
        o = smp.nuis_options()
        nu = types.SimpleNamespace(lam=o["lam"], lnlam=o["lnlam"], dt=o["dt"], norm=o["norm"])
        kn, kc = smp.nuis_get()
        l0 = smp.state()[1]
        smp.run(1)
        rec, rl = smp.nuis_last()
        kinds = set()
        for c in range(nch):
            ckn, ckc, logl = kn[c].copy(), kc[c].copy(), l0[c]
            for sub in range(o["nsub"]):
                par, partner, cnd, ok = (int(x) for x in rec[c, sub])
                tkn, tkc = ckn.copy(), ckc.copy()
                if partner < 0:
                    tkn[par] = cnd
                    inside = 0 <= cnd < len(nu.lam)
                else:
                    ph, sa = divmod(par - nph, nst)
                    sb = partner - nph - ph * nst
                    delta = cnd - int(ckc[ph, sa])
                    tkc[ph, sa], tkc[ph, sb] = cnd, int(ckc[ph, sb]) - delta
                    inside = abs(int(tkc[ph, sa])) <= o["kcmax"] and abs(int(tkc[ph, sb])) <= o["kcmax"]
                assert _bits(rl[c, sub, 0]) == _bits(logl), (c, sub)
                if inside:
                    ve, tce = TN._eff(p, nu, tkn, tkc)
                    ln = TN._norm(p, nu, tkn, _l1.logl(p, cur[c], ve, tce))
                    assert _bits(rl[c, sub, 1]) == _bits(ln), (c, sub, par, partner)
                    kinds.add((partner >= 0, ok))
                else:
                    assert not ok and _bits(rl[c, sub, 1]) == _bits(logl)
                if ok:
                    ckn, ckc, logl = tkn, tkc, rl[c, sub, 1]
            k1, c1 = smp.nuis_get()
            assert np.array_equal(k1[c], ckn) and np.array_equal(c1[c], ckc) and _bits(smp.state()[1][c]) == _bits(logl)
        assert {k for k, _ in kinds} == {False, True}, "nuisance step: not both a noise and a statics move"
        _sync(smp, "after the nuisance step")
        # velocity steps with the nuisance state held
        smp.nuis_disable()
        draw = _single_cell_draw(smp)
        cur = _sync(smp, "nuisance state held")
        for _ in range(2):
            _velocity_step(smp, cur, draw)
    finally:
        smp.close()


def test_tempered_swap_under_l1(monkeypatch):
    _dev()
    _env(monkeypatch, MCEIK_PERSIST="0", MCEIK_PIPES="1")
    from mceik_amd import mcmc
    p = _problem("PS")
    nch, betas = 8, np.array([1.0, 0.05])
    smp = mcmc.Sampler(p, nchains=nch)
    try:
        smp.temper_enable(betas=betas, swap_every=0)
        smp.likelihood_set(1)
        cur = _full_tables(smp)
        draw = _single_cell_draw(smp)
        for _ in range(2):
            _velocity_step(smp, cur, draw)               # (the hot rung's decisions use beta)
        v0, l0, n0, step = smp.state()
        smp.temper_swap(0)
        v1, l1, _, _ = smp.state()
        perm, lw, att, acc = TT._swap_round(betas, nch, l0, 0, step, p.seed, 0)
        assert np.array_equal(v1, v0[perm]) and np.array_equal(_bits(l1), _bits(lw))
        assert acc.sum() > 0, "no pair swapped"
        _sync(smp, "after the swap")
    finally:
        smp.close()


def _l1_run(p, nch, nsteps, env, monkeypatch):
    from mceik_amd import mcmc
    _env(monkeypatch, **env)
    smp = mcmc.Sampler(p, nchains=nch, max_samples=4)
    try:
        smp.likelihood_set(1)
        smp.hypo_enable(3)
        TN._enable(smp, TN._nu(p, every=3, offset=1))
        smp.fit_enable(zmax=64.0)
        smp.run(nsteps)
        raw = smp.fit_raw()
        return (smp.state(), smp.hypo_positions(), smp.nuis_get(), [raw[k] for k in _fit.ARRAYS], smp.fit_last(),
                smp.info())
    finally:
        smp.close()


def test_one_and_two_pipes_give_the_same_words(monkeypatch):
    _dev()
    p = _problem("PS")
    one = _l1_run(p, 10, 9, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, monkeypatch)
    two = _l1_run(p, 10, 9, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}, monkeypatch)
    assert one[5]["npipe"] == 1 and two[5]["npipe"] == 2
    TH._same(one[0], two[0], "state")
    assert np.array_equal(one[1], two[1])
    TH._same(one[2], two[2], "nuisance state")
    TH._same(one[3], two[3], "data-fit sums")
    TH._same(one[4], two[4], "fit_last")
    assert one[0][2].sum() > 0


@pytest.mark.parametrize("phases", ["P", "PS"])
def test_fit_stream_under_l1(phases, monkeypatch):
    """The data-fit stream's origin times are the medians and its residual words the restatement's."""
    _dev()
    _env(monkeypatch, MCEIK_PERSIST="0", MCEIK_PIPES="1")
    from mceik_amd import mcmc
    p = _problem(phases)
    nch, tick = 4, 2.0 ** -20
    smp = mcmc.Sampler(p, nchains=nch)
    try:
        smp.likelihood_set(1)
        smp.fit_enable(tick=tick, zmax=64.0)
        smp.run(3)
        cur = _sync(smp, "fit on")
        smp.fit_clear()
        smp.fit_enable(tick=tick, zmax=64.0)
        smp.fit_accumulate()
        smp.fit_accumulate()                             # the same state twice: the summary's means are its words
        q, zq, tq = smp.fit_last()
        inv = 1.0 / tick
        for c in range(nch):
            for e, (js, t0, _, res) in enumerate(_l1.pick_terms(p, cur[c])):
                assert tq[c, e] == (_fit.sat32(t0 * inv)[0] if js else 0), (c, e)
                for j, r in zip(js, res):
                    assert q[c, j] == _fit.sat32(r * inv)[0], (c, j)
                    assert zq[c, j] == _fit.sat32(((1.0 / p.var[j]) * r) * 1024.0)[0], (c, j)
            assert not q[c][p.obs_mask != 0].any()
        s = mcmc.fit_summary(smp)
        med = np.array([[t[1] for t in _l1.pick_terms(p, cur[c])] for c in range(nch)])
        assert s.count == 2 and np.array_equal(s.t0_mean, tq.astype(np.float64).mean(0) * tick)
        assert np.abs(s.t0_mean - med.mean(0)).max() <= tick / 2
        # the outlier's standardised residual is large and every other pick's is not dragged along
        j = int(np.argmax(np.abs(s.pick_zmean[p.obs_mask == 0])))
        assert np.flatnonzero(p.obs_mask == 0)[j] == 2 * 4 * max(1, p.nphase) + 3
    finally:
        smp.close()


@pytest.mark.parametrize("phases", ["P", "PS"])
def test_checkpoint_carries_the_norm(phases, monkeypatch):
    _dev()
    _env(monkeypatch, MCEIK_PERSIST="0", MCEIK_PIPES="1")
    from mceik_amd import mcmc
    p = _problem(phases)
    a, b, c, d = (mcmc.Sampler(p, nchains=4) for _ in range(4))
    try:
        for s in (a, b, c):
            s.likelihood_set(1)
        a.run(5)
        ck = a.checkpoint()
        assert ck["likelihood"] == 1 and ck["step"] == 5
        b.restore(ck, recompute_logl=(phases == "PS"))
        TH._same((b.state()[1],), (ck["logl"],), "logL after restore")
        b.run(5)
        c.run(10)
        TH._same(b.state(), c.state(), "5 + 5 vs 10")
        assert c.state()[2].sum() > 0
        # the other norm is refused, either way; a checkpoint without the field is L2
        before = d.state()
        with pytest.raises(ValueError):
            d.restore(ck)
        TH._same(d.state(), before, "refused restore")
        ck2 = d.checkpoint()
        assert ck2["likelihood"] == 2
        old = {k: x for k, x in ck2.items() if k != "likelihood"}
        before = b.state()
        for bad in (ck2, old):
            with pytest.raises(ValueError):
                b.restore(bad)
        TH._same(b.state(), before, "refused restore")
        d.restore(old)
    finally:
        for s in (a, b, c, d):
            s.close()


STREAMS = {
    "posterior": lambda s: s.posterior_enable(per_chain=False, nbins=8),
    "cov": lambda s: s.cov_enable([("model", 10)]),
    "ess": lambda s: s.ess_enable(3),
    "fit": lambda s: s.fit_enable(),
    "hypo": lambda s: s.hypo_enable(2),
    "nuis": lambda s: TN._enable(s, TN._nu(s.p, every=2, offset=1)),
    "vor": lambda s: s.vor_enable(kmin=1, kmax=6, k0=3),
}


@pytest.mark.parametrize("stream", sorted(STREAMS))
def test_set_is_refused_while_a_kept_stream_holds_states(stream, monkeypatch):
    _dev()
    _env(monkeypatch, MCEIK_PERSIST="0", MCEIK_PIPES="1")
    from mceik_amd import mcmc
    p = _problem("P")
    smp = mcmc.Sampler(p, nchains=4, max_samples=4)
    try:
        STREAMS[stream](smp)
        smp.likelihood_set(1)                            # enabled, no state held yet: allowed
        smp.likelihood_set(2)
        smp.run(2)
        before = smp.state()
        for norm in (1, 2):                              # (a refusal does not depend on the norm asked for)
            with pytest.raises(ValueError):
                smp.likelihood_set(norm)
        assert smp.likelihood == 2
        TH._same(smp.state(), before, stream)
        smp.run(1)                                       # ... and the chains go on under L2
    finally:
        smp.close()


def test_refusals_leave_the_state(monkeypatch):
    _dev()
    _env(monkeypatch, MCEIK_PERSIST="0", MCEIK_PIPES="1")
    from mceik_amd import _lib, mcmc
    p = _problem("P")
    smp = mcmc.Sampler(p, nchains=4)
    try:
        smp.run(2)
        before = smp.state()
        for bad in (0, 3, -1):
            with pytest.raises(ValueError):
                smp.likelihood_set(bad)
        L = _lib.lib()
        assert L.mceik_mcmc_likelihood_set(None, 1) == 1 and L.mceik_mcmc_likelihood_get(None) == 0
        smp.lang_enable(2, offset=1, sigma=4.0, dmax=8)
        with pytest.raises(ValueError):
            smp.likelihood_set(1)                        # Langevin moves are on
        assert smp.likelihood == 2
        TH._same(smp.state(), before, "refused set")
        smp.lang_disable()
        smp.likelihood_set(1)
        held = smp.state()
        with pytest.raises(ValueError):
            smp.lang_enable(2, offset=1, sigma=4.0, dmax=8)     # ... and refused while norm = 1
        with pytest.raises(ValueError):
            mcmc.logl_grad(smp)
        TH._same(smp.state(), held, "refused lang_enable")
        assert smp.lang_options()["every"] == 0
        smp.run(2)
        smp.likelihood_set(1)                            # the norm in force again: nothing to do
        smp.likelihood_set(2)
        smp.lang_enable(2, offset=1, sigma=4.0, dmax=8)
        smp.run(2)
    finally:
        smp.close()


def test_multi_step_is_off_under_l1(monkeypatch):
    """info()["multi_step"] is False under L1 and returns to its previous value under L2 (n = 32: the 16-z kernel)."""
    _dev()
    _env(monkeypatch, MCEIK_PERSIST="1")
    from mceik_amd import mcmc
    p = _problem("P", n=32)
    smp = mcmc.Sampler(p, nchains=4)
    twin = mcmc.Sampler(p, nchains=4)
    try:
        assert smp.info()["multi_step"]
        smp.run(3)
        l2 = smp.state()[1]
        smp.likelihood_set(1)
        assert not smp.info()["multi_step"]
        assert not np.array_equal(_bits(smp.state()[1]), _bits(l2))
        smp.likelihood_set(2)
        assert smp.info()["multi_step"]
        assert np.array_equal(_bits(smp.state()[1]), _bits(l2))
        smp.run(3)
        twin.run(6)
        TH._same(smp.state(), twin.state(), "L2 -> L1 -> L2 vs a sampler that never left L2")
    finally:
        smp.close()
        twin.close()
