"""Transdimensional Voronoi-cell models of the GPU sampler (csrc/vor.hip,
DESIGN.md s.22) against the CPU restatement tests/_vor.py, bit for bit: every
Voronoi step is restated from the state the sampler held before it (nuclei,
logL, beta), with the GPU's own logL' in the accept test, so the steps of other
kinds in between need no restatement of their own."""
import dataclasses

import numpy as np
import pytest

import _adjoint as A
import _lang as LG
import _oracle as O
import _vor as V

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _problem(seed=7, **kw):
    """The p16 problem of test_gpu_de.py: C2 at n = 16 (64 cells), 4 stations, 5 events, var = 2e-3."""
    from mceik_amd import mcmc
    if "p16" not in _PROBLEMS:
        p = mcmc.make_problem("C2", n=16, nstat=4, nev=5)
        p.var[:] = 2e-3
        _PROBLEMS["p16"] = p
    return dataclasses.replace(_PROBLEMS["p16"], seed=seed, _keep=[], **kw)


def _flat_problem(nref):
    """24 x 16 x 12 nodes: 6 x 4 x 3 = 72 cells at refinement 4 (fewer than a
    workgroup, not a multiple of 64) and 4608 cells at refinement 1 (4.5 raster tiles)."""
    from mceik_amd import mcmc
    if "flat" not in _PROBLEMS:
        p = mcmc.make_problem("C2", n=24, nstat=3, nev=4, seed=21)
        p.ny, p.nz = 16, 12
        p.sy = np.clip(p.sy, 2 * p.h, (p.ny - 3) * p.h)
        p.sz[:] = (p.nz - 1) * p.h
        p.ey = np.clip(p.ey, p.h, (p.ny - 2) * p.h)
        p.ez = np.clip(p.ez, p.h, (p.nz - 2) * p.h)
        _PROBLEMS["flat"] = p
    p = dataclasses.replace(_PROBLEMS["flat"], nref=tuple(nref), _keep=[])
    p.v_true = mcmc.cell_velocity(p)
    return p


def _ps_problem(seed):
    if "ps" not in _PROBLEMS:
        _PROBLEMS["ps"] = A.ps_problem()
    return dataclasses.replace(_PROBLEMS["ps"], seed=seed, _keep=[])


def _grid(p):
    return (p.ncx, p.ncy, p.ncz)


def _check_raster(smp):
    """v == raster(nuclei) for every chain and phase, the nuclei of a model in distinct cells."""
    p, nph = smp.p, max(1, smp.p.nphase)
    v = smp.state()[0].reshape(smp.nchains, nph, -1)
    cells, vals, counts = smp.vor_get()
    metric = smp.vor_options()["metric"]
    for c in range(smp.nchains):
        for ph in range(nph):
            k = counts[c, ph]
            assert len(set(cells[c, ph, :k].tolist())) == k
            assert np.array_equal(v[c, ph], V.raster(_grid(p), cells[c, ph, :k], vals[c, ph, :k], metric)), (c, ph)


def _beta(smp):
    if smp._temper is not None and len(smp._temper[0]) > 1:
        return np.repeat(np.asarray(smp._temper[0], np.float64), smp.nchains // len(smp._temper[0]))
    return None


def _vor_step(smp, hypo_every=0, nuis=None):
    """Runs the sampler's next step, which is a Voronoi step, and compares everything
    it reports with the restatement from the state before it."""
    p, nch = smp.p, smp.nchains
    nph = max(1, p.nphase)
    v0, l0, na0, gs = smp.state()
    c0, w0, k0 = smp.vor_get()
    o = smp.vor_options()
    ph = V.step_phase(int(gs), nph, hypo_every, nuis)
    smp.run(1)
    last = smp.vor_last()
    r = V.step(p, c0, w0, k0, l0, int(gs), ph, o, last["logl_prop"], chain_offset=smp.chain_offset, beta=_beta(smp))
    for c in range(nch):
        print(f"step {gs} phase {ph} chain {c}: {V.TYPES[r['type'][c]]} reason {r['reason'][c]} j {r['j'][c]} cell "
              f"{r['cell'][c]} value {r['value'][c]} k {k0[c, ph]} -> {r['k'][c]}, logL {l0[c]:.6f} -> "
              f"{r['logl_prop'][c]:.6f}, log u {r['logu'][c]:.4f}, accept {r['accept'][c]}")
    assert last["phase"] == ph and (smp.last_phase() == ph).all()
    for key in ("type", "reason", "j", "cell", "value", "k", "accept"):
        assert np.array_equal(last[key], r[key]), (key, last[key], r[key])
    assert np.array_equal(smp.last()[2], r["accept"])
    assert np.array_equal(_bits(last["logu"]), _bits(r["logu"]))
    assert np.array_equal(_bits(last["logl_prop"]), _bits(r["logl_prop"]))
    for c in range(nch):
        k = r["k"][c]
        assert last["cells"][c, :k].tolist() == r["pcells"][c] and last["vals"][c, :k].tolist() == r["pvals"][c], c
    assert np.array_equal(last["vprop"], r["vprop"])
    v1, l1, na1, _ = smp.state()
    c1, w1, k1 = smp.vor_get()
    assert np.array_equal(k1, r["counts"]) and np.array_equal(c1, r["cells"]) and np.array_equal(w1, r["vals"])
    assert np.array_equal(_bits(l1), _bits(r["logl"])) and np.array_equal(na1 - na0, r["accept"])
    v0, v1 = v0.reshape(nch, nph, -1), v1.reshape(nch, nph, -1)
    for c in range(nch):
        want = v0[c].copy()
        if r["accept"][c]:
            want[ph] = r["vprop"][c]
        else:
            assert not r["reason"][c] or _bits(l1[c]) == _bits(l0[c])
        assert np.array_equal(v1[c], want), c
    _check_raster(smp)
    return r


def _outcomes(r):
    return {(int(t), int(x)) for t, x in zip(r["type"], r["reason"])}


@pytest.mark.parametrize("nref", [(4, 4, 4), (1, 1, 1)])
def test_raster_kernel_equals_the_host_raster(nref):
    _dev()
    from mceik_amd import mcmc
    for p in (_problem(), _flat_problem(nref)):
        if nref != (4, 4, 4) and p.nx == 16:
            continue
        nch, ncell = 3, p.ncell
        smp = mcmc.Sampler(p, nchains=nch)
        try:
            for name, cells, vals, metric in V.raster_cases(_grid(p), p.vmin, p.vmax):
                k, kmax = len(cells), min(ncell, 64)
                C_, W_, K_ = (np.zeros((nch, 1, kmax), np.int32), np.zeros((nch, 1, kmax), np.int32),
                              np.full((nch, 1), k, np.int32))
                for c in range(nch):                        # the same set in another list order per chain
                    perm = np.random.default_rng([c, k]).permutation(k)
                    C_[c, 0, :k], W_[c, 0, :k] = np.asarray(cells)[perm], np.asarray(vals)[perm]
                smp.vor_enable(kmin=1, kmax=kmax, dv=5, metric=metric, nuclei=(C_, W_, K_))
                v = smp.state()[0]
                want = mcmc.vor_raster(p, cells, vals, metric)
                for c in range(nch):
                    assert np.array_equal(v[c], want), (name, c)
                assert np.array_equal(want, V.raster(_grid(p), cells, vals, metric))
        finally:
            smp.close()


def _crafted(p, nch=8, kmax=3):
    """Start nuclei per chain from which every rejection reason is one draw away:
    chains 0-2: kmin nuclei, in the corner cell at vmin and next to it at vmax;
    chains 3-5: kmax nuclei inside the grid; chains 6-7: kmin nuclei inside."""
    C_, W_, K_ = np.zeros((nch, 1, kmax), np.int32), np.zeros((nch, 1, kmax), np.int32), np.zeros((nch, 1), np.int32)
    for c in range(nch):
        if c < 3:
            nuc = [(0, p.vmin), (1, p.vmax)]
        elif c < 6:
            nuc = [(21, 4000), (42, 5000), (38, 6000)]
        else:
            nuc = [(21, 4000), (42, 5000)]
        K_[c, 0] = len(nuc)
        C_[c, 0, :len(nuc)], W_[c, 0, :len(nuc)] = [x[0] for x in nuc], [x[1] for x in nuc]
    return C_, W_, K_


_CRAFTED_OPTS = dict(kmin=2, kmax=3, dv=50, dmax=(1, 1, 0))
_CRAFTED_STEPS = 6


def _crafted_outcomes(p, seed):
    """What the restatement says steps 0 .. _CRAFTED_STEPS - 1 do from `_crafted` (set anew before every step)."""
    C_, W_, K_ = _crafted(p)
    o, seen = _CRAFTED_OPTS, set()
    for gs in range(_CRAFTED_STEPS):
        for c in range(C_.shape[0]):
            k = int(K_[c, 0])
            nuc = list(zip(C_[c, 0, :k].tolist(), W_[c, 0, :k].tolist()))
            d = V.draw(seed, c, gs, k, p.ncell, o["dv"], p.vmin, p.vmax, o["dmax"])
            seen.add((d["type"], V.apply(nuc, d, o["kmin"], o["kmax"], p.vmin, p.vmax, _grid(p))[0]))
    return seen


def test_every_move_type_and_rejection_reason_p_only_fp32():
    """Before every step the chains are put back on nuclei from which each
    rejection reason is one draw away; the seed is the first under which the
    restatement (integer arithmetic only: what happens before the forward does
    not depend on logL) reaches all ten outcomes within the steps."""
    _dev()
    from mceik_amd import mcmc
    seed = next(s for s in range(1, 400) if _crafted_outcomes(_problem(), s) == set(V.OUTCOMES))
    p = _problem(seed=seed)
    smp = mcmc.Sampler(p, nchains=8)
    try:
        with pytest.raises(RuntimeError):
            smp.vor_stats()                                  # never enabled
        smp.vor_enable(nuclei=_crafted(p), **_CRAFTED_OPTS)
        assert not smp.info()["multi_step"]
        seen, res = set(), []
        for gs in range(_CRAFTED_STEPS):
            if gs:
                smp.vor_set(*_crafted(p))
            res.append(_vor_step(smp))
            seen |= _outcomes(res[-1])
        assert seen == set(V.OUTCOMES), sorted(set(V.OUTCOMES) - seen)
        st = smp.vor_stats()
        for t, name in enumerate(V.TYPES):
            assert st[name]["attempts"] == sum(int((r["type"] == t).sum()) for r in res)
            assert st[name]["accepts"] == sum(int(r["accept"][r["type"] == t].sum()) for r in res)
            for q in (1, 2, 3):
                assert st[name][f"reason{q}"] == sum(int(((r["type"] == t) & (r["reason"] == q)).sum()) for r in res)
        assert sum(st[n]["attempts"] for n in V.TYPES) == 8 * _CRAFTED_STEPS
        assert smp.vor_stats(reset=True) == st and smp.vor_stats()["value"]["attempts"] == 0
    finally:
        smp.close()


def test_consecutive_steps_keep_v_the_raster_of_the_nuclei():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=11)
    smp = mcmc.Sampler(p, nchains=8)
    try:
        v0 = smp.state()[0]
        smp.vor_enable(kmin=1, kmax=6, k0=3, dmax=(2, 1, 1))
        cells, vals, counts = smp.vor_get()
        for c in range(8):                                   # the start draw, and the values v had there
            want = V.start_cells(p.seed, c, 0, 3, p.ncell)
            assert counts[c, 0] == 3 and cells[c, 0, :3].tolist() == want and np.array_equal(vals[c, 0, :3], v0[c][want])
        _check_raster(smp)
        res = [_vor_step(smp) for _ in range(10)]
        assert any(r["accept"].any() for r in res) and any((r["accept"] == 0).any() for r in res)
        ck = smp.checkpoint()
        smp.restore(ck, recompute_logl=True)                 # logL from scratch equals the carried logL
        assert np.array_equal(_bits(smp.state()[1]), _bits(ck["logl"]))
        _check_raster(smp)
    finally:
        smp.close()
    smp = mcmc.Sampler(p, nchains=4, chain_offset=4)         # the start draw is keyed by the global chain
    try:
        smp.vor_enable(kmin=1, kmax=6, k0=3)
        cells = smp.vor_get()[0]
        assert [cells[c, 0, :3].tolist() for c in range(4)] == [V.start_cells(p.seed, 4 + c, 0, 3, p.ncell) for c in range(4)]
    finally:
        smp.close()


def test_p_and_s_only_the_stepped_phase_changes():
    _dev()
    from mceik_amd import mcmc
    p = _ps_problem(seed=21)
    smp = mcmc.Sampler(p, nchains=4)
    try:
        smp.vor_enable(kmin=1, kmax=5, k0=2, dmax=(1, 1, 1))
        phases = []
        for _ in range(6):
            c0, w0, k0 = smp.vor_get()
            v0 = smp.state()[0]
            r = _vor_step(smp)
            ph = smp.vor_last()["phase"]
            phases.append(ph)
            c1, w1, k1 = smp.vor_get()
            assert np.array_equal(c0[:, 1 - ph], c1[:, 1 - ph]) and np.array_equal(w0[:, 1 - ph], w1[:, 1 - ph])
            assert np.array_equal(k0[:, 1 - ph], k1[:, 1 - ph])
            assert np.array_equal(v0[:, 1 - ph], smp.state()[0][:, 1 - ph])
            lo, hi = (p.vsmin, p.vsmax) if ph else (p.vmin, p.vmax)
            assert all(lo <= x <= hi for c in range(4) for x in r["pvals"][c])
        assert phases == [0, 1, 0, 1, 0, 1]
        ck = smp.checkpoint()                                # the other phase's current tables are unchanged too
        smp.restore(ck, recompute_logl=True)
        assert np.array_equal(_bits(smp.state()[1]), _bits(ck["logl"]))
    finally:
        smp.close()


def test_phase_counts_voronoi_steps_only():
    """Hypocentre steps 2, 5, 8 and nuisance steps 1, 5 (hypocentre wins), 9: the
    Voronoi steps 0, 3, 4, 6, 7, 10 alternate the phase."""
    _dev()
    from mceik_amd import mcmc
    p = _ps_problem(seed=23)
    smp = mcmc.Sampler(p, nchains=4)
    try:
        smp.hypo_enable(3, dmax=(1, 1, 1))
        smp.nuis_enable(4, offset=1, nsub=4, ladder=mcmc.nuis_ladder(11, 0.25, 4.0), statics_dt=1e-3, kcmax=20)
        smp.vor_enable(kmin=1, kmax=5, k0=2)
        phases = []
        for gs in range(11):
            if V.is_velocity_step(gs, 3, (4, 1)):
                _vor_step(smp, 3, (4, 1))
                phases.append(smp.vor_last()["phase"])
            else:
                smp.run(1)
                _check_raster(smp)
        assert phases == [0, 1, 0, 1, 0, 1]
    finally:
        smp.close()


def test_fp64_sampler():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=29)
    smp = mcmc.Sampler(p, nchains=8, precision=64)
    try:
        smp.vor_enable(kmin=1, kmax=6, k0=3)
        for _ in range(3):
            _vor_step(smp)
    finally:
        smp.close()


def _run(p, nchains, nsteps, setup, env, monkeypatch, max_samples=0):
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    from mceik_amd import mcmc
    smp = mcmc.Sampler(p, nchains=nchains, max_samples=max_samples)
    try:
        setup(smp)
        smp.run(nsteps)
        v, l, na, _ = smp.state()
        info = smp.info()
        out = {"v": v, "logl": l, "naccept": na, "npipe": info["npipe"], "multi_step": info["multi_step"]}
        if max_samples:
            out["samples"] = smp.samples()
        if smp._vor is not None:
            out["nuclei"] = smp.vor_get()
            out["stats"] = smp.vor_stats()
            out["last"] = smp.vor_last()
            out["moments"] = smp.vor_moments()
        return out
    finally:
        smp.close()


def _same_state(a, b):
    assert np.array_equal(a["v"], b["v"]) and np.array_equal(_bits(a["logl"]), _bits(b["logl"]))
    assert np.array_equal(a["naccept"], b["naccept"])


def _same_run(a, b):
    _same_state(a, b)
    for x, y in zip(a["nuclei"], b["nuclei"]):
        assert np.array_equal(x, y)
    assert a["stats"] == b["stats"]
    for x, y in zip(a["samples"], b["samples"]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    for k in a["last"]:
        assert np.array_equal(a["last"][k], b["last"][k]), k
    for k in a["moments"]:
        assert np.array_equal(a["moments"][k], b["moments"][k]), k


def test_pipes_and_multi_step_builds_do_not_change_a_bit(monkeypatch):
    _dev()
    p = _problem(seed=5)

    def setup(smp):
        smp.vor_enable(kmin=1, kmax=6, k0=3)

    one = _run(p, 10, 8, setup, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, monkeypatch, max_samples=8)
    two = _run(p, 10, 8, setup, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}, monkeypatch, max_samples=8)
    per = _run(p, 10, 8, setup, {"MCEIK_PERSIST": "1"}, monkeypatch, max_samples=8)
    assert one["npipe"] == 1 and two["npipe"] == 2 and not per["multi_step"]
    assert sum(one["stats"][n]["attempts"] for n in V.TYPES) == 80
    _same_run(one, two)
    _same_run(one, per)


def test_tempering_nuclei_travel_with_the_models():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=13)
    smp = mcmc.Sampler(p, nchains=8)
    try:
        smp.temper_enable(betas=[1.0, 1e-300], swap_every=2)
        smp.vor_enable(kmin=1, kmax=6, k0=3)
        # a round every pair of which swaps for certain: the hot chains get the nuclei of the four best logL
        cells, vals, counts = smp.vor_get()
        order = np.argsort(smp.state()[1], kind="stable")
        smp.vor_set(cells[order], vals[order], counts[order])
        v0, l0, _, _ = smp.state()
        assert (l0[4:] >= l0[:4]).all()
        cells, vals, counts = smp.vor_get()
        smp.temper_swap(0)
        v1, l1, _, _ = smp.state()
        swap = np.r_[4:8, 0:4]
        assert np.array_equal(v1, v0[swap]) and np.array_equal(_bits(l1), _bits(l0[swap]))
        for x, y in zip(smp.vor_get(), (cells, vals, counts)):
            assert np.array_equal(x, y[swap])
        _check_raster(smp)
        att, acc = smp.temper_stats(reset=True)
        assert att.sum() == 4 and acc.sum() == 4
        for gs in range(9):
            if gs % 2:                                       # no swap round before an odd step: restated
                r = _vor_step(smp)
                hot = slice(4, 8)                            # beta = 1e-300 accepts every valid move
                assert np.array_equal(r["accept"][hot], (r["reason"][hot] == 0).astype(np.uint8))
            else:                                            # (gs > 0: a swap round, then the step)
                smp.run(1)
                _check_raster(smp)
        assert smp.temper_stats()[0].sum() == 8              # rounds of parity 0 at steps 4 and 8
        ck = smp.checkpoint()
        smp.restore(ck, recompute_logl=True)
        assert np.array_equal(_bits(smp.state()[1]), _bits(ck["logl"]))
    finally:
        smp.close()


def test_moved_events_noise_and_statics_reach_the_accept():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=19)
    smp = mcmc.Sampler(p, nchains=8)
    try:
        smp.hypo_enable(3, dmax=(1, 1, 1))
        smp.nuis_enable(3, offset=1, nsub=4, ladder=mcmc.nuis_ladder(11, 0.25, 4.0), statics_dt=1e-3, kcmax=20)
        smp.vor_enable(kmin=1, kmax=6, k0=3)
        _vor_step(smp, 3, (3, 1))                            # step 0
        smp.run(5)                                           # nuisance, hypocentre, Voronoi, nuisance, hypocentre
        kn, kc = smp.nuis_get()
        hyp = smp.hypo_positions()
        assert (hyp != hyp[0]).any() or kc.any() or (kn != 5).any()
        inp = mcmc.logl_inputs(smp)
        r = _vor_step(smp, 3, (3, 1))                        # step 6
        ttab = smp.last()[0]
        valid = np.flatnonzero(r["reason"] == 0)
        assert valid.size
        for c in valid:                                      # logL' on the host from the GPU's tables and the chain's state
            ll = mcmc.logl_picks(p, ttab[c], inp["var"][c], inp["tcorr"][c])
            for t in inp["norm"][c]:
                ll = ll - float(t)
            assert _bits(ll) == _bits(r["logl_prop"][c]), c
        c = int(valid[0])                                    # and the tables are those of v' at the chain's moved events
        tt = O.forward_all_f32(O.make_problem(LG.at_positions(p, inp["hyp"][c])), r["vprop"][c].astype(np.int32))
        assert np.array_equal(np.asarray(tt, np.float32).reshape(ttab[c].shape).view(np.uint32), ttab[c].view(np.uint32))
        assert sum(smp.vor_stats()[n]["attempts"] for n in V.TYPES) == 3 * 8
    finally:
        smp.close()


def test_kept_steps_ring_and_moments():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=41)
    smp = mcmc.Sampler(p, nchains=8, max_samples=4)
    try:
        smp.temper_enable(betas=[1.0, 0.5], swap_every=3)
        smp.vor_enable(kmin=1, kmax=6, k0=3)
        hist, dens = np.zeros((1, 7), np.uint64), np.zeros((1, p.ncell), np.uint64)
        for n in range(1, 6):
            smp.run(1)                                       # a kept step (nburn = 0, keepK = 1) and a Voronoi step
            v, l, _, _ = smp.state()
            sv, sl = smp.samples()[:2]
            assert np.array_equal(np.asarray(sv)[-1].reshape(v.shape), v)    # the post-step model
            assert np.array_equal(_bits(np.asarray(sl)[-1]), _bits(l))
            cells, _, counts = smp.vor_get()
            for c in range(4):                               # the cold chains only
                hist[0, counts[c, 0]] += 1
                dens[0, cells[c, 0, :counts[c, 0]]] += 1
            m = smp.vor_moments()
            assert m["n"] == 4 * n and np.array_equal(m["hist"], hist) and np.array_equal(m["dens"], dens)
        s = smp.vor_summary()
        assert abs(s["k_posterior"].sum() - 1.0) < 1e-12 and s["density"].shape == (1, p.ncell)
        assert set(s["acceptance"]) == set(V.TYPES)
    finally:
        smp.close()


def test_checkpoint_after_an_odd_number_of_steps():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=37)
    opts = dict(kmin=1, kmax=6, k0=3, dmax=(1, 2, 1))
    smp = mcmc.Sampler(p, nchains=8)
    try:
        smp.vor_enable(**opts)
        smp.run(5)
        ck = smp.checkpoint()
        assert sum(ck["vor"]["stats"][n]["attempts"] for n in V.TYPES) == 40 and ck["vor"]["moments"]["n"] == 40
        smp.run(6)
        want, nuc, st, mom = smp.state(), smp.vor_get(), smp.vor_stats(), smp.vor_moments()
    finally:
        smp.close()
    smp = mcmc.Sampler(p, nchains=8)
    try:
        with pytest.raises(ValueError):
            smp.restore(ck)                                  # the models are off here
        smp.vor_enable(**dict(opts, dmax=(1, 1, 1)))
        with pytest.raises(ValueError):
            smp.restore(ck)                                  # other options
        smp.vor_enable(**dict(opts, k0=2))                   # (another start: the restore brings the nuclei)
        with pytest.raises(ValueError):
            smp.restore({k: x for k, x in ck.items() if k != "vor"})     # no nuclei for models that are on
        smp.restore(ck)
        assert smp.vor_stats() == ck["vor"]["stats"]
        smp.run(6)
        got = smp.state()
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
        assert np.array_equal(got[2], want[2]) and got[3] == want[3]
        for x, y in zip(smp.vor_get(), nuc):
            assert np.array_equal(x, y)
        assert smp.vor_stats() == st                         # counters rebased
        m = smp.vor_moments()
        assert m["n"] == mom["n"] and np.array_equal(m["hist"], mom["hist"]) and np.array_equal(m["dens"], mom["dens"])
    finally:
        smp.close()


def test_refusals_and_the_setter():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=3)
    smp = mcmc.Sampler(p, nchains=8)
    try:
        for kw in ({"kmin": 0}, {"kmin": 3, "kmax": 2}, {"kmax": 513}, {"kmax": 65}, {"kmin": 2, "k0": 1}, {"dv": 0},
                   {"dmax": (0, 0, 0)}, {"dmax": (-1, 1, 1)}, {"metric": (0, 1, 1)}, {"metric": (20000, 20000, 20000)}):
            with pytest.raises(ValueError):
                smp.vor_enable(**kw)
        with pytest.raises(RuntimeError):
            smp.vor_options()                                # still never enabled
        before = smp.state()
        others = (("block", lambda: smp.block_enable(0, 1), smp.block_disable),
                  ("prior", lambda: smp.prior_enable(sigma_smooth=40.0), smp.prior_disable),
                  ("lang", lambda: smp.lang_enable(2), smp.lang_disable),
                  ("de", lambda: smp.de_enable(2), smp.de_disable))
        for name, on, off in others:                         # each refuses the models, with no state change
            on()
            with pytest.raises(ValueError):
                smp.vor_enable()
            off()
        after = smp.state()
        assert np.array_equal(before[0], after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
        smp.vor_enable(kmin=1, kmax=4, k0=2)
        for name, on, off in others:                         # and the models refuse each
            with pytest.raises(ValueError):
                on()
        assert smp._block is None and smp._prior is None and smp._de is None and not smp.info()["multi_step"]
        # the setter validates: nothing changes on a refusal
        cells, vals, counts = smp.vor_get()
        state = smp.state()
        bad = []
        c, w, k = cells.copy(), vals.copy(), counts.copy()
        c[2, 0, 1] = c[2, 0, 0]
        bad.append((c, w, k))                                # two nuclei in one cell
        c, w, k = cells.copy(), vals.copy(), counts.copy()
        w[1, 0, 0] = p.vmax + 1
        bad.append((c, w, k))                                # a value outside the box
        c, w, k = cells.copy(), vals.copy(), counts.copy()
        c[0, 0, 0] = p.ncell
        bad.append((c, w, k))                                # a cell outside the grid
        for kk in (0, 5):
            c, w, k = cells.copy(), vals.copy(), counts.copy()
            k[3, 0] = kk
            bad.append((c, w, k))                            # a count outside [kmin, kmax]
        for b in bad:
            with pytest.raises(ValueError):
                smp.vor_set(*b)
        for x, y in zip(smp.vor_get(), (cells, vals, counts)):
            assert np.array_equal(x, y)
        assert np.array_equal(smp.state()[0], state[0]) and np.array_equal(_bits(smp.state()[1]), _bits(state[1]))
        # a valid set: the model and logL follow
        c, w, k = cells.copy(), vals.copy(), counts.copy()
        c[0, 0, :3], w[0, 0, :3], k[0, 0] = [5, 60, 33], [2000, 3000, 4000], 3
        smp.vor_set(c, w, k)
        _check_raster(smp)
        got = smp.state()
        assert np.array_equal(got[0][1:], state[0][1:]) and np.array_equal(_bits(got[1][1:]), _bits(state[1][1:]))
        assert _bits(got[1][0]) != _bits(state[1][0])
    finally:
        smp.close()


def test_after_disable_the_sampler_is_the_plain_one(monkeypatch):
    _dev()
    from mceik_amd import mcmc
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    p = _problem(seed=9)
    smp = mcmc.Sampler(p, nchains=4)
    plain = mcmc.Sampler(p, nchains=4)
    try:
        multi = plain.info()["multi_step"]
        smp.vor_enable(kmin=1, kmax=6, k0=3)
        smp.run(3)
        smp.vor_disable()
        assert not smp.vor_options()["on"] and smp.info()["multi_step"] == multi
        ck = smp.checkpoint()
        assert "vor" not in ck
        _check_raster(smp)                                   # v stands as the last raster
        plain.restore(ck)
        smp.run(5)
        plain.run(5)
        _same_state(dict(zip(("v", "logl", "naccept"), smp.state())), dict(zip(("v", "logl", "naccept"), plain.state())))
        assert (smp.state()[0] != ck["v"]).any()             # single cells moved again
    finally:
        smp.close()
        plain.close()
