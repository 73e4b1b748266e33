"""Discrete Langevin moves of the GPU sampler (csrc/lang.hip)
against the CPU restatement tests/_lang.py, bit for bit: every Langevin step
is restated from the state the sampler held before it (models, logL, beta,
hypocentres, effective var / tcorr), so the steps of other kinds in between
need no restatement of their own.

A failure is not provoked on the GPU: the `failed` path is the restatement's
unit logic (test_lang_host.py)."""
import dataclasses

import numpy as np
import pytest

import _adjoint as A
import _lang as LG

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
    """C2 at n = 16 (64 cells), 4 stations, 5 events; picks at sigma = 2 ms so
    that the drift is of the order of 1 per m/s."""
    from mceik_amd import mcmc
    if "p16" not in _PROBLEMS:
        p = mcmc.make_problem("C2", n=16, nstat=4, nev=5)
        p.var[:] = 2e-3
        _PROBLEMS["p16"] = p
    return dataclasses.replace(_PROBLEMS["p16"], seed=seed, _keep=[], **kw)


def _ps_problem(seed):
    if "ps" not in _PROBLEMS:
        _PROBLEMS["ps"] = A.ps_problem()
    return dataclasses.replace(_PROBLEMS["ps"], seed=seed, _keep=[])


def _lang_step(smp, sigma, dmax, prior=None):
    """Runs the sampler's next step, which is a Langevin step, and compares
    everything it reports with the restatement from the state before it."""
    from mceik_amd import mcmc
    p, nch = smp.p, smp.nchains
    v0, l0, na0, gs = smp.state()
    inp = mcmc.logl_inputs(smp)
    nuis = smp._nuis is not None
    beta = None
    if smp._temper is not None and len(smp._temper[0]) > 1:
        beta = np.repeat(np.asarray(smp._temper[0], np.float64), nch // len(smp._temper[0]))
    smp.run(1)
    v1, l1, na1, _ = smp.state()
    last = smp.lang_last()
    acc = smp.last()[2]
    out = []
    for c in range(nch):
        r = LG.step(p, smp.chain_offset + c, int(gs), v0[c], float(l0[c]), sigma, dmax,
                    beta=None if beta is None else float(beta[c]), prior=prior,
                    var=inp["var"][c] if nuis else None, tcorr=inp["tcorr"][c] if nuis else None,
                    norm=inp["norm"][c] if nuis else None, hyp=None if inp["hyp"] is None else inp["hyp"][c],
                    precision=smp.precision)
        print(f"step {gs} chain {c}: phase {r['phase']}, moved {int((r['delta'] != 0).sum())}, lqf {r['lqf']:.6f}, "
              f"lqr {r['lqr']:.6f}, logL {l0[c]:.6f} -> {r['logl_prop']:.6f}, accept {r['accept']}")
        assert last["phase"][c] == r["phase"], c
        assert np.array_equal(last["delta"][c], r["delta"]), c
        assert _bits(last["lqf"][c]) == _bits(r["lqf"]) and _bits(last["lqr"][c]) == _bits(r["lqr"]), c
        assert _bits(last["logl_prop"][c]) == _bits(r["logl_prop"]), c
        assert last["accept"][c] == r["accept"] == acc[c] and last["status"][c] == 0, c
        assert np.array_equal(v1[c].ravel(), r["v"].ravel()) and _bits(l1[c]) == _bits(r["logl"]), c
        assert na1[c] - na0[c] == r["accept"], c
        out.append(r)
    return out


def test_p_only_fp32_every_other_step():
    _dev()
    from mceik_amd import mcmc
    p = _problem()
    smp = mcmc.Sampler(p, nchains=3)
    try:
        smp.lang_enable(2, sigma=4.0, dmax=8)
        assert not smp.info()["multi_step"]
        res = []
        for gs in range(4):
            if gs % 2 == 0:
                res += _lang_step(smp, 4.0, 8)
            else:
                smp.run(1)
        st = smp.lang_stats()
        assert st["attempts"] == 6 and st["failed"] == 0 and st["accepts"] == sum(r["accept"] for r in res)
        assert st["moved"] == sum(int((r["delta"] != 0).sum()) for r in res if r["accept"])
        assert any((r["delta"] != 0).sum() > p.ncell // 2 for r in res)        # a step moves the whole model
        assert smp.lang_stats(reset=True) == st and smp.lang_stats()["attempts"] == 0
    finally:
        smp.close()


def _seed_with_phases(want):
    """A sampler seed whose chain 0 draws the phases `want` at steps 0, 1, ..."""
    for seed in range(1, 200):
        if [(int(LG.draw(seed, 0, gs, 0xFFFFFFFF)[0]) * 2) >> 32 for gs in range(len(want))] == list(want):
            return seed
    raise AssertionError("no seed")


def test_p_and_s_both_phases():
    _dev()
    from mceik_amd import mcmc
    p = _ps_problem(_seed_with_phases((0, 1)))
    smp = mcmc.Sampler(p, nchains=2)
    try:
        smp.lang_enable(1, sigma=3.0, dmax=6)
        res = _lang_step(smp, 3.0, 6) + _lang_step(smp, 3.0, 6)
        assert {res[0]["phase"], res[2]["phase"]} == {0, 1}
    finally:
        smp.close()


def test_box_edges_clip_the_supports():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=11)
    v0 = mcmc.initial_models(p, range(2))
    v0[:, 0:8] = p.vmin
    v0[:, 8:16] = p.vmax
    v0[:, 16:20] = p.vmin + 2
    v0[:, 20:24] = p.vmax - 3
    smp = mcmc.Sampler(p, nchains=2, v0=v0)
    try:
        smp.lang_enable(1, sigma=6.0, dmax=5)
        res = _lang_step(smp, 6.0, 5)
        for r in res:
            assert (r["delta"][0:8] >= 0).all() and (r["delta"][8:16] <= 0).all()
            assert (r["delta"][16:20] >= -2).all() and (r["delta"][20:24] <= 3).all()
    finally:
        smp.close()


def _run_plain(p, nchains, nsteps, setup, env, monkeypatch):
    """v, logL, and the Langevin reports of every step of a sampler set up by `setup`."""
    from mceik_amd import mcmc
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    smp = mcmc.Sampler(p, nchains=nchains)
    try:
        info = setup(smp)
        rep = []
        for _ in range(nsteps):
            smp.run(1)
            if smp._lang:
                rep.append(smp.lang_last())
        v, l, na, _ = smp.state()
        return v, l, na, rep, info, smp.info()
    finally:
        smp.close()


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])
    assert len(a[3]) == len(b[3])
    for x, y in zip(a[3], b[3]):
        for k in x:
            assert np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)), k


def test_chunks_and_pipes_do_not_change_a_bit(monkeypatch):
    _dev()
    p = _problem(seed=5)

    def all_chains(smp):
        smp.lang_enable(2, offset=1, sigma=4.0, dmax=8)
        return smp.lang_options()["chunk"]

    def one_chain(smp):
        # the smallest budget that holds one chain of the pipe: below it enable refuses
        lo, hi = 1, 1 << 31
        while lo < hi:
            mid = (lo + hi) // 2
            try:
                smp.lang_enable(2, offset=1, sigma=4.0, dmax=8, mem_bytes=mid)
                hi = mid
            except ValueError:
                lo = mid + 1
        smp.lang_enable(2, offset=1, sigma=4.0, dmax=8, mem_bytes=lo)
        with pytest.raises(ValueError):
            smp.lang_enable(2, offset=1, sigma=4.0, dmax=8, mem_bytes=lo - 1)
        smp.lang_enable(2, offset=1, sigma=4.0, dmax=8, mem_bytes=lo)
        return smp.lang_options()["chunk"]

    one = {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}
    base = _run_plain(p, 5, 4, all_chains, one, monkeypatch)
    assert base[4] == [5] and base[5]["npipe"] == 1
    small = _run_plain(p, 5, 4, one_chain, one, monkeypatch)
    assert small[4] == [1]
    _same(base, small)
    two = _run_plain(p, 5, 4, all_chains, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}, monkeypatch)
    assert two[5]["npipe"] == 2 and two[4] == [2, 3]
    _same(base, two)


def test_off_is_the_plain_sampler(monkeypatch):
    _dev()
    p = _problem(seed=9)

    def plain(smp):
        return None

    def on_off(smp):
        smp.lang_enable(1, sigma=4.0, dmax=8)
        assert not smp.info()["multi_step"]
        smp.lang_disable()
        assert smp.lang_options()["every"] == 0

    def never(smp):
        smp.lang_enable(100, offset=50, sigma=4.0, dmax=8)

    for env in ({}, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}):
        a = _run_plain(p, 4, 6, plain, env, monkeypatch)
        for setup in (on_off, never):
            b = _run_plain(p, 4, 6, setup, env, monkeypatch)
            assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])


def test_tempering_puts_beta_in_the_drift_and_the_ratio():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=13)
    smp = mcmc.Sampler(p, nchains=2)
    try:
        smp.temper_enable(betas=[1.0, 0.25], swap_every=2)
        smp.lang_enable(2, offset=1, sigma=4.0, dmax=8)
        smp.run(1)
        _lang_step(smp, 4.0, 8)          # (step 1 has no swap round: the state before it is the state it starts from)
    finally:
        smp.close()


def test_prior_enters_the_drift_and_the_fold():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=17)
    vref = np.clip(p.v_true, p.vmin, p.vmax).astype(np.int32)
    smp = mcmc.Sampler(p, nchains=2)
    try:
        smp.prior_enable(sigma_smooth=40.0, sigma_damp=60.0, vref=vref)
        smp.lang_enable(1, sigma=4.0, dmax=8)
        ws, wd = mcmc.prior_weight(40.0), mcmc.prior_weight(60.0)
        _lang_step(smp, 4.0, 8, prior=(ws, wd, vref))
    finally:
        smp.close()


def test_moved_events_noise_and_statics_reach_the_pick_weights():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=19)
    smp = mcmc.Sampler(p, nchains=2)
    try:
        smp.hypo_enable(3, dmax=(1, 1, 1))
        smp.nuis_enable(3, offset=1, nsub=4, ladder=mcmc.nuis_ladder(11, 0.25, 4.0), statics_dt=1e-3, kcmax=20)
        smp.lang_enable(3, sigma=4.0, dmax=8)
        _lang_step(smp, 4.0, 8)                              # step 0
        smp.run(5)                                           # nuisance, hypocentre, Langevin, nuisance, hypocentre
        kn, kc = smp.nuis_get()
        assert (smp.hypo_positions() != smp.hypo_positions()[0]).any() or kc.any() or (kn != 5).any()
        _lang_step(smp, 4.0, 8)                              # step 6
        assert smp.lang_stats()["attempts"] == 6
    finally:
        smp.close()


def test_replaces_the_block_step():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=23)
    smp = mcmc.Sampler(p, nchains=2)
    try:
        smp.block_enable(1, 2)
        smp.lang_enable(2, sigma=4.0, dmax=8)
        _lang_step(smp, 4.0, 8)
        smp.run(1)
        att, _ = smp.block_stats()
        assert att.sum() == 2                                # step 1 alone was a block step
    finally:
        smp.close()


def test_fp64_sampler():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=29)
    smp = mcmc.Sampler(p, nchains=2, precision=64)
    try:
        smp.lang_enable(1, sigma=4.0, dmax=8)
        _lang_step(smp, 4.0, 8)
    finally:
        smp.close()
