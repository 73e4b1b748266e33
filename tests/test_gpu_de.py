"""Differential-evolution moves of the GPU sampler (csrc/de.hip)
against the CPU restatement tests/_de.py, bit for bit: every DE step is restated
from the state the sampler held before it (models, logL, beta, hypocentres,
effective var / tcorr), so the steps of other kinds in between need no
restatement of their own.

A failed solve is not provoked on the GPU."""
import dataclasses

import numpy as np
import pytest

import _adjoint as A
import _de as DE

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
    """The p16 problem of test_gpu_lang.py: C2 at n = 16 (64 cells), 4 stations,
    5 events, var = 2e-3."""
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


def _near_models(p, nchains, amp=3, seed=0):
    """Start models close to each other (one chain's start model plus integer
    noise in [-amp, amp]), so that a DE move is small enough to be accepted now
    and then on this sharply peaked likelihood."""
    from mceik_amd import mcmc
    base = mcmc.initial_models(p, [0])[0]
    g = np.random.default_rng([p.seed, seed, 99])
    v = base[None] + g.integers(-amp, amp + 1, (nchains,) + base.shape)
    if p.nphase == 1:
        return np.clip(v, p.vmin, p.vmax).astype(np.int32)
    v[:, 0] = np.clip(v[:, 0], p.vmin, p.vmax)
    v[:, 1] = np.clip(v[:, 1], p.vsmin, p.vsmax)
    return v.astype(np.int32)


def _de_step(smp, prior=None):
    """Runs the sampler's next step, which is a DE step, and compares everything
    it reports with the restatement from the state before it."""
    from mceik_amd import mcmc
    p, nch = smp.p, smp.nchains
    nph = max(1, p.nphase)
    v0, l0, na0, gs = smp.state()
    inp = mcmc.logl_inputs(smp)
    nuis = smp._nuis is not None
    beta, ntemps = None, 1
    if smp._temper is not None and len(smp._temper[0]) > 1:
        ntemps = len(smp._temper[0])
        beta = np.repeat(np.asarray(smp._temper[0], np.float64), nch // ntemps)
    o = smp.de_options()
    smp.run(1)
    v1, l1, na1, _ = smp.state()
    last = smp.de_last()
    acc = smp.last()[2]
    r = DE.step(p, v0, l0, int(gs), (o["every"], o["offset"], o["gamma_q16"], o["cr_q16"]), ntemps=ntemps,
                chain_offset=smp.chain_offset, beta=beta, prior=prior, var=inp["var"] if nuis else None,
                tcorr=inp["tcorr"] if nuis else None, norm=inp["norm"] if nuis else None, hyp=inp["hyp"],
                precision=smp.precision)
    for c in range(nch):
        print(f"step {gs} (k {r['k']}, parity {r['par']}, phase {r['phase']}) chain {c}: mover {r['mover'][c]}, a {r['a'][c]}, "
              f"b {r['b'][c]}, moved {r['nmove'][c]}, inbox {r['inbox'][c]}, logL {l0[c]:.6f} -> {r['logl_prop'][c]:.6f}, "
              f"accept {r['accept'][c]}")
    assert last["phase"] == r["phase"] and (smp.last_phase() == r["phase"]).all()
    for k in ("mover", "a", "b", "inbox", "nmove", "status", "accept"):
        assert np.array_equal(last[k], r[k]), (k, last[k], r[k])
    assert np.array_equal(acc, r["accept"])
    assert np.array_equal(_bits(last["logl_prop"]), _bits(r["logl_prop"]))
    assert np.array_equal(v1.reshape(nch, nph, -1), r["v"])
    assert np.array_equal(_bits(l1), _bits(r["logl"]))
    assert np.array_equal(na1 - na0, r["accept"])
    d = v1.reshape(nch, nph, -1).astype(np.int64) - v0.reshape(nch, nph, -1)
    for c in range(nch):
        if r["accept"][c]:                                   # delta from v' - v; the other phase did not move
            assert np.array_equal(d[c, r["phase"]], r["delta"][c]), c
            assert nph == 1 or not d[c, 1 - r["phase"]].any(), c
        else:                                                # rejected movers and standing chains: untouched
            assert not d[c].any() and _bits(l1[c]) == _bits(l0[c]), c
    return r


def _in_box(r):
    return [(int(a), int(i)) for a, i, m in zip(r["accept"], r["inbox"], r["mover"]) if m]


def test_p_only_fp32_every_other_step():
    _dev()
    from mceik_amd import mcmc
    p = _problem()
    smp = mcmc.Sampler(p, nchains=8, v0=_near_models(p, 8))
    try:
        with pytest.raises(RuntimeError):
            smp.de_stats()                                   # never enabled
        smp.de_enable(2, gamma=0.3)
        assert not smp.info()["multi_step"]
        assert smp.de_options()["gamma_q16"] == round(0.3 * 65536) and smp.de_options()["cr_q16"] == 65536
        res = []
        for gs in range(8):
            if gs % 2 == 0:
                res.append(_de_step(smp))
            else:
                smp.run(1)
        assert {r["par"] for r in res} == {0, 1}             # both parities are seen
        assert [list(np.flatnonzero(r["mover"])) for r in res[:2]] == [[0, 2, 4, 6], [1, 3, 5, 7]]
        moves = sum((_in_box(r) for r in res), [])
        assert (1, 1) in moves and (0, 1) in moves           # an accepted and a rejected in-box move
        st = smp.de_stats()
        assert st["attempts"] == 16 and st["failed"] == 0
        assert st["accepts"] == sum(int(r["accept"].sum()) for r in res)
        assert st["outbox"] == sum(int((r["mover"] & (1 - r["inbox"])).sum()) for r in res)
        assert st["moved"] == sum(int(r["nmove"][r["accept"] == 1].sum()) for r in res)
        assert smp.de_stats(reset=True) == st and smp.de_stats()["attempts"] == 0
    finally:
        smp.close()


def test_refusals():
    _dev()
    from mceik_amd import mcmc
    p = _problem()
    smp = mcmc.Sampler(p, nchains=3)
    try:
        with pytest.raises(ValueError):
            smp.de_enable(1)                                 # a population of 3
    finally:
        smp.close()
    smp = mcmc.Sampler(p, nchains=8)
    try:
        for kw in ({"every": 0}, {"every": 2, "offset": 2}, {"every": 2, "offset": -1}, {"every": 1, "gamma": 2.5},
                   {"every": 1, "gamma": 0.0}, {"every": 1, "cr": 0.0}, {"every": 1, "cr": 1.5}):
            with pytest.raises(ValueError):
                smp.de_enable(**kw)
        smp.temper_enable(betas=[1.0, 0.5, 0.25, 0.125], swap_every=1)
        with pytest.raises(ValueError):
            smp.de_enable(1)                                 # rungs of 2
        smp.temper_disable()
        smp.de_enable(1)
        with pytest.raises(ValueError):
            smp.temper_enable(betas=[1.0, 0.5, 0.25, 0.125], swap_every=1)
        g = smp.de_options()["gamma"]
        assert abs(g - 2.38 / np.sqrt(2 * 64)) < 1.0 / 65536
    finally:
        smp.close()


def test_p_and_s_phase_cycle():
    _dev()
    from mceik_amd import mcmc
    p = _ps_problem(seed=21)
    smp = mcmc.Sampler(p, nchains=4, v0=_near_models(p, 4, amp=2))
    try:
        smp.de_enable(1, gamma=0.4)
        phases = []
        for _ in range(4):
            v0 = smp.state()[0]
            r = _de_step(smp)
            v1 = smp.state()[0]
            ph = r["phase"]
            phases.append(ph)
            assert np.array_equal(v0[:, 1 - ph], v1[:, 1 - ph])          # the other phase's model is unchanged
        assert phases == [0, 0, 1, 1]
        # the other phase's current tables are unchanged too: logL from scratch equals the carried logL
        ck = smp.checkpoint()
        smp.restore(ck, recompute_logl=True)
        assert np.array_equal(_bits(smp.state()[1]), _bits(ck["logl"]))
    finally:
        smp.close()


def _edge_models(p):
    """Eight chains around one model: small differences in cells 8 .. 15, and in
    chains 2, 3, 6, 7 (half the chains) cell 0 at vmin and cell 1 at vmax."""
    from mceik_amd import mcmc
    base = mcmc.initial_models(p, [0])[0]
    v = np.tile(base, (8, 1))
    for c in range(8):
        v[c, 8 + c] += c + 1
    v[[2, 3, 6, 7], 0] = p.vmin
    v[[2, 3, 6, 7], 1] = p.vmax
    return v.astype(np.int32)


def test_box_edge_rejects_the_whole_move():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=11)
    smp = mcmc.Sampler(p, nchains=8, v0=_edge_models(p))
    try:
        smp.de_enable(1, gamma=2.0)
        assert smp.de_options()["gamma_q16"] == 131072
        res = [_de_step(smp) for _ in range(4)]              # each next step still matches: slow_prop was restored
        moves = sum((_in_box(r) for r in res), [])
        assert (0, 0) in moves and (1, 1) in moves           # an out-of-box mover and an in-box accept
        assert (1, 0) not in moves
        assert smp.de_stats()["outbox"] == sum(1 for m in moves if m[1] == 0) > 0
    finally:
        smp.close()


def _run(p, nchains, nsteps, setup, env, monkeypatch, max_samples=0, v0=None):
    """state, samples and DE statistics of a sampler set up by `setup`."""
    from mceik_amd import mcmc
    for k in ("MCEIK_PERSIST", "MCEIK_PIPES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    smp = mcmc.Sampler(p, nchains=nchains, max_samples=max_samples, v0=v0)
    try:
        setup(smp)
        smp.run(nsteps)
        v, l, na, _ = smp.state()
        out = {"v": v, "logl": l, "naccept": na, "npipe": smp.info()["npipe"]}
        if max_samples:
            out["samples"] = smp.samples()
        if smp._de is not None:
            out["stats"] = smp.de_stats()
            out["last"] = smp.de_last()
        return out
    finally:
        smp.close()


def _same_state(a, b):
    assert np.array_equal(a["v"], b["v"]) and np.array_equal(_bits(a["logl"]), _bits(b["logl"]))
    assert np.array_equal(a["naccept"], b["naccept"])


def test_pipes_do_not_change_a_bit(monkeypatch):
    _dev()
    p = _problem(seed=5)
    v0 = _near_models(p, 10)

    def setup(smp):
        smp.de_enable(3, gamma=0.3)

    one = _run(p, 10, 12, setup, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "1"}, monkeypatch, max_samples=12, v0=v0)
    two = _run(p, 10, 12, setup, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}, monkeypatch, max_samples=12, v0=v0)
    assert one["npipe"] == 1 and two["npipe"] == 2
    _same_state(one, two)
    assert one["stats"] == two["stats"] and one["stats"]["attempts"] == 4 * 5
    for x, y in zip(one["samples"], two["samples"]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    for k in one["last"]:
        assert np.array_equal(one["last"][k], two["last"][k]), k


def test_off_is_the_plain_sampler(monkeypatch):
    _dev()
    p = _problem(seed=9)

    def plain(smp):
        return None

    def on_off(smp):
        smp.de_enable(1)
        assert not smp.info()["multi_step"]
        smp.de_disable()
        assert smp.de_options()["every"] == 0

    def never(smp):
        smp.de_enable(100, offset=50)

    for env in ({}, {"MCEIK_PERSIST": "0", "MCEIK_PIPES": "2"}):
        a = _run(p, 4, 6, plain, env, monkeypatch)
        for setup in (on_off, never):
            _same_state(a, _run(p, 4, 6, setup, env, monkeypatch))


def test_tempering_keeps_partners_in_the_rung():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=13)
    smp = mcmc.Sampler(p, nchains=8, v0=_near_models(p, 8))
    try:
        smp.temper_enable(betas=[1.0, 0.25], swap_every=2)
        smp.de_enable(2, gamma=0.3)
        res = [_de_step(smp)]                                # step 0: no swap round before it
        smp.run(1)
        # step 2 is a swap round and a DE step.  The round runs first: a twin sampler makes it alone, from the
        # state before the step, and the DE step is restated from the twin's state
        ck = smp.checkpoint()
        assert ck["step"] == 2
        twin = mcmc.Sampler(p, nchains=8)
        try:
            twin.temper_enable(betas=[1.0, 0.25], swap_every=2)
            twin.restore({k: x for k, x in ck.items() if k != "de"})
            twin.temper_swap(1)                              # parity (2 / 2) & 1, drawn at step 2
            vs, ls, _, _ = twin.state()
        finally:
            twin.close()
        smp.run(1)
        r = DE.step(p, vs, ls, 2, (2, 0, round(0.3 * 65536), 65536), ntemps=2, beta=np.repeat([1.0, 0.25], 4))
        res.append(r)
        last = smp.de_last()
        for k in ("mover", "a", "b", "inbox", "nmove", "accept"):
            assert np.array_equal(last[k], r[k]), k
        assert np.array_equal(_bits(last["logl_prop"]), _bits(r["logl_prop"]))
        v1, l1, _, _ = smp.state()
        assert np.array_equal(v1, r["v"][:, 0]) and np.array_equal(_bits(l1), _bits(r["logl"]))
        for r in res:
            for c in np.flatnonzero(r["mover"]):
                assert r["a"][c] // 4 == r["b"][c] // 4 == c // 4        # partners stay inside the rung
    finally:
        smp.close()


def test_prior_enters_the_fold():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=17)
    vref = np.clip(p.v_true, p.vmin, p.vmax).astype(np.int32)
    smp = mcmc.Sampler(p, nchains=8, v0=_near_models(p, 8))
    try:
        smp.prior_enable(sigma_smooth=40.0, sigma_damp=60.0, vref=vref)
        smp.de_enable(1, gamma=0.3)
        ws, wd = mcmc.prior_weight(40.0), mcmc.prior_weight(60.0)
        _de_step(smp, prior=(ws, wd, vref))
        _de_step(smp, prior=(ws, wd, vref))
    finally:
        smp.close()


def test_moved_events_noise_and_statics_reach_logl():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=19)
    smp = mcmc.Sampler(p, nchains=8, v0=_near_models(p, 8))
    try:
        smp.hypo_enable(3, dmax=(1, 1, 1))
        smp.nuis_enable(3, offset=1, nsub=4, ladder=mcmc.nuis_ladder(11, 0.25, 4.0), statics_dt=1e-3, kcmax=20)
        smp.de_enable(3, gamma=0.3)
        _de_step(smp)                                        # step 0
        smp.run(5)                                           # nuisance, hypocentre, DE, nuisance, hypocentre
        kn, kc = smp.nuis_get()
        assert (smp.hypo_positions() != smp.hypo_positions()[0]).any() or kc.any() or (kn != 5).any()
        _de_step(smp)                                        # step 6
        assert smp.de_stats()["attempts"] == 12
    finally:
        smp.close()


def test_fp64_sampler():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=29)
    smp = mcmc.Sampler(p, nchains=8, precision=64, v0=_near_models(p, 8))
    try:
        smp.de_enable(1, gamma=0.3)
        _de_step(smp)
    finally:
        smp.close()


def test_standing_chains_cost_no_solve():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=31)
    smp = mcmc.Sampler(p, nchains=10)
    try:
        smp.de_enable(1)
        unskipped = int((np.asarray(p.skip)[0] == 0).sum())
        for movers in (5, 5):
            n0 = smp.fsm_solves()
            smp.run(1)
            assert smp.fsm_solves() - n0 == movers * unskipped
    finally:
        smp.close()


def test_checkpoint_after_an_odd_number_of_de_steps():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=37)
    v0 = _near_models(p, 8)
    smp = mcmc.Sampler(p, nchains=8, v0=v0)
    try:
        smp.de_enable(2, gamma=0.3)
        smp.run(5)                                           # DE steps 0, 2, 4: three of them
        ck = smp.checkpoint()
        assert ck["de"]["attempts"] == 12 and ck["de"]["gamma_q16"] == round(0.3 * 65536)
        smp.run(6)
        want = smp.state()
        st = smp.de_stats()
    finally:
        smp.close()
    smp = mcmc.Sampler(p, nchains=8, v0=v0)
    try:
        smp.de_enable(2, gamma=0.5)
        with pytest.raises(ValueError):
            smp.restore(ck)                                  # another gamma
        smp.de_enable(2, gamma=0.3)
        smp.restore(ck)
        assert smp.de_stats() == {k: ck["de"][k] for k in st}
        smp.run(6)
        got = smp.state()
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
        assert np.array_equal(got[2], want[2]) and got[3] == want[3]
        assert smp.de_stats() == st                          # counters rebased
    finally:
        smp.close()


def test_kept_step_on_a_de_step():
    _dev()
    from mceik_amd import mcmc
    p = _problem(seed=41)
    smp = mcmc.Sampler(p, nchains=8, max_samples=4, v0=_near_models(p, 8))
    try:
        smp.posterior_enable(per_chain=True, nbins=0)
        smp.de_enable(1, gamma=0.3)
        smp.run(1)                                           # a kept step (nburn = 0, keepK = 1) and a DE step
        v, l, _, _ = smp.state()
        sv, sl = smp.samples()[:2]
        assert np.array_equal(np.asarray(sv)[-1].reshape(v.shape), v)    # every chain, standing ones included
        assert np.array_equal(_bits(np.asarray(sl)[-1]), _bits(l))
        raw = smp.posterior_raw()
        assert raw["n"] == 1 and np.array_equal(raw["sum"], v.astype(np.int64))
    finally:
        smp.close()
