"""Host-side pieces of the noise-scale and station-static moves (include/mceik.h
mceik_mcmc_nuis_*, mceik_nuis_draw): no GPU needed.

Sub-move `sub` of global chain g at step gs is restated from the oracle's
Philox4x32-10 and det_log:

    r = philox(counter {gs lo, gs hi, 3, sub}, key {g, seed})
    M = nnoise + nact[0] + nact[1];  q = (r[0] * M) >> 32
    q < nnoise: noise move of phase q by +-d, d = 1 + ((r[1] * dk) >> 32), minus iff r[2] & 1
    else, q -= nnoise: phase 0 iff q < nact[0]; a = q (- nact[0]); b = (r[1] * (nact - 1)) >> 32, b += b >= a;
          mag = 1 + (((r[2] >> 1) * dc) >> 31), minus iff r[2] & 1
    log u = det_log((r[3] + 0.5) / 2^32)
"""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from test_hypo_host import _offsets_c


def restated_draw(seed, gid, gs, sub, nnoise, nact, dk, dc):
    """((kind, phase, a, b, delta), log u)."""
    r = [int(x) for x in O.philox([gs & 0xFFFFFFFF, gs >> 32, 3, sub], [gid, seed])]
    na = list(nact) + [0, 0]
    q = (r[0] * (nnoise + na[0] + na[1])) >> 32
    sign = -1 if r[2] & 1 else 1
    logu = O.lib().oracle_det_log((float(r[3]) + 0.5) * (1.0 / 4294967296.0))
    if q < nnoise:
        return (0, q, 0, 0, sign * (1 + ((r[1] * dk) >> 32))), logu
    q -= nnoise
    ph = 0 if q < na[0] else 1
    a = q - (na[0] if ph else 0)
    b = (r[1] * (na[ph] - 1)) >> 32
    b += b >= a
    return (1, ph, a, b, sign * (1 + (((r[2] >> 1) * dc) >> 31))), logu


@pytest.mark.parametrize("seed,gid,gs,nnoise,nact,dk,dc", [
    (2016, 0, 0, 1, (4,), 2, 3),
    (2016, 3, 1, 2, (4, 3), 1, 1),
    (7, 1023, 11, 2, (0, 0), 5, 0),                   # noise only
    (7, 5, (1 << 32) + 9, 0, (4, 4), 0, 7),           # statics only; a step past 2^32: the counter's high word
    (7, 5, 3, 0, (2,), 0, 0),                         # nact = 2: the partner is the other station; dk = dc = 0
    (7, 6, 3, 1, (0, 2), 0, 0),                       # only the S phase has statics
    (0xFFFFFFFF, 0xFFFFFFFF, (1 << 40) - 1, 2, (100, 1000), 40, 1000),
])
def test_draw_equals_the_philox_restatement(seed, gid, gs, nnoise, nact, dk, dc):
    from mceik_amd import mcmc
    kinds = set()
    for sub in range(64):
        m, logu = mcmc.nuis_draw(seed, gid, gs, sub, nnoise, nact, dk, dc)
        mr, lr = restated_draw(seed, gid, gs, sub, nnoise, nact, dk, dc)
        assert m == mr, (sub, m, mr)
        assert np.float64(logu).tobytes() == np.float64(lr).tobytes() and logu < 0.0
        kind, ph, a, b, delta = m
        kinds.add(kind)
        if kind == 0:
            assert 0 <= ph < nnoise and 1 <= abs(delta) <= max(dk, 1)
        else:
            na = (list(nact) + [0])[ph]
            assert na >= 2 and 0 <= a < na and 0 <= b < na and a != b and 1 <= abs(delta) <= max(dc, 1)
    if nnoise + sum(nact) <= 12:                        # 64 draws over so few moves meet both kinds
        assert kinds == ({0} if not sum(nact) else {1} if not nnoise else {0, 1})
    else:
        assert kinds <= {0, 1}


def test_pair_draw_is_zero_sum_and_covers_its_range():
    """10^4 statics draws applied to a table of statics: each phase's sum never leaves 0, every station is drawn as
    a and as b, and every magnitude of [1, dc] turns up with both signs."""
    from mceik_amd import mcmc
    nact, dc = (5, 3), 4
    kc = [np.zeros(n, np.int64) for n in nact]
    seen_a, seen_b, mags = [set(), set()], [set(), set()], set()
    n = 0
    for gs in range(40):
        for sub in range(250):
            (kind, ph, a, b, delta), _ = mcmc.nuis_draw(11, gs % 7, gs, sub, 0, nact, 0, dc)
            assert kind == 1 and a != b
            kc[ph][a] += delta
            kc[ph][b] -= delta
            assert kc[0].sum() == 0 and kc[1].sum() == 0
            seen_a[ph].add(a)
            seen_b[ph].add(b)
            mags.add(delta)
            n += 1
    assert n == 10000
    assert [sorted(s) for s in seen_a] == [list(range(5)), list(range(3))] == [sorted(s) for s in seen_b]
    assert sorted(mags) == [-4, -3, -2, -1, 1, 2, 3, 4]
    assert any(k.any() for k in kc)


def test_draw_refuses_bad_arguments():
    from mceik_amd import mcmc
    for kw in (dict(sub=-1), dict(nnoise=3), dict(nnoise=-1), dict(nact=(1,)), dict(nact=(4, 1)), dict(nact=(-2,)),
               dict(dk=-1), dict(dc=-1), dict(nnoise=0, nact=(0, 0)), dict(nact=(2, 2, 2))):
        a = dict(seed=1, gchain=0, step=0, sub=0, nnoise=1, nact=(4,), dk=1, dc=1)
        a.update(kw)
        with pytest.raises(ValueError):
            mcmc.nuis_draw(**a)


@pytest.mark.parametrize("nk,lam_max", [(1, 1.0), (3, 2.0), (9, 4.0), (41, 10.0), (101, 1e3)])
def test_ladder_middle_entry_is_exact(nk, lam_max):
    from mceik_amd import mcmc
    lam, lnlam = mcmc.nuis_ladder(nk, 1.0 / lam_max, lam_max)
    assert lam.dtype == lnlam.dtype == np.float64 and lam.shape == lnlam.shape == (nk,)
    assert lam[nk // 2].tobytes() == np.float64(1.0).tobytes() and lnlam[nk // 2].tobytes() == np.float64(0.0).tobytes()
    assert (np.diff(lnlam) > 0).all() if nk > 1 else True
    assert np.allclose(np.diff(lnlam), np.log(lam_max) / max(nk // 2, 1), rtol=1e-12) and np.allclose(np.log(lam), lnlam)
    assert np.isclose(lam[-1], lam_max) and np.isclose(lam[0], 1.0 / lam_max)
    assert np.array_equal(lnlam, -lnlam[::-1])          # log-uniform around lam = 1
    assert mcmc.nuis_ladder(nk, None, lam_max)[0].tobytes() == lam.tobytes()


def test_ladder_refuses_bad_arguments():
    from mceik_amd import mcmc
    for args in ((8, 0.25, 4.0), (0, 0.25, 4.0), (9, 0.5, 4.0), (9, 2.0, 0.5), (9, None, float("inf"))):
        with pytest.raises(ValueError):
            mcmc.nuis_ladder(*args)


def test_active_stations():
    """The stations statics moves draw from: a used pick of the phase, in station order."""
    import dataclasses
    from mceik_amd import mcmc
    p = mcmc.make_problem("C2", n=24, nstat=4, nev=3, phases="PS", picks="analytic")
    assert [a.tolist() for a in mcmc.nuis_active(p)] == [[0, 1, 2, 3], [0, 1, 2, 3]]
    luse = p.luse.copy()
    luse[(p.obs_stat == 2) & (p.obs_phase == 1)] = 0     # station 2 loses its S picks
    q = dataclasses.replace(p, luse=luse, _keep=[])
    assert [a.tolist() for a in mcmc.nuis_active(q)] == [[0, 1, 2, 3], [0, 1, 3]]


def test_struct_layout_matches_the_header():
    from mceik_amd import _lib
    names = [f[0] for f in _lib.NuisOpts._fields_]
    c = _offsets_c("mceik.h", "mceik_nuis_opts", names)
    assert C.sizeof(_lib.NuisOpts) == c["sizeof"] == 72
    for n in names:
        assert getattr(_lib.NuisOpts, n).offset == c[n], n
    assert names == ["every", "offset", "nsub", "noise", "statics", "nk", "dk", "dc", "kcmax", "dt", "lam", "lnlam",
                     "norm"]
