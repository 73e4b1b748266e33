"""The smoothness / reference-model prior, host side (no GPU): the two entry
points that run the kernels' arithmetic on the CPU (mceik_prior_energy,
mceik_prior_delta; csrc/prior.h), against the definition
restated here in numpy int64 on the whole model."""
import ctypes as C
import types

import numpy as np
import pytest

GRID = types.SimpleNamespace(ncx=5, ncy=4, ncz=3)


def _grid(ncx, ncy, ncz):
    return types.SimpleNamespace(ncx=ncx, ncy=ncy, ncz=ncz)


def _energy(g, v, vref=None):
    """Es = sum over face-adjacent pairs (v_i - v_j)^2, Ed = sum (v_i - vref_i)^2, int64."""
    a = np.asarray(v, np.int64).reshape(g.ncz, g.ncy, g.ncx)
    es = sum(int((np.diff(a, axis=ax) ** 2).sum()) for ax in range(3))
    ed = 0 if vref is None else int(((a.ravel() - np.asarray(vref, np.int64).ravel()) ** 2).sum())
    return es, ed


def _models(g, seed=3, lo=1500, hi=9000):
    rng = np.random.default_rng(seed)
    n = g.ncx * g.ncy * g.ncz
    return rng.integers(lo, hi + 1, n).astype(np.int32), rng.integers(lo, hi + 1, n).astype(np.int32)


def test_delta_is_the_energy_difference_exhaustive():
    from mceik_amd import mcmc
    v, vref = _models(GRID)
    e0 = _energy(GRID, v, vref)
    ncell = GRID.ncx * GRID.ncy * GRID.ncz
    seen_clipped = seen_full = 0
    for cell in range(ncell):
        for R in range(9):
            for amp in (1, -1, 7, -7, 300, -300):
                cells, dv = mcmc.block_footprint(GRID, cell, R, amp)
                vp = v.copy()
                vp[cells] += dv
                e1 = _energy(GRID, vp, vref)
                want = (e1[0] - e0[0], e1[1] - e0[1])
                assert mcmc.prior_delta(GRID, v, cell, R, amp, vref) == want, (cell, R, amp)
                # the opposite sign applied to v' leads back: the exact negation
                back = mcmc.prior_delta(GRID, vp, cell, R, -amp, vref)
                assert back == (-want[0], -want[1]), (cell, R, amp)
                # without a reference model the roughness is the same and the damping 0
                assert mcmc.prior_delta(GRID, v, cell, R, amp) == (want[0], 0), (cell, R, amp)
                seen_clipped += len(cells) < (2 * R + 1) ** 3
                seen_full += len(cells) == ncell
    assert seen_clipped and seen_full


@pytest.mark.parametrize("shape", [(5, 4, 3), (1, 1, 7), (7, 1, 1), (6, 6, 6), (1, 1, 1)])
def test_energy_is_numpy(shape):
    from mceik_amd import mcmc
    g = _grid(*shape)
    v, vref = _models(g, seed=sum(shape))
    assert mcmc.prior_energy(g, v, vref) == _energy(g, v, vref)
    assert mcmc.prior_energy(g, v) == (_energy(g, v)[0], 0)          # null vref: Ed = 0
    if shape == (1, 1, 1):
        assert mcmc.prior_energy(g, v) == (0, 0)
    flat = np.full_like(v, 4000)
    assert mcmc.prior_energy(g, flat, flat) == (0, 0)


def test_delta_on_a_line_and_a_single_cell():
    """Degenerate grids: no +y / +z pairs, and no pair at all."""
    from mceik_amd import mcmc
    for shape in ((1, 1, 7), (7, 1, 1), (1, 1, 1)):
        g = _grid(*shape)
        v, vref = _models(g, seed=11)
        e0 = _energy(g, v, vref)
        for cell in range(v.size):
            for R in (0, 1, 8):
                cells, dv = mcmc.block_footprint(g, cell, R, -300)
                vp = v.copy()
                vp[cells] += dv
                e1 = _energy(g, vp, vref)
                assert mcmc.prior_delta(g, v, cell, R, -300, vref) == (e1[0] - e0[0], e1[1] - e0[1]), (shape, cell, R)


def test_null_outputs_and_raw_return_codes():
    from mceik_amd import _lib
    L = _lib.lib()
    v, vref = _models(GRID)
    pv, pr = v.ctypes.data_as(C.c_void_p), vref.ctypes.data_as(C.c_void_p)
    es, ed = C.c_longlong(-1), C.c_longlong(-1)
    assert L.mceik_prior_energy(5, 4, 3, pv, pr, None, None) == 0
    assert L.mceik_prior_energy(5, 4, 3, pv, pr, C.byref(es), None) == 0 and es.value == _energy(GRID, v)[0]
    assert L.mceik_prior_energy(5, 4, 3, pv, None, None, C.byref(ed)) == 0 and ed.value == 0
    assert L.mceik_prior_delta(5, 4, 3, pv, pr, 17, 2, 5, None, None) == 0
    assert L.mceik_prior_energy(5, 4, 3, None, pr, C.byref(es), C.byref(ed)) == 1
    assert L.mceik_prior_energy(0, 4, 3, pv, pr, C.byref(es), C.byref(ed)) == 1
    assert L.mceik_prior_energy(5, -4, 3, pv, pr, C.byref(es), C.byref(ed)) == 1
    assert L.mceik_prior_energy(1 << 16, 1 << 16, 1, pv, pr, C.byref(es), C.byref(ed)) == 1       # > INT_MAX cells
    assert L.mceik_prior_delta(5, 4, 3, None, pr, 17, 2, 5, C.byref(es), C.byref(ed)) == 1
    for cell, R, amp in ((-1, 1, 5), (60, 1, 5), (0, -1, 5), (0, 9, 5), (0, 1, 0), (0, 1, -2 ** 31)):
        assert L.mceik_prior_delta(5, 4, 3, pv, pr, cell, R, amp, C.byref(es), C.byref(ed)) == 1, (cell, R, amp)


def test_bad_arguments_raise():
    from mceik_amd import mcmc
    v, vref = _models(GRID)
    for cell, R, amp in ((-1, 1, 5), (60, 1, 5), (0, -1, 5), (0, 9, 5), (0, 1, 0)):
        with pytest.raises(ValueError):
            mcmc.prior_delta(GRID, v, cell, R, amp, vref)
    with pytest.raises(ValueError):
        mcmc.prior_energy(GRID, v[:-1])
    with pytest.raises(ValueError):
        mcmc.prior_energy(GRID, v, vref[:-1])
    with pytest.raises(ValueError):
        mcmc.prior_energy(_grid(0, 4, 3), v)
    with pytest.raises(ValueError):
        mcmc.prior_delta(GRID, v[:-1], 0, 0, 1)


def test_overflow_refusal():
    """3 ncell span^2 >= 2^53 is refused: below it every energy and difference is an integer a double holds.
    One cell: the largest span with 3 span^2 < 2^53 passes and the next one does not."""
    from mceik_amd import mcmc
    one = _grid(1, 1, 1)
    span = int(np.floor(np.sqrt(float(2 ** 53) / 3.0)))
    while 3 * (span + 1) ** 2 < 2 ** 53:
        span += 1
    while 3 * span ** 2 >= 2 ** 53:
        span -= 1
    assert 3 * span ** 2 < 2 ** 53 <= 3 * (span + 1) ** 2
    v = np.array([1], np.int32)
    assert mcmc.prior_energy(one, v, np.array([1 + span], np.int32)) == (0, span ** 2)
    with pytest.raises(ValueError):
        mcmc.prior_energy(one, v, np.array([2 + span], np.int32))
    # the amplitude counts twice: span + 2 |amp|
    ok = np.array([1 + span - 2 * 300], np.int32)
    assert mcmc.prior_delta(one, v, 0, 0, -300, ok) == (0, -300 * (2 * (1 - int(ok[0])) - 300))
    with pytest.raises(ValueError):
        mcmc.prior_delta(one, v, 0, 0, -300, np.array([2 + span - 2 * 300], np.int32))
    # the cell count enters: 6^3 cells of range 7500 pass, a range of 2^31 - 2 does not
    g = _grid(6, 6, 6)
    a, _ = _models(g)
    assert mcmc.prior_energy(g, a)[0] == _energy(g, a)[0]
    a[0], a[1] = 1, 2 ** 31 - 1
    assert 3 * 216 * (2 ** 31 - 2) ** 2 >= 2 ** 53
    with pytest.raises(ValueError):
        mcmc.prior_energy(g, a)
    with pytest.raises(ValueError):
        mcmc.prior_delta(g, a, 0, 0, 1)


def test_sigma_to_weight():
    from mceik_amd import mcmc
    assert mcmc.prior_weight(None) == (0.0, 0.0)
    assert mcmc.prior_weight(200.0) == (1.0 / (2.0 * 200.0 * 200.0),) * 2
    assert mcmc.prior_weight((150, None)) == (1.0 / (2.0 * 150.0 * 150.0), 0.0)
    for bad in (0.0, -1.0, float("inf"), float("nan"), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            mcmc.prior_weight(bad)
