"""Block proposals, host side (no GPU): the footprint of one proposal
(mceik_block_footprint, the arithmetic the two kernels of csrc/block.hip share;
DESIGN.md s.12), against the definition restated here."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest

GRID = types.SimpleNamespace(ncx=5, ncy=4, ncz=3)


def _fp(cell, radius, amp, g=GRID):
    from mceik_amd import mcmc
    return mcmc.block_footprint(g, cell, radius, amp)


def _xyz(cells, g=GRID):
    cells = np.asarray(cells)
    return cells % g.ncx, cells // g.ncx % g.ncy, cells // (g.ncx * g.ncy)


def _restated(cell, R, amp, g=GRID):
    """dv = floor(mag w / (R+1)^3) per in-grid offset, x fastest, zeros dropped."""
    cx, cy, cz = cell % g.ncx, cell // g.ncx % g.ncy, cell // (g.ncx * g.ncy)
    mag, out = abs(amp), []
    for dz, dy, dx in itertools.product(range(-R, R + 1), repeat=3):
        x, y, z = cx + dx, cy + dy, cz + dz
        if not (0 <= x < g.ncx and 0 <= y < g.ncy and 0 <= z < g.ncz):
            continue
        d = mag * (R + 1 - abs(dx)) * (R + 1 - abs(dy)) * (R + 1 - abs(dz)) // (R + 1) ** 3
        if d:
            out.append(((z * g.ncy + y) * g.ncx + x, -d if amp < 0 else d))
    return out


def test_radius_zero_is_one_cell():
    for cell in (0, 17, 59):
        for amp in (1, -1, 300, -299):
            cells, dv = _fp(cell, 0, amp)
            assert cells.tolist() == [cell] and dv.tolist() == [amp]
            assert cells.dtype == np.int32 and dv.dtype == np.int32


def test_symmetry_exhaustive():
    ncell = GRID.ncx * GRID.ncy * GRID.ncz
    for cell in range(ncell):
        for R in range(9):
            for mag in (1, 7, 300):
                cp, dp = _fp(cell, R, mag)
                cm, dm = _fp(cell, R, -mag)
                assert cp.tobytes() == cm.tobytes() and dp.tobytes() == (-dm).tobytes(), (cell, R, mag)
                assert (dp > 0).all() and dp[cp.tolist().index(cell)] == mag
                want = _restated(cell, R, mag)
                assert list(zip(cp.tolist(), dp.tolist())) == want, (cell, R, mag)


def test_clipping_at_a_corner():
    ncell = GRID.ncx * GRID.ncy * GRID.ncz
    for cell in (0, GRID.ncx - 1, ncell - 1, ncell - GRID.ncx):
        cells, dv = _fp(cell, 2, 300)
        assert 0 < len(cells) <= 27 and len(set(cells.tolist())) == len(cells)
        assert cells.min() >= 0 and cells.max() < ncell
        x, y, z = _xyz(cells)
        cx, cy, cz = _xyz(cell)
        assert (abs(x - cx) <= 2).all() and (abs(y - cy) <= 2).all() and (abs(z - cz) <= 2).all()
    # an interior-most centre of a grid large enough keeps all (2R+1)^3 cells
    big = types.SimpleNamespace(ncx=7, ncy=7, ncz=7)
    cells, dv = _fp((3 * 7 + 3) * 7 + 3, 2, 300, big)
    assert len(cells) == 125 and dv.sum() == sum(d for _, d in _restated((3 * 7 + 3) * 7 + 3, 2, 300, big))


def test_radius_eight_covers_the_grid():
    ncell = GRID.ncx * GRID.ncy * GRID.ncz
    for cell in (0, 31, ncell - 1):
        cells, dv = _fp(cell, 8, 300)
        assert sorted(cells.tolist()) == list(range(ncell))
        assert cells.tolist() == list(range(ncell))          # x fastest, clipped: ascending cell order
        assert (dv > 0).all()


def test_null_outputs_return_the_count():
    from mceik_amd import _lib
    f = _lib.lib().mceik_block_footprint
    for cell, R, amp in ((0, 2, 300), (31, 8, -7), (17, 0, 1), (31, 3, 1)):
        cells, dv = _fp(cell, R, amp)
        assert f(5, 4, 3, cell, R, amp, None, None) == len(cells)
        only = np.full(len(cells) + 1, -9, np.int32)
        assert f(5, 4, 3, cell, R, amp, only.ctypes.data_as(C.c_void_p), None) == len(cells)
        assert only[:-1].tobytes() == cells.tobytes() and only[-1] == -9
        only[:] = -9
        assert f(5, 4, 3, cell, R, amp, None, only.ctypes.data_as(C.c_void_p)) == len(cells)
        assert only[:-1].tobytes() == dv.tobytes() and only[-1] == -9
    # mag 1 at R 3: only the centre's weight reaches (R+1)^3
    assert f(5, 4, 3, 31, 3, 1, None, None) == 1


def test_monotone_along_every_axis():
    g = types.SimpleNamespace(ncx=9, ncy=8, ncz=7)
    centre = (3 * g.ncy + 4) * g.ncx + 4
    for R in range(9):
        for mag in (1, 7, 300):
            cells, dv = _fp(centre, R, mag, g)
            field = np.zeros(g.ncx * g.ncy * g.ncz, np.int64)
            field[cells] = np.abs(dv)
            field = field.reshape(g.ncz, g.ncy, g.ncx)
            for axis, c in ((2, 4), (1, 4), (0, 3)):
                up = np.moveaxis(field, axis, 0)
                assert (np.diff(up[c:], axis=0) <= 0).all(), (R, mag, axis)       # away from the centre: no growth
                assert (np.diff(up[:c + 1], axis=0) >= 0).all(), (R, mag, axis)


def test_bad_arguments():
    from mceik_amd import mcmc
    for cell, R, amp in ((-1, 1, 5), (60, 1, 5), (0, -1, 5), (0, 9, 5), (0, 1, 0)):
        with pytest.raises(ValueError):
            mcmc.block_footprint(GRID, cell, R, amp)
