"""Which sweep-kernel instance a batch launches and how much LDS a wave takes
(host-side: mceik_fsm_kernel_name / mceik_fsm_lds_bytes, no GPU).

The sampler's instances at the bench's C3 geometry, and the fp64 compact LDS
layout (fsm_common.h fsm_compact_layout: 16-bit block clocks, meta-only
column words) that gives the fp64 instance 8 waves per CU: 160 KiB of LDS
per CU / 8 = 20480 B per wave at most.  Geometries outside the compact
layout's bounds fall back to the runtime-kb instance."""
import ctypes as C

import numpy as np
import pytest

import _refinement as R

pytest.importorskip("torch")

LDS_PER_CU = 160 * 1024


def _batch(n, precision, fast=True, nstat=32, nmodel=1024, nref=(4, 4, 4), nxy=None):
    from mceik_amd.eikonal import BatchSolver
    nx = ny = nxy or n
    bs = BatchSolver(nx, ny, n, 100.0, 0.0, 0.0, 0.0, 50, 1e-8, precision, nref=nref, fast_sqrt=fast)
    return bs.describe(nmodel, nstat, 1, 1, nev=32)


def _info(b):
    from mceik_amd import _lib
    L = _lib.lib()
    return L.mceik_fsm_kernel_name(C.byref(b)).decode(), int(L.mceik_fsm_lds_bytes(C.byref(b)))


def test_c3_fp32_sampler_instance():
    name, lds = _info(_batch(128, 32))
    assert name == "fsm16_solve_kernel<2, 1>"
    assert lds <= LDS_PER_CU // 8, lds                  # 8 waves/CU (the VGPR limit)


def test_c3_fp64_sampler_instance_compact_layout():
    """bench.py's f64 record: the short-sqrt fp64 instance, compact LDS."""
    name, lds = _info(_batch(128, 64))
    assert name == "fsm_solve_kernel<double, 2, true, 2, 1, 4>"
    assert lds <= LDS_PER_CU // 8, lds                  # 8 waves/CU; the int layout took 25456 B (6)
    exact, _ = _info(_batch(128, 64, fast=False))
    assert exact == "fsm_solve_kernel<double, 2, false, 2, 1, 4>"


@pytest.mark.parametrize("nz,nxy", [(20, None), (32, 264)], ids=["kb3", "over_1024_blocks"])
def test_fp64_runtime_kb_fallback(nz, nxy):
    """kb != MCEIK_KB (nz = 20: 3 bricks) or more than MCEIK_MAX_BLOCKS z-blocks
    (264 x 264 x 32: 33 x 33 tiles x 1 block): the runtime-kb instance with
    int clocks (the compact layout's 16-bit clocks are bounded for <= 1024)."""
    name, _ = _info(_batch(nz, 64, nxy=nxy, nstat=2, nmodel=1))
    assert name == "fsm_solve_kernel<double, 2, false, 2, 1, 0>"


# ---- refinements other than 4 (tests/_refinement.py; the GPU side is tests/test_gpu_refinement.py) ----

def _cells(geo, nref, precision, fast, step_z, nmodel=2, nstat=3, nev=7):
    from mceik_amd.eikonal import BatchSolver
    bs = BatchSolver(*geo, 100.0, 0.0, 0.0, 0.0, 50, 1e-8, precision, nref=nref, fast_sqrt=fast)
    return bs.describe(nmodel, nstat, 1, 1, nev=nev, step_z=step_z)


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_refinement_instance(case):
    """The instance fill_launch / variant() / use_fsm16() pick per refinement
    class; every launch of the table is one the solve accepts."""
    from mceik_amd import _lib
    _, geo, nref, precision, fast, step_z, want = case
    b = _cells(geo, nref, precision, fast, step_z)
    name, lds = _info(b)
    assert name == want
    L = _lib.lib()
    assert L.mceik_fsm_step_z(C.byref(b)) == (16 if want.startswith("fsm16") else 8)
    assert L.mceik_fsm_check(C.byref(b)) == 0
    assert 0 < lds <= 64 * 1024


def test_refinement_table_reaches_every_cell_mode_instance():
    """Each of the 13 slow_mode 1 names of fsm_launch_name is selected by a
    row of the table whose nref is not (4, 4, 4)."""
    got = {_info(_cells(geo, nref, precision, fast, step_z))[0]
           for _, geo, nref, precision, fast, step_z, _ in R.CASES if tuple(nref) != (4, 4, 4)}
    assert len(R.CELL_MODE_NAMES) == 13
    assert got == R.CELL_MODE_NAMES, got ^ R.CELL_MODE_NAMES


def _magic_exact(n, nr):
    """The kernels' node -> cell map (tile_cells / column_tile / load_f):
    (node * ceil(2^20 / nr)) >> 20 in unsigned 32-bit arithmetic, against
    node / nr for every node of an axis of n nodes."""
    node = np.arange(n, dtype=np.uint32)
    magic = np.uint32(((1 << 20) + nr - 1) // nr)
    return bool(np.array_equal((node * magic) >> np.uint32(20), node // np.uint32(nr)))    # wraps mod 2^32


MAGIC_N = (8, 64, 1024, 3850, 4095, 4104, 16392)
MAGIC_NR = tuple(range(1, 301)) + (1000, 4095)


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_cell_map_exact_or_refused(axis, capfd):
    """For every axis length and refinement: the node -> cell multiply is
    exact on the whole axis, or the launch is refused (non-zero, with a
    message).  Nothing small is refused: every refusal at n <= 1024 and
    nr <= 64 would have to be inexact (there is none)."""
    from mceik_amd import _lib
    L = _lib.lib()
    refused_inexact = 0
    for n in MAGIC_N:
        for nr in MAGIC_NR:
            geo, nref = [8, 8, 8], [1, 1, 1]
            geo[axis], nref[axis] = n, nr
            for precision in (32, 64):
                b = _cells(tuple(geo), tuple(nref), precision, True, 0, nmodel=1, nstat=1, nev=0)
                rc = L.mceik_fsm_check(C.byref(b))
                err = capfd.readouterr().err
                exact = _magic_exact(n, nr)
                if rc == 0:
                    assert exact, (n, nr, precision)
                else:
                    assert err.strip(), (n, nr, precision)
                    if n <= 1024 and nr <= 64:
                        assert not exact, (n, nr, precision, err)
                    if n <= 4096:           # longer axes are refused as such
                        assert not exact and "not exact" in err, (n, nr, precision, err)
                        refused_inexact += 1
    # nr = 275 at node 3849 is the first miss (n = 3850 and 4095 both hold it)
    assert refused_inexact > 0


def test_cell_map_refusal_is_the_solve_and_the_sampler(capfd):
    """The refusal mceik_fsm_check pins is what mceik_fsm_batch_solve and
    Sampler creation return (both before any GPU call)."""
    from mceik_amd import _lib, mcmc
    L = _lib.lib()
    assert not _magic_exact(3850, 275) and _magic_exact(3850, 274)
    b = _cells((3850, 8, 8), (275, 1, 1), 32, True, 0, nmodel=1, nstat=1, nev=0)
    assert L.mceik_fsm_batch_solve(C.byref(b), None, 0, None) == 1
    assert "not exact" in capfd.readouterr().err
    b = _cells((4104, 9, 10), (1, 1, 1), 32, True, 0, nmodel=1, nstat=1, nev=0)
    assert L.mceik_fsm_batch_solve(C.byref(b), None, 0, None) == 1
    assert "invalid batch description" in capfd.readouterr().err
    p = mcmc.make_problem("C2", n=8, nstat=2, nev=2, nref=(275, 1, 1), picks="analytic")
    p.nx = 3850
    p.v_true = np.full(p.ncell, 4000, np.int32)
    with pytest.raises(RuntimeError, match=r"mceik_mcmc_init failed \(1\)"):
        mcmc.Sampler(p, nchains=1)
    assert "not exact" in capfd.readouterr().err
