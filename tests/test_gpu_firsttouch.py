"""First-touch z-blocks: the fixed-layout fp32 instances of
fsm16_kernel.hip do not fill the field with u_nan before a solve.  A z-block
is "touched" once all of its 8 KiB in HBM is valid for the current solve; an
untouched block is u_nan by definition, its loads are redirected to a line of
u_nan behind the field, its first visit writes it whole, and the end of the
solve fills what no visit wrote.  Whatever the field's slot held before --
the previous solve of the same wave, the previous call on the same workspace
-- must never reach a result.  Everything here is bitwise against the fp32
twin (oracle/fsm_impl.inc), with test_gpu_hold's helpers.
"""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from test_gpu_hold import H, NREF, _batch, _check, _dev, _expand, _inclusions, _problem

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _fixed_instance(bs, nmodel, nstat, nsrc):
    from mceik_amd import _lib
    return _lib.lib().mceik_fsm_kernel_name(C.byref(bs.describe(nmodel, nstat, nsrc, 1))).decode()


def _twin(scell_m, src_s, n3, maxit=50, max_sweeps=-1):
    nx, ny, nz = n3
    return O.eikonal_solve(nx, ny, nz, _expand(scell_m, nx, ny, nz).astype(np.float32), H, src_s, maxit=maxit,
                           tol=1e-8, dtype=np.float32, max_sweeps=max_sweeps)


def test_stale_slot_poison():
    """40^3, one wave: four solves that alternate a fast model (9000 m/s
    everywhere) with a slow high-contrast one (6500 m/s, 700 m/s inclusions)
    and change the source every time, handed out in that order.  Without
    fields the four solves share one field slot; with fields every solve has
    its own, which the second call (models reversed, same solver and
    workspace) reuses.  A segment leaked from a fast solve would win every
    min of the slow solve that follows it."""
    dev = _dev()
    n = 40
    ncell = n // 4
    slow_v = _inclusions(1, ncell, ncell, ncell, 5)[0]
    v = np.stack([np.full_like(slow_v, 9000), slow_v])
    scell = (1.0 / v.astype(np.float32)).astype(np.float32)
    src = np.array([[[0.0, 0.37 * (n - 1) * H, 0.61 * (n - 1) * H, (n - 1) * H]],
                    [[0.2, 0.83 * (n - 1) * H, 0.12 * (n - 1) * H, 0.45 * (n - 1) * H]]])
    ev = np.random.default_rng(9).integers(0, n ** 3, 24).astype(np.int32)
    order = [0, 3, 1, 2]                        # (model 0, source 0), (1, 1), (0, 1), (1, 0)
    bs = _batch(n, n, n, 32, 50)
    assert _fixed_instance(bs, 2, 2, 1).startswith("fsm16_solve_kernel<2"), "the fixed-layout instance"
    twin = {(m, s): _twin(scell[m], src[s], (n, n, n)) for m in range(2) for s in range(2)}
    for models in ((0, 1), (1, 0)):
        sl = torch.tensor(scell[list(models)].reshape(2, -1), device=dev)
        for want_fields in (False, True):
            out = bs.solve(torch.tensor(src), sl, ev_node=torch.tensor(ev), want_fields=want_fields, max_waves=1,
                           solve_order=order)
            assert out["step_z"] == 16
            tt = out["ttab"].cpu().numpy()
            for q in range(4):
                t, ierr, it = twin[(models[q // 2], q % 2)]
                assert np.array_equal(tt[q].view(np.uint32), t[ev].view(np.uint32)), (models, want_fields, q)
                assert int(out["niter"][q]) == it and int(out["ierr"][q]) == ierr, (models, want_fields, q)
                if want_fields:
                    u = out["u"][q].cpu().numpy().ravel()
                    bad = np.flatnonzero(u.view(np.uint32) != t.view(np.uint32))
                    assert bad.size == 0, (models, q, bad.size, int(bad[0]), float(u[bad[0]]), float(t[bad[0]]))


def test_every_sweep_budget():
    """(30, 26, 67), cut tiles in x and y and a cut last brick in z: the
    partial field after every sweep budget equals the twin's.  Early budgets
    leave most blocks untouched (the end-of-solve fill), later ones none."""
    dev = _dev()
    nx, ny, nz = 30, 26, 67
    scell, src = _problem(nx, ny, nz, 2, 31)
    bs = _batch(nx, ny, nz, 32, 50)
    assert _fixed_instance(bs, 2, 2, 1).startswith("fsm16_solve_kernel<2"), "the fixed-layout instance"
    sl = torch.tensor(scell.reshape(2, -1), device=dev)
    full = bs.solve(torch.tensor(src), sl, want_fields=True, max_waves=1)
    assert full["step_z"] == 16
    _check(full, scell, src, nx, ny, nz, 32, 50)
    niter = int(full["niter"].max())
    assert niter >= 4, niter
    for ms in range(1, 8 * niter + 1):
        out = bs.solve(torch.tensor(src), sl, want_fields=True, max_waves=1, max_sweeps=ms)
        _check(out, scell, src, nx, ny, nz, 32, 50, max_sweeps=ms)


def test_source_placement():
    """Source boxes in more than one z-block: next to the grid's first and
    at its last corner, across a tile corner and the z-block boundary
    (nodes x, y = 7 / 8, z = 31 / 32: eight blocks), and two sources per
    solve (nsrc 2) whose boxes share blocks.  Full solves and the first
    budgets, where almost every block is still untouched."""
    dev = _dev()
    nx, ny, nz = 30, 26, 67
    scell, _ = _problem(nx, ny, nz, 2, 83)
    scell = scell[1:]
    one = np.array([[[0.0, 0.3 * H, 0.3 * H, 0.3 * H]],
                    [[0.1, (nx - 1) * H, (ny - 1) * H, (nz - 1) * H]],
                    [[0.0, 7.5 * H, 7.5 * H, 31.5 * H]]])
    two = np.array([[[0.0, 7.5 * H, 7.5 * H, 31.5 * H], [0.05, 8.4 * H, 7.6 * H, 31.6 * H]],
                    [[0.3, 0.3 * H, 15.5 * H, 63.5 * H], [0.0, 23.6 * H, 8.2 * H, 32.4 * H]]])
    bs = _batch(nx, ny, nz, 32, 50)
    sl = torch.tensor(scell.reshape(1, -1), device=dev)
    for src in (one, two):
        assert _fixed_instance(bs, 1, len(src), src.shape[1]).startswith("fsm16_solve_kernel<2")
        for ms in (-1, 1, 2, 3, 9):
            out = bs.solve(torch.tensor(src), sl, want_fields=True, max_waves=1, max_sweeps=ms)
            assert out["step_z"] == 16
            _check(out, scell, src, nx, ny, nz, 32, 50, max_sweeps=ms)


def test_multi_step_launch(monkeypatch):
    """The multi-step sampler launch (fsm16_solve_kernel<2, 1, true>) shares
    the sweep: 3 steps of 8 chains equal the per-step launches bit for bit."""
    _dev()
    from test_gpu_multistep import _problem as mc_problem, _run
    p = mc_problem("P")
    ia, a, _ = _run(p, 8, 3, True, monkeypatch)
    ib, b, _ = _run(p, 8, 3, False, monkeypatch)
    assert ia["multi_step"] and not ib["multi_step"] and ia["step_z"] == 16
    assert ia["fixed_layout"] and ia["kernel"].startswith("fsm16_solve_kernel<2"), ia["kernel"]
    for n, x, y in zip(("v", "logl", "naccept", "step", "kept v", "kept logl", "tables", "accept"), a, b):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), n
        else:
            assert x == y, n
