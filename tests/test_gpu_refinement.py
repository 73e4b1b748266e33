"""The sweep kernels at inversion-cell refinements other than (4, 4, 4)
(tests/_refinement.py: the refinement classes and the instance each selects;
tests/test_fsm_instances.py pins the selection host-side).

At refinement 4 with 8-node tiles every cell quantity is a power of two and
tile-aligned; here cells straddle tile edges, z-blocks hold 11 or 12 z cells,
the node -> cell multiply has an error term, a cell spans two tiles or the
whole grid, and nref = 1 (the library default) runs the uncached per-cell
path.  Every case is bitwise against the twin on the expanded node field
(fp32: the stable-update twin, fp64: the reference's arithmetic), fields,
event tables, iterations and ierr, and proves that a one-node shift of the
cell map along x would have changed the twin.  The sampler runs at
(6, 6, 4), (3, 3, 3) and (1, 1, 1) against oracle_mcmc_run.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O
import _refinement as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

H = 100.0
NMODEL = 2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _sources(nz):
    # the bottom face (off-node in x, y), inside the grid off-node, and a start time of 0.1 s
    return np.array([[[0.0, 1234.5, 987.6, (nz - 1) * H]], [[0.0, 2130.0, 440.0, 1260.0]],
                     [[0.1, 1500.0, 1200.0, 1700.0]]])


@functools.lru_cache(maxsize=None)
def _inputs(geo, nref):
    """(cell slowness [NMODEL][ncz][ncy][ncx] fp32, sources, event nodes); i.i.d.
    integer velocities per cell, so every cell boundary moves bits."""
    nx, ny, nz = geo
    ncx, ncy, ncz = [-(-a // r) for a, r in zip(geo, nref)]
    rng = np.random.default_rng([41, nx, ny, nz, *nref])
    v = rng.integers(2500, 6501, (NMODEL, ncz, ncy, ncx)).astype(np.int32)
    scell = (1.0 / v.astype(np.float32)).astype(np.float32)
    ev = rng.integers(0, nx * ny * nz, 7).astype(np.int32)
    return scell, _sources(nz), ev


def _expand(scell_m, geo, nref, xshift=0):
    """Node field of one model: scell[k // nrz, j // nry, (i + xshift) // nrx] (clipped)."""
    nx, ny, nz = geo
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ci = np.minimum((i + xshift) // nref[0], scell_m.shape[2] - 1)
    return scell_m[k // nref[2], j // nref[1], ci].ravel()


@functools.lru_cache(maxsize=None)
def _twin(geo, nref, precision, max_sweeps=-1):
    """[(u, ierr, niter)] of solve m * 3 + s on the expanded fields (computed
    once per geometry and precision; callers do not modify it)."""
    scell, src, _ = _inputs(geo, nref)
    dt = np.float32 if precision == 32 else np.float64
    out = []
    for m in range(NMODEL):
        sfield = _expand(scell[m], geo, nref).astype(dt)
        for s in range(len(src)):
            out.append(O.eikonal_solve(*geo, sfield, H, src[s], dtype=dt, max_sweeps=max_sweeps))
    return out


@functools.lru_cache(maxsize=None)
def _not_vacuous(geo, nref, precision):
    """The twin on the cell map shifted by one node along x differs from the
    right twin in every model (a kernel with that off-by-one would fail); a
    single cell has no map to shift: there the two models differ."""
    scell, src, _ = _inputs(geo, nref)
    ut = np.uint32 if precision == 32 else np.uint64
    dt = np.float32 if precision == 32 else np.float64
    right = _twin(geo, nref, precision)
    if scell[0].size == 1:
        return bool((right[0][0].view(ut) != right[len(src)][0].view(ut)).any())
    for m in range(NMODEL):
        shifted, _, _ = O.eikonal_solve(*geo, _expand(scell[m], geo, nref, 1).astype(dt), H, src[0], dtype=dt)
        if not (shifted.view(ut) != right[m * len(src)][0].view(ut)).any():
            return False
    return True


def _solver(geo, nref, precision, fast):
    from mceik_amd.eikonal import BatchSolver
    return BatchSolver(*geo, H, 0.0, 0.0, 0.0, 50, 1e-8, precision, nref=nref, fast_sqrt=fast)


def _solve_and_check(case, max_waves=0, max_sweeps=-1):
    from mceik_amd import _lib
    _, geo, nref, precision, fast, step_z, want = case
    dev = _dev()
    scell, src, ev = _inputs(geo, nref)
    bs = _solver(geo, nref, precision, fast)
    kname = _lib.lib().mceik_fsm_kernel_name(
        C.byref(bs.describe(NMODEL, len(src), 1, 1, nev=len(ev), step_z=step_z))).decode()
    assert kname == want, kname
    out = bs.solve(torch.tensor(src), torch.tensor(scell.reshape(NMODEL, -1), device=dev), ev_node=torch.tensor(ev),
                   want_fields=True, max_waves=max_waves, max_sweeps=max_sweeps, step_z=step_z)
    assert out["step_z"] == (16 if want.startswith("fsm16") else 8)
    ut = np.uint32 if precision == 32 else np.uint64
    u = out["u"].cpu().numpy().reshape(NMODEL * len(src), -1)
    tt = out["ttab"].cpu().numpy()
    niter, ierr = out["niter"].cpu().numpy(), out["ierr"].cpu().numpy()
    for q, (t, t_ierr, t_it) in enumerate(_twin(geo, nref, precision, max_sweeps)):
        bad = np.flatnonzero(u[q].view(ut) != t.view(ut))
        assert bad.size == 0, (f"solve {q} (model {q // len(src)}, source {q % len(src)}), sweeps {max_sweeps}: "
                               f"{bad.size} nodes differ, first {bad[0]} gpu {u[q][bad[0]]!r} twin {t[bad[0]]!r}")
        with np.errstate(over="ignore"):            # a node no sweep has reached yet holds u_nan: inf as fp32
            want = t[ev].astype(np.float32)
        assert np.array_equal(tt[q].view(np.uint32), want.view(np.uint32)), q
        if max_sweeps < 0:
            assert (int(niter[q]), int(ierr[q])) == (t_it, t_ierr), q


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_refinement_bitwise_vs_twin(case):
    """2 models x 3 sources in one launch, fields, tables at 7 event nodes,
    iterations and ierr == the twin; the instance is the table's."""
    _, geo, nref, precision, _, _, _ = case
    _solve_and_check(case)
    assert _not_vacuous(geo, nref, precision)


# straddling 2 x 2 x 8 cells, the generic cache at 11 / 12 z cells, the uncached default
REUSE = [c for c in R.CASES if c[0].split("-")[0] in ("n664", "n3", "n1") and c[4]]


@pytest.mark.parametrize("case", REUSE, ids=[c[0] for c in REUSE])
def test_refinement_one_wave_takes_every_solve(case):
    """max_waves = 1: one wave runs the six solves in turn, so a cell cache or
    a column word left from the previous solve or model would show."""
    _solve_and_check(case, max_waves=1)


@pytest.mark.parametrize("max_sweeps", [1, 3, 9])
@pytest.mark.parametrize("case", REUSE, ids=[c[0] for c in REUSE])
def test_refinement_partial_sweeps(case, max_sweeps):
    """The field after 1, 3 and 9 sweeps == the twin's after as many (the
    held stream mid-solve at cells that are not tile-aligned)."""
    _solve_and_check(case, max_sweeps=max_sweeps)


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("nref", [(1, 1, 1), (4, 4, 4)], ids=["n1", "n4"])
def test_long_axis_is_refused(nref, precision, capfd):
    """4104 x 9 x 10: an axis past 4096 nodes, where (uint32)node * ceil(2^20 / nr)
    would wrap at nr = 1.  The host bounds every axis at 4096 (the product
    then stays below 2^32), so the launch is refused, not wrong."""
    from mceik_amd import _lib
    dev = _dev()
    geo = (4104, 9, 10)
    bs = _solver(geo, nref, precision, True)
    assert _lib.lib().mceik_fsm_check(C.byref(bs.describe(1, 1, 1, 1))) == 1
    ncell = int(np.prod([-(-a // r) for a, r in zip(geo, nref)]))
    with pytest.raises(RuntimeError, match=r"mceik_fsm_batch_solve failed \(1\)"):
        bs.solve(torch.tensor([[[0.0, 1234.5, 430.0, 900.0]]]), torch.full((1, ncell), 2.5e-4, device=dev),
                 want_fields=True)
    assert "invalid batch description" in capfd.readouterr().err


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("nref", [(1, 1, 1), (4, 4, 4)], ids=["n1", "n4"])
def test_longest_axis_bitwise(nref, precision):
    """4096 x 8 x 10, the longest axis the host accepts: the cell cache is
    off (fill_launch keeps it below 4096), so both refinements run the
    uncached multiply, whose largest product 4095 * 2^20 (nr = 1) is the
    closest a launch comes to 2^32.  One source near the far end of x and
    one iteration (8 sweeps, every direction over every node): the wave
    streams the 512 tiles one after the other, so a converged solve takes
    5 iterations and 4 to 6 s, and checks the indexing no further."""
    from mceik_amd import _lib
    dev = _dev()
    geo = (4096, 8, 10)
    ncx, ncy, ncz = [-(-a // r) for a, r in zip(geo, nref)]
    rng = np.random.default_rng([43, *nref])
    scell = (1.0 / rng.integers(2500, 6501, (ncz, ncy, ncx)).astype(np.float32)).astype(np.float32)
    src = np.array([[0.0, 401321.0, 430.0, 900.0]])
    ev = rng.integers(0, int(np.prod(geo)), 7).astype(np.int32)
    bs = _solver(geo, nref, precision, True)
    kname = _lib.lib().mceik_fsm_kernel_name(C.byref(bs.describe(1, 1, 1, 1, nev=7))).decode()
    assert kname == (R.UNCACHED32 if precision == 32 else R.UNCACHED64)
    out = bs.solve(torch.tensor(src[None]), torch.tensor(scell.reshape(1, -1), device=dev), ev_node=torch.tensor(ev),
                   want_fields=True, max_sweeps=8)
    dt, ut = (np.float32, np.uint32) if precision == 32 else (np.float64, np.uint64)
    t, _, _ = O.eikonal_solve(*geo, _expand(scell, geo, nref).astype(dt), H, src, dtype=dt, max_sweeps=8)
    u = out["u"].cpu().numpy().ravel()
    bad = np.flatnonzero(u.view(ut) != t.view(ut))
    assert bad.size == 0, f"{bad.size} nodes differ, first {bad[0]} gpu {u[bad[0]]!r} twin {t[bad[0]]!r}"
    assert np.array_equal(out["ttab"].cpu().numpy()[0].view(np.uint32), t[ev].astype(np.float32).view(np.uint32))
    shifted, _, _ = O.eikonal_solve(*geo, _expand(scell, geo, nref, 1).astype(dt), H, src, dtype=dt, max_sweeps=8)
    assert (shifted.view(ut) != t.view(ut)).any()


# ---- the sampler ----------------------------------------------------------
# id: (nref, n, phases, precision, kernel, seed); seeds chosen on the CPU from the
# oracle alone (_oracle_run) so that the 4 steps of the 4 chains hold an accept
# and a rejection inside the box
OFF, NCH, NSTEPS = 3, 4, 4
SAMPLER = {
    "n664-P": ((6, 6, 4), 32, "P", 32, R.FSM16_FT, 1),
    "n664-PS": ((6, 6, 4), 32, "PS", 32, R.FSM16_FT, 1),
    "n664-P-f64": ((6, 6, 4), 32, "P", 64, R.Z4_KB64, 1),
    "n3-PS": ((3, 3, 3), 32, "PS", 32, R.GEN32, 1),
    "n1-P": ((1, 1, 1), 24, "P", 32, R.UNCACHED32, 2),
    "n1-P-f64": ((1, 1, 1), 24, "P", 64, R.UNCACHED64, 2),
}


def _sampler_problem(cfg):
    from mceik_amd import mcmc
    nref, n, phases, _, _, seed = cfg
    p = mcmc.make_problem("C2", n=n, nstat=4, nev=6, nref=nref, picks="analytic", phases=phases, seed=seed)
    p.dvmax = 300
    p.var[:] = 1e-5
    return p


def _oracle_run(p, precision):
    """(P, v0, logl0, init tables, v, logl, accept [NSTEPS][NCH], in-box [NSTEPS][NCH]) from the CPU alone."""
    from mceik_amd import mcmc
    P = O.make_problem(p, precision=precision)
    v0 = mcmc.initial_models(p, range(OFF, OFF + NCH))
    tt0 = np.stack([O.forward_all_f32(P, v0[c].ravel()) for c in range(NCH)])       # [NCH][nphase][nstat][nev]
    logl0 = np.array([O.loglik(P, tt0[c]) for c in range(NCH)])
    v, logl = v0.copy(), logl0.copy()
    acc, inbox = np.zeros((NSTEPS, NCH), np.uint8), np.zeros((NSTEPS, NCH), bool)
    for i in range(NSTEPS):
        for c in range(NCH):
            inbox[i, c] = O.propose(P, OFF + c, i, v[c].ravel())[2]
        v, logl, a, _ = O.mcmc_run(P, v, logl, OFF, i, 1)
        acc[i] = a[0]
    return P, v0, logl0, tt0, v, logl, acc, inbox


@functools.lru_cache(maxsize=None)
def _sampler_reference(case):
    cfg = SAMPLER[case]
    p = _sampler_problem(cfg)
    return (p,) + _oracle_run(p, cfg[3])


def _sampler_check(case, monkeypatch, persist=None):
    from mceik_amd import mcmc
    _dev()
    nref, n, phases, precision, kernel, _ = SAMPLER[case]
    p, P, v0, logl0, tt0, vo, lo, acco, inbox = _sampler_reference(case)
    assert acco.any(), "no accept"
    assert (inbox & (acco == 0)).any(), "no rejection inside the box"
    if persist is not None:
        monkeypatch.setenv("MCEIK_PERSIST", "1" if persist else "0")
    s = mcmc.Sampler(p, nchains=NCH, chain_offset=OFF, precision=precision)
    info = s.info()
    assert info["kernel"] == kernel, info["kernel"]
    if persist is not None:
        assert info["multi_step"] == bool(persist) and info["step_z"] == 16
    else:
        assert not info["multi_step"] or info["step_z"] == 16
    gv0, gl0, _, _ = s.state()
    ttab, _, _, ierr = s.last(with_ierr=True)
    assert not ierr.any()
    assert np.array_equal(gv0, v0)
    assert np.array_equal(ttab.reshape(tt0.shape).view(np.uint32), tt0.view(np.uint32))
    assert np.array_equal(gl0.view(np.uint64), logl0.view(np.uint64))
    flags = []
    if info["multi_step"]:
        s.run(NSTEPS)               # one launch runs the four steps
    else:
        for _ in range(NSTEPS):
            s.run(1)
            flags.append(s.last()[2].copy())
    v, logl, nacc, step = s.state()
    last = s.last()[2]
    s.close()
    assert step == NSTEPS
    assert np.array_equal(v, vo)
    assert np.array_equal(logl.view(np.uint64), lo.view(np.uint64))
    assert np.array_equal(nacc, acco.sum(0))
    assert np.array_equal(last, acco[-1])
    if flags:
        assert np.array_equal(np.array(flags), acco)


@pytest.mark.parametrize("persist", [False, True], ids=["per_step", "multi_step"])
@pytest.mark.parametrize("case", ["n664-P", "n664-PS"])
def test_sampler_straddling_cells(case, persist, monkeypatch):
    """(6, 6, 4) at n = 32: 2 x 2 x 8 cells per z-block as at refinement 4, but
    cells straddle tile edges and the last cell of an axis is 2 nodes wide
    (x, y); the first-touch 16-z instance, per-step and multi-step launches."""
    _sampler_check(case, monkeypatch, persist)


@pytest.mark.parametrize("case", ["n664-P-f64", "n3-PS", "n1-P", "n1-P-f64"])
def test_sampler_other_refinements(case, monkeypatch):
    """The compact fp64 instance at (6, 6, 4); 11^3 cells in the 8-z generic
    cache; the library default nref = 1 (13824 cells per model, uncached)."""
    _sampler_check(case, monkeypatch)
