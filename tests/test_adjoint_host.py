"""The discrete adjoint's checker checked (no GPU): tests/_adjoint.py, the
numpy restatement of DESIGN.md s.17 the GPU results are compared against bit
for bit, against central finite differences of the fp64 oracle solve; the
pick-gradient of the objective; and what mceik_fsm_adjoint_check refuses.

Every bound is 4 x the maximum observed on this suite's own cases (the rule of
DESIGN.md s.8c); the observed figures are the OBS_* constants below and in
DESIGN.md s.17.  Each test prints what it measured."""
import ctypes as C

import numpy as np
import pytest

import _adjoint as A
import _oracle as O

H = 100.0
# observed maxima (this file's cases, x86-64 fp64)
OBS_FD_CELL = 3.0e-7        # |g - g_fd| / max|g|, cells checked (2.5e-8, 3.0e-7, 7.5e-8 per grid; box cases below)
OBS_FD_DIR = 1.2e-8         # directional derivative, relative (1.7e-9, 1.2e-8, 7.7e-9)
OBS_HOMOG = 1.7e-13         # |sum s g / J - 1| (6.9e-15, 1.4e-13, 1.7e-13)
OBS_F32_F64 = 1.04e-6       # restatement on the fp32 twin's field against the fp64 field's, / max|g|
OBS_PICK_FD = 1.4e-9        # logl_pick_grad against central differences (eps 1e-7 s), / max|g|


def _model(kind, nx, ny, nz, nref, seed):
    ncx, ncy, ncz = -(-nx // nref[0]), -(-ny // nref[1]), -(-nz // nref[2])
    rng = np.random.default_rng(seed)
    if kind == "random":
        v = 3000.0 + 2500.0 * rng.random(ncx * ncy * ncz)
    else:                                            # depth gradient with a little structure
        k = np.repeat(np.arange(ncz), ncx * ncy)
        v = 2500.0 + 3500.0 * (k + 0.5) / ncz + 100.0 * rng.random(ncx * ncy * ncz)
    return (1.0 / v).astype(np.float32)


def _events(nx, ny, nz, nev, seed):
    """Trilinear events with signed weights."""
    rng = np.random.default_rng(seed)
    ix, iy, iz = rng.integers(0, nx - 1, nev), rng.integers(0, ny - 1, nev), rng.integers(1, nz - 1, nev)
    node = ((iz * ny + iy) * nx + ix).astype(np.int32)
    frac = rng.random((nev, 3)).astype(np.float32)
    w = rng.normal(0.0, 1.0, nev)
    return node, frac, w


class Case:
    def __init__(self, nx, ny, nz, nref, kind, src, seed=3, nev=16, events=None):
        self.nx, self.ny, self.nz, self.nref, self.src = nx, ny, nz, nref, np.asarray(src, np.float64)
        self.cells = _model(kind, nx, ny, nz, nref, seed)
        self.node, self.frac, self.w = events if events is not None else _events(nx, ny, nz, nev, seed + 1)

    def solve(self, cells, dtype=np.float64):
        s = A.expand_cells(np.asarray(cells, dtype), self.nx, self.ny, self.nz, self.nref).ravel()
        u, ierr, _ = O.eikonal_solve(self.nx, self.ny, self.nz, s, H, self.src, maxit=200, tol=1e-13, dtype=dtype)
        assert ierr == 0
        return u

    def J(self, cells):
        u = self.solve(cells)
        t = 0.0
        for e in range(len(self.w)):
            t += self.w[e] * A.event_time64(u, self.nx, self.ny, self.nz, self.node[e],
                                            None if self.frac is None else self.frac[e])
        return t

    def restate(self, dtype=np.float64, sweeps=False, field=None):
        prec = 64 if dtype == np.float64 else 32
        cells = self.cells.astype(np.float64) if prec == 64 else self.cells
        u = self.solve(cells, dtype) if field is None else field
        f = A.forward_f(A.expand_cells(cells, self.nx, self.ny, self.nz, self.nref), H, prec)
        q = A.adjoint_source(self.nx, self.ny, self.nz, self.node, self.w, self.frac)
        return A.restate(u, self.nx, self.ny, self.nz, H, self.src, f, q, nref=self.nref, sweeps=sweeps)

    def fd_cell(self, c):
        s = self.cells.astype(np.float64)
        eps = 1e-6 * s[c]
        sp, sm = s.copy(), s.copy()
        sp[c] += eps; sm[c] -= eps
        return (self.J(sp) - self.J(sm)) / (2.0 * eps)

    def fd_dir(self, d):
        s = self.cells.astype(np.float64)
        return (self.J(s + 1e-6 * s * d) - self.J(s - 1e-6 * s * d)) / 2e-6       # = sum_c g_c s_c d_c


OFF_NODE = (0.0, 5.3 * H, 4.6 * H, 0.3 * H)             # off-node, near z = 0
CASES = {"17x13x11": (17, 13, 11, (4, 4, 4), "random"),
         "33x29x25_r352": (33, 29, 25, (3, 5, 2), "random"),
         "33x29x25_grad": (33, 29, 25, (4, 4, 4), "gradient")}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    c = Case(*CASES[request.param], OFF_NODE)
    c.name = request.param
    c.r = c.restate(sweeps=True)
    return c


def test_restatement_against_finite_differences(case):
    g = case.r["grad"]
    gmax = np.abs(g).max()
    rng = np.random.default_rng(11)
    cells = list(np.argsort(-np.abs(g))[:6]) + list(rng.choice(g.size, 4, replace=False))
    err = max(abs(case.fd_cell(c) - g[c]) for c in cells) / gmax
    d = rng.normal(0.0, 1.0, g.size)
    want = float(np.dot(g * case.cells.astype(np.float64), d))
    derr = abs(case.fd_dir(d) - want) / abs(want)
    print(f"{case.name}: cell FD error {err:.3e} of max|g|, directional {derr:.3e}")
    assert err <= 4 * OBS_FD_CELL
    assert derr <= 4 * OBS_FD_DIR


def test_sweep_form_reaches_the_same_bits(case):
    """The eight sweep orderings stop at the fixed point the decreasing-u pass
    computes, bit for bit, within a handful of iterations."""
    r = case.r
    assert r["status"] == 0 and 2 <= r["niter"] <= 8, r["niter"]
    assert np.array_equal(r["lam"].view(np.int64), r["lam_sweep"].view(np.int64))
    print(f"{case.name}: {r['niter']} iterations")


def test_homogeneity(case):
    """ts = 0: u is homogeneous of degree one in the slowness, so sum s g = J."""
    s = case.cells.astype(np.float64)
    J = case.J(s)
    dev = abs(float(np.dot(s, case.r["grad"])) / J - 1.0)
    print(f"{case.name}: homogeneity {dev:.3e}")
    assert dev <= 4 * OBS_HOMOG


def _fd_all_big(c, r, nbig=6):
    g = r["grad"]
    cells = np.argsort(-np.abs(g))[:nbig]
    return max(abs(c.fd_cell(k) - g[k]) for k in cells) / np.abs(g).max()


def test_event_on_a_boundary_node():
    """An event on a node of the source's box: lam * d is its only contribution."""
    nx, ny, nz = 17, 13, 11
    box = [A.bc_axis(n, 0.0, H, s) for n, s in zip((nx, ny, nz), OFF_NODE[1:])]
    node = np.array([(box[2][1] * ny + box[1][0]) * nx + box[0][1]], np.int32)
    c = Case(nx, ny, nz, (4, 4, 4), "random", OFF_NODE, events=(node, None, np.array([1.5])))
    r = c.restate()
    assert np.count_nonzero(r["g"]) == 1 and np.count_nonzero(r["grad"]) == 1
    err = _fd_all_big(c, r, 3)
    print(f"boundary-node event: FD error {err:.3e}")
    assert err <= 4 * OBS_FD_CELL


def test_box_clipped_by_the_grid_edge():
    """A source on the top face (the sampler's stations): the box is clipped."""
    nx, ny, nz = 17, 13, 11
    src = (0.0, 7.4 * H, 5.5 * H, (nz - 1) * H)
    assert A.bc_axis(nz, 0.0, H, src[3]) == (nz - 2, nz - 1, True)
    c = Case(nx, ny, nz, (4, 4, 4), "random", src)
    r = c.restate()
    err = _fd_all_big(c, r)
    print(f"clipped box: FD error {err:.3e}")
    assert err <= 4 * OBS_FD_CELL


def test_restatement_on_fp32_and_fp64_fields():
    c = Case(40, 40, 24, (4, 4, 4), "gradient", (0.0, 11.3 * H, 20.6 * H, 23 * H))
    g64, g32 = c.restate(np.float64)["grad"], c.restate(np.float32)["grad"]
    dev = np.abs(g32 - g64).max() / np.abs(g64).max()
    print(f"fp32 field against fp64 field: {dev:.3e} of max|g|")
    assert dev <= 4 * OBS_F32_F64


def _ps_problem():
    from mceik_amd import mcmc
    p = mcmc.make_problem("C2", n=16, nstat=4, nev=5, phases="PS")
    rng = np.random.default_rng(5)
    p.var = 0.05 + 0.4 * rng.random(p.var.size)
    p.luse[7] = 0
    p.pcorr = rng.normal(0.0, 0.01, p.nstat)
    return p, rng


def test_logl_pick_grad_against_finite_differences():
    from mceik_amd import mcmc
    p, rng = _ps_problem()
    tt = (0.3 + rng.random((2, p.nstat, p.nevents))).astype(np.float32)
    g = mcmc.logl_pick_grad(p, tt)
    assert g[7] == 0.0 and np.count_nonzero(g) == g.size - 1

    def logl64(t):                       # the objective on fp64 tables (logl_picks rounds its tables to fp32)
        q = 0.0
        for e in range(p.nevents):
            js = [j for j in range(p.obs_ptr[e], p.obs_ptr[e + 1]) if not p.obs_mask[j]]
            w = np.array([1.0 / p.var[j] for j in js])
            te = np.array([t[p.obs_phase[j], p.obs_stat[j], e] for j in js])
            tc = np.array([p.tobs[j] - p.tcorr[j] for j in js])
            t0 = float(np.dot(w / w.sum(), tc - te))
            q -= float((((w * 0.7071067811865475) * (tc - (te + t0))) ** 2).sum())
        return q
    t64 = tt.astype(np.float64)
    assert abs(logl64(t64) - mcmc.logl_picks(p, tt)) <= 1e-12 * abs(logl64(t64))
    err = 0.0
    for j in range(g.size):
        e = int(np.searchsorted(p.obs_ptr, j, side="right") - 1)
        tp, tm = t64.copy(), t64.copy()
        tp[p.obs_phase[j], p.obs_stat[j], e] += 1e-7
        tm[p.obs_phase[j], p.obs_stat[j], e] -= 1e-7
        fd = (logl64(tp) - logl64(tm)) / 2e-7
        err = max(err, abs(fd - g[j]) if not p.obs_mask[j] else 0.0)
    err /= np.abs(g).max()
    print(f"logl_pick_grad: FD error {err:.3e} of max|g|")
    assert err <= 4 * OBS_PICK_FD


def test_logl_gradient_against_the_oracle_loglik():
    """The whole composition on the CPU (fp32 twin's fields, pick gradient,
    restatement): logl_picks is the oracle's loglik bit for bit, and the
    gradient predicts the change of the oracle's logL under a +-16 m/s move of
    a 2 x 2 x 2 block of cells (a coarse check: the move is not small and the
    tables are fp32; tests/test_gpu_adjoint.py uses 4 x this discrepancy)."""
    from mceik_amd import mcmc
    p = A.ps_problem()
    v = mcmc.initial_models(p, [0])[0]
    P = O.make_problem(p)
    g, logl = A.cpu_logl_grad(p, v)
    assert logl == mcmc.logl_picks(p, O.forward_all_f32(P, v.ravel()))
    cells = A.block_cells(p)
    L = []
    for sgn in (+1, -1):
        w = v.copy()
        w[0, cells] += sgn * 16
        L.append(O.loglik(P, O.forward_all_f32(P, w.ravel())))
    fd, want = (L[0] - L[1]) / 32.0, float(g[cells].sum())
    dev = abs(fd - want) / abs(want)
    print(f"block move: FD {fd:.6e}, gradient {want:.6e}, discrepancy {dev:.3e}")
    assert dev <= 4 * A.OBS_BLOCK_DIR


def _desc(nsolve_models=1, nstat=1, nsrc=1, n=(17, 13, 11), max_groups=0):
    from mceik_amd import _lib
    b = _lib.FsmBatch()
    b.nx, b.ny, b.nz = n
    b.h, b.maxit, b.tol, b.precision = H, 50, 1e-8, 32
    b.nmodel, b.nstat, b.nsrc = nsolve_models, nstat, nsrc
    b.slow_mode, b.nrx, b.nry, b.nrz = 1, 4, 4, 4
    b.src = b.slow = 8                    # never dereferenced on the host
    d = _lib.FsmAdjoint()
    d.batch = C.pointer(b)
    d.u = 8
    d.grad_solve = 8
    d.max_groups = max_groups
    d._b = b
    return d


def test_ctypes_mirror_matches_the_header():
    from mceik_amd import _lib
    from test_capi import _offsets_c
    names = [f[0] for f in _lib.FsmAdjoint._fields_]
    c = _offsets_c("mceik.h", "mceik_fsm_adjoint", names)
    assert C.sizeof(_lib.FsmAdjoint) == c["sizeof"]
    for n in names:
        assert getattr(_lib.FsmAdjoint, n).offset == c[n], n


def test_check_refuses_and_workspace_sizing(capfd):
    from mceik_amd import _lib
    L = _lib.lib()
    chk = lambda d: L.mceik_fsm_adjoint_check(C.byref(d)) if d is not None else L.mceik_fsm_adjoint_check(None)
    assert chk(_desc()) == 0
    assert chk(None) == 1
    d = _desc(nsrc=2)
    assert chk(d) == 1 and "nsrc" in capfd.readouterr().err
    d = _desc(); d.u = None
    assert chk(d) == 1 and "u is NULL" in capfd.readouterr().err
    d = _desc(); d.batch = None
    assert chk(d) == 1
    for bad in ((1, 13, 11), (17, 13, 5000)):                # geometry the forward refuses
        assert chk(_desc(n=bad)) == 1
    d = _desc(n=(3850, 8, 8)); d._b.nrx = 275                # a refinement the forward refuses
    assert chk(d) == 1
    d = _desc(); d._b.nev = 3                                # events without a list or weights
    assert chk(d) == 1
    capfd.readouterr()
    ws = lambda **k: L.mceik_fsm_adjoint_workspace_bytes(C.byref(_desc(**k)))
    n = 17 * 13 * 11
    assert ws(nsolve_models=6, max_groups=2) == ws(nsolve_models=600, max_groups=2) == 2 * ((41 * n + 255) // 256 * 256)
    assert ws(nsolve_models=600, max_groups=4) == 2 * ws(nsolve_models=600, max_groups=2)
    assert ws(nsolve_models=600, nstat=3, max_groups=4) == ws(nsolve_models=600, max_groups=4)
    assert ws(nsolve_models=100000) == ws(nsolve_models=1000) == 256 * ws(nsolve_models=1)
