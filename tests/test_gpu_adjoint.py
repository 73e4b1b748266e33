"""The discrete adjoint on the GPU (mceik_fsm_adjoint, BatchSolver.adjoint,
mcmc.logl_grad) against tests/_adjoint.py, bit for bit, on the
fields the GPU forward returned: grad, grad_solve, lam, niter and status."""
import numpy as np
import pytest

import _adjoint as A
import _oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
H = 100.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Batch:
    """One batch: models x stations, events, weights; the GPU forward's fields."""

    def __init__(self, dev, n, nref, prec, nmodel=1, nstat=2, nev=16, trilinear=True, per_model=False, seed=1,
                 zero_row=None):
        from mceik_amd.eikonal import BatchSolver
        nx, ny, nz = n
        self.n, self.nref, self.prec, self.nmodel, self.nstat, self.nev = n, nref, prec, nmodel, nstat, nev
        rng = np.random.default_rng(seed)
        nr = nref or (1, 1, 1)
        ncell = (-(-nx // nr[0])) * (-(-ny // nr[1])) * (-(-nz // nr[2]))
        v = 3000.0 + 2500.0 * rng.random((nmodel, ncell))
        self.dtype = np.float64 if prec == 64 else np.float32
        self.slow = (1.0 / v).astype(np.float32 if nref else self.dtype)
        # stations: off-node in x, y; the first on the top face (a clipped box), the others off-node near z = 0
        self.src = np.stack([np.zeros(nstat), rng.uniform(2 * H, (nx - 3) * H, nstat),
                             rng.uniform(2 * H, (ny - 3) * H, nstat),
                             np.where(np.arange(nstat) == 0, (nz - 1) * H, 0.3 * H)], 1)
        rows = nmodel if per_model else 1
        ix, iy, iz = (rng.integers(0, m - 1, (rows, nev)) for m in n)
        node = ((iz * ny + iy) * nx + ix).astype(np.int32)
        node[:, 1] = node[:, 0]                                  # two events on one node
        self.node = node if per_model else node[0]
        self.frac = rng.random(node.shape + (3,)).astype(np.float32) if trilinear else None
        if self.frac is not None and not per_model:
            self.frac = self.frac[0]
        self.w = rng.normal(0.0, 1.0, (nmodel * nstat, nev))
        if zero_row is not None:
            self.w[zero_row] = 0.0
        self.bs = BatchSolver(nx, ny, nz, H, 0.0, 0.0, 0.0, 50, 1e-8, prec, nref=nref, fast_sqrt=nref is not None)
        self.t_src = torch.tensor(self.src[:, None, :])
        shape = (nmodel, -1) if nref else (nmodel, nz, ny, nx)
        self.t_slow = torch.tensor(self.slow.reshape(shape), device=dev)
        self.t_node = torch.tensor(self.node)
        self.t_frac = None if self.frac is None else torch.tensor(self.frac)
        fwd = self.bs.solve(self.t_src, self.t_slow, ev_node=self.t_node, ev_frac=self.t_frac, want_fields=True)
        torch.cuda.synchronize()
        assert int(fwd["ierr"].abs().max()) == 0
        self.t_u = fwd["u"]
        self.u = fwd["u"].cpu().numpy().reshape(nmodel * nstat, -1)
        self._ref = {}

    def adjoint(self, **kw):
        kw.setdefault("want_lambda", True)
        kw.setdefault("want_per_solve", True)
        out = self.bs.adjoint(self.t_src, self.t_slow, self.t_u, self.t_node, torch.tensor(self.w), ev_frac=self.t_frac,
                              **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}

    def ref(self, solve, cap=50):
        """The restatement of one solve on the GPU's field (computed once per cap)."""
        if (solve, cap) not in self._ref:
            nx, ny, nz = self.n
            m, s = divmod(solve, self.nstat)
            nodes = A.expand_cells(self.slow[m], nx, ny, nz, self.nref) if self.nref else self.slow[m]
            f = A.forward_f(nodes, H, self.prec)
            node = self.node[m] if self.node.ndim == 2 else self.node
            frac = None if self.frac is None else (self.frac[m] if self.node.ndim == 2 else self.frac)
            q = A.adjoint_source(nx, ny, nz, node, self.w[solve], frac)
            self._ref[solve, cap] = A.restate(self.u[solve], nx, ny, nz, H, self.src[s], f, q, nref=self.nref,
                                              sweeps=True, cap=cap)
        return self._ref[solve, cap]

    def check(self, out, skip=None, cap=50, per_solve=True):
        nsolve = self.nmodel * self.nstat
        rows = []
        for k in range(nsolve):
            if skip is not None and skip[0][k % self.nstat]:
                r = {"lam_sweep": np.zeros(self.u.shape[1]), "grad": np.zeros(out["grad"].shape[1]), "niter": 0,
                     "status": 0}
            else:
                r = self.ref(k, cap)
            rows.append(r["grad"])
            assert out["niter"][k] == r["niter"] and out["status"][k] == r["status"], (k, out["niter"][k], r["niter"])
            if "lam" in out:
                assert np.array_equal(_bits(out["lam"][k].ravel()), _bits(r["lam_sweep"])), k
            if per_solve:
                assert np.array_equal(_bits(out["grad_solve"][k]), _bits(r["grad"])), k
        for m in range(self.nmodel):
            want = A.station_sum(rows[m * self.nstat:(m + 1) * self.nstat])
            assert np.array_equal(_bits(out["grad"][m]), _bits(want)), m
        return rows


CASES = {
    "17x13x11_f32": dict(n=(17, 13, 11), nref=(4, 4, 4), prec=32),
    "33x29x25_r352_f32": dict(n=(33, 29, 25), nref=(3, 5, 2), prec=32, trilinear=False),
    "33x29x25_r352_f64": dict(n=(33, 29, 25), nref=(3, 5, 2), prec=64),
    "40x40x24_f32": dict(n=(40, 40, 24), nref=(4, 4, 4), prec=32),
    "field_13x9x11": dict(n=(13, 9, 11), nref=None, prec=32, trilinear=False),
    "field_13x9x11_f64": dict(n=(13, 9, 11), nref=None, prec=64),
}


@pytest.mark.parametrize("name", list(CASES))
def test_adjoint_bitwise_against_the_restatement(name):
    b = Batch(_dev(), **CASES[name])
    out = b.adjoint()
    assert not out["status"].any() and (out["niter"] >= 2).all()
    rows = b.check(out)
    assert all(np.abs(r).max() > 0 for r in rows)


@pytest.fixture(scope="module")
def six():
    """2 models x 3 stations, a list of events per model, a zero row of weights."""
    return Batch(_dev(), (17, 13, 11), (4, 4, 4), 32, nmodel=2, nstat=3, nev=8, per_model=True, seed=7, zero_row=4)


def test_per_model_events_zero_row_and_model_sums(six):
    out = six.adjoint()
    assert not out["status"].any()
    six.check(out)
    assert out["niter"][4] == 1 and not out["grad_solve"][4].any() and not out["lam"][4].any()
    assert not np.signbit(out["grad_solve"][4]).any()
    # grad alone: a workgroup takes a whole model, stations in order -- the same bits
    alone = six.adjoint(want_per_solve=False, want_lambda=False)
    assert np.array_equal(_bits(alone["grad"]), _bits(out["grad"]))
    assert np.array_equal(alone["niter"], out["niter"])


def test_skip_row(six):
    skip = np.array([[0, 1, 0]], np.uint8)
    out = six.adjoint(skip=torch.tensor(skip))
    six.check(out, skip=skip)
    for k in (1, 4):
        assert out["niter"][k] == 0 and not out["grad_solve"][k].any() and not out["lam"][k].any()
    alone = six.adjoint(skip=torch.tensor(skip), want_per_solve=False, want_lambda=False)
    assert np.array_equal(_bits(alone["grad"]), _bits(out["grad"]))


def test_schedule_independence_and_workspace_reuse(six):
    """max_groups 2 runs the 6 solves three to a workgroup in a reused slice;
    1 runs them all in one; 0 gives every solve a workgroup: identical bits."""
    outs = [six.adjoint(max_groups=g) for g in (0, 1, 2)]
    six.check(outs[2])
    for o in outs[1:]:
        for k in ("grad", "grad_solve", "lam", "niter", "status"):
            assert np.array_equal(o[k].view(np.uint8), outs[0][k].view(np.uint8)), k


def test_cap_of_one_sets_status_and_leaves_the_others(six):
    out = six.adjoint(maxit=1)
    assert list(out["status"]) == [1, 1, 1, 1, 0, 1] and list(out["niter"]) == [1] * 6
    six.check(out, cap=1)                       # the state after one iteration of eight sweeps
    full = six.adjoint()
    assert np.array_equal(_bits(out["grad_solve"][4]), _bits(full["grad_solve"][4]))


def test_refusals_raise():
    dev = _dev()
    b = Batch(dev, (13, 9, 11), None, 32, nstat=1, nev=2, trilinear=False)
    with pytest.raises(TypeError):
        b.bs.adjoint(b.t_src, b.t_slow, b.t_u.double(), b.t_node, torch.tensor(b.w))
    two = torch.tensor(np.repeat(b.src[:, None, :], 2, axis=1))
    with pytest.raises(ValueError):
        b.bs.adjoint(two, b.t_slow, b.t_u, b.t_node, torch.tensor(b.w))


# ---- logl_grad end to end ---------------------------------------------------

def _manual(smp, p, wrt):
    """logl_grad's composition spelled out with the public pieces."""
    from mceik_amd import mcmc
    from mceik_amd.eikonal import BatchSolver
    dev = torch.device("cuda", 0)
    nch, nph = smp.nchains, p.nphase
    v = smp.state()[0].reshape(nch, nph, p.ncell)
    inp = mcmc.logl_inputs(smp)
    bs = BatchSolver(p.nx, p.ny, p.nz, p.h, p.x0, p.y0, p.z0, p.maxit, p.tol, 32, nref=p.nref, fast_sqrt=True)
    src = torch.tensor(np.stack([np.zeros(p.nstat), p.sx, p.sy, p.sz], 1)[:, None, :])
    slow = torch.tensor((np.float32(1.0) / v.astype(np.float32)).reshape(nch * nph, -1), device=dev)
    if inp["hyp"] is None:
        node = torch.tensor(p.ev_node)
    else:
        h = inp["hyp"].astype(np.int64)
        node = torch.tensor(np.repeat(((h[..., 2] * p.ny + h[..., 1]) * p.nx + h[..., 0]).astype(np.int32), nph, 0))
    fwd = bs.solve(src, slow, ev_node=node, want_fields=True)
    tt = fwd["ttab"].cpu().numpy().reshape(nch, nph, p.nstat, p.nevents)
    w = np.zeros((nch, nph, p.nstat, p.nevents))
    for c in range(nch):
        dte = mcmc.logl_pick_grad(p, tt[c], inp["var"][c], inp["tcorr"][c])
        for e in range(p.nevents):
            for j in range(p.obs_ptr[e], p.obs_ptr[e + 1]):
                if not p.obs_mask[j]:
                    w[c, p.obs_phase[j], p.obs_stat[j], e] += dte[j]
    adj = bs.adjoint(src, slow, fwd["u"], node, torch.tensor(w.reshape(-1, p.nevents)), skip=torch.tensor(p.skip))
    g = adj["grad"].cpu().numpy().reshape(nch, -1)
    if wrt == "velocity":
        vv = v.reshape(nch, -1).astype(np.float64)
        g = -(g / (vv * vv))
    return g, tt


def test_logl_grad_end_to_end():
    _dev()
    from mceik_amd import mcmc
    p = A.ps_problem()
    smp = mcmc.Sampler(p, nchains=4)
    try:
        v, logl, _, _ = smp.state()
        g, ll = mcmc.logl_grad(smp, wrt="velocity")
        assert g.shape == (4, 2 * p.ncell) and np.isfinite(g).all()
        assert np.array_equal(_bits(ll), _bits(logl))                          # the sampler's own logL
        gm, tt = _manual(smp, p, "velocity")
        assert np.array_equal(_bits(g), _bits(gm))
        assert np.array_equal(tt.view(np.uint32), smp.last()[0].view(np.uint32))  # the sampler's tables
        gs, _ = mcmc.logl_grad(smp, chains=[2, 0], wrt="slowness", chunk=1)
        vv = v.reshape(4, -1).astype(np.float64)[[2, 0]]
        assert np.array_equal(_bits(-(gs / (vv * vv))), _bits(g[[2, 0]]))
        # the CPU composition on chain 0 (fp32 twin's fields): the same bits
        gc, lc = A.cpu_logl_grad(p, v[0])
        assert np.array_equal(_bits(gc), _bits(g[0])) and lc == logl[0]
        # a +-16 m/s move of a 2 x 2 x 2 block against the sampler's own logL
        cells = A.block_cells(p)
        v2 = np.stack([v[0], v[0]])
        v2[0, 0, cells] += 16
        v2[1, 0, cells] -= 16
        s2 = mcmc.Sampler(p, nchains=2, v0=v2)
        l2 = s2.state()[1]
        s2.close()
        fd, want = (l2[0] - l2[1]) / 32.0, float(g[0, cells].sum())
        dev = abs(fd - want) / abs(want)
        print(f"block move on the GPU: FD {fd:.6e}, gradient {want:.6e}, discrepancy {dev:.3e}")
        assert dev <= 4 * A.OBS_BLOCK_DIR
        # moved hypocentres, noise scale and statics
        smp.hypo_enable(3, dmax=(1, 1, 1))
        smp.nuis_enable(4, offset=1, nsub=4, ladder=mcmc.nuis_ladder(11, 0.25, 4.0), statics_dt=1e-3, kcmax=20)
        smp.run(12)
        logl = smp.state()[1]
        g, ll = mcmc.logl_grad(smp)
        assert np.array_equal(_bits(ll), _bits(logl))
        gm, _ = _manual(smp, p, "slowness")
        assert np.array_equal(_bits(g), _bits(gm))
        kn, kc = smp.nuis_get()
        assert (smp.hypo_positions() != smp.hypo_positions()[0]).any() or kc.any() or (kn != 5).any()
    finally:
        smp.close()
