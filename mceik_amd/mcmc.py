"""MCMC travel-time tomography sampler: host side of include/mceik.h.

A `Problem` carries the reference's driver data model (mceik_struct.h:
stations, CSR event catalogue, grid/MCMC/eikonal parameters); `Sampler`
drives one GPU's chains through libmceik_hip.so (propose -> batched FSM ->
L2 misfit with analytic origin time -> Metropolis).  Multi-GPU runs shard the
global chain ids over ranks (`shard`), one process per GPU.
"""
import ctypes as C
import hashlib
from dataclasses import dataclass, field

import numpy as np

from . import _lib

P_PRIMARY_PICK, S_PRIMARY_PICK = 1, 2

# the BASELINE.json configurations (SURVEY s.8): name -> (n, stations, events, chains)
CONFIGS = {
    "C1": dict(n=32, nstat=4, nev=4, nchains=1, h=1000.0, homogeneous=True),
    "C2": dict(n=64, nstat=16, nev=16, nchains=256, h=100.0, homogeneous=False),
    "C3": dict(n=128, nstat=32, nev=32, nchains=1024, h=100.0, homogeneous=False),
    "C4": dict(n=128, nstat=32, nev=32, nchains=8192, h=100.0, homogeneous=False),
    "C5": dict(n=256, nstat=64, nev=64, nchains=2048, h=100.0, homogeneous=False),
}


@dataclass
class Problem:
    """Grid, stations, events and picks of one tomography problem."""
    nx: int
    ny: int
    nz: int
    h: float
    nref: tuple = (4, 4, 4)
    x0: float = 0.0
    y0: float = 0.0
    z0: float = 0.0
    maxit: int = 50
    tol: float = 1e-8
    sx: np.ndarray = None           # station coordinates (m) = eikonal sources
    sy: np.ndarray = None
    sz: np.ndarray = None
    pcorr: np.ndarray = None
    ex: np.ndarray = None           # event coordinates (m)
    ey: np.ndarray = None
    ez: np.ndarray = None
    obs_ptr: np.ndarray = None      # CSR by event (0-based), mceik_catalog_struct.obsPtr
    obs_stat: np.ndarray = None     # 0-based station per observation
    pick_type: np.ndarray = None
    luse: np.ndarray = None
    tobs: np.ndarray = None
    var: np.ndarray = None
    vmin: int = 1500
    vmax: int = 9000
    dvmax: int = 50
    nphase: int = 1                 # velocity models per chain: 1 = P, 2 = P and S (homog.c:208-258)
    vsmin: int = 800                # S prior (nphase 2)
    vsmax: int = 5500
    mask_s: int = 0                 # nphase 1: ignore used S picks instead of refusing the catalog
    scorr: np.ndarray = None        # S static corrections (mceik_stations_struct.scorr)
    seed: int = 2016
    nburn: int = 0
    keepk: int = 1
    niter: int = 0                  # mcparms.niter: total proposals (Sampler.run(-1) runs the rest)
    tt_interp: int = 0              # 0: event times at the nearest node (reference); 1: trilinear in the cell
    v_true: np.ndarray = None       # [ncell] int, model used to make the picks
    vs_true: np.ndarray = None      # [ncell] int, S model of the picks (P/S problems)
    has_p: np.ndarray = None        # [nstat] lhasP (mceik_struct.h:43-46); None: stations with used P picks
    has_s: np.ndarray = None        # [nstat] lhasS; None: stations with used S picks
    lcartesian: int = 1             # mceik_stations_struct.lcartesian (the sampler takes metres only)
    _keep: list = field(default_factory=list, repr=False)

    @property
    def ncx(self):
        return -(-self.nx // self.nref[0])

    @property
    def ncy(self):
        return -(-self.ny // self.nref[1])

    @property
    def ncz(self):
        return -(-self.nz // self.nref[2])

    @property
    def ncell(self):
        return self.ncx * self.ncy * self.ncz

    @property
    def nstat(self):
        return len(self.sx)

    @property
    def nevents(self):
        return len(self.ex)

    # --- quantities the oracle mirror needs (tests/_oracle.make_problem) ---
    @property
    def nrx(self):
        return self.nref[0]

    @property
    def nry(self):
        return self.nref[1]

    @property
    def nrz(self):
        return self.nref[2]

    @property
    def ev_node(self):
        """Nearest node of each event, as the reference snaps sources (fsm3d.f90:697-711)."""
        def idx(n, x0, xs):
            xs = np.asarray(xs, dtype=np.float64)
            i = (((xs - x0) / self.h + 0.5).astype(np.int64))
            i = np.where(xs <= x0, 0, np.where(xs >= x0 + (n - 1) * self.h, n - 1, i))
            return i
        ix, iy, iz = idx(self.nx, self.x0, self.ex), idx(self.ny, self.y0, self.ey), idx(self.nz, self.z0, self.ez)
        return ((iz * self.ny + iy) * self.nx + ix).astype(np.int32)

    @property
    def ev_cell(self):
        """Trilinear mode (tt_interp = 1): (lowest corner node [nev] int32, fractions
        [nev][3] float32) of each event's grid cell, as mceik_mcmc_init computes them
        (sampler.hip cell_corner: i = trunc((x - x0)/h) clamped to [0, n-2], w = f - i in
        [0, 1] rounded once to fp32)."""
        def corner(n, x0, xs):
            f = (np.asarray(xs, dtype=np.float64) - x0) / self.h
            i = np.where(f <= 0.0, 0, np.trunc(np.maximum(f, 0.0))).astype(np.int64)
            i = np.minimum(i, n - 2)
            w = np.clip(f - i, 0.0, 1.0).astype(np.float32)
            return i, w
        ix, wx = corner(self.nx, self.x0, self.ex)
        iy, wy = corner(self.ny, self.y0, self.ey)
        iz, wz = corner(self.nz, self.z0, self.ez)
        return ((iz * self.ny + iy) * self.nx + ix).astype(np.int32), np.stack([wx, wy, wz], 1)

    @property
    def obs_used(self):
        """Observations the sampler fits (mceik_mcmc_init): used P picks, and used
        S picks when the chains hold an S model."""
        k = self.obs_stat
        ok = (self.luse != 0) & (k >= 0) & (k < self.nstat)
        sel = self.pick_type == P_PRIMARY_PICK
        if self.nphase > 1:
            sel = sel | (self.pick_type == S_PRIMARY_PICK)
        return ok & sel

    @property
    def obs_mask(self):
        return (~self.obs_used).astype(np.int32)

    @property
    def obs_phase(self):
        """0 = P, 1 = S: the model an observation is fit against."""
        return (self.obs_used & (self.pick_type == S_PRIMARY_PICK)).astype(np.int32)

    @property
    def tcorr(self):
        sc = self.scorr if self.scorr is not None else np.zeros(self.nstat)
        corr = np.where(self.obs_phase == 1, sc[self.obs_stat], self.pcorr[self.obs_stat])
        return np.where(self.obs_mask == 0, corr, 0.0)

    def station_flags(self):
        """(lhasP, lhasS) [nstat] int: the explicit has_p / has_s, else whether
        the station has a used pick of the phase (homog.c:230-235 sets them per
        station from its picks).  The sampler solves a station's P (S) table
        only when its flag is set."""
        def has(t):
            sel = (self.luse != 0) & (self.pick_type == t)
            return np.array([bool((sel & (self.obs_stat == k)).any()) for k in range(self.nstat)], np.int32)
        hp = np.asarray(self.has_p, np.int32) if self.has_p is not None else has(P_PRIMARY_PICK)
        hs = np.asarray(self.has_s, np.int32) if self.has_s is not None else has(S_PRIMARY_PICK)
        return hp, hs

    @property
    def skip(self):
        """[nphase][nstat] uint8: solves the sampler skips (no picks of that phase)."""
        hp, hs = self.station_flags()
        return np.stack([hp == 0, hs == 0][:max(1, self.nphase)]).astype(np.uint8)

    @property
    def n_s_picks(self):
        k = self.obs_stat
        return int(((self.luse != 0) & (k >= 0) & (k < self.nstat) & (self.pick_type == S_PRIMARY_PICK)).sum())

    # --- mceik_struct.h views (ctypes), kept alive on the problem ---
    def structs(self):
        keep = self._keep
        keep.clear()

        def dp(a):
            a = np.ascontiguousarray(a, dtype=np.float64); keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_double))

        def ip(a):
            a = np.ascontiguousarray(a, dtype=np.int32); keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_int))

        parms = _lib.MceikParms()
        parms.mcparms.nburnIn = int(self.nburn)
        parms.mcparms.niter = int(self.niter)
        parms.mcparms.keepK = int(self.keepk)
        parms.eikparms.tol = float(self.tol)
        parms.eikparms.maxit = int(self.maxit)
        parms.projnm = b"mceik_amd"
        parms.x0, parms.y0, parms.z0 = self.x0, self.y0, self.z0
        parms.dx = parms.dy = parms.dz = float(self.h)
        parms.ndivx = parms.ndivy = parms.ndivz = 1
        parms.nrefx, parms.nrefy, parms.nrefz = (int(v) for v in self.nref)
        st = _lib.StationsStruct()
        st.nstat = self.nstat
        st.lcartesian = int(self.lcartesian)
        st.xrec, st.yrec, st.zrec = dp(self.sx), dp(self.sy), dp(self.sz)
        st.pcorr = dp(self.pcorr)
        st.scorr = dp(self.scorr if self.scorr is not None else np.zeros(self.nstat))
        hp, hs = self.station_flags()
        st.lhasP = ip(hp)
        st.lhasS = ip(hs)
        cat = _lib.CatalogStruct()
        cat.nevents = self.nevents
        cat.xsrc, cat.ysrc, cat.zsrc = dp(self.ex), dp(self.ey), dp(self.ez)
        cat.tori = dp(np.zeros(self.nevents))
        cat.tobs = dp(self.tobs)
        cat.test = dp(np.zeros_like(self.tobs))
        cat.varObs = dp(self.var)
        cat.luseObs = ip(self.luse)
        cat.pickType = ip(self.pick_type)
        cat.statPtr = ip(self.obs_stat + 1)          # 1-based, homog.c:227
        cat.obsPtr = ip(self.obs_ptr)
        return parms, st, cat


def cell_velocity(p: Problem):
    """Heterogeneous base model on the inversion grid (SURVEY s.8d), int m/s."""
    k, j, i = np.meshgrid(np.arange(p.ncz), np.arange(p.ncy), np.arange(p.ncx), indexing="ij")
    xi, eta, zeta = (i + 0.5) / p.ncx, (j + 0.5) / p.ncy, (k + 0.5) / p.ncz
    v = 3000.0 + 4000.0 * zeta + 500.0 * np.sin(6 * np.pi * xi) * np.cos(4 * np.pi * eta) * np.sin(4 * np.pi * zeta)
    return np.rint(v).astype(np.int32).ravel()


def make_problem(config="C3", n=None, nstat=None, nev=None, h=None, homogeneous=None, nref=(4, 4, 4),
                 seed=2016, maxit=50, tol=1e-8, picks="analytic", phases="P"):
    """Synthetic problem of a BASELINE configuration (SURVEY s.8d).

    picks: 'analytic' -> straight-ray times in the mean velocity (no GPU needed);
           a callable(problem, phase) -> [nstat, nev] travel times in the P
           (phase 0) or S (phase 1) model, e.g. the GPU forward of `v_true` /
           `vs_true` (see `picks_from_forward`).  Gaussian noise (sigma 0.05 s)
           is added, varObs = 0.25 s^2 (homog.c:55-56).
    phases: 'P' (every station picks P of every event) or 'PS' (a P and an S
           pick per station and event, in homog.c's order, homog.c:203-229;
           the chains then hold a P and an S model, vs = vp / sqrt(3) as
           homog.c:53-54).
    """
    cfg = dict(CONFIGS[config])
    n = n or cfg["n"]; nstat = nstat or cfg["nstat"]; nev = nev or cfg["nev"]
    h = h or cfg["h"]
    homogeneous = cfg["homogeneous"] if homogeneous is None else homogeneous
    rng = np.random.default_rng(seed)
    p = Problem(nx=n, ny=n, nz=n, h=h, nref=tuple(nref), maxit=maxit, tol=tol, seed=seed)
    ext = (n - 1) * h
    # stations on the top face, x/y off-grid and >= 2 nodes from the edges
    p.sx = rng.uniform(2 * h, ext - 2 * h, nstat)
    p.sy = rng.uniform(2 * h, ext - 2 * h, nstat)
    p.sz = np.full(nstat, ext)
    p.pcorr = np.zeros(nstat)
    p.scorr = np.zeros(nstat)
    p.ex = rng.uniform(h, ext - h, nev)
    p.ey = rng.uniform(h, ext - h, nev)
    p.ez = rng.uniform(h, ext - h, nev)
    p.v_true = np.full(p.ncell, 2000 if config == "C1" else 4000, np.int32) if homogeneous else cell_velocity(p)
    nph = 2 if phases == "PS" else 1
    if phases not in ("P", "PS"):
        raise ValueError(f"phases: 'P' or 'PS', not {phases!r}")
    p.nphase = nph
    if nph == 2:
        p.vs_true = np.rint(p.v_true / np.sqrt(3.0)).astype(np.int32)
    # every station sees every event, CSR by event; per station P (then S)
    per = nstat * nph
    p.obs_ptr = (np.arange(nev + 1) * per).astype(np.int32)
    p.obs_stat = np.tile(np.repeat(np.arange(nstat, dtype=np.int32), nph), nev)
    p.pick_type = np.tile(np.arange(1, nph + 1, dtype=np.int32), nev * nstat)
    p.luse = np.ones(nev * per, np.int32)
    p.var = np.full(nev * per, 0.25)
    tt = np.empty((nph, nstat, nev))
    for ph in range(nph):
        if picks == "analytic":
            vmean = float(np.mean(p.vs_true if ph else p.v_true))
            d = np.sqrt((p.sx[:, None] - p.ex[None]) ** 2 + (p.sy[:, None] - p.ey[None]) ** 2 +
                        (p.sz[:, None] - p.ez[None]) ** 2)
            tt[ph] = d / vmean                           # [nstat, nev]
        else:
            tt[ph] = np.asarray(picks(p, ph) if nph == 2 else picks(p), dtype=np.float64).reshape(nstat, nev)
    # observation (e, k, ph) at e*per + k*nph + ph
    p.tobs = (tt.transpose(2, 1, 0).ravel() + rng.normal(0.0, 0.05, nev * per)).astype(np.float64)
    return p


def initial_models(p: Problem, chain_ids, amp=50):
    """Per-chain start model: v_true + integer noise in [-amp, amp], keyed by the
    GLOBAL chain id so the chains do not depend on how they are sharded.
    [n, ncell] for P problems, [n, 2, ncell] (P, S) for P/S problems."""
    if p.nphase == 1:
        out = np.empty((len(chain_ids), p.ncell), np.int32)
        for r, gid in enumerate(chain_ids):
            g = np.random.default_rng([p.seed, int(gid)])
            out[r] = np.clip(p.v_true + g.integers(-amp, amp + 1, p.ncell), p.vmin, p.vmax)
        return out
    out = np.empty((len(chain_ids), 2, p.ncell), np.int32)
    for r, gid in enumerate(chain_ids):
        g = np.random.default_rng([p.seed, int(gid)])
        out[r, 0] = np.clip(p.v_true + g.integers(-amp, amp + 1, p.ncell), p.vmin, p.vmax)
        g = np.random.default_rng([p.seed, int(gid), 1])
        out[r, 1] = np.clip(p.vs_true + g.integers(-amp, amp + 1, p.ncell), p.vsmin, p.vsmax)
    return out


def shard(nchains_total, rank, world):
    """Contiguous block of global chain ids for `rank` (SURVEY s.8e)."""
    base, extra = divmod(nchains_total, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def temper_ladder(ntemps, tmax):
    """The geometric ladder beta[r] = tmax^(-r / (ntemps - 1)), beta[0] = 1
    exactly (mceik_temper_ladder; host only)."""
    beta = np.empty(max(int(ntemps), 1), np.float64)
    if _lib.lib().mceik_temper_ladder(int(ntemps), float(tmax), beta.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("temper_ladder: ntemps >= 1 and a finite tmax >= 1")
    return beta


def cold_chain_ids(nchains_total, world, ntemps):
    """Global ids of the cold chains (beta = 1) of a tempered run under
    `shard`'s split: the first nchains / ntemps chains of every rank's shard
    (replica groups never span ranks).  int64 array, ascending."""
    out = []
    for rank in range(world):
        lo, hi = shard(nchains_total, rank, world)
        if (hi - lo) % ntemps:
            raise ValueError(f"rank {rank} holds {hi - lo} chains: not a multiple of ntemps = {ntemps}")
        out.append(np.arange(lo, lo + (hi - lo) // ntemps, dtype=np.int64))
    return np.concatenate(out) if out else np.empty(0, np.int64)


def block_footprint(p, cell, radius, amp):
    """The footprint of one block proposal (mceik_block_footprint; host only):
    (cells, dv) int32 arrays -- the cells of one ncx x ncy x ncz model of
    `p` that a proposal of signed amplitude `amp` and radius `radius` centred
    on `cell` touches, in x-fastest order of the offsets, and what each moves by."""
    n = (2 * int(radius) + 1) ** 3 if 0 <= int(radius) <= 8 else 1
    cells, dv = np.empty(n, np.int32), np.empty(n, np.int32)
    cnt = _lib.lib().mceik_block_footprint(int(p.ncx), int(p.ncy), int(p.ncz), int(cell), int(radius), int(amp),
                                           cells.ctypes.data_as(C.c_void_p), dv.ctypes.data_as(C.c_void_p))
    if cnt < 0:
        raise ValueError("block_footprint: cell inside the model, radius in [0, 8], amp != 0")
    return cells[:cnt].copy(), dv[:cnt].copy()


def _prior_model(grid, a, name):
    a = np.ascontiguousarray(a, dtype=np.int32).ravel()
    if a.size != int(grid.ncx) * int(grid.ncy) * int(grid.ncz):
        raise ValueError(f"{name}: one model of ncx * ncy * ncz cells")
    return a


def prior_energy(grid, v, vref=None):
    """(Es, Ed) of one ncx x ncy x ncz model `v` of `grid` (a Problem, or
    anything with ncx, ncy, ncz), cells x fastest (mceik_prior_energy; host
    only): the roughness sum of (v_i - v_j)^2 over face-adjacent pairs and the
    damping sum of (v_i - vref_i)^2 (0 without `vref`), exact integers."""
    v = _prior_model(grid, v, "v")
    r = None if vref is None else _prior_model(grid, vref, "vref")
    es, ed = C.c_longlong(0), C.c_longlong(0)
    rc = _lib.lib().mceik_prior_energy(int(grid.ncx), int(grid.ncy), int(grid.ncz), v.ctypes.data_as(C.c_void_p),
                                       None if r is None else r.ctypes.data_as(C.c_void_p), C.byref(es), C.byref(ed))
    if rc != 0:
        raise ValueError("prior_energy: a grid of at least one cell whose 3 ncell span^2 stays below 2^53")
    return es.value, ed.value


def prior_delta(grid, v, cell, radius, amp, vref=None):
    """(dEs, dEd): what `prior_energy` changes by when the block footprint
    (`block_footprint`) of signed amplitude `amp` and radius `radius` centred
    on `cell` is added to `v` (mceik_prior_delta; host only, the arithmetic of
    the sampler's fold kernel)."""
    v = _prior_model(grid, v, "v")
    r = None if vref is None else _prior_model(grid, vref, "vref")
    es, ed = C.c_longlong(0), C.c_longlong(0)
    rc = _lib.lib().mceik_prior_delta(int(grid.ncx), int(grid.ncy), int(grid.ncz), v.ctypes.data_as(C.c_void_p),
                                      None if r is None else r.ctypes.data_as(C.c_void_p), int(cell), int(radius),
                                      int(amp), C.byref(es), C.byref(ed))
    if rc != 0:
        raise ValueError("prior_delta: cell inside the model, radius in [0, 8], amp != 0, 3 ncell span^2 < 2^53")
    return es.value, ed.value


def hypo_draw(seed, gchain, step, e, dmax=(1, 1, 1)):
    """The hypocentre draw of event `e` of global chain `gchain` at global step
    `step` (mceik_hypo_draw; host only): (d int32 [3] in [-dmax, dmax] per axis,
    log u)."""
    dm = np.ascontiguousarray(dmax, dtype=np.int32).ravel()
    if dm.size != 3:
        raise ValueError("hypo_draw: dmax is one value per axis")
    d, logu = np.zeros(3, np.int32), C.c_double(0.0)
    rc = _lib.lib().mceik_hypo_draw(int(seed), int(gchain), int(step), int(e), dm.ctypes.data_as(C.c_void_p),
                                    d.ctypes.data_as(C.c_void_p), C.byref(logu))
    if rc != 0:
        raise ValueError("hypo_draw: e >= 0 and every dmax >= 0")
    return d, logu.value


def det_exp(x):
    """The sampler's deterministic exp (mceik_det_exp; host only): IEEE + - * /
    only, bit for bit what the Langevin kernels compute."""
    return float(_lib.lib().mceik_det_exp(float(x)))


def lang_cell(seed, gchain, step, cell, d, v, vlo, vhi, sigma, dmax):
    """The discrete Langevin proposal of one cell (mceik_lang_cell; host only):
    cell `cell` of global chain `gchain` at global step `step`, drift d, velocity
    v in the box [vlo, vhi].  Returns (delta, lo, logq float64 [hi - lo + 1]):
    the drawn move, the support's lowest value and log q of every support value
    lo, lo + 1, ..."""
    delta, lo, hi = C.c_int(0), C.c_int(0), C.c_int(0)
    logq = np.zeros(2 * _lib.LANG_DMAX_CAP + 1, np.float64)
    rc = _lib.lib().mceik_lang_cell(int(seed), int(gchain), int(step), int(cell), float(d), int(v), int(vlo), int(vhi),
                                    float(sigma), int(dmax), C.byref(delta), C.byref(lo), C.byref(hi),
                                    logq.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError(f"lang_cell: cell >= 0, sigma > 0, 1 <= dmax <= {_lib.LANG_DMAX_CAP}, vlo <= v <= vhi")
    return delta.value, lo.value, logq[:hi.value - lo.value + 1].copy()


DE_GQ_MAX, DE_CRQ_MAX = 131072, 65536


def de_delta(gq, d, word, crq=DE_CRQ_MAX):
    """The DE move of one cell (mceik_de_delta; host only): partners differing
    by d = v_a - v_b, the cell's 32-bit Philox word, gq = round(gamma * 65536),
    crq = round(cr * 65536).  0 unless (word >> 16) < crq, else floor((gq d + rr
    + 0.5) / 65536) with rr = word & 0xFFFF."""
    out = C.c_int(0)
    if _lib.lib().mceik_de_delta(int(gq), int(d), int(word) & 0xFFFFFFFF, int(crq), C.byref(out)) != 0:
        raise ValueError(f"de_delta: 1 <= gq <= {DE_GQ_MAX}, 1 <= crq <= {DE_CRQ_MAX}, delta within int32")
    return out.value


def de_draw(seed, gchain, step, nb):
    """The step draw of a DE mover (mceik_de_draw; host only): (i, j, log u),
    i != j the ordered pair of members of a partner set of nb >= 2."""
    i, j, logu = C.c_int(0), C.c_int(0), C.c_double(0.0)
    if _lib.lib().mceik_de_draw(int(seed), int(gchain), int(step), int(nb), C.byref(i), C.byref(j), C.byref(logu)) != 0:
        raise ValueError("de_draw: nb >= 2")
    return i.value, j.value, logu.value


def de_movers(nchains, ntemps, k):
    """DE step k of a sampler of `nchains` local chains in `ntemps` rungs (0 or
    1: untempered): (movers, partners), movers the local chains that move, in
    order, and partners[c] for each of them the partner set of its rung, in
    order: the population of a chain is its rung, rung r holds
    chains r * G + g, and g & 1 == k & 1 moves."""
    nt = max(1, int(ntemps))
    if nchains % nt:
        raise ValueError("de_movers: nchains is a multiple of ntemps")
    G, par = nchains // nt, int(k) & 1
    movers = [c for c in range(nchains) if ((c % G) & 1) == par]
    partners = {c: [(c // G) * G + g for g in range(G) if (g & 1) != par] for c in movers}
    return movers, partners


VOR_KMAX = 512
VOR_TYPES = ("value", "move", "birth", "death")
VOR_COUNTERS = ("attempts", "accepts", "reason1", "reason2", "reason3")


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def vor_raster(grid, cells, vals, metric=(1, 1, 1)):
    """The raster of Voronoi nuclei (mceik_vor_raster; host only): int32 [ncell]
    of the grid (a Problem, or (ncx, ncy, ncz)), v[cell] the value of the
    nucleus minimising (mx dx)^2 + (my dy)^2 + (mz dz)^2 in cell-index units,
    ties to the nucleus in the smaller cell."""
    ncx, ncy, ncz = (grid.ncx, grid.ncy, grid.ncz) if hasattr(grid, "ncx") else (int(x) for x in grid)
    c, w, m = _i32(cells).ravel(), _i32(vals).ravel(), _i32(metric).ravel()
    if c.size != w.size or m.size != 3:
        raise ValueError("vor_raster: as many values as cells, and a metric of three")
    v = np.empty(max(ncx * ncy * ncz, 1), np.int32)
    if _lib.lib().mceik_vor_raster(ncx, ncy, ncz, m.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                   w.ctypes.data_as(C.c_void_p), int(c.size), v.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("vor_raster: at least one nucleus, cells on the grid, a positive metric whose largest "
                         "squared distance fits 31 bits")
    return v


def vor_free_cell(cells, ncell, f):
    """The f-th (from 0) cell of [0, ncell) in ascending order that holds none
    of the nuclei `cells` (mceik_vor_free_cell; host only)."""
    c = _i32(cells).ravel()
    r = _lib.lib().mceik_vor_free_cell(c.ctypes.data_as(C.c_void_p), int(c.size), int(ncell), int(f))
    if r < 0:
        raise ValueError("vor_free_cell: cells in [0, ncell) and 0 <= f < ncell - k")
    return r


def vor_draw(seed, gchain, step, k, ncell, dv, vlo, vhi, dmax=(1, 1, 1)):
    """The draw of a Voronoi step (mceik_vor_draw; host only) for a phase model
    of k nuclei: {"type" (0 value, 1 move, 2 birth, 3 death), "j", "f", "delta",
    "wnew", "d" (dx, dy, dz), "logu"} -- each move type reads its own fields
    (DESIGN.md s.22)."""
    out, logu, dm = np.zeros(8, np.int32), C.c_double(0.0), _i32(dmax).ravel()
    if dm.size != 3 or _lib.lib().mceik_vor_draw(int(seed), int(gchain), int(step), int(k), int(ncell), int(dv), int(vlo),
                                                 int(vhi), dm.ctypes.data_as(C.c_void_p),
                                                 out.ctypes.data_as(C.c_void_p), C.byref(logu)) != 0:
        raise ValueError("vor_draw: 1 <= k <= ncell, dv >= 1, vlo <= vhi, dmax >= 0 per axis")
    return {"type": int(out[0]), "j": int(out[1]), "f": int(out[2]), "delta": int(out[3]), "wnew": int(out[4]),
            "d": (int(out[5]), int(out[6]), int(out[7])), "logu": logu.value}


def nuis_ladder(nk, lam_min, lam_max):
    """(lam, lnlam) float64 [nk]: a log-uniform noise ladder from lam_min to
    lam_max for `Sampler.nuis_enable`, lnlam[k] = (k - nk // 2) * ln(lam_max) /
    (nk // 2) and lam = exp(lnlam), so that the middle entry -- the chains'
    start value -- is exactly lam = 1.0, lnlam = 0.0.  nk is odd and lam_min is
    1 / lam_max (None: that): equal steps in ln lam on both sides of 1 are what
    makes a uniform prior on the index a log-uniform prior on the scale."""
    nk, lam_max = int(nk), float(lam_max)
    if nk < 1 or nk % 2 == 0:
        raise ValueError("nuis_ladder: nk is odd (the middle entry is the start value lam = 1)")
    if not (lam_max >= 1.0 and np.isfinite(lam_max)):
        raise ValueError("nuis_ladder: a finite lam_max >= 1")
    if lam_min is not None and not np.isclose(float(lam_min) * lam_max, 1.0, rtol=1e-12, atol=0.0):
        raise ValueError("nuis_ladder: lam_min is 1 / lam_max (a ladder with equal steps in ln lam around lam = 1)")
    mid = nk // 2
    lnlam = np.array([(k - mid) * (np.log(lam_max) / mid) if mid else 0.0 for k in range(nk)], np.float64)
    lam = np.exp(lnlam)
    lam[mid], lnlam[mid] = 1.0, 0.0
    return lam, lnlam


def nuis_active(p):
    """int32 [nphase] lists of the stations statics moves draw from: those with
    a used pick of the phase, in station order (`Sampler.nuis_enable`)."""
    used, ph = p.obs_mask == 0, p.obs_phase
    return [np.unique(p.obs_stat[used & (ph == q)]).astype(np.int32) for q in range(p.nphase)]


def nuis_draw(seed, gchain, step, sub, nnoise, nact, dk=1, dc=1):
    """Sub-move `sub` of global chain `gchain` at global step `step`
    (mceik_nuis_draw; host only): ((kind, phase, a, b, delta), log u) with kind
    0 a noise move of `phase` by delta ladder entries, kind 1 a statics move of
    the a-th and b-th active stations of `phase` by +delta and -delta units.
    nnoise = nphase with the noise part on, else 0; nact = active stations per
    phase that the statics part draws from (0 or >= 2 each)."""
    na = [int(x) for x in np.ravel(nact)] + [0]
    if len(na) > 3:
        raise ValueError("nuis_draw: nact is one count per phase")
    m, logu = np.zeros(5, np.int32), C.c_double(0.0)
    rc = _lib.lib().mceik_nuis_draw(int(seed), int(gchain), int(step), int(sub), int(nnoise), na[0], na[1], int(dk),
                                    int(dc), m.ctypes.data_as(C.c_void_p), C.byref(logu))
    if rc != 0:
        raise ValueError("nuis_draw: sub >= 0, nnoise in [0, 2], every nact 0 or >= 2, something to move, dk, dc >= 0")
    return tuple(int(x) for x in m), logu.value


def prior_weight(sigma):
    """w = 1 / (2 sigma^2) per phase from a sigma in m/s: a scalar (both
    phases) or a (P, S) pair; None is weight 0."""
    if sigma is None:
        return (0.0, 0.0)
    pair = tuple(sigma) if np.ndim(sigma) else (sigma, sigma)
    if len(pair) != 2:
        raise ValueError("a sigma is a scalar or a (P, S) pair")
    out = []
    for s in pair:
        if s is None:
            out.append(0.0)
            continue
        s = float(s)
        if not (s > 0.0 and np.isfinite(s)):
            raise ValueError("a sigma is positive and finite (None: weight 0)")
        out.append(1.0 / (2.0 * s * s))
    return tuple(out)


def _nuis_same(a, b):
    """Two option dicts of `Sampler.nuis_enable` describe the same moves."""
    def eq(x, y):
        if x is None or y is None:
            return x is None and y is None
        return np.asarray(x, np.float64).tobytes() == np.asarray(y, np.float64).tobytes()
    return set(a) == set(b) and all(eq(a[k], b[k]) for k in a)


_DE_COUNTERS = ("attempts", "accepts", "outbox", "failed", "moved")


class _Kept:
    """One accumulator of kept states as `Sampler` drives it (csrc/kept.h has the
    C side): `stem` of its mceik_mcmc_<stem>_* entry points and its checkpoint
    key, the Sampler attribute `attr` that holds the enabled options, and as
    functions of the sampler and those options the ordered table of its arrays
    `{key: (shape, dtype)}` (the order of get / set; `slots`: the full argument
    list where an option leaves arrays out), the `extra` entries of `*_raw()`,
    whether a checkpoint entry was taken with the `same` options, and the
    empty `*Partials`."""

    def __init__(self, stem, attr, not_enabled, mismatch, arrays, extra, same, partials, slots=None):
        self.stem, self.attr, self.not_enabled, self.mismatch = stem, attr, not_enabled, mismatch
        self.arrays, self.extra, self.same, self.partials, self.slots = arrays, extra, same, partials, slots


def _probe_list(raw):
    return [tuple(int(x) for x in pr) for pr in raw["probes"]]


def _posterior_arrays(smp, held):
    per_chain, nbins = held
    shape = smp.model_shape if per_chain else smp.model_shape[1:]
    return {"sum": (shape, np.int64), "sumsq": (shape, np.int64), "hist": (smp.model_shape[1:] + (nbins,), np.uint32)}


def _cov_arrays(smp, held):
    lst, within = held
    n, ncm, nch = len(lst), smp.p.nphase * smp.p.ncell, smp.nchains
    shapes = {"A": (n,), "G": (n, n), "S": (ncm,), "Q": (ncm,), "C": (n, ncm)}
    if within:
        shapes.update({"Ac": (nch, n), "Sc": (nch, ncm)})
    return {k: (sh, np.int64) for k, sh in shapes.items()}


def _ess_arrays(smp, held):
    L, lst = held
    ne, nch = smp.p.nphase * smp.p.ncell + len(lst), smp.nchains
    return {"Sc": ((nch, ne), np.int64), "pend": ((L - 1, nch, ne), np.int32), "A": ((L, ne), np.int64),
            "Q": ((L, ne, 2), np.uint64), "P": ((L, ne, 2), np.uint64)}


def _fit_arrays(smp, held):
    nbins, p = held[1], smp.p
    nobs, nev = len(p.tobs), p.nevents
    return {"sq": ((nobs,), np.int64), "szq": ((nobs,), np.int64), "sq2": ((nobs, 2), np.uint64),
            "szq2": ((nobs, 2), np.uint64), "stq": ((nev,), np.int64), "stq2": ((nev, 2), np.uint64),
            "hist": ((max(1, p.nphase), p.nstat, nbins), np.int64), "sat": ((3,), np.int64)}


def _posterior_parts(smp, held):
    p = smp.p
    bounds = [(p.vmin, p.vmax), (p.vsmin, p.vsmax)][:p.nphase]
    return PosteriorPartials(p.nphase * p.ncell, held[1], held[0], shape=smp.model_shape[1:], bounds=bounds)


_KEPT = {d.stem: d for d in (
    _Kept("posterior", "_post", "the posterior is not enabled (Sampler.posterior_enable)",
          "the checkpoint's posterior was accumulated with other options", _posterior_arrays,
          lambda held: {"per_chain": held[0], "nbins": held[1]},
          lambda held, raw: (bool(raw["per_chain"]), int(raw["nbins"])) == held, _posterior_parts),
    _Kept("cov", "_cov", "the covariances are not enabled (Sampler.cov_enable)",
          "the checkpoint's covariance sums were accumulated with another probe list or `within`", _cov_arrays,
          lambda held: {"probes": list(held[0]), "within": held[1]},
          lambda held, raw: (_probe_list(raw), bool(raw["within"])) == held,
          lambda smp, held: CovPartials(held[0], smp.p.nphase * smp.p.ncell, held[1], shape=smp.model_shape[1:]),
          slots=("A", "G", "S", "Q", "C", "Ac", "Sc")),
    _Kept("ess", "_ess", "the batch-means sums are not enabled (Sampler.ess_enable)",
          "the checkpoint's batch-means sums were accumulated with another nlevels or probe list", _ess_arrays,
          lambda held: {"nlevels": held[0], "probes": list(held[1])},
          lambda held, raw: (int(raw["nlevels"]), _probe_list(raw)) == held,
          lambda smp, held: EssPartials(smp.p.nphase * smp.p.ncell, held[0], probes=held[1], shape=smp.model_shape[1:])),
    _Kept("fit", "_fit", "the data-fit sums are not enabled (Sampler.fit_enable)",
          "the checkpoint's data-fit sums were accumulated with other options", _fit_arrays,
          lambda held: {"tick": held[0], "nbins": held[1], "zmax": held[2], "t0_ref": held[3].copy()},
          lambda held, raw: (float(raw["tick"]), int(raw["nbins"]), float(raw["zmax"])) == held[:3] and
          np.asarray(raw["t0_ref"], np.float64).tobytes() == held[3].tobytes(),
          lambda smp, held: FitPartials(len(smp.p.tobs), smp.p.nevents, max(1, smp.p.nphase), smp.p.nstat, held[1],
                                        held[0], held[2])))}


class Sampler:
    """One GPU's chains (include/mceik.h handle)."""

    def __init__(self, p: Problem, nchains, chain_offset=0, v0=None, max_samples=0, device=0, precision=32,
                 max_waves=0):
        self.p = p
        self.nchains = int(nchains)
        self.chain_offset = int(chain_offset)
        if v0 is None:
            v0 = initial_models(p, range(chain_offset, chain_offset + nchains))
        self.v0 = np.ascontiguousarray(v0, dtype=np.int32)
        assert self.v0.shape == self.model_shape, (self.v0.shape, self.model_shape)
        L = _lib.lib()
        parms, st, cat = p.structs()
        o = _lib.McmcOpts()
        o.nx, o.ny, o.nz = p.nx, p.ny, p.nz
        o.nchains, o.chain_offset = self.nchains, self.chain_offset
        o.vmin, o.vmax, o.dvmax, o.seed = p.vmin, p.vmax, p.dvmax, p.seed
        o.max_samples, o.device = int(max_samples), int(device)
        o.precision, o.max_waves = int(precision), int(max_waves)
        o.tt_interp = int(p.tt_interp)
        o.nphase, o.vsmin, o.vsmax, o.mask_s = int(p.nphase), int(p.vsmin), int(p.vsmax), int(p.mask_s)
        h = C.c_void_p()
        rc = L.mceik_mcmc_init(C.byref(parms), C.byref(st), C.byref(cat), C.byref(o),
                               self.v0.ctypes.data_as(C.c_void_p), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_init failed ({rc})")
        self._h = h
        self._L = L
        self.max_samples = int(max_samples)
        self.device, self.precision = int(device), (64 if int(precision) == 64 else 32)
        self._last_full = True          # the last forward solved every model (init / restore)
        self._post = None               # (per_chain, nbins) while the streaming posterior is enabled
        self._temper = None             # (betas, swap_every) while parallel tempering is enabled
        self._block = None              # (rmin, rmax) while block proposals are enabled
        self._prior = None              # (w_smooth, w_damp, vref digest) while the prior is enabled
        self._hypo = None               # (every, dmax, lo, hi) while hypocentre moves are enabled
        self._nuis = None               # the options while the sampler holds nuisance state (nuis_enable .. nuis_clear)
        self._stats_base = {}           # "temper" / "block" / "hypo" / "nuis" -> (attempts, accepts) of a restored
        #                                 checkpoint: added to the device counters (_move_stats)
        self._cov = None                # (probes [(kind, index)], within) while the sampler holds covariance sums
        self._lang = False              # Langevin moves were enabled at least once
        self._de = None                 # (every, offset, gq, crq) while DE moves are enabled
        self._vor = None                # (kmin, kmax, dv, dmax, metric) while Voronoi-cell models are enabled
        self._ess = None                # (nlevels, probes [(kind, index)]) while the sampler holds batch-means sums
        self._fit = None                # (tick, nbins, zmax, t0_ref) while the sampler holds data-fit sums
        self._fit_active = False        # ... and adds kept steps to them (fit_enable .. fit_disable)

    @property
    def model_shape(self):
        """Shape of the chains' models: [nchains, ncell] (P) or [nchains, 2, ncell] (P, S)."""
        p = self.p
        return (self.nchains, p.ncell) if p.nphase == 1 else (self.nchains, p.nphase, p.ncell)

    def set_stream(self, stream_ptr):
        self._L.mceik_mcmc_set_stream(self._h, C.c_void_p(stream_ptr))

    def run(self, nsteps):
        rc = self._L.mceik_mcmc_run(self._h, int(nsteps))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_run failed ({rc})")
        if nsteps:
            self._last_full = False

    def sync(self):
        rc = self._L.mceik_mcmc_sync(self._h)
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_sync failed ({rc})")

    def info(self):
        """mceik_mcmc_get_info as a dict (pipes, kernel instance, waves, workspaces)."""
        i = _lib.McmcInfo()
        if self._L.mceik_mcmc_get_info(self._h, C.byref(i)) != 0:
            raise RuntimeError("mceik_mcmc_get_info failed")
        n = i.npipe
        return {"npipe": n, "nphase": i.nphase, "step_z": i.step_z, "fixed_layout": bool(i.fixed_layout),
                "chains": list(i.chains[:n]), "waves": list(i.waves[:n]),
                "workspace_bytes": list(i.workspace_bytes[:n]), "lds_bytes": int(i.lds_bytes),
                "masked_s": i.masked_s, "kernel": i.kernel.decode(), "multi_step": bool(i.multi_step)}

    def likelihood_set(self, norm):
        """The likelihood's norm (mceik_mcmc_likelihood_set): 2 the
        weighted L2 misfit with the analytic origin time (default), 1 a Laplace
        density of scale var per pick with the weighted-median origin time.  Every
        chain's logL is recomputed with one full forward; models and step counter
        stay.  Refused (ValueError, nothing changed) for another norm, while
        Langevin moves are on, or while an enabled accumulator of kept states
        already holds states.  While norm = 1, `lang_enable` and `logl_grad` are
        refused and every step is a launch of its own."""
        rc = self._L.mceik_mcmc_likelihood_set(self._h, int(norm))
        if rc == 1:
            raise ValueError(f"likelihood_set({norm!r}) refused: norm is 1 or 2; Langevin moves must be off and no "
                             "enabled accumulator of kept states may hold states")
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_likelihood_set failed ({rc})")
        self._last_full = True

    @property
    def likelihood(self):
        """The likelihood's norm: 1 (Laplace) or 2 (Gaussian)."""
        return int(self._L.mceik_mcmc_likelihood_get(self._h))

    def state(self):
        v = np.empty(self.model_shape, np.int32)
        logl = np.empty(self.nchains, np.float64)
        nacc = np.empty(self.nchains, np.int64)
        step = C.c_longlong(0)
        rc = self._L.mceik_mcmc_get_state(self._h, v.ctypes.data_as(C.c_void_p), logl.ctypes.data_as(C.c_void_p),
                                          nacc.ctypes.data_as(C.c_void_p), C.byref(step))
        if rc != 0:
            raise RuntimeError("mceik_mcmc_get_state failed")
        return v, logl, nacc, step.value

    def last(self, with_ierr=False):
        """Host copies of the last forward's travel-time tables, iteration counts and
        accept flags (and the per-solve reference ierr if with_ierr).  After a step:
        [nchains, nstat, nev] / [nchains, nstat] of the model each proposal changed
        (`last_phase`); after init / restore with two models: [nchains, 2, nstat, nev]
        / [nchains, 2, nstat].  After a DE step (`de_enable`) accept is 0 for the
        standing chains, only the movers' rows are that step's, and `last_phase`
        is the step's phase for every chain."""
        tt, it, acc, ie = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._L.mceik_mcmc_last(self._h, C.byref(tt), C.byref(it), C.byref(acc), C.byref(ie))
        p = self.p
        mid = (p.nphase,) if (self._last_full and p.nphase > 1) else ()
        ttab = np.empty((self.nchains,) + mid + (p.nstat, p.nevents), np.float32)
        niter = np.empty((self.nchains,) + mid + (p.nstat,), np.int32)
        ierr = np.empty((self.nchains,) + mid + (p.nstat,), np.int32)
        a = np.empty(self.nchains, np.uint8)
        self.sync()
        for dst, src in ((ttab, tt), (niter, it), (a, acc), (ierr, ie)):
            if self._L.mceik_memcpy(dst.ctypes.data_as(C.c_void_p), src, dst.nbytes, 1) != 0:
                raise RuntimeError("mceik_memcpy failed")
        return (ttab, niter, a, ierr) if with_ierr else (ttab, niter, a)

    def last_phase(self):
        """The model each chain's last proposal changed (0 = P, 1 = S)."""
        ph = C.c_void_p()
        self._L.mceik_mcmc_last_phase(self._h, C.byref(ph))
        out = np.empty(self.nchains, np.int32)
        self.sync()
        if self._L.mceik_memcpy(out.ctypes.data_as(C.c_void_p), ph, out.nbytes, 1) != 0:
            raise RuntimeError("mceik_memcpy failed")
        return out

    def checkpoint(self):
        """Complete chain state (mceik_mcmc_checkpoint): dict of v, logl, naccept,
        step, nkept -- restore() into a sampler of the same problem/shard resumes
        the chains bit for bit."""
        v = np.empty(self.model_shape, np.int32)
        logl = np.empty(self.nchains, np.float64)
        nacc = np.empty(self.nchains, np.int64)
        step, nkept = C.c_longlong(0), C.c_int(0)
        if self._L.mceik_mcmc_checkpoint(self._h, v.ctypes.data_as(C.c_void_p), logl.ctypes.data_as(C.c_void_p),
                                         nacc.ctypes.data_as(C.c_void_p), C.byref(step), C.byref(nkept)) != 0:
            raise RuntimeError("mceik_mcmc_checkpoint failed")
        ck = {"v": v, "logl": logl, "naccept": nacc, "step": step.value, "nkept": nkept.value,
              "chain_offset": self.chain_offset, "seed": self.p.seed,
              "likelihood": self.likelihood}      # the norm decides what logl means
        for d in _KEPT.values():         # the accumulators, open batches included, belong to the state of a run that
            if getattr(self, d.attr) is not None:                                               # summarises itself
                ck[d.stem] = self._kept_raw(d)
        if self._temper is not None:     # the ladder decides what the chains sample; the counters ride along
            att, acc = self.temper_stats()
            ck["temper"] = {"betas": self._temper[0].copy(), "swap_every": self._temper[1],
                            "attempts": att, "accepts": acc}
        if self._block is not None:      # the radii decide what the chains propose; the counters ride along
            att, acc = self.block_stats()
            ck["block"] = {"rmin": self._block[0], "rmax": self._block[1], "attempts": att, "accepts": acc}
        if self._de is not None:         # the options decide what the chains propose; the counters ride along
            ck["de"] = dict(zip(("every", "offset", "gamma_q16", "cr_q16"), self._de), **self.de_stats())
        if self._vor is not None:        # the nuclei are chain state; the options decide what is proposed
            cells, vals, counts = self.vor_get()
            ck["vor"] = {"opts": self.vor_options(), "cells": cells, "vals": vals, "counts": counts,
                         "stats": self.vor_stats(), "moments": self.vor_moments()}
        if self._prior is not None:      # the weights and the reference model decide what the chains sample
            ck["prior"] = {"w_smooth": self._prior[0], "w_damp": self._prior[1], "vref_sha256": self._prior[2]}
        if self._hypo is not None:       # the positions are chain state; the options decide what is proposed
            att, acc = self.hypo_stats()
            n, sm, sq = self._hypo_moments()
            ck["hypo"] = {"every": self._hypo[0], "dmax": self._hypo[1], "lo": self._hypo[2], "hi": self._hypo[3],
                          "xyz": self.hypo_positions(), "attempts": att, "accepts": acc, "n": n, "sum": sm, "sq": sq}
        if self._nuis is not None:       # the values are chain state; the options decide what is proposed
            att, acc = self.nuis_stats()
            kn, kc = self.nuis_get()
            ck["nuis"] = {"opts": dict(self._nuis), "kn": kn, "kc": kc, "attempts": att, "accepts": acc,
                          "moments": self.nuis_moments()}
        return ck

    def restore(self, ck, recompute_logl=False):
        """Load a checkpoint() dict (mceik_mcmc_restore)."""
        if ck.get("chain_offset", self.chain_offset) != self.chain_offset or ck.get("seed", self.p.seed) != self.p.seed:
            raise ValueError("checkpoint belongs to another chain shard or seed")
        if int(ck.get("likelihood", 2)) != self.likelihood:      # a checkpoint without the entry is L2
            raise ValueError("the checkpoint was taken under the other likelihood norm (likelihood_set)")
        tk = ck.get("temper")            # a checkpoint without the entry carries no ladder and restores anywhere
        if tk is not None:
            mine = self._temper
            if mine is None or int(tk["swap_every"]) != mine[1] or \
                    np.asarray(tk["betas"], np.float64).tobytes() != mine[0].tobytes():
                raise ValueError("the checkpoint was taken with another temperature ladder or swap_every")
        bk = ck.get("block")             # likewise: a checkpoint without the entry restores anywhere
        if bk is not None and (self._block is None or (int(bk["rmin"]), int(bk["rmax"])) != self._block):
            raise ValueError("the checkpoint was taken with other block-proposal radii")
        dk = ck.get("de")                # likewise
        if dk is not None and (self._de is None or
                               tuple(int(dk[k]) for k in ("every", "offset", "gamma_q16", "cr_q16")) != self._de):
            raise ValueError("the checkpoint was taken with other DE-move options")
        vk = ck.get("vor")               # the nuclei describe v: a sampler with the models on wants them
        if vk is None and self._vor is not None:
            raise ValueError("Voronoi-cell models are on and the checkpoint carries no nuclei")
        if vk is not None:
            o = vk["opts"]
            if self._vor is None or (int(o["kmin"]), int(o["kmax"]), int(o["dv"]), tuple(int(x) for x in o["dmax"]),
                                     tuple(int(x) for x in o["metric"])) != self._vor:
                raise ValueError("the checkpoint was taken with other Voronoi-cell options")
            self.vor_set(vk["cells"], vk["vals"], vk["counts"], recompute_logl=False)   # (the restore below sets logL)
        pk = ck.get("prior")             # likewise
        if pk is not None and (self._prior is None or
                               (tuple(pk["w_smooth"]), tuple(pk["w_damp"]), pk["vref_sha256"]) != self._prior):
            raise ValueError("the checkpoint was taken with other prior weights or another reference model")
        hk = ck.get("hypo")              # likewise
        if hk is not None:
            if self._hypo is None or (int(hk["every"]), tuple(hk["dmax"]), tuple(hk["lo"]), tuple(hk["hi"])) != self._hypo:
                raise ValueError("the checkpoint was taken with other hypocentre-move options")
            self.hypo_set(hk["xyz"])     # (its forward is at the old models: the restore below sets logL)
        nk = ck.get("nuis")              # likewise; held values need the forward of the restore: it makes the
        if nk is not None:               # current tables every later nuisance step reads (and gives the saved logL)
            if self._nuis is None or not _nuis_same(nk["opts"], self._nuis):
                raise ValueError("the checkpoint was taken with other noise / statics options")
            self.nuis_set(nk["kn"], nk["kc"])
            recompute_logl = True
        elif self._nuis is not None:
            recompute_logl = True
        if self._fit_active and self.p.nphase == 1:
            recompute_logl = True        # a one-model sampler holds current tables for the data-fit sums: the forward makes them
        # a sampler without an accumulator ignores the checkpoint's entry; one with it wants sums of its own options
        kept = [(d, ck[d.stem]) for d in _KEPT.values() if ck.get(d.stem) is not None and getattr(self, d.attr) is not None]
        for d, raw in kept:
            if not d.same(getattr(self, d.attr), raw):
                raise ValueError(d.mismatch)
        v = np.ascontiguousarray(ck["v"], dtype=np.int32)
        assert v.shape == self.model_shape
        logl = None if recompute_logl else np.ascontiguousarray(ck["logl"], dtype=np.float64)
        nacc = np.ascontiguousarray(ck["naccept"], dtype=np.int64)
        rc = self._L.mceik_mcmc_restore(self._h, v.ctypes.data_as(C.c_void_p),
                                        None if logl is None else logl.ctypes.data_as(C.c_void_p),
                                        nacc.ctypes.data_as(C.c_void_p), int(ck["step"]), int(ck.get("nkept", 0)))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_restore failed ({rc})")
        if recompute_logl:
            self._last_full = True
        for d, raw in kept:
            self._kept_set(d, raw)
        if tk is not None:
            self._rebase_stats("temper", tk)
        if bk is not None:
            self._rebase_stats("block", bk)
        if dk is not None:               # zero the library's counters; the checkpoint's ride on as the base
            self.de_stats(reset=True)
            self._stats_base["de"] = {k: int(dk[k]) for k in _DE_COUNTERS}
        if vk is not None:               # zero the library's counters; the checkpoint's ride on as the base
            self.vor_stats(reset=True)
            self._stats_base["vor"] = {t: dict(vk["stats"][t]) for t in VOR_TYPES}
            self.vor_moments_set(vk["moments"])
        if hk is not None:
            self._rebase_stats("hypo", hk)
            sm = np.ascontiguousarray(hk["sum"], dtype=np.int64)
            sq = np.ascontiguousarray(hk["sq"], dtype=np.int64)
            assert sm.shape == (self.p.nevents, 3) and sq.shape == (self.p.nevents, 6)
            rc = self._L.mceik_mcmc_hypo_moments_set(self._h, int(hk["n"]), sm.ctypes.data_as(C.c_void_p),
                                                     sq.ctypes.data_as(C.c_void_p))
            if rc != 0:
                raise RuntimeError(f"mceik_mcmc_hypo_moments_set failed ({rc})")
        if nk is not None:
            self._rebase_stats("nuis", nk)
            self.nuis_moments_set(nk["moments"])

    # --- attempt / accept counters of the moves (mceik_mcmc_{temper,block,hypo,nuis}_stats) ---
    def _move_stats(self, name, n, reset, why=""):
        """(attempts, accepts) int64 [n] of move `name`: the library's counters
        plus those of a restored checkpoint (until a reset)."""
        att, acc = np.zeros(n, np.int64), np.zeros(n, np.int64)
        rc = getattr(self._L, f"mceik_mcmc_{name}_stats")(self._h, att.ctypes.data_as(C.c_void_p),
                                                          acc.ctypes.data_as(C.c_void_p), int(reset))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_{name}_stats failed ({rc}){why}")
        if name in self._stats_base:
            att, acc = att + self._stats_base[name][0], acc + self._stats_base[name][1]
        if reset:
            self._stats_base.pop(name, None)
        return att, acc

    def _rebase_stats(self, name, entry):
        """restore(): zero the library's counters of move `name`; the checkpoint's ride on as the base."""
        getattr(self, name + "_stats")(reset=True)
        self._stats_base[name] = tuple(np.asarray(entry[k], np.int64).copy() for k in ("attempts", "accepts"))

    # --- streaming posterior (include/mceik.h mceik_mcmc_posterior_*) ---
    def posterior_enable(self, per_chain=True, nbins=64):
        """Start (or reset) the streaming posterior: exact integer sums of v and
        v^2 per model entry over the kept steps of run() -- per chain (R-hat
        needs that; 16 bytes per chain and entry) or pooled over the chains --
        and a pooled histogram of `nbins` <= 128 bins over the prior range (0:
        none).  Works with max_samples = 0; the chains do not change."""
        o = _lib.PosteriorOpts(int(bool(per_chain)), int(nbins))
        rc = self._L.mceik_mcmc_posterior_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(f"mceik_mcmc_posterior_enable failed ({rc}): nbins in [0, 128]")
        self._post = (bool(per_chain), int(nbins))

    def posterior_disable(self):
        self._kept_clear(_KEPT["posterior"], "disable")

    def posterior_accumulate(self):
        """Add the chains' current state to the accumulators now (enqueued)."""
        self._kept_accumulate(_KEPT["posterior"])

    def posterior_raw(self):
        """The accumulators as host arrays: {"n": states per chain, "sum", "sumsq":
        int64 shaped like model_shape (per chain) or model_shape[1:] (pooled),
        "hist": uint32 model_shape[1:] + (nbins,), "per_chain", "nbins"}."""
        return self._kept_raw(_KEPT["posterior"])

    def _posterior_set(self, raw):
        d = _KEPT["posterior"]
        if not d.same(self._kept_on(d), raw):
            raise ValueError(d.mismatch)
        self._kept_set(d, raw)

    def posterior_partials(self):
        """The chain axis summed on the GPU into exact partials
        (`PosteriorPartials`): what ranks exchange and merge."""
        return self._kept_partials(_KEPT["posterior"])

    # --- the accumulators of kept states: one implementation over the rows of _KEPT ---
    def _kept_on(self, d):
        """The enabled options of accumulator `d`; RuntimeError while it is not enabled."""
        held = getattr(self, d.attr)
        if held is None:
            raise RuntimeError(d.not_enabled)
        return held

    def _kept_call(self, d, what, *args):
        return getattr(self._L, f"mceik_mcmc_{d.stem}_{what}")(self._h, *args)

    def _kept_disable(self, d):
        if self._kept_call(d, "disable") != 0:
            raise RuntimeError(f"mceik_mcmc_{d.stem}_disable failed")

    def _kept_clear(self, d, what="clear"):
        if self._kept_call(d, what) != 0:
            raise RuntimeError(f"mceik_mcmc_{d.stem}_{what} failed")
        setattr(self, d.attr, None)

    def _kept_accumulate(self, d):
        self._kept_on(d)
        rc = self._kept_call(d, "accumulate")
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_{d.stem}_accumulate failed ({rc})")

    @staticmethod
    def _kept_ptrs(d, arr):
        return [arr[k].ctypes.data_as(C.c_void_p) if k in arr else None for k in (d.slots or arr)]

    def _kept_raw(self, d):
        held = self._kept_on(d)
        out = {k: np.zeros(sh, dt) for k, (sh, dt) in d.arrays(self, held).items()}
        n = C.c_longlong(0)
        rc = self._kept_call(d, "get", C.byref(n), *self._kept_ptrs(d, out))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_{d.stem}_get failed ({rc})")
        out["n"] = n.value
        out.update(d.extra(held))
        return out

    def _kept_set(self, d, raw):
        table = d.arrays(self, self._kept_on(d))
        arr = {k: np.ascontiguousarray(raw[k], dtype=dt) for k, (sh, dt) in table.items()}
        assert all(arr[k].shape == sh for k, (sh, dt) in table.items())
        rc = self._kept_call(d, "set", int(raw["n"]), *self._kept_ptrs(d, arr))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_{d.stem}_set failed ({rc})")

    def _kept_partials(self, d):
        out = d.partials(self, self._kept_on(d))
        st = out._struct()
        rc = self._kept_call(d, "partials", C.byref(st))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_{d.stem}_partials failed ({rc})")
        out._took(st)
        return out

    # --- parallel tempering (include/mceik.h mceik_mcmc_temper_*) ---
    def temper_enable(self, betas=None, ntemps=None, tmax=None, swap_every=1):
        """Turn replica exchange on: pass the ladder `betas` (betas[0] == 1, non-
        increasing, > 0) or `ntemps` and `tmax` (the geometric ladder,
        `temper_ladder`).  nchains must be a multiple of the rungs; rung r of
        group g is local chain r * G + g, G = nchains / ntemps, so the cold
        chains are `cold_chains`.  Before every step gs > 0 with gs %
        swap_every == 0 neighbouring rungs try to swap states (0: never; see
        `temper_swap`).  Resets the swap counters."""
        if (betas is None) == (ntemps is None or tmax is None):
            raise ValueError("temper_enable: pass either betas or ntemps and tmax")
        b = temper_ladder(ntemps, tmax) if betas is None else np.ascontiguousarray(betas, dtype=np.float64).ravel()
        o = _lib.TemperOpts(len(b), int(swap_every), b.ctypes.data)
        rc = self._L.mceik_mcmc_temper_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_temper_enable failed ({rc}): nchains % ntemps == 0, betas[0] == 1, 0 < betas[r+1] <= "
                "betas[r], swap_every >= 0, and no states in an enabled posterior")
        self._temper = (b.copy(), int(swap_every))
        self._stats_base.pop("temper", None)

    def temper_disable(self):
        rc = self._L.mceik_mcmc_temper_disable(self._h)
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(f"mceik_mcmc_temper_disable failed ({rc})")
        self._temper = None
        self._stats_base.pop("temper", None)

    def _temper_on(self):
        if self._temper is None:
            raise RuntimeError("tempering is not enabled (Sampler.temper_enable)")
        return self._temper

    @property
    def cold_chains(self):
        """Local indices of the cold chains (beta = 1): range(0, G); every chain while tempering is off."""
        return range(self.nchains // (len(self._temper[0]) if self._temper is not None else 1))

    def temper_stats(self, reset=False):
        """(attempts, accepts) int64 [ntemps - 1]: swap rounds per rung pair (r, r + 1)."""
        return self._move_stats("temper", len(self._temper_on()[0]) - 1, reset)

    def temper_swap(self, parity):
        """One swap round now (enqueued): rungs r, r + 1 with r % 2 == parity, drawn at the current step."""
        self._temper_on()
        rc = self._L.mceik_mcmc_temper_swap(self._h, int(parity))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(f"mceik_mcmc_temper_swap failed ({rc}): parity 0 or 1")

    # --- block proposals (include/mceik.h mceik_mcmc_block_*) ---
    def block_enable(self, rmin=0, rmax=2):
        """Turn multi-cell proposals on: every step draws a radius R in [rmin,
        rmax] (inversion cells, 0 <= rmin <= rmax <= 8) beside the single-cell
        draw and moves the cells within R of the centre by the magnitude
        scaled with a separable triangular weight (`block_footprint`).  R = 0
        is the single-cell proposal.  Every step is then one launch (`info()
        ["multi_step"]` is False until `block_disable`).  Resets the counters."""
        o = _lib.BlockOpts(int(rmin), int(rmax))
        rc = self._L.mceik_mcmc_block_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_block_enable failed ({rc}): 0 <= rmin <= rmax <= 8")
        self._block = (int(rmin), int(rmax))
        self._stats_base.pop("block", None)

    def block_disable(self):
        if self._L.mceik_mcmc_block_disable(self._h) != 0:
            raise RuntimeError("mceik_mcmc_block_disable failed")
        self._block = None
        self._stats_base.pop("block", None)

    def block_stats(self, reset=False):
        """(attempts, accepts) int64 [rmax + 1]: proposals and accepted proposals by radius."""
        if self._block is None:
            raise RuntimeError("block proposals are not enabled (Sampler.block_enable)")
        return self._move_stats("block", self._block[1] + 1, reset)

    # --- discrete Langevin moves (include/mceik.h mceik_mcmc_lang_*) ---
    def lang_enable(self, every, offset=0, sigma=8.0, dmax=16, mem_bytes=None):
        """Turn gradient-informed moves on: global step gs with gs % every ==
        offset (and neither a hypocentre nor a nuisance step) moves every cell
        of one phase model of a chain at once, cell i by an integer in [-dmax,
        dmax] drawn from q_i(delta) ~ exp(0.5 d_i delta - delta^2 / (2 sigma^2))
        inside the box, d_i the exact gradient of the chain's log posterior
        (DESIGN.md s.18), with the Hastings term of the reverse move in the
        accept test.  A step costs two forwards with fields and two adjoint
        batches; `mem_bytes` (None: 2 GiB) bounds the fields and workspaces it
        holds, the chains run in chunks that fit.  Every step is then one
        launch (`info()["multi_step"]` is False until `lang_disable`).  Resets
        the counters."""
        o = _lib.LangOpts(int(every), int(offset), float(sigma), int(dmax), 0 if mem_bytes is None else int(mem_bytes))
        rc = self._L.mceik_mcmc_lang_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_lang_enable failed ({rc}): every > 0, 0 <= offset < every, sigma > 0, 1 <= dmax <= "
                f"{_lib.LANG_DMAX_CAP}, mem_bytes large enough for one chain")
        self._lang = True

    def lang_disable(self):
        if self._L.mceik_mcmc_lang_disable(self._h) != 0:
            raise RuntimeError("mceik_mcmc_lang_disable failed")

    def _lang_held(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): Langevin moves were never enabled (Sampler.lang_enable)")

    def lang_options(self):
        """The options in force (every = 0 after `lang_disable`) and "chunk": the
        chains per chunk of every pipe."""
        o = _lib.LangOpts()
        chunk = np.zeros(4, np.int32)
        self._lang_held(self._L.mceik_mcmc_lang_get(self._h, C.byref(o), chunk.ctypes.data_as(C.c_void_p)),
                        "mceik_mcmc_lang_get")
        return {"every": o.every, "offset": o.offset, "sigma": o.sigma, "dmax": o.dmax, "mem_bytes": o.mem_bytes,
                "chunk": [int(x) for x in chunk[:self.info()["npipe"]]]}

    def lang_stats(self, reset=False):
        """{"attempts", "accepts", "failed", "moved"} over the chains: Langevin
        steps tried, accepted, failed (a solve of the step did not converge),
        and cells that changed in the accepted steps."""
        t = [C.c_longlong(0) for _ in range(4)]
        self._lang_held(self._L.mceik_mcmc_lang_stats(self._h, *[C.byref(x) for x in t], int(reset)),
                        "mceik_mcmc_lang_stats")
        return dict(zip(("attempts", "accepts", "failed", "moved"), (int(x.value) for x in t)))

    def lang_last(self):
        """The last Langevin step: {"phase" int32 [nchains], "delta" int32
        [nchains, ncell] (the move of that phase's model, accepted or not),
        "lqf", "lqr", "logl_prop" float64 [nchains], "accept" uint8 [nchains],
        "status" int32 [nchains] (1: failed)}."""
        nch, nc = self.nchains, self.p.ncell
        out = {"phase": np.zeros(nch, np.int32), "delta": np.zeros((nch, nc), np.int32), "lqf": np.zeros(nch),
               "lqr": np.zeros(nch), "logl_prop": np.zeros(nch), "accept": np.zeros(nch, np.uint8),
               "status": np.zeros(nch, np.int32)}
        self._lang_held(self._L.mceik_mcmc_lang_last(self._h, *[a.ctypes.data_as(C.c_void_p) for a in out.values()]),
                        "mceik_mcmc_lang_last")
        return out

    # --- differential-evolution moves (include/mceik.h mceik_mcmc_de_*) ---
    def de_enable(self, every, offset=0, gamma=None, cr=1.0):
        """Turn differential-evolution (population) moves on: global step gs
        with gs % every == offset (and neither a hypocentre, a nuisance nor a
        Langevin step) proposes v + gamma (v_a - v_b) on one phase model of
        half the chains of every population -- a chain's temperature rung on
        this sampler -- from two chains a, b of the other half, which stands
        still on that step; each cell takes part with probability `cr`
        (DESIGN.md s.21).  The move is symmetric, costs one forward per moving
        chain, and is rejected whole when a cell would leave the box.  gamma
        and cr are rounded to units of 1 / 65536 (`de_options`).  gamma=None:
        2.38 / sqrt(2 cr ncell), the usual DE-MC scale for the cr * ncell cells
        that move, clipped to a representable value; how good that default is
        for this posterior has not been measured.  A population needs 4
        chains.  Every step is then one launch (`info()["multi_step"]` is
        False until `de_disable`).  Resets the counters."""
        cr = float(cr)
        if not (0.0 < cr <= 1.0):
            raise ValueError("de_enable: 0 < cr <= 1")
        if gamma is None:
            gamma = min(2.38 / np.sqrt(2.0 * cr * self.p.ncell), 2.0)
        gamma = float(gamma)
        if not (0.0 < gamma <= 2.0):
            raise ValueError("de_enable: 0 < gamma <= 2")
        gq = min(max(int(round(gamma * 65536.0)), 1), DE_GQ_MAX)
        crq = min(max(int(round(cr * 65536.0)), 1), DE_CRQ_MAX)
        o = _lib.DeOpts(int(every), int(offset), gq, crq)
        rc = self._L.mceik_mcmc_de_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_de_enable failed ({rc}): every >= 1, 0 <= offset < every, and 4 chains per population "
                "(temperature rung)")
        self._de = (int(every), int(offset), gq, crq)
        self._stats_base.pop("de", None)

    def de_disable(self):
        if self._L.mceik_mcmc_de_disable(self._h) != 0:
            raise RuntimeError("mceik_mcmc_de_disable failed")
        self._de = None
        self._stats_base.pop("de", None)

    def _de_held(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): DE moves were never enabled (Sampler.de_enable)")

    def de_options(self):
        """The options in force (every = 0 after `de_disable`): every, offset,
        gamma_q16, cr_q16 and the gamma and cr they stand for."""
        o = _lib.DeOpts()
        self._de_held(self._L.mceik_mcmc_de_get(self._h, C.byref(o)), "mceik_mcmc_de_get")
        return {"every": o.every, "offset": o.offset, "gamma_q16": o.gamma_q16, "cr_q16": o.cr_q16,
                "gamma": o.gamma_q16 / 65536.0, "cr": o.cr_q16 / 65536.0}

    def de_stats(self, reset=False):
        """{"attempts", "accepts", "outbox", "failed", "moved"} over the chains:
        DE moves tried, accepted, rejected because a cell left the box, failed
        (a solve of the move did not converge), and cells that changed in the
        accepted moves; plus those of a restored checkpoint (until a reset)."""
        t = [C.c_longlong(0) for _ in range(5)]
        self._de_held(self._L.mceik_mcmc_de_stats(self._h, *[C.byref(x) for x in t], int(reset)), "mceik_mcmc_de_stats")
        out = dict(zip(_DE_COUNTERS, (int(x.value) for x in t)))
        base = self._stats_base.get("de")
        if base is not None:
            out = {k: out[k] + base[k] for k in out}
        if reset:
            self._stats_base.pop("de", None)
        return out

    def de_last(self):
        """The last DE step: {"mover" int32 [nchains] (1: the chain moved), "a",
        "b" int32 [nchains] (the partners as local chains, -1 for standing
        chains), "phase" (-1: none yet), "nmove" int32 [nchains] (cells that the
        proposal changed), "inbox", "status" int32 [nchains] (1: failed),
        "logl_prop" float64 [nchains] (logL where the move left the box or
        failed, 0 for standing chains), "accept" uint8 [nchains]}.  After a DE
        step `last()` reports accept = 0 for the standing chains and only the
        movers' table rows are the step's; `last_phase()` is the step's phase
        for every chain."""
        nch = self.nchains
        i32 = lambda: np.zeros(nch, np.int32)  # noqa: E731
        out = {"mover": i32(), "a": i32(), "b": i32(), "phase": np.zeros(1, np.int32), "nmove": i32(), "inbox": i32(),
               "status": i32(), "logl_prop": np.zeros(nch), "accept": np.zeros(nch, np.uint8)}
        self._de_held(self._L.mceik_mcmc_de_last(self._h, *[a.ctypes.data_as(C.c_void_p) for a in out.values()]),
                      "mceik_mcmc_de_last")
        out["phase"] = int(out["phase"][0])
        return out

    # --- transdimensional Voronoi-cell models (include/mceik.h mceik_mcmc_vor_*) ---
    def _vor_nuclei(self, cells, vals, counts, kmax):
        shape = (self.nchains, max(1, self.p.nphase), kmax)
        c, w, k = _i32(cells), _i32(vals), _i32(counts)
        if c.size != np.prod(shape) or w.size != c.size or k.size != shape[0] * shape[1]:
            raise ValueError(f"nuclei: cells and vals {shape}, counts {shape[:2]}")
        return c.reshape(shape), w.reshape(shape), k.reshape(shape[:2])

    def vor_enable(self, kmin=1, kmax=64, k0=None, dv=None, dmax=(1, 1, 1), metric=(1, 1, 1), nuclei=None):
        """Turn transdimensional Voronoi-cell models on: each phase model of
        each chain becomes kmin <= k <= kmax (<= VOR_KMAX) nuclei (cell, value)
        in distinct cells, v is their raster (`vor_raster`), and every step that
        would propose a single cell draws one of four moves of one phase's
        nuclei instead -- value (+-[1, dv], default the problem's dvmax), move
        (up to dmax cells per axis), birth (a free cell, its value from the
        prior), death -- accepted iff log u < beta (logL' - logL): with a
        uniform prior on k, on the cells and on the values no Hastings factor
        remains.  nuclei = (cells, vals [nchains, nphase,
        kmax], counts [nchains, nphase]) starts from the caller's; otherwise k0
        (default kmin) distinct cells are drawn per chain and phase, each with
        the chain's current v of its cell.  The models are rastered and every
        logL recomputed with one forward.  Refused while block proposals, the
        smoothness prior, Langevin or DE moves are on, which in turn refuse
        while this is on.  Every step is then one launch
        (`info()["multi_step"]` is False until `vor_disable`).  Resets the
        counters."""
        o = _lib.VorOpts()
        o.kmin, o.kmax, o.dv = int(kmin), int(kmax), int(self.p.dvmax if dv is None else dv)
        o.k0 = int(kmin if k0 is None else k0)
        dm, me = tuple(int(x) for x in dmax), tuple(int(x) for x in metric)
        if len(dm) != 3 or len(me) != 3:
            raise ValueError("vor_enable: dmax and metric have three entries")
        o.dmax[:], o.metric[:] = dm, me
        ptr = [None, None, None]
        if nuclei is not None:
            if not 1 <= o.kmax <= VOR_KMAX:
                raise ValueError(f"vor_enable: 1 <= kmax <= {VOR_KMAX}")
            keep = self._vor_nuclei(*nuclei, o.kmax)
            ptr = [a.ctypes.data_as(C.c_void_p) for a in keep]
        rc = self._L.mceik_mcmc_vor_enable(self._h, C.byref(o), *ptr)
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_vor_enable failed ({rc}): 1 <= kmin <= k0 <= kmax <= min({VOR_KMAX}, ncell), dv >= 1, valid "
                "nuclei, and neither block proposals, the prior, Langevin nor DE moves on")
        self._vor = (o.kmin, o.kmax, o.dv, dm, me)
        self._stats_base.pop("vor", None)
        self._last_full = True

    def vor_disable(self):
        """Later steps propose single cells again, from v as it stands."""
        if self._L.mceik_mcmc_vor_disable(self._h) != 0:
            raise RuntimeError("mceik_mcmc_vor_disable failed")
        self._vor = None
        self._stats_base.pop("vor", None)

    def _vor_held(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): Voronoi-cell models were never enabled (Sampler.vor_enable)")

    def vor_options(self):
        """The options in force: kmin, kmax, k0 (0 when the caller gave the nuclei), dv, dmax, metric, on."""
        o, on = _lib.VorOpts(), C.c_int(0)
        self._vor_held(self._L.mceik_mcmc_vor_get(self._h, C.byref(o), C.byref(on), None, None, None), "mceik_mcmc_vor_get")
        return {"kmin": o.kmin, "kmax": o.kmax, "k0": o.k0, "dv": o.dv, "dmax": tuple(o.dmax), "metric": tuple(o.metric),
                "on": bool(on.value)}

    def vor_get(self):
        """(cells, vals int32 [nchains, nphase, kmax], counts int32 [nchains,
        nphase]): the nuclei; slots from a model's count on mean nothing."""
        kmax = self.vor_options()["kmax"]
        shape = (self.nchains, max(1, self.p.nphase), kmax)
        c, w, k = np.zeros(shape, np.int32), np.zeros(shape, np.int32), np.zeros(shape[:2], np.int32)
        self._vor_held(self._L.mceik_mcmc_vor_get(self._h, None, None, *[a.ctypes.data_as(C.c_void_p) for a in (c, w, k)]),
                       "mceik_mcmc_vor_get")
        return c, w, k

    def vor_set(self, cells, vals, counts, recompute_logl=True):
        """Replace the nuclei (validated: counts in [kmin, kmax], distinct cells,
        values in the box), raster them and recompute every logL."""
        if self._vor is None:
            raise RuntimeError("vor_set: Voronoi-cell models are off")
        keep = self._vor_nuclei(cells, vals, counts, self._vor[1])
        rc = self._L.mceik_mcmc_vor_set(self._h, *[a.ctypes.data_as(C.c_void_p) for a in keep], int(bool(recompute_logl)))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(f"mceik_mcmc_vor_set failed ({rc}): invalid nuclei")
        if recompute_logl:
            self._last_full = True

    def vor_rasterize(self):
        """Queue the raster of every model from its nuclei on the sampler's
        stream, without a synchronise (mceik_mcmc_vor_rasterize).  v is that
        raster already: this is for timing the kernel (tools/vor_cost.py)."""
        if self._L.mceik_mcmc_vor_rasterize(self._h) != 0:
            raise RuntimeError("mceik_mcmc_vor_rasterize failed: Voronoi-cell models are off")

    def vor_stats(self, reset=False):
        """{move type: {"attempts", "accepts", "reason1", "reason2", "reason3"}}
        over the chains; the reasons count moves rejected before their forward
        -- value: 1 left the box; move: 1 zero displacement, 2 outside the grid,
        3 occupied; birth: 1 k == kmax; death: 1 k == kmin -- plus those of a
        restored checkpoint (until a reset)."""
        t = np.zeros((4, 5), np.int64)
        self._vor_held(self._L.mceik_mcmc_vor_stats(self._h, t.ctypes.data_as(C.c_void_p), int(reset)),
                       "mceik_mcmc_vor_stats")
        out = {n: dict(zip(VOR_COUNTERS, (int(x) for x in t[i]))) for i, n in enumerate(VOR_TYPES)}
        base = self._stats_base.get("vor")
        if base is not None:
            out = {n: {k: out[n][k] + int(base[n][k]) for k in VOR_COUNTERS} for n in VOR_TYPES}
        if reset:
            self._stats_base.pop("vor", None)
        return out

    def vor_last(self):
        """The last Voronoi step: {"phase" (-1: none yet), "type", "reason" (0:
        not rejected before the forward), "j", "cell", "value" (the changed
        nucleus as proposed), "k" (the proposed count) int32 [nchains],
        "cells", "vals" int32 [nchains, kmax] (the proposed nuclei: the first
        k), "vprop" int32 [nchains, ncell] (their raster), "logu", "logl_prop" float64 [nchains] (logL where rejected before
        the forward), "accept" uint8 [nchains]}."""
        nch, kmax = self.nchains, self.vor_options()["kmax"]
        ph, rec = C.c_int(-1), np.zeros((nch, 8), np.int32)
        pc, pw = np.zeros((nch, kmax), np.int32), np.zeros((nch, kmax), np.int32)
        vp = np.zeros((nch, self.p.ncell), np.int32)
        lu, lp, acc = np.zeros(nch), np.zeros(nch), np.zeros(nch, np.uint8)
        self._vor_held(self._L.mceik_mcmc_vor_last(self._h, C.byref(ph), *[a.ctypes.data_as(C.c_void_p)
                                                                          for a in (rec, pc, pw, vp, lu, lp, acc)]),
                       "mceik_mcmc_vor_last")
        out = {"phase": ph.value}
        for i, n in enumerate(("type", "reason", "j", "cell", "value", "k")):
            out[n] = rec[:, i].copy()
        out.update(cells=pc, vals=pw, vprop=vp, logu=lu, logl_prop=lp, accept=acc)
        return out

    def vor_moments(self):
        """{"n", "hist" uint64 [nphase, kmax + 1], "dens" uint64 [nphase,
        ncell]}: exact sums over the cold chains of the kept steps -- states by
        k, and states with a nucleus in each cell.  They merge by addition."""
        nph, kmax = max(1, self.p.nphase), self.vor_options()["kmax"]
        n, hist, dens = C.c_longlong(0), np.zeros((nph, kmax + 1), np.uint64), np.zeros((nph, self.p.ncell), np.uint64)
        self._vor_held(self._L.mceik_mcmc_vor_moments(self._h, C.byref(n), hist.ctypes.data_as(C.c_void_p),
                                                      dens.ctypes.data_as(C.c_void_p)), "mceik_mcmc_vor_moments")
        return {"n": int(n.value), "hist": hist, "dens": dens}

    def vor_moments_set(self, m):
        hist = np.ascontiguousarray(m["hist"], dtype=np.uint64)
        dens = np.ascontiguousarray(m["dens"], dtype=np.uint64)
        nph, kmax = max(1, self.p.nphase), self.vor_options()["kmax"]
        if hist.shape != (nph, kmax + 1) or dens.shape != (nph, self.p.ncell):
            raise ValueError("vor_moments_set: hist [nphase, kmax + 1], dens [nphase, ncell]")
        self._vor_held(self._L.mceik_mcmc_vor_moments_set(self._h, int(m["n"]), hist.ctypes.data_as(C.c_void_p),
                                                          dens.ctypes.data_as(C.c_void_p)), "mceik_mcmc_vor_moments_set")

    def vor_summary(self, moments=None):
        """{"n", "k_posterior" float64 [nphase, kmax + 1] (the kept states'
        share by k), "k_mean" [nphase], "acceptance" {move type: accepts /
        attempts}, "density" float64 [nphase, ncell] (the share of kept states
        with a nucleus in the cell)} from `vor_moments()` (or merged ones)."""
        m = self.vor_moments() if moments is None else moments
        n = max(int(m["n"]), 1)
        kp = np.asarray(m["hist"], np.float64) / n
        st = self.vor_stats()
        return {"n": int(m["n"]), "k_posterior": kp, "k_mean": kp @ np.arange(kp.shape[1], dtype=np.float64),
                "acceptance": {t: st[t]["accepts"] / max(st[t]["attempts"], 1) for t in VOR_TYPES},
                "density": np.asarray(m["dens"], np.float64) / n}

    # --- smoothness / reference-model prior (include/mceik.h mceik_mcmc_prior_*) ---
    def prior_enable(self, sigma_smooth=None, sigma_damp=None, vref=None):
        """Turn the smoothness and reference-model prior on: log prior =
        -(ws Es + wd Ed) per phase model beside the uniform box, Es the sum of
        (v_i - v_j)^2 over face-adjacent cells, Ed the sum of (v_i - vref_i)^2
        (`prior_energy`), w = 1 / (2 sigma^2).  Sigmas in m/s: a scalar or a
        (P, S) pair, None = weight 0.  `vref`: one model shaped like a chain's
        (model_shape[1:]), shared by the chains; damping needs it.  Every step
        is then one launch (`info()["multi_step"]` is False until
        `prior_disable`)."""
        ws, wd = prior_weight(sigma_smooth), prior_weight(sigma_damp)
        if vref is None and any(wd):
            raise ValueError("prior_enable: sigma_damp needs a reference model vref")
        o = _lib.PriorOpts()
        o.w_smooth[0], o.w_smooth[1] = ws
        o.w_damp[0], o.w_damp[1] = wd
        r, digest = None, None
        if vref is not None:
            r = np.ascontiguousarray(vref, dtype=np.int32)
            if r.shape != self.model_shape[1:]:
                raise ValueError(f"prior_enable: vref shaped {self.model_shape[1:]}, not {r.shape}")
            o.vref = r.ctypes.data
            digest = hashlib.sha256(r.tobytes()).hexdigest()
        rc = self._L.mceik_mcmc_prior_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_prior_enable failed ({rc}): finite weights >= 0, vref inside the box, 3 ncell (hi - lo + "
                "2 dvmax)^2 < 2^53, and no states in an enabled posterior")
        self._prior = (ws, wd, digest)

    def prior_disable(self):
        rc = self._L.mceik_mcmc_prior_disable(self._h)
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(f"mceik_mcmc_prior_disable failed ({rc})")
        self._prior = None

    def _prior_on(self):
        if self._prior is None:
            raise RuntimeError("the prior is not enabled (Sampler.prior_enable)")
        return self._prior

    def prior_energy(self):
        """(Es, Ed) int64 [nchains, nphase]: the energies of every chain's current
        models, summed on the GPU."""
        self._prior_on()
        es, ed = (np.zeros((self.nchains, self.p.nphase), np.int64) for _ in range(2))
        rc = self._L.mceik_mcmc_prior_energy(self._h, es.ctypes.data_as(C.c_void_p), ed.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_prior_energy failed ({rc})")
        return es, ed

    def prior_last(self):
        """int64 [nchains, 2]: (dEs, dEd) of every chain's proposal of the last
        step, accepted or not; zeros for a proposal outside the box."""
        self._prior_on()
        de = np.zeros((self.nchains, 2), np.int64)
        rc = self._L.mceik_mcmc_prior_last(self._h, de.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_prior_last failed ({rc})")
        return de

    # --- hypocentre moves (include/mceik.h mceik_mcmc_hypo_*) ---
    def hypo_enable(self, every, dmax=(1, 1, 1), box=None):
        """Sample the event hypocentres with the velocity models: every chain
        carries a node (ix, iy, iz) per event, which starts at the catalogue's
        snapped node at the first enable.  With every = K > 0 global step gs is
        a hypocentre step iff gs % K == K - 1: instead of a velocity proposal
        every event of every chain draws a move of up to `dmax` nodes per axis
        and accepts or rejects it on its own (one forward of the chain's
        current models serves them all).  `box` = (lo, hi), two node triples
        (inclusive), bounds the positions; None is the whole grid.  Every step
        is then one launch (`info()["multi_step"]` is False until
        `hypo_disable`).  Resets the counters and the moments."""
        p = self.p
        lo, hi = ((0, 0, 0), (p.nx - 1, p.ny - 1, p.nz - 1)) if box is None else box
        dm, lo, hi = (tuple(int(x) for x in np.ravel(a)) for a in (dmax, lo, hi))
        if not (len(dm) == len(lo) == len(hi) == 3):
            raise ValueError("hypo_enable: dmax and the box corners are one value per axis")
        o = _lib.HypoOpts()
        o.every = int(every)
        for a in range(3):
            o.dmax[a], o.lo[a], o.hi[a] = dm[a], lo[a], hi[a]
        rc = self._L.mceik_mcmc_hypo_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_hypo_enable failed ({rc}): every >= 0, dmax >= 0, a box lo <= hi inside the grid that holds "
                "every chain's positions, tt_interp = 0, and no states in an enabled posterior")
        self._hypo = (int(every), dm, lo, hi)
        self._stats_base.pop("hypo", None)

    def hypo_disable(self):
        """Later steps are velocity steps again; the positions stay where they are, per chain."""
        if self._L.mceik_mcmc_hypo_disable(self._h) != 0:
            raise RuntimeError("mceik_mcmc_hypo_disable failed")
        self._hypo = None
        self._stats_base.pop("hypo", None)

    def hypo_positions(self):
        """int32 [nchains, nev, 3]: every chain's node (ix, iy, iz) per event (after a first `hypo_enable`)."""
        xyz = np.empty((self.nchains, self.p.nevents, 3), np.int32)
        rc = self._L.mceik_mcmc_hypo_get(self._h, None, xyz.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_hypo_get failed ({rc}): hypocentre moves were never enabled")
        return xyz

    def hypo_set(self, xyz):
        """Replace the positions (int [nchains, nev, 3], inside the grid, inside
        the box while enabled); one full forward recomputes logL."""
        xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        if xyz.shape != (self.nchains, self.p.nevents, 3):
            raise ValueError(f"hypo_set: positions shaped {(self.nchains, self.p.nevents, 3)}, not {xyz.shape}")
        rc = self._L.mceik_mcmc_hypo_set(self._h, xyz.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_hypo_set failed ({rc}): after a first hypo_enable, positions inside the grid / the box")
        self._last_full = True

    def hypo_stats(self, reset=False):
        """(attempts, accepts) int64 [nev]: moves tried and accepted per event, over the chains."""
        return self._move_stats("hypo", self.p.nevents, reset)

    def hypo_last(self):
        """The last hypocentre step: (cand int32 [nchains, nev, 3] = current + d,
        accept uint8 [nchains, nev], obj float64 [nchains, nev, 2] = objfn at the
        current and at the candidate node)."""
        nch, nev = self.nchains, self.p.nevents
        cand, acc, obj = np.zeros((nch, nev, 3), np.int32), np.zeros((nch, nev), np.uint8), np.zeros((nch, nev, 2))
        rc = self._L.mceik_mcmc_hypo_last(self._h, cand.ctypes.data_as(C.c_void_p), acc.ctypes.data_as(C.c_void_p),
                                          obj.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_hypo_last failed ({rc})")
        return cand, acc, obj

    def _hypo_moments(self):
        """(n, sum int64 [nev, 3], sq int64 [nev, 6]): the exact moments of the cold chains' kept positions."""
        nev = self.p.nevents
        n, sm, sq = C.c_longlong(0), np.zeros((nev, 3), np.int64), np.zeros((nev, 6), np.int64)
        rc = self._L.mceik_mcmc_hypo_moments_get(self._h, C.byref(n), sm.ctypes.data_as(C.c_void_p),
                                                 sq.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_hypo_moments_get failed ({rc})")
        return n.value, sm, sq

    def hypo_moments(self):
        """{"n", "sum" [nev, 3], "sq" [nev, 6] = (xx, yy, zz, xy, xz, yz)}: exact
        int64 sums of the cold chains' positions (nodes) over the kept steps
        since `hypo_enable`; ranks merge them by addition."""
        n, sm, sq = self._hypo_moments()
        return {"n": n, "sum": sm, "sq": sq}

    def hypo_summary(self, moments=None):
        """(mean [nev, 3] in metres = origin + h * mean node, cov [nev, 3, 3] in
        m^2) of every event's location over the cold chains' kept states, from
        the moments (this sampler's, or merged ones); NaN without states."""
        m = self.hypo_moments() if moments is None else moments
        n = int(m["n"])
        p = self.p
        sm, sq = np.asarray(m["sum"], np.float64), np.asarray(m["sq"], np.float64)
        if n <= 0:
            return np.full((p.nevents, 3), np.nan), np.full((p.nevents, 3, 3), np.nan)
        mu = sm / n
        second = np.empty((p.nevents, 3, 3))
        for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            second[:, a, b] = second[:, b, a] = sq[:, k] / n
        cov = (second - mu[:, :, None] * mu[:, None, :]) * (p.h * p.h)
        return np.array([p.x0, p.y0, p.z0]) + p.h * mu, cov

    # --- noise scale and station statics (include/mceik.h mceik_mcmc_nuis_*) ---
    def nuis_enable(self, every, offset=0, nsub=16, ladder=None, dk=1, statics_dt=None, dc=1, kcmax=0, norm=None):
        """Sample the noise scale and / or the station statics with the velocity
        models.  `ladder` = (lam, lnlam) from `nuis_ladder`
        turns the noise part on: every chain scales var of phase ph by
        lam[kn[ph]], a move is +-[1, max(dk, 1)] ladder entries.  `statics_dt`
        (seconds) turns the statics part on: every chain adds kc * statics_dt
        to the static of each (phase, station), |kc| <= kcmax, a move shifts a
        zero-sum pair of stations by +-[1, max(dc, 1)] units.  Global step gs
        is a nuisance step iff gs % every == offset: `nsub` sub-moves per chain
        from the tables the chain holds, no eikonal solve.  `norm` [nphase]
        weighs the noise normalisation (None: the used picks per phase).  The
        values start at lam = 1 and kc = 0, where every logL is the plain
        sampler's; they stay across `nuis_disable` and a second enable, until
        `nuis_clear`.  While they are held every step is one launch
        (`info()["multi_step"]` is False).  Resets the counters and the moments."""
        p = self.p
        o = _lib.NuisOpts()
        o.every, o.offset, o.nsub = int(every), int(offset), int(nsub)
        o.noise, o.statics = int(ladder is not None), int(statics_dt is not None)
        keep = []
        lam = lnlam = None
        if ladder is not None:
            lam, lnlam = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in ladder)
            if lam.size != lnlam.size:
                raise ValueError("nuis_enable: lam and lnlam are one ladder")
            o.nk, o.lam, o.lnlam = lam.size, lam.ctypes.data, lnlam.ctypes.data
            keep += [lam, lnlam]
        o.dk, o.dc, o.kcmax = int(dk), int(dc), int(kcmax)
        o.dt = float(statics_dt) if statics_dt is not None else 0.0
        if norm is not None:
            nm = np.ascontiguousarray(norm, dtype=np.float64).ravel()
            if nm.size != p.nphase:
                raise ValueError("nuis_enable: norm is one weight per phase")
            o.norm = nm.ctypes.data
            keep.append(nm)
        rc = self._L.mceik_mcmc_nuis_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_nuis_enable failed ({rc}): a ladder or statics_dt > 0, every > 0, 0 <= offset < every, "
                "nsub > 0, an odd ladder with the middle entry (1, 0), dk, dc, kcmax >= 0, something to move, held "
                "values that fit, and no states in an enabled posterior")
        self._nuis = {"every": int(every), "offset": int(offset), "nsub": int(nsub), "dk": int(dk), "dc": int(dc),
                      "kcmax": int(kcmax) if statics_dt is not None else None,
                      "dt": float(statics_dt) if statics_dt is not None else None,
                      "lam": None if lam is None else lam.copy(), "lnlam": None if lnlam is None else lnlam.copy(),
                      "norm": None if norm is None else nm.copy()}
        self._stats_base.pop("nuis", None)
        self._last_full = True

    def nuis_disable(self):
        """Later steps are velocity (and hypocentre) steps again; the values stay
        and every logL keeps honouring them."""
        if self._L.mceik_mcmc_nuis_disable(self._h) != 0:
            raise RuntimeError("mceik_mcmc_nuis_disable failed")
        if self._nuis is not None:
            self._nuis = dict(self._nuis, every=0)

    def nuis_clear(self):
        """Every chain back to lam = 1 and kc = 0, logL recomputed: the plain
        sampler again, multi-step launches included."""
        rc = self._L.mceik_mcmc_nuis_clear(self._h)
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(f"mceik_mcmc_nuis_clear failed ({rc})")
        self._nuis = None
        self._stats_base.pop("nuis", None)
        self._last_full = True

    def _nuis_held(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): the sampler holds no noise / statics values (nuis_enable)")

    def nuis_get(self):
        """(kn int32 [nchains, nphase], kc int32 [nchains, nphase, nstat]): every
        chain's ladder index per phase and static per (phase, station) in units."""
        p = self.p
        kn, kc = np.empty((self.nchains, p.nphase), np.int32), np.empty((self.nchains, p.nphase, p.nstat), np.int32)
        self._nuis_held(self._L.mceik_mcmc_nuis_get(self._h, None, None, None, None, kn.ctypes.data_as(C.c_void_p),
                                                    kc.ctypes.data_as(C.c_void_p)), "mceik_mcmc_nuis_get")
        return kn, kc

    def nuis_options(self):
        """The options in force as the library holds them: a dict with the
        ladder, norm and every (0 after `nuis_disable`)."""
        o = _lib.NuisOpts()
        self._nuis_held(self._L.mceik_mcmc_nuis_get(self._h, C.byref(o), None, None, None, None, None),
                        "mceik_mcmc_nuis_get")
        lam, lnlam, norm = np.empty(o.nk), np.empty(o.nk), np.empty(self.p.nphase)
        self._L.mceik_mcmc_nuis_get(self._h, None, lam.ctypes.data_as(C.c_void_p), lnlam.ctypes.data_as(C.c_void_p),
                                    norm.ctypes.data_as(C.c_void_p), None, None)
        return {"every": o.every, "offset": o.offset, "nsub": o.nsub, "noise": bool(o.noise), "statics": bool(o.statics),
                "dk": o.dk, "dc": o.dc, "kcmax": o.kcmax, "dt": o.dt, "lam": lam, "lnlam": lnlam, "norm": norm}

    def nuis_set(self, kn, kc):
        """Replace the values (indices inside the ladder, |kc| <= kcmax); logL is
        recomputed from the tables the sampler holds, without an eikonal solve."""
        p = self.p
        kn, kc = np.ascontiguousarray(kn, dtype=np.int32), np.ascontiguousarray(kc, dtype=np.int32)
        if kn.shape != (self.nchains, p.nphase) or kc.shape != (self.nchains, p.nphase, p.nstat):
            raise ValueError(f"nuis_set: kn {(self.nchains, p.nphase)} and kc {(self.nchains, p.nphase, p.nstat)}")
        rc = self._L.mceik_mcmc_nuis_set(self._h, kn.ctypes.data_as(C.c_void_p), kc.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_nuis_set failed ({rc}): after nuis_enable, indices inside the ladder, statics inside the box")

    def nuis_stats(self, reset=False):
        """(attempts, accepts) int64 [nphase + nphase * nstat] over the chains:
        entry ph the noise index of phase ph, entry nphase + ph * nstat + k the
        static of station k (a pair counts on both its stations)."""
        return self._move_stats("nuis", self.p.nphase * (1 + self.p.nstat), reset,
                                ": the sampler holds no noise / statics values (nuis_enable)")

    def nuis_last(self):
        """The last nuisance step, per chain and sub-move: (rec int32 [nchains,
        nsub, 4] = parameter (numbered as in `nuis_stats`), partner parameter
        (-1: a noise move), the parameter's candidate value, accepted; logl
        float64 [nchains, nsub, 2] = logL before the sub-move, logL' of the
        candidate (outside its box: logL))."""
        nsub = self.nuis_options()["nsub"]
        rec, logl = np.zeros((self.nchains, nsub, 4), np.int32), np.zeros((self.nchains, nsub, 2))
        self._nuis_held(self._L.mceik_mcmc_nuis_last(self._h, rec.ctypes.data_as(C.c_void_p),
                                                     logl.ctypes.data_as(C.c_void_p)), "mceik_mcmc_nuis_last")
        return rec, logl

    def nuis_moments(self):
        """{"n", "ksum" [nphase, 2] = sums of k, k^2, "hist" [nphase, nk], "csum"
        [nphase, nstat, 2] = sums of kc, kc^2}: exact int64 sums over the cold
        chains' kept states since `nuis_enable`; ranks merge them by addition."""
        p, nk = self.p, self.nuis_options()["lam"].size
        n = C.c_longlong(0)
        ks, hist, cs = np.zeros((p.nphase, 2), np.int64), np.zeros((p.nphase, nk), np.int64), \
            np.zeros((p.nphase, p.nstat, 2), np.int64)
        self._nuis_held(self._L.mceik_mcmc_nuis_moments_get(self._h, C.byref(n), ks.ctypes.data_as(C.c_void_p),
                                                            hist.ctypes.data_as(C.c_void_p), cs.ctypes.data_as(C.c_void_p)),
                        "mceik_mcmc_nuis_moments_get")
        return {"n": n.value, "ksum": ks, "hist": hist, "csum": cs}

    def nuis_moments_set(self, m):
        """Load moments (`nuis_moments`' dict: a checkpoint's, or merged ones)."""
        ks, hist, cs = (np.ascontiguousarray(m[k], dtype=np.int64) for k in ("ksum", "hist", "csum"))
        ref = self.nuis_moments()
        if any(a.shape != ref[k].shape for a, k in ((ks, "ksum"), (hist, "hist"), (cs, "csum"))):
            raise ValueError("nuis_moments_set: moments of another sampler shape or ladder")
        self._nuis_held(self._L.mceik_mcmc_nuis_moments_set(self._h, int(m["n"]), ks.ctypes.data_as(C.c_void_p),
                                                            hist.ctypes.data_as(C.c_void_p), cs.ctypes.data_as(C.c_void_p)),
                        "mceik_mcmc_nuis_moments_set")

    def nuis_summary(self, moments=None):
        """{"lnlam_mean", "lnlam_std" [nphase], "static_mean", "static_std"
        [nphase, nstat] in seconds} over the cold chains' kept states, from the
        moments (this sampler's, or merged ones) and the ladder's histogram;
        NaN without states."""
        m = self.nuis_moments() if moments is None else moments
        o = self.nuis_options()
        n, p = int(m["n"]), self.p
        if n <= 0:
            nan1, nan2 = np.full(p.nphase, np.nan), np.full((p.nphase, p.nstat), np.nan)
            return {"lnlam_mean": nan1, "lnlam_std": nan1.copy(), "static_mean": nan2, "static_std": nan2.copy()}
        w = np.asarray(m["hist"], np.float64) / n
        mu = w @ o["lnlam"]
        var = np.maximum(w @ (o["lnlam"] ** 2) - mu * mu, 0.0)
        cs = np.asarray(m["csum"], np.float64) / n
        cvar = np.maximum(cs[..., 1] - cs[..., 0] ** 2, 0.0)
        return {"lnlam_mean": mu, "lnlam_std": np.sqrt(var), "static_mean": cs[..., 0] * o["dt"],
                "static_std": np.sqrt(cvar) * o["dt"]}

    # --- probe-to-cell covariances (include/mceik.h mceik_mcmc_cov_*) ---
    def _cov_probe(self, pr):
        """(kind, index) of one probe tuple."""
        p = self.p
        pr = tuple(pr)
        name, args = pr[0], tuple(int(x) for x in pr[1:])

        def flat(a, b, nb):              # a * nb + b with b inside its row (the library checks the rest)
            if not 0 <= b < nb:
                raise ValueError(f"cov_enable: probe {pr!r} out of range")
            return a * nb + b
        if name == "model" and len(args) == 1:
            return 0, args[0]
        if name == "model" and len(args) == 2:
            return 0, flat(args[0], args[1], p.ncell)
        if name == "hypo" and len(args) == 2:
            return 1, flat(args[0], args[1], 3)
        if name == "static" and len(args) == 2:
            return 2, flat(args[0], args[1], p.nstat)
        if name == "noise" and len(args) == 1:
            return 3, args[0]
        raise ValueError(f"cov_enable: a probe is ('model', entry), ('model', phase, cell), ('hypo', event, axis), "
                         f"('static', phase, station) or ('noise', phase), not {pr!r}")

    def cov_enable(self, probes, within=False):
        """Stream the exact cross-moments of up to 64 probe scalars with every
        model entry over the cold chains' kept states of run() (DESIGN.md
        s.16): `cov_summary` then gives each probe's covariance and correlation
        map.  `probes`: ("model", entry) or ("model", phase, cell), ("hypo",
        event, axis) in node units (after a first `hypo_enable`), ("static",
        phase, station) and ("noise", phase) (while `nuis_enable`'s values are
        held with that part on); duplicates are allowed.  `within` also keeps
        per-chain sums (8 bytes per chain and entry) for the within-chain
        maps.  The chains do not change.  Enabling again with the list and
        `within` of held sums resumes them (`cov_disable` keeps them,
        `cov_clear` drops them); another list is refused while they hold states."""
        lst = [self._cov_probe(pr) for pr in probes]
        if not 1 <= len(lst) <= _lib.COV_MAX_PROBES:
            raise ValueError("cov_enable: 1 to 64 probes")
        o = _lib.CovOpts()
        o.np, o.within = len(lst), int(bool(within))
        for k, (kind, idx) in enumerate(lst):
            o.kind[k], o.index[k] = kind, idx
        rc = self._L.mceik_mcmc_cov_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_cov_enable failed ({rc}): indices in range, hypocentre / static / noise probes only while "
                "that state is held, and no held sums of another probe list or `within`")
        self._cov = (lst, bool(within))

    def cov_disable(self):
        """Stop accumulating; the sums stay (`cov_raw`, `cov_partials`, a later `cov_enable` of the same list)."""
        self._kept_disable(_KEPT["cov"])

    def cov_clear(self):
        """Drop the sums and the probe list."""
        self._kept_clear(_KEPT["cov"])

    def cov_accumulate(self):
        """Add the cold chains' current state to the sums now (enqueued)."""
        self._kept_accumulate(_KEPT["cov"])

    def cov_raw(self):
        """The accumulators as host arrays: {"n": states per chain, "probes":
        [(kind, index)], "within", int64 "A" [np], "G" [np, np], "S", "Q" [ncm],
        "C" [np, ncm] and with `within` "Ac" [nchains, np], "Sc" [nchains, ncm]}."""
        return self._kept_raw(_KEPT["cov"])

    def _cov_set(self, raw):
        self._kept_set(_KEPT["cov"], raw)

    def cov_partials(self):
        """The sums as exact partials (`CovPartials`), the chain axis of the
        per-chain sums reduced on the GPU: what ranks exchange and merge."""
        return self._kept_partials(_KEPT["cov"])

    # --- effective sample sizes by batch means (include/mceik.h mceik_mcmc_ess_*) ---
    def ess_enable(self, nlevels=8, probes=()):
        """Stream the batch-means sums of every model entry over the cold
        chains' kept states of run(): `ess_summary` then gives
        the integrated autocorrelation time at batch sizes 2^l, l < `nlevels`
        <= 16, the effective sample size and the Monte-Carlo standard error of
        the pooled mean.  `probes`: up to 64 scalars as in `cov_enable`
        (("hypo", event, axis), ("static", phase, station), ("noise", phase),
        ("model", ...)), further entries after the cells.  Device memory: (8 +
        4 (nlevels - 1)) bytes per chain and entry.  The chains do not change.
        Enabling again with the options of held sums resumes them
        (`ess_disable` keeps them, `ess_clear` drops them); other options are
        refused while they hold states, as is a hierarchy whose half batches
        would not fit 32 bits (max value x 2^(nlevels - 2) >= 2^31)."""
        lst = [self._cov_probe(pr) for pr in probes]
        if len(lst) > _lib.COV_MAX_PROBES:
            raise ValueError("ess_enable: at most 64 probes")
        o = _lib.EssOpts()
        o.nlevels, o.np = int(nlevels), len(lst)
        for k, (kind, idx) in enumerate(lst):
            o.kind[k], o.index[k] = kind, idx
        rc = self._L.mceik_mcmc_ess_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_ess_enable failed ({rc}): nlevels in [1, 16] with max value x 2^(nlevels - 2) < 2^31, probe "
                "indices in range and their state held, and no held sums of other options")
        self._ess = (int(nlevels), lst)

    def ess_disable(self):
        """Stop accumulating; the sums stay (`ess_raw`, `ess_partials`, a later `ess_enable` of the same options)."""
        self._kept_disable(_KEPT["ess"])

    def ess_clear(self):
        """Drop the sums."""
        self._kept_clear(_KEPT["ess"])

    def ess_accumulate(self):
        """Add the cold chains' current state to the sums now (enqueued)."""
        self._kept_accumulate(_KEPT["ess"])

    def ess_raw(self):
        """The accumulators as host arrays: {"n": states per chain, "nlevels",
        "probes": [(kind, index)], "Sc" int64 [nchains, ne], "pend" int32
        [nlevels - 1, nchains, ne], "A" int64 [nlevels, ne], "Q", "P" uint64
        [nlevels, ne, 2] (lo, hi words)}; ne = the model entries, then the probes."""
        return self._kept_raw(_KEPT["ess"])

    def _ess_set(self, raw):
        self._kept_set(_KEPT["ess"], raw)

    def ess_partials(self):
        """The pooled sums as exact partials (`EssPartials`): what ranks exchange and merge."""
        return self._kept_partials(_KEPT["ess"])

    # --- pick residuals, origin times and data-fit checks (include/mceik.h mceik_mcmc_fit_*) ---
    def fit_enable(self, tick=2.0 ** -20, nbins=64, zmax=8.0, t0_ref=None):
        """Stream the data side of run() over the cold chains' kept states
        (DESIGN.md s.20): `fit_summary` then gives per pick the mean and spread
        of its residual and of its standardised residual z, per event the
        origin time and a reduced misfit, per (phase, station) the mean
        residual, the rms of z and a histogram of z with `nbins` (even, 2 ..
        256) bins over [-`zmax`, `zmax`].  Residuals and origin times are
        summed in units of `tick` seconds (a power of two; |value| / tick <
        2^31, see `fit_check`); `t0_ref` [nev] (None: zeros) is subtracted
        from the origin times first, so absolute-epoch catalogues stay in
        range.  Everything is taken from the chain's current tables and
        effective observations, exactly as its logL sees them.  The chains do
        not change.  A one-model sampler holds its current tables while this is
        on and steps with one launch per step (`info()["multi_step"]` is False
        until `fit_disable`).  Enabling again with the options of held sums
        resumes them (`fit_disable` keeps them, `fit_clear` drops them); other
        options are refused while they hold states."""
        nev = self.p.nevents
        ref = np.zeros(nev) if t0_ref is None else np.ascontiguousarray(t0_ref, dtype=np.float64).ravel()
        if ref.size != nev:
            raise ValueError("fit_enable: t0_ref is one time per event")
        o = _lib.FitOpts()
        o.tick, o.nbins, o.zmax, o.t0_ref = float(tick), int(nbins), float(zmax), ref.ctypes.data
        rc = self._L.mceik_mcmc_fit_enable(self._h, C.byref(o))
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(
                f"mceik_mcmc_fit_enable failed ({rc}): tick a power of two, nbins even in [2, 256], zmax > 0, a finite "
                "t0_ref, and no held sums of other options")
        self._fit = (float(tick), int(nbins), float(zmax), ref.copy())
        self._fit_active = True

    def fit_disable(self):
        """Stop accumulating; the sums stay (`fit_raw`, `fit_partials`, a later `fit_enable` of the same options)."""
        self._kept_disable(_KEPT["fit"])
        self._fit_active = False

    def fit_clear(self):
        """Drop the sums."""
        self._kept_clear(_KEPT["fit"])
        self._fit_active = False

    def fit_accumulate(self):
        """Add the cold chains' current state to the sums now (enqueued)."""
        self._kept_accumulate(_KEPT["fit"])

    def fit_raw(self):
        """The accumulators as host arrays: {"n": states per chain, "tick",
        "nbins", "zmax", "t0_ref" [nev], "sq", "szq" int64 [nobs], "sq2", "szq2"
        uint64 [nobs, 2] (lo, hi words), "stq" int64 [nev], "stq2" uint64 [nev,
        2], "hist" int64 [nphase, nstat, nbins], "sat" int64 [3] (clamped q,
        zq, tq)}."""
        return self._kept_raw(_KEPT["fit"])

    def _fit_set(self, raw):
        self._kept_set(_KEPT["fit"], raw)

    def fit_partials(self):
        """The pooled sums as exact partials (`FitPartials`): what ranks exchange and merge."""
        return self._kept_partials(_KEPT["fit"])

    def fit_last(self):
        """The last kept step's integers of every chain: (q, zq int32 [nchains,
        nobs], tq int32 [nchains, nev]); q, zq are 0 for a masked pick, rows of
        chains that are not cold stay 0."""
        self._kept_on(_KEPT["fit"])
        q = np.zeros((self.nchains, len(self.p.tobs)), np.int32)
        zq, tq = np.zeros_like(q), np.zeros((self.nchains, self.p.nevents), np.int32)
        rc = self._L.mceik_mcmc_fit_last(self._h, *(a.ctypes.data_as(C.c_void_p) for a in (q, zq, tq)))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_fit_last failed ({rc})")
        return q, zq, tq

    def fsm_stats(self, reset=False):
        """(FSM kernel ms from hipEvents, launches, executed iterations summed over
        solves, (brick visits, column segments updated, segments changed, wave macro
        steps))."""
        ms, nl, it, tv = C.c_double(0), C.c_longlong(0), C.c_ulonglong(0), (C.c_ulonglong * 4)()
        if self._L.mceik_mcmc_fsm_stats(self._h, C.byref(ms), C.byref(nl), C.byref(it), tv, int(reset)) != 0:
            raise RuntimeError("mceik_mcmc_fsm_stats failed")
        return ms.value, nl.value, it.value, tuple(tv)

    def fsm_solves(self):
        """Solves executed since init or the last fsm_stats(reset=True) (mceik_mcmc_fsm_solves;
        solves of stations without picks of the phase are skipped, not counted)."""
        n = C.c_ulonglong(0)
        if self._L.mceik_mcmc_fsm_solves(self._h, C.byref(n)) != 0:
            raise RuntimeError("mceik_mcmc_fsm_solves failed")
        return n.value

    def samples(self, max_states=None, device_ptr=None):
        """Kept states [k, *model_shape] (host numpy, or copied into device_ptr).
        Every chain is kept; with tempering on, the cold chains are the first
        G = nchains / ntemps of them (`cold_chains`)."""
        max_states = self.max_samples if max_states is None else max_states
        n = C.c_int(0)
        if device_ptr is not None:
            self._L.mceik_mcmc_get_samples(self._h, C.c_void_p(device_ptr), None, max_states, 1, C.byref(n))
            return n.value
        v = np.empty((max(max_states, 1),) + self.model_shape, np.int32)
        lg = np.empty((max(max_states, 1), self.nchains), np.float64)
        self._L.mceik_mcmc_get_samples(self._h, v.ctypes.data_as(C.c_void_p), lg.ctypes.data_as(C.c_void_p),
                                       max_states, 0, C.byref(n))
        return v[:n.value], lg[:n.value]

    def close(self):
        if self._h:
            self._L.mceik_mcmc_finalize(C.byref(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Partials:
    """What the four *Partials share: `merge` through the C merge `_merge` of two
    `_struct()`s (ValueError `_mismatch` where they do not match), and `_took`,
    which copies back what a C call that filled a `_struct()` wrote into it."""
    _merge = _mismatch = None

    def _took(self, st):
        self.nchains, self.nkept = int(st.nchains), int(st.nkept)

    def merge(self, other):
        """self += other (the C merge: mceik_posterior_merge, mceik_cov_merge,
        mceik_ess_merge, mceik_fit_merge); both must hold the same entries,
        options and states per chain."""
        a, b = self._struct(), other._struct()
        if getattr(_lib.lib(), self._merge)(C.byref(a), C.byref(b)) != 0:
            raise ValueError(self._mismatch)
        self._took(a)
        return self


class PosteriorPartials(_Partials):
    """Host arrays of mceik_posterior_partials (include/mceik.h): per model
    entry S = sum_c sum_c (int64 [ncm]), Q = sum_c sumsq_c and P = sum_c sum_c^2
    (uint64 [ncm, 2]: lo, hi words of 128 bits) and the histogram widened to
    uint64 [ncm, nbins], over `nchains` chains of `nkept` states each.  Exact
    integers: partials of shards or ranks merge by addition, in any order.
    Plain attributes, so it travels as a host object (pickle)."""
    _merge, _mismatch = "mceik_posterior_merge", "posterior partials do not match (ncm, nbins, per_chain, nkept)"

    def __init__(self, ncm, nbins, per_chain, nchains=0, nkept=0, shape=None, bounds=None):
        self.ncm, self.nbins, self.per_chain = int(ncm), int(nbins), bool(per_chain)
        self.nchains, self.nkept = int(nchains), int(nkept)
        self.shape = tuple(shape) if shape is not None else (self.ncm,)
        self.bounds = [tuple(b) for b in bounds] if bounds is not None else None   # per phase (lo, hi) of the bins
        self.S = np.zeros(self.ncm, np.int64)
        self.Q = np.zeros((self.ncm, 2), np.uint64)
        self.P = np.zeros((self.ncm, 2), np.uint64)
        self.hist = np.zeros((self.ncm, self.nbins), np.uint64)

    def _struct(self):
        st = _lib.PosteriorPartials()
        st.ncm, st.nbins, st.per_chain = self.ncm, self.nbins, int(self.per_chain)
        st.nchains, st.nkept = self.nchains, self.nkept
        st.S, st.Q, st.P = self.S.ctypes.data, self.Q.ctypes.data, self.P.ctypes.data
        st.hist = self.hist.ctypes.data if self.nbins else None
        return st

    def finish(self):
        """(mean, var, rhat) float64 [ncm] (mceik_posterior_finish)."""
        mean, var, rhat = (np.empty(self.ncm, np.float64) for _ in range(3))
        st = self._struct()
        rc = _lib.lib().mceik_posterior_finish(C.byref(st), mean.ctypes.data_as(C.c_void_p),
                                               var.ctypes.data_as(C.c_void_p), rhat.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"mceik_posterior_finish failed ({rc})")
        return mean, var, rhat


class PosteriorSummary:
    """Posterior of the velocity models from merged `PosteriorPartials`:
    `mean`, `var` (sample variance over all chains and states), `rhat`
    (Gelman-Rubin; NaN in pooled mode, with fewer than 2 chains or states, and
    where no chain moved) shaped like one chain's model, `hist` [..., nbins]
    uint64, `count` states per chain over `nchains` chains."""

    def __init__(self, parts: PosteriorPartials):
        mean, var, rhat = parts.finish()
        sh = parts.shape
        self.mean, self.var, self.rhat = mean.reshape(sh), var.reshape(sh), rhat.reshape(sh)
        self.hist = parts.hist.reshape(sh + (parts.nbins,)).copy()
        self.count, self.nchains, self.nbins = parts.nkept, parts.nchains, parts.nbins
        self.bounds = parts.bounds

    def quantile(self, q):
        """Marginal q-quantile (0 <= q <= 1) of every model entry, in numpy from
        the histogram: the bin where the cumulative count reaches q x total,
        then linear inside that bin, whose edges are lo + b (hi - lo + 1) /
        nbins of the phase's prior range.  Its resolution is the bin width; an
        entry without counts gives NaN."""
        if not self.nbins or self.bounds is None:
            raise ValueError("quantile needs a histogram (nbins > 0) and the prior bounds")
        if not 0.0 <= q <= 1.0:
            raise ValueError("q in [0, 1]")
        h = self.hist.astype(np.float64)
        cum = np.cumsum(h, axis=-1)
        total = cum[..., -1]
        target = q * total
        b = np.minimum((cum < target[..., None]).sum(-1), self.nbins - 1)
        hb = np.take_along_axis(h, b[..., None], -1)[..., 0]
        below = np.take_along_axis(cum, b[..., None], -1)[..., 0] - hb
        frac = np.divide(target - below, hb, out=np.zeros_like(hb), where=hb > 0)
        lo = np.empty(self.mean.shape)
        width = np.empty(self.mean.shape)
        for ph, (l, u) in enumerate(self.bounds):
            sel = (ph,) if len(self.bounds) > 1 else ()
            lo[sel] = l
            width[sel] = (u - l + 1) / self.nbins
        out = lo + (b + frac) * width
        return np.where(total > 0, out, np.nan)


def _gather_merged(parts, group, dst):
    """This rank's exact partials (anything with merge()) gathered over the
    torch.distributed `group` as host objects and merged on rank `dst`: the
    merged partials there, None on the other ranks; without a group, `parts`."""
    if group is None:
        return parts
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    every = [None] * world if rank == dst else None
    dist.gather_object(parts, every, dst=dst, group=group)
    if rank != dst:
        return None
    parts = every[0]
    for other in every[1:]:
        parts.merge(other)
    return parts


def posterior_summary(smp: Sampler, group=None, dst=0):
    """`PosteriorSummary` of a sampler's streaming posterior.  With a
    torch.distributed `group` (one process per GPU, each with its chain shard)
    the ranks' exact partials are gathered as host objects and merged on rank
    `dst`, which gets the summary of all chains; the other ranks get None."""
    parts = _gather_merged(smp.posterior_partials(), group, dst)
    return None if parts is None else PosteriorSummary(parts)


class CovPartials(_Partials):
    """Host arrays of mceik_cov_partials (include/mceik.h) for the probe list
    `probes` [(kind, index)]: A [np] and S [ncm] int64; G [np, np, 2], Q [ncm,
    2], C [np, ncm, 2] and, within-chain, PA, P, T of the same shapes: uint64
    lo, hi words of 128-bit two's complement integers, over `nchains` chains
    of `nkept` states each.  Exact integers: partials of shards or ranks merge
    by addition, in any order.  Plain attributes, so it travels as a host
    object (pickle)."""
    _merge, _mismatch = "mceik_cov_merge", "covariance partials do not match (probes, ncm, within, nkept)"

    def __init__(self, probes, ncm, within, nchains=0, nkept=0, shape=None):
        self.probes = [(int(k), int(i)) for k, i in probes]
        self.np, self.ncm, self.within = len(self.probes), int(ncm), bool(within)
        self.nchains, self.nkept = int(nchains), int(nkept)
        self.shape = tuple(shape) if shape is not None else (self.ncm,)
        n = self.np
        self.A, self.S = np.zeros(n, np.int64), np.zeros(self.ncm, np.int64)
        self.G, self.Q, self.C = (np.zeros(sh + (2,), np.uint64) for sh in ((n, n), (self.ncm,), (n, self.ncm)))
        self.PA, self.P, self.T = (np.zeros(sh + (2,), np.uint64) for sh in ((n, n), (self.ncm,), (n, self.ncm)))

    def _struct(self):
        st = _lib.CovPartials()
        st.np, st.ncm, st.within = self.np, self.ncm, int(self.within)
        for k, (kind, idx) in enumerate(self.probes[:_lib.COV_MAX_PROBES]):
            st.kind[k], st.index[k] = kind, idx
        st.nchains, st.nkept = self.nchains, self.nkept
        for name in ("A", "S", "G", "Q", "C", "PA", "P", "T"):
            setattr(st, name, getattr(self, name).ctypes.data)
        return st

    def finish(self):
        """dict of float64 arrays (mceik_cov_finish): cov, corr, cov_within,
        corr_within [np, ncm]; probe_mean [np]; probe_cov, probe_corr,
        probe_cov_within, probe_corr_within [np, np]."""
        n, ncm = self.np, self.ncm
        out = {k: np.empty((n, ncm)) for k in ("cov", "corr", "cov_within", "corr_within")}
        out["probe_mean"] = np.empty(n)
        out.update({k: np.empty((n, n)) for k in ("probe_cov", "probe_corr", "probe_cov_within", "probe_corr_within")})
        st = self._struct()
        rc = _lib.lib().mceik_cov_finish(C.byref(st), *(a.ctypes.data_as(C.c_void_p) for a in out.values()))
        if rc != 0:
            raise RuntimeError(f"mceik_cov_finish failed ({rc})")
        return out


class CovSummary:
    """Trade-off maps from merged `CovPartials`: `cov`, `corr` (over all chains
    and states) and `cov_within`, `corr_within` (about each chain's own mean;
    NaN without `within`, with fewer than 2 states) of every probe with every
    model entry, shaped [np] + one chain's model shape; `probe_mean` [np] and
    the probe x probe `probe_cov`, `probe_corr`, `probe_cov_within`,
    `probe_corr_within` [np, np]; `probes` [(kind, index)], `count` states per
    chain over `nchains` chains.  A correlation with a constant quantity is NaN."""

    def __init__(self, parts: CovPartials):
        out = parts.finish()
        sh = (parts.np,) + parts.shape
        for k in ("cov", "corr", "cov_within", "corr_within"):
            setattr(self, k, out[k].reshape(sh))
        for k in ("probe_mean", "probe_cov", "probe_corr", "probe_cov_within", "probe_corr_within"):
            setattr(self, k, out[k])
        self.probes = list(parts.probes)
        self.count, self.nchains, self.within = parts.nkept, parts.nchains, parts.within


def cov_summary(smp: Sampler, group=None, dst=0):
    """`CovSummary` of a sampler's covariance sums.  With a torch.distributed
    `group` the ranks' exact partials are gathered as host objects and merged
    on rank `dst`, which gets the summary of all chains; the other ranks get
    None (as `posterior_summary`)."""
    parts = _gather_merged(smp.cov_partials(), group, dst)
    return None if parts is None else CovSummary(parts)


def ess_check(nlevels, xmax):
    """A hierarchy of `nlevels` batch sizes holds entries up to `xmax`
    (mceik_ess_check: nlevels in [1, 16] and xmax 2^(nlevels - 2) < 2^31)."""
    return _lib.lib().mceik_ess_check(int(nlevels), int(xmax)) == 0


def ess_lstar(nlevels, n):
    """The level `ess_summary` reports for n states per chain: min(nlevels - 1,
    floor(log2(n) / 2)), a batch of about sqrt(n) states (mceik_ess_lstar)."""
    return _lib.lib().mceik_ess_lstar(int(nlevels), int(n))


class EssPartials(_Partials):
    """Host arrays of mceik_ess_partials (include/mceik.h) over ne = `ncm`
    model entries + the `probes` [(kind, index)] and `nlevels` batch sizes 2^l:
    A int64 [nlevels, ne] (sum over chains of the closed level-l batch sums), Q
    and P uint64 [nlevels, ne, 2] (lo, hi words of 128 bits: the sum of the
    squared batch sums; the sum over chains of the squared cumulative sum at
    the last close), over `nchains` chains of `nkept` states each.  Exact
    integers: partials of shards or ranks merge by addition, in any order.
    Plain attributes, so it travels as a host object (pickle)."""
    _merge, _mismatch = "mceik_ess_merge", "batch-means partials do not match (ncm, probes, nlevels, nkept)"

    def __init__(self, ncm, nlevels, probes=(), nchains=0, nkept=0, shape=None):
        self.probes = [(int(k), int(i)) for k, i in probes]
        self.ncm, self.np, self.nlevels = int(ncm), len(self.probes), int(nlevels)
        self.nchains, self.nkept = int(nchains), int(nkept)
        self.shape = tuple(shape) if shape is not None else (self.ncm,)
        ne = self.ncm + self.np
        self.A = np.zeros((self.nlevels, ne), np.int64)
        self.Q = np.zeros((self.nlevels, ne, 2), np.uint64)
        self.P = np.zeros((self.nlevels, ne, 2), np.uint64)

    def _struct(self):
        st = _lib.EssPartials()
        st.ncm, st.np, st.nlevels = self.ncm, self.np, self.nlevels
        st.nchains, st.nkept = self.nchains, self.nkept
        st.A, st.Q, st.P = self.A.ctypes.data, self.Q.ctypes.data, self.P.ctypes.data
        return st

    def merge(self, other):
        """self += other (mceik_ess_merge); both must hold the same entries,
        probes, levels and states per chain."""
        if self.probes != other.probes:  # (the C struct carries their number only)
            raise ValueError(self._mismatch)
        return super().merge(other)

    def finish(self, level=None):
        """(tau [nlevels, ne], ess [ne], mcse [ne], level) (mceik_ess_finish);
        level None: the one `ess_lstar` picks."""
        ne = self.ncm + self.np
        tau, ess, mcse = np.empty((self.nlevels, ne)), np.empty(ne), np.empty(ne)
        st, used = self._struct(), C.c_int(0)
        rc = _lib.lib().mceik_ess_finish(C.byref(st), -1 if level is None else int(level), tau.ctypes.data_as(C.c_void_p),
                                         ess.ctypes.data_as(C.c_void_p), mcse.ctypes.data_as(C.c_void_p), C.byref(used))
        if rc != 0:
            raise ValueError(f"mceik_ess_finish failed ({rc}): level < nlevels")
        return tau, ess, mcse, used.value


class EssSummary:
    """Mixing of every model entry from merged `EssPartials`: `tau_levels`
    [nlevels, ...] the integrated autocorrelation time seen at batch size 2^l
    (a plateau over l means the batches have outgrown the correlation; a
    value still rising means `tau` is a lower bound), and at batch size
    2^`level` `tau`, `ess` = nchains count / tau and `mcse`, the standard error
    of the mean pooled over chains and states -- shaped like one chain's
    model.  `probe_tau_levels` [nlevels, np], `probe_tau`, `probe_ess`,
    `probe_mcse` [np]: the same for `probes` [(kind, index)].  NaN: an entry
    that never moved, levels with fewer than two closed batches.  `count`
    states per chain over `nchains` chains."""

    def __init__(self, parts: EssPartials, level=None):
        tau, ess, mcse, used = parts.finish(level)
        m, sh, L = parts.ncm, parts.shape, parts.nlevels
        self.tau_levels, self.probe_tau_levels = tau[:, :m].reshape((L,) + sh), tau[:, m:].copy()
        self.tau, self.probe_tau = self.tau_levels[used], self.probe_tau_levels[used]
        self.ess, self.probe_ess = ess[:m].reshape(sh), ess[m:].copy()
        self.mcse, self.probe_mcse = mcse[:m].reshape(sh), mcse[m:].copy()
        self.level, self.nlevels, self.probes = used, L, list(parts.probes)
        self.count, self.nchains = parts.nkept, parts.nchains


def ess_summary(smp: Sampler, group=None, level=None, dst=0):
    """`EssSummary` of a sampler's batch-means sums at batch size 2^`level`
    (None: `ess_lstar`'s choice, about sqrt(count) states).  With a
    torch.distributed `group` the ranks' exact partials are gathered as host
    objects and merged on rank `dst`, which gets the summary of all chains;
    the other ranks get None (as `posterior_summary`)."""
    parts = _gather_merged(smp.ess_partials(), group, dst)
    return None if parts is None else EssSummary(parts, level)


def fit_check(tick, rmax):
    """Residuals (and origin times less t0_ref) up to `rmax` seconds fit the
    32-bit words of `fit_enable` at `tick` (mceik_fit_check: tick a power of
    two and rmax / tick <= 2^31 - 1)."""
    return _lib.lib().mceik_fit_check(float(tick), float(rmax)) == 0


class FitPartials(_Partials):
    """Host arrays of mceik_fit_partials (include/mceik.h): sq, szq int64
    [nobs] (sums of the residuals in ticks and of 1024 z), sq2, szq2 uint64
    [nobs, 2] (lo, hi words of the 128-bit sums of their squares), stq int64
    [nev] and stq2 uint64 [nev, 2] (the origin times less t0_ref), hist int64
    [nphase, nstat, nbins], sat int64 [3] (clamped values), over `nchains`
    chains of `nkept` states each; obs_ptr, obs_stat, obs_phase, obs_mask and
    t0_ref say what the rows are.  Exact integers: partials of shards or ranks
    merge by addition, in any order.  Plain attributes, so it travels as a
    host object (pickle)."""
    _merge = "mceik_fit_merge"
    _mismatch = "data-fit partials do not match (observations, tick, nbins, zmax, t0_ref, nkept)"

    def __init__(self, nobs, nev, nphase, nstat, nbins, tick, zmax, nchains=0, nkept=0):
        self.nobs, self.nev, self.nphase, self.nstat, self.nbins = int(nobs), int(nev), int(nphase), int(nstat), int(nbins)
        self.tick, self.zmax = float(tick), float(zmax)
        self.nchains, self.nkept = int(nchains), int(nkept)
        self.obs_ptr = np.zeros(self.nev + 1, np.int32)
        self.obs_stat, self.obs_phase, self.obs_mask = (np.zeros(self.nobs, np.int32) for _ in range(3))
        self.t0_ref = np.zeros(self.nev, np.float64)
        self.sq, self.szq = np.zeros(self.nobs, np.int64), np.zeros(self.nobs, np.int64)
        self.sq2, self.szq2 = np.zeros((self.nobs, 2), np.uint64), np.zeros((self.nobs, 2), np.uint64)
        self.stq, self.stq2 = np.zeros(self.nev, np.int64), np.zeros((self.nev, 2), np.uint64)
        self.hist = np.zeros((self.nphase, self.nstat, self.nbins), np.int64)
        self.sat = np.zeros(3, np.int64)

    def _struct(self):
        st = _lib.FitPartials()
        st.nobs, st.nev, st.nphase, st.nstat, st.nbins = self.nobs, self.nev, self.nphase, self.nstat, self.nbins
        st.tick, st.zmax = self.tick, self.zmax
        st.nchains, st.nkept = self.nchains, self.nkept
        for name in ("obs_ptr", "obs_stat", "obs_phase", "obs_mask", "t0_ref", "sq", "szq", "sq2", "szq2", "stq", "stq2",
                     "hist"):
            setattr(st, name, getattr(self, name).ctypes.data)
        for k in range(3):
            st.sat[k] = int(self.sat[k])
        return st

    def _took(self, st):
        super()._took(st)
        self.sat[:] = list(st.sat)

    def finish(self):
        """dict of float64 arrays (mceik_fit_finish): pick_mean, pick_sd,
        pick_zmean, pick_zrms [nobs]; t0_mean, t0_sd, ev_misfit [nev];
        sta_mean, sta_zrms [nphase, nstat]; phase_zrms [nphase]."""
        out = {k: np.empty(self.nobs) for k in ("pick_mean", "pick_sd", "pick_zmean", "pick_zrms")}
        out.update({k: np.empty(self.nev) for k in ("t0_mean", "t0_sd", "ev_misfit")})
        out.update({k: np.empty((self.nphase, self.nstat)) for k in ("sta_mean", "sta_zrms")})
        out["phase_zrms"] = np.empty(self.nphase)
        st = self._struct()
        rc = _lib.lib().mceik_fit_finish(C.byref(st), *(a.ctypes.data_as(C.c_void_p) for a in out.values()))
        if rc != 0:
            raise RuntimeError(f"mceik_fit_finish failed ({rc})")
        return out


class FitSummary:
    """The data side of a run from merged `FitPartials`.  Per pick [nobs]:
    `pick_mean`, `pick_sd` (seconds) of the residual tobs - tcorr - (te + t0)
    and `pick_zmean`, `pick_zrms` of the standardised residual z (rms about 1
    where the noise level is right; under the L1 likelihood, `likelihood_set(1)`,
    var is a Laplace scale, the expected z^2 is 2, and t0 is the weighted median).
    Per event [nev]: `t0_mean`, `t0_sd` (the
    origin time, t0_ref added back) and `ev_misfit`, the mean over states of
    sum z^2 / (used picks - 1).  Per (phase, station) [nphase, nstat]:
    `sta_mean` (the mean residual: the data's estimate of a station static),
    `sta_zrms` and `hist` [nphase, nstat, nbins], the counts of z over
    `bin_edges` (the edge bins take the tails).  `phase_zrms` [nphase];
    `saturated` = (q, zq, tq) values that were clamped (0 in a healthy run).
    NaN: a masked pick, a row or event without used picks, fewer than 2
    states.  `count` states per chain over `nchains` chains."""

    def __init__(self, parts: FitPartials):
        for k, v in parts.finish().items():
            setattr(self, k, v)
        self.hist = parts.hist.copy()
        self.bin_edges = np.linspace(-parts.zmax, parts.zmax, parts.nbins + 1)
        self.saturated = tuple(int(x) for x in parts.sat)
        self.tick, self.count, self.nchains = parts.tick, parts.nkept, parts.nchains


def fit_summary(smp: Sampler, group=None, dst=0):
    """`FitSummary` of a sampler's data-fit sums.  With a torch.distributed
    `group` the ranks' exact partials are gathered as host objects and merged
    on rank `dst`, which gets the summary of all chains; the other ranks get
    None (as `posterior_summary`)."""
    parts = _gather_merged(smp.fit_partials(), group, dst)
    return None if parts is None else FitSummary(parts)


def picks_from_forward(device=0, precision=64):
    """picks callable for make_problem: GPU forward of the true model (fp64 by
    default: the reference's arithmetic, and a different kernel instance from
    the fp32 sampler so profiles of the two do not mix).  f(p) or f(p, phase):
    phase 1 solves the S model `vs_true`."""
    def f(p: Problem, phase=0):
        import torch
        from .eikonal import BatchSolver
        dev = torch.device("cuda", device)
        bs = BatchSolver(p.nx, p.ny, p.nz, p.h, p.x0, p.y0, p.z0, p.maxit, p.tol, precision, nref=p.nref)
        src = torch.tensor(np.stack([np.zeros(p.nstat), p.sx, p.sy, p.sz], 1)[:, None, :], dtype=torch.float64)
        vt = p.vs_true if phase else p.v_true
        slow = torch.tensor((1.0 / vt.astype(np.float32)).astype(np.float32).reshape(1, -1), device=dev)
        out = bs.solve(src, slow, ev_node=torch.tensor(p.ev_node))
        torch.cuda.synchronize(dev)
        return out["ttab"].cpu().numpy().reshape(p.nstat, p.nevents)
    return f


def weighted_median(x, w):
    """The lower weighted median of x with weights w (weightedMedian__double, the
    library's host code; csrc/l1.h): the smallest x_k whose weights at or below
    it, in (value, index) order, reach half the total."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    w = np.ascontiguousarray(w, dtype=np.float64).ravel()
    if x.size < 1 or x.size != w.size:
        raise ValueError("weighted_median: x and w of one length >= 1")
    ierr = C.c_int(0)
    t = _lib.lib().weightedMedian__double(int(x.size), x.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                          None, None, C.byref(ierr))
    if ierr.value != 0:
        raise RuntimeError("weightedMedian__double failed")
    return float(t)


def l1_event(x, w, mask=None):
    """(t0, objfn) of one event under the L1 likelihood (mceik_l1_event, the
    library's host code; csrc/l1.h): t0 the lower weighted median of the used
    residuals x with weights w, objfn = sum w |x - t0| in order; (0, 0) when no
    entry is used.  mask: 1 = not used."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    w = np.ascontiguousarray(w, dtype=np.float64).ravel()
    if x.size != w.size:
        raise ValueError("l1_event: x and w of one length")
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32).ravel()
    if m is not None and m.size != x.size:
        raise ValueError("l1_event: mask of the length of x")
    t0, obj = C.c_double(0.0), C.c_double(0.0)
    if _lib.lib().mceik_l1_event(int(x.size), None if m is None else m.ctypes.data_as(C.c_void_p),
                                 x.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), C.byref(t0),
                                 C.byref(obj)) != 0:
        raise RuntimeError("mceik_l1_event failed")
    return t0.value, obj.value


def _pick_terms(p: Problem, ttab, var, tcorr, with_t0=False, norm=2):
    """event_obj's arithmetic (csrc/mcmc_device.h) on the host, operation for
    operation in fp64: per event the used picks, their weights 1 / var, xnorm,
    the residuals tc - (te + t0) and objfn (with_t0: and, sixth, t0).  norm=1:
    event_obj_l1's (csrc/l1.h through `l1_event`): the third entry is the sum
    of the weights, t0 the weighted median, the residuals (tc - te) - t0."""
    if norm not in (1, 2):
        raise ValueError("norm: 1 or 2")
    tt = np.asarray(ttab, dtype=np.float32).astype(np.float64).reshape(max(1, p.nphase), p.nstat, p.nevents)
    var = np.asarray(p.var if var is None else var, dtype=np.float64)
    tcorr = np.asarray(p.tcorr if tcorr is None else tcorr, dtype=np.float64)
    mask, phase, stat, tobs, ptr = p.obs_mask, p.obs_phase, p.obs_stat, p.tobs, p.obs_ptr
    sqrt2i = 0.7071067811865475
    out = []
    for e in range(p.nevents):
        js = [j for j in range(int(ptr[e]), int(ptr[e + 1])) if not mask[j]]
        if norm == 1:
            w = [1.0 / float(var[j]) for j in js]
            x = [(float(tobs[j]) - float(tcorr[j])) - float(tt[phase[j], stat[j], e]) for j in js]
            wsum = 0.0
            for wj in w:
                wsum = wsum + wj
            t0, obj = l1_event(x, w)
            out.append((js, w, wsum, [xj - t0 for xj in x], obj) + ((t0,) if with_t0 else ()))
            continue
        xnorm = 0.0
        for j in js:
            xnorm = xnorm + 1.0 / float(var[j])
        t0 = 0.0
        for j in js:
            te = float(tt[phase[j], stat[j], e])
            t0 = t0 + ((1.0 / float(var[j])) / xnorm) * ((float(tobs[j]) - float(tcorr[j])) - te)
        obj, res = 0.0, []
        for j in js:
            te = float(tt[phase[j], stat[j], e])
            r = (float(tobs[j]) - float(tcorr[j])) - (te + t0)
            s = ((1.0 / float(var[j])) * sqrt2i) * r
            obj = obj + s * s
            res.append(r)
        out.append((js, [1.0 / float(var[j]) for j in js], xnorm, res, obj) + ((t0,) if with_t0 else ()))
    return out


def logl_picks(p: Problem, ttab, var=None, tcorr=None, norm=2):
    """logL = ((0 - objfn_0) - objfn_1) - ... of the tables ttab [nphase, nstat,
    nev] ([nstat, nev] with one model): the sampler's value bit for bit (the
    noise normalisation of DESIGN.md s.15 is the caller's).  var, tcorr [nobs]:
    effective values (None: the catalogue's).  norm: the likelihood's
    (`Sampler.likelihood_set`)."""
    logl = 0.0
    for _, _, _, _, obj in _pick_terms(p, ttab, var, tcorr, norm=norm):
        logl = logl - obj
    return logl


def logl_pick_grad(p: Problem, ttab, var=None, tcorr=None):
    """d logL / d te_j [nobs] (fp64, host) of `logl_picks`: the derivative of
    the sampler's objective with respect to the table value each used pick is
    fit against (0 for a masked pick).  The origin time t0 is the mean weighted
    by w = 1 / var while the objective weighs residuals by w^2 / 2, so t0 does
    not minimise it and its dependence on te stays:
      d logL / d te_j = w_j^2 r_j - (w_j / xnorm_e) sum_{i in e} w_i^2 r_i,
    r = tc - (te + t0), over the used picks of j's event."""
    g = np.zeros(len(p.tobs), np.float64)
    for js, w, xnorm, res, _ in _pick_terms(p, ttab, var, tcorr):
        s = 0.0
        for wi, ri in zip(w, res):
            s = s + (wi * wi) * ri
        for j, wj, rj in zip(js, w, res):
            g[j] = (wj * wj) * rj - (wj / xnorm) * s
    return g


def logl_inputs(smp: "Sampler"):
    """What a chain's logL depends on besides its models, as the sampler holds
    it now: {"hyp": int32 [nchains, nev, 3] or None (the catalogue's nodes),
    "var", "tcorr": [nchains, nobs] effective observations,
    "norm": [nchains, nphase] the noise normalisation terms norm[ph] *
    lnlam[kn[c][ph]], subtracted from logL in phase order}."""
    p, nch = smp.p, smp.nchains
    try:
        hyp = smp.hypo_positions()
    except RuntimeError:
        hyp = None
    var = np.tile(np.asarray(p.var, np.float64), (nch, 1))
    tcorr = np.tile(np.asarray(p.tcorr, np.float64), (nch, 1))
    norm = np.zeros((nch, max(1, p.nphase)))
    if smp._nuis is not None:
        kn, kc = smp.nuis_get()
        o = smp.nuis_options()
        ph, st = p.obs_phase, np.clip(p.obs_stat, 0, p.nstat - 1)
        for c in range(nch):
            if o["lam"].size:
                var[c] = var[c] * o["lam"][kn[c][ph]]
                norm[c] = o["norm"] * o["lnlam"][kn[c]]
            if o["statics"]:
                tcorr[c] = tcorr[c] + kc[c][ph, st].astype(np.float64) * o["dt"]
    return {"hyp": hyp, "var": var, "tcorr": tcorr, "norm": norm}


def logl_grad(smp: "Sampler", chains=None, wrt="slowness", chunk=None):
    """Exact gradient of the log likelihood of the chosen chains' current
    models with respect to every inversion cell: (grad float64 [nchain, nphase
    * ncell], logl float64 [nchain]).  One forward with fields and one adjoint
    solve per (chain, phase, station), in chunks of `chunk`
    chains (None: sized to about 2 GiB of fields).  Honours P and P+S models,
    mask_s, the station flags (a station without picks of a phase is skipped),
    tt_interp, the chains' current hypocentres and their noise scale and
    statics; logl is the sampler's own value for that state.

    wrt="slowness": d logL / d s of the cell slowness s = 1 / v the forward
    solves with; wrt="velocity": that times -1 / v^2.  This is the gradient of
    the UNTEMPERED LIKELIHOOD only: a tempered chain's beta, the smoothness /
    reference prior and the box are the caller's to add."""
    import torch
    from .eikonal import BatchSolver
    if wrt not in ("slowness", "velocity"):
        raise ValueError(f"wrt: 'slowness' or 'velocity', not {wrt!r}")
    if smp.likelihood != 2:
        raise ValueError("logl_grad: the sampler's likelihood is L1 (likelihood_set): the gradient of its "
                         "piecewise-linear objective is not provided")
    p = smp.p
    chains = list(range(smp.nchains)) if chains is None else [int(c) for c in chains]
    nph, nstat, nev, ncell = max(1, p.nphase), p.nstat, p.nevents, p.ncell
    dev = torch.device("cuda", smp.device)
    v = smp.state()[0].reshape(smp.nchains, nph, ncell)
    inp = logl_inputs(smp)
    bs = BatchSolver(p.nx, p.ny, p.nz, p.h, p.x0, p.y0, p.z0, p.maxit, p.tol, smp.precision, nref=p.nref,
                     fast_sqrt=True)
    src = torch.tensor(np.stack([np.zeros(nstat), p.sx, p.sy, p.sz], 1)[:, None, :], dtype=torch.float64)
    if chunk is None:
        per_chain = p.nx * p.ny * p.nz * (8 if smp.precision == 64 else 4) * nph * nstat
        chunk = max(1, (1 << 31) // per_chain)
    grad = np.empty((len(chains), nph * ncell), np.float64)
    logl = np.empty(len(chains), np.float64)
    for k0 in range(0, len(chains), int(chunk)):
        cs = chains[k0:k0 + int(chunk)]
        slow = torch.tensor((np.float32(1.0) / v[cs].astype(np.float32)).reshape(len(cs) * nph, ncell), device=dev)
        if p.tt_interp:
            node, frac = p.ev_cell
            ev_node, ev_frac = torch.tensor(node), torch.tensor(frac)
        elif inp["hyp"] is not None:
            h = inp["hyp"][cs].astype(np.int64)
            node = ((h[:, :, 2] * p.ny + h[:, :, 1]) * p.nx + h[:, :, 0]).astype(np.int32)
            ev_node, ev_frac = torch.tensor(np.repeat(node, nph, axis=0)), None      # a row per model
        else:
            ev_node, ev_frac = torch.tensor(p.ev_node), None
        fwd = bs.solve(src, slow, ev_node=ev_node, want_fields=True, ev_frac=ev_frac)
        ttab = fwd["ttab"].cpu().numpy().reshape(len(cs), nph, nstat, nev)
        ev_w = np.zeros((len(cs), nph, nstat, nev), np.float64)
        for i, c in enumerate(cs):
            dte = logl_pick_grad(p, ttab[i], inp["var"][c], inp["tcorr"][c])
            for e in range(nev):
                for j in range(int(p.obs_ptr[e]), int(p.obs_ptr[e + 1])):
                    if not p.obs_mask[j]:
                        ev_w[i, p.obs_phase[j], p.obs_stat[j], e] += dte[j]
            ll = logl_picks(p, ttab[i], inp["var"][c], inp["tcorr"][c])
            for term in inp["norm"][c]:
                ll = ll - float(term)
            logl[k0 + i] = ll
        adj = bs.adjoint(src, slow, fwd["u"], ev_node, torch.tensor(ev_w.reshape(-1, nev)), ev_frac=ev_frac,
                         skip=torch.tensor(p.skip))
        if int(adj["status"].max()) != 0:
            raise RuntimeError("logl_grad: an adjoint solve did not converge within maxit")
        g = adj["grad"].cpu().numpy().reshape(len(cs), nph * ncell)
        if wrt == "velocity":
            vv = v[cs].reshape(len(cs), nph * ncell).astype(np.float64)
            g = -(g / (vv * vv))
        grad[k0:k0 + len(cs)] = g
    return grad, logl


def bench_picks(p: Problem, sigma=5e-4, device=0):
    """bench.py's observations on `p` (in place): the GPU forward of the true
    model (`picks_from_forward`) plus N(0, sigma) noise drawn with seed
    p.seed + 1, and varObs = sigma^2 -- sigma at the scale one proposal moves
    a travel time (~1 ms for 50 m/s on a 400-m cell), so Metropolis both
    accepts and rejects (DESIGN.md s.7 "Accept rate")."""
    tt = picks_from_forward(device)(p)
    rng = np.random.default_rng(p.seed + 1)
    p.tobs = tt.T.ravel().astype(np.float64) + rng.normal(0.0, sigma, p.nevents * p.nstat)
    p.var[:] = sigma ** 2
    return p


def gather_kept(smp: Sampler, nchains_total, group=None, dst=0, device=None):
    """Checkpoint gather (SURVEY s.8e): the most recent kept state of every
    chain on every rank -> rank `dst`, in global chain order.

    One process per GPU; `smp` holds this rank's shard `shard(nchains_total,
    rank, world)`.  With `device` (a torch CUDA device) the states move as
    device tensors -- over RCCL for an nccl group, xGMI on one node -- else as
    host tensors (gloo).  Shards are padded to the largest one, as gather
    needs equal sizes.  Returns (v [nchains_total, ncell] int32, logl
    [nchains_total] float64) torch tensors on `dst`, (None, None) elsewhere.
    Every chain is gathered; with tempering on, cold = the first G of each
    shard (`cold_chain_ids`)."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    width = -(-nchains_total // world)
    ncell = smp.p.ncell * smp.p.nphase           # a chain's model entries
    if device is not None:
        v = torch.zeros((width, ncell), dtype=torch.int32, device=device)
        lg = torch.zeros((width,), dtype=torch.float64, device=device)
        got = C.c_int(0)
        rc = smp._L.mceik_mcmc_get_samples(smp._h, C.c_void_p(v.data_ptr()), C.c_void_p(lg.data_ptr()), 1, 1,
                                           C.byref(got))
        if rc != 0 or got.value != 1:
            raise RuntimeError("mceik_mcmc_get_samples: no kept state to gather")
    else:
        kv, kl = smp.samples(max_states=1)
        if len(kv) == 0:
            raise RuntimeError("no kept state to gather (max_samples = 0 or still in burn-in)")
        v = torch.zeros((width, ncell), dtype=torch.int32)
        lg = torch.zeros((width,), dtype=torch.float64)
        v[:smp.nchains] = torch.from_numpy(kv[0].reshape(smp.nchains, ncell))
        lg[:smp.nchains] = torch.from_numpy(kl[0])
    gv = [torch.empty_like(v) for _ in range(world)] if rank == dst else None
    gl = [torch.empty_like(lg) for _ in range(world)] if rank == dst else None
    dist.gather(v, gv, dst=dst, group=group)
    dist.gather(lg, gl, dst=dst, group=group)
    if rank != dst:
        return None, None
    parts = [shard(nchains_total, r, world) for r in range(world)]
    return (torch.cat([gv[r][:hi - lo] for r, (lo, hi) in enumerate(parts)]),
            torch.cat([gl[r][:hi - lo] for r, (lo, hi) in enumerate(parts)]))


def comm_ready():
    """(ok, reason) of this process for the library communicator: the library
    loads and RCCL has every entry point it uses (mceik_comm_available).  No
    GPU call."""
    try:
        L = _lib.lib()
    except (OSError, ImportError) as exc:
        return False, f"libmceik_hip.so: {exc}"
    if not L.mceik_comm_available():
        return False, "RCCL (librccl.so.1) cannot be loaded"
    return True, ""


class CommUnavailable(RuntimeError):
    """Raised on EVERY rank alike when some rank cannot build the communicator
    (agreed before the collective mceik_comm_init)."""


class Comm:
    """RCCL communicator of the library's checkpoint gather (include/mceik.h
    mceik_comm_*): one rank per GPU.  `bootstrap` moves the 128-byte id from
    rank 0 to the others (an MPI main uses MPI_Bcast; here any callable
    bytes -> bytes, e.g. over torch.distributed: see `from_torch`).  `agree`
    (world > 1) maps this rank's `comm_ready()` to every rank's, so that all
    ranks give up together, before any of them enters the collective
    mceik_comm_init (which would wait forever for a rank that cannot join)."""

    def __init__(self, rank, world, device, bootstrap=None, agree=None, ready=comm_ready):
        if world > 1 and agree is not None:
            every = agree(ready())
            bad = [(r, why) for r, (ok, why) in enumerate(every) if not ok]
            if bad:
                raise CommUnavailable("; ".join(f"rank {r}: {why}" for r, why in bad))
        L = _lib.lib()
        uid = (C.c_ubyte * 128)()
        mine = None
        if rank == 0 and L.mceik_comm_unique_id(uid) == 0:
            mine = bytes(uid)
        if world > 1:
            mine = bootstrap(mine if rank == 0 else None)     # every rank learns the id, or that there is none
        if mine is None:
            raise RuntimeError("mceik_comm_unique_id failed on rank 0")
        C.memmove(uid, mine, 128)
        h = C.c_void_p()
        if L.mceik_comm_init(uid, int(world), int(rank), int(device), C.byref(h)) != 0:
            raise RuntimeError("mceik_comm_init failed")
        self._h, self._L, self.rank, self.world = h, L, rank, world

    @classmethod
    def from_torch(cls, device, group=None, ready=comm_ready):
        """Bootstrap (and the readiness agreement) over an initialised
        torch.distributed group."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)

        def bcast(b):
            box = [b]
            dist.broadcast_object_list(box, src=0, group=group)
            return box[0]

        def agree(mine):
            every = [None] * world
            dist.all_gather_object(every, mine, group=group)
            return every
        return cls(rank, world, device, bcast, agree, ready)

    def gather(self, smp: Sampler, nchains_total, which=1, root=0, v_out=None, logl_out=None):
        """mceik_mcmc_gather: every rank's chains -> `root` in global chain order.
        which 0 = current state, 1 = most recent kept state.  v_out / logl_out:
        torch tensors (device: received in place) or numpy arrays on the root;
        by default the root gets host numpy arrays.  Returns (v, logl) on the
        root, (None, None) elsewhere.  Every chain is gathered; with tempering
        on, cold = the first G of each shard (`cold_chain_ids`)."""
        is_root = self.rank == root
        if is_root and v_out is None:
            v_out = np.empty((nchains_total,) + smp.model_shape[1:], np.int32)
            logl_out = np.empty(nchains_total, np.float64) if logl_out is None else logl_out

        def ptr(a):
            if a is None or not is_root:
                return None
            return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
        rc = self._L.mceik_mcmc_gather(smp._h, self._h, int(which), int(nchains_total), int(root),
                                       ptr(v_out), ptr(logl_out))
        if rc != 0:
            raise RuntimeError(f"mceik_mcmc_gather failed ({rc})")
        return (v_out, logl_out) if is_root else (None, None)

    def close(self):
        if self._h:
            self._L.mceik_comm_finalize(C.byref(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
