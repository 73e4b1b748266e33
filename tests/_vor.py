"""CPU restatement of the transdimensional Voronoi-cell step of the GPU sampler,
DESIGN.md s.22 operation by operation (the checker of mceik_mcmc_vor_*; imported
only by tests/).  Everything up to the accept test is integer arithmetic (Python
ints); the accept test is IEEE doubles without contraction.  The GPU results are
compared bit for bit.

The Philox rounds are tests/_de.py's transcription; the free-cell rule, the
raster and the four moves are stated here independently of the library's host
helpers, which tests/test_vor_host.py checks against them."""
from fractions import Fraction

import numpy as np

import _lang as LG
from _de import philox

STREAM = 6
M32 = 0xFFFFFFFF
VALUE, MOVE, BIRTH, DEATH = 0, 1, 2, 3
TYPES = ("value", "move", "birth", "death")
# (type, reason) of every way a move ends before the accept test
OUTCOMES = [(VALUE, 0), (VALUE, 1), (MOVE, 0), (MOVE, 1), (MOVE, 2), (MOVE, 3), (BIRTH, 0), (BIRTH, 1), (DEATH, 0),
            (DEATH, 1)]


def idx(r, n):
    return (int(r) * int(n)) >> 32


def words(seed, gchain, gs):
    """(a, b): the words of counters {gs, 6, 0} and {gs, 6, 1}."""
    return (philox([gs & M32, gs >> 32, STREAM, 0], [gchain, seed]),
            philox([gs & M32, gs >> 32, STREAM, 1], [gchain, seed]))


def decode(a, b, k, ncell, dv, vlo, vhi, dmax):
    """The draw of a model of k nuclei from its words (every field, as
    mceik_vor_draw reports them; a move type reads its own)."""
    mag = 1 + idx(a[2], dv)
    return {"type": a[0] >> 30, "j": idx(a[1], k), "f": idx(a[1], ncell - k), "delta": -mag if a[0] & 1 else mag,
            "wnew": vlo + idx(a[2], vhi - vlo + 1),
            "d": (idx(a[2], 2 * dmax[0] + 1) - dmax[0], idx(b[0], 2 * dmax[1] + 1) - dmax[1],
                  idx(b[1], 2 * dmax[2] + 1) - dmax[2]), "u": a[3]}


def draw(seed, gchain, gs, k, ncell, dv, vlo, vhi, dmax):
    a, b = words(seed, gchain, gs)
    d = decode(a, b, k, ncell, dv, vlo, vhi, dmax)
    d["logu"] = LG.det_log((float(d["u"]) + 0.5) * (1.0 / 4294967296.0))
    return d


def free_cell(cells, f):
    """The f-th (from 0) cell in ascending order that holds no nucleus."""
    x = int(f)
    for c in sorted(int(c) for c in cells):
        if c > x:
            break
        x += 1
    return x


def start_cells(seed, gchain, ph, k0, ncell):
    """Enable's start nuclei of one phase model: nucleus i sits in free cell
    idx(r0, ncell - i) of counter {i, ph, 6, 0xFFFFFFFF}."""
    cells = []
    for i in range(k0):
        r = philox([i, ph, STREAM, M32], [gchain, seed])
        cells.append(free_cell(cells, idx(r[0], ncell - i)))
    return cells


def raster(grid, cells, vals, metric=(1, 1, 1)):
    """v [ncell] of the nuclei: the nearest in (mx dx)^2 + (my dy)^2 + (mz dz)^2,
    ties to the smaller cell.  int64 throughout."""
    ncx, ncy, ncz = grid
    c = np.asarray(cells, np.int64)
    w = np.asarray(vals, np.int64)
    n = np.arange(ncx * ncy * ncz, dtype=np.int64)
    d2 = np.zeros((n.size, c.size), np.int64)
    for m, (of_n, of_c) in zip(metric, ((n % ncx, c % ncx), (n // ncx % ncy, c // ncx % ncy),
                                        (n // (ncx * ncy), c // (ncx * ncy)))):
        d2 += (int(m) * (of_c[None, :] - of_n[:, None])) ** 2
    key = d2 * (ncx * ncy * ncz) + c[None, :]           # (d2, cell) in one integer: cells < ncell
    return w[np.argmin(key, axis=1)]


def raster_cases(grid, vlo=1500, vhi=9000, kmax=64):
    """(name, cells, vals, metric) of the raster rules on `grid`: one nucleus;
    kmax nuclei; exact ties (cells 0 and 2 tie on cell 1, and on more in y and
    z; 0 and ncell - 1 tie across the middle); a metric other than (1, 1, 1)."""
    ncell = grid[0] * grid[1] * grid[2]
    g = np.random.default_rng([ncell, 5])
    k = min(ncell, kmax)
    many = g.permutation(ncell)[:k]
    return [("k1", [ncell // 3], [vlo + (vhi - vlo) // 3], (1, 1, 1)),
            ("kmax", many, g.integers(vlo, vhi + 1, k), (1, 1, 1)),
            ("ties", [2, 0, ncell - 1], [vlo + 30, vlo + 10, vlo + 20], (1, 1, 1)),
            ("metric112", many[:7], g.integers(vlo, vhi + 1, 7), (1, 1, 2))]


def apply(nuclei, d, kmin, kmax, vlo, vhi, grid):
    """The move of draw d on the list `nuclei` [(cell, value)]: (reason, j, cell,
    value, list') -- reason 0: valid, list' the proposed list; else list' is the
    list unchanged.  value: 1 left the box.  move: 1 zero displacement, 2
    outside the grid, 3 occupied.  birth: 1 k == kmax.  death: 1 k == kmin."""
    ncx, ncy, ncz = grid
    k, t, j = len(nuclei), d["type"], d["j"]
    out = list(nuclei)
    if t == BIRTH:
        if k >= kmax:
            return 1, -1, -1, -1, out
        c = free_cell([x[0] for x in nuclei], d["f"])
        return 0, k, c, d["wnew"], out + [(c, d["wnew"])]
    cj, wj = nuclei[j]
    if t == VALUE:
        w = wj + d["delta"]
        if w < vlo or w > vhi:
            return 1, j, cj, w, out
        out[j] = (cj, w)
        return 0, j, cj, w, out
    if t == MOVE:
        dx, dy, dz = d["d"]
        if dx == 0 and dy == 0 and dz == 0:
            return 1, j, cj, wj, out
        x, y, z = cj % ncx + dx, cj // ncx % ncy + dy, cj // (ncx * ncy) + dz
        if not (0 <= x < ncx and 0 <= y < ncy and 0 <= z < ncz):
            return 2, j, -1, wj, out
        c = (z * ncy + y) * ncx + x
        if any(c == x[0] for x in nuclei):
            return 3, j, c, wj, out
        out[j] = (c, wj)
        return 0, j, c, wj, out
    if k <= kmin:
        return 1, j, cj, wj, out
    out[j] = out[-1]                                    # the last slot moves into j
    return 0, j, cj, wj, out[:-1]


def is_velocity_step(gs, hypo_every=0, nuis=None):
    """plan_step's precedence while Voronoi-cell models are on: hypocentre, else
    nuisance (nuis = (every, offset) while state is held and moves are on), else velocity."""
    if hypo_every > 0 and gs % hypo_every == hypo_every - 1:
        return False
    if nuis is not None and gs % nuis[0] == nuis[1]:
        return False
    return True


def step_phase(gs, nphase, hypo_every=0, nuis=None):
    """The phase of Voronoi step gs: n % nphase, n the velocity steps below gs."""
    return sum(1 for g in range(gs) if is_velocity_step(g, hypo_every, nuis)) % max(1, nphase)


def count_idx(n):
    """How many 32-bit words r give idx(r, n) == i, for every i in [0, n)."""
    lo = [-((-i << 32) // n) for i in range(n + 1)]     # ceil(i 2^32 / n)
    return [lo[i + 1] - lo[i] for i in range(n)]


def draws_with_probability(k, ncell, dv, vlo, vhi, dmax):
    """Every distinct draw a model of k nuclei can get, as (probability,
    draw) with exact probabilities: the share of the words that decode to it.
    Words a move type does not read are summed out."""
    W = 1 << 32
    out = []
    cj, cmag = count_idx(k), count_idx(dv)
    for sign in (0, 1):                                 # a0: the top two bits and bit 0
        for j, nj in enumerate(cj):
            for m, nm in enumerate(cmag):
                mag = 1 + m
                out.append((Fraction(1 << 29, W) * Fraction(nj, W) * Fraction(nm, W),
                            {"type": VALUE, "j": j, "delta": -mag if sign else mag}))
    cd = [count_idx(2 * m + 1) for m in dmax]
    for j, nj in enumerate(cj):
        for ix, nx in enumerate(cd[0]):
            for iy, ny in enumerate(cd[1]):
                for iz, nz in enumerate(cd[2]):
                    out.append((Fraction(1, 4) * Fraction(nj, W) * Fraction(nx, W) * Fraction(ny, W) * Fraction(nz, W),
                                {"type": MOVE, "j": j, "d": (ix - dmax[0], iy - dmax[1], iz - dmax[2])}))
    if ncell - k > 0:
        for f, nf in enumerate(count_idx(ncell - k)):
            for w, nw in enumerate(count_idx(vhi - vlo + 1)):
                out.append((Fraction(1, 4) * Fraction(nf, W) * Fraction(nw, W),
                            {"type": BIRTH, "j": 0, "f": f, "wnew": vlo + w}))
    else:
        out.append((Fraction(1, 4), {"type": BIRTH, "j": 0, "f": 0, "wnew": vlo}))
    for j, nj in enumerate(cj):
        out.append((Fraction(1, 4) * Fraction(nj, W), {"type": DEATH, "j": j}))
    return out


def step(p, cells, vals, counts, logl, gs, ph, opts, logl_prop, chain_offset=0, beta=None):
    """One Voronoi step of every chain on phase ph from the state before it.
    cells, vals [nchains, nphase, kmax], counts [nchains, nphase], logl
    [nchains]; opts = vor_options(); logl_prop [nchains]: logL' of the proposed
    models (the GPU's own; read only for moves that reach the accept test).
    Returns per-chain arrays: what mceik_mcmc_vor_last reports, the proposed
    model of the phase, and nuclei, counts, logl afterwards."""
    grid, nc = (p.ncx, p.ncy, p.ncz), p.ncell
    kmin, kmax, dv, dmax, metric = opts["kmin"], opts["kmax"], opts["dv"], opts["dmax"], opts["metric"]
    vlo, vhi = (p.vsmin, p.vsmax) if ph else (p.vmin, p.vmax)
    nch = len(logl)
    out = {k: np.zeros(nch, np.int32) for k in ("type", "reason", "j", "cell", "value", "k")}
    out.update(logu=np.zeros(nch), accept=np.zeros(nch, np.uint8), logl_prop=np.zeros(nch), vprop=np.zeros((nch, nc), np.int64),
               pcells=[None] * nch, pvals=[None] * nch, cells=np.array(cells), vals=np.array(vals),
               counts=np.array(counts), logl=np.array(logl, np.float64))
    for c in range(nch):
        k = int(counts[c][ph])
        nuclei = [(int(cells[c][ph][i]), int(vals[c][ph][i])) for i in range(k)]
        d = draw(p.seed, chain_offset + c, int(gs), k, nc, dv, vlo, vhi, dmax)
        reason, j, cell, value, prop = apply(nuclei, d, kmin, kmax, vlo, vhi, grid)
        out["type"][c], out["reason"][c], out["j"][c], out["cell"][c], out["value"][c] = d["type"], reason, j, cell, value
        out["k"][c], out["logu"][c] = len(prop), d["logu"]
        out["pcells"][c], out["pvals"][c] = [x[0] for x in prop], [x[1] for x in prop]
        out["vprop"][c] = raster(grid, out["pcells"][c], out["pvals"][c], metric)
        lold = float(logl[c])
        out["logl_prop"][c] = lold
        if reason:
            continue
        ln = float(logl_prop[c])
        dl = ln - lold
        acc = d["logu"] < (float(beta[c]) * dl if beta is not None else dl)
        out["logl_prop"][c], out["accept"][c] = ln, int(acc)
        if acc:
            out["cells"][c, ph, :len(prop)] = out["pcells"][c]
            out["vals"][c, ph, :len(prop)] = out["pvals"][c]
            out["counts"][c, ph] = len(prop)
            out["logl"][c] = ln
    return out
