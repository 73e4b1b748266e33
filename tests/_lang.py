"""CPU restatement of the discrete Langevin step of the GPU sampler, DESIGN.md
s.18 operation by operation (the checker of mceik_mcmc_lang_*; imported only by
tests/).  Python floats are IEEE doubles and nothing here contracts, every sum
is explicit and sequential: the GPU results are compared bit for bit.

Built from tests/_adjoint.cpu_logl_grad (the fp32 twin's fields, the pick
weights, the adjoint's restatement), the oracle's forward and the sampler's
logL on the host (mcmc.logl_picks), and a transcription of the definition."""
import copy
import struct

import numpy as np

import _adjoint as A
import _oracle as O
from mceik_amd import mcmc

LOG2E = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
FACT = [6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0, 1.0]
STREAM = 4


def det_exp(x):
    """k = round-half-away(x log2 e), r = (x - k LN2_HI) - k
    LN2_LO, Taylor degree 13 in Horner form, times 2^k from its bits."""
    x = float(x)
    if x < -708.0:
        return 0.0
    if x > 709.0:
        return float("inf")
    if x != x:
        return x
    t = x * LOG2E
    k = int(t - 0.5) if t < 0.0 else int(t + 0.5)
    dk = float(k)
    r = (x - dk * LN2_HI) - dk * LN2_LO
    p = 1.0 / FACT[0]
    for f in FACT[1:]:
        p = p * r + 1.0 / f
    p = p * r + 1.0
    return p * struct.unpack("<d", struct.pack("<Q", (k + 1023) << 52))[0]


def det_log(x):
    return O.lib().oracle_det_log(float(x))


def draw(seed, gchain, gs, cell):
    """Philox words of the step draw (cell 0xFFFFFFFF) or of cell `cell`."""
    return O.philox([gs & 0xFFFFFFFF, gs >> 32, STREAM, cell], [gchain, seed])


def support(d, v, vlo, vhi, c, dmax):
    """(lo, hi, a [hi - lo + 1], amax, Z, log Z) of one cell's proposal."""
    lo, hi = max(-dmax, vlo - v), min(dmax, vhi - v)
    hd = 0.5 * float(d)
    a = [hd * float(k) - c * float(k * k) for k in range(lo, hi + 1)]
    amax = a[0]
    for x in a[1:]:
        if x > amax:
            amax = x
    Z = 0.0
    for x in a:
        Z = Z + det_exp(x - amax)
    return lo, hi, a, amax, Z, det_log(Z)


def cell(seed, gchain, gs, i, d, v, vlo, vhi, sigma, dmax):
    """mceik_lang_cell: (delta, lo, logq [hi - lo + 1])."""
    c = 1.0 / (2.0 * sigma * sigma)
    lo, hi, a, amax, Z, lz = support(d, v, vlo, vhi, c, dmax)
    u = (float(draw(seed, gchain, gs, i)[0]) + 0.5) * (1.0 / 4294967296.0)
    target, cum, pick = u * Z, 0.0, hi
    for k, x in enumerate(a):
        w = det_exp(x - amax)
        if cum + w > target:
            pick = lo + k
            break
        cum = cum + w
    return pick, lo, np.array([(x - amax) - lz for x in a])


def reduce256(terms):
    """Partial l of 256 adds terms l, l + 256, .. in order from 0.0; the total
    adds the partials in order from 0.0."""
    part = [0.0] * 256
    for i, t in enumerate(terms):
        part[i % 256] = part[i % 256] + t
    tot = 0.0
    for x in part:
        tot = tot + x
    return tot


def prior_grad(grid, v, vref, ws, wd):
    """gp [ncell] of one phase model: -(ws (double)(2 sum_nb (v_i - v_nb)) + wd
    (double)(2 (v_i - vref_i))), the integers exact."""
    ncx, ncy, ncz = grid
    v = [int(x) for x in np.ravel(v)]
    out = []
    for i, vi in enumerate(v):
        x, y, z = i % ncx, (i // ncx) % ncy, i // (ncx * ncy)
        sn = 0
        for ok, j in ((x > 0, i - 1), (x + 1 < ncx, i + 1), (y > 0, i - ncx), (y + 1 < ncy, i + ncx),
                      (z > 0, i - ncx * ncy), (z + 1 < ncz, i + ncx * ncy)):
            if ok:
                sn += vi - v[j]
        dd = 2 * (vi - int(np.ravel(vref)[i])) if vref is not None else 0
        out.append(-(ws * float(2 * sn) + wd * float(dd)))
    return out


def at_positions(p, hyp):
    """A copy of p whose events sit on the nodes hyp [nev, 3] (a chain's hypocentres)."""
    if hyp is None:
        return p
    q = copy.copy(p)
    q._keep = []
    h = np.asarray(hyp, np.float64)
    q.ex, q.ey, q.ez = p.x0 + h[:, 0] * p.h, p.y0 + h[:, 1] * p.h, p.z0 + h[:, 2] * p.h
    assert np.array_equal(q.ev_node, ((h[:, 2] * p.ny + h[:, 1]) * p.nx + h[:, 0]).astype(np.int32))
    return q


def cpu_logl_grad64(p, v, var=None, tcorr=None):
    """A.cpu_logl_grad for the fp64 sampler: the fp64 twin's fields and tables,
    f = (double)slowness * h; everything else the same."""
    nph, ncell = max(1, p.nphase), p.ncell
    v = np.asarray(v, np.int32).reshape(nph, ncell)
    tt = O.forward_all_f32(O.make_problem(p, 64), v.ravel())
    dte = mcmc.logl_pick_grad(p, tt, var, tcorr)
    ev_w = np.zeros((nph, p.nstat, p.nevents))
    for e in range(p.nevents):
        for j in range(int(p.obs_ptr[e]), int(p.obs_ptr[e + 1])):
            if not p.obs_mask[j]:
                ev_w[p.obs_phase[j], p.obs_stat[j], e] += dte[j]
    out = np.zeros(nph * ncell)
    for ph in range(nph):
        cells = (np.float32(1.0) / v[ph].astype(np.float32)).astype(np.float32)
        s = np.ascontiguousarray(A.expand_cells(cells, p.nx, p.ny, p.nz, p.nref).ravel())
        f = A.forward_f(s, p.h, 64)
        rows = []
        for k in range(p.nstat):
            if p.skip[ph][k]:
                rows.append(np.zeros(ncell))
                continue
            src = (0.0, p.sx[k], p.sy[k], p.sz[k])
            u, ierr, _ = O.eikonal_solve(p.nx, p.ny, p.nz, s.astype(np.float64), p.h, src, p.maxit, p.tol, p.x0, p.y0,
                                         p.z0, np.float64)
            assert ierr == 0
            q = A.adjoint_source(p.nx, p.ny, p.nz, p.ev_node, ev_w[ph, k], None)
            rows.append(A.restate(u, p.nx, p.ny, p.nz, p.h, src, f, q, p.nref, p.x0, p.y0, p.z0)["grad"])
        vv = v[ph].astype(np.float64)
        out[ph * ncell:(ph + 1) * ncell] = -(A.station_sum(rows) / (vv * vv))
    return out, tt


def state_eval(p, v, var=None, tcorr=None, norm=None, precision=32):
    """(d logL / d v [nphase * ncell], logL) of one chain's models: logL is the
    sampler's (the noise terms subtracted in phase order)."""
    if precision == 64:
        g, tt = cpu_logl_grad64(p, v, var, tcorr)
        ll = mcmc.logl_picks(p, tt, var, tcorr)
    else:
        g, ll0 = A.cpu_logl_grad(p, v, var, tcorr)
        tt = O.forward_all_f32(O.make_problem(p), np.asarray(v, np.int32).ravel())
        ll = mcmc.logl_picks(p, tt, var, tcorr)
        if var is None and tcorr is None:
            assert ll == ll0
    for t in (norm if norm is not None else ()):
        ll = ll - float(t)
    return g, ll


def step(p, gchain, gs, v, logl, sigma, dmax, beta=None, prior=None, var=None, tcorr=None, norm=None, hyp=None,
         failed=False, precision=32):
    """One Langevin step of one chain.  v [nphase, ncell] int; prior = (ws [2],
    wd [2], vref [nphase, ncell] or None) or None.  Returns the new v, logL and
    what mceik_mcmc_lang_last reports."""
    nph, nc = max(1, p.nphase), p.ncell
    v = np.asarray(v, np.int64).reshape(nph, nc)
    q = at_positions(p, hyp)
    c = 1.0 / (2.0 * sigma * sigma)
    r = draw(p.seed, gchain, gs, 0xFFFFFFFF)
    ph = (int(r[0]) * nph) >> 32
    logu = det_log((float(r[3]) + 0.5) * (1.0 / 4294967296.0))
    vlo, vhi = (p.vsmin, p.vsmax) if ph else (p.vmin, p.vmax)
    grid = (p.ncx, p.ncy, p.ncz)

    def drift(vv, g):
        gp = [0.0] * nc
        if prior is not None:
            ws, wd, vref = prior
            gp = prior_grad(grid, vv[ph], None if vref is None else np.asarray(vref).reshape(nph, nc)[ph], ws[ph], wd[ph])
        gg = [float(x) for x in g[ph * nc:(ph + 1) * nc]]
        return [(beta * gi if beta is not None else gi) + pi for gi, pi in zip(gg, gp)]

    g0, _ = state_eval(q, v, var, tcorr, norm, precision)
    d0 = drift(v, g0)
    delta, terms = np.zeros(nc, np.int64), []
    for i in range(nc):
        dl, lo, lq = cell(p.seed, gchain, gs, i, d0[i], int(v[ph, i]), vlo, vhi, sigma, dmax)
        delta[i] = dl
        terms.append(float(lq[dl - lo]))
    lqf = reduce256(terms)
    vp = v.copy()
    vp[ph] = v[ph] + delta
    g1, ll1 = state_eval(q, vp, var, tcorr, norm, precision)
    d1 = drift(vp, g1)
    terms = []
    for i in range(nc):
        lo, hi, a, amax, Z, lz = support(d1[i], int(vp[ph, i]), vlo, vhi, c, dmax)
        terms.append((a[-int(delta[i]) - lo] - amax) - lz)
    lqr = reduce256(terms)
    if prior is not None:
        ws, wd, vref = prior
        vr = None if vref is None else np.asarray(vref, np.int32).reshape(nph, nc)[ph]
        e0 = mcmc.prior_energy(p, v[ph].astype(np.int32), vr)
        e1 = mcmc.prior_energy(p, vp[ph].astype(np.int32), vr)
        dlp = -(ws[ph] * float(int(e1[0]) - int(e0[0])) + wd[ph] * float(int(e1[1]) - int(e0[1])))
        logu = logu - dlp
    dl = ll1 - logl
    acc = (not failed) and logu < (beta * dl if beta is not None else dl) + (lqr - lqf)
    return {"v": (vp if acc else v).astype(np.int32), "logl": ll1 if acc else logl, "phase": ph, "delta": delta.astype(np.int32),
            "lqf": lqf, "lqr": lqr, "logl_prop": ll1, "accept": int(acc), "status": int(failed)}
