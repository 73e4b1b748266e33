"""CPU restatement of the differential-evolution step of the GPU sampler,
DESIGN.md s.21 operation by operation (the checker of mceik_mcmc_de_*; imported
only by tests/).  The proposal is integer arithmetic (Python ints: no overflow
to think about); the accept test is IEEE doubles without contraction.  The GPU
results are compared bit for bit.

The forward and the logL are the oracle's, through tests/_lang.state_eval (its
gradient is not used); the Philox rounds are transcribed here, so that the
library's host helpers can be checked against an independent statement."""
import numpy as np

import _lang as LG
from mceik_amd import mcmc

STREAM = 5
M32 = 0xFFFFFFFF


def philox(ctr, key):
    """Philox4x32-10: counter [4], key [2] -> four 32-bit words."""
    c0, c1, c2, c3 = (int(x) & M32 for x in ctr)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def words(seed, gchain, gs, w3):
    """The words of the step draw (w3 = 0xFFFFFFFF) or of cells 4 w3 .. 4 w3 + 3."""
    return philox([gs & M32, gs >> 32, STREAM, w3], [gchain, seed])


def pair(r, nb):
    """The ordered pair (i, j), i != j in [0, nb), of the step draw's words r."""
    i = (r[0] * nb) >> 32
    j = (r[1] * (nb - 1)) >> 32
    j += j >= i
    return (j, i) if r[2] & 1 else (i, j)


def draw(seed, gchain, gs, nb):
    """mceik_de_draw: (i, j, log u)."""
    r = words(seed, gchain, gs, M32)
    i, j = pair(r, nb)
    return i, j, LG.det_log((float(r[3]) + 0.5) * (1.0 / 4294967296.0))


def delta(gq, d, w, crq):
    """mceik_de_delta: the move of a cell whose partners differ by d under word w."""
    if (w >> 16) >= crq:
        return 0
    return (2 * gq * int(d) + 2 * (w & 0xFFFF) + 1) >> 17       # (Python's >> floors, as an arithmetic shift does)


def cell_words(seed, gchain, gs, ncell):
    """The word of every cell 0 .. ncell - 1: word n & 3 of counter n >> 2."""
    out = []
    for q in range((ncell + 3) // 4):
        out += words(seed, gchain, gs, q)
    return out[:ncell]


def propose(v, va, vb, w, gq, crq, vlo, vhi, box="reject"):
    """(v', inbox, delta) of one phase model.  box = "reject": a cell outside
    [vlo, vhi] rejects the whole move (the definition).  box = "clamp": such a
    cell is clamped to the box instead -- NOT symmetric; the host test's control."""
    dl = [delta(gq, int(a) - int(b), int(x), crq) for a, b, x in zip(va, vb, w)]
    vp = [int(x) + d for x, d in zip(v, dl)]
    inbox = all(vlo <= x <= vhi for x in vp)
    if box == "clamp":
        vp = [min(max(x, vlo), vhi) for x in vp]
        inbox = True
    return vp, inbox, dl


def plan(gs, every, offset, nphase):
    """(k, par, ph) of DE step gs."""
    assert gs % every == offset
    k = (gs - offset) // every
    return k, k & 1, (k >> 1) % max(1, nphase)


def step(p, v, logl, gs, opts, ntemps=1, chain_offset=0, beta=None, prior=None, var=None, tcorr=None, norm=None,
         hyp=None, precision=32):
    """One DE step of the whole sampler from the state before it.  v [nchains,
    nphase, ncell] (or [nchains, ncell]) int, logl [nchains]; opts = (every,
    offset, gq, crq); beta [nchains] or None; prior = (ws [2], wd [2], vref or
    None) or None; var, tcorr [nchains, nobs], norm [nchains, nphase], hyp
    [nchains, nev, 3] or None each.  Returns a dict of per-chain lists / arrays:
    what mceik_mcmc_de_last reports, delta, and v, logl afterwards."""
    every, offset, gq, crq = opts
    nph, nc = max(1, p.nphase), p.ncell
    v = np.asarray(v, np.int64).reshape(-1, nph, nc)
    nch = v.shape[0]
    k, par, ph = plan(int(gs), every, offset, nph)
    movers, partners = mcmc.de_movers(nch, ntemps, k)
    vlo, vhi = (p.vsmin, p.vsmax) if ph else (p.vmin, p.vmax)
    out = {"k": k, "par": par, "phase": ph, "mover": np.zeros(nch, np.int32), "a": np.full(nch, -1, np.int32),
           "b": np.full(nch, -1, np.int32), "inbox": np.zeros(nch, np.int32), "nmove": np.zeros(nch, np.int32),
           "status": np.zeros(nch, np.int32), "logl_prop": np.zeros(nch), "accept": np.zeros(nch, np.uint8),
           "delta": np.zeros((nch, nc), np.int64), "v": v.copy(), "logl": np.array(logl, np.float64)}
    for c in movers:
        g = chain_offset + c
        ps = partners[c]
        i, j, logu = draw(p.seed, g, int(gs), len(ps))
        a, b = ps[i], ps[j]
        vp, inbox, dl = propose(v[c, ph], v[a, ph], v[b, ph], cell_words(p.seed, g, int(gs), nc), gq, crq, vlo, vhi)
        out["mover"][c], out["a"][c], out["b"][c], out["inbox"][c] = 1, a, b, int(inbox)
        out["nmove"][c] = sum(1 for d in dl if d)
        out["delta"][c] = dl
        lold = float(logl[c])
        out["logl_prop"][c] = lold
        if not inbox:
            continue
        vn = v[c].copy()
        vn[ph] = vp
        q = LG.at_positions(p, None if hyp is None else hyp[c])
        _, ln = LG.state_eval(q, vn, None if var is None else var[c], None if tcorr is None else tcorr[c],
                              None if norm is None else norm[c], precision)
        if prior is not None:
            ws, wd, vref = prior
            vr = None if vref is None else np.asarray(vref, np.int32).reshape(nph, nc)[ph]
            e0 = mcmc.prior_energy(p, v[c, ph].astype(np.int32), vr)
            e1 = mcmc.prior_energy(p, vn[ph].astype(np.int32), vr)
            dlp = -(ws[ph] * float(int(e1[0]) - int(e0[0])) + wd[ph] * float(int(e1[1]) - int(e0[1])))
            logu = logu - dlp
        d = ln - lold
        acc = logu < (float(beta[c]) * d if beta is not None else d)
        out["logl_prop"][c], out["accept"][c] = ln, int(acc)
        if acc:
            out["v"][c], out["logl"][c] = vn, ln
    return out
