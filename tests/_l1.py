"""The L1 (Laplace) objective with the weighted-median origin time (csrc/l1.h,
DESIGN.md s.23) restated with numpy, the definition literally:

    W = 0;  for j: W = W + w_j                     half = 0.5 * W
    for k (ascending):
        s = 0;  for j (ascending): s = s + ((x_j < x_k || (x_j == x_k && j <= k)) ? w_j : 0.0)
        if (s >= half && (best == none || x_k < x_best)) best = k
    t0  = x_best
    obj = 0;  for j: obj = obj + w_j * fabs(x_j - t0)

over the used observations j in order; none used: t0 = 0, obj = 0.  x may carry
a trailing axis (one column per grid point): every column is evaluated by the
same elementwise operations, each in `dtype`.  The tables of a model come from
the CPU oracle (tests/_oracle.py) through tests/_fit.py, as in tests/_lang.py."""
import numpy as np


def _cols(x, dtype):
    x = np.asarray(x, dtype)
    assert x.ndim in (1, 2)
    return x[:, None] if x.ndim == 1 else x


def _used(n, mask):
    return [j for j in range(n) if mask is None or not mask[j]]


def median(x, w, mask=None, dtype=np.float64):
    """The lower weighted median of the used rows of x [n] or [n, G]: a scalar or [G]."""
    X = _cols(x, dtype)
    w = np.asarray(w, dtype)
    n, G = X.shape
    js = _used(n, mask)
    best = np.zeros(G, dtype)
    if js:
        W = dtype(0)
        for j in js:
            W = dtype(W + w[j])
        half = dtype(dtype(0.5) * W)
        have = np.zeros(G, bool)
        for k in js:
            s = np.zeros(G, dtype)
            for j in js:
                s = s + np.where((X[j] < X[k]) | ((X[j] == X[k]) & (j <= k)), w[j], dtype(0))
            take = (s >= half) & (~have | (X[k] < best))
            best = np.where(take, X[k], best)
            have |= take
        assert have.all()
    return best[0] if np.ndim(x) <= 1 else best


def objective(x, w, t0, mask=None, dtype=np.float64):
    X = _cols(x, dtype)
    w = np.asarray(w, dtype)
    o = np.zeros(X.shape[1], dtype)
    t0 = np.asarray(t0, dtype)
    for j in _used(X.shape[0], mask):
        o = o + w[j] * np.abs(X[j] - t0)
    return o[0] if np.ndim(x) <= 1 else o


def event(x, w, mask=None, dtype=np.float64):
    """(t0, obj) of one event."""
    t0 = median(x, w, mask, dtype)
    return t0, objective(x, w, t0, mask, dtype)


def perm(x):
    """The indices in ascending (value, index) order."""
    x = np.asarray(x, np.float64)
    return np.array(sorted(range(len(x)), key=lambda i: (x[i], i)), np.int32)


def pick_terms(p, ttab, var=None, tcorr=None):
    """Per event (js, t0, obj, residuals (tc - te) - t0) of the sampler's L1 logL:
    x_j = (tobs_j - tcorr_j) - te_j, w_j = 1 / var_j, the tables widened from fp32."""
    tt = np.asarray(ttab, np.float32).astype(np.float64).reshape(max(1, p.nphase), p.nstat, p.nevents)
    var = np.asarray(p.var if var is None else var, np.float64)
    tcorr = np.asarray(p.tcorr if tcorr is None else tcorr, np.float64)
    mask, phase, stat, ptr = p.obs_mask, p.obs_phase, p.obs_stat, p.obs_ptr
    out = []
    for e in range(p.nevents):
        js = [j for j in range(int(ptr[e]), int(ptr[e + 1])) if not mask[j]]
        x = np.array([(p.tobs[j] - tcorr[j]) - tt[phase[j], stat[j], e] for j in js], np.float64)
        w = np.array([1.0 / var[j] for j in js], np.float64)
        t0, obj = event(x, w)
        out.append((js, float(t0), float(obj), [float(xj - t0) for xj in x]))
    return out


def event_objs(p, ttab, var=None, tcorr=None):
    return np.array([t[2] for t in pick_terms(p, ttab, var, tcorr)], np.float64)


def logl(p, ttab, var=None, tcorr=None, norm_terms=()):
    """logL = ((0 - objfn_0) - objfn_1) - ..., then minus the noise-ladder terms in order."""
    ll = 0.0
    for _, _, obj, _ in pick_terms(p, ttab, var, tcorr):
        ll = ll - obj
    for t in norm_terms:
        ll = ll - float(t)
    return ll


def gridsearch(ldgrd, ngrd, iwantOT, t0use, mask, tobs, varobs, test):
    """locate_l1_gridSearch__double64 as the library defines it: (t0, objfn) [ngrd]."""
    test = np.asarray(test, np.float64).reshape(-1, ldgrd)
    js = [j for j in range(len(tobs)) if mask[j] == 0]
    w = np.array([1.0 / varobs[j] for j in js], np.float64)
    W = 0.0
    for wj in w:
        W = W + float(wj)
    if iwantOT == 1 and js and abs(W - 1.0) > 1.e-14:
        w = w * (1.0 / W)
    x = np.array([tobs[j] - test[j, :ngrd] for j in js], np.float64).reshape(len(js), ngrd)
    t0 = median(x, w) if iwantOT == 1 else np.full(ngrd, t0use, np.float64)
    if iwantOT == 1 and not js:
        t0 = np.zeros(ngrd)
    return np.asarray(t0, np.float64).reshape(ngrd), np.asarray(objective(x, w, t0), np.float64).reshape(ngrd)


def relocate(tables, events, ngrd, iwantOT=1, t0use=0.0, log_pdf=True):
    """mceik_relocate_l1 in fp32: (out, t0) [nev, ngrd]; raw weights 1 / var."""
    f = np.float32
    tables = np.asarray(tables, f)
    out, t0s = np.zeros((len(events), ngrd), f), np.zeros((len(events), ngrd), f)
    for e, ev in enumerate(events):
        m = ev.get("mask")
        js = [i for i in range(len(ev["rows"])) if m is None or m[i] == 0]
        tc = [f(ev["tobs"][i]) - f(ev["tcorr"][i]) if ev.get("tcorr") is not None else f(ev["tobs"][i]) for i in js]
        w = np.array([f(1.0) / f(ev["varobs"][i]) for i in js], f)
        x = np.array([tc[k] - tables[ev["rows"][i], :ngrd] for k, i in enumerate(js)], f).reshape(len(js), ngrd)
        t0 = median(x, w, dtype=f) if iwantOT == 1 else np.full(ngrd, t0use, f)
        if iwantOT == 1 and not js:
            t0 = np.zeros(ngrd, f)
        o = np.asarray(objective(x, w, t0, dtype=f), f).reshape(ngrd)
        out[e], t0s[e] = (-o if log_pdf else o), t0
    return out, t0s
