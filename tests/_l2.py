"""The L2 grid searches restated with numpy, one IEEE operation per line, next
to the reference's own loops:

locate.c:923-1203 (locate_l2_gridSearch__double64 / __float64), the used picks
j (mask == 0) in catalogue order:

    tc_j = tobs_j - tcorr_j  (tobs_j without tcorr)      wt_j = 1 / var_j
    xnorm = 0;  for j: xnorm = xnorm + wt_j
    t0 = 0;     for j: w = wt_j / xnorm;    t0 = t0 + w * (tc_j - test_j)       (iwantOT == 1, else t0 = t0use)
    objfn = 0;  for j: w = wt_j * sqrt(1/2); res = w * (tc_j - (test_j + t0));  objfn = objfn + res * res

gridsearch.f90:176-540 (locate3d_gridsearch__double64 / __float64), the used
picks i (mask != 1) in order:

    xnorm = 0;  for i: xnorm = xnorm + var_i
    t0 = 0;     for i: wt = 1 / (var_i * xnorm);   t0 = t0 + wt * (tobs_i - test_i)    (iwantOT == 1, else t0 = 0)
    logPDF = 0; for i: wt = (1 / sqrt(2)) / var_i; res = wt * (tobs_i - (test_i + t0)); logPDF = logPDF + res * res

test_j is row j of the tables over the grid points, an array of `dtype`; every
line above is one elementwise numpy operation on such arrays, so each step is
one correctly rounded operation and nothing is fused.  mceik_relocate is the
fp32 locate.c form per event, the rows picked from shared tables."""
import numpy as np

SQRT2I = 0.7071067811865475                     # locate.c's constant; rounded to fp32 where dtype is


def _quiet():
    return np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def _l2_event(tc, wt, rows, iwantOT, t0use, ngrd, dtype):
    """The two loops of locate.c over the used picks: tc, wt scalars of dtype, rows arrays [ngrd] of dtype."""
    with _quiet():
        xnorm = dtype(0)
        for w in wt:
            xnorm = dtype(xnorm + w)
        if iwantOT == 1:
            t0 = np.zeros(ngrd, dtype)
            for j in range(len(tc)):
                w = dtype(wt[j] / xnorm)
                d = tc[j] - rows[j]
                p = w * d
                t0 = t0 + p
        else:
            t0 = np.full(ngrd, dtype(t0use), dtype)
        sqrt2i = dtype(SQRT2I)
        obj = np.zeros(ngrd, dtype)
        for j in range(len(tc)):
            w = dtype(wt[j] * sqrt2i)
            est = rows[j] + t0
            d = tc[j] - est
            res = w * d
            sq = res * res
            obj = obj + sq
    assert t0.dtype == dtype and obj.dtype == dtype
    return t0, obj


def gridsearch(ldgrd, ngrd, iwantOT, t0use, mask, tobs, tcorr, varobs, test, dtype=np.float64):
    """locate_l2_gridSearch__double64 (dtype float64) / __float64 (float32): (t0, objfn) [ngrd]."""
    dtype = np.dtype(dtype).type
    test = np.asarray(test, dtype).reshape(-1, ldgrd)
    tobs, varobs = np.asarray(tobs, dtype), np.asarray(varobs, dtype)
    tcorr = None if tcorr is None else np.asarray(tcorr, dtype)
    tc, wt, rows = [], [], []
    with _quiet():
        for j in range(len(tobs)):
            if mask[j] != 0:
                continue
            tc.append(tobs[j] if tcorr is None else dtype(tobs[j] - tcorr[j]))
            wt.append(dtype(dtype(1) / varobs[j]))
            rows.append(test[j, :ngrd])
    return _l2_event(tc, wt, rows, iwantOT, t0use, ngrd, dtype)


def gridsearch_f90(ldgrd, ngrd, iwantOT, mask, tobs, varobs, test, dtype=np.float64):
    """locate3d_gridsearch__double64 / __float64: logPDF [ngrd] (and t0 [ngrd], which the entry point keeps to itself).
    mask == 1 is masked, any other value is used."""
    dtype = np.dtype(dtype).type
    test = np.asarray(test, dtype).reshape(-1, ldgrd)
    tobs, varobs = np.asarray(tobs, dtype), np.asarray(varobs, dtype)
    use = [i for i in range(len(tobs)) if mask[i] != 1]
    with _quiet():
        t0 = np.zeros(ngrd, dtype)
        if iwantOT == 1:
            xnorm = dtype(0)
            for i in use:
                xnorm = dtype(xnorm + varobs[i])
            for i in use:
                wt = dtype(dtype(1) / dtype(varobs[i] * xnorm))
                d = tobs[i] - test[i, :ngrd]
                p = wt * d
                t0 = t0 + p
        sqrt2i = dtype(dtype(1) / np.sqrt(dtype(2)))
        lp = np.zeros(ngrd, dtype)
        for i in use:
            wt = dtype(sqrt2i / varobs[i])
            est = test[i, :ngrd] + t0
            d = tobs[i] - est
            res = wt * d
            sq = res * res
            lp = lp + sq
    assert t0.dtype == dtype and lp.dtype == dtype
    return lp, t0


def relocate(tables, events, ngrd, iwantOT=1, t0use=0.0, log_pdf=True):
    """mceik_relocate in fp32: (out, t0) [nev, ngrd]; out = -objfn if log_pdf.  events as eikonal.relocate takes them."""
    f = np.float32
    tables = np.asarray(tables, f)
    out, t0s = np.zeros((len(events), ngrd), f), np.zeros((len(events), ngrd), f)
    for e, ev in enumerate(events):
        m, tcorr = ev.get("mask"), ev.get("tcorr")
        tc, wt, rows = [], [], []
        with _quiet():
            for i, r in enumerate(ev["rows"]):
                if m is not None and m[i] != 0:
                    continue
                to = f(ev["tobs"][i])
                tc.append(to if tcorr is None else f(to - f(tcorr[i])))
                wt.append(f(f(1) / f(ev["varobs"][i])))
                rows.append(tables[r, :ngrd])
        t0, o = _l2_event(tc, wt, rows, iwantOT, t0use, ngrd, f)
        out[e], t0s[e] = (-o if log_pdf else o), t0
    return out, t0s
