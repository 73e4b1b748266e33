"""The L2 grid-search kernels (csrc/mcmc_kernels.hip: l2_gridsearch_kernel,
l2_gridsearch_f32_kernel, relocate_lds_kernel<256>, gridsearch_f90_kernel
<double> / <float>) through their four host paths (csrc/locate_dropin.hip), at
the shapes where such kernels go wrong, bit for bit against the numpy
restatement tests/_l2.py -- which tests/test_l2_host.py pins to the compiled
reference's vectors, to the C oracle on these very cases and to a long-double
evaluation.  Output buffers are filled with a sentinel first: nothing at or
past ngrd may be written.  Where the reference is NaN the NaN positions are
compared instead of the bits."""
import ctypes as C

import numpy as np
import pytest

import _l2
import test_l2_host as H

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENT = -7.0
# The launch caps, in blocks of 256 threads: l2_gridsearch() and gridsearch_f90() `if (blocks > 4096)`,
# l2_gridsearch_f32() `if (bx > 2048)` in csrc/mcmc_kernels.hip.  One point more than 256 * cap needs the stride.
CAP64, CAP32, TG = 4096, 2048, 256


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _buf(n, dtype):
    from mceik_amd.eikonal import aligned_empty
    a = aligned_empty(n, dtype)
    a[:] = SENT
    return a


def _untouched(a, ngrd, what):
    assert (a[ngrd:] == SENT).all(), (what, "written at or past ngrd")


# ---------------------------------------------------------------------------
# the drop-ins

def _locate_l2(c, mask, iwantOT, tcorr):
    """locate_l2_gridSearch__double64 / __float64 by c.dtype against the restatement."""
    from mceik_amd.eikonal import locate_l2_gridsearch, locate_l2_gridsearch_f32
    f = locate_l2_gridsearch if c.dtype == np.float64 else locate_l2_gridsearch_f32
    t0, obj = _buf(c.ldgrd, c.dtype), _buf(c.ldgrd, c.dtype)
    what = (c.dtype.__name__, c.ngrd, c.ldgrd, c.nobs, np.asarray(mask).tolist(), iwantOT, tcorr is None)
    assert f(c.ldgrd, c.ngrd, c.nobs, iwantOT, H.T0USE, mask, c.tobs, tcorr, c.varobs, c.test, t0, obj) == 0, what
    wt0, wobj = _l2.gridsearch(c.ldgrd, c.ngrd, iwantOT, H.T0USE, mask, c.tobs, tcorr, c.varobs, c.test, c.dtype)
    H.same(t0[:c.ngrd], wt0, what + ("t0",))
    H.same(obj[:c.ngrd], wobj, what + ("objfn",))
    _untouched(t0, c.ngrd, what)
    _untouched(obj, c.ngrd, what)
    return wt0, wobj


def _said(capfd):
    C.CDLL(None).fflush(None)                    # (the library prints through C stdio)
    return capfd.readouterr().out


def _locate3d(c, mask, iwantOT, capfd=None):
    """locate3d_gridsearch__double64 / __float64 by c.dtype against the restatement; gridsearch.f90:415 refuses a
    catalogue whose mask values sum to nobs (ierr 1, ' ...: No observations', logPDF untouched)."""
    from mceik_amd.eikonal import locate3d_gridsearch
    lp = _buf(c.ldgrd, c.dtype)
    what = (c.dtype.__name__, c.ngrd, c.ldgrd, c.nobs, np.asarray(mask).tolist(), iwantOT)
    if capfd is not None:
        _said(capfd)
    ierr = locate3d_gridsearch(c.ldgrd, c.ngrd, c.nobs, iwantOT, mask, c.tobs, c.varobs, c.test, lp)
    if int(np.sum(mask)) == c.nobs:
        assert ierr == 1, what
        if capfd is not None:
            name = "locate3d_gridsearch_double64" if c.dtype == np.float64 else "locate3d_gridsearch_float64"
            assert _said(capfd) == f" {name}: No observations\n", what
        _untouched(lp, 0, what)
        return None
    assert ierr == 0, what
    wlp, _ = _l2.gridsearch_f90(c.ldgrd, c.ngrd, iwantOT, mask, c.tobs, c.varobs, c.test, c.dtype)
    H.same(lp[:c.ngrd], wlp, what)
    _untouched(lp, c.ngrd, what)
    return wlp


@pytest.mark.parametrize("dtype,mult", [(np.float64, 8), (np.float32, 16)], ids=["double64", "float64"])
@pytest.mark.parametrize("ngrd,ldgrd", H.SHAPES)
def test_locate_l2_gridsearch_small_shapes(ngrd, ldgrd, dtype, mult):
    """1, 2, 3, 4, 5, 12, 33 picks; no mask, first and last masked, all but one masked (all masked with it: t0 = 0 or
    t0use, objfn = 0 as the restatement and the oracle give); iwantOT 1 and 0 with t0use 0.25; tcorr given and NULL."""
    _dev()
    empty = 0
    for c, mask, iwantOT in H.sweep(ngrd, ldgrd, dtype, mult):
        for tcorr in (c.tcorr, None):
            t0, obj = _locate_l2(c, mask, iwantOT, tcorr)
            if mask.all():
                empty += 1
                assert not obj.any() and (t0 == (0.0 if iwantOT else dtype(H.T0USE))).all()
            else:
                assert (obj >= 0).all()
    assert empty == 2 * 2 * 2                    # 1 and 2 picks with the first and the last masked


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double64", "float64"])
@pytest.mark.parametrize("ngrd,ldgrd", H.SHAPES)
def test_locate3d_gridsearch_small_shapes(ngrd, ldgrd, dtype, capfd):
    """The same picks and masks, and a mask value of 2, which counts as used -- except that the sum of the mask
    values decides 'No observations' (3 picks masked 1, 0, 2), as in the reference."""
    _dev()
    refused = 0
    for c, mask, iwantOT in H.sweep(ngrd, ldgrd, dtype, 64, H.MASKS + ("two",)):
        lp = _locate3d(c, mask, iwantOT, capfd)
        refused += lp is None
        assert lp is None or (lp >= 0).all()
    assert refused == 2 * 3                      # 1 and 2 picks 'ends'; 3 picks 'two'; each with iwantOT 1 and 0


# ---------------------------------------------------------------------------
# the grid-stride loops: one point more than threads * cap, two picks

def _stride_case(cap, mult, dtype):
    ngrd = TG * cap + 300
    return H.case(ngrd, H.ld_for(ngrd, mult), 2, seed=1, dtype=dtype)


def test_locate_l2_double64_grid_stride():
    _dev()
    c = _stride_case(CAP64, 8, np.float64)       # (compared whole: the first 300 points of the second stride and the
    _locate_l2(c, np.zeros(2, np.int32), 1, c.tcorr)    # last 300 like all the others)


def test_locate_l2_float64_grid_stride():
    _dev()
    c = _stride_case(CAP32, 16, np.float32)
    _locate_l2(c, np.zeros(2, np.int32), 1, c.tcorr)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["double64", "float64"])
def test_locate3d_gridsearch_grid_stride(dtype):
    _dev()
    _locate3d(_stride_case(CAP64, 64, dtype), np.zeros(2, np.int32), 1)


# ---------------------------------------------------------------------------
# mceik_relocate on the device interface

def _compact(events):
    """The batch arrays mceik_relocate takes (include/mceik_eikonal.h): the used picks of every event in order,
    tc = tobs - tcorr, wt = 1 / var and xnorm = sum wt in fp32."""
    f = np.float32
    ptr, rows, tc, wt, xn = [0], [], [], [], []
    for ev in events:
        m, tcorr, x = ev.get("mask"), ev.get("tcorr"), f(0)
        for i, r in enumerate(ev["rows"]):
            if m is not None and m[i] != 0:
                continue
            to = f(ev["tobs"][i])
            tc.append(to if tcorr is None else f(to - f(tcorr[i])))
            rows.append(int(r))
            with np.errstate(all="ignore"):
                wt.append(f(f(1) / f(ev["varobs"][i])))
                x = f(x + wt[-1])
        xn.append(x)
        ptr.append(len(rows))
    return ptr, rows, tc, wt, xn


def _relocate(tab, events, ngrd, single_pass, log_pdf=True, want_t0=True, iwantOT=1, t0use=0.0):
    """One mceik_relocate launch on sentinel-filled out / t0 [nev, ldgrd] against the restatement.  single_pass: the
    batch states nrows / nobs (the LDS kernel where its budget allows); otherwise the two-pass kernel."""
    from mceik_amd import _lib
    dev = _dev()
    tab = np.ascontiguousarray(tab, np.float32)
    nrows, ld = tab.shape
    nev = len(events)
    ptr, rows, tc, wt, xn = _compact(events)
    t = lambda a, dt: torch.tensor(np.asarray(a if len(a) else [0], dtype=dt), device=dev)
    d_tab, d_ptr, d_rows = torch.tensor(tab, device=dev), t(ptr, np.int32), t(rows, np.int32)
    d_tc, d_wt, d_xn = t(tc, np.float32), t(wt, np.float32), t(xn, np.float32)
    out = torch.full((nev, ld), SENT, dtype=torch.float32, device=dev)
    t0 = torch.full((nev, ld), SENT, dtype=torch.float32, device=dev)
    b = _lib.RelocateBatch()
    b.ldgrd, b.ngrd, b.nev, b.iwantOT, b.t0use = ld, ngrd, nev, iwantOT, t0use
    b.tables, b.ev_ptr, b.obs_row = d_tab.data_ptr(), d_ptr.data_ptr(), d_rows.data_ptr()
    b.tc, b.wt, b.xnorm = d_tc.data_ptr(), d_wt.data_ptr(), d_xn.data_ptr()
    b.t0, b.out, b.log_pdf = (t0.data_ptr() if want_t0 else None), out.data_ptr(), 1 if log_pdf else 0
    if single_pass:
        b.nrows, b.nobs = nrows, len(rows)
    what = (nrows, ngrd, ld, nev, len(rows), single_pass, log_pdf, want_t0, iwantOT)
    assert _lib.lib().mceik_relocate(C.byref(b), C.c_void_p(0)) == 0, what
    torch.cuda.synchronize(dev)
    out, t0 = out.cpu().numpy(), t0.cpu().numpy()
    wout, wt0 = _l2.relocate(tab, events, ngrd, iwantOT, t0use, log_pdf)
    H.same(out[:, :ngrd], wout, what + ("out",))
    _untouched(out.T, ngrd, what)
    if want_t0:
        H.same(t0[:, :ngrd], wt0, what + ("t0",))
    _untouched(t0.T, ngrd if want_t0 else 0, what)
    return wout, wt0


USED = (0, 1, 2, 3, 4, 5, 0, 7, 8, 9, 0)       # used picks per event: every n % 4, an empty event first, amid and last


def _events(nrows=7):
    """Rows repeated within an event and descending; masked picks among the used ones (the empty event in the middle
    has two picks, both masked; the other two have none); every other event with tcorr."""
    g = np.random.default_rng([nrows, 11])
    ev = []
    for e, used in enumerate(USED):
        n = used + (2 if e % 3 == 0 and e not in (0, len(USED) - 1) else 0)
        mask = np.zeros(n, np.int32)
        if n > used:
            mask[g.permutation(n)[:n - used]] = 1
        d = dict(rows=np.sort(g.integers(0, nrows, n))[::-1].tolist(), tobs=g.uniform(0.5, 3.5, n),
                 varobs=g.uniform(0.01, 0.2, n), mask=mask)
        if e % 2:
            d["tcorr"] = g.normal(0.0, 0.01, n)
        assert int((mask == 0).sum()) == used
        ev.append(d)
    assert any(len(set(d["rows"])) < len(d["rows"]) for d in ev) and len(ev[6]["rows"]) == 2
    return ev


@pytest.mark.parametrize("single_pass", [True, False], ids=["lds_single_pass", "two_pass"])
@pytest.mark.parametrize("log_pdf", [True, False])
def test_relocate_pair_loop_tails_and_empty_events(log_pdf, single_pass):
    """ngrd = 300 in ldgrd = 320, 7 table rows, 11 events of 0, 1, 2, 3, 4, 5, 0, 7, 8, 9 and 0 used picks: the
    4-way unrolled pair loops with every tail, group offsets (0, 0, 4, 8, 12, 16, 16, 24, ...) that differ from
    ev_ptr (0, 0, 1, 3, 6, 10, 10, 15, ...).  t0 given and NULL; iwantOT 1, and 0 with t0use 0.125."""
    tab = np.random.default_rng(300).uniform(0.2, 3.0, (7, 320)).astype(np.float32)
    ev = _events()
    out, t0 = _relocate(tab, ev, 300, single_pass, log_pdf)
    for e, used in enumerate(USED):              # an empty event: t0 = 0 and objfn = 0 (as a log-PDF: -0)
        assert used > 0 or not (out[e].any() or t0[e].any())
    assert out[2].any() and out[9].any()
    _relocate(tab, ev, 300, single_pass, log_pdf, want_t0=False)
    out0, t00 = _relocate(tab, ev, 300, single_pass, log_pdf, iwantOT=0, t0use=0.125)
    assert (t00 == np.float32(0.125)).all() and not np.array_equal(out0, out)
    _relocate(tab, ev, 300, single_pass, log_pdf, want_t0=False, iwantOT=0, t0use=0.125)


@pytest.mark.parametrize("single_pass", [True, False], ids=["lds_single_pass", "two_pass"])
def test_relocate_one_row_one_point(single_pass):
    tab = np.array([[1.25, 9.0, 9.0, 9.0]], np.float32)
    ev = [dict(rows=[0], tobs=[2.0], varobs=[0.1]),
          dict(rows=[0] * 5, tobs=[2.0, 2.5, 1.0, 3.0, 2.25], varobs=[0.1, 0.2, 0.05, 0.1, 0.15])]
    _relocate(tab, ev, 1, single_pass)


def test_relocate_two_pass_grid_stride():
    """The fp32 two-pass kernel's stride, batched: 2 events on 2 rows."""
    c = _stride_case(CAP32, 16, np.float32)
    ev = [dict(rows=[1, 0], tobs=c.tobs, varobs=c.varobs), dict(rows=[0, 1], tobs=c.tobs + 0.5, varobs=c.varobs, tcorr=c.tcorr)]
    _relocate(c.test.reshape(2, c.ldgrd), ev, c.ngrd, single_pass=False)


def test_relocate_ngrd_keyword():
    """eikonal.relocate(ngrd=): searches ngrd < ldgrd points; 1 <= ngrd <= ldgrd."""
    from mceik_amd.eikonal import relocate
    dev = _dev()
    tab = np.random.default_rng(301).uniform(0.2, 3.0, (7, 320)).astype(np.float32)
    ev = _events()
    for single_pass in (True, False):
        out, t0 = relocate(torch.tensor(tab, device=dev), ev, ngrd=300, single_pass=single_pass)
        assert tuple(out.shape) == (len(ev), 320)
        wout, wt0 = _l2.relocate(tab, ev, 300)
        H.same(out.cpu().numpy()[:, :300], wout)
        H.same(t0.cpu().numpy()[:, :300], wt0)
    for bad in (0, 321):
        with pytest.raises(ValueError):
            relocate(torch.tensor(tab, device=dev), ev, ngrd=bad)


# ---------------------------------------------------------------------------
# the single-pass kernel's 64 KiB

def _lds_bytes(nrows, nobs, nev):
    """The tables, the observation groups and the nev + 1 group offsets of relocate_lds_kernel<256>; the kernel's
    contract flag comes on top (4 bytes in the dynamic block; 16 static bytes before that)."""
    return nrows * 1024 + ((nobs + 3 * nev + 3) & ~3) * 16 + (nev + 1) * 4


@pytest.mark.parametrize("size,nev,nobs", [(65472, 15, 8), (65524, 12, 21), (65536, 15, 12), (65600, 15, 16)])
def test_relocate_at_the_lds_budget(size, nev, nobs):
    """nrows = 63, ngrd = 300: a batch that fits the 64 KiB with the flag, two within 16 bytes of them (where a
    flag outside the count once took the launch past 64 KiB), one past them.  mceik_relocate serves all four (the
    LDS kernel never with more than 64 KiB -- 65476 and 65528 bytes here -- the two-pass kernel otherwise), with
    the same words."""
    assert _lds_bytes(63, nobs, nev) == size
    g = np.random.default_rng([size, nev, nobs])
    tab = g.uniform(0.2, 3.0, (63, 320)).astype(np.float32)
    ev = []
    for e in range(nev):
        n = nobs // nev + (e < nobs % nev)
        ev.append(dict(rows=g.integers(0, 63, n).tolist(), tobs=g.uniform(0.5, 3.5, n), varobs=g.uniform(0.01, 0.2, n)))
    assert sum(len(d["rows"]) for d in ev) == nobs
    _relocate(tab, ev, 300, single_pass=True)


# ---------------------------------------------------------------------------
# fp32 edges: results in the subnormal range, squares that overflow

@pytest.mark.parametrize("edge", ["subnormal", "overflow"])
def test_fp32_edges(edge):
    """Variances near 1e19 (squared weighted residuals below FLT_MIN: a flush to zero or an approximate division
    would show) and tables near 1e20 (inf); tests/test_l2_host.py asserts that the references hold such values."""
    _dev()
    make = H.subnormal_case if edge == "subnormal" else H.overflow_case
    none = np.zeros(3, np.int32)
    c, f = make(), make(128)
    for iwantOT in (1, 0):
        _, obj = _locate_l2(c, none, iwantOT, None)
        lp = _locate3d(f, none, iwantOT)
        tiny = np.finfo(np.float32).tiny
        for a in (obj, lp):
            assert (((a > 0) & (a < tiny)).any() if edge == "subnormal" else np.isposinf(a).any())
        for single_pass in (True, False):
            _relocate(c.test.reshape(3, c.ldgrd), H.edge_events(c), c.ngrd, single_pass, iwantOT=iwantOT, t0use=H.T0USE)
