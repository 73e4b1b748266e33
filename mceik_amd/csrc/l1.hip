// l1.hip -- the L1 (Laplace) grid search with the weighted-median origin time
// on gfx950, and its C-ABI: locate_l1_gridSearch__double64 (locate.c:1205-1335),
// mceik_relocate_l1 and weightedMedian__double (declared at locate.c:73 and
// defined nowhere in the reference).  The arithmetic is l1.h's; DESIGN.md s.23.
//
// Kernel: lanes run along grid points (the [row][ldgrd] table reads are
// coalesced), one 64-lane block per 64 points and event.  The cost is the
// (k, j) pair loop of the median, n^2 per point, so the tables are read once:
// a lane forms its n residuals x_j = tc_j - test[row_j][g] and keeps them in a
// column of LDS of its own ([n][64]: lane = bank pair, no conflicts, no
// barrier -- nobody else reads the column).  The pair loop then reads x_j from
// LDS once per L1_KB candidates, w_j / tc_j / rows stay wave-uniform (scalar
// loads), and the body is compare / select / add.  An event with more picks
// than the LDS column holds re-forms x_j from global memory: the same fp
// operation on the same operands, hence the same bits.
//
// Deviations from locate.c:1205-1335, where it is undefined or broken:
//   - with masked picks its wtsum reads unwritten weights and obsPtr[iobs] =
//     iobs indexes the wrong table rows: the used observations are compacted
//     (row = the observation's own index), W is the sum of their weights;
//   - its stray printf of the sort count is left out;
//   - argument checks, messages and return codes are those of
//     locate_l2_gridSearch__double64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/mceik.h"
#include "l1.h"

#define L1_LANES 64
#define L1_LDS_BYTES 16384         // a block's residual tile: 32 fp64 / 64 fp32 picks per lane

namespace {

template <typename T, bool LIST>
__global__ __launch_bounds__(L1_LANES) void l1_gridsearch_kernel(int ldgrd, int ngrd, int nuse, int nrows, int iwantOT,
                                                                 T t0use, const int *__restrict__ ev_ptr,
                                                                 const int *__restrict__ row,
                                                                 const T *__restrict__ tc, const T *__restrict__ wt,
                                                                 const T *__restrict__ test, T *t0, T *objfn,
                                                                 int negate)
{
    constexpr int CAP = L1_LDS_BYTES / (L1_LANES * (int)sizeof(T));
    __shared__ T tile[CAP * L1_LANES];
    const int lane = threadIdx.x, g = blockIdx.x * L1_LANES + lane;
    if (g >= ngrd) return;
    const int e = LIST ? (int)blockIdx.y : 0;
    const int j0 = LIST ? ev_ptr[e] : 0, j1 = LIST ? ev_ptr[e + 1] : nuse;
    const size_t o = (size_t)e * ldgrd + g;
    if (nrows > 0) {
        // a row outside the tables: NaN, and nothing is read through it
        bool bad = false;
        for (int j = j0; j < j1; j++) bad |= (unsigned)row[j] >= (unsigned)nrows;
        if (bad) {
            if (t0) t0[o] = (T)__builtin_nanf("");
            objfn[o] = (T)__builtin_nanf("");
            return;
        }
    }
    auto used = [](int) -> bool { return true; };
    auto w_of = [&](int j) -> T { return wt[j]; };
    auto x_mem = [&](int j) -> T { return tc[j] - test[(size_t)ldgrd * row[j] + g]; };
    T t = t0use, obj;
    if (j1 - j0 <= CAP) {
        T *col = tile + lane;
        for (int j = j0; j < j1; j++) col[(j - j0) * L1_LANES] = x_mem(j);
        auto x_lds = [&](int j) -> T { return col[(j - j0) * L1_LANES]; };
        if (iwantOT == 1) t = l1::median<T>(j0, j1, used, x_lds, w_of, nullptr);
        obj = l1::objective<T>(j0, j1, used, x_lds, w_of, t);
    } else {
        if (iwantOT == 1) t = l1::median<T>(j0, j1, used, x_mem, w_of, nullptr);
        obj = l1::objective<T>(j0, j1, used, x_mem, w_of, t);
    }
    if (t0) t0[o] = t;
    objfn[o] = negate ? -obj : obj;
}

}  // namespace

hipError_t l1_gridsearch(int ldgrd, int ngrd, int nuse, int iwantOT, double t0use, const int *row, const double *tc,
                         const double *wt, const double *test, double *t0, double *objfn, hipStream_t st)
{
    hipLaunchKernelGGL((l1_gridsearch_kernel<double, false>), dim3((ngrd + L1_LANES - 1) / L1_LANES), dim3(L1_LANES), 0,
                       st, ldgrd, ngrd, nuse, 0, iwantOT, t0use, nullptr, row, tc, wt, test, t0, objfn, 0);
    return hipGetLastError();
}

hipError_t l1_gridsearch_f32(int ldgrd, int ngrd, int nev, int nrows, int iwantOT, float t0use, const int *ev_ptr,
                             const int *obs_row, const float *tc, const float *wt, const float *test, float *t0,
                             float *objfn, int negate, hipStream_t st)
{
    if (nev > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((l1_gridsearch_kernel<float, true>), dim3((ngrd + L1_LANES - 1) / L1_LANES, nev), dim3(L1_LANES),
                       0, st, ldgrd, ngrd, 0, nrows, iwantOT, t0use, ev_ptr, obs_row, tc, wt, test, t0, objfn, negate);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// weightedMedian__double (locate.c:73): the lower weighted median of x with
// weights w (l1.h), host code.  perm: the indices in ascending (value, index)
// order; *lsort: that order differs from perm on entry; *ierr = 1 (and 0.0
// returned) for n < 1 or a null x / w.
extern "C" double weightedMedian__double(const int n, const double *x, const double *w, int *perm, bool *lsort,
                                         int *ierr)
{
    if (n < 1 || !x || !w) {
        if (ierr) *ierr = 1;
        return 0.0;
    }
    if (ierr) *ierr = 0;
    if (perm) {
        std::vector<int> p((size_t)n);
        for (int i = 0; i < n; i++) p[i] = i;
        std::stable_sort(p.begin(), p.end(), [&](int a, int b) { return x[a] < x[b]; });
        bool diff = false;
        for (int i = 0; i < n; i++) { diff = diff || perm[i] != p[i]; perm[i] = p[i]; }
        if (lsort) *lsort = diff;
    } else if (lsort) {
        *lsort = false;
    }
    return l1::median<double>(0, n, [](int) { return true; }, [&](int j) { return x[j]; },
                              [&](int j) { return w[j]; }, nullptr);
}

// The event objective on host arrays (mask may be NULL): mceik_amd.mcmc.l1_event.
extern "C" int mceik_l1_event(int n, const int *mask, const double *x, const double *w, double *t0, double *obj)
{
    if (n < 0 || (n > 0 && (!x || !w)) || !obj) return 1;
    *obj = l1::event<double>(0, n, [&](int j) { return !mask || !mask[j]; }, [&](int j) { return x[j]; },
                             [&](int j) { return w[j]; }, t0);
    return 0;
}

// ---------------------------------------------------------------------------
// locate_l1_gridSearch__double64 drop-in (locate.c:1205-1335).
extern "C" int locate_l1_gridSearch__double64(int ldgrd, int ngrd, int nobs, int iwantOT, double t0use,
                                              const int *mask, const double *tobs, const double *varobs,
                                              const double *test, double *t0, double *objfn)
{
    const char *fcnm = "locate_l1_gridSearch__double64";
    if ((sizeof(double) * (size_t)ldgrd) % 64 != 0 || ldgrd < ngrd || nobs < 1 || !mask || !tobs ||
        !varobs || !test || !t0 || !objfn) {
        if ((sizeof(double) * (size_t)ldgrd) % 64 != 0) printf("%s: Error ldgrd must be divisible by 64\n", fcnm);
        if (ldgrd < ngrd) printf("%s: Error ldgrd < ngrd\n", fcnm);
        if (!mask) printf("%s: mask is null\n", fcnm);
        if (!tobs) printf("%s: tobs is null\n", fcnm);
        if (!varobs) printf("%s: varobs is null\n", fcnm);
        if (!test) printf("%s: test is null\n", fcnm);
        if (!t0) printf("%s: t0 is null\n", fcnm);
        if (!objfn) printf("%s: objfn is null\n", fcnm);
        return 1;
    }
    if (((uintptr_t)t0 % 64) || ((uintptr_t)test % 64) || ((uintptr_t)objfn % 64)) {
        printf("%s: Input arrays are not 64 bit aligned\n", fcnm);
        return 1;
    }
    std::vector<int> row;
    std::vector<double> tc, wt;
    double wtsum = 0.0;
    for (int i = 0; i < nobs; i++) {
        if (mask[i] != 0) continue;
        row.push_back(i);
        tc.push_back(tobs[i]);
        wt.push_back(1.0 / varobs[i]);
        wtsum = wtsum + wt.back();
    }
    const int nuse = (int)row.size();
    // (locate.c:1261-1268: with the origin time wanted the weights are normalised unless they already are)
    if (iwantOT == 1 && fabs(wtsum - 1.0) > 1.e-14) {
        const double wtsumi = 1.0 / wtsum;
        for (int j = 0; j < nuse; j++) wt[j] = wt[j] * wtsumi;
    }
    int *d_row = nullptr;
    double *d_tc = nullptr, *d_wt = nullptr, *d_test = nullptr, *d_t0 = nullptr, *d_obj = nullptr;
    int rc = 1;
    const size_t tb = (size_t)ldgrd * nobs * 8;
    if (hipMalloc(&d_row, (nuse + 1) * 4) != hipSuccess || hipMalloc(&d_tc, (nuse + 1) * 8) != hipSuccess ||
        hipMalloc(&d_wt, (nuse + 1) * 8) != hipSuccess || hipMalloc(&d_test, tb) != hipSuccess ||
        hipMalloc(&d_t0, (size_t)ngrd * 8 + 8) != hipSuccess || hipMalloc(&d_obj, (size_t)ngrd * 8 + 8) != hipSuccess)
        goto out;
    if (nuse) {
        if (hipMemcpy(d_row, row.data(), nuse * 4, hipMemcpyHostToDevice) != hipSuccess) goto out;
        if (hipMemcpy(d_tc, tc.data(), nuse * 8, hipMemcpyHostToDevice) != hipSuccess) goto out;
        if (hipMemcpy(d_wt, wt.data(), nuse * 8, hipMemcpyHostToDevice) != hipSuccess) goto out;
    }
    if (hipMemcpy(d_test, test, tb, hipMemcpyHostToDevice) != hipSuccess) goto out;
    if (ngrd > 0) {
        if (l1_gridsearch(ldgrd, ngrd, nuse, iwantOT, t0use, d_row, d_tc, d_wt, d_test, d_t0, d_obj, nullptr) != hipSuccess)
            goto out;
        if (hipMemcpy(t0, d_t0, (size_t)ngrd * 8, hipMemcpyDeviceToHost) != hipSuccess) goto out;
        if (hipMemcpy(objfn, d_obj, (size_t)ngrd * 8, hipMemcpyDeviceToHost) != hipSuccess) goto out;
    }
    rc = 0;
out:
    hipFree(d_row); hipFree(d_tc); hipFree(d_wt); hipFree(d_test); hipFree(d_t0); hipFree(d_obj);
    if (rc) printf("%s: device failure\n", fcnm);
    return rc;
}

// Relocation grid search of many events under the L1 objective: the sampler's
// convention (raw weights wt = 1/var, the weighted-median origin time) in fp32,
// on mceik_relocate's batch as it is (xnorm is ignored and may be NULL).
extern "C" int mceik_relocate_l1(const mceik_relocate_batch *b, void *stream)
{
    if (!b || b->ngrd < 1 || b->ldgrd < b->ngrd || b->nev < 1 || !b->tables || !b->ev_ptr || !b->obs_row ||
        !b->tc || !b->wt || !b->out) {
        fprintf(stderr, "mceik_relocate_l1: invalid batch description\n");
        return 1;
    }
    return l1_gridsearch_f32(b->ldgrd, b->ngrd, b->nev, b->nrows > 0 ? b->nrows : 0, b->iwantOT, b->t0use, b->ev_ptr,
                             b->obs_row, b->tc, b->wt, b->tables, b->t0, b->out, b->log_pdf ? 1 : 0,
                             (hipStream_t)stream) != hipSuccess;
}
