// locate_dropin.hip -- drop-in location grid searches of the C-ABI
// (include/locate.h locate3d_gridsearch__*, locate_l2_gridSearch__*;
// include/mceik.h mceik_relocate).  Host orchestration only; the kernels live
// in mcmc_kernels.hip.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/mceik.h"
#include "gridsearch.h"

// ---------------------------------------------------------------------------
// locate3d_gridsearch__double64 / __float64 drop-ins (gridsearch.f90:382-540).
template <typename T>
static void gridsearch_f90_dropin(const char *fcnm, const int *ldgrd, const int *ngrd, const int *nobs,
                                  const int *iwantOT, const int *mask, const T *tobs, const T *varobs, const T *test,
                                  T *logPDF, int *ierr)
{
    *ierr = 0;
    if (*ldgrd % 64 != 0) {
        printf(" %s: Require arrays be 64 byte aligned %d %d\n", fcnm, *ldgrd,
               sizeof(T) == 8 ? (8 * *ldgrd) % 64 : *ldgrd % 64);
        *ierr = 1;
        return;
    }
    if (*ngrd > *ldgrd) {
        printf(" %s: ngrd cannot be greater than ldgrd\n", fcnm);
        *ierr = 1;
        return;
    }
    long msum = 0;
    T vsum = (T)0;
    for (int i = 0; i < *nobs; i++) { msum += mask[i]; vsum = vsum + varobs[i]; }
    if (msum == *nobs) {
        printf(" %s: No observations\n", fcnm);
        *ierr = 1;
        return;
    }
    const T eps = sizeof(T) == 8 ? (T)DBL_EPSILON : (T)FLT_EPSILON;
    if ((vsum < (T)0 ? -vsum : vsum) < eps) {
        printf(" %s: Will be division by zero\n", fcnm);
        *ierr = 1;
        return;
    }
    T xnorm = (T)0;
    for (int i = 0; i < *nobs; i++) if (mask[i] != 1) xnorm = xnorm + varobs[i];
    const T one = (T)1, sqrt2i = one / (sizeof(T) == 8 ? (T)sqrt(2.0) : (T)sqrtf(2.0f));
    std::vector<int> row;
    std::vector<T> tob, w0, wl;
    for (int i = 0; i < *nobs; i++) {
        if (mask[i] == 1) continue;
        row.push_back(i);
        tob.push_back(tobs[i]);
        w0.push_back(one / (varobs[i] * xnorm));
        wl.push_back(sqrt2i / varobs[i]);
    }
    const int nuse = (int)row.size();
    const size_t tb = (size_t)*ldgrd * *nobs * sizeof(T);
    char *d = nullptr;
    const size_t a = ((size_t)nuse * 16 + 255) & ~(size_t)255;
    if (hipMalloc(&d, 4 * a + tb + (size_t)*ngrd * sizeof(T) + 64) != hipSuccess) {
        printf(" %s: device allocation failed\n", fcnm);
        *ierr = 1;
        return;
    }
    int *d_row = (int *)d;
    T *d_tob = (T *)(d + a), *d_w0 = (T *)(d + 2 * a), *d_wl = (T *)(d + 3 * a);
    T *d_test = (T *)(d + 4 * a), *d_lp = (T *)(d + 4 * a + tb);
    bool ok = hipMemcpy(d_row, row.data(), nuse * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d_tob, tob.data(), nuse * sizeof(T), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d_w0, w0.data(), nuse * sizeof(T), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d_wl, wl.data(), nuse * sizeof(T), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d_test, test, tb, hipMemcpyHostToDevice) == hipSuccess &&
              gridsearch_f90(sizeof(T) == 8, *ldgrd, *ngrd, nuse, *iwantOT, d_row, d_tob, d_w0, d_wl, d_test, d_lp,
                             nullptr) == hipSuccess &&
              hipMemcpy(logPDF, d_lp, (size_t)*ngrd * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
    hipFree(d);
    if (!ok) {
        printf(" %s: device failure\n", fcnm);
        *ierr = 1;
    }
}

extern "C" void locate3d_gridsearch__double64(const int *ldgrd, const int *ngrd, const int *nobs, const int *iwantOT,
                                              const int *mask, const double *tobs, const double *varobs,
                                              const double *test, double *logPDF, int *ierr)
{
    gridsearch_f90_dropin<double>("locate3d_gridsearch_double64", ldgrd, ngrd, nobs, iwantOT, mask, tobs, varobs,
                                  test, logPDF, ierr);
}

extern "C" void locate3d_gridsearch__float64(const int *ldgrd, const int *ngrd, const int *nobs, const int *iwantOT,
                                             const int *mask, const float *tobs, const float *varobs,
                                             const float *test, float *logPDF, int *ierr)
{
    gridsearch_f90_dropin<float>("locate3d_gridsearch_float64", ldgrd, ngrd, nobs, iwantOT, mask, tobs, varobs,
                                 test, logPDF, ierr);
}

// ---------------------------------------------------------------------------
// locate_l2_gridSearch__double64 drop-in (locate.c:923-1047).
extern "C" int locate_l2_gridSearch__double64(int ldgrd, int ngrd, int nobs, int iwantOT, double t0use,
                                              const int *mask, const double *tobs, const double *tcorr,
                                              const double *varobs, const double *test,
                                              double *t0, double *objfn)
{
    const char *fcnm = "locate_l2_gridSearch__double64";
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
    std::vector<int> use;
    std::vector<double> tc, wt;
    double xnorm = 0.0;
    for (int i = 0; i < nobs; i++) {
        if (mask[i] != 0) continue;
        tc.push_back(tcorr ? tobs[i] - tcorr[i] : tobs[i]);
        use.push_back(i);
        wt.push_back(1.0 / varobs[i]);
        xnorm = xnorm + wt.back();
    }
    int nuse = (int)use.size();
    int *d_use = nullptr;
    double *d_tc = nullptr, *d_wt = nullptr, *d_test = nullptr, *d_t0 = nullptr, *d_obj = nullptr;
    int rc = 1;
    size_t tb = (size_t)ldgrd * nobs * 8;
    if (hipMalloc(&d_use, (nuse + 1) * 4) != hipSuccess || hipMalloc(&d_tc, (nuse + 1) * 8) != hipSuccess ||
        hipMalloc(&d_wt, (nuse + 1) * 8) != hipSuccess || hipMalloc(&d_test, tb) != hipSuccess ||
        hipMalloc(&d_t0, (size_t)ngrd * 8 + 8) != hipSuccess || hipMalloc(&d_obj, (size_t)ngrd * 8 + 8) != hipSuccess)
        goto out;
    if (nuse) {
        hipMemcpy(d_use, use.data(), nuse * 4, hipMemcpyHostToDevice);
        hipMemcpy(d_tc, tc.data(), nuse * 8, hipMemcpyHostToDevice);
        hipMemcpy(d_wt, wt.data(), nuse * 8, hipMemcpyHostToDevice);
    }
    hipMemcpy(d_test, test, tb, hipMemcpyHostToDevice);
    if (l2_gridsearch(ldgrd, ngrd, nuse, iwantOT, t0use, d_use, d_tc, d_wt, xnorm, d_test, d_t0, d_obj, nullptr) != hipSuccess)
        goto out;
    if (hipMemcpy(t0, d_t0, (size_t)ngrd * 8, hipMemcpyDeviceToHost) != hipSuccess) goto out;
    if (hipMemcpy(objfn, d_obj, (size_t)ngrd * 8, hipMemcpyDeviceToHost) != hipSuccess) goto out;
    rc = 0;
out:
    hipFree(d_use); hipFree(d_tc); hipFree(d_wt); hipFree(d_test); hipFree(d_t0); hipFree(d_obj);
    if (rc) printf("%s: device failure\n", fcnm);
    return rc;
}

// ---------------------------------------------------------------------------
// locate_l2_gridSearch__float64 drop-in (locate.c:1079-1203): fp32 arithmetic.
extern "C" int locate_l2_gridSearch__float64(int ldgrd, int ngrd, int nobs, int iwantOT, float t0use,
                                             const int *mask, const float *tobs, const float *tcorr,
                                             const float *varobs, const float *test, float *t0, float *objfn)
{
    const char *fcnm = "locate_l2_gridSearch__float64";
    if ((sizeof(float) * (size_t)ldgrd) % 64 != 0 || ldgrd < ngrd || nobs < 1 || !mask || !tobs ||
        !varobs || !test || !t0 || !objfn) {
        if ((sizeof(float) * (size_t)ldgrd) % 64 != 0) printf("%s: Error ldgrd must be divisible by 64\n", fcnm);
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
    std::vector<float> tc, wt;
    float xnorm = 0.0f;
    for (int i = 0; i < nobs; i++) {
        if (mask[i] != 0) continue;
        tc.push_back(tcorr ? tobs[i] - tcorr[i] : tobs[i]);
        row.push_back(i);
        wt.push_back(1.0f / varobs[i]);
        xnorm = xnorm + wt.back();
    }
    const int nuse = (int)row.size();
    const int ptr[2] = {0, nuse};
    int *d_row = nullptr, *d_ptr = nullptr;
    float *d_tc = nullptr, *d_wt = nullptr, *d_xn = nullptr, *d_test = nullptr, *d_t0 = nullptr, *d_obj = nullptr;
    int rc = 1;
    const size_t tb = (size_t)ldgrd * nobs * 4, gb = (size_t)ldgrd * 4;
    if (hipMalloc(&d_row, (nuse + 1) * 4) != hipSuccess || hipMalloc(&d_ptr, 8) != hipSuccess ||
        hipMalloc(&d_tc, (nuse + 1) * 4) != hipSuccess || hipMalloc(&d_wt, (nuse + 1) * 4) != hipSuccess ||
        hipMalloc(&d_xn, 4) != hipSuccess || hipMalloc(&d_test, tb) != hipSuccess ||
        hipMalloc(&d_t0, gb) != hipSuccess || hipMalloc(&d_obj, gb) != hipSuccess)
        goto out;
    if (nuse) {
        hipMemcpy(d_row, row.data(), nuse * 4, hipMemcpyHostToDevice);
        hipMemcpy(d_tc, tc.data(), nuse * 4, hipMemcpyHostToDevice);
        hipMemcpy(d_wt, wt.data(), nuse * 4, hipMemcpyHostToDevice);
    }
    hipMemcpy(d_ptr, ptr, 8, hipMemcpyHostToDevice);
    hipMemcpy(d_xn, &xnorm, 4, hipMemcpyHostToDevice);
    hipMemcpy(d_test, test, tb, hipMemcpyHostToDevice);
    if (l2_gridsearch_f32(ldgrd, ngrd, 1, iwantOT, t0use, d_ptr, d_row, d_tc, d_wt, d_xn, d_test, d_t0, d_obj, 0,
                          nullptr) != hipSuccess)
        goto out;
    if (hipMemcpy(t0, d_t0, (size_t)ngrd * 4, hipMemcpyDeviceToHost) != hipSuccess) goto out;
    if (hipMemcpy(objfn, d_obj, (size_t)ngrd * 4, hipMemcpyDeviceToHost) != hipSuccess) goto out;
    rc = 0;
out:
    hipFree(d_row); hipFree(d_ptr); hipFree(d_tc); hipFree(d_wt); hipFree(d_xn);
    hipFree(d_test); hipFree(d_t0); hipFree(d_obj);
    if (rc) printf("%s: device failure\n", fcnm);
    return rc;
}

// Relocation grid search of many events against one model's station tables
// (SURVEY s.8f row 2): device arrays, one launch, enqueued on `stream`.
extern "C" int mceik_relocate(const mceik_relocate_batch *b, void *stream)
{
    if (!b || b->ngrd < 1 || b->ldgrd < b->ngrd || b->nev < 1 || !b->tables || !b->ev_ptr || !b->obs_row ||
        !b->tc || !b->wt || !b->xnorm || !b->out) {
        fprintf(stderr, "mceik_relocate: invalid batch description\n");
        return 1;
    }
    if (b->nrows > 0 && b->nobs >= 0 && relocate_lds_bytes(b->nrows, b->nobs, b->nev) <= 64 * 1024)
        return relocate_lds(b->ldgrd, b->ngrd, b->nrows, b->nev, b->nobs, b->iwantOT, b->t0use, b->ev_ptr, b->obs_row,
                            b->tc, b->wt, b->xnorm, b->tables, b->t0, b->out, b->log_pdf ? 1 : 0,
                            (hipStream_t)stream) != hipSuccess;
    return l2_gridsearch_f32(b->ldgrd, b->ngrd, b->nev, b->iwantOT, b->t0use, b->ev_ptr, b->obs_row, b->tc, b->wt,
                             b->xnorm, b->tables, b->t0, b->out, b->log_pdf ? 1 : 0, (hipStream_t)stream) != hipSuccess;
}
