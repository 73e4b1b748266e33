// l1.h -- the L1 (Laplace) event objective with the weighted-median origin
// time, one definition for host and device.  Every L1 site
// -- the grid-search kernels (l1.hip), the sampler's logL, the hypocentre and
// nuisance moves, the data-fit stream, weightedMedian__double -- calls these
// templates, so the sites agree bit for bit.
//
// For the used observations j of [j0, j1), in that (catalogue) order, with
// residual x_j and weight w_j > 0:
//   W = sum_j w_j;  half = 0.5 W
//   s_k = sum_j ((x_j < x_k || (x_j == x_k && j <= k)) ? w_j : 0)
//   t0 = x_k of the smallest x_k with s_k >= half (first k among equals):
//        the lower weighted median
//   obj = sum_j w_j |x_j - t0|
// Every sum is taken in ascending j, so a value does not depend on who
// computes it.  s_k is non-decreasing along the (value, index) order and its
// last value is W: exactly one k is chosen and no sort is needed.  No used
// observation: t0 = 0, obj = 0.
//
// used(j), x_of(j), w_of(j) are callables; x is never kept in a per-thread
// array (it would go to scratch): the pair loop re-evaluates x_of(j) -- from
// LDS or from memory, the caller's choice -- for L1_KB candidates k at a time,
// whose partial sums are independent (the same bits as one k at a time).
#pragma once
#include <hip/hip_runtime.h>

#define L1_KB 4                    // candidates k per pass over j

namespace l1 {

__host__ __device__ __forceinline__ double absv(double x) { return __builtin_fabs(x); }
__host__ __device__ __forceinline__ float absv(float x) { return __builtin_fabsf(x); }

// The lower weighted median (t0 above); *nused: the number of used observations.
template <typename T, typename U, typename X, typename Wf>
__host__ __device__ __forceinline__ T median(int j0, int j1, U used, X x_of, Wf w_of, int *nused)
{
    T W = (T)0;
    int n = 0;
    for (int j = j0; j < j1; j++)
        if (used(j)) { W = W + w_of(j); n++; }
    if (nused) *nused = n;
    if (!n) return (T)0;
    const T half = (T)0.5 * W;
    bool have = false;
    T xb = (T)0;
    for (int k0 = j0; k0 < j1; k0 += L1_KB) {
        T xk[L1_KB], s[L1_KB];
        bool uk[L1_KB];
#pragma unroll
        for (int i = 0; i < L1_KB; i++) {
            const int k = k0 + i;
            uk[i] = k < j1 && used(k);
            xk[i] = uk[i] ? x_of(k) : (T)0;
            s[i] = (T)0;
        }
        for (int j = j0; j < j1; j++) {
            if (!used(j)) continue;
            const T xj = x_of(j), wj = w_of(j);
            // (| and & on the comparisons' results, not || and &&: compare / select / add without a branch)
#pragma unroll
            for (int i = 0; i < L1_KB; i++)
                s[i] = s[i] + (((xj < xk[i]) | ((xj == xk[i]) & (j <= k0 + i))) ? wj : (T)0);
        }
#pragma unroll
        for (int i = 0; i < L1_KB; i++)
            if (uk[i] && s[i] >= half && (!have || xk[i] < xb)) { have = true; xb = xk[i]; }
    }
    // (no k reaches half only where a weight or a residual is not a number)
    return have ? xb : (T)__builtin_nanf("");
}

// obj = sum_j w_j |x_j - t0| at a given t0.
template <typename T, typename U, typename X, typename Wf>
__host__ __device__ __forceinline__ T objective(int j0, int j1, U used, X x_of, Wf w_of, T t0)
{
    T obj = (T)0;
    for (int j = j0; j < j1; j++)
        if (used(j)) obj = obj + w_of(j) * absv(x_of(j) - t0);
    return obj;
}

// The event objective at its own weighted-median origin time.
template <typename T, typename U, typename X, typename Wf>
__host__ __device__ __forceinline__ T event(int j0, int j1, U used, X x_of, Wf w_of, T *t0)
{
    const T t = median<T>(j0, j1, used, x_of, w_of, nullptr);
    if (t0) *t0 = t;
    return objective<T>(j0, j1, used, x_of, w_of, t);
}

}  // namespace l1

// l1.hip's host launchers (C++ linkage; device arrays).  One event, fp64:
// compacted observations (row of `test`, tc, wt as the caller scaled them).
hipError_t l1_gridsearch(int ldgrd, int ngrd, int nuse, int iwantOT, double t0use, const int *row, const double *tc,
                         const double *wt, const double *test, double *t0, double *objfn, hipStream_t st);
// A list of events, fp32 (mceik_relocate_batch's arrays); nrows > 0: rows are checked against it.
hipError_t l1_gridsearch_f32(int ldgrd, int ngrd, int nev, int nrows, int iwantOT, float t0use, const int *ev_ptr,
                             const int *obs_row, const float *tc, const float *wt, const float *test, float *t0,
                             float *objfn, int negate, hipStream_t st);
