// hypo.hip -- hypocentre moves of the GPU sampler (include/mceik.h
// mceik_mcmc_hypo_*), on gfx950.
//
// logL = -sum_e objfn_e, and given the velocity model the events are
// independent: one forward of every chain's current models, with every
// station's time extracted at each event's current node and at its candidate
// node, serves a Metropolis move of all nev hypocentres of the chain at once.
// Three kernels around that forward: the draw (one thread per chain and
// event), the per-event accept (likewise), and the chain's logL (one thread
// per chain, events in order).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "hypo.h"
#include "mcmc_common.h"
#include "mcmc_device.h"
#include "mcmc_host.h"
#include "nuis.h"

namespace {

__device__ __forceinline__ int hypo_node(const HypoDev &H, int x, int y, int z) { return (z * H.ny + y) * H.nx + x; }

__device__ __forceinline__ bool hypo_inside(const HypoDev &H, int x, int y, int z)
{
    return x >= H.lox && x <= H.hix && y >= H.loy && y <= H.hiy && z >= H.loz && z <= H.hiz;
}

// The draw, the candidate and both node lists of (chain c, event e).  A
// candidate outside the box is rejected, and its list entry is the current
// node (the forward still extracts a valid value, which nothing reads).
__global__ __launch_bounds__(64) void hypo_propose_kernel(McmcDev D, HypoDev H, uint64_t gs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= D.nchains * D.nev) return;
    const int c = i / D.nev, e = i - c * D.nev;
    int d[3];
    const uint32_t r3 = hypo_draw(D.seed, (uint32_t)(D.chain_offset + c), gs, e, H.dmx, H.dmy, H.dmz, d);
    const int x = H.hyp[3 * i], y = H.hyp[3 * i + 1], z = H.hyp[3 * i + 2];
    const int cx = x + d[0], cy = y + d[1], cz = z + d[2];
    H.cand[3 * i] = cx; H.cand[3 * i + 1] = cy; H.cand[3 * i + 2] = cz;
    H.logu[i] = mcmcd::det_log(((double)r3 + 0.5) * (1.0 / 4294967296.0));
    const int ncur = hypo_node(H, x, y, z);
    const int ncand = hypo_inside(H, cx, cy, cz) ? hypo_node(H, cx, cy, cz) : ncur;
    for (int ph = 0; ph < D.nphase; ph++) {
        int *row = H.ev2 + ((size_t)c * D.nphase + ph) * 2 * D.nev;
        row[e] = ncur;
        row[D.nev + e] = ncand;
    }
}

// mcmc_device.h event_obj's arithmetic (the same operations in the same
// order) on column col of the hypocentre step's tables, every phase from them.
__device__ __forceinline__ double hypo_event_obj(const McmcDev &D, const HypoDev &H, int c, int e, int col)
{
    const int nev2 = 2 * D.nev;
    const float *tt = H.ttab2 + (size_t)c * D.nphase * D.nstat * nev2;
    const double sqrt2i = 0.7071067811865475;
    auto te_of = [&](int j) -> double {
        const int ph = D.obs_phase ? D.obs_phase[j] : 0;
        return (double)tt[((size_t)ph * D.nstat + D.obs_stat[j]) * nev2 + col];
    };
    const int j0 = D.obs_ptr[e], j1 = D.obs_ptr[e + 1];
    if (D.l1)                       // the L1 likelihood: mcmc_device.h event_obj_l1's arithmetic
        return l1::event<double>(j0, j1, [&](int j) -> bool { return !D.obs_mask[j]; },
                                 [&](int j) -> double { return (D.tobs[j] - D.tcorr[j]) - te_of(j); },
                                 [&](int j) -> double { return 1.0 / D.var[j]; }, nullptr);
    double xnorm = 0.0, t0 = 0.0, obj = 0.0;
    for (int j = j0; j < j1; j++) if (!D.obs_mask[j]) xnorm = xnorm + 1.0 / D.var[j];
    for (int j = j0; j < j1; j++) {
        if (D.obs_mask[j]) continue;
        double te = te_of(j);
        double tc = D.tobs[j] - D.tcorr[j];
        t0 = t0 + ((1.0 / D.var[j]) / xnorm) * (tc - te);
    }
    for (int j = j0; j < j1; j++) {
        if (D.obs_mask[j]) continue;
        double te = te_of(j);
        double tc = D.tobs[j] - D.tcorr[j];
        double res = ((1.0 / D.var[j]) * sqrt2i) * (tc - (te + t0));
        obj = obj + res * res;
    }
    return obj;
}

// Metropolis for (chain c, event e): accept iff the candidate is inside the
// box and log u < obj_cur - obj_cand (tempering: beta[c] times that, one fp64
// multiply; the uniform box is not tempered).  An accepted event's position,
// list entries and (nphase 2) current-table columns move here; events touch
// disjoint entries.
__global__ __launch_bounds__(64) void hypo_accept_kernel(McmcDev D, HypoDev H, NuisDev N)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= D.nchains * D.nev) return;
    const int c = i / D.nev, e = i - c * D.nev;
    const McmcDev E = nuis_chain(D, N, c);      // the chain's effective observations (nuisance state)
    const double oc = hypo_event_obj(E, H, c, e, e), od = hypo_event_obj(E, H, c, e, D.nev + e);
    const int cx = H.cand[3 * i], cy = H.cand[3 * i + 1], cz = H.cand[3 * i + 2];
    const double dl = oc - od;
    int a = 0;
    if (hypo_inside(H, cx, cy, cz)) a = D.beta ? H.logu[i] < D.beta[c] * dl : H.logu[i] < dl;
    H.obj[2 * (size_t)i] = oc;
    H.obj[2 * (size_t)i + 1] = od;
    H.acc[i] = (unsigned char)a;
    atomicAdd(&H.attempts[e], 1ull);
    if (!a) return;
    atomicAdd(&H.accepts[e], 1ull);
    H.hyp[3 * i] = cx; H.hyp[3 * i + 1] = cy; H.hyp[3 * i + 2] = cz;
    const int node = hypo_node(H, cx, cy, cz);
    H.ev1[i] = node;
    if (H.evall)
        for (int ph = 0; ph < D.nphase; ph++) H.evall[((size_t)c * D.nphase + ph) * D.nev + e] = node;
    if (D.ttab_cur) {
        const size_t rows = (size_t)D.nphase * D.nstat;
        const float *src = H.ttab2 + (size_t)c * rows * 2 * D.nev + D.nev + e;
        float *dst = D.ttab_cur + (size_t)c * rows * D.nev + e;
        for (size_t r = 0; r < rows; r++) dst[r * D.nev] = src[r * 2 * D.nev];
    }
}

// The chain's logL from the accepted sides, events in order: bitwise what a
// full forward at the chain's models and new positions gives.  The step
// proposed no velocity: its accept flag is 0.
__global__ __launch_bounds__(64) void hypo_logl_kernel(McmcDev D, HypoDev H, NuisDev N, int keep_slot)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= D.nchains) return;
    double logl = 0.0;
    for (int e = 0; e < D.nev; e++) {
        const size_t i = (size_t)c * D.nev + e;
        logl = logl - H.obj[2 * i + (H.acc[i] ? 1 : 0)];
    }
    logl = nuis_logl(D, N, c, logl);
    D.logl[c] = logl;
    D.accept[c] = 0;
    if (keep_slot >= 0) D.keep_logl[(size_t)keep_slot * D.keep_stride + c] = logl;
}

// Sums of x, y, z, xx, yy, zz, xy, xz, yz per event over the first ncold
// chains: one thread per (event, term), exact integers (any order adds up).
__global__ __launch_bounds__(64) void hypo_moments_kernel(McmcDev D, HypoDev H, int ncold)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= D.nev * 9) return;
    const int e = i / 9, k = i - e * 9;
    // term k = p * q of the coordinates a, b (k < 3: the coordinate itself)
    const int a = k < 3 ? k : k < 6 ? k - 3 : k == 6 ? 0 : k == 7 ? 0 : 1;
    const int b = k < 3 ? -1 : k < 6 ? k - 3 : k == 6 ? 1 : 2;
    long long s = 0;
    for (int c = 0; c < ncold; c++) {
        const int *h = H.hyp + 3 * ((size_t)c * D.nev + e);
        const long long p = h[a];
        s += b < 0 ? p : p * (long long)h[b];
    }
    atomicAdd(reinterpret_cast<unsigned long long *>(H.mom) + i, (unsigned long long)s);
}

__global__ __launch_bounds__(64) void hypo_lists_kernel(McmcDev D, HypoDev H)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= D.nchains * D.nev) return;
    const int c = i / D.nev, e = i - c * D.nev;
    const int node = hypo_node(H, H.hyp[3 * i], H.hyp[3 * i + 1], H.hyp[3 * i + 2]);
    H.ev1[i] = node;
    if (H.evall)
        for (int ph = 0; ph < D.nphase; ph++) H.evall[((size_t)c * D.nphase + ph) * D.nev + e] = node;
}

}  // namespace

double hypo_det_log_host(double x)
{
    uint64_t b;
    memcpy(&b, &x, 8);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    const uint64_t mb = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    memcpy(&m, &mb, 8);
    if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }
    double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double p = 1.0 / 25.0;
    p = p * s2 + 1.0 / 23.0; p = p * s2 + 1.0 / 21.0; p = p * s2 + 1.0 / 19.0;
    p = p * s2 + 1.0 / 17.0; p = p * s2 + 1.0 / 15.0; p = p * s2 + 1.0 / 13.0;
    p = p * s2 + 1.0 / 11.0; p = p * s2 + 1.0 / 9.0;  p = p * s2 + 1.0 / 7.0;
    p = p * s2 + 1.0 / 5.0;  p = p * s2 + 1.0 / 3.0;  p = p * s2 + 1.0;
    double de = (double)e;
    return de * 6.93147180369123816490e-01 + (2.0 * s * p + de * 1.90821492927058770002e-10);
}

hipError_t hypo_propose(const McmcDev &D, const HypoDev &H, uint64_t gs, hipStream_t st)
{
    const int n = D.nchains * D.nev;
    hipLaunchKernelGGL(hypo_propose_kernel, dim3((n + 63) / 64), dim3(64), 0, st, D, H, gs);
    return hipGetLastError();
}

hipError_t hypo_accept(const McmcDev &D, const HypoDev &H, const NuisDev &N, int keep_slot, hipStream_t st)
{
    const int n = D.nchains * D.nev;
    hipLaunchKernelGGL(hypo_accept_kernel, dim3((n + 63) / 64), dim3(64), 0, st, D, H, N);
    hipLaunchKernelGGL(hypo_logl_kernel, dim3((D.nchains + 63) / 64), dim3(64), 0, st, D, H, N, keep_slot);
    if (keep_slot >= 0) return mcmc_keep(D, keep_slot, st);
    return hipGetLastError();
}

hipError_t hypo_moments(const McmcDev &D, const HypoDev &H, int ncold, hipStream_t st)
{
    if (ncold <= 0) return hipSuccess;
    hipLaunchKernelGGL(hypo_moments_kernel, dim3((D.nev * 9 + 63) / 64), dim3(64), 0, st, D, H, ncold);
    return hipGetLastError();
}

hipError_t hypo_lists(const McmcDev &D, const HypoDev &H, hipStream_t st)
{
    const int n = D.nchains * D.nev;
    hipLaunchKernelGGL(hypo_lists_kernel, dim3((n + 63) / 64), dim3(64), 0, st, D, H);
    return hipGetLastError();
}
