// lang.hip -- gradient-informed (discrete Langevin) moves of the sampler
// (include/mceik.h mceik_mcmc_lang_*), on gfx950.
//
// The kernels of one Langevin step around the forwards with fields and the
// adjoint batches that sampler.hip queues: the step draw, the pick weights of
// a state, the proposal (one workgroup per chain, its threads striding over
// the cells; the chain's log q reduced in a fixed order), the reverse log q
// at the proposed state, and the accept.  No atomics and no waits between
// workgroups; per-chain state that an earlier kernel of the step wrote is
// read through mcmcd::ldv.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lang.h"
#include "mcmc_common.h"
#include "mcmc_device.h"
#include "mcmc_host.h"
#include "nuis.h"
#include "prior.h"

namespace {

using mcmcd::ldv;

// Phase and log u of every chain's step; the proposal fields the other kernels
// and the accessors read (the move stays inside the box by construction).
__global__ void lang_draw_kernel(McmcDev D, LangDev L, uint64_t gs)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= D.nchains) return;
    uint32_t r[4];
    lang_uniform(D.seed, (uint32_t)(D.chain_offset + c), gs, 0xFFFFFFFFu, r);
    const int ph = (int)(((uint64_t)r[0] * (uint32_t)D.nphase) >> 32);
    D.prop_phase[c] = ph;
    D.prop_cell[c] = ph * D.ncell;
    D.prop_v[c] = ldv(&D.v[(size_t)c * D.ncm + (size_t)ph * D.ncell]);
    D.prop_inprior[c] = 1;
    D.prop_logu[c] = mcmcd::det_log(((double)r[3] + 0.5) * (1.0 / 4294967296.0));
}

// One thread per (chain, event): mcmc.logl_pick_grad operation for operation on
// the chain's effective var and tcorr, each used pick's term added to its
// (station, event) weight in pick order.  An event's picks touch column e only.
__global__ void lang_weights_kernel(McmcDev D, NuisDev N, int c0, int n, double *ev_w)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * D.nev) return;
    const int k = i / D.nev, e = i - k * D.nev, c = c0 + k;
    const McmcDev E = nuis_chain(D, N, c);
    const int pph = ldv(&D.prop_phase[c]);
    const float *tp = E.ttab + (size_t)c * E.nstat * E.nev;
    const float *tcur = E.ttab_cur ? E.ttab_cur + (size_t)c * E.nphase * E.nstat * E.nev : nullptr;
    auto te_of = [&](int j) -> double {
        const int ph = E.obs_phase ? E.obs_phase[j] : 0;
        const size_t q = (size_t)E.obs_stat[j] * E.nev + e;
        return (double)(ph == pph ? ldv(tp + q) : ldv(tcur + (size_t)ph * E.nstat * E.nev + q));
    };
    double *row = ev_w + (size_t)k * E.nstat * E.nev + e;
    for (int s = 0; s < E.nstat; s++) row[(size_t)s * E.nev] = 0.0;
    const int j0 = E.obs_ptr[e], j1 = E.obs_ptr[e + 1];
    double xnorm = 0.0, t0 = 0.0, sum = 0.0;
    for (int j = j0; j < j1; j++) if (!E.obs_mask[j]) xnorm = xnorm + 1.0 / ldv(&E.var[j]);
    for (int j = j0; j < j1; j++) {
        if (E.obs_mask[j]) continue;
        const double te = te_of(j);
        t0 = t0 + ((1.0 / ldv(&E.var[j])) / xnorm) * ((E.tobs[j] - ldv(&E.tcorr[j])) - te);
    }
    for (int j = j0; j < j1; j++) {
        if (E.obs_mask[j]) continue;
        const double w = 1.0 / ldv(&E.var[j]);
        const double r = (E.tobs[j] - ldv(&E.tcorr[j])) - (te_of(j) + t0);
        sum = sum + (w * w) * r;
    }
    for (int j = j0; j < j1; j++) {
        if (E.obs_mask[j]) continue;
        const int ph = E.obs_phase ? E.obs_phase[j] : 0;
        if (ph != pph) continue;                        // the other phase's model does not move
        const double w = 1.0 / ldv(&E.var[j]);
        const double r = (E.tobs[j] - ldv(&E.tcorr[j])) - (te_of(j) + t0);
        const double g = (w * w) * r - (w / xnorm) * sum;
        double *q = row + (size_t)E.obs_stat[j] * E.nev;
        *q = ldv(q) + g;
    }
}

// The prior's gradient at cell i of the model v (ncx x ncy x ncz, x fastest):
// -(ws (double)(2 sum_nb (v_i - v_nb)) + wd (double)(2 (v_i - vref_i))), the
// sums exact integers (no reference model: the second integer is 0).
__device__ __forceinline__ double lang_prior_grad(const BlockDev &B, const int *v, const int *vref, int i, double ws,
                                                  double wd)
{
    const int x = i % B.ncx, y = (i / B.ncx) % B.ncy, z = i / (B.ncx * B.ncy);
    const long long vi = ldv(v + i);
    long long sn = 0;
    if (x > 0) sn += vi - ldv(v + i - 1);
    if (x + 1 < B.ncx) sn += vi - ldv(v + i + 1);
    if (y > 0) sn += vi - ldv(v + i - B.ncx);
    if (y + 1 < B.ncy) sn += vi - ldv(v + i + B.ncx);
    if (z > 0) sn += vi - ldv(v + i - B.ncx * B.ncy);
    if (z + 1 < B.ncz) sn += vi - ldv(v + i + B.ncx * B.ncy);
    const long long dd = vref ? 2 * (vi - vref[i]) : 0;
    return -(ws * (double)(2 * sn) + wd * (double)dd);
}

// d_i of cell i: the chain's beta times d logL / d v_i (from the slowness
// gradient gs) plus the prior's gradient (0.0 with the prior off).
__device__ __forceinline__ double lang_drift(const McmcDev &D, const BlockDev &B, const PriorDev &P, int prior_on, int c,
                                             int ph, const int *v, int i, double gs)
{
    const double vv = (double)ldv(v + i);
    const double g = -(gs / (vv * vv));
    double gp = 0.0;
    if (prior_on)
        gp = lang_prior_grad(B, v, P.vref ? P.vref + (size_t)ph * D.ncell : nullptr, i, ph ? P.ws1 : P.ws0,
                             ph ? P.wd1 : P.wd0);
    return (D.beta ? ldv(&D.beta[c]) * g : g) + gp;
}

// Partial l adds the terms of cells l, l + 256, ... in order; the total adds
// the partials 0..255 in order (thread 0).
__device__ __forceinline__ double lang_reduce(double part, double *sh)
{
    sh[threadIdx.x] = part;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x == 0)
        for (int l = 0; l < LANG_THREADS; l++) tot = tot + sh[l];
    return tot;
}

__global__ __launch_bounds__(LANG_THREADS) void lang_propose_kernel(McmcDev D, BlockDev B, PriorDev P, int prior_on,
                                                                    LangDev L, uint64_t gs)
{
    __shared__ double sh[LANG_THREADS];
    __shared__ int shn[LANG_THREADS];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int ph = ldv(&D.prop_phase[c]);
    const int vlo = ph ? D.vsmin : D.vmin, vhi = ph ? D.vsmax : D.vmax;
    const size_t row = (size_t)c * D.ncm + (size_t)ph * D.ncell;
    const int *v = D.v + row;
    // the other phase's model is the current one
    for (int i = tid; i < D.ncm; i += LANG_THREADS)
        if (i / D.ncell != ph) L.vprop[(size_t)c * D.ncm + i] = ldv(&D.v[(size_t)c * D.ncm + i]);
    double part = 0.0;
    int nm = 0;
    for (int i = tid; i < D.ncell; i += LANG_THREADS) {
        const int vi = ldv(v + i);
        const double d = lang_drift(D, B, P, prior_on, c, ph, v, i, ldv(&L.g0[(size_t)c * D.ncell + i]));
        uint32_t r[4];
        const double u = lang_uniform(D.seed, (uint32_t)(D.chain_offset + c), gs, (uint32_t)i, r);
        const LangCell S = lang_cell(d, vi, vlo, vhi, L.c, L.dmax);
        const int delta = lang_pick(S, u);
        L.delta[(size_t)c * D.ncell + i] = delta;
        L.vprop[row + i] = vi + delta;
        D.slow_prop[row + i] = 1.0f / (float)(vi + delta);
        part = part + lang_logq(S, delta);
        nm += delta != 0;
    }
    shn[tid] = nm;
    const double tot = lang_reduce(part, sh);
    if (tid == 0) {
        int n = 0;
        for (int l = 0; l < LANG_THREADS; l++) n += shn[l];
        L.lq[3 * (size_t)c] = tot;
        L.nmove[c] = n;
    }
}

// lqr = sum_i log q'_i(-delta_i): the supports and drifts rebuilt about v'.
__global__ __launch_bounds__(LANG_THREADS) void lang_reverse_kernel(McmcDev D, BlockDev B, PriorDev P, int prior_on,
                                                                    LangDev L)
{
    __shared__ double sh[LANG_THREADS];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int ph = ldv(&D.prop_phase[c]);
    const int vlo = ph ? D.vsmin : D.vmin, vhi = ph ? D.vsmax : D.vmax;
    const int *v = L.vprop + (size_t)c * D.ncm + (size_t)ph * D.ncell;
    double part = 0.0;
    for (int i = tid; i < D.ncell; i += LANG_THREADS) {
        const double d = lang_drift(D, B, P, prior_on, c, ph, v, i, ldv(&L.g1[(size_t)c * D.ncell + i]));
        const LangCell S = lang_cell(d, ldv(v + i), vlo, vhi, L.c, L.dmax);
        part = part + lang_logq(S, -ldv(&L.delta[(size_t)c * D.ncell + i]));
    }
    const double tot = lang_reduce(part, sh);
    if (tid == 0) L.lq[3 * (size_t)c + 1] = tot;
}

// accept iff log u (folded with the prior's exact energy differences) < beta
// (logL' - logL) + (lqr - lqf) and no solve of the step failed; thread 0
// decides, the workgroup commits (v, slow_cur, the phase's current tables) or
// reverts (slow_prop).
__global__ __launch_bounds__(LANG_THREADS) void lang_accept_kernel(McmcDev D, NuisDev N, PriorDev P, int prior_on,
                                                                   LangDev L, int keep_slot)
{
    __shared__ int s_acc;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int ph = ldv(&D.prop_phase[c]);
    if (tid == 0) {
        double logu = ldv(&D.prop_logu[c]);
        if (prior_on) {
            const size_t r = (size_t)c * D.nphase + ph, ps = L.pen_stride;
            const long long dEs = (long long)(ldv(&L.pen[2 * ps + r]) - ldv(&L.pen[r]));
            const long long dEd = (long long)(ldv(&L.pen[3 * ps + r]) - ldv(&L.pen[ps + r]));
            logu = prior_fold_logu(logu, ph ? P.ws1 : P.ws0, ph ? P.wd1 : P.wd0, dEs, dEd);
        }
        int fail = 0;
        for (int s = 0; s < D.nstat; s++) {
            const size_t q = (size_t)c * D.nstat + s;
            const bool skipped = L.skip && L.skip[ph * D.nstat + s];    // its forward ran, its table is never read
            if (!skipped && (ldv(&L.ierr0[q]) | ldv(&L.ierr1[q]))) fail = 1;
            if (ldv(&L.ast0[q]) | ldv(&L.ast1[q])) fail = 1;
        }
        const double ln = nuis_logl(D, N, c, mcmcd::chain_loglik(nuis_chain(D, N, c), c, ph));
        const double lold = ldv(&D.logl[c]);
        const double dl = ln - lold;
        const double lqf = ldv(&L.lq[3 * (size_t)c]), lqr = ldv(&L.lq[3 * (size_t)c + 1]);
        const double rhs = (D.beta ? ldv(&D.beta[c]) * dl : dl) + (lqr - lqf);
        const int acc = !fail && logu < rhs;
        s_acc = acc;
        L.lq[3 * (size_t)c + 2] = ln;
        L.status[c] = fail;
        unsigned long long *cnt = L.cnt + 4 * (size_t)c;
        cnt[0] = ldv(&cnt[0]) + 1;
        if (acc) {
            cnt[1] = ldv(&cnt[1]) + 1;
            cnt[3] = ldv(&cnt[3]) + (unsigned long long)ldv(&L.nmove[c]);
            D.logl[c] = ln;
            D.naccept[c] = ldv(&D.naccept[c]) + 1;
        }
        if (fail) cnt[2] = ldv(&cnt[2]) + 1;
        D.accept[c] = (unsigned char)acc;
        if (keep_slot >= 0) D.keep_logl[(size_t)keep_slot * D.keep_stride + c] = acc ? ln : lold;
    }
    __syncthreads();
    const int acc = s_acc;
    const size_t row = (size_t)c * D.ncm + (size_t)ph * D.ncell;
    for (int i = tid; i < D.ncell; i += LANG_THREADS) {
        if (acc) {
            D.v[row + i] = ldv(&L.vprop[row + i]);
            D.slow_cur[row + i] = ldv(&D.slow_prop[row + i]);
        } else {
            D.slow_prop[row + i] = ldv(&D.slow_cur[row + i]);
        }
    }
    if (acc && D.ttab_cur) mcmcd::chain_copy_tables(D, c, ph, tid, LANG_THREADS);
}

}  // namespace

hipError_t lang_draw(const McmcDev &D, const LangDev &L, uint64_t gs, hipStream_t st)
{
    hipLaunchKernelGGL(lang_draw_kernel, dim3((D.nchains + 63) / 64), dim3(64), 0, st, D, L, gs);
    return hipGetLastError();
}

hipError_t lang_weights(const McmcDev &D, const NuisDev &N, int c0, int n, double *ev_w, hipStream_t st)
{
    hipLaunchKernelGGL(lang_weights_kernel, dim3((n * D.nev + 63) / 64), dim3(64), 0, st, D, N, c0, n, ev_w);
    return hipGetLastError();
}

hipError_t lang_propose(const McmcDev &D, const BlockDev &B, const PriorDev &P, bool prior_on, const LangDev &L,
                        uint64_t gs, hipStream_t st)
{
    hipLaunchKernelGGL(lang_propose_kernel, dim3(D.nchains), dim3(LANG_THREADS), 0, st, D, B, P, prior_on ? 1 : 0, L, gs);
    return hipGetLastError();
}

hipError_t lang_reverse(const McmcDev &D, const BlockDev &B, const PriorDev &P, bool prior_on, const LangDev &L,
                        hipStream_t st)
{
    hipLaunchKernelGGL(lang_reverse_kernel, dim3(D.nchains), dim3(LANG_THREADS), 0, st, D, B, P, prior_on ? 1 : 0, L);
    return hipGetLastError();
}

hipError_t lang_accept(const McmcDev &D, const NuisDev &N, const PriorDev &P, bool prior_on, const LangDev &L,
                       int keep_slot, hipStream_t st)
{
    hipLaunchKernelGGL(lang_accept_kernel, dim3(D.nchains), dim3(LANG_THREADS), 0, st, D, N, P, prior_on ? 1 : 0, L,
                       keep_slot);
    if (keep_slot >= 0) return mcmc_keep(D, keep_slot, st);
    return hipGetLastError();
}
