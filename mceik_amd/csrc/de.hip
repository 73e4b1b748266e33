// de.hip -- differential-evolution (population) moves of the sampler
// (include/mceik.h mceik_mcmc_de_*), on gfx950.
//
// The kernels of one DE step around the forward of the movers' proposed models
// that sampler.hip queues: the proposal (one workgroup per mover; its threads
// take four cells at a time, one Philox call per four cells), the scatter of
// the compact batch's tables into the movers' rows of the step batch, and the
// accept (one workgroup per chain of the pipe, standing chains included).  No
// atomics and no waits between workgroups; per-chain state that an earlier
// kernel of the step wrote is read through mcmcd::ldv.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "de.h"
#include "mcmc_common.h"
#include "mcmc_device.h"
#include "mcmc_host.h"
#include "nuis.h"
#include "prior.h"

namespace {

using mcmcd::ldv;

// Four consecutive ints of a row: one 16-byte load where the row allows it.
__device__ __forceinline__ void load4(const int *row, int i, int n, bool vec, int out[4])
{
    if (vec) {
        const int4 q = *reinterpret_cast<const int4 *>(row + i);
        out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
    } else {
        for (int k = 0; k < 4; k++) out[k] = i + k < n ? ldv(row + i + k) : 0;
    }
}

__global__ __launch_bounds__(DE_THREADS) void de_propose_kernel(McmcDev D, HypoDev H, DeDev L, uint64_t gs, int par,
                                                                int ph)
{
    __shared__ int sh_out[DE_THREADS], sh_nm[DE_THREADS];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int cs = L.mov[par][m];                       // the mover, as a chain of the sampler
    const int c = cs - L.off;                           // ... and of this pipe
    const int rung = cs / L.G;
    const int nb = de_nb(L.G, par);
    int i, j;
    const uint32_t r3 = de_draw(D.seed, (uint32_t)(D.chain_offset + c), gs, nb, &i, &j);
    const int ca = rung * L.G + 2 * i + (1 - par), cb = rung * L.G + 2 * j + (1 - par);
    const int vlo = ph ? D.vsmin : D.vmin, vhi = ph ? D.vsmax : D.vmax;
    const size_t row = (size_t)c * D.ncm + (size_t)ph * D.ncell;
    const int *v = D.v + row;
    const int *va = L.vall + (size_t)ca * D.ncm + (size_t)ph * D.ncell;
    const int *vb = L.vall + (size_t)cb * D.ncm + (size_t)ph * D.ncell;
    float *cslow = L.slow + (size_t)m * D.ncell;
    const bool vec = (D.ncell & 3) == 0;                // every row then starts on a 16-byte boundary
    // the other phase's model is the current one
    for (int k = tid; k < D.ncm; k += DE_THREADS)
        if (k / D.ncell != ph) L.vprop[(size_t)c * D.ncm + k] = ldv(&D.v[(size_t)c * D.ncm + k]);
    int out = 0, nm = 0;
    for (int q = tid * 4; q < D.ncell; q += DE_THREADS * 4) {
        int x[4], xa[4], xb[4];
        load4(v, q, D.ncell, vec, x);
        load4(va, q, D.ncell, vec, xa);
        load4(vb, q, D.ncell, vec, xb);
        uint32_t w[4];
        de_philox(D.seed, (uint32_t)(D.chain_offset + c), gs, (uint32_t)(q >> 2), w);
        int vp[4];
        float sp[4];
        for (int k = 0; k < 4; k++) {
            const long long delta = de_delta(L.gq, (long long)xa[k] - (long long)xb[k], w[k], L.crq);
            const long long vn = (long long)x[k] + delta;
            const bool in = vn >= vlo && vn <= vhi;
            if (q + k < D.ncell) {
                out |= !in;
                nm += delta != 0;
            }
            // a cell outside the box rejects the whole move; the forward still runs, on a model it can solve
            vp[k] = in ? (int)vn : x[k];
            sp[k] = 1.0f / (float)vp[k];
        }
        if (vec) {
            *reinterpret_cast<int4 *>(L.vprop + row + q) = make_int4(vp[0], vp[1], vp[2], vp[3]);
            *reinterpret_cast<float4 *>(cslow + q) = make_float4(sp[0], sp[1], sp[2], sp[3]);
            *reinterpret_cast<float4 *>(D.slow_prop + row + q) = make_float4(sp[0], sp[1], sp[2], sp[3]);
        } else {
            for (int k = 0; k < 4 && q + k < D.ncell; k++) {
                L.vprop[row + q + k] = vp[k];
                cslow[q + k] = sp[k];
                D.slow_prop[row + q + k] = sp[k];
            }
        }
    }
    if (H.hyp)
        for (int e = tid; e < D.nev; e += DE_THREADS) L.ev[(size_t)m * D.nev + e] = ldv(&H.ev1[(size_t)c * D.nev + e]);
    sh_out[tid] = out;
    sh_nm[tid] = nm;
    __syncthreads();
    if (tid == 0) {
        int o = 0, n = 0;
        for (int l = 0; l < DE_THREADS; l++) { o |= sh_out[l]; n += sh_nm[l]; }
        L.a[c] = ca;
        L.b[c] = cb;
        L.inbox[c] = !o;
        L.nmove[c] = n;
        D.prop_phase[c] = ph;
        D.prop_cell[c] = ph * D.ncell;
        D.prop_v[c] = ldv(v);
        D.prop_inprior[c] = !o;
        D.prop_logu[c] = mcmcd::det_log(((double)r3 + 0.5) * (1.0 / 4294967296.0));
    }
}

__global__ __launch_bounds__(DE_THREADS) void de_scatter_kernel(McmcDev D, DeDev L, int par)
{
    const int m = blockIdx.x, tid = threadIdx.x;
    const int c = L.mov[par][m] - L.off;
    const size_t n = (size_t)D.nstat * D.nev;
    const float *src = L.ttab + (size_t)m * n;
    float *dst = L.ttab_out + (size_t)c * n;
    for (size_t k = tid; k < n; k += DE_THREADS) dst[k] = ldv(src + k);
    for (int s = tid; s < D.nstat; s += DE_THREADS) {
        L.ierr_out[(size_t)c * D.nstat + s] = ldv(&L.ierr[(size_t)m * D.nstat + s]);
        L.niter_out[(size_t)c * D.nstat + s] = ldv(&L.niter[(size_t)m * D.nstat + s]);
    }
}

// Movers: accept iff v' is inside the box, no unskipped solve failed and log u
// (folded with the prior's exact energy differences) < beta (logL' - logL);
// thread 0 decides, the workgroup commits (v, slow_cur, the phase's current
// tables) or reverts (slow_prop).  Standing chains: accept = 0, nothing else moves.
__global__ __launch_bounds__(DE_THREADS) void de_accept_kernel(McmcDev D, NuisDev N, PriorDev P, int prior_on, DeDev L,
                                                               int par, int ph, int keep_slot)
{
    __shared__ int s_acc;
    const int c = blockIdx.x, tid = threadIdx.x;
    const bool mover = (((L.off + c) % L.G) & 1) == par;
    if (!mover) {
        if (tid == 0) {
            L.a[c] = -1;
            L.b[c] = -1;
            L.inbox[c] = 0;
            L.nmove[c] = 0;
            L.status[c] = 0;
            L.logl_prop[c] = 0.0;
            D.prop_phase[c] = ph;
            D.accept[c] = 0;
            if (keep_slot >= 0) D.keep_logl[(size_t)keep_slot * D.keep_stride + c] = ldv(&D.logl[c]);
        }
        return;
    }
    if (tid == 0) {
        const int inbox = ldv(&L.inbox[c]);
        const double lold = ldv(&D.logl[c]);
        int fail = 0;
        double ln = lold;
        if (inbox) {
            for (int s = 0; s < D.nstat; s++) {
                const bool skipped = L.skip && L.skip[ph * D.nstat + s];
                if (!skipped && ldv(&L.ierr_out[(size_t)c * D.nstat + s])) fail = 1;
            }
            if (!fail) ln = nuis_logl(D, N, c, mcmcd::chain_loglik(nuis_chain(D, N, c), c, ph));
        }
        double logu = ldv(&D.prop_logu[c]);
        if (prior_on && inbox) {
            const size_t r = (size_t)c * D.nphase + ph, ps = L.pen_stride;
            const long long dEs = (long long)(ldv(&L.pen[2 * ps + r]) - ldv(&L.pen[r]));
            const long long dEd = (long long)(ldv(&L.pen[3 * ps + r]) - ldv(&L.pen[ps + r]));
            logu = prior_fold_logu(logu, ph ? P.ws1 : P.ws0, ph ? P.wd1 : P.wd0, dEs, dEd);
        }
        const double dl = ln - lold;
        const int acc = inbox && !fail && logu < (D.beta ? ldv(&D.beta[c]) * dl : dl);
        s_acc = acc;
        L.logl_prop[c] = ln;
        L.status[c] = fail;
        unsigned long long *cnt = L.cnt + 5 * (size_t)c;
        cnt[0] = ldv(&cnt[0]) + 1;
        if (acc) {
            cnt[1] = ldv(&cnt[1]) + 1;
            cnt[4] = ldv(&cnt[4]) + (unsigned long long)ldv(&L.nmove[c]);
            D.logl[c] = ln;
            D.naccept[c] = ldv(&D.naccept[c]) + 1;
        }
        if (!inbox) cnt[2] = ldv(&cnt[2]) + 1;
        if (fail) cnt[3] = ldv(&cnt[3]) + 1;
        D.accept[c] = (unsigned char)acc;
        if (keep_slot >= 0) D.keep_logl[(size_t)keep_slot * D.keep_stride + c] = acc ? ln : lold;
    }
    __syncthreads();
    const int acc = s_acc;
    const size_t row = (size_t)c * D.ncm + (size_t)ph * D.ncell;
    for (int i = tid; i < D.ncell; i += DE_THREADS) {
        if (acc) {
            D.v[row + i] = ldv(&L.vprop[row + i]);
            D.slow_cur[row + i] = ldv(&D.slow_prop[row + i]);
        } else {
            D.slow_prop[row + i] = ldv(&D.slow_cur[row + i]);
        }
    }
    if (acc && D.ttab_cur) mcmcd::chain_copy_tables(D, c, ph, tid, DE_THREADS);
}

}  // namespace

hipError_t de_propose(const McmcDev &D, const HypoDev &H, const DeDev &L, uint64_t gs, int par, int ph, hipStream_t st)
{
    if (L.nmov[par] > 0)
        hipLaunchKernelGGL(de_propose_kernel, dim3(L.nmov[par]), dim3(DE_THREADS), 0, st, D, H, L, gs, par, ph);
    return hipGetLastError();
}

hipError_t de_scatter(const McmcDev &D, const DeDev &L, int par, hipStream_t st)
{
    if (L.nmov[par] > 0) hipLaunchKernelGGL(de_scatter_kernel, dim3(L.nmov[par]), dim3(DE_THREADS), 0, st, D, L, par);
    return hipGetLastError();
}

hipError_t de_accept(const McmcDev &D, const NuisDev &N, const PriorDev &P, bool prior_on, const DeDev &L, int par, int ph,
                     int keep_slot, hipStream_t st)
{
    hipLaunchKernelGGL(de_accept_kernel, dim3(D.nchains), dim3(DE_THREADS), 0, st, D, N, P, prior_on ? 1 : 0, L, par, ph,
                       keep_slot);
    if (keep_slot >= 0) return mcmc_keep(D, keep_slot, st);
    return hipGetLastError();
}
