// nuis.hip -- noise-scale and station-static moves of the GPU sampler
// (include/mceik.h mceik_mcmc_nuis_*), on gfx950.
//
// objfn_e depends on the pick uncertainty and the station statics only
// through tobs - tcorr and 1 / var: the travel-time tables of the chain's
// current models serve every candidate, so a move needs no eikonal solve.
// One 64-lane wave per chain runs the step's nsub sub-moves in sequence: the
// lanes take the events, objfn_e goes to LDS, every lane sums it in event
// order and takes the same decision.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_common.h"
#include "mcmc_device.h"
#include "mcmc_host.h"
#include "nuis.h"

namespace {

// A candidate of chain c: the ladder values of both phases and, for a statics
// move, the two stations of phase ph whose static differs from the LDS copy.
struct NuisCand {
    double lam0, lam1;
    int ph, sa, sb, va, vb;        // ph < 0: the statics are the LDS copy's
};

// mcmc_device.h event_obj's arithmetic (the same operations in the same
// order) on the effective observations of the candidate, each formed by its
// one fp64 operation: var[j] * lam and tcorr[j] + (double)kc * dt.  The
// travel times come from LDS (te) or, where they do not fit, from the chain's
// current tables.
__device__ __forceinline__ double nuis_event_obj(const McmcDev &D, const NuisDev &N, const float *tcur, const float *te,
                                                 const int *skc, const NuisCand &k, int e)
{
    const double sqrt2i = 0.7071067811865475;
    auto ph_of = [&](int j) -> int { return D.obs_phase ? D.obs_phase[j] : 0; };
    auto te_of = [&](int j) -> double {
        if (te) return (double)te[j];
        return (double)tcur[((size_t)ph_of(j) * D.nstat + D.obs_stat[j]) * D.nev + e];
    };
    auto var_of = [&](int j) -> double { return N.var0[j] * (ph_of(j) ? k.lam1 : k.lam0); };
    auto tcorr_of = [&](int j) -> double {
        const int ph = ph_of(j), st = D.obs_stat[j];
        int kc = skc[ph * D.nstat + st];
        if (ph == k.ph) kc = st == k.sa ? k.va : st == k.sb ? k.vb : kc;
        return N.tcorr0[j] + (double)kc * N.dt;
    };
    const int j0 = D.obs_ptr[e], j1 = D.obs_ptr[e + 1];
    if (D.l1)                       // the L1 likelihood: mcmc_device.h event_obj_l1's arithmetic on the candidate
        return l1::event<double>(j0, j1, [&](int j) -> bool { return !D.obs_mask[j]; },
                                 [&](int j) -> double { return (D.tobs[j] - tcorr_of(j)) - te_of(j); },
                                 [&](int j) -> double { return 1.0 / var_of(j); }, nullptr);
    double xnorm = 0.0, t0 = 0.0, obj = 0.0;
    for (int j = j0; j < j1; j++) if (!D.obs_mask[j]) xnorm = xnorm + 1.0 / var_of(j);
    for (int j = j0; j < j1; j++) {
        if (D.obs_mask[j]) continue;
        double t = te_of(j);
        double tc = D.tobs[j] - tcorr_of(j);
        t0 = t0 + ((1.0 / var_of(j)) / xnorm) * (tc - t);
    }
    for (int j = j0; j < j1; j++) {
        if (D.obs_mask[j]) continue;
        double t = te_of(j);
        double tc = D.tobs[j] - tcorr_of(j);
        double res = ((1.0 / var_of(j)) * sqrt2i) * (tc - (t + t0));
        obj = obj + res * res;
    }
    return obj;
}

// One block (one wave) per chain.  LDS: obj [nev] doubles | kc [nphase][nstat]
// ints | with N.lds_te the travel time of every observation, [nobs] floats.
__global__ __launch_bounds__(64) void nuis_step_kernel(McmcDev D, NuisDev N, uint64_t gs, int keep_slot)
{
    extern __shared__ double nuis_sm[];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int nph = D.nphase, nps = nph * D.nstat;
    double *sobj = nuis_sm;
    int *skc = (int *)(sobj + D.nev);
    float *ste = N.lds_te ? (float *)(skc + nps) : nullptr;
    const float *tcur = D.ttab_cur + (size_t)c * nps * D.nev;
    int *kcrow = N.kc + (size_t)c * nps;
    for (int i = lane; i < nps; i += 64) skc[i] = kcrow[i];
    if (ste)
        for (int e = lane; e < D.nev; e += 64)
            for (int j = D.obs_ptr[e]; j < D.obs_ptr[e + 1]; j++) {
                const int ph = D.obs_phase ? D.obs_phase[j] : 0;
                ste[j] = tcur[((size_t)ph * D.nstat + D.obs_stat[j]) * D.nev + e];
            }
    __syncthreads();
    int kn0 = N.kn[(size_t)c * nph], kn1 = nph > 1 ? N.kn[(size_t)c * nph + 1] : 0;
    double logl = D.logl[c];
    const int nnoise = N.noise_on ? nph : 0;
    for (int sub = 0; sub < N.nsub; sub++) {
        int m[5];
        const uint32_t r3 = nuis_draw(D.seed, (uint32_t)(D.chain_offset + c), gs, sub, nnoise, N.nact0, N.nact1, N.dk,
                                      N.dc, m);
        const double logu = mcmcd::det_log(((double)r3 + 0.5) * (1.0 / 4294967296.0));
        const int ph = m[1];
        int c0 = kn0, c1 = kn1, par, partner = -1, cand;
        NuisCand k;
        k.ph = -1; k.sa = k.sb = -1; k.va = k.vb = 0;
        bool inside;
        if (m[0] == 0) {
            cand = (ph ? kn1 : kn0) + m[4];
            inside = cand >= 0 && cand < N.nk;
            if (ph) c1 = cand; else c0 = cand;
            par = ph;
        } else {
            k.ph = ph;
            k.sa = N.act[ph * D.nstat + m[2]];
            k.sb = N.act[ph * D.nstat + m[3]];
            k.va = skc[ph * D.nstat + k.sa] + m[4];
            k.vb = skc[ph * D.nstat + k.sb] - m[4];
            inside = k.va >= -N.kcmax && k.va <= N.kcmax && k.vb >= -N.kcmax && k.vb <= N.kcmax;
            par = nph + ph * D.nstat + k.sa;
            partner = nph + ph * D.nstat + k.sb;
            cand = k.va;
        }
        double ln = logl;
        int acc = 0;
        if (inside) {                   // wave-uniform: every lane drew the same move
            k.lam0 = N.lam[c0];
            k.lam1 = N.lam[c1];
            for (int e = lane; e < D.nev; e += 64) sobj[e] = nuis_event_obj(D, N, tcur, ste, skc, k, e);
            __syncthreads();
            ln = 0.0;
            for (int e = 0; e < D.nev; e++) ln = ln - sobj[e];
            ln = ln - N.norm0 * N.lnlam[c0];
            if (nph > 1) ln = ln - N.norm1 * N.lnlam[c1];
            const double d = ln - logl;
            acc = D.beta ? logu < D.beta[c] * d : logu < d;
        }
        __syncthreads();                // sobj and skc are read: the next writes may follow
        if (lane == 0) {
            const size_t r = (size_t)c * N.nsub + sub;
            N.rec[4 * r] = par; N.rec[4 * r + 1] = partner; N.rec[4 * r + 2] = cand; N.rec[4 * r + 3] = acc;
            N.rlogl[2 * r] = logl; N.rlogl[2 * r + 1] = ln;
            atomicAdd(&N.attempts[par], 1ull);
            if (partner >= 0) atomicAdd(&N.attempts[partner], 1ull);
            if (acc) {
                atomicAdd(&N.accepts[par], 1ull);
                if (partner >= 0) atomicAdd(&N.accepts[partner], 1ull);
                if (m[0] == 1) {
                    skc[ph * D.nstat + k.sa] = k.va;
                    skc[ph * D.nstat + k.sb] = k.vb;
                }
            }
        }
        if (acc) {
            kn0 = c0;
            kn1 = c1;
            logl = ln;
        }
        __syncthreads();
    }
    // the accepted state, the chain's effective rows, logL; the step proposed no velocity: its accept flag is 0
    for (int i = lane; i < nps; i += 64) kcrow[i] = skc[i];
    const double l0 = N.lam[kn0], l1 = N.lam[kn1];
    double *ve = N.var_eff + (size_t)c * N.nobs, *tce = N.tcorr_eff + (size_t)c * N.nobs;
    for (int j = lane; j < N.nobs; j += 64) {
        const int ph = D.obs_phase ? D.obs_phase[j] : 0;
        ve[j] = N.var0[j] * (ph ? l1 : l0);
        tce[j] = N.tcorr0[j] + (double)skc[ph * D.nstat + D.obs_stat[j]] * N.dt;
    }
    if (lane == 0) {
        N.kn[(size_t)c * nph] = kn0;
        if (nph > 1) N.kn[(size_t)c * nph + 1] = kn1;
        D.logl[c] = logl;
        D.accept[c] = 0;
        if (keep_slot >= 0) D.keep_logl[(size_t)keep_slot * D.keep_stride + c] = logl;
    }
}

// The effective rows of every chain from its kn / kc: one thread per (chain, observation).
__global__ __launch_bounds__(256) void nuis_rows_kernel(McmcDev D, NuisDev N)
{
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= (size_t)D.nchains * N.nobs) return;
    const int c = (int)(i / N.nobs), j = (int)(i - (size_t)c * N.nobs);
    const int ph = D.obs_phase ? D.obs_phase[j] : 0;
    N.var_eff[i] = N.var0[j] * N.lam[N.kn[(size_t)c * D.nphase + ph]];
    N.tcorr_eff[i] = N.tcorr0[j] + (double)N.kc[((size_t)c * D.nphase + ph) * D.nstat + D.obs_stat[j]] * N.dt;
}

// Exact integer sums over the first ncold chains (any order adds up): thread
// i < nphase is phase i's ladder index (k, k^2, histogram), the others one
// (phase, station) each (kc, kc^2).
__global__ __launch_bounds__(64) void nuis_moments_kernel(McmcDev D, NuisDev N, int ncold)
{
    const int i = blockIdx.x * 64 + threadIdx.x, nph = D.nphase, nps = nph * D.nstat;
    if (i >= nph + nps) return;
    unsigned long long *mom = reinterpret_cast<unsigned long long *>(N.mom);
    long long s = 0, q = 0;
    if (i < nph) {
        for (int c = 0; c < ncold; c++) {
            const long long k = N.kn[(size_t)c * nph + i];
            s += k;
            q += k * k;
            atomicAdd(mom + 2 * nph + (size_t)i * N.nk + k, 1ull);
        }
        atomicAdd(mom + 2 * i, (unsigned long long)s);
        atomicAdd(mom + 2 * i + 1, (unsigned long long)q);
        return;
    }
    const int t = i - nph;
    for (int c = 0; c < ncold; c++) {
        const long long k = N.kc[(size_t)c * nps + t];
        s += k;
        q += k * k;
    }
    unsigned long long *ms = mom + 2 * nph + (size_t)nph * N.nk;
    atomicAdd(ms + 2 * t, (unsigned long long)s);
    atomicAdd(ms + 2 * t + 1, (unsigned long long)q);
}

}  // namespace

size_t nuis_lds_bytes(const McmcDev &D, const NuisDev &N, bool with_te)
{
    return (size_t)D.nev * 8 + (size_t)D.nphase * D.nstat * 4 + (with_te ? (size_t)N.nobs * 4 : 0);
}

hipError_t nuis_step(const McmcDev &D, const NuisDev &N, uint64_t gs, int keep_slot, hipStream_t st)
{
    // the observations' travel times in LDS where they fit (N.lds_te), else read from the tables at every use
    hipLaunchKernelGGL(nuis_step_kernel, dim3(D.nchains), dim3(64), nuis_lds_bytes(D, N, N.lds_te != 0), st, D, N, gs,
                       keep_slot);
    if (keep_slot >= 0) return mcmc_keep(D, keep_slot, st);
    return hipGetLastError();
}

hipError_t nuis_rows(const McmcDev &D, const NuisDev &N, hipStream_t st)
{
    const size_t n = (size_t)D.nchains * N.nobs;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(nuis_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, D, N);
    return hipGetLastError();
}

hipError_t nuis_moments(const McmcDev &D, const NuisDev &N, int ncold, hipStream_t st)
{
    if (ncold <= 0) return hipSuccess;
    const int n = D.nphase + D.nphase * D.nstat;
    hipLaunchKernelGGL(nuis_moments_kernel, dim3((n + 63) / 64), dim3(64), 0, st, D, N, ncold);
    return hipGetLastError();
}
