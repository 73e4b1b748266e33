// nuis.h -- noise-scale and station-static moves of the GPU sampler (nuis.hip;
// include/mceik.h mceik_mcmc_nuis_*): device state, the draw
// (host and device) and launchers (not public).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_common.h"

// Per-chain arrays are views (sampler.hip dev_view): a pipe's NuisDev points
// at its chains' rows.  The tables, counters and moments are the sampler's.
// kn == null: the sampler holds no nuisance state and every kernel that takes
// a NuisDev computes what it computed without one.
struct NuisDev {
    int nobs, nk, dk, dc, kcmax, nsub;
    int noise_on, statics_on;      // which parts the sub-moves draw from
    int lds_te;                    // a nuisance step stages the observations' travel times in LDS (they fit)
    int nact0, nact1;              // stations with a used pick of phase 0 / 1 that statics moves draw from (0 where < 2)
    double dt, norm0, norm1;
    const double *lam, *lnlam;     // [nk] the noise ladder and its logarithms (the host's tables)
    const int *act;                // [nphase][nstat] the active stations of each phase, in station order
    int *kn;                       // [nchains][nphase] ladder index
    int *kc;                       // [nchains][nphase][nstat] static in units of dt
    double *var_eff, *tcorr_eff;   // [nchains][nobs] the chains' effective observations
    const double *var0, *tcorr0;   // [nobs] the catalogue's
    int *rec;                      // [nchains][nsub][4] last nuisance step: parameter, partner, candidate, accepted
    double *rlogl;                 // [nchains][nsub][2] last nuisance step: logL, logL'
    unsigned long long *attempts, *accepts;   // [nphase + nphase * nstat] over chains
    long long *mom;                // [nphase][2] sums of k, k^2 | [nphase][nk] histogram | [nphase][nstat][2] sums of kc, kc^2
};

#define MCEIK_NUIS_STREAM 3u       // counter word 2: proposals 0, swaps 1, hypocentres 2
#define MCEIK_NUIS_LDS_MAX 65536   // bytes of LDS a nuisance step's block may use (MCEIK_NUIS_LDS: a test hook lowers it)

// Sub-move `sub` of global chain g at step gs (host and device): Philox4x32-10,
// counter {gs lo, gs hi, 3, sub}, key {g, seed}, outputs r0..r3.  M = (noise:
// nphase) + (statics: nact0 + nact1) moves; q = (r0 M) >> 32 picks a noise move
// of phase q, or station a (index into the phase's active list) of a statics
// move.  m = {kind (0 noise, 1 statics), phase, a, b, signed delta}; returns r3.
static inline __host__ __device__ void nuis_philox(uint32_t c[4], uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

static inline __host__ __device__ uint32_t nuis_draw(uint32_t seed, uint32_t g, uint64_t gs, int sub, int nnoise,
                                                     int nact0, int nact1, int dk, int dc, int m[5])
{
    uint32_t c[4] = {(uint32_t)gs, (uint32_t)(gs >> 32), MCEIK_NUIS_STREAM, (uint32_t)sub};
    nuis_philox(c, g, seed);
    const int M = nnoise + nact0 + nact1;
    int q = (int)(((uint64_t)c[0] * (uint32_t)M) >> 32);
    const int minus = (int)(c[2] & 1u);
    if (q < nnoise) {
        const int d = 1 + (int)(((uint64_t)c[1] * (uint32_t)dk) >> 32);
        m[0] = 0; m[1] = q; m[2] = 0; m[3] = 0; m[4] = minus ? -d : d;
        return c[3];
    }
    q -= nnoise;
    const int ph = q < nact0 ? 0 : 1, a = ph ? q - nact0 : q, na = ph ? nact1 : nact0;
    int b = (int)(((uint64_t)c[1] * (uint32_t)(na - 1)) >> 32);
    b += b >= a;
    const int mag = 1 + (int)(((uint64_t)(c[2] >> 1) * (uint32_t)dc) >> 31);
    m[0] = 1; m[1] = ph; m[2] = a; m[3] = b; m[4] = minus ? -mag : mag;
    return c[3];
}

#ifdef __HIPCC__
// What the kernels that evaluate logL do with the state: chain c's view of D
// with var / tcorr at its effective rows (mcmc_device.h event_obj serves
// unchanged), and the noise normalisation after the events' sum.
__device__ __forceinline__ McmcDev nuis_chain(const McmcDev &D, const NuisDev &N, int c)
{
    McmcDev E = D;
    if (N.kn) {
        E.var = N.var_eff + (size_t)c * N.nobs;
        E.tcorr = N.tcorr_eff + (size_t)c * N.nobs;
    }
    return E;
}

__device__ __forceinline__ double nuis_logl(const McmcDev &D, const NuisDev &N, int c, double l)
{
    if (!N.kn) return l;
    l = l - N.norm0 * N.lnlam[N.kn[(size_t)c * D.nphase]];
    if (D.nphase > 1) l = l - N.norm1 * N.lnlam[N.kn[(size_t)c * D.nphase + 1]];
    return l;
}
#endif

// One nuisance step of the chains of D / N: nsub sub-moves per chain in one
// launch (and the kept logL / state: keep_slot >= 0).  D.ttab_cur holds the
// chains' current tables.
hipError_t nuis_step(const McmcDev &D, const NuisDev &N, uint64_t gs, int keep_slot, hipStream_t st);
// var_eff / tcorr_eff from kn / kc, every chain of D / N.
hipError_t nuis_rows(const McmcDev &D, const NuisDev &N, hipStream_t st);
// Adds the first ncold chains' kn / kc of N to the moments.
hipError_t nuis_moments(const McmcDev &D, const NuisDev &N, int ncold, hipStream_t st);
// Bytes of LDS a nuisance step's block needs with (with_te) or without the
// observations' travel times staged in it.
size_t nuis_lds_bytes(const McmcDev &D, const NuisDev &N, bool with_te);
