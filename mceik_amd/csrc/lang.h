// lang.h -- gradient-informed (discrete Langevin) moves of the sampler
// (lang.hip; include/mceik.h mceik_mcmc_lang_*): device state,
// the per-cell proposal (host and device) and launchers (not public).
//
// A Langevin step moves every cell of one phase model of a chain at once, cell
// i by delta_i drawn from q_i(delta) ~ exp(0.5 d_i delta - delta^2 / (2
// sigma^2)) over the integers that keep the cell inside its box, d_i the
// derivative of the chain's tempered log posterior with respect to v_i (the
// adjoint's gradient, adjoint.hip, plus the prior's).  The proposal is not
// symmetric: the accept test carries lqr - lqf, the log proposal densities of
// the reverse and the forward move, which needs the gradient at the proposed
// state too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block.h"
#include "hypo.h"
#include "mcmc_common.h"
#include "mcmc_device.h"
#include "nuis.h"
#include "prior.h"

#define MCEIK_LANG_DMAX 32         // cap on dmax: a support holds at most 65 values
#define MCEIK_LANG_STREAM 4u       // counter word 2: proposals 0, swaps 1, hypocentres 2, nuisance moves 3
#define LANG_THREADS 256           // one workgroup per chain; the partial sums of the reduction

// Per-chain arrays are views (sampler.hip dev_view): a pipe's LangDev points at
// its chains' rows.
struct LangDev {
    double c;                      // 1 / (2 sigma^2), computed once on the host
    int dmax;
    const unsigned char *skip;     // [nphase][nstat] the sampler's skip rows, or null
    int *delta;                    // [nchains][ncell] the last step's move of the drawn phase
    int *vprop;                    // [nchains][nphase][ncell] the proposed models
    double *g0, *g1;               // [nchains][ncell] d logL / d slowness of the drawn phase at v, v'
    double *lq;                    // [nchains][3] lqf, lqr, logL'
    int *nmove;                    // [nchains] cells with delta != 0
    int *status;                   // [nchains] 1: a solve of the step failed (the step is a rejection)
    float *tt0;                    // [nchains][nstat][nev] tables of the drawn phase at v
    int *ierr0, *ierr1;            // [nchains][nstat] the forwards' ierr at v, v'
    int *ast0, *ast1;              // [nchains][nstat] the adjoint solves' status at v, v'
    int *niter;                    // [nchains][nstat] scratch of the forwards with fields
    unsigned long long *pen;       // [4][nchains * nphase] Es, Ed at v | Es, Ed at v' (prior on)
    size_t pen_stride;             // the sampler's nchains * nphase
    unsigned long long *cnt;       // [nchains][4] attempts, accepts, failed, cells moved
};

// The fields, workspaces and pick weights of one pipe (host side): a step
// walks the pipe's chains in chunks of `chunk`.
struct LangPipe {
    void *base;                    // one allocation
    void *u, *fws, *aws;
    double *ev_w;                  // [chunk][nstat][nev]
    double *gsolve;                // [chunk][nstat][ncell] the adjoint's per-solve rows (one workgroup per solve)
    size_t fws_bytes, aws_bytes;
    int chunk;
};

static inline __host__ __device__ double lang_log(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return mcmcd::det_log(x);
#else
    return hypo_det_log_host(x);
#endif
}

// The support of cell's proposal and its normalisation: the integers lo..hi, a
// of a value, amax and log Z (every loop runs at most 2 dmax +
// 1 times).
struct LangCell {
    int lo, hi;
    double hd, c, amax, Z, logZ;
};

static inline __host__ __device__ double lang_a(const LangCell &S, int delta)
{
    return S.hd * (double)delta - S.c * (double)(delta * delta);
}

static inline __host__ __device__ LangCell lang_cell(double d, int v, int vlo, int vhi, double c, int dmax)
{
    LangCell S;
    S.lo = vlo - v > -dmax ? vlo - v : -dmax;
    S.hi = vhi - v < dmax ? vhi - v : dmax;
    S.hd = 0.5 * d;
    S.c = c;
    S.amax = lang_a(S, S.lo);
    for (int k = S.lo + 1; k <= S.hi; k++) {
        const double a = lang_a(S, k);
        if (a > S.amax) S.amax = a;
    }
    double Z = 0.0;
    for (int k = S.lo; k <= S.hi; k++) Z = Z + mcmcd::det_exp(lang_a(S, k) - S.amax);
    S.Z = Z;
    S.logZ = lang_log(Z);
    return S;
}

static inline __host__ __device__ double lang_logq(const LangCell &S, int delta)
{
    return (lang_a(S, delta) - S.amax) - S.logZ;
}

// The draw: the first delta whose cumulative weight passes u Z, else hi.
static inline __host__ __device__ int lang_pick(const LangCell &S, double u)
{
    const double target = u * S.Z;
    double cum = 0.0;
    for (int k = S.lo; k <= S.hi; k++) {
        const double w = mcmcd::det_exp(lang_a(S, k) - S.amax);
        if (cum + w > target) return k;
        cum = cum + w;
    }
    return S.hi;
}

// The uniform of cell i of global chain g at step gs (cell 0xFFFFFFFF: the step draw's words in r).
static inline __host__ __device__ double lang_uniform(uint32_t seed, uint32_t g, uint64_t gs, uint32_t cell, uint32_t r[4])
{
    r[0] = (uint32_t)gs; r[1] = (uint32_t)(gs >> 32); r[2] = MCEIK_LANG_STREAM; r[3] = cell;
    nuis_philox(r, g, seed);
    return ((double)r[0] + 0.5) * (1.0 / 4294967296.0);
}

// The step draw (phase, log u); the forwards, pick weights and adjoints of the
// two states are the caller's (sampler.hip lang_step).
hipError_t lang_draw(const McmcDev &D, const LangDev &L, uint64_t gs, hipStream_t st);
// ev_w [n][nstat][nev] of chains [c0, c0 + n) of D / N: d logL / d t of every
// (station, event) time of the chain's drawn phase, its tables from D.ttab, the
// other phase's from D.ttab_cur.
hipError_t lang_weights(const McmcDev &D, const NuisDev &N, int c0, int n, double *ev_w, hipStream_t st);
// The proposal from g0 (delta, vprop, slow_prop, lqf), and lqr from g1.
hipError_t lang_propose(const McmcDev &D, const BlockDev &B, const PriorDev &P, bool prior_on, const LangDev &L,
                        uint64_t gs, hipStream_t st);
hipError_t lang_reverse(const McmcDev &D, const BlockDev &B, const PriorDev &P, bool prior_on, const LangDev &L,
                        hipStream_t st);
// The accept test, the commit or the revert, the counters and (keep_slot >= 0) the kept state.
hipError_t lang_accept(const McmcDev &D, const NuisDev &N, const PriorDev &P, bool prior_on, const LangDev &L,
                       int keep_slot, hipStream_t st);
