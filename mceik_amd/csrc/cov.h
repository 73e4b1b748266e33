// cov.h -- streaming probe-to-cell covariances of a sampler (cov.hip; the
// C-ABI is in include/mceik.h mceik_mcmc_cov_*, the scheme in DESIGN.md s.16;
// not public).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mceik.h"
#include "hypo.h"
#include "mcmc_common.h"
#include "nuis.h"

// Device accumulators.  A probe is one int32 scalar of a chain (kind, index):
// 0 v[c][index], 1 hyp[c][index] (index = 3 e + axis), 2 kc[c][index] (index =
// ph nstat + stat), 3 kn[c][index].  Everything is an exact integer sum, so it
// does not depend on the order in which states, chains or pipes are added.
// Wrap bound: a word wraps after 2^63 / (max |x| * vmax) accumulated states
// (chains x kept steps), more than 1e11 at the default prior (|x|, v <= 9000).
// Per-chain arrays are views (sampler.hip dev_view): a pipe's CovDev points at
// its chains' rows.  The pooled sums are the sampler's: pipes add atomically.
struct CovDev {
    int np, within, ncm;
    const int *kind, *index;       // [np] the probe list
    int *X;                        // [nchains][np] the probes' values of the state being added
    long long *A;                  // [np] sum of x_p
    long long *G;                  // [np][np] sum of x_p x_q
    long long *S, *Q;              // [ncm] sums of v_j, v_j^2
    long long *C;                  // [np][ncm] sum of x_p v_j
    long long *Ac;                 // within: [nchains][np] per-chain sum of x_p, else null
    long long *Sc;                 // within: [nchains][ncm] per-chain sum of v_j, else null
};

// Where the probes' values of a view's chains live (kind -> base, row length),
// and the probe gather itself: cov.hip's gather kernel and ess.hip's accumulate
// kernel read a probe through the same function.
struct CovSrc {
    const int *v, *hyp, *kc, *kn;
    int sv, shyp, skc, skn;
};

static inline CovSrc cov_src(const McmcDev &D, const HypoDev &H, const NuisDev &N)
{
    CovSrc R;
    R.v = D.v; R.sv = D.ncm;
    R.hyp = H.hyp; R.shyp = 3 * D.nev;
    R.kc = N.kc; R.skc = D.nphase * D.nstat;
    R.kn = N.kn; R.skn = D.nphase;
    return R;
}

// The same as a table by kind, for LDS: lanes of one wave look up different
// kinds, and a select over the kernel's arguments by kind can end up as a copy
// of them in scratch (it did in ess.hip's kernel).
struct CovTab {
    const int *base[4];
    int stride[4];
};

// Fills T (in LDS) from R; the caller synchronises the block before the first look-up.
__device__ __forceinline__ void cov_tab_stage(CovTab &T, const CovSrc &R)
{
    if (threadIdx.x == 0) {
        T.base[0] = R.v; T.base[1] = R.hyp; T.base[2] = R.kc; T.base[3] = R.kn;
        T.stride[0] = R.sv; T.stride[1] = R.shyp; T.stride[2] = R.skc; T.stride[3] = R.skn;
    }
}

// Probe (kind, index): where chain 0 of the view holds it, and the words from one chain to the next.
__device__ __forceinline__ const int *cov_probe_ptr(const CovTab &T, int kind, int index, int *stride)
{
    *stride = T.stride[kind];
    return T.base[kind] + index;
}

// Largest index + 1 of a probe of `kind` while the sampler holds that state, else 0
// (cov.hip; mceik_mcmc_cov_enable and mceik_mcmc_ess_enable validate with it).
long long mcmc_probe_limit(const mceik_mcmc *s, int kind);

struct McmcCov;                    // a sampler's covariance state (cov.hip)

// The step loop's side (sampler.hip mcmc_steps): the device state of p (the
// sampler's view: every chain), and the first n chains of view V added on
// stream st from the chains' state D / H / N of the same view (two launches:
// the probe gather, then the rank-n update); once every chain of a kept step
// is queued, count the state.
CovDev mcmc_cov_dev(const McmcCov *p);
hipError_t mcmc_cov_accumulate(const CovDev &V, const McmcDev &D, const HypoDev &H, const NuisDev &N, int n, hipStream_t st);
void mcmc_cov_counted(McmcCov *p);
bool mcmc_cov_holds_nuis(const McmcCov *p);      // a static or noise-index probe is registered
void mcmc_cov_free(McmcCov *p);
