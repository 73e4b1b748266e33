// posterior.h -- streaming posterior accumulators of a sampler (not public;
// the C-ABI is in include/mceik.h, the scheme in DESIGN.md s.10).
#pragma once
#include <hip/hip_runtime.h>

#include "mcmc_common.h"

#define MCEIK_POST_MAX_BINS 128

// Device accumulators.  Velocities are integers, so the sums are exact and do
// not depend on the order in which states, chains or pipes are added.
struct PostDev {
    int per_chain;                 // 1: sum/sumsq [nchains][ncm]; 0: [ncm] pooled over chains
    int nbins;                     // histogram bins per entry (0: none)
    long long *sum, *sumsq;
    unsigned *hist;                // [ncm][nbins] pooled over chains
};

struct McmcPost;                   // a sampler's posterior state (posterior.hip)

// What posterior.hip needs of a sampler (sampler_api.hip fills it).
struct McmcPostCtx {
    int device;
    hipStream_t stream;
    const McmcDev *D;
    McmcPost **slot;               // the sampler's posterior pointer (null: off)
    int ncold;                     // chains the posterior sees: [0, ncold) (parallel tempering: the cold ones)
};
int mcmc_post_ctx(mceik_mcmc *s, McmcPostCtx *out);

// The step loop's side (sampler.hip mcmc_steps): add the current models of the
// chains in view V (chains [chain_off, chain_off + V.nchains) of the sampler)
// on stream st; once every chain of a kept step is queued, count the state.
hipError_t mcmc_post_accumulate(McmcPost *p, const McmcDev &V, int chain_off, hipStream_t st);
void mcmc_post_counted(McmcPost *p);
long long mcmc_post_count(const McmcPost *p);   // states accumulated per chain
void mcmc_post_free(McmcPost *p);
