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

// The kept-state hook's side (sampler.hip kept_queue): add the current models
// of the first n chains of view D, which are chains [chain_off, chain_off + n)
// of the sampler, on stream st; once every chain of a kept step is queued,
// count the state.  cov.h and ess.h take their chains the same way.
hipError_t mcmc_post_accumulate(McmcPost *p, const McmcDev &D, int chain_off, int n, hipStream_t st);
void mcmc_post_counted(McmcPost *p);
long long mcmc_post_count(const McmcPost *p);   // states accumulated per chain
void mcmc_post_free(McmcPost *p);
