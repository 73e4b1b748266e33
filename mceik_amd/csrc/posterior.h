// posterior.h -- streaming posterior accumulators of a sampler (not public;
// the C-ABI is in include/mceik.h, the scheme in DESIGN.md s.10).
#pragma once
#include <hip/hip_runtime.h>

#include "kept.h"
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

// The posterior's row of mceik_mcmc::kept (kept.h), off: the kept-state hook
// (sampler.hip kept_queue) and the lifecycle (sampler_api.hip) reach
// posterior.hip through it.
KeptStream mcmc_post_stream();
