// ess.h -- streaming effective sample sizes of a sampler by batch means
// (ess.hip; the C-ABI is in include/mceik.h mceik_mcmc_ess_*, the scheme in
// DESIGN.md s.19; not public).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mceik.h"
#include "cov.h"
#include "hypo.h"
#include "mcmc_common.h"
#include "nuis.h"

// Device accumulators.  An entry is one of the ncm model cells or, after them,
// one of np probe scalars (cov.h's kinds); ne = ncm + np.  Batch sizes are 2^l,
// l = 0 .. nlevels - 1.  Everything is an exact integer sum, so it does not
// depend on the order in which chains, pipes or launches are added.
// Wrap bounds, with x the largest |value| of an entry, n states per chain and
// M chains:
//   pend  int32: a level-l batch sum is at most x 2^l; enable refuses x 2^(nlevels - 2) >= 2^31
//   Sc    int64: wraps after 2^63 / x states of a chain (1e15 at x = 9000)
//   A     int64: wraps after 2^63 / x states over all chains
//   Q     128 bits: at most M n 2^l x^2; P 128 bits: at most M (n x)^2 -- both
//         below 2^127 while Sc and A hold (M < 2^32)
// Q is unsigned.  P's increments b (2 Sc - b) and A's are negative where a
// probe is (station statics): both are two's complement, as are the adds.
// Per-chain arrays are indexed by the sampler's chain; a pipe's launch offsets
// them (ess.hip ess_accumulate's chain_off).  The pooled words are shared: every
// block adds atomically.
struct EssDev {
    int nlevels, ncm, np, ne;
    size_t pend_stride;            // words between two levels of pend: nchains (the sampler's) * ne
    const int *kind, *index;       // [np] the probe list
    long long *Sc;                 // [nchains][ne] cumulative sum of a chain's states
    int *pend;                     // [nlevels - 1][nchains][ne] first half of the open level-(l + 1) batch
    long long *A;                  // [nlevels][ne] sum over chains of the closed level-l batches
    unsigned long long *Q, *P;     // [nlevels][ne][2] (lo, hi): sum of B^2; sum over chains of Sc^2 at the last close
};

// The batch-means sums' row of mceik_mcmc::kept (kept.h), off.
KeptStream mcmc_ess_stream();
