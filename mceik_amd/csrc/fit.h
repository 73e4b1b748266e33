// fit.h -- streaming data-fit sums of a sampler: pick residuals, origin times
// and the histogram of the standardised residuals (fit.hip; the C-ABI is in
// include/mceik.h mceik_mcmc_fit_*, the scheme in DESIGN.md s.20; not public).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mceik.h"
#include "hypo.h"
#include "mcmc_common.h"
#include "nuis.h"

// Device state.  Per kept step and cold chain every event's origin time t0 and
// every used pick's residual r and standardised residual z are formed with
// event_obj's arithmetic from the chain's current tables (D.ttab_cur), turned
// into integers (q = r / tick, zq = 1024 z, tq = (t0 - t0_ref) / tick, each
// rounded half-even and clamped to +-(2^31 - 1)) and added to exact sums, so
// nothing depends on the order in which chains, pipes or launches are added.
// Wrap bounds: |q| < 2^31, so an int64 sum holds 2^32 states (over all chains)
// and a 128-bit sum of squares never wraps before it.
// The scratch rows are indexed by the sampler's chain; a pipe's launch offsets
// them (mcmc_fit_accumulate's chain_off).  The pooled words are shared: every
// block adds atomically.
struct FitDev {
    int nobs, nev, nbins;
    double inv_tick;               // 1 / tick: a power of two
    double hscale, half;           // nbins / (2 zmax), nbins / 2
    const double *t0_ref;          // [nev]
    int *q, *zq, *bin;             // [nchains][nobs] the last kept step's words (bin -1: a masked pick)
    int *tq;                       // [nchains][nev]
    long long *sq, *szq;           // [nobs] sums of q, zq
    unsigned long long *sq2, *szq2;    // [nobs][2] (lo, hi): sums of q^2, zq^2
    long long *stq;                // [nev]
    unsigned long long *stq2;      // [nev][2]
    unsigned long long *hist;      // [nphase][nstat][nbins]
    unsigned long long *sat;       // [3] clamped q, zq, tq
};

struct McmcFit;                    // a sampler's data-fit state (fit.hip)

// The kept-state hook's side (sampler.hip kept_queue), in posterior.h's
// convention: the first n chains of view D / H / N, which are chains
// [chain_off, chain_off + n) of the sampler, are added; once every chain of a
// kept step is queued, count the state.  D.ttab_cur holds the chains' current
// tables (at the chains' own event nodes: H is not read).
hipError_t mcmc_fit_accumulate(McmcFit *p, const McmcDev &D, const HypoDev &H, const NuisDev &N, int chain_off, int n,
                               hipStream_t st);
void mcmc_fit_counted(McmcFit *p);
long long mcmc_fit_count(const McmcFit *p);   // states accumulated per chain
void mcmc_fit_free(McmcFit *p);
