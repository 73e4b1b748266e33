// fit.h -- streaming data-fit sums of a sampler: pick residuals, origin times
// and the histogram of the standardised residuals (fit.hip; the C-ABI is in
// include/mceik.h mceik_mcmc_fit_*, the scheme in DESIGN.md s.20; not public).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mceik.h"
#include "hypo.h"
#include "kept.h"
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
// them (fit.hip fit_accumulate's chain_off).  The pooled words are shared: every
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

// The data-fit sums' row of mceik_mcmc::kept (kept.h), off; it is the one that
// makes a one-model sampler hold its current tables while on.
KeptStream mcmc_fit_stream();
