// kept.h -- one record for the sampler's accumulators of kept states: the
// streaming posterior (posterior.hip), the probe-to-cell covariances (cov.hip),
// the batch-means sums (ess.hip) and the data-fit sums (fit.hip); DESIGN.md
// s.25; not public.
//
// Each of the four files builds its device struct and says which arrays hold
// its sums (KeptArray); everything that only walks that list -- allocate
// zeroed, free, copy out, copy in -- is here, once.  The lifecycle over a
// sampler (enable's tail, disable, clear, accumulate, get, set) is declared in
// sampler.h and lives in sampler_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct McmcDev;
struct HypoDev;
struct NuisDev;

#define KEPT_MAX_ARRAYS 8
enum { KEPT_POST, KEPT_COV, KEPT_ESS, KEPT_FIT, KEPT_NSTREAM };   // mceik_mcmc::kept's rows, in hook order

// One accumulator array: where its device pointer lives, the bytes get / set
// move (0: the array does not exist with these options) and the bytes
// allocated past them.
struct KeptArray {
    void **dev;
    size_t bytes, slack;
};

// One accumulator of kept states.  state is null until an enable and again
// after a clear; on: kept steps add to it; n: states accumulated per chain.
// The functions take state as the file that set them made it.
struct KeptStream {
    void *state;
    bool on;
    long long n;
    const char *name;                  // for messages: "the covariance sums", ...
    bool needs_tables1;                // while on, a one-model sampler holds its current tables (mcmc_tables1_hold)
    // The arrays of the sums, in the order of the stream's get / set; returns how many.
    int (*arrays)(void *state, KeptArray out[KEPT_MAX_ARRAYS]);
    // Add the first n chains of view D / H / N, which are chains [chain_off,
    // chain_off + n) of the sampler, on stream st (n > 0); `count` states are
    // in the sums already, the same for every pipe of a kept step.
    hipError_t (*accumulate)(void *state, const McmcDev &D, const HypoDev &H, const NuisDev &N, int chain_off, int n,
                             long long count, hipStream_t st);
    void (*free_extra)(void *state);   // frees what `arrays` does not list, and state itself
    bool (*holds_nuis)(const void *state);   // a static or noise-index probe is registered (null: never)
};

// Every array of the list allocated and zeroed (one that is empty, slack included, stays null).
static inline bool kept_arrays_alloc(const KeptArray *a, int na)
{
    for (int k = 0; k < na; k++) {
        const size_t bytes = a[k].bytes + a[k].slack;
        if (!bytes) continue;
        if (hipMalloc(a[k].dev, bytes) != hipSuccess || hipMemset(*a[k].dev, 0, bytes) != hipSuccess) return false;
    }
    return true;
}

static inline void kept_arrays_free(const KeptArray *a, int na)
{
    for (int k = 0; k < na; k++) {
        if (*a[k].dev) (void)hipFree(*a[k].dev);
        *a[k].dev = nullptr;
    }
}

// The sums zeroed in place on stream st.
static inline hipError_t kept_arrays_zero(const KeptArray *a, int na, hipStream_t st)
{
    for (int k = 0; k < na; k++) {
        if (!a[k].bytes) continue;
        const hipError_t e = hipMemsetAsync(*a[k].dev, 0, a[k].bytes, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// set's rule: every array that exists needs its host side.
static inline bool kept_arrays_missing(const KeptArray *a, int na, const void *const *host)
{
    for (int k = 0; k < na; k++)
        if (a[k].bytes && !host[k]) return true;
    return false;
}

// get (to_host) / set: the arrays that exist and whose host side is given.
static inline hipError_t kept_arrays_copy(const KeptArray *a, int na, void *const *host, bool to_host)
{
    for (int k = 0; k < na; k++) {
        if (!a[k].bytes || !host[k]) continue;
        const hipError_t e = to_host ? hipMemcpy(host[k], *a[k].dev, a[k].bytes, hipMemcpyDeviceToHost)
                                     : hipMemcpy(*a[k].dev, host[k], a[k].bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
