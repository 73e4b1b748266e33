// cov.h -- streaming probe-to-cell covariances of a sampler (cov.hip; the
// C-ABI is in include/mceik.h mceik_mcmc_cov_*, the scheme in DESIGN.md s.16;
// not public).
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/mceik.h"
#include "hypo.h"
#include "kept.h"
#include "mcmc_common.h"
#include "nuis.h"

// Device accumulators.  A probe is one int32 scalar of a chain (kind, index):
// 0 v[c][index], 1 hyp[c][index] (index = 3 e + axis), 2 kc[c][index] (index =
// ph nstat + stat), 3 kn[c][index].  Everything is an exact integer sum, so it
// does not depend on the order in which states, chains or pipes are added.
// Wrap bound: a word wraps after 2^63 / (max |x| * vmax) accumulated states
// (chains x kept steps), more than 1e11 at the default prior (|x|, v <= 9000).
// Per-chain arrays are indexed by the sampler's chain; a pipe's launch offsets
// them (cov.hip cov_accumulate's chain_off).  The pooled sums are shared: pipes
// add atomically.
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

// A registered probe list, as cov.hip and ess.hip hold theirs: the host copy
// and the device copy [2][np] (kind, index) the kernels read.
struct ProbeList {
    int np;
    int kind[MCEIK_COV_MAX_PROBES], index[MCEIK_COV_MAX_PROBES];
    int *d;                        // kind = d, index = d + np (one word more than 2 np: np may be 0)
};

static inline bool probes_same(const ProbeList &L, int n, const int *kind, const int *index)
{
    return n == L.np && !memcmp(L.kind, kind, sizeof(int) * n) && !memcmp(L.index, index, sizeof(int) * n);
}

static inline bool probes_hold_nuis(const ProbeList &L)     // a static or noise-index probe is registered
{
    for (int k = 0; k < L.np; k++)
        if (L.kind[k] >= 2) return true;
    return false;
}

static inline bool probes_upload(ProbeList &L, int n, const int *kind, const int *index)     // allocates L.d
{
    L.np = n;
    memcpy(L.kind, kind, sizeof(int) * n);
    memcpy(L.index, index, sizeof(int) * n);
    return hipMalloc((void **)&L.d, (2 * (size_t)n + 1) * sizeof(int)) == hipSuccess &&
           (!n || (hipMemcpy(L.d, kind, n * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
                   hipMemcpy(L.d + n, index, n * sizeof(int), hipMemcpyHostToDevice) == hipSuccess));
}

// The covariances' row of mceik_mcmc::kept (kept.h), off.
KeptStream mcmc_cov_stream();
