// ess.hip -- streaming effective sample sizes by batch means
// (include/mceik.h mceik_mcmc_ess_*, mceik_ess_*), on gfx950.
//
// Kept states cannot be stored, so the integrated autocorrelation time of
// every model entry (and of a few probe scalars) is streamed: per chain and
// entry the cumulative sum and the open halves of a hierarchy of batches of
// 2^l states, and pooled over the chains per level the exact integer sums of
// the closed batch sums, of their squares and of the squared cumulative sums.
// Integer sums do not depend on the order of accumulation: pipes, launch
// paths, shards and ranks all give the same words, and partials merge by
// plain addition.  tau, ESS and the Monte-Carlo standard error are formed on
// the host from exact 128-bit numerators (mceik_ess_finish: no GPU call).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define HIPCHK_WHO "mceik_ess"
#include "ess.h"
#include "host_util.h"
#include "sampler.h"

#define ESS_TILE 64                // entries per block: lane = entry
#define ESS_SLICE 64               // chains per block: wave w takes chains w, w + 4, ... of the slice

// w (lo, hi) += x modulo 2^128 by two 64-bit vector atomics: the low word
// first, its carry (the returned old value tells) into the high word.  The
// adds of one word are serialised, every wrap of the low word is seen by
// exactly one adder, so the sum is exact in any order.
__device__ __forceinline__ void ess_add128(unsigned long long *w, u128 x)
{
    const unsigned long long lo = (unsigned long long)x;
    unsigned long long hi = (unsigned long long)(x >> 64);
    if (lo) {
        const unsigned long long old = atomicAdd(&w[0], lo);
        hi += (unsigned long long)(old + lo < old);
    }
    if (hi) atomicAdd(&w[1], hi);
}

// One launch adds state number t of the view's chains; k = trailing zero bits
// of t, nl = min(k, nlevels - 1) + 1 <= NL levels close.  A block owns a tile
// of 64 consecutive entries x a slice of 64 chains; lane = entry, so a wave
// reads and writes whole rows of v / Sc / pend (256 / 512 / 256 contiguous
// bytes), U chains in flight.  A step with k = 0 moves 24 B per chain and
// entry (v, Sc twice, pend[0]); every further closing level reads 4 B more.
// The closing levels' partial sums (A 64 bits, Q and P 128 bits: five words a
// level) stay in registers, NL and the level loops being compile-time; the
// four waves' sums meet in LDS, one wave at a time, and leave as 64-bit vector
// atomics, one 128-bit add per word and block: the chain slices and the pipes
// share the pooled words.  A lane past entry ncm reads its probe where cov.h's
// gather finds it.
template <int NL, int U>
__global__ __launch_bounds__(256) void ess_accumulate_kernel(EssDev E, CovSrc R, int nchains, int k, int nl)
{
    __shared__ unsigned long long red[5 * NL][ESS_TILE];
    __shared__ CovTab tab;
    constexpr int NP = NL > 1 ? NL - 1 : 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * ESS_TILE + lane, ne = E.ne, ncm = E.ncm;
    const bool live = i < ne;
    const size_t ii = live ? i : 0;                  // a tail tile's dead lanes read entry 0 and write nothing
    cov_tab_stage(tab, R);
    __syncthreads();
    // the entry's value in chain 0 of the view, and the words to the next chain's: a cell of v or a probe
    const bool cell = ii < (size_t)ncm;
    int vs;
    const int *__restrict__ vp = cov_probe_ptr(tab, cell ? 0 : E.kind[ii - ncm], cell ? (int)ii : E.index[ii - ncm], &vs);
    const int c0 = blockIdx.y * ESS_SLICE;
    const int c1 = nchains < c0 + ESS_SLICE ? nchains : c0 + ESS_SLICE;
    const bool put = k <= E.nlevels - 2;             // the state opens a level-(k + 1) batch: pend[k] takes its first half
    const size_t ps = E.pend_stride;
    long long *__restrict__ Sc = E.Sc;
    int *__restrict__ pend = E.pend;
    long long a[NL];
    u128 q[NL], p[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) { a[l] = 0; q[l] = 0; p[l] = 0; }
    for (int c = c0 + wave; c < c1; c += 4 * U) {
        int v[U], pe[U][NP];
        long long sc[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int cc = c + 4 * u;
            const size_t cl = (size_t)(cc < c1 ? cc : c);
            v[u] = vp[cl * vs];
            sc[u] = Sc[cl * ne + ii];
#pragma unroll
            for (int l = 0; l < NL - 1; l++)
                if (l < nl - 1) pe[u][l] = pend[l * ps + cl * ne + ii];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int cc = c + 4 * u;
            if (cc >= c1) continue;
            const size_t row = (size_t)cc * ne + ii;
            long long b = v[u];
            const long long s = sc[u] + b;
            if (live) Sc[row] = s;
#pragma unroll
            for (int l = 0; l < NL; l++)
                if (l < nl) {
                    a[l] += b;
                    q[l] += (u128)((i128)b * b);
                    p[l] += (u128)((i128)b * (2 * (i128)s - b));
                    if (l < nl - 1) b += pe[u][l];
                }
            if (put && live) pend[(size_t)(nl - 1) * ps + row] = (int)b;
        }
    }
    for (int w = 1; w < 4; w++) {
        if (wave == w) {
#pragma unroll
            for (int l = 0; l < NL; l++)
                if (l < nl) {
                    red[5 * l][lane] = (unsigned long long)a[l];
                    red[5 * l + 1][lane] = (unsigned long long)q[l];
                    red[5 * l + 2][lane] = (unsigned long long)(q[l] >> 64);
                    red[5 * l + 3][lane] = (unsigned long long)p[l];
                    red[5 * l + 4][lane] = (unsigned long long)(p[l] >> 64);
                }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int l = 0; l < NL; l++)
                if (l < nl) {
                    a[l] += (long long)red[5 * l][lane];
                    q[l] += ((u128)red[5 * l + 2][lane] << 64) | red[5 * l + 1][lane];
                    p[l] += ((u128)red[5 * l + 4][lane] << 64) | red[5 * l + 3][lane];
                }
        }
        __syncthreads();
    }
    if (wave == 0 && live) {
#pragma unroll
        for (int l = 0; l < NL; l++)
            if (l < nl) {
                const size_t e = (size_t)l * ne + i;
                if (a[l]) atomicAdd((unsigned long long *)&E.A[e], (unsigned long long)a[l]);
                ess_add128(E.Q + 2 * e, q[l]);
                ess_add128(E.P + 2 * e, p[l]);
            }
    }
}

// ---------------------------------------------------------------------------
// a sampler's ESS state
struct McmcEss {
    EssDev E;                      // every chain of the sampler
    int nchains;
    ProbeList probes;
};

enum { ESS_SC, ESS_PEND, ESS_A, ESS_Q, ESS_P, ESS_NARR };     // the arrays in the order of mceik_mcmc_ess_get / _set

static int ess_arrays(void *state, KeptArray out[KEPT_MAX_ARRAYS])     // (pend: 4-byte words; none at one level)
{
    McmcEss *p = (McmcEss *)state;
    const size_t ne = p->E.ne, nch = p->nchains, L = p->E.nlevels;
    out[ESS_SC] = {(void **)&p->E.Sc, nch * ne * 8, 0};
    out[ESS_PEND] = {(void **)&p->E.pend, (L - 1) * nch * ne * 4, 0};
    out[ESS_A] = {(void **)&p->E.A, L * ne * 8, 0};
    out[ESS_Q] = {(void **)&p->E.Q, 2 * L * ne * 8, 0};
    out[ESS_P] = {(void **)&p->E.P, 2 * L * ne * 8, 0};
    return ESS_NARR;
}

static bool ess_holds_nuis(const void *state) { return probes_hold_nuis(((const McmcEss *)state)->probes); }

static void ess_free_extra(void *state)
{
    McmcEss *p = (McmcEss *)state;
    if (p->probes.d) hipFree(p->probes.d);
    delete p;
}

template <int NL, int U>
static void ess_launch(const EssDev &E, const CovSrc &R, int n, int k, int nl, hipStream_t st)
{
    const dim3 grid((E.ne + ESS_TILE - 1) / ESS_TILE, (n + ESS_SLICE - 1) / ESS_SLICE);
    hipLaunchKernelGGL((ess_accumulate_kernel<NL, U>), grid, dim3(256), 0, st, E, R, n, k, nl);
}

// The kept-state hook's side (kept.h KeptStream::accumulate): the chains are
// added as kept state number t = count + 1 of the chain, k the trailing zero
// bits of t.
static hipError_t ess_accumulate(void *state, const McmcDev &D, const HypoDev &H, const NuisDev &N, int chain_off, int n,
                                 long long count, hipStream_t st)
{
    const McmcEss *p = (const McmcEss *)state;
    if (n <= 0) return hipSuccess;
    const int k = __builtin_ctzll((unsigned long long)(count + 1));
    EssDev E = p->E;
    E.Sc += (size_t)chain_off * E.ne;
    if (E.pend) E.pend += (size_t)chain_off * E.ne;
    const CovSrc R = cov_src(D, H, N);
    const int nl = (k < E.nlevels - 1 ? k : E.nlevels - 1) + 1;
    // most launches close one or two levels: four chains in flight there, fewer where a thread holds more partial sums
    if (nl <= 1) ess_launch<1, 4>(E, R, n, k, nl, st);
    else if (nl <= 2) ess_launch<2, 4>(E, R, n, k, nl, st);
    else if (nl <= 4) ess_launch<4, 2>(E, R, n, k, nl, st);
    else if (nl <= 8) ess_launch<8, 1>(E, R, n, k, nl, st);
    else ess_launch<16, 1>(E, R, n, k, nl, st);
    return hipGetLastError();
}

KeptStream mcmc_ess_stream()
{
    KeptStream k = {};
    k.name = "the batch-means sums";
    k.arrays = ess_arrays;
    k.accumulate = ess_accumulate;
    k.free_extra = ess_free_extra;
    k.holds_nuis = ess_holds_nuis;
    return k;
}

static bool ess_same(const McmcEss *p, const mceik_ess_opts *o)
{
    return p->E.nlevels == o->nlevels && probes_same(p->probes, o->np, o->kind, o->index);
}

extern "C" int mceik_ess_check(int nlevels, long long xmax)
{
    if (nlevels < 1 || nlevels > MCEIK_ESS_MAX_LEVELS || xmax < 0) return 1;
    if (nlevels >= 2 && xmax >= (1LL << 31) >> (nlevels - 2)) return 1;     // xmax 2^(nlevels - 2) >= 2^31
    return 0;
}

extern "C" int mceik_mcmc_ess_enable(mceik_mcmc *s, const mceik_ess_opts *o)
{
    if (!s || !o || o->np < 0 || o->np > MCEIK_COV_MAX_PROBES) return 1;
    const McmcDev &D = s->D;
    long long xmax = D.vmax;
    if (D.nphase > 1 && D.vsmax > xmax) xmax = D.vsmax;
    for (int k = 0; k < o->np; k++) {
        const long long hi = mcmc_probe_limit(s, o->kind[k]);
        if (hi < 0 || o->index[k] < 0 || o->index[k] >= hi) return 1;   // (a probe whose state is not held has no valid index)
        long long x = 0;
        switch (o->kind[k]) {
        case 1: x = std::max(s->H.nx, std::max(s->H.ny, s->H.nz)); break;
        case 2: x = s->N.kcmax; break;
        case 3: x = s->N.nk; break;
        }
        if (x > xmax) xmax = x;
    }
    if (mceik_ess_check(o->nlevels, xmax)) {
        if (o->nlevels >= 1 && o->nlevels <= MCEIK_ESS_MAX_LEVELS)
            fprintf(stderr, "mceik_mcmc_ess_enable: %lld x 2^(nlevels - 2) >= 2^31 at nlevels = %d: a half batch would not "
                            "fit its 32-bit word\n", xmax, o->nlevels);
        return 1;
    }
    KeptStream &ks = s->kept[KEPT_ESS];
    const int rc = kept_enable_held(s, ks, ks.state && ess_same((const McmcEss *)ks.state, o), "mceik_mcmc_ess_enable");
    if (rc != KEPT_REPLACE) return rc;
    DeviceScope dg(s->device);
    McmcEss *p = new McmcEss();
    memset(p, 0, sizeof(*p));
    p->E.nlevels = o->nlevels;
    p->E.ncm = D.ncm;
    p->E.np = o->np;
    p->E.ne = D.ncm + o->np;
    p->E.pend_stride = (size_t)D.nchains * p->E.ne;
    p->nchains = D.nchains;
    KeptArray a[KEPT_MAX_ARRAYS];
    const int na = ess_arrays(p, a);
    if (!probes_upload(p->probes, o->np, o->kind, o->index) || !kept_arrays_alloc(a, na)) {
        (void)hipGetLastError();
        fprintf(stderr, "mceik_mcmc_ess_enable: out of device memory (%zu B of accumulators)\n",
                a[ESS_SC].bytes + a[ESS_PEND].bytes + a[ESS_A].bytes + a[ESS_Q].bytes + a[ESS_P].bytes);
        kept_state_free(ks, p);
        return -1;
    }
    p->E.kind = p->probes.d;
    p->E.index = p->probes.d + o->np;
    return kept_publish(s, ks, p, "mceik_mcmc_ess_enable");
}

extern "C" int mceik_mcmc_ess_disable(mceik_mcmc *s) { return s ? kept_disable(s, s->kept[KEPT_ESS]) : 1; }

extern "C" int mceik_mcmc_ess_clear(mceik_mcmc *s) { return s ? kept_clear(s, s->kept[KEPT_ESS]) : 1; }

extern "C" int mceik_mcmc_ess_accumulate(mceik_mcmc *s) { return s ? kept_accumulate(s, s->kept[KEPT_ESS]) : 1; }

extern "C" int mceik_mcmc_ess_get(mceik_mcmc *s, long long *n, long long *Sc, int *pend, long long *A,
                                  unsigned long long *Q, unsigned long long *P)
{
    void *const host[] = {Sc, pend, A, Q, P};
    return s ? kept_get(s, s->kept[KEPT_ESS], n, host) : 1;
}

extern "C" int mceik_mcmc_ess_set(mceik_mcmc *s, long long n, const long long *Sc, const int *pend, const long long *A,
                                  const unsigned long long *Q, const unsigned long long *P)
{
    const void *const host[] = {Sc, pend, A, Q, P};
    return s ? kept_set(s, s->kept[KEPT_ESS], n, host) : 1;
}

extern "C" int mceik_mcmc_ess_partials(mceik_mcmc *s, mceik_ess_partials *out)
{
    if (!s || !out || !s->kept[KEPT_ESS].state || !out->A || !out->Q || !out->P) return 1;
    McmcEss *p = (McmcEss *)s->kept[KEPT_ESS].state;
    if (mceik_mcmc_sync(s)) return -1;
    DeviceScope dg(s->device);
    KeptArray a[KEPT_MAX_ARRAYS];
    ess_arrays(p, a);
    HIPCHK(hipMemcpy(out->A, p->E.A, a[ESS_A].bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->Q, p->E.Q, a[ESS_Q].bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->P, p->E.P, a[ESS_P].bytes, hipMemcpyDeviceToHost));
    out->ncm = p->E.ncm;
    out->np = p->E.np;
    out->nlevels = p->E.nlevels;
    out->nchains = temper_cold(s);
    out->nkept = s->kept[KEPT_ESS].n;
    return 0;
}

// ---------------------------------------------------------------------------
// host only from here: no GPU call
static bool ess_parts_ok(const mceik_ess_partials *p)
{
    return p && p->ncm >= 0 && p->np >= 0 && p->np <= MCEIK_COV_MAX_PROBES && p->nlevels >= 1 &&
           p->nlevels <= MCEIK_ESS_MAX_LEVELS && p->nchains >= 0 && p->nkept >= 0 && p->A && p->Q && p->P;
}

extern "C" int mceik_ess_lstar(int nlevels, long long n)
{
    int lg = 0;                        // floor(log2 n); floor(lg / 2) = floor(log2(n) / 2)
    while (n > 1 && (n >> (lg + 1)) > 0) lg++;
    const int l = lg / 2;
    return l < nlevels - 1 ? l : (nlevels > 1 ? nlevels - 1 : 0);
}

extern "C" int mceik_ess_merge(mceik_ess_partials *dst, const mceik_ess_partials *src)
{
    if (!ess_parts_ok(dst) || !ess_parts_ok(src)) return 1;
    if (dst->ncm != src->ncm || dst->np != src->np || dst->nlevels != src->nlevels || dst->nkept != src->nkept) return 1;
    const size_t m = (size_t)dst->nlevels * ((size_t)dst->ncm + dst->np);
    for (size_t k = 0; k < m; k++)
        dst->A[k] = (long long)((unsigned long long)dst->A[k] + (unsigned long long)src->A[k]);
    add128(dst->Q, src->Q, m);
    add128(dst->P, src->P, m);
    dst->nchains += src->nchains;
    return 0;
}

extern "C" int mceik_ess_finish(const mceik_ess_partials *p, int level, double *tau, double *ess, double *mcse,
                                int *level_used)
{
    if (!ess_parts_ok(p) || level >= p->nlevels) return 1;
    const long long M = p->nchains, n = p->nkept;
    const int L = p->nlevels, ls = level < 0 ? mceik_ess_lstar(L, n) : level;
    const size_t ne = (size_t)p->ncm + p->np;
    const double dM = (double)M, dN = dM * (double)n;
    if (level_used) *level_used = ls;
    for (size_t j = 0; j < ne; j++) {
        double s2[MCEIK_ESS_MAX_LEVELS];
        bool moved = M >= 1;
        for (int l = 0; l < L; l++) {
            const long long nb = n >> l;
            const size_t e = (size_t)l * ne + j;
            const i128 N = (i128)nb * (i128)get128(p->Q + 2 * e) - (i128)get128(p->P + 2 * e);
            if (l == 0 && N == 0) moved = false;
            s2[l] = nb >= 2 ? (double)N / (dM * (double)nb * (double)(nb - 1)) : NAN;
        }
        double tl = NAN;
        for (int l = 0; l < L; l++) {
            const double t = moved ? s2[l] / (ldexp(1.0, l) * s2[0]) : NAN;
            if (tau) tau[(size_t)l * ne + j] = t;
            if (l == ls) tl = t;
        }
        if (ess) ess[j] = dN / tl;
        if (mcse) mcse[j] = tl == tl ? sqrt(s2[ls] / ldexp(1.0, ls) / dN) : NAN;
    }
    return 0;
}
