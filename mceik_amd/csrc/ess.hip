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
    long long n;                   // states accumulated per chain
    ProbeList probes;
};

void mcmc_ess_counted(McmcEss *p) { p->n++; }

long long mcmc_ess_count(const McmcEss *p) { return p->n; }

int mcmc_ess_k(const McmcEss *p) { return __builtin_ctzll((unsigned long long)(p->n + 1)); }

bool mcmc_ess_holds_nuis(const McmcEss *p) { return probes_hold_nuis(p->probes); }

void mcmc_ess_free(McmcEss *p)
{
    if (!p) return;
    void *all[] = {p->probes.d, p->E.Sc, p->E.pend, p->E.A, p->E.Q, p->E.P};
    for (void *q : all)
        if (q) hipFree(q);
    delete p;
}

template <int NL, int U>
static void ess_launch(const EssDev &E, const CovSrc &R, int n, int k, int nl, hipStream_t st)
{
    const dim3 grid((E.ne + ESS_TILE - 1) / ESS_TILE, (n + ESS_SLICE - 1) / ESS_SLICE);
    hipLaunchKernelGGL((ess_accumulate_kernel<NL, U>), grid, dim3(256), 0, st, E, R, n, k, nl);
}

hipError_t mcmc_ess_accumulate(McmcEss *p, const McmcDev &D, const HypoDev &H, const NuisDev &N, int chain_off, int n,
                               int k, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
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

// words (of 8 bytes; pend: of 4) of Sc, pend, A, Q, P
static size_t ess_words(const McmcEss *p, int which)
{
    const size_t ne = p->E.ne, nch = p->nchains, L = p->E.nlevels;
    const size_t w[5] = {nch * ne, (L - 1) * nch * ne, L * ne, 2 * L * ne, 2 * L * ne};
    return w[which];
}

static void **ess_array(McmcEss *p, int which)
{
    void **a[5] = {(void **)&p->E.Sc, (void **)&p->E.pend, (void **)&p->E.A, (void **)&p->E.Q, (void **)&p->E.P};
    return a[which];
}

static size_t ess_bytes(const McmcEss *p, int which) { return ess_words(p, which) * (which == 1 ? 4 : 8); }

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
    McmcEss *p = s->ess;
    if (p && !ess_same(p, o) && p->n > 0) return 1;
    if (p && ess_same(p, o)) {                      // the held sums go on
        s->ess_on = true;
        return 0;
    }
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->ess = nullptr;
    s->ess_on = false;
    mcmc_ess_free(p);
    p = new McmcEss();
    memset(p, 0, sizeof(*p));
    p->E.nlevels = o->nlevels;
    p->E.ncm = D.ncm;
    p->E.np = o->np;
    p->E.ne = D.ncm + o->np;
    p->E.pend_stride = (size_t)D.nchains * p->E.ne;
    p->nchains = D.nchains;
    bool ok = probes_upload(p->probes, o->np, o->kind, o->index);
    for (int a = 0; a < 5 && ok; a++) {
        if (!ess_bytes(p, a)) continue;             // one level: no pend
        ok = hipMalloc(ess_array(p, a), ess_bytes(p, a)) == hipSuccess &&
             hipMemset(*ess_array(p, a), 0, ess_bytes(p, a)) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        fprintf(stderr, "mceik_mcmc_ess_enable: out of device memory (%zu B of accumulators)\n",
                ess_bytes(p, 0) + ess_bytes(p, 1) + ess_bytes(p, 2) + ess_bytes(p, 3) + ess_bytes(p, 4));
        mcmc_ess_free(p);
        return -1;
    }
    p->E.kind = p->probes.d;
    p->E.index = p->probes.d + o->np;
    s->ess = p;
    s->ess_on = true;
    return 0;
}

extern "C" int mceik_mcmc_ess_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    s->ess_on = false;                 // host state only: queued steps keep the kernels they were queued with
    return 0;
}

extern "C" int mceik_mcmc_ess_clear(mceik_mcmc *s)
{
    if (!s) return 1;
    if (!s->ess) return 0;
    DeviceScope dg(s->device);
    const hipError_t e = hipStreamSynchronize(s->stream);
    mcmc_ess_free(s->ess);
    s->ess = nullptr;
    s->ess_on = false;
    return e == hipSuccess ? 0 : -1;
}

extern "C" int mceik_mcmc_ess_accumulate(mceik_mcmc *s)
{
    if (!s || !s->ess || !s->ess_on) return 1;
    DeviceScope dg(s->device);
    // tempering: the cold chains
    HIPCHK(mcmc_ess_accumulate(s->ess, s->D, s->H, s->N, 0, temper_cold(s), mcmc_ess_k(s->ess), s->stream));
    mcmc_ess_counted(s->ess);
    return 0;
}

extern "C" int mceik_mcmc_ess_get(mceik_mcmc *s, long long *n, long long *Sc, int *pend, long long *A,
                                  unsigned long long *Q, unsigned long long *P)
{
    if (!s || !s->ess) return 1;
    McmcEss *p = s->ess;
    if (mceik_mcmc_sync(s)) return -1;
    DeviceScope dg(s->device);
    if (n) *n = p->n;
    void *dst[5] = {Sc, pend, A, Q, P};
    for (int a = 0; a < 5; a++)
        if (dst[a] && ess_bytes(p, a)) HIPCHK(hipMemcpy(dst[a], *ess_array(p, a), ess_bytes(p, a), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_ess_set(mceik_mcmc *s, long long n, const long long *Sc, const int *pend, const long long *A,
                                  const unsigned long long *Q, const unsigned long long *P)
{
    if (!s || !s->ess || n < 0) return 1;
    McmcEss *p = s->ess;
    const void *src[5] = {Sc, pend, A, Q, P};
    for (int a = 0; a < 5; a++)
        if (!src[a] && ess_bytes(p, a)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    for (int a = 0; a < 5; a++)
        if (ess_bytes(p, a)) HIPCHK(hipMemcpy(*ess_array(p, a), src[a], ess_bytes(p, a), hipMemcpyHostToDevice));
    p->n = n;
    return 0;
}

extern "C" int mceik_mcmc_ess_partials(mceik_mcmc *s, mceik_ess_partials *out)
{
    if (!s || !out || !s->ess || !out->A || !out->Q || !out->P) return 1;
    McmcEss *p = s->ess;
    if (mceik_mcmc_sync(s)) return -1;
    DeviceScope dg(s->device);
    HIPCHK(hipMemcpy(out->A, p->E.A, ess_bytes(p, 2), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->Q, p->E.Q, ess_bytes(p, 3), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->P, p->E.P, ess_bytes(p, 4), hipMemcpyDeviceToHost));
    out->ncm = p->E.ncm;
    out->np = p->E.np;
    out->nlevels = p->E.nlevels;
    out->nchains = temper_cold(s);
    out->nkept = p->n;
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
