// cov.hip -- streaming probe-to-cell covariances: trade-off maps
// (include/mceik.h mceik_mcmc_cov_*, mceik_cov_*), on gfx950.
//
// For a handful of probe scalars x_p of a chain (a model entry, a hypocentre
// axis, a station static, a noise index) a sampler keeps the exact integer
// cross-moments C[p][j] = sum x_p v_j with every model entry beside the sums
// of x, x x', v and v^2, over the cold chains and the kept states.  Integer
// sums do not depend on the order of accumulation: pipes, launch paths, shards
// and ranks all give the same words, and partials merge by plain addition.
// Covariances and correlations, pooled and within-chain, are formed on the
// host from exact 128-bit numerators (mceik_cov_finish: no GPU call).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define HIPCHK_WHO "mceik_cov"
#include "host_util.h"
#include "sampler.h"

#define COV_TILE 64                // model entries per block: lane = entry
#define COV_SLICE 64               // chains per block: wave w takes chains w, w + 4, ... of the slice, four in flight
#define COV_GROUP 16               // probes per block (blockIdx.z): their accumulators stay in registers
#define COV_RGROUP 8               // probes per block of the within-chain reduce (128-bit accumulators)

// Probe gather: one block per slice of 64 chains.  X[c][p] of the slice goes to
// LDS and to global memory (the accumulate launch reads it), A_c takes it, and
// the slice's part of A and G goes out as one atomic per word (the slices and
// the pipes share them).
__global__ __launch_bounds__(256) void cov_gather_kernel(CovDev V, CovSrc R, int nchains)
{
    extern __shared__ int cov_xs[];                  // [COV_SLICE][np]
    __shared__ CovTab tab;
    const int np = V.np, c0 = blockIdx.x * COV_SLICE;
    const int nc = nchains - c0 < COV_SLICE ? nchains - c0 : COV_SLICE;
    cov_tab_stage(tab, R);
    __syncthreads();
    for (int k = threadIdx.x; k < nc * np; k += 256) {
        const int cl = k / np, p = k - cl * np;
        const size_t c = (size_t)(c0 + cl);
        int st;
        const int *src = cov_probe_ptr(tab, V.kind[p], V.index[p], &st);
        const int x = src[c * st];
        cov_xs[k] = x;
        V.X[c * np + p] = x;
        if (V.Ac) V.Ac[c * np + p] += x;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < np * np; k += 256) {
        const int p = k / np, q = k - p * np;
        long long g = 0;
        for (int cl = 0; cl < nc; cl++) g += (long long)cov_xs[cl * np + p] * cov_xs[cl * np + q];
        atomicAdd((unsigned long long *)&V.G[k], (unsigned long long)g);
    }
    for (int p = threadIdx.x; p < np; p += 256) {
        long long a = 0;
        for (int cl = 0; cl < nc; cl++) a += cov_xs[cl * np + p];
        atomicAdd((unsigned long long *)&V.A[p], (unsigned long long)a);
    }
}

// The rank-nchains update C[p][j] += sum_c X[c][p] v[c][j] (and S, Q, S_c with
// it).  A block owns a tile of 64 consecutive entries x a slice of 64 chains x
// a group of 16 probes; lane = entry, so a wave reads a chain's v row as one
// 256-byte line, and the chain's probe row is the same for the whole wave (it
// comes through scalar loads: the gather launch wrote it).  Every lane keeps
// the group's 16 sums as 64-bit register pairs, one v_mad_i64_i32 per probe
// and chain, with four chains' rows in flight.  64 probes in one pass would
// need 128 accumulator registers and a 101 KB reduction buffer: one block per
// CU; groups of 16 (32 registers, 27 KB) keep five waves per SIMD and re-read
// the v row once per group, from L2.  The
// four waves' sums meet in LDS and leave as one 64-bit vector atomic per (p, j)
// and block: the chain slices and the pipes share C, S and Q.  Group 0 also
// sums v and v^2 and, WITHIN, adds v to the chain's own row of S_c (one thread
// of the grid owns each word of it).
template <bool WITHIN>
__global__ __launch_bounds__(256) void cov_accumulate_kernel(CovDev V, const int *__restrict__ X,
                                                             const int *__restrict__ vp, long long *__restrict__ Sc,
                                                             int nchains)
{
    __shared__ long long red[3][COV_GROUP + 2][COV_TILE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * COV_TILE + lane, ncm = V.ncm, np = V.np;
    const bool live = i < ncm;
    const size_t ii = live ? i : 0;                  // a tail tile's dead lanes read entry 0 and write nothing
    const int c0 = blockIdx.y * COV_SLICE;
    const int c1 = nchains < c0 + COV_SLICE ? nchains : c0 + COV_SLICE;
    const int p0 = blockIdx.z * COV_GROUP;
    const int cnt = np - p0 < COV_GROUP ? np - p0 : COV_GROUP;
    const bool first = blockIdx.z == 0;
    long long acc[COV_GROUP], ps = 0, pq = 0;
#pragma unroll
    for (int u = 0; u < COV_GROUP; u++) acc[u] = 0;
    for (int c = c0 + wave; c < c1; c += 16) {
        int vv[4];                                   // four chains' v rows in flight, as post_accumulate_kernel
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int cc = c + 4 * k;
            vv[k] = vp[(size_t)(cc < c1 ? cc : c) * ncm + ii];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int cc = c + 4 * k;
            if (cc >= c1) continue;
            const int *xr = X + (size_t)cc * np + p0;
            const long long w = vv[k];
#pragma unroll
            for (int u = 0; u < COV_GROUP; u++)
                if (u < cnt) acc[u] += (long long)xr[u] * w;
            if (first) {
                ps += w;
                pq += w * w;
                if (WITHIN && live) Sc[(size_t)cc * ncm + i] += w;
            }
        }
    }
    if (wave) {
#pragma unroll
        for (int u = 0; u < COV_GROUP; u++) red[wave - 1][u][lane] = acc[u];
        red[wave - 1][COV_GROUP][lane] = ps;
        red[wave - 1][COV_GROUP + 1][lane] = pq;
    }
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int u = 0; u < COV_GROUP; u++)
            if (u < cnt) {
                const long long t = acc[u] + red[0][u][lane] + red[1][u][lane] + red[2][u][lane];
                atomicAdd((unsigned long long *)&V.C[(size_t)(p0 + u) * ncm + i], (unsigned long long)t);
            }
        if (first) {
            const long long ts = ps + red[0][COV_GROUP][lane] + red[1][COV_GROUP][lane] + red[2][COV_GROUP][lane];
            const long long tq = pq + red[0][COV_GROUP + 1][lane] + red[1][COV_GROUP + 1][lane] +
                                 red[2][COV_GROUP + 1][lane];
            atomicAdd((unsigned long long *)&V.S[i], (unsigned long long)ts);
            atomicAdd((unsigned long long *)&V.Q[i], (unsigned long long)tq);
        }
    }
}

__device__ __forceinline__ void cov_put128(unsigned long long *w, unsigned __int128 x)
{
    w[0] = (unsigned long long)x;
    w[1] = (unsigned long long)(x >> 64);
}

// Within-chain reduce (partials only): the chain axis of the per-chain sums
// into T[p][j] = sum_c A_c[c][p] S_c[c][j], P[j] = sum_c S_c[c][j]^2 and PA[p][q]
// = sum_c A_c[c][p] A_c[c][q], 128 bits each (lo, hi words).  The accumulate
// kernel's shape with a chain loop per entry: lane = entry, a group of 8 probes
// per block (blockIdx.y), a chain's A_c row uniform over the wave.  The blocks
// past the entry tiles take 64 (p, q) pairs of PA each.
__global__ __launch_bounds__(64) void cov_reduce_kernel(CovDev V, const long long *__restrict__ Ac,
                                                        const long long *__restrict__ Sc, int nchains,
                                                        unsigned long long *T, unsigned long long *P,
                                                        unsigned long long *PA)
{
    const int ncm = V.ncm, np = V.np, ntile = (ncm + COV_TILE - 1) / COV_TILE, lane = threadIdx.x;
    if ((int)blockIdx.x >= ntile) {
        const int k = ((int)blockIdx.x - ntile) * 64 + lane;
        if (blockIdx.y || k >= np * np) return;
        const int p = k / np, q = k - p * np;
        __int128 t = 0;
        for (int c = 0; c < nchains; c++) t += (__int128)Ac[(size_t)c * np + p] * Ac[(size_t)c * np + q];
        cov_put128(PA + 2 * (size_t)k, (unsigned __int128)t);
        return;
    }
    const int i = blockIdx.x * COV_TILE + lane;
    const bool live = i < ncm;
    const size_t ii = live ? i : 0;
    const int p0 = blockIdx.y * COV_RGROUP;
    const int cnt = np - p0 < COV_RGROUP ? np - p0 : COV_RGROUP;
    __int128 t[COV_RGROUP];
    unsigned __int128 pp = 0;
#pragma unroll
    for (int u = 0; u < COV_RGROUP; u++) t[u] = 0;
    for (int c = 0; c < nchains; c++) {
        const long long *ar = Ac + (size_t)c * np + p0;
        const long long s = Sc[(size_t)c * ncm + ii];
#pragma unroll
        for (int u = 0; u < COV_RGROUP; u++)
            if (u < cnt) t[u] += (__int128)ar[u] * s;
        pp += (unsigned __int128)((__int128)s * s);
    }
    if (!live) return;
#pragma unroll
    for (int u = 0; u < COV_RGROUP; u++)
        if (u < cnt) cov_put128(T + 2 * ((size_t)(p0 + u) * ncm + i), (unsigned __int128)t[u]);
    if (blockIdx.y == 0) cov_put128(P + 2 * (size_t)i, pp);
}

// ---------------------------------------------------------------------------
// a sampler's covariance state
struct McmcCov {
    CovDev V;                      // every chain of the sampler
    int nchains;
    ProbeList probes;
    unsigned long long *d_T, *d_P, *d_PA;   // within: partials scratch [np][ncm][2], [ncm][2], [np][np][2]
};

static int cov_arrays(void *state, KeptArray out[KEPT_MAX_ARRAYS])     // A, G, S, Q, C and, within, Ac, Sc
{
    McmcCov *p = (McmcCov *)state;
    const size_t np = p->V.np, ncm = p->V.ncm, nch = p->nchains;
    long long **a[7] = {&p->V.A, &p->V.G, &p->V.S, &p->V.Q, &p->V.C, &p->V.Ac, &p->V.Sc};
    const size_t w[7] = {np, np * np, ncm, ncm, np * ncm, nch * np, nch * ncm};
    const int na = p->V.within ? 7 : 5;
    for (int k = 0; k < na; k++) out[k] = {(void **)a[k], w[k] * 8, 0};
    return na;
}

static bool cov_holds_nuis(const void *state) { return probes_hold_nuis(((const McmcCov *)state)->probes); }

static void cov_free_extra(void *state)
{
    McmcCov *p = (McmcCov *)state;
    void *all[] = {p->probes.d, p->V.X, p->d_T, p->d_P, p->d_PA};
    for (void *q : all)
        if (q) hipFree(q);
    delete p;
}

// The kept-state hook's side (kept.h KeptStream::accumulate): two launches,
// the probe gather, then the rank-n update.
static hipError_t cov_accumulate(void *state, const McmcDev &D, const HypoDev &H, const NuisDev &N, int chain_off, int n,
                                 long long, hipStream_t st)
{
    const McmcCov *p = (const McmcCov *)state;
    if (n <= 0) return hipSuccess;
    CovDev V = p->V;                   // the chains' rows of the per-chain arrays
    V.X += (size_t)chain_off * V.np;
    if (V.Ac) V.Ac += (size_t)chain_off * V.np;
    if (V.Sc) V.Sc += (size_t)chain_off * V.ncm;
    const CovSrc R = cov_src(D, H, N);
    const int nslice = (n + COV_SLICE - 1) / COV_SLICE;
    hipLaunchKernelGGL(cov_gather_kernel, dim3(nslice), dim3(256), (size_t)COV_SLICE * V.np * sizeof(int), st, V, R, n);
    const dim3 grid((V.ncm + COV_TILE - 1) / COV_TILE, nslice, (V.np + COV_GROUP - 1) / COV_GROUP);
    if (V.within) hipLaunchKernelGGL(cov_accumulate_kernel<true>, grid, dim3(256), 0, st, V, V.X, D.v, V.Sc, n);
    else hipLaunchKernelGGL(cov_accumulate_kernel<false>, grid, dim3(256), 0, st, V, V.X, D.v, V.Sc, n);
    return hipGetLastError();
}

KeptStream mcmc_cov_stream()
{
    KeptStream k = {};
    k.name = "the covariance sums";
    k.arrays = cov_arrays;
    k.accumulate = cov_accumulate;
    k.free_extra = cov_free_extra;
    k.holds_nuis = cov_holds_nuis;
    return k;
}

static bool cov_same(const McmcCov *p, const mceik_cov_opts *o)
{
    return p->V.within == (o->within ? 1 : 0) && probes_same(p->probes, o->np, o->kind, o->index);
}

long long mcmc_probe_limit(const mceik_mcmc *s, int kind)
{
    const McmcDev &D = s->D;
    switch (kind) {
    case 0: return D.ncm;
    case 1: return s->H.hyp ? 3LL * D.nev : 0;
    case 2: return s->N.kn && s->N.statics_on ? (long long)D.nphase * D.nstat : 0;
    case 3: return s->N.kn && s->N.noise_on ? D.nphase : 0;
    default: return -1;
    }
}

extern "C" int mceik_mcmc_cov_enable(mceik_mcmc *s, const mceik_cov_opts *o)
{
    if (!s || !o || o->np < 1 || o->np > MCEIK_COV_MAX_PROBES) return 1;
    const McmcDev &D = s->D;
    for (int k = 0; k < o->np; k++) {
        const long long hi = mcmc_probe_limit(s, o->kind[k]);
        if (hi < 0 || o->index[k] < 0 || o->index[k] >= hi) return 1;   // (a probe whose state is not held has no valid index)
    }
    KeptStream &k = s->kept[KEPT_COV];
    const int rc = kept_enable_held(s, k, k.state && cov_same((const McmcCov *)k.state, o), "mceik_mcmc_cov_enable");
    if (rc != KEPT_REPLACE) return rc;
    DeviceScope dg(s->device);
    McmcCov *p = new McmcCov();
    memset(p, 0, sizeof(*p));
    p->V.np = o->np;
    p->V.within = o->within ? 1 : 0;
    p->V.ncm = D.ncm;
    p->nchains = D.nchains;
    const size_t np = o->np, ncm = D.ncm, xbytes = (size_t)D.nchains * np * sizeof(int);
    KeptArray a[KEPT_MAX_ARRAYS];
    bool ok = probes_upload(p->probes, o->np, o->kind, o->index) && hipMalloc((void **)&p->V.X, xbytes) == hipSuccess &&
              hipMemset(p->V.X, 0, xbytes) == hipSuccess && kept_arrays_alloc(a, cov_arrays(p, a));
    if (ok && p->V.within)
        ok = hipMalloc((void **)&p->d_T, np * ncm * 16) == hipSuccess && hipMalloc((void **)&p->d_P, ncm * 16) == hipSuccess &&
             hipMalloc((void **)&p->d_PA, np * np * 16) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        fprintf(stderr, "mceik_mcmc_cov_enable: out of device memory (%zu B of accumulators)\n",
                8 * ((np + 2) * ncm + (p->V.within ? (size_t)D.nchains * (ncm + np) : 0)));
        kept_state_free(k, p);
        return -1;
    }
    p->V.kind = p->probes.d;
    p->V.index = p->probes.d + np;
    return kept_publish(s, k, p, "mceik_mcmc_cov_enable");
}

extern "C" int mceik_mcmc_cov_disable(mceik_mcmc *s) { return s ? kept_disable(s, s->kept[KEPT_COV]) : 1; }

extern "C" int mceik_mcmc_cov_clear(mceik_mcmc *s) { return s ? kept_clear(s, s->kept[KEPT_COV]) : 1; }

extern "C" int mceik_mcmc_cov_accumulate(mceik_mcmc *s) { return s ? kept_accumulate(s, s->kept[KEPT_COV]) : 1; }

extern "C" int mceik_mcmc_cov_get(mceik_mcmc *s, long long *n, long long *A, long long *G, long long *S, long long *Q,
                                  long long *C, long long *Ac, long long *Sc)
{
    void *const host[] = {A, G, S, Q, C, Ac, Sc};
    return s ? kept_get(s, s->kept[KEPT_COV], n, host) : 1;
}

extern "C" int mceik_mcmc_cov_set(mceik_mcmc *s, long long n, const long long *A, const long long *G, const long long *S,
                                  const long long *Q, const long long *C, const long long *Ac, const long long *Sc)
{
    const void *const host[] = {A, G, S, Q, C, Ac, Sc};
    return s ? kept_set(s, s->kept[KEPT_COV], n, host) : 1;
}

// int64 words widened to 128-bit two's complement (lo, hi).
static void cov_widen(unsigned long long *dst, const long long *src, size_t n)
{
    for (size_t k = 0; k < n; k++) {
        dst[2 * k] = (unsigned long long)src[k];
        dst[2 * k + 1] = src[k] < 0 ? ~0ull : 0ull;
    }
}

extern "C" int mceik_mcmc_cov_partials(mceik_mcmc *s, mceik_cov_partials *out)
{
    if (!s || !out || !s->kept[KEPT_COV].state) return 1;
    const McmcCov *p = (const McmcCov *)s->kept[KEPT_COV].state;
    if (!out->A || !out->S || !out->G || !out->Q || !out->C) return 1;
    const int within = p->V.within, ncold = temper_cold(s);
    if (within && (!out->PA || !out->P || !out->T)) return 1;
    const size_t np = p->V.np, ncm = p->V.ncm;
    if (within) {
        DeviceScope dg(s->device);
        const int ntile = (int)((ncm + COV_TILE - 1) / COV_TILE), npair = (int)((np * np + 63) / 64);
        hipLaunchKernelGGL(cov_reduce_kernel, dim3(ntile + npair, (unsigned)((np + COV_RGROUP - 1) / COV_RGROUP)), dim3(64), 0,
                           s->stream, p->V, p->V.Ac, p->V.Sc, ncold, p->d_T, p->d_P, p->d_PA);
        HIPCHK(hipGetLastError());
    }
    if (mceik_mcmc_sync(s)) return -1;
    DeviceScope dg(s->device);
    std::vector<long long> w(np * ncm > np * np ? np * ncm : np * np);
    HIPCHK(hipMemcpy(out->A, p->V.A, np * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->S, p->V.S, ncm * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(w.data(), p->V.G, np * np * 8, hipMemcpyDeviceToHost));
    cov_widen(out->G, w.data(), np * np);
    HIPCHK(hipMemcpy(w.data(), p->V.Q, ncm * 8, hipMemcpyDeviceToHost));
    cov_widen(out->Q, w.data(), ncm);
    HIPCHK(hipMemcpy(w.data(), p->V.C, np * ncm * 8, hipMemcpyDeviceToHost));
    cov_widen(out->C, w.data(), np * ncm);
    if (within) {
        HIPCHK(hipMemcpy(out->PA, p->d_PA, np * np * 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out->P, p->d_P, ncm * 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out->T, p->d_T, np * ncm * 16, hipMemcpyDeviceToHost));
    } else {
        if (out->PA) memset(out->PA, 0, np * np * 16);
        if (out->P) memset(out->P, 0, ncm * 16);
        if (out->T) memset(out->T, 0, np * ncm * 16);
    }
    out->np = (int)np;
    out->ncm = (int)ncm;
    out->within = within;
    memset(out->kind, 0, sizeof(out->kind));
    memset(out->index, 0, sizeof(out->index));
    memcpy(out->kind, p->probes.kind, np * sizeof(int));
    memcpy(out->index, p->probes.index, np * sizeof(int));
    out->nchains = ncold;
    out->nkept = s->kept[KEPT_COV].n;
    return 0;
}

// ---------------------------------------------------------------------------
// host only from here: no GPU call

static bool cov_parts_ok(const mceik_cov_partials *p)
{
    return p && p->np >= 1 && p->np <= MCEIK_COV_MAX_PROBES && p->ncm >= 0 && p->nchains >= 0 && p->nkept >= 0 && p->A &&
           p->S && p->G && p->Q && p->C && (!p->within || (p->PA && p->P && p->T));
}

extern "C" int mceik_cov_merge(mceik_cov_partials *dst, const mceik_cov_partials *src)
{
    if (!cov_parts_ok(dst) || !cov_parts_ok(src)) return 1;
    if (dst->np != src->np || dst->ncm != src->ncm || (dst->within != 0) != (src->within != 0) || dst->nkept != src->nkept)
        return 1;
    for (int k = 0; k < dst->np; k++)
        if (dst->kind[k] != src->kind[k] || dst->index[k] != src->index[k]) return 1;
    const size_t np = dst->np, ncm = dst->ncm;
    for (size_t k = 0; k < np; k++) dst->A[k] += src->A[k];
    for (size_t k = 0; k < ncm; k++) dst->S[k] += src->S[k];
    add128(dst->G, src->G, np * np);
    add128(dst->Q, src->Q, ncm);
    add128(dst->C, src->C, np * ncm);
    if (dst->within) {
        add128(dst->PA, src->PA, np * np);
        add128(dst->P, src->P, ncm);
        add128(dst->T, src->T, np * ncm);
    }
    dst->nchains += src->nchains;
    return 0;
}

extern "C" int mceik_cov_finish(const mceik_cov_partials *p, double *cov, double *corr, double *covw, double *corrw,
                                double *pmean, double *pcov, double *pcorr, double *pcovw, double *pcorrw)
{
    if (!cov_parts_ok(p)) return 1;
    const long long M = p->nchains, n = p->nkept;
    const size_t np = p->np, ncm = p->ncm;
    const i128 N = (i128)M * n;
    const bool pooled = N >= 2, within = p->within && n >= 2 && M >= 1;
    const double dN = (double)N, den = dN * (double)(N - 1);                      // N (N - 1)
    const double denw = (double)M * (double)n * (double)(n - 1);                  // M n (n - 1)
    // the variance numerators (exact) and the variances, once
    std::vector<i128> nx(np), nwx(np), nv(ncm), nwv(ncm);
    std::vector<double> vx(np), wx(np), vv(ncm), wv(ncm);
    for (size_t k = 0; k < np; k++) {
        const i128 A = p->A[k], G = (i128)get128(p->G + 2 * (k * np + k));
        nx[k] = N * G - A * A;
        vx[k] = (double)nx[k] / den;
        nwx[k] = within ? (i128)n * G - (i128)get128(p->PA + 2 * (k * np + k)) : 0;
        wx[k] = (double)nwx[k] / denw;
    }
    for (size_t j = 0; j < ncm; j++) {
        const i128 S = p->S[j], Q = (i128)get128(p->Q + 2 * j);
        nv[j] = N * Q - S * S;
        vv[j] = (double)nv[j] / den;
        nwv[j] = within ? (i128)n * Q - (i128)get128(p->P + 2 * j) : 0;
        wv[j] = (double)nwv[j] / denw;
    }
    for (size_t k = 0; k < np; k++) {
        const i128 A = p->A[k];
        if (pmean) pmean[k] = N > 0 ? (double)A / dN : NAN;
        for (size_t j = 0; j < ncm; j++) {
            const size_t e = k * ncm + j;
            const i128 C = (i128)get128(p->C + 2 * e);
            const double c = pooled ? (double)(N * C - A * (i128)p->S[j]) / den : NAN;
            if (cov) cov[e] = c;
            if (corr) corr[e] = pooled && nx[k] != 0 && nv[j] != 0 ? c / sqrt(vx[k] * vv[j]) : NAN;
            const double cw = within ? (double)((i128)n * C - (i128)get128(p->T + 2 * e)) / denw : NAN;
            if (covw) covw[e] = cw;
            if (corrw) corrw[e] = within && nwx[k] != 0 && nwv[j] != 0 ? cw / sqrt(wx[k] * wv[j]) : NAN;
        }
        for (size_t q = 0; q < np; q++) {
            const size_t e = k * np + q;
            const i128 G = (i128)get128(p->G + 2 * e);
            const double c = pooled ? (double)(N * G - A * (i128)p->A[q]) / den : NAN;
            if (pcov) pcov[e] = c;
            if (pcorr) pcorr[e] = pooled && nx[k] != 0 && nx[q] != 0 ? c / sqrt(vx[k] * vx[q]) : NAN;
            const double cw = within ? (double)((i128)n * G - (i128)get128(p->PA + 2 * e)) / denw : NAN;
            if (pcovw) pcovw[e] = cw;
            if (pcorrw) pcorrw[e] = within && nwx[k] != 0 && nwx[q] != 0 ? cw / sqrt(wx[k] * wx[q]) : NAN;
        }
    }
    return 0;
}
