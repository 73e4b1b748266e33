// posterior.hip -- streaming posterior moments, histograms and R-hat
// (include/mceik.h mceik_mcmc_posterior_*, mceik_posterior_*).
//
// Cell velocities are integers, so a sampler keeps per model entry the exact
// integer sums  sum = sum_t v_t  and  sumsq = sum_t v_t^2  over its kept
// states (per chain, or pooled over chains) and a pooled histogram.  Integer
// sums do not depend on the order of accumulation: pipes, launch paths, shards
// and ranks all give the same words, and partials merge by plain addition.
// Mean, variance and R-hat are formed on the host from exact 128-bit
// numerators (mceik_posterior_finish: no GPU call).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/mceik.h"
#define HIPCHK_WHO "mceik_posterior"
#include "host_util.h"
#include "sampler.h"

#define POST_TILE 64               // model entries per block: lane = entry
#define POST_SLICE 64              // chains per block: wave w takes chains w, w + 4, ... of the slice

// Histogram bin of value v in [lo, lo + span): (v - lo) * nbins / span in
// integers, clamped to [0, nbins - 1].  narrow: span * nbins fits 31 bits, so
// the 32-bit quotient is the 64-bit one.
__device__ __forceinline__ int post_bin(int v, int lo, int span, int nbins, bool narrow)
{
    int b;
    if (narrow) {
        const int d = v > lo ? v - lo : 0;
        b = (int)((unsigned)d * (unsigned)nbins / (unsigned)span);
    } else {
        b = (int)(((long long)v - lo) * nbins / span);
    }
    return b < 0 ? 0 : (b > nbins - 1 ? nbins - 1 : b);
}

// One launch adds the current models D.v of the view's chains.  A block owns a
// tile of 64 consecutive entries x a slice of 64 chains; lane = entry, so a
// wave reads and writes whole rows of v / sum / sumsq (256 / 512 / 512
// contiguous bytes), four chains in flight.  The tile's histogram lives in LDS
// as [bin][lane] (lanes of one instruction sit on different banks) with LDS
// atomics between the four waves, and goes to global memory once per block
// (vector atomics: the chain slices and the pipes share a tile).  Pooled mode
// sums the slice in registers, then over the waves in LDS, and issues one
// global atomic per entry and moment.
template <bool PER_CHAIN>
__global__ __launch_bounds__(256) void post_accumulate_kernel(McmcDev D, PostDev P, int narrow)
{
    extern __shared__ unsigned lds_hist[];           // [nbins][64]
    __shared__ long long red[2][4][POST_TILE];       // pooled mode: the waves' partial sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * POST_TILE + lane;
    const bool live = i < D.ncm;
    const int c0 = blockIdx.y * POST_SLICE;
    const int c1 = D.nchains < c0 + POST_SLICE ? D.nchains : c0 + POST_SLICE;
    const int nbins = P.nbins;
    if (nbins) {
        for (int k = threadIdx.x; k < nbins * POST_TILE; k += 256) lds_hist[k] = 0u;
        __syncthreads();
    }
    const bool sph = i >= D.ncell;                   // entry i belongs to phase i / ncell
    const int lo = sph ? D.vsmin : D.vmin;
    const int span = (sph ? D.vsmax : D.vmax) - lo + 1;
    const int *__restrict__ vp = D.v;
    long long *__restrict__ sum = P.sum;
    long long *__restrict__ sumsq = P.sumsq;
    long long ps = 0, pq = 0;
    if (live) {
        for (int c = c0 + wave; c < c1; c += 16) {
            int v[4];
            long long s[4], q[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int cc = c + 4 * u;
                const size_t k = (size_t)(cc < c1 ? cc : c) * D.ncm + i;
                v[u] = vp[k];
                if (PER_CHAIN) { s[u] = sum[k]; q[u] = sumsq[k]; }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int cc = c + 4 * u;
                if (cc >= c1) continue;
                const size_t k = (size_t)cc * D.ncm + i;
                const long long w = v[u];
                if (PER_CHAIN) {
                    sum[k] = s[u] + w;
                    sumsq[k] = q[u] + w * w;
                } else {
                    ps += w;
                    pq += w * w;
                }
                if (nbins) atomicAdd(&lds_hist[post_bin(v[u], lo, span, nbins, narrow) * POST_TILE + lane], 1u);
            }
        }
    }
    if (!PER_CHAIN) {
        red[0][wave][lane] = ps;
        red[1][wave][lane] = pq;
        __syncthreads();
        if (wave == 0 && live) {
            const long long ts = red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane];
            const long long tq = red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane];
            atomicAdd((unsigned long long *)&P.sum[i], (unsigned long long)ts);
            atomicAdd((unsigned long long *)&P.sumsq[i], (unsigned long long)tq);
        }
    }
    if (nbins) {
        __syncthreads();
        // the tile's part of hist [ncm][nbins] is contiguous: word g = entry * nbins + bin
        const int left = D.ncm - blockIdx.x * POST_TILE;
        const int nent = left < POST_TILE ? left : POST_TILE;
        unsigned *gh = P.hist + (size_t)blockIdx.x * POST_TILE * nbins;
        for (int g = threadIdx.x; g < nent * nbins; g += 256) {
            const int e = g / nbins, b = g - e * nbins;
            const unsigned cnt = lds_hist[b * POST_TILE + e];
            if (cnt) atomicAdd(&gh[g], cnt);
        }
    }
}

// The chain axis summed per entry into exact partials: S = sum_c sum_c,
// Q = sum_c sumsq_c and P = sum_c sum_c^2 in 128 bits (lo, hi words).  Lanes
// run along the entries, so every chain's row is read coalesced.  Pooled
// accumulators are S and Q already; P = 0.
__global__ __launch_bounds__(64) void post_reduce_kernel(PostDev A, int nchains, int ncm, long long *S,
                                                         unsigned long long *Q, unsigned long long *Pp)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= ncm) return;
    long long s = 0;
    unsigned __int128 q = 0, p = 0;
    if (A.per_chain) {
        for (int c = 0; c < nchains; c++) {
            const size_t k = (size_t)c * ncm + i;
            const long long a = A.sum[k];
            s += a;
            q += (unsigned long long)A.sumsq[k];
            p += (unsigned __int128)((__int128)a * a);
        }
    } else {
        s = A.sum[i];
        q = (unsigned long long)A.sumsq[i];
    }
    S[i] = s;
    Q[2 * (size_t)i] = (unsigned long long)q;
    Q[2 * (size_t)i + 1] = (unsigned long long)(q >> 64);
    Pp[2 * (size_t)i] = (unsigned long long)p;
    Pp[2 * (size_t)i + 1] = (unsigned long long)(p >> 64);
}

// ---------------------------------------------------------------------------
// a sampler's posterior state
struct McmcPost {
    PostDev P;
    int nchains, ncm;
    long long *d_S;                // partials scratch [ncm], [ncm][2], [ncm][2]
    unsigned long long *d_Q, *d_P;
};

static size_t post_rows(const McmcPost *p) { return p->P.per_chain ? (size_t)p->nchains : 1; }

static int post_arrays(void *state, KeptArray out[KEPT_MAX_ARRAYS])     // sum, sumsq, hist (4-byte words; none at nbins = 0)
{
    McmcPost *p = (McmcPost *)state;
    const size_t m = post_rows(p) * p->ncm * 8;
    out[0] = {(void **)&p->P.sum, m, 0};
    out[1] = {(void **)&p->P.sumsq, m, 0};
    out[2] = {(void **)&p->P.hist, (size_t)p->ncm * p->P.nbins * 4, 0};
    return 3;
}

static void post_free_extra(void *state)
{
    McmcPost *p = (McmcPost *)state;
    if (p->d_S) hipFree(p->d_S);
    if (p->d_Q) hipFree(p->d_Q);
    if (p->d_P) hipFree(p->d_P);
    delete p;
}

// The kept-state hook's side (kept.h KeptStream::accumulate): add the current
// models of the first n chains of view D.
static hipError_t post_accumulate(void *state, const McmcDev &D, const HypoDev &, const NuisDev &, int chain_off, int n,
                                  long long, hipStream_t st)
{
    const McmcPost *p = (const McmcPost *)state;
    if (n <= 0) return hipSuccess;
    McmcDev V = D;                     // the kernel adds every chain of the view it is given
    V.nchains = n;
    PostDev A = p->P;
    if (A.per_chain) {
        A.sum += (size_t)chain_off * p->ncm;
        A.sumsq += (size_t)chain_off * p->ncm;
    }
    // the 32-bit bin quotient is exact when (span - 1) * nbins < 2^31 for both priors
    const long long sp = (long long)V.vmax - V.vmin, ss = V.nphase > 1 ? (long long)V.vsmax - V.vsmin : 0;
    const int narrow = A.nbins && sp >= 0 && ss >= 0 && (sp > ss ? sp : ss) * A.nbins < (1LL << 31) ? 1 : 0;
    const dim3 grid((V.ncm + POST_TILE - 1) / POST_TILE, (V.nchains + POST_SLICE - 1) / POST_SLICE);
    const size_t lds = (size_t)A.nbins * POST_TILE * sizeof(unsigned);
    if (A.per_chain) hipLaunchKernelGGL(post_accumulate_kernel<true>, grid, dim3(256), lds, st, V, A, narrow);
    else hipLaunchKernelGGL(post_accumulate_kernel<false>, grid, dim3(256), lds, st, V, A, narrow);
    return hipGetLastError();
}

KeptStream mcmc_post_stream()
{
    KeptStream k = {};
    k.name = "the streaming posterior";
    k.arrays = post_arrays;
    k.accumulate = post_accumulate;
    k.free_extra = post_free_extra;
    return k;
}

// The posterior has no disabled state that keeps its sums: enabling always
// starts from zero (other options: from new arrays), disabling drops it.
extern "C" int mceik_mcmc_posterior_enable(mceik_mcmc *s, const mceik_posterior_opts *o)
{
    if (!s || !o) return 1;
    if (o->nbins < 0 || o->nbins > MCEIK_POST_MAX_BINS) return 1;
    DeviceScope dg(s->device);
    const int per_chain = o->per_chain ? 1 : 0;
    KeptStream &k = s->kept[KEPT_POST];
    McmcPost *p = (McmcPost *)k.state;
    if (p && (p->P.per_chain != per_chain || p->P.nbins != o->nbins)) {
        if (kept_clear(s, k)) return -1;
        p = nullptr;
    }
    KeptArray a[KEPT_MAX_ARRAYS];
    if (!p) {
        p = new McmcPost();
        memset(p, 0, sizeof(*p));
        p->P.per_chain = per_chain;
        p->P.nbins = o->nbins;
        p->nchains = s->D.nchains;
        p->ncm = s->D.ncm;
        const size_t m = (size_t)p->ncm;
        if (!kept_arrays_alloc(a, post_arrays(p, a)) || hipMalloc((void **)&p->d_S, m * 8) != hipSuccess ||
            hipMalloc((void **)&p->d_Q, m * 16) != hipSuccess || hipMalloc((void **)&p->d_P, m * 16) != hipSuccess) {
            (void)hipGetLastError();
            fprintf(stderr, "mceik_mcmc_posterior_enable: out of device memory (%zu B of moments)\n",
                    2 * post_rows(p) * m * 8);
            kept_state_free(k, p);
            return -1;
        }
        kept_publish(s, k, p, "mceik_mcmc_posterior_enable");
    }
    if (kept_arrays_zero(a, post_arrays(p, a), s->stream) != hipSuccess) {
        (void)hipGetLastError();
        kept_clear(s, k);
        return -1;
    }
    k.n = 0;
    return 0;
}

extern "C" int mceik_mcmc_posterior_disable(mceik_mcmc *s) { return s ? kept_clear(s, s->kept[KEPT_POST]) : 1; }

extern "C" int mceik_mcmc_posterior_accumulate(mceik_mcmc *s) { return s ? kept_accumulate(s, s->kept[KEPT_POST]) : 1; }

extern "C" int mceik_mcmc_posterior_get(mceik_mcmc *s, long long *n, long long *sum, long long *sumsq, unsigned *hist)
{
    void *const host[] = {sum, sumsq, hist};
    return s ? kept_get(s, s->kept[KEPT_POST], n, host) : 1;
}

extern "C" int mceik_mcmc_posterior_set(mceik_mcmc *s, long long n, const long long *sum, const long long *sumsq,
                                        const unsigned *hist)
{
    const void *const host[] = {sum, sumsq, hist};
    return s ? kept_set(s, s->kept[KEPT_POST], n, host) : 1;
}

extern "C" int mceik_mcmc_posterior_partials(mceik_mcmc *s, mceik_posterior_partials *out)
{
    if (!s || !out || !s->kept[KEPT_POST].state) return 1;
    const McmcPost *p = (const McmcPost *)s->kept[KEPT_POST].state;
    if (!out->S || !out->Q || !out->P || (p->P.nbins && !out->hist)) return 1;
    const int ncm = p->ncm, ncold = temper_cold(s);
    {
        DeviceScope dg(s->device);
        hipLaunchKernelGGL(post_reduce_kernel, dim3((ncm + 63) / 64), dim3(64), 0, s->stream, p->P, ncold, ncm,
                           p->d_S, p->d_Q, p->d_P);
        HIPCHK(hipGetLastError());
    }
    if (mceik_mcmc_sync(s)) return -1;
    DeviceScope dg(s->device);
    HIPCHK(hipMemcpy(out->S, p->d_S, (size_t)ncm * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->Q, p->d_Q, (size_t)ncm * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->P, p->d_P, (size_t)ncm * 16, hipMemcpyDeviceToHost));
    if (p->P.nbins) {
        const size_t nh = (size_t)ncm * p->P.nbins;
        std::vector<unsigned> h(nh);
        HIPCHK(hipMemcpy(h.data(), p->P.hist, nh * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nh; k++) out->hist[k] = h[k];
    }
    out->ncm = ncm;
    out->nbins = p->P.nbins;
    out->per_chain = p->P.per_chain;
    out->nchains = ncold;
    out->nkept = s->kept[KEPT_POST].n;
    return 0;
}

// ---------------------------------------------------------------------------
// host only from here: no GPU call
extern "C" int mceik_posterior_merge(mceik_posterior_partials *dst, const mceik_posterior_partials *src)
{
    if (!dst || !src || !dst->S || !dst->Q || !dst->P || !src->S || !src->Q || !src->P) return 1;
    if (dst->ncm != src->ncm || dst->nbins != src->nbins || dst->per_chain != src->per_chain ||
        dst->nkept != src->nkept || dst->ncm < 0 || dst->nbins < 0)
        return 1;
    if (dst->nbins && (!dst->hist || !src->hist)) return 1;
    for (int i = 0; i < dst->ncm; i++) dst->S[i] += src->S[i];
    add128(dst->Q, src->Q, (size_t)dst->ncm);
    add128(dst->P, src->P, (size_t)dst->ncm);
    const size_t nh = (size_t)dst->ncm * dst->nbins;
    for (size_t k = 0; k < nh; k++) dst->hist[k] += src->hist[k];
    dst->nchains += src->nchains;
    return 0;
}

extern "C" int mceik_posterior_finish(const mceik_posterior_partials *p, double *mean, double *var, double *rhat)
{
    if (!p || !p->S || !p->Q || !p->P || p->ncm < 0 || p->nchains < 0 || p->nkept < 0) return 1;
    const long long M = p->nchains, n = p->nkept;
    const i128 N = (i128)M * n;
    const double dM = (double)M, dn = (double)n, dN = (double)N;
    const bool has_r = p->per_chain && M >= 2 && n >= 2;
    for (int i = 0; i < p->ncm; i++) {
        const i128 S = p->S[i];
        const i128 Q = (i128)get128(p->Q + 2 * (size_t)i), P = (i128)get128(p->P + 2 * (size_t)i);
        if (mean) mean[i] = N > 0 ? (double)S / dN : NAN;
        if (var) var[i] = N >= 2 ? (double)(N * Q - S * S) / (dN * (double)(N - 1)) : NAN;
        if (!rhat) continue;
        const i128 wnum = (i128)n * Q - P;
        if (!has_r || wnum == 0) {
            rhat[i] = NAN;
            continue;
        }
        const double W = (double)wnum / (dM * dn * (double)(n - 1));
        const double Bn = (double)((i128)M * P - S * S) / (dM * (double)(M - 1) * (dn * dn));
        rhat[i] = sqrt(((double)(n - 1) / dn * W + Bn) / W);
    }
    return 0;
}
