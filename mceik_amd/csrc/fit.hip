// fit.hip -- streaming pick residuals, origin times and data-fit checks
// (include/mceik.h mceik_mcmc_fit_*, mceik_fit_*), on gfx950.
//
// Kept states cannot be stored, so the data side of a run is streamed: per
// kept step and cold chain the origin time of every event and the residual of
// every used pick, exactly as the chain's logL sees them (event_obj's
// arithmetic on the chain's current tables and effective observations), as
// integers in exact sums.  Integer sums do not depend on the order of
// accumulation: pipes, launch paths, shards and ranks all give the same
// words, and partials merge by plain addition.  Means, spreads and the
// reduced misfits are formed on the host (mceik_fit_finish: no GPU call).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define HIPCHK_WHO "mceik_fit"
#include "fit.h"
#include "host_util.h"
#include "mcmc_device.h"
#include "sampler.h"

#define FIT_LANES 64               // picks (events) per block of the reduction: lane = pick
#define FIT_SLICE 64               // chains per block of the reduction
#define FIT_ZSCALE 1024.0          // zq = z * 1024
#define FIT_QMAX 2147483647.0

// rint(x) clamped to +-(2^31 - 1); a clamped value (and a NaN, which becomes
// the upper bound) is counted.
__device__ __forceinline__ int fit_sat32(double x, unsigned &nsat)
{
    const double r = rint(x);
    if (!(r <= FIT_QMAX)) { nsat++; return 2147483647; }
    if (r < -FIT_QMAX) { nsat++; return -2147483647; }
    return (int)r;
}

// w (lo, hi) += x modulo 2^128 (ess.hip's pair: the low word first, its carry
// into the high word).
__device__ __forceinline__ void fit_add128(unsigned long long *w, u128 x)
{
    const unsigned long long lo = (unsigned long long)x;
    unsigned long long hi = (unsigned long long)(x >> 64);
    if (lo) {
        const unsigned long long old = atomicAdd(&w[0], lo);
        hi += (unsigned long long)(old + lo < old);
    }
    if (hi) atomicAdd(&w[1], hi);
}

// One thread per (chain, event), events fastest: event_obj's three passes over
// the event's picks in CSR order with every phase from the current tables, so
// t0 and the residuals are the logL's bit for bit; the words of the pass go to
// the scratch rows of the chain.
__global__ __launch_bounds__(256) void fit_residual_kernel(McmcDev D, NuisDev N, FitDev F, int nchains)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nchains * D.nev) return;
    const int c = t / D.nev, e = t - c * D.nev;
    const McmcDev E = nuis_chain(D, N, c);
    const float *tcur = E.ttab_cur + (size_t)c * E.nphase * E.nstat * E.nev;
    auto te_of = [&](int j) -> double {
        const int ph = E.obs_phase ? E.obs_phase[j] : 0;
        return (double)mcmcd::ldv(tcur + ((size_t)ph * E.nstat + E.obs_stat[j]) * E.nev + e);
    };
    const int j0 = E.obs_ptr[e], j1 = E.obs_ptr[e + 1];
    int *q = F.q + (size_t)c * F.nobs, *zq = F.zq + (size_t)c * F.nobs, *bin = F.bin + (size_t)c * F.nobs;
    unsigned nsq = 0, nsz = 0, nst = 0;
    double xnorm = 0.0, t0 = 0.0;
    int nused = 0;
    for (int j = j0; j < j1; j++)
        if (!E.obs_mask[j]) { xnorm = xnorm + 1.0 / mcmcd::ldv(&E.var[j]); nused++; }
    if (E.l1) {
        // the L1 likelihood: the origin time is the weighted median of the logL (event_obj_l1's arithmetic)
        t0 = l1::median<double>(j0, j1, [&](int j) -> bool { return !E.obs_mask[j]; },
                                [&](int j) -> double { return (E.tobs[j] - mcmcd::ldv(&E.tcorr[j])) - te_of(j); },
                                [&](int j) -> double { return 1.0 / mcmcd::ldv(&E.var[j]); }, nullptr);
    } else {
        for (int j = j0; j < j1; j++) {
            if (E.obs_mask[j]) continue;
            const double te = te_of(j);
            const double tc = E.tobs[j] - mcmcd::ldv(&E.tcorr[j]);
            t0 = t0 + ((1.0 / mcmcd::ldv(&E.var[j])) / xnorm) * (tc - te);
        }
    }
    for (int j = j0; j < j1; j++) {
        if (E.obs_mask[j]) { q[j] = 0; zq[j] = 0; bin[j] = -1; continue; }
        const double te = te_of(j);
        const double tc = E.tobs[j] - mcmcd::ldv(&E.tcorr[j]);
        const double r = E.l1 ? (tc - te) - t0 : tc - (te + t0);
        const double z = (1.0 / mcmcd::ldv(&E.var[j])) * r;
        q[j] = fit_sat32(r * F.inv_tick, nsq);
        zq[j] = fit_sat32(z * FIT_ZSCALE, nsz);
        const double b = floor(z * F.hscale + F.half);
        bin[j] = !(b >= 0.0) ? 0 : b > (double)(F.nbins - 1) ? F.nbins - 1 : (int)b;
    }
    // (an event without a used pick has no origin time: its word stays 0)
    F.tq[(size_t)c * F.nev + e] = nused ? fit_sat32((t0 - F.t0_ref[e]) * F.inv_tick, nst) : 0;
    if (nsq) atomicAdd(&F.sat[0], (unsigned long long)nsq);
    if (nsz) atomicAdd(&F.sat[1], (unsigned long long)nsz);
    if (nst) atomicAdd(&F.sat[2], (unsigned long long)nst);
}

// Blocks [0, nbp) x slices: lane = pick, the slice's chains in a loop (a wave
// reads 256 contiguous bytes of q / zq / bin per chain); the sums stay in
// registers and leave as one atomic add per pooled word, the pipes and slices
// sharing the words.  The lane counts its bins in a column of LDS of its own
// ([bin][lane]: no conflicts, no atomics) and adds the nonzero ones to the
// row of its (phase, station).  Blocks [nbp, ...) do the same for the events'
// origin times.
__global__ __launch_bounds__(FIT_LANES) void fit_reduce_kernel(FitDev F, const int *obs_stat, const int *obs_phase,
                                                                const int *obs_mask, const int *obs_ptr, int nstat,
                                                                int nchains, int nbp)
{
    extern __shared__ unsigned fit_hl[];            // [nbins][FIT_LANES]
    const int lane = threadIdx.x;
    const int c0 = blockIdx.y * FIT_SLICE;
    const int c1 = nchains < c0 + FIT_SLICE ? nchains : c0 + FIT_SLICE;
    if ((int)blockIdx.x < nbp) {
        const int j = blockIdx.x * FIT_LANES + lane;
        if (j >= F.nobs || obs_mask[j]) return;
        for (int b = 0; b < F.nbins; b++) fit_hl[b * FIT_LANES + lane] = 0;
        long long a = 0, az = 0;
        u128 s2 = 0, sz2 = 0;
        for (int c = c0; c < c1; c++) {
            const size_t k = (size_t)c * F.nobs + j;
            const long long x = F.q[k], z = F.zq[k];
            const int b = F.bin[k];
            a += x;
            az += z;
            s2 += (u128)(unsigned long long)(x * x);
            sz2 += (u128)(unsigned long long)(z * z);
            if ((unsigned)b < (unsigned)F.nbins) fit_hl[b * FIT_LANES + lane]++;
        }
        if (a) atomicAdd((unsigned long long *)&F.sq[j], (unsigned long long)a);
        if (az) atomicAdd((unsigned long long *)&F.szq[j], (unsigned long long)az);
        fit_add128(F.sq2 + 2 * (size_t)j, s2);
        fit_add128(F.szq2 + 2 * (size_t)j, sz2);
        unsigned long long *row = F.hist + ((size_t)(obs_phase ? obs_phase[j] : 0) * nstat + obs_stat[j]) * F.nbins;
        for (int b = 0; b < F.nbins; b++) {
            const unsigned h = fit_hl[b * FIT_LANES + lane];
            if (h) atomicAdd(&row[b], (unsigned long long)h);
        }
    } else {
        const int e = ((int)blockIdx.x - nbp) * FIT_LANES + lane;
        if (e >= F.nev) return;
        long long a = 0;
        u128 s2 = 0;
        for (int c = c0; c < c1; c++) {
            const long long x = F.tq[(size_t)c * F.nev + e];
            a += x;
            s2 += (u128)(unsigned long long)(x * x);
        }
        if (a) atomicAdd((unsigned long long *)&F.stq[e], (unsigned long long)a);
        fit_add128(F.stq2 + 2 * (size_t)e, s2);
    }
}

// ---------------------------------------------------------------------------
// a sampler's data-fit state
#define FIT_NARR 8                 // sq, szq, sq2, szq2, stq, stq2, hist, sat

struct McmcFit {
    FitDev F;                      // every chain of the sampler
    int nchains, nphase, nstat;
    double tick, zmax;
    std::vector<double> t0_ref;    // [nev]
    double *d_t0_ref;
};

// sq, szq, sq2, szq2, stq, stq2, hist, sat: words of 8 bytes, 16 bytes of slack each
static int fit_arrays(void *state, KeptArray out[KEPT_MAX_ARRAYS])
{
    McmcFit *p = (McmcFit *)state;
    const size_t no = p->F.nobs, ne = p->F.nev;
    void **a[FIT_NARR] = {(void **)&p->F.sq,  (void **)&p->F.szq,  (void **)&p->F.sq2,  (void **)&p->F.szq2,
                          (void **)&p->F.stq, (void **)&p->F.stq2, (void **)&p->F.hist, (void **)&p->F.sat};
    const size_t w[FIT_NARR] = {no, no, 2 * no, 2 * no, ne, 2 * ne, (size_t)p->nphase * p->nstat * p->F.nbins, 3};
    for (int k = 0; k < FIT_NARR; k++) out[k] = {a[k], w[k] * 8, 16};
    return FIT_NARR;
}

static void fit_free_extra(void *state)
{
    McmcFit *p = (McmcFit *)state;
    void *all[] = {p->F.q, p->F.zq, p->F.bin, p->F.tq, p->d_t0_ref};
    for (void *q : all)
        if (q) hipFree(q);
    delete p;
}

// The kept-state hook's side (kept.h KeptStream::accumulate).  D.ttab_cur holds
// the chains' current tables (at the chains' own event nodes: H is not read).
static hipError_t fit_accumulate(void *state, const McmcDev &D, const HypoDev &, const NuisDev &N, int chain_off, int n,
                                 long long, hipStream_t st)
{
    const McmcFit *p = (const McmcFit *)state;
    if (n <= 0) return hipSuccess;
    if (!D.ttab_cur) return hipErrorInvalidValue;    // (enable makes a one-model sampler hold its current tables)
    FitDev F = p->F;
    F.q += (size_t)chain_off * F.nobs;
    F.zq += (size_t)chain_off * F.nobs;
    F.bin += (size_t)chain_off * F.nobs;
    F.tq += (size_t)chain_off * F.nev;
    const long long nt = (long long)n * D.nev;
    hipLaunchKernelGGL(fit_residual_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, D, N, F, n);
    const int nbp = (F.nobs + FIT_LANES - 1) / FIT_LANES, nbe = (F.nev + FIT_LANES - 1) / FIT_LANES;
    const dim3 grid(nbp + nbe, (n + FIT_SLICE - 1) / FIT_SLICE);
    hipLaunchKernelGGL(fit_reduce_kernel, grid, dim3(FIT_LANES), (size_t)F.nbins * FIT_LANES * sizeof(unsigned), st, F,
                       D.obs_stat, D.obs_phase, D.obs_mask, D.obs_ptr, D.nstat, n, nbp);
    return hipGetLastError();
}

KeptStream mcmc_fit_stream()
{
    KeptStream k = {};
    k.name = "the data-fit sums";
    k.needs_tables1 = true;
    k.arrays = fit_arrays;
    k.accumulate = fit_accumulate;
    k.free_extra = fit_free_extra;
    return k;
}

// tick = 2^k, k in [-64, 64]
static bool fit_tick_ok(double tick)
{
    int ex = 0;
    if (!(tick > 0.0) || !(tick <= 1.8446744073709552e19)) return false;
    return frexp(tick, &ex) == 0.5 && ex >= -63 && ex <= 65;
}

extern "C" int mceik_fit_check(double tick, double rmax)
{
    if (!fit_tick_ok(tick) || !(rmax >= 0.0)) return 1;
    return rint(rmax * (1.0 / tick)) <= FIT_QMAX ? 0 : 1;
}

static bool fit_same(const McmcFit *p, const mceik_fit_opts *o)
{
    if (p->tick != o->tick || p->F.nbins != o->nbins || p->zmax != o->zmax) return false;
    for (int e = 0; e < p->F.nev; e++) {
        const double r = o->t0_ref ? o->t0_ref[e] : 0.0;
        if (memcmp(&p->t0_ref[e], &r, 8) != 0) return false;
    }
    return true;
}

extern "C" int mceik_mcmc_fit_enable(mceik_mcmc *s, const mceik_fit_opts *o)
{
    if (!s || !o) return 1;
    if (!fit_tick_ok(o->tick) || o->nbins < 2 || o->nbins > MCEIK_FIT_MAX_BINS || o->nbins % 2 != 0 ||
        !(o->zmax > 0.0) || !(o->zmax <= 1e300))
        return 1;
    const McmcDev &D = s->D;
    const int nobs = (int)s->h_ostat.size(), nev = D.nev;
    for (int e = 0; e < nev && o->t0_ref; e++)
        if (!(fabs(o->t0_ref[e]) <= 1e300)) return 1;
    KeptStream &k = s->kept[KEPT_FIT];
    const int rc = kept_enable_held(s, k, k.state && fit_same((const McmcFit *)k.state, o), "mceik_mcmc_fit_enable");
    if (rc != KEPT_REPLACE) return rc;
    DeviceScope dg(s->device);
    McmcFit *p = new McmcFit();
    p->F.nobs = nobs;
    p->F.nev = nev;
    p->F.nbins = o->nbins;
    p->F.inv_tick = 1.0 / o->tick;
    p->F.hscale = (double)o->nbins / (2.0 * o->zmax);
    p->F.half = (double)(o->nbins / 2);
    p->nchains = D.nchains;
    p->nphase = D.nphase;
    p->nstat = D.nstat;
    p->tick = o->tick;
    p->zmax = o->zmax;
    p->t0_ref.assign((size_t)nev, 0.0);
    if (o->t0_ref) p->t0_ref.assign(o->t0_ref, o->t0_ref + nev);
    const size_t nch = (size_t)D.nchains, no = nobs > 0 ? nobs : 1;
    KeptArray a[KEPT_MAX_ARRAYS], rows[5] = {{(void **)&p->F.q, nch * no * 4, 0},
                                             {(void **)&p->F.zq, nch * no * 4, 0},
                                             {(void **)&p->F.bin, nch * no * 4, 0},
                                             {(void **)&p->F.tq, nch * nev * 4, 0},
                                             {(void **)&p->d_t0_ref, (size_t)nev * 8, 0}};
    const bool ok = kept_arrays_alloc(rows, 5) && kept_arrays_alloc(a, fit_arrays(p, a)) &&
                    hipMemcpy(p->d_t0_ref, p->t0_ref.data(), (size_t)nev * 8, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        fprintf(stderr, "mceik_mcmc_fit_enable: out of device memory (%zu B of scratch rows)\n",
                nch * (3 * no + nev) * 4);
        kept_state_free(k, p);
        return -1;
    }
    p->F.t0_ref = p->d_t0_ref;
    return kept_publish(s, k, p, "mceik_mcmc_fit_enable");
}

extern "C" int mceik_mcmc_fit_disable(mceik_mcmc *s) { return s ? kept_disable(s, s->kept[KEPT_FIT]) : 1; }

extern "C" int mceik_mcmc_fit_clear(mceik_mcmc *s) { return s ? kept_clear(s, s->kept[KEPT_FIT]) : 1; }

extern "C" int mceik_mcmc_fit_accumulate(mceik_mcmc *s) { return s ? kept_accumulate(s, s->kept[KEPT_FIT]) : 1; }

extern "C" int mceik_mcmc_fit_get(mceik_mcmc *s, long long *n, long long *sq, long long *szq, unsigned long long *sq2,
                                  unsigned long long *szq2, long long *stq, unsigned long long *stq2, long long *hist,
                                  long long *sat)
{
    void *const host[] = {sq, szq, sq2, szq2, stq, stq2, hist, sat};
    return s ? kept_get(s, s->kept[KEPT_FIT], n, host) : 1;
}

extern "C" int mceik_mcmc_fit_set(mceik_mcmc *s, long long n, const long long *sq, const long long *szq,
                                  const unsigned long long *sq2, const unsigned long long *szq2, const long long *stq,
                                  const unsigned long long *stq2, const long long *hist, const long long *sat)
{
    const void *const host[] = {sq, szq, sq2, szq2, stq, stq2, hist, sat};
    return s ? kept_set(s, s->kept[KEPT_FIT], n, host) : 1;
}

extern "C" int mceik_mcmc_fit_last(mceik_mcmc *s, int *q, int *zq, int *tq)
{
    if (!s || !s->kept[KEPT_FIT].state) return 1;
    const McmcFit *p = (const McmcFit *)s->kept[KEPT_FIT].state;
    if (mceik_mcmc_sync(s)) return -1;
    DeviceScope dg(s->device);
    const size_t nch = (size_t)p->nchains;
    if (q && p->F.nobs) HIPCHK(hipMemcpy(q, p->F.q, nch * p->F.nobs * 4, hipMemcpyDeviceToHost));
    if (zq && p->F.nobs) HIPCHK(hipMemcpy(zq, p->F.zq, nch * p->F.nobs * 4, hipMemcpyDeviceToHost));
    if (tq) HIPCHK(hipMemcpy(tq, p->F.tq, nch * p->F.nev * 4, hipMemcpyDeviceToHost));
    return 0;
}

static bool fit_parts_ok(const mceik_fit_partials *p)
{
    return p && p->nobs >= 0 && p->nev >= 1 && p->nphase >= 1 && p->nphase <= 2 && p->nstat >= 1 && p->nbins >= 2 &&
           p->nbins <= MCEIK_FIT_MAX_BINS && p->nchains >= 0 && p->nkept >= 0 && p->obs_ptr && p->obs_stat &&
           p->obs_phase && p->obs_mask && p->t0_ref && p->sq && p->szq && p->sq2 && p->szq2 && p->stq && p->stq2 &&
           p->hist;
}

extern "C" int mceik_mcmc_fit_partials(mceik_mcmc *s, mceik_fit_partials *out)
{
    if (!s || !out || !s->kept[KEPT_FIT].state) return 1;
    const McmcFit *p = (const McmcFit *)s->kept[KEPT_FIT].state;
    out->nobs = p->F.nobs; out->nev = p->F.nev; out->nphase = p->nphase; out->nstat = p->nstat; out->nbins = p->F.nbins;
    if (!fit_parts_ok(out)) return 1;
    out->tick = p->tick;
    out->zmax = p->zmax;
    out->nchains = temper_cold(s);
    out->nkept = s->kept[KEPT_FIT].n;
    if (mceik_mcmc_fit_get(s, nullptr, out->sq, out->szq, out->sq2, out->szq2, out->stq, out->stq2, out->hist, out->sat))
        return -1;
    DeviceScope dg(s->device);
    HIPCHK(hipMemcpy(out->obs_ptr, s->D.obs_ptr, ((size_t)p->F.nev + 1) * sizeof(int), hipMemcpyDeviceToHost));
    for (int j = 0; j < p->F.nobs; j++) {
        out->obs_stat[j] = s->h_ostat[j];
        out->obs_phase[j] = s->h_ophase[j];
        out->obs_mask[j] = s->h_omask[j];
    }
    memcpy(out->t0_ref, p->t0_ref.data(), (size_t)p->F.nev * 8);
    return 0;
}

// ---------------------------------------------------------------------------
// host only from here: no GPU call
extern "C" int mceik_fit_merge(mceik_fit_partials *dst, const mceik_fit_partials *src)
{
    if (!fit_parts_ok(dst) || !fit_parts_ok(src)) return 1;
    if (dst->nobs != src->nobs || dst->nev != src->nev || dst->nphase != src->nphase || dst->nstat != src->nstat ||
        dst->nbins != src->nbins || dst->tick != src->tick || dst->zmax != src->zmax || dst->nkept != src->nkept)
        return 1;
    const size_t no = (size_t)dst->nobs, ne = (size_t)dst->nev;
    if (memcmp(dst->obs_ptr, src->obs_ptr, (ne + 1) * sizeof(int)) || memcmp(dst->obs_stat, src->obs_stat, no * sizeof(int)) ||
        memcmp(dst->obs_phase, src->obs_phase, no * sizeof(int)) || memcmp(dst->obs_mask, src->obs_mask, no * sizeof(int)) ||
        memcmp(dst->t0_ref, src->t0_ref, ne * 8))
        return 1;
    auto add64 = [](long long *d, const long long *a, size_t n) {
        for (size_t k = 0; k < n; k++) d[k] = (long long)((unsigned long long)d[k] + (unsigned long long)a[k]);
    };
    add64(dst->sq, src->sq, no);
    add64(dst->szq, src->szq, no);
    add64(dst->stq, src->stq, ne);
    add64(dst->hist, src->hist, (size_t)dst->nphase * dst->nstat * dst->nbins);
    add64(dst->sat, src->sat, 3);
    add128(dst->sq2, src->sq2, no);
    add128(dst->szq2, src->szq2, no);
    add128(dst->stq2, src->stq2, ne);
    dst->nchains += src->nchains;
    return 0;
}

// mean and sample standard deviation of N values with sum S and sum of squares
// Q, in units of `unit`: the numerator N Q - S^2 is an exact integer (below
// 2^127 while N < 2^32 and |value| < 2^31), converted to double once.
static void fit_mean_sd(long long S, u128 Q, double dN, long long N, double unit, double *mean, double *sd)
{
    *mean = (double)S * unit / dN;
    const i128 num = (i128)N * (i128)Q - (i128)S * (i128)S;
    *sd = sqrt((double)num / (dN * (dN - 1.0))) * unit;
}

extern "C" int mceik_fit_finish(const mceik_fit_partials *p, double *pick_mean, double *pick_sd, double *pick_zmean,
                                double *pick_zrms, double *t0_mean, double *t0_sd, double *ev_misfit, double *sta_mean,
                                double *sta_zrms, double *phase_zrms)
{
    if (!fit_parts_ok(p)) return 1;
    const long long N = p->nchains * p->nkept;
    const bool have = p->nkept >= 2 && p->nchains >= 1;
    const double dN = (double)N, zs2 = FIT_ZSCALE * FIT_ZSCALE;
    const int nrow = p->nphase * p->nstat;
    for (int j = 0; j < p->nobs; j++) {
        double m = NAN, sd = NAN, zm = NAN, zr = NAN;
        if (have && !p->obs_mask[j]) {
            fit_mean_sd(p->sq[j], get128(p->sq2 + 2 * (size_t)j), dN, N, p->tick, &m, &sd);
            zm = (double)p->szq[j] / FIT_ZSCALE / dN;
            zr = sqrt((double)get128(p->szq2 + 2 * (size_t)j) / (zs2 * dN));
        }
        if (pick_mean) pick_mean[j] = m;
        if (pick_sd) pick_sd[j] = sd;
        if (pick_zmean) pick_zmean[j] = zm;
        if (pick_zrms) pick_zrms[j] = zr;
    }
    for (int e = 0; e < p->nev; e++) {
        long long nused = 0;
        u128 z2 = 0;
        for (int j = p->obs_ptr[e]; j < p->obs_ptr[e + 1]; j++)
            if (!p->obs_mask[j]) { nused++; z2 += get128(p->szq2 + 2 * (size_t)j); }
        double m = NAN, sd = NAN;
        if (have && nused >= 1) {
            fit_mean_sd(p->stq[e], get128(p->stq2 + 2 * (size_t)e), dN, N, p->tick, &m, &sd);
            m = m + p->t0_ref[e];
        }
        if (t0_mean) t0_mean[e] = m;
        if (t0_sd) t0_sd[e] = sd;
        if (ev_misfit) ev_misfit[e] = have && nused >= 2 ? (double)z2 / (zs2 * dN * (double)(nused - 1)) : NAN;
    }
    std::vector<long long> cnt((size_t)nrow, 0), sq((size_t)nrow, 0);
    std::vector<u128> z2((size_t)nrow, 0);
    for (int j = 0; j < p->nobs; j++) {
        if (p->obs_mask[j]) continue;
        const size_t r = (size_t)p->obs_phase[j] * p->nstat + p->obs_stat[j];
        if (p->obs_phase[j] < 0 || p->obs_phase[j] >= p->nphase || p->obs_stat[j] < 0 || p->obs_stat[j] >= p->nstat) return 1;
        cnt[r]++;
        sq[r] = (long long)((unsigned long long)sq[r] + (unsigned long long)p->sq[j]);
        z2[r] += get128(p->szq2 + 2 * (size_t)j);
    }
    for (int ph = 0; ph < p->nphase; ph++) {
        long long pc = 0;
        u128 pz = 0;
        for (int k = 0; k < p->nstat; k++) {
            const size_t r = (size_t)ph * p->nstat + k;
            const bool any = have && cnt[r] > 0;
            if (sta_mean) sta_mean[r] = any ? (double)sq[r] * p->tick / (dN * (double)cnt[r]) : NAN;
            if (sta_zrms) sta_zrms[r] = any ? sqrt((double)z2[r] / (zs2 * dN * (double)cnt[r])) : NAN;
            pc += cnt[r];
            pz += z2[r];
        }
        if (phase_zrms) phase_zrms[ph] = have && pc > 0 ? sqrt((double)pz / (zs2 * dN * (double)pc)) : NAN;
    }
    return 0;
}
