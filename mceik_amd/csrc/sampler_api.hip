// sampler_api.hip -- the sampler's accessors of the C-ABI (include/mceik.h:
// sync, state, checkpoint / restore, kept samples, info, FSM statistics) and
// its parallel-tempering, block-proposal, prior, hypocentre, noise / statics,
// Langevin, differential-evolution and Voronoi-cell entry points.
// The sampler itself is sampler.hip.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fsm_batch.h"
#include "fsm_host.h"
#include "host_util.h"
#include "mcmc_host.h"
#include "sampler.h"

// Voronoi-cell models are on: the moves that change single cells of v are refused.
static int vor_refuses(const mceik_mcmc *s, const char *who)
{
    if (!s->vor_on) return 0;
    fprintf(stderr, "%s: Voronoi-cell models are on (mceik_mcmc_vor_enable): v is the raster of the nuclei, which this "
                    "feature would not keep\n", who);
    return 1;
}

// The posterior holds states: a change of what the chains sample is refused.
static bool post_holds_states(const mceik_mcmc *s) { return s->kept[KEPT_POST].state && s->kept[KEPT_POST].n > 0; }

// The body of the *_stats entry points: n words of each counter array to the
// host (synchronises), then with reset nreset zero words from `zero` on.
static int get_counts(mceik_mcmc *s, const unsigned long long *att, const unsigned long long *acc, size_t n,
                      long long *attempts, long long *accepts, int reset, unsigned long long *zero, size_t nreset)
{
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (attempts && n) HIPCHK(hipMemcpy(attempts, att, n * 8, hipMemcpyDeviceToHost));
    if (accepts && n) HIPCHK(hipMemcpy(accepts, acc, n * 8, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(zero, 0, nreset * 8));
    return 0;
}

// One forward of every model of every chain at the chains' positions, and
// logL from it (not timed, not counted in the FSM stats).  Synchronises.
static int forward_logl(mceik_mcmc *s, const char *who)
{
    unsigned long long keep[MCEIK_ITERS_N];
    HIPCHK(hipMemcpy(keep, s->d_iters, sizeof(keep), hipMemcpyDeviceToHost));
    if (mcmc_forward_all(s)) return -1;
    HIPCHK(mcmc_init_loglik(s->D, s->N, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(s->d_iters, keep, sizeof(keep), hipMemcpyHostToDevice));
    return check_forward_ierr(s, who) ? 2 : 0;
}

// A one-model sampler's current tables (sampler.h).
int mcmc_tables1_hold(mceik_mcmc *s, const char *who)
{
    if (s->D.nphase != 1 || s->D.ttab_cur) return 0;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (!s->ttab_cur1 && dalloc(s, &s->ttab_cur1, (size_t)s->D.nchains * s->D.nstat * s->D.nev)) return -1;
    s->D.ttab_cur = s->ttab_cur1;
    s->fb_all.ttab = s->ttab_cur1;
    if (pipes_refresh(s)) return -1;
    return forward_logl(s, who);
}

int mcmc_tables1_drop(mceik_mcmc *s)
{
    if (s->D.nphase != 1 || !s->D.ttab_cur || s->N.kn || kept_needs_tables1(s)) return 0;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->D.ttab_cur = nullptr;
    s->fb_all.ttab = s->fb.ttab;
    return pipes_refresh(s);
}

// ---------------------------------------------------------------------------
// the lifecycle of the accumulators of kept states (sampler.h; kept.h)

void kept_state_free(KeptStream &k, void *state)
{
    if (!state) return;
    KeptArray a[KEPT_MAX_ARRAYS];
    kept_arrays_free(a, k.arrays(state, a));
    k.free_extra(state);
}

int kept_enable_held(mceik_mcmc *s, KeptStream &k, bool same, const char *who)
{
    if (k.state && same) {                           // the held sums go on
        k.on = true;
        return k.needs_tables1 ? mcmc_tables1_hold(s, who) : 0;
    }
    if (k.state && k.n > 0) return 1;                // held states of other options
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    void *old = k.state;
    k.state = nullptr;
    k.on = false;
    k.n = 0;
    kept_state_free(k, old);
    return KEPT_REPLACE;
}

int kept_publish(mceik_mcmc *s, KeptStream &k, void *state, const char *who)
{
    k.state = state;
    k.on = true;
    k.n = 0;
    return k.needs_tables1 ? mcmc_tables1_hold(s, who) : 0;
}

int kept_disable(mceik_mcmc *s, KeptStream &k)
{
    if (!k.on) return 0;
    k.on = false;                      // host state only: queued steps keep the kernels they were queued with
    return k.needs_tables1 ? mcmc_tables1_drop(s) : 0;   // (a one-model sampler stops holding its current tables unless nuisance state needs them)
}

int kept_clear(mceik_mcmc *s, KeptStream &k)
{
    if (!k.state) return 0;
    DeviceScope dg(s->device);
    const hipError_t e = hipStreamSynchronize(s->stream);
    kept_state_free(k, k.state);
    k.state = nullptr;
    k.on = false;
    k.n = 0;
    const int rc = k.needs_tables1 ? mcmc_tables1_drop(s) : 0;
    return e == hipSuccess ? rc : -1;
}

int kept_accumulate(mceik_mcmc *s, KeptStream &k)
{
    if (!k.state || !k.on) return 1;
    DeviceScope dg(s->device);
    HIPCHK(k.accumulate(k.state, s->D, s->H, s->N, 0, temper_cold(s), k.n, s->stream));   // tempering: the cold chains
    k.n++;
    return 0;
}

int kept_get(mceik_mcmc *s, KeptStream &k, long long *n, void *const *host)
{
    if (!k.state) return 1;
    if (mceik_mcmc_sync(s)) return -1;
    DeviceScope dg(s->device);
    if (n) *n = k.n;
    KeptArray a[KEPT_MAX_ARRAYS];
    const int na = k.arrays(k.state, a);
    HIPCHK(kept_arrays_copy(a, na, host, true));
    return 0;
}

int kept_set(mceik_mcmc *s, KeptStream &k, long long n, const void *const *host)
{
    if (!k.state || n < 0) return 1;
    KeptArray a[KEPT_MAX_ARRAYS];
    const int na = k.arrays(k.state, a);
    if (kept_arrays_missing(a, na, host)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(kept_arrays_copy(a, na, (void *const *)host, false));
    k.n = n;
    return 0;
}

// ---------------------------------------------------------------------------
// the likelihood's norm (include/mceik.h mceik_mcmc_likelihood_*)

// An enabled accumulator of kept states holds some: a change of what the
// chains sample would mix two posteriors in its sums.
static const char *kept_stream_holding(const mceik_mcmc *s)
{
    for (const KeptStream &k : s->kept)
        if (k.on && k.n > 0) return k.name;
    if (s->hypo_on && s->hyp_n > 0) return "the hypocentre moments";
    if (s->nuis_on && s->nuis_n > 0) return "the noise / statics moments";
    if (s->vor_on && s->vor_n > 0) return "the Voronoi-cell moments";
    return nullptr;
}

extern "C" int mceik_mcmc_likelihood_set(mceik_mcmc *s, int norm)
{
    if (!s || (norm != 1 && norm != 2)) return 1;
    const char *who = "mceik_mcmc_likelihood_set";
    if (s->lang_on) {
        fprintf(stderr, "%s: Langevin moves are on: their gradient is the L2 misfit's\n", who);
        return 1;
    }
    if (const char *what = kept_stream_holding(s)) {
        fprintf(stderr, "%s: %s already hold states of the other likelihood\n", who, what);
        return 1;
    }
    if ((s->D.l1 != 0) == (norm == 1)) return 0;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->D.l1 = norm == 1 ? 1 : 0;
    if (pipes_refresh(s)) return -1;
    return forward_logl(s, who);       // every chain's logL under the new norm; step counter and models untouched
}

extern "C" int mceik_mcmc_likelihood_get(const mceik_mcmc *s) { return s ? (s->D.l1 ? 1 : 2) : 0; }

// ---------------------------------------------------------------------------
// parallel tempering (include/mceik.h mceik_mcmc_temper_*)

extern "C" int mceik_temper_ladder(int ntemps, double tmax, double *beta)
{
    if (ntemps < 1 || !beta || !(tmax >= 1.0) || !(tmax <= DBL_MAX)) return 1;
    beta[0] = 1.0;
    for (int r = 1; r < ntemps; r++) beta[r] = pow(tmax, -(double)r / (double)(ntemps - 1));
    return 0;
}

extern "C" int mceik_mcmc_temper_enable(mceik_mcmc *s, const mceik_temper_opts *o)
{
    if (!s || !o || !o->beta || o->ntemps < 1 || o->swap_every < 0) return 1;
    const int nch = s->D.nchains, nt = o->ntemps;
    if (nch % nt != 0 || o->beta[0] != 1.0) return 1;
    for (int r = 0; r + 1 < nt; r++)
        if (!(o->beta[r + 1] > 0.0 && o->beta[r + 1] <= o->beta[r])) return 1;
    if (post_holds_states(s)) return 1;
    if (s->de_on && nch / nt < 4) {
        fprintf(stderr, "mceik_mcmc_temper_enable: DE moves are on and a rung would hold %d chains; a DE population "
                        "needs 4\n", nch / nt);
        return 1;
    }
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (!s->d_beta && (dalloc(s, &s->d_beta, nch) || dalloc(s, &s->d_tflag, nch) || dalloc(s, &s->d_tcnt, 2 * (size_t)nch)))
        return -1;
    const int G = nch / nt;
    std::vector<double> bc(nch);
    for (int c = 0; c < nch; c++) bc[c] = o->beta[c / G];
    HIPCHK(hipMemcpy(s->d_beta, bc.data(), (size_t)nch * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(s->d_tcnt, 0, 2 * (size_t)nch * 8));
    s->beta.assign(o->beta, o->beta + nt);
    s->ntemps = nt;
    s->swap_every = o->swap_every;
    s->D.beta = nt > 1 ? s->d_beta : nullptr;       // one rung is the untempered sampler
    return s->De.a ? de_lists(s) : pipes_refresh(s);   // D.beta changed, and the DE populations with the rungs
}

extern "C" int mceik_mcmc_temper_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    if (!s->ntemps) return 0;
    if (post_holds_states(s)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->ntemps = 0;
    s->swap_every = 0;
    s->beta.clear();
    s->D.beta = nullptr;
    return s->De.a ? de_lists(s) : pipes_refresh(s);   // D.beta changed, and the DE populations with the rungs
}

extern "C" int mceik_mcmc_temper_get(mceik_mcmc *s, int *ntemps, int *swap_every, double *beta)
{
    if (!s || !s->ntemps) return 1;
    if (ntemps) *ntemps = s->ntemps;
    if (swap_every) *swap_every = s->swap_every;
    if (beta) memcpy(beta, s->beta.data(), (size_t)s->ntemps * 8);
    return 0;
}

extern "C" int mceik_mcmc_temper_stats(mceik_mcmc *s, long long *attempts, long long *accepts, int reset)
{
    if (!s || !s->ntemps) return 1;
    return get_counts(s, s->d_tcnt, s->d_tcnt + s->D.nchains, (size_t)s->ntemps - 1, attempts, accepts, reset, s->d_tcnt,
                      2 * (size_t)s->D.nchains);
}

extern "C" int mceik_mcmc_temper_swap(mceik_mcmc *s, int parity)
{
    if (!s || !s->ntemps || (parity != 0 && parity != 1)) return 1;
    DeviceScope dg(s->device);
    return temper_round(s, parity);
}

// ---------------------------------------------------------------------------
// block proposals (include/mceik.h mceik_mcmc_block_*)

extern "C" int mceik_mcmc_block_enable(mceik_mcmc *s, const mceik_block_opts *o)
{
    if (!s || !o || o->rmin < 0 || o->rmax < o->rmin || o->rmax > MCEIK_BLOCK_RMAX) return 1;
    if (vor_refuses(s, "mceik_mcmc_block_enable")) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const int nch = s->D.nchains, nr = MCEIK_BLOCK_RMAX + 1;
    if (!s->d_bcnt) {                  // all three or none: a failed enable leaves the sampler as it was
        unsigned long long *cnt = nullptr;
        int *amp = nullptr, *rad = nullptr;
        if (dalloc(s, &cnt, 2 * (size_t)nr) || dalloc(s, &amp, nch) || dalloc(s, &rad, nch)) return -1;
        s->d_bcnt = cnt;
        s->B.prop_amp = amp;
        s->B.prop_rad = rad;
    }
    HIPCHK(hipMemset(s->d_bcnt, 0, 2 * (size_t)nr * 8));
    s->B.rmin = o->rmin;
    s->B.rmax = o->rmax;
    s->B.attempts = s->d_bcnt;
    s->B.accepts = s->d_bcnt + nr;
    s->block_on = true;
    return pipes_refresh(s);
}

extern "C" int mceik_mcmc_block_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    if (!s->block_on) return 0;
    s->block_on = false;               // host state only: queued steps keep the kernels they were queued with
    DeviceScope dg(s->device);
    return pipes_refresh(s);
}

extern "C" int mceik_mcmc_block_get(mceik_mcmc *s, int *rmin, int *rmax)
{
    if (!s || !s->block_on) return 1;
    if (rmin) *rmin = s->B.rmin;
    if (rmax) *rmax = s->B.rmax;
    return 0;
}

extern "C" int mceik_mcmc_block_stats(mceik_mcmc *s, long long *attempts, long long *accepts, int reset)
{
    if (!s || !s->block_on) return 1;
    return get_counts(s, s->B.attempts, s->B.accepts, (size_t)s->B.rmax + 1, attempts, accepts, reset, s->d_bcnt,
                      2 * (size_t)(MCEIK_BLOCK_RMAX + 1));
}

extern "C" int mceik_block_footprint(int ncx, int ncy, int ncz, int cell, int radius, int amp, int *cells, int *dv)
{
    if (ncx < 1 || ncy < 1 || ncz < 1 || (long long)ncx * ncy * ncz > INT_MAX || cell < 0 || cell >= ncx * ncy * ncz ||
        radius < 0 || radius > MCEIK_BLOCK_RMAX || amp == 0 || amp == INT_MIN)
        return -1;
    const int cx = cell % ncx, cy = (cell / ncx) % ncy, cz = cell / (ncx * ncy);
    const int mag = amp < 0 ? -amp : amp, n = 2 * radius + 1;
    int cnt = 0;
    for (int k = 0; k < n * n * n; k++) {
        int t = 0;
        const int d = block_dv(ncx, ncy, ncz, cx, cy, cz, radius, mag, k, &t);
        if (!d) continue;
        if (cells) cells[cnt] = t;
        if (dv) dv[cnt] = amp < 0 ? -d : d;
        cnt++;
    }
    return cnt;
}

// ---------------------------------------------------------------------------
// smoothness / reference-model prior (include/mceik.h mceik_mcmc_prior_*)

static bool prior_weight_ok(double w) { return w >= 0.0 && w <= DBL_MAX; }

extern "C" int mceik_mcmc_prior_enable(mceik_mcmc *s, const mceik_prior_opts *o)
{
    if (!s || !o) return 1;
    if (vor_refuses(s, "mceik_mcmc_prior_enable")) return 1;
    const McmcDev &D = s->D;
    for (int ph = 0; ph < 2; ph++)
        if (!prior_weight_ok(o->w_smooth[ph]) || !prior_weight_ok(o->w_damp[ph])) return 1;
    for (int ph = 0; ph < D.nphase; ph++) {
        const long long lo = ph ? D.vsmin : D.vmin, hi = ph ? D.vsmax : D.vmax;
        if (!prior_fits(D.ncell, hi - lo + 2LL * D.dvmax)) {
            fprintf(stderr, "mceik_mcmc_prior_enable: 3 ncell (hi - lo + 2 dvmax)^2 >= 2^53 for the %s model: the "
                            "energies would not convert to double exactly\n", ph ? "S" : "P");
            return 1;
        }
    }
    if (o->vref)
        for (int i = 0; i < D.ncm; i++) {
            const bool sph = i >= D.ncell;
            const int lo = sph ? D.vsmin : D.vmin, hi = sph ? D.vsmax : D.vmax;
            if (o->vref[i] < lo || o->vref[i] > hi) {
                fprintf(stderr, "mceik_mcmc_prior_enable: vref[%d] = %d outside the box [%d, %d]\n", i, o->vref[i], lo, hi);
                return 1;
            }
        }
    if (post_holds_states(s)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const int nch = D.nchains;
    if (!s->P.dE) {                    // all three or none: a failed enable leaves the sampler as it was
        long long *dE = nullptr;
        unsigned long long *pen = nullptr;
        int *vref = nullptr;
        if (dalloc(s, &dE, 2 * (size_t)nch) || dalloc(s, &pen, 2 * (size_t)nch * D.nphase) || dalloc(s, &vref, D.ncm))
            return -1;
        s->P.dE = dE;
        s->d_pen = pen;
        s->d_vref = vref;
    }
    HIPCHK(hipMemset(s->P.dE, 0, 2 * (size_t)nch * 8));
    if (o->vref) HIPCHK(hipMemcpy(s->d_vref, o->vref, (size_t)D.ncm * sizeof(int), hipMemcpyHostToDevice));
    s->prior_vref = o->vref != nullptr;
    s->P.vref = o->vref ? s->d_vref : nullptr;
    s->P.ws0 = o->w_smooth[0]; s->P.ws1 = o->w_smooth[1];
    s->P.wd0 = o->w_damp[0]; s->P.wd1 = o->w_damp[1];
    s->prior_on = true;
    return pipes_refresh(s);
}

extern "C" int mceik_mcmc_prior_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    if (!s->prior_on) return 0;
    if (post_holds_states(s)) return 1;
    s->prior_on = false;               // host state only: queued steps keep the kernels they were queued with
    return 0;
}

extern "C" int mceik_mcmc_prior_get(mceik_mcmc *s, mceik_prior_opts *o, int *vref)
{
    if (!s || !s->prior_on) return 1;
    if (o) {
        o->w_smooth[0] = s->P.ws0; o->w_smooth[1] = s->P.ws1;
        o->w_damp[0] = s->P.wd0; o->w_damp[1] = s->P.wd1;
        o->vref = s->prior_vref ? vref : nullptr;
    }
    if (vref && s->prior_vref) {
        DeviceScope dg(s->device);
        HIPCHK(hipMemcpy(vref, s->d_vref, (size_t)s->D.ncm * sizeof(int), hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int mceik_mcmc_prior_energy(mceik_mcmc *s, long long *Es, long long *Ed)
{
    if (!s || !s->prior_on) return 1;
    DeviceScope dg(s->device);
    const size_t n = (size_t)s->D.nchains * s->D.nphase;
    HIPCHK(hipMemsetAsync(s->d_pen, 0, 2 * n * 8, s->stream));
    HIPCHK(prior_energy(s->D, s->B, s->P, s->d_pen, s->d_pen + n, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (Es) HIPCHK(hipMemcpy(Es, s->d_pen, n * 8, hipMemcpyDeviceToHost));
    if (Ed) HIPCHK(hipMemcpy(Ed, s->d_pen + n, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_prior_last(mceik_mcmc *s, long long *dE)
{
    if (!s || !s->prior_on || !dE) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(dE, s->P.dE, 2 * (size_t)s->D.nchains * 8, hipMemcpyDeviceToHost));
    return 0;
}

static int prior_grid_ok(int ncx, int ncy, int ncz)
{
    return ncx >= 1 && ncy >= 1 && ncz >= 1 && (long long)ncx * ncy * ncz <= INT_MAX;
}

// Largest minus smallest value of v (and vref) over n cells.
static long long prior_span(const int *v, const int *vref, int n)
{
    long long lo = v[0], hi = v[0];
    for (int i = 0; i < n; i++) {
        lo = std::min<long long>(lo, v[i]);
        hi = std::max<long long>(hi, v[i]);
        if (vref) {
            lo = std::min<long long>(lo, vref[i]);
            hi = std::max<long long>(hi, vref[i]);
        }
    }
    return hi - lo;
}

extern "C" int mceik_prior_energy(int ncx, int ncy, int ncz, const int *v, const int *vref, long long *Es,
                                  long long *Ed)
{
    if (!prior_grid_ok(ncx, ncy, ncz) || !v) return 1;
    const int n = ncx * ncy * ncz;
    if (!prior_fits(n, prior_span(v, vref, n))) return 1;
    long long es = 0, ed = 0;
    for (int i = 0; i < n; i++) prior_energy_cell(ncx, ncy, ncz, i, v, vref, &es, &ed);
    if (Es) *Es = es;
    if (Ed) *Ed = ed;
    return 0;
}

extern "C" int mceik_prior_delta(int ncx, int ncy, int ncz, const int *v, const int *vref, int cell, int radius,
                                 int amp, long long *dEs, long long *dEd)
{
    if (!prior_grid_ok(ncx, ncy, ncz) || !v || cell < 0 || cell >= ncx * ncy * ncz || radius < 0 ||
        radius > MCEIK_BLOCK_RMAX || amp == 0 || amp == INT_MIN)
        return 1;
    const int n = ncx * ncy * ncz;
    if (!prior_fits(n, prior_span(v, vref, n) + 2LL * (amp < 0 ? -(long long)amp : amp))) return 1;
    const int cx = cell % ncx, cy = (cell / ncx) % ncy, cz = cell / (ncx * ncy);
    const int m = 2 * radius + 2;
    long long es = 0, ed = 0;
    for (int k = 0; k < m * m * m; k++) prior_delta_cell(ncx, ncy, ncz, cx, cy, cz, radius, amp, k, v, vref, &es, &ed);
    if (dEs) *dEs = es;
    if (dEd) *dEd = ed;
    return 0;
}

// ---------------------------------------------------------------------------
// hypocentre moves (include/mceik.h mceik_mcmc_hypo_*)

static bool hypo_in(const int *q, const int *lo, const int *hi)
{
    return q[0] >= lo[0] && q[0] <= hi[0] && q[1] >= lo[1] && q[1] <= hi[1] && q[2] >= lo[2] && q[2] <= hi[2];
}

// Every position of xyz [n][3] inside [lo, hi]; names the first that is not.
static bool hypo_all_in(const char *who, const int *xyz, size_t n, int nev, const int *lo, const int *hi)
{
    for (size_t i = 0; i < n; i++)
        if (!hypo_in(xyz + 3 * i, lo, hi)) {
            fprintf(stderr, "%s: chain %zu, event %zu at node (%d, %d, %d) outside [%d, %d] x [%d, %d] x [%d, %d]\n", who,
                    i / nev, i % nev, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
            return false;
        }
    return true;
}

extern "C" int mceik_mcmc_hypo_enable(mceik_mcmc *s, const mceik_hypo_opts *o)
{
    if (!s || !o || o->every < 0) return 1;
    const McmcDev &D = s->D;
    const int n[3] = {s->fb.nx, s->fb.ny, s->fb.nz};
    for (int a = 0; a < 3; a++)
        if (o->dmax[a] < 0 || o->dmax[a] > 0x3fffffff || o->lo[a] > o->hi[a] || o->lo[a] < 0 || o->hi[a] >= n[a]) return 1;
    if (s->tt_interp) {
        fprintf(stderr, "mceik_mcmc_hypo_enable: hypocentres move by whole nodes; not with tt_interp = 1\n");
        return 1;
    }
    if (post_holds_states(s)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const int nch = D.nchains, nev = D.nev, nph = D.nphase;
    const size_t ne = (size_t)nch * nev;
    // the chains' positions: the catalogue's snapped nodes before the first enable
    std::vector<int> xyz(ne * 3);
    if (s->H.hyp) {
        HIPCHK(hipMemcpy(xyz.data(), s->H.hyp, xyz.size() * sizeof(int), hipMemcpyDeviceToHost));
    } else {
        for (size_t i = 0; i < ne; i++) {
            const int node = s->ev_host[i % nev];
            xyz[3 * i] = node % n[0];
            xyz[3 * i + 1] = node / n[0] % n[1];
            xyz[3 * i + 2] = node / (n[0] * n[1]);
        }
    }
    if (!hypo_all_in("mceik_mcmc_hypo_enable", xyz.data(), ne, nev, o->lo, o->hi)) return 1;
    HypoDev &H = s->H;
    if (!H.hyp) {                      // every array or none: a failed enable leaves the sampler as it was
        HypoDev N;
        memset(&N, 0, sizeof(N));
        unsigned long long *cnt = nullptr;
        if (dput(s, &N.hyp, xyz.data(), xyz.size()) || dalloc(s, &N.ev1, ne) || (nph > 1 && dalloc(s, &N.evall, ne * nph)) ||
            dalloc(s, &N.ev2, 2 * ne * nph) || dalloc(s, &N.ttab2, 2 * ne * nph * D.nstat) || dalloc(s, &N.cand, 3 * ne) ||
            dalloc(s, &N.acc, ne) || dalloc(s, &N.obj, 2 * ne) || dalloc(s, &N.logu, ne) || dalloc(s, &cnt, 2 * (size_t)nev) ||
            dalloc(s, &N.mom, 9 * (size_t)nev))
            return -1;
        N.nx = n[0]; N.ny = n[1]; N.nz = n[2];
        N.attempts = cnt;
        N.accepts = cnt + nev;
        HIPCHK(hypo_lists(D, N, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        H = N;
        s->d_hcnt = cnt;
        // from here on every chain has event lists of its own: a row per model of the batch
        s->fb.ev_node = H.ev1;
        s->fb.ev_stride = nev;
        s->fb_all.ev_node = nph > 1 ? H.evall : H.ev1;
        s->fb_all.ev_stride = nev;
        // a hypocentre step: every current model at [current | candidate], tables of its own
        s->fb_hyp = s->fb_all;
        s->fb_hyp.slow = D.slow_cur;
        s->fb_hyp.ev_node = H.ev2;
        s->fb_hyp.nev = 2 * nev;
        s->fb_hyp.ev_stride = 2 * nev;
        s->fb_hyp.ttab = H.ttab2;
        s->fb_hyp.solve_order = nullptr;
        s->fb_hyp.solve_clock = nullptr;
    }
    HIPCHK(hipMemset(s->d_hcnt, 0, 2 * (size_t)nev * 8));
    HIPCHK(hipMemset(H.mom, 0, 9 * (size_t)nev * 8));
    s->hyp_n = 0;
    H.dmx = o->dmax[0]; H.dmy = o->dmax[1]; H.dmz = o->dmax[2];
    H.lox = o->lo[0]; H.loy = o->lo[1]; H.loz = o->lo[2];
    H.hix = o->hi[0]; H.hiy = o->hi[1]; H.hiz = o->hi[2];
    s->hypo_every = o->every;
    s->hypo_on = true;
    return pipes_refresh(s);
}

extern "C" int mceik_mcmc_hypo_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    s->hypo_on = false;                // host state only: queued steps keep the kernels they were queued with
    return 0;
}

extern "C" int mceik_mcmc_hypo_get(mceik_mcmc *s, mceik_hypo_opts *o, int *xyz)
{
    if (!s || !s->H.hyp) return 1;
    const HypoDev &H = s->H;
    if (o) {
        o->every = s->hypo_on ? s->hypo_every : 0;
        o->dmax[0] = H.dmx; o->dmax[1] = H.dmy; o->dmax[2] = H.dmz;
        o->lo[0] = H.lox; o->lo[1] = H.loy; o->lo[2] = H.loz;
        o->hi[0] = H.hix; o->hi[1] = H.hiy; o->hi[2] = H.hiz;
    }
    if (xyz) {
        DeviceScope dg(s->device);
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipMemcpy(xyz, H.hyp, (size_t)s->D.nchains * s->D.nev * 3 * sizeof(int), hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int mceik_mcmc_hypo_set(mceik_mcmc *s, const int *xyz)
{
    if (!s || !s->H.hyp || !xyz) return 1;
    const HypoDev &H = s->H;
    const size_t ne = (size_t)s->D.nchains * s->D.nev;
    const int glo[3] = {0, 0, 0}, ghi[3] = {H.nx - 1, H.ny - 1, H.nz - 1};
    const int blo[3] = {H.lox, H.loy, H.loz}, bhi[3] = {H.hix, H.hiy, H.hiz};
    if (!hypo_all_in("mceik_mcmc_hypo_set", xyz, ne, s->D.nev, s->hypo_on ? blo : glo, s->hypo_on ? bhi : ghi)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(H.hyp, xyz, ne * 3 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hypo_lists(s->D, H, s->stream));
    return forward_logl(s, "mceik_mcmc_hypo_set");
}

extern "C" int mceik_mcmc_hypo_stats(mceik_mcmc *s, long long *attempts, long long *accepts, int reset)
{
    if (!s || !s->H.hyp) return 1;
    const size_t n = s->D.nev;
    return get_counts(s, s->H.attempts, s->H.accepts, n, attempts, accepts, reset, s->d_hcnt, 2 * n);
}

extern "C" int mceik_mcmc_hypo_last(mceik_mcmc *s, int *cand, unsigned char *accept, double *obj)
{
    if (!s || !s->H.hyp) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t ne = (size_t)s->D.nchains * s->D.nev;
    if (cand) HIPCHK(hipMemcpy(cand, s->H.cand, ne * 3 * sizeof(int), hipMemcpyDeviceToHost));
    if (accept) HIPCHK(hipMemcpy(accept, s->H.acc, ne, hipMemcpyDeviceToHost));
    if (obj) HIPCHK(hipMemcpy(obj, s->H.obj, ne * 2 * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_hypo_moments_get(mceik_mcmc *s, long long *n, long long *sum, long long *sq)
{
    if (!s || !s->H.hyp) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const int nev = s->D.nev;
    std::vector<long long> m((size_t)nev * 9);
    HIPCHK(hipMemcpy(m.data(), s->H.mom, m.size() * 8, hipMemcpyDeviceToHost));
    if (n) *n = s->hyp_n;
    for (int e = 0; e < nev; e++) {
        for (int k = 0; k < 3 && sum; k++) sum[3 * e + k] = m[9 * (size_t)e + k];
        for (int k = 0; k < 6 && sq; k++) sq[6 * e + k] = m[9 * (size_t)e + 3 + k];
    }
    return 0;
}

extern "C" int mceik_mcmc_hypo_moments_set(mceik_mcmc *s, long long n, const long long *sum, const long long *sq)
{
    if (!s || !s->H.hyp || n < 0 || !sum || !sq) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const int nev = s->D.nev;
    std::vector<long long> m((size_t)nev * 9);
    for (int e = 0; e < nev; e++) {
        for (int k = 0; k < 3; k++) m[9 * (size_t)e + k] = sum[3 * e + k];
        for (int k = 0; k < 6; k++) m[9 * (size_t)e + 3 + k] = sq[6 * e + k];
    }
    HIPCHK(hipMemcpy(s->H.mom, m.data(), m.size() * 8, hipMemcpyHostToDevice));
    s->hyp_n = n;
    return 0;
}

extern "C" int mceik_hypo_draw(uint32_t seed, uint32_t gchain, uint64_t step, int e, const int dmax[3], int d[3],
                               double *logu)
{
    if (e < 0 || !dmax || !d || dmax[0] < 0 || dmax[1] < 0 || dmax[2] < 0) return 1;
    const uint32_t r3 = hypo_draw(seed, gchain, step, e, dmax[0], dmax[1], dmax[2], d);
    if (logu) *logu = hypo_det_log_host(((double)r3 + 0.5) * (1.0 / 4294967296.0));
    return 0;
}

// ---------------------------------------------------------------------------
// noise-scale and station-static moves (include/mceik.h mceik_mcmc_nuis_*)

static size_t nuis_npar(const McmcDev &D) { return (size_t)D.nphase + (size_t)D.nphase * D.nstat; }
static size_t nuis_nmom(const McmcDev &D, int nk) { return 2 * (size_t)D.nphase + (size_t)D.nphase * nk + 2 * (size_t)D.nphase * D.nstat; }

// Every ladder index inside [0, nk) and every static inside [-kcmax, kcmax].
static bool nuis_state_ok(const McmcDev &D, const int *kn, const int *kc, int nk, int kcmax)
{
    const size_t nn = (size_t)D.nchains * D.nphase, nc = nn * D.nstat;
    for (size_t i = 0; i < nn; i++) if (kn[i] < 0 || kn[i] >= nk) return false;
    for (size_t i = 0; i < nc; i++) if (kc[i] < -kcmax || kc[i] > kcmax) return false;
    return true;
}

extern "C" int mceik_mcmc_nuis_enable(mceik_mcmc *s, const mceik_nuis_opts *o)
{
    if (!s || !o) return 1;
    McmcDev &D = s->D;
    const int nph = D.nphase, nst = D.nstat, nch = D.nchains, nobs = (int)s->h_ostat.size();
    const bool noise = o->noise != 0, statics = o->statics != 0;
    if (!noise && !statics) return 1;
    if (o->every <= 0 || o->offset < 0 || o->offset >= o->every || o->nsub <= 0) return 1;
    if (o->dk < 0 || o->dc < 0 || o->kcmax < 0 || o->dc > 0x3fffffff || o->kcmax > 0x3fffffff) return 1;
    if (statics && !(o->dt > 0.0 && o->dt <= DBL_MAX)) return 1;
    // the ladder: an odd number of entries, the middle one the start value (1, 0) exactly; statics alone need none
    static const double one = 1.0, zero = 0.0;
    const bool own = !noise && !o->lam && !o->lnlam;
    const int nk = own ? 1 : o->nk;
    const double *lam = own ? &one : o->lam, *lnlam = own ? &zero : o->lnlam;
    if (nk < 1 || nk % 2 == 0 || !lam || !lnlam || lam[nk / 2] != 1.0 || lnlam[nk / 2] != 0.0) return 1;
    for (int k = 0; k < nk; k++)
        if (!(lam[k] > 0.0 && lam[k] <= DBL_MAX) || !(fabs(lnlam[k]) <= DBL_MAX)) return 1;
    // the stations statics moves draw from: those with a used pick of the phase, in station order
    std::vector<int> act((size_t)nph * nst, 0);
    int nact[2] = {0, 0};
    double norm[2] = {0.0, 0.0};
    {
        std::vector<unsigned char> has((size_t)nph * nst, 0);
        for (int j = 0; j < nobs; j++)
            if (!s->h_omask[j]) {
                has[(size_t)s->h_ophase[j] * nst + s->h_ostat[j]] = 1;
                norm[s->h_ophase[j]] += 1.0;
            }
        for (int ph = 0; ph < nph; ph++)
            for (int k = 0; k < nst; k++)
                if (has[(size_t)ph * nst + k]) act[(size_t)ph * nst + nact[ph]++] = k;
    }
    for (int ph = 0; ph < 2; ph++) {
        if (!statics || nact[ph] < 2) nact[ph] = 0;         // a pair needs two stations
        if (o->norm && ph < nph) norm[ph] = o->norm[ph];
        if (!(fabs(norm[ph]) <= DBL_MAX)) return 1;
    }
    if ((noise ? nph : 0) + nact[0] + nact[1] == 0) return 1;
    if (post_holds_states(s)) return 1;
    // MCEIK_NUIS_LDS (test hook): fewer bytes of LDS for a nuisance step's block, so that small problems take
    // the path without the staged travel times
    size_t lds_max = MCEIK_NUIS_LDS_MAX;
    if (const char *lds_env = getenv("MCEIK_NUIS_LDS")) lds_max = std::min<size_t>(lds_max, strtoul(lds_env, nullptr, 10));
    NuisDev T;
    memset(&T, 0, sizeof(T));
    T.nobs = nobs;
    if (nuis_lds_bytes(D, T, false) > lds_max) {
        fprintf(stderr, "mceik_mcmc_nuis_enable: 8 nev + 4 nphase nstat = %zu B exceed the %zu B of LDS a nuisance step "
                        "uses\n", nuis_lds_bytes(D, T, false), lds_max);
        return 1;
    }
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nn = (size_t)nch * nph, nc = nn * nst;
    if (s->N.kn) {
        // state is held: its indices keep their meaning on a ladder of the same length only, its statics in the new box
        std::vector<int> kn(nn), kc(nc);
        HIPCHK(hipMemcpy(kn.data(), s->N.kn, nn * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(kc.data(), s->N.kc, nc * sizeof(int), hipMemcpyDeviceToHost));
        if (nk != s->N.nk || !nuis_state_ok(D, kn.data(), kc.data(), nk, statics ? o->kcmax : 0x3fffffff)) return 1;
    }
    NuisDev &B = s->Nbuf;
    if (!B.kn) {                       // every array or none: a failed enable leaves the sampler as it was
        NuisDev A;
        memset(&A, 0, sizeof(A));
        unsigned long long *cnt = nullptr;
        int *dact = nullptr;
        float *tc1 = s->ttab_cur1;     // (shared with the data-fit sums: whichever needed them first made them)
        if (dalloc(s, &A.kn, nn) || dalloc(s, &A.kc, nc) || dalloc(s, &A.var_eff, (size_t)nch * nobs) ||
            dalloc(s, &A.tcorr_eff, (size_t)nch * nobs) || dalloc(s, &cnt, 2 * nuis_npar(D)) || dalloc(s, &dact, (size_t)nph * nst) ||
            (nph == 1 && !tc1 && dalloc(s, &tc1, (size_t)nch * nst * D.nev)))
            return -1;
        A.attempts = cnt;
        A.accepts = cnt + nuis_npar(D);
        A.act = dact;
        A.var0 = D.var;
        A.tcorr0 = D.tcorr;
        A.nobs = nobs;
        B = A;
        s->ttab_cur1 = tc1;
    }
    if (o->nsub > s->nuis_cap_sub) {
        int *rec = nullptr;
        double *rl = nullptr;
        if (dalloc(s, &rec, 4 * (size_t)nch * o->nsub) || dalloc(s, &rl, 2 * (size_t)nch * o->nsub)) return -1;
        B.rec = rec;
        B.rlogl = rl;
        s->nuis_cap_sub = o->nsub;
    }
    if (nk > s->nuis_cap_nk) {
        double *tab = nullptr;
        long long *mom = nullptr;
        if (dalloc(s, &tab, 2 * (size_t)nk) || dalloc(s, &mom, nuis_nmom(D, nk))) return -1;
        B.lam = tab;
        B.lnlam = tab + nk;
        B.mom = mom;
        s->nuis_cap_nk = nk;
    }
    HIPCHK(hipMemcpy((void *)B.lam, lam, (size_t)nk * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((void *)B.lnlam, lnlam, (size_t)nk * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((void *)B.act, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(B.attempts, 0, 2 * nuis_npar(D) * 8));
    HIPCHK(hipMemset(B.mom, 0, nuis_nmom(D, nk) * 8));
    HIPCHK(hipMemset(B.rec, 0, 4 * (size_t)nch * o->nsub * sizeof(int)));
    HIPCHK(hipMemset(B.rlogl, 0, 2 * (size_t)nch * o->nsub * 8));
    if (!s->N.kn) {                    // the start values: the ladder's middle entry, no static
        std::vector<int> kn(nn, nk / 2);
        HIPCHK(hipMemcpy(B.kn, kn.data(), nn * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(B.kc, 0, nc * sizeof(int)));
    }
    B.nk = nk; B.dk = o->dk; B.dc = o->dc; B.nsub = o->nsub;
    B.noise_on = noise; B.statics_on = statics;
    B.lds_te = nuis_lds_bytes(D, B, true) <= lds_max;
    B.nact0 = nact[0]; B.nact1 = nact[1];
    if (statics) { B.kcmax = o->kcmax; B.dt = o->dt; }
    else if (!s->N.kn) { B.kcmax = 0; B.dt = 0.0; }        // (statics held from an earlier enable keep their dt)
    B.norm0 = norm[0]; B.norm1 = norm[1];
    s->N = B;
    s->nuis_n = 0;
    s->nuis_every = o->every;
    s->nuis_offset = o->offset;
    s->nuis_on = true;
    if (nph == 1) {                    // a one-model sampler keeps its current tables while the state is held
        D.ttab_cur = s->ttab_cur1;
        s->fb_all.ttab = s->ttab_cur1;
    }
    if (pipes_refresh(s)) return -1;
    HIPCHK(nuis_rows(D, s->N, s->stream));
    return forward_logl(s, "mceik_mcmc_nuis_enable");       // fills the current tables; logL with the state
}

extern "C" int mceik_mcmc_nuis_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    s->nuis_on = false;                // host state only: the values stay and every logL keeps honouring them
    return 0;
}

extern "C" int mceik_mcmc_nuis_clear(mceik_mcmc *s)
{
    if (!s) return 1;
    if (!s->N.kn) return 0;
    if (post_holds_states(s)) return 1;
    for (const KeptStream &k : s->kept)
        if (k.on && k.holds_nuis && k.holds_nuis(k.state)) return 1;   // a registered probe reads the values
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->nuis_on = false;
    memset(&s->N, 0, sizeof(s->N));
    if (s->D.nphase == 1 && !kept_needs_tables1(s)) {       // (the data-fit sums keep reading the current tables)
        s->D.ttab_cur = nullptr;
        s->fb_all.ttab = s->fb.ttab;
    }
    if (pipes_refresh(s)) return -1;
    return forward_logl(s, "mceik_mcmc_nuis_clear");
}

extern "C" int mceik_mcmc_nuis_get(mceik_mcmc *s, mceik_nuis_opts *o, double *lam, double *lnlam, double *norm, int *kn,
                                   int *kc)
{
    if (!s || !s->N.kn) return 1;
    const NuisDev &N = s->N;
    const McmcDev &D = s->D;
    if (o) {
        memset(o, 0, sizeof(*o));
        o->every = s->nuis_on ? s->nuis_every : 0;
        o->offset = s->nuis_offset; o->nsub = N.nsub;
        o->noise = N.noise_on; o->statics = N.statics_on;
        o->nk = N.nk; o->dk = N.dk; o->dc = N.dc; o->kcmax = N.kcmax; o->dt = N.dt;
    }
    if (norm) {
        norm[0] = N.norm0;
        if (D.nphase > 1) norm[1] = N.norm1;
    }
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nn = (size_t)D.nchains * D.nphase;
    if (lam) HIPCHK(hipMemcpy(lam, N.lam, (size_t)N.nk * 8, hipMemcpyDeviceToHost));
    if (lnlam) HIPCHK(hipMemcpy(lnlam, N.lnlam, (size_t)N.nk * 8, hipMemcpyDeviceToHost));
    if (kn) HIPCHK(hipMemcpy(kn, N.kn, nn * sizeof(int), hipMemcpyDeviceToHost));
    if (kc) HIPCHK(hipMemcpy(kc, N.kc, nn * D.nstat * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_nuis_set(mceik_mcmc *s, const int *kn, const int *kc)
{
    if (!s || !s->N.kn || !kn || !kc) return 1;
    const NuisDev &N = s->N;
    const McmcDev &D = s->D;
    if (!nuis_state_ok(D, kn, kc, N.nk, N.kcmax)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nn = (size_t)D.nchains * D.nphase;
    HIPCHK(hipMemcpy(N.kn, kn, nn * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(N.kc, kc, nn * D.nstat * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(nuis_rows(D, N, s->stream));
    HIPCHK(mcmc_init_loglik(D, N, s->stream));          // from the kept current tables: no solve
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int mceik_mcmc_nuis_stats(mceik_mcmc *s, long long *attempts, long long *accepts, int reset)
{
    if (!s || !s->N.kn) return 1;
    const size_t n = nuis_npar(s->D);
    return get_counts(s, s->N.attempts, s->N.accepts, n, attempts, accepts, reset, s->N.attempts, 2 * n);
}

extern "C" int mceik_mcmc_nuis_last(mceik_mcmc *s, int *rec, double *logl)
{
    if (!s || !s->N.kn) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t n = (size_t)s->D.nchains * s->N.nsub;
    if (rec) HIPCHK(hipMemcpy(rec, s->N.rec, 4 * n * sizeof(int), hipMemcpyDeviceToHost));
    if (logl) HIPCHK(hipMemcpy(logl, s->N.rlogl, 2 * n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_nuis_moments_get(mceik_mcmc *s, long long *n, long long *ksum, long long *hist, long long *csum)
{
    if (!s || !s->N.kn) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const McmcDev &D = s->D;
    const size_t a = 2 * (size_t)D.nphase, b = (size_t)D.nphase * s->N.nk, c = 2 * (size_t)D.nphase * D.nstat;
    if (n) *n = s->nuis_n;
    if (ksum) HIPCHK(hipMemcpy(ksum, s->N.mom, a * 8, hipMemcpyDeviceToHost));
    if (hist) HIPCHK(hipMemcpy(hist, s->N.mom + a, b * 8, hipMemcpyDeviceToHost));
    if (csum) HIPCHK(hipMemcpy(csum, s->N.mom + a + b, c * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_nuis_moments_set(mceik_mcmc *s, long long n, const long long *ksum, const long long *hist,
                                           const long long *csum)
{
    if (!s || !s->N.kn || n < 0 || !ksum || !hist || !csum) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const McmcDev &D = s->D;
    const size_t a = 2 * (size_t)D.nphase, b = (size_t)D.nphase * s->N.nk, c = 2 * (size_t)D.nphase * D.nstat;
    HIPCHK(hipMemcpy(s->N.mom, ksum, a * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->N.mom + a, hist, b * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->N.mom + a + b, csum, c * 8, hipMemcpyHostToDevice));
    s->nuis_n = n;
    return 0;
}

extern "C" int mceik_nuis_draw(uint32_t seed, uint32_t gchain, uint64_t step, int sub, int nnoise, int nact0, int nact1,
                               int dk, int dc, int m[5], double *logu)
{
    if (sub < 0 || !m || nnoise < 0 || nnoise > 2 || nact0 < 0 || nact1 < 0 || nact0 == 1 || nact1 == 1 || dk < 0 ||
        dc < 0 || dc > 0x3fffffff || (long long)nnoise + nact0 + nact1 < 1 || (long long)nnoise + nact0 + nact1 > INT_MAX)
        return 1;
    const uint32_t r3 = nuis_draw(seed, gchain, step, sub, nnoise, nact0, nact1, dk, dc, m);
    if (logu) *logu = hypo_det_log_host(((double)r3 + 0.5) * (1.0 / 4294967296.0));
    return 0;
}

// ---------------------------------------------------------------------------
// discrete Langevin moves (include/mceik.h mceik_mcmc_lang_*)

static void lang_pipes_free(mceik_mcmc *s)
{
    for (LangPipe &lp : s->lang_pipe) {
        if (lp.base) hipFree(lp.base);
        memset(&lp, 0, sizeof(lp));
    }
}

extern "C" int mceik_mcmc_lang_enable(mceik_mcmc *s, const mceik_lang_opts *o)
{
    if (!s || !o) return 1;
    if (vor_refuses(s, "mceik_mcmc_lang_enable")) return 1;
    if (s->D.l1) {
        fprintf(stderr, "mceik_mcmc_lang_enable: the L1 likelihood is on (mceik_mcmc_likelihood_set): the gradient of "
                        "its piecewise-linear objective is not provided\n");
        return 1;
    }
    if (o->every <= 0 || o->offset < 0 || o->offset >= o->every || !(o->sigma > 0.0 && o->sigma <= DBL_MAX) ||
        o->dmax < 1 || o->dmax > MCEIK_LANG_DMAX)
        return 1;
    const double c = 1.0 / (2.0 * o->sigma * o->sigma);
    if (!(c > 0.0 && c <= DBL_MAX)) return 1;
    const McmcDev &D = s->D;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    // the chunk of every pipe: the most chains whose fields, workspaces and pick weights fit its share of the budget
    const size_t mem = o->mem_bytes ? o->mem_bytes : (size_t)1 << 31, share = mem / s->npipe;
    int chunk[MCEIK_MAX_PIPES] = {0};
    size_t need[MCEIK_MAX_PIPES][6];
    for (int k = 0; k < s->npipe; k++) {
        int m = s->pipe[k].D.nchains;
        for (; m >= 1; m--) {
            size_t *q = need[k];
            q[5] = lang_pipe_bytes(s, k, m, &q[0], &q[1], &q[2], &q[3], &q[4]);
            if (q[5] <= share) break;
        }
        if (m < 1) {
            fprintf(stderr, "mceik_mcmc_lang_enable: mem_bytes = %zu holds no chain of pipe %d (one needs %zu B)\n", mem,
                    k, need[k][5]);
            return 1;
        }
        chunk[k] = m;
    }
    LangDev &L = s->L;
    const size_t nch = D.nchains, ns = nch * D.nstat;
    if (!L.delta) {                    // every array or none: a failed enable leaves the sampler as it was
        LangDev A;
        memset(&A, 0, sizeof(A));
        if (dalloc(s, &A.delta, nch * D.ncell) || dalloc(s, &A.vprop, nch * D.ncm) || dalloc(s, &A.g0, nch * D.ncell) ||
            dalloc(s, &A.g1, nch * D.ncell) || dalloc(s, &A.lq, 3 * nch) || dalloc(s, &A.nmove, nch) ||
            dalloc(s, &A.status, nch) || dalloc(s, &A.tt0, ns * D.nev) || dalloc(s, &A.ierr0, ns) ||
            dalloc(s, &A.ierr1, ns) || dalloc(s, &A.ast0, ns) || dalloc(s, &A.ast1, ns) || dalloc(s, &A.niter, ns) ||
            dalloc(s, &A.pen, 4 * nch * D.nphase) || dalloc(s, &A.cnt, 4 * nch))
            return -1;
        A.pen_stride = nch * D.nphase;
        A.skip = s->fb.skip;
        L = A;
    }
    lang_pipes_free(s);
    for (int k = 0; k < s->npipe; k++) {
        LangPipe &lp = s->lang_pipe[k];
        const size_t *q = need[k];
        if (hipMalloc(&lp.base, q[5]) != hipSuccess) {
            (void)hipGetLastError();
            lp.base = nullptr;
            lang_pipes_free(s);
            s->lang_on = false;
            fprintf(stderr, "mceik_mcmc_lang_enable: cannot allocate %zu B for pipe %d\n", q[5], k);
            return -1;
        }
        char *b = (char *)lp.base;
        lp.u = b; lp.fws = b + q[0]; lp.aws = b + q[0] + q[1]; lp.ev_w = (double *)(b + q[0] + q[1] + q[2]);
        lp.gsolve = (double *)(b + q[0] + q[1] + q[2] + q[3]);
        lp.fws_bytes = q[1]; lp.aws_bytes = q[2];
        lp.chunk = chunk[k];
    }
    HIPCHK(hipMemset(L.cnt, 0, 4 * nch * 8));
    L.c = c;
    L.dmax = o->dmax;
    s->lang_every = o->every;
    s->lang_offset = o->offset;
    s->lang_sigma = o->sigma;
    s->lang_mem = mem;
    s->lang_on = true;
    return pipes_refresh(s);
}

extern "C" int mceik_mcmc_lang_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    s->lang_on = false;                // host state only: queued steps keep the kernels they were queued with
    return 0;
}

extern "C" int mceik_mcmc_lang_get(mceik_mcmc *s, mceik_lang_opts *o, int *chunk)
{
    if (!s || !s->L.delta) return 1;
    if (o) {
        o->every = s->lang_on ? s->lang_every : 0;
        o->offset = s->lang_offset;
        o->sigma = s->lang_sigma;
        o->dmax = s->L.dmax;
        o->mem_bytes = s->lang_mem;
    }
    for (int k = 0; k < s->npipe && chunk; k++) chunk[k] = s->lang_pipe[k].chunk;
    return 0;
}

extern "C" int mceik_mcmc_lang_stats(mceik_mcmc *s, long long *attempts, long long *accepts, long long *failed,
                                     long long *moved, int reset)
{
    if (!s || !s->L.delta) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nch = s->D.nchains;
    std::vector<unsigned long long> cnt(4 * nch);
    HIPCHK(hipMemcpy(cnt.data(), s->L.cnt, cnt.size() * 8, hipMemcpyDeviceToHost));
    long long t[4] = {0, 0, 0, 0};
    for (size_t c = 0; c < nch; c++)
        for (int q = 0; q < 4; q++) t[q] += (long long)cnt[4 * c + q];
    if (attempts) *attempts = t[0];
    if (accepts) *accepts = t[1];
    if (failed) *failed = t[2];
    if (moved) *moved = t[3];
    if (reset) HIPCHK(hipMemset(s->L.cnt, 0, cnt.size() * 8));
    return 0;
}

extern "C" int mceik_mcmc_lang_last(mceik_mcmc *s, int *phase, int *delta, double *lqf, double *lqr, double *logl_prop,
                                    unsigned char *accept, int *status)
{
    if (!s || !s->L.delta) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nch = s->D.nchains;
    if (phase) HIPCHK(hipMemcpy(phase, s->D.prop_phase, nch * sizeof(int), hipMemcpyDeviceToHost));
    if (delta) HIPCHK(hipMemcpy(delta, s->L.delta, nch * s->D.ncell * sizeof(int), hipMemcpyDeviceToHost));
    if (lqf || lqr || logl_prop) {
        std::vector<double> lq(3 * nch);
        HIPCHK(hipMemcpy(lq.data(), s->L.lq, lq.size() * 8, hipMemcpyDeviceToHost));
        for (size_t c = 0; c < nch; c++) {
            if (lqf) lqf[c] = lq[3 * c];
            if (lqr) lqr[c] = lq[3 * c + 1];
            if (logl_prop) logl_prop[c] = lq[3 * c + 2];
        }
    }
    if (accept) HIPCHK(hipMemcpy(accept, s->D.accept, nch, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, s->L.status, nch * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" double mceik_det_exp(double x) { return mcmcd::det_exp(x); }

extern "C" int mceik_lang_cell(uint32_t seed, uint32_t gchain, uint64_t step, int cell, double d, int v, int vlo, int vhi,
                               double sigma, int dmax, int *delta, int *lo, int *hi, double *logq)
{
    if (cell < 0 || !(sigma > 0.0 && sigma <= DBL_MAX) || dmax < 1 || dmax > MCEIK_LANG_DMAX || v < vlo || v > vhi)
        return 1;
    const double c = 1.0 / (2.0 * sigma * sigma);
    uint32_t r[4];
    const double u = lang_uniform(seed, gchain, step, (uint32_t)cell, r);
    const LangCell S = lang_cell(d, v, vlo, vhi, c, dmax);
    if (delta) *delta = lang_pick(S, u);
    if (lo) *lo = S.lo;
    if (hi) *hi = S.hi;
    for (int k = S.lo; k <= S.hi && logq; k++) logq[k - S.lo] = lang_logq(S, k);
    return 0;
}

// ---------------------------------------------------------------------------
// differential-evolution moves (include/mceik.h mceik_mcmc_de_*)

int de_lists(mceik_mcmc *s)
{
    if (!s->De.a) return 0;
    const int nch = s->D.nchains, G = temper_cold(s);
    for (int par = 0; par < 2; par++) {
        s->de_mov[par].clear();
        for (int c = 0; c < nch; c++)
            if (((c % G) & 1) == par) s->de_mov[par].push_back(c);
    }
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    for (int par = 0; par < 2; par++)
        if (!s->de_mov[par].empty())
            HIPCHK(hipMemcpy(s->d_demov + (size_t)par * nch, s->de_mov[par].data(), s->de_mov[par].size() * sizeof(int),
                             hipMemcpyHostToDevice));
    s->De.G = G;
    return pipes_refresh(s);
}

extern "C" int mceik_mcmc_de_enable(mceik_mcmc *s, const mceik_de_opts *o)
{
    if (!s || !o) return 1;
    if (vor_refuses(s, "mceik_mcmc_de_enable")) return 1;
    if (o->every < 1 || o->offset < 0 || o->offset >= o->every) {
        fprintf(stderr, "mceik_mcmc_de_enable: every >= 1 and 0 <= offset < every\n");
        return 1;
    }
    if (o->gamma_q16 < 1 || o->gamma_q16 > MCEIK_DE_GQ_MAX || o->cr_q16 < 1 || o->cr_q16 > MCEIK_DE_CRQ_MAX) {
        fprintf(stderr, "mceik_mcmc_de_enable: 1 <= gamma_q16 <= %d and 1 <= cr_q16 <= %d\n", MCEIK_DE_GQ_MAX,
                MCEIK_DE_CRQ_MAX);
        return 1;
    }
    if (temper_cold(s) < 4) {
        fprintf(stderr, "mceik_mcmc_de_enable: a population (the chains of one temperature rung) has %d chains; a "
                        "partner set needs two, so a population needs 4\n", temper_cold(s));
        return 1;
    }
    const McmcDev &D = s->D;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    DeDev &L = s->De;
    const size_t nch = D.nchains, ns = nch * D.nstat;
    if (!L.a) {                        // every array or none: a failed enable leaves the sampler as it was
        DeDev A;
        memset(&A, 0, sizeof(A));
        int *mov = nullptr;
        if (dalloc(s, &A.a, nch) || dalloc(s, &A.b, nch) || dalloc(s, &A.inbox, nch) || dalloc(s, &A.nmove, nch) ||
            dalloc(s, &A.status, nch) || dalloc(s, &A.logl_prop, nch) || dalloc(s, &A.vprop, nch * D.ncm) ||
            dalloc(s, &A.pen, 4 * nch * D.nphase) || dalloc(s, &A.cnt, 5 * nch) || dalloc(s, &A.slow, nch * D.ncell) ||
            dalloc(s, &A.ttab, ns * D.nev) || dalloc(s, &A.ierr, ns) || dalloc(s, &A.niter, ns) ||
            dalloc(s, &A.ev, nch * D.nev) || dalloc(s, &mov, 2 * nch))
            return -1;
        A.pen_stride = nch * D.nphase;
        A.skip = s->fb.skip;
        A.vall = D.v;
        L = A;
        s->d_demov = mov;
        s->de_last_ph = -1;
    }
    HIPCHK(hipMemset(L.cnt, 0, 5 * nch * 8));
    L.gq = o->gamma_q16;
    L.crq = o->cr_q16;
    s->de_every = o->every;
    s->de_offset = o->offset;
    s->de_on = true;
    return de_lists(s);
}

extern "C" int mceik_mcmc_de_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    s->de_on = false;                  // host state only: queued steps keep the kernels they were queued with
    return 0;
}

extern "C" int mceik_mcmc_de_get(mceik_mcmc *s, mceik_de_opts *o)
{
    if (!s || !s->De.a) return 1;
    if (o) {
        o->every = s->de_on ? s->de_every : 0;
        o->offset = s->de_offset;
        o->gamma_q16 = s->De.gq;
        o->cr_q16 = s->De.crq;
    }
    return 0;
}

extern "C" int mceik_mcmc_de_stats(mceik_mcmc *s, long long *attempts, long long *accepts, long long *outbox,
                                   long long *failed, long long *moved, int reset)
{
    if (!s || !s->De.a) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nch = s->D.nchains;
    std::vector<unsigned long long> cnt(5 * nch);
    HIPCHK(hipMemcpy(cnt.data(), s->De.cnt, cnt.size() * 8, hipMemcpyDeviceToHost));
    long long t[5] = {0, 0, 0, 0, 0};
    for (size_t c = 0; c < nch; c++)
        for (int q = 0; q < 5; q++) t[q] += (long long)cnt[5 * c + q];
    if (attempts) *attempts = t[0];
    if (accepts) *accepts = t[1];
    if (outbox) *outbox = t[2];
    if (failed) *failed = t[3];
    if (moved) *moved = t[4];
    if (reset) HIPCHK(hipMemset(s->De.cnt, 0, cnt.size() * 8));
    return 0;
}

extern "C" int mceik_mcmc_de_last(mceik_mcmc *s, int *mover, int *a, int *b, int *phase, int *nmove, int *inbox,
                                  int *status, double *logl_prop, unsigned char *accept)
{
    if (!s || !s->De.a) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nch = s->D.nchains;
    const DeDev &L = s->De;
    std::vector<int> ha(nch);
    HIPCHK(hipMemcpy(ha.data(), L.a, nch * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < nch && mover; c++) mover[c] = s->de_last_ph >= 0 && ha[c] >= 0;
    if (a) memcpy(a, ha.data(), nch * sizeof(int));
    if (b) HIPCHK(hipMemcpy(b, L.b, nch * sizeof(int), hipMemcpyDeviceToHost));
    if (phase) *phase = s->de_last_ph;
    if (nmove) HIPCHK(hipMemcpy(nmove, L.nmove, nch * sizeof(int), hipMemcpyDeviceToHost));
    if (inbox) HIPCHK(hipMemcpy(inbox, L.inbox, nch * sizeof(int), hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, L.status, nch * sizeof(int), hipMemcpyDeviceToHost));
    if (logl_prop) HIPCHK(hipMemcpy(logl_prop, L.logl_prop, nch * 8, hipMemcpyDeviceToHost));
    if (accept) HIPCHK(hipMemcpy(accept, s->D.accept, nch, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_de_delta(int gq, int d, uint32_t word, int crq, int *delta)
{
    if (gq < 1 || gq > MCEIK_DE_GQ_MAX || crq < 1 || crq > MCEIK_DE_CRQ_MAX || !delta) return 1;
    const long long x = de_delta(gq, (long long)d, word, crq);
    if (x < INT_MIN || x > INT_MAX) return 1;
    *delta = (int)x;
    return 0;
}

extern "C" int mceik_de_draw(uint32_t seed, uint32_t gchain, uint64_t step, int nb, int *i, int *j, double *logu)
{
    if (nb < 2) return 1;
    int a, b;
    const uint32_t r3 = de_draw(seed, gchain, step, nb, &a, &b);
    if (i) *i = a;
    if (j) *j = b;
    if (logu) *logu = hypo_det_log_host(((double)r3 + 0.5) * (1.0 / 4294967296.0));
    return 0;
}

// ---------------------------------------------------------------------------
// Voronoi-cell models (include/mceik.h mceik_mcmc_vor_*)

// Nuclei lists [nchains][nphase][kmax] with counts [nchains][nphase]: counts in
// [kmin, kmax], cells distinct and on the grid, values in the phase's box.
static int vor_check(const mceik_mcmc *s, const char *who, int kmin, int kmax, const int *cells, const int *vals,
                     const int *counts)
{
    const McmcDev &D = s->D;
    std::vector<int> sorted;
    for (int r = 0; r < D.nchains * D.nphase; r++) {
        const int ph = r % D.nphase, k = counts[r];
        const int lo = ph ? D.vsmin : D.vmin, hi = ph ? D.vsmax : D.vmax;
        if (k < kmin || k > kmax) {
            fprintf(stderr, "%s: chain %d phase %d has %d nuclei outside [%d, %d]\n", who, r / D.nphase, ph, k, kmin, kmax);
            return 1;
        }
        const int *c = cells + (size_t)r * kmax, *w = vals + (size_t)r * kmax;
        for (int j = 0; j < k; j++)
            if (c[j] < 0 || c[j] >= D.ncell || w[j] < lo || w[j] > hi) {
                fprintf(stderr, "%s: chain %d phase %d nucleus %d: cell %d outside [0, %d) or value %d outside [%d, %d]\n",
                        who, r / D.nphase, ph, j, c[j], D.ncell, w[j], lo, hi);
                return 1;
            }
        sorted.assign(c, c + k);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
            fprintf(stderr, "%s: chain %d phase %d has two nuclei in one cell\n", who, r / D.nphase, ph);
            return 1;
        }
    }
    return 0;
}

// The nuclei to the device, every chain's v, slow_cur and slow_prop from their
// raster and, with recompute, logL from one full forward.  Synchronises.
static int vor_load(mceik_mcmc *s, const char *who, const int *cells, const int *vals, const int *counts, bool recompute)
{
    const McmcDev &D = s->D;
    const VorDev &L = s->V;
    const size_t nr = (size_t)D.nchains * D.nphase;
    HIPCHK(hipMemcpy(L.cell, cells, nr * L.kmax * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.val, vals, nr * L.kmax * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.cnt_k, counts, nr * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(vor_raster(L, D.ncell, (int)nr, L.cell, L.val, L.cnt_k, D.v, (size_t)D.ncell, D.slow_cur, D.slow_prop,
                      (size_t)D.ncell, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (recompute) return forward_logl(s, who);
    return 0;
}

extern "C" int mceik_mcmc_vor_enable(mceik_mcmc *s, const mceik_vor_opts *o, const int *cells, const int *vals,
                                     const int *counts)
{
    if (!s || !o) return 1;
    const char *who = "mceik_mcmc_vor_enable";
    const McmcDev &D = s->D;
    if ((cells || vals || counts) && !(cells && vals && counts)) return 1;
    if (o->kmin < 1 || o->kmax < o->kmin || o->kmax > MCEIK_VOR_KMAX || o->kmax > D.ncell || o->dv < 1 ||
        (!cells && (o->k0 < o->kmin || o->k0 > o->kmax))) {
        fprintf(stderr, "%s: 1 <= kmin <= k0 <= kmax <= min(%d, ncell) and dv >= 1\n", who, MCEIK_VOR_KMAX);
        return 1;
    }
    for (int a = 0; a < 3; a++)
        if (o->dmax[a] < 0 || o->dmax[a] > 32767 || o->metric[a] < 1 || o->metric[a] > 32767) {
            fprintf(stderr, "%s: 0 <= dmax <= 32767 and 1 <= metric <= 32767 per axis\n", who);
            return 1;
        }
    if (o->dmax[0] + o->dmax[1] + o->dmax[2] == 0) {
        fprintf(stderr, "%s: dmax is zero on every axis: no nucleus could move\n", who);
        return 1;
    }
    if (vor_d2max(s->B.ncx, s->B.ncy, s->B.ncz, o->metric[0], o->metric[1], o->metric[2]) < 0) {
        fprintf(stderr, "%s: the largest squared distance of this grid under this metric does not fit 31 bits\n", who);
        return 1;
    }
    if (s->block_on || s->prior_on || s->lang_on || s->de_on) {
        fprintf(stderr, "%s: %s on: they change single cells of v, which would no longer be the raster of the nuclei\n",
                who, s->block_on ? "block proposals are" : s->prior_on ? "the smoothness prior is" :
                     s->lang_on ? "Langevin moves are" : "DE moves are");
        return 1;
    }
    if (cells && vor_check(s, who, o->kmin, o->kmax, cells, vals, counts)) return 1;
    if (post_holds_states(s)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nch = D.nchains, nr = nch * D.nphase, cap = MCEIK_VOR_KMAX;
    if (!s->V.cell) {                  // every array or none: a failed enable leaves the sampler as it was
        VorDev A;
        memset(&A, 0, sizeof(A));
        if (dalloc(s, &A.cell, nr * cap) || dalloc(s, &A.val, nr * cap) || dalloc(s, &A.cnt_k, nr) ||
            dalloc(s, &A.pcell, nch * cap) || dalloc(s, &A.pval, nch * cap) || dalloc(s, &A.pk, nch) ||
            dalloc(s, &A.rec, nch * VOR_NREC) || dalloc(s, &A.logl_prop, nch) || dalloc(s, &A.vprop, nch * D.ncell) ||
            dalloc(s, &A.cnt, nch * 4 * VOR_NCNT) || dalloc(s, &A.hist, (size_t)D.nphase * (cap + 1)) ||
            dalloc(s, &A.dens, (size_t)D.nphase * D.ncell))
            return -1;
        s->V = A;
    }
    // the start nuclei: the caller's, or k0 drawn per chain and phase, each at the chain's current v of its cell
    std::vector<int> hc(nr * o->kmax, 0), hw(nr * o->kmax, 0), hk(nr, o->k0);
    if (cells) {
        memcpy(hc.data(), cells, hc.size() * sizeof(int));
        memcpy(hw.data(), vals, hw.size() * sizeof(int));
        memcpy(hk.data(), counts, hk.size() * sizeof(int));
    } else {
        std::vector<int> v(nch * D.ncm);
        HIPCHK(hipMemcpy(v.data(), D.v, v.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < nr; r++) {
            const uint32_t g = (uint32_t)(D.chain_offset + (int)(r / D.nphase));
            int *c = hc.data() + r * o->kmax, *w = hw.data() + r * o->kmax;
            for (int i = 0; i < o->k0; i++) {
                uint32_t q[4];
                vor_philox(D.seed, g, (uint32_t)i, (uint32_t)(r % D.nphase), 0xFFFFFFFFu, q);
                c[i] = vor_free_cell(c, i, vor_idx(q[0], D.ncell - i));
                w[i] = v[r * D.ncell + c[i]];
            }
        }
    }
    VorDev &L = s->V;
    const bool resized = L.kmax != o->kmax;
    L.kmin = o->kmin; L.kmax = o->kmax; L.dv = o->dv;
    L.dmx = o->dmax[0]; L.dmy = o->dmax[1]; L.dmz = o->dmax[2];
    L.mx = o->metric[0]; L.my = o->metric[1]; L.mz = o->metric[2];
    L.ncx = s->B.ncx; L.ncy = s->B.ncy; L.ncz = s->B.ncz;
    HIPCHK(hipMemset(L.cnt, 0, nch * 4 * VOR_NCNT * 8));
    if (resized) {                     // the histogram's rows have another length: the moments start over
        HIPCHK(hipMemset(L.hist, 0, (size_t)D.nphase * (cap + 1) * 8));
        HIPCHK(hipMemset(L.dens, 0, (size_t)D.nphase * D.ncell * 8));
        s->vor_n = 0;
    }
    s->vor_k0 = cells ? 0 : o->k0;
    s->vor_last_ph = -1;
    s->vor_on = true;
    if (pipes_refresh(s)) return -1;
    return vor_load(s, who, hc.data(), hw.data(), hk.data(), true);
}

extern "C" int mceik_mcmc_vor_disable(mceik_mcmc *s)
{
    if (!s) return 1;
    if (!s->vor_on) return 0;
    if (post_holds_states(s)) return 1;
    s->vor_on = false;                 // host state only: v stays the last raster, an ordinary cell model
    return 0;
}

extern "C" int mceik_mcmc_vor_get(mceik_mcmc *s, mceik_vor_opts *o, int *on, int *cells, int *vals, int *counts)
{
    if (!s || !s->V.cell) return 1;
    const VorDev &L = s->V;
    if (o) {
        o->kmin = L.kmin; o->kmax = L.kmax; o->k0 = s->vor_k0; o->dv = L.dv;
        o->dmax[0] = L.dmx; o->dmax[1] = L.dmy; o->dmax[2] = L.dmz;
        o->metric[0] = L.mx; o->metric[1] = L.my; o->metric[2] = L.mz;
    }
    if (on) *on = s->vor_on ? 1 : 0;
    if (!cells && !vals && !counts) return 0;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nr = (size_t)s->D.nchains * s->D.nphase;
    if (cells) HIPCHK(hipMemcpy(cells, L.cell, nr * L.kmax * sizeof(int), hipMemcpyDeviceToHost));
    if (vals) HIPCHK(hipMemcpy(vals, L.val, nr * L.kmax * sizeof(int), hipMemcpyDeviceToHost));
    if (counts) HIPCHK(hipMemcpy(counts, L.cnt_k, nr * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_vor_set(mceik_mcmc *s, const int *cells, const int *vals, const int *counts, int recompute)
{
    if (!s || !s->vor_on || !cells || !vals || !counts) return 1;
    if (vor_check(s, "mceik_mcmc_vor_set", s->V.kmin, s->V.kmax, cells, vals, counts)) return 1;
    if (post_holds_states(s)) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    return vor_load(s, "mceik_mcmc_vor_set", cells, vals, counts, recompute != 0);
}

extern "C" int mceik_mcmc_vor_rasterize(mceik_mcmc *s)
{
    if (!s || !s->vor_on) return 1;
    DeviceScope dg(s->device);
    const McmcDev &D = s->D;
    HIPCHK(vor_raster(s->V, D.ncell, D.nchains * D.nphase, s->V.cell, s->V.val, s->V.cnt_k, D.v, (size_t)D.ncell, D.slow_cur,
                      D.slow_prop, (size_t)D.ncell, s->stream));
    return 0;
}

extern "C" int mceik_mcmc_vor_stats(mceik_mcmc *s, long long *counters, int reset)
{
    if (!s || !s->V.cell) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nch = s->D.nchains, n = 4 * VOR_NCNT;
    std::vector<unsigned long long> cnt(nch * n);
    HIPCHK(hipMemcpy(cnt.data(), s->V.cnt, cnt.size() * 8, hipMemcpyDeviceToHost));
    for (size_t q = 0; q < n && counters; q++) {
        long long t = 0;
        for (size_t c = 0; c < nch; c++) t += (long long)cnt[c * n + q];
        counters[q] = t;
    }
    if (reset) HIPCHK(hipMemset(s->V.cnt, 0, cnt.size() * 8));
    return 0;
}

extern "C" int mceik_mcmc_vor_last(mceik_mcmc *s, int *phase, int *rec, int *pcells, int *pvals, int *vprop, double *logu,
                                   double *logl_prop, unsigned char *accept)
{
    if (!s || !s->V.cell) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t nch = s->D.nchains;
    const VorDev &L = s->V;
    if (phase) *phase = s->vor_last_ph;
    if (rec) HIPCHK(hipMemcpy(rec, L.rec, nch * VOR_NREC * sizeof(int), hipMemcpyDeviceToHost));
    if (pcells) HIPCHK(hipMemcpy(pcells, L.pcell, nch * L.kmax * sizeof(int), hipMemcpyDeviceToHost));
    if (pvals) HIPCHK(hipMemcpy(pvals, L.pval, nch * L.kmax * sizeof(int), hipMemcpyDeviceToHost));
    if (vprop) HIPCHK(hipMemcpy(vprop, L.vprop, nch * s->D.ncell * sizeof(int), hipMemcpyDeviceToHost));
    if (logu) HIPCHK(hipMemcpy(logu, s->D.prop_logu, nch * 8, hipMemcpyDeviceToHost));
    if (logl_prop) HIPCHK(hipMemcpy(logl_prop, L.logl_prop, nch * 8, hipMemcpyDeviceToHost));
    if (accept) HIPCHK(hipMemcpy(accept, s->D.accept, nch, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_vor_moments(mceik_mcmc *s, long long *n, unsigned long long *hist, unsigned long long *dens)
{
    if (!s || !s->V.cell) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (n) *n = s->vor_n;
    if (hist) HIPCHK(hipMemcpy(hist, s->V.hist, (size_t)s->D.nphase * (s->V.kmax + 1) * 8, hipMemcpyDeviceToHost));
    if (dens) HIPCHK(hipMemcpy(dens, s->V.dens, (size_t)s->D.nphase * s->D.ncell * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mceik_mcmc_vor_moments_set(mceik_mcmc *s, long long n, const unsigned long long *hist,
                                          const unsigned long long *dens)
{
    if (!s || !s->V.cell || n < 0 || !hist || !dens) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(s->V.hist, hist, (size_t)s->D.nphase * (s->V.kmax + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->V.dens, dens, (size_t)s->D.nphase * s->D.ncell * 8, hipMemcpyHostToDevice));
    s->vor_n = n;
    return 0;
}

static int vor_grid_ok(int ncx, int ncy, int ncz)
{
    return ncx >= 1 && ncy >= 1 && ncz >= 1 && (long long)ncx * ncy * ncz <= INT_MAX;
}

extern "C" int mceik_vor_raster(int ncx, int ncy, int ncz, const int *metric, const int *cells, const int *vals, int k,
                                int *v)
{
    if (!vor_grid_ok(ncx, ncy, ncz) || !metric || !cells || !vals || !v || k < 1) return 1;
    if (metric[0] < 1 || metric[1] < 1 || metric[2] < 1 || metric[0] > 32767 || metric[1] > 32767 || metric[2] > 32767 ||
        vor_d2max(ncx, ncy, ncz, metric[0], metric[1], metric[2]) < 0)
        return 1;
    for (int j = 0; j < k; j++)
        if (cells[j] < 0 || cells[j] >= ncx * ncy * ncz) return 1;
    vor_raster_host(ncx, ncy, ncz, metric[0], metric[1], metric[2], cells, vals, k, v);
    return 0;
}

extern "C" int mceik_vor_free_cell(const int *cells, int k, int ncell, int f)
{
    if (k < 0 || (k > 0 && !cells) || ncell < 1 || f < 0 || f >= ncell - k) return -1;
    for (int j = 0; j < k; j++)
        if (cells[j] < 0 || cells[j] >= ncell) return -1;
    return vor_free_cell(cells, k, f);
}

extern "C" int mceik_vor_draw(uint32_t seed, uint32_t gchain, uint64_t step, int k, int ncell, int dv, int vlo, int vhi,
                              const int *dmax, int *out, double *logu)
{
    if (k < 1 || k > ncell || dv < 1 || vhi < vlo || !dmax || dmax[0] < 0 || dmax[1] < 0 || dmax[2] < 0) return 1;
    const VorDraw d = vor_draw(seed, gchain, step, k, ncell, dv, vlo, vhi, dmax[0], dmax[1], dmax[2]);
    if (out) {
        out[0] = d.type; out[1] = d.j; out[2] = d.f; out[3] = d.minus ? -d.mag : d.mag; out[4] = d.wnew;
        out[5] = d.dx; out[6] = d.dy; out[7] = d.dz;
    }
    if (logu) *logu = hypo_det_log_host(((double)d.u + 0.5) * (1.0 / 4294967296.0));
    return 0;
}

// After a stream synchronisation: a multi-step launch whose wave gave up
// waiting for a chain's step (the broken-queue flag) failed, and the chains'
// state is not to be trusted; every later synchronising call (and the
// gather, through mcmc_shard_view) reports it until mceik_mcmc_restore
// reloads a state.
static int mc_queue_check(mceik_mcmc *s, const char *who)
{
    if (!s->persist) return 0;
    unsigned flag = 0;
    HIPCHK(hipMemcpy(&flag, s->d_sync + MC_SYNC_WORDS(s->D.nchains) - 1, sizeof(flag), hipMemcpyDeviceToHost));
    if (!flag) return 0;
    fprintf(stderr, "%s: a multi-step launch timed out waiting for a chain's previous step (broken work queue); "
                    "the chain state is invalid\n", who);
    return -1;
}

extern "C" int mceik_mcmc_sync(mceik_mcmc *s)
{
    if (!s) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    return mc_queue_check(s, "mceik_mcmc_sync");
}

extern "C" int mceik_mcmc_get_state(mceik_mcmc *s, int *v, double *logl, long long *naccept, long long *step)
{
    if (!s) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (mc_queue_check(s, "mceik_mcmc_get_state")) return -1;
    const McmcDev &D = s->D;
    if (v) HIPCHK(hipMemcpy(v, D.v, (size_t)D.nchains * D.ncm * 4, hipMemcpyDeviceToHost));
    if (logl) HIPCHK(hipMemcpy(logl, D.logl, (size_t)D.nchains * 8, hipMemcpyDeviceToHost));
    if (naccept) HIPCHK(hipMemcpy(naccept, D.naccept, (size_t)D.nchains * 8, hipMemcpyDeviceToHost));
    if (step) *step = s->step;
    return 0;
}

extern "C" int mceik_mcmc_checkpoint(mceik_mcmc *s, int *v, double *logl, long long *naccept, long long *step,
                                     int *nkept)
{
    if (!s) return 1;
    if (mceik_mcmc_get_state(s, v, logl, naccept, step)) return -1;
    if (nkept) *nkept = s->nkept;
    return 0;
}

extern "C" int mceik_mcmc_restore(mceik_mcmc *s, const int *v, const double *logl, const long long *naccept,
                                  long long step, int nkept)
{
    if (!s || !v || step < 0 || nkept < 0) return 1;
    DeviceScope dg(s->device);
    McmcDev &D = s->D;
    const size_t n = (size_t)D.nchains * D.ncm;
    for (size_t i = 0; i < n; i++) {
        const bool sph = (int)(i % (size_t)D.ncm) >= D.ncell;
        const int lo = sph ? D.vsmin : D.vmin, hi = sph ? D.vsmax : D.vmax;
        if (v[i] < lo || v[i] > hi) {
            fprintf(stderr, "mceik_mcmc_restore: v[%zu] = %d outside the prior [%d, %d]\n", i, v[i], lo, hi);
            return 1;
        }
    }
    std::vector<float> sl(n);
    for (size_t i = 0; i < n; i++) sl[i] = 1.0f / (float)v[i];
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(D.v, v, n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.slow_cur, sl.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.slow_prop, sl.data(), n * sizeof(float), hipMemcpyHostToDevice));
    if (naccept) HIPCHK(hipMemcpy(D.naccept, naccept, (size_t)D.nchains * 8, hipMemcpyHostToDevice));
    else HIPCHK(hipMemset(D.naccept, 0, (size_t)D.nchains * 8));
    if (logl) {
        HIPCHK(hipMemcpy(D.logl, logl, (size_t)D.nchains * 8, hipMemcpyHostToDevice));
    } else if (int rc = forward_logl(s, "mceik_mcmc_restore")) {
        return rc;
    }
    s->step = step;
    s->nkept = nkept;
    s->nkept_base = nkept;
    if (s->persist) {
        // the restored state replaces whatever a broken multi-step launch left: clear its flag
        HIPCHK(hipMemset(s->d_sync + MC_SYNC_WORDS(s->D.nchains) - 1, 0, sizeof(unsigned)));
    }
    return 0;
}

extern "C" int mceik_mcmc_get_samples(mceik_mcmc *s, void *v_out, double *logl_out, int max, int kind, int *nkept)
{
    if (!s) return 1;
    int have = std::min(s->nkept - s->nkept_base, s->max_samples);
    int n = have < max ? have : max;
    if (nkept) *nkept = n;
    if (n <= 0) return 0;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (mc_queue_check(s, "mceik_mcmc_get_samples")) return -1;
    hipMemcpyKind k = kind ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t per = (size_t)s->D.nchains * s->D.ncm;
    // ring slot of the i-th of the n most recent states: (nkept - n + i) mod max_samples
    int i = 0;
    while (i < n) {
        const int slot = (int)(((long long)s->nkept - n + i) % s->max_samples);
        const int run = std::min(n - i, s->max_samples - slot);     // contiguous slots
        if (v_out)
            HIPCHK(hipMemcpy((int *)v_out + (size_t)i * per, s->D.keep_v + (size_t)slot * per,
                             (size_t)run * per * 4, k));
        if (logl_out)
            HIPCHK(hipMemcpy(logl_out + (size_t)i * s->D.nchains, s->D.keep_logl + (size_t)slot * s->D.nchains,
                             (size_t)run * s->D.nchains * 8, k));
        i += run;
    }
    return 0;
}

// Device view of this sampler's chain shard for comm.hip's gather: which = 0
// the current state, 1 the most recent kept state (1 if none is kept).
int mcmc_shard_view(mceik_mcmc *s, int which, McmcShard *out)
{
    if (!s || !out) return 1;
    const McmcDev &D = s->D;
    out->device = s->device; out->stream = s->stream;
    out->nchains = D.nchains; out->chain_offset = D.chain_offset; out->ncell = D.ncm;
    {   // a broken multi-step launch left no valid state to gather (-1)
        DeviceScope dg(s->device);
        if (hipStreamSynchronize(s->stream) != hipSuccess || mc_queue_check(s, "mceik_mcmc_gather")) return -1;
    }
    if (which == 0) {
        out->v = D.v; out->logl = D.logl;
        return 0;
    }
    if (s->max_samples <= 0 || s->nkept - s->nkept_base <= 0) return 1;
    const int slot = (int)(((long long)s->nkept - 1) % s->max_samples);
    out->v = D.keep_v + (size_t)slot * D.nchains * D.ncm;
    out->logl = D.keep_logl + (size_t)slot * D.nchains;
    return 0;
}

extern "C" int mceik_mcmc_last(mceik_mcmc *s, const float **ttab, const int **niter, const unsigned char **accept,
                               const int **ierr)
{
    if (!s) return 1;
    if (ttab) *ttab = s->last_ttab;
    if (niter) *niter = s->fb.niter;
    if (accept) *accept = s->D.accept;
    if (ierr) *ierr = s->d_ierr;
    return 0;
}

extern "C" int mceik_mcmc_last_phase(mceik_mcmc *s, const int **phase)
{
    if (!s || !phase) return 1;
    *phase = s->D.prop_phase;
    return 0;
}

extern "C" int mceik_mcmc_get_info(mceik_mcmc *s, mceik_mcmc_info *info)
{
    if (!s || !info) return 1;
    DeviceScope dg(s->device);
    memset(info, 0, sizeof(*info));
    info->npipe = s->npipe;
    info->multi_step = mcmc_multi_step(s) ? 1 : 0;
    info->nphase = s->D.nphase;
    info->masked_s = s->masked_s;
    FsmLaunch L;
    fill_launch(L, &s->fb);
    const int is_double = s->fb.precision == 64;
    info->step_z = fsm_launch_kind(L, is_double);
    info->fixed_layout = info->step_z == 16 && fsm16_fixed_layout(L) ? 1 : 0;
    info->lds_bytes = fsm_launch_lds_bytes(L, is_double);
    snprintf(info->kernel, sizeof(info->kernel), "%s", fsm_launch_name(L, is_double));
    for (int k = 0; k < s->npipe && k < 4; k++) {
        const Pipe &p = s->pipe[k];
        info->chains[k] = p.fb.nmodel;
        info->waves[k] = ws_layout(&p.fb).nwaves;
        info->workspace_bytes[k] = p.ws_bytes;
    }
    return 0;
}

extern "C" int mceik_mcmc_fsm_stats(mceik_mcmc *s, double *fsm_ms, long long *nlaunch, unsigned long long *iters,
                                    unsigned long long *visits, int reset)
{
    if (!s) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (mc_queue_check(s, "mceik_mcmc_fsm_stats")) return -1;
    while (s->ev_folded < s->nlaunch) {
        if (fold_launch(s, s->ev_folded)) return -1;
        s->ev_folded++;
    }
    unsigned long long it[MCEIK_ITERS_N] = {0};
    HIPCHK(hipMemcpy(it, s->d_iters, sizeof(it), hipMemcpyDeviceToHost));
    {   // accounting build: requested bytes per launch by category
        unsigned long long tsum = 0;
        for (int k = 0; k < MCEIK_TRAFFIC_N; k++) tsum += it[6 + k];
        if (tsum && s->nlaunch) {
            static const char *nm[MCEIK_TRAFFIC_N] = {"own_load", "halo_load", "zup_load", "own_store",
                                                      "u0_store", "cell_load", "verify_load", "init_gather"};
            fprintf(stderr, "mceik traffic (requested bytes per FSM launch, %lld launches):", s->nlaunch);
            for (int k = 0; k < MCEIK_TRAFFIC_N; k++) fprintf(stderr, " %s=%.6e", nm[k], (double)it[6 + k] / s->nlaunch);
            fprintf(stderr, " total=%.6e\n", (double)tsum / s->nlaunch);
        }
    }
    if (fsm_ms) *fsm_ms = s->fsm_ms;
    if (nlaunch) *nlaunch = s->nlaunch;
    if (iters) *iters = it[0];
    if (visits) { visits[0] = it[1]; visits[1] = it[2]; visits[2] = it[3]; visits[3] = it[4]; }
    if (reset) {
        s->fsm_ms = 0.0;
        s->nlaunch = 0;
        s->ev_folded = 0;
        HIPCHK(hipMemset(s->d_iters, 0, MCEIK_ITERS_N * sizeof(unsigned long long)));
    }
    return 0;
}

extern "C" int mceik_mcmc_fsm_solves(mceik_mcmc *s, unsigned long long *solves)
{
    if (!s || !solves) return 1;
    DeviceScope dg(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (mc_queue_check(s, "mceik_mcmc_fsm_solves")) return -1;
    HIPCHK(hipMemcpy(solves, s->d_iters + 5, sizeof(*solves), hipMemcpyDeviceToHost));
    return 0;
}
