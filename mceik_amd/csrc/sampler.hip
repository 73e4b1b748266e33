// sampler.hip -- the per-GPU MCMC sampler of the C-ABI (include/mceik.h
// mceik_mcmc_init / _set_stream / _run / _finalize): device state at init
// time, the pipes, the forward launch and the step loop.
//
// Host orchestration only.  The numerics live in fsm_kernel.hip,
// fsm16_kernel.hip, mcmc_kernels.hip, temper.hip, block.hip, prior.hip,
// hypo.hip, nuis.hip, lang.hip, de.hip, vor.hip, adjoint.hip, posterior.hip,
// cov.hip, ess.hip and fit.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fsm_batch.h"
#include "host_util.h"
#include "mcmc_host.h"
#include "sampler.h"
#include "temper.h"

static int source_index(int n, double x0, double dx, double xs)   // fsm3d.f90:697-711 (0-based)
{
    if (xs <= x0) return 0;
    if (xs >= x0 + (double)(n - 1) * dx) return n - 1;
    return (int)((xs - x0) / dx + 0.5);
}

// Trilinear mode (mceik_mcmc_opts.tt_interp; no reference counterpart): the
// lowest corner i of the grid cell holding xs, clamped to [0, n-2], and the
// fraction w = (xs - x0)/dx - i in [0, 1] rounded once to fp32.  Positions
// outside the grid clamp to its faces (w = 0 or 1), the snapping rule's
// clamping (fsm3d.f90:697-711).
static int cell_corner(int n, double x0, double dx, double xs, float *w)
{
    if (n < 2) { *w = 0.0f; return 0; }
    const double f = (xs - x0) / dx;
    int i = f <= 0.0 ? 0 : (int)f;
    if (i > n - 2) i = n - 2;
    double r = f - (double)i;
    r = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
    *w = (float)r;
    return i;
}

// Adds the elapsed time of timed launch k (its pair is complete once its end
// event is) to fsm_ms.  Blocks only when MCEIK_EV_RING launches are queued.
int fold_launch(mceik_mcmc *s, long long k)
{
    const int r = (int)(k % MCEIK_EV_RING);
    float t = 0.f;
    HIPCHK(hipEventSynchronize(s->ev[2 * r + 1]));
    HIPCHK(hipEventElapsedTime(&t, s->ev[2 * r], s->ev[2 * r + 1]));
    s->fsm_ms += t;
    return 0;
}

// Pipe k's stream, resolved at use: mceik_mcmc_set_stream may change the
// sampler's, which one pipe steps on.
static hipStream_t pipe_stream(const mceik_mcmc *s, int k) { return s->npipe > 1 ? s->pipe[k].st : s->stream; }

// The FSM launch of pipe k's batch on its stream: the step batch, or with hyp
// the hypocentre step's (every model of the pipe's chains at [current |
// candidate]), or `other` in the pipe's workspace (a DE step's compact batch).
static int mcmc_forward(mceik_mcmc *s, bool timed, int k, const McmcExt *ext = nullptr, bool hyp = false,
                        const mceik_fsm_batch *other = nullptr)
{
    Pipe &p = s->pipe[k];
    const hipStream_t st = pipe_stream(s, k);
    int r = 0;
    if (timed) {
        // the ring slot of launch nlaunch - RING is reused: fold that launch first
        while (s->ev_folded <= s->nlaunch - MCEIK_EV_RING) {
            if (fold_launch(s, s->ev_folded)) return -1;
            s->ev_folded++;
        }
        r = (int)(s->nlaunch % MCEIK_EV_RING);
        while (s->ev_made <= r) {
            HIPCHK(hipEventCreate(&s->ev[2 * s->ev_made]));
            HIPCHK(hipEventCreate(&s->ev[2 * s->ev_made + 1]));
            s->ev_made++;
        }
        HIPCHK(hipEventRecord(s->ev[2 * r], st));
    }
    if (fsm_batch_solve_impl(other ? other : hyp ? &p.fb_hyp : &p.fb, p.ws, p.ws_bytes, st, ext)) return -1;
    s->last_ttab = s->fb.ttab;
    if (timed) {
        HIPCHK(hipEventRecord(s->ev[2 * r + 1], st));
        s->nlaunch++;
    }
    if (s->d_order && s->npipe == 1 && !hyp && !other) {  // the next launch pulls this launch's longest solves first (one pipe only)
        HIPCHK(mcmc_lpt_order(s->d_clock, p.fb.nmodel * p.fb.nstat, s->d_order, st));
        // the batch the next launch uses, and the sampler's, which pipes_refresh derives it from
        p.fb.solve_order = s->fb.solve_order = s->d_order;
    }
    return 0;
}

// Untimed forward of every model of every chain (init, restore): tables into
// ttab_cur (nphase 2, or nuisance state held) or the step tables (nphase 1).
int mcmc_forward_all(mceik_mcmc *s)
{
    if (mceik_fsm_batch_solve(&s->fb_all, s->ws, s->ws_bytes, s->stream)) return -1;
    s->last_ttab = s->fb_all.ttab;
    return 0;
}

// MCEIK_SOLVE_CLOCK_REPORT=1: how busy the persistent waves were in the last
// launch (sum of solve durations / (waves x launch span)); synchronises.
static void clock_report(mceik_mcmc *s, const char *tag)
{
    const size_t n = (size_t)s->fb.nmodel * s->fb.nstat;
    std::vector<unsigned long long> clk(n * 2);
    if ((s->npipe > 1 ? hipDeviceSynchronize() : hipStreamSynchronize(s->stream)) != hipSuccess ||
        hipMemcpy(clk.data(), s->d_clock, clk.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return;
    unsigned long long t0 = ~0ull, t1 = 0;
    double busy = 0.0, dmin = 1e30, dmax = 0.0;
    for (size_t i = 0; i < clk.size(); i += 2) {
        t0 = clk[i] < t0 ? clk[i] : t0;
        t1 = clk[i + 1] > t1 ? clk[i + 1] : t1;
        const double d = (double)(clk[i + 1] - clk[i]);
        busy += d;
        dmin = d < dmin ? d : dmin;
        dmax = d > dmax ? d : dmax;
    }
    const int nw = ws_layout(&s->fb).nwaves;
    fprintf(stderr, "mceik solve clock (%s, %s order): %zu solves on %d waves, launch %.1f ms, solve %.1f..%.1f ms "
                    "(mean %.1f), waves busy %.2f%%\n", tag, s->d_order ? "longest-first" : "id", n, nw,
            (t1 - t0) * 1e-5, dmin * 1e-5, dmax * 1e-5, busy / n * 1e-5, 100.0 * busy / ((double)nw * (double)(t1 - t0)));
}

// A view of chains [off, off + n) of the sampler's device state / batch.
static McmcDev dev_view(const McmcDev &D, int off, int n)
{
    McmcDev V = D;
    const size_t o = (size_t)off, oc = o * D.ncm;
    V.nchains = n;
    V.chain_offset = D.chain_offset + off;
    V.v += oc; V.slow_cur += oc; V.slow_prop += oc;
    V.logl += o; V.naccept += o;
    V.prop_cell += o; V.prop_phase += o; V.prop_v += o; V.prop_inprior += o; V.prop_logu += o; V.accept += o;
    V.ttab += o * D.nstat * D.nev;
    if (V.ttab_cur) V.ttab_cur += o * D.nphase * D.nstat * D.nev;
    if (V.keep_v) V.keep_v += oc;
    if (V.keep_logl) V.keep_logl += o;
    if (V.beta) V.beta += o;
    return V;
}

// The same view of the block state's per-chain arrays (the counters are the sampler's).
static BlockDev dev_view(const BlockDev &B, int off)
{
    BlockDev V = B;
    if (V.prop_amp) V.prop_amp += off;
    if (V.prop_rad) V.prop_rad += off;
    return V;
}

// The same view of the prior state: dE is [nchains][2].
static PriorDev dev_view(const PriorDev &P, int off)
{
    PriorDev V = P;
    if (V.dE) V.dE += 2 * (size_t)off;
    return V;
}

// The same view of the hypocentre state's per-chain arrays (the counters and moments are the sampler's).
static HypoDev dev_view(const HypoDev &H, const McmcDev &D, int off)
{
    HypoDev V = H;
    if (!H.hyp) return V;
    const size_t o = (size_t)off, oe = o * D.nev;
    V.hyp += 3 * oe; V.ev1 += oe; V.cand += 3 * oe; V.acc += oe; V.obj += 2 * oe; V.logu += oe;
    if (V.evall) V.evall += oe * D.nphase;
    V.ev2 += 2 * oe * D.nphase;
    V.ttab2 += 2 * oe * D.nphase * D.nstat;
    return V;
}

// The same view of the nuisance state's per-chain arrays (the tables, counters and moments are the sampler's).
static NuisDev dev_view(const NuisDev &N, const McmcDev &D, int off)
{
    NuisDev V = N;
    if (!N.kn) return V;
    const size_t o = (size_t)off;
    V.kn += o * D.nphase; V.kc += o * D.nphase * D.nstat;
    V.var_eff += o * N.nobs; V.tcorr_eff += o * N.nobs;
    V.rec += 4 * o * N.nsub; V.rlogl += 2 * o * N.nsub;
    return V;
}

// The same view of the Langevin state's per-chain arrays.
static LangDev dev_view(const LangDev &L, const McmcDev &D, int off)
{
    LangDev V = L;
    if (!L.delta) return V;
    const size_t o = (size_t)off, os = o * D.nstat;
    V.delta += o * D.ncell; V.vprop += o * D.ncm; V.g0 += o * D.ncell; V.g1 += o * D.ncell;
    V.lq += 3 * o; V.nmove += o; V.status += o; V.cnt += 4 * o;
    V.tt0 += os * D.nev;
    V.ierr0 += os; V.ierr1 += os; V.ast0 += os; V.ast1 += os; V.niter += os;
    V.pen += o * D.nphase;
    return V;
}

// The same view of the DE state's per-chain arrays; the compact buffers of the
// pipe's movers start at the pipe's own rows (a pipe has at most as many movers
// as chains), its mover lists are the parts of the sampler's that fall on its
// chains (movs: the host's copy of those).
static DeDev dev_view(const DeDev &L, const McmcDev &D, const mceik_fsm_batch &fb, const std::vector<int> *movs,
                      const int *d_mov, int off, int n)
{
    DeDev V = L;
    if (!L.a) return V;
    const size_t o = (size_t)off, os = o * D.nstat;
    V.off = off;
    V.a += o; V.b += o; V.inbox += o; V.nmove += o; V.status += o; V.logl_prop += o;
    V.vprop += o * D.ncm;
    V.pen += o * D.nphase;
    V.cnt += 5 * o;
    V.slow += o * D.ncell; V.ttab += os * D.nev; V.ierr += os; V.niter += os; V.ev += o * D.nev;
    V.ttab_out = fb.ttab + os * D.nev;
    V.ierr_out = fb.ierr + os;
    V.niter_out = fb.niter + os;
    for (int par = 0; par < 2; par++) {
        const std::vector<int> &m = movs[par];
        const size_t lo = std::lower_bound(m.begin(), m.end(), off) - m.begin();
        const size_t hi = std::lower_bound(m.begin(), m.end(), off + n) - m.begin();
        V.mov[par] = d_mov + (size_t)par * D.nchains + lo;
        V.nmov[par] = (int)(hi - lo);
    }
    return V;
}

// The same view of the Voronoi state's per-chain arrays (the moments are the sampler's).
static VorDev dev_view(const VorDev &L, const McmcDev &D, int off)
{
    VorDev V = L;
    if (!L.cell) return V;
    const size_t o = (size_t)off, on = o * D.nphase * L.kmax;
    V.cell += on; V.val += on; V.cnt_k += o * D.nphase;
    V.pcell += o * L.kmax; V.pval += o * L.kmax; V.pk += o;
    V.rec += o * VOR_NREC; V.logl_prop += o;
    V.vprop += o * D.ncell;
    V.cnt += o * 4 * VOR_NCNT;
    return V;
}

// Chains [off, off + n) of the hypocentre step's batch: nphase models per
// chain.  It runs in the workspace of the pipe's step batch sb, so it keeps at
// most that batch's resident waves (the workspace grows with the waves only).
static mceik_fsm_batch hyp_batch_view(const mceik_fsm_batch &b, const mceik_fsm_batch &sb, int off, int n, size_t ncm,
                                      int nphase)
{
    mceik_fsm_batch V = b;
    const size_t om = (size_t)off * nphase, os = om * b.nstat;
    V.nmodel = n * nphase;
    V.slow = (const float *)b.slow + (size_t)off * ncm;
    V.ev_node = b.ev_node + om * b.ev_stride;
    V.ttab = b.ttab + os * b.nev;
    V.niter = b.niter + os;
    V.ierr = b.ierr + os;
    V.max_waves = ws_layout(&sb).nwaves;
    return V;
}

static mceik_fsm_batch batch_view(const mceik_fsm_batch &b, int off, int n, size_t ncm)
{
    mceik_fsm_batch V = b;
    const size_t o = (size_t)off, os = o * b.nstat;
    V.nmodel = n;
    V.slow = (const float *)b.slow + o * ncm;       // a chain's models are ncm = nphase * ncell floats
    if (V.model_phase) V.model_phase = b.model_phase + o;
    V.ttab = b.ttab + os * b.nev;
    if (b.ev_stride) V.ev_node = b.ev_node + o * b.ev_stride;     // per-chain event lists (hypocentre moves)
    V.niter = b.niter + os;
    V.ierr = b.ierr + os;
    V.solve_order = nullptr;
    V.solve_clock = b.solve_clock ? b.solve_clock + 2 * os : nullptr;
    return V;
}

// The chain split: pipe k of np takes chains [pipe_lo(k), pipe_lo(k + 1)) of nch.
static int pipe_lo(int nch, int k, int np) { return (int)((long long)nch * k / np); }

int pipes_refresh(mceik_mcmc *s)
{
    const int nch = s->D.nchains, np = s->npipe;
    for (int k = 0; k < np; k++) {
        Pipe &p = s->pipe[k];
        const int lo = pipe_lo(nch, k, np), n = pipe_lo(nch, k + 1, np) - lo;
        p.D = dev_view(s->D, lo, n);
        p.B = dev_view(s->B, lo);
        p.P = dev_view(s->P, lo);
        p.fb = batch_view(s->fb, lo, n, (size_t)s->D.ncm);
        p.H = dev_view(s->H, s->D, lo);
        p.N = dev_view(s->N, s->D, lo);
        p.L = dev_view(s->L, s->D, lo);
        p.De = dev_view(s->De, s->D, s->fb, s->de_mov, s->d_demov, lo, n);
        p.V = dev_view(s->V, s->D, lo);
        if (s->H.hyp) p.fb_hyp = hyp_batch_view(s->fb_hyp, p.fb, lo, n, (size_t)s->D.ncm, s->D.nphase);
    }
    // the longest-first order covers the whole batch: one pipe's (mcmc_forward)
    if (np == 1) s->pipe[0].fb.solve_order = s->fb.solve_order;
    if (s->d_dev) HIPCHK(hipMemcpy(s->d_dev, &s->D, sizeof(McmcDev), hipMemcpyHostToDevice));
    return 0;
}

// np pipes: parts of the chains, their own streams and workspaces (pipe 0
// reuses the sampler's).  Returns nonzero on a HIP failure; falls back to one
// pipe (with a message) when the extra workspaces do not fit.
static int pipes_setup(mceik_mcmc *s, int np)
{
    Pipe *P = s->pipe;
    const int nch = s->D.nchains;
    s->npipe = 1;                      // one pipe: every chain on the sampler's workspace and stream
    P[0].ws = s->ws;
    P[0].ws_bytes = s->ws_bytes;
    if (np < 2) return pipes_refresh(s);
    // The scratch budget binds (large grids: fewer resident waves than the
    // occupancy allows): pipes would have to share those waves, and splitting
    // them lengthens each half's queue tail more than the other half fills
    // (C5: 24.3 vs 25.1 proposals/s, profiles/r03_cfg): run one pipe.
    const int w1 = ws_layout(&s->fb).nwaves;
    if (w1 < fsm_batch_waves_uncapped(&s->fb)) {
        fprintf(stderr, "mceik_mcmc_init: the FSM scratch budget caps the waves (%d); running one pipe\n", w1);
        return pipes_refresh(s);
    }
    // workspaces: carved out of the sampler's own when they fit in it together
    // (budget-capped grids), else pipe 0 reuses it and the others get their own
    size_t sum = 0, need[MCEIK_MAX_PIPES];
    for (int k = 0; k < np; k++) {
        const int lo = pipe_lo(nch, k, np);
        const mceik_fsm_batch b = batch_view(s->fb, lo, pipe_lo(nch, k + 1, np) - lo, (size_t)s->D.ncm);
        sum += (need[k] = (mceik_fsm_workspace_bytes(&b) + 255) & ~(size_t)255);
    }
    bool fit = true;
    size_t extra = 0;
    if (sum <= s->ws_bytes) {
        size_t off = 0;
        for (int k = 0; k < np; k++) {
            P[k].ws = (char *)s->ws + off;
            P[k].ws_bytes = need[k];
            off += need[k];
        }
    } else {
        fit = need[0] <= s->ws_bytes;
        for (int k = 1; k < np && fit; k++) {
            extra += need[k];
            if (hipMalloc(&P[k].ws, need[k]) != hipSuccess) {
                (void)hipGetLastError();
                P[k].ws = nullptr;
                fit = false;
            } else {
                P[k].ws_bytes = need[k];
                P[k].ws_own = true;
            }
        }
    }
    if (!fit) {
        for (int k = 1; k < np; k++) {
            if (P[k].ws_own && P[k].ws) hipFree(P[k].ws);
            P[k].ws = nullptr;
            P[k].ws_bytes = 0;
            P[k].ws_own = false;
        }
        fprintf(stderr, "mceik_mcmc_init: %d pipes need %zu B more FSM workspace; running one pipe\n", np, extra);
        return pipes_refresh(s);
    }
    s->npipe = np;                     // finalize releases whatever was created
    for (int k = 0; k < np; k++) {
        HIPCHK(hipStreamCreateWithFlags(&P[k].st, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&P[k].join, hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&s->pfork, hipEventDisableTiming));
    return pipes_refresh(s);
}

// After a forward: every solve's reference ierr must be 0 (a station on the
// grid's first node is the SETBCS quirk, fsm3d.f90:736-745, ierr = 1; its table
// would stay u_nan).  Synchronises; names the failing stations.
int check_forward_ierr(mceik_mcmc *s, const char *who)
{
    const int np = s->D.nphase, ns = s->D.nstat;
    const size_t n = (size_t)s->D.nchains * np * ns;     // the full batch: [chain][phase][station]
    std::vector<int> ie(n);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(ie.data(), s->d_ierr, n * sizeof(int), hipMemcpyDeviceToHost));
    int bad = 0;
    for (int ph = 0; ph < np; ph++)
        for (int st = 0; st < ns; st++) {
            int e = 0;
            for (int c = 0; c < s->D.nchains && !e; c++) e = ie[((size_t)c * np + ph) * ns + st];
            if (e) {
                fprintf(stderr, "%s: station %d (0-based)%s: eikonal solve ierr = %d%s\n", who, st,
                        np > 1 ? (ph ? ", S model" : ", P model") : "", e,
                        e == 1 ? " (source on the grid's first node or outside it, fsm3d.f90:736-745)" : "");
                bad = 1;
            }
        }
    return bad;
}

extern "C" int mceik_mcmc_init(const struct mceik_parms_struct *parms, const struct mceik_stations_struct *st,
                               const struct mceik_catalog_struct *cat, const mceik_mcmc_opts *o,
                               const int *v0, mceik_mcmc **out)
{
    if (!parms || !st || !cat || !o || !v0 || !out) return 1;
    *out = nullptr;
    if (parms->dx != parms->dy || parms->dx != parms->dz || parms->dx <= 0.0) {
        fprintf(stderr, "mceik_mcmc_init: the eikonal solver needs dx = dy = dz\n");
        return 1;
    }
    const int nphase = o->nphase <= 1 ? 1 : o->nphase;
    if (o->nx < 2 || o->ny < 2 || o->nz < 2 || o->nchains < 1 || st->nstat < 1 || cat->nevents < 1 ||
        o->vmin < 1 || o->vmax < o->vmin || o->dvmax < 1 || !(o->precision == 0 || o->precision == 32 ||
                                                              o->precision == 64) ||
        nphase > 2 || (nphase == 2 && (o->vsmin < 1 || o->vsmax < o->vsmin))) {
        fprintf(stderr, "mceik_mcmc_init: invalid options\n");
        return 1;
    }
    {
        // the forward solve's own geometry check (mceik_fsm_check: host only, it names the reason)
        mceik_fsm_batch g;
        memset(&g, 0, sizeof(g));
        g.nx = o->nx; g.ny = o->ny; g.nz = o->nz;
        g.precision = o->precision == 64 ? 64 : 32;
        g.nmodel = o->nchains; g.nstat = st->nstat; g.nsrc = 1;
        g.slow_mode = 1; g.nrx = parms->nrefx; g.nry = parms->nrefy; g.nrz = parms->nrefz;
        g.fast_sqrt = parms->dx / (double)(nphase == 2 ? std::max(o->vmax, o->vsmax) : o->vmax) >= 1e-12 ? 1 : 0;
        if (mceik_fsm_check(&g)) {
            fprintf(stderr, "mceik_mcmc_init: the eikonal solver refuses this grid\n");
            return 1;
        }
    }
    for (int e = 0; e < cat->nevents; e++)
        if (cat->obsPtr[e + 1] < cat->obsPtr[e]) {
            fprintf(stderr, "mceik_mcmc_init: obsPtr must be non-decreasing\n");
            return 1;
        }
    const int nstat = st->nstat, nev = cat->nevents, nch = o->nchains;
    const int nobs = cat->obsPtr[nev];
    // observations fit: used P picks, and used S picks against the S model
    // (nphase 2); a P-only sampler refuses a catalog with S picks unless told
    // to ignore them (mask_s), so no observation disappears silently
    int nsused = 0;
    for (int j = 0; j < nobs; j++) {
        const int k = cat->statPtr[j] - 1;
        if (cat->luseObs[j] != 0 && cat->pickType[j] == S_PRIMARY_PICK && k >= 0 && k < nstat) nsused++;
    }
    if (nphase == 1 && nsused > 0) {
        if (!o->mask_s) {
            fprintf(stderr, "mceik_mcmc_init: the catalog holds %d used S picks; set nphase = 2 (joint P and S "
                            "models) or mask_s = 1 (fit the P picks only)\n", nsused);
            return 1;
        }
        fprintf(stderr, "mceik_mcmc_init: ignoring %d S picks (nphase 1, mask_s)\n", nsused);
    }
    auto fit_obs = [&](int j) {
        const int k = cat->statPtr[j] - 1;
        return cat->luseObs[j] != 0 && k >= 0 && k < nstat &&
               (cat->pickType[j] == P_PRIMARY_PICK || (nphase == 2 && cat->pickType[j] == S_PRIMARY_PICK));
    };
    for (int j = 0; j < nobs; j++)
        if (fit_obs(j) && !(cat->varObs[j] > 0.0)) {
            fprintf(stderr, "mceik_mcmc_init: observation %d has varObs <= 0\n", j);
            return 1;
        }
    // station coordinates are metres on the grid (lcartesian = 1, as homog.c
    // sets them); geographic station lists are not converted
    if (st->lcartesian != 1) {
        fprintf(stderr, "mceik_mcmc_init: stations.lcartesian = %d: only Cartesian station coordinates (metres, "
                        "lcartesian = 1) are supported\n", st->lcartesian);
        return 1;
    }
    // Tables only for the phases a station has picks of (lhasP / lhasS,
    // mceik_struct.h:43-46; homog.c:313-335 builds exactly those): the other
    // solves are skipped.  A fit pick at a station without its flag would
    // read a table never made, so the catalog is refused.
    std::vector<unsigned char> skip((size_t)nphase * nstat, 0);
    for (int k = 0; k < nstat; k++) {
        skip[k] = st->lhasP ? st->lhasP[k] == 0 : 0;
        if (nphase == 2) skip[(size_t)nstat + k] = st->lhasS ? st->lhasS[k] == 0 : 0;
    }
    for (int j = 0; j < nobs; j++)
        if (fit_obs(j)) {
            const int k = cat->statPtr[j] - 1, sph = cat->pickType[j] == S_PRIMARY_PICK;
            if (skip[(size_t)sph * nstat + k]) {
                fprintf(stderr, "mceik_mcmc_init: observation %d is a used %s pick at station %d (1-based) whose "
                                "%s = 0\n", j, sph ? "S" : "P", k + 1, sph ? "lhasS" : "lhasP");
                return 1;
            }
        }
    int nskip = 0;
    for (unsigned char c : skip) nskip += c;
    DeviceScope dg(o->device);
    if (hipSetDevice(o->device) != hipSuccess) return -1;
    mceik_mcmc *s = new mceik_mcmc();
    s->kept[KEPT_POST] = mcmc_post_stream();
    s->kept[KEPT_COV] = mcmc_cov_stream();
    s->kept[KEPT_ESS] = mcmc_ess_stream();
    s->kept[KEPT_FIT] = mcmc_fit_stream();
    s->device = o->device;
    s->stream = nullptr;
    s->step = 0;
    s->nkept = 0;
    s->masked_s = nphase == 1 ? nsused : 0;
    s->tt_interp = o->tt_interp ? 1 : 0;
    s->nburn = parms->mcparms.nburnIn;
    s->keepk = parms->mcparms.keepK > 0 ? parms->mcparms.keepK : 1;
    s->niter_total = parms->mcparms.niter;
    s->max_samples = o->max_samples > 0 ? o->max_samples : 0;
    int nrx = parms->nrefx > 0 ? parms->nrefx : 1, nry = parms->nrefy > 0 ? parms->nrefy : 1,
        nrz = parms->nrefz > 0 ? parms->nrefz : 1;
    int ncx = mceik_div_up(o->nx, nrx), ncy = mceik_div_up(o->ny, nry), ncz = mceik_div_up(o->nz, nrz);
    int ncell = ncx * ncy * ncz;
    const int ncm = ncell * nphase;
    McmcDev &D = s->D;
    memset(&D, 0, sizeof(D));
    D.nchains = nch; D.chain_offset = o->chain_offset; D.ncell = ncell; D.nstat = nstat; D.nev = nev;
    D.nphase = nphase; D.ncm = ncm;
    D.keep_stride = nch;
    D.vmin = o->vmin; D.vmax = o->vmax; D.dvmax = o->dvmax; D.seed = o->seed;
    D.vsmin = nphase == 2 ? o->vsmin : 0; D.vsmax = nphase == 2 ? o->vsmax : 0;
    memset(&s->B, 0, sizeof(s->B));
    s->B.ncx = ncx; s->B.ncy = ncy; s->B.ncz = ncz;
    memset(&s->P, 0, sizeof(s->P));
    memset(&s->N, 0, sizeof(s->N));
    memset(&s->Nbuf, 0, sizeof(s->Nbuf));
    // host-side problem tables
    std::vector<double> src((size_t)nstat * 4);
    for (int i = 0; i < nstat; i++) {
        src[i * 4 + 0] = 0.0; src[i * 4 + 1] = st->xrec[i]; src[i * 4 + 2] = st->yrec[i]; src[i * 4 + 3] = st->zrec[i];
    }
    std::vector<int> ev(nev);
    std::vector<float> evf(o->tt_interp ? (size_t)nev * 3 : 0);
    for (int e = 0; e < nev; e++) {
        int ix, iy, iz;
        if (o->tt_interp) {   // lowest corner of the event's cell + fractions (trilinear mode)
            ix = cell_corner(o->nx, parms->x0, parms->dx, cat->xsrc[e], &evf[3 * e]);
            iy = cell_corner(o->ny, parms->y0, parms->dx, cat->ysrc[e], &evf[3 * e + 1]);
            iz = cell_corner(o->nz, parms->z0, parms->dx, cat->zsrc[e], &evf[3 * e + 2]);
        } else {
            ix = source_index(o->nx, parms->x0, parms->dx, cat->xsrc[e]);
            iy = source_index(o->ny, parms->y0, parms->dx, cat->ysrc[e]);
            iz = source_index(o->nz, parms->z0, parms->dx, cat->zsrc[e]);
        }
        ev[e] = (iz * o->ny + iy) * o->nx + ix;
    }
    s->ev_host = ev;
    std::vector<int> ostat(nobs > 0 ? nobs : 1), omask(nobs > 0 ? nobs : 1), ophase(nobs > 0 ? nobs : 1);
    std::vector<double> tcorr(nobs > 0 ? nobs : 1);
    for (int j = 0; j < nobs; j++) {
        int k = cat->statPtr[j] - 1;
        int use = fit_obs(j);
        int sph = use && cat->pickType[j] == S_PRIMARY_PICK;
        ostat[j] = use ? k : 0;
        omask[j] = !use;
        ophase[j] = sph;
        const double *corr = sph ? st->scorr : st->pcorr;       // static corrections (mceik_struct.h:42-44)
        tcorr[j] = (use && corr) ? corr[k] : 0.0;
    }
    s->h_ostat = ostat; s->h_omask = omask; s->h_ophase = ophase;
    s->h_ostat.resize(nobs > 0 ? nobs : 0); s->h_omask.resize(nobs > 0 ? nobs : 0); s->h_ophase.resize(nobs > 0 ? nobs : 0);
    std::vector<float> sl((size_t)nch * ncm);
    for (size_t i = 0; i < sl.size(); i++) sl[i] = 1.0f / (float)v0[i];
    int rc = 0;
    double *d_src = nullptr;
    int *d_ev = nullptr, *d_optr = nullptr;
    float *d_tt = nullptr;
    int *d_niter = nullptr;
    rc |= dput(s, &d_src, src.data(), src.size());
    rc |= dput(s, &d_ev, ev.data(), ev.size());
    float *d_evf = nullptr;
    if (o->tt_interp) rc |= dput(s, &d_evf, evf.data(), evf.size());
    rc |= dput(s, &d_optr, (const int *)cat->obsPtr, (size_t)nev + 1);
    int *d_ostat = nullptr, *d_omask = nullptr, *d_ophase = nullptr;
    double *d_tobs = nullptr, *d_tcorr = nullptr, *d_var = nullptr;
    rc |= dput(s, &d_ostat, ostat.data(), ostat.size());
    rc |= dput(s, &d_omask, omask.data(), omask.size());
    rc |= dput(s, &d_ophase, ophase.data(), ophase.size());
    rc |= dput(s, &d_tobs, (const double *)cat->tobs, (size_t)(nobs > 0 ? nobs : 0));
    rc |= dput(s, &d_tcorr, tcorr.data(), tcorr.size());
    rc |= dput(s, &d_var, (const double *)cat->varObs, (size_t)(nobs > 0 ? nobs : 0));
    unsigned char *d_skip = nullptr;
    if (nskip) rc |= dput(s, &d_skip, skip.data(), skip.size());
    rc |= dput(s, &D.v, v0, (size_t)nch * ncm);
    rc |= dput(s, &D.slow_cur, sl.data(), sl.size());
    rc |= dput(s, &D.slow_prop, sl.data(), sl.size());
    rc |= dalloc(s, &D.logl, nch);
    rc |= dalloc(s, &D.naccept, nch);
    rc |= dalloc(s, &D.prop_cell, nch);
    rc |= dalloc(s, &D.prop_phase, nch);
    rc |= dalloc(s, &D.prop_v, nch);
    rc |= dalloc(s, &D.prop_inprior, nch);
    rc |= dalloc(s, &D.prop_logu, nch);
    rc |= dalloc(s, &D.accept, nch);
    rc |= dalloc(s, &d_tt, (size_t)nch * nstat * nev);
    if (nphase > 1) rc |= dalloc(s, &D.ttab_cur, (size_t)nch * nphase * nstat * nev);
    rc |= dalloc(s, &d_niter, (size_t)nch * nphase * nstat);
    rc |= dalloc(s, &s->d_ierr, (size_t)nch * nphase * nstat);
    rc |= dalloc(s, &s->d_iters, MCEIK_ITERS_N);       // [0] iterations, [1..4] visit_stats, [5] solves, [6..] traffic
    if (s->max_samples) {
        rc |= dalloc(s, &D.keep_v, (size_t)s->max_samples * nch * ncm);
        rc |= dalloc(s, &D.keep_logl, (size_t)s->max_samples * nch);
    }
    if (rc) { mceik_mcmc_finalize(&s); return -1; }
    D.ttab = d_tt; D.obs_ptr = d_optr; D.obs_stat = d_ostat; D.obs_mask = d_omask;
    D.obs_phase = nphase > 1 ? d_ophase : nullptr;
    D.tobs = d_tobs; D.tcorr = d_tcorr; D.var = d_var;
    // the step batch: one solve per (chain, station) of the model the proposal
    // changed (model_phase = prop_phase: the other model's tables stay valid)
    mceik_fsm_batch &b = s->fb;
    memset(&b, 0, sizeof(b));
    b.nx = o->nx; b.ny = o->ny; b.nz = o->nz; b.h = parms->dx;
    b.x0 = parms->x0; b.y0 = parms->y0; b.z0 = parms->z0;
    b.maxit = parms->eikparms.maxit; b.tol = parms->eikparms.tol;
    b.precision = o->precision == 64 ? 64 : 32;
    b.nmodel = nch; b.nstat = nstat; b.nsrc = 1; b.src = d_src;
    b.slow_mode = 1; b.slow = D.slow_prop; b.nrx = nrx; b.nry = nry; b.nrz = nrz;
    b.model_phase = nphase > 1 ? D.prop_phase : nullptr;
    b.nphase = nphase;
    b.nev = nev; b.ev_node = d_ev; b.ev_frac = d_evf; b.ttab = d_tt; b.u_out = nullptr; b.niter = d_niter; b.ierr = s->d_ierr;
    b.max_sweeps = -1;
    b.iter_total = s->d_iters;
    b.visit_stats = s->d_iters + 1;
    b.solve_count = s->d_iters + 5;
    b.traffic = s->d_iters + 6;
    b.skip = d_skip;
    b.max_waves = o->max_waves > 0 ? o->max_waves : 0;
    // f = h/v stays a normal float: the short correctly rounded sqrt (fp32 only)
    const int vhi = nphase == 2 ? std::max(o->vmax, o->vsmax) : o->vmax;
    b.fast_sqrt = parms->dx / (double)vhi >= 1e-12 ? 1 : 0;      // f = h*s >= 1e-12: the short sqrt (fp32, fp64)
    // the full batch (init, restore): every model of every chain, models
    // [chain][phase] in place of model_phase, tables into ttab_cur
    s->fb_all = b;
    if (nphase > 1) {
        s->fb_all.nmodel = nch * nphase;
        s->fb_all.model_phase = nullptr;
        s->fb_all.ttab = D.ttab_cur;
    }
    s->last_ttab = s->fb_all.ttab;
    s->ws_bytes = std::max(mceik_fsm_workspace_bytes(&b), mceik_fsm_workspace_bytes(&s->fb_all));
    if (hipMalloc(&s->ws, s->ws_bytes) != hipSuccess) {
        fprintf(stderr, "mceik_mcmc_init: cannot allocate %zu B of FSM workspace\n", s->ws_bytes);
        s->ws = nullptr;
        mceik_mcmc_finalize(&s);
        return -1;
    }
    // initial log-likelihood of every chain.  Every launch stamps its solves
    // (solve_clock) and with MCEIK_LPT=1 the next launch drains each queue
    // longest solve first (mcmc_lpt_order; the init forward runs in id order).
    // Off by default: at C3 the waves are 96.6% busy in id order and longest-
    // first made the mean solve 4% slower.
    // MCEIK_SOLVE_CLOCK_REPORT=1: print how busy the persistent waves were
    // (init forward; diagnostic for the work-queue tail)
    const char *lpt_env = getenv("MCEIK_LPT");
    const bool lpt = lpt_env && lpt_env[0] == '1';
    const char *rep_env = getenv("MCEIK_SOLVE_CLOCK_REPORT");
    const bool report = rep_env && rep_env[0] == '1';
    if ((lpt || report) && dalloc(s, &s->d_clock, (size_t)nch * nphase * nstat * 2)) {
        mceik_mcmc_finalize(&s);
        return -1;
    }
    if (lpt && dalloc(s, &s->d_order, (size_t)nch * nstat)) {
        mceik_mcmc_finalize(&s);
        return -1;
    }
    b.solve_clock = s->d_clock;
    b.solve_order = nullptr;
    s->fb_all.solve_clock = s->d_clock;
    s->fb_all.solve_order = nullptr;
    if (mcmc_forward_all(s) || mcmc_init_loglik(D, s->N, s->stream) != hipSuccess ||
        hipStreamSynchronize(s->stream) != hipSuccess) {
        mceik_mcmc_finalize(&s);
        return -1;
    }
    if (check_forward_ierr(s, "mceik_mcmc_init")) {
        mceik_mcmc_finalize(&s);
        return 2;
    }
    s->report = report;
    if (report) clock_report(s, "init");
    // Multi-step launches by default where a step is at most
    // 4 solves per resident wave (the per-step tail is then a large share: C2
    // +1.1% over two pipes; at C3's 16 solves per wave two pipes are 1% ahead);
    // MCEIK_PERSIST=1 / 0 forces them on / off
    const char *persist_env = getenv("MCEIK_PERSIST");
    const bool short_steps = (long long)b.nmodel * b.nstat <= 4LL * ws_layout(&b).nwaves;
    s->persist = (persist_env ? persist_env[0] == '1' : short_steps) && b.precision == 32 &&
                 mceik_fsm_step_z(&b) == 16 && !lpt;
    if (s->persist && (dalloc(s, &s->d_sync, MC_SYNC_WORDS(nch)) || dput(s, &s->d_dev, &D, 1))) {
        mceik_mcmc_finalize(&s);
        return -1;
    }
    // MCEIK_MC_SPIN_LIMIT (test hook): polls before a multi-step wait gives up
    const char *spin_env = getenv("MCEIK_MC_SPIN_LIMIT");
    s->spin_limit = spin_env ? (unsigned)strtoul(spin_env, nullptr, 10) : 1u << 24;
    const char *pipe_env = getenv("MCEIK_PIPES");       // default 2; MCEIK_PIPES=1: one pipe
    int np = s->persist ? 1 : pipe_env ? atoi(pipe_env) : 2;
    np = np < 1 ? 1 : np > MCEIK_MAX_PIPES ? MCEIK_MAX_PIPES : np;
    if (np > nch) np = nch;
    if (pipes_setup(s, np)) {
        mceik_mcmc_finalize(&s);
        return -1;
    }
    hipMemset(s->d_iters, 0, MCEIK_ITERS_N * sizeof(unsigned long long));
    *out = s;
    return 0;
}

extern "C" int mceik_mcmc_set_stream(mceik_mcmc *s, void *stream)
{
    if (!s) return 1;
    s->stream = (hipStream_t)stream;
    return 0;
}

// The keep rule of the kept states and of the posterior: step gs is kept when
// gs >= nburnIn && (gs - nburnIn) % keepK == 0.
static bool kept_step(const mceik_mcmc *s, long long gs)
{
    return gs >= s->nburn && (gs - s->nburn) % s->keepk == 0;
}

// Chains the consumers of a kept state see: the cold ones while tempering is on.
int temper_cold(const mceik_mcmc *s) { return s->ntemps > 0 ? s->D.nchains / s->ntemps : s->D.nchains; }

// How many of chains [off, off + n) are cold: the first chains of a pipe's view.
static int cold_in(const mceik_mcmc *s, int off, int n) { return std::max(0, std::min(n, temper_cold(s) - off)); }

static long long next_kept_step(const mceik_mcmc *s)     // the first kept step >= s->step
{
    if (s->step < s->nburn) return s->nburn;
    const long long r = (s->step - s->nburn) % s->keepk;
    return r ? s->step + s->keepk - r : s->step;
}

int temper_round(mceik_mcmc *s, int parity)
{
    // (per-chain hypocentres and nuisance state travel with their models, enabled or not; nuclei while they
    // describe the models)
    HIPCHK(temper_swap_round(s->D, s->ntemps, parity, (uint64_t)s->step, s->d_tflag, s->d_tcnt,
                             s->d_tcnt + s->D.nchains, s->stream, s->H.hyp ? &s->H : nullptr, s->N.kn ? &s->N : nullptr,
                             s->vor_on ? &s->V : nullptr));
    return 0;
}

// What global step gs is.  A step has one kind, by precedence: hypocentre (gs %
// hypo_every == hypo_every - 1), else nuisance (gs % nuis_every == nuis_offset
// while state is held), else Langevin (gs % lang_every == lang_offset), else DE
// (gs % de_every == de_offset), else a velocity proposal.  A swap round belongs
// to step gs > 0 with gs % swap_every == 0 and runs before its proposal, with
// parity (gs / swap_every) & 1.  DE step k = (gs - de_offset) / de_every moves
// the chains of parity k & 1 of every population on phase (k >> 1) % nphase.
// While Voronoi-cell models are on a velocity step is a Voronoi step: the n-th
// such step (n counts the velocity steps below gs under the options in force)
// works on phase n % nphase.
enum StepKind { STEP_VELOCITY, STEP_HYPO, STEP_NUIS, STEP_LANG, STEP_DE };

struct StepPlan {
    StepKind kind;
    bool swap;
    int parity;
    bool kept;                         // kept_step(gs)
    int de_par, de_ph;                 // STEP_DE: the movers' parity and the phase
    int vor_ph;                        // STEP_VELOCITY while Voronoi-cell models are on: the phase
};

// Steps g in [0, gs) with g % m == r (0 <= r < m).
static long long count_mod(long long gs, long long m, long long r) { return gs > r ? (gs - r + m - 1) / m : 0; }

// Velocity steps below gs while neither Langevin nor DE moves are on (Voronoi-
// cell models refuse both): gs minus the hypocentre steps, minus the nuisance
// steps that are not hypocentre steps too.
static long long velocity_steps_below(const mceik_mcmc *s, long long gs)
{
    const bool hy = s->hypo_on && s->hypo_every > 0;
    const bool nu = s->nuis_on && s->N.kn && s->nuis_every > 0;
    long long n = gs;
    if (hy) n -= count_mod(gs, s->hypo_every, s->hypo_every - 1);
    if (nu) n -= count_mod(gs, s->nuis_every, s->nuis_offset);
    if (hy && nu) {
        // steps that are both: the first one x below the common period, then one per period
        long long a = s->hypo_every, b = s->nuis_every;
        while (b) { const long long t = a % b; a = b; b = t; }
        const long long period = (long long)s->hypo_every / a * s->nuis_every;
        for (long long x = s->hypo_every - 1; x < period; x += s->hypo_every)
            if (x % s->nuis_every == s->nuis_offset) {
                n += count_mod(gs, period, x);
                break;
            }
    }
    return n;
}

static StepPlan plan_step(const mceik_mcmc *s, long long gs)
{
    StepPlan q;
    if (s->hypo_on && s->hypo_every > 0 && gs % s->hypo_every == s->hypo_every - 1) q.kind = STEP_HYPO;
    else if (s->nuis_on && s->N.kn && s->nuis_every > 0 && gs % s->nuis_every == s->nuis_offset) q.kind = STEP_NUIS;
    else if (s->lang_on && s->lang_every > 0 && gs % s->lang_every == s->lang_offset) q.kind = STEP_LANG;
    else if (s->de_on && s->de_every > 0 && gs % s->de_every == s->de_offset) q.kind = STEP_DE;
    else q.kind = STEP_VELOCITY;
    const long long dk = q.kind == STEP_DE ? (gs - s->de_offset) / s->de_every : 0;
    q.de_par = (int)(dk & 1);
    q.de_ph = (int)((dk >> 1) % s->D.nphase);
    q.swap = s->ntemps > 1 && s->swap_every > 0 && gs > 0 && gs % s->swap_every == 0;
    q.parity = q.swap ? (int)((gs / s->swap_every) & 1) : 0;
    q.kept = kept_step(s, gs);
    q.vor_ph = s->vor_on && q.kind == STEP_VELOCITY ? (int)(velocity_steps_below(s, gs) % s->D.nphase) : 0;
    return q;
}

// The kept-state hook.  Seven consumers see the cold chains of a kept step:
// the four accumulators of s->kept (posterior, covariances, batch means, data
// fit) and the moments that live in their moves' state (hypocentre, nuisance,
// Voronoi).
// kept_queue queues those that are on for the cold chains of pipe p's view on
// stream st; kept_counted counts the state on the host once every pipe is
// queued (an accumulator is handed the count before the step, so every pipe
// passes the same one).  One pipe views every chain, so the multi-step branch calls the
// same two, where mcmc_multi_step rules the hypocentre and nuisance moments out.
static int kept_queue(mceik_mcmc *s, const Pipe &p, hipStream_t st)
{
    const int off = p.D.chain_offset - s->D.chain_offset, n = cold_in(s, off, p.D.nchains);
    if (n <= 0) return 0;
    for (const KeptStream &k : s->kept)
        if (k.on) HIPCHK(k.accumulate(k.state, p.D, p.H, p.N, off, n, k.n, st));
    if (s->hypo_on) HIPCHK(hypo_moments(p.D, p.H, n, st));
    if (s->nuis_on && s->N.kn) HIPCHK(nuis_moments(p.D, p.N, n, st));
    if (s->vor_on) HIPCHK(vor_moments(p.D, p.V, n, st));
    return 0;
}

static bool kept_any_on(const mceik_mcmc *s)
{
    for (const KeptStream &k : s->kept)
        if (k.on) return true;
    return false;
}

static void kept_counted(mceik_mcmc *s)
{
    for (KeptStream &k : s->kept)
        if (k.on) k.n++;
    if (s->hypo_on) s->hyp_n += temper_cold(s);
    if (s->nuis_on && s->N.kn) s->nuis_n += temper_cold(s);
    if (s->vor_on) s->vor_n += temper_cold(s);
}

// Chains [off, off + m) of pipe p's step batch as a Langevin step runs them:
// the forward with fields (no skip: a skipped solve has no field) of slowness
// `slow` into tables `ttab`, fields into u.
static mceik_fsm_batch lang_batch(const mceik_mcmc *s, const Pipe &p, int off, int m, const float *slow, float *ttab,
                                  void *u, int *ierr, int *niter)
{
    mceik_fsm_batch b = batch_view(p.fb, off, m, (size_t)s->D.ncm);
    const size_t os = (size_t)off * b.nstat;
    b.slow = slow + (size_t)off * s->D.ncm;
    b.ttab = ttab + os * b.nev;
    b.u_out = u;
    b.skip = nullptr;
    b.ierr = ierr + os;
    b.niter = niter + os;
    b.solve_order = nullptr;
    b.solve_clock = nullptr;
    return b;
}

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t lang_pipe_bytes(const mceik_mcmc *s, int k, int m, size_t *u, size_t *fws, size_t *aws, size_t *evw, size_t *gs)
{
    const Pipe &p = s->pipe[k];
    const size_t n = (size_t)s->fb.nx * s->fb.ny * s->fb.nz, es = s->fb.precision == 64 ? 8 : 4;
    const mceik_fsm_batch b = lang_batch(s, p, 0, m, s->D.slow_cur, s->L.tt0, (void *)s->D.slow_cur, s->d_ierr, s->d_ierr);
    mceik_fsm_adjoint a;
    memset(&a, 0, sizeof(a));
    a.batch = &b;
    a.grad = a.grad_solve = (double *)s->D.logl;      // (sizing only: one workgroup per solve)
    *u = up256((size_t)m * b.nstat * n * es);
    *fws = up256(mceik_fsm_workspace_bytes(&b));
    *aws = up256(mceik_fsm_adjoint_workspace_bytes(&a));
    *evw = up256((size_t)m * b.nstat * b.nev * sizeof(double));
    *gs = up256((size_t)m * b.nstat * s->D.ncell * sizeof(double));
    return *u + *fws + *aws + *evw + *gs;
}

// One Langevin step of pipe k: the step draw; at the current
// state, chunk by chunk, the forward with fields, the pick weights and the
// adjoint batch; the proposal; the same three at the proposed state (its
// tables are the step's, as after any velocity proposal); the reverse log q and
// the accept.  Everything is queued on the pipe's stream.
static int lang_step(mceik_mcmc *s, int k, uint64_t step, int slot)
{
    const Pipe &p = s->pipe[k];
    const LangPipe &lp = s->lang_pipe[k];
    const hipStream_t st = pipe_stream(s, k);
    const McmcDev &D = p.D;
    const LangDev &L = p.L;
    HIPCHK(lang_draw(D, L, step, st));
    for (int state = 0; state < 2; state++) {
        if (state) HIPCHK(lang_propose(D, p.B, p.P, s->prior_on, L, step, st));
        McmcDev W = D;                  // the pick weights read the state's tables of the drawn phase
        if (!state) W.ttab = L.tt0;
        for (int off = 0; off < D.nchains; off += lp.chunk) {
            const int m = std::min(lp.chunk, D.nchains - off);
            mceik_fsm_batch b = lang_batch(s, p, off, m, state ? D.slow_prop : D.slow_cur, (float *)W.ttab, lp.u,
                                           state ? L.ierr1 : L.ierr0, L.niter);
            if (fsm_batch_solve_impl(&b, lp.fws, lp.fws_bytes, st, nullptr)) return -1;
            HIPCHK(lang_weights(W, p.N, off, m, lp.ev_w, st));
            b.skip = s->fb.skip;        // the adjoint takes the sampler's skip rows
            mceik_fsm_adjoint a;
            memset(&a, 0, sizeof(a));
            a.batch = &b;
            a.u = lp.u;
            a.ev_w = lp.ev_w;
            a.grad = (state ? L.g1 : L.g0) + (size_t)off * D.ncell;
            a.grad_solve = lp.gsolve;   // a workgroup per solve; the model's rows are then summed in station order
            a.status = (state ? L.ast1 : L.ast0) + (size_t)off * D.nstat;
            if (mceik_fsm_adjoint_solve(&a, lp.aws, lp.aws_bytes, st)) return -1;
        }
    }
    s->last_ttab = s->fb.ttab;
    if (s->prior_on) {                  // the full integer energies of v and v' (prior.hip's kernel adds into zeroed words)
        const size_t ps = L.pen_stride, nb = (size_t)D.nchains * D.nphase * sizeof(unsigned long long);
        for (int q = 0; q < 4; q++) HIPCHK(hipMemsetAsync(L.pen + q * ps, 0, nb, st));
        McmcDev V = D;
        V.v = L.vprop;
        HIPCHK(prior_energy(D, p.B, p.P, L.pen, L.pen + ps, st));
        HIPCHK(prior_energy(V, p.B, p.P, L.pen + 2 * ps, L.pen + 3 * ps, st));
    }
    HIPCHK(lang_reverse(D, p.B, p.P, s->prior_on, L, st));
    HIPCHK(lang_accept(D, p.N, p.P, s->prior_on, L, slot, st));
    return 0;
}

// The pipes join the sampler's stream and fork again: everything queued on any
// pipe so far is ordered before everything queued on any pipe from here on.
static int pipes_join_fork(mceik_mcmc *s)
{
    const int np = s->npipe;
    if (np < 2) return 0;
    for (int k = 0; k < np; k++) {
        HIPCHK(hipEventRecord(s->pipe[k].join, s->pipe[k].st));
        HIPCHK(hipStreamWaitEvent(s->stream, s->pipe[k].join, 0));
    }
    HIPCHK(hipEventRecord(s->pfork, s->stream));
    for (int k = 0; k < np; k++) HIPCHK(hipStreamWaitEvent(s->pipe[k].st, s->pfork, 0));
    return 0;
}

// The proposals of a DE step, every pipe's.  A proposal reads
// the partners' models, which may be another pipe's chains: the pipes join and
// fork before it (a swap round of the same step has done that already), and no
// pipe goes on before every pipe's proposal has run, so nothing of this or a
// later step writes a model that a proposal still reads.
static int de_proposals(mceik_mcmc *s, uint64_t step, const StepPlan &q)
{
    const int np = s->npipe;
    if (!q.swap && pipes_join_fork(s)) return -1;
    for (int k = 0; k < np; k++) {
        const Pipe &p = s->pipe[k];
        HIPCHK(de_propose(p.D, p.H, p.De, step, q.de_par, q.de_ph, pipe_stream(s, k)));
    }
    if (pipes_join_fork(s)) return -1;
    s->de_last_ph = q.de_ph;
    return 0;
}

// The rest of pipe k's DE step: one forward of its movers' proposed models of
// phase ph (the compact batch: a standing chain costs no solve), the tables
// into the movers' rows of the step batch, the prior's full energies, the accept.
static int de_step(mceik_mcmc *s, int k, const StepPlan &q, int slot)
{
    const Pipe &p = s->pipe[k];
    const hipStream_t st = pipe_stream(s, k);
    const McmcDev &D = p.D;
    const DeDev &L = p.De;
    const int nmov = L.nmov[q.de_par];
    if (nmov > 0) {
        mceik_fsm_batch b = batch_view(p.fb, 0, nmov, (size_t)s->D.ncm);
        b.slow = L.slow;
        b.model_phase = nullptr;
        b.nphase = 1;
        b.skip = s->fb.skip ? s->fb.skip + (size_t)q.de_ph * D.nstat : nullptr;
        b.ttab = L.ttab;
        b.ierr = L.ierr;
        b.niter = L.niter;
        if (b.ev_stride > 0) {
            b.ev_node = L.ev;
            b.ev_stride = D.nev;
        }
        b.solve_order = nullptr;
        b.solve_clock = nullptr;
        b.max_waves = ws_layout(&p.fb).nwaves;      // it runs in the step batch's workspace
        if (mcmc_forward(s, true, k, nullptr, false, &b)) return -1;
        HIPCHK(de_scatter(D, L, q.de_par, st));
    }
    if (s->prior_on) {                  // the full integer energies of v and v' (prior.hip's kernel adds into zeroed words)
        const size_t ps = L.pen_stride, nb = (size_t)D.nchains * D.nphase * sizeof(unsigned long long);
        for (int i = 0; i < 4; i++) HIPCHK(hipMemsetAsync(L.pen + i * ps, 0, nb, st));
        McmcDev V = D;
        V.v = L.vprop;                  // (a standing chain's row is stale: its energies are never read)
        HIPCHK(prior_energy(D, p.B, p.P, L.pen, L.pen + ps, st));
        HIPCHK(prior_energy(V, p.B, p.P, L.pen + 2 * ps, L.pen + 3 * ps, st));
    }
    HIPCHK(de_accept(D, p.N, p.P, s->prior_on, L, q.de_par, q.de_ph, slot, st));
    return 0;
}

// Steps of one call.  Returns -1 on a HIP failure; the caller joins the pipes
// whatever happened, so the caller's stream is always ordered after every
// kernel this call queued on the internal streams.
static int mcmc_steps(mceik_mcmc *s, int nsteps)
{
    if (mcmc_multi_step(s)) {
        // the first step's proposals here, then up to MCEIK_MC_CHUNK steps per
        // FSM launch (the kernel accepts, keeps and proposes the rest)
        for (int done = 0; done < nsteps;) {
            int n = std::min(nsteps - done, MCEIK_MC_CHUNK);
            // an accumulator of kept states on: the launch ends right after the
            // next kept step, when every chain's current state is its state after that step
            if (kept_any_on(s)) n = (int)std::min<long long>(n, next_kept_step(s) - s->step + 1);
            // tempering: this step's swap round first; the launch ends before the next one
            const StepPlan q = plan_step(s, s->step);         // (a velocity step: mcmc_multi_step)
            if (q.swap && temper_round(s, q.parity)) return -1;
            if (s->ntemps > 1 && s->swap_every > 0)
                n = (int)std::min<long long>(n, (s->step / s->swap_every + 1) * s->swap_every - s->step);
            McmcExt x;
            x.dev = s->d_dev; x.sync = s->d_sync; x.spin_limit = s->spin_limit;
            x.step0 = (int)s->step; x.nsteps = n;
            x.nburn = s->nburn; x.keepk = s->keepk; x.maxs = s->max_samples; x.nkept0 = s->nkept;
            HIPCHK(mcmc_propose(s->D, (uint64_t)s->step, s->stream));
            if (mcmc_forward(s, true, 0, &x)) return -1;
            for (int i = 0; i < n; i++, s->step++)
                if (s->max_samples && kept_step(s, s->step)) s->nkept++;
            if (kept_step(s, s->step - 1)) {                   // one pipe: it views every chain
                if (kept_queue(s, s->pipe[0], s->stream)) return -1;
                kept_counted(s);
            }
            if (s->report) clock_report(s, "steps");
            done += n;
        }
        return 0;
    }
    const int np = s->npipe;
    const bool blk = s->block_on;
    for (int i = 0; i < nsteps; i++) {
        uint64_t step = (uint64_t)s->step;
        int slot = -1;
        const StepPlan q = plan_step(s, s->step);
        if (s->max_samples && q.kept) {
            slot = s->nkept % s->max_samples;
            s->nkept++;
        }
        if (q.swap) {
            // one round for the whole sampler on its own stream: the pipes join it
            // and fork again (their split need not fall on a group boundary)
            for (int k = 0; k < np && np > 1; k++) {
                HIPCHK(hipEventRecord(s->pipe[k].join, s->pipe[k].st));
                HIPCHK(hipStreamWaitEvent(s->stream, s->pipe[k].join, 0));
            }
            if (temper_round(s, q.parity)) return -1;
            if (np > 1) {
                HIPCHK(hipEventRecord(s->pfork, s->stream));
                for (int k = 0; k < np; k++) HIPCHK(hipStreamWaitEvent(s->pipe[k].st, s->pfork, 0));
            }
        }
        if (q.kind == STEP_DE && de_proposals(s, step, q)) return -1;
        for (int k = 0; k < np; k++) {
            const Pipe &p = s->pipe[k];
            const hipStream_t st = pipe_stream(s, k);
            switch (q.kind) {
            case STEP_HYPO:         // every event of every chain moves on one forward of the current models
                HIPCHK(hypo_propose(p.D, p.H, step, st));
                if (mcmc_forward(s, true, k, nullptr, true)) return -1;
                HIPCHK(hypo_accept(p.D, p.H, p.N, slot, st));
                break;
            case STEP_NUIS:         // nsub sub-moves per chain from the tables the chain holds: no forward
                HIPCHK(nuis_step(p.D, p.N, step, slot, st));
                break;
            case STEP_LANG:         // every cell of one model moves along its gradient: two forwards, two adjoints
                if (lang_step(s, k, step, slot)) return -1;
                break;
            case STEP_DE:           // half of every population moves a whole model along a difference of two others: one forward
                if (de_step(s, k, q, slot)) return -1;
                break;
            case STEP_VELOCITY:
                if (s->vor_on) {    // one move of the nuclei of one phase model: the raster, one forward
                    HIPCHK(vor_propose(p.D, p.V, step, q.vor_ph, st));
                    if (mcmc_forward(s, true, k)) return -1;
                    HIPCHK(vor_accept(p.D, p.V, p.N, q.vor_ph, slot, st));
                    s->vor_last_ph = q.vor_ph;
                    break;
                }
                HIPCHK(blk ? block_propose(p.D, p.B, step, st) : mcmc_propose(p.D, step, st));
                if (s->prior_on) HIPCHK(prior_fold(p.D, p.B, p.P, blk, st));
                if (mcmc_forward(s, true, k)) return -1;
                HIPCHK(blk ? block_accept(p.D, p.B, p.N, slot, st) : mcmc_accept(p.D, p.N, slot, st));
                break;
            }
            if (q.kept && kept_queue(s, p, st)) return -1;
        }
        if (q.kept) kept_counted(s);
        if (s->report) clock_report(s, "step");
        s->step++;
    }
    return 0;
}

extern "C" int mceik_mcmc_run(mceik_mcmc *s, int nsteps)
{
    if (!s) return 1;
    if (nsteps < 0) {
        const long long left = (long long)s->niter_total - s->step;
        nsteps = left > 0 ? (int)left : 0;
    }
    DeviceScope dg(s->device);
    const int np = s->npipe;
    if (np > 1) {                       // both pipes start after the caller's stream
        HIPCHK(hipEventRecord(s->pfork, s->stream));
        for (int k = 0; k < np; k++) HIPCHK(hipStreamWaitEvent(s->pipe[k].st, s->pfork, 0));
    }
    int rc = mcmc_steps(s, nsteps);
    if (np > 1) {                       // the caller's stream continues after every pipe, also on failure
        for (int k = 0; k < np; k++) {
            if (hipEventRecord(s->pipe[k].join, s->pipe[k].st) != hipSuccess ||
                hipStreamWaitEvent(s->stream, s->pipe[k].join, 0) != hipSuccess) {
                // cannot order the caller's stream after pipe k: wait for it here
                if (hipStreamSynchronize(s->pipe[k].st) != hipSuccess) rc = -1;
                rc = rc ? rc : -1;
            }
        }
    }
    return rc;
}

extern "C" int mceik_mcmc_finalize(mceik_mcmc **ps)
{
    if (!ps || !*ps) return 0;
    mceik_mcmc *s = *ps;
    DeviceScope dg(s->device);
    hipStreamSynchronize(s->stream);
    for (Pipe &p : s->pipe) {
        if (p.st) {
            hipStreamSynchronize(p.st);
            hipStreamDestroy(p.st);
        }
        if (p.join) hipEventDestroy(p.join);
    }
    if (s->pfork) hipEventDestroy(s->pfork);
    for (Pipe &p : s->pipe) if (p.ws_own && p.ws) hipFree(p.ws);
    for (LangPipe &lp : s->lang_pipe) if (lp.base) hipFree(lp.base);
    for (void *p : s->allocs) hipFree(p);
    for (KeptStream &k : s->kept) kept_state_free(k, k.state);
    for (int i = 0; i < 2 * s->ev_made; i++) hipEventDestroy(s->ev[i]);
    if (s->ws) hipFree(s->ws);
    delete s;
    *ps = nullptr;
    return 0;
}
