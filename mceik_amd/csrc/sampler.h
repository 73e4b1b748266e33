// sampler.h -- the per-GPU MCMC sampler's host state (include/mceik.h
// mceik_mcmc; not public), shared by sampler.hip (init, pipes, step plan, step
// loop, kept-state hook, finalize), sampler_api.hip (accessors, the entry
// points of the moves, the lifecycle of the kept-state accumulators) and the
// feature files that keep their state in it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <vector>

#include "../../include/mceik.h"
#include "block.h"
#include "cov.h"
#include "de.h"
#include "ess.h"
#include "fit.h"
#include "fsm_common.h"
#include "hypo.h"
#include "kept.h"
#include "lang.h"
#include "nuis.h"
#include "posterior.h"
#include "prior.h"
#include "vor.h"

#define MCEIK_EV_RING 32           // hipEvent pairs around timed FSM launches (fixed ring)
#define MCEIK_MAX_PIPES 4
#define MCEIK_ITERS_N (6 + MCEIK_TRAFFIC_N)   // d_iters: iterations, 4 visit statistics, solves, traffic

// A pipe: a part of the chains stepped on a stream of its own.  D, B, P, H, N, L, De, V, fb
// and fb_hyp are views of the sampler's restricted to the pipe's chains;
// pipes_refresh alone writes them.  (The accumulators of kept states,
// mceik_mcmc::kept, have no views: a KeptStream's accumulate takes the pipe's
// chain offset.)
struct Pipe {
    McmcDev D;
    BlockDev B;
    PriorDev P;
    HypoDev H;
    NuisDev N;
    LangDev L;                         // (arrays null before the first lang_enable)
    DeDev De;                          // (arrays null before the first de_enable)
    VorDev V;                          // (arrays null before the first vor_enable)
    mceik_fsm_batch fb;
    mceik_fsm_batch fb_hyp;            // a hypocentre step's batch (every model of the pipe's chains)
    void *ws;                          // the pipe's workspace: a part of the sampler's ws, ws itself, or its own
    size_t ws_bytes;
    bool ws_own;                       // ws was allocated for the pipe
    hipStream_t st;                    // made with more than one pipe only: one pipe steps on the sampler's stream
    hipEvent_t join;
};

struct mceik_mcmc {
    McmcDev D;
    hipEvent_t ev[2 * MCEIK_EV_RING];  // pairs around FSM launches (timing)
    int ev_made;                       // pairs created so far
    long long nlaunch;                 // timed launches since the last reset
    long long ev_folded;               // launches whose pair has been folded into fsm_ms
    double fsm_ms;                     // folded kernel time (ms)
    unsigned long long *d_iters;
    int *d_ierr;
    unsigned long long *d_clock;       // per-solve start/end stamps of the last launch (queue order, report)
    int *d_order;                      // longest-first queue order for the next launch (MCEIK_LPT=1), or null
    bool report;                       // MCEIK_SOLVE_CLOCK_REPORT=1
    // Two pipes (default; MCEIK_PIPES=1 turns them off): the chains run as two
    // halves on two streams of their own, each half's next FSM launch queued
    // behind its own accept, so one half's launch fills the waves the other
    // half's queue tail leaves idle.  Results are those of
    // one pipe bit for bit.  npipe >= 1 once init has set the pipes up: one pipe
    // is pipe[0] viewing every chain, with the sampler's workspace and stream.
    int npipe;
    Pipe pipe[MCEIK_MAX_PIPES];
    hipEvent_t pfork;
    // Multi-step launches (MCEIK_PERSIST=1, where the 16-z kernel runs): one
    // FSM launch runs up to MCEIK_MC_CHUNK steps, the
    // chain epilogue (accept, kept state, next proposal) inside the kernel
    // (fsm16_kernel.hip mc_finish), so no step waits for the slowest chain of
    // the one before.  d_dev: device copy of D; d_sync: the launch's queues.
    bool persist;
    unsigned spin_limit;               // multi-step launches: polls before a wait counts as a broken queue
    McmcDev *d_dev;
    unsigned *d_sync;
    mceik_fsm_batch fb;                // a step's batch: every chain's proposed model x stations
    mceik_fsm_batch fb_all;            // init / restore: every model of every chain (= fb with one model)
    const float *last_ttab;            // tables of the last forward (mceik_mcmc_last)
    int masked_s;                      // S picks ignored (nphase 1, mask_s)
    int device, max_samples, nburn, keepk, nkept, niter_total;
    int nkept_base;                    // nkept at the last restore: earlier states are not in the ring
    long long step;
    // The accumulators of kept states (kept.h): the streaming
    // posterior (s.10), the probe-to-cell covariances (s.16), the batch-means
    // sums (s.19) and the data-fit sums (s.20); all off by default.  While one
    // is on, a multi-step launch ends right after the next kept step.  The
    // posterior is on whenever it has state; the others keep their sums over a
    // disable.  While the data-fit sums are on, a one-model sampler holds its
    // current tables (D.ttab_cur = ttab_cur1, as with nuisance state) and takes
    // the per-step branch, whose accept copies them.
    KeptStream kept[KEPT_NSTREAM];
    // Parallel tempering (temper.hip); ntemps = 0: off.  Rung r
    // of replica group g is chain r * G + g (G = nchains / ntemps), so the cold
    // chains are [0, G).  plan_step (sampler.hip) says which steps a swap round
    // precedes, and its parity.
    int ntemps, swap_every;
    std::vector<double> beta;          // the ladder [ntemps]
    double *d_beta;                    // [nchains] the chains' beta (D.beta while ntemps > 1)
    int *d_tflag;                      // [nchains] the round's swap flag per pair
    unsigned long long *d_tcnt;        // [2][nchains] attempts, accepts per rung pair
    // Block proposals (block.hip); off by default.  B holds the
    // cell grid from init on; while on, every step takes the per-step branch
    // with block.hip's two kernels in place of propose / accept.
    bool block_on;
    BlockDev B;
    unsigned long long *d_bcnt;        // [2][MCEIK_BLOCK_RMAX + 1] attempts, accepts by radius
    // Smoothness / reference-model prior (prior.hip); off by
    // default.  While on, every step takes the per-step branch with
    // prior_fold between the proposal and the forward.
    bool prior_on;
    PriorDev P;
    bool prior_vref;                   // a reference model is loaded (P.vref == d_vref)
    int *d_vref;                       // [nphase][ncell]
    unsigned long long *d_pen;         // [2][nchains * nphase] Es, Ed of mceik_mcmc_prior_energy
    // Hypocentre moves (hypo.hip); off by default.  H.hyp is
    // null until the first enable, which starts every chain at the catalogue's
    // snapped nodes (ev_host) and switches fb / fb_all to per-chain event lists
    // (ev_stride); the positions then stay per chain, also after disable.
    // While on, every step takes the per-step branch; plan_step says which
    // steps are hypocentre steps.
    bool hypo_on;
    int hypo_every;
    HypoDev H;
    mceik_fsm_batch fb_hyp;            // fb_all on slow_cur with the [current | candidate] lists, tables into H.ttab2
    std::vector<int> ev_host;          // [nev] the catalogue's snapped nodes
    int tt_interp;                     // trilinear mode (hypocentre moves are refused)
    unsigned long long *d_hcnt;        // [2][nev] attempts, accepts
    long long hyp_n;                   // states in the moments (cold chains x kept steps)
    // Noise-scale and station-static moves (nuis.hip); off by
    // default.  N.kn is null until an enable and again after a clear: while it
    // is set the sampler holds nuisance state, every step takes the per-step
    // branch, every logL honours the state, and a one-model sampler keeps its
    // current tables too (D.ttab_cur = ttab_cur1, which the full forward then
    // fills).  plan_step says which steps are nuisance steps.
    bool nuis_on;
    int nuis_every, nuis_offset;
    NuisDev N;
    NuisDev Nbuf;                      // the arrays of the first enable, kept across clear
    int nuis_cap_sub, nuis_cap_nk;     // sub-moves / ladder entries the arrays hold
    float *ttab_cur1;                  // one model: [nchains][nstat][nev] current tables while N.kn is set or the data-fit sums are on
    long long nuis_n;                  // states in the moments (cold chains x kept steps)
    std::vector<int> h_ostat, h_omask, h_ophase;   // [nobs] the observations' station, mask and phase (host copies)
    // Discrete Langevin moves (lang.hip); off by default.  L's
    // arrays are null until the first enable, which allocates everything a step
    // uses: the per-chain arrays, and per pipe (lang_pipe) the fields, the
    // workspaces of the forward with fields and of the adjoint, and the pick
    // weights, sized to lang_mem.  While on, every step takes the per-step
    // branch; plan_step says which steps are Langevin steps.
    bool lang_on;
    int lang_every, lang_offset;
    double lang_sigma;
    size_t lang_mem;
    LangDev L;
    LangPipe lang_pipe[MCEIK_MAX_PIPES];
    // Differential-evolution moves (de.hip); off by default.
    // De's arrays are null until the first enable, which allocates everything a
    // step uses.  While on, every step takes the per-step branch; plan_step says
    // which steps are DE steps, their parity and their phase.  d_demov: both
    // parities' mover lists of the whole sampler, ascending (de_lists rebuilds
    // them when the populations change: enable, tempering on / off); a pipe's
    // lists are the parts that fall on its chains.
    bool de_on;
    int de_every, de_offset;
    DeDev De;
    int *d_demov;                      // [2][nchains]
    std::vector<int> de_mov[2];        // the host's copy
    int de_last_ph;                    // the last DE step's phase (-1: none yet)
    // Voronoi-cell models (vor.hip); off by default.  V's arrays
    // are null until the first enable.  While on, every chain's v is the raster
    // of its nuclei, every step takes the per-step branch and every velocity
    // step is a Voronoi step: vor.hip's kernels in place of propose / accept.
    // plan_step says which phase a step works on.
    bool vor_on;
    int vor_k0;                        // the start count of the last enable (reported only)
    VorDev V;
    int vor_last_ph;                   // the last Voronoi step's phase (-1: none yet)
    long long vor_n;                   // states in the moments (cold chains x kept steps)
    hipStream_t stream;
    void *ws;
    size_t ws_bytes;
    std::vector<void *> allocs;
};

template <typename T>
static int dalloc(mceik_mcmc *s, T **p, size_t count)
{
    void *q = nullptr;
    if (hipMalloc(&q, count * sizeof(T) + 16) != hipSuccess) return -1;
    hipMemset(q, 0, count * sizeof(T) + 16);
    s->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}

template <typename T>
static int dput(mceik_mcmc *s, T **p, const T *host, size_t count)
{
    if (dalloc(s, p, count)) return -1;
    if (count && hipMemcpy(*p, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return -1;
    return 0;
}

// sampler.hip, as sampler_api.hip uses it
int fold_launch(mceik_mcmc *s, long long k);
int mcmc_forward_all(mceik_mcmc *s);
int check_forward_ierr(mceik_mcmc *s, const char *who);
int temper_cold(const mceik_mcmc *s);
int temper_round(mceik_mcmc *s, int parity);
// The sampler runs multi-step launches now.  It was built for them (persist:
// one pipe), and no feature that needs a launch per step is on: block
// proposals (the multi-step kernel's epilogue is single-cell); the prior (its
// fold sits between a step's proposal and its forward); hypocentre moves (a
// hypocentre step has kernels and a batch of its own); held nuisance state (it
// enters every logL, which the multi-step kernel's epilogue does not know);
// Langevin moves and DE moves (such a step is a pipeline of launches of its own);
// Voronoi-cell models (a velocity step rasters the proposed nuclei before its
// forward, and the multi-step kernel's epilogue knows no nuclei); the
// data-fit sums of a one-model sampler (they read the chains' current tables,
// which the multi-step kernel's epilogue keeps for two models only); the L1
// likelihood (the multi-step kernel's epilogue evaluates the L2 misfit only).
static inline bool kept_needs_tables1(const mceik_mcmc *s)     // an accumulator that reads the current tables is on
{
    for (const KeptStream &k : s->kept)
        if (k.on && k.needs_tables1) return true;
    return false;
}
static inline bool mcmc_multi_step(const mceik_mcmc *s)
{
    return s->persist && !s->block_on && !s->prior_on && !s->hypo_on && !s->N.kn && !s->lang_on && !s->de_on && !s->vor_on &&
           !(kept_needs_tables1(s) && s->D.nphase == 1) && !s->D.l1;
}
// A one-model sampler's current tables (sampler_api.hip).  hold: while nuisance
// state is held or the data-fit sums are on, D.ttab_cur = ttab_cur1 (allocated
// on first need); when they were not held yet, one full forward fills them
// (logL is recomputed from them: the same value).  drop: once neither needs
// them, the sampler is the plain one again.  Both synchronise; two models: no-ops.
int mcmc_tables1_hold(mceik_mcmc *s, const char *who);
int mcmc_tables1_drop(mceik_mcmc *s);
// The lifecycle of a kept-state accumulator k of s (sampler_api.hip), behind
// the four files' entry points.  kept_enable_held is enable's tail once the
// options are valid, `same` saying that the held state has them.  It returns
// what enable returns when the call is decided (the held sums go on: 0 or
// mcmc_tables1_hold's code; held states of other options are refused: 1; a
// HIP failure: -1), or KEPT_REPLACE once the old state is gone (synchronised,
// freed): the caller builds its state, allocates its arrays and ends with
// kept_publish, or frees a failed one with kept_state_free.
#define KEPT_REPLACE (-2)
int kept_enable_held(mceik_mcmc *s, KeptStream &k, bool same, const char *who);
int kept_publish(mceik_mcmc *s, KeptStream &k, void *state, const char *who);
void kept_state_free(KeptStream &k, void *state);
int kept_disable(mceik_mcmc *s, KeptStream &k);                 // stop adding; the sums stay
int kept_clear(mceik_mcmc *s, KeptStream &k);                   // drop the state (synchronises)
int kept_accumulate(mceik_mcmc *s, KeptStream &k);              // the cold chains' current state, now
int kept_get(mceik_mcmc *s, KeptStream &k, long long *n, void *const *host);
int kept_set(mceik_mcmc *s, KeptStream &k, long long n, const void *const *host);
// Bytes pipe k's Langevin step needs for chunks of m chains: the fields (u), the
// workspaces of the forward with fields (fws) and of the adjoint (aws), the
// pick weights (evw) and the adjoint's per-solve rows (gs), each a multiple of
// 256; returns their sum.
size_t lang_pipe_bytes(const mceik_mcmc *s, int k, int m, size_t *u, size_t *fws, size_t *aws, size_t *evw, size_t *gs);
// The DE mover lists for the populations in force (G = temper_cold); uploads
// them and refreshes the pipes.  No-op before the first de_enable.  Synchronises.
int de_lists(mceik_mcmc *s);
// Recomputes every pipe's D, B, P, H, N, L, De, V and fb from the sampler's (and a multi-step
// sampler's device copy of D): call after any change to s->D, s->B, s->P, s->H, s->N, s->L, s->De, s->V or s->fb.
int pipes_refresh(mceik_mcmc *s);
