/*
 * mceik.h -- MCMC travel-time tomography driver API (libmceik_hip.so, gfx950).
 *
 * The reference's include/mceik.h:1-14 declares nothing; its data model
 * (mceik_struct.h) is kept and this header fills the driver slot that
 * homog.c:343-415 occupies.  One process drives one GPU; an MPI harness
 * passes its rank/size and shards chains.  Every function
 * returns 0 on success (h5io.c convention).
 */
#ifndef _mceik_h__
#define _mceik_h__ 1   /* the reference's guard (include/mceik.h:1-2): this header replaces it */
#include <stdint.h>
/* the reference's mceik.h pulls in <mpi.h> and "os.h" (include/mceik.h:3-4):
 * a harness built with an MPI compiler gets the MPI declarations from here as
 * before; the library itself needs no MPI at build or link time */
#if defined(__has_include)
#if __has_include(<mpi.h>)
#include <mpi.h>
#endif
#endif
#include "os.h"
#include "mceik_struct.h"
#include "mceik_eikonal.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mceik_mcmc mceik_mcmc;   /* opaque per-GPU sampler */

/* Sampler options beyond mceik_parms_struct. */
typedef struct mceik_mcmc_opts {
    int nx, ny, nz;            /* eikonal grid (parms->dx = dy = dz = h)     */
    int nchains;               /* chains on this GPU                         */
    int chain_offset;          /* global id of the first chain (rank shard)  */
    int vmin, vmax;            /* uniform prior on cell velocity (m/s)       */
    int dvmax;                 /* proposal: +-[1, dvmax] m/s on one cell     */
    uint32_t seed;             /* Philox key                                 */
    int max_samples;           /* device sample ring capacity (states)       */
    int device;                /* HIP device ordinal                         */
    int precision;             /* FSM arithmetic: 32 (0 = default) or 64; tables are fp32 at rest
                                  either way (fsm3d.f90:1855-1875)           */
    int max_waves;             /* cap on resident FSM waves (0 = occupancy x CUs) */
    int tt_interp;             /* event travel times: 0 = value at the event's nearest node (the
                                  reference's snapping, fsm3d.f90:697-711); 1 = trilinear
                                  interpolation in the event's grid cell (mceik_fsm_batch.ev_frac) */
    int nphase;                /* velocity models per chain: 1 (or 0) = P only; 2 = joint P and S
                                  (homog.c:208-258 makes both; the catalog's pickType selects the
                                  model an observation is fit against, mceik_struct.h:4-8)   */
    int vsmin, vsmax;          /* nphase 2: uniform prior on S cell velocity (m/s)          */
    int mask_s;                /* nphase 1 and the catalog holds used S picks: 0 = init fails
                                  (naming the count), 1 = fit the P picks and ignore the S picks */
} mceik_mcmc_opts;

/* What mceik_mcmc_init set up (diagnostic; mceik_mcmc_info). */
typedef struct mceik_mcmc_info {
    int npipe;                 /* chain groups on streams of their own (1 = one FSM launch per step) */
    int nphase;                /* velocity models per chain (1 = P, 2 = P and S)              */
    int step_z;                /* z nodes per macro step of the sampler's FSM kernel (16 or 8) */
    int fixed_layout;          /* 1: the compile-time LDS layout instance                   */
    int chains[4];             /* chains of pipe k (k < npipe)                               */
    int waves[4];              /* resident FSM waves of pipe k's launch                     */
    size_t workspace_bytes[4]; /* FSM scratch of pipe k                                     */
    size_t lds_bytes;          /* LDS per FSM wave                                           */
    int masked_s;              /* S observations ignored (nphase 1 with mask_s = 1)          */
    char kernel[64];           /* the FSM kernel instance (rocprof name)                    */
    int multi_step;            /* 1: one FSM launch runs up to 64 steps, no barrier between
                                  them (the chain epilogue in the kernel; default when a step
                                  is <= 4 solves per wave, MCEIK_PERSIST=1/0 forces);
                                  0: per-step propose / FSM / accept launches               */
} mceik_mcmc_info;

/* ---- run configuration (host only; csrc/parms.c) ----------------------
 * The reference's mains hard-code their parameters (homog.c:73-89,
 * fsm3d.f90:2085-2100); these fill mceik_parms_struct (mceik_struct.h:68-90)
 * and the sampler options from an INI file ([general] projnm scratch_dir;
 * [grid] x0 y0 z0 dx dy dz nx ny nz ndivx ndivy ndivz nrefx nrefy nrefz
 * tt_interp; [eikonal] tol maxit precision max_waves; [mcmc] resdir nburnIn
 * niter keepK nchains chain_offset vmin vmax dvmax seed max_samples device),
 * names case-insensitive, ';'/'#' comments.  Either record pointer may be NULL. */
/* homog.c's grid (32 x 29 x 26 nodes at 1 km), tol 1e-8, maxit 50, seed 2016. */
int mceik_parms_defaults(struct mceik_parms_struct *parms, mceik_mcmc_opts *opts);
/* key "section:name": 0 ok, 1 unknown key, 2 invalid value (message on stderr). */
int mceik_parms_set(struct mceik_parms_struct *parms, mceik_mcmc_opts *opts, const char *key, const char *value);
/* 0 ok, -1 cannot open, > 0 the line number of the first bad line. */
int mceik_parms_read(const char *path, struct mceik_parms_struct *parms, mceik_mcmc_opts *opts);
/* Applies [--]section:key=value arguments and --config FILE / --config=FILE
 * (in argument order, argv[0] skipped); returns the count consumed or -1. */
int mceik_parms_args(int argc, char **argv, struct mceik_parms_struct *parms, mceik_mcmc_opts *opts);
/* Writes every key back in INI form (0 ok). */
int mceik_parms_write(const char *path, const struct mceik_parms_struct *parms, const mceik_mcmc_opts *opts);

/* v0: host [nchains][nphase][ncell] int m/s (P model, then S model when
 * nphase = 2), ncell = ceil(nx/nrefx)*ceil(ny/nrefy)*ceil(nz/nrefz), cell
 * index x fastest.  Computes each chain's initial logL.  Stations need
 * Cartesian coordinates (lcartesian = 1); a station gets a P table only when
 * lhasP[k] and an S table only when lhasS[k] is set (NULL arrays: every
 * station), the other solves are skipped.  Returns 1 on invalid arguments
 * (lcartesian != 1, a used pick at a station without its phase flag, used S
 * picks with nphase 1 unless mask_s), 2 when a station's solve fails (the
 * reference's ierr), -1 on a device failure.  A failed multi-step queue
 * (mceik_mcmc_get_info multi_step) is reported as -1 by the next
 * synchronising call (sync, get_state, get_samples, checkpoint).
 * Every array below sized [nchains][ncell] is [nchains][nphase][ncell]. */
int mceik_mcmc_init(const struct mceik_parms_struct *parms,
                    const struct mceik_stations_struct *stations,
                    const struct mceik_catalog_struct *catalog,
                    const mceik_mcmc_opts *opts, const int *v0, mceik_mcmc **out);
/* Enqueue nsteps proposals for every chain (propose -> FSM -> misfit ->
 * Metropolis); keeps states per mcparms (nburnIn, keepK). Asynchronous.
 * nsteps < 0: run the remaining mcparms.niter - step proposals (mceik_struct.h:58). */
int mceik_mcmc_run(mceik_mcmc *s, int nsteps);
int mceik_mcmc_set_stream(mceik_mcmc *s, void *stream);
int mceik_mcmc_sync(mceik_mcmc *s);
/* Host copies of the chain state. Any pointer may be NULL. */
int mceik_mcmc_get_state(mceik_mcmc *s, int *v, double *logl, long long *naccept, long long *step);
/* Kept samples: copies the n = min(max, kept, max_samples) most recent kept
 * states, oldest first, into v_out [n][nchains][ncell] and logl_out
 * [n][nchains] (both host memory for kind 0, both device memory for kind 1);
 * returns n in *nkept. */
int mceik_mcmc_get_samples(mceik_mcmc *s, void *v_out, double *logl_out, int max, int kind, int *nkept);
/* Diagnostics of the last step: device pointers to the travel-time table
 * [nchains][nstat][nev] (fp32), per-solve iteration counts and reference ierr
 * [nchains][nstat] (int), and accept flags [nchains].  With nphase 2 a step
 * re-solves only the model its proposal changed: the tables are that phase's
 * (mceik_mcmc_last_phase); after init they are [nchains][nphase][nstat][nev]
 * and niter/ierr [nchains][nphase][nstat].  Any pointer may be NULL. */
int mceik_mcmc_last(mceik_mcmc *s, const float **ttab, const int **niter, const unsigned char **accept,
                    const int **ierr);
/* Device pointer to the last step's proposed phase per chain [nchains] (0 = P, 1 = S). */
int mceik_mcmc_last_phase(mceik_mcmc *s, const int **phase);
/* Fills *info (host). */
int mceik_mcmc_get_info(mceik_mcmc *s, mceik_mcmc_info *info);
/* Checkpoint / resume.  The proposal RNG is Philox keyed by (global chain,
 * step), so (v, logl, naccept, step, nkept) is the complete chain state:
 * restoring it into a sampler built with the same problem, seed and chain
 * shard continues the chains bit for bit.  checkpoint: host copies
 * (synchronises; any pointer may be NULL).  restore: host arrays for this
 * sampler's chains; logl == NULL recomputes it with one forward. */
int mceik_mcmc_checkpoint(mceik_mcmc *s, int *v, double *logl, long long *naccept, long long *step, int *nkept);
int mceik_mcmc_restore(mceik_mcmc *s, const int *v, const double *logl, const long long *naccept,
                       long long step, int nkept);
/* FSM accounting since init (or the last reset): kernel time of every FSM
 * launch from hipEvents on the sampler's stream (ms), launches, and the
 * sum over solves of executed iterations (8 sweeps each) and visits[4] = brick
 * visits (8x8x8 nodes in one sweep; unchanged z-blocks are skipped), column
 * segments updated, segments changed, wave macro steps (mceik_fsm_batch.visit_stats).
 * Synchronises. */
int mceik_mcmc_fsm_stats(mceik_mcmc *s, double *fsm_ms, long long *nlaunch, unsigned long long *iters,
                         unsigned long long *visits, int reset);
/* Solves executed since init (or the last fsm_stats reset): solves of a
 * station without picks of the solve's phase are skipped (lhasP / lhasS,
 * homog.c:313-335) and not counted.  Synchronises. */
int mceik_mcmc_fsm_solves(mceik_mcmc *s, unsigned long long *solves);
int mceik_mcmc_finalize(mceik_mcmc **s);

/* ---- streaming posterior (csrc/posterior.hip) -------------
 * A run's kept states do not fit anywhere at production sizes, so a sampler
 * can summarise them as it goes.  Cell velocities are integers: per model
 * entry (ncm = nphase * ncell of them) the sampler keeps the exact integer
 * sums of v and v^2 over the accumulated states and a histogram, so the
 * result does not depend on the order of accumulation and shards or ranks
 * merge by plain addition.  Off by default; with it off nothing changes.
 *
 * per_chain = 1: sum, sumsq are [nchains][ncm] (needed for R-hat; 16 bytes per
 * chain and entry).  per_chain = 0: [ncm], pooled over the chains.  nbins in
 * [0, 128]: hist is [ncm][nbins] uint32 pooled over the chains (0: none; a
 * count wraps past 2^32 - 1 = nchains x states); a value v of phase ph falls
 * in bin clamp((long long)(v - lo) * nbins / (hi - lo + 1), 0, nbins - 1),
 * (lo, hi) = (vmin, vmax) for P and (vsmin, vsmax) for S, in integers.
 *
 * While enabled, mceik_mcmc_run adds every chain's state after step gs when
 * gs >= nburnIn && (gs - nburnIn) % keepK == 0 -- the rule of the kept states,
 * whatever max_samples is (0 included) -- by a kernel queued behind the
 * step: no host synchronisation.  The chains are bit for bit those of a run
 * with the posterior off.  Cost with multi-step launches
 * (mceik_mcmc_info.multi_step): a launch then ends right after the next kept
 * step: keepK = 1 means one step per launch (C2: -18% proposals/s, keepK = 8
 * -4%); a large keepK adds one launch boundary per kept step.
 *
 * Every function returns 0, 1 on invalid arguments (posterior not enabled,
 * nbins out of range, partials that do not match) or -1 on a device failure. */
typedef struct mceik_posterior_opts { int per_chain; int nbins; } mceik_posterior_opts;
typedef struct mceik_posterior_partials {      /* caller-allocated host arrays */
    int ncm, nbins, per_chain;
    long long nchains, nkept;                  /* chains summed, states per chain */
    long long *S;                              /* [ncm] sum over chains of sum */
    unsigned long long *Q, *P;                 /* [ncm][2] = lo, hi words: sum over chains of sumsq, of sum^2 */
    unsigned long long *hist;                  /* [ncm][nbins], widened for merging */
} mceik_posterior_partials;
/* Allocates and zeroes the accumulators; on an enabled sampler: resets them
 * (with other options: reallocates). */
int mceik_mcmc_posterior_enable(mceik_mcmc *s, const mceik_posterior_opts *o);
int mceik_mcmc_posterior_disable(mceik_mcmc *s);
/* Adds the chains' current state now (enqueued on the sampler's stream). */
int mceik_mcmc_posterior_accumulate(mceik_mcmc *s);
/* Host copies of / replacements for the accumulators (checkpoints): n states
 * per chain, sum and sumsq [nchains][ncm] or [ncm], hist [ncm][nbins].  get
 * synchronises, any pointer may be NULL; set needs sum, sumsq, and hist when
 * nbins > 0. */
int mceik_mcmc_posterior_get(mceik_mcmc *s, long long *n, long long *sum, long long *sumsq, unsigned *hist);
int mceik_mcmc_posterior_set(mceik_mcmc *s, long long n, const long long *sum, const long long *sumsq,
                             const unsigned *hist);
/* The chain axis summed on the device into exact partials: S = sum_c sum_c,
 * Q = sum_c sumsq_c, P = sum_c sum_c^2 (128 bits; pooled mode: P = 0).  Fills
 * every scalar of *out and the arrays it points to (hist only when nbins > 0).
 * Synchronises. */
int mceik_mcmc_posterior_partials(mceik_mcmc *s, mceik_posterior_partials *out);
/* Host only (no GPU call).  merge: dst += src; 1 unless ncm, nbins, per_chain
 * and nkept agree.  finish: with M = nchains, n = nkept, N = M n every
 * numerator is an exact 128-bit integer converted to double once, then
 *   mean = S / N,   var = (N Q - S^2) / (N (N - 1)),
 *   W = (n Q - P) / (M n (n - 1)),   B/n = (M P - S^2) / (M (M - 1) n^2),
 *   rhat = sqrt(((n - 1)/n W + B/n) / W)
 * (pooled sample variance; Gelman-Rubin potential scale reduction).  rhat is
 * NaN when per_chain = 0, M < 2, n < 2 or the W numerator is 0 (no variance
 * within any chain); var is NaN when N < 2, mean when N = 0.  mean, var, rhat:
 * [ncm], any may be NULL. */
int mceik_posterior_merge(mceik_posterior_partials *dst, const mceik_posterior_partials *src);
int mceik_posterior_finish(const mceik_posterior_partials *p, double *mean, double *var, double *rhat);

/* ---- parallel tempering / replica exchange (csrc/temper.hip)
 * Off by default; with it off nothing changes.  A sampler of nchains chains
 * and ntemps rungs (nchains % ntemps == 0) holds G = nchains / ntemps replica
 * groups; rung r of group g is local chain r * G + g, so the cold chains
 * (beta = 1) are the local chains [0, G) = the global chains chain_offset +
 * [0, G).  Groups never span ranks.  A chain index never changes its rung:
 * swaps exchange states, not temperatures, so kept samples, get_state, gather,
 * naccept and per-chain posterior rows keep their meaning (cold = the first G
 * chains of each shard; naccept[c] counts at chain c's temperature).
 *
 * Ladder: beta[ntemps] with beta[0] == 1.0 exactly and 0 < beta[r+1] <=
 * beta[r]; ntemps = 1 is the untempered sampler.  Chain c accepts a proposal
 * inside the prior iff log u < beta[c / G] * (logL' - logL) (one fp64
 * multiply; the uniform prior is not tempered).
 *
 * Swaps: with K = swap_every > 0, before the proposal of global step gs > 0
 * with gs % K == 0 a swap round runs; it belongs to step gs (a checkpoint
 * taken at step == gs has not done it, the resumed run does it first).
 * parity = (gs / K) & 1; every group g and rung r with r % 2 == parity and
 * r + 1 < ntemps forms the pair a = r * G + g, b = a + G, draws Philox4x32-10
 * with counter {(uint32)gs, (uint32)(gs >> 32), 1, 0} and key {chain_offset +
 * a, seed} (the proposals use counter word 2 = 0), log u = log((out[0] + 0.5)
 * / 2^32) by the sampler's deterministic log, and swaps iff
 *   log u < (beta[r] - beta[r+1]) * (logL[b] - logL[a]).
 * A swap exchanges the two chains' models, logL and the hidden state that
 * goes with them; naccept stays.  attempts[r] / accepts[r] count per rung pair.
 * Both kernels are queued on the sampler's stream: no host synchronisation.
 * With multi-step launches (mceik_mcmc_info.multi_step) a launch ends before
 * the next swap step.
 *
 * While tempering is on the streaming posterior sees the cold chains only
 * (partials.nchains = G; the accumulators keep their [nchains][ncm] shape, the
 * hot rows stay zero); enable / disable return 1 while an enabled posterior
 * holds states.  The kept ring and mceik_mcmc_gather keep every chain.
 *
 * Every function returns 0, 1 on invalid arguments (not enabled, parity not 0
 * or 1, a bad ladder, nchains % ntemps != 0) or -1 on a device failure. */
typedef struct mceik_temper_opts { int ntemps; int swap_every; const double *beta; } mceik_temper_opts;
/* Turns tempering on (or replaces the ladder); resets the counters. */
int mceik_mcmc_temper_enable(mceik_mcmc *s, const mceik_temper_opts *o);
int mceik_mcmc_temper_disable(mceik_mcmc *s);
/* The options in force; beta [ntemps] or NULL. */
int mceik_mcmc_temper_get(mceik_mcmc *s, int *ntemps, int *swap_every, double *beta);
/* attempts, accepts [ntemps - 1] (either may be NULL).  Synchronises. */
int mceik_mcmc_temper_stats(mceik_mcmc *s, long long *attempts, long long *accepts, int reset);
/* One swap round now, Philox counter = the current step; enqueued. */
int mceik_mcmc_temper_swap(mceik_mcmc *s, int parity);
/* Host only: the geometric ladder beta[r] = tmax^(-r / (ntemps - 1)), beta[0]
 * = 1 exactly (ntemps >= 1, finite tmax >= 1, else 1). */
int mceik_temper_ladder(int ntemps, double tmax, double *beta);

/* ---- multi-cell (block) proposals (csrc/block.hip) --------
 * Off by default; with it off nothing changes.  A block proposal moves a
 * smooth neighbourhood of inversion cells of one model at once; the forward
 * costs the same.  Options: radii rmin, rmax in inversion cells, 0 <= rmin <=
 * rmax <= 8.
 *
 * Draw: the single-cell draw unchanged -- Philox4x32-10, counter {(uint32)step,
 * (uint32)(step >> 32), 0, 0}, key {global chain, seed}, outputs r0..r3; centre
 * cell = (r0 * ncm) >> 32 over the chain's [nphase][ncell] entries, phase =
 * cell / ncell, mag = 1 + ((r1 * dvmax) >> 32), sign = r2 & 1 (1 = minus), U
 * from r3 -- plus the radius R = rmin + (((uint64)(r2 >> 1) * (rmax - rmin +
 * 1)) >> 31).
 *
 * Footprint: with (cx, cy, cz) the centre within its model (cell % ncell, x
 * fastest), every offset (dx, dy, dz) in [-R, R]^3 whose target lies inside
 * [0, ncx) x [0, ncy) x [0, ncz) moves by
 *   dv = ((int64)mag * w) / (R+1)^3,  w = (R+1-|dx|) (R+1-|dy|) (R+1-|dz|)
 * (integer floor of non-negative operands; the sign is applied afterwards);
 * entries with dv == 0 are not touched.  The footprint is clipped at the grid
 * faces and never leaves the phase's model.  R = 0 is the single-cell
 * proposal, bit for bit.
 *
 * The proposal is inside the prior iff every touched entry's new value is
 * within its phase's bounds; otherwise it is rejected (the forward still
 * runs).  The accept rule is unchanged, tempering's beta included; no Hastings
 * term is needed: the move with the same centre, mag and R and the opposite
 * sign is drawn with equal probability and its dv are the exact negations.
 *
 * While enabled every step is one launch of each kernel (a sampler built for
 * multi-step launches steps per launch: mceik_mcmc_info.multi_step reports 0
 * until disable); swap rounds and the streaming posterior run as on the
 * per-step path.  mceik_mcmc_last's accept flags and mceik_mcmc_last_phase
 * keep their meaning.  attempts[R] / accepts[R] count the proposals of radius
 * R and the accepted ones.
 *
 * Every function returns 0, 1 on invalid arguments (NULL, radii out of range,
 * not enabled) or -1 on a device failure. */
typedef struct mceik_block_opts { int rmin, rmax; } mceik_block_opts;
/* Turns block proposals on (or replaces the radii); resets the counters.  Synchronises. */
int mceik_mcmc_block_enable(mceik_mcmc *s, const mceik_block_opts *o);
/* Later steps are single-cell again; the counters stay until the next enable. */
int mceik_mcmc_block_disable(mceik_mcmc *s);
/* The radii in force (either may be NULL). */
int mceik_mcmc_block_get(mceik_mcmc *s, int *rmin, int *rmax);
/* attempts, accepts [rmax + 1], by radius (either may be NULL).  Synchronises. */
int mceik_mcmc_block_stats(mceik_mcmc *s, long long *attempts, long long *accepts, int reset);
/* Host only: the footprint of one proposal of signed amplitude amp (the
 * centre's dv, != 0) and radius 0..8 centred on `cell` of an ncx x ncy x ncz
 * model: the touched cells in x-fastest order of the offsets and their dv
 * (each up to (2 radius + 1)^3 entries; either may be NULL).  Returns the
 * touched count, -1 on invalid arguments. */
int mceik_block_footprint(int ncx, int ncy, int ncz, int cell, int radius, int amp, int *cells, int *dv);

/* ---- smoothness and reference-model prior (csrc/prior.hip) -
 * Off by default; with it off nothing changes.  Besides the uniform box every
 * chain's phase model (ncx x ncy x ncz inversion cells, x fastest) then carries
 * two exact integer energies:
 *   roughness Es = sum over face-adjacent cell pairs (i, j) of (v_i - v_j)^2
 *             (pairs never join the P and the S model),
 *   damping   Ed = sum_i (v_i - vref_i)^2 against vref[nphase * ncell], one
 *             reference model shared by all chains (vref NULL: Ed = 0),
 * and log prior = -(w_smooth[ph] Es + w_damp[ph] Ed): a Gaussian Markov random
 * field truncated to the box.  The weights are finite and >= 0, w = 1 / (2
 * sigma^2) with sigma in m/s; [0] is the P model's, [1] the S model's.
 *
 * Accept rule: for a pending proposal inside the box that touches phase ph,
 * with dEs = Es(v') - Es(v) and dEd likewise (exact integers),
 *   dlp = -(w_smooth[ph] * (double)dEs + w_damp[ph] * (double)dEd)
 *   thr = log u - dlp
 *   accept iff thr < logL' - logL     (tempering: thr < beta * (logL' - logL);
 *                                      the prior is not tempered)
 * in IEEE double without contraction.  With all weights zero thr == log u and
 * the sampler is the plain one bit for bit.  Tempering's swap rule does not
 * change: both replicas carry the untempered prior, which cancels.  logL and
 * the kept logL stay the likelihood.
 *
 * enable refuses (1) a sampler where 3 ncell (hi - lo + 2 dvmax)^2 >= 2^53 for
 * a phase's box [lo, hi] (below that every energy and difference converts to
 * double exactly), a vref entry outside its phase's box, and a weight that is
 * negative or not finite.  While enabled every step is one launch
 * (mceik_mcmc_info.multi_step reports 0 until disable), with one more kernel
 * between the proposal and the forward; a run gains no host synchronisation.
 * enable / disable return 1 while an enabled posterior holds states.
 *
 * Every function returns 0, 1 on invalid arguments (NULL, not enabled, the
 * refusals above) or -1 on a device failure. */
typedef struct mceik_prior_opts { double w_smooth[2], w_damp[2]; const int *vref; } mceik_prior_opts;
/* Turns the prior on (or replaces the weights and vref).  Synchronises. */
int mceik_mcmc_prior_enable(mceik_mcmc *s, const mceik_prior_opts *o);
/* Later steps are the plain sampler's again. */
int mceik_mcmc_prior_disable(mceik_mcmc *s);
/* The options in force (o may be NULL).  vref: host [nphase * ncell] or NULL;
 * it is filled, and o->vref points to it, when a reference model is loaded,
 * else o->vref is NULL. */
int mceik_mcmc_prior_get(mceik_mcmc *s, mceik_prior_opts *o, int *vref);
/* Es, Ed [nchains][nphase] of the chains' current models, summed on the GPU
 * (either may be NULL).  Synchronises. */
int mceik_mcmc_prior_energy(mceik_mcmc *s, long long *Es, long long *Ed);
/* dE [nchains][2] = (dEs, dEd) of every chain's proposal of the last step,
 * accepted or not; 0, 0 for a proposal outside the box.  Synchronises. */
int mceik_mcmc_prior_last(mceik_mcmc *s, long long *dE);
/* Host only (no GPU call), the arithmetic the kernels run.  energy: Es, Ed of
 * one ncx x ncy x ncz model v (vref NULL: Ed = 0).  delta: their change under
 * the block footprint (mceik_block_footprint) of signed amplitude amp != 0 and
 * radius 0..8 centred on `cell`, evaluated on the unchanged v.  Outputs may be
 * NULL.  Both return 1 on invalid arguments, and where 3 ncell span^2 >= 2^53
 * with span the range of the values in v and vref (delta: plus 2 |amp|). */
int mceik_prior_energy(int ncx, int ncy, int ncz, const int *v, const int *vref, long long *Es, long long *Ed);
int mceik_prior_delta(int ncx, int ncy, int ncz, const int *v, const int *vref, int cell, int radius, int amp,
                      long long *dEs, long long *dEd);

/* ---- hypocentre moves (csrc/hypo.hip) --------------------
 * Off by default; with it off nothing changes: every chain fits its picks at
 * the catalogue's hypocentres snapped to their nearest nodes.  Enabled, every
 * chain carries a position of its own per event, hyp[nchains][nev][3] = node
 * indices (ix, iy, iz), 0-based, which start at the catalogue's nodes at the
 * first enable and from then on stay per chain, also after disable.  Origin
 * time stays marginalised analytically, as in every objfn.
 *
 * With every = K > 0 global step gs is a hypocentre step iff gs % K == K - 1.
 * It replaces that step's velocity proposal: v and naccept do not change,
 * mceik_mcmc_last's accept flags are 0, the kept-state and posterior rules
 * apply with the step's new logL, a swap round of gs runs first.  Block
 * proposals and the prior act on velocity steps only.  For chain c (global id
 * g) and event e:
 *   r = Philox4x32-10(counter {(uint32)gs, (uint32)(gs >> 32), 2, e}, key {g, seed})
 *       (counter word 2: proposals 0, swaps 1)
 *   d[a] = (int)(((uint64)r[a] * (2 dmax[a] + 1)) >> 32) - dmax[a],  a = 0, 1, 2
 *   log u = det_log((r[3] + 0.5) / 2^32)
 *   candidate = current + d; inside iff lo[a] <= candidate[a] <= hi[a] on every axis
 * (a symmetric draw: no Hastings term).  One forward of the chain's current
 * models extracts every station's time at each event's current and candidate
 * node; obj_cur and obj_cand are the event's objfn (the sampler's L2 misfit
 * with the analytic origin time, the same operations in the same order) at
 * the two, every phase from that forward, and
 *   accept iff inside and log u < obj_cur - obj_cand
 *              (tempering: log u < beta * (obj_cur - obj_cand), one fp64
 *               multiply; the uniform box is not tempered)
 * per event: logL = -sum_e objfn_e and the events are independent given the
 * model, so every event's move is an exact Metropolis step.  Then logL = 0;
 * logL = logL - obj_sel[e] in event order (obj_sel: the accepted side's
 * value), bitwise the logL of a full forward at the chain's models and new
 * positions.  A tempering swap exchanges the two chains' positions with their
 * models; its rule does not change (the box is the same for both replicas).
 *
 * While enabled every step is one launch of each kernel
 * (mceik_mcmc_info.multi_step reports 0 until disable), and after every kept
 * step (nburnIn / keepK) the cold chains' positions are added to exact
 * integer moments per event: n states, sum[nev][3] of (x, y, z) and sq[nev][6]
 * of (xx, yy, zz, xy, xz, yz) in nodes -- the location mean and covariance
 * without stored states; pipes and ranks merge them by addition.
 *
 * enable refuses (1): NULL options, every < 0, a dmax < 0, lo > hi or a box
 * outside the grid, a chain's current position outside the box, a sampler with
 * tt_interp = 1, and an enabled posterior that holds states.  The other
 * functions return 1 before the first enable.  A checkpoint is
 * mceik_mcmc_checkpoint plus hypo_get and hypo_moments_get; a resume is
 * hypo_set, then mceik_mcmc_restore with the saved logl (two models: with
 * logl NULL, as every two-model resume, so that its forward makes the current
 * tables of both models; it gives the saved logl), then hypo_moments_set.
 * Positions are not part of the kept ring nor of mceik_mcmc_gather.
 *
 * Every function returns 0, 1 on invalid arguments or -1 on a device failure. */
typedef struct mceik_hypo_opts { int every; int dmax[3]; int lo[3], hi[3]; } mceik_hypo_opts;
/* Turns hypocentre moves on (or replaces the options).  Synchronises; resets
 * the counters and the moments. */
int mceik_mcmc_hypo_enable(mceik_mcmc *s, const mceik_hypo_opts *o);
/* Later steps are velocity steps again; the positions stay, per chain. */
int mceik_mcmc_hypo_disable(mceik_mcmc *s);
/* The options in force (every = 0 after disable; o may be NULL) and the
 * positions xyz [nchains][nev][3] (or NULL).  Synchronises. */
int mceik_mcmc_hypo_get(mceik_mcmc *s, mceik_hypo_opts *o, int *xyz);
/* Replaces the positions (inside the grid; inside the box while enabled); one
 * full forward recomputes logL (2: a solve failed, as mceik_mcmc_restore).
 * Synchronises. */
int mceik_mcmc_hypo_set(mceik_mcmc *s, const int *xyz);
/* attempts, accepts [nev]: moves tried and accepted per event over the chains
 * (either may be NULL).  Synchronises. */
int mceik_mcmc_hypo_stats(mceik_mcmc *s, long long *attempts, long long *accepts, int reset);
/* The last hypocentre step: cand [nchains][nev][3] = current + d (also when
 * outside), accept [nchains][nev], obj [nchains][nev][2] = objfn at the
 * current, the candidate node (a candidate outside: at the current node).
 * Any may be NULL.  Synchronises. */
int mceik_mcmc_hypo_last(mceik_mcmc *s, int *cand, unsigned char *accept, double *obj);
/* The moments: n, sum [nev][3], sq [nev][6] (get: any may be NULL). */
int mceik_mcmc_hypo_moments_get(mceik_mcmc *s, long long *n, long long *sum, long long *sq);
int mceik_mcmc_hypo_moments_set(mceik_mcmc *s, long long n, const long long *sum, const long long *sq);
/* Host only (no GPU call): the draw of event e of global chain gchain at
 * global step `step`: d[3] and log u (may be NULL). */
int mceik_hypo_draw(uint32_t seed, uint32_t gchain, uint64_t step, int e, const int dmax[3], int d[3], double *logu);

/* ---- noise scale and station statics (csrc/nuis.hip) -----
 * Off by default; with it off nothing changes: every chain takes the pick
 * uncertainty var[j] and the station corrections tcorr[j] from the catalogue.
 * Enabled, every chain carries integer state of its own:
 *   kn[nchains][nphase]         index into a noise ladder lam[nk], lnlam[nk]
 *                               (fp64 tables the caller passes; nk odd, the
 *                               middle entry exactly lam = 1, lnlam = 0: the
 *                               start value), uniform prior on the index;
 *   kc[nchains][nphase][nstat]  station static in units of dt seconds, uniform
 *                               prior on |kc| <= kcmax, start value 0.
 * The effective observations of chain c take one fp64 operation each,
 *   var_eff[j]   = var[j] * lam[kn[c][ph(j)]]
 *   tcorr_eff[j] = tcorr[j] + (double)kc[c][ph(j)][stat(j)] * dt
 *   logL[c]      = (((0 - obj_0) - obj_1) ... - obj_{nev-1}) - norm[0] * lnlam[kn[c][0]]
 *                                                  (two models: - norm[1] * lnlam[kn[c][1]])
 * with obj_e the sampler's objfn of event e on the effective arrays (the same
 * operations in the same order) and norm[ph] an option (NULL: the number of
 * used, unmasked picks of phase ph).  var enters objfn as 1 / var on the
 * residual, so lam scales sigma and the term is the Gaussian normalisation
 * with the origin time at its plug-in value (the profile form; a caller may
 * pass norm[ph] reduced by the events' degrees of freedom).  At the start
 * values every logL is today's bit for bit.  While a sampler holds this state
 * every logL it evaluates honours it -- velocity accepts (single cell, block),
 * hypocentre moves, restore with logl NULL -- every step is one launch of each
 * kernel (mceik_mcmc_info.multi_step reports 0), and a one-model sampler keeps
 * the tables of its current model, as a two-model sampler always does.
 *
 * Global step gs is a nuisance step iff gs % every == offset (a step that is
 * also a hypocentre step is a hypocentre step).  It replaces that step's
 * velocity proposal and runs no eikonal solve: v and naccept do not change,
 * mceik_mcmc_last's accept flags are 0, the kept-state and posterior rules
 * apply with the new logL, a swap round of gs runs first.  A chain (global id
 * g) runs nsub sub-moves in sequence, sub-move `sub` drawing
 *   r = Philox4x32-10(counter {(uint32)gs, (uint32)(gs >> 32), 3, sub}, key {g, seed})
 *   M = (noise: nphase) + (statics: nact[0] + nact[1]),  q = (r0 * M) >> 32
 * where nact[ph] counts the stations with a used pick of phase ph (a phase
 * with fewer than two counts 0: it has no statics moves).
 *   q < nphase (noise on): a noise move of phase q, k' = k +- d,
 *     d = 1 + ((r1 * dk) >> 32), minus iff r2 & 1; k' outside [0, nk) is rejected.
 *   otherwise a statics move of a zero-sum pair of one phase: a = the q-th of
 *     the remaining range over the phases' active stations (station order),
 *     partner b = (r1 * (nact - 1)) >> 32, b += (b >= a),
 *     mag = 1 + (((r2 >> 1) * dc) >> 31), minus iff r2 & 1;
 *     kc[a] += s mag, kc[b] -= s mag, rejected if either leaves the box.  The
 *     pair keeps the phase's sum of statics at its start value exactly: the
 *     direction the analytic origin time absorbs is never moved along.
 *   log u = det_log((r3 + 0.5) / 2^32); accept iff log u < logL' - logL
 *     (tempering: log u < beta * (logL' - logL); the boxes are not tempered).
 * Both draws are symmetric: no Hastings term.  A tempering swap exchanges the
 * two chains' kn, kc, effective observations and current tables with their
 * models; its rule does not change.
 *
 * After every kept step (nburnIn / keepK) while enabled the cold chains add
 * to exact integer moments: n states, per phase the sums of k and k^2 and a
 * histogram over the ladder, per (phase, station) the sums of kc and kc^2;
 * pipes and ranks merge them by addition.
 *
 * enable refuses (1): NULL options, both parts off, every <= 0, offset
 * outside [0, every), nsub <= 0, nk even or a ladder whose middle entry is not
 * exactly (1, 0) (lam and lnlam may both be NULL with noise off), dk, dc or
 * kcmax negative, dt <= 0 with statics on, nothing to move, held state that
 * does not fit the new ladder length or box, 8 nev + 4 nphase nstat above
 * 64 KiB, and an enabled posterior that holds states.  tt_interp = 1 is
 * allowed.  enable runs one full forward (not counted in the FSM statistics).
 * disable stops the nuisance steps and keeps the values; clear returns every
 * chain to the start values, recomputes logL and gives multi-step launches
 * back.  The other functions return 1 while no state is held.  A checkpoint
 * is mceik_mcmc_checkpoint plus nuis_get and nuis_moments_get; a resume is
 * nuis_set, then mceik_mcmc_restore with logl NULL (its forward makes the
 * current tables; it gives the saved logl), then nuis_moments_set.  The values
 * are not part of the kept ring nor of mceik_mcmc_gather.
 *
 * Every function returns 0, 1 on invalid arguments or -1 on a device failure. */
typedef struct mceik_nuis_opts {
    int every, offset, nsub;
    int noise, statics;            /* which parts move (either or both) */
    int nk, dk;                    /* ladder entries; a noise move is +-[1, max(dk, 1)] entries */
    int dc, kcmax;                 /* a statics move is +-[1, max(dc, 1)] units; the box */
    double dt;                     /* seconds per unit of kc */
    const double *lam, *lnlam;     /* [nk] */
    const double *norm;            /* [nphase] or NULL */
} mceik_nuis_opts;
/* Turns the moves on (or replaces the options; held values stay).  Synchronises;
 * resets the counters and the moments. */
int mceik_mcmc_nuis_enable(mceik_mcmc *s, const mceik_nuis_opts *o);
int mceik_mcmc_nuis_disable(mceik_mcmc *s);
int mceik_mcmc_nuis_clear(mceik_mcmc *s);
/* The options in force (every = 0 after disable; the pointers of o are NULL),
 * the ladder [nk], norm [nphase], kn [nchains][nphase] and kc
 * [nchains][nphase][nstat].  Any may be NULL.  Synchronises. */
int mceik_mcmc_nuis_get(mceik_mcmc *s, mceik_nuis_opts *o, double *lam, double *lnlam, double *norm, int *kn, int *kc);
/* Replaces the values (inside the ladder and the box) and recomputes logL
 * from the current tables the sampler holds: no eikonal solve.  Synchronises. */
int mceik_mcmc_nuis_set(mceik_mcmc *s, const int *kn, const int *kc);
/* attempts, accepts [nphase + nphase * nstat] over the chains: entry ph is the
 * noise index of phase ph, entry nphase + ph * nstat + k the static of station
 * k (a pair counts on both its stations).  Either may be NULL.  Synchronises. */
int mceik_mcmc_nuis_stats(mceik_mcmc *s, long long *attempts, long long *accepts, int reset);
/* The last nuisance step: rec [nchains][nsub][4] = parameter (numbered as in
 * nuis_stats), partner parameter (-1: a noise move), candidate value of the
 * parameter, accepted; logl [nchains][nsub][2] = logL before the sub-move and
 * logL' of the candidate (a candidate outside its box: logL).  Synchronises. */
int mceik_mcmc_nuis_last(mceik_mcmc *s, int *rec, double *logl);
/* The moments: n, ksum [nphase][2] = sums of k, k^2, hist [nphase][nk], csum
 * [nphase][nstat][2] = sums of kc, kc^2 (get: any may be NULL). */
int mceik_mcmc_nuis_moments_get(mceik_mcmc *s, long long *n, long long *ksum, long long *hist, long long *csum);
int mceik_mcmc_nuis_moments_set(mceik_mcmc *s, long long n, const long long *ksum, const long long *hist,
                                const long long *csum);
/* Host only (no GPU call): sub-move `sub` of global chain gchain at global
 * step `step` with nnoise = (noise: nphase, else 0) and nact0 / nact1 active
 * stations per phase (0 or >= 2): m = {kind (0 noise, 1 statics), phase, a, b
 * (indices into the phase's active stations; 0 for a noise move), signed
 * step} and log u (may be NULL). */
int mceik_nuis_draw(uint32_t seed, uint32_t gchain, uint64_t step, int sub, int nnoise, int nact0, int nact1, int dk,
                    int dc, int m[5], double *logu);

/* ---- probe-to-cell covariances / trade-off maps (csrc/cov.hip)
 * Off by default; with it off nothing changes.  Every other summary is a
 * marginal; this one streams, for 1 <= np <= 64 probe quantities, the exact
 * cross-moments of each probe with every model entry, so that a row of the
 * (out of reach) joint covariance can be read: how a cell, an event's depth or
 * a station's static co-varies with the whole model.  A probe is one int32
 * scalar of a chain, named by (kind, index):
 *   kind 0  model entry      v[c][index]            index in [0, nphase * ncell)
 *   kind 1  hypocentre       hyp[c][e][axis]        index = 3 e + axis (node units); needs the positions held
 *                                                   (after the first hypo_enable, also after hypo_disable)
 *   kind 2  station static   kc[c][ph][stat]        index = ph * nstat + stat; needs nuisance state with statics on
 *   kind 3  noise index      kn[c][ph]              index = ph; needs nuisance state with noise on
 * Duplicate probes are allowed.  With x_p probe p's value and v_j model entry
 * j, over the cold chains c and the accumulated states t the sampler keeps in
 * int64 (ncm = nphase * ncell)
 *   n                        states per chain
 *   A[np] = sum x_p          G[np][np] = sum x_p x_q
 *   S[ncm] = sum v_j         Q[ncm] = sum v_j^2         C[np][ncm] = sum x_p v_j
 * and with within = 1 also the per-chain sums A_c[nchains][np] = sum_t x_p and
 * S_c[nchains][ncm] = sum_t v_j (rows of hot chains stay zero).  Memory: 8 (np
 * + 2) ncm bytes pooled (17 MB at 32 768 entries and 64 probes), within = 1
 * adds 8 nchains (ncm + np) (269 MB at 1024 chains).  Every word is an exact
 * integer sum: the order of accumulation, pipes, shards and ranks do not
 * matter.  A word wraps after 2^63 / (max |x| * vmax) accumulated states
 * (chains x kept steps): more than 1e11 at the default prior.
 *
 * While enabled, mceik_mcmc_run adds the state after every kept step (the rule
 * of the kept states and of the posterior, whatever max_samples is) by two
 * kernels queued behind the step: no host synchronisation, and the chains are
 * bit for bit those of a run without it.  With multi-step launches a launch
 * ends right after the next kept step, as for the streaming posterior.
 *
 * enable returns 1 for np outside [1, 64], an unknown kind, an index out of
 * range, a probe whose state is not held, and while the accumulators hold
 * states of another probe list or another `within`; with the list and
 * `within` of the held sums it resumes them.  disable stops accumulating and
 * keeps the sums; clear drops them.  While a kind 2 or 3 probe is registered
 * and accumulation is enabled, mceik_mcmc_nuis_clear returns 1.
 * Every function returns 0, 1 on invalid arguments or -1 on a device failure. */
#define MCEIK_COV_MAX_PROBES 64
typedef struct mceik_cov_opts {
    int np;
    int kind[MCEIK_COV_MAX_PROBES], index[MCEIK_COV_MAX_PROBES];
    int within;
} mceik_cov_opts;
typedef struct mceik_cov_partials {            /* caller-allocated host arrays */
    int np, ncm, within;
    int kind[MCEIK_COV_MAX_PROBES], index[MCEIK_COV_MAX_PROBES];
    long long nchains, nkept;                  /* chains summed, states per chain */
    long long *A, *S;                          /* [np], [ncm] */
    /* 128-bit two's complement, lo then hi word: sums of products ... */
    unsigned long long *G, *Q, *C;             /* [np][np][2], [ncm][2], [np][ncm][2] */
    /* ... and, within = 1 (else zero; may be NULL), sums over chains of products of per-chain sums:
     * PA[p][q] = sum_c A_c[c][p] A_c[c][q],  P[j] = sum_c S_c[c][j]^2,  T[p][j] = sum_c A_c[c][p] S_c[c][j] */
    unsigned long long *PA, *P, *T;            /* [np][np][2], [ncm][2], [np][ncm][2] */
} mceik_cov_partials;
int mceik_mcmc_cov_enable(mceik_mcmc *s, const mceik_cov_opts *o);
int mceik_mcmc_cov_disable(mceik_mcmc *s);
int mceik_mcmc_cov_clear(mceik_mcmc *s);
/* Adds the cold chains' current state now (enqueued on the sampler's stream). */
int mceik_mcmc_cov_accumulate(mceik_mcmc *s);
/* Host copies of / replacements for the accumulators (checkpoints): n, A [np],
 * G [np][np], S, Q [ncm], C [np][ncm], Ac [nchains][np], Sc [nchains][ncm]
 * (the last two with within = 1 only).  get synchronises, any pointer may be
 * NULL; set needs every array the sampler holds. */
int mceik_mcmc_cov_get(mceik_mcmc *s, long long *n, long long *A, long long *G, long long *S, long long *Q,
                       long long *C, long long *Ac, long long *Sc);
int mceik_mcmc_cov_set(mceik_mcmc *s, long long n, const long long *A, const long long *G, const long long *S,
                       const long long *Q, const long long *C, const long long *Ac, const long long *Sc);
/* The accumulators as partials, and with within = 1 the chain axis reduced on
 * the device into PA, P and T.  Fills every scalar of *out, the probe list and
 * the arrays it points to.  Synchronises. */
int mceik_mcmc_cov_partials(mceik_mcmc *s, mceik_cov_partials *out);
/* Host only (no GPU call).  merge: dst += src, every word with its carry; 1
 * unless np, the probe lists, ncm, within and nkept agree.  finish: with M =
 * nchains, n = nkept, N = M n every numerator is an exact 128-bit integer
 * converted to double once, then only *, / and sqrt:
 *   cov[p][j]   = (N C - A_p S_j) / (N (N - 1)),  var_x[p] from G_pp, var_v[j] from Q_j likewise
 *   corr[p][j]  = cov / sqrt(var_x[p] var_v[j])
 *   covw[p][j]  = (n C - T) / (M n (n - 1)),  Wx[p] = (n G_pp - PA_pp) / (M n (n - 1)),  Wv[j] = (n Q_j - P_j) / (M n (n - 1))
 *   corrw[p][j] = covw / sqrt(Wx[p] Wv[j])
 * (pooled over all chains and states; within-chain: about each chain's own
 * mean, meaningful while R-hat is not yet 1).  pmean[p] = A_p / N; pcov, pcorr,
 * pcovw, pcorrw [np][np] come the same way from G and PA.  NaN: the pooled
 * quantities when N < 2 (pmean when N = 0), the within-chain ones when within
 * = 0, n < 2 or M < 1, a correlation whose variance numerator is 0.  cov, corr,
 * covw, corrw: [np][ncm]; any output may be NULL. */
int mceik_cov_merge(mceik_cov_partials *dst, const mceik_cov_partials *src);
int mceik_cov_finish(const mceik_cov_partials *p, double *cov, double *corr, double *covw, double *corrw, double *pmean,
                     double *pcov, double *pcorr, double *pcovw, double *pcorrw);

/* ---- effective sample sizes by batch means (csrc/ess.hip) --
 * Integrated autocorrelation time, effective sample size and Monte-Carlo
 * standard error of every model entry (and of up to 64 probe scalars, the
 * kinds of the covariance probes above), streamed: kept states are never
 * stored.  Off by default; with it off nothing changes.
 *
 * An entry j is one of the ncm = nphase * ncell cells or, after them, one of
 * the np probes: ne = ncm + np entries.  Batch sizes are 2^l, l = 0 ..
 * nlevels - 1 (1 <= nlevels <= 16).  Let t = 1, 2, ... count the states added
 * to a chain.  Per chain c and entry the sampler holds
 *   Sc[c][j]       int64   the sum of all states added so far
 *   pend[l][c][j]  int32   l = 0 .. nlevels - 2: the first half of the open level-(l + 1) batch
 * and pooled over the cold chains, per level and entry, the exact sums
 *   A[l][j]  int64     sum over chains of the chain's closed level-l batch sums
 *   Q[l][j]  128 bits  sum over chains and closed level-l batches of B^2
 *   P[l][j]  128 bits  sum over chains of (Sc at the chain's last level-l close)^2
 * Adding state number t (value v; k = trailing zero bits of t, kk = min(k,
 * nlevels - 1)):  b = v; Sc += v; for l = 0 .. kk: { A[l] += b; Q[l] += b b;
 * P[l] += b (2 Sc - b); if (l == k && l <= nlevels - 2) { pend[l] = b; stop; }
 * if (l < kk) b += pend[l]; }.  Every update is an integer addition: the words
 * do not depend on the order of chains, pipes, launches, shards or ranks, and
 * partials merge by addition.  Probe entries may be negative: A and P are
 * two's complement, Q is unsigned.
 *
 * Memory: (8 + 4 (nlevels - 1)) nchains ne bytes per chain plus 40 nlevels ne
 * pooled (1024 chains x 32 768 entries: 1.2 GB at nlevels = 8, 1.7 GB at 12).
 * A word of pend holds a batch sum of 2^(nlevels - 2) states: enable refuses
 * (1) when x 2^(nlevels - 2) >= 2^31 for x the largest value an entry can
 * take: max(vmax, vsmax), a grid dimension for a hypocentre probe, kcmax for
 * a static, the ladder length for a noise index (mceik_ess_check).  Sc and A
 * wrap after 2^63 / x states (of a chain; of all chains); while they hold, Q
 * and P stay below 2^127.
 *
 * While enabled, mceik_mcmc_run adds the cold chains' state after every kept
 * step (the rule of the kept states and of the posterior, whatever
 * max_samples is) by one kernel queued behind the step: no host
 * synchronisation, and the chains are bit for bit those of a run without it.
 * With multi-step launches a launch ends right after the next kept step, as
 * for the streaming posterior.
 *
 * enable returns 1 for nlevels outside [1, 16], np outside [0, 64], an unknown
 * kind, an index out of range, a probe whose state is not held, the bound
 * above, and while the accumulators hold states of other options; with the
 * options of the held sums it resumes them.  disable stops accumulating and
 * keeps the sums; clear drops them.  While a kind 2 or 3 probe is registered
 * and accumulation is enabled, mceik_mcmc_nuis_clear returns 1.
 * Every function returns 0, 1 on invalid arguments or -1 on a device failure. */
#define MCEIK_ESS_MAX_LEVELS 16
typedef struct mceik_ess_opts {
    int nlevels;
    int np;                                    /* probes: 0 .. MCEIK_COV_MAX_PROBES */
    int kind[MCEIK_COV_MAX_PROBES], index[MCEIK_COV_MAX_PROBES];
} mceik_ess_opts;
typedef struct mceik_ess_partials {            /* caller-allocated host arrays */
    int ncm, np, nlevels;                      /* ne = ncm + np entries */
    long long nchains, nkept;                  /* chains summed, states per chain */
    long long *A;                              /* [nlevels][ne] */
    unsigned long long *Q, *P;                 /* [nlevels][ne][2] = lo, hi words */
} mceik_ess_partials;
int mceik_mcmc_ess_enable(mceik_mcmc *s, const mceik_ess_opts *o);
int mceik_mcmc_ess_disable(mceik_mcmc *s);
int mceik_mcmc_ess_clear(mceik_mcmc *s);
/* Adds the cold chains' current state now (enqueued on the sampler's stream). */
int mceik_mcmc_ess_accumulate(mceik_mcmc *s);
/* Host copies of / replacements for the accumulators (checkpoints): n states
 * per chain, Sc [nchains][ne], pend [nlevels - 1][nchains][ne], A [nlevels][ne],
 * Q, P [nlevels][ne][2].  get synchronises, any pointer may be NULL; set needs
 * every array (pend only when nlevels > 1). */
int mceik_mcmc_ess_get(mceik_mcmc *s, long long *n, long long *Sc, int *pend, long long *A, unsigned long long *Q,
                       unsigned long long *P);
int mceik_mcmc_ess_set(mceik_mcmc *s, long long n, const long long *Sc, const int *pend, const long long *A,
                       const unsigned long long *Q, const unsigned long long *P);
/* The pooled words as partials.  Fills every scalar of *out and the arrays it
 * points to.  Synchronises. */
int mceik_mcmc_ess_partials(mceik_mcmc *s, mceik_ess_partials *out);
/* Host only (no GPU call).
 * check: 0 when nlevels is in [1, 16] and xmax 2^(nlevels - 2) < 2^31, else 1.
 * lstar: the reported level min(nlevels - 1, floor(log2(n) / 2)), a batch of
 * about sqrt(n) states (0 for n < 1).
 * merge: dst += src, every word with its carry; 1 unless ncm, np, nlevels and
 * nkept agree.
 * finish: with M = nchains, n = nkept, nb_l = n >> l the numerator N_l = nb_l
 * Q_l - P_l is an exact 128-bit integer converted to double once, then only
 * *, / and sqrt:
 *   s2_l  = N_l / (M nb_l (nb_l - 1))       the within-chain variance of the level-l batch sums
 *   tau_l = s2_l / (2^l s2_0)               the integrated autocorrelation time seen at batch size 2^l
 *   ess   = M n / tau_L,   mcse = sqrt(s2_L / 2^L / (M n))    at L = level, or lstar when level < 0
 * (mcse: the standard error of the mean pooled over chains and states).  NaN:
 * tau_l where nb_l < 2; everything of an entry whose N_0 is 0 (it never moved:
 * R-hat's rule) and when M < 1; ess and mcse where tau_L is NaN.  tau:
 * [nlevels][ne]; ess, mcse: [ne]; any may be NULL; *level_used gets L.
 * Returns 1 for level >= nlevels. */
int mceik_ess_check(int nlevels, long long xmax);
int mceik_ess_lstar(int nlevels, long long n);
int mceik_ess_merge(mceik_ess_partials *dst, const mceik_ess_partials *src);
int mceik_ess_finish(const mceik_ess_partials *p, int level, double *tau, double *ess, double *mcse, int *level_used);

/* ---- pick residuals, origin times and data-fit checks (csrc/fit.hip)
 * The data side of a run, streamed: per pick the mean and spread of its
 * residual and of its standardised residual, per event the origin time and a
 * reduced misfit, per (phase, station) the mean residual and a histogram of
 * the standardised residuals.  Kept states are never stored and no forward
 * solve is repeated.  Off by default; with it off nothing changes.
 *
 * Per kept step and cold chain, from the chain's current state exactly as its
 * logL sees it (the chain's effective var / tcorr while nuisance state is
 * held, its own event nodes, trilinear tables under tt_interp): for every
 * event e the objective's arithmetic in fp64 over the event's
 * used picks j in CSR order, every table value te_j from the chain's current
 * tables,
 *   xnorm = sum_j 1 / var_j                        (from 0.0, in order)
 *   t0    = sum_j ((1 / var_j) / xnorm) (tc_j - te_j),   tc_j = tobs_j - tcorr_j
 *   r_j   = tc_j - (te_j + t0),   z_j = (1.0 / var_j) * r_j      (objfn = sum z^2 / 2)
 * and the integers, rint = fp64 round-half-even, sat32 = clamp to +-(2^31 - 1):
 *   q_j  = sat32(rint(r_j * (1 / tick)))           tick: a power of two (seconds), so the scaling is exact
 *   zq_j = sat32(rint(z_j * 1024.0))
 *   tq_e = sat32(rint((t0 - t0_ref[e]) * (1 / tick)))     (0 for an event without a used pick)
 *   b_j  = clamp(floor(z_j * (nbins / (2 zmax)) + nbins / 2), 0, nbins - 1)   in that order, in fp64
 * Every clamp of q, zq, tq bumps sat[0], sat[1], sat[2] (a NaN clamps to the
 * upper bound).  Masked picks contribute nothing.  The sums, pooled over the
 * cold chains and the kept steps:
 *   sq, szq [nobs]  int64      sums of q, zq (two's complement)
 *   sq2, szq2 [nobs][2]        sums of q^2, zq^2: 128 bits as unsigned (lo, hi) words
 *   stq [nev] int64, stq2 [nev][2]                 the same of tq
 *   hist [nphase][nstat][nbins] int64              counts of b_j by the pick's phase and station
 * Every update is an integer addition: the words do not depend on the order of
 * chains, pipes, launches, shards or ranks, and partials merge by addition.
 * |q| < 2^31, so an int64 sum holds 2^32 states (chains x kept steps) and a
 * 128-bit sum of squares never wraps before it.  Memory: 4 (3 nobs + nev)
 * bytes per chain (the last kept step's words, mceik_mcmc_fit_last) plus 48
 * nobs + 24 nev + 8 nphase nstat nbins pooled.
 *
 * While enabled, mceik_mcmc_run adds the cold chains' state after every kept
 * step by two kernels queued behind the step: no host synchronisation, and
 * the chains are bit for bit those of a run without it.  With multi-step
 * launches a launch ends right after the next kept step, as for the streaming
 * posterior.  A one-model sampler holds its current tables while enabled, as
 * it does while nuisance state is held (enable runs one forward to fill them
 * when they were not held), and steps with one launch per step
 * (mceik_mcmc_info.multi_step reports 0 until disable): the per-step accept
 * keeps the tables current, the multi-step kernel only does for two models.
 *
 * enable returns 1 for a tick that is not 2^k (k in [-64, 64]), nbins odd or
 * outside [2, 256], zmax not positive and finite, a t0_ref that is not finite,
 * and while the accumulators hold states of other options; with the options
 * of the held sums it resumes them.  t0_ref NULL: zeros.  disable stops
 * accumulating and keeps the sums; clear drops them.
 * Every function returns 0, 1 on invalid arguments or -1 on a device failure
 * (enable: 2 when the forward that fills the tables fails). */
#define MCEIK_FIT_MAX_BINS 256
typedef struct mceik_fit_opts {
    double tick;                               /* seconds per unit of q and tq: 2^k */
    int nbins;                                 /* even, 2 .. MCEIK_FIT_MAX_BINS */
    double zmax;                               /* the histogram covers [-zmax, zmax]; the edge bins take the tails */
    const double *t0_ref;                      /* [nev] subtracted from t0 before scaling, or NULL */
} mceik_fit_opts;
typedef struct mceik_fit_partials {            /* caller-allocated host arrays */
    int nobs, nev, nphase, nstat, nbins;
    double tick, zmax;
    long long nchains, nkept;                  /* chains summed, states per chain */
    int *obs_ptr;                              /* [nev + 1] the catalogue's CSR rows */
    int *obs_stat, *obs_phase, *obs_mask;      /* [nobs] station, phase (0 P, 1 S), 1 = not fit */
    double *t0_ref;                            /* [nev] */
    long long *sq, *szq;                       /* [nobs] */
    unsigned long long *sq2, *szq2;            /* [nobs][2] = lo, hi words */
    long long *stq;                            /* [nev] */
    unsigned long long *stq2;                  /* [nev][2] */
    long long *hist;                           /* [nphase][nstat][nbins] */
    long long sat[3];                          /* clamped q, zq, tq */
} mceik_fit_partials;
int mceik_mcmc_fit_enable(mceik_mcmc *s, const mceik_fit_opts *o);
int mceik_mcmc_fit_disable(mceik_mcmc *s);
int mceik_mcmc_fit_clear(mceik_mcmc *s);
/* Adds the cold chains' current state now (enqueued on the sampler's stream). */
int mceik_mcmc_fit_accumulate(mceik_mcmc *s);
/* Host copies of / replacements for the accumulators (checkpoints): n states
 * per chain and the arrays above (sat [3]).  get synchronises, any pointer may
 * be NULL; set needs every array. */
int mceik_mcmc_fit_get(mceik_mcmc *s, long long *n, long long *sq, long long *szq, unsigned long long *sq2,
                       unsigned long long *szq2, long long *stq, unsigned long long *stq2, long long *hist,
                       long long *sat);
int mceik_mcmc_fit_set(mceik_mcmc *s, long long n, const long long *sq, const long long *szq,
                       const unsigned long long *sq2, const unsigned long long *szq2, const long long *stq,
                       const unsigned long long *stq2, const long long *hist, const long long *sat);
/* The pooled words as partials.  Fills every scalar of *out and the arrays it
 * points to.  Synchronises. */
int mceik_mcmc_fit_partials(mceik_mcmc *s, mceik_fit_partials *out);
/* The last kept step's words of every chain of the sampler (rows of chains
 * that are not cold stay 0): q, zq [nchains][nobs] (0 for a masked pick), tq
 * [nchains][nev]; any may be NULL.  Synchronises. */
int mceik_mcmc_fit_last(mceik_mcmc *s, int *q, int *zq, int *tq);
/* Host only (no GPU call).
 * check: 0 when tick is 2^k, k in [-64, 64], and a residual of rmax >= 0
 * seconds does not saturate (rint(rmax / tick) <= 2^31 - 1), else 1.
 * merge: dst += src, every word with its carry; 1 unless the shapes, tick,
 * zmax, t0_ref, the observations' rows and nkept agree.
 * finish: with N = nchains nkept, every exact sum (for a standard deviation
 * the exact integer N Q - S^2) is converted to double once, then only *, / and
 * sqrt:
 *   pick_mean = sq tick / N            pick_sd = sqrt((N sq2 - sq^2) / (N (N - 1))) tick      [nobs]
 *   pick_zmean = szq / 1024 / N        pick_zrms = sqrt(szq2 / (1024^2 N))                    [nobs]
 *   t0_mean, t0_sd: the same of stq, stq2, the mean plus t0_ref                              [nev]
 *   ev_misfit = (sum over the event's used picks of szq2) / (1024^2 N (used picks - 1))      [nev]
 *   sta_mean = (sum over the row's used picks of sq) tick / (N picks): the data's estimate
 *   of a station static; sta_zrms = sqrt(sum of szq2 / (1024^2 N picks))         [nphase][nstat]
 *   phase_zrms: the same over every used pick of the phase                                [nphase]
 * NaN: everything when nkept < 2 or nchains < 1; a masked pick; an event or a
 * row without a used pick (ev_misfit: with fewer than two).  Any output may be
 * NULL. */
int mceik_fit_check(double tick, double rmax);
int mceik_fit_merge(mceik_fit_partials *dst, const mceik_fit_partials *src);
int mceik_fit_finish(const mceik_fit_partials *p, double *pick_mean, double *pick_sd, double *pick_zmean,
                     double *pick_zrms, double *t0_mean, double *t0_sd, double *ev_misfit, double *sta_mean,
                     double *sta_zrms, double *phase_zrms);

/* ---- multi-rank runs (one process per GPU; csrc/comm.hip) ---------------
 * The sampler's only collective is the checkpoint gather (SURVEY s.8e) over
 * RCCL (xGMI on one node).  Bootstrap as RCCL's: rank 0 calls
 * mceik_comm_unique_id, the launcher broadcasts the bytes (MPI_Bcast in a
 * C/MPI main -- MPI keeps launch and bootstrap, the role of broadcast.c and
 * mpiutils.f90:346-426), then every rank calls mceik_comm_init with its GPU. */
#define MCEIK_COMM_ID_BYTES 128
typedef struct mceik_comm mceik_comm;
/* 1 if this process can build a communicator (RCCL loads and has every entry
 * point the library uses), else 0.  Local, no GPU call: a launcher agrees on
 * it over all ranks BEFORE mceik_comm_init, which is collective and would
 * leave the other ranks waiting for a rank that cannot join. */
int mceik_comm_available(void);
int mceik_comm_unique_id(unsigned char id[MCEIK_COMM_ID_BYTES]);
int mceik_comm_init(const unsigned char id[MCEIK_COMM_ID_BYTES], int nranks, int rank, int device,
                    mceik_comm **out);
int mceik_comm_finalize(mceik_comm **c);
/* Collective over c: every rank's chains -> root, in global chain order.
 * which = 0 the current state (mceik_mcmc_get_state), 1 the most recent kept
 * state (every rank must hold one).  The ranks' shards [chain_offset,
 * chain_offset + nchains) must tile [0, nchains_total) (else every rank
 * returns 2).  On the root v_out [nchains_total][ncell] and logl_out
 * [nchains_total] are host or device memory (either may be NULL; device
 * memory of the communicator's GPU is received into directly, without
 * staging); other ranks pass NULL.
 * Synchronises the sampler's stream. */
int mceik_mcmc_gather(mceik_mcmc *s, mceik_comm *c, int which, int nchains_total, int root, int *v_out,
                      double *logl_out);

/* ---- discrete adjoint of the batched solve (csrc/adjoint.hip)
 * For every solve (model m, station s) of a finished batch and adjoint weights
 * ev_w[solve][e] on its event times, the exact derivative of
 *   J = sum_e ev_w[solve][e] * t(solve, e)
 * of the first-order solver with respect to the slowness of every inversion
 * cell (slow_mode 1) or node (slow_mode 0), all cells at once: one adjoint
 * solve per (model, station).  t(solve, e) is the table value the forward
 * samples (the node ev_node, or with ev_frac the trilinear value; ev_stride as
 * in the forward).  Arithmetic: fp64 on (double)u, IEEE + - * / and the sqrt of
 * the boundary distance, no contraction, fixed summation orders, no atomics:
 * the results do not depend on the launch, max_groups or the schedule
 * (DESIGN.md s.17 gives every operation).
 *
 * `batch` gives the geometry, precision, slowness (slow, slow_mode, nr*,
 * model_phase, nphase), sources (src; nsrc must be 1), events (nev, ev_node,
 * ev_frac, ev_stride) and skip of the forward; its output pointers are not
 * used.  u: the forward's fields (mceik_fsm_batch.u_out of the same batch,
 * [nsolve][nz][ny][nx], fp32 or fp64 as batch->precision).  A solve of a skip
 * row reads no field and yields zeros, niter 0, status 0.
 *
 * Outputs (device; any may be NULL): grad [nmodel][ncell] = the model's solves
 * summed in station order (ncell = ncz ncy ncx, or nz ny nx in slow_mode 0),
 * grad_solve [nsolve][ncell], lam [nsolve][nz ny nx] = the adjoint field (with
 * unit weights the sensitivity / coverage of the picks), niter [nsolve] =
 * iterations of eight sweeps run, the verifying one included, status [nsolve]:
 * 0 converged, 1 the cap was hit (the outputs are those of the last
 * iteration), 2 the source's boundary box leaves the grid (the forward's ierr
 * 1; zeros).  maxit: cap on the iterations (0 = batch->maxit).  max_groups:
 * cap on the resident workgroups (0 = 256); a workgroup runs its solves one
 * after the other in its slice of the workspace, which is sized by the
 * resident workgroups, not by the solves.  With grad and without grad_solve a
 * workgroup takes a whole model (its stations in order).
 *
 * check: 0, or 1 with the reason on stderr (host only, no GPU call): NULL
 * description, batch or u, a batch mceik_fsm_check refuses, nsrc != 1, events
 * without ev_node or ev_w, a bad ev_stride, negative maxit or max_groups.
 * solve enqueues on `stream` (no host synchronisation, no allocation) and
 * returns 0, 1 (check, workspace too small) or -1 (device failure). */
typedef struct mceik_fsm_adjoint {
    const mceik_fsm_batch *batch;
    const void *u;              /* device [nsolve][nz*ny*nx]                  */
    const double *ev_w;         /* device [nsolve][nev]                       */
    double *grad;               /* device [nmodel][ncell] or NULL             */
    double *grad_solve;         /* device [nsolve][ncell] or NULL             */
    double *lam;                /* device [nsolve][nz*ny*nx] or NULL          */
    int *niter, *status;        /* device [nsolve] or NULL                    */
    int maxit;                  /* 0: batch->maxit                            */
    int max_groups;             /* 0: 256                                     */
} mceik_fsm_adjoint;
size_t mceik_fsm_adjoint_workspace_bytes(const mceik_fsm_adjoint *d);
int mceik_fsm_adjoint_check(const mceik_fsm_adjoint *d);
int mceik_fsm_adjoint_solve(const mceik_fsm_adjoint *d, void *workspace, size_t workspace_bytes, void *stream);

/* ---- gradient-informed (discrete Langevin) moves (csrc/lang.hip)
 * Off by default; with it off nothing changes.  Every other velocity proposal
 * draws its cell and its sign without looking at the data.  A Langevin step
 * moves every cell of one phase model of a chain at once, each cell biased
 * along the exact gradient of the chain's log posterior (the discrete adjoint
 * above plus the prior's gradient): the discrete Langevin proposal of Zhang,
 * Liu & Liu 2022 on the integer velocities.  The proposal is not symmetric, so
 * the accept test carries a Hastings term, which costs a second gradient at
 * the proposed state: a step is two forwards with fields and two adjoint
 * batches of the drawn model, all on the GPU.
 *
 * Global step gs is a Langevin step iff gs % every == offset and it is neither
 * a hypocentre nor a nuisance step.  It replaces that step's velocity proposal
 * (single-cell or block); the kept-state, posterior, covariance, moments and
 * swap-round rules apply as on any velocity step.  For chain c (global id g,
 * beta its inverse temperature):
 *   step draw  r = Philox4x32-10(counter {(uint32)gs, (uint32)(gs >> 32), 4, 0xFFFFFFFF}, key {g, seed})
 *              (counter word 2: proposals 0, swaps 1, hypocentres 2, nuisance moves 3)
 *              ph = (r0 * nphase) >> 32: every cell of model ph moves, no other;
 *              log u = det_log((r3 + 0.5) / 2^32)
 *   cell draw  counter {.., .., 4, i} for cell i of the model: u_i = (r0 + 0.5) / 2^32
 *   drift      d_i = beta * g_i + gp_i (untempered: no multiply), g_i = d logL / d v_i
 *              of the chain's current state = -(gs_i / (v_i * v_i)) with gs the
 *              adjoint's slowness gradient under the pick weights d logL / d t
 *              (station flags, hypocentres, noise scale, statics and tt_interp
 *              honoured); gp_i = 0.0 with the prior off, else
 *              -(ws * (double)(2 * sum_nb (v_i - v_nb)) + wd * (double)(2 * (v_i - vref_i)))
 *              over the face neighbours, exact integers (no vref: the second is 0)
 *   proposal   with c = 1 / (2 sigma sigma) and the support delta = lo..hi, lo =
 *              max(-dmax, vlo - v_i), hi = min(dmax, vhi - v_i) ([vlo, vhi] the
 *              phase's box, which is therefore never left):
 *                a(delta) = (0.5 * d_i) * (double)delta - c * (double)(delta * delta)
 *                amax = max a, w(delta) = det_exp(a(delta) - amax), Z = 0.0 + w(lo) + .. + w(hi)
 *                delta_i = the first delta with cum + w(delta) > u_i * Z (cum from 0.0 in
 *                support order), else hi;  log q_i(delta) = (a(delta) - amax) - det_log(Z)
 *   lqf        = sum_i log q_i(delta_i), reduced without atomics: partial l of 256
 *              adds cells l, l + 256, .. in order from 0.0, the total adds the
 *              partials in order from 0.0
 *   reverse    at v' = v + delta the same forward, pick weights and adjoint give g',
 *              d' uses g' and the prior's gradient at v', the supports are rebuilt
 *              about v', lqr = sum_i log q'_i(-delta_i)
 *   accept iff log u < beta * (logL' - logL) + (lqr - lqf)
 *              (prior on: log u folded with the exact differences of the full
 *              integer energies of v' and v, as in the prior's accept rule)
 * in IEEE double without contraction; det_exp is the deterministic exp next to
 * the sampler's log (mceik_det_exp).  A chain one of whose adjoint solves
 * returned a nonzero status, or one of whose forwards a nonzero ierr, at
 * either state, rejects and counts as failed.  No gradient is kept between
 * steps.  A tempering swap needs nothing new.
 *
 * Memory: a forward with fields stores each field twice, so a pipe walks its
 * chains in chunks sized so that fields, workspaces and pick weights of all
 * pipes stay under mem_bytes (0: 2 GiB); the chunk size and the number of
 * pipes do not change a bit of the result.  Everything is allocated at
 * enable.  While enabled every step is one launch of each kernel
 * (mceik_mcmc_info.multi_step reports 0 until disable).
 *
 * enable returns 1 on NULL options, every <= 0, an offset outside [0, every),
 * sigma <= 0, dmax < 1 or above MCEIK_LANG_DMAX_CAP, and a budget too small for
 * one chain of a pipe.  The other functions return 1 before the first enable.
 * Every function returns 0, 1 on invalid arguments or -1 on a device failure. */
#define MCEIK_LANG_DMAX_CAP 32
typedef struct mceik_lang_opts { int every, offset; double sigma; int dmax; size_t mem_bytes; } mceik_lang_opts;
/* Turns the moves on (or replaces the options); resets the counters.  Synchronises. */
int mceik_mcmc_lang_enable(mceik_mcmc *s, const mceik_lang_opts *o);
/* Later steps are the sampler's other velocity proposals again. */
int mceik_mcmc_lang_disable(mceik_mcmc *s);
/* The options in force (every = 0 after disable; o may be NULL) and the chunk,
 * in chains, of every pipe (chunk [npipe] or NULL). */
int mceik_mcmc_lang_get(mceik_mcmc *s, mceik_lang_opts *o, int *chunk);
/* Over the chains: Langevin steps tried, accepted, failed (a solve's status),
 * and cells with delta != 0 of the accepted steps.  Any may be NULL.  Synchronises. */
int mceik_mcmc_lang_stats(mceik_mcmc *s, long long *attempts, long long *accepts, long long *failed, long long *moved,
                          int reset);
/* The last Langevin step: phase [nchains], delta [nchains][ncell] of that
 * phase's model, lqf, lqr, logL' [nchains], accept [nchains], status [nchains]
 * (1: failed).  Any may be NULL.  Synchronises. */
int mceik_mcmc_lang_last(mceik_mcmc *s, int *phase, int *delta, double *lqf, double *lqr, double *logl_prop,
                         unsigned char *accept, int *status);
/* Host only (no GPU call), the arithmetic the kernels run.  det_exp: x < -708
 * gives 0, x > 709 inf, a NaN itself.  lang_cell: the proposal of cell `cell`
 * of global chain gchain at global step `step` with drift d at velocity v in
 * the box [vlo, vhi]: the drawn delta, the support's ends lo, hi and logq [hi -
 * lo + 1] of every support value (room for 2 dmax + 1; any output may be
 * NULL); 1 on sigma <= 0, dmax outside [1, cap], v outside the box. */
double mceik_det_exp(double x);
int mceik_lang_cell(uint32_t seed, uint32_t gchain, uint64_t step, int cell, double d, int v, int vlo, int vhi,
                    double sigma, int dmax, int *delta, int *lo, int *hi, double *logq);

/* ---- differential-evolution (population) moves (csrc/de.hip)
 * Off by default; with it off nothing changes.  The chains of a sampler all
 * sample the same posterior, so the spread of their current states estimates
 * its scale and correlations.  A DE step (DE-MC, ter Braak 2006, with the
 * crossover of DREAM, Vrugt et al. 2009) proposes v + gamma (v_a - v_b) on one
 * phase model of a chain from two other chains a, b.  It moves a whole model,
 * it is symmetric (no gradient, no Hastings term) and it costs one forward per
 * moving chain, as a single-cell step does.  Everything up to the accept test
 * is integer arithmetic, so the proposal is symmetric exactly.
 *
 * Options: every, offset; gq = gamma_q16 = round(gamma * 65536) in [1, 131072];
 * crq = cr_q16 = round(cr * 65536) in [1, 65536] (cr: the probability that a
 * cell takes part).
 *
 * Global step gs is a DE step iff gs % every == offset and it is neither a
 * hypocentre, a nuisance nor a Langevin step; it replaces that step's velocity
 * proposal.  A swap round that falls on the step runs first.  DE step k = (gs
 * - offset) / every has parity par = k & 1 and phase ph = (k >> 1) % nphase,
 * common to all chains.
 *   populations  the population of a chain is its temperature rung on this
 *              sampler: rung r holds local chains r * G + g, g in [0, G)
 *              (untempered: one rung, G = nchains).  Chains with (g & 1) == par
 *              are the step's movers; the others of the rung, ordered by g, are
 *              its partner set of nb members and stand still: no proposal, no
 *              forward, accept = 0, state, logL and naccept untouched.  (Movers
 *              that read each other while both move would not leave the product
 *              posterior invariant; with the partner set fixed each mover's
 *              kernel is a symmetric Metropolis kernel for a fixed pair set.)
 *   step draw  of mover c (global id g): r = Philox4x32-10(counter {(uint32)gs,
 *              (uint32)(gs >> 32), 5, 0xFFFFFFFF}, key {g, seed})
 *              (counter word 2: proposals 0, swaps 1, hypocentres 2, nuisance
 *              moves 3, Langevin 4);  i = (r0 * nb) >> 32;  j = (r1 * (nb - 1))
 *              >> 32, j += (j >= i);  r2 & 1: i and j swap;  a, b = the i-th and
 *              j-th members of the partner set;  log u = det_log((r3 + 0.5) / 2^32)
 *   cell n     of phase ph: w = word n & 3 of Philox(counter {.., .., 5, n >> 2});
 *              the cell takes part iff (w >> 16) < crq; then with d = v_a[n] -
 *              v_b[n] and rr = w & 0xFFFF
 *                delta = (2 * gq * d + 2 * rr + 1) >> 17    (int64, arithmetic shift)
 *              = floor((gq d + rr + 0.5) / 65536), else delta = 0.  The numerator
 *              is odd, so delta(d, rr) == -delta(-d, 65535 - rr) always: with the
 *              swap bit the reverse move is exactly as likely as the move.
 *              v' = v + delta on phase ph; the other phase does not change.
 *   box        a cell of v' outside [vmin, vmax] (phase 1: [vsmin, vsmax])
 *              rejects the whole move (clamping a cell, or leaving it unmoved,
 *              would not be symmetric).  Its forward still runs -- on v' with
 *              those cells left at v -- and is never read; logL' is reported
 *              as logL.
 *   accept iff v' is inside the box, no unskipped solve of the mover failed
 *              (ierr) and log u < beta * (logL' - logL), log u folded with the
 *              exact differences of the prior's full integer energies of v'
 *              and v when the prior is on; logL' honours moved hypocentres,
 *              noise scale and statics.
 * A kept step keeps every chain, standing ones included.  After a DE step
 * mceik_mcmc_last's accept is 0 for standing chains, only the movers' table
 * rows are the step's, and mceik_mcmc_last_phase is ph for all chains.
 * Whether the move pays in effective samples per second depends on the
 * problem; tools/ess_compare.py measures it.
 *
 * enable returns 1 (with a message) on a population of fewer than 4 chains,
 * every < 1, an offset outside [0, every), gq or crq out of range; tempering
 * cannot be switched to rungs of fewer than 4 chains while DE moves are on.
 * While enabled every step is one launch of each kernel (mceik_mcmc_info.
 * multi_step reports 0 until disable).  The other functions return 1 before
 * the first enable.  Every function returns 0, 1 on invalid arguments or -1 on
 * a device failure. */
typedef struct mceik_de_opts { int every, offset, gamma_q16, cr_q16; } mceik_de_opts;
/* Turns the moves on (or replaces the options); resets the counters.  Synchronises. */
int mceik_mcmc_de_enable(mceik_mcmc *s, const mceik_de_opts *o);
/* Later steps are the sampler's other velocity proposals again. */
int mceik_mcmc_de_disable(mceik_mcmc *s);
/* The options in force (every = 0 after disable; o may be NULL). */
int mceik_mcmc_de_get(mceik_mcmc *s, mceik_de_opts *o);
/* Over the chains: DE moves tried, accepted, rejected for leaving the box,
 * failed (a solve's ierr), and cells with delta != 0 of the accepted moves.
 * Any may be NULL.  Synchronises. */
int mceik_mcmc_de_stats(mceik_mcmc *s, long long *attempts, long long *accepts, long long *outbox, long long *failed,
                        long long *moved, int reset);
/* The last DE step: mover [nchains] (1: the chain moved), a, b [nchains] (the
 * partners as local chains; -1 for standing chains), *phase (-1: no DE step
 * yet), nmove [nchains] (cells with delta != 0), inbox, status (1: failed),
 * logL' [nchains] (logL where the move left the box or failed; 0 for standing
 * chains), accept [nchains].  Any may be NULL.  Synchronises. */
int mceik_mcmc_de_last(mceik_mcmc *s, int *mover, int *a, int *b, int *phase, int *nmove, int *inbox, int *status,
                       double *logl_prop, unsigned char *accept);
/* Host only (no GPU call), the arithmetic the kernels run.  de_delta: the move
 * of a cell whose partners differ by d under the cell's word; 1 on gq or crq
 * out of range.  de_draw: the ordered pair i != j in [0, nb) and log u of
 * global chain gchain at global step `step`; 1 on nb < 2. */
int mceik_de_delta(int gq, int d, uint32_t word, int crq, int *delta);
int mceik_de_draw(uint32_t seed, uint32_t gchain, uint64_t step, int nb, int *i, int *j, double *logu);

/* ---------------------------------------------------------------------------
 * Transdimensional Voronoi-cell models (no reference
 * counterpart).  Off by default.  While on, each phase model of each chain is a
 * list of k nuclei (inversion cell, int velocity), kmin <= k <= kmax <=
 * MCEIK_VOR_KMAX (512), in distinct cells, and the chain's cell model v is
 * their raster:
 *   v[cell] = the value of the nucleus minimising d2 = (mx dx)^2 + (my dy)^2 +
 *             (mz dz)^2 (differences of cell indices per axis; metric = (mx,
 *             my, mz)), ties to the nucleus in the smaller cell.
 * List order is state (a birth appends, a death of slot j moves the last slot
 * into j) but never changes v.  Every step that would propose a single cell is
 * a Voronoi step instead; hypocentre and nuisance steps and swap rounds run as
 * before (a swap exchanges the nuclei with the models).  Voronoi step n (n
 * counts such steps below the global step under the options in force) works on
 * phase n % nphase.  Global chain g at global step gs draws Philox4x32-10, key
 * {g, seed}, counters {gs lo, gs hi, 6, 0} -> a0..a3 and {gs lo, gs hi, 6, 1}
 * -> b0..b3; idx(r, n) = floor(r n / 2^32):
 *   type = a0 >> 30   0 value: nucleus j = idx(a1, k) moves by delta = +-(1 +
 *                       idx(a2, dv)), minus iff a0 & 1; leaving the box rejects
 *                     1 move: nucleus j moves by (idx(a2, 2 dmax_x + 1) - dmax_x,
 *                       idx(b0, ..y..) - dmax_y, idx(b1, ..z..) - dmax_z) cells;
 *                       a zero displacement, a target outside the grid and a
 *                       target cell that holds a nucleus each reject
 *                     2 birth: k == kmax rejects; else a nucleus in the
 *                       idx(a1, ncell - k)-th free cell, ascending, with value
 *                       vlo + idx(a2, vhi - vlo + 1) (a draw from the prior)
 *                     3 death: k == kmin rejects; else nucleus j goes
 *   log u = det_log((a3 + 0.5) / 2^32)
 * The prior is uniform on k, on sets of k distinct cells and on values, so
 * every Hastings factor cancels: accept iff the move was not rejected above and
 * log u < beta (logL' - logL), logL' honouring moved hypocentres, noise scale
 * and statics.  A rejected move still runs the step's forward.
 *
 * enable takes the caller's nuclei (cells, vals [nchains][nphase][kmax], counts
 * [nchains][nphase]; validated) or, all three NULL, draws k0 distinct cells per
 * chain and phase (nucleus i in free cell idx(r0, ncell - i) of counter {i,
 * phase, 6, 0xFFFFFFFF}, key {g, seed}), each with the chain's current v of its
 * cell; it then rasters every model and recomputes every logL with one full
 * forward.  It returns 1 (with a message, nothing changed) on options out of
 * range, a grid / metric whose largest d2 does not fit 31 bits, invalid nuclei,
 * or while block proposals, the smoothness prior, Langevin moves or DE moves
 * are on; those four refuse to be enabled while Voronoi-cell models are on.
 * disable leaves v as it stands.  While on, every step is one launch of each
 * kernel (mceik_mcmc_info.multi_step reports 0), and mceik_mcmc_restore's v
 * must be the raster of the nuclei in force (set them first).  The other
 * functions return 1 before the first enable.  Every function returns 0, 1 on
 * invalid arguments or -1 on a device failure. */
#define MCEIK_VOR_KMAX 512
typedef struct mceik_vor_opts { int kmin, kmax, k0, dv; int dmax[3]; int metric[3]; } mceik_vor_opts;
/* Turns the models on (or replaces options and nuclei); resets the counters. */
int mceik_mcmc_vor_enable(mceik_mcmc *s, const mceik_vor_opts *o, const int *cells, const int *vals, const int *counts);
int mceik_mcmc_vor_disable(mceik_mcmc *s);
/* The options, *on, and the nuclei ([nchains][nphase][kmax], counts [nchains][nphase]).  Any may be NULL. */
int mceik_mcmc_vor_get(mceik_mcmc *s, mceik_vor_opts *o, int *on, int *cells, int *vals, int *counts);
/* Replaces the nuclei (validated: counts in range, distinct cells, values in
 * the box; 1 and nothing changed otherwise), rasters them and, with recompute,
 * recomputes every logL with one full forward. */
int mceik_mcmc_vor_set(mceik_mcmc *s, const int *cells, const int *vals, const int *counts, int recompute);
/* Queues the raster of every model from the nuclei in force on the sampler's
 * stream (v, and both slowness rows; no synchronisation).  It changes nothing
 * -- v is that raster already -- and exists to be timed (tools/vor_cost.py). */
int mceik_mcmc_vor_rasterize(mceik_mcmc *s);
/* counters [4][5] over the chains, by move type: attempts, accepts, rejections
 * for reason 1, 2, 3 (value: 1 left the box; move: 1 zero displacement, 2
 * outside the grid, 3 occupied; birth: 1 k == kmax; death: 1 k == kmin). */
int mceik_mcmc_vor_stats(mceik_mcmc *s, long long *counters, int reset);
/* The last Voronoi step: *phase (-1: none yet); rec [nchains][8] = type, reason
 * (0: not rejected before the forward), j (birth: the new slot, -1 when
 * rejected), cell, value of the changed nucleus as proposed (cell -1: outside
 * the grid or no birth), k', 0, 0; the proposed nuclei [nchains][kmax] (the
 * first k'; the current ones where rejected); vprop [nchains][ncell], their
 * raster (the stepped phase's proposed model); log u, logL' (logL where
 * rejected before the forward) and accept [nchains].  Any may be NULL. */
int mceik_mcmc_vor_last(mceik_mcmc *s, int *phase, int *rec, int *pcells, int *pvals, int *vprop, double *logu,
                        double *logl_prop, unsigned char *accept);
/* Exact sums over the kept states' cold chains: *n states, hist [nphase][kmax +
 * 1] states by k, dens [nphase][ncell] states with a nucleus in the cell.
 * They merge by addition; _set loads them (checkpoints). */
int mceik_mcmc_vor_moments(mceik_mcmc *s, long long *n, unsigned long long *hist, unsigned long long *dens);
int mceik_mcmc_vor_moments_set(mceik_mcmc *s, long long n, const unsigned long long *hist, const unsigned long long *dens);
/* Host only (no GPU call), the arithmetic the kernels run.  vor_raster: v [ncx
 * ncy ncz] of k >= 1 nuclei; 1 on invalid arguments.  vor_free_cell: the f-th
 * (from 0) cell in ascending order holding none of the k nuclei, f < ncell - k;
 * -1 on invalid arguments.  vor_draw: out [8] = type, j, f, signed delta, the
 * birth value, dx, dy, dz of global chain gchain at global step `step` for a
 * model of k nuclei, and log u. */
int mceik_vor_raster(int ncx, int ncy, int ncz, const int *metric, const int *cells, const int *vals, int k, int *v);
int mceik_vor_free_cell(const int *cells, int k, int ncell, int f);
int mceik_vor_draw(uint32_t seed, uint32_t gchain, uint64_t step, int k, int ncell, int dv, int vlo, int vhi,
                   const int *dmax, int *out, double *logu);

/* ---- the likelihood's norm (csrc/l1.h) ------------------
 * norm = 2 (default): the weighted L2 misfit with the analytic origin time.
 * norm = 1: a Laplace density of scale var_j per pick, the origin time of an
 * event its lower weighted median.  For the used picks j of event e in
 * catalogue order, x_j = (tobs_j - tcorr_j) - te_j and w_j = 1 / var_j:
 *   W = sum_j w_j;  s_k = sum_j ((x_j < x_k || (x_j == x_k && j <= k)) ? w_j : 0)
 *   t0 = the smallest x_k with s_k >= 0.5 W;  objfn_e = sum_j w_j |x_j - t0|
 * (every sum in ascending j; no used pick: 0) and logL = -sum_e objfn_e, plus
 * the noise-ladder term of held nuisance state as under L2.  The norm is a
 * property of the sampler: the single-cell, block, DE and Voronoi accepts,
 * hypocentre and nuisance moves, tempering swaps and the data-fit stream (whose
 * origin time becomes the median) all follow it.  While norm = 1 every step is
 * one launch of each kernel (mceik_mcmc_info.multi_step reports 0).
 *
 * set recomputes every chain's logL under the new norm with one full forward;
 * the step counter and the models are untouched.  It returns 1, with nothing
 * changed, for a norm other than 1 or 2, while Langevin moves are on, or while
 * an enabled accumulator of kept states (posterior, covariances, batch means,
 * data fit, the hypocentre / nuisance / Voronoi moments) already holds states;
 * 2 when a solve of the forward failed; -1 on a device failure.
 * mceik_mcmc_lang_enable is refused while norm = 1.  get returns 1 or 2 (0:
 * null handle).  A checkpoint does not carry the norm: the caller restores
 * into a sampler of the same norm (mceik_amd.mcmc.Sampler does). */
int mceik_mcmc_likelihood_set(mceik_mcmc *s, int norm);
int mceik_mcmc_likelihood_get(const mceik_mcmc *s);
/* Host only (no GPU call): the event objective above on n residuals x with
 * weights w (mask may be NULL; 1 = not used); *t0 (may be NULL) the median. */
int mceik_l1_event(int n, const int *mask, const double *x, const double *w, double *t0, double *obj);

#ifdef __cplusplus
}
#endif
#endif
