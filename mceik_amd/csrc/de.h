// de.h -- differential-evolution (population) moves of the sampler (de.hip;
// include/mceik.h mceik_mcmc_de_*): device state, the integer
// proposal (host and device) and launchers (not public).
//
// A DE step proposes v + gamma (v_a - v_b) on one phase model of a chain from
// two other chains of its population (its temperature rung on this sampler).
// The chains of a rung split by the parity of their index in it: one half
// moves, the other half stands still and is the partner set the movers draw a
// and b from, so each mover's kernel is a symmetric Metropolis kernel for a
// fixed pair set.  Everything up to the accept test is integer arithmetic: the
// proposal is exactly symmetric and needs no gradient and no Hastings term.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block.h"
#include "hypo.h"
#include "mcmc_common.h"
#include "nuis.h"
#include "prior.h"

#define MCEIK_DE_STREAM 5u         // counter word 2: proposals 0, swaps 1, hypocentres 2, nuisance moves 3, Langevin 4
#define MCEIK_DE_GQ_MAX 131072     // gamma <= 2 in units of 1 / 65536
#define MCEIK_DE_CRQ_MAX 65536     // crossover probability <= 1 in units of 1 / 65536
#define DE_THREADS 256             // one workgroup per mover (per chain in the accept)

// Per-chain arrays are views (sampler.hip dev_view): a pipe's DeDev points at
// its chains' rows, and its compact buffers at rows [0, its movers) of its own
// part.  vall, G and the mover lists are the sampler's.
struct DeDev {
    int gq, crq;                   // round(gamma 65536), round(cr 65536)
    int G;                         // chains per population: the sampler's nchains / rungs
    int off;                       // the pipe's first chain in the sampler (mover lists and a, b count from the sampler's)
    const int *vall;               // the sampler's D.v: partners may be another pipe's chains
    const unsigned char *skip;     // [nphase][nstat] the sampler's skip rows, or null
    const int *mov[2];             // the pipe's movers of parity 0 / 1, ascending (chains of the sampler)
    int nmov[2];
    int *a, *b;                    // [nchains] last DE step: the partners (chains of the sampler), -1: stood still
    int *inbox, *nmove, *status;   // [nchains] last DE step: v' inside the box, cells with delta != 0, 1: a solve failed
    double *logl_prop;             // [nchains] last DE step: logL' (in the box and no failure, else logL)
    int *vprop;                    // [nchains][nphase][ncell] the movers' proposed models
    unsigned long long *pen;       // [4][nchains * nphase] Es, Ed at v | Es, Ed at v' (prior on)
    size_t pen_stride;             // the sampler's nchains * nphase
    unsigned long long *cnt;       // [nchains][5] attempts, accepts, out of box, failed, cells moved
    // the forward's compact batch: row m is the pipe's m-th mover
    float *slow;                   // [nmov][ncell] the proposed model of the step's phase
    float *ttab;                   // [nmov][nstat][nev]
    int *ierr, *niter;             // [nmov][nstat]
    int *ev;                       // [nmov][nev] the movers' event nodes (per-chain hypocentres), else unused
    // where de_scatter puts them: the pipe's rows of the step batch
    float *ttab_out;               // [nchains][nstat][nev]
    int *ierr_out, *niter_out;     // [nchains][nstat]
};

static inline __host__ __device__ void de_philox(uint32_t seed, uint32_t g, uint64_t gs, uint32_t w3, uint32_t r[4])
{
    r[0] = (uint32_t)gs; r[1] = (uint32_t)(gs >> 32); r[2] = MCEIK_DE_STREAM; r[3] = w3;
    nuis_philox(r, g, seed);
}

// The step draw of global chain g at step gs from a partner set of nb >= 2:
// the ordered pair i != j of its members; returns r3 (log u = det_log((r3 +
// 0.5) / 2^32)).  Bit 0 of r2 swaps the pair, so both orders are equally likely.
static inline __host__ __device__ uint32_t de_draw(uint32_t seed, uint32_t g, uint64_t gs, int nb, int *pi, int *pj)
{
    uint32_t r[4];
    de_philox(seed, g, gs, 0xFFFFFFFFu, r);
    int i = (int)(((uint64_t)r[0] * (uint32_t)nb) >> 32);
    int j = (int)(((uint64_t)r[1] * (uint32_t)(nb - 1)) >> 32);
    j += j >= i;
    if (r[2] & 1u) { const int t = i; i = j; j = t; }
    *pi = i; *pj = j;
    return r[3];
}

// The move of a cell whose partners differ by d = v_a - v_b under the cell's
// word w: 0 unless (w >> 16) < crq, else floor((gq d + rr + 0.5) / 65536) with
// rr = w & 0xFFFF.  The numerator 2 gq d + 2 rr + 1 is odd, so delta(d, rr) ==
// -delta(-d, 65535 - rr) for every input.
static inline __host__ __device__ long long de_delta(int gq, long long d, uint32_t w, int crq)
{
    if ((int)(w >> 16) >= crq) return 0;
    const long long rr = (long long)(w & 0xFFFFu);
    return (2 * (long long)gq * d + 2 * rr + 1) >> 17;
}

// Members of the partner set of a step of parity par in a population of G:
// the chains g of the rung with (g & 1) != par, the t-th being 2 t + (1 - par).
static inline __host__ __device__ int de_nb(int G, int par) { return par ? (G + 1) / 2 : G / 2; }

// The proposal of the pipe's movers of parity par on phase ph: a, b, vprop, the
// compact slowness rows (and slow_prop), the box flag, nmove, the movers' event
// nodes (H.hyp).  Reads the partners' models from L.vall.
hipError_t de_propose(const McmcDev &D, const HypoDev &H, const DeDev &L, uint64_t gs, int par, int ph, hipStream_t st);
// The compact tables, ierr and niter into the movers' rows of the step batch.
hipError_t de_scatter(const McmcDev &D, const DeDev &L, int par, hipStream_t st);
// The accept test of the movers, the commit or the revert, the counters; the
// standing chains' accept = 0; (keep_slot >= 0) the kept logL and state of every chain.
hipError_t de_accept(const McmcDev &D, const NuisDev &N, const PriorDev &P, bool prior_on, const DeDev &L, int par, int ph,
                     int keep_slot, hipStream_t st);
