// hypo.h -- hypocentre moves of the GPU sampler (hypo.hip; include/mceik.h
// mceik_mcmc_hypo_*): device state and launchers (not public).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_common.h"
#include "nuis.h"

// Per-chain arrays are views (sampler.hip dev_view): a pipe's HypoDev points
// at its chains' rows.  The counters and moments are the sampler's.
struct HypoDev {
    int nx, ny, nz;                // the eikonal grid (node = (iz * ny + iy) * nx + ix)
    int dmx, dmy, dmz;             // largest move per axis (nodes)
    int lox, loy, loz, hix, hiy, hiz;   // the box (nodes, inclusive)
    int *hyp;                      // [nchains][nev][3] current nodes (ix, iy, iz)
    int *ev1;                      // [nchains][nev] their linear nodes: the velocity steps' event lists
    int *evall;                    // nphase 2: [nchains][nphase][nev] the same per model (the full forward), else null
    int *ev2;                      // [nchains][nphase][2 nev] = current | candidate: a hypocentre step's lists
    float *ttab2;                  // [nchains][nphase][nstat][2 nev] a hypocentre step's tables
    int *cand;                     // [nchains][nev][3] last hypocentre step: current + d
    unsigned char *acc;            // [nchains][nev] last hypocentre step: accepted
    double *obj;                   // [nchains][nev][2] last hypocentre step: objfn at current, candidate
    double *logu;                  // [nchains][nev] last hypocentre step: log u
    unsigned long long *attempts, *accepts;   // [nev] over chains
    long long *mom;                // [nev][9] sums of x, y, z, xx, yy, zz, xy, xz, yz over kept cold states
};

// The draw of event e of global chain g at step gs (host and device): d[3] in
// [-dmax, dmax] per axis and the uniform's 32 bits r3 (log u = det_log((r3 +
// 0.5) / 2^32)).  Philox4x32-10, counter {gs lo, gs hi, 2, e}, key {g, seed}.
#define MCEIK_HYPO_STREAM 2u       // counter word 2: proposals 0, swaps 1

static inline __host__ __device__ void hypo_philox(uint32_t c[4], uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

static inline __host__ __device__ uint32_t hypo_draw(uint32_t seed, uint32_t g, uint64_t gs, int e, int dmx, int dmy,
                                                     int dmz, int d[3])
{
    uint32_t c[4] = {(uint32_t)gs, (uint32_t)(gs >> 32), MCEIK_HYPO_STREAM, (uint32_t)e};
    hypo_philox(c, g, seed);
    d[0] = (int)(((uint64_t)c[0] * (uint32_t)(2 * dmx + 1)) >> 32) - dmx;
    d[1] = (int)(((uint64_t)c[1] * (uint32_t)(2 * dmy + 1)) >> 32) - dmy;
    d[2] = (int)(((uint64_t)c[2] * (uint32_t)(2 * dmz + 1)) >> 32) - dmz;
    return c[3];
}

// Host twin of mcmc_device.h det_log (IEEE basic operations only).
double hypo_det_log_host(double x);

// One hypocentre step of the chains of D / H: the draw and the [current |
// candidate] lists before the forward ...
hipError_t hypo_propose(const McmcDev &D, const HypoDev &H, uint64_t gs, hipStream_t st);
// ... and, after it, the per-event accepts, then the chains' logL (and kept logL / state: keep_slot >= 0).
hipError_t hypo_accept(const McmcDev &D, const HypoDev &H, const NuisDev &N, int keep_slot, hipStream_t st);
// Adds the first ncold chains' positions of H to the moments.
hipError_t hypo_moments(const McmcDev &D, const HypoDev &H, int ncold, hipStream_t st);
// ev1 (and evall) from hyp, every chain of D / H.
hipError_t hypo_lists(const McmcDev &D, const HypoDev &H, hipStream_t st);
