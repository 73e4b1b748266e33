// block.h -- multi-cell (block) proposals of the sampler (not public; the
// C-ABI is in include/mceik.h, the definition in DESIGN.md s.12).
//
// A block proposal keeps the single-cell draw (mcmc_device.h chain_propose:
// centre cell, magnitude, sign, U) and adds a radius R in [rmin, rmax] from the
// upper 31 bits of the sign word.  Every cell of the centre's model within
// [-R, R]^3 of the centre moves by the magnitude scaled with a separable
// triangular weight, floored to an integer; R = 0 is the single-cell proposal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_common.h"
#include "nuis.h"

#define MCEIK_BLOCK_RMAX 8          // largest radius (inversion cells): 17^3 candidates

// The block state of a sampler next to its McmcDev (a struct of its own: the
// sweep kernels take McmcDev and must not change).  A pipe's view offsets the
// per-chain arrays like dev_view offsets McmcDev's.
struct BlockDev {
    int ncx, ncy, ncz;              // inversion cells per axis (ncx * ncy * ncz == McmcDev.ncell)
    int rmin, rmax;
    int *prop_amp;                  // [nchains] signed amplitude of the pending proposal (the centre's dv)
    int *prop_rad;                  // [nchains] its radius
    unsigned long long *attempts;   // [MCEIK_BLOCK_RMAX + 1] proposals by radius (the whole sampler's)
    unsigned long long *accepts;    // [MCEIK_BLOCK_RMAX + 1] accepted proposals by radius
};

// The radius of a draw: r2 is Philox output word 2 (bit 0 is the sign).
__host__ __device__ inline int block_radius(uint32_t r2, int rmin, int rmax)
{
    return rmin + (int)(((uint64_t)(r2 >> 1) * (uint32_t)(rmax - rmin + 1)) >> 31);
}

// Candidate k in [0, (2R+1)^3) of the footprint centred on cell (cx, cy, cz),
// x fastest: offset (dx, dy, dz) = (k % n - R, k / n % n - R, k / n^2 - R), n =
// 2R + 1.  Returns |dv| = floor(mag * w / (R+1)^3), w = (R+1-|dx|) (R+1-|dy|)
// (R+1-|dz|), and the target's index within the model in *cell; 0 when the
// target lies outside the grid (the footprint is clipped at the faces) or the
// floor is 0 (the cell is not touched).  mag >= 1.
__host__ __device__ inline int block_dv(int ncx, int ncy, int ncz, int cx, int cy, int cz, int R, int mag, int k,
                                        int *cell)
{
    const int n = 2 * R + 1, r1 = R + 1;
    const int dx = k % n - R, dy = (k / n) % n - R, dz = k / (n * n) - R;
    const int x = cx + dx, y = cy + dy, z = cz + dz;
    if (x < 0 || x >= ncx || y < 0 || y >= ncy || z < 0 || z >= ncz) return 0;
    const int w = (r1 - (dx < 0 ? -dx : dx)) * (r1 - (dy < 0 ? -dy : dy)) * (r1 - (dz < 0 ? -dz : dz));
    *cell = (z * ncy + y) * ncx + x;
    return (int)(((int64_t)mag * w) / (r1 * r1 * r1));
}

// Proposals of step `step` for D's chains (B the matching view), on st.
hipError_t block_propose(const McmcDev &D, const BlockDev &B, uint64_t step, hipStream_t st);
// Metropolis accept/reject of the pending block proposals and, with keep_slot
// >= 0, the kept-state copy (as mcmc_accept).
hipError_t block_accept(const McmcDev &D, const BlockDev &B, const NuisDev &N, int keep_slot, hipStream_t st);
