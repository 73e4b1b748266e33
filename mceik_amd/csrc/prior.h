// prior.h -- smoothness and reference-model prior of the sampler (not public;
// the C-ABI is in include/mceik.h, the definition in DESIGN.md s.13).
//
// Per chain and phase model (ncx x ncy x ncz cells, x fastest) two exact
// integer energies: roughness Es = sum over face-adjacent pairs (v_i - v_j)^2
// and damping Ed = sum_i (v_i - vref_i)^2.  log prior = -(ws Es + wd Ed); the
// uniform box stays in force.  A pending proposal's change of both is folded
// into its threshold: prop_logu := logu - dlp, so the accept kernels stay as
// they are.  The arithmetic below is shared by the two kernels (prior.hip) and
// the host entry points mceik_prior_energy / mceik_prior_delta.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block.h"
#include "mcmc_common.h"

// The prior state of a sampler next to its McmcDev and BlockDev (the cell grid
// is BlockDev's).  A pipe's view offsets dE like dev_view offsets McmcDev's
// per-chain arrays.  Named weights: an indexed array would be copied to scratch.
struct PriorDev {
    double ws0, ws1;                // roughness weight of the P, S model: 1 / (2 sigma^2)
    double wd0, wd1;                // damping weight
    const int *vref;                // [nphase][ncell] reference model shared by the chains, null: no damping
    long long *dE;                  // [nchains][2] (dEs, dEd) of the pending / last proposal
};

// Signed dv of the footprint (block_dv) at offset (dx, dy, dz) from the centre:
// 0 outside [-R, R]^3 and outside the grid.  amp != 0 is the centre's dv.
__host__ __device__ inline int prior_dv(int ncx, int ncy, int ncz, int cx, int cy, int cz, int R, int amp, int dx,
                                        int dy, int dz)
{
    if (dx < -R || dx > R || dy < -R || dy > R || dz < -R || dz > R) return 0;
    const int n = 2 * R + 1;
    int t = 0;
    const int d = block_dv(ncx, ncy, ncz, cx, cy, cz, R, amp < 0 ? -amp : amp, ((dz + R) * n + (dy + R)) * n + dx + R,
                           &t);
    return amp < 0 ? -d : d;
}

// Lower cell k in [0, (2R+2)^3) of a proposal centred on (cx, cy, cz), x
// fastest: offset (k % m - R - 1, k / m % m - R - 1, k / m^2 - R - 1), m = 2R +
// 2.  Adds to *es the change of the cell's +x, +y and +z pairs, delta (2 (v_p -
// v_q) + delta) with delta = dv_p - dv_q, and to *ed the cell's own dv (2 (v -
// vref) + dv).  Every pair with a touched end has exactly one lower cell in
// that range, so the sum over k is E(v') - E(v).  v, vref: the phase's model
// (vref null: no damping); only cells inside the grid are read.
__host__ __device__ inline void prior_delta_cell(int ncx, int ncy, int ncz, int cx, int cy, int cz, int R, int amp,
                                                 int k, const int *v, const int *vref, long long *es, long long *ed)
{
    const int m = 2 * R + 2;
    const int dx = k % m - R - 1, dy = (k / m) % m - R - 1, dz = k / (m * m) - R - 1;
    const int x = cx + dx, y = cy + dy, z = cz + dz;
    if (x < 0 || x >= ncx || y < 0 || y >= ncy || z < 0 || z >= ncz) return;
    const int p = (z * ncy + y) * ncx + x;
    const long long dp = prior_dv(ncx, ncy, ncz, cx, cy, cz, R, amp, dx, dy, dz);
    const long long vp = v[p];
    if (dp && vref) *ed += dp * (2 * (vp - vref[p]) + dp);
    if (x + 1 < ncx) {
        const long long d = dp - prior_dv(ncx, ncy, ncz, cx, cy, cz, R, amp, dx + 1, dy, dz);
        if (d) *es += d * (2 * (vp - v[p + 1]) + d);
    }
    if (y + 1 < ncy) {
        const long long d = dp - prior_dv(ncx, ncy, ncz, cx, cy, cz, R, amp, dx, dy + 1, dz);
        if (d) *es += d * (2 * (vp - v[p + ncx]) + d);
    }
    if (z + 1 < ncz) {
        const long long d = dp - prior_dv(ncx, ncy, ncz, cx, cy, cz, R, amp, dx, dy, dz + 1);
        if (d) *es += d * (2 * (vp - v[p + ncx * ncy]) + d);
    }
}

// Cell i's share of the full energies: its +x, +y, +z pairs and its own damping term.
__host__ __device__ inline void prior_energy_cell(int ncx, int ncy, int ncz, int i, const int *v, const int *vref,
                                                  long long *es, long long *ed)
{
    const int x = i % ncx, y = (i / ncx) % ncy, z = i / (ncx * ncy);
    const long long vi = v[i];
    if (x + 1 < ncx) { const long long d = vi - v[i + 1]; *es += d * d; }
    if (y + 1 < ncy) { const long long d = vi - v[i + ncx]; *es += d * d; }
    if (z + 1 < ncz) { const long long d = vi - v[i + ncx * ncy]; *es += d * d; }
    if (vref) { const long long d = vi - vref[i]; *ed += d * d; }
}

// The folded threshold: two multiplies, one add, one negation, one subtraction
// (the build does not contract).  Zero weights give logu back bit for bit.
__host__ __device__ inline double prior_fold_logu(double logu, double ws, double wd, long long dEs, long long dEd)
{
    const double dlp = -(ws * (double)dEs + wd * (double)dEd);
    return logu - dlp;
}

// Every energy and every difference of a model of ncell cells whose values
// span at most `span` is below 2^53 in magnitude (3 pairs per cell bound the
// roughness), so it converts to double exactly.
static inline bool prior_fits(long long ncell, long long span)
{
    if (ncell < 0 || span < 0) return false;
    return (unsigned __int128)3 * (unsigned __int128)ncell * (unsigned __int128)span * (unsigned __int128)span <
           ((unsigned __int128)1 << 53);
}

// Folds the prior into the pending proposals of D's chains (B, P the matching
// views; blk: the proposals are block.hip's), on st after the proposal kernel.
hipError_t prior_fold(const McmcDev &D, const BlockDev &B, const PriorDev &P, bool blk, hipStream_t st);
// Full Es, Ed [nchains][nphase] of D's chains into zeroed device arrays, on st.
hipError_t prior_energy(const McmcDev &D, const BlockDev &B, const PriorDev &P, unsigned long long *Es,
                        unsigned long long *Ed, hipStream_t st);
