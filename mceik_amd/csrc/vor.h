// vor.h -- transdimensional Voronoi-cell models of the sampler (vor.hip;
// include/mceik.h mceik_mcmc_vor_*): device state, the integer
// draw and proposal (host and device) and launchers (not public).
//
// While the feature is on a chain's phase model is a list of k nuclei (cell,
// value), kmin <= k <= kmax, in distinct inversion cells; the cell model v the
// forward reads is their raster: v[cell] is the value of the nucleus nearest in
// the integer metric d2 = (mx dx)^2 + (my dy)^2 + (mz dz)^2, ties to the
// smaller nucleus cell.  A Voronoi step draws one of four moves (value, move,
// birth, death), each with probability 1/4; with the birth value drawn from the
// prior every Hastings factor cancels and all four accept iff
// log u < beta (logL' - logL).
//
// The draw of global chain g at global step gs: two Philox4x32-10 calls, key
// {g, seed}, counters {gs lo, gs hi, 6, 0} -> a[0..3] and {gs lo, gs hi, 6, 1}
// -> b[0..3]; idx(r, n) = floor(r n / 2^32):
//   type   a0 >> 30            0 value, 1 move, 2 birth, 3 death
//   sign   a0 & 1              value: delta < 0 when set
//   j      idx(a1, k)          value, move, death: the nucleus (list slot)
//   f      idx(a1, ncell - k)  birth: the f-th free cell, ascending
//   mag    1 + idx(a2, dv)     value: |delta|
//   wnew   vlo + idx(a2, vhi - vlo + 1)   birth: the value, from the prior
//   dx     idx(a2, 2 dmax_x + 1) - dmax_x   move; dy from b0, dz from b1
//   U      a3                  log u = det_log((a3 + 0.5) / 2^32)
// Enable's start nuclei use counter {i, phase, 6, 0xFFFFFFFF}: the i-th nucleus
// sits in free cell idx(r0, ncell - i) of the i before it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_common.h"
#include "nuis.h"

#define MCEIK_VOR_STREAM 6u        // counter word 2: proposals 0, swaps 1, hypocentres 2, nuisance 3, Langevin 4, DE 5
#define MCEIK_VOR_KMAX 512         // most nuclei of one phase model (the raster stages them in LDS)
#define VOR_THREADS 256
#define VOR_TILE (4 * VOR_THREADS) // cells of one raster workgroup
#define VOR_NREC 8                 // ints per chain of the last step's record
#define VOR_NCNT 5                 // counters per move type: attempts, accepts, rejection reasons 1..3

enum { VOR_VALUE = 0, VOR_MOVE = 1, VOR_BIRTH = 2, VOR_DEATH = 3 };
// Why a move was rejected before its forward (0: it was not).  value: 1 the
// value left the box.  move: 1 zero displacement, 2 target outside the grid, 3
// target cell occupied.  birth: 1 k == kmax.  death: 1 k == kmin.

// Per-chain arrays are views (sampler.hip dev_view): a pipe's VorDev points at
// its chains' rows.  hist and dens are the sampler's.
struct VorDev {
    int kmin, kmax, dv;
    int dmx, dmy, dmz;             // largest displacement of a move per axis (cells)
    int mx, my, mz;                // the metric
    int ncx, ncy, ncz;
    int *cell, *val;               // [nchains][nphase][kmax] the nuclei; slots >= count are not read
    int *cnt_k;                    // [nchains][nphase] their counts
    int *pcell, *pval;             // [nchains][kmax] the pending proposal's nuclei of the stepped phase
    int *pk;                       // [nchains] their count
    int *rec;                      // [nchains][VOR_NREC] last step: type, reason, j, cell, value, k', 0, 0
    double *logl_prop;             // [nchains] last step: logL' (logL where rejected before the forward)
    int *vprop;                    // [nchains][ncell] the proposed model of the stepped phase
    unsigned long long *cnt;       // [nchains][4][VOR_NCNT]
    unsigned long long *hist;      // [nphase][kmax + 1] kept states by k
    unsigned long long *dens;      // [nphase][ncell] kept states with a nucleus in the cell
};

static inline __host__ __device__ int vor_idx(uint32_t r, int n) { return (int)(((uint64_t)r * (uint32_t)n) >> 32); }

static inline __host__ __device__ void vor_philox(uint32_t seed, uint32_t g, uint32_t w0, uint32_t w1, uint32_t w3,
                                                  uint32_t r[4])
{
    r[0] = w0; r[1] = w1; r[2] = MCEIK_VOR_STREAM; r[3] = w3;
    nuis_philox(r, g, seed);
}

struct VorDraw {
    int type, minus, j, f, mag, wnew, dx, dy, dz;
    uint32_t u;
};

// The step draw of global chain g at global step gs for a phase model of k
// nuclei in a grid of ncell cells and the box [vlo, vhi] (the layout above).
static inline __host__ __device__ VorDraw vor_draw(uint32_t seed, uint32_t g, uint64_t gs, int k, int ncell, int dv,
                                                   int vlo, int vhi, int dmx, int dmy, int dmz)
{
    uint32_t a[4], b[4];
    vor_philox(seed, g, (uint32_t)gs, (uint32_t)(gs >> 32), 0u, a);
    vor_philox(seed, g, (uint32_t)gs, (uint32_t)(gs >> 32), 1u, b);
    VorDraw d;
    d.type = (int)(a[0] >> 30);
    d.minus = (int)(a[0] & 1u);
    d.j = vor_idx(a[1], k);
    d.f = vor_idx(a[1], ncell - k);
    d.mag = 1 + vor_idx(a[2], dv);
    d.wnew = vlo + vor_idx(a[2], vhi - vlo + 1);
    d.dx = vor_idx(a[2], 2 * dmx + 1) - dmx;
    d.dy = vor_idx(b[0], 2 * dmy + 1) - dmy;
    d.dz = vor_idx(b[1], 2 * dmz + 1) - dmz;
    d.u = a[3];
    return d;
}

// The move of draw d on a model of k nuclei, nucleus d.j being (cj, wj), up to
// the tests that need the whole list: returns the rejection reason (0: none so
// far), the target in *tc, *tv.  A move with reason 0 still needs its target
// cell tested for a nucleus (reason 3); a birth with reason 0 sits in free cell
// d.f (*tc = -1 here).
static inline __host__ __device__ int vor_target(const VorDraw &d, int k, int kmin, int kmax, int cj, int wj, int vlo,
                                                 int vhi, int ncx, int ncy, int ncz, int *tc, int *tv)
{
    *tc = cj; *tv = wj;
    switch (d.type) {
    case VOR_VALUE:
        *tv = wj + (d.minus ? -d.mag : d.mag);
        return *tv < vlo || *tv > vhi ? 1 : 0;
    case VOR_MOVE: {
        if (d.dx == 0 && d.dy == 0 && d.dz == 0) return 1;
        const int x = cj % ncx + d.dx, y = (cj / ncx) % ncy + d.dy, z = cj / (ncx * ncy) + d.dz;
        if (x < 0 || x >= ncx || y < 0 || y >= ncy || z < 0 || z >= ncz) { *tc = -1; return 2; }
        *tc = (z * ncy + y) * ncx + x;
        return 0;
    }
    case VOR_BIRTH:
        *tc = -1; *tv = k < kmax ? d.wnew : -1;
        return k >= kmax ? 1 : 0;
    default:
        return k <= kmin ? 1 : 0;
    }
}

// The f-th (from 0) cell in ascending order that holds none of the k nuclei,
// f < ncell - k: the fixed point of x = f + #{cells <= x}, reached from x = f
// by iteration (x never passes the answer).  List order does not matter.
static inline int vor_free_cell(const int *cells, int k, int f)
{
    int x = f;
    for (;;) {
        int n = 0;
        for (int j = 0; j < k; j++) n += cells[j] <= x;
        if (f + n == x) return x;
        x = f + n;
    }
}

// The raster of k nuclei on the host (the kernel's rule): v [ncx ncy ncz].
static inline void vor_raster_host(int ncx, int ncy, int ncz, int mx, int my, int mz, const int *cells, const int *vals,
                                   int k, int *v)
{
    for (int z = 0, c = 0; z < ncz; z++)
        for (int y = 0; y < ncy; y++)
            for (int x = 0; x < ncx; x++, c++) {
                int bd = 0, bc = -1, bv = 0;
                for (int j = 0; j < k; j++) {
                    const int cj = cells[j];
                    const int ex = mx * (cj % ncx - x), ey = my * ((cj / ncx) % ncy - y), ez = mz * (cj / (ncx * ncy) - z);
                    const int d = ex * ex + ey * ey + ez * ez;
                    if (bc < 0 || d < bd || (d == bd && cj < bc)) { bd = d; bc = cj; bv = vals[j]; }
                }
                v[c] = bv;
            }
}

// Largest d2 of a grid under a metric, or -1 when it does not fit an int.
static inline long long vor_d2max(int ncx, int ncy, int ncz, int mx, int my, int mz)
{
    const long long ex = (long long)mx * (ncx - 1), ey = (long long)my * (ncy - 1), ez = (long long)mz * (ncz - 1);
    if (ex > 46340 || ey > 46340 || ez > 46340) return -1;     // (46341^2 > 2^31 - 1 already)
    const long long d = ex * ex + ey * ey + ez * ez;
    return d < 2147483647LL ? d : -1;
}

// nrows rasters: row r has cnt[r] nuclei at cell / val + r * L.kmax and writes
// ncell ints at vout + r * vstride and their fp32 reciprocals at s1 + r *
// sstride (and s2 + r * sstride unless null).
hipError_t vor_raster(const VorDev &L, int ncell, int nrows, const int *cell, const int *val, const int *cnt, int *vout,
                      size_t vstride, float *s1, float *s2, size_t sstride, hipStream_t st);
// The proposals of Voronoi step gs on phase ph for D's chains (L the matching
// view): the draw, the proposed nuclei, their raster into vprop / slow_prop.
hipError_t vor_propose(const McmcDev &D, const VorDev &L, uint64_t gs, int ph, hipStream_t st);
// The accept test, the commit or the revert, the counters; (keep_slot >= 0) the
// kept logL and state.
hipError_t vor_accept(const McmcDev &D, const VorDev &L, const NuisDev &N, int ph, int keep_slot, hipStream_t st);
// Adds the first ncold chains' nuclei to the histogram of k and the density.
hipError_t vor_moments(const McmcDev &D, const VorDev &L, int ncold, hipStream_t st);
