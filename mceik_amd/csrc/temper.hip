// temper.hip -- replica exchange between the temperature rungs of a sampler
// (include/mceik.h mceik_mcmc_temper_*), on gfx950.
//
// Rung r of replica group g is local chain r * G + g.  A swap round pairs rung
// r with rung r + 1 for every r of the round's parity; an accepted pair
// exchanges its two chains' STATES (model rows, slowness rows, logL, current
// tables), so a chain index keeps its temperature.  Two kernels: one thread
// per pair decides, one block per (row tile, pair) moves the rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_common.h"
#include "mcmc_device.h"
#include "temper.h"

#define TEMPER_BLOCK 256
#define TEMPER_TILE (TEMPER_BLOCK * 4 * 4)                 // dwords of a row per block: 16 KiB
#define TEMPER_MAX_GRID_Y 65535

namespace {

// Pair p: lower chain a = p (rung r = p / G), upper chain b = p + G.  Draws
// Philox4x32-10 with counter {gs, 1, 0} (the proposals use word 2 = 0) and
// key {global chain a, seed}; swaps iff log u < (beta_a - beta_b) (logL_b -
// logL_a).  The logL values move here, the rows in temper_exchange_kernel.
__global__ __launch_bounds__(64) void temper_decide_kernel(McmcDev D, int G, int npairs, int parity, uint64_t gs,
                                                           int *flag, unsigned long long *attempts,
                                                           unsigned long long *accepts)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= npairs) return;
    const int r = p / G;
    if ((r & 1) != parity) {
        flag[p] = 0;
        return;
    }
    const int a = p, b = p + G;
    uint32_t ctr[4] = {(uint32_t)gs, (uint32_t)(gs >> 32), 1u, 0u};
    mcmcd::philox4x32_10(ctr, (uint32_t)(D.chain_offset + a), D.seed);
    const double logu = mcmcd::det_log(((double)ctr[0] + 0.5) * (1.0 / 4294967296.0));
    const double la = D.logl[a], lb = D.logl[b];
    const int sw = logu < (D.beta[a] - D.beta[b]) * (lb - la);
    if (sw) {
        D.logl[a] = lb;
        D.logl[b] = la;
        atomicAdd(&accepts[r], 1ull);
    }
    atomicAdd(&attempts[r], 1ull);
    flag[p] = sw;
}

// The per-chain rows an accepted pair exchanges: 4-byte elements, row c of
// array k at pk + c * lenk; blockIdx.x in [tk, t(k+1)) works on array k (t0 =
// 0; an array that is not there has the tile range of its predecessor's end).
// Named members: an indexed array would be copied to scratch.
struct TemperRows {
    unsigned *p0, *p1, *p2, *p3;
    int len0, len1, len2, len3;
    int t1, t2, t3, t4;
};

__device__ __forceinline__ void temper_swap16(unsigned *ra, unsigned *rb, int i0, int len)
{
    // four 16-byte accesses per lane and row in flight, TEMPER_BLOCK * 4 dwords apart
    const int s = TEMPER_BLOCK * 4, i1 = i0 + s, i2 = i1 + s, i3 = i2 + s;
    const bool q0 = i0 + 4 <= len, q1 = i1 + 4 <= len, q2 = i2 + 4 <= len, q3 = i3 + 4 <= len;
    uint4 a0, a1, a2, a3, b0, b1, b2, b3;
    if (q0) { a0 = *reinterpret_cast<const uint4 *>(ra + i0); b0 = *reinterpret_cast<const uint4 *>(rb + i0); }
    if (q1) { a1 = *reinterpret_cast<const uint4 *>(ra + i1); b1 = *reinterpret_cast<const uint4 *>(rb + i1); }
    if (q2) { a2 = *reinterpret_cast<const uint4 *>(ra + i2); b2 = *reinterpret_cast<const uint4 *>(rb + i2); }
    if (q3) { a3 = *reinterpret_cast<const uint4 *>(ra + i3); b3 = *reinterpret_cast<const uint4 *>(rb + i3); }
    if (q0) { *reinterpret_cast<uint4 *>(ra + i0) = b0; *reinterpret_cast<uint4 *>(rb + i0) = a0; }
    if (q1) { *reinterpret_cast<uint4 *>(ra + i1) = b1; *reinterpret_cast<uint4 *>(rb + i1) = a1; }
    if (q2) { *reinterpret_cast<uint4 *>(ra + i2) = b2; *reinterpret_cast<uint4 *>(rb + i2) = a2; }
    if (q3) { *reinterpret_cast<uint4 *>(ra + i3) = b3; *reinterpret_cast<uint4 *>(rb + i3) = a3; }
}

__device__ __forceinline__ void temper_swap4(unsigned *ra, unsigned *rb, int i0, int len)
{
    const int s = TEMPER_BLOCK, i1 = i0 + s, i2 = i1 + s, i3 = i2 + s;
    const bool q0 = i0 < len, q1 = i1 < len, q2 = i2 < len, q3 = i3 < len;
    unsigned a0, a1, a2, a3, b0, b1, b2, b3;
    if (q0) { a0 = ra[i0]; b0 = rb[i0]; }
    if (q1) { a1 = ra[i1]; b1 = rb[i1]; }
    if (q2) { a2 = ra[i2]; b2 = rb[i2]; }
    if (q3) { a3 = ra[i3]; b3 = rb[i3]; }
    if (q0) { ra[i0] = b0; rb[i0] = a0; }
    if (q1) { ra[i1] = b1; rb[i1] = a1; }
    if (q2) { ra[i2] = b2; rb[i2] = a2; }
    if (q3) { ra[i3] = b3; rb[i3] = a3; }
}

// grid (row tiles of every array, pairs): a block of an accepted pair reads
// its tile of both rows into registers and writes them crosswise; each element
// belongs to exactly one thread, so the exchange is in place.  Lanes run along
// the row.  16-byte accesses when both rows start on a 16-byte boundary (the
// tile start is a multiple of 16 KiB into the row), the row's last len % 4
// dwords by the block that holds them; one dword per lane and access
// otherwise (an odd row length misaligns every second row).
__global__ __launch_bounds__(TEMPER_BLOCK) void temper_exchange_kernel(TemperRows R, const int *flag, int pair0, int G)
{
    const int pair = pair0 + blockIdx.y;
    if (!flag[pair]) return;
    const int bx = blockIdx.x;
    unsigned *base = bx < R.t1 ? R.p0 : bx < R.t2 ? R.p1 : bx < R.t3 ? R.p2 : R.p3;
    const int len = bx < R.t1 ? R.len0 : bx < R.t2 ? R.len1 : bx < R.t3 ? R.len2 : R.len3;
    const int t0 = bx < R.t1 ? 0 : bx < R.t2 ? R.t1 : bx < R.t3 ? R.t2 : R.t3;
    unsigned *ra = base + (size_t)pair * len, *rb = base + (size_t)(pair + G) * len;
    const int e0 = (bx - t0) * TEMPER_TILE;
    const int tid = threadIdx.x;
    if ((((uintptr_t)ra | (uintptr_t)rb) & 15) == 0) {
        temper_swap16(ra, rb, e0 + tid * 4, len);
        const int tail = len & ~3;                         // the row's last len % 4 dwords
        if (tail >= e0 && tail < e0 + TEMPER_TILE && tid < (len & 3)) {
            const unsigned ya = ra[tail + tid], yb = rb[tail + tid];
            ra[tail + tid] = yb;
            rb[tail + tid] = ya;
        }
    } else {
        for (int h = 0; h < 4; h++) temper_swap4(ra, rb, e0 + h * (TEMPER_TILE / 4) + tid, len);
    }
}

}  // namespace

hipError_t temper_swap_round(const McmcDev &D, int ntemps, int parity, uint64_t gs, int *flag,
                             unsigned long long *attempts, unsigned long long *accepts, hipStream_t st,
                             const HypoDev *H, const NuisDev *N, const VorDev *V)
{
    if (ntemps < 2 || !D.beta) return hipSuccess;
    const int G = D.nchains / ntemps, npairs = (ntemps - 1) * G;
    if (npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(temper_decide_kernel, dim3((npairs + 63) / 64), dim3(64), 0, st, D, G, npairs, parity, gs, flag,
                       attempts, accepts);
    // v, slow_cur and slow_prop rows of ncm entries; the current tables where the sampler keeps them
    const int nt = (D.ncm + TEMPER_TILE - 1) / TEMPER_TILE;
    const int ltab = D.ttab_cur ? D.nphase * D.nstat * D.nev : 0;
    TemperRows R;
    R.p0 = (unsigned *)D.v; R.p1 = (unsigned *)D.slow_cur; R.p2 = (unsigned *)D.slow_prop; R.p3 = (unsigned *)D.ttab_cur;
    R.len0 = R.len1 = R.len2 = D.ncm;
    R.len3 = ltab;
    R.t1 = nt; R.t2 = 2 * nt; R.t3 = 3 * nt;
    R.t4 = 3 * nt + (ltab + TEMPER_TILE - 1) / TEMPER_TILE;
    for (int p0 = 0; p0 < npairs; p0 += TEMPER_MAX_GRID_Y) {
        const int np = npairs - p0 < TEMPER_MAX_GRID_Y ? npairs - p0 : TEMPER_MAX_GRID_Y;
        hipLaunchKernelGGL(temper_exchange_kernel, dim3(R.t4, np), dim3(TEMPER_BLOCK), 0, st, R, flag, p0, G);
    }
    if (H && H->hyp) {
        // the positions and the event lists derived from them (hypo.h): rows of 3 nev, nev and nphase * nev ints
        auto tiles = [](int len) { return (len + TEMPER_TILE - 1) / TEMPER_TILE; };
        TemperRows Q;
        Q.p0 = (unsigned *)H->hyp; Q.p1 = (unsigned *)H->ev1; Q.p2 = (unsigned *)H->evall; Q.p3 = nullptr;
        Q.len0 = 3 * D.nev; Q.len1 = D.nev; Q.len2 = H->evall ? D.nphase * D.nev : 0; Q.len3 = 0;
        Q.t1 = tiles(Q.len0); Q.t2 = Q.t1 + tiles(Q.len1); Q.t3 = Q.t2 + tiles(Q.len2); Q.t4 = Q.t3;
        for (int p0 = 0; p0 < npairs; p0 += TEMPER_MAX_GRID_Y) {
            const int np = npairs - p0 < TEMPER_MAX_GRID_Y ? npairs - p0 : TEMPER_MAX_GRID_Y;
            hipLaunchKernelGGL(temper_exchange_kernel, dim3(Q.t4, np), dim3(TEMPER_BLOCK), 0, st, Q, flag, p0, G);
        }
    }
    if (N && N->kn) {
        // the ladder indices, the statics and the effective rows (nuis.h): rows of nphase and nphase * nstat
        // ints and of nobs doubles
        auto tiles = [](int len) { return (len + TEMPER_TILE - 1) / TEMPER_TILE; };
        TemperRows Q;
        Q.p0 = (unsigned *)N->kn; Q.p1 = (unsigned *)N->kc; Q.p2 = (unsigned *)N->var_eff; Q.p3 = (unsigned *)N->tcorr_eff;
        Q.len0 = D.nphase; Q.len1 = D.nphase * D.nstat; Q.len2 = Q.len3 = 2 * N->nobs;
        Q.t1 = tiles(Q.len0); Q.t2 = Q.t1 + tiles(Q.len1); Q.t3 = Q.t2 + tiles(Q.len2); Q.t4 = Q.t3 + tiles(Q.len3);
        for (int p0 = 0; p0 < npairs; p0 += TEMPER_MAX_GRID_Y) {
            const int np = npairs - p0 < TEMPER_MAX_GRID_Y ? npairs - p0 : TEMPER_MAX_GRID_Y;
            hipLaunchKernelGGL(temper_exchange_kernel, dim3(Q.t4, np), dim3(TEMPER_BLOCK), 0, st, Q, flag, p0, G);
        }
    }
    if (V && V->cell) {
        // the nuclei and their counts (vor.h): rows of nphase * kmax ints twice and of nphase ints
        auto tiles = [](int len) { return (len + TEMPER_TILE - 1) / TEMPER_TILE; };
        TemperRows Q;
        Q.p0 = (unsigned *)V->cell; Q.p1 = (unsigned *)V->val; Q.p2 = (unsigned *)V->cnt_k; Q.p3 = nullptr;
        Q.len0 = Q.len1 = D.nphase * V->kmax; Q.len2 = D.nphase; Q.len3 = 0;
        Q.t1 = tiles(Q.len0); Q.t2 = Q.t1 + tiles(Q.len1); Q.t3 = Q.t2 + tiles(Q.len2); Q.t4 = Q.t3;
        for (int p0 = 0; p0 < npairs; p0 += TEMPER_MAX_GRID_Y) {
            const int np = npairs - p0 < TEMPER_MAX_GRID_Y ? npairs - p0 : TEMPER_MAX_GRID_Y;
            hipLaunchKernelGGL(temper_exchange_kernel, dim3(Q.t4, np), dim3(TEMPER_BLOCK), 0, st, Q, flag, p0, G);
        }
    }
    return hipGetLastError();
}
