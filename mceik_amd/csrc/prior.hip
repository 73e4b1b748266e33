// prior.hip -- smoothness and reference-model prior of the sampler
// (include/mceik.h mceik_mcmc_prior_*), on gfx950.
//
// prior_fold_kernel runs between the proposal kernel and the forward while
// the prior is on: one 64-lane wave per chain evaluates the exact integer
// change of the two energies under the pending proposal (prior.h
// prior_delta_cell over the (2R+2)^3 lower cells, x fastest) on the unchanged
// model and rewrites prop_logu to logu - dlp.  The accept kernels and the
// sweep kernels do not know about it.  prior_energy_kernel is the full sum,
// on demand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block.h"
#include "mcmc_common.h"
#include "prior.h"

#define PRIOR_THREADS 256
#define PRIOR_CHAINS (PRIOR_THREADS / 64)
#define PRIOR_ENERGY_CELLS 4        // cells per thread of prior_energy_kernel

namespace {

__device__ __forceinline__ long long wave_sum(long long x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ __launch_bounds__(PRIOR_THREADS) void prior_fold_kernel(McmcDev D, BlockDev B, PriorDev P, int blk)
{
    const int c = blockIdx.x * PRIOR_CHAINS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= D.nchains) return;                         // whole waves leave: no barrier below
    if (!D.prop_inprior[c]) {                           // outside the box: rejected whatever the prior says
        if (lane == 0) {
            P.dE[2 * (size_t)c] = 0;
            P.dE[2 * (size_t)c + 1] = 0;
        }
        return;
    }
    const int cell = D.prop_cell[c], ph = D.prop_phase[c];
    const int cc = cell - ph * D.ncell;
    const size_t row = (size_t)c * D.ncm + (size_t)ph * D.ncell;
    const int *v = D.v + row;
    const int *vref = P.vref ? P.vref + (size_t)ph * D.ncell : nullptr;
    int amp, R;
    if (blk) {
        amp = B.prop_amp[c];
        R = B.prop_rad[c];
    } else {
        amp = D.prop_v[c] - v[cc];
        R = 0;
    }
    const int cx = cc % B.ncx, cy = (cc / B.ncx) % B.ncy, cz = cc / (B.ncx * B.ncy);
    const int m = 2 * R + 2, m3 = m * m * m;
    long long es = 0, ed = 0;
    for (int k = lane; k < m3; k += 64) prior_delta_cell(B.ncx, B.ncy, B.ncz, cx, cy, cz, R, amp, k, v, vref, &es, &ed);
    es = wave_sum(es);
    ed = wave_sum(ed);
    if (lane == 0) {
        P.dE[2 * (size_t)c] = es;
        P.dE[2 * (size_t)c + 1] = ed;
        D.prop_logu[c] = prior_fold_logu(D.prop_logu[c], ph ? P.ws1 : P.ws0, ph ? P.wd1 : P.wd0, es, ed);
    }
}

// grid: tiles blocks per (chain, phase) row of v; lanes run along the
// flattened cell index, neighbours come from the same row.
__global__ __launch_bounds__(PRIOR_THREADS) void prior_energy_kernel(McmcDev D, BlockDev B, PriorDev P, int tiles,
                                                                     unsigned long long *Es, unsigned long long *Ed)
{
    __shared__ long long part[2][PRIOR_CHAINS];
    const int r = blockIdx.x / tiles, tile = blockIdx.x % tiles;    // r = chain * nphase + phase
    const int ph = r % D.nphase;
    const int *v = D.v + (size_t)r * D.ncell;
    const int *vref = P.vref ? P.vref + (size_t)ph * D.ncell : nullptr;
    long long es = 0, ed = 0;
    for (int i = tile * PRIOR_THREADS + threadIdx.x; i < D.ncell; i += tiles * PRIOR_THREADS)
        prior_energy_cell(B.ncx, B.ncy, B.ncz, i, v, vref, &es, &ed);
    es = wave_sum(es);
    ed = wave_sum(ed);
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = es;
        part[1][threadIdx.x >> 6] = ed;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long a = 0, b = 0;
        for (int w = 0; w < PRIOR_CHAINS; w++) { a += part[0][w]; b += part[1][w]; }
        atomicAdd(&Es[r], (unsigned long long)a);
        if (vref) atomicAdd(&Ed[r], (unsigned long long)b);
    }
}

}  // namespace

hipError_t prior_fold(const McmcDev &D, const BlockDev &B, const PriorDev &P, bool blk, hipStream_t st)
{
    hipLaunchKernelGGL(prior_fold_kernel, dim3((D.nchains + PRIOR_CHAINS - 1) / PRIOR_CHAINS), dim3(PRIOR_THREADS), 0,
                       st, D, B, P, blk ? 1 : 0);
    return hipGetLastError();
}

hipError_t prior_energy(const McmcDev &D, const BlockDev &B, const PriorDev &P, unsigned long long *Es,
                        unsigned long long *Ed, hipStream_t st)
{
    const int per = PRIOR_THREADS * PRIOR_ENERGY_CELLS;
    const int tiles = (D.ncell + per - 1) / per;
    hipLaunchKernelGGL(prior_energy_kernel, dim3((unsigned)(D.nchains * D.nphase * tiles)), dim3(PRIOR_THREADS), 0, st,
                       D, B, P, tiles, Es, Ed);
    return hipGetLastError();
}
