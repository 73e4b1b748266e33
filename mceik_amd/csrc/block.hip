// block.hip -- multi-cell (block) proposals of the sampler (include/mceik.h
// mceik_mcmc_block_*), on gfx950.
//
// Two kernels stand in for propose_kernel / accept_kernel while block
// proposals are on: one 64-lane wave per chain, the lanes enumerating the
// (2R+1)^3 candidates of the footprint x fastest, so the reads and writes of
// v, slow_cur and slow_prop are runs along x.  The draw, the logL
// (mcmcd::chain_loglik) and the accept test are those of the single-cell
// kernels: rmin = rmax = 0 reproduces them bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block.h"
#include "mcmc_common.h"
#include "mcmc_device.h"
#include "mcmc_host.h"
#include "nuis.h"

#define BLOCK_THREADS 256
#define BLOCK_CHAINS (BLOCK_THREADS / 64)

namespace {

__device__ __forceinline__ bool wave_all(bool p) { return __ballot(!p) == 0ull; }

// One proposal per chain (wave): the draw of chain_propose plus the radius;
// pass 1 tests the prior over the footprint (reduced over the wave), pass 2
// writes the proposed slowness when every touched entry stays inside it.
__global__ __launch_bounds__(BLOCK_THREADS) void block_propose_kernel(McmcDev D, BlockDev B, uint64_t step)
{
    const int c = blockIdx.x * BLOCK_CHAINS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= D.nchains) return;                         // whole waves leave: no barrier below
    uint32_t ctr[4] = {(uint32_t)step, (uint32_t)(step >> 32), 0u, 0u};
    mcmcd::philox4x32_10(ctr, (uint32_t)(D.chain_offset + c), D.seed);
    const int cell = (int)(((uint64_t)ctr[0] * (uint32_t)D.ncm) >> 32);
    const int mag = 1 + (int)(((uint64_t)ctr[1] * (uint32_t)D.dvmax) >> 32);
    const int minus = (int)(ctr[2] & 1u);
    const int R = block_radius(ctr[2], B.rmin, B.rmax);
    const int ph = cell >= D.ncell ? 1 : 0;
    const int cc = cell - ph * D.ncell;
    const int cx = cc % B.ncx, cy = (cc / B.ncx) % B.ncy, cz = cc / (B.ncx * B.ncy);
    const int lo = ph ? D.vsmin : D.vmin, hi = ph ? D.vsmax : D.vmax;
    const size_t row = (size_t)c * D.ncm + (size_t)ph * D.ncell;
    const int n3 = (2 * R + 1) * (2 * R + 1) * (2 * R + 1);
    bool ok = true;
    for (int k = lane; k < n3; k += 64) {
        int t = 0;
        const int dv = block_dv(B.ncx, B.ncy, B.ncz, cx, cy, cz, R, mag, k, &t);
        if (dv) {
            const int vn = D.v[row + t] + (minus ? -dv : dv);
            ok = ok && vn >= lo && vn <= hi;
        }
    }
    const bool inp = wave_all(ok);
    if (inp) {
        for (int k = lane; k < n3; k += 64) {
            int t = 0;
            const int dv = block_dv(B.ncx, B.ncy, B.ncz, cx, cy, cz, R, mag, k, &t);
            if (dv) D.slow_prop[row + t] = 1.0f / (float)(D.v[row + t] + (minus ? -dv : dv));
        }
    }
    if (lane == 0) {
        D.prop_cell[c] = cell;
        D.prop_phase[c] = ph;
        D.prop_v[c] = D.v[row + cc] + (minus ? -mag : mag);     // the centre moves by the whole magnitude
        D.prop_inprior[c] = inp ? 1 : 0;
        D.prop_logu[c] = mcmcd::det_log(((double)ctr[3] + 0.5) * (1.0 / 4294967296.0));
        B.prop_amp[c] = minus ? -mag : mag;
        B.prop_rad[c] = R;
    }
}

// accept_kernel's decision for chain (wave) c, every lane alike; lane 0 writes
// the chain's scalars, the wave commits (v, slow_cur) or reverts (slow_prop)
// the footprint and, with two models, copies the accepted phase's tables.
__global__ __launch_bounds__(BLOCK_THREADS) void block_accept_kernel(McmcDev D, BlockDev B, NuisDev N, int keep_slot)
{
    const int c = blockIdx.x * BLOCK_CHAINS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= D.nchains) return;
    const int inp = D.prop_inprior[c], ph = D.prop_phase[c];
    const int cell = D.prop_cell[c], amp = B.prop_amp[c], R = B.prop_rad[c];
    const double lold = D.logl[c];
    int acc = 0;
    double ln = 0.0;
    if (inp) {
        ln = nuis_logl(D, N, c, mcmcd::chain_loglik(nuis_chain(D, N, c), c, ph));
        const double d = ln - lold;
        acc = D.beta ? D.prop_logu[c] < D.beta[c] * d : D.prop_logu[c] < d;
        const int cc = cell - ph * D.ncell;
        const int cx = cc % B.ncx, cy = (cc / B.ncx) % B.ncy, cz = cc / (B.ncx * B.ncy);
        const int mag = amp < 0 ? -amp : amp;
        const size_t row = (size_t)c * D.ncm + (size_t)ph * D.ncell;
        const int n3 = (2 * R + 1) * (2 * R + 1) * (2 * R + 1);
        for (int k = lane; k < n3; k += 64) {
            int t = 0;
            const int dv = block_dv(B.ncx, B.ncy, B.ncz, cx, cy, cz, R, mag, k, &t);
            if (!dv) continue;
            if (acc) {
                D.v[row + t] = D.v[row + t] + (amp < 0 ? -dv : dv);
                D.slow_cur[row + t] = D.slow_prop[row + t];
            } else {
                D.slow_prop[row + t] = D.slow_cur[row + t];
            }
        }
        if (acc && D.ttab_cur) mcmcd::chain_copy_tables(D, c, ph, lane, 64);
    }
    if (lane == 0) {
        if (acc) {
            D.logl[c] = ln;
            D.naccept[c] = D.naccept[c] + 1;
            atomicAdd(&B.accepts[R], 1ull);
        }
        atomicAdd(&B.attempts[R], 1ull);
        D.accept[c] = (unsigned char)acc;
        if (keep_slot >= 0) D.keep_logl[(size_t)keep_slot * D.keep_stride + c] = acc ? ln : lold;
    }
}

}  // namespace

hipError_t block_propose(const McmcDev &D, const BlockDev &B, uint64_t step, hipStream_t st)
{
    hipLaunchKernelGGL(block_propose_kernel, dim3((D.nchains + BLOCK_CHAINS - 1) / BLOCK_CHAINS), dim3(BLOCK_THREADS),
                       0, st, D, B, step);
    return hipGetLastError();
}

hipError_t block_accept(const McmcDev &D, const BlockDev &B, const NuisDev &N, int keep_slot, hipStream_t st)
{
    hipLaunchKernelGGL(block_accept_kernel, dim3((D.nchains + BLOCK_CHAINS - 1) / BLOCK_CHAINS), dim3(BLOCK_THREADS),
                       0, st, D, B, N, keep_slot);
    if (keep_slot >= 0) return mcmc_keep(D, keep_slot, st);
    return hipGetLastError();
}
