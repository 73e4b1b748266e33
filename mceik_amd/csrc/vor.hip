// vor.hip -- transdimensional Voronoi-cell models of the sampler
// (include/mceik.h mceik_mcmc_vor_*), on gfx950.
//
// The kernels of a Voronoi step around the ordinary step batch's forward: the
// draw (one wave per chain: the list tests are ballots over the nuclei), the
// raster of the proposed nuclei (grid over cell tiles x chains; the nuclei
// staged in LDS and read by every lane at once, lanes along cells), the accept
// (one workgroup per chain) and the moments of kept states.  Per-chain state
// that an earlier kernel of the step wrote is read through mcmcd::ldv.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_common.h"
#include "mcmc_device.h"
#include "mcmc_host.h"
#include "nuis.h"
#include "vor.h"

#define VOR_DRAW_CHAINS (VOR_THREADS / 64)

namespace {

using mcmcd::ldv;

// #{j < k: cells[j] <= x} over the wave (every lane gets the count).
__device__ __forceinline__ int wave_count_le(const int *cells, int k, int x, int lane)
{
    int n = 0;
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + lane;
        const bool p = j < k && ldv(&cells[j]) <= x;
        n += __popcll(__ballot(p));
    }
    return n;
}

// One wave per chain: the draw, the move's validity, the proposed nuclei of
// phase ph into pcell / pval / pk, the record.
__global__ __launch_bounds__(VOR_THREADS) void vor_draw_kernel(McmcDev D, VorDev L, uint64_t gs, int ph)
{
    const int c = blockIdx.x * VOR_DRAW_CHAINS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= D.nchains) return;                         // whole waves leave: no barrier below
    const size_t row = ((size_t)c * D.nphase + ph) * L.kmax;
    const int *cells = L.cell + row, *vals = L.val + row;
    const int k = ldv(&L.cnt_k[(size_t)c * D.nphase + ph]);
    const int vlo = ph ? D.vsmin : D.vmin, vhi = ph ? D.vsmax : D.vmax;
    const VorDraw d = vor_draw(D.seed, (uint32_t)(D.chain_offset + c), gs, k, D.ncell, L.dv, vlo, vhi, L.dmx, L.dmy, L.dmz);
    const bool birth = d.type == VOR_BIRTH;
    const int cj = birth ? 0 : ldv(&cells[d.j]), wj = birth ? 0 : ldv(&vals[d.j]);
    int tc, tv;
    int reason = vor_target(d, k, L.kmin, L.kmax, cj, wj, vlo, vhi, L.ncx, L.ncy, L.ncz, &tc, &tv);
    if (!reason && d.type == VOR_MOVE) {                // the target cell must be free
        bool occ = false;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            occ = occ || (j < k && ldv(&cells[j]) == tc);
        }
        if (__ballot(occ) != 0ull) reason = 3;
    }
    if (!reason && birth) {                             // the f-th free cell: x = f + #{cells <= x} from x = f
        int x = d.f;
        for (;;) {
            const int y = d.f + wave_count_le(cells, k, x, lane);
            if (y == x) break;
            x = y;
        }
        tc = x;
    }
    const bool ok = reason == 0;
    int kp = k;
    if (ok && birth) kp = k + 1;
    if (ok && d.type == VOR_DEATH) kp = k - 1;
    int *pc = L.pcell + (size_t)c * L.kmax, *pv = L.pval + (size_t)c * L.kmax;
    for (int j = lane; j < kp; j += 64) {
        int cc, vv;
        if (ok && birth && j == k) { cc = tc; vv = tv; }
        else if (ok && d.type == VOR_DEATH && j == d.j) { cc = ldv(&cells[k - 1]); vv = ldv(&vals[k - 1]); }
        else if (ok && d.type <= VOR_MOVE && j == d.j) { cc = tc; vv = tv; }
        else { cc = ldv(&cells[j]); vv = ldv(&vals[j]); }
        pc[j] = cc;
        pv[j] = vv;
    }
    if (lane == 0) {
        L.pk[c] = kp;
        int *r = L.rec + (size_t)c * VOR_NREC;
        r[0] = d.type; r[1] = reason;
        r[2] = birth ? (ok ? k : -1) : d.j;
        r[3] = tc; r[4] = tv; r[5] = kp; r[6] = 0; r[7] = 0;
        D.prop_phase[c] = ph;
        D.prop_cell[c] = ph * D.ncell;
        D.prop_v[c] = ldv(&D.v[(size_t)c * D.ncm + (size_t)ph * D.ncell]);
        D.prop_inprior[c] = ok ? 1 : 0;
        D.prop_logu[c] = mcmcd::det_log(((double)d.u + 0.5) * (1.0 / 4294967296.0));
    }
}

// grid (cell tiles, rows).  The row's nuclei go to LDS once as (mx x, my y, mz
// z, cell); every lane then reads the same nucleus at a time (a broadcast: no
// bank conflicts) and keeps the nearest by (d2, cell).  A thread takes four
// cells VOR_THREADS apart, so the stores of v and 1/v are coalesced runs.
__global__ __launch_bounds__(VOR_THREADS) void vor_raster_kernel(VorDev L, int ncell, const int *cell, const int *val,
                                                                 const int *cnt, int *vout, size_t vstride, float *s1,
                                                                 float *s2, size_t sstride, int row0)
{
    __shared__ int4 sn[MCEIK_VOR_KMAX];
    __shared__ int sw[MCEIK_VOR_KMAX];
    const int r = row0 + blockIdx.y, tid = threadIdx.x;
    const int k = ldv(&cnt[r]);
    const int *cells = cell + (size_t)r * L.kmax, *vals = val + (size_t)r * L.kmax;
    const int nxy = L.ncx * L.ncy;
    for (int j = tid; j < k; j += VOR_THREADS) {
        const int cj = ldv(&cells[j]);
        sn[j] = make_int4(L.mx * (cj % L.ncx), L.my * ((cj / L.ncx) % L.ncy), L.mz * (cj / nxy), cj);
        sw[j] = ldv(&vals[j]);
    }
    __syncthreads();
    const int c0 = blockIdx.x * VOR_TILE + tid;
    int X[4], Y[4], Z[4], bd[4], bc[4], bj[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int cc = min(c0 + i * VOR_THREADS, ncell - 1);     // (a lane past the row computes a cell it does not store)
        X[i] = L.mx * (cc % L.ncx); Y[i] = L.my * ((cc / L.ncx) % L.ncy); Z[i] = L.mz * (cc / nxy);
        bd[i] = 0x7fffffff; bc[i] = 0x7fffffff; bj[i] = 0;
    }
    for (int j = 0; j < k; j++) {
        const int4 n = sn[j];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ex = n.x - X[i], ey = n.y - Y[i], ez = n.z - Z[i];
            const int d = ex * ex + ey * ey + ez * ez;
            const bool better = d < bd[i] || (d == bd[i] && n.w < bc[i]);
            bd[i] = better ? d : bd[i];
            bc[i] = better ? n.w : bc[i];
            bj[i] = better ? j : bj[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int cc = c0 + i * VOR_THREADS;
        if (cc < ncell) {
            const int w = sw[bj[i]];
            const float sl = 1.0f / (float)w;
            vout[(size_t)r * vstride + cc] = w;
            s1[(size_t)r * sstride + cc] = sl;
            if (s2) s2[(size_t)r * sstride + cc] = sl;
        }
    }
}

// One workgroup per chain.  Thread 0 decides: accept iff the move was valid and
// log u < beta (logL' - logL), logL' from the step's tables (nuisance state
// honoured).  The workgroup commits (nuclei, v, slow_cur, the phase's current
// tables) or reverts (slow_prop).
__global__ __launch_bounds__(VOR_THREADS) void vor_accept_kernel(McmcDev D, VorDev L, NuisDev N, int ph, int keep_slot)
{
    __shared__ int s_acc;
    const int c = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        const int *r = L.rec + (size_t)c * VOR_NREC;
        const int type = ldv(&r[0]), reason = ldv(&r[1]);
        const double lold = ldv(&D.logl[c]);
        double ln = lold;
        int acc = 0;
        if (!reason) {
            ln = nuis_logl(D, N, c, mcmcd::chain_loglik(nuis_chain(D, N, c), c, ph));
            const double d = ln - lold;
            const double logu = ldv(&D.prop_logu[c]);
            acc = D.beta ? logu < ldv(&D.beta[c]) * d : logu < d;
        }
        s_acc = acc;
        L.logl_prop[c] = ln;
        unsigned long long *cnt = L.cnt + ((size_t)c * 4 + type) * VOR_NCNT;
        cnt[0] = ldv(&cnt[0]) + 1;
        if (acc) {
            cnt[1] = ldv(&cnt[1]) + 1;
            D.logl[c] = ln;
            D.naccept[c] = ldv(&D.naccept[c]) + 1;
        }
        if (reason) cnt[1 + reason] = ldv(&cnt[1 + reason]) + 1;
        D.accept[c] = (unsigned char)acc;
        if (keep_slot >= 0) D.keep_logl[(size_t)keep_slot * D.keep_stride + c] = acc ? ln : lold;
    }
    __syncthreads();
    const int acc = s_acc;
    const size_t row = (size_t)c * D.ncm + (size_t)ph * D.ncell;
    for (int i = tid; i < D.ncell; i += VOR_THREADS) {
        if (acc) {
            D.v[row + i] = ldv(&L.vprop[(size_t)c * D.ncell + i]);
            D.slow_cur[row + i] = ldv(&D.slow_prop[row + i]);
        } else {
            D.slow_prop[row + i] = ldv(&D.slow_cur[row + i]);
        }
    }
    if (acc) {
        const size_t nrow = ((size_t)c * D.nphase + ph) * L.kmax;
        const int kp = ldv(&L.pk[c]);
        for (int j = tid; j < kp; j += VOR_THREADS) {
            L.cell[nrow + j] = ldv(&L.pcell[(size_t)c * L.kmax + j]);
            L.val[nrow + j] = ldv(&L.pval[(size_t)c * L.kmax + j]);
        }
        if (tid == 0) L.cnt_k[(size_t)c * D.nphase + ph] = kp;
        if (D.ttab_cur) mcmcd::chain_copy_tables(D, c, ph, tid, VOR_THREADS);
    }
}

// grid (chains, phases): one more kept state in the histogram of k and in the
// density of every cell that holds a nucleus (integer atomics: exact sums).
__global__ __launch_bounds__(VOR_THREADS) void vor_moments_kernel(McmcDev D, VorDev L)
{
    const int c = blockIdx.x, ph = blockIdx.y, tid = threadIdx.x;
    const size_t r = (size_t)c * D.nphase + ph;
    const int k = ldv(&L.cnt_k[r]);
    for (int j = tid; j < k; j += VOR_THREADS)
        atomicAdd(&L.dens[(size_t)ph * D.ncell + ldv(&L.cell[r * L.kmax + j])], 1ull);
    if (tid == 0) atomicAdd(&L.hist[(size_t)ph * (L.kmax + 1) + k], 1ull);
}

}  // namespace

hipError_t vor_raster(const VorDev &L, int ncell, int nrows, const int *cell, const int *val, const int *cnt, int *vout,
                      size_t vstride, float *s1, float *s2, size_t sstride, hipStream_t st)
{
    const int nt = (ncell + VOR_TILE - 1) / VOR_TILE, ymax = 65535;
    for (int r0 = 0; r0 < nrows; r0 += ymax) {
        const int n = nrows - r0 < ymax ? nrows - r0 : ymax;
        hipLaunchKernelGGL(vor_raster_kernel, dim3(nt, n), dim3(VOR_THREADS), 0, st, L, ncell, cell, val, cnt, vout,
                           vstride, s1, s2, sstride, r0);
    }
    return hipGetLastError();
}

hipError_t vor_propose(const McmcDev &D, const VorDev &L, uint64_t gs, int ph, hipStream_t st)
{
    hipLaunchKernelGGL(vor_draw_kernel, dim3((D.nchains + VOR_DRAW_CHAINS - 1) / VOR_DRAW_CHAINS), dim3(VOR_THREADS), 0,
                       st, D, L, gs, ph);
    // row c: the chain's proposed nuclei -> vprop row c and the stepped phase's row of slow_prop
    return vor_raster(L, D.ncell, D.nchains, L.pcell, L.pval, L.pk, L.vprop, (size_t)D.ncell,
                      D.slow_prop + (size_t)ph * D.ncell, nullptr, (size_t)D.ncm, st);
}

hipError_t vor_accept(const McmcDev &D, const VorDev &L, const NuisDev &N, int ph, int keep_slot, hipStream_t st)
{
    hipLaunchKernelGGL(vor_accept_kernel, dim3(D.nchains), dim3(VOR_THREADS), 0, st, D, L, N, ph, keep_slot);
    if (keep_slot >= 0) return mcmc_keep(D, keep_slot, st);
    return hipGetLastError();
}

hipError_t vor_moments(const McmcDev &D, const VorDev &L, int ncold, hipStream_t st)
{
    if (ncold <= 0) return hipSuccess;
    hipLaunchKernelGGL(vor_moments_kernel, dim3(ncold, D.nphase), dim3(VOR_THREADS), 0, st, D, L);
    return hipGetLastError();
}
