// adjoint.hip -- the discrete adjoint of the fast-sweeping eikonal solve
// (include/mceik.h mceik_fsm_adjoint_*; DESIGN.md s.17 defines every
// operation, tests/_adjoint.py restates them).
//
// At the converged field every non-boundary node i satisfies
// sum_k (u_i - a_k)^2 = f_i^2 over its participating upwind neighbours a_k, so
// du_i/da_k = (u_i - a_k) / D_i and du_i/df_i = f_i / D_i with D_i = sum_k (u_i
// - a_k).  The adjoint field lam_j = q_j + sum_n lam_n (u_n - u_j) / D_n over
// the nodes n that take j as an upwind neighbour follows the strict order of u
// (a DAG), so the eight sweep orderings of the forward reach its unique fixed
// point; all arithmetic is fp64 on (double)u, IEEE + - * / (and the sqrt of
// the SETBCS distance), no contraction, no atomics.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "adjoint.h"
#include "fsm_batch.h"
#include "host_util.h"

namespace {

// A load through a vector-register address: the workspace changes during the
// kernel, and a wave-uniform address could otherwise become a scalar-cache
// load, which the vector stores do not invalidate.
template <typename T>
__device__ __forceinline__ T vld(const T *p)
{
    asm volatile("" : "+v"(p));
    return *p;
}

// EIKONAL_SOURCE_INDEX / EIKONAL_INIT_GRID of one axis (fsm_device.h
// init_field): the 0-based inclusive node range of the SETBCS box, false when
// a candidate node lies outside the grid (the forward's ierr = 1).
__device__ __forceinline__ bool adj_box_axis(int n, double x0, double dx, double xs, int &lo, int &hi)
{
    int is;
    if (xs <= x0) is = 1;
    else if (xs >= x0 + (double)(n - 1) * dx) is = n;
    else is = (int)((xs - x0) / dx + 0.5) + 1;
    const double xe = x0 + (double)(is - 1) * dx;
    int a, b;
    if (xe > xs) { a = is - 1; b = is; }
    else if (xe < xs) { a = is; b = is + 1; }
    else { a = is - 1; b = is < n - 1 ? is + 1 : is; }
    lo = a - 1; hi = b - 1;
    return a >= 1 && b <= n;
}

struct AdjBox {
    int lo[3], hi[3];
    __device__ __forceinline__ bool has(int x, int y, int z) const
    {
        return x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2];
    }
};

// Upwind choice, participation and D of node (x, y, z) of field u.
template <typename R>
__device__ __forceinline__ unsigned adj_node(const AdjLaunch &A, const R *u, int x, int y, int z, double &ui, double (&a)[3],
                                             double &D)
{
    const int nxy = A.nx * A.ny;
    const size_t i = (size_t)z * nxy + (size_t)y * A.nx + x;
    ui = (double)u[i];
    const double m[3] = {x > 0 ? (double)u[i - 1] : ui, y > 0 ? (double)u[i - A.nx] : ui, z > 0 ? (double)u[i - nxy] : ui};
    const double p[3] = {x < A.nx - 1 ? (double)u[i + 1] : ui, y < A.ny - 1 ? (double)u[i + A.nx] : ui,
                         z < A.nz - 1 ? (double)u[i + nxy] : ui};
    unsigned fl = 0;
    D = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const bool minus = m[k] < p[k];
        a[k] = minus ? m[k] : p[k];
        if (!minus) fl |= ADJ_SIDE(k);
        if (a[k] < ui) {
            fl |= ADJ_PART(k);
            D = D + (ui - a[k]);
        }
    }
    return fl;
}

// f of node (x, y, z): the forward's product in its precision, promoted.
template <typename R>
__device__ __forceinline__ double adj_f(const AdjLaunch &A, const void *slow_model, int x, int y, int z)
{
    if (A.slow_mode == 0) {
        const R s = reinterpret_cast<const R *>(slow_model)[((size_t)z * A.ny + y) * A.nx + x];
        return (double)(s * (R)A.h);
    }
    const float s = reinterpret_cast<const float *>(slow_model)[((size_t)(z / A.nrz) * A.ncy + y / A.nry) * A.ncx + x / A.nrx];
    return (double)((R)s * (R)A.h);
}

// One solve in the calling workgroup's slice.  Every loop is bounded and every
// barrier is reached by all threads (the bounds are workgroup-uniform).
template <typename R>
__device__ void adjoint_solve(const AdjLaunch &A, int solve, double *lam, double *q, double *w, unsigned char *flags)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int nx = A.nx, ny = A.ny, nz = A.nz, nxy = nx * ny, n = nxy * nz;
    const int ncell = A.ncx * A.ncy * A.ncz;
    const int m = solve / A.nstat, station = solve - m * A.nstat;
    const int ph = A.model_phase ? A.model_phase[m] : (A.nphase > 1 ? m % A.nphase : 0);
    double *gm = A.grad ? A.grad + (size_t)m * ncell : nullptr;
    double *gs = A.grad_solve ? A.grad_solve + (size_t)solve * ncell : nullptr;
    double *lo = A.lam ? A.lam + (size_t)solve * n : nullptr;

    const double *sp = A.src + (size_t)station * 4;
    AdjBox box;
    const int nn[3] = {nx, ny, nz};
    const double org[3] = {A.x0, A.y0, A.z0};
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = adj_box_axis(nn[k], org[k], A.h, sp[1 + k], box.lo[k], box.hi[k]) && ok;
    const bool skipped = A.skip && A.skip[ph * A.nstat + station];
    if (skipped || !ok) {
        // no field is read: zeros (the model's sum still takes the station's 0.0, in station order)
        for (int c = tid; c < ncell; c += nt) {
            if (gs) gs[c] = 0.0;
            if (A.by_model && gm) gm[c] = (station == 0 ? 0.0 : vld(gm + c)) + 0.0;
        }
        if (lo) for (int i = tid; i < n; i += nt) lo[i] = 0.0;
        if (tid == 0) {
            if (A.niter) A.niter[solve] = 0;
            if (A.status) A.status[solve] = skipped ? 0 : 2;
        }
        __syncthreads();
        return;
    }
    const R *u = reinterpret_cast<const R *>(A.u) + (size_t)solve * n;
    const size_t entry = A.slow_mode == 0 ? (size_t)m * n
                                          : (A.model_phase ? (size_t)m * A.nphase + A.model_phase[m] : (size_t)m) * ncell;
    const void *slow_model = A.slow_mode == 0 ? (const void *)(reinterpret_cast<const R *>(A.slow) + entry)
                                              : (const void *)(reinterpret_cast<const float *>(A.slow) + entry);

    // pre-pass: weights and flags of every node; q = 0
    for (int i = tid; i < n; i += nt) {
        const int z = i / nxy, r = i - z * nxy, y = r / nx, x = r - y * nx;
        double ui, a[3], D;
        unsigned fl = adj_node<R>(A, u, x, y, z, ui, a, D);
        if (box.has(x, y, z)) fl |= ADJ_BC;
#pragma unroll
        for (int k = 0; k < 3; k++) w[(size_t)k * n + i] = (fl & ADJ_PART(k)) ? (ui - a[k]) / D : 0.0;
        flags[i] = (unsigned char)fl;
        q[i] = 0.0;
    }
    __syncthreads();
    // adjoint source, events in order (one thread: a sequential sum per node)
    if (tid == 0) {
        const int row = A.ev_stride > 0 ? m * A.ev_stride : 0;
        for (int e = 0; e < A.nev; e++) {
            const int node = A.ev_node[row + e];
            if (node < 0 || node >= n) continue;
            const double we = A.ev_w[(size_t)solve * A.nev + e];
            if (!A.ev_frac) {
                q[node] = vld(q + node) + we;
                continue;
            }
            const int z = node / nxy, r = node - z * nxy, y = r / nx, x = r - y * nx;
            const int x1 = min(x + 1, nx - 1), y1 = min(y + 1, ny - 1), z1 = min(z + 1, nz - 1);
            const float *fr = A.ev_frac + 3 * (size_t)(row + e);
            const double wx = (double)fr[0], wy = (double)fr[1], wz = (double)fr[2];
            for (int k = 0; k < 8; k++) {
                const int c = ((k & 4) ? z1 : z) * nxy + ((k & 2) ? y1 : y) * nx + ((k & 1) ? x1 : x);
                const double wt = (((k & 1) ? wx : 1.0 - wx) * ((k & 2) ? wy : 1.0 - wy)) * ((k & 4) ? wz : 1.0 - wz);
                q[c] = vld(q + c) + we * wt;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) lam[i] = vld(q + i);
    __syncthreads();

    // the eight sweep orderings by hyperplane levels (a level's nodes never
    // neighbour each other), until one whole iteration changes no bit
    const int nlev = nx + ny + nz - 2;
    int it = 0, status = 1;
    while (it < A.cap) {
        it++;
        int changed = 0;
        for (int sw = 0; sw < 8; sw++) {
            const bool rx = sw & 1, ry = sw & 2, rz = sw & 4;
            for (int lev = 0; lev < nlev; lev++) {
                const int kz0 = max(0, lev - (nx - 1) - (ny - 1)), kz1 = min(nz - 1, lev);
                const int cnt = (kz1 - kz0 + 1) * ny;
                for (int id = tid; id < cnt; id += nt) {
                    const int kz = kz0 + id / ny, ky = id % ny, kx = lev - kz - ky;
                    if (kx < 0 || kx >= nx) continue;
                    const int x = rx ? nx - 1 - kx : kx, y = ry ? ny - 1 - ky : ky, z = rz ? nz - 1 - kz : kz;
                    const int j = z * nxy + y * nx + x;
                    double acc = vld(q + j);
                    // pull order x-, x+, y-, y+, z-, z+: neighbour nb counts when it is no boundary node,
                    // participates on the axis and chose the side j is on
                    const int pos[3] = {x, y, z}, lim[3] = {nx - 1, ny - 1, nz - 1}, str[3] = {1, nx, nxy};
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        if (pos[k] > 0) {
                            const int nb = j - str[k];
                            const unsigned fl = vld(flags + nb);
                            if ((fl & (ADJ_BC | ADJ_PART(k) | ADJ_SIDE(k))) == (ADJ_PART(k) | ADJ_SIDE(k)))
                                acc = acc + vld(lam + nb) * vld(w + (size_t)k * n + nb);
                        }
                        if (pos[k] < lim[k]) {
                            const int nb = j + str[k];
                            const unsigned fl = vld(flags + nb);
                            if ((fl & (ADJ_BC | ADJ_PART(k) | ADJ_SIDE(k))) == ADJ_PART(k))
                                acc = acc + vld(lam + nb) * vld(w + (size_t)k * n + nb);
                        }
                    }
                    if (__double_as_longlong(acc) != __double_as_longlong(vld(lam + j))) {
                        lam[j] = acc;
                        changed = 1;
                    }
                }
                __syncthreads();
            }
        }
        if (!__syncthreads_or(changed)) {
            status = 0;
            break;
        }
    }
    if (tid == 0) {
        if (A.niter) A.niter[solve] = it;
        if (A.status) A.status[solve] = status;
    }
    if (lo) for (int i = tid; i < n; i += nt) lo[i] = vld(lam + i);

    // node gradients summed per cell: x inside a row, rows over y, planes over z, each from 0.0
    for (int c = tid; c < ncell; c += nt) {
        const int cz = c / (A.ncx * A.ncy), r = c - cz * A.ncx * A.ncy, cy = r / A.ncx, cx = r - cy * A.ncx;
        double cell = 0.0;
        for (int z = cz * A.nrz; z < min(nz, (cz + 1) * A.nrz); z++) {
            double plane = 0.0;
            for (int y = cy * A.nry; y < min(ny, (cy + 1) * A.nry); y++) {
                double rowsum = 0.0;
                for (int x = cx * A.nrx; x < min(nx, (cx + 1) * A.nrx); x++) {
                    const int i = z * nxy + y * nx + x;
                    const double l = vld(lam + i);
                    double g = 0.0;
                    if (box.has(x, y, z)) {
                        const double xx = A.x0 + (double)x * A.h, yy = A.y0 + (double)y * A.h, zz = A.z0 + (double)z * A.h;
                        const double dx = sp[1] - xx, dy = sp[2] - yy, dz = sp[3] - zz;
                        g = l * __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
                    } else {
                        double ui, a[3], D;
                        adj_node<R>(A, u, x, y, z, ui, a, D);
                        if (D > 0.0) g = (l * (adj_f<R>(A, slow_model, x, y, z) / D)) * A.h;
                    }
                    rowsum = rowsum + g;
                }
                plane = plane + rowsum;
            }
            cell = cell + plane;
        }
        if (gs) gs[c] = cell;
        if (A.by_model && gm) gm[c] = (station == 0 ? 0.0 : vld(gm + c)) + cell;
    }
    __syncthreads();
}

template <typename R>
__global__ __launch_bounds__(ADJ_THREADS) void adjoint_kernel(AdjLaunch A)
{
    const size_t n = (size_t)A.nx * A.ny * A.nz;
    char *ws = A.ws + (size_t)blockIdx.x * A.ws_group;
    double *lam = reinterpret_cast<double *>(ws), *q = lam + n, *w = q + n;
    unsigned char *flags = reinterpret_cast<unsigned char *>(w + 3 * n);
    const int nitems = A.by_model ? A.nmodel : A.nsolve;
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int s0 = A.by_model ? item * A.nstat : item, s1 = A.by_model ? s0 + A.nstat : s0 + 1;
        for (int solve = s0; solve < s1; solve++) adjoint_solve<R>(A, solve, lam, q, w, flags);
    }
}

// grad[m][c] = 0.0 + the model's per-solve rows in station order.
__global__ void adjoint_station_sum(const double *gs, double *grad, int nmodel, int nstat, int ncell)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nmodel * ncell) return;
    const size_t m = i / ncell, c = i - m * ncell;
    double g = 0.0;
    for (int s = 0; s < nstat; s++) g = g + gs[(m * nstat + s) * ncell + c];
    grad[i] = g;
}

struct AdjPlan {
    AdjLaunch A;
    int groups;
    size_t total;
};

int adj_refuse(const char *why)
{
    fprintf(stderr, "mceik_fsm_adjoint: %s\n", why);
    return 1;
}

AdjPlan adj_plan(const mceik_fsm_adjoint *d)
{
    const mceik_fsm_batch *b = d->batch;
    FsmLaunch L;
    fill_launch(L, b);
    AdjPlan P;
    memset(&P, 0, sizeof(P));
    AdjLaunch &A = P.A;
    A.nx = b->nx; A.ny = b->ny; A.nz = b->nz;
    A.slow_mode = b->slow_mode;
    if (b->slow_mode == 1) {
        A.nrx = L.nrx; A.nry = L.nry; A.nrz = L.nrz;
        A.ncx = L.ncx; A.ncy = L.ncy; A.ncz = L.ncz;
    } else {                                             // field mode: every node is a cell of its own
        A.nrx = A.nry = A.nrz = 1;
        A.ncx = b->nx; A.ncy = b->ny; A.ncz = b->nz;
    }
    A.nmodel = b->nmodel; A.nstat = b->nstat; A.nsolve = b->nmodel * b->nstat;
    A.nphase = L.nphase;
    A.cap = d->maxit > 0 ? d->maxit : b->maxit;
    A.by_model = d->grad && !d->grad_solve;
    A.nev = b->nev; A.ev_stride = b->ev_stride;
    A.h = b->h; A.x0 = b->x0; A.y0 = b->y0; A.z0 = b->z0;
    A.src = b->src; A.slow = b->slow;
    A.model_phase = b->slow_mode == 1 ? b->model_phase : nullptr;
    A.skip = b->skip;
    A.ev_node = b->ev_node; A.ev_frac = b->ev_frac; A.ev_w = d->ev_w;
    A.u = d->u;
    A.grad = d->grad; A.grad_solve = d->grad_solve; A.lam = d->lam;
    A.niter = d->niter; A.status = d->status;
    const size_t n = (size_t)b->nx * b->ny * b->nz;
    A.ws_group = adj_group_bytes(n);
    const int nitems = A.by_model ? A.nmodel : A.nsolve;
    const int cap = d->max_groups > 0 ? d->max_groups : ADJ_DEFAULT_GROUPS;
    P.groups = nitems < cap ? nitems : cap;
    P.total = (size_t)P.groups * A.ws_group;
    return P;
}

}  // namespace

extern "C" int mceik_fsm_adjoint_check(const mceik_fsm_adjoint *d)
{
    if (!d || !d->batch) return adj_refuse("no description or no batch");
    const mceik_fsm_batch *b = d->batch;
    if (mceik_fsm_check(b)) return adj_refuse("the forward refuses this batch");
    if (b->nsrc != 1) return adj_refuse("one source per solve (nsrc = 1): with several the boundary boxes overlap");
    if (!d->u) return adj_refuse("u is NULL (the forward's fields, mceik_fsm_batch.u_out)");
    if (!b->src || !b->slow) return adj_refuse("the batch holds no sources or no slowness");
    if (b->slow_mode != 0 && b->slow_mode != 1) return adj_refuse("slow_mode must be 0 or 1");
    if (b->nev < 0 || (b->nev > 0 && (!b->ev_node || !d->ev_w))) return adj_refuse("events without ev_node or ev_w");
    if (b->ev_stride < 0 ||
        (b->ev_stride > 0 && (b->ev_stride < b->nev || (long long)b->nmodel * b->ev_stride > 0x7fffffffLL)))
        return adj_refuse("ev_stride must be 0 or >= nev, with nmodel * ev_stride below 2^31");
    if (d->maxit < 0 || d->max_groups < 0) return adj_refuse("maxit and max_groups must not be negative");
    return 0;
}

extern "C" size_t mceik_fsm_adjoint_workspace_bytes(const mceik_fsm_adjoint *d)
{
    if (!d || !d->batch || d->batch->nx < 1 || d->batch->ny < 1 || d->batch->nz < 1 || d->batch->nmodel < 1 ||
        d->batch->nstat < 1)
        return 0;
    return adj_plan(d).total;
}

extern "C" int mceik_fsm_adjoint_solve(const mceik_fsm_adjoint *d, void *workspace, size_t workspace_bytes, void *stream)
{
    if (mceik_fsm_adjoint_check(d)) return 1;
    AdjPlan P = adj_plan(d);
    if (!workspace || workspace_bytes < P.total) {
        fprintf(stderr, "mceik_fsm_adjoint: workspace too small (%zu < %zu)\n", workspace_bytes, P.total);
        return 1;
    }
    P.A.ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (d->batch->precision == 64)
        hipLaunchKernelGGL(adjoint_kernel<double>, dim3(P.groups), dim3(ADJ_THREADS), 0, st, P.A);
    else
        hipLaunchKernelGGL(adjoint_kernel<float>, dim3(P.groups), dim3(ADJ_THREADS), 0, st, P.A);
    HIPCHK(hipGetLastError());
    if (d->grad && d->grad_solve) {
        const int ncell = P.A.ncx * P.A.ncy * P.A.ncz;
        const size_t tot = (size_t)P.A.nmodel * ncell;
        hipLaunchKernelGGL(adjoint_station_sum, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, d->grad_solve,
                           d->grad, P.A.nmodel, P.A.nstat, ncell);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
