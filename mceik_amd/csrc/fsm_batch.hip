// fsm_batch.hip -- the batched FSM solve of the C-ABI (include/mceik.h
// mceik_fsm_*, include/mceik_eikonal.h eikonal3d_batch_solve).
//
// Host orchestration only: argument checks, launch sizing, the workspace
// layout and kernel enqueueing.  The numerics live in fsm_kernel.hip and
// fsm16_kernel.hip.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fsm_batch.h"
#include "fsm_host.h"
#include "host_util.h"

// ---------------------------------------------------------------------------
// Convergence threshold T: the smallest power of two with
// spacing(T^-) = T * 2^-p >= tol, p = 24 (fp32) or 53 (fp64).  A node whose
// value was >= T when it changed has moved by >= tol, so only nodes below T
// need their start-of-iteration value kept for the |u0 - u| < tol test.
static double conv_threshold(double tol, int is_double)
{
    double tolr = is_double ? tol : (double)(float)tol;
    if (!(tolr > 0.0)) return HUGE_VAL;
    int p = is_double ? 53 : 24;
    int k = (int)ceil(log2(tolr)) + p;
    while (ldexp(1.0, k - p) < tolr) k++;
    while (ldexp(1.0, k - 1 - p) >= tolr) k--;
    double T = ldexp(1.0, k);
    double big = is_double ? DBL_MAX : (double)FLT_MAX;
    return T > big ? HUGE_VAL : T;
}

void fill_launch(FsmLaunch &L, const mceik_fsm_batch *b)
{
    memset(&L, 0, sizeof(L));
    L.nx = b->nx; L.ny = b->ny; L.nz = b->nz;
    fsm_geometry(&L, b->precision == 64 ? 8 : 4);
    L.maxit = b->maxit; L.max_sweeps = b->max_sweeps;
    L.tol = b->tol; L.h = b->h; L.x0 = b->x0; L.y0 = b->y0; L.z0 = b->z0;
    int is_double = b->precision == 64;
    double T = conv_threshold(b->tol, is_double);
    L.conv_thresh = is_double ? (T == HUGE_VAL ? DBL_MAX : T) : (T == HUGE_VAL ? (double)FLT_MAX : T);
    L.nsolve = b->nmodel * b->nstat; L.nstat = b->nstat; L.nsrc = b->nsrc;
    L.src = b->src;
    L.slow_mode = b->slow_mode;
    L.nrx = b->nrx > 0 ? b->nrx : 1; L.nry = b->nry > 0 ? b->nry : 1; L.nrz = b->nrz > 0 ? b->nrz : 1;
    L.ncx = mceik_div_up(L.nx, L.nrx); L.ncy = mceik_div_up(L.ny, L.nry); L.ncz = mceik_div_up(L.nz, L.nrz);
    L.magic_rx = ((1u << 20) + L.nrx - 1) / L.nrx;
    L.magic_ry = ((1u << 20) + L.nry - 1) / L.nry;
    L.magic_rz = ((1u << 20) + L.nrz - 1) / L.nrz;
    L.ev_node = b->ev_node; L.nev = b->nev; L.ttab = b->ttab; L.ev_frac = b->ev_frac;
    L.ev_stride = b->ev_stride;
    L.model_phase = b->slow_mode == 1 ? b->model_phase : nullptr;
    L.skip = b->skip;
    L.solve_count = b->solve_count;
    L.nphase = b->nphase > 0 ? b->nphase : 1;
    // LDS cell cache when every z-block's cells fit: ccb = the most cells a z-block of a tile touches
    // (2 x 2 x 8 at nref = 4, kb = 4; 4 x 4 x 11 at nref = 3; 8 x 8 x 32 at nref = 1, which does not
    // fit and runs uncached).  Sized here with true divisions, indexed by the kernels with the magic
    // multiply: mceik_fsm_check refuses the refinements at which the two differ (nr >= 275)
    {
        auto span = [](int a, int e, int nr) { return e / nr - a / nr + 1; };
        int mx = 0, my = 0, mz = 0;
        for (int t = 0; t < L.ntx; t++) {
            int v = span(t * 8, t * 8 + 7 < L.nx - 1 ? t * 8 + 7 : L.nx - 1, L.nrx); mx = v > mx ? v : mx;
        }
        for (int t = 0; t < L.nty; t++) {
            int v = span(t * 8, t * 8 + 7 < L.ny - 1 ? t * 8 + 7 : L.ny - 1, L.nry); my = v > my ? v : my;
        }
        for (int t = 0; t < L.nzk; t++) {
            int a = t * L.kb * 8, e = a + L.kb * 8 - 1 < L.nz - 1 ? a + L.kb * 8 - 1 : L.nz - 1;
            int v = span(a, e, L.nrz); mz = v > mz ? v : mz;
        }
        L.ccb = mx * my * mz;
        L.cell_cache = b->slow_mode == 1 && L.ccb <= MCEIK_CC_MAX && L.nx < 4096 && L.ny < 4096 && L.nz < 4096;
        if (!L.cell_cache) L.ccb = 0;
    }
    L.fast_sqrt = b->fast_sqrt;
    L.niter = b->niter; L.ierr = b->ierr;
    L.iter_total = b->iter_total;
    L.visit_stats = b->visit_stats;
    L.solve_order = b->solve_order;
    L.solve_clock = b->solve_clock;
    L.max_waves = b->max_waves;
    L.traffic = b->traffic;
    L.step_z = b->step_z;
    // (fsm16's first-touch instance: one line of u_nan behind every field slot)
    L.u_stride = L.field_elems +
                 (fsm_launch_kind(L, is_double) == 16 && fsm16_fixed_layout(L) ? FSM16_UNAN_LINE / 4 : 0);
}

static int g_device_cus = 0;

int device_cus()
{
    if (g_device_cus == 0) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess)
            g_device_cus = p.multiProcessorCount;
        else
            g_device_cus = 256;
    }
    return g_device_cus;
}

// Scratch budget for the per-wave u / u0 fields, fixed at the first call (so
// workspace_bytes and batch_solve agree): MCEIK_FSM_WS_GB if set, else the
// device memory free at that moment less an 8-GiB margin (the sampler's other
// arrays, the caller's tensors), at most 80% of the total (230 GB on a 288-GB
// MI355X).  A sampler with several pipes splits it between them (pipes_setup).
static size_t ws_budget_bytes()
{
    static size_t budget = 0;
    if (budget == 0) {
        const char *e = getenv("MCEIK_FSM_WS_GB");
        double gb = e ? atof(e) : 0.0;
        if (gb > 0.0) {
            budget = (size_t)(gb * 1073741824.0);
        } else {
            size_t fr = 0, tot = 0;
            const size_t margin = (size_t)8 << 30;
            if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot) {
                // at 256^3 (128 MiB of u + u0 per wave): 6.7 waves/CU
                budget = tot / 5 * 4;
                const size_t avail = fr > 2 * margin ? fr - margin : fr / 2;
                if (avail < budget) budget = avail;
            } else {
                budget = (size_t)96 << 30;
            }
        }
    }
    return budget;
}

// Waves a launch keeps resident (one solve each): occupancy x CUs, at most nsolve.
static int batch_waves(const FsmLaunch &L, int is_double)
{
    int per_cu = fsm_occupancy(L, is_double);
    if (per_cu < 1) per_cu = 1;
    // tuning knob: fewer resident waves per CU (L2 working set experiments)
    static const int env_cap = [] { const char *e = getenv("MCEIK_WAVES_PER_CU"); return e ? atoi(e) : 0; }();
    if (env_cap > 0 && env_cap < per_cu) per_cu = env_cap;
    long w = (long)per_cu * device_cus();
    if (L.max_waves > 0 && w > L.max_waves) w = L.max_waves;
    if (w > L.nsolve) w = L.nsolve;
    static const bool report = getenv("MCEIK_LAUNCH_REPORT") != nullptr;
    if (report)
        fprintf(stderr, "mceik fsm launch: %d-z steps, %d waves/CU (occupancy), %ld resident waves, %zu B LDS per wave\n",
                fsm_launch_kind(L, is_double), per_cu, w, fsm_launch_lds_bytes(L, is_double));
    return (int)(w < 1 ? 1 : w);
}

int fsm_batch_waves_uncapped(const mceik_fsm_batch *b)
{
    FsmLaunch L;
    fill_launch(L, b);
    return batch_waves(L, b->precision == 64);
}

WsLayout ws_layout(const mceik_fsm_batch *b)
{
    FsmLaunch L;
    fill_launch(L, b);
    int is_double = b->precision == 64;
    size_t es = is_double ? 8 : 4;
    WsLayout w;
    w.nwaves = batch_waves(L, is_double);
    // the held stream's per-wave z-face copies: read only by the 16-z kernel (the 8-z / fp64
    // instances read the z-boundary nodes from the field)
    const size_t zfw = fsm_launch_kind(L, is_double) == 16 ? zf_bytes(L, es) : 0;
    // Every resident wave owns a u and a u0 scratch field: cap the waves so the
    // scratch stays within a fixed budget (deterministic across calls; 256^3
    // fp32 fields are 67 MB, 2048 waves would need 275 GB).  Waves then take
    // several solves each from the queue.
    {
        const size_t per_wave = (L.u_stride + L.field_elems) * es + zfw;
        const long cap = (long)(ws_budget_bytes() / (per_wave ? per_wave : 1));
        if (cap >= 1 && w.nwaves > cap) w.nwaves = (int)cap;
    }
    w.counter = 0;
    w.slow = 1024;
    size_t slow_bytes = b->slow_mode == 0 ? (size_t)b->nmodel * L.field_elems * es : 0;
    w.u = w.slow + ((slow_bytes + 255) & ~(size_t)255);
    size_t nu = b->u_out ? (size_t)L.nsolve : (size_t)w.nwaves;
    w.u0 = w.u + nu * L.u_stride * es;
    w.zf = w.u0 + (size_t)w.nwaves * L.field_elems * es;          // the held stream's z-face copies
    w.total = w.zf + (size_t)w.nwaves * zfw;
    return w;
}

extern "C" size_t mceik_fsm_workspace_bytes(const mceik_fsm_batch *b)
{
    return ws_layout(b).total;
}

extern "C" int mceik_fsm_step_z(const mceik_fsm_batch *b)
{
    if (!b) return 0;
    FsmLaunch L;
    fill_launch(L, b);
    return fsm_launch_kind(L, b->precision == 64);
}

extern "C" const char *mceik_fsm_kernel_name(const mceik_fsm_batch *b)
{
    if (!b) return "";
    FsmLaunch L;
    fill_launch(L, b);
    return fsm_launch_name(L, b->precision == 64);
}

extern "C" size_t mceik_fsm_lds_bytes(const mceik_fsm_batch *b)
{
    if (!b) return 0;
    FsmLaunch L;
    fill_launch(L, b);
    return fsm_launch_lds_bytes(L, b->precision == 64);
}

extern "C" double mceik_fsm_bytes_per_node_sweep(const mceik_fsm_batch *b)
{
    // u read + u write per node visit; slowness read once per node per model
    // pass, shared by the nstat stations of that model (SURVEY s.8d: N(8+4/S)).
    double es = b->precision == 64 ? 8.0 : 4.0;
    double s = b->slow_mode == 0 ? es : 4.0 / ((double)b->nrx * b->nry * b->nrz);
    return 2.0 * es + s / (b->nstat > 0 ? b->nstat : 1);
}

extern "C" int mceik_fsm_batch_solve(const mceik_fsm_batch *b, void *workspace, size_t workspace_bytes,
                                     void *stream)
{
    return fsm_batch_solve_impl(b, workspace, workspace_bytes, stream, nullptr);
}

// The kernels' node -> cell map, (node * ceil(2^20 / nr)) >> 20 in unsigned
// 32-bit arithmetic (FsmLaunch.magic_r*), against node / nr for every node of
// an axis of n <= 4096 nodes (the product stays below 2^32).  With
// m = ceil(2^20 / nr), e = m nr - 2^20 and node = q nr + r the product is
// q 2^20 + (q e + r m), so the map is exact iff q e + r m < 2^20; the term
// grows with q and with r, so the axis' last node and the last node of its
// last whole cell decide.  (Exact for every n <= 4096 up to nr = 274; the
// first miss is nr = 275 at node 3849.)
static bool cell_map_exact(int n, int nr)
{
    const uint64_t m = ((1u << 20) + (uint64_t)nr - 1) / nr, e = m * nr - (1u << 20);
    const int last = n - 1, whole = n / nr * nr - 1;
    for (int node : {last, whole}) {
        if (node < 0) continue;
        if ((uint64_t)(node / nr) * e + (uint64_t)(node % nr) * m >= 1u << 20) return false;
    }
    return true;
}

// Everything mceik_fsm_batch_solve refuses before it looks at the workspace
// (host only: no GPU call).
extern "C" int mceik_fsm_check(const mceik_fsm_batch *b)
{
    if (!b || b->nx < 2 || b->ny < 2 || b->nz < 2 || b->nx > 4096 || b->ny > 4096 || b->nz > 4096 ||
        b->nsrc < 1 ||
        b->nmodel < 1 || b->nstat < 1 || !(b->precision == 32 || b->precision == 64)) {
        fprintf(stderr, "mceik_fsm_batch_solve: invalid batch description\n");
        return 1;
    }
    FsmLaunch G;
    fill_launch(G, b);
    if (b->slow_mode == 1) {
        const int n[3] = {G.nx, G.ny, G.nz}, nr[3] = {G.nrx, G.nry, G.nrz};
        for (int a = 0; a < 3; a++)
            if (!cell_map_exact(n[a], nr[a])) {
                fprintf(stderr, "mceik_fsm_batch_solve: refinement %d on the %c axis of %d nodes: the sweep kernels' "
                                "20-bit node -> cell multiply is not exact there\n", nr[a], "xyz"[a], n[a]);
                return 1;
            }
    }
    if (G.field_elems * (b->precision == 64 ? 8 : 4) >= (size_t)1 << 31) {
        fprintf(stderr, "mceik_fsm_batch_solve: one travel-time field must stay below 2 GiB\n");
        return 1;
    }
    if (fsm_launch_lds_bytes(G, b->precision == 64) > MCEIK_MAX_LDS) {
        fprintf(stderr, "mceik_fsm_batch_solve: %d x %d x %d z-blocks exceed the LDS block tables\n", G.ntx, G.nty,
                G.nzk);
        return 1;
    }
    // the held stream's 16-bit sweep clocks (fsm_hold.h hold_clock_bound)
    const bool held = fsm_launch_kind(G, b->precision == 64) == 16 || fsm_compact_layout(G, 8);
    const int infl = fsm_launch_kind(G, b->precision == 64) == 16 ? fsm16_geo(G).infl : G.infl;
    if (held && hold_clock_bound(G.nblocks, infl) >= 65536) {
        fprintf(stderr, "mceik_fsm_batch_solve: %d z-blocks overflow the held stream's 16-bit clocks\n", G.nblocks);
        return 1;
    }
    return 0;
}

int fsm_batch_solve_impl(const mceik_fsm_batch *b, void *workspace, size_t workspace_bytes, void *stream,
                         const McmcExt *ext)
{
    if (mceik_fsm_check(b)) return 1;
    WsLayout w = ws_layout(b);
    if (!workspace || workspace_bytes < w.total) {
        fprintf(stderr, "mceik_fsm_batch_solve: workspace too small (%zu < %zu)\n", workspace_bytes, w.total);
        return 1;
    }
    if (b->skip && b->u_out) {
        // a skipped solve never sweeps, so its u slot would hold stale workspace
        fprintf(stderr, "mceik_fsm_batch_solve: skip and u_out cannot be combined (a skipped solve has no field)\n");
        return 1;
    }
    // per-model event lists: rows of at least nev entries, indexed in int
    if (b->ev_stride < 0 || (b->ev_stride > 0 && (b->ev_stride < b->nev ||
                                                  (long long)b->nmodel * b->ev_stride > 0x7fffffffLL))) {
        fprintf(stderr, "mceik_fsm_batch_solve: ev_stride must be 0 or >= nev, with nmodel * ev_stride below 2^31\n");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    int is_double = b->precision == 64;
    FsmLaunch L;
    fill_launch(L, b);
    char *ws = (char *)workspace;
    L.counter = (unsigned *)(ws + w.counter);
    HIPCHK(fsm_zero_words(L.counter, 256, st));          // 8 queue heads, 128 B apart (graph-safe)
    if (b->slow_mode == 0) {
        void *sb = ws + w.slow;
        if (is_double)
            HIPCHK(fsm_to_brick_f64((const double *)b->slow, sb, 1, L, b->nmodel, st));
        else
            HIPCHK(fsm_to_brick_f32((const float *)b->slow, (float *)sb, L, b->nmodel, st));
        L.slow = sb;
    } else {
        L.slow = b->slow;
    }
    L.u = ws + w.u;
    L.u0 = ws + w.u0;
    L.zf = ws + w.zf;
    L.slot_per_solve = b->u_out ? 1 : 0;
    if (ext) {
        if (is_double || fsm_launch_kind(L, 0) != 16 || b->solve_order || b->u_out) return 1;
        L.mc_dev = ext->dev;
        L.mc_sync = ext->sync;
        L.mc_spin_limit = ext->spin_limit;
        L.mc_step0 = ext->step0; L.mc_nsteps = ext->nsteps;
        L.mc_nburn = ext->nburn; L.mc_keepk = ext->keepk; L.mc_maxs = ext->maxs; L.mc_nkept0 = ext->nkept0;
        // the broken-queue flag (last word) persists until the sampler reports it
        HIPCHK(fsm_zero_words(ext->sync, MC_SYNC_WORDS(L.nsolve / L.nstat) - 1, st));
    }
    HIPCHK(fsm_launch(L, is_double, w.nwaves, st));
    if (b->u_out) {
        if (is_double) HIPCHK(fsm_from_brick_f64(L.u, 1, (double *)b->u_out, L, L.nsolve, st));
        else HIPCHK(fsm_from_brick_f32((const float *)L.u, (float *)b->u_out, L, L.nsolve, st));
    }
    return 0;
}

// The plain-argument batched extension SURVEY s.8b names: nmodels x
// nstations single-source solves (fp32, the sampler's arithmetic) of
// per-node slowness fields in one call.  Pointers may be host or device
// memory (host arrays are staged); synchronous.  Solve m*nstations + s
// uses model m and station s.
static bool is_device_ptr(const void *p)
{
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

extern "C" int eikonal3d_batch_solve(int nmodels, int nstations, int nx, int ny, int nz, double h, double x0,
                                     double y0, double z0, int maxit, double tol, const double *src,
                                     const float *slow, float *u, int *niter, int *ierr)
{
    if (nmodels < 1 || nstations < 1 || !src || !slow || !u) return 1;
    const size_t n = (size_t)nx * ny * nz, nsolve = (size_t)nmodels * nstations;
    mceik_fsm_batch b;
    memset(&b, 0, sizeof(b));
    b.nx = nx; b.ny = ny; b.nz = nz; b.h = h; b.x0 = x0; b.y0 = y0; b.z0 = z0;
    b.maxit = maxit; b.tol = tol; b.precision = 32;
    b.nmodel = nmodels; b.nstat = nstations; b.nsrc = 1; b.slow_mode = 0; b.max_sweeps = -1;
    std::vector<void *> tmp;
    auto stage = [&](const void *p, size_t bytes, bool in) -> void * {
        if (is_device_ptr(p)) return const_cast<void *>(p);
        void *d = nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
        tmp.push_back(d);
        if (in && hipMemcpy(d, p, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    };
    int rc = 0;
    void *d_src = stage(src, (size_t)nstations * 4 * sizeof(double), true);
    void *d_slow = stage(slow, (size_t)nmodels * n * sizeof(float), true);
    void *d_u = stage(u, nsolve * n * sizeof(float), false);
    void *d_it = niter ? stage(niter, nsolve * sizeof(int), false) : nullptr;
    void *d_ie = ierr ? stage(ierr, nsolve * sizeof(int), false) : nullptr;
    void *ws = nullptr;
    if (!d_src || !d_slow || !d_u || (niter && !d_it) || (ierr && !d_ie)) rc = -1;
    if (!rc) {
        b.src = (const double *)d_src; b.slow = d_slow; b.u_out = d_u;
        b.niter = (int *)d_it; b.ierr = (int *)d_ie;
        const size_t wsb = mceik_fsm_workspace_bytes(&b);
        if (hipMalloc(&ws, wsb) != hipSuccess) rc = -1;
        else rc = mceik_fsm_batch_solve(&b, ws, wsb, nullptr);
        if (!rc && hipDeviceSynchronize() != hipSuccess) rc = -1;
    }
    if (!rc && d_u != u) rc = hipMemcpy(u, d_u, nsolve * n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess;
    if (!rc && niter && d_it != niter) rc = hipMemcpy(niter, d_it, nsolve * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess;
    if (!rc && ierr && d_ie != ierr) rc = hipMemcpy(ierr, d_ie, nsolve * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess;
    if (ws) hipFree(ws);
    for (void *p : tmp) hipFree(p);
    return rc;
}

extern "C" int mceik_memcpy(void *dst, const void *src, size_t bytes, int kind)
{
    hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIPCHK(hipMemcpy(dst, src, bytes, k));
    return 0;
}
