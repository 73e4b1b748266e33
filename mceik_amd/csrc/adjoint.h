// adjoint.h -- the discrete adjoint of the batched eikonal solve (adjoint.hip;
// the C-ABI is in include/mceik.h mceik_fsm_adjoint_*, the definition in
// DESIGN.md s.17; not public).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mceik.h"

#define ADJ_THREADS 512          // one workgroup per resident solve
#define ADJ_DEFAULT_GROUPS 256   // resident workgroups when max_groups = 0 (one per CU of an MI355X)

// Per-node flags of the pre-pass: bit k (0..2) = axis k's chosen upwind side
// (0 minus, 1 plus), bit 3 + k = axis k participates (a_k < u), bit 6 = the
// node lies in the source's SETBCS box.
#define ADJ_SIDE(k) (1u << (k))
#define ADJ_PART(k) (8u << (k))
#define ADJ_BC 64u

// One launch.  A workgroup owns one slice of the workspace and runs its items
// (solves, or with by_model a model's stations in order) one after the other
// in it: lam [n] | q [n] | w [3][n] fp64 | flags [n] u8.
struct AdjLaunch {
    int nx, ny, nz, ncx, ncy, ncz, nrx, nry, nrz;
    int nmodel, nstat, nsolve, nphase, slow_mode, cap, by_model;
    int nev, ev_stride;
    double h, x0, y0, z0;
    const double *src;           // [nstat][4]
    const void *slow;
    const int *model_phase;
    const unsigned char *skip;
    const int *ev_node;
    const float *ev_frac;
    const double *ev_w;          // [nsolve][nev]
    const void *u;               // [nsolve][n] fp32 / fp64
    double *grad, *grad_solve, *lam;
    int *niter, *status;
    char *ws;
    size_t ws_group;             // bytes of one workgroup's slice
};

// Bytes of one workgroup's slice for a field of n nodes.
static inline size_t adj_group_bytes(size_t n)
{
    return ((n * (5 * sizeof(double) + 1)) + 255) & ~(size_t)255;
}
