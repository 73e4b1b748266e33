// fsm_batch.h -- launch sizing and workspace layout of the batched FSM solve
// (fsm_batch.hip), as the sampler and the single-solve drop-ins use them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/mceik.h"
#include "fsm_common.h"

void fill_launch(FsmLaunch &L, const mceik_fsm_batch *b);
int device_cus();

// Waves of a batch before the scratch budget caps them.
int fsm_batch_waves_uncapped(const mceik_fsm_batch *b);

// Workspace: [8 queue heads, 1 KiB][slow brick copy (mode 0)][u scratch][u0 scratch]
struct WsLayout {
    size_t counter, slow, u, u0, zf, total;
    int nwaves;
};
WsLayout ws_layout(const mceik_fsm_batch *b);

// The sampler's multi-step launch (FsmLaunch mc_*): not part of the public batch.
#define MCEIK_MC_CHUNK 64        // steps per multi-step launch (bounds one kernel's duration)
struct McmcExt {
    const void *dev;             // device copy of the sampler's McmcDev
    unsigned *sync;              // MC_SYNC_WORDS(nchains) words, zeroed here before the launch (but the last)
    unsigned spin_limit;
    int step0, nsteps, nburn, keepk, maxs, nkept0;
};

// mceik_fsm_batch_solve with the multi-step extension (ext may be null).
int fsm_batch_solve_impl(const mceik_fsm_batch *b, void *workspace, size_t workspace_bytes, void *stream,
                         const McmcExt *ext);
