// fsm_host.h -- host launchers of the batched FSM kernels (fsm_kernel.hip,
// fsm16_kernel.hip), C++ linkage; fsm_batch.hip is their caller.
#pragma once
#include <hip/hip_runtime.h>

#include "fsm_common.h"

// fsm_kernel.hip: the instance a launch runs (8-z variants or the 16-z kernel)
hipError_t fsm_launch(const FsmLaunch &L, int is_double, int nwaves, hipStream_t st);
hipError_t fsm_zero_words(unsigned *p, int n, hipStream_t st);
int fsm_occupancy(const FsmLaunch &L, int is_double);
size_t fsm_launch_lds_bytes(const FsmLaunch &L, int is_double);
int fsm_launch_kind(const FsmLaunch &L, int is_double);
const char *fsm_launch_name(const FsmLaunch &L, int is_double);
hipError_t fsm_to_brick_f64(const double *src, void *dst, int dst_double, const FsmLaunch &L, int nfield, hipStream_t st);
hipError_t fsm_from_brick_f64(const void *src, int src_double, double *dst, const FsmLaunch &L, int nfield, hipStream_t st);
hipError_t fsm_from_brick_f32(const float *src, float *dst, const FsmLaunch &L, int nfield, hipStream_t st);
hipError_t fsm_to_brick_f32(const float *src, float *dst, const FsmLaunch &L, int nfield, hipStream_t st);

// fsm16_kernel.hip: the 16-z-step kernel (fsm_kernel.hip's use_fsm16 picks it)
hipError_t fsm16_launch(const FsmLaunch &L, int nwaves, hipStream_t st);
int fsm16_occupancy(const FsmLaunch &L);
