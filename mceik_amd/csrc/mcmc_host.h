// mcmc_host.h -- host launchers of the sampler's kernels (mcmc_kernels.hip),
// C++ linkage; sampler.hip and block.hip are their callers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_common.h"
#include "nuis.h"

hipError_t mcmc_propose(const McmcDev &D, uint64_t step, hipStream_t st);
// N: the chains' nuisance state (nuis.h; N.kn null: none)
hipError_t mcmc_init_loglik(const McmcDev &D, const NuisDev &N, hipStream_t st);
hipError_t mcmc_accept(const McmcDev &D, const NuisDev &N, int keep_slot, hipStream_t st);
// The kept-state copy alone (block.hip's accept launches it after its own kernel).
hipError_t mcmc_keep(const McmcDev &D, int keep_slot, hipStream_t st);
hipError_t mcmc_lpt_order(const unsigned long long *clk, int nsolve, int *order, hipStream_t st);
