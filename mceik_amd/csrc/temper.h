// temper.h -- the swap round of parallel tempering (not public; the C-ABI is
// in include/mceik.h, the definition in DESIGN.md s.11).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hypo.h"
#include "mcmc_common.h"
#include "nuis.h"
#include "vor.h"

// One swap round of the whole sampler (D is the sampler's state, never a
// pipe's view; D.beta set) on stream st: the decide kernel, then the exchange
// kernel.  Pair p in [0, (ntemps - 1) * G), G = D.nchains / ntemps, is lower
// chain p and upper chain p + G (rung p / G); pairs whose rung has the other
// parity sit the round out.  gs is the Philox counter (the global step the
// round belongs to).  flag: [(ntemps - 1) * G] ints of scratch; attempts,
// accepts: [ntemps - 1] counters.  H (or null): the chains' hypocentres and
// event lists, N (or null) their nuisance state (kn, kc and the effective
// rows), exchanged with the models; the current tables wherever the sampler
// keeps them (D.ttab_cur).  V (or null): the sampler's Voronoi state, whose
// nuclei rows and counts are exchanged with the models.  No host synchronisation.
hipError_t temper_swap_round(const McmcDev &D, int ntemps, int parity, uint64_t gs, int *flag,
                             unsigned long long *attempts, unsigned long long *accepts, hipStream_t st,
                             const HypoDev *H = nullptr, const NuisDev *N = nullptr, const VorDev *V = nullptr);
