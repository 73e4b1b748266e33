// host_util.h -- host-side helpers every translation unit shares (not public).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

// Runs the calling scope on `dev` and restores the caller's device: every
// entry point runs on its object's device.
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceScope()
    {
        if (prev >= 0) hipSetDevice(prev);
    }
};

// 128-bit integers as two 64-bit words (lo, hi): the exact partials of
// posterior.hip, cov.hip and ess.hip.  Two's complement, so a signed sum adds
// through the same words (cast get128's value where the sign matters).
typedef unsigned __int128 u128;
typedef __int128 i128;

static inline u128 get128(const unsigned long long *w) { return ((u128)w[1] << 64) | w[0]; }

static inline void add128(unsigned long long *d, const unsigned long long *a, size_t n = 1)    // d[k] += a[k], n values
{
    for (size_t k = 0; k < n; k++) {
        const u128 t = get128(d + 2 * k) + get128(a + 2 * k);
        d[2 * k] = (unsigned long long)t;
        d[2 * k + 1] = (unsigned long long)(t >> 64);
    }
}

// HIPCHK(x): on a HIP failure print "<who>: x failed: <error> (file:line)" and
// return -1 from the calling function.  A file that reports under another
// name than mceik_hip defines HIPCHK_WHO before including this header.
#ifndef HIPCHK_WHO
#define HIPCHK_WHO "mceik_hip"
#endif
#define HIPCHK(x)                                                                      \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, HIPCHK_WHO ": %s failed: %s (%s:%d)\n", #x,                \
                    hipGetErrorString(e_), __FILE__, __LINE__);                        \
            return -1;                                                                 \
        }                                                                              \
    } while (0)
