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
