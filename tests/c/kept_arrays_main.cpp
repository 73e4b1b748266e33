// The descriptor-list helpers of mceik_amd/csrc/kept.h on host memory: the HIP
// calls they make are renamed to the stubs below, so this program needs no GPU
// and can be built with -fsanitize=address,undefined (host buffers are exactly
// as long as a descriptor says, so a helper that moved one byte more is caught).
// Prints "ok" and returns 0, or says what failed.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static int live = 0, fail_at = -1, nmalloc = 0;

static hipError_t stub_malloc(void **p, size_t n)
{
    if (nmalloc++ == fail_at) return hipErrorOutOfMemory;
    *p = malloc(n);
    memset(*p, 0xAB, n);
    live++;
    return hipSuccess;
}
static hipError_t stub_free(void *p) { free(p); live--; return hipSuccess; }
static hipError_t stub_memset(void *p, int v, size_t n) { memset(p, v, n); return hipSuccess; }
static hipError_t stub_memset_async(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
static hipError_t stub_memcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }

#define hipMalloc stub_malloc
#define hipFree stub_free
#define hipMemset stub_memset
#define hipMemsetAsync stub_memset_async
#define hipMemcpy stub_memcpy
#include "../../mceik_amd/csrc/kept.h"

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            printf("line %d: %s\n", __LINE__, #x);                     \
            return 1;                                                  \
        }                                                              \
    } while (0)

static bool all_bytes(const void *p, int v, size_t n)
{
    for (size_t k = 0; k < n; k++)
        if (((const unsigned char *)p)[k] != (unsigned char)v) return false;
    return true;
}

// One list: sizes and slacks as given; the whole lifecycle on it.
static int run(const std::vector<size_t> &bytes, size_t slack)
{
    const int na = (int)bytes.size();
    std::vector<void *> dev(na, nullptr);
    std::vector<KeptArray> a(na);
    for (int k = 0; k < na; k++) a[k] = {&dev[k], bytes[k], slack};
    nmalloc = 0; fail_at = -1;
    CHECK(kept_arrays_alloc(a.data(), na));
    for (int k = 0; k < na; k++) {
        CHECK((dev[k] != nullptr) == (bytes[k] + slack > 0));
        if (dev[k]) CHECK(all_bytes(dev[k], 0, bytes[k] + slack));
    }
    // set: every existing array needs its host side; what is given is copied, byte for byte
    std::vector<std::vector<unsigned char>> src(na), dst(na);
    std::vector<const void *> hs(na);
    std::vector<void *> hd(na);
    for (int k = 0; k < na; k++) {
        src[k].assign(bytes[k], (unsigned char)(k + 1));
        dst[k].assign(bytes[k], 0xEE);
        hs[k] = bytes[k] ? src[k].data() : nullptr;
        hd[k] = bytes[k] ? dst[k].data() : nullptr;
    }
    CHECK(!kept_arrays_missing(a.data(), na, hs.data()));
    for (int k = 0; k < na; k++) {
        if (!bytes[k]) continue;
        const void *keep = hs[k];
        hs[k] = nullptr;
        CHECK(kept_arrays_missing(a.data(), na, hs.data()));
        hs[k] = keep;
    }
    CHECK(kept_arrays_copy(a.data(), na, (void *const *)hs.data(), false) == hipSuccess);
    for (int k = 0; k < na; k++)
        if (dev[k]) CHECK(all_bytes(dev[k], k + 1, bytes[k]) && all_bytes((char *)dev[k] + bytes[k], 0, slack));
    // get: a null host pointer is skipped, the others receive exactly `bytes`
    for (int skip = -1; skip < na; skip++) {
        for (int k = 0; k < na; k++) {
            dst[k].assign(bytes[k], 0xEE);
            hd[k] = bytes[k] && k != skip ? dst[k].data() : nullptr;
        }
        CHECK(kept_arrays_copy(a.data(), na, hd.data(), true) == hipSuccess);
        for (int k = 0; k < na; k++) CHECK(all_bytes(dst[k].data(), k == skip ? 0xEE : k + 1, bytes[k]));
    }
    // zero in place: the sums, not the slack (it is zero from the allocation on)
    CHECK(kept_arrays_zero(a.data(), na, nullptr) == hipSuccess);
    for (int k = 0; k < na; k++)
        if (dev[k]) CHECK(all_bytes(dev[k], 0, bytes[k] + slack));
    kept_arrays_free(a.data(), na);
    for (int k = 0; k < na; k++) CHECK(!dev[k]);
    CHECK(live == 0);
    kept_arrays_free(a.data(), na);                   // twice is harmless
    // an allocation that fails at any place leaves a list that frees cleanly
    int nexist = 0;
    for (int k = 0; k < na; k++) nexist += bytes[k] + slack > 0;
    for (int f = 0; f < nexist; f++) {
        nmalloc = 0; fail_at = f;
        CHECK(!kept_arrays_alloc(a.data(), na));
        CHECK(live == f);
        kept_arrays_free(a.data(), na);
        CHECK(live == 0);
    }
    return 0;
}

int main()
{
    if (run({24, 24, 40}, 0)) return 1;               // the posterior: sum, sumsq, hist
    if (run({24, 24, 0}, 0)) return 1;                // ... without bins
    if (run({8, 64, 96, 96, 768, 32, 384}, 0)) return 1;   // covariances, within
    if (run({160, 0, 40, 80, 80}, 0)) return 1;       // batch means at one level: no pend
    if (run({160, 320, 120, 240, 240}, 0)) return 1;
    if (run({48, 48, 96, 96, 16, 32, 512, 24}, 16)) return 1;   // data fit: 16 bytes of slack each
    if (run({0, 0, 0, 0, 16, 32, 512, 24}, 16)) return 1;       // ... without observations: slack alone is allocated
    if (run({}, 0)) return 1;
    printf("ok\n");
    return 0;
}
