// rt_device.hpp -- the host units' device plumbing: error checks, the RAII device buffer, the
// device check, the launch-failure epilogue, event timing and the counter read-back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/rt_hip.h"

#define HIP_OK(expr)                                             \
    do {                                                         \
        hipError_t e_ = (expr);                                  \
        if (e_ != hipSuccess) {                                  \
            std::fprintf(stderr, "[rt_hip] %s failed: %s\n", #expr, hipGetErrorString(e_)); \
            return RT_E_HIP;                                     \
        }                                                        \
    } while (0)

struct DevBuf {  // RAII device allocation
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    void reset() {  // free and null
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t alloc(size_t b) {  // a fresh allocation of b bytes (what the buffer held is freed)
        reset();
        bytes = b;
        return hipMalloc(&p, b ? b : 16);
    }
    hipError_t upload(const void *src, size_t b) {
        hipError_t e = alloc(b);
        if (e != hipSuccess || !b) return e;
        return hipMemcpy(p, src, b, hipMemcpyHostToDevice);
    }
    // at least b bytes of capacity (contents undefined; `bytes` stays the capacity)
    hipError_t reserve(size_t b) { return p && bytes >= b ? hipSuccess : alloc(b); }
    // copy b bytes in, reusing the allocation when it is large enough (a scene update); `bytes`
    // stays the capacity
    hipError_t store(const void *src, size_t b) {
        if (!p || b > bytes) {
            hipError_t e = alloc(b);
            if (e != hipSuccess) return e;
        }
        return b ? hipMemcpy(p, src, b, hipMemcpyHostToDevice) : hipSuccess;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

inline int check_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return RT_E_NODEVICE;
    if (device >= 0) {
        if (device >= count) return RT_E_NODEVICE;
        if (hipSetDevice(device) != hipSuccess) return RT_E_HIP;
    }
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return RT_E_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cur) != hipSuccess) return RT_E_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RT_E_NODEVICE;
    return RT_OK;
}

// a failed enqueue: prints what failed, returns RT_E_HIP
inline int hip_failed(const char *what, hipError_t e) {
    std::fprintf(stderr, "[rt_hip] %s: %s\n", what, hipGetErrorString(e));
    return RT_E_HIP;
}
// the epilogue of every function that enqueues a render or a query
inline int launch_failed(hipError_t e) { return hip_failed("launch failed", e); }

// device time of the work enqueued by `fn` on the null stream
template <class F> int timed(F &&fn, double *ms) {
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    HIP_OK(hipEventRecord(e0, nullptr));
    const int rc = fn();
    HIP_OK(hipEventRecord(e1, nullptr));
    HIP_OK(hipEventSynchronize(e1));
    float t = 0.0f;
    (void)hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (ms) *ms = t;
    return rc;
}

// the six device counters of a render or query (d_ctr) and its time into *st
inline int read_stats(const void *d_ctr, double ms, rt_stats *st) {
    unsigned long long c[6];
    HIP_OK(hipMemcpy(c, d_ctr, sizeof(c), hipMemcpyDeviceToHost));
    st->segments = c[0]; st->node_visits = c[1]; st->prim_tests = c[2];
    st->shadow_queries = c[3]; st->stack_drops = c[4]; st->nan_drops = c[5];
    st->ms = ms;
    return RT_OK;
}
