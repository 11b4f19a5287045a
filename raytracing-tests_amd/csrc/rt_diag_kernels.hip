// rt_diag_kernels.hip -- kernels no render reaches: the sample-parallel pass's statistics behind
// the debug ABI (rt_capi_debug.hip) and the exhaustive check of rt_math.hpp's shortened sequences.
#include "rt_kernels.hpp"
#include "rt_math.hpp"

namespace rtk {

// diagnostics: log2 histogram of rays per sample over the last sample-parallel render
__global__ void k_spec_hist(const uint4 *ctr, size_t n, unsigned long long *out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned v = ctr[i].x;
        if (v == 0) continue;
        const int b = 31 - __clz(v);
        atomicAdd(out + 2 + b, 1ull);
        atomicAdd(out + 34 + b, (unsigned long long)v);
        atomicMax(out, (unsigned long long)v);
        atomicAdd(out + 1, 1ull);
    }
}
// diagnostics: per pixel unit (sample-0 rays, max rays of a sample, that sample, rank in `order`)
__global__ void k_spec_pixels(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *order, uint32_t *out) {
    const uint32_t pu = blockIdx.x * blockDim.x + threadIdx.x;
    if (pu >= P) return;  // no cross-lane work in this kernel
    uint32_t mx = 0, arg = 0;
    for (uint32_t s = 0; s < S; s++) {
        const uint32_t v = ctr[(size_t)pu * S + s].x;
        if (v > mx) { mx = v; arg = s; }
    }
    out[4 * (size_t)pu] = ctr[(size_t)pu * S].x;
    out[4 * (size_t)pu + 1] = mx;
    out[4 * (size_t)pu + 2] = arg;
    out[4 * (size_t)order[pu] + 3] = pu;  // out[.3] of row r = the pixel at order rank r
}
hipError_t spec_pixels(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *order, uint32_t *d_out,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_spec_pixels, dim3((P + 255) / 256), dim3(256), 0, s, ctr, P, S, order, d_out);
    return hipGetLastError();
}
// diagnostics: where re-executed samples first read a stale entry (RT_DEBUG_FIRST_STALE runs):
// out[b] = samples, out[16 + b] = their rays, bucket b = 16 * first_stale_segment / rays
__global__ void k_spec_list_stale(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *list, const unsigned *count,
                                  unsigned long long *out) {
    const unsigned n = *count;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 c = ctr[spec_rec_ix(list[i], P, S)];
        if (!(c.y & 0x80000000u) || c.x == 0) continue;
        const unsigned b = min(15u, (unsigned)(((unsigned long long)(c.y & 0x7fffffffu) * 16ull) / c.x));
        atomicAdd(out + b, 1ull);
        atomicAdd(out + 16 + b, (unsigned long long)c.x);
    }
}
hipError_t spec_list_stale(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *list, const unsigned *count,
                           unsigned long long *d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_list_stale, dim3(1024), dim3(256), 0, s, ctr, P, S, list, count, d_out);
    return hipGetLastError();
}
// diagnostics: log2 histogram of the rays of the samples on the (first) re-execution list
__global__ void k_spec_list_hist(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *list, const unsigned *count,
                                 unsigned long long *out) {
    const unsigned n = *count;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned v = ctr[spec_rec_ix(list[i], P, S)].x;
        if (v == 0) continue;
        const int b = 31 - __clz(v);
        atomicAdd(out + 2 + b, 1ull);
        atomicAdd(out + 34 + b, (unsigned long long)v);
        atomicMax(out, (unsigned long long)v);
        atomicAdd(out + 1, 1ull);
    }
}
hipError_t spec_list_hist(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *list, const unsigned *count,
                          unsigned long long *d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_list_hist, dim3(1024), dim3(256), 0, s, ctr, P, S, list, count, d_out);
    return hipGetLastError();
}
hipError_t spec_hist(const uint4 *ctr, size_t n, unsigned long long *d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_hist, dim3(2048), dim3(256), 0, s, ctr, n, d_out);
    return hipGetLastError();
}
// The shortened sequences of rt_math.hpp against the compiler's correctly rounded ones over
// every bit pattern x (NaN == NaN): which 0 = rcp_sqrt_domain(sqrt(x)) vs 1.0f / sqrt(x).
// (An unscaled sqrt candidate failed here for 20.7M inputs, the denormal and tiny ones.)
__global__ __launch_bounds__(kBlock) void k_check_fastmath(int which, unsigned long long *bad, unsigned *first) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < (1ull << 32); i += stride) {
        const float xi = __uint_as_float((uint32_t)i);
        const float b = __builtin_sqrtf(xi);
        const float x = rcp_sqrt_domain(b), y = 1.0f / b;
        if (__float_as_uint(x) != __float_as_uint(y) && !(x != x && y != y)) {
            atomicAdd(bad, 1ull);
            atomicMin(first, (uint32_t)i);
        }
    }
}
hipError_t launch_check_fastmath(int which, unsigned long long *bad, unsigned *first, hipStream_t s) {
    hipLaunchKernelGGL(k_check_fastmath, dim3(4096), dim3(kBlock), 0, s, which, bad, first);
    return hipGetLastError();
}

}  // namespace rtk
