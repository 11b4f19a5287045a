// rt_trace.hip -- batched closest-hit ray queries on an INW device scene (rt_trace_rays_async).
//
// One lane answers one query with the render kernels' own closest-hit walk (inw_closest,
// rt_inw_walk.hpp): the 4-wide culling walk where it is exact, else the reference's LBVH walk
// (01_BoundingVolumeHierarchy/computeShaderSrc.glsl:431-473, 04...glsl:524-563), on an empty
// 40-float stack in LDS.  No sample loop, no pending-ray stack, no fold: the kernel is the walk
// alone, so its registers and its rate are the walk's.
#include "rt_inw_walk.hpp"

namespace rtk {

// A query is 2 float4 (rt_ray: origin, tmax | direction, time ratio), an answer 2 float4 (rt_hit:
// t, id, normal.xy | normal.z, extra, 0, 0).  The grid is persistent: each wave claims 64
// consecutive queries from `queue` until none are left.
// ANY (RT_TRACE_ANY): no normal or extra data is computed; the walk is the closest-hit one, so the
// reported object is the closest (the contract allows any accepted one).
// FU: the wide walk culls with one fma per plane (cull4nf<true>).  Its error bound needs the ray
// origin within 1000 of the world origin on every axis (rt_inw_walk.hpp, cull4nf); the host checks
// the scene's boxes, the kernel each query's origin: a lane whose origin is farther out runs with
// dfs_high past the stack, which is the walks' own "a push could drop" condition, so inw_closest
// hands it to the reference's stack walk.
// The origin test holds without the fused cull too.  The wide walk stops at t * 1.0001 + 1e-3 because a
// hit lies no nearer than its box entry; from 10^6 away the object test's t is off by hundreds (the
// quadratic cancels) while the box entry is not, t < entry for every hit, and the reference -- which
// then keeps the first hit its depth-first order reaches -- and the near-to-far walk answered
// differently (tests/test_gpu_query_edges.py, class org_1e6).
template <bool ANY, bool FU>
__global__ __launch_bounds__(kBlock) void k_inw_trace(InwScene S, const float4 *__restrict__ rays, uint32_t n_rays,
                                                      uint32_t invert, float4 *__restrict__ hits,
                                                      unsigned long long *counters, unsigned *queue) {
    __shared__ float lds[kFStack * kBlock];
    Ctr c;
    FStack K{lds + threadIdx.x, 0};
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(queue, 64u);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (base >= n_rays) break;
        const uint32_t q = base + lane;
        if (q < n_rays) {
            const float4 r0 = rays[2 * (size_t)q], r1 = rays[2 * (size_t)q + 1];
            const f3 o = mk(r0.x, r0.y, r0.z), d = mk(r1.x, r1.y, r1.z);
            const float tmax = r0.w, ratio = r1.w;
            float tlim = tmax, extra = 0.0f, g = -1.0f;
            f3 n = f3{0, 0, 0};
            c.seg++;
            if (tmax > 0.0f) {  // else (or NaN) a miss by the shader's tests: t > 0 && t < t_limiting never holds
                InwScene Sq = S;
                if (!(fabsf(o.x) <= 1000.0f && fabsf(o.y) <= 1000.0f && fabsf(o.z) <= 1000.0f))
                    Sq.dfs_high = (uint32_t)kFStack + 1u;
                // the time ratio is the caller's: the time-bin trees (and the swept tree's boxes) cover
                // ratios 0..1 only, and the bin index of any other ratio (or NaN) names no tree
                if (!(ratio >= 0.0f && ratio <= 1.0f)) Sq.dfs_high = (uint32_t)kFStack + 1u;
                K.size = 0;
                g = inw_closest<!ANY, false, FU>(Sq, K, o, d, ratio, invert != 0u, tlim, n, extra, -1.0f, c);
            }
            const bool hit = tlim < tmax;  // t_limiting ended below tmax
            if (ANY || !hit) { n = f3{0, 0, 0}; extra = 0.0f; }
            hits[2 * (size_t)q] = make_float4(hit ? tlim : tmax, __int_as_float(hit ? (int)g : -1), n.x, n.y);
            hits[2 * (size_t)q + 1] = make_float4(n.z, extra, 0.0f, 0.0f);
        }
    }
    if (!counters) return;
    const unsigned long long v[4] = {c.seg, c.nodes, c.prims, c.drops};
    const int slot[4] = {0, 1, 2, 4};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned long long s = wave_sum(v[i]);
        if (lane == 0 && s) atomicAdd(counters + slot[i], s);
    }
}

namespace {
template <bool ANY, bool FU>
int trace_blocks() {  // resident blocks per CU, asked once
    static const int nb = occupancy_of(k_inw_trace<ANY, FU>, kBlock);
    return nb;
}
template <bool ANY, bool FU>
hipError_t trace_info(int info[4]) {
    return kernel_info(k_inw_trace<ANY, FU>, trace_blocks<ANY, FU>(), info);
}
}  // namespace

int inw_trace_blocks_per_cu(bool any, bool fused) {
    return any ? (fused ? trace_blocks<true, true>() : trace_blocks<true, false>())
               : (fused ? trace_blocks<false, true>() : trace_blocks<false, false>());
}

hipError_t inw_trace_kernel_info(bool any, bool fused, int info[4]) {
    return any ? (fused ? trace_info<true, true>(info) : trace_info<true, false>(info))
               : (fused ? trace_info<false, true>(info) : trace_info<false, false>(info));
}

hipError_t launch_inw_trace(const InwScene &sc, const float4 *rays, uint32_t n_rays, bool invert, bool any,
                            float4 *hits, unsigned long long *counters, unsigned *queue, int cus, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(queue, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const bool fu = sc.fused != 0;
    const dim3 g(claim_grid(n_rays, cus, inw_trace_blocks_per_cu(any, fu), 0).grid), b(kBlock);  // claims of 64
    const uint32_t inv = invert ? 1u : 0u;
    if (any) {
        if (fu) hipLaunchKernelGGL((k_inw_trace<true, true>), g, b, 0, s, sc, rays, n_rays, inv, hits, counters, queue);
        else hipLaunchKernelGGL((k_inw_trace<true, false>), g, b, 0, s, sc, rays, n_rays, inv, hits, counters, queue);
    } else {
        if (fu) hipLaunchKernelGGL((k_inw_trace<false, true>), g, b, 0, s, sc, rays, n_rays, inv, hits, counters, queue);
        else hipLaunchKernelGGL((k_inw_trace<false, false>), g, b, 0, s, sc, rays, n_rays, inv, hits, counters, queue);
    }
    return hipGetLastError();
}

}  // namespace rtk
