// rt_trace_iow.hip -- batched closest-hit ray queries on an IOW-03 device scene (rt_trace_iow_rays_async).
//
// One lane answers one query with the render kernels' own LaunchRay (iow_launch_ray, rt_iow_walk.hpp;
// 03_Shadows_and_Materials/computeShaderSrc.glsl:196-256): the 4-wide culling walk with postponed
// leaves where the direction is near unit length and the scene has a BVH, else the reference's linear
// loop.  No sample loop, no ray stack, no speculation records: the kernel is the search and its hit
// evaluation alone, so its registers and its rate are theirs.
#include "rt_iow_walk.hpp"

namespace rtk {

// A query is 2 float4 (rt_ray: origin, tmax | direction, ratio -- ignored here), an answer 2 float4
// (rt_hit: t, id, normal.xy | normal.z, extra, 0, 0).  The grid is persistent: each wave claims
// 64 * rounds consecutive queries from `queue` with one atomic and answers them 64 at a time, until
// none are left.  One claim per 64 queries caps the kernel at about 5.5 G queries/s on an MI355X
// whatever the rays (the same-address atomics serialise, about 12 ns each: DESIGN.md 5.8), so large
// batches claim up to kClaimRounds x 64 (claim_grid).
// LN: the scene's 4-wide BVH (at most kIowLdsNodes nodes) is staged in the block's LDS at 7 float4
// per node and the per-lane link stack has 16 slots (13 usable: the branch-free pushes of a step may
// write 3 above the top); else nodes come from global memory at 8 float4 and the stack has 32 (29).
// A walk that overflows re-runs the linear loop (iow_launch_ray).  S.nodes == null: the linear loop.
// ANY (RT_TRACE_ANY): the search is the closest-hit one; the normal and extra are not reported.
// Lanes without a walk -- the ragged tail of a batch, tmax <= 0 or NaN, directions sent to the linear
// loop -- sit outside the walk's branch, so its __all / __ballot votes count walking lanes only.
template <bool ANY, bool LN>
__global__ __launch_bounds__(kBlock) void k_iow_trace(IowScene S, int leaf_batch, const float4 *__restrict__ rays,
                                                      uint32_t n_rays, float4 *__restrict__ hits,
                                                      unsigned long long *counters, unsigned *queue,
                                                      uint32_t rounds) {
    using Cfg = IowCfg<false, 1, LN>;
    __shared__ short lds_bvh[Cfg::BS * kBlock];
    __shared__ float4 s_nodes[LN ? kIowLdsNodes * 7 : 1];
    short *bstk = lds_bvh + threadIdx.x;  // bslot's layout
    const float4 *nodes = iow_stage_nodes<LN>(S, s_nodes);
    Frame F{};
    F.leaf_batch = leaf_batch;
    Ctr c;
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(queue, 64u * rounds);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (base >= n_rays) break;
#pragma unroll 1
        for (uint32_t k = 0; k < rounds; k++) {
            const uint32_t q = base + k * 64u + lane;  // < 2^32: n_rays <= 2^31
            if (q >= n_rays) continue;
            const float4 r0 = rays[2 * (size_t)q], r1 = rays[2 * (size_t)q + 1];
            const f3 o = mk(r0.x, r0.y, r0.z), d = mk(r1.x, r1.y, r1.z);
            const float tmax = r0.w;
            float t = tmax, extra = 0.0f;
            int id = -1;
            f3 n = f3{0, 0, 0};
            if (tmax > 0.0f) {  // else (or NaN) a miss by the shader's test: min_t > t && t > 0 never holds
                float min_t = tmax;
                int best = -1;
                const RayRet r = iow_launch_ray<Cfg::BS - 3, Cfg::NS>(
                    S, F, o, d, tmax, 1.0f, c, bstk, nodes, [&](float m, int j) { min_t = m; best = j; });
                if (min_t < tmax) {
                    t = min_t; id = best;
                    if (!ANY) { n = r.normal; extra = r.material.z; }
                }
            } else {
                c.seg++;
            }
            hits[2 * (size_t)q] = make_float4(t, __int_as_float(id), n.x, n.y);
            hits[2 * (size_t)q + 1] = make_float4(n.z, extra, 0.0f, 0.0f);
        }
    }
    if (!counters) return;
    const unsigned long long v[3] = {c.seg, c.nodes, c.prims};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const unsigned long long s = wave_sum(v[i]);
        if (lane == 0 && s) atomicAdd(counters + i, s);
    }
}

namespace {
template <bool ANY, bool LN>
int trace_blocks() {  // resident blocks per CU, asked once
    static const int nb = occupancy_of(k_iow_trace<ANY, LN>, kBlock);
    return nb;
}
template <bool ANY, bool LN>
hipError_t trace_info(int info[4]) {
    return kernel_info(k_iow_trace<ANY, LN>, trace_blocks<ANY, LN>(), info);
}
}  // namespace

int iow_trace_blocks_per_cu(bool any, bool ln) {
    return any ? (ln ? trace_blocks<true, true>() : trace_blocks<true, false>())
               : (ln ? trace_blocks<false, true>() : trace_blocks<false, false>());
}

hipError_t iow_trace_kernel_info(bool any, bool ln, int info[4]) {
    return any ? (ln ? trace_info<true, true>(info) : trace_info<true, false>(info))
               : (ln ? trace_info<false, true>(info) : trace_info<false, false>(info));
}

hipError_t launch_iow_trace(const IowScene &sc, int leaf_batch, const float4 *rays, uint32_t n_rays, bool any,
                            float4 *hits, unsigned long long *counters, unsigned *queue, int cus, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(queue, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const bool ln = iow_lds(sc);
    const ClaimGrid cg = claim_grid(n_rays, cus, iow_trace_blocks_per_cu(any, ln), 0);
    const dim3 g(cg.grid), b(kBlock);
    if (any) {
        if (ln) hipLaunchKernelGGL((k_iow_trace<true, true>), g, b, 0, s, sc, leaf_batch, rays, n_rays, hits, counters, queue, cg.rounds);
        else hipLaunchKernelGGL((k_iow_trace<true, false>), g, b, 0, s, sc, leaf_batch, rays, n_rays, hits, counters, queue, cg.rounds);
    } else {
        if (ln) hipLaunchKernelGGL((k_iow_trace<false, true>), g, b, 0, s, sc, leaf_batch, rays, n_rays, hits, counters, queue, cg.rounds);
        else hipLaunchKernelGGL((k_iow_trace<false, false>), g, b, 0, s, sc, leaf_batch, rays, n_rays, hits, counters, queue, cg.rounds);
    }
    return hipGetLastError();
}

}  // namespace rtk
