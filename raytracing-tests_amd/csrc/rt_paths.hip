// rt_paths.hip -- batched path (radiance) queries on an INW device scene (rt_path_rays_async).
//
// One query is one invocation of the reference shaders' out_Pixel ray loop
// (01_BoundingVolumeHierarchy/computeShaderSrc.glsl:414-597, 04_Lights_Camera_And_Action/
// computeShaderSrc.glsl:510-713) started from the caller's ray instead of the camera's: an empty
// 40-float stack, push_ray(o, d, 1, 0), then the render kernels' own segment body (inw_segment,
// rt_inw_shade.hpp) until the stack is empty.  No pixels, no camera, no End() fold: a frame is the
// fold of the path queries of its camera rays, bit for bit.
#include "rt_inw_shade.hpp"

namespace rtk {

// Waves per SIMD.  The 40 KB of stacks allow 4 blocks per CU, but at 4 waves (128 VGPRs) the INW-01
// instances spill 11 to 12 registers to scratch; at 3 neither layout uses scratch (DESIGN.md 5.9 has
// the table).
constexpr int kPathWaves = 3;

// A query is 2 float4 (rt_path_ray: origin, sample | direction, pad), an answer 2 float4
// (rt_path_out: rgb, depth | segments, drops, nans, status).
// The grid is persistent and so is every lane: one lane owns one path at a time on its column of
// the LDS stacks, and a lane whose path ends takes the next unanswered query at once -- paths of
// one batch run from 1 to hundreds of segments, so a wave that waited for its longest path would
// idle most of its lanes.  A wave claims 64 * rounds consecutive queries from `queue` with one
// atomic (one claim per 64 queries caps a kernel near 5.5 G claims/s: DESIGN.md 5.8) and hands
// indices of that range to its free lanes by ballot and popcount: no atomic per lane or per query.
// No wave retires while the queue holds queries.
// FU: the wide walk culls with one fma per plane (cull4nf<true>); its error bound needs ray origins
// within 1000 of the world origin on every axis.  Bounce origins lie on objects inside the scene's
// boxes (the host checks those); a path whose query origin is farther out runs with dfs_high past
// the stack, the walks' own "a push could drop" condition, which sends all of it to the
// reference's walks (as k_inw_trace does per query).  The origin test holds without the fused cull
// too: thousands of units from the objects the object test's t falls below the hit's own box entry,
// which the wide walk's cut at t * 1.0001 + 1e-3 assumes it never does (rt_trace.hip).
template <bool LIGHTS, bool FU>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kPathWaves)))
void k_inw_paths(InwScene S, const float4 *__restrict__ rays, uint32_t n_rays, uint32_t spp, int max_bounces,
                 float inv_spp, uint32_t invert, float4 *__restrict__ out, unsigned long long *counters,
                 unsigned *queue, uint32_t rounds) {
    __shared__ float lds[kFStack * kBlock];
    Frame F{};  // what inw_segment reads of a frame: the bounce limit, 1 / spp, the child order, no MULTIFOCUS
    F.max_bounces = max_bounces;
    F.inv_spp = inv_spp;
    F.dir[0] = F.dir[1] = F.dir[2] = invert ? 1.0f : -1.0f;  // invert = dot(dir, (1, 1, 1)) > 0
    F.n_focus = 0;
    Ctr c;
    FStack K{lds + threadIdx.x, 0};
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t next = 0, end = 0;  // the wave's claimed range not handed out yet (wave-uniform)
    bool drained = false;        // the queue is empty (wave-uniform)
    bool busy = false;
    uint32_t q = 0, dfs_high = S.dfs_high;
    uint32_t seg0 = 0, drops0 = 0, nans0 = 0;
    int s = 0;
    f3 col = f3{0, 0, 0};
    float dep = 0.0f;
    for (;;) {
        while (!drained) {  // hand queries to the free lanes
            const unsigned long long free = __ballot(!busy);
            if (free == 0) break;
            if (next >= end) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(queue, 64u * rounds);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base >= n_rays) { drained = true; break; }
                next = base;
                end = n_rays - base < 64u * rounds ? n_rays : base + 64u * rounds;  // < 2^32: n_rays <= 2^31
            }
            const uint32_t avail = end - next, want = (uint32_t)__popcll(free);
            const uint32_t rank = (uint32_t)__popcll(free & below);
            if (!busy && rank < avail) {
                q = next + rank;
                const float4 r0 = rays[2 * (size_t)q], r1 = rays[2 * (size_t)q + 1];
                const uint32_t sample = __float_as_uint(r0.w);
                if (sample >= spp) {  // no path: status 1, the lane stays free
                    out[2 * (size_t)q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    out[2 * (size_t)q + 1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(1u));
                } else {
                    const f3 o = mk(r0.x, r0.y, r0.z), d = mk(r1.x, r1.y, r1.z);
                    dfs_high = S.dfs_high;
                    if (!(fabsf(o.x) <= 1000.0f && fabsf(o.y) <= 1000.0f && fabsf(o.z) <= 1000.0f))
                        dfs_high = (uint32_t)kFStack + 1u;
                    s = (int)sample;
                    K.reset(0);
                    K.push_ray(o, d, 1.0f, 0.0f, c);
                    col = f3{0, 0, 0};
                    dep = 0.0f;
                    seg0 = c.seg; drops0 = c.drops; nans0 = c.nans;
                    busy = true;
                }
            }
            next += want < avail ? want : avail;
        }
        if (__ballot(busy) == 0) break;  // only once the queue is empty
        if (!busy) continue;
        InwScene Sq = S;
        Sq.dfs_high = dfs_high;
        inw_segment<LIGHTS, false, FU>(Sq, F, K, s, col, dep, c);
        if (K.size == 0) {  // the path is done
            out[2 * (size_t)q] = make_float4(col.x, col.y, col.z, dep);
            out[2 * (size_t)q + 1] = make_float4(__uint_as_float(c.seg - seg0), __uint_as_float(c.drops - drops0),
                                                 __uint_as_float(c.nans - nans0), __uint_as_float(0u));
            busy = false;
        }
    }
    if (!counters) return;
    const unsigned long long v[6] = {c.seg, c.nodes, c.prims, c.shadow, c.drops, c.nans};
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const unsigned long long t = wave_sum(v[i]);
        if (lane == 0 && t) atomicAdd(counters + i, t);
    }
}

namespace {
int g_max_blocks = 0;  // rt_debug_paths_max_blocks: 0 = the resident grid

template <bool LIGHTS, bool FU>
int paths_blocks() {  // resident blocks per CU, asked once
    static const int nb = occupancy_of(k_inw_paths<LIGHTS, FU>, kBlock);
    return nb;
}
template <bool LIGHTS, bool FU>
hipError_t paths_info(int info[4]) {
    return kernel_info(k_inw_paths<LIGHTS, FU>, paths_blocks<LIGHTS, FU>(), info);
}
}  // namespace

int inw_paths_blocks_per_cu(bool lights, bool fused) {
    return lights ? (fused ? paths_blocks<true, true>() : paths_blocks<true, false>())
                  : (fused ? paths_blocks<false, true>() : paths_blocks<false, false>());
}

hipError_t inw_paths_kernel_info(bool lights, bool fused, int info[4]) {
    return lights ? (fused ? paths_info<true, true>(info) : paths_info<true, false>(info))
                  : (fused ? paths_info<false, true>(info) : paths_info<false, false>(info));
}

int inw_paths_max_blocks(int blocks) {
    const int prev = g_max_blocks;
    g_max_blocks = blocks > 0 ? blocks : 0;
    return prev;
}

hipError_t launch_inw_paths(const InwScene &sc, const float4 *rays, uint32_t n_rays, int spp, int max_bounces,
                            bool invert, float4 *out, unsigned long long *counters, unsigned *queue, int cus,
                            hipStream_t s) {
    const hipError_t e = hipMemsetAsync(queue, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const bool lights = sc.layout == 4, fu = sc.fused != 0;
    const ClaimGrid cg = claim_grid(n_rays, cus, inw_paths_blocks_per_cu(lights, fu), g_max_blocks);
    const dim3 g(cg.grid), b(kBlock);
    const float inv_spp = 1.0f / (float)spp;  // as make_frame forms it
    const uint32_t inv = invert ? 1u : 0u;
    if (lights) {
        if (fu) hipLaunchKernelGGL((k_inw_paths<true, true>), g, b, 0, s, sc, rays, n_rays, (uint32_t)spp, max_bounces, inv_spp, inv, out, counters, queue, cg.rounds);
        else hipLaunchKernelGGL((k_inw_paths<true, false>), g, b, 0, s, sc, rays, n_rays, (uint32_t)spp, max_bounces, inv_spp, inv, out, counters, queue, cg.rounds);
    } else {
        if (fu) hipLaunchKernelGGL((k_inw_paths<false, true>), g, b, 0, s, sc, rays, n_rays, (uint32_t)spp, max_bounces, inv_spp, inv, out, counters, queue, cg.rounds);
        else hipLaunchKernelGGL((k_inw_paths<false, false>), g, b, 0, s, sc, rays, n_rays, (uint32_t)spp, max_bounces, inv_spp, inv, out, counters, queue, cg.rounds);
    }
    return hipGetLastError();
}

}  // namespace rtk
