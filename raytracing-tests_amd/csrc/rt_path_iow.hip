// rt_path_iow.hip -- batched path (radiance) queries on an IOW-03 device scene (rt_path_iow_rays_async).
//
// One query is one invocation of the reference shader's LaunchRays (03_Shadows_and_Materials/
// computeShaderSrc.glsl:285-358) for the caller's ray: an empty 4-entry ray stack whose RI fields hold
// the state the caller passes in, push(o, d, 1, 1, 0), then the render kernels' own segment body
// (iow_segment, rt_iow_shade.hpp) until the stack is empty.  The RI fields go back to the caller, and
// the queries of a chain hand them to each other, so a pixel is the fold of one chain: no pixels, no
// camera, no speculation records, no wave-cooperative search.
#include "rt_iow_shade.hpp"

namespace rtk {

// Waves per SIMD = resident 256-lane blocks per CU.  LDS decides: the LN instance holds 36,864 B of ray
// stacks, 8,192 B of link stacks and 26,880 B of staged nodes (71,936 B: 2 blocks in a CU's 160 KB),
// the other one 36,864 + 16,384 B (3 blocks).  Neither uses scratch at these.
template <bool LN> constexpr int kPathIowWaves = LN ? 2 : 3;

// A query is 3 float4 (rt_path_iow_ray: origin, sample | direction, pad | ri_in), an answer 3 float4
// (rt_path_iow_out: rgb, stale | segments, drops, nans, status | ri_out).
// The work unit is a chain: queries [k * chain, (k + 1) * chain) run in order on one lane, on that
// lane's column of the LDS ray stacks, so each finds the RI fields as its predecessor left them -- what
// a pixel's samples do in the renders.  The grid is persistent and so is every lane: a wave claims
// 64 * rounds consecutive chains from `queue` with one atomic and hands them to its free lanes by
// ballot and popcount (k_inw_paths' scheme: no atomic per lane or per query), and no wave retires
// while the queue holds chains.  Each trip of the wave's loop starts the next query of every lane
// that owns a chain but has no path, then runs one segment of every path.
// Lanes without a path -- free lanes, the ragged tail, lanes answering a sample >= spp query -- sit
// outside the segment's branch, so the __all / __ballot votes of iow_launch_ray count walking lanes
// only.
// LN: the scene's 4-wide BVH is staged in LDS as k_iow_trace stages it (7 float4 per node, 16 link
// slots per lane); else nodes come from global memory (8 float4, 32 slots), or S.nodes == null runs
// the linear loop.
template <bool LN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kPathIowWaves<LN>)))
void k_iow_paths(IowScene S, int leaf_batch, int max_bounces, const float4 *__restrict__ rays, uint32_t n_rays,
                 uint32_t chain, uint32_t n_chains, uint32_t spp, float4 *__restrict__ out,
                 unsigned long long *counters, unsigned *queue, uint32_t rounds) {
    using Cfg = IowCfg<false, 1, LN>;
    using Stack = IowStack<false>;
    __shared__ float lds[kIowStack * Stack::kSlot * kBlock];
    __shared__ short lds_bvh[Cfg::BS * kBlock];
    __shared__ float4 s_nodes[LN ? kIowLdsNodes * 7 : 1];
    short *bstk = lds_bvh + threadIdx.x;  // bslot's layout
    const float4 *nodes = iow_stage_nodes<LN>(S, s_nodes);
    Frame F{};  // what iow_segment reads of a frame: the bounce limit and the leaf batch; no diagnostics
    F.max_bounces = max_bounces;
    F.leaf_batch = leaf_batch;
    Ctr c;
    Stack K{lds + threadIdx.x, nullptr, 0};
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t next = 0, end = 0;  // the wave's claimed chains not handed out yet (wave-uniform)
    bool drained = false;        // the queue is empty (wave-uniform)
    bool busy = false;           // the lane owns a chain: queries [q, qend) are unanswered
    bool walking = false;        // ... and query q's path is under way
    bool fresh = false;          // ... and q is the chain's first query
    uint32_t q = 0, qend = 0;
    uint32_t seg0 = 0, drops0 = 0, nans0 = 0;
    int sidx = 0, skip = 0;
    f3 col = f3{0, 0, 0};
    for (;;) {
        while (!drained) {  // hand chains to the free lanes
            const unsigned long long free = __ballot(!busy);
            if (free == 0) break;
            if (next >= end) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(queue, 64u * rounds);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base >= n_chains) { drained = true; break; }
                next = base;
                end = n_chains - base < 64u * rounds ? n_chains : base + 64u * rounds;  // < 2^32: n_chains <= 2^31
            }
            const uint32_t avail = end - next, want = (uint32_t)__popcll(free);
            const uint32_t rank = (uint32_t)__popcll(free & below);
            if (!busy && rank < avail) {
                q = (next + rank) * chain;  // < n_rays <= 2^31
                qend = n_rays - q < chain ? n_rays : q + chain;
                busy = true;
                fresh = true;
            }
            next += want < avail ? want : avail;
        }
        if (busy && !walking) {  // the chain's next query
            const float4 r0 = rays[3 * (size_t)q], r1 = rays[3 * (size_t)q + 1];
            if (fresh) {  // the chain's incoming state; later queries find their predecessor's
                const float4 r2 = rays[3 * (size_t)q + 2];
                K.at(0, 7) = r2.x; K.at(1, 7) = r2.y; K.at(2, 7) = r2.z; K.at(3, 7) = r2.w;
                fresh = false;
            }
            const uint32_t sample = __float_as_uint(r0.w);
            if (sample >= spp) {  // no path: status 1, the state passes through
                out[3 * (size_t)q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                out[3 * (size_t)q + 1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(1u));
                out[3 * (size_t)q + 2] = make_float4(K.at(0, 7), K.at(1, 7), K.at(2, 7), K.at(3, 7));
                q++;
                busy = q < qend;
            } else {
                K.size = 0;
                K.wmask = K.rmask = 0u;
                skip = 0;
                sidx = (int)sample;
                col = f3{0, 0, 0};
                seg0 = c.seg; drops0 = c.drops; nans0 = c.nans;
                K.push(mk(r0.x, r0.y, r0.z), mk(r1.x, r1.y, r1.z), 1.0f, 1.0f, 0, c);
                walking = true;
            }
        }
        if (__ballot(busy) == 0) {
            if (drained) break;
            continue;
        }
        if (walking) {
            iow_segment<false, Cfg::BS, Cfg::NS>(S, F, K, skip, col, sidx, c, bstk, nodes);
            if (K.size == 0) {  // the path is done
                out[3 * (size_t)q] = make_float4(col.x, col.y, col.z, __uint_as_float(K.rmask));
                out[3 * (size_t)q + 1] = make_float4(__uint_as_float(c.seg - seg0), __uint_as_float(c.drops - drops0),
                                                     __uint_as_float(c.nans - nans0), __uint_as_float(0u));
                out[3 * (size_t)q + 2] = make_float4(K.at(0, 7), K.at(1, 7), K.at(2, 7), K.at(3, 7));
                walking = false;
                q++;
                busy = q < qend;
            }
        }
    }
    if (!counters) return;
    const unsigned long long v[6] = {c.seg, c.nodes, c.prims, 0ull, c.drops, c.nans};
#pragma unroll
    for (int i = 0; i < 6; i++) {
        if (i == 3) continue;  // no shadow queries in IOW-03
        const unsigned long long t = wave_sum(v[i]);
        if (lane == 0 && t) atomicAdd(counters + i, t);
    }
}

namespace {
int g_max_blocks = 0;  // rt_debug_path_iow_max_blocks: 0 = the resident grid

template <bool LN>
int path_iow_blocks() {  // resident blocks per CU, asked once
    static const int nb = occupancy_of(k_iow_paths<LN>, kBlock);
    return nb;
}
template <bool LN>
hipError_t path_iow_info(int info[4]) {
    return kernel_info(k_iow_paths<LN>, path_iow_blocks<LN>(), info);
}
}  // namespace

int iow_paths_blocks_per_cu(bool ln) { return ln ? path_iow_blocks<true>() : path_iow_blocks<false>(); }

hipError_t iow_paths_kernel_info(bool ln, int info[4]) {
    return ln ? path_iow_info<true>(info) : path_iow_info<false>(info);
}

int iow_paths_max_blocks(int blocks) {
    const int prev = g_max_blocks;
    g_max_blocks = blocks > 0 ? blocks : 0;
    return prev;
}

hipError_t launch_iow_paths(const IowScene &sc, int leaf_batch, int max_bounces, const float4 *rays, uint32_t n_rays,
                            uint32_t chain, int spp, float4 *out, unsigned long long *counters, unsigned *queue,
                            int cus, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(queue, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const bool ln = iow_lds(sc);
    const uint32_t n_chains = n_rays / chain + (n_rays % chain ? 1u : 0u);  // the last chain may be short
    const ClaimGrid cg = claim_grid(n_chains, cus, iow_paths_blocks_per_cu(ln), g_max_blocks);
    const dim3 g(cg.grid), b(kBlock);
    if (ln) hipLaunchKernelGGL((k_iow_paths<true>), g, b, 0, s, sc, leaf_batch, max_bounces, rays, n_rays, chain, n_chains, (uint32_t)spp, out, counters, queue, cg.rounds);
    else hipLaunchKernelGGL((k_iow_paths<false>), g, b, 0, s, sc, leaf_batch, max_bounces, rays, n_rays, chain, n_chains, (uint32_t)spp, out, counters, queue, cg.rounds);
    return hipGetLastError();
}

}  // namespace rtk
