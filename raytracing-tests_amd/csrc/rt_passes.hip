// rt_passes.hip -- progressive sample passes on a device scene (rt_render_pass_async).
//
// A pass renders samples [s0, s1) of every pixel of the frame's rectangle and leaves each pixel's
// fold state behind, so that the next pass continues where this one stopped and the last one holds
// the frame rt_render_image_async writes, bit for bit.  The folds are sequential float sums in
// sample order (INW: End(), 01_BoundingVolumeHierarchy/computeShaderSrc.glsl:625-675; IOW-03:
// out_Pixel, 03_Shadows_and_Materials/computeShaderSrc.glsl:383-417), so cutting the sample loop
// anywhere changes no bit; an IOW-03 sample also inherits the RI fields of the four ray-stack slots
// (the state rt_path_iow_rays_async hands from query to query).
//
// IOW-03: k_iow_pass is the path-query kernel (rt_path_iow.hip) with the camera ray and the fold moved
// inside: a persistent grid, a lane owns one pixel at a time, a wave claims 64 * rounds consecutive
// units with one atomic and hands them to its free lanes by ballot and mbcnt.
// INW: the first form, a fused kernel of the same mould (k_inw_pass: a lane owned a pixel for the whole
// pass and ran its samples one after the other), took twice the time of the composition below on the
// C3 frame (DESIGN.md 5.13 has both numbers).  So an INW pass is three launches per chunk of samples:
// k_pass_rays writes the render's own camera rays of (unit, sample) as path queries, unit-major, into
// the scene's pass workspace; the unchanged path kernel (k_inw_paths) answers them, every sample on a
// lane of its own; k_pass_fold folds a pixel's answers into its state in sample order and writes the
// image.
// Units map to pixels by unit_pixel: 8x8 blocks of the rectangle.
#include "rt_render_common.hpp"
#include "rt_pass_common.hpp"
#include "rt_inw_shade.hpp"
#include "rt_iow_shade.hpp"

namespace rtk {

// Waves per SIMD, the IOW-03 path kernel's (kPathIowWaves): bound by LDS, 2 blocks per CU with the
// nodes staged, 3 without.  DESIGN.md 5.13 has the table.
template <bool LN> constexpr int kPassIowWaves = LN ? 2 : 3;

// One lane per record: record u * ns + j (rt_path_ray: origin, sample | direction, pad) is the camera
// ray of sample s0 + j of unit u's pixel, by the render's own sample start; a unit past the rectangle's
// edge gets sample = 0xffffffff, which the path kernel answers without a path.  n = units * ns <= 2^31.
__global__ __launch_bounds__(kBlock)
void k_pass_rays(Frame Fin, InwScene S, uint32_t s0, uint32_t ns, uint32_t n, float4 *__restrict__ rays) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= n) return;
    Frame F{};
    pass_frame(F, Fin);
    const uint32_t u = i / ns, j = i - u * ns;
    const UnitPix p = unit_pixel(F, u);
    float4 *r = rays + 2 * (size_t)i;
    if (p.in_image) {
        PassRay K;
        Ctr c;
        inw_start_sample(S, F, K, p.x, p.y, (int)(s0 + j), c);
        r[0] = make_float4(K.o.x, K.o.y, K.o.z, __uint_as_float(s0 + j));
        r[1] = make_float4(K.d.x, K.d.y, K.d.z, 0.0f);
    } else {
        r[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
        r[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// One lane per unit: End() over the unit's ns answers (rt_path_out: rgb, depth | ...) in sample order,
// from the pixel's state (not read when s0 == 0: the first sample is assigned) -- sqrt(colour) added,
// the depth of sample spp / 2 -- and the state back: the first float4 of the pixel's rt_pass_state.
// k > 0: the chunk is the pass's last, and the image acc * RN(1 / k) and the depth are written.
__global__ __launch_bounds__(kBlock)
void k_pass_fold(Frame Fin, uint32_t s0, uint32_t ns, uint32_t k, uint32_t n_units, const float4 *__restrict__ out,
                 float4 *__restrict__ state) {
    const uint32_t u = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (u >= n_units) return;
    Frame F{};
    pass_frame(F, Fin);
    const UnitPix p = unit_pixel(F, u);
    if (!p.in_image) return;
    const uint32_t mid = (uint32_t)F.spp / 2u;
    f3 acc = f3{0, 0, 0};
    float dmid = 0.0f;
    if (s0 != 0) {
        const float4 a = state[2 * p.out];
        acc = f3{a.x, a.y, a.z};
        dmid = a.w;
    }
    const float4 *a = out + 2 * (size_t)u * ns;
    for (uint32_t j = 0; j < ns; j++) {
        const float4 r = a[2 * (size_t)j];
        const f3 g = f3{__builtin_sqrtf(r.x), __builtin_sqrtf(r.y), __builtin_sqrtf(r.z)};
        acc = sel(s0 + j == 0, g, acc + g);
        if (s0 + j == mid) dmid = r.w;
    }
    state[2 * p.out] = make_float4(acc.x, acc.y, acc.z, dmid);
    if (k == 0) return;
    if (F.out_rgba) {
        const f3 v = acc * rcp((float)k);
        reinterpret_cast<float4 *>(F.out_rgba)[p.out] = make_float4(v.x, v.y, v.z, 1.0f);
    }
    if (F.out_depth) F.out_depth[p.out] = dmid;
}

// s1 <= the scene's s_stop (the ring schedule's early return).  s0 >= s1 (a pass that begins at or
// past the early return) renders nothing: the state stays and the image is written from it.
template <bool LN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kPassIowWaves<LN>)))
void k_iow_pass(Frame Fin, IowScene S, uint32_t s0, uint32_t s1, float4 *__restrict__ state, unsigned *queue,
                uint32_t rounds, uint32_t n_units) {
    Frame F{}, Fs{};
    pass_frame(F, Fin);
    pass_seg_frame(Fs, Fin);
    using Cfg = IowCfg<false, 1, LN>;
    using Stack = IowStack<false>;
    __shared__ float lds[kIowStack * Stack::kSlot * kBlock];
    __shared__ short lds_bvh[Cfg::BS * kBlock];
    __shared__ float4 s_nodes[LN ? kIowLdsNodes * 7 : 1];
    short *bstk = lds_bvh + threadIdx.x;  // bslot's layout
    const float4 *nodes = iow_stage_nodes<LN>(S, s_nodes);
    Ctr c;
    Stack K{lds + threadIdx.x, nullptr, 0};
    const uint32_t lane = threadIdx.x & 63u;
    // out_Pixel's per-frame scalars (03...glsl:370-380); the per-pixel ones are kept per lane
    const int grid = iow_ring_grid(F.spp);
    const float aspect = iow_aspect(F.W, F.H);
    const float dsx = iow_px_dsx(aspect, F.W, grid), dsy = iow_px_dsy(F.H, grid);
    const float inv_k = rcp((float)s1);
    uint32_t next = 0, end = 0;  // the wave's claimed range not handed out yet (wave-uniform)
    bool drained = false;        // the queue is empty (wave-uniform)
    bool busy = false;           // the lane owns a pixel: samples [s, s1) are left
    bool walking = false;        // ... and sample s's path is under way
    uint32_t s = 0, out = 0;     // out = y * W + x < 2^31
    int skip = 0;
    float sx = 0.0f, sy = 0.0f;
    f3 fc = f3{0, 0, 0}, col = f3{0, 0, 0};
    for (;;) {
        while (!drained) {  // hand pixels to the free lanes
            const unsigned long long free = __ballot(!busy);
            if (free == 0) break;
            if (next >= end) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(queue, 64u * rounds);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base >= n_units) { drained = true; break; }
                next = base;
                end = n_units - base < 64u * rounds ? n_units : base + 64u * rounds;  // n_units < 2^31
            }
            const uint32_t avail = end - next, want = (uint32_t)__popcll(free);
            const uint32_t rank = lanes_below(free);
            if (!busy && rank < avail) {
                const UnitPix p = unit_pixel(F, next + rank);
                if (p.in_image) {  // a unit past the rectangle's edge: the lane stays free
                    out = (uint32_t)p.out;
                    s = s0;
                    fc = f3{0, 0, 0};
                    if (s0 == 0) {
                        for (int e = 0; e < kIowStack; e++) K.at(e, 7) = 0.0f;  // stale RI slots start at 0
                    } else {
                        const float4 a = state[2 * (size_t)out], r = state[2 * (size_t)out + 1];
                        fc = f3{a.x, a.y, a.z};
                        K.at(0, 7) = r.x; K.at(1, 7) = r.y; K.at(2, 7) = r.z; K.at(3, 7) = r.w;
                    }
                    if (s0 < s1) {
                        sx = iow_px_sx(aspect, p.x, F.W);
                        sy = iow_px_sy(p.y, F.H);
                        busy = true;
                    } else {  // nothing left to render: the image from the state as it is
                        if (F.out_rgba) {
                            const f3 v = fc * inv_k;
                            reinterpret_cast<float4 *>(F.out_rgba)[out] = make_float4(v.x, v.y, v.z, 1.0f);
                        }
                        if (F.out_depth) F.out_depth[out] = 0.0f;
                    }
                }
            }
            next += want < avail ? want : avail;
        }
        if (busy && !walking) {  // start sample s
            f3 ro, rd;
            iow_camera_ray(S, F, sx, sy, dsx, dsy, (int)s, ro, rd);
            K.size = 0;
            K.wmask = K.rmask = 0u;
            skip = 0;
            col = f3{0, 0, 0};
            K.push(ro, rd, 1.0f, 1.0f, 0, c);
            walking = true;
        }
        if (__ballot(busy) == 0) {
            if (drained) break;
            continue;
        }
        if (walking) {
            iow_segment<false, Cfg::BS, Cfg::NS>(S, Fs, K, skip, col, (int)s, c, bstk, nodes);
            if (K.size == 0) {  // sample done: out_Pixel's sum
                fc = fc + col;
                s++;
                walking = false;
                if (s >= s1) {
                    state[2 * (size_t)out] = make_float4(fc.x, fc.y, fc.z, 0.0f);
                    state[2 * (size_t)out + 1] = make_float4(K.at(0, 7), K.at(1, 7), K.at(2, 7), K.at(3, 7));
                    if (F.out_rgba) {
                        const f3 v = fc * inv_k;
                        reinterpret_cast<float4 *>(F.out_rgba)[out] = make_float4(v.x, v.y, v.z, 1.0f);
                    }
                    if (F.out_depth) F.out_depth[out] = 0.0f;
                    busy = false;
                }
            }
        }
    }
    flush(F, c);
}

constexpr uint32_t kPassRounds = 16;  // units per claim: at most 16 x 64 (the rule of launch_inw_paths)

namespace {
int g_max_blocks = 0;  // rt_debug_pass_max_blocks: 0 = the resident grid

template <class Kn>
int pass_blocks(Kn kernel) {
    return occupancy_of(kernel, kBlock);
}
template <class Kn>
hipError_t pass_info(Kn kernel, int info[4]) {
    hipFuncAttributes a;
    const hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(kernel));
    if (e != hipSuccess) return e;
    info[0] = a.numRegs;
    info[1] = (int)a.localSizeBytes;
    info[2] = (int)a.sharedSizeBytes;
    info[3] = pass_blocks(kernel);
    return hipSuccess;
}
// resident blocks per CU of the instance a scene runs, asked once each
int iow_pass_blocks(bool ln) {
    static const int nb[2] = {pass_blocks(k_iow_pass<false>), pass_blocks(k_iow_pass<true>)};
    return nb[ln ? 1 : 0];
}
// the grid and the claim size: every wave of the grid gets at least four claims (launch_inw_paths' rule)
void pass_grid(uint32_t n_units, int cus, int per_cu, dim3 &g, uint32_t &rounds) {
    const uint32_t need = (n_units + (uint32_t)kBlock - 1u) / (uint32_t)kBlock;
    uint32_t cap = (uint32_t)(cus > 0 ? cus : 1) * (uint32_t)per_cu;
    if (g_max_blocks > 0 && (uint32_t)g_max_blocks < cap) cap = (uint32_t)g_max_blocks;
    g = dim3(need < cap ? need : cap);
    const uint32_t per_wave = n_units / (64u * g.x * (uint32_t)(kBlock / 64) * 4u);
    rounds = per_wave < 1u ? 1u : (per_wave > kPassRounds ? kPassRounds : per_wave);
}
}  // namespace

hipError_t pass_kernel_info(int which, int info[4]) {
    switch (which) {
        case 0: return pass_info(k_pass_rays, info);
        case 1: return pass_info(k_pass_fold, info);
        case 2: return pass_info(k_iow_pass<true>, info);
        case 3: return pass_info(k_iow_pass<false>, info);
    }
    return hipErrorInvalidValue;
}

int pass_max_blocks_now() { return g_max_blocks; }

int pass_max_blocks(int blocks) {
    const int prev = g_max_blocks;
    g_max_blocks = blocks > 0 ? blocks : 0;
    return prev;
}

hipError_t launch_pass_rays(const Frame &f, const InwScene &sc, uint32_t s0, uint32_t ns, float4 *rays,
                            hipStream_t s) {
    const uint32_t n = units_of(f) * ns;  // <= 2^31 (the caller's chunks)
    const dim3 g((n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock), b(kBlock);
    hipLaunchKernelGGL(k_pass_rays, g, b, 0, s, f, sc, s0, ns, n, rays);
    return hipGetLastError();
}

hipError_t launch_pass_fold(const Frame &f, uint32_t s0, uint32_t ns, uint32_t k, const float4 *out, float4 *state,
                            hipStream_t s) {
    const uint32_t n_units = units_of(f);
    const dim3 g((n_units + (uint32_t)kBlock - 1u) / (uint32_t)kBlock), b(kBlock);
    hipLaunchKernelGGL(k_pass_fold, g, b, 0, s, f, s0, ns, k, n_units, out, state);
    return hipGetLastError();
}

hipError_t launch_iow_pass(const Frame &f, const IowScene &sc, uint32_t s0, uint32_t s1, float4 *state,
                           unsigned *queue, int cus, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(queue, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const bool ln = iow_lds(sc);
    const uint32_t n_units = units_of(f);
    dim3 g;
    uint32_t rounds;
    pass_grid(n_units, cus, iow_pass_blocks(ln), g, rounds);
    const dim3 b(kBlock);
    if (ln) hipLaunchKernelGGL((k_iow_pass<true>), g, b, 0, s, f, sc, s0, s1, state, queue, rounds, n_units);
    else hipLaunchKernelGGL((k_iow_pass<false>), g, b, 0, s, f, sc, s0, s1, state, queue, rounds, n_units);
    return hipGetLastError();
}

}  // namespace rtk
