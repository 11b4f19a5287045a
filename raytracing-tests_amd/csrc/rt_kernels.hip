// rt_kernels.hip -- the render hot path for gfx950 (CDNA4, wave64).
//
// One thread renders one pixel and walks its samples in order, exactly like the
// reference's invocation (IOW) or workgroup (INW) does, so the per-pixel reduction order
// is the reference's sequential one.  A 256-thread block covers a 16x16 pixel tile with
// each wave on an 8x8 quadrant (coherent camera rays).  Per-thread ray / node stacks live
// in LDS in a [slot][thread] layout: lane l of a wave touches bank (l mod 32) whatever the
// stack depth, so divergent stack pointers never conflict.
//
// Kernels and the shaders they replace (paths relative to /root/reference/Raytracing-Sandbox/Src/):
//   k_iow01 <- In-One-Weekend/01_Adding_Sphere/computeShaderSrc.glsl:98-146
//   k_iow03 <- In-One-Weekend/03_Shadows_and_Materials/computeShaderSrc.glsl:196-430
//   k_inw   <- In-Next-Week/01_BoundingVolumeHierarchy/computeShaderSrc.glsl:230-675 (LIGHTS=false)
//              In-Next-Week/04_Lights_Camera_And_Action/computeShaderSrc.glsl:243-773 (LIGHTS=true)
#include <cstdlib>
#include <type_traits>

#include "rt_kernels.hpp"
#include "rt_math.hpp"
#include "rt_inw_walk.hpp"
#include "rt_iow_walk.hpp"
#include "rt_iow_shade.hpp"
#include "rt_inw_shade.hpp"

namespace rtk {


// ----------------------------------------------------------------------- pixel mapping
struct Pix { int x, y; bool in_image; size_t out; bool valid; };

__device__ __forceinline__ Pix map_pixel(const Frame &f) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lx = ((wave & 1) << 3) | (lane & 7), ly = ((wave >> 1) << 3) | (lane >> 3);
    Pix p;
    if (f.tiles == nullptr) {
        const int nbx = (f.tw + 15) >> 4;
        const int bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
        const int rx = bx * 16 + lx, ry = by * 16 + ly;
        p.x = f.x0 + rx; p.y = f.y0 + ry;
        p.valid = rx < f.tw && ry < f.th && p.x >= 0 && p.y >= 0 && p.x < f.W && p.y < f.H;
        p.in_image = p.valid;
        p.out = (size_t)p.y * f.W + p.x;
    } else {
        const int per = f.tile_size >> 4, sub = per * per;
        const int tile = blockIdx.x / sub, s = blockIdx.x % sub;
        const int ix = (s % per) * 16 + lx, iy = (s / per) * 16 + ly;
        p.x = f.tiles[2 * tile] * f.tile_size + ix;
        p.y = f.tiles[2 * tile + 1] * f.tile_size + iy;
        p.in_image = p.x < f.W && p.y < f.H;
        p.valid = true;  // packed slots outside the image are written as zero
        p.out = (size_t)tile * f.tile_size * f.tile_size + (size_t)iy * f.tile_size + ix;
    }
    return p;
}

// Finer phase split of the wave-cooperative segment (diagnostic builds only, -DRT_DIAG_SPLIT):
// reuses tally slots that stay zero in that mode (see tools/latency_probe.py).
#ifdef RT_DIAG_SPLIT
#define SPL_T0(t) const unsigned long long t = (unsigned long long)clock64()
#define SPL_CYC(w, slot, t)                                                           \
    do {                                                                              \
        if (w) {                                                                      \
            const unsigned long long d_ = (unsigned long long)clock64() - (t);        \
            if (first_active_lane()) (w)[slot] += d_;                                 \
        }                                                                             \
    } while (0)
#else
#define SPL_T0(t) ((void)0)
#define SPL_CYC(w, slot, t) ((void)0)
#endif

__device__ __forceinline__ void flush(const Frame &f, const Ctr &c) {
    if (c.wdbg && (threadIdx.x & 63) == 0)
        for (int i = 0; i < kDbgSlots; i++) atomicAdd(f.dbg + i, c.wdbg[i]);
    if (!f.counters) return;
    unsigned long long v[6] = {c.seg, c.nodes, c.prims, c.shadow, c.drops, c.nans};
#pragma unroll
    for (int i = 0; i < 6; i++) {
        unsigned long long s = wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(f.counters + i, s);
    }
    if (f.walk_ctr) {
        const unsigned long long s = wave_sum((unsigned long long)c.refw);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(f.walk_ctr, s);
    }
}

// ============================================================================ IOW-01
__global__ __launch_bounds__(kBlock) void k_iow01(Frame f) {
    Pix px = map_pixel(f);
    if (!px.valid) return;  // no cross-lane work in this kernel
    f3 color = f3{0, 0, 0};
    if (px.in_image) {
        const f3 D = mk(f.dir[0], f.dir[1], f.dir[2]), P = mk(f.pos[0], f.pos[1], f.pos[2]);
        const f3 C = mk(f.sphere[0], f.sphere[1], f.sphere[2]);
        const float R = f.sphere[3];
        float aspect = (float)f.W * rcp((float)f.H);
        f3 cr = cross(D, f3{0, 1, 0}), cu = cross(cr, D);
        float sx = ((float)px.x * 2.0f - (float)f.W) * rcp(2.0f * (float)f.W);
        sx *= aspect;
        float sy = ((float)px.y * 2.0f - (float)f.H) * rcp(2.0f * (float)f.H);
        f3 pis = ((P + D * f.focus) + cr * sx) + cu * sy;
        // CreatePlane((0,-2,0),(0,-2,1),(1,-2,0))
        const f3 p1 = f3{0, -2, 0};
        f3 pn = normalize(cross(f3{0, -2, 1} - p1, f3{1, -2, 0} - p1));
        float pw = -(pn.x * p1.x + pn.y * p1.y + pn.z * p1.z);
        f3 ro = P, rd = normalize(pis - P);
        color = background(rd, false);
        float min_depth = 10000.0f;
        float t = -(pn.x * ro.x + pn.y * ro.y + pn.z * ro.z + pw) * rcp(pn.x * rd.x + pn.y * rd.y + pn.z * rd.z);
        if (min_depth > t && t > 0.0f) { color = f3{0.8f, 0.1f, 0.7f}; min_depth = t; }
        f3 rs = ro - C;
        float hb = dot(rd, rs), a = dot(rd, rd), c = dot(rs, rs) - R * R;
        float det = hb * hb - a * c;
        t = (det > 0.0f && hb < 0.0f) ? ((-hb - __builtin_sqrtf(det)) * rcp(a)) : -1.0f;
        if (min_depth > t && t > 0.0f) {
            f3 ip = ro + rd * t;
            color = f.show_normal ? normalize(ip - C) : f3{1, 0, 0};
        }
    }
    reinterpret_cast<float4 *>(f.out_rgba)[px.out] = make_float4(color.x, color.y, color.z, px.in_image ? 1.0f : 0.0f);
}

// ============================================================================ IOW-03
// (the object records, the closest-hit search and its evaluation: rt_iow_walk.hpp)

// ---------------------------------------------------------------- wave-cooperative closest hit
// When only a few lanes of a wave still trace (the long samples at the end of a pass), the
// wave runs their closest-hit queries one ray at a time with all 64 lanes: every lane culls
// 1/64 of the objects against their conservative boxes (the BVH's leaf boxes), the survivors
// are compacted into a wave list in LDS and tested exactly in parallel, and a wave reduction
// applies the reference's (t, lowest index) rule.  The candidate set is a superset of the one
// the BVH walk tests, so the winner and its t bits are the same (DESIGN.md "k_iow03s").
// Requires all 64 lanes active.
__device__ __forceinline__ float wave_min_all(float v) {
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false)));   // quad [1,0,3,2]
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false)));   // quad [2,3,0,1]
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false)));  // row half-mirror
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false)));  // row mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
__device__ __forceinline__ float bcast_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Closest hit of one (wave-uniform) ray with the whole wave.  wl: the wave's LDS list, entry k
// at lane k & 63's BVH-stack slot k >> 6 (bslot), cap entries (a multiple of 64 * kCoopR).  Returns the
// (uniform) winner and its cold record; nbox / nprim are the boxes and objects tested.  The
// loads of a batch of kCoopR boxes per lane, and a candidate's hot and cold records, are
// issued together: a lone ray's query costs about two memory latencies, not one per step.
constexpr int kCoopR = 8;
__device__ void iow_coop_search(const IowScene &S, f3 go, f3 gd, float max_t, short *wl, int cap, float &t_out,
                                int &j_out, float4 &c0_out, float4 &c1_out, uint32_t &nbox, uint32_t &nprim,
                                unsigned long long *wdbg = nullptr) {
    const int lane = (int)(threadIdx.x & 63);
    float bt = max_t;
    int bj = -1;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0;  // cold record of this lane's best
    nbox = 0; nprim = 0;
    t_out = max_t; j_out = -1; c0_out = b0; c1_out = b0;
    const float dl2 = dot(gd, gd);
    if (!(dl2 > 0.0f)) {  // zero / NaN direction: no object can hit (see iow_launch_ray)
        nprim = S.n;
        return;
    }
    f3 td_id, nd_id;
    iow_id_dirs(gd, td_id, nd_id);
    const bool cull = S.obox != nullptr && dl2 > 0.998f && dl2 < 1.002f;
    const f3 id = f3{__builtin_amdgcn_rcpf(gd.x), __builtin_amdgcn_rcpf(gd.y), __builtin_amdgcn_rcpf(gd.z)};
    const float lim = max_t * 1.0001f + 1e-3f;
    const uint32_t n = S.n;
    uint32_t j0 = 0;
    while (j0 < n) {
        uint32_t cnt = 0, jb = j0;
        SPL_T0(t_cull);
        if (cull) {
            for (; j0 < n && cnt + 64 * kCoopR <= (uint32_t)cap; j0 += 64 * kCoopR) {
                const float2 *ob2 = reinterpret_cast<const float2 *>(S.obox + n);
                float4 a[kCoopR];
                float2 b[kCoopR];
#pragma unroll
                for (int r = 0; r < kCoopR; r++) {
                    const uint32_t j = j0 + 64 * r + lane, jj = j < n ? j : n - 1;
                    a[r] = S.obox[jj];
                    b[r] = ob2[jj];
                }
#pragma unroll
                for (int r = 0; r < kCoopR; r++) {
                    const uint32_t j = j0 + 64 * r + lane;
                    const bool cand =
                        j < n && cull_t(a[r].x, a[r].y, a[r].z, a[r].w, b[r].x, b[r].y, go, id, lim) != kMiss;
                    const unsigned long long cm = __ballot(cand);
                    if (cand) {
                        const uint32_t k = cnt + lanes_below(cm);
                        bslot(wl + (k & 63), (int)(k >> 6)) = (short)j;
                    }
                    cnt += (uint32_t)__popcll(cm);
                }
            }
            nbox += (j0 < n ? j0 : n) - jb;
        } else {
            cnt = n - j0 < (uint32_t)cap ? n - j0 : (uint32_t)cap;
            j0 += cnt;
        }
        SPL_CYC(wdbg, kDbgTrav, t_cull);
        SPL_T0(t_exact);
        for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
            const uint32_t k = k0 + lane;
            if (k < cnt) {
                const int j = cull ? (int)bslot(wl + (k & 63), (int)(k >> 6)) : (int)(jb + k);
                const float4 *cold = reinterpret_cast<const float4 *>(S.cold + (size_t)j * kIowCold);
                const float4 q0 = cold[0], q1 = cold[1];
                const int was = bj;
                iow_test(S, j, go, gd, td_id, nd_id, bt, bj);
                if (bj != was) { b0 = q0; b1 = q1; }
            }
        }
        nprim += cnt;
        SPL_CYC(wdbg, kDbgTravLanes, t_exact);
    }
    SPL_T0(t_red);
    const float tm = wave_min_all(bj >= 0 ? bt : max_t);
    unsigned long long m = __ballot(bj >= 0 && bt == tm);
    if (m == 0) return;
    int jm = -1, lm = 0;
    for (; m; m &= m - 1) {  // usually one lane; exact ties keep the lowest object index
        const int l = __ffsll((long long)m) - 1;
        const int j = __builtin_amdgcn_readlane(bj, l);
        if (jm < 0 || j < jm) { jm = j; lm = l; }
    }
    t_out = tm;
    j_out = jm;
    c0_out = make_float4(bcast_f(b0.x, lm), bcast_f(b0.y, lm), bcast_f(b0.z, lm), bcast_f(b0.w, lm));
    c1_out = make_float4(bcast_f(b1.x, lm), bcast_f(b1.y, lm), bcast_f(b1.z, lm), bcast_f(b1.w, lm));
    SPL_CYC(wdbg, kDbgLeaf, t_red);
}

// The segment step of a work loop, called with every lane of the wave (seg: this lane has a
// ray to trace).  With at most F.coop_max tracing lanes the wave runs their closest-hit
// queries cooperatively (iow_coop_search), one ray after another; otherwise each lane walks
// the BVH for its own ray.
template <bool NARROW, int BS, int NS>
__device__ __forceinline__ void iow_seg_step(const IowScene &S, const Frame &F, IowStack<NARROW> &K, int &skip,
                                             f3 &sample, int sidx, Ctr &c, short *bstk, const float4 *nodes, bool seg) {
    const unsigned long long m = __ballot(seg);
    if (m == 0) return;
    if (__popcll(m) > F.coop_max) {
        if (seg) iow_segment<NARROW, BS, NS>(S, F, K, skip, sample, sidx, c, bstk, nodes);
        return;
    }
    constexpr int kCap = BS * 64;  // the wave's BVH-stack slots, as a list
    short *wl = bstk - (threadIdx.x & 63);
    DBG_T0(F, t_pop);
    SegIn in{};
    if (seg) in = iow_seg_pop(S, K, sidx);
    DBG_CYC(F, c, kDbgCycSpare2, t_pop);
    DBG_T0(F, t_q);
    float my_t = 32000.0f;
    int my_j = -1;
    float4 my_c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), my_c1 = my_c0;
    uint32_t my_box = 0, my_prim = 0;
    for (unsigned long long mm = m; mm; mm &= mm - 1) {
        const int L = __ffsll((long long)mm) - 1;
        const f3 go = f3{bcast_f(in.co.x, L), bcast_f(in.co.y, L), bcast_f(in.co.z, L)};
        const f3 gd = f3{bcast_f(in.cd.x, L), bcast_f(in.cd.y, L), bcast_f(in.cd.z, L)};
        float t;
        int j;
        float4 c0, c1;
        uint32_t nb, np;
        iow_coop_search(S, go, gd, 32000.0f, wl, kCap, t, j, c0, c1, nb, np, c.wdbg);
        if ((int)(threadIdx.x & 63) == L) { my_t = t; my_j = j; my_c0 = c0; my_c1 = c1; my_box = nb; my_prim = np; }
    }
    DBG_CYC(F, c, kDbgCycSpare0, t_q);
    DBG_T0(F, t_sh);
    if (seg) {
        c.seg++; c.nodes += my_box; c.prims += my_prim;
        SPL_T0(t_ev);
        f3 td_id, nd_id;
        iow_id_dirs(in.cd, td_id, nd_id);
        const RayRet data =
            iow_eval_c(S, in.co, in.cd, td_id, nd_id, my_t, my_j, 32000.0f, in.contribution, my_c0, my_c1);
        SPL_CYC(c.wdbg, kDbgCycRay, t_ev);
        SPL_T0(t_sd);
        iow_seg_shade(S, F, K, skip, sample, sidx, c, in, data);
        SPL_CYC(c.wdbg, kDbgCycTrav, t_sd);
    }
    DBG_CYC(F, c, kDbgCycSpare1, t_sh);
}

// ---------------------------------------------------------------- persistent work queue
// Work unit = one pixel.  A wave keeps all 64 lanes busy: a lane that finishes its pixel
// takes the next one with a wave-aggregated atomic (ballot -> popcount -> one atomicAdd ->
// per-lane rank by masked popcount), so divergent path lengths never idle the wave.
struct UnitPix { int x, y; bool in_image; size_t out; };

__device__ __forceinline__ UnitPix unit_pixel(const Frame &f, uint32_t u) {
    UnitPix p;
    const int l = (int)(u & 63u);
    if (f.tiles == nullptr) {
        const int b = (int)(u >> 6), nbx = (f.tw + 7) >> 3;
        const int rx = (b % nbx) * 8 + (l & 7), ry = (b / nbx) * 8 + (l >> 3);
        p.x = f.x0 + rx; p.y = f.y0 + ry;
        p.in_image = rx < f.tw && ry < f.th && p.x >= 0 && p.y >= 0 && p.x < f.W && p.y < f.H;
        p.out = p.in_image ? (size_t)p.y * f.W + p.x : (size_t)-1;
    } else {
        const uint32_t area = (uint32_t)f.tile_size * f.tile_size;
        const int t = (int)(u / area), r = (int)(u % area), per = f.tile_size >> 3;
        const int b = r >> 6;
        const int ix = (b % per) * 8 + (l & 7), iy = (b / per) * 8 + (l >> 3);
        p.x = f.tiles[2 * t] * f.tile_size + ix;
        p.y = f.tiles[2 * t + 1] * f.tile_size + iy;
        p.in_image = p.x < f.W && p.y < f.H;
        p.out = (size_t)t * area + (size_t)iy * f.tile_size + ix;
    }
    return p;
}

__device__ __forceinline__ uint32_t units_total(const Frame &f) {
    if (f.tiles) return (uint32_t)f.n_tiles * f.tile_size * f.tile_size;
    return (uint32_t)(((f.tw + 7) >> 3) * ((f.th + 7) >> 3)) * 64u;
}

// wave-aggregated fetch: lanes with `need` get consecutive unit ids
__device__ __forceinline__ uint32_t fetch_unit(unsigned *counter, bool need) {
    const unsigned long long mask = __ballot(need);
    if (mask == 0) return 0xffffffffu;
    const int lane = (int)(threadIdx.x & 63);
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(mask));
    base = __shfl(base, leader, 64);
    const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    return need ? base + rank : 0xffffffffu;
}

__device__ __forceinline__ void write_px(const Frame &f, const UnitPix &p, f3 c, float depth) {
    if (p.out == (size_t)-1) return;
    reinterpret_cast<float4 *>(f.out_rgba)[p.out] = make_float4(c.x, c.y, c.z, p.in_image ? 1.0f : 0.0f);
    if (f.out_depth) f.out_depth[p.out] = depth;
}

// wave-aggregated slot allocation for parking (same ballot / popcount / rank scheme)
__device__ __forceinline__ uint32_t park_slot(unsigned *count, bool need) {
    const unsigned long long mask = __ballot(need);
    const int lane = (int)(threadIdx.x & 63);
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned)__popcll(mask));
    base = __shfl(base, leader, 64);
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ float ibits(int v) { return __int_as_float(v); }
__device__ __forceinline__ float ubits(uint32_t v) { return __uint_as_float(v); }

template <bool NARROW, int SUB, bool LN>
__device__ __forceinline__ void iow03_body(const Frame &f, const IowScene &S, const Chunk &ch, const Cont &ct,
                                           unsigned *counter, int s_stop) {
    using Stack = IowStack<NARROW>;
    using Cfg = IowCfg<NARROW, SUB, LN>;
    constexpr int kFl = kIowStack * Stack::kSlot;  // stack floats per lane
    __shared__ float lds[SUB * kFl * kBlock];
    __shared__ unsigned char lds_b[NARROW ? SUB * kIowStack * kBlock : 1];
    __shared__ short lds_bvh[SUB * Cfg::BS * kBlock];
    __shared__ unsigned long long s_dbg[SUB * kBlock / 64][kDbgSlots];
    __shared__ float4 s_nodes[LN ? kIowLdsNodes * 7 : 1];
    const int sb = (int)(threadIdx.x / kBlock), tl = (int)(threadIdx.x % kBlock);
    short *bstk = lds_bvh + sb * Cfg::BS * kBlock + tl;  // bslot's layout
    const float4 *nodes = iow_stage_nodes<LN>(S, s_nodes);
    Ctr c;
    if (f.dbg) {
        c.wdbg = s_dbg[threadIdx.x >> 6];
        if ((threadIdx.x & 63) < kDbgSlots) c.wdbg[threadIdx.x & 63] = 0;
    }
    Stack K{lds + sb * kFl * kBlock + tl, lds_b + (NARROW ? sb * kIowStack * kBlock + tl : 0), 0};
    const uint32_t total = ct.in ? *ct.in_count : (ch.order_count ? *ch.order_count : units_total(f));
    const bool may_park = ct.out != nullptr && total >= ct.park_min;
    const int W = f.W, H = f.H, spp = f.spp;
    const int s_end = ch.s_end < s_stop ? ch.s_end : s_stop;
    int grid = 1;
    while (grid * grid < spp) grid++;
    const float aspect = (float)W * rcp((float)H);
    const float dsx = iow_px_dsx(aspect, W, grid);
    const float dsy = iow_px_dsy(H, grid);
    bool live = true;     // lane may still find work
    bool busy = false;    // lane owns a pixel
    UnitPix px{};
    uint32_t unit = 0, urays = 0;
    float sx = 0, sy = 0;
    f3 fc = f3{0, 0, 0}, sample = f3{0, 0, 0};
    int s = 0, skip = 0;
    for (;;) {
        DBG_T0(f, t_loop);
        const uint32_t q = fetch_unit(counter, live && !busy);
        if (live && !busy) {
            if (q >= total) live = false;
            else if (ct.in) {  // resume a parked lane
                const float4 *p = ct.in + (size_t)q * kContSlots;
                const float4 m = p[0], a = p[1], b = p[2];
                unit = __float_as_uint(m.x); s = __float_as_int(m.y); skip = __float_as_int(m.z);
                K.size = __float_as_int(m.w);
                fc = f3{a.x, a.y, a.z}; urays = __float_as_uint(a.w);
                sample = f3{b.x, b.y, b.z};
                const float *fl = reinterpret_cast<const float *>(p + 3);
                for (int k = 0; k < kFl; k++) K.base[k * kBlock] = fl[k];
                if constexpr (NARROW)
                    for (int e = 0; e < kIowStack; e++) K.set_bounced(e, __float_as_int(fl[kFl + e]));
                px = unit_pixel(f, unit);
                sx = iow_px_sx(aspect, px.x, W);
                sy = iow_px_sy(px.y, H);
                busy = true;
            } else {
                unit = ch.order ? ch.order[q] : q;
                px = unit_pixel(f, unit);
                if (!px.in_image) {
                    if (ch.final_chunk) write_px(f, px, f3{0, 0, 0}, 0.0f);
                    if (ch.cost) ch.cost[unit] = 0;
                } else {
                    busy = true;
                    sx = iow_px_sx(aspect, px.x, W);
                    sy = iow_px_sy(px.y, H);
                    s = ch.per_unit_begin ? __float_as_int(ch.state[2 * (size_t)unit].w) : ch.s_begin;
                    K.size = 0;
                    urays = 0;
                    if (s == 0) {
                        fc = f3{0, 0, 0};
                        for (int e = 0; e < kIowStack; e++) K.at(e, 7) = 0.0f;  // stale RI slots start at 0
                    } else {  // resume the pixel where the previous chunk parked it
                        const float4 a0 = ch.state[2 * (size_t)unit], a1 = ch.state[2 * (size_t)unit + 1];
                        fc = f3{a0.x, a0.y, a0.z};
                        K.at(0, 7) = a1.x; K.at(1, 7) = a1.y; K.at(2, 7) = a1.z; K.at(3, 7) = a1.w;
                    }
                }
            }
        }
        if (__ballot(live) == 0) break;
        if (may_park && __ballot(!live) != 0 && __popcll(__ballot(busy)) < kParkBelow) {
            // queue drained and the wave is under half busy: park the busy lanes, free the SIMD
            const uint32_t slot = park_slot(ct.out_count, busy);
            if (busy) {
                float4 *p = ct.out + (size_t)slot * kContSlots;
                p[0] = make_float4(ubits(unit), ibits(s), ibits(skip), ibits(K.size));
                p[1] = make_float4(fc.x, fc.y, fc.z, ubits(urays));
                p[2] = make_float4(sample.x, sample.y, sample.z, 0.0f);
                float *fl = reinterpret_cast<float *>(p + 3);
                for (int k = 0; k < kFl; k++) fl[k] = K.base[k * kBlock];
                if constexpr (NARROW)
                    for (int e = 0; e < kIowStack; e++) fl[kFl + e] = ibits(K.bounced(e));
            }
            break;
        }
        DBG_TALLY(f, c, kDbgOuter, busy);
        if (ch.rec_col) {
            // take every following sample whose speculative record assumed the exact stack
            // state (the RI of the entries it read before writing them) from its record
            while (busy && K.size == 0 && s < s_end) {
                const size_t u = (size_t)unit * ch.rec_S + s;  // the record of unit s * rec_P + unit
                const float4 cl = ch.rec_col[u], a = ch.rec_assume[u];
                const uint32_t fl = __float_as_uint(cl.w), rm = fl & 15u, wm = (fl >> 4) & 15u;
                if (((rm & 2u) && __float_as_uint(a.x) != __float_as_uint(K.at(1, 7))) ||
                    ((rm & 4u) && __float_as_uint(a.y) != __float_as_uint(K.at(2, 7))) ||
                    ((rm & 8u) && __float_as_uint(a.z) != __float_as_uint(K.at(3, 7))))
                    break;
                const float4 fn = ch.rec_fin[u];
                const uint4 ct4 = ch.rec_ctr[u];
                fc = fc + f3{cl.x, cl.y, cl.z};
                if (wm & 2u) K.at(1, 7) = fn.x;
                if (wm & 4u) K.at(2, 7) = fn.y;
                if (wm & 8u) K.at(3, 7) = fn.z;
                c.seg += ct4.x; c.drops += ct4.y; c.nans += ct4.z; c.nodes += ct4.w;
                c.prims += __float_as_uint(fn.w);
                urays += ct4.x;
                s++;
            }
        }
        if (busy && K.size == 0 && s < s_end) {  // start sample s
            f3 ro, rd;
            iow_camera_ray(S, f, sx, sy, dsx, dsy, s, ro, rd);
            if (f.show_normal) {
                fc = fc + iow_launch_ray<Cfg::BS - 3, Cfg::NS>(S, f, ro, rd, 32000.0f, 1.0f, c, bstk, nodes).normal;
                s++;
                urays++;
            } else {
                K.push(ro, rd, 1.0f, 1.0f, 0, c);
                sample = f3{0, 0, 0};
                skip = 0;
            }
        }
        DBG_TALLY(f, c, kDbgSeg, busy && K.size > 0);
        DBG_CYC(f, c, kDbgCycCam, t_loop);
        DBG_T0(f, t_seg);
        {
            const bool seg = busy && K.size > 0;
            iow_seg_step<NARROW, Cfg::BS, Cfg::NS>(S, f, K, skip, sample, s, c, bstk, nodes, seg);
            if (seg) {
                urays++;
                if (K.size == 0) { fc = fc + sample; s++; }
            }
        }
        DBG_CYC(f, c, kDbgCycSeg, t_seg);
        if (busy && K.size == 0 && s >= s_end) {
            if (s_end >= s_stop) {
                if (ch.final_chunk) write_px(f, px, fc * rcp((float)s_stop), 0.0f);
                else if (ch.state) {  // early-return pixels: keep the final colour for the last launch
                    ch.state[2 * (size_t)unit] = make_float4(fc.x, fc.y, fc.z, 0.0f);
                }
            } else if (ch.state) {
                ch.state[2 * (size_t)unit] = make_float4(fc.x, fc.y, fc.z, 0.0f);
                ch.state[2 * (size_t)unit + 1] = make_float4(K.at(0, 7), K.at(1, 7), K.at(2, 7), K.at(3, 7));
            }
            if (ch.cost) ch.cost[unit] = urays;
            if (f.px_rays) f.px_rays[unit] = urays;
            busy = false;
        }
    }
    flush(f, c);
}

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3)))
void k_iow03(Frame f, IowScene S, Chunk ch, Cont ct, unsigned *counter, int s_stop) {
    iow03_body<false, 1, false>(f, S, ch, ct, counter, s_stop);
}
__global__ __launch_bounds__(3 * kBlock) void k_iow03L(Frame f, IowScene S, Chunk ch, Cont ct, unsigned *counter,
                                                       int s_stop) {
    iow03_body<false, 3, true>(f, S, ch, ct, counter, s_stop);
}
// u_NumOfBounce <= 255: byte bounce counts + 12-deep BVH stack -> 39 KB LDS per block (A/B layout)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3)))
void k_iow03n(Frame f, IowScene S, Chunk ch, Cont ct, unsigned *counter, int s_stop) {
    iow03_body<true, 1, false>(f, S, ch, ct, counter, s_stop);
}

// ============================================================================ IOW-03, sample-parallel
// One unit = one sample of one pixel (u = s*P + pu), so a heavy pixel's samples run on many
// lanes at once instead of one after another.  Exactness: a sample's result is a function of
// the pixel, the sample index and the RI left in stack entries 1..3 by the samples before it
// (entry 0 is always written before any read).  The sample runs with an assumed value for
// those entries (zeros in the first pass, else what the last resolve computed) and records
// which entries it read before writing (rmask) and which it wrote (wmask); the resolve replays
// the pixel in sample order and re-queues exactly the samples whose assumption was wrong.
// ---------------------------------------------------------------- alternative runs
// The slots (first, count) of unit u's alternative runs; count 0: none.  Open addressing over
// alt_hcap entries, key u + 1.
__device__ __forceinline__ uint2 alt_find(const SpecRecs &R, uint32_t u) {
    if (!R.alt_hash) return make_uint2(0u, 0u);
    uint32_t h = (u * 2654435761u) % R.alt_hcap;
    for (uint32_t i = 0; i < R.alt_hcap; i++) {
        const uint2 e = R.alt_hash[h];
        if (e.x == 0u) break;
        if (e.x == u + 1u) return make_uint2(e.y & 0xffffffu, e.y >> 24);
        h = h + 1u == R.alt_hcap ? 0u : h + 1u;
    }
    return make_uint2(0u, 0u);
}
// A finished alternative run of u (finished in a launch other than `launch`, whose records are
// stable) whose assumption holds on the entries it read under the exact state E: copied into
// u's records, which then read as a finished exact execution (flags tagged with `tag_launch`).
// Returns its slot + 1, or 0.
__device__ uint32_t alt_adopt(const SpecRecs &R, uint32_t u, uint32_t E1, uint32_t E2, uint32_t E3, uint32_t launch,
                              uint32_t tag_launch) {
    const uint2 fk = alt_find(R, u);
    for (uint32_t i = 0; i < fk.y; i++) {
        const AltRec &A = R.alt[fk.x + i];
        const uint32_t st = __hip_atomic_load(&A.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st == 0u || st == launch + 1u || A.u != u) continue;  // (A.u: a record of this unit only)
        const unsigned fl = __float_as_uint(A.col.w), rm = fl & 15u;
        if (((rm & 2u) && __float_as_uint(A.assume.x) != E1) || ((rm & 4u) && __float_as_uint(A.assume.y) != E2) ||
            ((rm & 8u) && __float_as_uint(A.assume.z) != E3))
            continue;
        R.assume[R.ix(u)] = A.assume;
        R.fin[R.ix(u)] = A.fin;
        R.ctr[R.ix(u)] = A.ctr;
        R.col[R.ix(u)] = make_float4(A.col.x, A.col.y, A.col.z,
                               __uint_as_float((fl & ~(63u << 10)) | ((tag_launch & 63u) << 10)));
        return fk.x + i + 1u;
    }
    return 0u;
}

template <bool NARROW, int SUB, bool LN>
__device__ __forceinline__ void iow03s_body(const Frame &f, const IowScene &S, const SpecRecs &R, int mode,
                                            const Cont &ct, unsigned *counter) {
    using Stack = IowStack<NARROW>;
    using Cfg = IowCfg<NARROW, SUB, LN>;
    constexpr int kFl = kIowStack * Stack::kSlot;
    constexpr int BCAP = Cfg::BS - 3;
    __shared__ float lds[SUB * kFl * kBlock];
    __shared__ unsigned char lds_b[NARROW ? SUB * kIowStack * kBlock : 1];
    __shared__ short lds_bvh[SUB * Cfg::BS * kBlock];
    __shared__ unsigned long long s_dbg[SUB * kBlock / 64][kDbgSlots];
    __shared__ float4 s_nodes[LN ? kIowLdsNodes * 7 : 1];
    const int sb = (int)(threadIdx.x / kBlock), tl = (int)(threadIdx.x % kBlock);
    short *bstk = lds_bvh + sb * Cfg::BS * kBlock + tl;  // bslot's layout
    const float4 *nodes = iow_stage_nodes<LN>(S, s_nodes);
    Ctr c;  // per unit here: written to the unit's record, never flushed
    if (f.dbg) {
        c.wdbg = s_dbg[threadIdx.x >> 6];
        if ((threadIdx.x & 63) < kDbgSlots) c.wdbg[threadIdx.x & 63] = 0;
    }
    Stack K{lds + sb * kFl * kBlock + tl, lds_b + (NARROW ? sb * kIowStack * kBlock + tl : 0), 0};
    // units: the parked lanes of ct.in first, then fresh units of the mode ([fresh_lo, fresh_hi)
    // in a mixed launch; all of them in a first launch; none in a plain resume launch)
    const uint32_t nin = ct.in ? *ct.in_count : 0u;
    const uint32_t f_lo = ct.mixed ? ct.fresh_lo : 0u;
    const uint32_t f_n = ct.mixed ? ct.fresh_hi - ct.fresh_lo
                       : (ct.in ? 0u : (mode == kSpecList ? *R.list_count
                                                          : (mode == kSpecFirst ? R.P : R.order_n * (R.S - 1))));
    const uint32_t total = nin + f_n;
    const bool may_park = ct.out != nullptr && total >= ct.park_min;
    const int park_below = ct.park_below ? ct.park_below : kParkBelow;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t wcap = ct.spread ? max(1u, (total + n_waves - 1u) / n_waves) : 64u;
    const int W = f.W, H = f.H, spp = f.spp;
    int grid = 1;
    while (grid * grid < spp) grid++;
    const float aspect = (float)W * rcp((float)H);
    const float dsx = iow_px_dsx(aspect, W, grid);
    const float dsy = iow_px_dsy(H, grid);
    bool live = true, busy = false;
    bool solo = false;  // wave-uniform: the wave holds one unit from the sorted head
    const uint32_t solo_n = min(min(ct.solo_n, n_waves), total);
    bool solo_open = solo_n != 0;  // wave-uniform: the queue head may still be below solo_n
    uint32_t u = 0, urays = 0;
    int skip = 0;
    f3 sample = f3{0, 0, 0};
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    const unsigned started_tag = (1u << 9) | ((R.epoch & 0xffffu) << 16);  // heavy-first: taken, unfinished
    uint32_t useg = 0;  // segments of the current unit in this launch (ct.seg_budget)
    // exact: the unit was (re)started with its exact incoming state (a frontier or fixf restart),
    // so the state after it is exact too and the lane may go on down its pixel's chain
    bool exact = false;
    uint32_t alt_slot = 0;  // an alternative run: its slot + 1 (its record goes to R.alt)
    // the lane's state at a segment boundary -> a continuation slot (13 float4)
    auto park = [&](float4 *p) {
        p[0] = make_float4(ubits(u), ibits(skip), ibits(K.size), ubits(K.wmask | (K.rmask << 4)));
        p[1] = make_float4(sample.x, sample.y, sample.z, ubits(urays));
        p[2] = make_float4(ubits(c.seg), ubits(c.nodes), ubits(c.prims), ubits(c.drops));
        // .y: restart flag (k_iow03_fixf), .z: exact, .w: alternative slot + 1 (bits)
        p[12] = make_float4(ubits(c.nans), 0.0f, exact ? 1.0f : 0.0f, ubits(alt_slot));
        float *fl = reinterpret_cast<float *>(p + 3);
        for (int k = 0; k < kFl; k++) fl[k] = K.base[k * kBlock];
        if constexpr (NARROW)
            for (int e = 0; e < kIowStack; e++) fl[kFl + e] = ibits(K.bounced(e));
    };
    // start unit u (sample s of pixel pu) with assumed stack RI a.xyz in entries 1..3
    auto begin = [&](uint32_t u_, float4 a) {
        u = u_;
#ifdef RT_DIAG
        if (R.dbg_start) R.dbg_start[u] = (ct.launch_id & 0xffffu) | ((R.dbg_start[u] >> 16) + 1u) << 16;
#endif
        const uint32_t pu = u % R.P;
        const int s = (int)(u / R.P);
        const UnitPix px = unit_pixel(f, pu);
        busy = true;
        c.seg = c.nodes = c.prims = c.drops = c.nans = 0;
        urays = 0;
        useg = 0;
        skip = 0;
        sample = f3{0, 0, 0};
        K.size = 0; K.wmask = 0; K.rmask = 0;
        K.at(0, 7) = 0.0f; K.at(1, 7) = a.x; K.at(2, 7) = a.y; K.at(3, 7) = a.z;
        const float sx = iow_px_sx(aspect, px.x, W);
        const float sy = iow_px_sy(px.y, H);
        f3 ro, rd;
        iow_camera_ray(S, f, sx, sy, dsx, dsy, s, ro, rd);
        if (f.show_normal) {  // one ray, no stack: the normal is the sample
            sample = iow_launch_ray<BCAP, Cfg::NS>(S, f, ro, rd, 32000.0f, 1.0f, c, bstk, nodes).normal;
            urays = 1;
        } else K.push(ro, rd, 1.0f, 1.0f, 0, c);
    };
    for (;;) {
        // spread: a wave holds at most wcap units, so a few long samples get a wave each (and the
        // wave-cooperative closest hits) instead of sharing one
        bool want = live && !busy;
        if (wcap < 64u) {
            const int room = (int)wcap - __popcll(__ballot(busy));
            want = want && (int)lanes_below(__ballot(want)) < room;
        }
        // solo head: the queue is read only while this wave has not yet seen it pass solo_n (the
        // counter only grows), so the check costs a load per wave at the start of a launch
        if (solo) {
            if (__ballot(busy) != 0) want = false;  // keep the head unit alone
            else solo = false;
        }
        if (!solo && solo_open && __ballot(want) != 0) {
            const uint32_t head = __builtin_amdgcn_readfirstlane(__hip_atomic_load(
                counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (head >= solo_n) solo_open = false;
            else want = want && __ballot(busy) == 0 && lanes_below(__ballot(want)) == 0;
        }
        const uint32_t q = fetch_unit(counter, want);
        if (solo_open && __ballot(want && q < solo_n) != 0) solo = true;
        if (want) {
            if (q >= total) live = false;
            else if (q < nin && ct.in[(size_t)q * kContSlots + 12].y == 3.0f) {  // an alternative run
                const uint32_t slot = __float_as_uint(ct.in[(size_t)q * kContSlots + 12].z);
                u = __float_as_uint(ct.in[(size_t)q * kContSlots].x);
                begin(u, R.alt[slot].assume);
                exact = false;
                alt_slot = slot + 1u;
            } else if (q < nin && ct.in[(size_t)q * kContSlots + 12].y != 0.0f) {  // doomed while parked: restart exact
                u = __float_as_uint(ct.in[(size_t)q * kContSlots].x);
                begin(u, R.assume[R.ix(u)]);
                exact = ct.chain != 0;
                alt_slot = 0;
            } else if (q < nin) {  // resume a parked lane
                const float4 *p = ct.in + (size_t)q * kContSlots;
                const float4 m = p[0], a = p[1], b = p[2];
                u = __float_as_uint(m.x); skip = __float_as_int(m.y); K.size = __float_as_int(m.z);
                K.wmask = __float_as_uint(m.w) & 15u; K.rmask = __float_as_uint(m.w) >> 4;
                sample = f3{a.x, a.y, a.z}; urays = __float_as_uint(a.w);
                c.seg = __float_as_uint(b.x); c.nodes = __float_as_uint(b.y); c.prims = __float_as_uint(b.z);
                c.drops = __float_as_uint(b.w); c.nans = __float_as_uint(p[12].x);
                exact = p[12].z != 0.0f;
                alt_slot = __float_as_uint(p[12].w);
                const float *fl = reinterpret_cast<const float *>(p + 3);
                for (int k = 0; k < kFl; k++) K.base[k * kBlock] = fl[k];
                if constexpr (NARROW)
                    for (int e = 0; e < kIowStack; e++) K.set_bounced(e, __float_as_int(fl[kFl + e]));
                useg = 0;
                busy = true;
            } else {
                // kSpecFirst: sample 0 of every pixel; kSpecRest: samples 1.. pixel-major, pixels
                // in R.order (heaviest sample 0 first); kSpecList: the re-execution list
                const uint32_t qf = f_lo + (q - nin);
                bool fresh = true;
                if (ct.fresh_mode == 0) {
                    u = mode == kSpecList ? R.list[qf]
                        : (mode == kSpecFirst ? qf : (1u + qf % (R.S - 1)) * R.P + R.order[R.order_base + qf / (R.S - 1)]);
                } else {  // heavy-first enumerations of kSpecRest (a unit may come up twice: run it once)
                    const uint32_t n_px = R.order_n ? R.order_n : R.P, nr = R.S - 1u - R.n_heavy;
                    uint32_t s_, rank;
                    if (ct.fresh_mode == 1) { rank = (qf / (R.S - 1u)) * R.probe_stride; s_ = 1u + qf % (R.S - 1u); }
                    else if (ct.fresh_mode == 2) { s_ = R.sorder[qf / n_px]; rank = qf % n_px; }
                    else { s_ = R.sorder[R.n_heavy + qf % nr]; rank = qf / nr; }
                    u = s_ * R.P + R.order[R.order_base + rank];
                    const uint32_t tag = __float_as_uint(R.col[R.ix(u)].w);
                    fresh = !((tag >> 16) == (R.epoch & 0xffffu) && (tag & 0x300u) != 0u);
                }
                if (fresh && unit_pixel(f, u % R.P).in_image) {
                    if (ct.fresh_mode != 0) R.col[R.ix(u)].w = ubits(started_tag);
                    begin(u, mode == kSpecFirst ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : R.assume[R.ix(u)]);
                    exact = false;
                    alt_slot = 0;
                }
            }
        }
        if (__ballot(live) == 0) break;
        if (may_park && __ballot(!live) != 0 && __popcll(__ballot(busy)) < park_below) {
            const uint32_t slot = park_slot(ct.out_count, busy);
            if (busy) park(ct.out + (size_t)slot * kContSlots);
            break;
        }
        DBG_TALLY(f, c, kDbgOuter, busy);
        DBG_TALLY(f, c, kDbgSeg, busy && K.size > 0);
        DBG_T0(f, t_seg);
        {
            const bool seg = busy && K.size > 0;
            iow_seg_step<NARROW, Cfg::BS, Cfg::NS>(S, f, K, skip, sample, (int)(u / R.P), c, bstk, nodes, seg);
            if (seg) { urays++; useg++; }
        }
        DBG_CYC(f, c, kDbgCycSeg, t_seg);
        if (ct.seg_budget) {  // budgeted round: a unit that used its segments parks (per lane)
            const bool over = busy && K.size > 0 && useg >= ct.seg_budget;
            if (__ballot(over) != 0) {
                const uint32_t slot = park_slot(ct.out_count, over);
                if (over) { park(ct.out + (size_t)slot * kContSlots); busy = false; }
            }
        }
        if (busy && K.size == 0 && alt_slot) {  // an alternative run done: its own record
            AltRec &A = R.alt[alt_slot - 1u];
            A.col = make_float4(sample.x, sample.y, sample.z, ubits(K.rmask | (K.wmask << 4) | done_tag));
            A.fin = make_float4(K.at(1, 7), K.at(2, 7), K.at(3, 7), ubits(c.prims));
            A.ctr = make_uint4(c.seg, c.drops, c.nans, c.nodes);
            __threadfence();
            __hip_atomic_store(&A.state, ct.launch_id + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            busy = false;
            alt_slot = 0;
        }
        if (busy && K.size == 0) {  // sample done: record it
            R.col[R.ix(u)] = make_float4(sample.x, sample.y, sample.z,
                                   ubits(K.rmask | (K.wmask << 4) | done_tag | ((ct.launch_id & 63u) << 10)));
            R.fin[R.ix(u)] = make_float4(K.at(1, 7), K.at(2, 7), K.at(3, 7), ubits(c.prims));
            R.ctr[R.ix(u)] = make_uint4(c.seg, c.drops, c.nans, c.nodes);
#ifdef RT_DIAG
            if (R.dbg_end) R.dbg_end[u] = ct.launch_id;
#endif
            busy = false;
            if (exact) {
                // Chain following: the stack this exact sample left is the exact incoming state of
                // the next sample.  Walk the pixel's following finished samples while their
                // assumptions hold on the entries they read; re-run the first one that does not,
                // here and now, with the exact state.  A pixel whose samples all mispredict (each
                // reads the entry its predecessor wrote) then runs down its chain on one lane,
                // not one sample per frontier round.  Stops at an unfinished sample (running or
                // queued elsewhere), which the frontier handles.
                // Other lanes of this launch may write these records, so only records finished in
                // an earlier launch (stable since that kernel boundary) are read, with
                // device-coherent loads; a record is claimed for a re-run by a compare-and-swap of
                // its flags, and a read whose flags changed meanwhile stops the walk.
                const uint32_t pu = u % R.P;
                uint32_t E1 = __float_as_uint(K.at(1, 7)), E2 = __float_as_uint(K.at(2, 7)),
                         E3 = __float_as_uint(K.at(3, 7));
                auto ld = [](const float *p) {
                    return __hip_atomic_load(reinterpret_cast<const unsigned *>(p), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
                };
                for (uint32_t t = u / R.P + 1u; t < R.S; t++) {
                    const uint32_t v = t * R.P + pu;
                    unsigned *flp = reinterpret_cast<unsigned *>(&R.col[R.ix(v)].w);
                    const unsigned fl = ld(&R.col[R.ix(v)].w);
                    if ((fl & 0xffff0100u) != done_tag || ((fl >> 10) & 63u) == (ct.launch_id & 63u)) break;
                    const unsigned rm = fl & 15u, wm = (fl >> 4) & 15u;
                    const unsigned a1 = ld(&R.assume[R.ix(v)].x), a2 = ld(&R.assume[R.ix(v)].y), a3 = ld(&R.assume[R.ix(v)].z);
                    const unsigned f1 = ld(&R.fin[R.ix(v)].x), f2 = ld(&R.fin[R.ix(v)].y), f3v = ld(&R.fin[R.ix(v)].z);
                    __atomic_thread_fence(__ATOMIC_ACQUIRE);
                    if (ld(&R.col[R.ix(v)].w) != fl) break;
                    if (((rm & 2u) && a1 != E1) || ((rm & 4u) && a2 != E2) || ((rm & 8u) && a3 != E3)) {
                        unsigned expect = fl;
                        if (!__hip_atomic_compare_exchange_strong(flp, &expect, started_tag, __ATOMIC_ACQ_REL,
                                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                            break;
                        const uint32_t got = alt_adopt(R, v, E1, E2, E3, ct.launch_id, ct.launch_id);
                        if (got) {  // an alternative run already holds its exact execution
                            const AltRec &A = R.alt[got - 1u];
                            const unsigned awm = (__float_as_uint(A.col.w) >> 4) & 15u;
                            if (awm & 2u) E1 = __float_as_uint(A.fin.x);
                            if (awm & 4u) E2 = __float_as_uint(A.fin.y);
                            if (awm & 8u) E3 = __float_as_uint(A.fin.z);
                            continue;
                        }
                        const float4 e = make_float4(__uint_as_float(E1), __uint_as_float(E2), __uint_as_float(E3), 0.0f);
                        R.assume[R.ix(v)] = e;
                        begin(v, e);
                        break;
                    }
                    if (wm & 2u) E1 = f1;
                    if (wm & 4u) E2 = f2;
                    if (wm & 8u) E3 = f3v;
                }
                exact = busy;
            }
        }
    }
    if (c.wdbg && (threadIdx.x & 63) == 0)
        for (int i = 0; i < kDbgSlots; i++) atomicAdd(f.dbg + i, c.wdbg[i]);
}

__global__ __launch_bounds__(kBlock) void k_iow03s(Frame f, IowScene S, SpecRecs R, int mode, Cont ct,
                                                   unsigned *counter) {
    iow03s_body<false, 1, false>(f, S, R, mode, ct, counter);
}
__global__ __launch_bounds__(3 * kBlock) void k_iow03sL(Frame f, IowScene S, SpecRecs R, int mode, Cont ct,
                                                        unsigned *counter) {
    iow03s_body<false, 3, true>(f, S, R, mode, ct, counter);
}

// After the sample-0 pass: every later sample of a pixel assumes, for each stack entry 1..3,
// the RI sample 0 left there, or `prior` where sample 0 never wrote it (a guess, checked by
// the resolve; `prior` is the scene's most common refractive index, the value such entries
// almost always hold once any sample has pushed there).  Pixels are keyed by sample 0's ray
// count so the rest run heaviest first.
__global__ __launch_bounds__(kBlock) void k_iow03_prep(Frame f, SpecRecs R, unsigned *key, float prior,
                                                       uint32_t prior_from) {
    const uint32_t pu = blockIdx.x * kBlock + threadIdx.x;
    if (pu >= R.P) return;  // no cross-lane work in this kernel
    const UnitPix px = unit_pixel(f, pu);
    if (!px.in_image) { key[pu] = 0; return; }
    const uint32_t wm = (__float_as_uint(R.col[R.ix(pu)].w) >> 4) & 15u;
    const float4 fn = R.fin[R.ix(pu)];
    const float4 e0 = make_float4((wm & 2u) ? fn.x : 0.0f, (wm & 4u) ? fn.y : 0.0f, (wm & 8u) ? fn.z : 0.0f, 0.0f);
    // From prior_from on every entry is guessed as the prior: sample 0 starts from the all-zero
    // stack no later sample sees (a stale 0 makes target_RI 0 and forces TIR, 03...glsl:316-327),
    // so the values it leaves are a worse guess of the steady state than the scene's most common
    // RI (tests/analysis/fork_stats.py: mispredicted rays 2.6% -> 0.8% on C2).
    const float4 e1 = make_float4(prior, prior, prior, 0.0f);
    for (uint32_t s = 1; s < R.S; s++) R.assume[R.ix((size_t)s * R.P + pu)] = s >= prior_from ? e1 : e0;
#ifdef RT_DIAG
    if (R.exact && (R.exact_mode & 2))
        for (uint32_t s = 1; s < R.S; s++) R.assume[R.ix((size_t)s * R.P + pu)] = R.exact[(size_t)s * R.P + pu];
#endif
    if (R.front)  // sample 0 is exact: the frontier starts at sample 1 with its final entries
        R.front[pu] = make_uint4(1u, __float_as_uint(e0.x), __float_as_uint(e0.y), __float_as_uint(e0.z));
    if (R.front2) R.front2[pu] = make_uint4(0xffffffffu, 0u, 0u, 0u);
    key[pu] = R.ctr[R.ix(pu)].x;
}

// ---------------------------------------------------------------- checkpoint rounds
// Between the rounds of the speculative pass (kernel boundaries, so every finished record is
// visible), each pixel's frontier advances over its finished samples in sample order while
// their assumptions match the exact state E.  The first finished sample whose assumption was
// wrong gets E and is queued at once for an exact re-run in the next round (its record is
// marked unfinished until then), so a mispredicted sample -- long ones especially -- is re-run
// while the pass still has other work, not in a re-execution pass after it.  Samples behind the
// frontier keep speculating; the resolve after the pass checks everything again.
__global__ __launch_bounds__(kBlock) void k_iow03_frontier(Frame f, SpecRecs R, float4 *cont, unsigned *count,
                                                           uint32_t cap) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = R.order_n ? R.order_n : R.P;
    if (i >= n) return;  // no cross-lane work in this kernel
    const uint32_t pu = R.order_n ? R.order[R.order_base + i] : i;
    if (!unit_pixel(f, pu).in_image) return;
    uint4 st = R.front[pu];
    if (st.x >= R.S) return;
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    // queue sample u for an exact re-run with incoming state E (its record is marked unfinished)
    auto requeue = [&](size_t u, uint32_t e1, uint32_t e2, uint32_t e3) {
        const uint32_t slot = atomicAdd(count, 1u);
        if (slot >= cap) { atomicSub(count, 1u); return; }  // full: leave it to the resolve after the pass
        R.assume[R.ix(u)] = make_float4(__uint_as_float(e1), __uint_as_float(e2), __uint_as_float(e3), 0.0f);
        R.col[R.ix(u)].w = __uint_as_float((1u << 9) | ((R.epoch & 0xffffu) << 16));  // queued: unfinished
        float4 *p = cont + (size_t)slot * kContSlots;
        p[0] = make_float4(__uint_as_float((uint32_t)u), 0.0f, 0.0f, 0.0f);
        p[12] = make_float4(0.0f, 1.0f, 0.0f, 0.0f);  // restart with the (now exact) assumption
    };
    uint32_t s = st.x;
    bool queued = false;
    for (; s < R.S; s++) {
        const size_t u = (size_t)s * R.P + pu;
        unsigned fl = __float_as_uint(R.col[R.ix(u)].w);
        if ((fl & 0xffff0100u) != done_tag) {  // still running (or queued): an alternative may hold it
            if (!R.alt || !alt_adopt(R, (uint32_t)u, st.y, st.z, st.w, 0xffffffffu, 0u)) break;
            fl = __float_as_uint(R.col[R.ix(u)].w);
        }
        const float4 a = R.assume[R.ix(u)];
        const unsigned rm = fl & 15u, wm = (fl >> 4) & 15u;
        if (((rm & 2u) && __float_as_uint(a.x) != st.y) || ((rm & 4u) && __float_as_uint(a.y) != st.z) ||
            ((rm & 8u) && __float_as_uint(a.z) != st.w)) {
            if (R.alt && alt_adopt(R, (uint32_t)u, st.y, st.z, st.w, 0xffffffffu, 0u)) {
                fl = __float_as_uint(R.col[R.ix(u)].w);  // the adopted alternative is exact: go on
            } else {
                requeue(u, st.y, st.z, st.w);
                queued = true;
                break;
            }
        }
        const unsigned wm2 = (fl >> 4) & 15u;
        (void)wm;
        const float4 fn = R.fin[R.ix(u)];
        if (wm2 & 2u) st.y = __float_as_uint(fn.x);
        if (wm2 & 4u) st.z = __float_as_uint(fn.y);
        if (wm2 & 8u) st.w = __float_as_uint(fn.z);
    }
    st.x = s;
    R.front[pu] = st;
    // Anchored scan past the blocked sample s.  A finished sample that read no entry it had not
    // written (rmask 0) is exact whatever came before it, and so are the entries it wrote; a
    // finished sample whose reads are all of known entries is exact if its assumption matches
    // them.  Knowledge of entries 1..3 is tracked from s + 1 on (none known at first); once all
    // three are known, a mispredicted finished sample is re-queued at once with the exact state,
    // and the first unfinished one is handed to k_iow03_fixf (front2).  The scan goes on past
    // unfinished and mispredicted samples (knowledge restarts at the next anchor) up to
    // scan_max samples past the frontier.  So a misprediction
    // behind a long running sample is repaired without waiting for that sample (anchors --
    // samples with rmask 0 that write all three entries -- are 18% of the samples of the bench
    // scene, tests/analysis/fork_stats.py).
    if (!R.front2) return;
    uint4 f2 = make_uint4(0xffffffffu, 0u, 0u, 0u);
    if (!queued && s < R.S) {
        unsigned known = 0;
        uint32_t E[4] = {0u, 0u, 0u, 0u};
        const uint32_t k_end = min(R.S, s + 1u + R.scan_max);
        for (uint32_t k = s + 1u; k < k_end; k++) {
            const size_t u = (size_t)k * R.P + pu;
            const unsigned fl = __float_as_uint(R.col[R.ix(u)].w);
            if ((fl & 0xffff0100u) != done_tag) {  // unfinished: fixf may patch the first one
                if (known == 14u && f2.x == 0xffffffffu) f2 = make_uint4(k, E[1], E[2], E[3]);
                known = 0;  // its outputs are unknown; later anchors restore knowledge
                continue;
            }
            const unsigned rm = fl & 14u, wm = (fl >> 4) & 14u;
            if (rm & ~known) { known &= ~wm; continue; }  // read an unknown entry: its writes are unknown
            const float4 a = R.assume[R.ix(u)];
            const bool bad = ((rm & 2u) && __float_as_uint(a.x) != E[1]) ||
                             ((rm & 4u) && __float_as_uint(a.y) != E[2]) ||
                             ((rm & 8u) && __float_as_uint(a.z) != E[3]);
            unsigned wmx = wm;
            if (bad) {  // mispredicted: adopt an alternative, or re-run it now if the whole state is known
                if (known == 14u && R.alt && alt_adopt(R, (uint32_t)u, E[1], E[2], E[3], 0xffffffffu, 0u)) {
                    wmx = (__float_as_uint(R.col[R.ix(u)].w) >> 4) & 14u;
                } else {
                    if (known == 14u) requeue(u, E[1], E[2], E[3]);
                    known = 0;
                    continue;
                }
            }
            const float4 fn = R.fin[R.ix(u)];
            if (wmx & 2u) E[1] = __float_as_uint(fn.x);
            if (wmx & 4u) E[2] = __float_as_uint(fn.y);
            if (wmx & 8u) E[3] = __float_as_uint(fn.z);
            known |= wmx;
        }
    }
    R.front2[pu] = f2;
}
// Alternative runs (RT_SPEC_ALT, between tail rounds): for each pixel, every finished sample
// past the frontier that read exactly one stale entry before writing it, traced at least
// alt_min_seg segments and has no alternatives yet gets one run per other value that entry can
// hold (R.alt_vals), queued as restart records with flag 3.  Such a sample is where a dependent
// chain forms: if its guess was wrong, the frontier adopts the matching alternative instead of
// re-running a long sample once the samples before it are done.
__global__ __launch_bounds__(kBlock) void k_iow03_altspawn(Frame f, SpecRecs R, float4 *cont, unsigned *count,
                                                           uint32_t cap) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = R.order_n ? R.order_n : R.P;
    if (i >= n) return;  // no cross-lane work in this kernel
    const uint32_t pu = R.order_n ? R.order[R.order_base + i] : i;
    if (!unit_pixel(f, pu).in_image) return;
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    for (uint32_t s = R.front[pu].x; s < R.S; s++) {
        const uint32_t u = s * R.P + pu;
        const unsigned fl = __float_as_uint(R.col[R.ix(u)].w);
        if ((fl & 0xffff0100u) != done_tag) continue;
        const unsigned rm = fl & 14u;
        if (rm == 0u || (rm & (rm - 1u)) != 0u) continue;  // exactly one stale entry read
        if (R.ctr[R.ix(u)].x < R.alt_min_seg) continue;
        if (alt_find(R, u).y != 0u) continue;
        const int e = rm == 2u ? 0 : (rm == 4u ? 1 : 2);
        const float4 a = R.assume[R.ix(u)];
        const float ae = e == 0 ? a.x : (e == 1 ? a.y : a.z);
        uint32_t k = 0;
        for (int v = 0; v < R.n_alt_vals; v++) k += __float_as_uint(R.alt_vals[v]) != __float_as_uint(ae);
        if (k == 0u) continue;
        const uint32_t first = atomicAdd(R.alt_count, k);
        if (first + k > R.alt_cap) { atomicSub(R.alt_count, k); return; }
        const uint32_t slot = atomicAdd(count, k);
        if (slot + k > cap) { atomicSub(count, k); return; }  // leaves the claimed alt slots unused
        uint32_t j = 0;
        for (int v = 0; v < R.n_alt_vals; v++) {
            if (__float_as_uint(R.alt_vals[v]) == __float_as_uint(ae)) continue;
            AltRec &A = R.alt[first + j];
            A.u = u;
            A.state = 0u;
            float4 b = a;
            if (e == 0) b.x = R.alt_vals[v]; else if (e == 1) b.y = R.alt_vals[v]; else b.z = R.alt_vals[v];
            A.assume = b;
            float4 *p = cont + (size_t)(slot + j) * kContSlots;
            p[0] = make_float4(__uint_as_float(u), 0.0f, 0.0f, 0.0f);
            p[12] = make_float4(0.0f, 3.0f, __uint_as_float(first + j), 0.0f);  // start an alternative run
            j++;
        }
        // publish u -> (first, k) in the hash (open addressing, key u + 1)
        uint32_t h = (u * 2654435761u) % R.alt_hcap;
        for (uint32_t t = 0; t < R.alt_hcap; t++) {
            const unsigned prev = atomicCAS(&R.alt_hash[h].x, 0u, u + 1u);
            if (prev == 0u) { R.alt_hash[h].y = first | (k << 24); break; }
            h = h + 1u == R.alt_hcap ? 0u : h + 1u;
        }
    }
}

// Parked samples at their pixel's frontier: the exact incoming state E is known.  Entries the
// sample neither read nor wrote get E (exact: it would have started with them); if an entry it
// already read differs from E it restarts with E.  Either way its assumption becomes exact, so
// long samples stop waiting for a later resolve pass to find them wrong.
__global__ __launch_bounds__(kBlock) void k_iow03_fixf(Frame f, SpecRecs R, float4 *cont, const unsigned *count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= *count) return;  // no cross-lane work in this kernel
    float4 *p = cont + (size_t)i * kContSlots;
    if (p[12].y != 0.0f || __float_as_uint(p[12].w) != 0u) return;  // a restart already / an alternative run
    const uint32_t u = __float_as_uint(p[0].x);
    const uint32_t pu = u % R.P, s = u / R.P;
    uint4 st = R.front[pu];
    if (st.x != s) {  // not at the frontier: past it, its exact state may come from the anchored scan
        if (!R.front2) return;
        st = R.front2[pu];
        if (st.x != s) return;
    }
    const unsigned E[3] = {st.y, st.z, st.w};
    const unsigned masks = __float_as_uint(p[0].w), wm = masks & 15u, rm = masks >> 4;
    float4 a = R.assume[R.ix(u)];
    float *av = &a.x;
    bool doomed = false;
    for (int k = 1; k <= 3; k++)
        if (((rm >> k) & 1u) && __float_as_uint(av[k - 1]) != E[k - 1]) doomed = true;
    if (doomed) {
        R.assume[R.ix(u)] = make_float4(__uint_as_float(E[0]), __uint_as_float(E[1]), __uint_as_float(E[2]), 0.0f);
        p[12].y = 1.0f;
        return;
    }
    float *fl = reinterpret_cast<float *>(p + 3);  // parked stack, [entry*9 + field], RI = field 7
    for (int k = 1; k <= 3; k++)
        if (!((wm >> k) & 1u) && !((rm >> k) & 1u)) {
            fl[k * 9 + 7] = __uint_as_float(E[k - 1]);
            av[k - 1] = __uint_as_float(E[k - 1]);
        }
    R.assume[R.ix(u)] = a;
}

// Replay of each pixel's samples in order (one lane per pixel unit; records are [s][pu], so
// consecutive lanes read consecutive records).
__global__ __launch_bounds__(kBlock) void k_iow03_resolve(Frame f, SpecRecs R, int final_pass, float4 *state) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // pixel i of the group (or of all units)
    const bool valid = R.order_n ? i < R.order_n : i < R.P;
    const uint32_t pu = valid ? (R.order_n ? R.order[R.order_base + i] : i) : 0;
    const UnitPix px = unit_pixel(f, valid ? pu : 0);
    bool work = valid && px.in_image;
    uint32_t E1 = 0, E2 = 0, E3 = 0;  // exact RI bits of entries 1..3 before sample s
    f3 fc = f3{0, 0, 0};
    unsigned long long seg = 0, drops = 0, nans = 0, nodes = 0, prims = 0;
    int first_bad = -1;
    uint32_t s = 0;
    for (; work && s < R.S; s++) {
        const size_t u = (size_t)s * R.P + pu;
        float4 cl = R.col[R.ix(u)];
        uint32_t fl = __float_as_uint(cl.w), rm = fl & 15u, wm = (fl >> 4) & 15u;
        float4 a = R.assume[R.ix(u)];
#ifdef RT_DIAG
        if (final_pass && R.exact && (R.exact_mode & 1) && first_bad < 0)
            R.exact[u] = make_float4(__uint_as_float(E1), __uint_as_float(E2), __uint_as_float(E3), 0.0f);
#endif
        bool bad = ((rm & 2u) && __float_as_uint(a.x) != E1) || ((rm & 4u) && __float_as_uint(a.y) != E2) ||
                   ((rm & 8u) && __float_as_uint(a.z) != E3);
        if (bad && first_bad < 0 && R.alt && alt_adopt(R, (uint32_t)u, E1, E2, E3, 0xffffffffu, 0u)) {
            cl = R.col[R.ix(u)];  // an alternative run under the exact state: adopted
            fl = __float_as_uint(cl.w); rm = fl & 15u; wm = (fl >> 4) & 15u;
            a = R.assume[R.ix(u)];
            bad = false;
        }
        if (bad) {
            if (first_bad < 0) first_bad = (int)s;
            if (final_pass) break;  // the sequential kernel takes over from here
            R.assume[R.ix(u)] = make_float4(__uint_as_float(E1), __uint_as_float(E2), __uint_as_float(E3), 0.0f);
            R.list[atomicAdd(R.list_count, 1u)] = (uint32_t)u;
        }
        if (first_bad < 0) {  // still exact: accumulate in sample order
            fc = fc + f3{cl.x, cl.y, cl.z};
            const uint4 ct4 = R.ctr[R.ix(u)];
            seg += ct4.x; drops += ct4.y; nans += ct4.z; nodes += ct4.w;
            prims += __float_as_uint(R.fin[R.ix(u)].w);
        }
        const float4 fn = R.fin[R.ix(u)];  // the record's own outputs (a guess while it is queued)
        if (wm & 2u) E1 = __float_as_uint(fn.x);
        if (wm & 4u) E2 = __float_as_uint(fn.y);
        if (wm & 8u) E3 = __float_as_uint(fn.z);
    }
    if (final_pass && valid && !px.in_image) write_px(f, px, f3{0, 0, 0}, 0.0f);  // tile padding
    if (final_pass && work) {
        if (first_bad < 0) {
            write_px(f, px, fc * rcp((float)R.S), 0.0f);
            if (f.px_rays) f.px_rays[pu] = (unsigned)seg;
        } else {  // resume state for the sequential kernel: colour sum, first sample, stack RI
            state[2 * (size_t)pu] = make_float4(fc.x, fc.y, fc.z, __int_as_float(first_bad));
            state[2 * (size_t)pu + 1] = make_float4(0.0f, __uint_as_float(E1), __uint_as_float(E2), __uint_as_float(E3));
            R.fb_list[atomicAdd(R.fb_count, 1u)] = pu;
        }
    }
    if (final_pass && f.counters) {
        const unsigned long long v[5] = {seg, nodes, prims, drops, nans};
        const int slot[5] = {0, 1, 2, 4, 5};
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const unsigned long long t = wave_sum(v[i]);
            if ((threadIdx.x & 63) == 0 && t) atomicAdd(f.counters + slot[i], t);
        }
    }
}

// ============================================================================ INW
// (the stacks and the closest-hit / surrounding-RI walks: rt_inw_walk.hpp; the sample start and the
// segment body, inw_segment: rt_inw_shade.hpp)

template <bool LIGHTS>
__global__ __launch_bounds__(kBlock) void k_inw(Frame f, InwScene S, Chunk ch, Cont ct, unsigned *counter) {
    __shared__ float lds[kFStack * kBlock];
    Ctr c;
    FStack K{lds + threadIdx.x, 0};
    const uint32_t total = ct.in ? *ct.in_count : units_total(f);
    const bool may_park = ct.out != nullptr && total >= ct.park_min;
    const int s_end = ch.s_end < f.spp ? ch.s_end : f.spp;
    bool live = true, busy = false;
    UnitPix px{};
    uint32_t unit = 0, urays = 0;
    f3 acc = f3{0, 0, 0}, col = f3{0, 0, 0};
    float dmid = 0.0f, dep = 0.0f;
    int s = 0;
    K.size = 0;
    for (;;) {
        const uint32_t q = fetch_unit(counter, live && !busy);
        if (live && !busy) {
            if (q >= total) live = false;
            else if (ct.in) {  // resume a parked lane
                const float4 *p = ct.in + (size_t)q * kContSlots;
                const float4 m = p[0], a = p[1], b = p[2];
                unit = __float_as_uint(m.x); s = __float_as_int(m.y); K.size = __float_as_uint(m.z);
                urays = __float_as_uint(m.w);
                acc = f3{a.x, a.y, a.z}; dmid = a.w;
                col = f3{b.x, b.y, b.z}; dep = b.w;
                const float *fl = reinterpret_cast<const float *>(p + 3);
                for (int k = 0; k < kFStack; k++) K.base[k * kBlock] = fl[k];
                px = unit_pixel(f, unit);
                busy = true;
            } else {
                unit = ch.order ? ch.order[q] : q;
                px = unit_pixel(f, unit);
                if (!px.in_image) {
                    if (ch.final_chunk) write_px(f, px, f3{0, 0, 0}, 0.0f);
                    if (ch.cost) ch.cost[unit] = 0;
                } else {
                    busy = true;
                    s = ch.s_begin;
                    K.size = 0;
                    urays = 0;
                    if (s == 0) { acc = f3{0, 0, 0}; dmid = 0.0f; }
                    else {
                        const float4 a0 = ch.state[2 * (size_t)unit];
                        acc = f3{a0.x, a0.y, a0.z};
                        dmid = a0.w;
                    }
                }
            }
        }
        if (__ballot(live) == 0) break;
        if (may_park && __ballot(!live) != 0 && __popcll(__ballot(busy)) < kParkBelow) {
            const uint32_t slot = park_slot(ct.out_count, busy);
            if (busy) {
                float4 *p = ct.out + (size_t)slot * kContSlots;
                p[0] = make_float4(ubits(unit), ibits(s), ubits(K.size), ubits(urays));
                p[1] = make_float4(acc.x, acc.y, acc.z, dmid);
                p[2] = make_float4(col.x, col.y, col.z, dep);
                float *fl = reinterpret_cast<float *>(p + 3);
                for (int k = 0; k < kFStack; k++) fl[k] = K.base[k * kBlock];
            }
            break;
        }
        DBG_TALLY(f, c, kDbgOuter, busy);
        if (!busy) continue;
        // one ray segment per iteration (samples of a pixel are independent invocations)
        if (K.size == 0) { inw_start_sample(S, f, K, px.x, px.y, s, c); col = f3{0, 0, 0}; dep = 0.0f; }
        DBG_TALLY(f, c, kDbgSeg, true);
        inw_segment<LIGHTS>(S, f, K, s, col, dep, c);
        urays++;
        if (K.size == 0) {  // sample done: End() accumulates sqrt(colour) in sample order
            f3 g = f3{__builtin_sqrtf(col.x), __builtin_sqrtf(col.y), __builtin_sqrtf(col.z)};
            acc = sel(s == 0, g, acc + g);
            if (s == f.spp / 2) dmid = dep;
            s++;
            if (s >= s_end) {
                if (ch.final_chunk) write_px(f, px, acc * rcp((float)f.spp), dmid);
                else ch.state[2 * (size_t)unit] = make_float4(acc.x, acc.y, acc.z, dmid);
                if (ch.cost) ch.cost[unit] = urays;
                busy = false;
            }
        }
    }
    flush(f, c);
}

// ---------------------------------------------------------------- INW wave counts
// Waves per SIMD of the 256-lane INW kernels: INW-04 (LIGHTS) at 3 (159 VGPRs, no spills);
// INW-01 at 4 (128 VGPRs with a few spills, 8% faster on C3 than 3 waves in round 2).
constexpr int kInwWaves = 3;
constexpr int kInw01Waves = 4;  // INW-01: 128 VGPRs with a few spills, 8% faster on C3 than 3 waves

// ---------------------------------------------------------------- INW: on-chip End() folds
// End() (01_BVH...glsl:625-653, 664-675) adds each sample's sqrt(colour) in sample order and
// stores the mean.  The INW kernels below keep that sum on chip.  A wave claims work from the
// global queue, hands its samples to its lanes as a stream g = 0, 1, 2, ... in a fixed order, and
// a lane that finishes a sample takes the next stream entry at once (lane persistence).  A
// finished sample stores its sqrt(colour) into the wave's private ring; the wave folds the ring in
// each pixel's sample order, End()'s float order, and writes a pixel when its last sample is
// folded.  The ring: k_inw_pm's 768-lane instances keep it in LDS (InwScene::lring, the default:
// 256 entries per wave as r, g, b planes; an entry is finished when no busy lane holds it); the
// other kernels keep a global ring of {sqrt(colour), tag g} per wave (16 KB per wave at 1024
// entries, not L2-resident at the chip's 3,000-odd waves: it reaches the fabric).
// The middle sample's depth goes with the pixel's colour.  Entries beyond the oldest unfolded one + ring size are not issued (a
// straggling sample holds the window; the other lanes keep running until it fills).  Counters
// accumulate per lane.  Two stream orders, one per kind of ray coherence:
//  - k_inw_pm (pixel-major): the wave claims pixels and runs all samples of one pixel back to
//    back, so its 64 lanes trace 64 consecutive samples of one pixel -- nearly the same ray where
//    lens, motion and scatter offsets are small next to the scene's detail (C3: 10k small
//    spheres, neighbouring pixels see different spheres).  The fold is wave-serial: once per
//    iteration the wave loads the next 64 ring entries and every lane adds the leading finished
//    run in order (each lane computes the same sum).
//  - k_inw_sm (sample-major): the wave claims 8x8 pixel blocks and runs one sample index over the
//    64 pixels of the block at a time (rows s = 0, 1, ...), so its lanes trace neighbouring
//    pixels at one lens offset, time and scatter direction -- the same ray where the scene is
//    coarse next to a pixel (C5: the Cornell walls).  The fold is lane-parallel: lane p holds
//    pixel p's sum and adds its own samples as they finish.
// k_inw_probe picks one per frame on the device (mode[]): over a sparse set of 8x8 blocks it
// traces one primary ray per pixel; the frame is "coarse" when most blocks with a hit see one
// object in all their pixels.  Both kernels are launched; the one not picked exits at once.
// A fold-ring entry's tag: the low 26 bits of its stream position and the frame's ring epoch
// (0..62) in the high 6 (InwScene::ring_epoch).  An entry left by one of the 62 frames before
// carries another epoch, and the host clears the rings with 0xff bytes (an epoch of 63, never
// valid) whenever the epoch wraps to 0, so a stale entry never passes for a finished one and no
// per-frame clear is needed.  Within a frame, slot g mod R last held g - R (R <= 2^16 < 2^26).
// The fold kernels' framebuffer stores.  Measured and not kept (round 5): nontemporal stores here
// raised C5's L2-to-fabric writes from 4.7 to 37 GB per frame (each streaming 16-B store leaves L2
// as its own partial-line write) at the same frame time.
__device__ __forceinline__ void fb_store(const Frame &f, size_t o, float4 v) {
    reinterpret_cast<float4 *>(f.out_rgba)[o] = v;
}
__device__ __forceinline__ void depth_store(const Frame &f, size_t o, float d) { f.out_depth[o] = d; }
__device__ __forceinline__ uint32_t ring_tag(const InwScene &S, uint32_t g) {
    return (g & 0x03ffffffu) | S.ring_epoch;
}
__device__ __forceinline__ float rdl(float v, uint32_t l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l));
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// the probe's verdict: mode[0] = blocks with a hit, mode[1] = those whose pixels all see one object
__device__ __forceinline__ bool inw_sample_major(const uint32_t *mode, uint32_t force) {
    if (force == 1u) return false;
    if (force == 2u) return true;
    const uint32_t hit = uni(mode[0]), same = uni(mode[1]);
    return 2u * same >= hit && hit > 0u;
}
// Pixel beams (DESIGN.md §5 "Pixel beams").  A pixel's primary rays all pass through its focal
// point F = co + cd * focus and leave the lens disk around C0 = co + cd (radius <= delta0), so they
// lie within beam_R of the central ray C0 + t * cd over t in [beam_tmin, beam_tfar] (host bounds).
// One lane per pixel unit walks the culling BVH with that ray against the boxes inflated by
// beam_R and keeps the beam_cap leaves of smallest entry t, sorted; beam_cut is the smallest
// entry t of a leaf it could not keep.
constexpr int kBeamBlock = 128, kBeamStack = 48, kBeamCapMax = 32;
__global__ __launch_bounds__(kBeamBlock) void k_inw_beam(Frame f, InwScene S, const uint32_t *mode, uint32_t force) {
    if (inw_sample_major(mode, force)) return;
    __shared__ int st[kBeamStack * kBeamBlock];
    __shared__ uint2 lst[kBeamCapMax * kBeamBlock];
    const uint32_t u = blockIdx.x * kBeamBlock + threadIdx.x, lane = threadIdx.x & 63u;
    if (u >= units_total(f)) return;  // whole waves (units come in 8x8 blocks of 64)
    const UnitPix px = unit_pixel(f, u);
    const uint32_t bo = blockIdx.y * S.beam_units;  // time bin blockIdx.y (beam_bins > 1): its tree, its lists
    uint32_t *nout = const_cast<uint32_t *>(S.beam_n) + bo;
    float *cout = const_cast<float *>(S.beam_cut) + bo;
    const uint32_t cap = S.beam_cap;
    uint2 *L = lst + threadIdx.x;
    uint32_t nl = 0;
    float cut = kMiss;
    bool off = false;
    if (px.in_image) {
        const f3 cd = inw_pixel_dir(f, px.x, px.y);
        const f3 o = mk(f.pos[0], f.pos[1], f.pos[2]) + cd;
        const f3 id = f3{rcp(cd.x), rcp(cd.y), rcp(cd.z)};
        off = !(__builtin_isfinite(id.x) && __builtin_isfinite(id.y) && __builtin_isfinite(id.z));
        const float R = S.beam_R, t0 = S.beam_tmin, t1 = S.beam_tfar;
        // near / far planes of each axis for this direction, inflated outward by R
        const uint32_t ox = cd.x < 0.0f ? 3u : 0u, oy = cd.y < 0.0f ? 4u : 1u, oz = cd.z < 0.0f ? 5u : 2u;
        const f3 rn = f3{cd.x < 0.0f ? R : -R, cd.y < 0.0f ? R : -R, cd.z < 0.0f ? R : -R};
        int *stk = st + threadIdx.x;
        int sp = 0, cur = S.beam_bins > 1u ? (int)(1u + S.wbin_base + blockIdx.y * S.wbin_stride) : S.wroot;
        while (!off) {
            const float4 *nd = S.wnodes + kInwNodeF4 * (cur - 1);
            const float4 nx = nd[ox], fx = nd[ox + 3], ny = nd[oy], fy = nd[oy + 3], nz = nd[oz], fz = nd[oz + 3];
            const float4 lk = nd[9];
            const float nxa[4] = {nx.x, nx.y, nx.z, nx.w}, fxa[4] = {fx.x, fx.y, fx.z, fx.w};
            const float nya[4] = {ny.x, ny.y, ny.z, ny.w}, fya[4] = {fy.x, fy.y, fy.z, fy.w};
            const float nza[4] = {nz.x, nz.y, nz.z, nz.w}, fza[4] = {fz.x, fz.y, fz.z, fz.w};
            const int lka[4] = {__float_as_int(lk.x), __float_as_int(lk.y), __float_as_int(lk.z), __float_as_int(lk.w)};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float te = fmaxf(fmaxf(((nxa[k] + rn.x) - o.x) * id.x, ((nya[k] + rn.y) - o.y) * id.y),
                                       ((nza[k] + rn.z) - o.z) * id.z);
                const float tx = fminf(fminf(((fxa[k] - rn.x) - o.x) * id.x, ((fya[k] - rn.y) - o.y) * id.y),
                                       ((fza[k] - rn.z) - o.z) * id.z);
                if (!(fmaxf(te, t0) <= fminf(tx, t1))) continue;
                const int l = lka[k];
                if (l > 0) {
                    if (sp == kBeamStack) off = true;
                    else stk[(sp++) * kBeamBlock] = l;
                } else {  // keep the cap smallest entries, sorted (insertion)
                    float tv = te;
                    uint32_t gv = (uint32_t)(-l);
                    if (nl == cap) {
                        const float last = __uint_as_float(L[(cap - 1) * kBeamBlock].y);
                        if (!(tv < last)) { cut = fminf(cut, tv); continue; }
                        cut = fminf(cut, last);
                        nl--;
                    }
                    uint32_t j = nl;
                    while (j > 0 && __uint_as_float(L[(j - 1) * kBeamBlock].y) > tv) {
                        L[j * kBeamBlock] = L[(j - 1) * kBeamBlock];
                        j--;
                    }
                    L[j * kBeamBlock] = make_uint2(gv, __float_as_uint(tv));
                    nl++;
                }
            }
            if (off || sp == 0) break;
            cur = stk[(--sp) * kBeamBlock];
        }
    }
    // The block's 64 lists packed densely in its region of 64 * cap entries, in unit order (the
    // fold kernel claims a block's pixels one after another, so their lists share cache lines):
    // beam_n[u] = offset in the region << 8 | count
    const uint32_t cnt = off ? 0u : nl;
    uint32_t incl = cnt;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += y;
    }
    const uint32_t at = incl - cnt;
    const size_t base = ((size_t)bo + (u & ~63u)) * cap + at;
    if (S.beam16) {  // object ids < 2^16: the id and the high half of max(t, 0) (t rounded down)
        uint32_t *dst = reinterpret_cast<uint32_t *>(const_cast<uint2 *>(S.beam)) + base;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint2 e = L[j * kBeamBlock];
            const uint32_t tb = __uint_as_float(e.y) > 0.0f ? e.y : 0u;
            dst[j] = (e.x & 0xffffu) | (tb & 0xffff0000u);
        }
    } else {
        uint2 *dst = const_cast<uint2 *>(S.beam) + base;
        for (uint32_t j = 0; j < cnt; j++) dst[j] = L[j * kBeamBlock];
    }
    nout[u] = off ? kBeamOff : (at << 8) | nl;
    cout[u] = px.in_image ? cut : kMiss;
}

template <bool LIGHTS>
__global__ __launch_bounds__(kBlock) void k_inw_probe(Frame f, InwScene S, uint32_t stride, uint32_t *mode) {
    __shared__ float lds[kFStack * kBlock];
    Ctr c;  // not flushed: the probe's rays are not the frame's
    FStack K{lds + threadIdx.x, 0};
    const uint32_t lane = threadIdx.x & 63u, nblk = units_total(f) / 64u;
    const uint32_t blk = ((blockIdx.x * kBlock + threadIdx.x) >> 6) * stride;
    if (blk >= nblk) return;  // whole waves (blk is per wave)
    const UnitPix px = unit_pixel(f, blk * 64u + lane);
    int id = -2;  // -2: outside the image, -1: no hit, else the object
    if (px.in_image) {
        const int s = f.spp / 2;
        inw_start_sample(S, f, K, px.x, px.y, s, c);
        K.size -= 8;
        const uint32_t b = K.size;
        const f3 o = mk(K.at(b), K.at(b + 1), K.at(b + 2)), d = mk(K.at(b + 3), K.at(b + 4), K.at(b + 5));
        const f3 D = mk(f.dir[0], f.dir[1], f.dir[2]);
        float tlim = kMaxT, extra = 0.0f;
        f3 nrm;
        const float g = inw_closest<false>(S, K, o, d, (float)s * f.inv_spp, dot(D, f3{1, 1, 1}) > 0.0f, tlim, nrm,
                                           extra, -1.0f, c);
        id = tlim < kMaxT ? (int)g : -1;
    }
    const int id0 = __shfl(id, __ffsll((long long)__ballot(id != -2)) - 1, 64);
    const bool any_hit = __ballot(id >= 0) != 0ull, same = __ballot(id != -2 && id != id0) == 0ull;
    if (lane == 0 && any_hit) {
        atomicAdd(mode, 1u);
        if (same) atomicAdd(mode + 1, 1u);
    }
}

// Sky blocks (DESIGN.md §5.1 "Sky blocks"; rt_options.inw_sky_blocks).  An 8x8 block whose 64 units
// have an empty and complete beam list in every time bin (count 0, cut kMiss, not kBeamOff) holds
// no pixel whose primary rays can reach a culling box: inw_closest_beam answers "no hit" for every
// such ray that passes its `ok` test, and the sample is the miss branch of inw_segment.  k_inw_sky
// renders those blocks without stacks, walk or ring; the claim-order kernels put them first and
// k_inw_pm's queues start past them.  A block with a ray that fails the test is left to k_inw_pm (its flag cleared).
// Bookkeeping: kSkyInfo uints after the claim order's 256 buckets.
enum { kSkySkip = 0,     // blocks at the head of the claim order that k_inw_pm skips (k_inw_order_scan)
       kSkyFlagged = 1,  // blocks the classifier flagged
       kSkyDone = 2,     // ... of them, those k_inw_sky rendered
       kSkyHead = 3,     // k_inw_order_scatter: cursor of the sky blocks at the head of the order
       kSkyInfo = 16 };
// one wave per 8x8 block; on a sample-major frame every flag is cleared
__global__ __launch_bounds__(kBlock) void k_inw_sky_classify(Frame f, InwScene S, uint32_t *flag, uint32_t *info,
                                                             const uint32_t *mode, uint32_t force) {
    const uint32_t lane = threadIdx.x & 63u, nblk = units_total(f) / 64u;
    const uint32_t blk = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (blk >= nblk) return;  // whole waves
    bool empty = !inw_sample_major(mode, force);
    const uint32_t nb = S.beam_bins > 1u ? S.beam_bins : 1u, u = blk * 64u + lane;
    for (uint32_t b = 0; b < nb && empty; b++) {  // padding units have empty lists too (k_inw_beam)
        const uint32_t nw = S.beam_n[b * S.beam_units + u];
        empty = nw != kBeamOff && (nw & 0xffu) == 0u && S.beam_cut[b * S.beam_units + u] == kMiss;
    }
    const bool sky = __ballot(!empty) == 0ull;
    if (lane == 0) {
        flag[blk] = sky ? 1u : 0u;
        if (sky) atomicAdd(info + kSkyFlagged, 1u);
    }
}
// One 512-lane block per flagged 8x8 block, a wave per row of 8 pixels.  A pass takes 8 samples of
// each pixel (lane = sample * 8 + pixel): the camera ray, the `ok` test, background(cd) and the
// three square roots, staged in LDS; then lane (channel * 8 + pixel) adds its pixel's 8 values in
// sample order -- End()'s sum, one chain per pixel and channel, 24 chains abreast.
// The test is inw_closest_beam's `ok` for a fresh sample, from below: a direction component of
// magnitude >= 2^-100 is non-zero with a finite correctly rounded reciprocal, so no reciprocal is
// computed (a smaller or NaN component sends the block to k_inw_pm, which is always exact).
constexpr int kSkyBlock = 512, kSkyPlane = 72;  // a channel's 64 staged values, padded: the three planes on distinct banks
__global__ __launch_bounds__(kSkyBlock) __attribute__((amdgpu_waves_per_eu(8))) void k_inw_sky(Frame f, InwScene S, uint32_t *flag, uint32_t *info) {
    const uint32_t blk = blockIdx.x;
    if (!uni(flag[blk])) return;  // the whole block
    __shared__ float s_sq[(kSkyBlock / 64) * 3 * kSkyPlane];
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, row = threadIdx.x >> 6, p = lane & 7u, k = lane >> 3;
    float *sq = s_sq + row * (3 * kSkyPlane);
    const UnitPix px = unit_pixel(f, blk * 64u + row * 8u + p);
    const f3 pcd = px.in_image ? inw_pixel_dir(f, px.x, px.y) : f3{0, 0, 0};
    // the fold's lanes: pixel fp of the row, channel fc
    const uint32_t fp = lane & 7u, fc = lane >> 3;
    const bool folds = fc < 3u && __shfl((int)px.in_image, (int)fp, 64) != 0;
    const uint32_t spp = (uint32_t)f.spp;
    float acc = 0.0f;
    bool bad = false;
    for (uint32_t s0 = 0; s0 < spp; s0 += 8u) {
        const uint32_t s = s0 + k;
        if (px.in_image && s < spp) {
            f3 o, d;
            inw_camera_ray(S, f, pcd, (int)s, o, d);
            bad = bad || !(__builtin_fabsf(d.x) >= 0x1p-100f && __builtin_fabsf(d.y) >= 0x1p-100f &&
                           __builtin_fabsf(d.z) >= 0x1p-100f);
            const f3 col = f3{0, 0, 0} + background(d, false) * 1.0f;  // inw_segment's miss branch
            sq[lane] = __builtin_sqrtf(col.x);
            sq[kSkyPlane + lane] = __builtin_sqrtf(col.y);
            sq[2 * kSkyPlane + lane] = __builtin_sqrtf(col.z);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (folds) {
            const uint32_t n = spp - s0 < 8u ? spp - s0 : 8u;
            const float *v = sq + fc * kSkyPlane + fp;
            uint32_t j = 0;
            if (s0 == 0) { acc = v[0]; j = 1; }
            if (n == 8u) {
                float a[8];
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++) a[q] = v[q * 8u];
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++)
                    if (q >= j) acc = acc + a[q];
            } else {
                for (; j < n; j++) acc = acc + v[j * 8u];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(&s_bad, 1u);
    __syncthreads();
    if (s_bad) {  // some ray fails the test: nothing written, k_inw_pm renders the block
        if (threadIdx.x == 0) flag[blk] = 0u;
        return;
    }
    // the row's stores: 8 lanes, 128 B of colour and 32 B of depth (End()'s imageStores, 01_BVH...glsl:652, 667-668)
    const float inv = rcp((float)f.spp);
    const float ax = __shfl(acc, (int)p, 64), ay = __shfl(acc, (int)(8u + p), 64), az = __shfl(acc, (int)(16u + p), 64);
    if (k == 0 && px.out != (size_t)-1) {
        fb_store(f, px.out, make_float4(px.in_image ? ax * inv : 0.0f, px.in_image ? ay * inv : 0.0f,
                                        px.in_image ? az * inv : 0.0f, px.in_image ? 1.0f : 0.0f));
        if (f.out_depth) depth_store(f, px.out, px.in_image ? kMaxT : 0.0f);  // the middle sample's depth: a miss
    }
    // one segment per sample; no node, test, shadow ray, drop or NaN
    const unsigned long long rays = (unsigned long long)__popcll(__ballot(k == 0 && px.in_image)) * spp;
    if (lane == 0 && rays && f.counters) atomicAdd(f.counters, rays);
    if (threadIdx.x == 0) atomicAdd(info + kSkyDone, 1u);
}

// Claim order (DESIGN.md §5 "Claim order"): a persistent fold kernel's tail is the last pixels
// it claims -- a wave needs spp / 64 rounds of samples for one pixel, so expensive pixels claimed
// last leave the rest of the chip idle.  k_inw_cost estimates each pixel's cost from the primary
// rays of two of its samples, the costlier (a miss or a diffuse hit ends the sample; a reflective /
// refractive hit starts a chain of about log(0.01) / log(coefficient) segments, two-sided for
// refraction), keys each 8x8 block by its costliest pixel and buckets it (256 log-scale keys);
// k_inw_order_scan / k_inw_order_scatter lay
// the blocks out costliest first, and k_inw_pm claims through that order.  The order only decides
// which wave traces which pixel when: every pixel's samples and sums are the same.  Pixel-major
// frames only: the three kernels exit at once when the probe picked k_inw_sm, whose 8x8 blocks
// keep their spatial order (measured: C5 3% slower with it, the blocks' locality lost).
// flag (null: none): the sky blocks k_inw_sky rendered (below); they get no bucket, key kSkyKey
constexpr uint32_t kSkyKey = 0xffffffffu;
template <bool LIGHTS>
__global__ __launch_bounds__(kBlock) void k_inw_cost(Frame f, InwScene S, uint32_t *key, uint32_t *hist,
                                                     const uint32_t *mode, uint32_t force, const uint32_t *flag) {
    if (inw_sample_major(mode, force)) return;
    __shared__ float lds[kFStack * kBlock];
    Ctr c;  // not flushed: these rays are not the frame's
    FStack K{lds + threadIdx.x, 0};
    // every pixel of the block (a wave per block), two samples each; the block's key is its
    // costliest pixel's, so the blocks claimed last hold no expensive pixel
    const uint32_t lane = threadIdx.x & 63u, nblk = units_total(f) / 64u, p = lane;
    const uint32_t blk = ((blockIdx.x * kBlock + threadIdx.x) >> 6);
    float est = 0.0f;
    if (blk < nblk && flag && uni(flag[blk])) {  // (wave-uniform: blk is per wave)
        if (p == 0) key[blk] = kSkyKey;
        return;
    }
    if (blk < nblk) {
        const UnitPix px = unit_pixel(f, blk * 64u + p);
        for (int si = 0; si < 2 && px.in_image; si++) {
            const int s = si == 0 ? f.spp / 2 : f.spp / 4;
            K.size = 0;
            inw_start_sample(S, f, K, px.x, px.y, s, c);
            K.size -= 8;
            const uint32_t b = K.size;
            const f3 o = mk(K.at(b), K.at(b + 1), K.at(b + 2)), d = mk(K.at(b + 3), K.at(b + 4), K.at(b + 5));
            const f3 D = mk(f.dir[0], f.dir[1], f.dir[2]);
            float tlim = kMaxT, extra = 0.0f;
            f3 nrm;
            const float g = inw_closest<false>(S, K, o, d, (float)s * f.inv_spp, dot(D, f3{1, 1, 1}) > 0.0f, tlim,
                                               nrm, extra, -1.0f, c);
            float e1 = 1.0f;
            if (tlim < kMaxT) {
                const float4 m0 = S.cold[2 * (int)g];
                const float m = fminf(fmaxf(m0.x, m0.y), 0.99f);
                if (LIGHTS) e1 += (float)S.n_lights;
                if (m > 0.002f) {
                    const float n = fminf((float)f.max_bounces, 1.0f + __logf(0.01f) / __logf(m));
                    e1 += n * (m0.x > 0.002f ? 2.0f : 1.0f) * (LIGHTS ? 1.0f + (float)S.n_lights : 1.0f);
                }
            }
            est = fmaxf(est, e1);
        }
    }
    for (int o = 32; o >= 1; o >>= 1) est = fmaxf(est, __shfl_xor(est, o, 64));
    est *= 16.0f;  // the scale of the 16-pixel sums this key replaced
    if (p == 0 && blk < nblk) {
        const uint32_t k = (uint32_t)fminf(255.0f, 16.0f * __log2f(1.0f + est));
        key[blk] = k;
        atomicAdd(hist + (255u - k), 1u);
    }
}
// exclusive scan of the 256 bucket counts (one 256-lane block).  The blocks without a bucket -- the
// sky blocks, nblk less the buckets' sum -- lead the order, so the buckets' offsets start past them;
// hist[256 + kSkySkip] = their count
__global__ __launch_bounds__(256) void k_inw_order_scan(uint32_t *hist, uint32_t nblk, const uint32_t *mode, uint32_t force) {
    if (inw_sample_major(mode, force)) return;
    __shared__ uint32_t t[256];
    const uint32_t i = threadIdx.x;
    const uint32_t v = hist[i];
    t[i] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 256u; o <<= 1) {
        const uint32_t a = i >= o ? t[i - o] : 0u;
        __syncthreads();
        t[i] += a;
        __syncthreads();
    }
    const uint32_t skip = nblk - t[255];
    hist[i] = skip + t[i] - v;
    if (i == 0u) hist[256u + kSkySkip] = skip;
}
__global__ __launch_bounds__(kBlock) void k_inw_order_scatter(const uint32_t *key, uint32_t *off, uint32_t *order,
                                                               uint32_t nblk, const uint32_t *mode, uint32_t force) {
    if (inw_sample_major(mode, force)) return;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nblk) return;
    const uint32_t k = key[i];
    order[atomicAdd(k == kSkyKey ? off + 256u + kSkyHead : off + (255u - k), 1u)] = i;
}
// k_inw_pm claims through the order from its queues' counters on: they start past the sky blocks
// (counter[0]: the one queue, in units; counter[64 + 16 x]: queue x of the per-XCD queues, which
// holds the claim ordinals congruent to x mod 8), so k_inw_pm itself knows nothing of them
__global__ __launch_bounds__(64) void k_inw_sky_queues(const uint32_t *info, unsigned *counter) {
    const uint32_t x = threadIdx.x, skip = info[kSkySkip];
    if (x == 0u) counter[0] = skip * 64u;
    if (x < 8u) counter[64u + 16u * x] = skip > x ? ((skip - x + 7u) >> 3) * 64u : 0u;
}

// pixel-major stream (see above): entry g = (claimed pixel ordinal j, sample s).  LN: 768-lane
// blocks (3 waves per SIMD) that stage the top of the wide BVH in the LDS their three 256-lane
// stacks leave free (kInwLdsNodes nodes)
// GQ (DESIGN.md §5.1 "GQ"; LN, FU, LRING and INW-01 only): the reference's 40-float stacks in
// global memory (GStack, S.gstk), the wide walks' node stacks in LDS (kWStack entries per lane), the
// closest-hit walks over the quantised nodes, the top kQLdsNodes of them staged in LDS
// k_inw_pm's LDS fold ring: channel c of entry e.  Planes (r, g, b of 256 entries each): the fold's
// lanes 0, 1, 2 read one plane each at the same entry, addresses 1 KB apart, one bank: a 3-way
// conflict per read.  Interleaving the channels (3 e + c) spreads them over 3 banks, but C3 ran 0.5%
// slower (DESIGN_HISTORY.md §J).
#define RIX(c, e) ((c) * kPmLdsRing + (e))
template <bool LN, bool GQ>
constexpr int pm_sub() { return GQ ? kGqSub : (LN ? 3 : 1); }
template <bool LIGHTS, bool LN = false, bool FU = false, bool LRING = false, bool GQ = false>
__global__ __launch_bounds__((pm_sub<LN, GQ>() * kBlock)) __attribute__((amdgpu_waves_per_eu((LN ? pm_sub<LN, GQ>() : (LIGHTS ? kInwWaves : kInw01Waves))))) void k_inw_pm(Frame f, InwScene S0, float4 *ring, uint32_t rmask, unsigned *counter, const uint32_t *mode, uint32_t force, const uint32_t *border) {
    static_assert(!GQ || (LN && FU && LRING && !LIGHTS), "GQ: the C3 instance only");
    if (inw_sample_major(mode, force)) return;  // the probe picked k_inw_sm for this frame
    constexpr int SUB = pm_sub<LN, GQ>();
    // FStack instances: the three 256-lane 40-float stacks; GQ: the wide walks' node stacks (the
    // 40-float stacks are global), the LDS that frees holding the top of the quantised culling BVH
    __shared__ float lds[SUB * (GQ ? kWStack : kFStack) * kBlock];
    // per wave: the middle sample's depth of claimed ordinal j (slot j % 64; at most 64 ordinals lie
    // between the fold and the issue), written out with the pixel's colour
    __shared__ float s_pdep[SUB * kBlock];
    InwScene S = S0;
    // LRING: the fold ring in LDS, after the first kPmLdsNodes staged nodes (InwScene::lring; an
    // instance of its own: as a per-frame branch it cost 1% of C3 in either mode)
    constexpr bool LR = LN && LRING;
    // WLN: the walks read staged nodes.  The LDS-ring instances stage none: the top 5 nodes the
    // ring leaves room for sit in L1 anyway, and the walk loop without the LDS branch (its exec
    // masking and the base pointer kept in a VGPR lane) ran C3 2% faster.  GQ
    // stages kQLdsNodes quantised nodes beside its ring
    constexpr bool WLN = LN && (!LR || GQ);
    float *lr;  // LR: this wave's ring, three planes (r, g, b) of kPmLdsRing floats
    if constexpr (GQ) {
        __shared__ float s_ring[SUB * kBlock / 64 * 3 * kPmLdsRing];
        lr = s_ring + uni((threadIdx.x >> 6) * (3u * kPmLdsRing));
        const uint32_t n = S.qnodes ? (S.n_wnodes < (uint32_t)kQLdsNodes ? S.n_wnodes : (uint32_t)kQLdsNodes) : 0u;
        for (uint32_t i = threadIdx.x; i < n * (uint32_t)kQNodeF4; i += SUB * kBlock) g_inw_qlds[i] = S.qnodes[i];
        __syncthreads();
        S.n_lnodes = n;
    } else {
        lr = reinterpret_cast<float *>(g_inw_lnodes + kPmLdsNodes * kInwNodeF4) + uni((threadIdx.x >> 6) * (3u * kPmLdsRing));
        if constexpr (WLN) {
            const uint32_t cap = (uint32_t)kInwLdsNodes;
            const uint32_t n = S.wnodes ? (S.n_wnodes < cap ? S.n_wnodes : cap) : 0u;
            for (uint32_t i = threadIdx.x; i < n * (uint32_t)kInwNodeF4; i += SUB * kBlock) g_inw_lnodes[i] = S.wnodes[i];
            // no wide walk: the stackless LBVH walks read the top of the LBVH (2 float4 per node) there
            const uint32_t nb = (!S.wnodes && S.sl) ? min(2u * S.n - 1u, cap * (uint32_t)kInwNodeF4 / 2u) : 0u;
            for (uint32_t i = threadIdx.x; i < 2u * nb; i += SUB * kBlock) g_inw_lnodes[i] = S.nodes[i];
            __syncthreads();
            S.n_lnodes = n;
            S.n_blds = nb;
        }
    }
    Ctr c;
#ifdef RT_DIAG_SPLIT
    const unsigned long long t_start = wall_clock64();  // the tail split (tools/inw_split.py)
    unsigned long long t_qd = 0;
#endif
    using KS = std::conditional_t<GQ, GStack, FStack>;
    KS K;
    if constexpr (GQ) {
        K.col = S.gstk + ((size_t)blockIdx.x * (SUB * kBlock) + threadIdx.x);
        K.stride = gridDim.x * (SUB * kBlock);
        K.ws = lds + (threadIdx.x / kBlock) * (kWStack * kBlock) + (threadIdx.x % kBlock);
        K.rc = false;
    } else {
        K.base = lds + (threadIdx.x / kBlock) * (kFStack * kBlock) + (threadIdx.x % kBlock);
    }
    K.size = 0;
    const uint32_t lane = threadIdx.x & 63u;
    if constexpr (LR) rmask = kPmLdsRing - 1u;
    const uint32_t rsize = rmask + 1u;
    float4 *wr = ring + (size_t)uni((blockIdx.x * (SUB * kBlock) + threadIdx.x) >> 6) * rsize;
    float *pdep = s_pdep + (threadIdx.x & ~63u);
    const uint32_t spp = (uint32_t)f.spp, mid = spp / 2u, total = units_total(f);
    const float inv = rcp((float)f.spp);
    // wave-uniform: stream positions (entry gi / fold gf) as (pixel ordinal, sample), claims
    uint32_t gi = 0, ji = 0, si = 0;   // next entry to issue: pixel ordinal ji, sample si
    uint32_t gf = 0, jf = 0, sf = 0;   // next entry to fold
    uint32_t nclaimed = 0;             // pixel ordinals claimed so far
    bool qdone = false;
    uint32_t xq = 0;                   // S.xcdq: queues found empty (from this block's XCD on)
    const uint32_t nblk8 = total / 64u;  // 8x8 blocks (units come in whole blocks)
    f3 acc = f3{0, 0, 0};              // running End() sum of pixel jf (the same in every lane)
    float accc = 0.0f;                 // LR: lane c < 3 holds channel c of that sum
    uint32_t pix_slot = 0xffffffffu;   // lane l: the unit of the claimed ordinal j with j % 64 == l
    // per lane: the sample it traces
    bool busy = false;
    uint32_t g = 0, pj = 0;  // the lane's stream entry and its pixel's ordinal slot (j % 64)
    int s = 0;
    UnitPix px{};
    uint32_t bu = kBeamOff;  // the lane's pixel unit for its beam list (S.beam)
    uint32_t pu = 0xffffffffu;  // the unit px and pcd belong to: a lane's next sample is mostly the same pixel's
    f3 pcd = f3{0, 0, 0};
    f3 col = f3{0, 0, 0};
    float dep = 0.0f;
    K.size = 0;
    for (;;) {
        // ---- fold the finished entries gf, gf+1, ... (stored in earlier iterations)
        INW_T0(t_fold);
        if (gf != gi) {
            const uint32_t k = gf + lane;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uint32_t n;
            bool continue_fold = true;  // (the LDS-ring fold below finishes the run itself)
            if constexpr (LR) {
                // Every issued entry is either held by a busy lane or stored, so the entries below
                // the smallest one a busy lane holds are finished: no tags.  LDS ops of one wave
                // complete in order, so the stores of earlier iterations are visible.
                n = uni(__ockl_wfred_min_u32(busy ? g - gf : 0xffffffffu));  // DPP reduction
                if (n > gi - gf) n = gi - gf;
                if (n > 64u) n = 64u;
                if (lane < n) {
                    const uint32_t e = k & rmask;
                    v = make_float4(lr[RIX(0u, e)], lr[RIX(1u, e)], lr[RIX(2u, e)], 0.0f);
                }
            } else {
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's ring stores have landed (same CU: L1 write-through)
                bool fin = false;
                if (k - gf < gi - gf) {
                    v = wr[k & rmask];
                    fin = __float_as_uint(v.w) == ring_tag(S, k);
                }
                const unsigned long long m = __ballot(fin);
                n = ~m == 0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
            }
            if constexpr (LR) {
                // LDS ring: lanes 0, 1, 2 add the r, g, b planes' entries straight from LDS, each
                // its channel in sample order (the same float additions, two instructions per entry
                // instead of three readlanes and three adds); the run splits at pixel ends
                const uint32_t lc = lane < 3u ? lane : 0u;  // this lane's channel
                for (uint32_t i = 0; i < n;) {
                    const uint32_t e = i + (n - i < spp - sf ? n - i : spp - sf);
                    if (lane < 3u) {
                        uint32_t j = i;
                        if (sf == 0) { accc = lr[RIX(lc, (gf + j) & rmask)]; j++; }
                        constexpr uint32_t kFU = 4;  // loads in flight, then the adds in order (8, 16: same time)
                        for (; j + kFU <= e; j += kFU) {
                            float a[kFU];
#pragma unroll
                            for (uint32_t u = 0; u < kFU; u++) a[u] = lr[RIX(lc, (gf + j + u) & rmask)];
#pragma unroll
                            for (uint32_t u = 0; u < kFU; u++) accc = accc + a[u];
                        }
                        for (; j < e; j++) accc = accc + lr[RIX(lc, (gf + j) & rmask)];
                    }
                    sf += e - i;
                    i = e;
                    if (sf == spp) {  // pixel jf complete: End()'s imageStores (01_BVH...glsl:652, 667-668)
                        const uint32_t unit = uni((uint32_t)__builtin_amdgcn_readlane((int)pix_slot, (int)(jf & 63u)));
                        const float ax = rdl(accc, 0u), ay = rdl(accc, 1u), az = rdl(accc, 2u);
                        if (lane == 0) {
                            const UnitPix p = unit_pixel(f, unit);
                            if (p.out != (size_t)-1) {
                                fb_store(f, p.out,
                                         make_float4(p.in_image ? ax * inv : 0.0f, p.in_image ? ay * inv : 0.0f,
                                                     p.in_image ? az * inv : 0.0f, p.in_image ? 1.0f : 0.0f));
                                if (f.out_depth) depth_store(f, p.out, pdep[jf & 63u]);
                            }
                        }
                        sf = 0;
                        jf++;
                    }
                }
                gf += n;
                continue_fold = false;
            }
            // the run splits at pixel ends: per pixel, its entries are added with no test between them
            for (uint32_t i = 0; continue_fold && i < n;) {
                const uint32_t e = i + (n - i < spp - sf ? n - i : spp - sf);
                uint32_t j = i;
                if (sf == 0) { acc = f3{rdl(v.x, j), rdl(v.y, j), rdl(v.z, j)}; j++; }
                for (; j + 4u <= e; j += 4u) {  // four adds in order, one loop test
                    acc = acc + f3{rdl(v.x, j), rdl(v.y, j), rdl(v.z, j)};
                    acc = acc + f3{rdl(v.x, j + 1u), rdl(v.y, j + 1u), rdl(v.z, j + 1u)};
                    acc = acc + f3{rdl(v.x, j + 2u), rdl(v.y, j + 2u), rdl(v.z, j + 2u)};
                    acc = acc + f3{rdl(v.x, j + 3u), rdl(v.y, j + 3u), rdl(v.z, j + 3u)};
                }
                for (; j < e; j++) acc = acc + f3{rdl(v.x, j), rdl(v.y, j), rdl(v.z, j)};
                sf += e - i;
                i = e;
                if (sf == spp) {  // pixel jf complete: End()'s imageStores (01_BVH...glsl:652, 667-668)
                    const uint32_t unit = uni((uint32_t)__builtin_amdgcn_readlane((int)pix_slot, (int)(jf & 63u)));
                    if (lane == 0) {
                        const UnitPix p = unit_pixel(f, unit);
                        if (p.out != (size_t)-1) {
                            fb_store(f, p.out,
                                     make_float4(p.in_image ? acc.x * inv : 0.0f, p.in_image ? acc.y * inv : 0.0f,
                                                 p.in_image ? acc.z * inv : 0.0f, p.in_image ? 1.0f : 0.0f));
                            if (f.out_depth) depth_store(f, p.out, pdep[jf & 63u]);
                        }
                    }
                    sf = 0;
                    jf++;
                }
            }
            if (continue_fold) gf += n;
        }
        INW_CYC(c, 2, t_fold);
        INW_T0(t_issue);
        // ---- claim pixels for the free lanes (at most 64 pixels between fold and issue)
        const unsigned long long fm = __ballot(!busy);
        const uint32_t nfree = (uint32_t)__popcll(fm);
        if (!qdone && nfree) {
            // ordinals the free lanes would reach: ji + (si + nfree - 1) / spp, capped at jf + 63
            uint32_t need = ji + (si + nfree - 1u) / spp + 1u;
            if (need > jf + 64u) need = jf + 64u;
            if (need > nclaimed) {
                const uint32_t want = need - nclaimed;
                uint32_t base = 0, got = 0, qx = 0;
                if (S.xcdq) {
                    // per-XCD queues (rt_options.inw_claim_xcd): queue x holds the blocks of claim
                    // ordinal b = x mod 8, in claim order, so a block's pixels -- whole 128-B lines of
                    // the framebuffer per block row -- are written through one XCD's L2 (workgroups go
                    // to the XCDs round robin); a wave whose queue is empty takes from the next ones
                    while (xq < 8u) {  // wave-uniform
                        qx = (blockIdx.x + xq) & 7u;
                        const uint32_t nb = nblk8 > qx ? (nblk8 - qx + 7u) >> 3 : 0u, qt = nb * 64u;
                        if (lane == 0) base = atomicAdd(counter + 64u + 16u * qx, want);
                        base = uni((uint32_t)__shfl((int)base, 0, 64));
                        if (base < qt) {
                            got = min(want, qt - base);
                            if (base + want >= qt) xq++;
                            break;
                        }
                        xq++;
                    }
                    if (xq >= 8u) qdone = true;
                } else {
                    if (lane == 0) base = atomicAdd(counter, want);
                    base = uni((uint32_t)__shfl((int)base, 0, 64));
                    got = want;
                    if (base >= total) { got = 0; qdone = true; }
                    else if (base + want >= total) { got = total - base; qdone = true; }
                }
#ifdef RT_DIAG_SPLIT
                if (qdone && t_qd == 0) t_qd = wall_clock64();
#endif
                const uint32_t rel = (lane - nclaimed) & 63u;
                if (rel < got) {  // ordinal -> unit through the claim order (block-wise)
                    uint32_t u = base + rel;
                    if (S.xcdq) u = (((u >> 6) << 3) + qx) * 64u + (u & 63u);  // queue ordinal -> claim ordinal
                    pix_slot = border ? border[u >> 6] * 64u + (u & 63u) : u;
                }
                nclaimed += got;
            }
        }
        // ---- issue: free lanes take stream entries in lane order, within the window
        {
            const uint32_t rank = (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
            uint32_t avail = rsize - (gi - gf);
            const uint64_t left = (uint64_t)(nclaimed - ji) * spp - si;  // entries of claimed pixels not issued
            if ((uint64_t)avail > left) avail = (uint32_t)left;
            const uint32_t take = nfree < avail ? nfree : avail;
            if (take) {
                // this lane's entry: pixel ji + adv / spp, sample adv % spp (adv < spp + 64: one
                // subtraction when spp >= 64)
                const uint32_t adv = si + rank;
                const uint32_t q = spp >= 64u ? (adv >= spp ? 1u : 0u) : adv / spp;
                const uint32_t jl = ji + q;
                const uint32_t unit = (uint32_t)__shfl((int)pix_slot, (int)(jl & 63u), 64);
                if (!busy && rank < take) {
                    g = gi + rank;
                    pj = jl & 63u;
                    s = (int)(adv - q * spp);
                    if (unit != pu) {
                        pu = unit;
                        px = unit_pixel(f, unit);
                        if (px.in_image) pcd = inw_pixel_dir(f, px.x, px.y);
                    }
                    bu = S.beam ? unit : kBeamOff;
                    col = f3{0, 0, 0};
                    dep = 0.0f;
                    if (px.in_image) {
                        busy = true;
                        inw_start_sample_cd(S, f, K, pcd, s, c);
                    } else {  // a padding slot: an empty sample, folded as zero
                        if ((uint32_t)s == mid) pdep[pj] = 0.0f;
                        if constexpr (LR) {
                            const uint32_t e = g & rmask;
                            lr[RIX(0u, e)] = 0.0f; lr[RIX(1u, e)] = 0.0f; lr[RIX(2u, e)] = 0.0f;
                        } else {
                            wr[g & rmask] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ring_tag(S, g)));
                        }
                    }
                }
                gi += take;
                const uint32_t a2 = si + take;
                ji += a2 / spp;
                si = a2 % spp;
            }
        }
        INW_CYC(c, 3, t_issue);
        if (qdone && ji == nclaimed && gf == gi && __ballot(busy) == 0) break;
        // ---- one ray segment per busy lane (samples are independent invocations)
        INW_T0(t_seg);
        OCC_TALLY(c, kOccSeg, busy);
        // Two rounds per iteration (DESIGN.md §5 "Primary and bounce rounds"): primary rays take
        // the beam lists, bounce rays the wide walk, two code paths a wave runs one after the other
        // (one walk trip then carries only the lanes with a bounce ray).  Round 0 runs the lanes
        // whose next ray is a primary one; round 1 every lane with a ray left, the bounce rays those
        // primaries just pushed included, so the walk runs with the bounce rays of the whole wave.
        // INW-04 (LIGHTS) keeps one round: with its shadow walks the two-round loop spills 17 VGPRs
        constexpr int kRounds = LIGHTS ? 1 : 2;
#pragma unroll 1
        for (int round = 2 - kRounds; round < 2; round++) {
            const bool prim = bu != kBeamOff && K.top_primary();
            const bool go = busy && (round == 0 ? prim : K.size > 0u);
            INW_T0(t_rnd);
            if (go) {
                if (f.px_rays) atomicAdd(f.px_rays + px.out, 1u);  // rt_debug_pixel_rays (diagnostics only)
                inw_segment<LIGHTS, WLN, FU, GQ>(S, f, K, s, col, dep, c, bu);
            }
#ifdef RT_DIAG_SPLIT
            c.rnd[round] += (unsigned long long)clock64() - t_rnd;
#endif
            if (busy && K.size == 0) {  // sample done: its sqrt(colour) (01_BVH...glsl:670) to the ring
                if constexpr (LR) {
                    const uint32_t e = g & rmask;
                    lr[RIX(0u, e)] = __builtin_sqrtf(col.x);
                    lr[RIX(1u, e)] = __builtin_sqrtf(col.y);
                    lr[RIX(2u, e)] = __builtin_sqrtf(col.z);
                } else {
                    wr[g & rmask] = make_float4(__builtin_sqrtf(col.x), __builtin_sqrtf(col.y), __builtin_sqrtf(col.z),
                                                __uint_as_float(ring_tag(S, g)));
                }
                if ((uint32_t)s == mid) pdep[pj] = dep;  // 01_BVH...glsl:667-668, stored with the pixel's colour
                busy = false;
            }
        }
        INW_CYC(c, 4, t_seg);
    }
#ifdef RT_DIAG_SPLIT
    // phases 0-1 and 5-7 run inside `if (busy)`: the wave's time there is the largest of its lanes'
    for (int k = 0; k < 8; k++) {
        if (k >= 2 && k < 5) continue;
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long t = __shfl_xor(c.cyc[k], o, 64);
            c.cyc[k] = t > c.cyc[k] ? t : c.cyc[k];
        }
    }
    if (f.dbg && lane == 0) {
        for (int k = 0; k < 8; k++) atomicAdd(f.dbg + 8 + k, c.cyc[k]);
        atomicAdd(f.dbg + 24, c.rnd[0]);
        atomicAdd(f.dbg + 25, c.rnd[1]);
        // wall clock (100 MHz): first / last wave start, first queue drain, first / last wave exit
        const unsigned long long t_end = wall_clock64();
        unsigned long long *t = reinterpret_cast<unsigned long long *>(f.dbg) + 16;
        atomicMin(t, t_start); atomicMax(t + 1, t_start);
        if (t_qd) atomicMin(t + 2, t_qd);
        atomicMin(t + 3, t_end); atomicMax(t + 4, t_end);
    }
#endif
#ifdef RT_DIAG_OCC
    if (f.dbg && lane == 0)
        for (int k = 0; k < kOccSlots; k++) atomicAdd(f.dbg + 32 + k, c.occ[k]);
#endif
    flush(f, c);
}

// sample-major stream (see above): entry g = block ordinal b, sample s, pixel p (b * 64 * spp + s * 64 + p)
// LRING: the fold ring in LDS after the first kPmLdsNodes staged nodes, as k_inw_pm's (InwScene::
// lring_sm: chosen when the scene's BVH top fits those nodes, so the staging loses nothing)
template <bool LIGHTS, bool LN = false, bool FU = false, bool LRING = false>
__global__ __launch_bounds__(LN ? 3 * kBlock : kBlock) __attribute__((amdgpu_waves_per_eu(LN ? 3 : (LIGHTS ? kInwWaves : kInw01Waves)))) void k_inw_sm(Frame f, InwScene S0, float4 *ring, uint32_t rmask, unsigned *counter, const uint32_t *mode, uint32_t force, const uint32_t *) {
    if (!inw_sample_major(mode, force)) return;  // the probe picked k_inw_pm for this frame
    constexpr int SUB = LN ? 3 : 1;
    constexpr bool LR = LN && LRING;
    __shared__ float lds[SUB * kFStack * kBlock];
    InwScene S = S0;
    if constexpr (LN) {
        const uint32_t cap = LR ? (uint32_t)kPmLdsNodes : (uint32_t)kInwLdsNodes;
        const uint32_t n = S.wnodes ? (S.n_wnodes < cap ? S.n_wnodes : cap) : 0u;
        for (uint32_t i = threadIdx.x; i < n * (uint32_t)kInwNodeF4; i += SUB * kBlock) g_inw_lnodes[i] = S.wnodes[i];
        const uint32_t nb = (!S.wnodes && S.sl) ? min(2u * S.n - 1u, cap * (uint32_t)kInwNodeF4 / 2u) : 0u;
        for (uint32_t i = threadIdx.x; i < 2u * nb; i += SUB * kBlock) g_inw_lnodes[i] = S.nodes[i];
        __syncthreads();
        S.n_lnodes = n;
        S.n_blds = nb;
    }
    Ctr c;
    FStack K{lds + (threadIdx.x / kBlock) * (kFStack * kBlock) + (threadIdx.x % kBlock), 0};
    const uint32_t lane = threadIdx.x & 63u;
    if constexpr (LR) rmask = kPmLdsRing - 1u;
    const uint32_t rsize = rmask + 1u;
    float4 *wr = ring + (size_t)uni((blockIdx.x * (SUB * kBlock) + threadIdx.x) >> 6) * rsize;
    // LR: this wave's ring, three planes (r, g, b) of kPmLdsRing floats
    float *lr = reinterpret_cast<float *>(g_inw_lnodes + kPmLdsNodes * kInwNodeF4) + uni((threadIdx.x >> 6) * (3u * kPmLdsRing));
    const uint32_t spp = (uint32_t)f.spp, mid = spp / 2u, nblk = units_total(f) / 64u;
    const uint32_t E = 64u * spp;  // entries per block
    const float inv = rcp((float)f.spp);
    // wave-uniform issue state: next entry = offset ei of block ordinal bi; gi = bi * E + ei
    uint32_t gi = 0, bi = 0, ei = 0, nclaimed = 0;
    bool qdone = false;
    uint32_t blk_slot = 0xffffffffu;  // lane l: the block id of ordinal j with j % 64 == l
    // per-lane fold state: pixel `lane` of block ordinal bf, next sample sf
    uint32_t bf = 0, sf = 0;
    f3 acc = f3{0, 0, 0};
    // per-lane trace state
    bool busy = false;
    uint32_t g = 0;
    int s = 0;
    UnitPix px{};
    f3 col = f3{0, 0, 0};
    float dep = 0.0f;
    K.size = 0;
    for (;;) {
        // ---- fold: lane p adds the finished samples of its pixel, in order (up to 2 per iteration)
        {
            if constexpr (!LR) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's ring stores have landed (same CU: L1 write-through)
            // LR: every issued entry is either held by a busy lane or stored (LDS ops of one wave
            // complete in order), so the issued entries below the oldest one a busy lane holds are
            // finished: no tags (the window keeps every unfolded entry from being overwritten)
            uint32_t hold = 0u;
            if constexpr (LR) hold = uni(__ockl_wfred_min_u32(busy ? g - (gi - rsize) : 0xffffffffu));
            const uint32_t my_blk = (uint32_t)__shfl((int)blk_slot, (int)(bf & 63u), 64);
            if (bf != nclaimed) {
                uint32_t gg[2];
                float4 v[2];
                bool fin[2];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const uint32_t sk = sf + (uint32_t)k;
                    gg[k] = bf * E + (sk < spp ? sk : spp - 1u) * 64u + lane;
                    const uint32_t rel = gg[k] - (gi - rsize);
                    const bool ok = sk < spp && rel < rsize;  // issued (and inside the window)
                    if constexpr (LR) {
                        fin[k] = ok && rel < hold;
                        const uint32_t e = gg[k] & rmask;
                        v[k] = fin[k] ? make_float4(lr[e], lr[kPmLdsRing + e], lr[2u * kPmLdsRing + e], 0.0f)
                                      : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    } else {
                        v[k] = ok ? wr[gg[k] & rmask] : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(~ring_tag(S, gg[k])));
                        fin[k] = __float_as_uint(v[k].w) == ring_tag(S, gg[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (!fin[k] || sf == spp) break;
                    const f3 gv = f3{v[k].x, v[k].y, v[k].z};
                    acc = sf == 0 ? gv : acc + gv;
                    if (++sf == spp) {  // pixel complete: End()'s imageStore (01_BVH...glsl:652)
                        const UnitPix p = unit_pixel(f, my_blk * 64u + lane);
                        if (p.out != (size_t)-1)
                            fb_store(f, p.out,
                                     make_float4(p.in_image ? acc.x * inv : 0.0f, p.in_image ? acc.y * inv : 0.0f,
                                                 p.in_image ? acc.z * inv : 0.0f, p.in_image ? 1.0f : 0.0f));
                    }
                }
                if (sf == spp) { sf = 0; bf++; }
            }
        }
        // the ring window starts at the oldest unfolded entry of the wave (a lane whose next sample
        // is not issued yet holds nothing back)
        const uint32_t gnext = bf == nclaimed ? gi : bf * E + sf * 64u + lane;
        const int dl = (int)(gi - gnext);
        uint32_t dmax = dl > 0 ? (uint32_t)dl : 0u, bmin = bf;
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t t = (uint32_t)__shfl_xor((int)dmax, o, 64), tb = (uint32_t)__shfl_xor((int)bmin, o, 64);
            dmax = t > dmax ? t : dmax;
            bmin = tb < bmin ? tb : bmin;
        }
        dmax = uni(dmax);
        bmin = uni(bmin);
        // ---- claim blocks for the free lanes (at most 64 blocks between fold and issue)
        const unsigned long long fm = __ballot(!busy);
        const uint32_t nfree = (uint32_t)__popcll(fm);
        if (!qdone && nfree) {
            uint32_t need = bi + (ei + nfree - 1u) / E + 1u;
            if (need > bmin + 64u) need = bmin + 64u;
            if (need > nclaimed) {
                const uint32_t want = need - nclaimed;
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(counter, want);
                base = uni((uint32_t)__shfl((int)base, 0, 64));
                uint32_t got = want;
                if (base >= nblk) { got = 0; qdone = true; }
                else if (base + want >= nblk) { got = nblk - base; qdone = true; }
                const uint32_t rel = (lane - nclaimed) & 63u;
                if (rel < got) blk_slot = base + rel;
                nclaimed += got;
            }
        }
        // ---- issue: free lanes take the next stream entries in lane order, inside the window
        {
            const uint32_t rank = (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
            uint32_t avail = rsize - dmax;
            const uint64_t left = (uint64_t)(nclaimed - bi) * E - ei;
            if ((uint64_t)avail > left) avail = (uint32_t)left;
            const uint32_t take = nfree < avail ? nfree : avail;
            if (take) {
                uint32_t b = bi, e = ei + rank;
                if (e >= E) { e -= E; b++; }
                const uint32_t blk = (uint32_t)__shfl((int)blk_slot, (int)(b & 63u), 64);
                if (!busy && rank < take) {
                    g = gi + rank;
                    s = (int)(e >> 6);
                    px = unit_pixel(f, blk * 64u + (e & 63u));
                    col = f3{0, 0, 0};
                    dep = 0.0f;
                    if (px.in_image) {
                        busy = true;
                        inw_start_sample(S, f, K, px.x, px.y, s, c);
                    } else {  // a padding slot: an empty sample, folded as zero
                        if ((uint32_t)s == mid && f.out_depth && px.out != (size_t)-1) depth_store(f, px.out, 0.0f);
                        if constexpr (LR) {
                            const uint32_t e = g & rmask;
                            lr[e] = 0.0f; lr[kPmLdsRing + e] = 0.0f; lr[2u * kPmLdsRing + e] = 0.0f;
                        } else wr[g & rmask] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ring_tag(S, g)));
                    }
                }
                gi += take;
                ei += take;
                if (ei >= E) { ei -= E; bi++; }
            }
        }
        if (qdone && bi == nclaimed && bmin == nclaimed && __ballot(busy) == 0) break;
        OCC_TALLY(c, kOccSeg, busy);
        if (busy) {
            inw_segment<LIGHTS, LN, FU>(S, f, K, s, col, dep, c);
            if (f.px_rays) atomicAdd(f.px_rays + px.out, 1u);  // rt_debug_pixel_rays (diagnostics only)
        }
        if (busy && K.size == 0) {  // sample done: its sqrt(colour) (01_BVH...glsl:670) to the ring
            if constexpr (LR) {
                const uint32_t e = g & rmask;
                lr[e] = __builtin_sqrtf(col.x);
                lr[kPmLdsRing + e] = __builtin_sqrtf(col.y);
                lr[2u * kPmLdsRing + e] = __builtin_sqrtf(col.z);
            } else
                wr[g & rmask] = make_float4(__builtin_sqrtf(col.x), __builtin_sqrtf(col.y), __builtin_sqrtf(col.z),
                                            __uint_as_float(ring_tag(S, g)));
            if ((uint32_t)s == mid && f.out_depth) depth_store(f, px.out, dep);  // 01_BVH...glsl:667-668
            busy = false;
        }
    }
#ifdef RT_DIAG_OCC
    if (f.dbg && lane == 0)
        for (int k = 0; k < kOccSlots; k++) atomicAdd(f.dbg + 32 + k, c.occ[k]);
#endif
    flush(f, c);
}


// ============================================================================ launch
uint32_t units_of(const Frame &f) {
    return f.tiles ? (uint32_t)f.n_tiles * f.tile_size * f.tile_size
                   : (uint32_t)(((f.tw + 7) >> 3) * ((f.th + 7) >> 3)) * 64u;
}
static unsigned grid_of(uint32_t units, int blocks_cap) {
    uint64_t b = ((uint64_t)units + kBlock - 1) / kBlock;
    if (b > (uint64_t)blocks_cap) b = blocks_cap;
    return (unsigned)(b ? b : 1);
}
static dim3 grid_iow01(const Frame &f) {
    if (f.tiles) { const int per = f.tile_size >> 4; return dim3((unsigned)(f.n_tiles * per * per)); }
    return dim3((unsigned)(((f.tw + 15) >> 4) * ((f.th + 15) >> 4)));
}

bool iow_narrow(const Frame &f) {  // A/B switch (measured slower: VGPR spills)
    return f.max_bounces <= 255 && f.narrow != 0;
}

// the LDS-node kernels (k_iow03L / k_iow03sL) when the BVH fits and rt_options.iow_lds_bvh is on
bool iow_lds(const IowScene &sc) {
    return sc.lds_on && sc.nodes != nullptr && sc.n_nodes > 0 && sc.n_nodes <= (uint32_t)kIowLdsNodes;
}

int resident_blocks_per_cu(int kind) {
    int nb = 0;
    hipError_t e;
    if (kind == 3) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_iow03, kBlock, 0);
    else if (kind == 9) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_iow03L, 3 * kBlock, 0);
    else if (kind == 10) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_iow03sL, 3 * kBlock, 0);
    else if (kind == 4) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_iow03n, kBlock, 0);
    else if (kind == 5) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_iow03s, kBlock, 0);
    else if (kind == 14) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inw<true>, kBlock, 0);
    else if (kind == 15) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inw_pm<false>, kBlock, 0);
    else if (kind == 16) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inw_pm<true>, kBlock, 0);
    else if (kind == 17) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inw_pm<false, true>, 3 * kBlock, 0);
    else if (kind == 18) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inw_pm<true, true>, 3 * kBlock, 0);
    else if (kind == 19)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inw_pm<false, true, true, true, true>, pm_sub<true, true>() * kBlock, 0);
    else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inw<false>, kBlock, 0);
    return (e == hipSuccess && nb > 0) ? nb : 2;
}

hipError_t launch_iow01(const Frame &f, hipStream_t s) {
    hipLaunchKernelGGL(k_iow01, grid_iow01(f), dim3(kBlock), 0, s, f);
    return hipGetLastError();
}
hipError_t launch_iow03(const Frame &f, const IowScene &sc, const Chunk &ch, const Cont &ct, uint32_t n_units,
                        unsigned *counter, int s_stop, int blocks_cap, hipStream_t s) {
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    if (!iow_narrow(f) && iow_lds(sc)) {
        const dim3 g(grid_of((n_units + 2) / 3, blocks_cap / 3));  // blocks_cap counts 256-lane slots
        hipLaunchKernelGGL(k_iow03L, g, dim3(3 * kBlock), 0, s, f, sc, ch, ct, counter, s_stop);
        return hipGetLastError();
    }
    const dim3 g(grid_of(n_units, blocks_cap));
    if (iow_narrow(f)) hipLaunchKernelGGL(k_iow03n, g, dim3(kBlock), 0, s, f, sc, ch, ct, counter, s_stop);
    else hipLaunchKernelGGL(k_iow03, g, dim3(kBlock), 0, s, f, sc, ch, ct, counter, s_stop);
    return hipGetLastError();
}
hipError_t launch_iow03_spec(const Frame &f, const IowScene &sc, const SpecRecs &R, int mode, const Cont &ct,
                             uint32_t n_units, unsigned *counter, int blocks_cap, hipStream_t s) {
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    if (iow_lds(sc))
        hipLaunchKernelGGL(k_iow03sL, dim3(grid_of((n_units + 2) / 3, blocks_cap / 3)), dim3(3 * kBlock), 0, s, f, sc, R,
                           mode, ct, counter);
    else
        hipLaunchKernelGGL(k_iow03s, dim3(grid_of(n_units, blocks_cap)), dim3(kBlock), 0, s, f, sc, R, mode, ct,
                           counter);
    return hipGetLastError();
}
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
__global__ void k_spec_list_keys(SpecRecs R, unsigned *keys, size_t n) {
    const unsigned cnt = *R.list_count;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        keys[i] = i < cnt ? min(R.ctr[R.ix(R.list[i])].x, 0xffffffu) : 0u;
}
hipError_t spec_list_keys(const SpecRecs &R, unsigned *keys, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_list_keys, dim3(4096), dim3(256), 0, s, R, keys, n);
    return hipGetLastError();
}
// ---------------------------------------------------------------- heavy-first enumeration
// cost of sample index s (1..S-1) over the probe pixels: finished records (block s-1)
__global__ __launch_bounds__(kBlock) void k_sample_cost(SpecRecs R, unsigned long long *fcost) {
    __shared__ unsigned long long part[kBlock / 64];
    const uint32_t s = blockIdx.x + 1u;
    const uint32_t n_px = R.order_n ? R.order_n : R.P;
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    unsigned long long acc = 0;
    for (uint32_t i = threadIdx.x; (size_t)i * R.probe_stride < n_px; i += kBlock) {
        const size_t u = (size_t)s * R.P + R.order[R.order_base + i * R.probe_stride];
        if ((__float_as_uint(R.col[R.ix(u)].w) & 0xffff0100u) == done_tag) acc += R.ctr[R.ix(u)].x;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kBlock / 64; w++) t += part[w];
        atomicAdd(fcost + s, t);
    }
}
// progress of the parked lanes (the long samples still running) counts toward their index
__global__ __launch_bounds__(kBlock) void k_sample_cost_parked(SpecRecs R, const float4 *cont, const unsigned *count,
                                                               unsigned long long *fcost) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= *count) return;  // no cross-lane work in this kernel
    const float4 *p = cont + (size_t)i * kContSlots;
    if (p[12].y != 0.0f) return;
    const uint32_t u = __float_as_uint(p[0].x);
    atomicAdd(fcost + u / R.P, (unsigned long long)__float_as_uint(p[2].x));
}
// rank the indices 1..S-1 by cost, most expensive first (ties: lower index first)
__global__ __launch_bounds__(1024) void k_sample_rank(SpecRecs R, const unsigned long long *fcost, uint32_t *sorder) {
    for (uint32_t s = 1u + threadIdx.x; s < R.S; s += 1024u) {
        const unsigned long long c = fcost[s];
        uint32_t rank = 0;
        for (uint32_t t = 1; t < R.S; t++) rank += (fcost[t] > c || (fcost[t] == c && t < s)) ? 1u : 0u;
        sorder[rank] = s;
    }
}
// per pixel: the most rays among its heavy samples (finished records), for the re-sort
__global__ __launch_bounds__(kBlock) void k_pixel_key(Frame f, SpecRecs R, unsigned *key) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n_px = R.order_n ? R.order_n : R.P;
    if (i >= n_px) return;  // no cross-lane work in this kernel
    const uint32_t pu = R.order[R.order_base + i];
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    unsigned k = R.ctr[R.ix(pu)].x;  // sample 0
    for (uint32_t j = 0; j < R.n_heavy; j++) {
        const size_t u = (size_t)R.sorder[j] * R.P + pu;
        if ((__float_as_uint(R.col[R.ix(u)].w) & 0xffff0100u) == done_tag) k = max(k, R.ctr[R.ix(u)].x);
    }
    key[pu] = unit_pixel(f, pu).in_image ? k : 0u;
}
__global__ __launch_bounds__(kBlock) void k_pixel_key_parked(SpecRecs R, const float4 *cont, const unsigned *count,
                                                             unsigned *key) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= *count) return;  // no cross-lane work in this kernel
    const float4 *p = cont + (size_t)i * kContSlots;
    if (p[12].y != 0.0f) return;
    const uint32_t u = __float_as_uint(p[0].x);
    atomicMax(key + u % R.P, __float_as_uint(p[2].x));
}
hipError_t launch_iow03_sample_order(const Frame &f, const SpecRecs &R, const float4 *cont, const unsigned *count,
                                     int max_lanes, unsigned long long *fcost, uint32_t *sorder, hipStream_t s) {
    hipError_t e = hipMemsetAsync(fcost, 0, sizeof(unsigned long long) * R.S, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sample_cost, dim3(R.S - 1u), dim3(kBlock), 0, s, R, fcost);
    const unsigned blocks = (unsigned)((max_lanes + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_sample_cost_parked, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, R, cont, count, fcost);
    hipLaunchKernelGGL(k_sample_rank, dim3(1), dim3(1024), 0, s, R, fcost, sorder);
    return hipGetLastError();
}
hipError_t launch_iow03_pixel_key(const Frame &f, const SpecRecs &R, const float4 *cont, const unsigned *count,
                                  int max_lanes, unsigned *key, hipStream_t s) {
    const uint32_t n_px = R.order_n ? R.order_n : R.P;
    hipLaunchKernelGGL(k_pixel_key, dim3((n_px + kBlock - 1) / kBlock), dim3(kBlock), 0, s, f, R, key);
    const unsigned blocks = (unsigned)((max_lanes + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_pixel_key_parked, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, R, cont, count, key);
    return hipGetLastError();
}
hipError_t launch_iow03_frontier(const Frame &f, const SpecRecs &R, float4 *cont, unsigned *count, uint32_t cap,
                                 hipStream_t s) {
    const uint32_t n = R.order_n ? R.order_n : R.P;
    hipLaunchKernelGGL(k_iow03_frontier, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, f, R, cont, count, cap);
    return hipGetLastError();
}
hipError_t launch_iow03_altspawn(const Frame &f, const SpecRecs &R, float4 *cont, unsigned *count, uint32_t cap,
                                 hipStream_t s) {
    const uint32_t n = R.order_n ? R.order_n : R.P;
    const unsigned blocks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_iow03_altspawn, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, f, R, cont, count, cap);
    return hipGetLastError();
}
hipError_t launch_iow03_fixf(const Frame &f, const SpecRecs &R, float4 *cont, const unsigned *count, int max_lanes,
                             hipStream_t s) {
    const unsigned blocks = (unsigned)((max_lanes + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_iow03_fixf, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, f, R, cont, count);
    return hipGetLastError();
}
hipError_t launch_iow03_prep(const Frame &f, const SpecRecs &R, unsigned *key, float prior, uint32_t prior_from,
                             hipStream_t s) {
    const unsigned blocks = (R.P + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_iow03_prep, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, f, R, key, prior, prior_from);
    return hipGetLastError();
}
hipError_t launch_iow03_resolve(const Frame &f, const SpecRecs &R, bool final_pass, float4 *state, hipStream_t s) {
    const unsigned blocks = ((R.order_n ? R.order_n : R.P) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_iow03_resolve, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, f, R, final_pass ? 1 : 0, state);
    return hipGetLastError();
}
hipError_t launch_inw_beam(const Frame &f, const InwScene &sc, const uint32_t *mode, uint32_t force, hipStream_t s) {
    const uint32_t n = units_of(f);
    const uint32_t nb = sc.beam_bins > 1u ? sc.beam_bins : 1u;
    hipLaunchKernelGGL(k_inw_beam, dim3((n + kBeamBlock - 1) / kBeamBlock, nb), dim3(kBeamBlock), 0, s, f, sc, mode, force);
    return hipGetLastError();
}
size_t inw_cost_uints(uint32_t nblk) { return 3 * size_t(nblk) + 256 + kSkyInfo; }
size_t inw_sky_info_at(uint32_t nblk) { return 2 * size_t(nblk) + 256; }
// One frame of the on-chip-fold INW kernels: the probe (unless forced), then k_inw_pm and
// k_inw_sm, of which the one the probe did not pick exits at once.  ring: blocks * 4 waves *
// max(ring_pm, ring_sm) float4; mode: 2 uints (zeroed here).  force: 0 = probe, 1 = pm, 2 = sm.
// sky (needs cost and sc.beam): the sky blocks rendered by k_inw_sky -- the beam lists, the
// classifier and k_inw_sky then come before the claim-order kernels, which put the blocks whose flag
// k_inw_sky left standing at the head of the order, and k_inw_sky_queues starts k_inw_pm's queues
// past them.
hipError_t launch_inw_fold(const Frame &f, const InwScene &sc, float4 *ring, uint32_t ring_pm, uint32_t ring_sm,
                           unsigned *counter, uint32_t *mode, uint32_t force, int blocks, int blocks_ln,
                           uint32_t *cost, bool sky, hipStream_t s) {
    for (uint32_t r : {ring_pm, ring_sm})
        if (r < 64 || (r & (r - 1))) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(mode, 0, 2 * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    // the probe first: the claim-order and beam kernels below read its verdict and exit at once
    // on a sample-major frame
    if (force == 0) {
        const uint32_t nblk = units_of(f) / 64u, waves = 1024u;  // ~1024 probe blocks of 8x8 pixels
        const uint32_t stride = nblk > waves ? nblk / waves : 1u, nw = (nblk + stride - 1u) / stride;
        const dim3 g((nw + 3u) / 4u);
        if (sc.layout == 4) hipLaunchKernelGGL(k_inw_probe<true>, g, dim3(kBlock), 0, s, f, sc, stride, mode);
        else hipLaunchKernelGGL(k_inw_probe<false>, g, dim3(kBlock), 0, s, f, sc, stride, mode);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // claim order of k_inw_pm (cost: 3 * nblk + 256 + kSkyInfo uints -- keys, the order, buckets, the
    // sky blocks' bookkeeping and flags -- or null = unit order)
    const uint32_t *border = nullptr;
    const bool order = cost && units_of(f) >= 64u;
    sky = sky && order && sc.beam;
    if (order) {
        const uint32_t nblk = units_of(f) / 64u;
        uint32_t *key = cost, *ord = cost + nblk, *hist = cost + 2 * nblk, *flag = hist + 256 + kSkyInfo;
        if ((e = hipMemsetAsync(hist, 0, (256 + kSkyInfo) * sizeof(uint32_t), s)) != hipSuccess) return e;
        const dim3 g((nblk + 3u) / 4u);  // 4 blocks of 8x8 pixels per 256-lane block
        if (sky) {
            if ((e = launch_inw_beam(f, sc, mode, force, s)) != hipSuccess) return e;
            hipLaunchKernelGGL(k_inw_sky_classify, g, dim3(kBlock), 0, s, f, sc, flag, hist + 256, mode, force);
            hipLaunchKernelGGL(k_inw_sky, dim3(nblk), dim3(kSkyBlock), 0, s, f, sc, flag, hist + 256);
        }
        const uint32_t *fl = sky ? flag : nullptr;
        if (sc.layout == 4) hipLaunchKernelGGL(k_inw_cost<true>, g, dim3(kBlock), 0, s, f, sc, key, hist, mode, force, fl);
        else hipLaunchKernelGGL(k_inw_cost<false>, g, dim3(kBlock), 0, s, f, sc, key, hist, mode, force, fl);
        hipLaunchKernelGGL(k_inw_order_scan, dim3(1), dim3(256), 0, s, hist, nblk, mode, force);
        hipLaunchKernelGGL(k_inw_order_scatter, dim3((nblk + kBlock - 1) / kBlock), dim3(kBlock), 0, s, key, hist,
                           ord, nblk, mode, force);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        border = ord;
    }
    if (sc.beam && !sky && (e = launch_inw_beam(f, sc, mode, force, s)) != hipSuccess) return e;
    for (int k = 0; k < 2; k++) {  // (pm, then sm) each with its own queue counter
        if ((e = hipMemsetAsync(counter + 16 * k, 0, sizeof(unsigned), s)) != hipSuccess) return e;
        if (k == 0 && sc.xcdq && (e = hipMemsetAsync(counter + 64, 0, 8 * 16 * sizeof(unsigned), s)) != hipSuccess)
            return e;  // k_inw_pm's per-XCD queues
        if (k == 0 && sky) hipLaunchKernelGGL(k_inw_sky_queues, dim3(1), dim3(64), 0, s, cost + inw_sky_info_at(units_of(f) / 64u), counter);
        const uint32_t rm = (k == 0 ? ring_pm : ring_sm) - 1u;
        unsigned *ctr = counter + 16 * k;
        if (blocks_ln > 0) {  // the LDS-staged BVH top (768-lane blocks); FU: the fused-fma cull
            const dim3 g(blocks_ln), b(3 * kBlock);
#define RT_INW_LN_LAUNCH(L, F)                                                                              \
    do {                                                                                                    \
        if (k == 0 && sc.lring) hipLaunchKernelGGL((k_inw_pm<L, true, F, true>), g, b, 0, s, f, sc, ring, rm, ctr, mode, force, border); \
        else if (k == 0) hipLaunchKernelGGL((k_inw_pm<L, true, F>), g, b, 0, s, f, sc, ring, rm, ctr, mode, force, border); \
        else if (sc.lring_sm) hipLaunchKernelGGL((k_inw_sm<L, true, F, true>), g, b, 0, s, f, sc, ring, rm, ctr, mode, force, border); \
        else hipLaunchKernelGGL((k_inw_sm<L, true, F>), g, b, 0, s, f, sc, ring, rm, ctr, mode, force, border);        \
    } while (0)
            if (k == 0 && sc.layout != 4 && sc.fused && sc.lring && sc.gstk && sc.gq_blocks)  // GQ
                hipLaunchKernelGGL((k_inw_pm<false, true, true, true, true>), dim3(sc.gq_blocks),
                                   dim3(pm_sub<true, true>() * kBlock), 0, s, f, sc, ring, rm, ctr, mode, force, border);
            else if (sc.layout == 4) {
                if (sc.fused) RT_INW_LN_LAUNCH(true, true);
                else RT_INW_LN_LAUNCH(true, false);
            } else {
                if (sc.fused) RT_INW_LN_LAUNCH(false, true);
                else RT_INW_LN_LAUNCH(false, false);
            }
#undef RT_INW_LN_LAUNCH
        } else if (sc.layout == 4) {
            if (k == 0) hipLaunchKernelGGL(k_inw_pm<true>, dim3(blocks), dim3(kBlock), 0, s, f, sc, ring, rm, counter, mode, force, border);
            else hipLaunchKernelGGL(k_inw_sm<true>, dim3(blocks), dim3(kBlock), 0, s, f, sc, ring, rm, counter + 16, mode, force, border);
        } else {
            if (k == 0) hipLaunchKernelGGL(k_inw_pm<false>, dim3(blocks), dim3(kBlock), 0, s, f, sc, ring, rm, counter, mode, force, border);
            else hipLaunchKernelGGL(k_inw_sm<false>, dim3(blocks), dim3(kBlock), 0, s, f, sc, ring, rm, counter + 16, mode, force, border);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t launch_inw(const Frame &f, const InwScene &sc, const Chunk &ch, const Cont &ct, uint32_t n_units,
                      unsigned *counter, int blocks_cap, hipStream_t s) {
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const dim3 g(grid_of(n_units, blocks_cap));
    if (sc.layout == 4) hipLaunchKernelGGL(k_inw<true>, g, dim3(kBlock), 0, s, f, sc, ch, ct, counter);
    else hipLaunchKernelGGL(k_inw<false>, g, dim3(kBlock), 0, s, f, sc, ch, ct, counter);
    return hipGetLastError();
}

}  // namespace rtk

namespace rtk {
// The shortened sequences of rt_math.hpp against the compiler's correctly rounded ones over
// every bit pattern x (NaN == NaN): which 0 = rcp_sqrt_domain(sqrt(x)) vs 1.0f / sqrt(x).
// (An unscaled sqrt candidate failed here for 20.7M inputs, the denormal and tiny ones.)
__global__ __launch_bounds__(kBlock) void k_check_fastmath(int which, unsigned long long *bad, unsigned *first) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < (1ull << 32); i += stride) {
        const float xi = __uint_as_float((uint32_t)i);
        (void)which;
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
