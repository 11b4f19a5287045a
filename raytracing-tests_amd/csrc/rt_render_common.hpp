// rt_render_common.hpp -- what the render units share (rt_iow_render.hip, rt_iow_spec.hip,
// rt_inw_render.hip, rt_inw_fold.hip): the pixel mappings, the persistent work queue's
// wave-aggregated claims, the counter flush, and the launch side's grid size (the occupancy query is
// rt_kernels.hpp's occupancy_of).
//
// One thread renders one pixel and walks its samples in order, exactly like the
// reference's invocation (IOW) or workgroup (INW) does, so the per-pixel reduction order
// is the reference's sequential one.  A 256-thread block covers a 16x16 pixel tile with
// each wave on an 8x8 quadrant (coherent camera rays).  Per-thread ray / node stacks live
// in LDS in a [slot][thread] layout: lane l of a wave touches bank (l mod 32) whatever the
// stack depth, so divergent stack pointers never conflict.
#pragma once
#include "rt_kernels.hpp"
#include "rt_math.hpp"
#include "rt_inw_walk.hpp"  // Ctr

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

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
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

// ============================================================================ launch
static unsigned grid_of(uint32_t units, int blocks_cap) {
    uint64_t b = ((uint64_t)units + kBlock - 1) / kBlock;
    if (b > (uint64_t)blocks_cap) b = blocks_cap;
    return (unsigned)(b ? b : 1);
}

}  // namespace rtk
