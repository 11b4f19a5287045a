// rt_inw_render.hip -- the per-pixel In-Next-Week render kernel for gfx950 and its launch: one
// thread per pixel on the persistent work queue (rt_render_common.hpp), a ray segment per iteration.
//
//   k_inw <- In-Next-Week/01_BoundingVolumeHierarchy/computeShaderSrc.glsl:230-675 (LIGHTS=false)
//            In-Next-Week/04_Lights_Camera_And_Action/computeShaderSrc.glsl:243-773 (LIGHTS=true)
// (paths relative to the reference's Raytracing-Sandbox/Src/)
#include "rt_render_common.hpp"
#include "rt_inw_shade.hpp"
#include "rt_iow_walk.hpp"  // DBG_TALLY

namespace rtk {

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

// ============================================================================ launch
int inw_render_blocks_per_cu(RenderKernel k) {
    return k == RenderKernel::Inw04 ? occupancy_of(k_inw<true>, kBlock) : occupancy_of(k_inw<false>, kBlock);
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
