// rt_iow_render.hip -- the In-One-Weekend render kernels for gfx950 (CDNA4, wave64): IOW-01 and
// the sequential IOW-03 kernels, one thread per pixel walking its samples in order
// (rt_render_common.hpp), and their launches.
//
// Kernels and the shaders they replace (paths relative to the reference's Raytracing-Sandbox/Src/):
//   k_iow01 <- In-One-Weekend/01_Adding_Sphere/computeShaderSrc.glsl:98-146
//   k_iow03 <- In-One-Weekend/03_Shadows_and_Materials/computeShaderSrc.glsl:196-430
#include "rt_render_common.hpp"
#include "rt_iow_coop.hpp"

namespace rtk {

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

// ============================================================================ launch
uint32_t units_of(const Frame &f) {
    return f.tiles ? (uint32_t)f.n_tiles * f.tile_size * f.tile_size
                   : (uint32_t)(((f.tw + 7) >> 3) * ((f.th + 7) >> 3)) * 64u;
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

int iow_render_blocks_per_cu(RenderKernel k) {
    if (k == RenderKernel::Iow03Lds) return occupancy_of(k_iow03L, 3 * kBlock);
    if (k == RenderKernel::Iow03Narrow) return occupancy_of(k_iow03n, kBlock);
    return occupancy_of(k_iow03, kBlock);
}
// every render kernel's occupancy, asked of the unit that owns the kernel
int resident_blocks_per_cu(RenderKernel k) {
    switch (k) {
    case RenderKernel::Iow03: case RenderKernel::Iow03Narrow: case RenderKernel::Iow03Lds:
        return iow_render_blocks_per_cu(k);
    case RenderKernel::Iow03Spec: case RenderKernel::Iow03SpecLds:
        return iow_spec_blocks_per_cu(k);
    case RenderKernel::Inw01: case RenderKernel::Inw04:
        return inw_render_blocks_per_cu(k);
    case RenderKernel::InwPm01: case RenderKernel::InwPm04: case RenderKernel::InwPmLn01:
    case RenderKernel::InwPmLn04: case RenderKernel::InwPmGq:
        return inw_fold_blocks_per_cu(k);
    }
    return 2;  // not an enumerator: the answer of a failed query
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

}  // namespace rtk
