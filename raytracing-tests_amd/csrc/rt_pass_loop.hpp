// rt_pass_loop.hpp -- the IOW-03 pass loop, shared by k_iow_pass (rt_passes.hip) and k_iow_adapt
// (rt_adaptive.hip): the path-query kernel (rt_path_iow.hip) with the camera ray and the fold moved inside.
// A persistent grid, a lane owns one pixel at a time, a wave claims 64 * rounds consecutive units with one
// atomic and hands them to its free lanes by ballot and mbcnt.  What the two kernels differ in comes from a
// source object: which pixel a unit is, the sample a lane starts and stops at, the divisor of the image,
// and whether `even` is folded beside the sum.
#pragma once
#include "rt_pass_common.hpp"
#include "rt_iow_shade.hpp"

namespace rtk {

// Waves per SIMD, the IOW-03 path kernel's (kPathIowWaves): bound by LDS, 2 blocks per CU with the
// nodes staged, 3 without.  DESIGN.md 5.13 has the table.
template <bool LN> constexpr int kPassIowWaves = LN ? 2 : 3;

// Every unit of the frame's rectangle (unit_pixel) renders samples [s0, s1); the image is acc * inv_k.
// All its answers are wave-uniform: none reads a lane's own sample or last sample.
// TL: the units are those of the frame's packed tile list (rt_render_pass_tiles_async) and the state and
// image are indexed by slot; a slot outside the image gets the zero image the tile renders write.
template <bool TL>
struct UniformPassOf {
    static constexpr bool kEven = false;
    uint32_t s0, s1;
    float inv_k;
    __device__ __forceinline__ void frame(Frame &F, const Frame &in) const { pass_frame_of<TL>(F, in); }
    __device__ __forceinline__ UnitPix pixel(const Frame &F, uint32_t u) const { return pass_unit_pixel<TL>(F, u); }
    __device__ __forceinline__ void outside(const Frame &F, const UnitPix &p) const {
        if (TL) pass_write_outside(F, p.out);
    }
    __device__ __forceinline__ uint32_t first(size_t, f3 &) const { return s0; }
    __device__ __forceinline__ bool fresh(uint32_t) const { return s0 == 0; }
    __device__ __forceinline__ bool left(uint32_t) const { return s0 < s1; }
    __device__ __forceinline__ uint32_t last(uint32_t) const { return s1; }
    __device__ __forceinline__ uint32_t last_of(uint32_t) const { return s1; }
    __device__ __forceinline__ float inv(uint32_t) const { return inv_k; }
    __device__ __forceinline__ void keep(size_t, f3, uint32_t) const {}
};
using UniformPass = UniformPassOf<false>;

// What the two list sources share: an entry's pixel renders samples [count, min(count + ns, stop)), count =
// its aux's (aux: even.xyz, the count's bits), folds `even` and leaves even and the new count behind; the
// image is acc * RN(1 / count).  A skipped entry writes nothing.
struct CountedPass {
    static constexpr bool kEven = true;
    float4 *__restrict__ aux;
    uint32_t stop, ns;
    __device__ __forceinline__ void outside(const Frame &, const UnitPix &) const {}
    __device__ __forceinline__ uint32_t first(size_t out, f3 &ev) const {
        const float4 x = aux[out];
        ev = f3{x.x, x.y, x.z};
        return __float_as_uint(x.w);
    }
    __device__ __forceinline__ bool fresh(uint32_t s) const { return s == 0; }
    __device__ __forceinline__ bool left(uint32_t s) const { return s < stop; }
    __device__ __forceinline__ uint32_t last(uint32_t s) const { return ns < stop - s ? s + ns : stop; }
    __device__ __forceinline__ uint32_t last_of(uint32_t s1) const { return s1; }
    __device__ __forceinline__ float inv(uint32_t s) const { return rcp((float)s); }
    __device__ __forceinline__ void keep(size_t out, f3 ev, uint32_t s) const {
        aux[out] = make_float4(ev.x, ev.y, ev.z, __uint_as_float(s));
    }
};

// Unit u is list entry u, a pixel of the image; state, aux and image are indexed by y * W + x.
struct ListPass : CountedPass {
    const int2 *__restrict__ pixels;
    __device__ ListPass(const int2 *px, float4 *aux_, uint32_t stop_, uint32_t ns_)
        : CountedPass{aux_, stop_, ns_}, pixels(px) {}
    __device__ __forceinline__ void frame(Frame &F, const Frame &in) const { pass_frame(F, in); }
    __device__ __forceinline__ UnitPix pixel(const Frame &F, uint32_t u) const {
        const int2 p = pixels[u];
        UnitPix q;
        q.x = p.x; q.y = p.y;
        q.in_image = listed(F, p);
        q.out = (size_t)((uint32_t)p.y * (uint32_t)F.W + (uint32_t)p.x);
        return q;
    }
};

// The same on a packed tile list (rt_render_pass_slots_async): unit u is slot entry u (slot_pixel), and state,
// aux and image are indexed by slot.  The zero image of the slots outside the image stays the uniform tile
// pass's business.
struct SlotPass : CountedPass {
    const uint32_t *__restrict__ slots;
    __device__ SlotPass(const uint32_t *sl, float4 *aux_, uint32_t stop_, uint32_t ns_)
        : CountedPass{aux_, stop_, ns_}, slots(sl) {}
    __device__ __forceinline__ void frame(Frame &F, const Frame &in) const { pass_frame_tiles(F, in); }
    __device__ __forceinline__ UnitPix pixel(const Frame &F, uint32_t u) const { return slot_pixel(F, slots[u]); }
};

// state: 2 float4 per pixel of the image (rt_pass_state: the sum | the RI fields of the four ray-stack
// slots), read when a pixel does not start at sample 0 and left as the state after its last sample.  A
// pixel with nothing left to render has its image rewritten from its state as it is.  n_units < 2^31.
template <bool LN, class Src>
__device__ __forceinline__ void iow_pass_loop(const Frame &Fin, const IowScene &S, const Src &src,
                                              float4 *__restrict__ state, unsigned *queue, uint32_t rounds,
                                              uint32_t n_units) {
    Frame F{}, Fs{};
    src.frame(F, Fin);
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
    uint32_t next = 0, end = 0;  // the wave's claimed range not handed out yet (wave-uniform)
    bool drained = false;        // the queue is empty (wave-uniform)
    bool busy = false;           // the lane owns a pixel: samples [s, s1) are left
    bool walking = false;        // ... and sample s's path is under way
    uint32_t s = 0, s1 = 0, out = 0;  // out = y * W + x, or the slot, < 2^31
    int skip = 0;
    float sx = 0.0f, sy = 0.0f;
    f3 fc = f3{0, 0, 0}, ev = f3{0, 0, 0}, col = f3{0, 0, 0};
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
                end = n_units - base < 64u * rounds ? n_units : base + 64u * rounds;
            }
            const uint32_t avail = end - next, want = (uint32_t)__popcll(free);
            const uint32_t rank = lanes_below(free);
            if (!busy && rank < avail) {
                const UnitPix p = src.pixel(F, next + rank);
                if (p.in_image) {  // a unit outside the image: the lane stays free
                    out = (uint32_t)p.out;
                    s = src.first(out, ev);
                    fc = f3{0, 0, 0};
                    if (src.fresh(s)) {
                        if (Src::kEven) ev = f3{0, 0, 0};
                        for (int e = 0; e < kIowStack; e++) K.at(e, 7) = 0.0f;  // stale RI slots start at 0
                    } else {
                        const float4 a = state[2 * (size_t)out], r = state[2 * (size_t)out + 1];
                        fc = f3{a.x, a.y, a.z};
                        K.at(0, 7) = r.x; K.at(1, 7) = r.y; K.at(2, 7) = r.z; K.at(3, 7) = r.w;
                    }
                    if (src.left(s)) {
                        s1 = src.last(s);
                        sx = iow_px_sx(aspect, p.x, F.W);
                        sy = iow_px_sy(p.y, F.H);
                        busy = true;
                    } else {  // nothing left to render: the image from the state as it is
                        pass_write_image(F, out, fc, src.inv(s), 0.0f);
                    }
                } else {
                    src.outside(F, p);  // a tile list's slot outside the image: the zero image
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
            if (K.size == 0) {  // sample done: out_Pixel's sum, and the even samples' beside it
                fc = fc + col;
                if (Src::kEven && (s & 1u) == 0) ev = ev + col;
                s++;
                walking = false;
                if (s >= src.last_of(s1)) {
                    state[2 * (size_t)out] = make_float4(fc.x, fc.y, fc.z, 0.0f);
                    state[2 * (size_t)out + 1] = make_float4(K.at(0, 7), K.at(1, 7), K.at(2, 7), K.at(3, 7));
                    src.keep(out, ev, s);
                    pass_write_image(F, out, fc, src.inv(s), 0.0f);
                    busy = false;
                }
            }
        }
    }
    flush(F, c);
}

}  // namespace rtk
