// rt_pass_common.hpp -- what the pass units share (rt_passes.hip, rt_adaptive.hip): the camera-ray catcher of
// inw_start_sample, the frame as the pass kernels rebuild it, a list entry's test, the image write, and for
// the INW pairs (k_pass_rays / k_adapt_rays, k_pass_fold / k_adapt_fold) the record writer and the fold's
// start from the state.  The IOW-03 loop is in rt_pass_loop.hpp.
#pragma once
#include "rt_render_common.hpp"
#include "rt_inw_shade.hpp"

namespace rtk {

// What inw_start_sample pushes through instead of a stack: it keeps the camera ray.
struct PassRay {
    f3 o = f3{0, 0, 0}, d = f3{0, 0, 0};
    __device__ __forceinline__ void reset(int) {}
    __device__ __forceinline__ void push(float, Ctr &) {}
    __device__ __forceinline__ void push_ray(f3 o_, f3 d_, float, float, Ctr &) { o = o_; d = d_; }
};

// The host's frame as the kernels read it, in two parts, each with everything a pass never has (packed
// tiles, MULTIFOCUS, diagnostics) a constant 0, so the code for it goes, as in the path kernels:
// what the pixel mapping, the camera ray and the outputs read ...
__device__ __forceinline__ void pass_frame(Frame &F, const Frame &in) {
    F.W = in.W; F.H = in.H; F.spp = in.spp;
    F.x0 = in.x0; F.y0 = in.y0; F.tw = in.tw; F.th = in.th;
    F.out_rgba = in.out_rgba; F.out_depth = in.out_depth; F.counters = in.counters;
    F.pos[0] = in.pos[0]; F.pos[1] = in.pos[1]; F.pos[2] = in.pos[2];
    F.dir[0] = in.dir[0]; F.dir[1] = in.dir[1]; F.dir[2] = in.dir[2];
    F.aperture = in.aperture; F.focus = in.focus; F.screen_dist = in.screen_dist;
}
// The same with the packed tile list kept: the frame of the tile-list instances (rt_render_pass_tiles_async).
// The rectangle instances never call it, so they keep `tiles` a constant 0 and lose the list's code.
__device__ __forceinline__ void pass_frame_tiles(Frame &F, const Frame &in) {
    pass_frame(F, in);
    F.tiles = in.tiles; F.n_tiles = in.n_tiles; F.tile_size = in.tile_size;
}
template <bool TL>
__device__ __forceinline__ void pass_frame_of(Frame &F, const Frame &in) {
    if (TL) pass_frame_tiles(F, in);
    else pass_frame(F, in);
}
// Unit u's pixel: unit_pixel, which a tile-list instance reads with the list known to be there (units
// tile-major, 8x8 blocks inside a tile; p.out = the slot tile * T * T + iy * T + ix).
template <bool TL>
__device__ __forceinline__ UnitPix pass_unit_pixel(const Frame &F, uint32_t u) {
    if (TL) __builtin_assume(F.tiles != nullptr);
    return unit_pixel(F, u);
}
// ... and what a segment reads (k_inw_paths' and k_iow_paths' frames)
__device__ __forceinline__ void pass_seg_frame(Frame &F, const Frame &in) {
    F.max_bounces = in.max_bounces;
    F.inv_spp = in.inv_spp;
    F.dir[0] = in.dir[0]; F.dir[1] = in.dir[1]; F.dir[2] = in.dir[2];
    F.leaf_batch = in.leaf_batch;
}

// A list entry: inside the image or skipped ({-1, -1} is rt_pass_select_async's padding).
__device__ __forceinline__ bool listed(const Frame &F, int2 p) {
    return p.x >= 0 && p.y >= 0 && p.x < F.W && p.y < F.H;
}

// A list entry of the adaptive passes: a pixel of the image, or, on a packed tile list (TL), a slot
// tile * T * T + iy * T + ix (0xffffffff is rt_pass_select_tiles_async's padding).
template <bool TL> struct PassEntryOf { using type = int2; };
template <> struct PassEntryOf<true> { using type = uint32_t; };
template <bool TL> using PassEntry = typename PassEntryOf<TL>::type;
constexpr uint32_t kSlotNone = 0xffffffffu;

// A slot entry's pixel: handled (in_image) when the slot is below the list's n_tiles * T * T <= 2^31 and its
// pixel lies inside the image; out = the slot.  T need not be a power of two.
__device__ __forceinline__ UnitPix slot_pixel(const Frame &F, uint32_t slot) {
    UnitPix q;
    q.x = q.y = -1;
    q.in_image = false;
    q.out = slot;
    const uint32_t T = (uint32_t)F.tile_size, area = T * T;
    if (slot < (uint32_t)F.n_tiles * area) {
        const uint32_t t = slot / area, r = slot - t * area, iy = r / T, ix = r - iy * T;
        q.x = F.tiles[2 * t] * F.tile_size + (int)ix;
        q.y = F.tiles[2 * t + 1] * F.tile_size + (int)iy;
        q.in_image = listed(F, make_int2(q.x, q.y));
    }
    return q;
}

// The image of a pixel with k samples folded: acc * RN(1 / k), and the depth.
__device__ __forceinline__ void pass_write_image(const Frame &F, size_t o, f3 acc, float inv_k, float depth) {
    if (F.out_rgba) {
        const f3 v = acc * inv_k;
        reinterpret_cast<float4 *>(F.out_rgba)[o] = make_float4(v.x, v.y, v.z, 1.0f);
    }
    if (F.out_depth) F.out_depth[o] = depth;
}

// A packed slot outside the image: (0, 0, 0, 0) and the depth 0, as rt_render_tiles_async writes it.
__device__ __forceinline__ void pass_write_outside(const Frame &F, size_t o) {
    if (F.out_rgba) reinterpret_cast<float4 *>(F.out_rgba)[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (F.out_depth) F.out_depth[o] = 0.0f;
}

// ------------------------------------------------------------------------------------------ INW
// A path-query record (rt_path_ray: origin, sample | direction, pad): the camera ray of sample s of pixel
// (x, y) by the render's own sample start ...
__device__ __forceinline__ void pass_ray_record(const InwScene &S, const Frame &F, int x, int y, uint32_t s, float4 *r) {
    PassRay K;
    Ctr c;
    inw_start_sample(S, F, K, x, y, (int)s, c);
    r[0] = make_float4(K.o.x, K.o.y, K.o.z, __uint_as_float(s));
    r[1] = make_float4(K.d.x, K.d.y, K.d.z, 0.0f);
}
// ... or the record of no sample (0xffffffff), which the path kernel answers without a path.
__device__ __forceinline__ void pass_no_record(float4 *r) {
    r[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
    r[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// Where End()'s fold of the pixel at o starts from sample c: its state (rt_pass_state's first float4: the
// sum, the depth of sample spp / 2), not read when c == 0, where the first sample is assigned.
__device__ __forceinline__ void pass_fold_begin(const float4 *state, size_t o, uint32_t c, f3 &acc, float &dmid) {
    acc = f3{0, 0, 0};
    dmid = 0.0f;
    if (c != 0) {
        const float4 a = state[2 * o];
        acc = f3{a.x, a.y, a.z};
        dmid = a.w;
    }
}

}  // namespace rtk
