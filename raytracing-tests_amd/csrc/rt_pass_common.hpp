// rt_pass_common.hpp -- what the pass units share (rt_passes.hip, rt_adaptive.hip): the camera-ray catcher of
// inw_start_sample and the frame as the pass kernels rebuild it.
#pragma once
#include "rt_render_common.hpp"

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
// ... and what a segment reads (k_inw_paths' and k_iow_paths' frames)
__device__ __forceinline__ void pass_seg_frame(Frame &F, const Frame &in) {
    F.max_bounces = in.max_bounces;
    F.inv_spp = in.inv_spp;
    F.dir[0] = in.dir[0]; F.dir[1] = in.dir[1]; F.dir[2] = in.dir[2];
    F.leaf_batch = in.leaf_batch;
}

}  // namespace rtk
