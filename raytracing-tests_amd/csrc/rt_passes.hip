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
// units with one atomic and hands them to its free lanes by ballot and mbcnt.  The loop is
// iow_pass_loop (rt_pass_loop.hpp), which the adaptive passes' k_iow_adapt runs too; this kernel gives it
// the source that renders [s0, s1) of every unit of the rectangle.
// INW: the first form, a fused kernel of the same mould (k_inw_pass: a lane owned a pixel for the whole
// pass and ran its samples one after the other), took twice the time of the composition below on the
// C3 frame (DESIGN.md 5.13 has both numbers).  So an INW pass is three launches per chunk of samples:
// k_pass_rays writes the render's own camera rays of (unit, sample) as path queries, unit-major, into
// the scene's pass workspace; the unchanged path kernel (k_inw_paths) answers them, every sample on a
// lane of its own; k_pass_fold folds a pixel's answers into its state in sample order and writes the
// image.  What the two INW kernels share with the adaptive passes' pair (the record writer, the fold's start
// from the state, the image write) is in rt_pass_common.hpp.
// Units map to pixels by unit_pixel: 8x8 blocks of the rectangle.
// Every kernel has a second instance, TL, for rt_render_pass_tiles_async: its units are those of a packed tile
// list (tile-major, 8x8 blocks inside a tile), state and image are indexed by slot, and a slot outside the
// image gets no path, keeps its state bytes and has the zero image written.  The rectangle instances drop
// the list (pass_frame) and keep their code.
#include "rt_pass_loop.hpp"

namespace rtk {

// One lane per record: record u * ns + j is the camera ray of sample s0 + j of unit u's pixel
// (pass_ray_record); a unit past the rectangle's edge gets the invalid sample.  n = units * ns <= 2^31.
template <bool TL>
__global__ __launch_bounds__(kBlock)
void k_pass_rays(Frame Fin, InwScene S, uint32_t s0, uint32_t ns, uint32_t n, float4 *__restrict__ rays) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= n) return;
    Frame F{};
    pass_frame_of<TL>(F, Fin);
    const uint32_t u = i / ns, j = i - u * ns;
    const UnitPix p = pass_unit_pixel<TL>(F, u);
    float4 *r = rays + 2 * (size_t)i;
    if (p.in_image) pass_ray_record(S, F, p.x, p.y, s0 + j, r);
    else pass_no_record(r);
}

// One lane per unit: End() over the unit's ns answers (rt_path_out: rgb, depth | ...) in sample order,
// from the pixel's state (pass_fold_begin) -- sqrt(colour) added, the depth of sample spp / 2 -- and the
// state back: the first float4 of the pixel's rt_pass_state.
// k > 0: the chunk is the pass's last, and the image acc * RN(1 / k) and the depth are written (TL: and the
// zero image of the slots outside the image).
template <bool TL>
__global__ __launch_bounds__(kBlock)
void k_pass_fold(Frame Fin, uint32_t s0, uint32_t ns, uint32_t k, uint32_t n_units, const float4 *__restrict__ out,
                 float4 *__restrict__ state) {
    const uint32_t u = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (u >= n_units) return;
    Frame F{};
    pass_frame_of<TL>(F, Fin);
    const UnitPix p = pass_unit_pixel<TL>(F, u);
    if (!p.in_image) {
        if (TL && k != 0) pass_write_outside(F, p.out);
        return;
    }
    const uint32_t mid = (uint32_t)F.spp / 2u;
    f3 acc;
    float dmid;
    pass_fold_begin(state, p.out, s0, acc, dmid);
    const float4 *a = out + 2 * (size_t)u * ns;
    for (uint32_t j = 0; j < ns; j++) {
        const float4 r = a[2 * (size_t)j];
        const f3 g = f3{__builtin_sqrtf(r.x), __builtin_sqrtf(r.y), __builtin_sqrtf(r.z)};
        acc = sel(s0 + j == 0, g, acc + g);
        if (s0 + j == mid) dmid = r.w;
    }
    state[2 * p.out] = make_float4(acc.x, acc.y, acc.z, dmid);
    if (k == 0) return;
    pass_write_image(F, p.out, acc, rcp((float)k), dmid);
}

// The shared loop over the rectangle's units, every pixel from s0 to s1.
// s1 <= the scene's s_stop (the ring schedule's early return).  s0 >= s1 (a pass that begins at or
// past the early return) renders nothing: the state stays and the image is written from it.
template <bool LN, bool TL>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kPassIowWaves<LN>)))
void k_iow_pass(Frame Fin, IowScene S, uint32_t s0, uint32_t s1, float4 *__restrict__ state, unsigned *queue,
                uint32_t rounds, uint32_t n_units) {
    iow_pass_loop<LN>(Fin, S, UniformPassOf<TL>{s0, s1, rcp((float)s1)}, state, queue, rounds, n_units);
}

namespace {
int g_max_blocks = 0;  // rt_debug_pass_max_blocks: 0 = the resident grid

template <class Kn>
hipError_t pass_info(Kn kernel, int info[4]) {
    return kernel_info(kernel, occupancy_of(kernel, kBlock), info);
}
// resident blocks per CU of the instance a scene runs, asked once each
int iow_pass_blocks(bool ln, bool tl) {
    static const int nb[4] = {occupancy_of(k_iow_pass<false, false>, kBlock), occupancy_of(k_iow_pass<true, false>, kBlock),
                              occupancy_of(k_iow_pass<false, true>, kBlock), occupancy_of(k_iow_pass<true, true>, kBlock)};
    return nb[(tl ? 2 : 0) + (ln ? 1 : 0)];
}
}  // namespace

hipError_t pass_kernel_info(int which, int info[4]) {
    switch (which) {
        case 0: return pass_info(k_pass_rays<false>, info);
        case 1: return pass_info(k_pass_fold<false>, info);
        case 2: return pass_info(k_iow_pass<true, false>, info);
        case 3: return pass_info(k_iow_pass<false, false>, info);
        case 4: return pass_info(k_pass_rays<true>, info);  // the tile-list instances
        case 5: return pass_info(k_pass_fold<true>, info);
        case 6: return pass_info(k_iow_pass<true, true>, info);
        case 7: return pass_info(k_iow_pass<false, true>, info);
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
    if (f.tiles) hipLaunchKernelGGL(k_pass_rays<true>, g, b, 0, s, f, sc, s0, ns, n, rays);
    else hipLaunchKernelGGL(k_pass_rays<false>, g, b, 0, s, f, sc, s0, ns, n, rays);
    return hipGetLastError();
}

hipError_t launch_pass_fold(const Frame &f, uint32_t s0, uint32_t ns, uint32_t k, const float4 *out, float4 *state,
                            hipStream_t s) {
    const uint32_t n_units = units_of(f);
    const dim3 g((n_units + (uint32_t)kBlock - 1u) / (uint32_t)kBlock), b(kBlock);
    if (f.tiles) hipLaunchKernelGGL(k_pass_fold<true>, g, b, 0, s, f, s0, ns, k, n_units, out, state);
    else hipLaunchKernelGGL(k_pass_fold<false>, g, b, 0, s, f, s0, ns, k, n_units, out, state);
    return hipGetLastError();
}

hipError_t launch_iow_pass(const Frame &f, const IowScene &sc, uint32_t s0, uint32_t s1, float4 *state,
                           unsigned *queue, int cus, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(queue, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const bool ln = iow_lds(sc);
    const uint32_t n_units = units_of(f);
    const bool tl = f.tiles != nullptr;
    const ClaimGrid cg = claim_grid(n_units, cus, iow_pass_blocks(ln, tl), g_max_blocks);
    const dim3 g(cg.grid), b(kBlock);
    if (tl && ln) hipLaunchKernelGGL((k_iow_pass<true, true>), g, b, 0, s, f, sc, s0, s1, state, queue, cg.rounds, n_units);
    else if (tl) hipLaunchKernelGGL((k_iow_pass<false, true>), g, b, 0, s, f, sc, s0, s1, state, queue, cg.rounds, n_units);
    else if (ln) hipLaunchKernelGGL((k_iow_pass<true, false>), g, b, 0, s, f, sc, s0, s1, state, queue, cg.rounds, n_units);
    else hipLaunchKernelGGL((k_iow_pass<false, false>), g, b, 0, s, f, sc, s0, s1, state, queue, cg.rounds, n_units);
    return hipGetLastError();
}

}  // namespace rtk
