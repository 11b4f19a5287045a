// rt_pixels.hip -- pixel queries: the shaders' camera rays and pixel folds as kernels of their own
// (rt_camera_rays_async, rt_pixel_query_async).
//
// k_camera_rays writes, per (pixel, sample), the ray the render kernels push for it, as a path-query
// record: INW by the render's own sample start (inw_start_sample, rt_inw_shade.hpp: out_Pixel's
// prologue, 01_BoundingVolumeHierarchy/computeShaderSrc.glsl:366-410, single focus), IOW-03 by
// iow_camera_ray and the pixel's scalars (rt_iow_shade.hpp: 03_Shadows_and_Materials/
// computeShaderSrc.glsl:370-406).  k_pixel_fold folds the path queries' answers of a pixel as the
// render kernels fold its samples: End() (01_BVH...glsl:625-675) and out_Pixel's mean (03...glsl:383-417).
// Between the two runs the unchanged path kernel, so a pixel query is the render's pixel bit for bit.
#include "rt_inw_shade.hpp"
#include "rt_iow_shade.hpp"

namespace rtk {

// What inw_start_sample_cd pushes through instead of a stack: it keeps the camera ray.
struct RayCatch {
    f3 o = f3{0, 0, 0}, d = f3{0, 0, 0};
    __device__ __forceinline__ void reset(int) {}
    __device__ __forceinline__ void push(float, Ctr &) {}
    __device__ __forceinline__ void push_ray(f3 o_, f3 d_, float, float, Ctr &) { o = o_; d = d_; }
};

template <bool IOW> struct PixelScene { using type = InwScene; };
template <> struct PixelScene<true> { using type = IowScene; };

// One lane per record: record i is sample s0 + i % ns of pixel pixels[i / ns].  A record is 2 float4
// (rt_path_ray: origin, sample | direction, pad) or 3 (rt_path_iow_ray: ... | ri_in = 0); the lanes of
// a wave store to consecutive records.  A pixel outside the image, a sample index >= spp and an IOW-03
// sample at the ring schedule's early-return marker (03...glsl:396) give sample = 0xffffffff and zeros.
// INW: the pixel's direction is recomputed per lane (inw_pixel_dir inside inw_start_sample), the
// render's own call.  n <= 2^31.
template <bool IOW>
__global__ __launch_bounds__(kBlock)
void k_camera_rays(Frame F, typename PixelScene<IOW>::type S, const int2 *__restrict__ pixels, uint32_t n, uint32_t s0,
                   uint32_t ns, float4 *__restrict__ rays) {
    constexpr uint32_t kRec = IOW ? 3u : 2u;
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = i / ns, j = i - k * ns;
    const int2 px = pixels[k];
    const uint32_t spp = (uint32_t)F.spp;
    bool ok = px.x >= 0 && px.x < F.W && px.y >= 0 && px.y < F.H && s0 < spp && j < spp - s0;
    const int s = ok ? (int)(s0 + j) : 0;
    f3 o = f3{0, 0, 0}, d = f3{0, 0, 0};
    if constexpr (IOW) {
        if (ok && S.ring[2 * s] < 0) ok = false;  // the early return: the pixel ends before this sample
        if (ok) {
            const int grid = iow_ring_grid(F.spp);
            const float aspect = iow_aspect(F.W, F.H);
            iow_camera_ray(S, F, iow_px_sx(aspect, px.x, F.W), iow_px_sy(px.y, F.H), iow_px_dsx(aspect, F.W, grid),
                           iow_px_dsy(F.H, grid), s, o, d);
        }
    } else {
        if (ok) {
            RayCatch K;
            Ctr c;
            inw_start_sample(S, F, K, px.x, px.y, s, c);
            o = K.o;
            d = K.d;
        }
    }
    float4 *r = rays + (size_t)kRec * i;
    if (ok) {
        r[0] = make_float4(o.x, o.y, o.z, __uint_as_float((uint32_t)s));
        r[1] = make_float4(d.x, d.y, d.z, 0.0f);
    } else {
        r[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
        r[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if constexpr (IOW) r[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// One wave per pixel (four pixels per 256-lane block): a query of a few thousand pixels spreads over
// the chip, and a pixel's records are read 64 samples at a time, one per lane, at consecutive addresses.
constexpr int kFoldPixels = kBlock / 64;

__device__ __forceinline__ float rdl(float v, uint32_t l) {  // lane l's value (l wave-uniform)
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l));
}

// A pixel's spp answers (rt_path_out / rt_path_iow_out, sample order) are at samples + pixel * spp
// records; one rt_pixel_out (rgba | depth, segments, drops, nans) per pixel.  The float additions run
// in sample order in every lane alike -- the order is part of the result -- over values read across
// the wave (k_inw_pm's fold does the same); the loads, the square roots and the counts run a lane per
// sample.
//   INW: End() as the render kernels fold it -- the first sample's sqrt(colour) assigned, the others
//   added, times RN(1 / spp); the depth of sample spp / 2.
//   IOW-03: out_Pixel's sum from 0 in sample order, times RN(1 / spp); the first status = 1 answer is
//   the ring schedule's early return at sample s: the pixel is the sum so far times RN(1 / s), as
//   k_iow03 writes it (s = 0 cannot be reached through rt_sample_tables' schedule; it would give 0 * inf).
// A pixel outside the image gives zeros, as the renders write them.
template <bool IOW>
__global__ __launch_bounds__(kBlock)
void k_pixel_fold(Frame F, const int2 *__restrict__ pixels, uint32_t n_pixels, const float4 *__restrict__ samples,
                  float4 *__restrict__ out) {
    constexpr uint32_t kRec = IOW ? 3u : 2u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = blockIdx.x * (uint32_t)kFoldPixels + (threadIdx.x >> 6);  // wave-uniform
    if (k >= n_pixels) return;
    const int2 px = pixels[k];
    if (!(px.x >= 0 && px.x < F.W && px.y >= 0 && px.y < F.H)) {
        if (lane == 0) {
            out[2 * (size_t)k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            out[2 * (size_t)k + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        return;
    }
    const float4 *a = samples + (size_t)k * (size_t)F.spp * kRec;
    const uint32_t spp = (uint32_t)F.spp, mid = spp / 2u;
    unsigned long long seg = 0, drops = 0, nans = 0;  // this lane's samples
    f3 acc = f3{0, 0, 0};
    float dmid = 0.0f;
    uint32_t s_end = spp;  // IOW-03: the sample the pixel stopped at
    for (uint32_t base = 0; base < s_end; base += 64u) {
        const uint32_t s = base + lane;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
        if (s < spp) { r0 = a[kRec * (size_t)s]; r1 = a[kRec * (size_t)s + 1]; }
        uint32_t n = spp - base < 64u ? spp - base : 64u;  // samples of this round (wave-uniform)
        f3 g = f3{r0.x, r0.y, r0.z};
        if constexpr (IOW) {
            const unsigned long long stop = __ballot(s < spp && __float_as_uint(r1.w) != 0u);
            if (stop) { n = (uint32_t)__ffsll((long long)stop) - 1u; s_end = base + n; }
        } else {
            g = f3{__builtin_sqrtf(r0.x), __builtin_sqrtf(r0.y), __builtin_sqrtf(r0.z)};
            if (mid >= base && mid < base + 64u) dmid = rdl(r0.w, mid - base);
        }
        if (lane < n) {
            seg += __float_as_uint(r1.x);
            drops += __float_as_uint(r1.y);
            nans += __float_as_uint(r1.z);
        }
        uint32_t j = 0;
        if (!IOW && base == 0u) { acc = f3{rdl(g.x, 0u), rdl(g.y, 0u), rdl(g.z, 0u)}; j = 1; }
        for (; j < n; j++) acc = acc + f3{rdl(g.x, j), rdl(g.y, j), rdl(g.z, j)};
    }
    seg = wave_sum(seg); drops = wave_sum(drops); nans = wave_sum(nans);
    if (lane != 0) return;
    const f3 c = acc * rcp((float)(IOW ? s_end : spp));
    out[2 * (size_t)k] = make_float4(c.x, c.y, c.z, 1.0f);
    out[2 * (size_t)k + 1] = make_float4(dmid, __uint_as_float((uint32_t)seg), __uint_as_float((uint32_t)drops),
                                         __uint_as_float((uint32_t)nans));
}

hipError_t pixels_kernel_info(int which, int info[4]) {
    switch (which) {
        case 0: return kernel_info(k_camera_rays<false>, occupancy_of(k_camera_rays<false>, kBlock), info);
        case 1: return kernel_info(k_camera_rays<true>, occupancy_of(k_camera_rays<true>, kBlock), info);
        case 2: return kernel_info(k_pixel_fold<false>, occupancy_of(k_pixel_fold<false>, kBlock), info);
        case 3: return kernel_info(k_pixel_fold<true>, occupancy_of(k_pixel_fold<true>, kBlock), info);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_camera_rays(const Frame &f, const InwScene &sc, const int2 *pixels, uint32_t n, uint32_t s0,
                              uint32_t ns, float4 *rays, hipStream_t s) {
    const dim3 g((n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock), b(kBlock);  // n <= 2^31: 2^23 blocks at most
    hipLaunchKernelGGL((k_camera_rays<false>), g, b, 0, s, f, sc, pixels, n, s0, ns, rays);
    return hipGetLastError();
}

hipError_t launch_camera_rays(const Frame &f, const IowScene &sc, const int2 *pixels, uint32_t n, uint32_t s0,
                              uint32_t ns, float4 *rays, hipStream_t s) {
    const dim3 g((n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock), b(kBlock);
    hipLaunchKernelGGL((k_camera_rays<true>), g, b, 0, s, f, sc, pixels, n, s0, ns, rays);
    return hipGetLastError();
}

hipError_t launch_pixel_fold(const Frame &f, bool iow, const int2 *pixels, uint32_t n_pixels, const float4 *samples,
                             float4 *out, hipStream_t s) {
    const dim3 g((n_pixels + (uint32_t)kFoldPixels - 1u) / (uint32_t)kFoldPixels), b(kBlock);
    if (iow) hipLaunchKernelGGL((k_pixel_fold<true>), g, b, 0, s, f, pixels, n_pixels, samples, out);
    else hipLaunchKernelGGL((k_pixel_fold<false>), g, b, 0, s, f, pixels, n_pixels, samples, out);
    return hipGetLastError();
}

}  // namespace rtk
