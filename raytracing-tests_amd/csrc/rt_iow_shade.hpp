// rt_iow_shade.hpp -- one ray segment of the IOW-03 sample loop as device functions: the scatter
// direction, the 4-entry ray stack, and pop / closest hit / shade / push (LaunchRays,
// 03_Shadows_and_Materials/computeShaderSrc.glsl:258-358).  Included by rt_iow_coop.hpp (the render
// kernels of rt_iow_render.hip and rt_iow_spec.hip) and rt_path_iow.hip (the path-query kernel), so both run the same segment.
#pragma once
#include "rt_iow_walk.hpp"

namespace rtk {

__device__ __forceinline__ f3 fib_dir(float4 t, float s, f3 focus) {
    float x = t.x * s, y = t.y * s, z = t.z * s;
    f3 yc = focus;
    f3 zc = normalize(cross(f3{0, 1.0f, 0}, yc));
    f3 xc = normalize(cross(yc, zc));
    return normalize(focus + ((xc * x + yc * y) + zc * z));
}

__device__ __forceinline__ float schlick(float cosine, float ri) {
    float r0 = (1.0f - ri) * rcp(1.0f + ri);
    r0 = r0 * r0;
    float q = 1.0f - cosine;
    return r0 + (1.0f - r0) * (q * q * q * q * q);
}

// IOW ray stack (03...glsl:258-283): 4 entries of {orig, dirn, contribution, RI, bounces}.
// The entries outlive a sample: the parent-RI lookup (03...glsl:316-319) may read slots above
// the stack top that an earlier sample of the same pixel wrote, so a pixel's samples stay in
// order on one lane and the LDS slots persist across them.
// Two layouts: WIDE keeps `bounced` as a ninth float (any u_NumOfBounce); NARROW keeps it as
// a byte (u_NumOfBounce <= 255), which with a 12-entry BVH stack fits 4 blocks per CU in LDS.
constexpr int kIowStack = 4;
template <bool NARROW>
struct IowStack {
    static constexpr int kSlot = NARROW ? 8 : 9;
    float *base;          // LDS, [slot][thread]
    unsigned char *bb;    // NARROW: LDS, [entry][thread]
    int size;
    // sample-parallel mode: entries written by this sample, and entries whose stale RI this
    // sample read before writing them (its dependence on the previous sample's stack)
    unsigned wmask = 0, rmask = 0;
    __device__ __forceinline__ float &at(int entry, int k) { return base[(entry * kSlot + k) * kBlock]; }
    __device__ __forceinline__ int bounced(int e) {
        if constexpr (NARROW) return bb[e * kBlock];
        else return (int)at(e, 8);
    }
    __device__ __forceinline__ void set_bounced(int e, int b) {
        if constexpr (NARROW) bb[e * kBlock] = (unsigned char)b;
        else at(e, 8) = (float)b;
    }
    __device__ __forceinline__ void push(f3 o, f3 d, float contrib, float ri, int b, Ctr &c) {
        if (size < kIowStack) {
            at(size, 0) = o.x; at(size, 1) = o.y; at(size, 2) = o.z;
            at(size, 3) = d.x; at(size, 4) = d.y; at(size, 5) = d.z;
            at(size, 6) = contrib; at(size, 7) = ri; set_bounced(size, b);
            wmask |= 1u << size;
            size++;
        } else c.drops++;
    }
};

// One ray segment of LaunchRays (03...glsl:285-358): pop, closest hit, shade and push.
struct SegIn { f3 co, cd; float contribution, ri; int bounced; float4 fib; };
template <bool NARROW>
__device__ __forceinline__ SegIn iow_seg_pop(const IowScene &S, IowStack<NARROW> &K, int sidx) {
    K.size--;
    const int e = K.size;
    SegIn in;
    in.fib = reinterpret_cast<const float4 *>(S.fib)[sidx];  // fibonacciHemiSpherePtDirn's point (03...glsl:164-184)
    in.co = mk(K.at(e, 0), K.at(e, 1), K.at(e, 2));
    in.cd = mk(K.at(e, 3), K.at(e, 4), K.at(e, 5));
    in.contribution = K.at(e, 6); in.ri = K.at(e, 7);
    in.bounced = K.bounced(e);
    return in;
}
template <bool NARROW>
__device__ __forceinline__ void iow_seg_shade(const IowScene &S, const Frame &F, IowStack<NARROW> &K, int &skip,
                                              f3 &sample, int sidx, Ctr &c, const SegIn &in, const RayRet &data) {
    const f3 cd = in.cd;
    const float contribution = in.contribution, ri = in.ri;
    int bounced = in.bounced;
    const bool hit = dot(data.normal, data.normal) > 0.9f;
    sample = sample + sel(hit, data.color, background(cd, false)) * contribution;
    if (bounced < F.max_bounces && hit) {
        bounced++;
        bool spawnRefl = false, spawnRefr = false;
        f3 refr_dir = f3{0, 0, 0}, refl_dir = f3{0, 0, 0};
        float cos_t = dot(data.normal, cd);
        float sin_t = __builtin_sqrtf(1.0f - cos_t * cos_t);
        float target_ri;
        {
            int pi = K.size - 1 - skip;
            float parent = (pi < 0) ? 1.0f : (pi < kIowStack ? K.at(pi, 7) : 0.0f);
            target_ri = cos_t > 0.0f ? parent : data.material.z;
            if (cos_t > 0.0f && pi >= 0 && pi < kIowStack && !((K.wmask >> pi) & 1u)) {
                // diagnostics (RT_DEBUG_FIRST_STALE): the segment of the first stale read replaces
                // the unit's drop counter
#ifdef RT_DIAG
                if (F.dbg_first_stale && K.rmask == 0u) c.drops = 0x80000000u | c.seg;
#endif
                K.rmask |= 1u << pi;
            }
        }
        float rr = (ri * rcp(target_ri)) * sin_t;
        float refr_c = data.material.x, refl_c = data.material.y;
        f3 n_ = sel(cos_t > 0.0f, data.normal, -data.normal);
        if (cos_t < 0.0f) {
            refl_dir = fib_dir(in.fib, data.scat1, data.reflected); spawnRefl = true;
            float inc = refr_c * schlick(-cos_t, ri * rcp(target_ri));
            refr_c -= inc; refl_c += inc;
        } else if (rr > 1.0f) {
            refr_dir = data.reflected; spawnRefl = true; refl_c = 1.0f;  // sic (03...glsl:332)
        }
        if (rr <= 1.0f) {
            f3 yc = n_ * cos_t, xc = cd - yc;
            spawnRefr = true;
            refr_dir = n_ * rr + xc * __builtin_sqrtf(1.0f - rr * rr);
            refr_dir = fib_dir(in.fib, data.scat0, refr_dir);
        }
        skip = (spawnRefl && spawnRefr) ? skip - 1 : (spawnRefl ? skip : (spawnRefr ? skip + 1 : 0));
        if (spawnRefl) {
            if (__builtin_isnan(dot(refl_dir, refl_dir))) c.nans++;
            K.push(data.point - n_ * 0.000015f, refl_dir, contribution * refl_c, ri, bounced, c);
        }
        if (spawnRefr) {
            if (__builtin_isnan(dot(refr_dir, refr_dir))) c.nans++;
            K.push(data.point + n_ * 0.000015f, refr_dir, contribution * refr_c, target_ri, bounced, c);
        }
    } else skip = 0;
}
// BS: BVH-stack slots per lane (logical depth BS - 3: 3 spare push slots); NS: node stride
template <bool NARROW, int BS, int NS>
__device__ __forceinline__ void iow_segment(const IowScene &S, const Frame &F, IowStack<NARROW> &K, int &skip,
                                            f3 &sample, int sidx, Ctr &c, short *bstk, const float4 *nodes) {
    const SegIn in = iow_seg_pop(S, K, sidx);
    const RayRet data = iow_launch_ray<BS - 3, NS>(S, F, in.co, in.cd, 32000.0f, in.contribution, c, bstk, nodes);
    iow_seg_shade(S, F, K, skip, sample, sidx, c, in, data);
}

// Camera ray of sample s of a pixel, out_Pixel 03...glsl:370-406
struct IowPixelCam { float sx, sy; };
__device__ __forceinline__ void iow_camera_ray(const IowScene &S, const Frame &f, float sx, float sy, float dsx,
                                               float dsy, int s, f3 &ro, f3 &rd) {
    const f3 D = mk(f.dir[0], f.dir[1], f.dir[2]), P = mk(f.pos[0], f.pos[1], f.pos[2]);
    const f3 up = f3{0, 1, 0};
    f3 look_at = P + D * f.focus;
    f3 cr = cross(D, up), cu = cross(cr, D);
    const int ix = S.ring[2 * s], iy = S.ring[2 * s + 1];
    float rx = (S.sunflower[2 * s] * f.aperture) * 0.5f, ry = (S.sunflower[2 * s + 1] * f.aperture) * 0.5f;
    ro = (P + cr * rx) + cu * ry;
    f3 ld = normalize(look_at - ro);
    f3 r_ = cross(ld, up), u_ = cross(cr, ld);
    rd = normalize((ld * f.screen_dist + r_ * (sx + dsx * (float)ix)) + u_ * (sy + dsy * (float)iy));
}
// The four scalars it takes, as out_Pixel forms them (03...glsl:370-380): the pixel's screen position
// (sx, sy) and the sub-pixel steps (dsx, dsy).  The render kernels (rt_iow_render.hip, rt_iow_spec.hip) and k_camera_rays
// (rt_pixels.hip) call these.
// The ring schedule's grid and the aspect ratio under them: k_camera_rays calls these two; the render
// kernels keep the same two statements inline (calling them here changed their device code's bytes,
// the grid loop's).
__device__ __forceinline__ int iow_ring_grid(int spp) {
    int grid = 1;
    while (grid * grid < spp) grid++;
    return grid;
}
__device__ __forceinline__ float iow_aspect(int W, int H) { return (float)W * rcp((float)H); }
__device__ __forceinline__ float iow_px_dsx(float aspect, int W, int grid) { return aspect * rcp((float)(W * grid)); }
__device__ __forceinline__ float iow_px_dsy(int H, int grid) { return 1.0f * rcp((float)(H * grid)); }
__device__ __forceinline__ float iow_px_sx(float aspect, int x, int W) {
    return (aspect * ((float)x * 2.0f - (float)W)) * rcp(2.0f * (float)W);
}
__device__ __forceinline__ float iow_px_sy(int y, int H) { return ((float)y * 2.0f - (float)H) * rcp(2.0f * (float)H); }

}  // namespace rtk
