// rt_inw_shade.hpp -- one iteration of the INW shaders' ray loop as a device function
// (inw_segment: pop a ray, closest hit, material and texture, surrounding RI, INW-04's shadow rays,
// the scatter step and its pushes on the 40-float stack), with the sample start of out_Pixel's
// prologue and the helpers they use.  Included by rt_inw_render.hip and rt_inw_fold.hip (the render kernels) and
// rt_paths.hip (the path-query kernel), so a frame and a path query run the same segment.
#pragma once
#include "rt_kernels.hpp"
#include "rt_math.hpp"
#include "rt_inw_walk.hpp"  // the stacks, the walks, Ctr and the diagnostic macros (INW_T0, INW_CYC, OCC_TALLY)

namespace rtk {

__device__ __forceinline__ bool is_lit_geom(const InwScene &S, uint32_t in) {  // 04...glsl:468-474
    bool r = false;
    for (uint32_t i = 0; i < S.n_lights && !r; i++) r = in == __float_as_uint(S.lights[i * 7 + 6]);
    return r;
}
__device__ __forceinline__ uint32_t f2u(float f) { return f <= 0.0f ? 0u : (uint32_t)f; }

// deviateWithLinmit90deg 01_BVH...glsl:28-46, power = 1
__device__ __forceinline__ f3 deviate(const InwScene &S, f3 dir, float tan_theta, int s) {
    float ap = (2.0f * tan_theta) * 0.5f;
    float nx = S.sunflower[2 * s] * ap, ny = S.sunflower[2 * s + 1] * ap;
    f3 right = cross(dir, f3{0, 1, 0});
    f3 up = cross(right, dir);
    return normalize(dir + (right * nx + up * ny) * 0.1f);
}

// Camera ray of sample s (out_Pixel prologue, 01_BVH...glsl:366-410): push it, reset the sample.
// the pixel's camera direction (01_BVH...glsl:366-386)
__device__ __forceinline__ f3 inw_pixel_dir(const Frame &F, int px, int py) {
    const f3 D = mk(F.dir[0], F.dir[1], F.dir[2]);
    float aspect = (float)F.W * rcp((float)F.H);
    float srx = (float)px * rcp((float)F.W) - 0.5f;
    float sry = (float)py * rcp((float)F.H) - 0.5f;
    srx *= aspect;
    const f3 up = f3{0, 1, 0};
    f3 cr = cross(D, up), cu = cross(cr, D);
    return normalize((D * F.screen_dist + cr * srx) + cu * sry);
}
// The single-focus camera ray of sample s (01_BVH...glsl:402-410): from the lens point, one unit
// behind the tip, at the focal point.  Shared by the sample start below and k_inw_sky.
__device__ __forceinline__ void inw_camera_ray(const InwScene &S, const Frame &F, f3 cd, int s, f3 &o, f3 &d) {
    const f3 up = f3{0, 1, 0};
    f3 co = mk(F.pos[0], F.pos[1], F.pos[2]);
    float ox = S.sunflower[2 * s] * (F.aperture * 0.5f), oy = S.sunflower[2 * s + 1] * (F.aperture * 0.5f);
    f3 rr = cross(cd, up), ru = cross(rr, cd);
    f3 tip = ((co + cd) + rr * ox) + ru * oy;
    d = normalize((co + cd * F.focus) - tip);
    o = tip - d;
}
// cd: the pixel's direction (inw_pixel_dir), which callers that keep it per pixel pass in
template <class KS>
__device__ __forceinline__ void inw_start_sample_cd(const InwScene &S, const Frame &F, KS &K, f3 cd, int s, Ctr &c) {
    K.reset(0);
    if (F.n_focus > 0) {  // MULTIFOCUS lens record (01_BVH...glsl:388-400): stack floats 0..5
        const f3 up = f3{0, 1, 0};
        f3 co = mk(F.pos[0], F.pos[1], F.pos[2]);
        float ox = S.sunflower[2 * s] * (F.aperture * 0.5f), oy = S.sunflower[2 * s + 1] * (F.aperture * 0.5f);
        f3 rr = cross(cd, up), ru = cross(rr, cd);
        const float first_limit = F.focus_list[0] * 0.5f;
        const f3 nd = normalize((cd * first_limit + rr * ox) + ru * oy);
        const f3 rn = normalize((-rr) * ox - ru * oy);
        const float mult = rcp(dot(cd, nd));
        K.push(rn.x, c); K.push(rn.y, c); K.push(rn.z, c);
        K.push(mult, c); K.push(first_limit, c); K.push(0.0f, c);
        K.push_ray(co, nd, 1.0f, 0.0f, c);
        return;
    }
    f3 o, la;
    inw_camera_ray(S, F, cd, s, o, la);
    K.push_ray(o, la, 1.0f, 0.0f, c);
}
template <class KS>
__device__ __forceinline__ void inw_start_sample(const InwScene &S, const Frame &F, KS &K, int px, int py, int s,
                                                 Ctr &c) {
    inw_start_sample_cd(S, F, K, inw_pixel_dir(F, px, py), s, c);
}

// texture(u_MaterialTextures[k], st) in a compute shader: lambda = 0, so the magnification
// filter GL_NEAREST applies (utility.cpp:182), with GL_REPEAT (utility.cpp:191-192)
__device__ __forceinline__ int tex_wrap(float u, int size) {
    const float f = __builtin_floorf(u);
    if (!(f == f) || f > 2147483520.0f || f < -2147483520.0f) return 0;  // NaN / inf: texel 0
    const int i = (int)f % size;
    return i < 0 ? i + size : i;
}
// FillHitMaterialData 04...glsl:416-464 (TextureIndex > 0): cube projection of the
// object-space hit position onto a 6-face strip, nearest texel
__device__ f3 inw_tex_color(const InwScene &S, uint32_t k, f3 lp) {
    lp = normalize(lp);
    float mx = lp.x;
    uint32_t face = mx > 0 ? 1u : 3u;
    f3 fd = f3{1, 0, 0} * (mx > 0 ? 1.0f : -1.0f);
    if (__builtin_fabsf(mx) < __builtin_fabsf(lp.y)) {
        mx = lp.y;
        face = mx > 0 ? 0u : 5u;
        fd = f3{0, 1, 0} * (mx > 0 ? 1.0f : -1.0f);
    }
    if (__builtin_fabsf(mx) < __builtin_fabsf(lp.z)) {
        mx = lp.z;
        face = mx > 0 ? 2u : 4u;
        fd = f3{0, 0, 1} * (mx > 0 ? 1.0f : -1.0f);
    }
    lp = lp * rcp(dot(lp, fd));
    lp = lp * 0.5f;
    lp = lp + f3{0.5f, 0.5f, 0.5f};
    float u, v;
    switch (face) {
        case 0: u = lp.x; v = 1.0f - lp.z; break;
        case 1: u = 1.0f - lp.y; v = 1.0f - lp.z; break;
        case 2: u = lp.x; v = lp.y; break;
        case 3: u = lp.z; v = lp.y; break;
        case 4: u = 1.0f - lp.y; v = 1.0f - lp.x; break;
        default: u = lp.z; v = 1.0f - lp.x; break;
    }
    const int4 ti = S.tex_info[k];
    const int i = tex_wrap(((float)face * 0.16666f + u * 0.16666f) * (float)ti.y, ti.y);
    const int j = tex_wrap(v * (float)ti.z, ti.z);
    const float4 c = S.tex[(size_t)ti.x + (size_t)j * (size_t)ti.y + (size_t)i];
    return f3{c.x, c.y, c.z};
}

// One iteration of out_Pixel's ray loop (01_BVH...glsl:414-597 / 04...glsl:510-713):
// pop a ray, closest hit, surrounding RI, shadow rays, push reflect/refract, accumulate.
// bunit: the lane's pixel unit when its primary ray may use the pixel's beam list (k_inw_pm), else kBeamOff
// QN (k_inw_pm's GQ instance): the wide closest-hit walks read the quantised nodes (inw_closest)
template <bool LIGHTS, bool LN = false, bool FU = false, bool QN = false, class KS = FStack>
__device__ void inw_segment(const InwScene &S, const Frame &F, KS &K, int s, f3 &color, float &depth, Ctr &c,
                            uint32_t bunit = kBeamOff) {
    constexpr bool RLN = LN && !QN;  // the LBVH / RI walks' staged nodes (none in the GQ instance)
    const f3 D = mk(F.dir[0], F.dir[1], F.dir[2]);
    const float ratio = (float)s * F.inv_spp;
    const bool invert = dot(D, f3{1, 1, 1}) > 0.0f;
    INW_T0(t_fn);
#ifdef RT_DIAG_SPLIT
    unsigned long long t_tail = 0;  // the scatter and pushes after the RI (phase 7)
#endif
    do {
        f3 co, cd;
        float contribution, bounced;
        K.pop_ray(co, cd, contribution, bounced);
        bounced = (float)(int)bounced;
        c.seg++;
        // SET LIMIT (01_BVH...glsl:424-428): a MULTIFOCUS primary ray stops at the lens
        const bool mf0 = !LIGHTS && F.n_focus > 0 && (int)(bounced + 0.1f) == 0;
        const float tlim0 = mf0 ? K.at(4) : kMaxT;
        float tlim = tlim0, extra = 0.0f;
        f3 normal = f3{0, 0, 0};
        INW_CYC(c, 5, t_fn);  // the pop and the segment's prologue
        INW_T0(t_ch);
        float fg;
        bool beam_ok = false;
        if (bunit != kBeamOff && (int)(bounced + 0.1f) == 0 && !mf0)  // a primary ray (pushed rays have bounced >= 1)
            fg = inw_closest_beam<true>(S, K, co, cd, ratio, invert, tlim, normal, extra, LIGHTS ? -1.0f : 0.0f, c, bunit,
                                        beam_ok);
        if (!beam_ok)
            fg = inw_closest<true, LN, FU, !LIGHTS, QN>(S, K, co, cd, ratio, invert, tlim, normal, extra,
                                                        LIGHTS ? -1.0f : 0.0f, c);
        INW_CYC(c, 0, t_ch);
        INW_T0(t_mat);
        const f3 hitpoint = co + cd * tlim;
        if (!(tlim < tlim0)) {
            if (mf0 && (int)(K.at(5) + 0.1f) < F.n_focus) {  // next focal lens, 01_BVH...glsl:506-528
                const f3 rn = mk(K.at(0), K.at(1), K.at(2));
                K.at(0) = -K.at(0); K.at(1) = -K.at(1); K.at(2) = -K.at(2);
                const float mult = K.at(3), dist = K.at(4);
                const f3 no = co + cd * (mult * dist), nd = reflect(cd, rn);
                const int lens = (int)(K.at(5) + 0.1f);
                if (lens < F.n_focus - 1)
                    K.at(4) = (F.focus_list[lens + 1] - F.focus_list[lens]) * 0.5f +
                              (F.focus_list[lens] - (lens > 0 ? F.focus_list[lens - 1 > 0 ? lens - 1 : 0] : 0.0f)) *
                                  0.5f;
                else K.at(4) = kMaxT - mult * K.at(4);
                K.at(5) = K.at(5) + 1.0f;
                K.reset(6);
                K.push_ray(no, nd, 1.0f, 0.0f, c);
                break;
            }
            color = color + background(cd, LIGHTS && S.n_lights > 0) * contribution;
            depth = tlim;
            if (mf0) K.reset(0);  // 01_BVH...glsl:531-535
            break;
        }
        const float4 m0 = S.cold[2 * (int)fg], m1 = S.cold[2 * (int)fg + 1];
        const float m_refr = m0.x, m_refl = m0.y, m_srfr = m0.z, m_srfl = m0.w;
        f3 m_color = mk(m1.x, m1.y, m1.z);
        const float m_ri = LIGHTS ? extra : m1.w;
        if (LIGHTS && S.n_tex) {  // layout 4 keeps the TextureIndex (uint bits) in m1.w
            const uint32_t ti = __float_as_uint(m1.w);
            if (ti - 1u < S.n_tex) {  // 04...glsl:416; local position :569 (no motion offset)
                const float4 h0 = S.hot[7 * (int)fg], h1 = S.hot[7 * (int)fg + 1], h2 = S.hot[7 * (int)fg + 2];
                const m3 R{mk(h0.w, h1.x, h1.y), mk(h1.z, h1.w, h2.x), mk(h2.y, h2.z, h2.w)};
                m_color = mulv(m_color, inw_tex_color(S, ti - 1u, tmul(R, hitpoint - mk(h0.x, h0.y, h0.z))));
            }
        }
        // The surrounding RI (01_BVH...glsl:486-502) is read only by the refract calls below: on an
        // outer hit of a refractive object, or on an inner hit.  Where the scatter branch will not
        // run or reads no RI, the walk is skipped -- when it cannot drop a push (the wide walk's
        // condition; its drops are counted) and the walk is the wide one (whose node counts are
        // this build's own).  INW-04 decides after its shadow rays, which scale the contribution.
        INW_CYC(c, 6, t_mat);  // a hit's material (and texture)
        const bool ri_forced = S.wnodes == nullptr || K.size + S.dfs_high > (uint32_t)kFStack;
        const bool ri_read = (m_refl > 0.002f || m_refr > 0.002f) && (m_refr > 0.002f || dot(normal, cd) > 0.0f);
        float surr = 1.0f;
        if (!LIGHTS && (ri_forced || (ri_read && contribution > 0.01f && bounced + 1.0f < (float)F.max_bounces)))
        {
            INW_T0(t_ri);
            OCC_TALLY(c, kOccRi, true);
            surr = inw_ri<RLN>(S, K, hitpoint + normal * 0.001f, ratio, c);
            INW_CYC(c, 1, t_ri);
        }
#ifdef RT_DIAG_SPLIT
        t_tail = clock64();
#endif
        if (mf0) K.reset(0);  // 01_BVH...glsl:544-549: the lens record goes after a primary hit
        if (LIGHTS) {  // 04...glsl:604-665
            uint32_t is_lit = S.n_lights > 0 ? 0u : (uint32_t)is_lit_geom(S, f2u(fg + 0.1f));
            if (is_lit == 0) {
                for (uint32_t i = 0; i < S.n_lights; i++) {
                    const float *lt = S.lights + i * 7;
                    f3 bmin = mk(lt[0], lt[1], lt[2]), bmax = mk(lt[3], lt[4], lt[5]);
                    f3 so = hitpoint + normal * 0.0001f;
                    float sl = len((bmax + bmin) * 0.5f - so) + len(bmax - bmin);
                    f3 sd = normalize((bmin + (bmax - bmin) * ratio) - so);
                    c.shadow++;
                    f3 dummy_n; float dummy_e;
                    float sg = inw_closest<false, LN, FU, !LIGHTS, QN>(S, K, so, sd, ratio, invert, sl, dummy_n,
                                                                       dummy_e, -1.0f, c);
                    is_lit += (uint32_t)is_lit_geom(S, f2u(sg + 0.1f));
                }
                const uint32_t nl = S.n_lights > 1 ? S.n_lights : 1u;
                contribution *= (float)is_lit * rcp((float)nl);
                if (ri_forced || (ri_read && contribution > 0.01f && bounced < (float)F.max_bounces))
                    surr = inw_ri<RLN>(S, K, hitpoint + normal * 0.001f, ratio, c);
            } else {
                if (ri_forced) (void)inw_ri<RLN>(S, K, hitpoint + normal * 0.001f, ratio, c);
                color = f3{1, 1, 1};
                K.reset(0);
                break;
            }
        }
        bool ok;
        if (!LIGHTS) { bounced += 1.0f; ok = bounced < (float)F.max_bounces; }
        else ok = bounced < (float)F.max_bounces;
        if ((m_refl > 0.002f || m_refr > 0.002f) && contribution > 0.01f && ok) {
            if (LIGHTS) bounced += 1.0f;
            f3 refl = f3{0, 0, 0}, refr = f3{0, 0, 0};
            f3 nrm = normal;
            if (!(dot(nrm, cd) > 0.0f)) {
                if (m_refl > 0.002f) {
                    refl = normalize(reflect(cd, nrm));
                    if (m_srfl > 0.001f) refl = deviate(S, refl, m_srfl, s);
                }
                if (m_refr > 0.002f) {
                    refr = normalize(refract(cd, nrm, surr * rcp(m_ri)));
                    if (m_srfr > 0.001f) refr = deviate(S, refr, m_srfr, s);
                }
            } else {
                nrm = nrm * -1.0f;
                refr = refract(cd, nrm, m_ri * rcp(surr));
                if (dot(refr, refr) < 0.1f) refl = reflect(cd, nrm);
            }
            float carried = 0.0f;
            const float rr2 = dot(refr, refr);
            if (__builtin_isnan(rr2)) c.nans++;
            if (rr2 > 0.1f) {
                carried += m_refr;
                K.push_ray(hitpoint - nrm * 0.0001f, refr, contribution * m_refr, bounced, c);
            }
            if (dot(refl, refl) > 0.1f) {
                carried += m_refl;
                K.push_ray(hitpoint + nrm * 0.0001f, refl, contribution * m_refl, bounced, c);
            }
            contribution *= (1.0f - 0.5f * carried);
        }
        color = color + m_color * contribution;
    } while (false);
#ifdef RT_DIAG_SPLIT
    if (t_tail) c.cyc[7] += clock64() - t_tail;
#endif
}

}  // namespace rtk
