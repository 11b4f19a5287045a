// rt_iow_coop.hpp -- the segment step of the IOW-03 render kernels' work loops: the
// wave-cooperative closest hit and the choice between it and the per-lane BVH walk.  Included by
// rt_iow_render.hip (k_iow03*) and rt_iow_spec.hip (k_iow03s*), so both run the same step.  It
// stays out of rt_iow_shade.hpp because it needs the render units' SPL_* timing macros, which the
// query units that include that header do not have.
#pragma once
#include "rt_render_common.hpp"
#include "rt_iow_walk.hpp"
#include "rt_iow_shade.hpp"

namespace rtk {

// ---------------------------------------------------------------- wave-cooperative closest hit
// When only a few lanes of a wave still trace (the long samples at the end of a pass), the
// wave runs their closest-hit queries one ray at a time with all 64 lanes: every lane culls
// 1/64 of the objects against their conservative boxes (the BVH's leaf boxes), the survivors
// are compacted into a wave list in LDS and tested exactly in parallel, and a wave reduction
// applies the reference's (t, lowest index) rule.  The candidate set is a superset of the one
// the BVH walk tests, so the winner and its t bits are the same (DESIGN.md "k_iow03s").
// Requires all 64 lanes active.
__device__ __forceinline__ float wave_min_all(float v) {
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false)));   // quad [1,0,3,2]
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false)));   // quad [2,3,0,1]
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false)));  // row half-mirror
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false)));  // row mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
__device__ __forceinline__ float bcast_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// Closest hit of one (wave-uniform) ray with the whole wave.  wl: the wave's LDS list, entry k
// at lane k & 63's BVH-stack slot k >> 6 (bslot), cap entries (a multiple of 64 * kCoopR).  Returns the
// (uniform) winner and its cold record; nbox / nprim are the boxes and objects tested.  The
// loads of a batch of kCoopR boxes per lane, and a candidate's hot and cold records, are
// issued together: a lone ray's query costs about two memory latencies, not one per step.
constexpr int kCoopR = 8;
__device__ void iow_coop_search(const IowScene &S, f3 go, f3 gd, float max_t, short *wl, int cap, float &t_out,
                                int &j_out, float4 &c0_out, float4 &c1_out, uint32_t &nbox, uint32_t &nprim,
                                unsigned long long *wdbg = nullptr) {
    const int lane = (int)(threadIdx.x & 63);
    float bt = max_t;
    int bj = -1;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0;  // cold record of this lane's best
    nbox = 0; nprim = 0;
    t_out = max_t; j_out = -1; c0_out = b0; c1_out = b0;
    const float dl2 = dot(gd, gd);
    if (!(dl2 > 0.0f)) {  // zero / NaN direction: no object can hit (see iow_launch_ray)
        nprim = S.n;
        return;
    }
    f3 td_id, nd_id;
    iow_id_dirs(gd, td_id, nd_id);
    const bool cull = S.obox != nullptr && dl2 > 0.998f && dl2 < 1.002f;
    const f3 id = f3{__builtin_amdgcn_rcpf(gd.x), __builtin_amdgcn_rcpf(gd.y), __builtin_amdgcn_rcpf(gd.z)};
    const float lim = max_t * 1.0001f + 1e-3f;
    const uint32_t n = S.n;
    uint32_t j0 = 0;
    while (j0 < n) {
        uint32_t cnt = 0, jb = j0;
        SPL_T0(t_cull);
        if (cull) {
            for (; j0 < n && cnt + 64 * kCoopR <= (uint32_t)cap; j0 += 64 * kCoopR) {
                const float2 *ob2 = reinterpret_cast<const float2 *>(S.obox + n);
                float4 a[kCoopR];
                float2 b[kCoopR];
#pragma unroll
                for (int r = 0; r < kCoopR; r++) {
                    const uint32_t j = j0 + 64 * r + lane, jj = j < n ? j : n - 1;
                    a[r] = S.obox[jj];
                    b[r] = ob2[jj];
                }
#pragma unroll
                for (int r = 0; r < kCoopR; r++) {
                    const uint32_t j = j0 + 64 * r + lane;
                    const bool cand =
                        j < n && cull_t(a[r].x, a[r].y, a[r].z, a[r].w, b[r].x, b[r].y, go, id, lim) != kMiss;
                    const unsigned long long cm = __ballot(cand);
                    if (cand) {
                        const uint32_t k = cnt + lanes_below(cm);
                        bslot(wl + (k & 63), (int)(k >> 6)) = (short)j;
                    }
                    cnt += (uint32_t)__popcll(cm);
                }
            }
            nbox += (j0 < n ? j0 : n) - jb;
        } else {
            cnt = n - j0 < (uint32_t)cap ? n - j0 : (uint32_t)cap;
            j0 += cnt;
        }
        SPL_CYC(wdbg, kDbgTrav, t_cull);
        SPL_T0(t_exact);
        for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
            const uint32_t k = k0 + lane;
            if (k < cnt) {
                const int j = cull ? (int)bslot(wl + (k & 63), (int)(k >> 6)) : (int)(jb + k);
                const float4 *cold = reinterpret_cast<const float4 *>(S.cold + (size_t)j * kIowCold);
                const float4 q0 = cold[0], q1 = cold[1];
                const int was = bj;
                iow_test(S, j, go, gd, td_id, nd_id, bt, bj);
                if (bj != was) { b0 = q0; b1 = q1; }
            }
        }
        nprim += cnt;
        SPL_CYC(wdbg, kDbgTravLanes, t_exact);
    }
    SPL_T0(t_red);
    const float tm = wave_min_all(bj >= 0 ? bt : max_t);
    unsigned long long m = __ballot(bj >= 0 && bt == tm);
    if (m == 0) return;
    int jm = -1, lm = 0;
    for (; m; m &= m - 1) {  // usually one lane; exact ties keep the lowest object index
        const int l = __ffsll((long long)m) - 1;
        const int j = __builtin_amdgcn_readlane(bj, l);
        if (jm < 0 || j < jm) { jm = j; lm = l; }
    }
    t_out = tm;
    j_out = jm;
    c0_out = make_float4(bcast_f(b0.x, lm), bcast_f(b0.y, lm), bcast_f(b0.z, lm), bcast_f(b0.w, lm));
    c1_out = make_float4(bcast_f(b1.x, lm), bcast_f(b1.y, lm), bcast_f(b1.z, lm), bcast_f(b1.w, lm));
    SPL_CYC(wdbg, kDbgLeaf, t_red);
}

// The segment step of a work loop, called with every lane of the wave (seg: this lane has a
// ray to trace).  With at most F.coop_max tracing lanes the wave runs their closest-hit
// queries cooperatively (iow_coop_search), one ray after another; otherwise each lane walks
// the BVH for its own ray.
template <bool NARROW, int BS, int NS>
__device__ __forceinline__ void iow_seg_step(const IowScene &S, const Frame &F, IowStack<NARROW> &K, int &skip,
                                             f3 &sample, int sidx, Ctr &c, short *bstk, const float4 *nodes, bool seg) {
    const unsigned long long m = __ballot(seg);
    if (m == 0) return;
    if (__popcll(m) > F.coop_max) {
        if (seg) iow_segment<NARROW, BS, NS>(S, F, K, skip, sample, sidx, c, bstk, nodes);
        return;
    }
    constexpr int kCap = BS * 64;  // the wave's BVH-stack slots, as a list
    short *wl = bstk - (threadIdx.x & 63);
    DBG_T0(F, t_pop);
    SegIn in{};
    if (seg) in = iow_seg_pop(S, K, sidx);
    DBG_CYC(F, c, kDbgCycSpare2, t_pop);
    DBG_T0(F, t_q);
    float my_t = 32000.0f;
    int my_j = -1;
    float4 my_c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), my_c1 = my_c0;
    uint32_t my_box = 0, my_prim = 0;
    for (unsigned long long mm = m; mm; mm &= mm - 1) {
        const int L = __ffsll((long long)mm) - 1;
        const f3 go = f3{bcast_f(in.co.x, L), bcast_f(in.co.y, L), bcast_f(in.co.z, L)};
        const f3 gd = f3{bcast_f(in.cd.x, L), bcast_f(in.cd.y, L), bcast_f(in.cd.z, L)};
        float t;
        int j;
        float4 c0, c1;
        uint32_t nb, np;
        iow_coop_search(S, go, gd, 32000.0f, wl, kCap, t, j, c0, c1, nb, np, c.wdbg);
        if ((int)(threadIdx.x & 63) == L) { my_t = t; my_j = j; my_c0 = c0; my_c1 = c1; my_box = nb; my_prim = np; }
    }
    DBG_CYC(F, c, kDbgCycSpare0, t_q);
    DBG_T0(F, t_sh);
    if (seg) {
        c.seg++; c.nodes += my_box; c.prims += my_prim;
        SPL_T0(t_ev);
        f3 td_id, nd_id;
        iow_id_dirs(in.cd, td_id, nd_id);
        const RayRet data =
            iow_eval_c(S, in.co, in.cd, td_id, nd_id, my_t, my_j, 32000.0f, in.contribution, my_c0, my_c1);
        SPL_CYC(c.wdbg, kDbgCycRay, t_ev);
        SPL_T0(t_sd);
        iow_seg_shade(S, F, K, skip, sample, sidx, c, in, data);
        SPL_CYC(c.wdbg, kDbgCycTrav, t_sd);
    }
    DBG_CYC(F, c, kDbgCycSpare1, t_sh);
}

}  // namespace rtk
