// rt_iow_walk.hpp -- the IOW-03 closest-hit search as device functions: the object records and
// their exact tests, the 4-wide culling walk with postponed leaves (nodes in LDS or global memory),
// the reference's linear loop, and the hit evaluation (LaunchRay, 03...glsl:196-256).  Included by
// rt_iow_render.hip and rt_iow_spec.hip (the render kernels) and rt_trace_iow.hip (the ray-query kernel), so both run the
// same search.
#pragma once
#include "rt_kernels.hpp"
#include "rt_math.hpp"
#include "rt_inw_walk.hpp"  // Ctr, kMiss, pk, cswap

namespace rtk {

// Diagnostics (rt_debug_counters).  Tallies go to a per-wave LDS row, written by the first
// active lane, so they cost no registers when off and are exact inside divergent code.
__device__ __forceinline__ bool first_active_lane() {
    return (int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1;
}
// wave cycles of a phase (shader clock)
#define DBG_T0(f, t) const unsigned long long t = c.wdbg ? (unsigned long long)clock64() : 0ull
#define DBG_CYC(f, c, slot, t)                                                        \
    do {                                                                              \
        if ((c).wdbg) {                                                               \
            const unsigned long long d_ = (unsigned long long)clock64() - (t);        \
            if (first_active_lane()) (c).wdbg[slot] += d_;                            \
        }                                                                             \
    } while (0)
// count one wave-iteration of a phase and how many lanes take part
#define DBG_TALLY(f, c, slot, pred)                                                   \
    do {                                                                              \
        if ((c).wdbg) {                                                               \
            const unsigned long long m_ = __ballot(pred);                             \
            if (first_active_lane()) {                                                \
                (c).wdbg[slot] += 1; (c).wdbg[(slot) + 1] += (unsigned long long)__popcll(m_); \
            }                                                                         \
        }                                                                             \
    } while (0)

struct RayRet { f3 point, normal, reflected, color, material; float scat0, scat1; };

struct IowObj { f3 pos; int type; m3 M; f3 scale, is; };

__device__ __forceinline__ IowObj iow_obj(const float *__restrict__ h) {
    IowObj o;
    o.pos = mk(h[0], h[1], h[2]);
    o.type = (int)h[3];
    o.M.c0 = mk(h[4], h[5], h[6]); o.M.c1 = mk(h[7], h[8], h[9]); o.M.c2 = mk(h[10], h[11], h[12]);
    o.scale = mk(h[13], h[14], h[15]);
    o.is = mk(h[16], h[17], h[18]);
    return o;
}

// Culling-only slab test for the IOW BVH (never decides a hit: the exact object test does).
// Boxes are inflated on the host and the limit carries relative slack, so an object whose
// exact t can win is never culled.  (plane - o) * (1/d) keeps a small relative error in t;
// the fused form plane*(1/d) - o*(1/d) would cancel catastrophically for large o/d (INW uses it
// only under the bound of cull4nf below).
__device__ __forceinline__ bool cull_slab(float4 n0, float4 n1, f3 o, f3 id, float lim, float &te) {
    const float x0 = (n0.x - o.x) * id.x, x1 = (n0.w - o.x) * id.x;
    const float y0 = (n0.y - o.y) * id.y, y1 = (n1.x - o.y) * id.y;
    const float z0 = (n0.z - o.z) * id.z, z1 = (n1.y - o.z) * id.z;
    te = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    const float tx = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    return te <= tx && tx >= -1e-3f && te <= lim;
}

// Same test for one child of a 4-wide node; returns the entry t, or kMiss when culled.
__device__ __forceinline__ float cull_t(float lx, float ly, float lz, float hx, float hy, float hz, f3 o, f3 id,
                                        float lim) {
    const float x0 = (lx - o.x) * id.x, x1 = (hx - o.x) * id.x;
    const float y0 = (ly - o.y) * id.y, y1 = (hy - o.y) * id.y;
    const float z0 = (lz - o.z) * id.z, z1 = (hz - o.z) * id.z;
    const float te = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    const float tx = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    return (te <= tx && tx >= -1e-3f && te <= lim) ? te : kMiss;
}
// The four children of a 4-wide node at once.  The node is SoA over the children (lx = the
// four children's low x planes, ...), so (plane - o) * (1/d) runs on child pairs with packed
// fp32 arithmetic (v_pk_add_f32 / v_pk_mul_f32: two lanes' worth per instruction); min / max
// stay scalar.  Same operations and rounding per plane as cull_t.
// The planes arrive already split into near and far by the ray's octant (the caller
// loads plane a + 3 s_a as near and a + 3 (1 - s_a) as far, s_a = 1 when d_a < 0).  With a finite,
// nonzero reciprocal the slab value (p - o) * (1/d) is monotone in p, so the near plane's value is
// the min of the pair and the far plane's the max: te and tx have cull_t's bits and the 12 min / max
// per node are gone.  A zero component (1/d = inf) keeps at least the boxes cull_t keeps: the pair
// form's fminf / fmaxf drop a NaN (origin on a plane) and then cull, the octant form keeps the box.
// The culling BVH only decides which objects get the exact test (iow_launch_ray), so that is exact.
__device__ __forceinline__ void cull4o(const float4 nx, const float4 ny, const float4 nz, const float4 fx,
                                       const float4 fy, const float4 fz, f3 o, f3 id, float lim, float &t0,
                                       float &t1, float &t2, float &t3) {
    const pf2 ox = pk(o.x, o.x), oy = pk(o.y, o.y), oz = pk(o.z, o.z);
    const pf2 ix = pk(id.x, id.x), iy = pk(id.y, id.y), iz = pk(id.z, id.z);
    const pf2 ax01 = (pk(nx.x, nx.y) - ox) * ix, bx01 = (pk(fx.x, fx.y) - ox) * ix;
    const pf2 ay01 = (pk(ny.x, ny.y) - oy) * iy, by01 = (pk(fy.x, fy.y) - oy) * iy;
    const pf2 az01 = (pk(nz.x, nz.y) - oz) * iz, bz01 = (pk(fz.x, fz.y) - oz) * iz;
    const pf2 ax23 = (pk(nx.z, nx.w) - ox) * ix, bx23 = (pk(fx.z, fx.w) - ox) * ix;
    const pf2 ay23 = (pk(ny.z, ny.w) - oy) * iy, by23 = (pk(fy.z, fy.w) - oy) * iy;
    const pf2 az23 = (pk(nz.z, nz.w) - oz) * iz, bz23 = (pk(fz.z, fz.w) - oz) * iz;
    auto one = [&](float n0, float f0, float n1, float f1, float n2, float f2) {
        const float te = fmaxf(fmaxf(n0, n1), n2);
        const float tx = fminf(fminf(f0, f1), f2);
        return (te <= tx && tx >= -1e-3f && te <= lim) ? te : kMiss;
    };
    t0 = one(ax01.x, bx01.x, ay01.x, by01.x, az01.x, bz01.x);
    t1 = one(ax01.y, bx01.y, ay01.y, by01.y, az01.y, bz01.y);
    t2 = one(ax23.x, bx23.x, ay23.x, by23.x, az23.x, bz23.x);
    t3 = one(ax23.y, bx23.y, ay23.y, by23.y, az23.y, bz23.y);
}

// Local ray of an object (the `M*(o-p)`, `normalize(M*d)` of t_RayXObj, 03...glsl:55-73).
// Objects whose matrix is glm::mat3(1) transform the direction identically, so M*gd and
// normalize(M*gd) are evaluated once per ray and passed in (same operations, same bits: 1*x
// folds to x, the 0*y terms are kept because IEEE forbids folding them).
__device__ __forceinline__ void iow_local(const float *h, const IowObj &ob, f3 go, f3 gd, f3 td_id, f3 nd_id, f3 &to,
                                          f3 &td, f3 &nd) {
    const m3 I = m3{f3{1.0f, 0.0f, 0.0f}, f3{0.0f, 1.0f, 0.0f}, f3{0.0f, 0.0f, 1.0f}};
    if (h[19] != 0.0f) { to = mul(I, go - ob.pos); td = td_id; nd = nd_id; }
    else { to = mul(ob.M, go - ob.pos); td = mul(ob.M, gd); nd = normalize(td); }
}
__device__ __forceinline__ void iow_id_dirs(f3 gd, f3 &td_id, f3 &nd_id) {
    const m3 I = m3{f3{1.0f, 0.0f, 0.0f}, f3{0.0f, 1.0f, 0.0f}, f3{0.0f, 0.0f, 1.0f}};
    td_id = mul(I, gd);
    nd_id = normalize(td_id);
}
// exact test of object j; keeps the reference's rule: nearer t, or the lower index on a tie
__device__ __forceinline__ void iow_test(const IowScene &S, int j, f3 go, f3 gd, f3 td_id, f3 nd_id, float &min_t,
                                         int &best) {
    const float *h = S.hot + (size_t)j * kIowHot;
    const IowObj ob = iow_obj(h);
    f3 to, td, nd;
    iow_local(h, ob, go, gd, td_id, nd_id, to, td, nd);
    float t = -1.0f;
    if (ob.type == 2) t = t_ellipsoid(to, nd, ob.is);
    else if (ob.type == 1) t = t_cuboid(to, nd, ob.scale);
    if (t > 0.0f && (t < min_t || (t == min_t && j < best))) { min_t = t; best = j; }
}

// Hit attributes of the winner `best` at min_t (LaunchRay's tail, 03...glsl:221-255): the
// closest hit's normal and attributes are evaluated once after the search.
// cold = the winner's cold record (colour3, material3, scatter2) when min_t < max_t;
// td_id / nd_id = iow_id_dirs(gd), already computed by the search
__device__ __forceinline__ RayRet iow_eval_c(const IowScene &S, f3 go, f3 gd, f3 td_id, f3 nd_id, float min_t, int best,
                                             float max_t, float contrib, float4 c0, float4 c1) {
    RayRet r;
    if (min_t < max_t) {
        const float *hb = S.hot + (size_t)best * kIowHot;
        const IowObj ob = iow_obj(hb);
        f3 best_to, best_td, best_nd;
        iow_local(hb, ob, go, gd, td_id, nd_id, best_to, best_td, best_nd);
        f3 h = best_to + best_nd * min_t;
        f3 n = ob.type == 2 ? f3{h.x * ob.is.x * ob.scale.x, h.y * ob.is.y * ob.scale.y, h.z * ob.is.z * ob.scale.z}
                            : (ob.type == 1 ? cuboid_normal(h, ob.scale) : f3{0, 0, 0});
        r.color = mk(c0.x, c0.y, c0.z);
        r.material = mk(c0.w, c1.x, c1.y);
        r.scat0 = c1.z; r.scat1 = c1.w;
        const bool inside = dot(n, best_td) > 0.0f;
        f3 n_ = sel(inside, -n, n);
        f3 refl = reflect(best_td, n_);
        if (!inside) {
            f3 nir = normalize(cross(n_, best_td));
            f3 nn = normalize(cross(nir, n_));
            float s = r.scat1;
            float k = rcp_sqrt_domain(__builtin_sqrtf(1.0f + s * s));
            f3 mr = n_ * (s * k) + nn * k;
            refl = sel(dot(refl, n_) > dot(mr, n_), refl, mr);
        }
        r.point = go + gd * min_t;
        if (hb[19] != 0.0f) {
            // M is glm::mat3(1) (iow_local): inverse(M) is the constant the same formula gives
            // for the identity, folded at compile time (IEEE folding keeps its signed zeros and
            // the 0*x products of mul), so the bits are those of the general branch
            const m3 I = m3{f3{1.0f, 0.0f, 0.0f}, f3{0.0f, 1.0f, 0.0f}, f3{0.0f, 0.0f, 1.0f}};
            const m3 inv = inverse(I);
            r.normal = normalize(mul(inv, n));
            r.reflected = normalize(mul(inv, refl));
        } else {
            const m3 inv = inverse(ob.M);
            r.normal = normalize(mul(inv, n));
            r.reflected = normalize(mul(inv, refl));
        }
        r.color = r.color * contrib;
    } else {
        r.point = f3{0, 0, 0}; r.normal = f3{0, 0, 0};
        r.reflected = r.color = r.material = f3{0, 0, 0};
        r.scat0 = r.scat1 = 0.0f;
    }
    return r;
}
__device__ __forceinline__ RayRet iow_eval(const IowScene &S, f3 go, f3 gd, f3 td_id, f3 nd_id, float min_t, int best,
                                           float max_t, float contrib) {
    float4 c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c1 = c0;
    if (min_t < max_t) {
        const float4 *cold = reinterpret_cast<const float4 *>(S.cold + (size_t)best * kIowCold);
        c0 = cold[0]; c1 = cold[1];
    }
    return iow_eval_c(S, go, gd, td_id, nd_id, min_t, best, max_t, contrib, c0, c1);
}

// IOW BVH-stack slot p of a lane (16-bit links), [slot][lane]: two lanes share a dword, so two
// lanes of an LDS access group whose stack depths differ hit one bank (a 2-way conflict).  The
// conflict-free pair layout cost more in address arithmetic than the conflicts did
// (DESIGN_HISTORY.md §J).  b = the lane's base, lds + lane.
__device__ __forceinline__ short &bslot(short *b, int p) { return b[p * kBlock]; }

// LaunchRay 03...glsl:196-256.  The reference loops over every object and keeps the first
// strictly nearer hit, i.e. the minimum t with the lowest index among exact ties.  The BVH
// walk visits a superset of the objects that can attain that minimum and applies the same
// (t, index) rule, so it returns the same object and the same t bits.
// nodes: the 4-wide BVH (NS float4 per node: in LDS, 7; in global memory, 8), or null.
// tap(min_t, best) sees the search's result before the evaluation: the ray-query kernel
// (rt_trace_iow.hip) takes t and the object index from it; the render kernels pass none.
struct IowNoTap { __device__ __forceinline__ void operator()(float, int) const {} };
template <int BCAP, int NS = 8, class Tap = IowNoTap>
__device__ RayRet iow_launch_ray(const IowScene &S, const Frame &F_, f3 go, f3 gd, float max_t, float contrib,
                                 Ctr &c, short *bstk, const float4 *nodes, Tap tap = Tap{}) {
    DBG_T0(F_, t_ray);
    float min_t = max_t;
    int best = -1;
    c.seg++;
    f3 td_id, nd_id;
    iow_id_dirs(gd, td_id, nd_id);
    auto test = [&](int j) {
        c.prims++;
        iow_test(S, j, go, gd, td_id, nd_id, min_t, best);
    };
    const float dl2 = dot(gd, gd);
    if (!(dl2 > 0.0f)) {
        // zero or NaN direction (the TIR branch pushes the uninitialised reflection_dirn,
        // 03...glsl:331-332): normalize(M*gd) is NaN for every object, so every t is -1 and
        // the reference's loop finds no hit -- skip it.
        c.prims += S.n;
    } else if (nodes != nullptr && dl2 > 0.998f && dl2 < 1.002f) {
        // Ordered walk with postponed leaves (speculative traversal): a lane that reaches a
        // leaf parks it and keeps walking inner nodes; primitive tests run when every lane
        // of the wave holds one (or has finished), so they execute with full lanes.
        const f3 id = f3{__builtin_amdgcn_rcpf(gd.x), __builtin_amdgcn_rcpf(gd.y), __builtin_amdgcn_rcpf(gd.z)};
        // 4-wide BVH.  cur = link of the next node to enter: > 0 = wide node cur-1, <= 0 =
        // leaf of object -cur.  One step loads a 112-B node (7 x float4, SoA over the four
        // children), tests the four boxes, enters the nearest hit child and pushes the others
        // farthest-first.
        DBG_T0(F_, t_trav);
        // the ray's near / far plane of each axis (cull4o): low planes are float4 0-2, high 3-5
        const int nxo = gd.x < 0.0f ? 3 : 0, nyo = gd.y < 0.0f ? 4 : 1, nzo = gd.z < 0.0f ? 5 : 2;
        const int fxo = 3 - nxo, fyo = 5 - nyo, fzo = 7 - nzo;
        int sp = 0, pend = -1, cur = S.root_link;
        bool walking = true, ovf = false;  // ovf: a child was dropped by a full stack
        float lim = min_t * 1.0001f + 1e-3f;  // culling limit, follows min_t
        for (;;) {
            DBG_TALLY(F_, c, kDbgTrav, walking);
            if (walking) {
                bool pop;
                if (cur > 0) {
                    const float4 *nd = nodes + NS * (cur - 1);
                    const float4 lk = nd[6];  // child links as int bits (set_iow_bvh)
                    c.nodes += 4;
                    float t0, t1, t2, t3;
                    cull4o(nd[nxo], nd[nyo], nd[nzo], nd[fxo], nd[fyo], nd[fzo], go, id, lim, t0, t1, t2, t3);
                    int k0 = __float_as_int(lk.x), k1 = __float_as_int(lk.y), k2 = __float_as_int(lk.z),
                        k3 = __float_as_int(lk.w);
                    // sort (t, link) ascending; misses carry t = +inf
                    cswap(t0, k0, t1, k1); cswap(t2, k2, t3, k3);
                    cswap(t0, k0, t2, k2); cswap(t1, k1, t3, k3);
                    cswap(t1, k1, t2, k2);
                    // branch-free pushes, farthest first: a miss is written above the top and
                    // overwritten before it could be popped (the array has 3 spare entries)
                    int p = sp;
                    bslot(bstk, p) = (short)k3; p += t3 != kMiss;
                    bslot(bstk, p) = (short)k2; p += t2 != kMiss;
                    bslot(bstk, p) = (short)k1; p += t1 != kMiss;
                    if (p > BCAP) { ovf = true; p = BCAP; }
                    sp = p;
                    cur = k0;
                    pop = t0 == kMiss;
                } else {
                    pop = pend < 0;  // a leaf waits while the lane still holds one
                    if (pop) pend = -cur;
                }
                if (pop) {
                    if (sp == 0) walking = false;
                    else cur = bslot(bstk, --sp);
                }
            }
            if (__all(!walking || pend >= 0) || __popcll(__ballot(pend >= 0)) >= F_.leaf_batch) {
                DBG_TALLY(F_, c, kDbgLeaf, pend >= 0);
                DBG_T0(F_, t_leaf);
                if (pend >= 0) { test(pend); pend = -1; lim = min_t * 1.0001f + 1e-3f; }
                DBG_CYC(F_, c, kDbgCycLeaf, t_leaf);
                if (__all(!walking)) break;
            }
        }
        // a dropped subtree may hold the winner: the linear loop covers every object, and the
        // (t, index) rule makes re-testing the visited ones harmless
        if (ovf) for (uint32_t j = 0; j < S.n; j++) test((int)j);
        DBG_CYC(F_, c, kDbgCycTrav, t_trav);
    } else {
        for (uint32_t j = 0; j < S.n; j++) test((int)j);  // also the path for zero / NaN directions
    }
    tap(min_t, best);
    RayRet r = iow_eval(S, go, gd, td_id, nd_id, min_t, best, max_t, contrib);
    DBG_CYC(F_, c, kDbgCycRay, t_ray);
    return r;
}

// Kernel configurations of the IOW-03 work loops.  SUB: 256-thread sub-blocks per block, each
// with its own [slot][thread] stack arrays (stride kBlock).  LN: the whole 4-wide BVH is copied
// into the block's LDS (7 float4 per node) when it has at most kIowLdsNodes nodes: one
// 768-thread block per CU shares it, so node fetches cost LDS latency instead of L2 latency.
constexpr int kIowLdsNodes = 240;
template <bool NARROW, int SUB, bool LN>
struct IowCfg {
    static constexpr int BS = LN ? 16 : (NARROW ? 12 : kIowBvhStack);  // BVH-stack slots per lane
    static constexpr int NS = LN ? 7 : 8;                               // float4 per BVH node
    static constexpr int kThreads = SUB * kBlock;
};
// copy the BVH into LDS (7 float4 per node, dropping the pad) and return the node base
template <bool LN>
__device__ __forceinline__ const float4 *iow_stage_nodes(const IowScene &S, float4 *s_nodes) {
    if constexpr (!LN) return S.nodes;
    else {
        const uint32_t total = S.n_nodes * 7u;
        for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) s_nodes[i] = S.nodes[(i / 7u) * 8u + i % 7u];
        __syncthreads();
        return s_nodes;
    }
}

}  // namespace rtk
