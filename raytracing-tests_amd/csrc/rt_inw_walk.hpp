// rt_inw_walk.hpp -- the INW closest-hit and surrounding-RI walks as device functions: the
// reference's LBVH walks (01_BVH...glsl:431-473, 486-502) on the 40-float stack, the stackless
// forms, the 4-wide culling walk with its node fetches and object tests, the beam-list and RI-grid
// queries, and inw_closest / inw_ri, which pick among them.  Included by rt_inw_render.hip and
// rt_inw_fold.hip (the render kernels) and rt_trace.hip (the ray-query kernel), so both run the same walk.
#pragma once
#include "rt_kernels.hpp"
#include "rt_math.hpp"

namespace rtk {

// occupancy slots (RT_DIAG_OCC): pairs (wave iterations, lanes) of: the fold loop's iterations with
// busy lanes; wide-walk trips with walking lanes; their node steps; leaf batches; beam-list trips;
// reference-walk entries (lanes that fell back); surrounding-RI queries; node steps with the
// lanes on the first stepping lane's node; node steps where every stepping lane is on one node
enum { kOccSeg = 0, kOccWalk = 2, kOccNode = 4, kOccLeaf = 6, kOccBeam = 8, kOccRef = 10, kOccRi = 12, kOccSame = 14,
       kOccUni = 16, kOccSlots = 18 };
struct Ctr {
    uint32_t seg = 0, nodes = 0, prims = 0, shadow = 0, drops = 0, nans = 0;
    uint32_t refw = 0;  // INW closest-hit queries the wide walk / beam list handed to the LBVH walks (Frame::walk_ctr)
    unsigned long long *wdbg = nullptr;  // diagnostics: this wave's kDbg* row in LDS, or null
#ifdef RT_DIAG_SPLIT
    unsigned long long cyc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // INW phase cycles of this wave (k_inw_pm/sm)
    unsigned long long rnd[2] = {0, 0};  // k_inw_pm: wave cycles of the primary (0) and bounce (1) rounds
#endif
#ifdef RT_DIAG_OCC
    unsigned long long occ[kOccSlots] = {};  // INW lane occupancy per phase (OCC_TALLY), wave-uniform
#endif
};
// INW lane occupancy (diagnostic builds, -DRT_DIAG_OCC; tools/inw_occ.py): per phase, the wave
// iterations and the lanes in them doing that phase's work, summed into Frame::dbg[32 + slot] at exit
#ifdef RT_DIAG_OCC
#define OCC_TALLY(c, k, pred)                                                    \
    do {                                                                         \
        (c).occ[k] += 1;                                                         \
        (c).occ[(k) + 1] += (unsigned long long)__popcll(__ballot(pred));        \
    } while (0)
#else
#define OCC_TALLY(c, k, pred) ((void)0)
#endif
// INW phase split (diagnostic builds, -DRT_DIAG_SPLIT): shader-clock cycles per wave of a phase,
// summed into Frame::dbg slots by the fold kernels at exit
#ifdef RT_DIAG_SPLIT
#define INW_T0(t) const unsigned long long t = (unsigned long long)clock64()
#define INW_CYC(c, k, t) ((c).cyc[k] += (unsigned long long)clock64() - (t))
#else
#define INW_T0(t) ((void)0)
#define INW_CYC(c, k, t) ((void)0)
#endif

// a culled child of a 4-wide node (cull_t, cull4nf)
constexpr float kMiss = __builtin_huge_valf();
// child pairs for packed fp32 arithmetic (v_pk_add_f32 / v_pk_mul_f32)
typedef float pf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pf2 pk(float a, float b) { return pf2{a, b}; }
__device__ __forceinline__ void cswap(float &ta, int &ka, float &tb, int &kb) {
    const bool sw = tb < ta;
    const float t = sw ? tb : ta;
    const int k = sw ? kb : ka;
    tb = sw ? ta : tb; kb = sw ? ka : kb;
    ta = t; ka = k;
}

constexpr float kMaxT = 32000.0f;

struct FStack {  // FLT_STACK (01_BVH...glsl:81-107) in LDS, [slot][thread]
    float *base;
    uint32_t size;
    __device__ __forceinline__ float &at(uint32_t k) { return base[k * kBlock]; }
    __device__ __forceinline__ void push(float v, Ctr &c) {
        if (size < kFStack) { at(size) = v; size++; } else c.drops++;
    }
    __device__ __forceinline__ void push_ray(f3 o, f3 d, float contrib, float bounced, Ctr &c) {
        if (size < kFStack - 7) {
            at(size) = o.x; at(size + 1) = o.y; at(size + 2) = o.z;
            at(size + 3) = d.x; at(size + 4) = d.y; at(size + 5) = d.z;
            at(size + 6) = contrib; at(size + 7) = bounced;
            size += 8;
        } else c.drops++;
    }
    // the top ray (8 floats: origin, direction, contribution, bounced) off the stack
    __device__ __forceinline__ void pop_ray(f3 &o, f3 &d, float &contrib, float &bounced) {
        size -= 8;
        o = f3{at(size), at(size + 1), at(size + 2)};
        d = f3{at(size + 3), at(size + 4), at(size + 5)};
        contrib = at(size + 6);
        bounced = at(size + 7);
    }
    __device__ __forceinline__ void reset(uint32_t n) { size = n; }
    // the top entry is a primary ray (bounced == 0)
    __device__ __forceinline__ bool top_primary() { return size >= 8u && at(size - 1u) == 0.0f; }
    // the wide walks' node stack: the free part above the stack (+ extra floats), kBlock apart;
    // cap = entries left after `spare` slots for branch-free pushes
    __device__ __forceinline__ float *walk_stack(uint32_t extra, int spare, int &cap) {
        cap = kFStack - spare - (int)(size + extra);
        return &at(size + extra);
    }
};

// The same stack for k_inw_pm's GQ instance (DESIGN.md §5.1 "GQ"): the 40 floats in global memory
// ([slot4][lane] float4 columns, `stride` lanes apart; touched about once per segment), the top ray
// in registers -- a segment pops the ray the one before pushed last, so most pops read no memory
// -- and the wide walks' node stack in LDS (kWStack entries per lane, kBlock apart).  The
// capacity and drop semantics are FStack's: size counts every float, pushes drop when it is full.
// Invariant: a primary ray (bounced 0) is only ever the register top (pushed at a sample's start or
// by the MULTIFOCUS chain, popped by the next segment), so top_primary reads no memory.
struct GStack {
    float4 *col;        // this lane's column: slot4 k at col[k * stride]
    uint32_t stride;
    uint32_t size;
    float *ws;          // LDS node stack of the wide walks
    bool rc;            // the top 8 floats are the register ray (r0, r1); their memory is stale
    float4 r0, r1;      // o.xyz d.x | d.yz contrib bounced
    __device__ __forceinline__ float &at(uint32_t k) {
        return reinterpret_cast<float *>(col + (size_t)(k >> 2) * stride)[k & 3u];
    }
    __device__ __forceinline__ void flush() {  // the register ray to its slots size - 8 .. size - 1
        const uint32_t b = size - 8u;
        if ((b & 3u) == 0u) {
            col[(size_t)(b >> 2) * stride] = r0;
            col[(size_t)((b >> 2) + 1u) * stride] = r1;
        } else {
            at(b) = r0.x; at(b + 1) = r0.y; at(b + 2) = r0.z; at(b + 3) = r0.w;
            at(b + 4) = r1.x; at(b + 5) = r1.y; at(b + 6) = r1.z; at(b + 7) = r1.w;
        }
        rc = false;
    }
    __device__ __forceinline__ void push(float v, Ctr &c) {
        if (size < kFStack) {
            if (rc) flush();
            at(size) = v;
            size++;
        } else c.drops++;
    }
    __device__ __forceinline__ void push_ray(f3 o, f3 d, float contrib, float bounced, Ctr &c) {
        if (size < kFStack - 7) {
            if (rc) flush();
            r0 = make_float4(o.x, o.y, o.z, d.x);
            r1 = make_float4(d.y, d.z, contrib, bounced);
            rc = true;
            size += 8;
        } else c.drops++;
    }
    __device__ __forceinline__ void pop_ray(f3 &o, f3 &d, float &contrib, float &bounced) {
        size -= 8;
        if (!rc) {
            if ((size & 3u) == 0u) {
                r0 = col[(size_t)(size >> 2) * stride];
                r1 = col[(size_t)((size >> 2) + 1u) * stride];
            } else {
                r0 = make_float4(at(size), at(size + 1), at(size + 2), at(size + 3));
                r1 = make_float4(at(size + 4), at(size + 5), at(size + 6), at(size + 7));
            }
        }
        rc = false;
        o = f3{r0.x, r0.y, r0.z};
        d = f3{r0.w, r1.x, r1.y};
        contrib = r1.z;
        bounced = r1.w;
    }
    __device__ __forceinline__ void reset(uint32_t n) { size = n; rc = false; }
    __device__ __forceinline__ bool top_primary() { return rc && r1.w == 0.0f; }
    __device__ __forceinline__ float *walk_stack(uint32_t, int spare, int &cap) {
        cap = kWStack - spare;
        return ws;
    }
};

// ident: the rotation is exactly the identity (the host marks the record's type field with + 0.5;
// int(type + 0.1) still reads the type): the wide walk's object test then skips both 3 x 3 products
// and, for a cuboid, reuses the ray's reciprocals (DESIGN.md §5.2 "Unrotated objects")
struct Xf { f3 pos, scale, delta, is, is2; m3 R; int type; bool ident; float extra, ri_acc; };

__device__ __forceinline__ Xf load_xf(const InwScene &S, int g) {
    const float4 *h = S.hot + (size_t)g * 7;
    float4 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], q = h[6];
    Xf x;
    x.pos = mk(a.x, a.y, a.z);
    x.R.c0 = mk(a.w, b.x, b.y); x.R.c1 = mk(b.z, b.w, c.x); x.R.c2 = mk(c.y, c.z, c.w);
    x.scale = mk(d.x, d.y, d.z);
    x.delta = mk(d.w, e.x, e.y);
    x.type = (int)(e.z + 0.1f);
    x.ident = e.z - (float)x.type > 0.25f;
    x.extra = e.w;
    x.is = mk(f.x, f.y, f.z);
    x.is2 = mk(f.w, q.x, q.y);
    x.ri_acc = q.z;
    return x;
}

// TestIntersectAABB 01_BVH...glsl:187-208 (reciprocals of the ray direction hoisted)
// EO (default): the shader's early outs.  !EO: every axis evaluated -- the same result, with the
// node's two loads issued together (see test_aabb_te below); INW-04's reference walks (its
// axis-aligned rays) run 1.1% faster that way at C5, INW-01's early-out code generation is 1% faster at C3
template <bool EO = true>
__device__ __forceinline__ bool test_aabb(float4 n0, float4 n1, f3 o, f3 id, float tlim) {
    float a = (n0.x - o.x) * id.x, b = (n0.w - o.x) * id.x;
    float tmin = fminf(a, b), tmax = fmaxf(a, b);
    if constexpr (EO) {
        if (tmax <= tmin) return false;  // axis 0 re-applied by the loop is idempotent
        a = (n0.y - o.y) * id.y; b = (n1.x - o.y) * id.y;
        tmin = fmaxf(fminf(a, b), tmin); tmax = fminf(fmaxf(a, b), tmax);
        if (tmax <= tmin) return false;
        a = (n0.z - o.z) * id.z; b = (n1.y - o.z) * id.z;
        tmin = fmaxf(fminf(a, b), tmin); tmax = fminf(fmaxf(a, b), tmax);
        if (tmax <= tmin) return false;
        return tlim > 0.0f ? tlim > tmin : true;
    } else {
        bool ok = !(tmax <= tmin);
        a = (n0.y - o.y) * id.y; b = (n1.x - o.y) * id.y;
        tmin = fmaxf(fminf(a, b), tmin); tmax = fminf(fmaxf(a, b), tmax);
        ok = ok && !(tmax <= tmin);
        a = (n0.z - o.z) * id.z; b = (n1.y - o.z) * id.z;
        tmin = fmaxf(fminf(a, b), tmin); tmax = fminf(fmaxf(a, b), tmax);
        ok = ok && !(tmax <= tmin);
        return ok && (tlim > 0.0f ? tlim > tmin : true);
    }
}

// The same test, also returning the entry t it compares (te) -- the wide walk's guard below.  Every
// axis is evaluated (test_aabb returns at the first failing one): the same result and, when it
// passes, the same te.  Without the early outs the compiler issues the box's loads together
// instead of one round trip per axis: C3 201.7 -> 196.5 ms, C5 6.92 -> 6.79 s (same-box A/B,
// profiles/r05_ab_leaf_test.json)
__device__ __forceinline__ bool test_aabb_te(float4 n0, float4 n1, f3 o, f3 id, float tlim, float &te) {
    float a = (n0.x - o.x) * id.x, b = (n0.w - o.x) * id.x;
    float tmin = fminf(a, b), tmax = fmaxf(a, b);
    bool ok = !(tmax <= tmin);
    a = (n0.y - o.y) * id.y; b = (n1.x - o.y) * id.y;
    tmin = fmaxf(fminf(a, b), tmin); tmax = fminf(fmaxf(a, b), tmax);
    ok = ok && !(tmax <= tmin);
    a = (n0.z - o.z) * id.z; b = (n1.y - o.z) * id.z;
    tmin = fmaxf(fminf(a, b), tmin); tmax = fminf(fmaxf(a, b), tmax);
    ok = ok && !(tmax <= tmin);
    te = tmin;
    return ok && (tlim > 0.0f ? tlim > tmin : true);
}

// closest-hit LBVH DFS (01_BVH...glsl:431-473, 04...glsl:524-563, shadow 620-657)
template <bool WANT_NORMAL, bool EO = true, class KS = FStack>
__device__ float inw_traverse(const InwScene &S, KS &K, f3 o, f3 d, float ratio, bool invert,
                              float &tlim, f3 &normal, float &extra, float init_geom, Ctr &c) {
    float final_geom = init_geom;
    const uint32_t I = K.size;
    const f3 id = f3{rcp(d.x), rcp(d.y), rcp(d.z)};
    K.push(0.0f, c);
    for (;;) {
        float geom = -1.0f;
        while (K.size > I) {
            K.size--;
            const int node = (int)K.at(K.size);
            const float4 n0 = S.nodes[2 * node], n1 = S.nodes[2 * node + 1];
            c.nodes++;
            if (test_aabb<EO>(n0, n1, o, id, tlim)) {
                const float left = n1.z;
                if (left > 0.1f) {
                    const float right = left + 1.0f;
                    K.push(invert ? right : left, c);
                    K.push(invert ? left : right, c);
                } else { geom = -left; break; }
            }
        }
        if (!(geom > -0.9f)) break;
        c.prims++;
        // IntersectRay / IntersectRayMinimal
        const Xf x = load_xf(S, (int)geom);
        f3 ov = (o - x.pos) + x.delta * (1.0f - ratio);
        f3 to = tmul(x.R, ov), td = tmul(x.R, d);
        float t = -1.0f;
        if (x.type == 1) t = t_ellipsoid(to, td, x.is);
        else if (x.type == 2) t = t_cuboid(to, td, x.scale);
        if (t > 0.0f && t < tlim) {
            tlim = t;
            final_geom = geom;
            if (WANT_NORMAL) {
                f3 h = to + td * t, nl;
                if (x.type == 1) nl = normalize(f3{h.x * x.is2.x, h.y * x.is2.y, h.z * x.is2.z});
                else if (x.type == 2) nl = cuboid_normal(h, x.scale);
                else nl = f3{0, 0, 0};
                normal = mul(x.R, nl);
                extra = x.extra;
            }
        }
    }
    K.size = I;
    return final_geom;
}

// Surrounding refractive index (01_BVH...glsl:272-345, 486-502)
template <class KS = FStack>
__device__ float inw_surrounding_ri(const InwScene &S, KS &K, f3 hp, float ratio, Ctr &c) {
    float acc = 0.0f;
    uint32_t cnt = 0;
    const uint32_t I = K.size;
    K.push(0.0f, c);
    while (K.size > I) {
        K.size--;
        const int node = (int)K.at(K.size);
        const float4 n0 = S.nodes[2 * node], n1 = S.nodes[2 * node + 1];
        c.nodes++;
        if (hp.x <= n0.w && hp.y <= n1.x && hp.z <= n1.y && hp.x >= n0.x && hp.y >= n0.y && hp.z >= n0.z) {
            const float left = n1.z;
            if (left < 0.1f) {
                c.prims++;
                const Xf x = load_xf(S, (int)(-left));
                f3 v = (hp - x.pos) + x.delta * (1.0f - ratio);
                v = tmul(x.R, v);
                v.x *= x.is.x; v.y *= x.is.y; v.z *= x.is.z;
                bool inside;
                if (x.type == 1) inside = dot(v, v) <= 1.0f;
                else if (x.type == 2) inside = fabsf(v.x) <= 0.5f && fabsf(v.y) <= 0.5f && fabsf(v.z) <= 0.5f;
                else inside = false;
                if (inside) { acc += x.ri_acc; cnt++; }
            } else {
                K.push(left, c);
                K.push(left + 1.0f, c);
            }
        }
    }
    if (acc > 1.0f) acc *= rcp((float)cnt);
    else acc = 1.0f;
    return acc;
}

// ---------------------------------------------------------------- LDS-staged top of the wide BVH
// (measured in DESIGN.md §5): kernels instantiated with LN copy the first n_lnodes wide
// nodes -- the top levels, as bvh4_collapse numbers them breadth first -- into LDS and read them
// there; deeper nodes come from global memory.
// INW wide node: 10 float4, SoA over the 4 children: planes lx ly lz hx hy hz, then lx ly lz again,
// then the child links.  The repeat lets a ray read its near and far planes of axis a at
// a + 3*s_a and a + 3 + 3*s_a (s_a = 1 when d_a < 0): one per-lane offset per axis (inw_wnode_nf_buf).
constexpr int kInwNodeF4 = 10;
// 236 nodes (36.9 KB): what the 3 x 256-lane stacks (120 KB) and k_inw_pm's depth slots (3 KB)
// leave of 160 KB
// (kInwLdsNodes = 236: rt_kernels.hpp)
__shared__ float4 g_inw_lnodes[kInwLdsNodes * kInwNodeF4];
// k_inw_pm / k_inw_sm with LN and InwScene::lring / lring_sm: room for kPmLdsNodes nodes, then the
// 12 waves' fold rings of kPmLdsRing entries (r, g, b planes) in the same LDS (a
// 256-entry window costs 0.5% against 1024, 128 entries 7%; the ring takes the LDS of all but 5
// nodes, which were worth 1.5%, and saves 1% of global ring traffic -- 0.57 against 42 GB of
// L2-to-fabric traffic per C3 frame).  k_inw_pm's ring instances leave those 5 slots unused (its
// walks read no staged node), k_inw_sm's stage the BVH there when it fits
static_assert(kPmLdsNodes * kInwNodeF4 * 16 + 12 * 3 * kPmLdsRing * 4 <= kInwLdsNodes * kInwNodeF4 * 16, "LDS ring");
template <bool LN>
__device__ __forceinline__ const float4 *inw_node_ptr(const InwScene &S, int cur) {
    if (LN && (uint32_t)(cur - 1) < S.n_lnodes) return g_inw_lnodes + kInwNodeF4 * (cur - 1);
    return S.wnodes + kInwNodeF4 * (cur - 1);
}
template <bool LN>
__device__ __forceinline__ void inw_wnode(const InwScene &S, int cur, float4 &lx, float4 &ly, float4 &lz, float4 &hx,
                                          float4 &hy, float4 &hz, float4 &lk) {
    const float4 *nd = inw_node_ptr<LN>(S, cur);
    lx = nd[0]; ly = nd[1]; lz = nd[2]; hx = nd[3]; hy = nd[4]; hz = nd[5]; lk = nd[9];
}
// The near and far planes of the four children for this ray's octant (oa = a + 3*s_a), fetched
// from global memory as buffer loads: the node's byte offset is 32 bits (a node
// index times 160), the octant offsets and the far planes' +48 / the links' +144 fold into the
// instructions, so a node step spends 4 VALU on addresses instead of the 64-bit pointer sums (~10)
// (C3 185.9 -> 184.2 ms on one box, profiles/r06_ab_gq_waves.json)
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
// The buffer-load walk's node layout: 10 float4 (wnodes: the far planes 48 B after the near ones)
// or, with InwScene::cnodes, 7 float4 (the far plane of axis a at a + 3 (1 - s_a): its own offset)
struct WnodeBuf {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t stride, lk;     // bytes per node, offset of the links
    uint32_t fx, fy, fz;     // far-plane offsets of this ray's octant
};
__device__ __forceinline__ WnodeBuf wnode_buf(const InwScene &S, uint32_t oxb, uint32_t oyb, uint32_t ozb) {
    WnodeBuf w;
    const bool c = S.cnodes != nullptr;
    w.stride = c ? 112u : (uint32_t)kInwNodeF4 * 16u;
    w.lk = c ? 96u : 144u;
    // cnodes: near at 16 a + 48 s_a, far at 16 a + 48 (1 - s_a): near + far = 32 a + 48
    w.fx = c ? 48u - oxb : oxb + 48u;
    w.fy = c ? 80u - oyb : oyb + 48u;
    w.fz = c ? 112u - ozb : ozb + 48u;
    // dword 3 = 0x00020000: the gfx9-family raw-buffer format word; num_records bounds the nodes
    w.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(c ? S.cnodes : S.wnodes), (short)0,
                                             (int)(S.n_wnodes * w.stride), 0x00020000);
    return w;
}
template <bool LN>
__device__ __forceinline__ void inw_wnode_nf_buf(const InwScene &S, const WnodeBuf &W, int cur, uint32_t oxb,
                                                 uint32_t oyb, uint32_t ozb, float4 &nx, float4 &ny, float4 &nz,
                                                 float4 &fx, float4 &fy, float4 &fz, float4 &lk) {
    if (LN && (uint32_t)(cur - 1) < S.n_lnodes) {  // ds_read_b128 (a generic pointer would make flat loads)
        const float4 *nd = g_inw_lnodes + kInwNodeF4 * (cur - 1);
        const float4 *px = nd + (oxb >> 4), *py = nd + (oyb >> 4), *pz = nd + (ozb >> 4);
        nx = px[0]; fx = px[3]; ny = py[0]; fy = py[3]; nz = pz[0]; fz = pz[3]; lk = nd[9];
        return;
    }
    const uint32_t b = __umul24((uint32_t)(cur - 1), W.stride);  // v_mul_u32_u24 (ids < 2^24)
    nx = bload4(W.rs, b + oxb); fx = bload4(W.rs, b + W.fx);
    ny = bload4(W.rs, b + oyb); fy = bload4(W.rs, b + W.fy);
    nz = bload4(W.rs, b + ozb); fz = bload4(W.rs, b + W.fz);
    lk = bload4(W.rs, b + W.lk);
}
// FU: one fused multiply-add per plane, plane * (1/d) + (-o * (1/d)), the second term computed
// once per ray (noid).  Its rounding error in t is at most |o| * 2^-23 * |1/d| per axis, against a
// culling-box inflation of e >= 1e-3 (x |1/d| in t), so it stays conservative while
// |o| * 2^-23 < e: the host enables it (InwScene::fused) only when every ray origin (the camera,
// the scene's boxes) lies within 1000 of the origin.  The wide walk runs with finite reciprocals
// only (an infinite one would make every plane's fma NaN).
// The culling test with the planes already split into near and far by the ray's octant.  With a
// finite, nonzero reciprocal, the slab value of a plane is monotone in the plane (each step is a
// correctly rounded monotone function), so the near plane's value is the min of the pair and the
// far plane's the max: the same te and tx bits as min / max of the pair, without the 6 min/max per child.
// The test te <= tx && tx >= -1e-3 && te <= lim is max(te, -1e-3) <= min(tx, lim) (lim > 0).
template <bool FU>
__device__ __forceinline__ void cull4nf(const float4 nx, const float4 ny, const float4 nz, const float4 fx,
                                        const float4 fy, const float4 fz, f3 o, f3 id, f3 noid, float lim, float &t0,
                                        float &t1, float &t2, float &t3) {
    const pf2 ix = pk(id.x, id.x), iy = pk(id.y, id.y), iz = pk(id.z, id.z);
    pf2 a[12];
    const float4 *pl[6] = {&nx, &ny, &nz, &fx, &fy, &fz};
    const pf2 iv[3] = {ix, iy, iz};
    if constexpr (FU) {
        const pf2 nv[3] = {pk(noid.x, noid.x), pk(noid.y, noid.y), pk(noid.z, noid.z)};
#pragma unroll
        for (int k = 0; k < 6; k++) {
            a[2 * k] = __builtin_elementwise_fma(pk(pl[k]->x, pl[k]->y), iv[k % 3], nv[k % 3]);
            a[2 * k + 1] = __builtin_elementwise_fma(pk(pl[k]->z, pl[k]->w), iv[k % 3], nv[k % 3]);
        }
    } else {
        const pf2 ov[3] = {pk(o.x, o.x), pk(o.y, o.y), pk(o.z, o.z)};
#pragma unroll
        for (int k = 0; k < 6; k++) {
            a[2 * k] = (pk(pl[k]->x, pl[k]->y) - ov[k % 3]) * iv[k % 3];
            a[2 * k + 1] = (pk(pl[k]->z, pl[k]->w) - ov[k % 3]) * iv[k % 3];
        }
    }
    // a[2k + h]: plane k (near x, y, z, far x, y, z) of children 2h, 2h + 1
    auto one = [&](float n0, float n1, float n2, float f0, float f1, float f2) {
        const float te = fmaxf(fmaxf(n0, n1), n2), tx = fminf(fminf(f0, f1), f2);
        return fmaxf(te, -1e-3f) <= fminf(tx, lim) ? te : kMiss;
    };
    t0 = one(a[0].x, a[2].x, a[4].x, a[6].x, a[8].x, a[10].x);
    t1 = one(a[0].y, a[2].y, a[4].y, a[6].y, a[8].y, a[10].y);
    t2 = one(a[1].x, a[3].x, a[5].x, a[7].x, a[9].x, a[11].x);
    t3 = one(a[1].y, a[3].y, a[5].y, a[7].y, a[9].y, a[11].y);
}

// ---------------------------------------------------------------- quantised wide nodes (GQ)
// DESIGN.md §5.2 "Quantised nodes": 4 float4 per node instead of 10 (InwScene::qnodes; built by
// rt_build.hip: k_quantize_wnodes), so a node step is 4 loads (64 B, half a cache line) instead of 7
// (112 B), and 1,168 nodes fit the LDS the global FStack frees.  k_inw_pm's GQ instance stages the
// first n_lnodes of them (the top levels, breadth first) in g_inw_qlds.
__shared__ float4 g_inw_qlds[kQLdsNodes * kQNodeF4];
template <bool LN>
__device__ __forceinline__ void inw_qnode(const InwScene &S, int cur, float4 &a, float4 &b, float4 &c, float4 &lk) {
    if (LN && (uint32_t)(cur - 1) < S.n_lnodes) {  // ds_read_b128
        const float4 *nd = g_inw_qlds + kQNodeF4 * (cur - 1);
        a = nd[0]; b = nd[1]; c = nd[2]; lk = nd[3];
        return;
    }
    const float4 *nd = S.qnodes + kQNodeF4 * (cur - 1);
    a = nd[0]; b = nd[1]; c = nd[2]; lk = nd[3];
}
// The fused cull of a quantised node: per axis sf = s * (1/d), of = fma(o, 1/d, -ray.o * (1/d)),
// and each plane's t = fma(byte, sf, of) (one v_cvt_f32_ubyte per plane, pairs of fma packed).
// hx/hy/hz: the ray's direction is negative on that axis, so its near planes are the high ones.
__device__ __forceinline__ float ub(uint32_t v, int k) { return (float)((v >> (8 * k)) & 0xffu); }
__device__ __forceinline__ void cull4q(const float4 a, const float4 b, const float4 c, bool hx, bool hy, bool hz, f3 fid,
                                      f3 noid, float lim, float &t0, float &t1, float &t2, float &t3) {
    const float sf[3] = {a.w * fid.x, b.x * fid.y, b.y * fid.z};
    const float of[3] = {__builtin_fmaf(a.x, fid.x, noid.x), __builtin_fmaf(a.y, fid.y, noid.y),
                         __builtin_fmaf(a.z, fid.z, noid.z)};
    const uint32_t lx = __float_as_uint(b.z), ly = __float_as_uint(b.w), lz = __float_as_uint(c.x);
    const uint32_t ux = __float_as_uint(c.y), uy = __float_as_uint(c.z), uz = __float_as_uint(c.w);
    const uint32_t q[6] = {hx ? ux : lx, hy ? uy : ly, hz ? uz : lz, hx ? lx : ux, hy ? ly : uy, hz ? lz : uz};
    pf2 t[12];  // t[2p + h]: plane p (near x, y, z, far x, y, z) of children 2h, 2h + 1
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const pf2 s2 = pk(sf[p % 3], sf[p % 3]), o2 = pk(of[p % 3], of[p % 3]);
        t[2 * p] = __builtin_elementwise_fma(pk(ub(q[p], 0), ub(q[p], 1)), s2, o2);
        t[2 * p + 1] = __builtin_elementwise_fma(pk(ub(q[p], 2), ub(q[p], 3)), s2, o2);
    }
    auto one = [&](float n0, float n1, float n2, float f0, float f1, float f2) {
        const float te = fmaxf(fmaxf(n0, n1), n2), tx = fminf(fminf(f0, f1), f2);
        return fmaxf(te, -1e-3f) <= fminf(tx, lim) ? te : kMiss;
    };
    t0 = one(t[0].x, t[2].x, t[4].x, t[6].x, t[8].x, t[10].x);
    t1 = one(t[0].y, t[2].y, t[4].y, t[6].y, t[8].y, t[10].y);
    t2 = one(t[1].x, t[3].x, t[5].x, t[7].x, t[9].x, t[11].x);
    t3 = one(t[1].y, t[3].y, t[5].y, t[7].y, t[9].y, t[11].y);
}

// An empty asm that reads the object-space ray: the compiler must have it (so the object record's
// loads) before the caller's box-test branch, instead of sinking the loads behind the branch --
// one round trip for box and record instead of two or three (leaf tests, beam candidates)
__device__ __forceinline__ void keep_before_branch(f3 to, f3 td) {
    asm volatile("" ::"v"(to.x), "v"(to.y), "v"(to.z), "v"(td.x), "v"(td.y), "v"(td.z));
}

// Scalar loads of wave-uniform records (constant address space: s_load through the scalar cache,
// no vector-memory / TA work)
typedef float sv4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const sv4f csv4f;
__device__ __forceinline__ float4 sload4(const float4 *p, int i) {
    const sv4f v = ((const csv4f *)(const void *)p)[i];
    return make_float4(v.x, v.y, v.z, v.w);
}

// ---------------------------------------------------------------- INW wide walk
// The reference's closest hit (01_BVH...glsl:431-473) is the nearest hit among the objects whose
// LBVH leaf box its depth-first walk reaches, ties to the one it reaches first.  With finite ray
// reciprocals the walk reaches every leaf whose own box test passes (an ancestor box holds the
// leaf box, and the slab intervals are monotone in the planes), as long as its 40-float stack
// drops no push -- guaranteed while size + dfs_high <= 40.  Under those conditions the ordered
// walk of the 4-wide culling BVH below, the reference's test of the leaf box with the initial
// limit, the exact object test and the (t, depth-first rank) rule pick the same object with the
// same t; its normal and extra data are then computed as the reference computes them.  The
// walk's stack lives in the free part of the shared stack above K.size.  Node and primitive
// counters count this walk's own work.  ok = false: the conditions do not hold (or the walk's
// stack overflowed) and the caller runs the reference walk.
// One more condition: the reference tests a leaf box against its running limit, so it skips an
// object whose box entry te is not below the best t found so far.  Normally t >= te for a hit
// inside its own box, and then skipping it changes nothing; but where an object's face coincides
// with its box face, rounding can put t an ulp below te.  Any accepted candidate with t < te
// therefore hands the ray to the reference walk (ok = false).
// Postponed leaves are tested once every walking lane holds one; a smaller batch (once this many
// lanes hold one) was an experiment, and 65 = more than a wave = off
constexpr int kInwLeafBatch = 65;
// QN: the quantised nodes (S.qnodes, cull4q; requires FU), LN then meaning the staged ones in g_inw_qlds.
// The hit object's normal and extra data (01_BVH...glsl:FillHitData's inputs) at t = bt.  SP with
// sphere records: from their third float4 (RN(1/RN(s*s)) per axis, extra) -- R = I, so the
// object-space ray is the world one (h's components are nonzero products: the same floats) and
// mul(I, nl) is evaluated with the literal identity, the same operations as with R loaded
template <bool SP>
__device__ __forceinline__ void inw_hit_normal(const InwScene &S, int bg, f3 o, f3 d, float ratio, float bt, f3 &normal,
                                               float &extra) {
    if (SP && S.sph) {
        const float4 p = S.sph[3 * bg], q = S.sph[3 * bg + 1], w = S.sph[3 * bg + 2];
        const f3 ov = (o - mk(p.x, p.y, p.z)) + mk(q.x, q.y, q.z) * (1.0f - ratio);
        const f3 h = ov + d * bt;
        const f3 nl = normalize(f3{h.x * w.x, h.y * w.y, h.z * w.z});
        const m3 I = m3{f3{1.0f, 0.0f, 0.0f}, f3{0.0f, 1.0f, 0.0f}, f3{0.0f, 0.0f, 1.0f}};
        normal = mul(I, nl);
        extra = w.w;
        return;
    }
    const Xf x = load_xf(S, bg);
    f3 ov = (o - x.pos) + x.delta * (1.0f - ratio);
    if (x.ident) {  // R = I: h = ov + d bt has the same floats (d has no zero component here), and
                    // mul(I, nl) with the literal identity repeats the loaded R's operations
        const f3 h = ov + d * bt;
        f3 nl;
        if (x.type == 1) nl = normalize(f3{h.x * x.is2.x, h.y * x.is2.y, h.z * x.is2.z});
        else if (x.type == 2) nl = cuboid_normal(h, x.scale);
        else nl = f3{0, 0, 0};
        const m3 I = m3{f3{1.0f, 0.0f, 0.0f}, f3{0.0f, 1.0f, 0.0f}, f3{0.0f, 0.0f, 1.0f}};
        normal = mul(I, nl);
        extra = x.extra;
        return;
    }
    f3 to = tmul(x.R, ov), td = tmul(x.R, d);
    f3 h = to + td * bt, nl;
    if (x.type == 1) nl = normalize(f3{h.x * x.is2.x, h.y * x.is2.y, h.z * x.is2.z});
    else if (x.type == 2) nl = cuboid_normal(h, x.scale);
    else nl = f3{0, 0, 0};
    normal = mul(x.R, nl);
    extra = x.extra;
}

// SP: the sphere-record object test is compiled in (INW-01 kernels; INW-04's keep their registers)
// The trip (one iteration of the loop below) has one divergent region, the node step; the rest of
// a lane's state machine is selects on integers, so the compiler keeps no loop-carried lane mask
// to re-merge after every region (DESIGN.md §5.2 "The walk trip").  A lane's state is `cur`: a
// node (> 0), a leaf (<= 0: object -cur) or kWalkDone (it walks no more: its stack ran empty or
// overflowed, or the walk's conditions never held for it).  A node step whose nearest surviving
// child is a leaf takes it in its own trip when the lane holds none (DESIGN.md §5.2 "Leaf takes").
constexpr int kWalkDone = (-2147483647 - 1);
template <bool WANT_NORMAL, bool LN = false, bool FU = false, bool QN = false, class KS = FStack, bool SP = true>
__device__ float inw_traverse_wide(const InwScene &S, KS &K, f3 o, f3 d, float ratio, bool invert, float &tlim,
                                   f3 &normal, float &extra, float init_geom, Ctr &c, bool &ok) {
    static_assert(!QN || FU, "quantised nodes are culled with the fused planes");
    const f3 id = f3{rcp(d.x), rcp(d.y), rcp(d.z)};  // the reference's reciprocals (test_aabb)
    ok = S.wnodes != nullptr && K.size + S.dfs_high <= (uint32_t)kFStack && __builtin_isfinite(id.x) &&
         __builtin_isfinite(id.y) && __builtin_isfinite(id.z) && d.x != 0.0f && d.y != 0.0f && d.z != 0.0f;
    if (!__any(ok)) return init_geom;
    const float tlim0 = tlim;
    float bt = tlim0;
    int bg = -1;
    uint32_t br = 0xffffffffu;
    const uint32_t *rank = S.rank + (invert ? S.n : 0u);
    // the culling planes use the reference's (correctly rounded) reciprocals too: no second set of
    // three (round 5 took v_rcp approximations), C3 184.6 -> 184.0 ms (profiles/r06_ab_walk_tweaks.json)
    const f3 fid = id;
    const f3 noid = f3{-(o.x * fid.x), -(o.y * fid.y), -(o.z * fid.z)};  // the fused cull's per-ray term (FU)
    // the fused planes need a finite per-ray term: a direction component near the smallest normal
    // float with |o| ~ 10^3 overflows it, and every fma would be -inf or NaN (every child culled);
    // such a ray takes the reference walk
    if (FU) ok = ok && __builtin_isfinite(noid.x) && __builtin_isfinite(noid.y) && __builtin_isfinite(noid.z);
    // 3 spare slots for branch-free pushes
    int cap;
    float *const wsb = K.walk_stack(0u, 3, cap);  // entry p at wsb[p * kBlock]
    const uint32_t ox = d.x < 0.0f ? 3u : 0u, oy = d.y < 0.0f ? 4u : 1u, oz = d.z < 0.0f ? 5u : 2u;
    const WnodeBuf wrs = wnode_buf(S, ox * 16u, oy * 16u, oz * 16u);
    int sp = 0, pend = -1, cur = S.wroot;
    if (!LN && S.wbins > 1u) {  // the ray's time-bin tree (the staged nodes are the swept tree's)
        const int b = min((int)(ratio * (float)S.wbins), (int)S.wbins - 1);
        cur = 1 + (int)S.wbin_base + b * (int)S.wbin_stride;
    }
    cur = ok ? cur : kWalkDone;
    float lim = bt * 1.0001f + 1e-3f;
    // the leaf-entry guard: the best hit's leaf-box entry, and the smallest t of the
    // other hits; the reference's walk accepts the best hit for certain when t2 > bte
    float bte = 0.0f, t2 = tlim0;
    auto leaf = [&](int g) {
        c.prims++;
        const float4 n0 = S.leafbox[2 * g], n1 = S.leafbox[2 * g + 1];
        float te, t = -1.0f;
        if (SP && S.sph) {  // a sphere scene: 2 float4 instead of 7, no rotation (R = I: tmul(R, v) = v)
            const float4 p = S.sph[3 * g], q = S.sph[3 * g + 1];
            const bool inb = test_aabb_te(n0, n1, o, id, tlim0, te);
            const f3 to = (o - mk(p.x, p.y, p.z)) + mk(q.x, q.y, q.z) * (1.0f - ratio);
            keep_before_branch(to, d);
            if (!inb) return;
            t = t_ellipsoid(to, d, f3{p.w, p.w, p.w});
        } else {
            const Xf x = load_xf(S, g);  // loaded with the box, before its test: one memory latency
            const bool inb = test_aabb_te(n0, n1, o, id, tlim0, te);
            const f3 ov = (o - x.pos) + x.delta * (1.0f - ratio);
            if (x.ident) {  // R = I: tmul(R, v) is v (up to zero signs, which t cannot see; d has no
                            // zero component here), and rcp(d) is the ray's own id
                keep_before_branch(ov, d);
                if (!inb) return;
                if (x.type == 1) t = t_ellipsoid(ov, d, x.is);
                else if (x.type == 2) t = t_cuboid_rcp(ov, id, x.scale);
            } else {
                f3 to = tmul(x.R, ov), td = tmul(x.R, d);
                keep_before_branch(to, td);
                if (!inb) return;
                if (x.type == 1) t = t_ellipsoid(to, td, x.is);
                else if (x.type == 2) t = t_cuboid(to, td, x.scale);
            }
        }
        if (t > 0.0f && t < tlim0) {
            const uint32_t r = rank[g];
            if (t < bt || (t == bt && r < br)) {
                if (bg >= 0) t2 = fminf(t2, bt);
                bt = t; bg = g; br = r; bte = te; lim = bt * 1.0001f + 1e-3f;
            } else {
                t2 = fminf(t2, t);
            }
        }
    };
    for (;;) {
        OCC_TALLY(c, kOccWalk, cur != kWalkDone);
        OCC_TALLY(c, kOccNode, cur > 0);
#ifdef RT_DIAG_OCC
        {  // how often a node step's lanes share one node (a wave-uniform node load would serve them)
            const unsigned long long m = __ballot(cur > 0);
            if (m) {
                const int c0 = __builtin_amdgcn_readlane(cur, (int)__builtin_ctzll(m));
                const bool on = cur == c0;
                OCC_TALLY(c, kOccSame, on);
                if (__ballot(cur > 0 && cur != c0) == 0ull) OCC_TALLY(c, kOccUni, on);
            }
        }
#endif
        // the node step: what it leaves for a lane not on a node is "stay": the same cur and sp,
        // a nearest child that is no miss
        int nxt = cur, p = sp;
        float tn = 0.0f;
        if (cur > 0) {
            float4 lk;
            float c0, c1, c2, c3;
            if constexpr (QN) {
                float4 qa, qb, qc;
                inw_qnode<LN>(S, cur, qa, qb, qc, lk);
                cull4q(qa, qb, qc, ox != 0u, oy != 1u, oz != 2u, fid, noid, lim, c0, c1, c2, c3);
            } else {
                float4 nx, ny, nz, fx, fy, fz;
                inw_wnode_nf_buf<LN>(S, wrs, cur, ox * 16u, oy * 16u, oz * 16u, nx, ny, nz, fx, fy, fz, lk);
                cull4nf<FU>(nx, ny, nz, fx, fy, fz, o, fid, noid, lim, c0, c1, c2, c3);
            }
            c.nodes += 4;
            int k0 = __float_as_int(lk.x), k1 = __float_as_int(lk.y), k2 = __float_as_int(lk.z),
                k3 = __float_as_int(lk.w);
            cswap(c0, k0, c1, k1); cswap(c2, k2, c3, k3);
            cswap(c0, k0, c2, k2); cswap(c1, k1, c3, k3);
            cswap(c1, k1, c2, k2);
            // branch-free pushes, farthest first (a miss is overwritten before a pop)
            wsb[p * kBlock] = __int_as_float(k3); p += c3 != kMiss;
            wsb[p * kBlock] = __int_as_float(k2); p += c2 != kMiss;
            wsb[p * kBlock] = __int_as_float(k1); p += c1 != kMiss;
            nxt = k0;
            tn = c0;
        }
        // (a lane not on a node keeps p = sp, which is <= cap or -1.  This needs cap >= 0, that is
        // K.size <= kFStack - 3 at entry: the render kernels walk after pop_ray, size <= 32, the
        // query kernel at size 0, and GStack's cap is a constant.  With cap < 0 an idle lane would
        // count as overflowed and go to the reference walk: the same result, for more work)
        const bool over = p > cap;
        // a leaf is taken (and the lane pops) unless the lane still holds one: then it waits on it.
        // The leaf is the lane's own state or, in the node step's own trip, the step's nearest
        // surviving child (nxt is either: a lane not on a node has nxt = cur and no miss)
        const bool miss = tn == kMiss;
        const bool take = nxt <= 0 && nxt != kWalkDone && !miss && pend < 0;
        pend = take ? -nxt : pend;
        const bool pop = take || miss;
        // every lane reads the entry under its top (its own column: q <= cap + 2, the spare slots;
        // at p <= 0 a value nobody uses)
        const int q = max(p - 1, 0);
        const int top = __float_as_int(wsb[q * kBlock]);
        cur = pop ? (p > 0 ? top : kWalkDone) : nxt;
        sp = pop ? q : p;
        // a push past cap ends the lane's walk; sp = -1 carries the overflow to the end
        cur = over ? kWalkDone : cur;
        sp = over ? -1 : sp;
        // postponed leaves are tested once every walking lane holds one (or kInwLeafBatch lanes)
        if (__all(cur == kWalkDone || pend >= 0) ||
            (kInwLeafBatch < 65 && __popcll(__ballot(pend >= 0)) >= (unsigned)kInwLeafBatch)) {
            OCC_TALLY(c, kOccLeaf, pend >= 0);
            if (pend >= 0) { leaf(pend); pend = -1; }
            if (__all(cur == kWalkDone)) break;
        }
    }
    // the best hit passes the reference's leaf-box test for certain unless another hit's t could
    // have lowered its running limit to the box entry first (rare: a face on its box, C5)
    if (sp < 0 || (bg >= 0 && !(t2 > bte))) ok = false;
    if (!ok) return init_geom;
    if (bg < 0) return init_geom;
    tlim = bt;
    if (WANT_NORMAL) inw_hit_normal<SP>(S, bg, o, d, ratio, bt, normal, extra);
    return (float)bg;
}

// load_xf by scalar loads (sload4): the beam lists' candidates are the same object for every active
// lane of one pixel (they step through the list together)
__device__ __forceinline__ Xf load_xf_s(const InwScene &S, int g) {  // load_xf of a wave-uniform g
    const float4 a = sload4(S.hot, 7 * g), b = sload4(S.hot, 7 * g + 1), c = sload4(S.hot, 7 * g + 2),
                 d = sload4(S.hot, 7 * g + 3), e = sload4(S.hot, 7 * g + 4), f = sload4(S.hot, 7 * g + 5),
                 q = sload4(S.hot, 7 * g + 6);
    Xf x;
    x.pos = mk(a.x, a.y, a.z);
    x.R.c0 = mk(a.w, b.x, b.y); x.R.c1 = mk(b.z, b.w, c.x); x.R.c2 = mk(c.y, c.z, c.w);
    x.scale = mk(d.x, d.y, d.z);
    x.delta = mk(d.w, e.x, e.y);
    x.type = (int)(e.z + 0.1f);
    x.ident = e.z - (float)x.type > 0.25f;
    x.extra = e.w;
    x.is = mk(f.x, f.y, f.z);
    x.is2 = mk(f.w, q.x, q.y);
    x.ri_acc = q.z;
    return x;
}

// Closest hit of a primary ray from its pixel's beam list (DESIGN.md §5 "Pixel beams").  The list
// holds every object whose culling box the beam of the pixel's primary rays can cross, in the
// order of the central ray's entry t into the box inflated by beam_R; a sample ray hitting object
// j at t has entry(j) <= t * beam_kappa, so the candidates past bt * kappa (+ slack) cannot win.
// Each candidate gets the wide walk's leaf test (the reference's leaf box with the initial limit,
// the exact test, the leaf-entry guard, the (t, depth-first rank) rule), so the winner is the
// wide walk's and the reference walk's.  ok = false: the list does not decide this ray (no list,
// the wide walk's conditions fail, or candidates beyond the stored ones could still win).
template <bool WANT_NORMAL, class KS = FStack>
__device__ float inw_closest_beam(const InwScene &S, const KS &K, f3 o, f3 d, float ratio, bool invert, float &tlim,
                                  f3 &normal, float &extra, float init_geom, Ctr &c, uint32_t unit, bool &ok) {
    const f3 id = f3{rcp(d.x), rcp(d.y), rcp(d.z)};  // the reference's reciprocals (test_aabb)
    // the ray's time bin's list (beam_bins > 1): bin b's counts, cuts and lists after those of bins < b
    const uint32_t bo = S.beam_bins > 1u ? min((uint32_t)(ratio * (float)S.beam_bins), S.beam_bins - 1u) * S.beam_units : 0u;
    const uint32_t nw = S.beam_n[bo + unit], n = nw & 0xffu;  // k_inw_beam: offset in the block's region << 8 | count
    ok = nw != kBeamOff && K.size + S.dfs_high <= (uint32_t)kFStack && __builtin_isfinite(id.x) &&
         __builtin_isfinite(id.y) && __builtin_isfinite(id.z) && d.x != 0.0f && d.y != 0.0f && d.z != 0.0f;
    const float tlim0 = tlim;
    float bt = tlim0;
    int bg = -1;
    uint32_t br = 0xffffffffu;
    const uint32_t *rank = S.rank + (invert ? S.n : 0u);
    const size_t lbase = ((size_t)bo + (unit & ~63u)) * S.beam_cap + (nw >> 8);
    const uint2 *list = S.beam + lbase;
    const uint32_t *list16 = reinterpret_cast<const uint32_t *>(S.beam) + lbase;
    const float kap = S.beam_kappa;
    float lim = bt * kap + 0.01f;
    bool ovf = false;
    float bte = 0.0f, t2 = tlim0;  // the leaf-entry guard's state (inw_traverse_wide)
    uint32_t k = 0;
    // packed entries hold t rounded down (and 0 for a negative entry): the list stays sorted, and a
    // ray stops at a stored t above lim no earlier than at the exact one
    auto entry = [&](uint32_t j) {
        if (S.beam16) {
            const uint32_t p = list16[j];
            return make_uint2(p & 0xffffu, p & 0xffff0000u);
        }
        return list[j];
    };
    uint2 en = ok && n > 0u ? entry(0) : make_uint2(0u, 0u);  // the next entry, loaded a candidate ahead
    for (;;) {
        bool act = ok && k < n;
        uint2 e = make_uint2(0u, 0u);
        if (act) {
            e = en;
            act = __uint_as_float(e.y) <= lim;
        }
        if (!__any(act)) break;
        OCC_TALLY(c, kOccBeam, act);
        if (act) {
            if (k + 1u < n) en = entry(k + 1u);
            const int g = (int)e.x;
            c.prims++;
            float4 n0, n1;
            float te, t = -1.0f;
            bool inb;
            // one candidate for every active lane (a wave's lanes trace samples of one pixel and step
            // through its list together): scalar loads, C3 184.7 -> 182.5 ms
            // (profiles/r06_ab_beam_sload_ring_il.json)
            const int g0 = __builtin_amdgcn_readfirstlane(g);
            const bool uni_g = __ballot(g != g0) == 0ull;
            if (S.sph) {  // a sphere scene (inw_traverse_wide's leaf test): 2 float4, R = I
                float4 p, q;
                if (uni_g) {
                    n0 = sload4(S.leafbox, 2 * g0); n1 = sload4(S.leafbox, 2 * g0 + 1);
                    p = sload4(S.sph, 3 * g0); q = sload4(S.sph, 3 * g0 + 1);
                } else {
                    n0 = S.leafbox[2 * g]; n1 = S.leafbox[2 * g + 1];
                    p = S.sph[3 * g]; q = S.sph[3 * g + 1];
                }
                inb = test_aabb_te(n0, n1, o, id, tlim0, te);
                const f3 to = (o - mk(p.x, p.y, p.z)) + mk(q.x, q.y, q.z) * (1.0f - ratio);
                keep_before_branch(to, d);
                if (inb) t = t_ellipsoid(to, d, f3{p.w, p.w, p.w});
            } else {
                Xf x;
                if (uni_g) {
                    n0 = sload4(S.leafbox, 2 * g0); n1 = sload4(S.leafbox, 2 * g0 + 1);
                    x = load_xf_s(S, g0);
                } else {
                    n0 = S.leafbox[2 * g]; n1 = S.leafbox[2 * g + 1];
                    x = load_xf(S, g);
                }
                inb = test_aabb_te(n0, n1, o, id, tlim0, te);
                f3 ov = (o - x.pos) + x.delta * (1.0f - ratio);
                f3 to = tmul(x.R, ov), td = tmul(x.R, d);
                keep_before_branch(to, td);
                if (inb) {
                    if (x.type == 1) t = t_ellipsoid(to, td, x.is);
                    else if (x.type == 2) t = t_cuboid(to, td, x.scale);
                }
            }
            if (inb) {
                if (t > 0.0f && t < tlim0) {
                    const uint32_t r = rank[g];
                    if (t < bt || (t == bt && r < br)) {  // the leaf-entry guard as in inw_traverse_wide
                        if (bg >= 0) t2 = fminf(t2, bt);
                        bt = t; bg = g; br = r; bte = te; lim = bt * kap * 1.00001f + 0.01f;
                    } else {
                        t2 = fminf(t2, t);
                    }
                }
            }
            k++;
        }
    }
    if (bg >= 0 && !(t2 > bte)) ovf = true;
    // candidates not stored (entry >= cut) could still be reached below lim
    if (ok && (ovf || !(lim < S.beam_cut[bo + unit]))) ok = false;
    if (!ok) return init_geom;
    if (bg < 0) return init_geom;
    tlim = bt;
    if (WANT_NORMAL) inw_hit_normal<true>(S, bg, o, d, ratio, bt, normal, extra);
    return (float)bg;
}

// The surrounding-RI walk (01_BVH...glsl:486-502) sums the RI of every object holding the point,
// in its depth-first order (right child first).  Same conditions as above: the objects are those
// whose leaf box holds the point (inclusive, as the reference compares) and whose inside test
// passes, found by a walk of the culling BVH and summed in rank order.  ok = false: fall back.
constexpr int kRiMax = 8;
template <bool LN = false, class KS = FStack>
__device__ float inw_surrounding_ri_wide(const InwScene &S, KS &K, f3 hp, float ratio, Ctr &c, bool &ok) {
    ok = S.wnodes != nullptr && K.size + S.dfs_high <= (uint32_t)kFStack;
    if (!__any(ok)) return 1.0f;
    int cap;
    float *const wsb = K.walk_stack(0u, 4, cap);  // entry p at wsb[p * kBlock]
    uint32_t rk[kRiMax];
    float rv[kRiMax];
    int nin = 0;
    int sp = 0, cur = S.wroot;
    bool walking = ok;
    while (walking) {
        if (cur > 0) {
            float4 lx, ly, lz, hx, hy, hz, lk;
            inw_wnode<LN>(S, cur, lx, ly, lz, hx, hy, hz, lk);
            c.nodes += 4;
            const bool i0 = hp.x >= lx.x && hp.x <= hx.x && hp.y >= ly.x && hp.y <= hy.x && hp.z >= lz.x && hp.z <= hz.x;
            const bool i1 = hp.x >= lx.y && hp.x <= hx.y && hp.y >= ly.y && hp.y <= hy.y && hp.z >= lz.y && hp.z <= hz.y;
            const bool i2 = hp.x >= lx.z && hp.x <= hx.z && hp.y >= ly.z && hp.y <= hy.z && hp.z >= lz.z && hp.z <= hz.z;
            const bool i3 = hp.x >= lx.w && hp.x <= hx.w && hp.y >= ly.w && hp.y <= hy.w && hp.z >= lz.w && hp.z <= hz.w;
            int p = sp;
            wsb[p * kBlock] = lk.x; p += i0;
            wsb[p * kBlock] = lk.y; p += i1;
            wsb[p * kBlock] = lk.z; p += i2;
            wsb[p * kBlock] = lk.w; p += i3;
            if (p > cap) { ok = false; break; }
            sp = p;
        } else {
            const int g = -cur;
            c.prims++;
            const float4 n0 = S.leafbox[2 * g], n1 = S.leafbox[2 * g + 1];
            const Xf x = load_xf(S, g);  // loaded with the box, before its test
            if (hp.x <= n0.w && hp.y <= n1.x && hp.z <= n1.y && hp.x >= n0.x && hp.y >= n0.y && hp.z >= n0.z) {
                f3 v = (hp - x.pos) + x.delta * (1.0f - ratio);
                v = tmul(x.R, v);
                v.x *= x.is.x; v.y *= x.is.y; v.z *= x.is.z;
                bool inside;
                if (x.type == 1) inside = dot(v, v) <= 1.0f;
                else if (x.type == 2) inside = fabsf(v.x) <= 0.5f && fabsf(v.y) <= 0.5f && fabsf(v.z) <= 0.5f;
                else inside = false;
                if (inside) {
                    if (nin == kRiMax) { ok = false; break; }
                    rk[nin] = S.rank[g];
                    rv[nin] = x.ri_acc;
                    nin++;
                }
            }
        }
        if (sp == 0) walking = false;
        else cur = __float_as_int(wsb[(--sp) * kBlock]);
    }
    if (!ok) return 1.0f;
    // sum in the reference's order (insertion sort by rank; a handful of objects at most)
    for (int i = 1; i < nin; i++)
        for (int j = i; j > 0 && rk[j] < rk[j - 1]; j--) {
            const uint32_t tr = rk[j]; rk[j] = rk[j - 1]; rk[j - 1] = tr;
            const float tv = rv[j]; rv[j] = rv[j - 1]; rv[j - 1] = tv;
        }
    float acc = 0.0f;
    for (int i = 0; i < nin; i++) acc += rv[i];
    if (acc > 1.0f) acc *= rcp((float)nin);
    else acc = 1.0f;
    return acc;
}

// The surrounding-RI walk (inw_surrounding_ri_wide) through the RI grid: the objects whose
// leaf box holds the point are all listed in the point's cell (their boxes were entered with a
// margin wider than the rounding of the cell index), so testing that cell's objects with the
// walk's comparisons finds the same objects; they are summed in depth-first rank order.
__device__ float inw_ri_grid(const InwScene &S, f3 hp, float ratio, Ctr &c, bool &ok) {
    ok = true;
    if (!(hp.x >= S.ri_lo[0] && hp.y >= S.ri_lo[1] && hp.z >= S.ri_lo[2] && hp.x <= S.ri_hi[0] &&
          hp.y <= S.ri_hi[1] && hp.z <= S.ri_hi[2]))
        return 1.0f;  // outside every leaf box (or NaN: no comparison holds, as in the walk)
    const int cx = min(max((int)((hp.x - S.ri_lo[0]) * S.ri_inv[0]), 0), S.ri_dim[0] - 1);
    const int cy = min(max((int)((hp.y - S.ri_lo[1]) * S.ri_inv[1]), 0), S.ri_dim[1] - 1);
    const int cz = min(max((int)((hp.z - S.ri_lo[2]) * S.ri_inv[2]), 0), S.ri_dim[2] - 1);
    const uint32_t cell = ((uint32_t)cz * (uint32_t)S.ri_dim[1] + (uint32_t)cy) * (uint32_t)S.ri_dim[0] + (uint32_t)cx;
    const uint32_t b = S.ri_cells[cell], e = S.ri_cells[cell + 1];
    uint32_t rk[kRiMax];
    float rv[kRiMax];
    int nin = 0;
    // an object's leaf box, record and rank are loaded together (one round trip; the hit object
    // itself is always listed and inside its box), the next id while this one is tested
    uint32_t gn = b < e ? S.ri_ids[b] : 0u;
    for (uint32_t k = b; k < e; k++) {
        const int g = (int)gn;
        if (k + 1 < e) gn = S.ri_ids[k + 1];
        c.prims++;
        const float4 n0 = S.leafbox[2 * g], n1 = S.leafbox[2 * g + 1];
        const uint32_t rg = S.rank[g];
        bool inside;
        float ri;
        if (S.sph) {  // sphere records (RI in q.w): R = I, so v = ov * is, the same floats
            const float4 p = S.sph[3 * g], q = S.sph[3 * g + 1];
            if (!(hp.x <= n0.w && hp.y <= n1.x && hp.z <= n1.y && hp.x >= n0.x && hp.y >= n0.y && hp.z >= n0.z)) continue;
            f3 v = (hp - mk(p.x, p.y, p.z)) + mk(q.x, q.y, q.z) * (1.0f - ratio);
            v.x *= p.w; v.y *= p.w; v.z *= p.w;
            inside = dot(v, v) <= 1.0f;
            ri = q.w;
        } else {
            const Xf x = load_xf(S, g);
            if (!(hp.x <= n0.w && hp.y <= n1.x && hp.z <= n1.y && hp.x >= n0.x && hp.y >= n0.y && hp.z >= n0.z)) continue;
            f3 v = (hp - x.pos) + x.delta * (1.0f - ratio);
            v = tmul(x.R, v);
            v.x *= x.is.x; v.y *= x.is.y; v.z *= x.is.z;
            if (x.type == 1) inside = dot(v, v) <= 1.0f;
            else if (x.type == 2) inside = fabsf(v.x) <= 0.5f && fabsf(v.y) <= 0.5f && fabsf(v.z) <= 0.5f;
            else inside = false;
            ri = x.ri_acc;
        }
        if (inside) {
            if (nin == kRiMax) { ok = false; return 1.0f; }
            rk[nin] = rg;
            rv[nin] = ri;
            nin++;
        }
    }
    for (int i = 1; i < nin; i++)
        for (int j = i; j > 0 && rk[j] < rk[j - 1]; j--) {
            const uint32_t tr = rk[j]; rk[j] = rk[j - 1]; rk[j - 1] = tr;
            const float tv = rv[j]; rv[j] = rv[j - 1]; rv[j - 1] = tv;
        }
    float acc = 0.0f;
    for (int i = 0; i < nin; i++) acc += rv[i];
    if (acc > 1.0f) acc *= rcp((float)nin);
    else acc = 1.0f;
    return acc;
}

// ---------------------------------------------------------------- stackless LBVH walks
// The reference walks its LBVH depth first with the shared 40-float stack (01_BVH...glsl:431-476;
// RI: 486-502, 272-345).  Its node buffer is written breadth first with the two children of a node
// next to each other and rightData = the parent (lbvh.h:236-269), so the left children sit at odd
// indices and their right siblings at the next one; the host checks that layout (InwScene::sl).
// The same depth-first order then needs no stack: the closest-hit walk pops (invert ? left :
// right) first (it pushes the other one first, :456-460), so after the first child's subtree
// comes its sibling, and after the second child's subtree the walk climbs to the parent and on.
// Every node the reference pops is visited once, in the same order, with the same running limit:
// the same box tests, leaves, hit, node and primitive counts.  Where a reference push could drop
// (size + dfs_high > 40) the result depends on the stack, and the caller runs the stack walk.
// Climbing past a second child reads one float, the parent's own parent link.
template <bool LN>
__device__ __forceinline__ void lbvh_node(const InwScene &S, uint32_t i, float4 &n0, float4 &n1) {
    if (LN && i < S.n_blds) {  // LDS-staged top of the LBVH (ds_read_b128)
        n0 = g_inw_lnodes[2 * i];
        n1 = g_inw_lnodes[2 * i + 1];
        return;
    }
    n0 = S.nodes[2 * i];
    n1 = S.nodes[2 * i + 1];
}
template <bool LN>
__device__ __forceinline__ float lbvh_parent(const InwScene &S, uint32_t i) {
    if (LN && i < S.n_blds) return g_inw_lnodes[2 * i + 1].w;
    return reinterpret_cast<const float *>(S.nodes)[8 * (size_t)i + 7];
}
// The node after the subtree of `cur` in depth-first order (0 = the walk is over).  first_odd:
// the first-visited child of a node has an odd index (invert) or an even one.  par: cur's parent.
template <bool LN>
__device__ __forceinline__ uint32_t lbvh_next(const InwScene &S, uint32_t cur, float par, uint32_t first_odd) {
    for (;;) {
        if (cur == 0u) return 0u;
        if ((cur & 1u) == first_odd) return first_odd ? cur + 1u : cur - 1u;  // its sibling comes next
        cur = (uint32_t)par;  // a second child: its parent's subtree is done
        if (cur == 0u) return 0u;
        par = lbvh_parent<LN>(S, cur);
    }
}

template <bool WANT_NORMAL, bool LN = false, bool EO = true>
__device__ float inw_traverse_sl(const InwScene &S, f3 o, f3 d, float ratio, bool invert, float &tlim, f3 &normal,
                                 float &extra, float init_geom, Ctr &c) {
    float final_geom = init_geom;
    const f3 id = f3{rcp(d.x), rcp(d.y), rcp(d.z)};
    const uint32_t first_odd = invert ? 1u : 0u;
    uint32_t cur = 0u;
    for (;;) {
        float4 n0, n1;
        lbvh_node<LN>(S, cur, n0, n1);
        c.nodes++;
        if (test_aabb<EO>(n0, n1, o, id, tlim)) {
            const float left = n1.z;
            if (left > 0.1f) {  // descend: the child the reference pops first
                const uint32_t L = (uint32_t)left;
                cur = invert ? L : L + 1u;
                continue;
            }
            c.prims++;  // IntersectRay / IntersectRayMinimal (as inw_traverse)
            const float geom = -left;
            const Xf x = load_xf(S, (int)geom);
            f3 ov = (o - x.pos) + x.delta * (1.0f - ratio);
            f3 to = tmul(x.R, ov), td = tmul(x.R, d);
            float t = -1.0f;
            if (x.type == 1) t = t_ellipsoid(to, td, x.is);
            else if (x.type == 2) t = t_cuboid(to, td, x.scale);
            if (t > 0.0f && t < tlim) {
                tlim = t;
                final_geom = geom;
                if (WANT_NORMAL) {
                    f3 h = to + td * t, nl;
                    if (x.type == 1) nl = normalize(f3{h.x * x.is2.x, h.y * x.is2.y, h.z * x.is2.z});
                    else if (x.type == 2) nl = cuboid_normal(h, x.scale);
                    else nl = f3{0, 0, 0};
                    normal = mul(x.R, nl);
                    extra = x.extra;
                }
            }
        }
        cur = lbvh_next<LN>(S, cur, n1.w, first_odd);
        if (cur == 0u) break;
    }
    return final_geom;
}

// the surrounding-RI point walk (01_BVH...glsl:486-502): pushes left, then left + 1, so it pops
// the right (even) child first
template <bool LN = false>
__device__ float inw_surrounding_ri_sl(const InwScene &S, f3 hp, float ratio, Ctr &c) {
    float acc = 0.0f;
    uint32_t cnt = 0, cur = 0u;
    for (;;) {
        float4 n0, n1;
        lbvh_node<LN>(S, cur, n0, n1);
        c.nodes++;
        if (hp.x <= n0.w && hp.y <= n1.x && hp.z <= n1.y && hp.x >= n0.x && hp.y >= n0.y && hp.z >= n0.z) {
            const float left = n1.z;
            if (!(left < 0.1f)) {
                cur = (uint32_t)left + 1u;
                continue;
            }
            c.prims++;
            const Xf x = load_xf(S, (int)(-left));
            f3 v = (hp - x.pos) + x.delta * (1.0f - ratio);
            v = tmul(x.R, v);
            v.x *= x.is.x; v.y *= x.is.y; v.z *= x.is.z;
            bool inside;
            if (x.type == 1) inside = dot(v, v) <= 1.0f;
            else if (x.type == 2) inside = fabsf(v.x) <= 0.5f && fabsf(v.y) <= 0.5f && fabsf(v.z) <= 0.5f;
            else inside = false;
            if (inside) { acc += x.ri_acc; cnt++; }
        }
        cur = lbvh_next<LN>(S, cur, n1.w, 0u);
        if (cur == 0u) break;
    }
    if (acc > 1.0f) acc *= rcp((float)cnt);
    else acc = 1.0f;
    return acc;
}

// EO: the reference walks' box test with the shader's early outs (INW-01) or all axes (INW-04)
// QN: the wide walk reads the quantised nodes (LN: the staged ones); the LBVH walks then read no
// staged node (their LDS is not filled in the GQ instance)
template <bool WANT_NORMAL, bool LN = false, bool FU = false, bool EO = true, bool QN = false, class KS = FStack>
__device__ __forceinline__ float inw_closest(const InwScene &S, KS &K, f3 o, f3 d, float ratio, bool invert,
                                             float &tlim, f3 &normal, float &extra, float init_geom, Ctr &c) {
    bool ok = false;
    const float g = inw_traverse_wide<WANT_NORMAL, LN, FU, QN, KS, EO>(S, K, o, d, ratio, invert, tlim, normal, extra,
                                                                       init_geom, c, ok);
    OCC_TALLY(c, kOccRef, !ok);
    if (ok) return g;
    c.refw++;
    if (S.sl && K.size + S.dfs_high <= (uint32_t)kFStack)  // no push of the reference walk could drop
        return inw_traverse_sl<WANT_NORMAL, LN && !QN, EO>(S, o, d, ratio, invert, tlim, normal, extra, init_geom, c);
    return inw_traverse<WANT_NORMAL, EO>(S, K, o, d, ratio, invert, tlim, normal, extra, init_geom, c);
}
template <bool LN = false, class KS = FStack>
__device__ __forceinline__ float inw_ri(const InwScene &S, KS &K, f3 hp, float ratio, Ctr &c) {
    bool ok = false;
    if (S.ri_cells && K.size + S.dfs_high <= (uint32_t)kFStack) {  // no push of the walk could drop
        const float g = inw_ri_grid(S, hp, ratio, c, ok);
        if (ok) return g;
    }
    const float r = inw_surrounding_ri_wide<LN>(S, K, hp, ratio, c, ok);
    if (ok) return r;
    if (S.sl && K.size + S.dfs_high <= (uint32_t)kFStack) return inw_surrounding_ri_sl<LN>(S, hp, ratio, c);
    return inw_surrounding_ri(S, K, hp, ratio, c);
}

}  // namespace rtk
