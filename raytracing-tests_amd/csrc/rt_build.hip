// rt_build.hip -- the INW wide walk's per-redraw structures built on the device (DESIGN.md §4-5
// "Device build"), from the LBVH the device just built (rt_lbvh.hip; the reference rebuilds it on
// every redraw, In-Next-Week/base.h:96-175, ConstructLBVH_Buff at :135-142):
//   - every object's LBVH leaf box, and its culling box (the leaf box inflated as the host build
//     inflates it, rtamd::inw_wide_build);
//   - the depth-first ranks of the objects in the reference walk's order for both child orders,
//     and the walk's stack high-water mark (each from the object's / node's path to the root);
//   - a binary SAH tree over the culling boxes, built top-down one level per launch with 32
//     centroid bins per axis (a block per node range), collapsed to the 4-wide culling BVH the
//     kernels walk, one level per launch, numbered breadth first (top levels first: the LDS
//     staging takes the first nodes);
//   - the surrounding-RI grid (counts, scan, fill).
// An update from device-resident records (rt_dev_scene_inw_update_device) also gets its
// hot, cold and sphere records and its decisions here (k_inw_prepare) and the time-bin trees: K more
// runs of the same SAH levels and collapse over k_bin_boxes' boxes, laid out by k_bin_place.
// The same SAH levels and collapse build the IOW-03 culling BVH of a scene update
// (iow_cull_build_device) over boxes made from the hot records (k_iow_boxes).
// An IOW-03 update from device-resident records (rt_dev_scene_iow03_update_device) makes
// those hot records, the cold records and the RI priors here too (k_iow_prepare, k_iow_mode,
// k_iow_priors around a radix sort of the RI keys).
// The host path (rtamd::inw_wide_build: a full-sweep SAH) stays for fresh scenes; binned with 32
// bins its SAH cost over the C3 leaf boxes is within 0.3% of the sweep's (16.80 against 16.75).
// Every structure is a culling or bookkeeping structure: the walks' results do not depend on
// its shape, so frames are bit-identical to those of the host-built scene.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>

#include "rt_host.hpp"
#include "rt_kernels.hpp"

namespace rtk {
namespace {

constexpr int kB = 256;
constexpr int kBins = 32;
constexpr int kLevelBatch = 8;   // levels launched between two reads of the pending-task count
constexpr int kSahFirst = 20;    // the binary SAH levels launched before the first read (C3's tree: ~20)
constexpr int kMaxLevels = 256;  // binary SAH levels launched at most; a deeper tree (a chain-like scene,
                                 // where a split peels one object off per level) returns
                                 // hipErrorNotSupported and the caller builds on the host (rt_capi.hip)

// orderable bits of a float (a < b <=> ford(a) < ford(b)) for atomic min / max
__device__ __forceinline__ uint32_t ford(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fdeo(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__device__ __forceinline__ uint32_t parent_of(const float4 *nodes, uint32_t i) { return (uint32_t)nodes[2 * i + 1].w; }
__device__ __forceinline__ bool lbvh_leaf(const float4 *nodes, uint32_t i) { return !(nodes[2 * i + 1].z > 0.1f); }

// per LBVH node: leaf -> its object's leaf box, culling box (inflated as rtamd::inw_wide_build),
// centroid, leaf node; the largest |coordinate| of the culling boxes (wbound, as uint bits)
__global__ __launch_bounds__(kB) void k_leaves(const float4 *nodes, uint32_t nn, uint32_t n, float4 *leafbox,
                                               float *box, float *cen, uint32_t *leafnode, uint32_t *ids,
                                               uint32_t *meta) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= nn) return;  // no cross-lane work in this kernel
    const float4 n0 = nodes[2 * i], n1 = nodes[2 * i + 1];
    if (n1.z > 0.1f) return;
    const uint32_t g = (uint32_t)(-n1.z);
    if (g >= n) return;  // (the device LBVH never does this)
    leafnode[g] = i;
    ids[g] = g;
    leafbox[2 * g] = n0;
    leafbox[2 * g + 1] = n1;
    const float b[6] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y};
    float big = 0.0f;
    for (int k = 0; k < 6; k++) big = fmaxf(big, fabsf(b[k]));
    float wb = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float e = (b[3 + k] - b[k]) * 1e-3f + 1e-3f + big * 1e-5f;
        const float lo = b[k] - e, hi = b[3 + k] + e;
        box[6 * g + k] = lo;
        box[6 * g + 3 + k] = hi;
        cen[3 * g + k] = 0.5f * (lo + hi);
        wb = fmaxf(wb, fmaxf(fabsf(lo), fabsf(hi)));
    }
    atomicMax(meta + 3, __float_as_uint(wb));  // non-negative: uint order = value order
}

// depth-first ranks (01_BVH...glsl:456-460: invert = 0 pops the right child, at the even index,
// first; invert = 1 the left one): the leaves of every earlier-visited sibling on the path
__global__ __launch_bounds__(kB) void k_ranks(const float4 *nodes, uint32_t n, const uint32_t *leafnode,
                                              const uint32_t *lcnt, uint32_t *rank) {
    const uint32_t g = blockIdx.x * kB + threadIdx.x;
    if (g >= n) return;  // no cross-lane work in this kernel
    uint32_t i = leafnode[g], r0 = 0, r1 = 0;
    while (i != 0u) {
        const uint32_t sib = (i & 1u) ? i + 1u : i - 1u;
        const uint32_t c = lbvh_leaf(nodes, sib) ? 1u : lcnt[sib];
        if (i & 1u) r0 += c;  // a left child comes after its right sibling when invert = 0
        else r1 += c;         // a right child after its left sibling when invert = 1
        i = parent_of(nodes, i);
    }
    rank[g] = r0;
    rank[n + g] = r1;
}

// the reference walk's stack high-water mark: popping node X leaves s(X) entries, s(root) = 0,
// a first-visited child has its parent's s + 1, the other one its parent's s; pushing X's children
// makes s(X) + 2 (both child orders; at least 1, the root push)
__global__ __launch_bounds__(kB) void k_high(const float4 *nodes, uint32_t nn, uint32_t *meta) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= nn) return;  // no cross-lane work in this kernel
    if (lbvh_leaf(nodes, i)) {
        if (i == 0u) atomicMax(meta + 2, 1u);
        return;
    }
    uint32_t s0 = 0, s1 = 0, j = i;
    while (j != 0u) {
        if (j & 1u) s1++;  // invert = 1 visits the left (odd) child first
        else s0++;         // invert = 0 the right (even) one
        j = parent_of(nodes, j);
    }
    atomicMax(meta + 2, (s0 > s1 ? s0 : s1) + 2u);
}

__device__ __forceinline__ float box_area(float x0, float y0, float z0, float x1, float y1, float z1) {
    const float dx = fmaxf(x1 - x0, 0.0f), dy = fmaxf(y1 - y0, 0.0f), dz = fmaxf(z1 - z0, 0.0f);
    return dx * dy + dy * dz + dz * dx;
}
__device__ __forceinline__ int bin_of(float c, float cmn, float scale) {
    return min(kBins - 1, max(0, (int)((c - cmn) * scale)));
}

// One level of the binned SAH build.  Task = (node, lo, hi, cb) over ids[lo, hi), hi - lo >= 2: the
// node takes the split of least SAH cost over 3 x (kBins - 1) bin boundaries (ties to the lower
// (axis, boundary); a range whose centroids share one bin on every axis splits in the middle),
// stably partitions its ids from ids_in into ids_out (the levels ping-pong between the two
// arrays: every range of a level is written by its parent's task) and makes its children.
// Numbering without counters: a range of m objects has 2m - 1 nodes, so a node's descendants own
// the 2m - 2 ids from cb: its children are the pair cb, cb + 1 (the layout the collapse reads),
// the left child's descendants follow from cb + 2, the right child's after those.  A child of one
// object is written as a leaf (first child = -object, as the LBVH layout) by the lane that places
// the object; the others are appended to the next level's tasks.  Ranges of more than kWaveMax
// objects take a block, the others one wave (no barriers; the top levels hold the few big
// ranges, the deep levels thousands of small ones).  Both paths pick the same split from the same
// bins (costs are min / max folds and exact counts); a block bins an evenly spaced sample of a
// range of more than kSahSample objects.
constexpr uint32_t kWaveMax = 256;
constexpr int kU = 8;  // loads in flight per lane in the block path's loops
constexpr uint32_t kSahSample = 2048;  // objects binned per range (evenly spaced) above this
struct SahBins {
    uint32_t cnt[3][kBins];
    uint32_t bb[3][kBins][6];  // orderable bits: lo min, hi max
};
__device__ __forceinline__ void bins_clear(SahBins &sb, uint32_t t, uint32_t nt) {
    for (uint32_t k = t; k < 3u * kBins; k += nt) {
        sb.cnt[k / kBins][k % kBins] = 0u;
        for (int j = 0; j < 6; j++) sb.bb[k / kBins][k % kBins][j] = j < 3 ? 0xffffffffu : 0u;
    }
}
__device__ __forceinline__ void bins_add(SahBins &sb, const float *bx, const float *c, const float *cmn,
                                         const float *scale, const bool *ax_ok) {
    for (int a = 0; a < 3; a++) {
        if (!ax_ok[a]) continue;
        const int b = bin_of(c[a], cmn[a], scale[a]);
        atomicAdd(&sb.cnt[a][b], 1u);
        for (int k = 0; k < 3; k++) {
            atomicMin(&sb.bb[a][b][k], ford(bx[k]));
            atomicMax(&sb.bb[a][b][3 + k], ford(bx[3 + k]));
        }
    }
}
__device__ __forceinline__ void load_item(const float *box, const float *cen, uint32_t g, float *bx, float *c) {
    for (int k = 0; k < 6; k++) bx[k] = box[6 * g + k];
    for (int k = 0; k < 3; k++) c[k] = cen[3 * g + k];
}
__device__ __forceinline__ void write_leaf(float *bin, uint32_t node, const float *box, uint32_t g) {
    float *o = bin + (size_t)node * 8;
    for (int k = 0; k < 6; k++) o[k] = box[6 * g + k];
    o[6] = -(float)g;
    o[7] = 0.0f;
}
// the object placed at position `dst` of a task split at nl: a child of one object is a leaf
__device__ __forceinline__ void place(uint32_t g, uint32_t dst, const uint4 tk, uint32_t nl, uint32_t *ids_out,
                                      float *bin, const float *box) {
    ids_out[dst] = g;
    const uint32_t lo = tk.y, hi = tk.z;
    if (nl == 1u && dst == lo) write_leaf(bin, tk.w, box, g);
    if (hi - lo - nl == 1u && dst == lo + nl) write_leaf(bin, tk.w + 1u, box, g);
}
// the task's node record and its internal children's tasks (one lane)
__device__ __forceinline__ void sah_emit(const uint4 tk, uint32_t nl, const float *nbox, float *bin, uint4 *tout,
                                         uint32_t *cnt_out) {
    const uint32_t node = tk.x, lo = tk.y, hi = tk.z, cb = tk.w, nr = hi - lo - nl;
    float *o = bin + (size_t)node * 8;
    for (int k = 0; k < 6; k++) o[k] = nbox[k];
    o[6] = (float)cb;
    o[7] = 0.0f;
    const uint32_t k = (nl > 1u ? 1u : 0u) + (nr > 1u ? 1u : 0u);
    if (!k) return;
    uint32_t slot = atomicAdd(cnt_out, k);
    if (nl > 1u) tout[slot++] = make_uint4(cb, lo, lo + nl, cb + 2u);
    if (nr > 1u) tout[slot] = make_uint4(cb + 1u, lo + nl, hi, cb + 2u + 2u * (nl - 1u));
}
__device__ __forceinline__ void bounds_init(float *v) {
    for (int k = 0; k < 3; k++) { v[k] = v[6 + k] = __builtin_huge_valf(); v[3 + k] = v[9 + k] = -__builtin_huge_valf(); }
}
__device__ __forceinline__ void bounds_add(float *v, const float *bx, const float *c) {
    for (int k = 0; k < 3; k++) {
        v[k] = fminf(v[k], bx[k]);
        v[3 + k] = fmaxf(v[3 + k], bx[3 + k]);
        v[6 + k] = fminf(v[6 + k], c[k]);
        v[9 + k] = fmaxf(v[9 + k], c[k]);
    }
}
__device__ __forceinline__ void bounds_wave(float *v) {  // butterfly: every lane holds the result
    for (int k = 0; k < 12; k++) {
        const bool mx = (k % 6) >= 3;
        for (int off = 32; off >= 1; off >>= 1) {
            const float w = __shfl_xor(v[k], off, 64);
            v[k] = mx ? fmaxf(v[k], w) : fminf(v[k], w);
        }
    }
}
__device__ __forceinline__ void bin_frame(const float *v, float *cmn, float *scale, bool *ax_ok) {
    for (int a = 0; a < 3; a++) {
        cmn[a] = v[6 + a];
        const float ext = v[9 + a] - cmn[a];
        ax_ok[a] = ext > 0.0f;
        scale[a] = ax_ok[a] ? (float)kBins / ext : 0.0f;
    }
}
// least-cost boundary over the bins, one wave: lane k < 31 evaluates boundary k of each axis from
// prefix / suffix folds over lanes 0..31 (empty bins fold as the identity); returns (axis *
// (kBins - 1) + boundary, or -1) and the left count in nl
__device__ __forceinline__ int sah_pick(const SahBins &sb, const bool *ax_ok, uint32_t lane, uint32_t m, uint32_t &nl) {
    float bc = __builtin_huge_valf();
    int bi = 0x7fffffff;
    uint32_t pcnt[3] = {0u, 0u, 0u};
    const uint32_t l = lane & 31u;
    for (int a = 0; a < 3; a++) {
        if (!ax_ok[a]) continue;  // uniform
        uint32_t c = sb.cnt[a][l];
        float b[6];
        for (int j = 0; j < 6; j++)
            b[j] = c ? fdeo(sb.bb[a][l][j]) : (j < 3 ? __builtin_huge_valf() : -__builtin_huge_valf());
        uint32_t pc = c, sc = c;
        float p[6], q[6];
        for (int j = 0; j < 6; j++) p[j] = q[j] = b[j];
        for (uint32_t off = 1; off < 32u; off <<= 1) {
            const uint32_t up = __shfl_up(pc, off, 32), dn = __shfl_down(sc, off, 32);
            float pu[6], qd[6];
            for (int j = 0; j < 6; j++) { pu[j] = __shfl_up(p[j], off, 32); qd[j] = __shfl_down(q[j], off, 32); }
            if (l >= off) {
                pc += up;
                for (int j = 0; j < 3; j++) { p[j] = fminf(p[j], pu[j]); p[3 + j] = fmaxf(p[3 + j], pu[3 + j]); }
            }
            if (l + off < 32u) {
                sc += dn;
                for (int j = 0; j < 3; j++) { q[j] = fminf(q[j], qd[j]); q[3 + j] = fmaxf(q[3 + j], qd[3 + j]); }
            }
        }
        // boundary l: left = bins 0..l (prefix at l), right = bins l+1.. (suffix at l+1)
        const uint32_t nr = __shfl_down(sc, 1, 32);
        float r[6];
        for (int j = 0; j < 6; j++) r[j] = __shfl_down(q[j], 1, 32);
        pcnt[a] = pc;
        if (l < (uint32_t)(kBins - 1) && pc && nr) {
            const float cost = box_area(p[0], p[1], p[2], p[3], p[4], p[5]) * (float)pc +
                               box_area(r[0], r[1], r[2], r[3], r[4], r[5]) * (float)nr;
            if (cost < bc) { bc = cost; bi = a * (kBins - 1) + (int)l; }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {  // least (cost, index)
        const float c2 = __shfl_xor(bc, off, 64);
        const int i2 = __shfl_xor(bi, off, 64);
        if (c2 < bc || (c2 == bc && i2 < bi)) { bc = c2; bi = i2; }
    }
    if (!(bc < __builtin_huge_valf())) { nl = m / 2u; return -1; }
    const int a = bi / (kBins - 1), k = bi % (kBins - 1);
    nl = __shfl(a == 0 ? pcnt[0] : a == 1 ? pcnt[1] : pcnt[2], k, 64);
    return bi;
}
__device__ __forceinline__ bool goes_left(int best, float c, uint32_t pos, uint32_t nl, float cmn, float scale, int k) {
    return best >= 0 ? bin_of(c, cmn, scale) <= k : pos < nl;
}

__global__ __launch_bounds__(kB) void k_sah_level(const uint4 *tin, const uint32_t *cnt_in, uint4 *tout,
                                                  uint32_t *cnt_out, const uint32_t *ids_in, uint32_t *ids_out,
                                                  const float *box, const float *cen, float *bin) {
    __shared__ float s_red[12][kB / 64];
    __shared__ SahBins s_bins;
    __shared__ SahBins s_wbins[kB / 64];
    __shared__ uint32_t s_wl[kB / 64];
    __shared__ float s_box[12];
    __shared__ int s_split[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t ntask = *cnt_in;
    // big ranges: a block each
    for (uint32_t t = blockIdx.x; t < ntask; t += gridDim.x) {  // uniform per block
        const uint4 tk = tin[t];
        const uint32_t lo = tk.y, hi = tk.z, m = hi - lo;
        if (m <= kWaveMax) continue;
        float v[12];
        bounds_init(v);
        for (uint32_t base = lo + tid; base < hi; base += kB * kU) {
            uint32_t g[kU];
            for (int u = 0; u < kU; u++) g[u] = base + u * kB < hi ? ids_in[base + u * kB] : 0xffffffffu;
            for (int u = 0; u < kU; u++)
                if (g[u] != 0xffffffffu) {
                    float bx[6], c[3];
                    load_item(box, cen, g[u], bx, c);
                    bounds_add(v, bx, c);
                }
        }
        bounds_wave(v);
        if (lane < 12u) {
            float x = v[0];
            for (int k = 1; k < 12; k++) x = lane == (uint32_t)k ? v[k] : x;
            s_red[lane][wv] = x;
        }
        bins_clear(s_bins, tid, kB);
        __syncthreads();
        if (tid < 12u) {
            const bool mx = (tid % 6u) >= 3u;
            float r = s_red[tid][0];
            for (uint32_t w = 1; w < kB / 64; w++) r = mx ? fmaxf(r, s_red[tid][w]) : fminf(r, s_red[tid][w]);
            s_box[tid] = r;
        }
        __syncthreads();
        float cmn[3], scale[3];
        bool ax_ok[3];
        bin_frame(s_box, cmn, scale, ax_ok);
        // bins: each thread takes a contiguous run of the range (neighbouring ids are often
        // neighbouring objects, which share bins: spread them over the wave's lanes).  A range of
        // more than kSahSample objects bins kSahSample of them, evenly spaced: the split is chosen
        // from the sample, the partition below counts the true sides (the top levels' LDS atomics
        // otherwise serialise one block on 21 atomics per object)
        {
            const bool smp = m > kSahSample;
            const uint32_t ms = smp ? kSahSample : m;
            const uint32_t per = (ms + kB - 1) / kB, k0 = tid * per, k1 = min(ms, k0 + per);
            for (uint32_t base = k0; base < k1; base += kU) {
                uint32_t g[kU];
                for (int u = 0; u < kU; u++) {
                    const uint32_t k = base + u;
                    const uint32_t q = smp ? lo + (uint32_t)(((uint64_t)k * m) / kSahSample) : lo + k;
                    g[u] = k < k1 ? ids_in[q] : 0xffffffffu;
                }
                for (int u = 0; u < kU; u++)
                    if (g[u] != 0xffffffffu) {
                        float bx[6], c[3];
                        load_item(box, cen, g[u], bx, c);
                        bins_add(s_bins, bx, c, cmn, scale, ax_ok);
                    }
            }
        }
        __syncthreads();
        if (wv == 0) {
            uint32_t nl = 0;
            const int best = sah_pick(s_bins, ax_ok, lane, m, nl);
            if (lane == 0) { s_split[0] = best; s_split[1] = (int)nl; }
        }
        __syncthreads();
        const int best = s_split[0];
        const uint32_t nl_pick = (uint32_t)s_split[1];  // the sample's left count when sampled
        // stable partition by side: a wave per quarter of the range (64-aligned), a count pass,
        // then each wave places its quarter from the counts of the quarters before it
        const int a = best >= 0 ? best / (kBins - 1) : 0, k = best >= 0 ? best % (kBins - 1) : 0;
        const uint32_t seg = ((m + 4u * 64u - 1u) / (4u * 64u)) * 64u;
        const uint32_t s0 = min(hi, lo + wv * seg), s1 = min(hi, s0 + seg);
        const uint64_t lt = lane ? (~0ull >> (64u - lane)) : 0ull;
        uint32_t nleft = 0;
        for (uint32_t base = s0; base < s1; base += 64u * kU) {
            float c[kU];
            for (int u = 0; u < kU; u++) {
                const uint32_t q = base + 64u * u + lane;
                c[u] = q < s1 && best >= 0 ? cen[3 * ids_in[q] + a] : 0.0f;
            }
            for (int u = 0; u < kU; u++) {
                const uint32_t q = base + 64u * u + lane;
                nleft += (uint32_t)__popcll(__ballot(q < s1 && goes_left(best, c[u], q - lo, nl_pick, cmn[a], scale[a], k)));
            }
        }
        if (lane == 0) s_wl[wv] = nleft;
        __syncthreads();
        uint32_t left = 0, nl = 0;  // nl: the true left count
        for (uint32_t w = 0; w < kB / 64; w++) {
            if (w < wv) left += s_wl[w];
            nl += s_wl[w];
        }
        uint32_t right = (s0 - lo) - left;
        for (uint32_t base = s0; base < s1; base += 64u * kU) {
            uint32_t g[kU];
            float c[kU];
            for (int u = 0; u < kU; u++) {
                const uint32_t q = base + 64u * u + lane;
                g[u] = q < s1 ? ids_in[q] : 0u;
                c[u] = q < s1 && best >= 0 ? cen[3 * g[u] + a] : 0.0f;
            }
            for (int u = 0; u < kU; u++) {
                const uint32_t q = base + 64u * u + lane;
                const bool has = q < s1, isl = has && goes_left(best, c[u], q - lo, nl, cmn[a], scale[a], k);
                const uint64_t ml = __ballot(isl), mh = __ballot(has);
                const uint32_t bl = (uint32_t)__popcll(ml & lt), bh = (uint32_t)__popcll(mh & lt);
                if (has) place(g[u], isl ? lo + left + bl : lo + nl + right + (bh - bl), tk, nl, ids_out, bin, box);
                left += (uint32_t)__popcll(ml);
                right += (uint32_t)(__popcll(mh) - __popcll(ml));
            }
        }
        if (tid == 0) sah_emit(tk, nl, s_box, bin, tout, cnt_out);
        __syncthreads();  // s_wl, s_box and s_split are the next task's
    }
    // small ranges: a wave each
    SahBins &wb = s_wbins[wv];
    const uint32_t nw = gridDim.x * (kB / 64);
    for (uint32_t t = blockIdx.x * (kB / 64) + wv; t < ntask; t += nw) {  // uniform per wave
        const uint4 tk = tin[t];
        const uint32_t lo = tk.y, hi = tk.z, m = hi - lo;
        if (m > kWaveMax) continue;
        uint32_t g[kWaveMax / 64];
        for (uint32_t j = 0; j < kWaveMax / 64; j++) {
            const uint32_t q = lo + lane + 64u * j;
            g[j] = q < hi ? ids_in[q] : 0u;
        }
        float v[12];
        bounds_init(v);
        for (uint32_t j = 0; j < kWaveMax / 64; j++)
            if (lo + lane + 64u * j < hi) {
                float bx[6], c[3];
                load_item(box, cen, g[j], bx, c);
                bounds_add(v, bx, c);
            }
        bounds_wave(v);
        float cmn[3], scale[3];
        bool ax_ok[3];
        bin_frame(v, cmn, scale, ax_ok);
        bins_clear(wb, lane, 64u);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t j = 0; j < kWaveMax / 64; j++)
            if (lo + lane + 64u * j < hi) {
                float bx[6], c[3];
                load_item(box, cen, g[j], bx, c);
                bins_add(wb, bx, c, cmn, scale, ax_ok);
            }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t nl = 0;
        const int best = sah_pick(wb, ax_ok, lane, m, nl);
        const int a = best >= 0 ? best / (kBins - 1) : 0, k = best >= 0 ? best % (kBins - 1) : 0;
        uint32_t left = 0, right = 0;
        const uint64_t lt = lane ? (~0ull >> (64u - lane)) : 0ull;
        for (uint32_t j = 0; j < kWaveMax / 64 && lo + 64u * j < hi; j++) {  // uniform
            const uint32_t q = lo + lane + 64u * j;
            const bool has = q < hi;
            const bool isl = has && goes_left(best, best >= 0 ? cen[3 * g[j] + a] : 0.0f, q - lo, nl, cmn[a], scale[a], k);
            const uint64_t ml = __ballot(isl), mh = __ballot(has);
            const uint32_t bl = (uint32_t)__popcll(ml & lt), bh = (uint32_t)__popcll(mh & lt);
            if (has) place(g[j], isl ? lo + left + bl : lo + nl + right + (bh - bl), tk, nl, ids_out, bin, box);
            left += (uint32_t)__popcll(ml);
            right += (uint32_t)(__popcll(mh) - __popcll(ml));
        }
        if (lane == 0) {
            float nb[6];
            for (int j = 0; j < 6; j++) nb[j] = v[j];
            sah_emit(tk, nl, nb, bin, tout, cnt_out);
        }
        // the bins are reused by the wave's next task: its reads above are done (wave in order)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// One level of the 4-wide collapse (rtamd::bvh4_collapse): a wide node gathers its binary node's
// children and opens the largest-area internal one until it holds four; internal children become
// the next level's wide nodes.  Wide node = 10 float4: lx ly lz hx hy hz (SoA over the 4
// children), lx ly lz again, the links (int bits: wide index + 1, or -object; an empty slot is a
// box at 1e30 with link 1e9, culled by every ray).  Numbering breadth first without a node
// counter: level wl + 1's wide nodes follow all earlier levels' (the prefix of the level counts),
// in the order of their task slots; a wave takes its slots with one atomic.  meta[1] sums the
// wide nodes (the root counted by the caller).  NF4 = float4 per wide node: 10 is the INW node above,
// 8 the IOW-03 node (the six planes, the links, one unused float4; rtamd::iow_cull_build).
__device__ __forceinline__ float bin_area(const float *bin, int i) {
    const float *b = bin + (size_t)i * 8;
    const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    return dx * dy + dy * dz + dz * dx;
}
template <int NF4>
__global__ __launch_bounds__(kB) void k_collapse_level(const uint2 *tin, uint32_t *wlvl_cnt, int wl, uint2 *tout,
                                                       const float *bin, float4 *wnodes, uint32_t *meta) {
    const uint32_t t = blockIdx.x * kB + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t ntask = wlvl_cnt[wl];
    if (blockIdx.x * kB + (threadIdx.x & ~63u) >= ntask) return;  // whole waves only (the scan below)
    // wide nodes before level wl + 1: the level counts 0..wl
    uint32_t before = 0;
    for (int i = (int)lane; i <= wl; i += 64) before += wlvl_cnt[i];
    for (int off = 32; off >= 1; off >>= 1) before += (uint32_t)__shfl_xor((int)before, off, 64);
    const bool act = t < ntask;
    auto is_leaf = [&](int i) { return !(bin[(size_t)i * 8 + 6] > 0.1f); };
    auto first = [&](int i) { return (int)bin[(size_t)i * 8 + 6]; };
    int ch[4] = {-1, -1, -1, -1};
    int nch = 0;
    uint2 tk = make_uint2(0u, 0u);
    if (act) {
        tk = tin[t];
        ch[0] = first((int)tk.x);
        ch[1] = ch[0] + 1;
        nch = 2;
        while (nch < 4) {
            int pick = -1;
            for (int k = 0; k < nch; k++)
                if (!is_leaf(ch[k]) && (pick < 0 || bin_area(bin, ch[k]) > bin_area(bin, ch[pick]))) pick = k;
            if (pick < 0) break;
            const int b = ch[pick];
            for (int k = pick; k < nch - 1; k++) ch[k] = ch[k + 1];
            ch[nch - 1] = first(b);
            ch[nch] = first(b) + 1;
            nch++;
        }
    }
    bool internal[4];
    uint32_t nk = 0;
    for (int k = 0; k < 4; k++) {
        internal[k] = k < nch && !is_leaf(ch[k]);
        nk += internal[k] ? 1u : 0u;
    }
    uint32_t incl = nk;  // inclusive scan of the wave's internal-child counts
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    uint32_t base = 0;
    if (lane == 63u && total) {
        base = atomicAdd(wlvl_cnt + wl + 1, total);
        atomicAdd(meta + 1, total);
    }
    base = __shfl(base, 63, 64);
    if (!act) return;
    uint32_t slot = base + incl - nk;
    float pl[6][4];
    int lk[4];
    for (int k = 0; k < 4; k++) {
        if (k >= nch) {
            for (int a = 0; a < 6; a++) pl[a][k] = 1e30f;
            lk[k] = 1000000000;
            continue;
        }
        const float *bb = bin + (size_t)ch[k] * 8;
        for (int a = 0; a < 6; a++) pl[a][k] = bb[a];
        if (!internal[k]) lk[k] = (int)bb[6];
        else {
            const uint32_t w = before + slot;
            tout[slot++] = make_uint2((uint32_t)ch[k], w);
            lk[k] = (int)w + 1;
        }
    }
    float4 *o = wnodes + (size_t)tk.y * NF4;
    for (int a = 0; a < 6; a++) o[a] = make_float4(pl[a][0], pl[a][1], pl[a][2], pl[a][3]);
    const float4 links = make_float4(__int_as_float(lk[0]), __int_as_float(lk[1]), __int_as_float(lk[2]), __int_as_float(lk[3]));
    if constexpr (NF4 == 10) {
        for (int a = 0; a < 3; a++) o[6 + a] = o[a];
        o[9] = links;
    } else {
        static_assert(NF4 == 8, "the INW (10) or the IOW-03 (8) wide node");
        o[6] = links;
        o[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// IOW-03: every object's culling box from its hot record (pos3 type M9 scale3 ...), by the statements
// of rtamd::iow_cull_build in their order (|M^T| times the local half extents, inflated; plain IEEE
// operations under -ffp-contract=off, so the boxes equal the host's bit for bit): obox as the kernels
// read it, and the SAH build's box / cen / ids.  meta[0] is set when some box value is not finite.
__global__ __launch_bounds__(kB) void k_iow_boxes(const float *hot, uint32_t n, float4 *obox, float *box, float *cen,
                                                  uint32_t *ids, uint32_t *meta) {
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    if (j >= n) return;  // no cross-lane work in this kernel
    const float *r = hot + (size_t)j * kIowHot;
    const bool ell = (int)r[3] == RT_IOW_ELLIPSOID;
    float h[3];
    for (int k = 0; k < 3; k++) h[k] = fabsf(r[13 + k]) * (ell ? 1.0f : 0.5f);
    const float big = fmaxf(fabsf(r[0]), fmaxf(fabsf(r[1]), fabsf(r[2])));
    float b[6];
    bool fin = true;
    for (int k = 0; k < 3; k++) {
        const float *col = r + 4 + 3 * k;  // column k of M
        float e = fabsf(col[0]) * h[0] + fabsf(col[1]) * h[1] + fabsf(col[2]) * h[2];
        e = e * 1.001f + 1e-3f + big * 1e-5f;
        b[k] = r[k] - e;
        b[3 + k] = r[k] + e;
        fin = fin && isfinite(b[k]) && isfinite(b[3 + k]);
    }
    obox[j] = make_float4(b[0], b[1], b[2], b[3]);
    reinterpret_cast<float2 *>(obox + n)[j] = make_float2(b[4], b[5]);
    for (int k = 0; k < 3; k++) {
        box[6 * j + k] = b[k];
        box[6 * j + 3 + k] = b[3 + k];
        cen[3 * j + k] = 0.5f * (b[k] + b[3 + k]);
    }
    ids[j] = j;
    if (!fin) atomicOr(meta, 1u);
}

// ---- IOW-03 update from device-resident records (rt_dev_scene_iow03_update_device)
// The hot and cold records of every object by the statements of iow_records (rt_scene_build.hip): plain
// copies, the three 1 / scale as the correctly rounded divide, the identity flag from the rotation's
// bit patterns (glm::mat3(1): a -0.0 off the diagonal is not the identity), pad floats zero -- so the
// bytes equal the host's.  keys: the orderable bits of the RI (record float 20) for the priors' sort.
// One lane per object, no LDS; VEC: rec is 16-byte aligned (a record is 96 bytes: six float4 loads).
template <bool VEC>
__global__ __launch_bounds__(kB) void k_iow_prepare(const float *types, const float *rec, uint32_t n, float4 *hot,
                                                    float4 *cold, uint32_t *keys) {
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    if (j >= n) return;  // no cross-lane work in this kernel
    float r[24];
    if constexpr (VEC) {
        const float4 *src = reinterpret_cast<const float4 *>(rec) + (size_t)j * 6;
        for (int k = 0; k < 6; k++) {
            const float4 v = src[k];
            r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w;
        }
    } else {
        const float *src = rec + (size_t)j * 24;
        for (int k = 0; k < 24; k++) r[k] = src[k];
    }
    bool ident = true;
    for (int k = 0; k < 9; k++) ident = ident && __float_as_uint(r[3 + k]) == ((k % 4) == 0 ? 0x3f800000u : 0u);
    float4 *h = hot + (size_t)j * (kIowHot / 4);
    h[0] = make_float4(r[0], r[1], r[2], types[j]);
    h[1] = make_float4(r[3], r[4], r[5], r[6]);
    h[2] = make_float4(r[7], r[8], r[9], r[10]);
    h[3] = make_float4(r[11], r[12], r[13], r[14]);
    h[4] = make_float4(1.0f / r[12], 1.0f / r[13], 1.0f / r[14], ident ? 1.0f : 0.0f);
    float4 *c = cold + (size_t)j * (kIowCold / 4);
    c[0] = make_float4(r[15], r[16], r[17], r[18]);
    c[1] = make_float4(r[19], r[20], r[21], r[22]);
    keys[j] = ford(r[20]);
}

// The RI priors (iow_priors, rt_scene_build.hip) from the sorted keys.  Runs are compared by == as the
// host compares them, so -0.0 joins +0.0's run (their keys are neighbours); the distinct values are bit
// patterns, i.e. distinct keys.  NaNs order by their bits here: outside the priors' contract (the host's
// std::sort has none for them), but every search below ends and stays inside [0, n).
constexpr uint32_t kKeyZero = 0x80000000u, kKeyNegZero = 0x7fffffffu, kKeyOne = 0xbf800000u;  // ford(0.0f), (-0.0f), (1.0f)
__device__ __forceinline__ uint32_t ri_class(uint32_t key) { return key == kKeyNegZero ? kKeyZero : key; }
// the first index in (lo, n) whose key (CLS: whose == class) is above keys[lo]'s, or n
template <bool CLS>
__device__ __forceinline__ uint32_t run_end(const uint32_t *keys, uint32_t n, uint32_t lo) {
    const uint32_t k0 = CLS ? ri_class(keys[lo]) : keys[lo];
    uint32_t a = lo + 1u, b = n;  // keys[lo .. a) are not above k0, keys[b .. n) are
    while (a < b) {
        const uint32_t m = a + (b - a) / 2u;
        const uint32_t km = CLS ? ri_class(keys[m]) : keys[m];
        if (km > k0) b = m;
        else a = m + 1u;
    }
    return a;
}
// The mode: every lane at the head of a run finds the run's end by bisection; (length, ~key of the head)
// orders as the host's scan picks (the longest run, the smallest value among equals); a wave folds its
// lanes, one atomic per wave.  best: zeroed by the launcher.
__global__ __launch_bounds__(kB) void k_iow_mode(const uint32_t *keys, uint32_t n, unsigned long long *best) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    unsigned long long v = 0ull;
    if (i < n && (i == 0u || ri_class(keys[i - 1u]) != ri_class(keys[i])))
        v = ((unsigned long long)(run_end<true>(keys, n, i) - i) << 32) | (unsigned long long)(~keys[i]);
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, off, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63u) == 0u && v) atomicMax(best, v);
}
// The ten result words {ri_prior, alt_vals[8], n_alt_vals as a float}: the mode decoded, and the ascending
// distinct bit patterns of {0.0f, 1.0f} and the RIs when there are at most 8 (else none, all zero): at
// most 9 bisections by one lane, the list kept in LDS (indexed at run time).
__global__ __launch_bounds__(64) void k_iow_priors(const uint32_t *keys, uint32_t n, const unsigned long long *best,
                                                   uint32_t *out) {
    __shared__ uint32_t s_v[8];
    if (threadIdx.x != 0u) return;
    uint32_t nd = 0u;
    bool over = false;
    for (uint32_t pos = 0u; pos < n; pos = run_end<false>(keys, n, pos)) {
        if (nd == 8u) { over = true; break; }
        s_v[nd++] = keys[pos];
    }
    for (int e = 0; e < 2 && !over; e++) {  // 0.0f and 1.0f join the list where they are not in it
        const uint32_t k = e ? kKeyOne : kKeyZero;
        uint32_t p = 0u;
        while (p < nd && s_v[p] < k) p++;
        if (p < nd && s_v[p] == k) continue;
        if (nd == 8u) { over = true; break; }
        for (uint32_t q = nd; q > p; q--) s_v[q] = s_v[q - 1u];
        s_v[p] = k;
        nd++;
    }
    if (over) nd = 0u;
    out[0] = __float_as_uint(fdeo(~(uint32_t)(*best & 0xffffffffull)));
    for (uint32_t v = 0u; v < 8u; v++) out[1u + v] = v < nd ? __float_as_uint(fdeo(s_v[v])) : 0u;
    out[9] = __float_as_uint((float)nd);
}

// ---- surrounding-RI grid (rtamd::ri_grid_build): bounds, per-cell counts, offsets, ids
__global__ __launch_bounds__(kB) void k_ri_bounds(const float4 *leafbox, uint32_t n, uint32_t *bnd) {
    const uint32_t g = blockIdx.x * kB + threadIdx.x;
    uint32_t v[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    if (g < n) {
        const float4 n0 = leafbox[2 * g], n1 = leafbox[2 * g + 1];
        v[0] = ford(n0.x); v[1] = ford(n0.y); v[2] = ford(n0.z);
        v[3] = ford(n0.w); v[4] = ford(n1.x); v[5] = ford(n1.y);
    }
    for (int off = 32; off >= 1; off >>= 1)  // a wave's bounds, then one atomic per wave and bound
        for (int a = 0; a < 6; a++) {
            const uint32_t w = (uint32_t)__shfl_xor((int)v[a], off, 64);
            v[a] = a < 3 ? min(v[a], w) : max(v[a], w);
        }
    if ((threadIdx.x & 63u) == 0u)
        for (int a = 0; a < 3; a++) {
            atomicMin(bnd + a, v[a]);
            atomicMax(bnd + 3 + a, v[3 + a]);
        }
}
struct RiDims { double lo[3], inv[3]; int dim[3]; };
__device__ __forceinline__ void ri_range(const RiDims &d, float lo_v, float hi_v, int a, int &c0, int &c1) {
    const double m = 1e-3 / d.inv[a];
    c0 = max(0, min(d.dim[a] - 1, (int)floor(((double)lo_v - m - d.lo[a]) * d.inv[a])));
    c1 = max(0, min(d.dim[a] - 1, (int)floor(((double)hi_v + m - d.lo[a]) * d.inv[a])));
}
// pass 0: counts (cnt[c + 1]; flag when a cell lists more than 64); pass 1: ids through fill[c]
__global__ __launch_bounds__(kB) void k_ri_cells(const float4 *leafbox, uint32_t n, RiDims d, int pass, uint32_t *cnt,
                                                 uint32_t *fill, uint32_t *ids, uint32_t *flag) {
    const uint32_t g = blockIdx.x * kB + threadIdx.x;
    if (g >= n) return;  // no cross-lane work in this kernel
    // pass 0 stops once a cell is known to list more than 64 objects (the grid is dropped then, as
    // the host build stops at the first such cell): the count does not grow to O(n x cells) atomics
    if (pass == 0 && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const float4 n0 = leafbox[2 * g], n1 = leafbox[2 * g + 1];
    const float lo[3] = {n0.x, n0.y, n0.z}, hi[3] = {n0.w, n1.x, n1.y};
    int r0[3], r1[3];
    for (int a = 0; a < 3; a++) ri_range(d, lo[a], hi[a], a, r0[a], r1[a]);
    for (int z = r0[2]; z <= r1[2]; z++) {
        if (pass == 0 && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        for (int y = r0[1]; y <= r1[1]; y++)
            for (int x = r0[0]; x <= r1[0]; x++) {
                const size_t c = ((size_t)z * (size_t)d.dim[1] + (size_t)y) * (size_t)d.dim[0] + (size_t)x;
                if (pass == 0) {
                    if (atomicAdd(cnt + c + 1, 1u) >= 64u) atomicOr(flag, 1u);
                } else {
                    ids[atomicAdd(fill + c, 1u)] = g;
                }
            }
    }
}

inline uint32_t nblk(size_t n) { return (uint32_t)((n + kB - 1) / kB); }

// ---- quantised wide nodes (InwScene::qnodes, DESIGN.md §5.2 "Quantised nodes")
// Per node and axis: origin o (a float at or below the lowest child plane minus the margin m) and
// scale s >= 1e-4 (o + 255 s at or above the highest plane plus m); a child's low plane becomes
// the byte q with o + q s <= lo - m, its high plane the byte with o + q s >= hi + m (real
// arithmetic, checked in double on the exact float values).  An empty slot (link 1e9) gets low
// bytes 255 and high bytes 0: an interval reversed by 255 s >= 0.0255, which no rounding of the
// walk's fma closes.  The walk computes t = fma(q, s / d, (o - ray origin) / d); DESIGN.md §2 bounds
// its error below m / |d| while every coordinate and ray origin lies within 1000 of the origin (the
// fused cull's condition, required for these nodes), so the decoded boxes stay conservative.
__device__ __forceinline__ float f32_next_up(float f) {  // finite f: the next float above
    if (f == 0.0f) return __uint_as_float(1u);
    const uint32_t u = __float_as_uint(f);
    return __uint_as_float(f > 0.0f ? u + 1u : u - 1u);
}
__device__ __forceinline__ float f32_next_down(float f) { return -f32_next_up(-f); }
__device__ __forceinline__ float f32_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = f32_next_down(f);
    return f;
}
__device__ __forceinline__ float f32_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = f32_next_up(f);
    return f;
}
__global__ __launch_bounds__(kB) void k_quantize_wnodes(const float4 *wn, uint32_t nw, float4 *qn, float margin) {
    const uint32_t w = blockIdx.x * kB + threadIdx.x;
    if (w >= nw) return;  // no cross-lane work in this kernel
    const float4 *nd = wn + (size_t)w * 10;
    const float4 pl4[6] = {nd[0], nd[1], nd[2], nd[3], nd[4], nd[5]};
    const float4 lk = nd[9];
    auto comp = [](const float4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; };
    bool empty[4];
    for (int k = 0; k < 4; k++) empty[k] = __float_as_int(comp(lk, k)) == 1000000000;
    const double m = (double)margin;
    float org[3], scl[3];
    uint32_t qlo[3] = {0u, 0u, 0u}, qhi[3] = {0u, 0u, 0u};
    for (int a = 0; a < 3; a++) {
        double nlo = 0.0, nhi = 0.0;
        bool any = false;
        for (int k = 0; k < 4; k++) {
            if (empty[k]) continue;
            const double lo = comp(pl4[a], k), hi = comp(pl4[3 + a], k);
            nlo = any ? fmin(nlo, lo) : lo;
            nhi = any ? fmax(nhi, hi) : hi;
            any = true;
        }
        const float o = f32_down(nlo - m);
        float s = f32_up(fmax(((nhi + m) - (double)o) / 255.0, 1e-4));
        while ((double)o + 255.0 * (double)s < nhi + m) s = f32_next_up(s);
        org[a] = o;
        scl[a] = s;
        for (int k = 0; k < 4; k++) {
            uint32_t ql = 255u, qh = 0u;
            if (!empty[k]) {
                const double lo = (double)comp(pl4[a], k) - m, hi = (double)comp(pl4[3 + a], k) + m;
                int q = (int)floor((lo - (double)o) / (double)s);
                q = q < 0 ? 0 : (q > 255 ? 255 : q);
                while (q > 0 && (double)o + (double)q * (double)s > lo) q--;
                int r = (int)ceil((hi - (double)o) / (double)s);
                r = r < 0 ? 0 : (r > 255 ? 255 : r);
                while (r < 255 && (double)o + (double)r * (double)s < hi) r++;
                ql = (uint32_t)q;
                qh = (uint32_t)r;
            }
            qlo[a] |= ql << (8 * k);
            qhi[a] |= qh << (8 * k);
        }
    }
    float4 *o4 = qn + (size_t)w * kQNodeF4;
    o4[0] = make_float4(org[0], org[1], org[2], scl[0]);
    o4[1] = make_float4(scl[1], scl[2], __uint_as_float(qlo[0]), __uint_as_float(qlo[1]));
    o4[2] = make_float4(__uint_as_float(qlo[2]), __uint_as_float(qhi[0]), __uint_as_float(qhi[1]), __uint_as_float(qhi[2]));
    o4[3] = lk;
}

}  // namespace

hipError_t inw_quantize_wnodes(const float4 *wnodes, uint32_t nw, float4 *qnodes, float margin, hipStream_t s) {
    if (!nw) return hipSuccess;
    if (!wnodes || !qnodes || !(margin > 0.0f)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_quantize_wnodes, dim3(nblk(nw)), dim3(kB), 0, s, wnodes, nw, qnodes, margin);
    return hipGetLastError();
}

// workspace carve-up (256-B aligned pieces)
struct BuildWs {
    float *box, *cen, *bin;
    uint32_t *leafnode, *ids, *ids2, *meta, *lvl_cnt, *wlvl_cnt;
    uint4 *task[2];
    uint2 *wtask[2];
    uint32_t *ri_bnd, *ri_flag;
};
static size_t carve(void *ws, uint32_t n, BuildWs *w) {
    const size_t nn = 2 * (size_t)n - 1;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = static_cast<char *>(ws) + off;
        off += (bytes + 255) & ~(size_t)255;
        return static_cast<void *>(p);
    };
    BuildWs t{};
    t.box = static_cast<float *>(take((size_t)n * 6 * 4));
    t.cen = static_cast<float *>(take((size_t)n * 3 * 4));
    t.bin = static_cast<float *>(take(nn * 8 * 4));
    t.leafnode = static_cast<uint32_t *>(take((size_t)n * 4));
    t.ids = static_cast<uint32_t *>(take((size_t)n * 4));
    t.ids2 = static_cast<uint32_t *>(take((size_t)n * 4));
    t.meta = static_cast<uint32_t *>(take(16 * 4));
    t.lvl_cnt = static_cast<uint32_t *>(take((kMaxLevels + 1) * 4));
    t.wlvl_cnt = static_cast<uint32_t *>(take((kMaxLevels + 1) * 4));
    t.task[0] = static_cast<uint4 *>(take((size_t)n * 16));
    t.task[1] = static_cast<uint4 *>(take((size_t)n * 16));
    t.wtask[0] = static_cast<uint2 *>(take((size_t)n * 8));
    t.wtask[1] = static_cast<uint2 *>(take((size_t)n * 8));
    t.ri_bnd = static_cast<uint32_t *>(take(8 * 4));
    t.ri_flag = static_cast<uint32_t *>(take(4));
    if (w) *w = t;
    return off;
}

size_t inw_build_workspace_bytes(uint32_t n) { return n ? carve(reinterpret_cast<void *>(256), n, nullptr) + 256 : 0; }

#define BUILD_HIP(expr)                                                                   \
    do {                                                                                  \
        const hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) return e_;                                                  \
    } while (0)

// The level loops both families share: the binary SAH tree over w.box / w.cen / w.ids (one k_sah_level
// launch per level) and its 4-wide collapse into wnodes (NF4 float4 per node, one k_collapse_level
// launch per level).  The pending-task counts are read back every few levels; the last read brings
// the counters (meta: [0] the caller's flag word, [1] wide nodes, [2], [3] the INW walk's high-water
// mark and wbound, [4..13] the ten words a caller placed there after build_begin: the IOW-03 priors)
// and w.ri_bnd along.  hipErrorNotSupported: deeper than lvl_cap.
constexpr int kMetaRead = 14;
struct BuildLevels {
    int depth;
    uint32_t meta[kMetaRead], bnd[6];
};
static int level_cap(int max_levels) { return max_levels > 0 && max_levels < kMaxLevels ? max_levels : kMaxLevels; }
static hipError_t build_begin(const BuildWs &w, hipStream_t s) {
    BUILD_HIP(hipMemsetAsync(w.meta, 0, 16 * 4, s));
    BUILD_HIP(hipMemsetAsync(w.lvl_cnt, 0, (kMaxLevels + 1) * 4, s));
    BUILD_HIP(hipMemsetAsync(w.wlvl_cnt, 0, (kMaxLevels + 1) * 4, s));
    return hipSuccess;
}
template <int NF4>
static hipError_t build_levels(const BuildWs &w, uint32_t n, float4 *wnodes, int lvl_cap, hipStream_t s, BuildLevels &out) {
    // binary SAH tree: root task (node 0, all objects, its descendants from node 1)
    const uint32_t one = 1u;
    const uint4 root = make_uint4(0u, 0u, n, 1u);
    BUILD_HIP(hipMemcpyAsync(w.task[0], &root, sizeof(root), hipMemcpyHostToDevice, s));
    BUILD_HIP(hipMemcpyAsync(w.lvl_cnt, &one, 4, hipMemcpyHostToDevice, s));
    int lvl = 0;
    for (int batch = kSahFirst;; batch = kLevelBatch) {
        for (int k = 0; k < batch && lvl < lvl_cap; k++, lvl++)
            hipLaunchKernelGGL(k_sah_level, dim3(1024), dim3(kB), 0, s, w.task[lvl & 1], w.lvl_cnt + lvl,
                               w.task[(lvl + 1) & 1], w.lvl_cnt + lvl + 1, (lvl & 1) ? w.ids2 : w.ids,
                               (lvl & 1) ? w.ids : w.ids2, w.box, w.cen, w.bin);
        BUILD_HIP(hipGetLastError());
        uint32_t pending = 0;
        BUILD_HIP(hipMemcpyAsync(&pending, w.lvl_cnt + lvl, 4, hipMemcpyDeviceToHost, s));
        BUILD_HIP(hipStreamSynchronize(s));
        if (pending == 0) break;
        if (lvl >= lvl_cap) return hipErrorNotSupported;  // deeper than the cap: the caller builds on the host
    }
    // 4-wide collapse; meta[1] = wide node counter (1: the root, from binary node 0)
    const uint2 wroot = make_uint2(0u, 0u);
    BUILD_HIP(hipMemcpyAsync(w.wtask[0], &wroot, sizeof(wroot), hipMemcpyHostToDevice, s));
    BUILD_HIP(hipMemcpyAsync(w.wlvl_cnt, &one, 4, hipMemcpyHostToDevice, s));
    BUILD_HIP(hipMemcpyAsync(w.meta + 1, &one, 4, hipMemcpyHostToDevice, s));
    int wl = 0;
    for (;;) {
        for (int k = 0; k < kLevelBatch && wl < lvl_cap; k++, wl++)
            hipLaunchKernelGGL(k_collapse_level<NF4>, dim3(nblk(n)), dim3(kB), 0, s, w.wtask[wl & 1], w.wlvl_cnt, wl,
                               w.wtask[(wl + 1) & 1], w.bin, wnodes, w.meta);
        BUILD_HIP(hipGetLastError());
        // this batch's level counts, the counters (meta) and the RI bounds in one read
        // (a level cap below the batch size launches fewer levels: the read starts at level 0 then)
        const int l0 = wl > kLevelBatch ? wl - kLevelBatch : 0, nl = wl - l0;
        uint32_t rb[kLevelBatch + 1 + kMetaRead + 6];
        BUILD_HIP(hipMemcpyAsync(rb, w.wlvl_cnt + l0, (size_t)(nl + 1) * 4, hipMemcpyDeviceToHost, s));
        BUILD_HIP(hipMemcpyAsync(rb + kLevelBatch + 1, w.meta, kMetaRead * 4, hipMemcpyDeviceToHost, s));
        BUILD_HIP(hipMemcpyAsync(rb + kLevelBatch + 1 + kMetaRead, w.ri_bnd, 6 * 4, hipMemcpyDeviceToHost, s));
        BUILD_HIP(hipStreamSynchronize(s));
        if (rb[nl] == 0) {
            int d = l0;
            while (d < wl && rb[d - l0] != 0) d++;
            out.depth = d;
            for (int k = 0; k < kMetaRead; k++) out.meta[k] = rb[kLevelBatch + 1 + k];
            for (int k = 0; k < 6; k++) out.bnd[k] = rb[kLevelBatch + 1 + kMetaRead + k];
            break;
        }
        if (wl >= lvl_cap) return hipErrorNotSupported;
    }
    return hipSuccess;
}

hipError_t inw_wide_build_device(const float4 *nodes, const uint32_t *lcnt, uint32_t n, void *ws, size_t ws_bytes,
                                 InwWideDev &out, hipStream_t s, int max_levels) {
    const int lvl_cap = level_cap(max_levels);
    if (n < 2 || !nodes || !lcnt || !ws || ws_bytes < inw_build_workspace_bytes(n) || !out.wnodes || !out.rank || !out.leafbox)
        return hipErrorInvalidValue;
    BuildWs w;
    carve(ws, n, &w);
    const uint32_t nn = 2 * n - 1;
    BUILD_HIP(build_begin(w, s));
    hipLaunchKernelGGL(k_leaves, dim3(nblk(nn)), dim3(kB), 0, s, nodes, nn, n, out.leafbox, w.box, w.cen, w.leafnode,
                       w.ids, w.meta);
    hipLaunchKernelGGL(k_ranks, dim3(nblk(n)), dim3(kB), 0, s, nodes, n, w.leafnode, lcnt, out.rank);
    hipLaunchKernelGGL(k_high, dim3(nblk(nn)), dim3(kB), 0, s, nodes, nn, w.meta);
    // the RI grid's bounds (the leaf boxes'), read back with the counts below
    const uint32_t binit[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    BUILD_HIP(hipMemcpyAsync(w.ri_bnd, binit, sizeof(binit), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ri_bounds, dim3(nblk(n)), dim3(kB), 0, s, out.leafbox, n, w.ri_bnd);
    BUILD_HIP(hipGetLastError());
    BuildLevels r;
    BUILD_HIP(build_levels<10>(w, n, out.wnodes, lvl_cap, s, r));
    out.depth = r.depth;
    out.n_wnodes = r.meta[1];
    out.dfs_high = r.meta[2] ? r.meta[2] : 1u;
    out.wbound = __builtin_bit_cast(float, r.meta[3]);
    auto dec = [](uint32_t u) { return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); };
    for (int a = 0; a < 3; a++) { out.ri_lo[a] = dec(r.bnd[a]); out.ri_hi[a] = dec(r.bnd[3 + a]); }
    return hipSuccess;
}

hipError_t iow_cull_build_device(const float *hot, uint32_t n, void *ws, size_t ws_bytes, float4 *wide, float4 *obox,
                                 IowCullDev &out, hipStream_t s, int max_levels, const uint32_t *d_priors) {
    if (n < 2 || n >= 16384 || !hot || !ws || ws_bytes < inw_build_workspace_bytes(n) || !wide || !obox)
        return hipErrorInvalidValue;
    BuildWs w;
    carve(ws, n, &w);
    BUILD_HIP(build_begin(w, s));
    // the priors' ten words ride in the counters' read-back (meta[4..13])
    if (d_priors) BUILD_HIP(hipMemcpyAsync(w.meta + 4, d_priors, 10 * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_iow_boxes, dim3(nblk(n)), dim3(kB), 0, s, hot, n, obox, w.box, w.cen, w.ids, w.meta);
    BUILD_HIP(hipGetLastError());
    BuildLevels r;
    BUILD_HIP(build_levels<8>(w, n, wide, level_cap(max_levels), s, r));
    out.n_wide = r.meta[1];
    out.depth = r.depth;
    out.nonfinite = r.meta[0];
    for (int k = 0; k < 10; k++) out.priors[k] = r.meta[4 + k];
    return hipSuccess;
}

// iow_prepare_device's workspace (256-B aligned pieces): the RI keys, the sorted keys, the mode's word,
// the ten result words, the radix sort's own
struct PrepWs {
    uint32_t *keys, *sorted, *out;
    unsigned long long *best;
    void *tmp;
    size_t tmp_bytes;
};
static size_t carve_prep(void *ws, uint32_t n, PrepWs *p) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *q = static_cast<char *>(ws) + off;
        off += (bytes + 255) & ~(size_t)255;
        return static_cast<void *>(q);
    };
    PrepWs t{};
    t.keys = static_cast<uint32_t *>(take((size_t)n * 4));
    t.sorted = static_cast<uint32_t *>(take((size_t)n * 4));
    t.best = static_cast<unsigned long long *>(take(8));
    t.out = static_cast<uint32_t *>(take(16 * 4));
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t.tmp_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n);
    t.tmp = take(t.tmp_bytes);
    if (p) *p = t;
    return off;
}

size_t iow_prepare_workspace_bytes(uint32_t n) { return n ? carve_prep(reinterpret_cast<void *>(256), n, nullptr) : 0; }

hipError_t iow_prepare_device(const float *types, const float *rec, uint32_t n, float *hot, float *cold, void *ws,
                              size_t ws_bytes, const uint32_t **d_priors, hipStream_t s) {
    if (!types || !rec || !n || n > 0x7fffffffu || !hot || !cold || !ws || ws_bytes < iow_prepare_workspace_bytes(n) ||
        !d_priors || (reinterpret_cast<uintptr_t>(ws) & 255u))
        return hipErrorInvalidValue;
    PrepWs p;
    carve_prep(ws, n, &p);
    float4 *h4 = reinterpret_cast<float4 *>(hot), *c4 = reinterpret_cast<float4 *>(cold);
    if (reinterpret_cast<uintptr_t>(rec) & 15u)
        hipLaunchKernelGGL(k_iow_prepare<false>, dim3(nblk(n)), dim3(kB), 0, s, types, rec, n, h4, c4, p.keys);
    else
        hipLaunchKernelGGL(k_iow_prepare<true>, dim3(nblk(n)), dim3(kB), 0, s, types, rec, n, h4, c4, p.keys);
    BUILD_HIP(hipGetLastError());
    size_t tb = p.tmp_bytes;
    BUILD_HIP(hipcub::DeviceRadixSort::SortKeys(p.tmp, tb, (const uint32_t *)p.keys, p.sorted, (int)n, 0, 32, s));
    BUILD_HIP(hipMemsetAsync(p.best, 0, 8, s));
    hipLaunchKernelGGL(k_iow_mode, dim3(nblk(n)), dim3(kB), 0, s, p.sorted, n, p.best);
    hipLaunchKernelGGL(k_iow_priors, dim3(1), dim3(64), 0, s, p.sorted, n, p.best, p.out);
    *d_priors = p.out;
    return hipGetLastError();
}

hipError_t update_iow_kernel_info(int which, int info[4]) {
    switch (which) {
        case 0: return kernel_info(k_iow_prepare<true>, occupancy_of(k_iow_prepare<true>, kB), info);
        case 1: return kernel_info(k_iow_prepare<false>, occupancy_of(k_iow_prepare<false>, kB), info);
        case 2: return kernel_info(k_iow_mode, occupancy_of(k_iow_mode, kB), info);
        case 3: return kernel_info(k_iow_priors, occupancy_of(k_iow_priors, 64), info);
        default: return hipErrorInvalidValue;
    }
}

// The wide nodes without the repeated low planes (InwScene::cnodes): 7 float4 per node, lx ly lz
// hx hy hz links, for the buffer-load walk (a ray's far plane of axis a sits at a + 3 (1 - s_a))
__global__ __launch_bounds__(kB) void k_compact_wnodes(const float4 *wn, uint32_t nw, float4 *cn) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= nw * 7u) return;
    const uint32_t w = i / 7u, k = i - 7u * w;
    cn[i] = wn[(size_t)w * 10 + (k < 6u ? k : 9u)];
}
hipError_t inw_compact_wnodes(const float4 *wnodes, uint32_t nw, float4 *cnodes, hipStream_t s) {
    if (!nw) return hipSuccess;
    hipLaunchKernelGGL(k_compact_wnodes, dim3(nblk(nw * 7u)), dim3(kB), 0, s, wnodes, nw, cnodes);
    return hipGetLastError();
}

// ---- scene update from device-resident records (rt_dev_scene_inw_update_device)
namespace {

// A block's records (up to kB of 28 floats) staged in LDS: the block reads its 28-KB run of the record
// array as consecutive float4 (whole lines; consecutive floats when the caller's pointer is not 16-B
// aligned), then every lane takes its own record from LDS.  The odd stride spreads a wave's lanes over
// the banks.
constexpr int kRecPad = 29;
__device__ __forceinline__ void stage_records(const float *geom, uint32_t n, float *s_rec) {
    const uint32_t first = blockIdx.x * kB, cnt = min((uint32_t)kB, n - first);
    const float *src = geom + (size_t)first * 28;
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {  // uniform
        const float4 *src4 = reinterpret_cast<const float4 *>(src);
        for (uint32_t i = threadIdx.x; i < cnt * 7u; i += kB) {
            const float4 v = src4[i];
            const uint32_t r = i / 7u;
            float *o = s_rec + r * kRecPad + 4u * (i - 7u * r);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < cnt * 28u; i += kB) s_rec[(i / 28u) * kRecPad + i % 28u] = src[i];
    }
    __syncthreads();
}

// the words k_inw_prepare reduces (dec[0]; dec[2..3] hold the stick-out maximum, a non-negative double
// whose bits order as a uint64)
constexpr uint32_t kDecNotSpheres = 1u, kDecMoving = 2u, kDecTextured = 4u, kDecNonFinite = 8u, kDecBinNonFinite = 16u;

// Records and decisions: the hot, cold and sphere records of every object by the statements of
// inw_records / inw_sphere_records (rt_scene_build.hip) in their order -- plain IEEE operations under
// -ffp-contract=off with the correctly rounded divide, so the bytes equal the host's -- and the
// update's decisions: all spheres, any delta not zero, any TextureIndex >= 1, rtamd::inw_stick_out's
// maximum over the caller's boxes (its float64 expression; +inf where it meets a value that is not
// finite) and whether rtamd::inw_bin_boxes would refuse an extent.  A wave folds its lanes, a block
// its waves, one atomic per block and word.
__global__ __launch_bounds__(kB) void k_inw_prepare(const float *geom, const float *aabbs, uint32_t n, int layout,
                                                    float4 *hot, float4 *cold, float4 *sph, uint32_t *dec) {
    __shared__ float s_rec[kB * kRecPad];
    __shared__ uint32_t s_fl[kB / 64];
    __shared__ double s_worst[kB / 64];
    stage_records(geom, n, s_rec);
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    uint32_t fl = 0u;
    double worst = 0.0;
    if (j < n) {
        float f[28];
        for (int k = 0; k < 28; k++) f[k] = s_rec[threadIdx.x * kRecPad + k];
        bool ident = true;  // the rotation exactly the identity (entries 1 and +-0)
        for (int k = 0; k < 9; k++) ident = ident && f[3 + k] == ((k % 4) == 0 ? 1.0f : 0.0f);
        const float ri = layout == 4 ? f[19] : f[20];
        float is[3], is2[3];
        for (int k = 0; k < 3; k++) {
            is[k] = 1.0f / f[12 + k];
            is2[k] = 1.0f / (f[12 + k] * f[12 + k]);
        }
        const float type = ident && (f[18] == 1.0f || f[18] == 2.0f) ? f[18] + 0.5f : f[18];
        float4 *h = hot + (size_t)j * (kInwHot / 4);
        h[0] = make_float4(f[0], f[1], f[2], f[3]);
        h[1] = make_float4(f[4], f[5], f[6], f[7]);
        h[2] = make_float4(f[8], f[9], f[10], f[11]);
        h[3] = make_float4(f[12], f[13], f[14], f[15]);
        h[4] = make_float4(f[16], f[17], type, f[19]);
        h[5] = make_float4(is[0], is[1], is[2], is2[0]);
        h[6] = make_float4(is2[1], is2[2], ri, 0.0f);
        float4 *c = cold + (size_t)j * (kInwCold / 4);
        if (layout == 1) {
            c[0] = make_float4(f[21], f[22], f[23], f[24]);
            c[1] = make_float4(f[25], f[26], f[27], f[20]);
        } else {
            const float ti = f[27] + 0.1f;
            const uint32_t tu = ti <= 0.0f ? 0u : (ti >= 4294967040.0f ? 0xffffffffu : (uint32_t)ti);
            c[0] = make_float4(f[20], f[21], f[22], f[23]);
            c[1] = make_float4(f[24], f[25], f[26], __uint_as_float(tu));
            if (ti >= 1.0f) fl |= kDecTextured;
        }
        float4 *o = sph + (size_t)j * 3;
        o[0] = make_float4(f[0], f[1], f[2], is[0]);
        o[1] = make_float4(f[15], f[16], f[17], ri);
        o[2] = make_float4(is2[0], is2[1], is2[2], f[19]);
        if ((int)(f[18] + 0.1f) != 1 || !(f[12] == f[13] && f[13] == f[14]) || !isfinite(f[12]) || !ident)
            fl |= kDecNotSpheres;
        if (f[15] != 0.0f || f[16] != 0.0f || f[17] != 0.0f) fl |= kDecMoving;
        // rtamd::inw_stick_out over the caller's box, and inw_bin_boxes' extent test
        const float *b = aabbs + (size_t)j * 6;
        float bx[6];
        for (int k = 0; k < 6; k++) bx[k] = b[k];
        const bool cuboid = (int)(f[18] + 0.1f) == 2;
        double big = 1.0;
        for (int k = 0; k < 6; k++) big = fmax(big, fabs((double)bx[k]));
        const double margin = (double)rtamd::kInwStickOut * big;
        bool bad = false;
        for (int a = 0; a < 3 && !bad; a++) {
            double e = 0.0;
            for (int cc = 0; cc < 3; cc++) {
                const double x = (double)f[3 + 3 * cc + a] * (double)f[12 + cc];
                e += cuboid ? 0.5 * fabs(x) : x * x;
            }
            if (!cuboid) e = sqrt(e);
            const double c1 = (double)f[a], c0 = c1 - (double)f[15 + a];
            const double out = fmax((double)bx[a] - (fmin(c0, c1) - e), (fmax(c0, c1) + e) - (double)bx[3 + a]);
            if (!isfinite(c0) || !isfinite(c1) || !isfinite(e) || isnan(bx[a]) || isnan(bx[3 + a]) || isnan(out)) bad = true;
            else worst = fmax(worst, out / margin);
        }
        if (bad) {
            worst = (double)__builtin_huge_valf();
            fl |= kDecNonFinite;
        }
        for (int a = 0; a < 3; a++) {
            double row = 0.0, col = 0.0;
            for (int cc = 0; cc < 3; cc++) {
                const double x = (double)f[3 + 3 * a + cc] * f[12 + cc], y = (double)f[3 + 3 * cc + a] * f[12 + cc];
                row += x * x;
                col += y * y;
            }
            if (!isfinite(sqrt(fmax(row, col)))) fl |= kDecBinNonFinite;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        fl |= (uint32_t)__shfl_xor((int)fl, off, 64);
        worst = fmax(worst, __shfl_xor(worst, off, 64));
    }
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (lane == 0u) { s_fl[wv] = fl; s_worst[wv] = worst; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < kB / 64; w++) { fl |= s_fl[w]; worst = fmax(worst, s_worst[w]); }
        if (fl) atomicOr(dec, fl);
        atomicMax(reinterpret_cast<unsigned long long *>(dec + 2), (unsigned long long)__double_as_longlong(worst));
    }
}

// rtamd::inw_bin_boxes' box of one record over the time ratios [r0, r1]: the centre segment widened by
// the half extent under both orientation conventions, inflated, rounded outward to float (its
// float64 expression, statement by statement)
__device__ __forceinline__ void bin_box(const float *f, double r0, double r1, float *bx) {
    double lo[3], hi[3];
    float big = 0.0f;
    for (int a = 0; a < 3; a++) {
        double row = 0.0, col = 0.0;
        for (int c = 0; c < 3; c++) {
            const double x = (double)f[3 + 3 * a + c] * f[12 + c], y = (double)f[3 + 3 * c + a] * f[12 + c];
            row += x * x;
            col += y * y;
        }
        const double e = sqrt(fmax(row, col));
        const double c0 = (double)f[a] - (double)f[15 + a] * (1.0 - r0);
        const double c1 = (double)f[a] - (double)f[15 + a] * (1.0 - r1);
        lo[a] = fmin(c0, c1) - e;
        hi[a] = fmax(c0, c1) + e;
        big = fmaxf(big, (float)fmax(fabs(lo[a]), fabs(hi[a])));
    }
    for (int a = 0; a < 3; a++) {
        const double e = (hi[a] - lo[a]) * 1e-3 + 1e-3 + (double)big * 1e-5;
        bx[a] = f32_down(lo[a] - e);
        bx[3 + a] = f32_up(hi[a] + e);
    }
}

// time bin [r0, r1]: every object's box into the SAH build's box / cen / ids, the largest |coordinate|
// into meta[3] (as k_leaves)
__global__ __launch_bounds__(kB) void k_bin_boxes(const float *geom, uint32_t n, double r0, double r1, float *box,
                                                  float *cen, uint32_t *ids, uint32_t *meta) {
    __shared__ float s_rec[kB * kRecPad];
    stage_records(geom, n, s_rec);
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    float wb = 0.0f;
    if (j < n) {
        float bx[6];
        bin_box(s_rec + threadIdx.x * kRecPad, r0, r1, bx);
        for (int k = 0; k < 3; k++) {
            box[6 * j + k] = bx[k];
            box[6 * j + 3 + k] = bx[3 + k];
            cen[3 * j + k] = 0.5f * (bx[k] + bx[3 + k]);
            wb = fmaxf(wb, fmaxf(fabsf(bx[k]), fabsf(bx[3 + k])));
        }
        ids[j] = j;
    }
    for (int off = 32; off >= 1; off >>= 1) wb = fmaxf(wb, __shfl_xor(wb, off, 64));
    if ((threadIdx.x & 63u) == 0u) atomicMax(meta + 3, __float_as_uint(wb));  // non-negative: uint order = value order
}

// the whole shutter interval as one bin: the boxes rt_inw_swept_boxes_async writes
__global__ __launch_bounds__(kB) void k_swept_boxes(const float *geom, uint32_t n, float *out) {
    __shared__ float s_rec[kB * kRecPad];
    stage_records(geom, n, s_rec);
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    if (j >= n) return;  // no cross-lane work after the staging
    float bx[6];
    bin_box(s_rec + threadIdx.x * kRecPad, 0.0, 1.0, bx);
    for (int k = 0; k < 6; k++) out[6 * (size_t)j + k] = bx[k];
}

// The bin trees into the scene's node array (rtamd::inw_wide_add_bins' layout): tree b, built with
// links of its own at tmp + b * n nodes, goes to node n0 + b * stride with its node links rebased to
// the whole array; the slots of a tree's stride past its nodes become empty nodes (planes 1e30, links 1e9).
struct BinTrees { uint32_t nw[16]; };
__global__ __launch_bounds__(kB) void k_bin_place(const float4 *tmp, uint32_t n, uint32_t bins, uint32_t stride,
                                                  uint32_t n0, BinTrees t, float4 *wnodes) {
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= bins * stride * 10u) return;  // no cross-lane work in this kernel
    const uint32_t node = i / 10u, r = i - 10u * node, b = node / stride, k = node - b * stride;
    float4 v;
    if (k >= t.nw[b]) {
        const float e = r < 9u ? 1e30f : __int_as_float(1000000000);
        v = make_float4(e, e, e, e);
    } else {
        v = tmp[((size_t)b * n + k) * 10 + r];
        if (r == 9u) {
            const int base = (int)(n0 + b * stride);
            int lk[4] = {__float_as_int(v.x), __float_as_int(v.y), __float_as_int(v.z), __float_as_int(v.w)};
            for (int c = 0; c < 4; c++)
                if (lk[c] > 0 && (uint32_t)lk[c] <= t.nw[b]) lk[c] += base;
            v = make_float4(__int_as_float(lk[0]), __int_as_float(lk[1]), __int_as_float(lk[2]), __int_as_float(lk[3]));
        }
    }
    wnodes[(size_t)(n0 + node) * 10 + r] = v;
}

}  // namespace

hipError_t inw_prepare_device(const float *geom, const float *aabbs, uint32_t n, int layout, float *hot, float *cold,
                              float *sph, uint32_t *dec, hipStream_t s) {
    if (!geom || !aabbs || !n || !hot || !cold || !sph || !dec) return hipErrorInvalidValue;
    BUILD_HIP(hipMemsetAsync(dec, 0, 8 * 4, s));
    hipLaunchKernelGGL(k_inw_prepare, dim3(nblk(n)), dim3(kB), 0, s, geom, aabbs, n, layout, reinterpret_cast<float4 *>(hot),
                       reinterpret_cast<float4 *>(cold), reinterpret_cast<float4 *>(sph), dec);
    return hipGetLastError();
}

InwDecisions inw_decisions(const uint32_t dec[8]) {
    InwDecisions d{};
    d.spheres = !(dec[0] & kDecNotSpheres);
    d.moving = (dec[0] & kDecMoving) != 0u;
    d.textured = (dec[0] & kDecTextured) != 0u;
    d.bins_finite = !(dec[0] & kDecBinNonFinite);
    const uint64_t bits = (uint64_t)dec[2] | ((uint64_t)dec[3] << 32);
    d.stick_out = __builtin_bit_cast(double, bits);
    return d;
}

hipError_t inw_swept_boxes_device(const float *geom, uint32_t n, float *out, hipStream_t s) {
    if (!n) return hipSuccess;
    if (!geom || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_swept_boxes, dim3(nblk(n)), dim3(kB), 0, s, geom, n, out);
    return hipGetLastError();
}

hipError_t inw_bin_trees_device(const float *geom, uint32_t n, uint32_t bins, void *ws, size_t ws_bytes, float4 *tmp,
                                InwBinsDev &out, hipStream_t s, int max_levels) {
    if (n < 2 || bins < 2 || bins > 16 || !geom || !ws || ws_bytes < inw_build_workspace_bytes(n) || !tmp)
        return hipErrorInvalidValue;
    BuildWs w;
    carve(ws, n, &w);
    out.stride = 0;
    out.wbound = 0.0f;
    for (uint32_t b = 0; b < bins; b++) {
        BUILD_HIP(build_begin(w, s));
        hipLaunchKernelGGL(k_bin_boxes, dim3(nblk(n)), dim3(kB), 0, s, geom, n, double(b) / bins, double(b + 1) / bins,
                           w.box, w.cen, w.ids, w.meta);
        BUILD_HIP(hipGetLastError());
        BuildLevels r;
        BUILD_HIP(build_levels<10>(w, n, tmp + (size_t)b * n * 10, level_cap(max_levels), s, r));
        out.nw[b] = r.meta[1];
        out.stride = std::max(out.stride, r.meta[1]);
        out.wbound = std::max(out.wbound, __builtin_bit_cast(float, r.meta[3]));
    }
    return hipSuccess;
}

hipError_t inw_bin_place_device(const float4 *tmp, uint32_t n, uint32_t bins, const InwBinsDev &t, uint32_t n0,
                                float4 *wnodes, hipStream_t s) {
    if (!tmp || !wnodes || bins < 2 || bins > 16 || !t.stride) return hipErrorInvalidValue;
    BinTrees bt{};
    for (uint32_t b = 0; b < bins; b++) bt.nw[b] = t.nw[b];
    hipLaunchKernelGGL(k_bin_place, dim3(nblk((size_t)bins * t.stride * 10)), dim3(kB), 0, s, tmp, n, bins, t.stride, n0, bt,
                       wnodes);
    return hipGetLastError();
}

hipError_t update_kernel_info(int which, int info[4]) {
    switch (which) {
        case 0: return kernel_info(k_inw_prepare, occupancy_of(k_inw_prepare, kB), info);
        case 1: return kernel_info(k_bin_boxes, occupancy_of(k_bin_boxes, kB), info);
        case 2: return kernel_info(k_swept_boxes, occupancy_of(k_swept_boxes, kB), info);
        case 3: return kernel_info(k_bin_place, occupancy_of(k_bin_place, kB), info);
        default: return hipErrorInvalidValue;
    }
}

size_t ri_scan_temp_bytes(size_t cells) {
    size_t sb = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, sb, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)cells);
    return sb;
}

static RiDims ri_dims(const double lo[3], const double inv[3], const int dim[3]) {
    RiDims d{};
    for (int a = 0; a < 3; a++) { d.lo[a] = lo[a]; d.inv[a] = inv[a]; d.dim[a] = dim[a]; }
    return d;
}

hipError_t ri_count_device(const float4 *leafbox, uint32_t n, void *ws, const double lo[3], const double inv[3],
                           const int dim[3], uint32_t *cells, void *tmp, size_t tmp_bytes, uint32_t *total,
                           uint32_t *over, hipStream_t s) {
    BuildWs w;
    carve(ws, n, &w);
    const RiDims d = ri_dims(lo, inv, dim);
    const size_t nc = (size_t)dim[0] * dim[1] * dim[2];
    BUILD_HIP(hipMemsetAsync(cells, 0, (nc + 1) * 4, s));
    BUILD_HIP(hipMemsetAsync(w.ri_flag, 0, 4, s));
    hipLaunchKernelGGL(k_ri_cells, dim3(nblk(n)), dim3(kB), 0, s, leafbox, n, d, 0, cells, nullptr, nullptr, w.ri_flag);
    BUILD_HIP(hipGetLastError());
    size_t sb = tmp_bytes;
    BUILD_HIP(hipcub::DeviceScan::InclusiveSum(tmp, sb, cells, cells, (int)(nc + 1), s));
    uint32_t tail[2];
    BUILD_HIP(hipMemcpyAsync(tail, cells + nc, 4, hipMemcpyDeviceToHost, s));
    BUILD_HIP(hipMemcpyAsync(tail + 1, w.ri_flag, 4, hipMemcpyDeviceToHost, s));
    BUILD_HIP(hipStreamSynchronize(s));
    *total = tail[0];
    *over = tail[1];
    return hipSuccess;
}

hipError_t ri_fill_device(const float4 *leafbox, uint32_t n, const double lo[3], const double inv[3], const int dim[3],
                          const uint32_t *cells, uint32_t *fill, uint32_t *ids, hipStream_t s) {
    const RiDims d = ri_dims(lo, inv, dim);
    const size_t nc = (size_t)dim[0] * dim[1] * dim[2];
    BUILD_HIP(hipMemcpyAsync(fill, cells, nc * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_ri_cells, dim3(nblk(n)), dim3(kB), 0, s, leafbox, n, d, 1, nullptr, fill, ids, nullptr);
    return hipGetLastError();
}

}  // namespace rtk
