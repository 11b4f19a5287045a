// rt_adaptive.hip -- adaptive sample passes on a device scene (rt_render_pass_pixels_async,
// rt_pass_select_async): a pass over a packed pixel list in which every pixel continues from its own
// sample count, and the ordered compaction of the pixels that still need samples.
//
// A listed pixel with count c renders samples [c, min(c + ns, S)) and folds them exactly as
// rt_render_pass_async folds them (rt_passes.hip), so a pixel that stopped after n samples holds, bit for
// bit, the state and image a uniform pass leaves after n samples.  Beside the state (rt_pass_state) a
// pixel keeps an rt_pass_aux: its count and `even`, the same fold restricted to the even sample indices,
// which the error estimate |acc / n - even / ceil(n / 2)| is formed from.
//
// INW: the composition of rt_passes.hip driven by the list -- k_adapt_rays writes the camera rays of
// (entry, j < ns) as path queries, sample = count + j (the invalid sample past S or for an entry outside
// the image), the unchanged path kernel answers them, k_adapt_fold folds an entry's answers in sample
// order and advances its count, so the next chunk's rays start from the new count.
// IOW-03: k_iow_adapt is k_iow_pass with the pixel, its first sample and its RI fields taken from the list
// entry, the pixel's count and its state, and `even` folded beside the sum: both run iow_pass_loop
// (rt_pass_loop.hpp), this one with the list as its source.
// Shared with rt_passes.hip through rt_pass_common.hpp: the frames, listed(), the INW record writer, the
// fold's start from the state and the image write.  The INW folds' sample loops stay in their kernels: moved
// into one function, k_adapt_fold's registers changed (29 SGPRs, or 40 VGPRs, against the pinned 27 / 39).
// Select: a stable partition of the rectangle's units (unit_pixel's order) in three plain launches --
// per-block counts, an exclusive scan of the block partials in one block, the scatter.  No block waits on
// another block.
// Every kernel but the scan has a second instance, TL, for rt_render_pass_slots_async and
// rt_pass_select_tiles_async: a list entry is a slot of a packed tile list (PassEntry<TL>), state, aux, image,
// err and answers are indexed by slot, and the select's units are the list's.  The pixel-list instances drop
// the tile list with pass_frame and keep their code, as rt_passes.hip's rectangle instances do.
#include <type_traits>

#include "rt_pass_loop.hpp"

namespace rtk {

// rt_pass_aux as the kernels read it: (even.xyz, count bits)
__device__ __forceinline__ uint32_t aux_count(const float4 *aux, size_t out) { return __float_as_uint(aux[out].w); }

// A list entry as the INW pair reads it: its pixel, whether it is handled, and (TL) its slot.  The index of
// its state, aux and image is y * W + x, or the slot on a packed tile list.
struct Entry { int x, y; bool listed; uint32_t slot; };
template <bool TL>
__device__ __forceinline__ Entry entry_of(const Frame &F, PassEntry<TL> e) {
    if constexpr (TL) {
        const UnitPix q = slot_pixel(F, e);
        return Entry{q.x, q.y, q.in_image, e};
    } else {
        return Entry{e.x, e.y, listed(F, e), 0u};
    }
}
template <bool TL>
__device__ __forceinline__ size_t entry_index(const Frame &F, const Entry &p) {
    return TL ? (size_t)p.slot : (size_t)p.y * F.W + p.x;
}

// ------------------------------------------------------------------------------------------ INW
// One lane per record: record k * ns + j is the camera ray of sample count + j of entry k's pixel
// (pass_ray_record); the sample is the invalid one past `stop` or for an entry outside the image.
// n = n_pixels * ns <= 2^31.
template <bool TL>
__global__ __launch_bounds__(kBlock)
void k_adapt_rays(Frame Fin, InwScene S, const PassEntry<TL> *__restrict__ pixels, const float4 *__restrict__ aux,
                  uint32_t stop, uint32_t ns, uint32_t n, float4 *__restrict__ rays) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= n) return;
    Frame F{};
    pass_frame_of<TL>(F, Fin);
    const uint32_t k = i / ns, j = i - k * ns;
    const Entry p = entry_of<TL>(F, pixels[k]);
    float4 *r = rays + 2 * (size_t)i;
    uint32_t s = 0xffffffffu;
    if (p.listed) {
        const uint32_t c = aux_count(aux, entry_index<TL>(F, p));
        if (c < stop && j < stop - c) s = c + j;
    }
    if (s != 0xffffffffu) pass_ray_record(S, F, p.x, p.y, s, r);
    else pass_no_record(r);
}

// One lane per entry: End() over the entry's answers of samples [c, min(c + ns, stop)) in sample order,
// from the pixel's state (pass_fold_begin) and aux -- sqrt(colour) added to acc and, at even samples, to
// even; the depth of sample spp / 2 -- and the state, the aux and the new count back.  last: the chunk is
// the pass's last, and the image acc * RN(1 / count) and the depth are written (also for an entry that had
// nothing left to render).
template <bool TL>
__global__ __launch_bounds__(kBlock)
void k_adapt_fold(Frame Fin, const PassEntry<TL> *__restrict__ pixels, uint32_t n_pixels, uint32_t stop, uint32_t ns,
                  uint32_t last, const float4 *__restrict__ out, float4 *__restrict__ state,
                  float4 *__restrict__ aux) {
    const uint32_t k = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (k >= n_pixels) return;
    Frame F{};
    pass_frame_of<TL>(F, Fin);
    const Entry p = entry_of<TL>(F, pixels[k]);
    if (!p.listed) return;
    const size_t o = entry_index<TL>(F, p);
    const uint32_t mid = (uint32_t)F.spp / 2u;
    const float4 x = aux[o];
    const uint32_t c = __float_as_uint(x.w);
    f3 acc, ev = f3{x.x, x.y, x.z};
    float dmid;
    pass_fold_begin(state, o, c, acc, dmid);
    const uint32_t m = c < stop ? (ns < stop - c ? ns : stop - c) : 0u;  // samples to fold
    const float4 *a = out + 2 * (size_t)k * ns;
    for (uint32_t j = 0; j < m; j++) {
        const float4 r = a[2 * (size_t)j];
        const f3 g = f3{__builtin_sqrtf(r.x), __builtin_sqrtf(r.y), __builtin_sqrtf(r.z)};
        const uint32_t s = c + j;
        acc = sel(s == 0, g, acc + g);
        if ((s & 1u) == 0) ev = sel(s == 0, g, ev + g);
        if (s == mid) dmid = r.w;
    }
    const uint32_t c1 = c + m;
    if (m != 0) {
        state[2 * o] = make_float4(acc.x, acc.y, acc.z, dmid);
        aux[o] = make_float4(ev.x, ev.y, ev.z, __uint_as_float(c1));
    }
    if (!last) return;
    pass_write_image(F, o, acc, rcp((float)c1), dmid);
}

// ------------------------------------------------------------------------------------------ IOW-03
// The shared loop over the list: a lane's samples are [count, min(count + ns, stop)); an entry with
// nothing left has its image rewritten from its state.
template <bool LN, bool TL>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kPassIowWaves<LN>)))
void k_iow_adapt(Frame Fin, IowScene S, const PassEntry<TL> *__restrict__ pixels, uint32_t stop, uint32_t ns,
                 float4 *__restrict__ state, float4 *__restrict__ aux, unsigned *queue, uint32_t rounds,
                 uint32_t n_units) {
    using Src = std::conditional_t<TL, SlotPass, ListPass>;
    iow_pass_loop<LN>(Fin, S, Src{pixels, aux, stop, ns}, state, queue, rounds, n_units);
}

// ------------------------------------------------------------------------------------------ select
// What the three select kernels share.  The error of a pixel with n samples: a = acc * RN(1 / n),
// e = even * RN(1 / ceil(n / 2)), err = (|a.x - e.x| + |a.y - e.y|) + |a.z - e.z| in binary32, +inf for
// n < 2; the pixel is active iff n < stop and (n < min_samples or not err <= tol): a NaN keeps sampling.
struct Select {
    const float4 *state, *aux;
    float tol;
    uint32_t min_samples, stop;
};
__device__ __forceinline__ bool select_active(const Select &Q, size_t o, float &err) {
    const float4 x = Q.aux[o];
    const uint32_t n = __float_as_uint(x.w);
    err = __builtin_inff();
    if (n >= 2) {
        const float4 s = Q.state[2 * o];
        const float in = rcp((float)n), ih = rcp((float)((n + 1u) / 2u));
        const f3 a = f3{s.x, s.y, s.z} * in, e = f3{x.x, x.y, x.z} * ih;
        err = (__builtin_fabsf(a.x - e.x) + __builtin_fabsf(a.y - e.y)) + __builtin_fabsf(a.z - e.z);
    }
    return n < Q.stop && (n < Q.min_samples || !(err <= Q.tol));
}
// the rectangle of a frame for unit_pixel, or (TL) its packed tile list, everything else 0
template <bool TL>
__device__ __forceinline__ void select_frame(Frame &F, const Frame &in) {
    F.W = in.W; F.H = in.H;
    if (TL) { F.tiles = in.tiles; F.n_tiles = in.n_tiles; F.tile_size = in.tile_size; }
    else { F.x0 = in.x0; F.y0 = in.y0; F.tw = in.tw; F.th = in.th; }
}

constexpr int kSelWaves = kBlock / 64;

// 1: a lane per unit, a block's (active, inactive) counts into part[block]; the error image.
// TL, here and in the scatter: the units of a packed tile list, state, aux and err indexed by slot.
template <bool TL>
__global__ __launch_bounds__(kBlock)
void k_select_count(Frame Fin, Select Q, uint32_t n_units, uint2 *__restrict__ part, float *__restrict__ d_err) {
    __shared__ uint2 s_cnt[kSelWaves];
    Frame F{};
    select_frame<TL>(F, Fin);
    const uint32_t u = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    bool in = false, act = false;
    if (u < n_units) {
        const UnitPix p = pass_unit_pixel<TL>(F, u);
        if (p.in_image) {
            float err;
            in = true;
            act = select_active(Q, p.out, err);
            if (d_err) d_err[p.out] = err;
        }
    }
    const uint32_t na = (uint32_t)__popcll(__ballot(act)), ni = (uint32_t)__popcll(__ballot(in && !act));
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = make_uint2(na, ni);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 t = make_uint2(0u, 0u);
        for (int w = 0; w < kSelWaves; w++) { t.x += s_cnt[w].x; t.y += s_cnt[w].y; }
        part[blockIdx.x] = t;
    }
}

// 2: one block: part[0 .. n) becomes its exclusive scan, part[n] the totals, *n_active the active total.
__global__ __launch_bounds__(kBlock)
void k_select_scan(uint2 *__restrict__ part, uint32_t n, uint32_t *__restrict__ n_active) {
    __shared__ uint2 s_sum[kSelWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint2 carry = make_uint2(0u, 0u);  // the totals of the rounds before (block-uniform)
    for (uint32_t base = 0; base < n; base += (uint32_t)kBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint2 v = i < n ? part[i] : make_uint2(0u, 0u);
        uint2 inc = v;  // inclusive scan over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ax = __shfl_up(inc.x, d, 64), ay = __shfl_up(inc.y, d, 64);
            if (lane >= (uint32_t)d) { inc.x += ax; inc.y += ay; }
        }
        if (lane == 63u) s_sum[wave] = inc;
        __syncthreads();
        uint2 off = carry, tot = carry;
        for (uint32_t w = 0; w < (uint32_t)kSelWaves; w++) {
            if (w < wave) { off.x += s_sum[w].x; off.y += s_sum[w].y; }
            tot.x += s_sum[w].x; tot.y += s_sum[w].y;
        }
        if (i < n) part[i] = make_uint2(off.x + inc.x - v.x, off.y + inc.y - v.y);
        carry = tot;
        __syncthreads();  // s_sum is rewritten by the next round
    }
    if (threadIdx.x == 0) {
        part[n] = carry;
        *n_active = carry.x;
    }
}

// 3: the scatter: an active unit's pixel at its active rank, an inactive one's {-1, -1} at the active
// total + its inactive rank (so the list's tail, up to the rectangle's pixel count, is padding).  TL: the
// slots, and 0xffffffff for the padding.
template <bool TL>
__device__ __forceinline__ PassEntry<TL> select_entry(const UnitPix &p) {
    if constexpr (TL) return (uint32_t)p.out;
    else return make_int2(p.x, p.y);
}
template <bool TL>
__device__ __forceinline__ PassEntry<TL> select_none() {
    if constexpr (TL) return kSlotNone;
    else return make_int2(-1, -1);
}

template <bool TL>
__global__ __launch_bounds__(kBlock)
void k_select_scatter(Frame Fin, Select Q, uint32_t n_units, uint32_t n_blocks, const uint2 *__restrict__ part,
                      PassEntry<TL> *__restrict__ list) {
    __shared__ uint2 s_cnt[kSelWaves];
    Frame F{};
    select_frame<TL>(F, Fin);
    const uint32_t u = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    bool in = false, act = false;
    PassEntry<TL> px = select_none<TL>();
    if (u < n_units) {
        const UnitPix p = pass_unit_pixel<TL>(F, u);
        if (p.in_image) {
            float err;
            in = true;
            act = select_active(Q, p.out, err);
            px = select_entry<TL>(p);
        }
    }
    const unsigned long long ma = __ballot(act), mi = __ballot(in && !act);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) s_cnt[wave] = make_uint2((uint32_t)__popcll(ma), (uint32_t)__popcll(mi));
    __syncthreads();
    uint2 off = part[blockIdx.x];
    for (uint32_t w = 0; w < (uint32_t)kSelWaves; w++)
        if (w < wave) { off.x += s_cnt[w].x; off.y += s_cnt[w].y; }
    const uint32_t total = part[n_blocks].x;
    if (act) list[off.x + lanes_below(ma)] = px;
    else if (in) list[total + off.y + lanes_below(mi)] = select_none<TL>();
}

// ------------------------------------------------------------------------------------------ launch
namespace {
int g_chunk_cap = 0;  // rt_debug_adaptive_chunk: 0 = none

template <class Kn>
hipError_t adapt_info(Kn kernel, int info[4]) {
    return kernel_info(kernel, occupancy_of(kernel, kBlock), info);
}
// resident blocks per CU of the instance a scene runs, asked once each
int iow_adapt_blocks(bool ln, bool tl) {
    static const int nb[4] = {occupancy_of(k_iow_adapt<false, false>, kBlock), occupancy_of(k_iow_adapt<true, false>, kBlock),
                              occupancy_of(k_iow_adapt<false, true>, kBlock), occupancy_of(k_iow_adapt<true, true>, kBlock)};
    return nb[(tl ? 2 : 0) + (ln ? 1 : 0)];
}
dim3 lanes_grid(uint32_t n) { return dim3((n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock); }

// The launches, one body for the pixel list (TL = false) and the slot list of f's packed tile list.
template <bool TL>
hipError_t adapt_rays(const Frame &f, const InwScene &sc, const PassEntry<TL> *list, uint32_t n_list, const float4 *aux,
                      uint32_t stop, uint32_t ns, float4 *rays, hipStream_t s) {
    const uint32_t n = n_list * ns;  // <= 2^31 (the caller's chunks)
    hipLaunchKernelGGL(k_adapt_rays<TL>, lanes_grid(n), dim3(kBlock), 0, s, f, sc, list, aux, stop, ns, n, rays);
    return hipGetLastError();
}

template <bool TL>
hipError_t adapt_fold(const Frame &f, const PassEntry<TL> *list, uint32_t n_list, uint32_t stop, uint32_t ns, bool last,
                      const float4 *out, float4 *state, float4 *aux, hipStream_t s) {
    hipLaunchKernelGGL(k_adapt_fold<TL>, lanes_grid(n_list), dim3(kBlock), 0, s, f, list, n_list, stop, ns,
                       last ? 1u : 0u, out, state, aux);
    return hipGetLastError();
}

template <bool TL>
hipError_t iow_adapt(const Frame &f, const IowScene &sc, const PassEntry<TL> *list, uint32_t n_list, uint32_t stop,
                     uint32_t ns, float4 *state, float4 *aux, unsigned *queue, int cus, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(queue, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const bool ln = iow_lds(sc);
    const ClaimGrid cg = claim_grid(n_list, cus, iow_adapt_blocks(ln, TL), pass_max_blocks_now());
    const dim3 g(cg.grid), b(kBlock);
    if (ln) hipLaunchKernelGGL((k_iow_adapt<true, TL>), g, b, 0, s, f, sc, list, stop, ns, state, aux, queue, cg.rounds, n_list);
    else hipLaunchKernelGGL((k_iow_adapt<false, TL>), g, b, 0, s, f, sc, list, stop, ns, state, aux, queue, cg.rounds, n_list);
    return hipGetLastError();
}

template <bool TL>
hipError_t pass_select(const Frame &f, const float4 *state, const float4 *aux, float tol, uint32_t min_samples,
                       uint32_t stop, PassEntry<TL> *list, uint32_t *n_active, float *err, uint2 *part, hipStream_t s) {
    const uint32_t n_units = units_of(f), n_blocks = select_blocks(f);
    const Select q{state, aux, tol, min_samples, stop};
    const dim3 g(n_blocks), b(kBlock);
    hipLaunchKernelGGL(k_select_count<TL>, g, b, 0, s, f, q, n_units, part, err);
    hipLaunchKernelGGL(k_select_scan, dim3(1), b, 0, s, part, n_blocks, n_active);
    hipLaunchKernelGGL(k_select_scatter<TL>, g, b, 0, s, f, q, n_units, n_blocks, part, list);
    return hipGetLastError();
}
}  // namespace

hipError_t adaptive_kernel_info(int which, int info[4]) {
    switch (which) {
        case 0: return adapt_info(k_adapt_rays<false>, info);
        case 1: return adapt_info(k_adapt_fold<false>, info);
        case 2: return adapt_info(k_iow_adapt<true, false>, info);
        case 3: return adapt_info(k_iow_adapt<false, false>, info);
        case 4: return adapt_info(k_select_count<false>, info);
        case 5: return adapt_info(k_select_scan, info);
        case 6: return adapt_info(k_select_scatter<false>, info);
        case 7: return adapt_info(k_adapt_rays<true>, info);  // the tile-list instances
        case 8: return adapt_info(k_adapt_fold<true>, info);
        case 9: return adapt_info(k_iow_adapt<true, true>, info);
        case 10: return adapt_info(k_iow_adapt<false, true>, info);
        case 11: return adapt_info(k_select_count<true>, info);
        case 12: return adapt_info(k_select_scatter<true>, info);
    }
    return hipErrorInvalidValue;
}

int adaptive_chunk_cap_now() { return g_chunk_cap; }

int adaptive_chunk_cap(int samples) {
    const int prev = g_chunk_cap;
    g_chunk_cap = samples > 0 ? samples : 0;
    return prev;
}

hipError_t launch_adapt_rays(const Frame &f, const InwScene &sc, const int2 *pixels, uint32_t n_pixels,
                             const float4 *aux, uint32_t stop, uint32_t ns, float4 *rays, hipStream_t s) {
    return adapt_rays<false>(f, sc, pixels, n_pixels, aux, stop, ns, rays, s);
}
hipError_t launch_adapt_rays(const Frame &f, const InwScene &sc, const uint32_t *slots, uint32_t n_slots,
                             const float4 *aux, uint32_t stop, uint32_t ns, float4 *rays, hipStream_t s) {
    return adapt_rays<true>(f, sc, slots, n_slots, aux, stop, ns, rays, s);
}

hipError_t launch_adapt_fold(const Frame &f, const int2 *pixels, uint32_t n_pixels, uint32_t stop, uint32_t ns,
                             bool last, const float4 *out, float4 *state, float4 *aux, hipStream_t s) {
    return adapt_fold<false>(f, pixels, n_pixels, stop, ns, last, out, state, aux, s);
}
hipError_t launch_adapt_fold(const Frame &f, const uint32_t *slots, uint32_t n_slots, uint32_t stop, uint32_t ns,
                             bool last, const float4 *out, float4 *state, float4 *aux, hipStream_t s) {
    return adapt_fold<true>(f, slots, n_slots, stop, ns, last, out, state, aux, s);
}

hipError_t launch_iow_adapt(const Frame &f, const IowScene &sc, const int2 *pixels, uint32_t n_pixels, uint32_t stop,
                            uint32_t ns, float4 *state, float4 *aux, unsigned *queue, int cus, hipStream_t s) {
    return iow_adapt<false>(f, sc, pixels, n_pixels, stop, ns, state, aux, queue, cus, s);
}
hipError_t launch_iow_adapt(const Frame &f, const IowScene &sc, const uint32_t *slots, uint32_t n_slots, uint32_t stop,
                            uint32_t ns, float4 *state, float4 *aux, unsigned *queue, int cus, hipStream_t s) {
    return iow_adapt<true>(f, sc, slots, n_slots, stop, ns, state, aux, queue, cus, s);
}

uint32_t select_blocks(const Frame &f) { return (units_of(f) + (uint32_t)kBlock - 1u) / (uint32_t)kBlock; }

hipError_t launch_pass_select(const Frame &f, const float4 *state, const float4 *aux, float tol, uint32_t min_samples,
                              uint32_t stop, int2 *list, uint32_t *n_active, float *err, uint2 *part, hipStream_t s) {
    return pass_select<false>(f, state, aux, tol, min_samples, stop, list, n_active, err, part, s);
}
hipError_t launch_pass_select(const Frame &f, const float4 *state, const float4 *aux, float tol, uint32_t min_samples,
                              uint32_t stop, uint32_t *slots, uint32_t *n_active, float *err, uint2 *part, hipStream_t s) {
    return pass_select<true>(f, state, aux, tol, min_samples, stop, slots, n_active, err, part, s);
}

}  // namespace rtk
