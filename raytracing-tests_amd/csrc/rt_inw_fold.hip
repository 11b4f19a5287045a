// rt_inw_fold.hip -- the In-Next-Week fold pipeline for gfx950: the pixel beams, the
// probe, the sky blocks, the claim order, and the two kernels that keep End()'s sum on chip,
// k_inw_pm (pixel-major) and k_inw_sm (sample-major), with launch_inw_fold, which runs them.  The
// flagship configurations (C3, C5) render here.
#include <type_traits>

#include "rt_render_common.hpp"
#include "rt_inw_shade.hpp"

namespace rtk {

// ---------------------------------------------------------------- INW wave counts
// Waves per SIMD of the 256-lane INW kernels: INW-04 (LIGHTS) at 3 (159 VGPRs, no spills);
// INW-01 at 4 (128 VGPRs with a few spills, 8% faster on C3 than 3 waves in round 2).
constexpr int kInwWaves = 3;
constexpr int kInw01Waves = 4;  // INW-01: 128 VGPRs with a few spills, 8% faster on C3 than 3 waves

// ---------------------------------------------------------------- INW: on-chip End() folds
// End() (01_BVH...glsl:625-653, 664-675) adds each sample's sqrt(colour) in sample order and
// stores the mean.  The INW kernels below keep that sum on chip.  A wave claims work from the
// global queue, hands its samples to its lanes as a stream g = 0, 1, 2, ... in a fixed order, and
// a lane that finishes a sample takes the next stream entry at once (lane persistence).  A
// finished sample stores its sqrt(colour) into the wave's private ring; the wave folds the ring in
// each pixel's sample order, End()'s float order, and writes a pixel when its last sample is
// folded.  The ring: k_inw_pm's 768-lane instances keep it in LDS (InwScene::lring, the default:
// 256 entries per wave as r, g, b planes; an entry is finished when no busy lane holds it); the
// other kernels keep a global ring of {sqrt(colour), tag g} per wave (16 KB per wave at 1024
// entries, not L2-resident at the chip's 3,000-odd waves: it reaches the fabric).
// The middle sample's depth goes with the pixel's colour.  Entries beyond the oldest unfolded one + ring size are not issued (a
// straggling sample holds the window; the other lanes keep running until it fills).  Counters
// accumulate per lane.  Two stream orders, one per kind of ray coherence:
//  - k_inw_pm (pixel-major): the wave claims pixels and runs all samples of one pixel back to
//    back, so its 64 lanes trace 64 consecutive samples of one pixel -- nearly the same ray where
//    lens, motion and scatter offsets are small next to the scene's detail (C3: 10k small
//    spheres, neighbouring pixels see different spheres).  The fold is wave-serial: once per
//    iteration the wave loads the next 64 ring entries and every lane adds the leading finished
//    run in order (each lane computes the same sum).
//  - k_inw_sm (sample-major): the wave claims 8x8 pixel blocks and runs one sample index over the
//    64 pixels of the block at a time (rows s = 0, 1, ...), so its lanes trace neighbouring
//    pixels at one lens offset, time and scatter direction -- the same ray where the scene is
//    coarse next to a pixel (C5: the Cornell walls).  The fold is lane-parallel: lane p holds
//    pixel p's sum and adds its own samples as they finish.
// k_inw_probe picks one per frame on the device (mode[]): over a sparse set of 8x8 blocks it
// traces one primary ray per pixel; the frame is "coarse" when most blocks with a hit see one
// object in all their pixels.  Both kernels are launched; the one not picked exits at once.
// A fold-ring entry's tag: the low 26 bits of its stream position and the frame's ring epoch
// (0..62) in the high 6 (InwScene::ring_epoch).  An entry left by one of the 62 frames before
// carries another epoch, and the host clears the rings with 0xff bytes (an epoch of 63, never
// valid) whenever the epoch wraps to 0, so a stale entry never passes for a finished one and no
// per-frame clear is needed.  Within a frame, slot g mod R last held g - R (R <= 2^16 < 2^26).
// The fold kernels' framebuffer stores.  Measured and not kept (round 5): nontemporal stores here
// raised C5's L2-to-fabric writes from 4.7 to 37 GB per frame (each streaming 16-B store leaves L2
// as its own partial-line write) at the same frame time.
__device__ __forceinline__ void fb_store(const Frame &f, size_t o, float4 v) {
    reinterpret_cast<float4 *>(f.out_rgba)[o] = v;
}
__device__ __forceinline__ void depth_store(const Frame &f, size_t o, float d) { f.out_depth[o] = d; }
__device__ __forceinline__ uint32_t ring_tag(const InwScene &S, uint32_t g) {
    return (g & 0x03ffffffu) | S.ring_epoch;
}
__device__ __forceinline__ float rdl(float v, uint32_t l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l));
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// the probe's verdict: mode[0] = blocks with a hit, mode[1] = those whose pixels all see one object
__device__ __forceinline__ bool inw_sample_major(const uint32_t *mode, uint32_t force) {
    if (force == 1u) return false;
    if (force == 2u) return true;
    const uint32_t hit = uni(mode[0]), same = uni(mode[1]);
    return 2u * same >= hit && hit > 0u;
}
// Pixel beams (DESIGN.md §5 "Pixel beams").  A pixel's primary rays all pass through its focal
// point F = co + cd * focus and leave the lens disk around C0 = co + cd (radius <= delta0), so they
// lie within beam_R of the central ray C0 + t * cd over t in [beam_tmin, beam_tfar] (host bounds).
// One lane per pixel unit walks the culling BVH with that ray against the boxes inflated by
// beam_R and keeps the beam_cap leaves of smallest entry t, sorted; beam_cut is the smallest
// entry t of a leaf it could not keep.
// bp (rt_options.inw_beam_prune, rt_beam_prune.hpp): a child that passes that test is tested again
// with the beam's radius over its own depth interval (bp.mode >= 1), and a leaf of a sphere scene
// against the segment its centre sweeps in the list's time bin (bp.mode = 2).  A leaf that fails
// can be touched by no primary ray of the pixel: it is neither listed nor counted in the cut.  The
// key of a listed leaf stays the entry into the box inflated by beam_R.
constexpr int kBeamBlock = 128, kBeamStack = 48, kBeamCapMax = 32;
__global__ __launch_bounds__(kBeamBlock) void k_inw_beam(Frame f, InwScene S, const uint32_t *mode, uint32_t force,
                                                         BeamPrune bp) {
    if (inw_sample_major(mode, force)) return;
    __shared__ int st[kBeamStack * kBeamBlock];
    __shared__ uint2 lst[kBeamCapMax * kBeamBlock];
    const uint32_t u = blockIdx.x * kBeamBlock + threadIdx.x, lane = threadIdx.x & 63u;
    if (u >= units_total(f)) return;  // whole waves (units come in 8x8 blocks of 64)
    const UnitPix px = unit_pixel(f, u);
    const uint32_t bo = blockIdx.y * S.beam_units;  // time bin blockIdx.y (beam_bins > 1): its tree, its lists
    uint32_t *nout = const_cast<uint32_t *>(S.beam_n) + bo;
    float *cout = const_cast<float *>(S.beam_cut) + bo;
    const uint32_t cap = S.beam_cap;
    uint2 *L = lst + threadIdx.x;
    uint32_t nl = 0;
    float cut = kMiss;
    bool off = false;
    if (px.in_image) {
        const f3 cd = inw_pixel_dir(f, px.x, px.y);
        const f3 o = mk(f.pos[0], f.pos[1], f.pos[2]) + cd;
        const f3 id = f3{rcp(cd.x), rcp(cd.y), rcp(cd.z)};
        off = !(__builtin_isfinite(id.x) && __builtin_isfinite(id.y) && __builtin_isfinite(id.z));
        const float R = S.beam_R, t0 = S.beam_tmin, t1 = S.beam_tfar;
        // near / far planes of each axis for this direction, inflated outward by R
        const uint32_t ox = cd.x < 0.0f ? 3u : 0u, oy = cd.y < 0.0f ? 4u : 1u, oz = cd.z < 0.0f ? 5u : 2u;
        const f3 rn = f3{cd.x < 0.0f ? R : -R, cd.y < 0.0f ? R : -R, cd.z < 0.0f ? R : -R};
        const float oa[3] = {o.x, o.y, o.z}, ida[3] = {id.x, id.y, id.z}, cda[3] = {cd.x, cd.y, cd.z};
        const bool neg[3] = {cd.x < 0.0f, cd.y < 0.0f, cd.z < 0.0f};
        int *stk = st + threadIdx.x;
        int sp = 0, cur = S.beam_bins > 1u ? (int)(1u + S.wbin_base + blockIdx.y * S.wbin_stride) : S.wroot;
        while (!off) {
            const float4 *nd = S.wnodes + kInwNodeF4 * (cur - 1);
            const float4 nx = nd[ox], fx = nd[ox + 3], ny = nd[oy], fy = nd[oy + 3], nz = nd[oz], fz = nd[oz + 3];
            const float4 lk = nd[9];
            const float nxa[4] = {nx.x, nx.y, nx.z, nx.w}, fxa[4] = {fx.x, fx.y, fx.z, fx.w};
            const float nya[4] = {ny.x, ny.y, ny.z, ny.w}, fya[4] = {fy.x, fy.y, fy.z, fy.w};
            const float nza[4] = {nz.x, nz.y, nz.z, nz.w}, fza[4] = {fz.x, fz.y, fz.z, fz.w};
            const int lka[4] = {__float_as_int(lk.x), __float_as_int(lk.y), __float_as_int(lk.z), __float_as_int(lk.w)};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float te = fmaxf(fmaxf(((nxa[k] + rn.x) - o.x) * id.x, ((nya[k] + rn.y) - o.y) * id.y),
                                       ((nza[k] + rn.z) - o.z) * id.z);
                const float tx = fminf(fminf(((fxa[k] - rn.x) - o.x) * id.x, ((fya[k] - rn.y) - o.y) * id.y),
                                       ((fza[k] - rn.z) - o.z) * id.z);
                if (!(fmaxf(te, t0) <= fminf(tx, t1))) continue;
                const int l = lka[k];
                if (bp.mode) {
                    const float nr[3] = {nxa[k], nya[k], nza[k]}, fr[3] = {fxa[k], fya[k], fza[k]};
                    if (!beam_box_keep(bp, nr, fr, oa, ida, neg, te, tx)) continue;
                    if (l <= 0 && bp.mode >= 2u && S.sph) {
                        const float4 p = S.sph[3 * (uint32_t)(-l)], q = S.sph[3 * (uint32_t)(-l) + 1];
                        const float pa[4] = {p.x, p.y, p.z, p.w}, qa[3] = {q.x, q.y, q.z};
                        if (!beam_sphere_keep(bp, oa, cda, pa, qa, S.beam_bins > 1u ? blockIdx.y : 0u)) continue;
                    }
                }
                if (l > 0) {
                    if (sp == kBeamStack) off = true;
                    else stk[(sp++) * kBeamBlock] = l;
                } else {  // keep the cap smallest entries, sorted (insertion)
                    float tv = te;
                    uint32_t gv = (uint32_t)(-l);
                    if (nl == cap) {
                        const float last = __uint_as_float(L[(cap - 1) * kBeamBlock].y);
                        if (!(tv < last)) { cut = fminf(cut, tv); continue; }
                        cut = fminf(cut, last);
                        nl--;
                    }
                    uint32_t j = nl;
                    while (j > 0 && __uint_as_float(L[(j - 1) * kBeamBlock].y) > tv) {
                        L[j * kBeamBlock] = L[(j - 1) * kBeamBlock];
                        j--;
                    }
                    L[j * kBeamBlock] = make_uint2(gv, __float_as_uint(tv));
                    nl++;
                }
            }
            if (off || sp == 0) break;
            cur = stk[(--sp) * kBeamBlock];
        }
    }
    // The block's 64 lists packed densely in its region of 64 * cap entries, in unit order (the
    // fold kernel claims a block's pixels one after another, so their lists share cache lines):
    // beam_n[u] = offset in the region << 8 | count
    const uint32_t cnt = off ? 0u : nl;
    uint32_t incl = cnt;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += y;
    }
    const uint32_t at = incl - cnt;
    const size_t base = ((size_t)bo + (u & ~63u)) * cap + at;
    if (S.beam16) {  // object ids < 2^16: the id and the high half of max(t, 0) (t rounded down)
        uint32_t *dst = reinterpret_cast<uint32_t *>(const_cast<uint2 *>(S.beam)) + base;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint2 e = L[j * kBeamBlock];
            const uint32_t tb = __uint_as_float(e.y) > 0.0f ? e.y : 0u;
            dst[j] = (e.x & 0xffffu) | (tb & 0xffff0000u);
        }
    } else {
        uint2 *dst = const_cast<uint2 *>(S.beam) + base;
        for (uint32_t j = 0; j < cnt; j++) dst[j] = L[j * kBeamBlock];
    }
    nout[u] = off ? kBeamOff : (at << 8) | nl;
    cout[u] = px.in_image ? cut : kMiss;
}

template <bool LIGHTS>
__global__ __launch_bounds__(kBlock) void k_inw_probe(Frame f, InwScene S, uint32_t stride, uint32_t *mode) {
    __shared__ float lds[kFStack * kBlock];
    Ctr c;  // not flushed: the probe's rays are not the frame's
    FStack K{lds + threadIdx.x, 0};
    const uint32_t lane = threadIdx.x & 63u, nblk = units_total(f) / 64u;
    const uint32_t blk = ((blockIdx.x * kBlock + threadIdx.x) >> 6) * stride;
    if (blk >= nblk) return;  // whole waves (blk is per wave)
    const UnitPix px = unit_pixel(f, blk * 64u + lane);
    int id = -2;  // -2: outside the image, -1: no hit, else the object
    if (px.in_image) {
        const int s = f.spp / 2;
        inw_start_sample(S, f, K, px.x, px.y, s, c);
        K.size -= 8;
        const uint32_t b = K.size;
        const f3 o = mk(K.at(b), K.at(b + 1), K.at(b + 2)), d = mk(K.at(b + 3), K.at(b + 4), K.at(b + 5));
        const f3 D = mk(f.dir[0], f.dir[1], f.dir[2]);
        float tlim = kMaxT, extra = 0.0f;
        f3 nrm;
        const float g = inw_closest<false>(S, K, o, d, (float)s * f.inv_spp, dot(D, f3{1, 1, 1}) > 0.0f, tlim, nrm,
                                           extra, -1.0f, c);
        id = tlim < kMaxT ? (int)g : -1;
    }
    const int id0 = __shfl(id, __ffsll((long long)__ballot(id != -2)) - 1, 64);
    const bool any_hit = __ballot(id >= 0) != 0ull, same = __ballot(id != -2 && id != id0) == 0ull;
    if (lane == 0 && any_hit) {
        atomicAdd(mode, 1u);
        if (same) atomicAdd(mode + 1, 1u);
    }
}

// Sky blocks (DESIGN.md §5.1 "Sky blocks"; rt_options.inw_sky_blocks).  An 8x8 block whose 64 units
// have an empty and complete beam list in every time bin (count 0, cut kMiss, not kBeamOff) holds
// no pixel whose primary rays can reach a culling box: inw_closest_beam answers "no hit" for every
// such ray that passes its `ok` test, and the sample is the miss branch of inw_segment.  k_inw_sky
// renders those blocks without stacks, walk or ring; the claim-order kernels put them first and
// k_inw_pm's queues start past them.  A block with a ray that fails the test is left to k_inw_pm (its flag cleared).
// Bookkeeping: kSkyInfo uints after the claim order's 256 buckets.
enum { kSkySkip = 0,     // blocks at the head of the claim order that k_inw_pm skips (k_inw_order_scan)
       kSkyFlagged = 1,  // blocks the classifier flagged
       kSkyDone = 2,     // ... of them, those k_inw_sky rendered
       kSkyHead = 3,     // k_inw_order_scatter: cursor of the sky blocks at the head of the order
       kSkyInfo = 16 };
// one wave per 8x8 block; on a sample-major frame every flag is cleared
__global__ __launch_bounds__(kBlock) void k_inw_sky_classify(Frame f, InwScene S, uint32_t *flag, uint32_t *info,
                                                             const uint32_t *mode, uint32_t force) {
    const uint32_t lane = threadIdx.x & 63u, nblk = units_total(f) / 64u;
    const uint32_t blk = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (blk >= nblk) return;  // whole waves
    bool empty = !inw_sample_major(mode, force);
    const uint32_t nb = S.beam_bins > 1u ? S.beam_bins : 1u, u = blk * 64u + lane;
    for (uint32_t b = 0; b < nb && empty; b++) {  // padding units have empty lists too (k_inw_beam)
        const uint32_t nw = S.beam_n[b * S.beam_units + u];
        empty = nw != kBeamOff && (nw & 0xffu) == 0u && S.beam_cut[b * S.beam_units + u] == kMiss;
    }
    const bool sky = __ballot(!empty) == 0ull;
    if (lane == 0) {
        flag[blk] = sky ? 1u : 0u;
        if (sky) atomicAdd(info + kSkyFlagged, 1u);
    }
}
// One 512-lane block per flagged 8x8 block, a wave per row of 8 pixels.  A pass takes 8 samples of
// each pixel (lane = sample * 8 + pixel): the camera ray, the `ok` test, background(cd) and the
// three square roots, staged in LDS; then lane (channel * 8 + pixel) adds its pixel's 8 values in
// sample order -- End()'s sum, one chain per pixel and channel, 24 chains abreast.
// The test is inw_closest_beam's `ok` for a fresh sample, from below: a direction component of
// magnitude >= 2^-100 is non-zero with a finite correctly rounded reciprocal, so no reciprocal is
// computed (a smaller or NaN component sends the block to k_inw_pm, which is always exact).
constexpr int kSkyBlock = 512, kSkyPlane = 72;  // a channel's 64 staged values, padded: the three planes on distinct banks
__global__ __launch_bounds__(kSkyBlock) __attribute__((amdgpu_waves_per_eu(8))) void k_inw_sky(Frame f, InwScene S, uint32_t *flag, uint32_t *info) {
    const uint32_t blk = blockIdx.x;
    if (!uni(flag[blk])) return;  // the whole block
    __shared__ float s_sq[(kSkyBlock / 64) * 3 * kSkyPlane];
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, row = threadIdx.x >> 6, p = lane & 7u, k = lane >> 3;
    float *sq = s_sq + row * (3 * kSkyPlane);
    const UnitPix px = unit_pixel(f, blk * 64u + row * 8u + p);
    const f3 pcd = px.in_image ? inw_pixel_dir(f, px.x, px.y) : f3{0, 0, 0};
    // the fold's lanes: pixel fp of the row, channel fc
    const uint32_t fp = lane & 7u, fc = lane >> 3;
    const bool folds = fc < 3u && __shfl((int)px.in_image, (int)fp, 64) != 0;
    const uint32_t spp = (uint32_t)f.spp;
    float acc = 0.0f;
    bool bad = false;
    for (uint32_t s0 = 0; s0 < spp; s0 += 8u) {
        const uint32_t s = s0 + k;
        if (px.in_image && s < spp) {
            f3 o, d;
            inw_camera_ray(S, f, pcd, (int)s, o, d);
            bad = bad || !(__builtin_fabsf(d.x) >= 0x1p-100f && __builtin_fabsf(d.y) >= 0x1p-100f &&
                           __builtin_fabsf(d.z) >= 0x1p-100f);
            const f3 col = f3{0, 0, 0} + background(d, false) * 1.0f;  // inw_segment's miss branch
            sq[lane] = __builtin_sqrtf(col.x);
            sq[kSkyPlane + lane] = __builtin_sqrtf(col.y);
            sq[2 * kSkyPlane + lane] = __builtin_sqrtf(col.z);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (folds) {
            const uint32_t n = spp - s0 < 8u ? spp - s0 : 8u;
            const float *v = sq + fc * kSkyPlane + fp;
            uint32_t j = 0;
            if (s0 == 0) { acc = v[0]; j = 1; }
            if (n == 8u) {
                float a[8];
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++) a[q] = v[q * 8u];
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++)
                    if (q >= j) acc = acc + a[q];
            } else {
                for (; j < n; j++) acc = acc + v[j * 8u];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(&s_bad, 1u);
    __syncthreads();
    if (s_bad) {  // some ray fails the test: nothing written, k_inw_pm renders the block
        if (threadIdx.x == 0) flag[blk] = 0u;
        return;
    }
    // the row's stores: 8 lanes, 128 B of colour and 32 B of depth (End()'s imageStores, 01_BVH...glsl:652, 667-668)
    const float inv = rcp((float)f.spp);
    const float ax = __shfl(acc, (int)p, 64), ay = __shfl(acc, (int)(8u + p), 64), az = __shfl(acc, (int)(16u + p), 64);
    if (k == 0 && px.out != (size_t)-1) {
        fb_store(f, px.out, make_float4(px.in_image ? ax * inv : 0.0f, px.in_image ? ay * inv : 0.0f,
                                        px.in_image ? az * inv : 0.0f, px.in_image ? 1.0f : 0.0f));
        if (f.out_depth) depth_store(f, px.out, px.in_image ? kMaxT : 0.0f);  // the middle sample's depth: a miss
    }
    // one segment per sample; no node, test, shadow ray, drop or NaN
    const unsigned long long rays = (unsigned long long)__popcll(__ballot(k == 0 && px.in_image)) * spp;
    if (lane == 0 && rays && f.counters) atomicAdd(f.counters, rays);
    if (threadIdx.x == 0) atomicAdd(info + kSkyDone, 1u);
}

// Claim order (DESIGN.md §5 "Claim order"): a persistent fold kernel's tail is the last pixels
// it claims -- a wave needs spp / 64 rounds of samples for one pixel, so expensive pixels claimed
// last leave the rest of the chip idle.  k_inw_cost estimates each pixel's cost from the primary
// rays of two of its samples, the costlier (a miss or a diffuse hit ends the sample; a reflective /
// refractive hit starts a chain of about log(0.01) / log(coefficient) segments, two-sided for
// refraction), keys each 8x8 block by its costliest pixel and buckets it (256 log-scale keys);
// k_inw_order_scan / k_inw_order_scatter lay
// the blocks out costliest first, and k_inw_pm claims through that order.  The order only decides
// which wave traces which pixel when: every pixel's samples and sums are the same.  Pixel-major
// frames only: the three kernels exit at once when the probe picked k_inw_sm, whose 8x8 blocks
// keep their spatial order (measured: C5 3% slower with it, the blocks' locality lost).
// flag (null: none): the sky blocks k_inw_sky rendered (below); they get no bucket, key kSkyKey
constexpr uint32_t kSkyKey = 0xffffffffu;
template <bool LIGHTS>
__global__ __launch_bounds__(kBlock) void k_inw_cost(Frame f, InwScene S, uint32_t *key, uint32_t *hist,
                                                     const uint32_t *mode, uint32_t force, const uint32_t *flag) {
    if (inw_sample_major(mode, force)) return;
    __shared__ float lds[kFStack * kBlock];
    Ctr c;  // not flushed: these rays are not the frame's
    FStack K{lds + threadIdx.x, 0};
    // every pixel of the block (a wave per block), two samples each; the block's key is its
    // costliest pixel's, so the blocks claimed last hold no expensive pixel
    const uint32_t lane = threadIdx.x & 63u, nblk = units_total(f) / 64u, p = lane;
    const uint32_t blk = ((blockIdx.x * kBlock + threadIdx.x) >> 6);
    float est = 0.0f;
    if (blk < nblk && flag && uni(flag[blk])) {  // (wave-uniform: blk is per wave)
        if (p == 0) key[blk] = kSkyKey;
        return;
    }
    if (blk < nblk) {
        const UnitPix px = unit_pixel(f, blk * 64u + p);
        for (int si = 0; si < 2 && px.in_image; si++) {
            const int s = si == 0 ? f.spp / 2 : f.spp / 4;
            K.size = 0;
            inw_start_sample(S, f, K, px.x, px.y, s, c);
            K.size -= 8;
            const uint32_t b = K.size;
            const f3 o = mk(K.at(b), K.at(b + 1), K.at(b + 2)), d = mk(K.at(b + 3), K.at(b + 4), K.at(b + 5));
            const f3 D = mk(f.dir[0], f.dir[1], f.dir[2]);
            float tlim = kMaxT, extra = 0.0f;
            f3 nrm;
            const float g = inw_closest<false>(S, K, o, d, (float)s * f.inv_spp, dot(D, f3{1, 1, 1}) > 0.0f, tlim,
                                               nrm, extra, -1.0f, c);
            float e1 = 1.0f;
            if (tlim < kMaxT) {
                const float4 m0 = S.cold[2 * (int)g];
                const float m = fminf(fmaxf(m0.x, m0.y), 0.99f);
                if (LIGHTS) e1 += (float)S.n_lights;
                if (m > 0.002f) {
                    const float n = fminf((float)f.max_bounces, 1.0f + __logf(0.01f) / __logf(m));
                    e1 += n * (m0.x > 0.002f ? 2.0f : 1.0f) * (LIGHTS ? 1.0f + (float)S.n_lights : 1.0f);
                }
            }
            est = fmaxf(est, e1);
        }
    }
    for (int o = 32; o >= 1; o >>= 1) est = fmaxf(est, __shfl_xor(est, o, 64));
    est *= 16.0f;  // the scale of the 16-pixel sums this key replaced
    if (p == 0 && blk < nblk) {
        const uint32_t k = (uint32_t)fminf(255.0f, 16.0f * __log2f(1.0f + est));
        key[blk] = k;
        atomicAdd(hist + (255u - k), 1u);
    }
}
// exclusive scan of the 256 bucket counts (one 256-lane block).  The blocks without a bucket -- the
// sky blocks, nblk less the buckets' sum -- lead the order, so the buckets' offsets start past them;
// hist[256 + kSkySkip] = their count
__global__ __launch_bounds__(256) void k_inw_order_scan(uint32_t *hist, uint32_t nblk, const uint32_t *mode, uint32_t force) {
    if (inw_sample_major(mode, force)) return;
    __shared__ uint32_t t[256];
    const uint32_t i = threadIdx.x;
    const uint32_t v = hist[i];
    t[i] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 256u; o <<= 1) {
        const uint32_t a = i >= o ? t[i - o] : 0u;
        __syncthreads();
        t[i] += a;
        __syncthreads();
    }
    const uint32_t skip = nblk - t[255];
    hist[i] = skip + t[i] - v;
    if (i == 0u) hist[256u + kSkySkip] = skip;
}
__global__ __launch_bounds__(kBlock) void k_inw_order_scatter(const uint32_t *key, uint32_t *off, uint32_t *order,
                                                               uint32_t nblk, const uint32_t *mode, uint32_t force) {
    if (inw_sample_major(mode, force)) return;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nblk) return;
    const uint32_t k = key[i];
    order[atomicAdd(k == kSkyKey ? off + 256u + kSkyHead : off + (255u - k), 1u)] = i;
}
// k_inw_pm claims through the order from its queues' counters on: they start past the sky blocks
// (counter[0]: the one queue, in units; counter[64 + 16 x]: queue x of the per-XCD queues, which
// holds the claim ordinals congruent to x mod 8), so k_inw_pm itself knows nothing of them
__global__ __launch_bounds__(64) void k_inw_sky_queues(const uint32_t *info, unsigned *counter) {
    const uint32_t x = threadIdx.x, skip = info[kSkySkip];
    if (x == 0u) counter[0] = skip * 64u;
    if (x < 8u) counter[64u + 16u * x] = skip > x ? ((skip - x + 7u) >> 3) * 64u : 0u;
}

// pixel-major stream (see above): entry g = (claimed pixel ordinal j, sample s).  LN: 768-lane
// blocks (3 waves per SIMD) that stage the top of the wide BVH in the LDS their three 256-lane
// stacks leave free (kInwLdsNodes nodes)
// GQ (DESIGN.md §5.1 "GQ"; LN, FU, LRING and INW-01 only): the reference's 40-float stacks in
// global memory (GStack, S.gstk), the wide walks' node stacks in LDS (kWStack entries per lane), the
// closest-hit walks over the quantised nodes, the top kQLdsNodes of them staged in LDS
// k_inw_pm's LDS fold ring: channel c of entry e.  Planes (r, g, b of 256 entries each): the fold's
// lanes 0, 1, 2 read one plane each at the same entry, addresses 1 KB apart, one bank: a 3-way
// conflict per read.  Interleaving the channels (3 e + c) spreads them over 3 banks, but C3 ran 0.5%
// slower (DESIGN_HISTORY.md §J).
#define RIX(c, e) ((c) * kPmLdsRing + (e))
template <bool LN, bool GQ>
constexpr int pm_sub() { return GQ ? kGqSub : (LN ? 3 : 1); }
template <bool LIGHTS, bool LN = false, bool FU = false, bool LRING = false, bool GQ = false>
__global__ __launch_bounds__((pm_sub<LN, GQ>() * kBlock)) __attribute__((amdgpu_waves_per_eu((LN ? pm_sub<LN, GQ>() : (LIGHTS ? kInwWaves : kInw01Waves))))) void k_inw_pm(Frame f, InwScene S0, float4 *ring, uint32_t rmask, unsigned *counter, const uint32_t *mode, uint32_t force, const uint32_t *border) {
    static_assert(!GQ || (LN && FU && LRING && !LIGHTS), "GQ: the C3 instance only");
    if (inw_sample_major(mode, force)) return;  // the probe picked k_inw_sm for this frame
    constexpr int SUB = pm_sub<LN, GQ>();
    // FStack instances: the three 256-lane 40-float stacks; GQ: the wide walks' node stacks (the
    // 40-float stacks are global), the LDS that frees holding the top of the quantised culling BVH
    __shared__ float lds[SUB * (GQ ? kWStack : kFStack) * kBlock];
    // per wave: the middle sample's depth of claimed ordinal j (slot j % 64; at most 64 ordinals lie
    // between the fold and the issue), written out with the pixel's colour
    __shared__ float s_pdep[SUB * kBlock];
    InwScene S = S0;
    // LRING: the fold ring in LDS, after the first kPmLdsNodes staged nodes (InwScene::lring; an
    // instance of its own: as a per-frame branch it cost 1% of C3 in either mode)
    constexpr bool LR = LN && LRING;
    // WLN: the walks read staged nodes.  The LDS-ring instances stage none: the top 5 nodes the
    // ring leaves room for sit in L1 anyway, and the walk loop without the LDS branch (its exec
    // masking and the base pointer kept in a VGPR lane) ran C3 2% faster.  GQ
    // stages kQLdsNodes quantised nodes beside its ring
    constexpr bool WLN = LN && (!LR || GQ);
    float *lr;  // LR: this wave's ring, three planes (r, g, b) of kPmLdsRing floats
    if constexpr (GQ) {
        __shared__ float s_ring[SUB * kBlock / 64 * 3 * kPmLdsRing];
        lr = s_ring + uni((threadIdx.x >> 6) * (3u * kPmLdsRing));
        const uint32_t n = S.qnodes ? (S.n_wnodes < (uint32_t)kQLdsNodes ? S.n_wnodes : (uint32_t)kQLdsNodes) : 0u;
        for (uint32_t i = threadIdx.x; i < n * (uint32_t)kQNodeF4; i += SUB * kBlock) g_inw_qlds[i] = S.qnodes[i];
        __syncthreads();
        S.n_lnodes = n;
    } else {
        lr = reinterpret_cast<float *>(g_inw_lnodes + kPmLdsNodes * kInwNodeF4) + uni((threadIdx.x >> 6) * (3u * kPmLdsRing));
        if constexpr (WLN) {
            const uint32_t cap = (uint32_t)kInwLdsNodes;
            const uint32_t n = S.wnodes ? (S.n_wnodes < cap ? S.n_wnodes : cap) : 0u;
            for (uint32_t i = threadIdx.x; i < n * (uint32_t)kInwNodeF4; i += SUB * kBlock) g_inw_lnodes[i] = S.wnodes[i];
            // no wide walk: the stackless LBVH walks read the top of the LBVH (2 float4 per node) there
            const uint32_t nb = (!S.wnodes && S.sl) ? min(2u * S.n - 1u, cap * (uint32_t)kInwNodeF4 / 2u) : 0u;
            for (uint32_t i = threadIdx.x; i < 2u * nb; i += SUB * kBlock) g_inw_lnodes[i] = S.nodes[i];
            __syncthreads();
            S.n_lnodes = n;
            S.n_blds = nb;
        }
    }
    Ctr c;
#ifdef RT_DIAG_SPLIT
    const unsigned long long t_start = wall_clock64();  // the tail split (tools/inw_split.py)
    unsigned long long t_qd = 0;
#endif
    using KS = std::conditional_t<GQ, GStack, FStack>;
    KS K;
    if constexpr (GQ) {
        K.col = S.gstk + ((size_t)blockIdx.x * (SUB * kBlock) + threadIdx.x);
        K.stride = gridDim.x * (SUB * kBlock);
        K.ws = lds + (threadIdx.x / kBlock) * (kWStack * kBlock) + (threadIdx.x % kBlock);
        K.rc = false;
    } else {
        K.base = lds + (threadIdx.x / kBlock) * (kFStack * kBlock) + (threadIdx.x % kBlock);
    }
    K.size = 0;
    const uint32_t lane = threadIdx.x & 63u;
    if constexpr (LR) rmask = kPmLdsRing - 1u;
    const uint32_t rsize = rmask + 1u;
    float4 *wr = ring + (size_t)uni((blockIdx.x * (SUB * kBlock) + threadIdx.x) >> 6) * rsize;
    float *pdep = s_pdep + (threadIdx.x & ~63u);
    const uint32_t spp = (uint32_t)f.spp, mid = spp / 2u, total = units_total(f);
    const float inv = rcp((float)f.spp);
    // wave-uniform: stream positions (entry gi / fold gf) as (pixel ordinal, sample), claims
    uint32_t gi = 0, ji = 0, si = 0;   // next entry to issue: pixel ordinal ji, sample si
    uint32_t gf = 0, jf = 0, sf = 0;   // next entry to fold
    uint32_t nclaimed = 0;             // pixel ordinals claimed so far
    bool qdone = false;
    uint32_t xq = 0;                   // S.xcdq: queues found empty (from this block's XCD on)
    const uint32_t nblk8 = total / 64u;  // 8x8 blocks (units come in whole blocks)
    f3 acc = f3{0, 0, 0};              // running End() sum of pixel jf (the same in every lane)
    float accc = 0.0f;                 // LR: lane c < 3 holds channel c of that sum
    uint32_t pix_slot = 0xffffffffu;   // lane l: the unit of the claimed ordinal j with j % 64 == l
    // per lane: the sample it traces
    bool busy = false;
    uint32_t g = 0, pj = 0;  // the lane's stream entry and its pixel's ordinal slot (j % 64)
    int s = 0;
    UnitPix px{};
    uint32_t bu = kBeamOff;  // the lane's pixel unit for its beam list (S.beam)
    uint32_t pu = 0xffffffffu;  // the unit px and pcd belong to: a lane's next sample is mostly the same pixel's
    f3 pcd = f3{0, 0, 0};
    f3 col = f3{0, 0, 0};
    float dep = 0.0f;
    K.size = 0;
    for (;;) {
        // ---- fold the finished entries gf, gf+1, ... (stored in earlier iterations)
        INW_T0(t_fold);
        if (gf != gi) {
            const uint32_t k = gf + lane;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uint32_t n;
            bool continue_fold = true;  // (the LDS-ring fold below finishes the run itself)
            if constexpr (LR) {
                // Every issued entry is either held by a busy lane or stored, so the entries below
                // the smallest one a busy lane holds are finished: no tags.  LDS ops of one wave
                // complete in order, so the stores of earlier iterations are visible.
                n = uni(__ockl_wfred_min_u32(busy ? g - gf : 0xffffffffu));  // DPP reduction
                if (n > gi - gf) n = gi - gf;
                if (n > 64u) n = 64u;
                if (lane < n) {
                    const uint32_t e = k & rmask;
                    v = make_float4(lr[RIX(0u, e)], lr[RIX(1u, e)], lr[RIX(2u, e)], 0.0f);
                }
            } else {
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's ring stores have landed (same CU: L1 write-through)
                bool fin = false;
                if (k - gf < gi - gf) {
                    v = wr[k & rmask];
                    fin = __float_as_uint(v.w) == ring_tag(S, k);
                }
                const unsigned long long m = __ballot(fin);
                n = ~m == 0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
            }
            if constexpr (LR) {
                // LDS ring: lanes 0, 1, 2 add the r, g, b planes' entries straight from LDS, each
                // its channel in sample order (the same float additions, two instructions per entry
                // instead of three readlanes and three adds); the run splits at pixel ends
                const uint32_t lc = lane < 3u ? lane : 0u;  // this lane's channel
                for (uint32_t i = 0; i < n;) {
                    const uint32_t e = i + (n - i < spp - sf ? n - i : spp - sf);
                    if (lane < 3u) {
                        uint32_t j = i;
                        if (sf == 0) { accc = lr[RIX(lc, (gf + j) & rmask)]; j++; }
                        constexpr uint32_t kFU = 4;  // loads in flight, then the adds in order (8, 16: same time)
                        for (; j + kFU <= e; j += kFU) {
                            float a[kFU];
#pragma unroll
                            for (uint32_t u = 0; u < kFU; u++) a[u] = lr[RIX(lc, (gf + j + u) & rmask)];
#pragma unroll
                            for (uint32_t u = 0; u < kFU; u++) accc = accc + a[u];
                        }
                        for (; j < e; j++) accc = accc + lr[RIX(lc, (gf + j) & rmask)];
                    }
                    sf += e - i;
                    i = e;
                    if (sf == spp) {  // pixel jf complete: End()'s imageStores (01_BVH...glsl:652, 667-668)
                        const uint32_t unit = uni((uint32_t)__builtin_amdgcn_readlane((int)pix_slot, (int)(jf & 63u)));
                        const float ax = rdl(accc, 0u), ay = rdl(accc, 1u), az = rdl(accc, 2u);
                        if (lane == 0) {
                            const UnitPix p = unit_pixel(f, unit);
                            if (p.out != (size_t)-1) {
                                fb_store(f, p.out,
                                         make_float4(p.in_image ? ax * inv : 0.0f, p.in_image ? ay * inv : 0.0f,
                                                     p.in_image ? az * inv : 0.0f, p.in_image ? 1.0f : 0.0f));
                                if (f.out_depth) depth_store(f, p.out, pdep[jf & 63u]);
                            }
                        }
                        sf = 0;
                        jf++;
                    }
                }
                gf += n;
                continue_fold = false;
            }
            // the run splits at pixel ends: per pixel, its entries are added with no test between them
            for (uint32_t i = 0; continue_fold && i < n;) {
                const uint32_t e = i + (n - i < spp - sf ? n - i : spp - sf);
                uint32_t j = i;
                if (sf == 0) { acc = f3{rdl(v.x, j), rdl(v.y, j), rdl(v.z, j)}; j++; }
                for (; j + 4u <= e; j += 4u) {  // four adds in order, one loop test
                    acc = acc + f3{rdl(v.x, j), rdl(v.y, j), rdl(v.z, j)};
                    acc = acc + f3{rdl(v.x, j + 1u), rdl(v.y, j + 1u), rdl(v.z, j + 1u)};
                    acc = acc + f3{rdl(v.x, j + 2u), rdl(v.y, j + 2u), rdl(v.z, j + 2u)};
                    acc = acc + f3{rdl(v.x, j + 3u), rdl(v.y, j + 3u), rdl(v.z, j + 3u)};
                }
                for (; j < e; j++) acc = acc + f3{rdl(v.x, j), rdl(v.y, j), rdl(v.z, j)};
                sf += e - i;
                i = e;
                if (sf == spp) {  // pixel jf complete: End()'s imageStores (01_BVH...glsl:652, 667-668)
                    const uint32_t unit = uni((uint32_t)__builtin_amdgcn_readlane((int)pix_slot, (int)(jf & 63u)));
                    if (lane == 0) {
                        const UnitPix p = unit_pixel(f, unit);
                        if (p.out != (size_t)-1) {
                            fb_store(f, p.out,
                                     make_float4(p.in_image ? acc.x * inv : 0.0f, p.in_image ? acc.y * inv : 0.0f,
                                                 p.in_image ? acc.z * inv : 0.0f, p.in_image ? 1.0f : 0.0f));
                            if (f.out_depth) depth_store(f, p.out, pdep[jf & 63u]);
                        }
                    }
                    sf = 0;
                    jf++;
                }
            }
            if (continue_fold) gf += n;
        }
        INW_CYC(c, 2, t_fold);
        INW_T0(t_issue);
        // ---- claim pixels for the free lanes (at most 64 pixels between fold and issue)
        const unsigned long long fm = __ballot(!busy);
        const uint32_t nfree = (uint32_t)__popcll(fm);
        if (!qdone && nfree) {
            // ordinals the free lanes would reach: ji + (si + nfree - 1) / spp, capped at jf + 63
            uint32_t need = ji + (si + nfree - 1u) / spp + 1u;
            if (need > jf + 64u) need = jf + 64u;
            if (need > nclaimed) {
                const uint32_t want = need - nclaimed;
                uint32_t base = 0, got = 0, qx = 0;
                if (S.xcdq) {
                    // per-XCD queues (rt_options.inw_claim_xcd): queue x holds the blocks of claim
                    // ordinal b = x mod 8, in claim order, so a block's pixels -- whole 128-B lines of
                    // the framebuffer per block row -- are written through one XCD's L2 (workgroups go
                    // to the XCDs round robin); a wave whose queue is empty takes from the next ones
                    while (xq < 8u) {  // wave-uniform
                        qx = (blockIdx.x + xq) & 7u;
                        const uint32_t nb = nblk8 > qx ? (nblk8 - qx + 7u) >> 3 : 0u, qt = nb * 64u;
                        if (lane == 0) base = atomicAdd(counter + 64u + 16u * qx, want);
                        base = uni((uint32_t)__shfl((int)base, 0, 64));
                        if (base < qt) {
                            got = min(want, qt - base);
                            if (base + want >= qt) xq++;
                            break;
                        }
                        xq++;
                    }
                    if (xq >= 8u) qdone = true;
                } else {
                    if (lane == 0) base = atomicAdd(counter, want);
                    base = uni((uint32_t)__shfl((int)base, 0, 64));
                    got = want;
                    if (base >= total) { got = 0; qdone = true; }
                    else if (base + want >= total) { got = total - base; qdone = true; }
                }
#ifdef RT_DIAG_SPLIT
                if (qdone && t_qd == 0) t_qd = wall_clock64();
#endif
                const uint32_t rel = (lane - nclaimed) & 63u;
                if (rel < got) {  // ordinal -> unit through the claim order (block-wise)
                    uint32_t u = base + rel;
                    if (S.xcdq) u = (((u >> 6) << 3) + qx) * 64u + (u & 63u);  // queue ordinal -> claim ordinal
                    pix_slot = border ? border[u >> 6] * 64u + (u & 63u) : u;
                }
                nclaimed += got;
            }
        }
        // ---- issue: free lanes take stream entries in lane order, within the window
        {
            const uint32_t rank = (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
            uint32_t avail = rsize - (gi - gf);
            const uint64_t left = (uint64_t)(nclaimed - ji) * spp - si;  // entries of claimed pixels not issued
            if ((uint64_t)avail > left) avail = (uint32_t)left;
            const uint32_t take = nfree < avail ? nfree : avail;
            if (take) {
                // this lane's entry: pixel ji + adv / spp, sample adv % spp (adv < spp + 64: one
                // subtraction when spp >= 64)
                const uint32_t adv = si + rank;
                const uint32_t q = spp >= 64u ? (adv >= spp ? 1u : 0u) : adv / spp;
                const uint32_t jl = ji + q;
                const uint32_t unit = (uint32_t)__shfl((int)pix_slot, (int)(jl & 63u), 64);
                if (!busy && rank < take) {
                    g = gi + rank;
                    pj = jl & 63u;
                    s = (int)(adv - q * spp);
                    if (unit != pu) {
                        pu = unit;
                        px = unit_pixel(f, unit);
                        if (px.in_image) pcd = inw_pixel_dir(f, px.x, px.y);
                    }
                    bu = S.beam ? unit : kBeamOff;
                    col = f3{0, 0, 0};
                    dep = 0.0f;
                    if (px.in_image) {
                        busy = true;
                        inw_start_sample_cd(S, f, K, pcd, s, c);
                    } else {  // a padding slot: an empty sample, folded as zero
                        if ((uint32_t)s == mid) pdep[pj] = 0.0f;
                        if constexpr (LR) {
                            const uint32_t e = g & rmask;
                            lr[RIX(0u, e)] = 0.0f; lr[RIX(1u, e)] = 0.0f; lr[RIX(2u, e)] = 0.0f;
                        } else {
                            wr[g & rmask] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ring_tag(S, g)));
                        }
                    }
                }
                gi += take;
                const uint32_t a2 = si + take;
                ji += a2 / spp;
                si = a2 % spp;
            }
        }
        INW_CYC(c, 3, t_issue);
        if (qdone && ji == nclaimed && gf == gi && __ballot(busy) == 0) break;
        // ---- one ray segment per busy lane (samples are independent invocations)
        INW_T0(t_seg);
        OCC_TALLY(c, kOccSeg, busy);
        // Two rounds per iteration (DESIGN.md §5 "Primary and bounce rounds"): primary rays take
        // the beam lists, bounce rays the wide walk, two code paths a wave runs one after the other
        // (one walk trip then carries only the lanes with a bounce ray).  Round 0 runs the lanes
        // whose next ray is a primary one; round 1 every lane with a ray left, the bounce rays those
        // primaries just pushed included, so the walk runs with the bounce rays of the whole wave.
        // INW-04 (LIGHTS) keeps one round: with its shadow walks the two-round loop spills 17 VGPRs
        constexpr int kRounds = LIGHTS ? 1 : 2;
#pragma unroll 1
        for (int round = 2 - kRounds; round < 2; round++) {
            const bool prim = bu != kBeamOff && K.top_primary();
            const bool go = busy && (round == 0 ? prim : K.size > 0u);
            INW_T0(t_rnd);
            if (go) {
                if (f.px_rays) atomicAdd(f.px_rays + px.out, 1u);  // rt_debug_pixel_rays (diagnostics only)
                inw_segment<LIGHTS, WLN, FU, GQ>(S, f, K, s, col, dep, c, bu);
            }
#ifdef RT_DIAG_SPLIT
            c.rnd[round] += (unsigned long long)clock64() - t_rnd;
#endif
            if (busy && K.size == 0) {  // sample done: its sqrt(colour) (01_BVH...glsl:670) to the ring
                if constexpr (LR) {
                    const uint32_t e = g & rmask;
                    lr[RIX(0u, e)] = __builtin_sqrtf(col.x);
                    lr[RIX(1u, e)] = __builtin_sqrtf(col.y);
                    lr[RIX(2u, e)] = __builtin_sqrtf(col.z);
                } else {
                    wr[g & rmask] = make_float4(__builtin_sqrtf(col.x), __builtin_sqrtf(col.y), __builtin_sqrtf(col.z),
                                                __uint_as_float(ring_tag(S, g)));
                }
                if ((uint32_t)s == mid) pdep[pj] = dep;  // 01_BVH...glsl:667-668, stored with the pixel's colour
                busy = false;
            }
        }
        INW_CYC(c, 4, t_seg);
    }
#ifdef RT_DIAG_SPLIT
    // phases 0-1 and 5-7 run inside `if (busy)`: the wave's time there is the largest of its lanes'
    for (int k = 0; k < 8; k++) {
        if (k >= 2 && k < 5) continue;
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long t = __shfl_xor(c.cyc[k], o, 64);
            c.cyc[k] = t > c.cyc[k] ? t : c.cyc[k];
        }
    }
    if (f.dbg && lane == 0) {
        for (int k = 0; k < 8; k++) atomicAdd(f.dbg + 8 + k, c.cyc[k]);
        atomicAdd(f.dbg + 24, c.rnd[0]);
        atomicAdd(f.dbg + 25, c.rnd[1]);
        // wall clock (100 MHz): first / last wave start, first queue drain, first / last wave exit
        const unsigned long long t_end = wall_clock64();
        unsigned long long *t = reinterpret_cast<unsigned long long *>(f.dbg) + 16;
        atomicMin(t, t_start); atomicMax(t + 1, t_start);
        if (t_qd) atomicMin(t + 2, t_qd);
        atomicMin(t + 3, t_end); atomicMax(t + 4, t_end);
    }
#endif
#ifdef RT_DIAG_OCC
    if (f.dbg && lane == 0)
        for (int k = 0; k < kOccSlots; k++) atomicAdd(f.dbg + 32 + k, c.occ[k]);
#endif
    flush(f, c);
}

// sample-major stream (see above): entry g = block ordinal b, sample s, pixel p (b * 64 * spp + s * 64 + p)
// LRING: the fold ring in LDS after the first kPmLdsNodes staged nodes, as k_inw_pm's (InwScene::
// lring_sm: chosen when the scene's BVH top fits those nodes, so the staging loses nothing)
template <bool LIGHTS, bool LN = false, bool FU = false, bool LRING = false>
__global__ __launch_bounds__(LN ? 3 * kBlock : kBlock) __attribute__((amdgpu_waves_per_eu(LN ? 3 : (LIGHTS ? kInwWaves : kInw01Waves)))) void k_inw_sm(Frame f, InwScene S0, float4 *ring, uint32_t rmask, unsigned *counter, const uint32_t *mode, uint32_t force, const uint32_t *) {
    if (!inw_sample_major(mode, force)) return;  // the probe picked k_inw_pm for this frame
    constexpr int SUB = LN ? 3 : 1;
    constexpr bool LR = LN && LRING;
    __shared__ float lds[SUB * kFStack * kBlock];
    InwScene S = S0;
    if constexpr (LN) {
        const uint32_t cap = LR ? (uint32_t)kPmLdsNodes : (uint32_t)kInwLdsNodes;
        const uint32_t n = S.wnodes ? (S.n_wnodes < cap ? S.n_wnodes : cap) : 0u;
        for (uint32_t i = threadIdx.x; i < n * (uint32_t)kInwNodeF4; i += SUB * kBlock) g_inw_lnodes[i] = S.wnodes[i];
        const uint32_t nb = (!S.wnodes && S.sl) ? min(2u * S.n - 1u, cap * (uint32_t)kInwNodeF4 / 2u) : 0u;
        for (uint32_t i = threadIdx.x; i < 2u * nb; i += SUB * kBlock) g_inw_lnodes[i] = S.nodes[i];
        __syncthreads();
        S.n_lnodes = n;
        S.n_blds = nb;
    }
    Ctr c;
    FStack K{lds + (threadIdx.x / kBlock) * (kFStack * kBlock) + (threadIdx.x % kBlock), 0};
    const uint32_t lane = threadIdx.x & 63u;
    if constexpr (LR) rmask = kPmLdsRing - 1u;
    const uint32_t rsize = rmask + 1u;
    float4 *wr = ring + (size_t)uni((blockIdx.x * (SUB * kBlock) + threadIdx.x) >> 6) * rsize;
    // LR: this wave's ring, three planes (r, g, b) of kPmLdsRing floats
    float *lr = reinterpret_cast<float *>(g_inw_lnodes + kPmLdsNodes * kInwNodeF4) + uni((threadIdx.x >> 6) * (3u * kPmLdsRing));
    const uint32_t spp = (uint32_t)f.spp, mid = spp / 2u, nblk = units_total(f) / 64u;
    const uint32_t E = 64u * spp;  // entries per block
    const float inv = rcp((float)f.spp);
    // wave-uniform issue state: next entry = offset ei of block ordinal bi; gi = bi * E + ei
    uint32_t gi = 0, bi = 0, ei = 0, nclaimed = 0;
    bool qdone = false;
    uint32_t blk_slot = 0xffffffffu;  // lane l: the block id of ordinal j with j % 64 == l
    // per-lane fold state: pixel `lane` of block ordinal bf, next sample sf
    uint32_t bf = 0, sf = 0;
    f3 acc = f3{0, 0, 0};
    // per-lane trace state
    bool busy = false;
    uint32_t g = 0;
    int s = 0;
    UnitPix px{};
    f3 col = f3{0, 0, 0};
    float dep = 0.0f;
    K.size = 0;
    for (;;) {
        // ---- fold: lane p adds the finished samples of its pixel, in order (up to 2 per iteration)
        {
            if constexpr (!LR) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's ring stores have landed (same CU: L1 write-through)
            // LR: every issued entry is either held by a busy lane or stored (LDS ops of one wave
            // complete in order), so the issued entries below the oldest one a busy lane holds are
            // finished: no tags (the window keeps every unfolded entry from being overwritten)
            uint32_t hold = 0u;
            if constexpr (LR) hold = uni(__ockl_wfred_min_u32(busy ? g - (gi - rsize) : 0xffffffffu));
            const uint32_t my_blk = (uint32_t)__shfl((int)blk_slot, (int)(bf & 63u), 64);
            if (bf != nclaimed) {
                uint32_t gg[2];
                float4 v[2];
                bool fin[2];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const uint32_t sk = sf + (uint32_t)k;
                    gg[k] = bf * E + (sk < spp ? sk : spp - 1u) * 64u + lane;
                    const uint32_t rel = gg[k] - (gi - rsize);
                    const bool ok = sk < spp && rel < rsize;  // issued (and inside the window)
                    if constexpr (LR) {
                        fin[k] = ok && rel < hold;
                        const uint32_t e = gg[k] & rmask;
                        v[k] = fin[k] ? make_float4(lr[e], lr[kPmLdsRing + e], lr[2u * kPmLdsRing + e], 0.0f)
                                      : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    } else {
                        v[k] = ok ? wr[gg[k] & rmask] : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(~ring_tag(S, gg[k])));
                        fin[k] = __float_as_uint(v[k].w) == ring_tag(S, gg[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (!fin[k] || sf == spp) break;
                    const f3 gv = f3{v[k].x, v[k].y, v[k].z};
                    acc = sf == 0 ? gv : acc + gv;
                    if (++sf == spp) {  // pixel complete: End()'s imageStore (01_BVH...glsl:652)
                        const UnitPix p = unit_pixel(f, my_blk * 64u + lane);
                        if (p.out != (size_t)-1)
                            fb_store(f, p.out,
                                     make_float4(p.in_image ? acc.x * inv : 0.0f, p.in_image ? acc.y * inv : 0.0f,
                                                 p.in_image ? acc.z * inv : 0.0f, p.in_image ? 1.0f : 0.0f));
                    }
                }
                if (sf == spp) { sf = 0; bf++; }
            }
        }
        // the ring window starts at the oldest unfolded entry of the wave (a lane whose next sample
        // is not issued yet holds nothing back)
        const uint32_t gnext = bf == nclaimed ? gi : bf * E + sf * 64u + lane;
        const int dl = (int)(gi - gnext);
        uint32_t dmax = dl > 0 ? (uint32_t)dl : 0u, bmin = bf;
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t t = (uint32_t)__shfl_xor((int)dmax, o, 64), tb = (uint32_t)__shfl_xor((int)bmin, o, 64);
            dmax = t > dmax ? t : dmax;
            bmin = tb < bmin ? tb : bmin;
        }
        dmax = uni(dmax);
        bmin = uni(bmin);
        // ---- claim blocks for the free lanes (at most 64 blocks between fold and issue)
        const unsigned long long fm = __ballot(!busy);
        const uint32_t nfree = (uint32_t)__popcll(fm);
        if (!qdone && nfree) {
            uint32_t need = bi + (ei + nfree - 1u) / E + 1u;
            if (need > bmin + 64u) need = bmin + 64u;
            if (need > nclaimed) {
                const uint32_t want = need - nclaimed;
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(counter, want);
                base = uni((uint32_t)__shfl((int)base, 0, 64));
                uint32_t got = want;
                if (base >= nblk) { got = 0; qdone = true; }
                else if (base + want >= nblk) { got = nblk - base; qdone = true; }
                const uint32_t rel = (lane - nclaimed) & 63u;
                if (rel < got) blk_slot = base + rel;
                nclaimed += got;
            }
        }
        // ---- issue: free lanes take the next stream entries in lane order, inside the window
        {
            const uint32_t rank = (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
            uint32_t avail = rsize - dmax;
            const uint64_t left = (uint64_t)(nclaimed - bi) * E - ei;
            if ((uint64_t)avail > left) avail = (uint32_t)left;
            const uint32_t take = nfree < avail ? nfree : avail;
            if (take) {
                uint32_t b = bi, e = ei + rank;
                if (e >= E) { e -= E; b++; }
                const uint32_t blk = (uint32_t)__shfl((int)blk_slot, (int)(b & 63u), 64);
                if (!busy && rank < take) {
                    g = gi + rank;
                    s = (int)(e >> 6);
                    px = unit_pixel(f, blk * 64u + (e & 63u));
                    col = f3{0, 0, 0};
                    dep = 0.0f;
                    if (px.in_image) {
                        busy = true;
                        inw_start_sample(S, f, K, px.x, px.y, s, c);
                    } else {  // a padding slot: an empty sample, folded as zero
                        if ((uint32_t)s == mid && f.out_depth && px.out != (size_t)-1) depth_store(f, px.out, 0.0f);
                        if constexpr (LR) {
                            const uint32_t e = g & rmask;
                            lr[e] = 0.0f; lr[kPmLdsRing + e] = 0.0f; lr[2u * kPmLdsRing + e] = 0.0f;
                        } else wr[g & rmask] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ring_tag(S, g)));
                    }
                }
                gi += take;
                ei += take;
                if (ei >= E) { ei -= E; bi++; }
            }
        }
        if (qdone && bi == nclaimed && bmin == nclaimed && __ballot(busy) == 0) break;
        OCC_TALLY(c, kOccSeg, busy);
        if (busy) {
            inw_segment<LIGHTS, LN, FU>(S, f, K, s, col, dep, c);
            if (f.px_rays) atomicAdd(f.px_rays + px.out, 1u);  // rt_debug_pixel_rays (diagnostics only)
        }
        if (busy && K.size == 0) {  // sample done: its sqrt(colour) (01_BVH...glsl:670) to the ring
            if constexpr (LR) {
                const uint32_t e = g & rmask;
                lr[e] = __builtin_sqrtf(col.x);
                lr[kPmLdsRing + e] = __builtin_sqrtf(col.y);
                lr[2u * kPmLdsRing + e] = __builtin_sqrtf(col.z);
            } else
                wr[g & rmask] = make_float4(__builtin_sqrtf(col.x), __builtin_sqrtf(col.y), __builtin_sqrtf(col.z),
                                            __uint_as_float(ring_tag(S, g)));
            if ((uint32_t)s == mid && f.out_depth) depth_store(f, px.out, dep);  // 01_BVH...glsl:667-668
            busy = false;
        }
    }
#ifdef RT_DIAG_OCC
    if (f.dbg && lane == 0)
        for (int k = 0; k < kOccSlots; k++) atomicAdd(f.dbg + 32 + k, c.occ[k]);
#endif
    flush(f, c);
}

// ============================================================================ launch
int inw_fold_blocks_per_cu(RenderKernel k) {
    switch (k) {
    case RenderKernel::InwPm04: return occupancy_of(k_inw_pm<true>, kBlock);
    case RenderKernel::InwPmLn01: return occupancy_of(k_inw_pm<false, true>, 3 * kBlock);
    case RenderKernel::InwPmLn04: return occupancy_of(k_inw_pm<true, true>, 3 * kBlock);
    case RenderKernel::InwPmGq:
        return occupancy_of(k_inw_pm<false, true, true, true, true>, pm_sub<true, true>() * kBlock);
    default: return occupancy_of(k_inw_pm<false>, kBlock);
    }
}
hipError_t launch_inw_beam(const Frame &f, const InwScene &sc, const BeamPrune &bp, const uint32_t *mode, uint32_t force,
                           hipStream_t s) {
    const uint32_t n = units_of(f);
    const uint32_t nb = sc.beam_bins > 1u ? sc.beam_bins : 1u;
    hipLaunchKernelGGL(k_inw_beam, dim3((n + kBeamBlock - 1) / kBeamBlock, nb), dim3(kBeamBlock), 0, s, f, sc, mode, force, bp);
    return hipGetLastError();
}
size_t inw_cost_uints(uint32_t nblk) { return 3 * size_t(nblk) + 256 + kSkyInfo; }
size_t inw_sky_info_at(uint32_t nblk) { return 2 * size_t(nblk) + 256; }
// One frame of the on-chip-fold INW kernels: the probe (unless forced), then k_inw_pm and
// k_inw_sm, of which the one the probe did not pick exits at once.  ring: blocks * 4 waves *
// max(ring_pm, ring_sm) float4; mode: 2 uints (zeroed here).  force: 0 = probe, 1 = pm, 2 = sm.
// sky (needs cost and sc.beam): the sky blocks rendered by k_inw_sky -- the beam lists, the
// classifier and k_inw_sky then come before the claim-order kernels, which put the blocks whose flag
// k_inw_sky left standing at the head of the order, and k_inw_sky_queues starts k_inw_pm's queues
// past them.
hipError_t launch_inw_fold(const Frame &f, const InwScene &sc, float4 *ring, uint32_t ring_pm, uint32_t ring_sm,
                           unsigned *counter, uint32_t *mode, uint32_t force, int blocks, int blocks_ln,
                           uint32_t *cost, bool sky, const BeamPrune &bp, hipStream_t s) {
    for (uint32_t r : {ring_pm, ring_sm})
        if (r < 64 || (r & (r - 1))) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(mode, 0, 2 * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    // the probe first: the claim-order and beam kernels below read its verdict and exit at once
    // on a sample-major frame
    if (force == 0) {
        const uint32_t nblk = units_of(f) / 64u, waves = 1024u;  // ~1024 probe blocks of 8x8 pixels
        const uint32_t stride = nblk > waves ? nblk / waves : 1u, nw = (nblk + stride - 1u) / stride;
        const dim3 g((nw + 3u) / 4u);
        if (sc.layout == 4) hipLaunchKernelGGL(k_inw_probe<true>, g, dim3(kBlock), 0, s, f, sc, stride, mode);
        else hipLaunchKernelGGL(k_inw_probe<false>, g, dim3(kBlock), 0, s, f, sc, stride, mode);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // claim order of k_inw_pm (cost: 3 * nblk + 256 + kSkyInfo uints -- keys, the order, buckets, the
    // sky blocks' bookkeeping and flags -- or null = unit order)
    const uint32_t *border = nullptr;
    const bool order = cost && units_of(f) >= 64u;
    sky = sky && order && sc.beam;
    if (order) {
        const uint32_t nblk = units_of(f) / 64u;
        uint32_t *key = cost, *ord = cost + nblk, *hist = cost + 2 * nblk, *flag = hist + 256 + kSkyInfo;
        if ((e = hipMemsetAsync(hist, 0, (256 + kSkyInfo) * sizeof(uint32_t), s)) != hipSuccess) return e;
        const dim3 g((nblk + 3u) / 4u);  // 4 blocks of 8x8 pixels per 256-lane block
        if (sky) {
            if ((e = launch_inw_beam(f, sc, bp, mode, force, s)) != hipSuccess) return e;
            hipLaunchKernelGGL(k_inw_sky_classify, g, dim3(kBlock), 0, s, f, sc, flag, hist + 256, mode, force);
            hipLaunchKernelGGL(k_inw_sky, dim3(nblk), dim3(kSkyBlock), 0, s, f, sc, flag, hist + 256);
        }
        const uint32_t *fl = sky ? flag : nullptr;
        if (sc.layout == 4) hipLaunchKernelGGL(k_inw_cost<true>, g, dim3(kBlock), 0, s, f, sc, key, hist, mode, force, fl);
        else hipLaunchKernelGGL(k_inw_cost<false>, g, dim3(kBlock), 0, s, f, sc, key, hist, mode, force, fl);
        hipLaunchKernelGGL(k_inw_order_scan, dim3(1), dim3(256), 0, s, hist, nblk, mode, force);
        hipLaunchKernelGGL(k_inw_order_scatter, dim3((nblk + kBlock - 1) / kBlock), dim3(kBlock), 0, s, key, hist,
                           ord, nblk, mode, force);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        border = ord;
    }
    if (sc.beam && !sky && (e = launch_inw_beam(f, sc, bp, mode, force, s)) != hipSuccess) return e;
    for (int k = 0; k < 2; k++) {  // (pm, then sm) each with its own queue counter
        if ((e = hipMemsetAsync(counter + 16 * k, 0, sizeof(unsigned), s)) != hipSuccess) return e;
        if (k == 0 && sc.xcdq && (e = hipMemsetAsync(counter + 64, 0, 8 * 16 * sizeof(unsigned), s)) != hipSuccess)
            return e;  // k_inw_pm's per-XCD queues
        if (k == 0 && sky) hipLaunchKernelGGL(k_inw_sky_queues, dim3(1), dim3(64), 0, s, cost + inw_sky_info_at(units_of(f) / 64u), counter);
        const uint32_t rm = (k == 0 ? ring_pm : ring_sm) - 1u;
        unsigned *ctr = counter + 16 * k;
        if (blocks_ln > 0) {  // the LDS-staged BVH top (768-lane blocks); FU: the fused-fma cull
            const dim3 g(blocks_ln), b(3 * kBlock);
#define RT_INW_LN_LAUNCH(L, F)                                                                              \
    do {                                                                                                    \
        if (k == 0 && sc.lring) hipLaunchKernelGGL((k_inw_pm<L, true, F, true>), g, b, 0, s, f, sc, ring, rm, ctr, mode, force, border); \
        else if (k == 0) hipLaunchKernelGGL((k_inw_pm<L, true, F>), g, b, 0, s, f, sc, ring, rm, ctr, mode, force, border); \
        else if (sc.lring_sm) hipLaunchKernelGGL((k_inw_sm<L, true, F, true>), g, b, 0, s, f, sc, ring, rm, ctr, mode, force, border); \
        else hipLaunchKernelGGL((k_inw_sm<L, true, F>), g, b, 0, s, f, sc, ring, rm, ctr, mode, force, border);        \
    } while (0)
            if (k == 0 && sc.layout != 4 && sc.fused && sc.lring && sc.gstk && sc.gq_blocks)  // GQ
                hipLaunchKernelGGL((k_inw_pm<false, true, true, true, true>), dim3(sc.gq_blocks),
                                   dim3(pm_sub<true, true>() * kBlock), 0, s, f, sc, ring, rm, ctr, mode, force, border);
            else if (sc.layout == 4) {
                if (sc.fused) RT_INW_LN_LAUNCH(true, true);
                else RT_INW_LN_LAUNCH(true, false);
            } else {
                if (sc.fused) RT_INW_LN_LAUNCH(false, true);
                else RT_INW_LN_LAUNCH(false, false);
            }
#undef RT_INW_LN_LAUNCH
        } else if (sc.layout == 4) {
            if (k == 0) hipLaunchKernelGGL(k_inw_pm<true>, dim3(blocks), dim3(kBlock), 0, s, f, sc, ring, rm, counter, mode, force, border);
            else hipLaunchKernelGGL(k_inw_sm<true>, dim3(blocks), dim3(kBlock), 0, s, f, sc, ring, rm, counter + 16, mode, force, border);
        } else {
            if (k == 0) hipLaunchKernelGGL(k_inw_pm<false>, dim3(blocks), dim3(kBlock), 0, s, f, sc, ring, rm, counter, mode, force, border);
            else hipLaunchKernelGGL(k_inw_sm<false>, dim3(blocks), dim3(kBlock), 0, s, f, sc, ring, rm, counter + 16, mode, force, border);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rtk
