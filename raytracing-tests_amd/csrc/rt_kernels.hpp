// rt_kernels.hpp -- launch-side declarations shared by the kernel units (rt_iow_render.hip,
// rt_iow_spec.hip, rt_inw_render.hip, rt_inw_fold.hip, rt_diag_kernels.hip and the query, build and
// stage units) and the host units that launch them (rt_scene_build.hip, rt_launch*.hip, rt_capi*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_beam_prune.hpp"

namespace rtk {

// Per-launch uniforms, computed on the host exactly as the reference host + shader
// prologue would (camera vectors are derived on the device with the contract's ops).
struct Frame {
    int W, H, spp, max_bounces, show_normal;
    // pixel mapping: rect mode (tiles == nullptr) or tile-list mode
    int x0, y0, tw, th;
    const int *tiles;
    int n_tiles, tile_size;
    float *out_rgba;    // full image (rect mode) or packed tiles (tile mode)
    float *out_depth;   // may be null
    unsigned long long *counters;  // 6 x u64
    float pos[3], dir[3];
    float aperture, focus, screen_dist, inv_spp;
    float sphere[4];    // IOW-01 only
    unsigned long long *dbg;  // optional lane-occupancy counters (kDbg* slots), null in production
    int leaf_batch;           // IOW-03 walk: test postponed leaves once this many lanes hold one
    unsigned *px_rays;        // optional: rays cast per work unit, written when its pixel completes (IOW);
                              // INW fold kernels add one per segment at the output pixel's index
    int coop_max;             // IOW-03: wave-cooperative closest hits when at most this many lanes trace
    int dbg_first_stale;      // diagnostics: record the segment of a sample's first stale read (corrupts drops)
    // INW-01 MULTIFOCUS (01_BVH...glsl:388-404, 505-549; "#if MULTIFOCUS" in the reference):
    // n_focus = 0 is the single-focus camera the reference builds, 1..9 the lens chain
    int n_focus;
    float focus_list[9];
    int narrow;               // rt_options.iow_narrow (host side: iow_narrow)
    unsigned long long *walk_ctr;  // INW: closest-hit queries that fell back to the LBVH walks (added to; may be null)
};
// lane-occupancy counters (per wave-iteration: 1 and popcount of the participating lanes)
enum { kDbgOuter = 0, kDbgOuterLanes, kDbgTrav, kDbgTravLanes, kDbgLeaf, kDbgLeafLanes, kDbgSeg, kDbgSegLanes,
       // per-wave shader-clock cycles (IOW-03): camera-ray part of the work loop, closest-hit
       // queries, their BVH walk (incl. leaf tests), the leaf tests, ray segments (incl. query)
       kDbgCycCam, kDbgCycRay, kDbgCycTrav, kDbgCycLeaf, kDbgCycSeg, kDbgCycSpare0, kDbgCycSpare1, kDbgCycSpare2,
       kDbgSlots = 16 };

// IOW-03 device scene: "hot" records walked by the linear loop + "cold" hit attributes.
constexpr int kIowHot = 20;   // pos3 type M9 scale3 inv_scale3 pad
constexpr int kIowCold = 8;   // color3 material3 scat2
// INW device scene
constexpr int kInwHot = 28;   // pos3 R9 scale3 delta3 type extra inv_scale3 inv_s2_3 ri_acc pad
constexpr int kInwCold = 8;   // refr refl srfr srfl color3 ri

constexpr int kIowBvhStack = 32;  // IOW BVH traversal stack entries; a ray that overflows it also runs the linear loop
struct IowScene {
    const float *hot, *cold;
    uint32_t n;
    const float4 *nodes;     // conservative 4-wide BVH over the objects (8 float4 per node) or null = linear loop
    const float *sunflower;  // spp*2
    const float *fib;        // spp*4 (xyz + pad)
    const int *ring;         // spp*2
    int root_link;           // link of the BVH root (wide node 0 -> 1)
    const float4 *obox;      // the BVH leaves' conservative boxes: n float4 (lo.xyz, hi.x), n float2 (hi.yz); or null
    uint32_t n_nodes;        // 4-wide BVH nodes
    int lds_on;              // rt_options.iow_lds_bvh: the LDS-staged kernels may run (iow_lds)
};
struct InwScene {
    const float4 *hot;       // n * 7 float4
    const float4 *cold;      // n * 2 float4
    const float4 *nodes;     // (2n-1) * 2 float4
    const float *lights;     // L * 7
    uint32_t n, n_lights;
    int layout;
    const float *sunflower;  // spp*2
    // u_MaterialTextures (04...glsl:10): texels as float4 (unorm8 / 255, converted on the
    // host), tex_info[k] = (first texel, width, height, 0); n_tex = 0: none bound
    const float4 *tex;
    const int4 *tex_info;
    uint32_t n_tex;
    // Wide walk (DESIGN.md "INW wide walk"; null wnodes = off): a 4-wide culling BVH over the
    // LBVH leaf boxes, each object's rank in the reference's depth-first order for either child
    // order (rank[g] with invert false, rank[n + g] with invert true), its LBVH leaf node, and the
    // depth-first stack high-water mark (pushes can only drop when size + dfs_high > 40)
    const float4 *wnodes = nullptr;
    // the same nodes as 7 float4 (lx ly lz hx hy hz links; DESIGN.md §5.2 "Compact nodes"), read by
    // the buffer-load walk from global memory when set (the LDS staging and the other walks keep wnodes)
    const float4 *cnodes = nullptr;
    int wroot = 0;
    const uint32_t *rank = nullptr;
    const float4 *leafbox = nullptr;  // per object: its LBVH leaf node (2 float4: the reference's leaf box)
    // Sphere scenes (DESIGN.md §5.2 "Sphere records"; null = off): every object an ellipsoid of equal
    // scales with the identity rotation; per object 3 float4, (position, RN(1/scale)), (position -
    // last_position, its RI) and (RN(1/RN(scale^2)) per axis, extra: the hit normal's inputs).  The wide walk's, the beam lists' and the RI grid's object tests read
    // these instead of the 7-float4 record: R = I makes the object-space ray the world one, the same
    // floats (up to the signs of zero terms, which neither t nor the inside test can see); the
    // winner's normal still comes from the full record
    const float4 *sph = nullptr;
    uint32_t dfs_high = 0;
    uint32_t n_wnodes = 0;  // wide nodes
    uint32_t n_lnodes = 0;  // the first n_lnodes wide nodes are staged in LDS (LN kernels only)
    // Time-bin trees (wbins = 0: none): the wide closest-hit walk of a ray with time
    // ratio r starts at node 1 + wbin_base + b * wbin_stride, b = min(int(r * wbins), wbins - 1),
    // the root of the tree over the boxes the objects sweep in [b / wbins, (b + 1) / wbins]
    uint32_t wbins = 0, wbin_base = 0, wbin_stride = 0;
    // Stackless LBVH walks (rt_options.inw_stackless; DESIGN.md §5 "Stackless LBVH
    // walk"): the reference's depth-first walks without their stack, by parent links, wherever no
    // push of the reference walk could drop (size + dfs_high <= 40).  sl = 0: off (or the node
    // buffer lacks the layout: left children at odd indices, right = left + 1, rightData = parent)
    uint32_t sl = 0;
    uint32_t n_blds = 0;    // LN kernels without the wide walk: the first n_blds LBVH nodes staged in LDS
    int fused = 0;          // the wide walk culls with one fma per plane (cull4nf<true>; set per frame)
    uint32_t lring = 0;       // k_inw_pm (768-lane instances): the fold ring in LDS (kPmLdsRing entries per wave)
    uint32_t lring_sm = 0;    // k_inw_sm (768-lane instances): the same
    uint32_t xcdq = 0;        // k_inw_pm claims from per-XCD queues (rt_options.inw_claim_xcd)
    uint32_t ring_epoch = 0;  // fold-ring tags: the frame's epoch (0..62) << 26 (ring_tag, rt_inw_fold.hip)
    // Quantised wide nodes (DESIGN.md §5.2 "Quantised nodes"; null = off): the culling BVH of
    // wnodes as 4 float4 per node -- origin.xyz, scale.x | scale.yz, low-plane bytes x, y | low z,
    // high x, y, z (byte k = child k) | links -- each plane rounded outward (rt_build.hip:
    // k_quantize_wnodes).  Read by the wide closest-hit walk of the k_inw_pm<..., GQ> instance, which
    // also stages the first n_lnodes of them in LDS and keeps the reference's 40-float stack in
    // global memory (gstk: kFStack / 4 float4 per lane of the grid, [slot4][lane]).
    const float4 *qnodes = nullptr;
    float4 *gstk = nullptr;
    uint32_t gq_blocks = 0;  // the GQ instance's grid (kGqSub * kBlock lanes per block, resident blocks)
    // Pixel beams (DESIGN.md §5 "Pixel beams"; null beam = off): for each pixel unit, the objects
    // whose culling box the beam of its primary rays can cross, sorted by the entry t of the
    // central ray into the box inflated by beam_R (k_inw_beam).  The 64 lists of an 8x8 block are
    // packed in unit order in the block's region of 64 * beam_cap entries: beam_n[u] = offset in
    // the region << 8 | count (kBeamOff: use the wide walk), beam_cut[u] = every object with an
    // entry below it is listed.
    const uint2 *beam = nullptr;  // beam_cap entries per unit: object id, entry t (float bits); beam16:
                                  // one uint32 each, id in the low half, t's high half (t rounded down)
    uint32_t beam16 = 0;
    const uint32_t *beam_n = nullptr;
    const float *beam_cut = nullptr;
    uint32_t beam_cap = 0;
    // beam_bins > 1: one list per pixel unit and time bin (k_inw_beam walks bin b's tree, the one at
    // 1 + wbin_base + b * wbin_stride): the lists, counts and cuts of bin b follow those of bins < b
    // (beam_units units each); a primary ray reads its time bin's list
    uint32_t beam_bins = 0, beam_units = 0;
    float beam_R = 0.0f, beam_tmin = 0.0f, beam_tfar = 0.0f, beam_kappa = 0.0f;
    // Surrounding-RI grid (DESIGN.md §5 "RI grid"; null ri_cells = off): a uniform grid over the
    // LBVH leaf boxes; cell c lists (ri_ids[ri_cells[c] .. ri_cells[c + 1]]) every object whose
    // leaf box, widened by a margin above the rounding of the cell index, overlaps the cell.
    const uint32_t *ri_cells = nullptr, *ri_ids = nullptr;
    float ri_lo[3] = {0, 0, 0}, ri_hi[3] = {0, 0, 0}, ri_inv[3] = {0, 0, 0};
    int ri_dim[3] = {0, 0, 0};
};
constexpr uint32_t kBeamOff = 0xffffffffu;

// One launch of a chunked render: samples [s_begin, s_end) of every pixel unit.  A pixel's
// samples must run in order (IOW-03 reads stale stack slots of earlier samples), so the
// per-pixel state (accumulator + the IOW stack's RI slots) is parked in `state` between
// launches, `cost` records the rays each unit spent, and `order` (a permutation of unit ids,
// longest first) lets the next launch schedule the expensive pixels first.
struct Chunk {
    int s_begin, s_end;      // sample range of this launch
    int final_chunk;         // write the image (else park the state)
    float4 *state;           // 2 float4 per unit (may be null for a single-chunk render)
    const unsigned *order;   // unit permutation or null (natural order)
    unsigned *cost;          // rays per unit in this launch, or null
    const unsigned *order_count;  // device count of `order` entries (null: all units)
    int per_unit_begin;      // first sample of each unit = bits of state[2*unit].w (else s_begin)
    // sample-parallel records (SpecRecs, below) to validate before running a sample, or null:
    // a sample whose record assumed the exact incoming stack state is taken from the record
    const float4 *rec_col, *rec_fin, *rec_assume;
    const uint4 *rec_ctr;
    uint32_t rec_P, rec_S;  // their layout: unit s * rec_P + pu at pu * rec_S + s (SpecRecs::ix)
};

// Sample-parallel IOW-03 (DESIGN.md "Sample-parallel speculation").  A unit is one (pixel,
// sample) pair, u = s*P + pu.  Each sample runs with an assumed incoming stack state (the RI
// of entries 1..3 that earlier samples of the pixel left behind) and records what it read and
// wrote; a resolve pass replays the pixel's samples in order and re-queues every sample whose
// assumption was wrong.  Records are SoA over u.
struct AltRec {  // an alternative run of a speculative sample (RT_SPEC_ALT, DESIGN.md "Alternative runs")
    uint32_t u;      // unit (s * P + pu)
    uint32_t state;  // 0 queued / running, else 1 + the launch it finished in
    uint32_t pad0, pad1;
    float4 assume, col, fin;
    uint4 ctr;
};
struct SpecRecs {
    float4 *col;       // rgb of the sample, flags (bits: rmask 0-3, wmask 4-7)
    float4 *fin;       // RI of entries 1..3 after the sample, prim tests (bits)
    uint4 *ctr;        // segments, stack drops, NaN directions, node visits
    float4 *assume;    // assumed RI of entries 1..3 before the sample
    uint32_t P, S;     // pixel units, samples per pixel (s_stop)
    // The record of unit u = s * P + pu sits at pu * S + s: a pixel's samples are adjacent, so the
    // waves of the bulk pass (consecutive samples of one pixel) read and write whole lines, and the
    // per-pixel sample walks (chain following, the frontier rounds) stay in one line for 8 samples
    // (DESIGN.md §5.4).  u < 2^32; q = mulhi(u, pmag) is u / P or one more.
    __host__ __device__ __forceinline__ size_t ix(size_t u) const {
        const uint32_t uu = (uint32_t)u;
#ifdef __HIP_DEVICE_COMPILE__
        uint32_t q = __umulhi(uu, pmag);
#else
        uint32_t q = (uint32_t)(((uint64_t)uu * pmag) >> 32);
#endif
        int32_t r = (int32_t)(uu - q * P);
        if (r < 0) { q--; r += (int32_t)P; }
        return (size_t)(uint32_t)r * S + q;
    }
    uint32_t *list;    // re-execution list (units)
    unsigned *list_count;
    uint32_t *fb_list; // pixels left to the sequential kernel after the last resolve
    unsigned *fb_count;
    const uint32_t *order;  // pixel units, heaviest sample 0 first (kSpecRest)
    uint32_t order_base, order_n;  // this group's slice of `order` (order_n == 0: all P units)
    uint4 *pstate;     // asynchronous windows: per pixel unit 3 x uint4 of frontier state
    uint32_t epoch;    // frame tag: finished records carry it in their flags
    uint4 *front;      // checkpoint rounds: per pixel unit (first unvalidated sample, exact RI bits of entries 1..3)
    // heavy-first enumeration (fresh_mode 1..3): sample indices 1..S-1 by measured cost, most
    // expensive first; the first n_heavy of them run for every pixel before the rest
    const uint32_t *sorder;
    uint32_t probe_stride, n_heavy;
    // diagnostics (RT_SPEC_ORACLE=1): the final resolve stores every sample's exact incoming
    // RI of entries 1..3 (exact_mode bit 0) and the next render's guesses copy them (bit 1), so
    // a frame runs with no misprediction -- the bound any better guess could reach
    float4 *exact = nullptr;
    int exact_mode = 0;
    // checkpoint rounds: per pixel unit, the first unfinished sample past the main frontier whose
    // exact incoming state the anchored scan of k_iow03_frontier found, and that state (x =
    // 0xffffffff: none); k_iow03_fixf patches or restarts it like a sample at the frontier
    uint4 *front2 = nullptr;
    uint32_t scan_max = 0;  // samples the anchored scan may look past the main frontier (0 = off)
    // diagnostics (RT_DEBUG_TIMES=1): per unit, the launch of its last start (bits 0-15) and its
    // start count (bits 16-31), and the launch it finished in (rt_debug_spec_times)
    uint32_t *dbg_start = nullptr, *dbg_end = nullptr;
    // alternative runs: records, a hash u -> (first slot, count) with key u + 1 (0 = empty), the
    // slot counter, the values a stale entry can hold, and the segment count that makes a
    // sample long enough to get alternatives
    AltRec *alt = nullptr;
    uint2 *alt_hash = nullptr;
    unsigned *alt_count = nullptr;
    uint32_t alt_cap = 0, alt_hcap = 0, alt_min_seg = 0;
    float alt_vals[8] = {};
    int n_alt_vals = 0;
    uint32_t pmag = 0;  // ceil(2^32 / P) (spec_pmag): ix() divides a unit by P with one mulhi
};
// ceil(2^32 / P) for SpecRecs::pmag (P >= 2)
inline uint32_t spec_pmag(uint32_t P) { return (uint32_t)(((1ull << 32) + P - 1) / P); }
// the record index of unit u (SpecRecs::ix) by plain division (diagnostics, host reads)
__host__ __device__ inline size_t spec_rec_ix(size_t u, uint32_t P, uint32_t S) { return (u % P) * S + u / P; }
enum { kSpecFirst = 0, kSpecRest = 1, kSpecList = 2 };

// Tail compaction between launches.  Once the work queue is empty, a wave whose busy lanes
// fall below kParkBelow parks them (state at a ray-segment boundary) in `out`, slot ids from
// a wave-aggregated atomic on `out_count`, and exits; the next launch resumes the parked
// lanes from `in` in full waves.  in == null: the launch's units are pixels.  out == null or
// fewer than park_min units in the launch: lanes run to completion (the final round).
constexpr int kBlock = 256;      // threads per block of every render kernel
constexpr int kInwLdsNodes = 236;        // wide BVH nodes the INW fold kernels stage in LDS (rt_inw_fold.hip)
constexpr uint32_t kPmLdsRing = 256;     // k_inw_pm's LDS fold ring: entries per wave (InwScene::lring) ...
constexpr uint32_t kPmLdsNodes = 5;      // ... and the nodes it leaves staged
// k_inw_pm's GQ instance (DESIGN.md §5.1 "GQ": the reference's 40-float stacks in global memory):
// kGqSub 256-lane sub-blocks per block (= waves per SIMD; 1 block per CU), per block the wide walks'
// node stacks in LDS (kWStack entries per lane), the fold rings (3 KB per wave), the depth slots,
// and in the rest of the CU's 160 KB the top of the culling BVH: kQLdsNodes quantised nodes
// (64 B each)
constexpr int kFStack = 40;  // stack_capacity (FLT_STACK, 01_BVH...glsl:80)
constexpr int kWStack = 16;
constexpr int kQNodeF4 = 4;
constexpr int kGqSub = 3;
constexpr int kGqLdsFree = 163840 - kGqSub * kWStack * kBlock * 4 - kGqSub * 4 * 3 * (int)kPmLdsRing * 4 -
                           kGqSub * kBlock * 4;
constexpr int kQLdsNodes = kGqLdsFree / 64;
constexpr int kParkBelow = 32;    // park when fewer than half the wave's lanes are busy
constexpr int kContSlots = 13;    // float4 per parked lane
struct Cont {
    const float4 *in;
    const unsigned *in_count;
    float4 *out;
    unsigned *out_count;
    uint32_t park_min;
    // sample-parallel checkpoint rounds: a launch takes the parked lanes of `in` first, then the
    // fresh units [fresh_lo, fresh_hi) of its mode (mixed != 0); park_below = 65 parks every
    // busy lane once the queue drains (0 = kParkBelow, the tail-compaction rule)
    int mixed, park_below;
    uint32_t fresh_lo, fresh_hi;
    // fresh units of kSpecRest: 0 = samples 1.. pixel-major in R.order; 1 = probe (every sample
    // of every probe_stride-th pixel of R.order); 2 = the n_heavy costliest sample indices,
    // sample-major; 3 = the other indices, pixel-major.  Modes 1-3 skip units already started.
    int fresh_mode;
    uint32_t seg_budget;  // > 0: a lane parks its unit after this many segments in the launch
    int spread;           // a wave takes at most ceil(units / waves) units at a time
    // units sorted longest first (the LPT re-execution list): while the queue head is below
    // min(solo_n, waves), an empty wave takes one unit and keeps it alone to the end, so
    // the longest samples run with the wave-cooperative closest hits instead of sharing a wave
    uint32_t solo_n;
    uint32_t launch_id;  // sequence number of the launch in the frame (diagnostics)
    int chain;           // exact restarts follow their pixel's chain of mispredicted samples
};

hipError_t launch_iow01(const Frame &f, hipStream_t s);
// rt_stages.hip: IOW-00 gradient, IOW-02 groups (records N x 18, ring = sample-table ring
// schedule, pw[i] = pow(0.4, i) for i < max_bounces)
hipError_t launch_iow00(int W, int H, float *out, hipStream_t s);
hipError_t launch_iow02(const Frame &f, const float *types, const float *rec, uint32_t n, const int *ring,
                        const float *pw, int cull_front, int cull_back, hipStream_t s);
// Persistent work-queue launches: `counter` (one u32, device) is zeroed on `s` before the
// kernel; at most `blocks_cap` blocks are launched (they pull pixels until none are left).
// n_units: pixel units (cont.in == null) or parked lanes to resume (host-known count)
hipError_t launch_iow03(const Frame &f, const IowScene &sc, const Chunk &ch, const Cont &ct, uint32_t n_units,
                        unsigned *counter, int s_stop, int blocks_cap, hipStream_t s);
hipError_t launch_inw(const Frame &f, const InwScene &sc, const Chunk &ch, const Cont &ct, uint32_t n_units,
                      unsigned *counter, int blocks_cap, hipStream_t s);
uint32_t units_of(const Frame &f);
// sample-parallel IOW-03 pass over the units of `mode` (kSpec*)
hipError_t launch_iow03_spec(const Frame &f, const IowScene &sc, const SpecRecs &R, int mode, const Cont &ct,
                             uint32_t n_units, unsigned *counter, int blocks_cap, hipStream_t s);
// LBVH build on the device (rt_lbvh.hip); ws = lbvh_workspace_bytes(n) of scratch; lcnt (optional,
// 2n - 1 entries): every node's leaf count, in the output's (breadth-first) numbering
size_t lbvh_workspace_bytes(uint32_t n);
hipError_t lbvh_build_device(const float *aabb, uint32_t n, float *out, void *ws, size_t ws_bytes, hipStream_t s,
                             uint32_t *lcnt = nullptr);
// INW wide walk structures built on the device from a device LBVH (rt_build.hip, DESIGN.md
// "Device build"): 4-wide culling BVH (10 float4 per node, <= n nodes), depth-first ranks (2n),
// leaf boxes (2n float4); out's scalars are filled in.  Synchronises the stream (level counts).
struct InwWideDev {
    float4 *wnodes;
    uint32_t *rank;
    float4 *leafbox;
    uint32_t n_wnodes, dfs_high;
    int depth;
    float wbound;
    float ri_lo[3], ri_hi[3];  // bounds of the leaf boxes (the RI grid's extent)
};
size_t inw_build_workspace_bytes(uint32_t n);
// nodes: the device LBVH (lbvh_build_device), lcnt: its leaf counts (lbvh_build_device's lcnt)
// max_levels (0 = 256): the binary SAH and collapse levels launched at most; a deeper tree returns
// hipErrorNotSupported (the caller then builds on the host)
hipError_t inw_wide_build_device(const float4 *nodes, const uint32_t *lcnt, uint32_t n, void *ws, size_t ws_bytes,
                                 InwWideDev &out, hipStream_t s, int max_levels = 0);
// The IOW-03 culling structures built on the device from the uploaded hot records (rt_build.hip,
// DESIGN.md §5.12): the object boxes as the kernels read them (obox: n float4 (lo xyz, hi x), then n
// float2 (hi y, hi z); bit-equal to rtamd::iow_cull_build's) and a 4-wide culling BVH over them by the
// same binned SAH levels and collapse as the INW build (wide: 8 float4 per node, <= n nodes).
// 2 <= n < 16384; ws holds inw_build_workspace_bytes(n).  Synchronises the stream (level counts).
// hipErrorNotSupported: deeper than max_levels; nonfinite != 0: some box value is not finite (the
// tree is then not to be used); in both cases the caller builds on the host.
// d_priors (may be null): iow_prepare_device's ten result words, which then come back in the same copy
// as the build's counts (priors; unwritten when the build returns an error).
struct IowCullDev {
    uint32_t n_wide;
    int depth;
    uint32_t nonfinite;
    uint32_t priors[10];
};
hipError_t iow_cull_build_device(const float *hot, uint32_t n, void *ws, size_t ws_bytes, float4 *wide, float4 *obox,
                                 IowCullDev &out, hipStream_t s, int max_levels = 0, const uint32_t *d_priors = nullptr);
// An IOW-03 update from device-resident records (rt_build.hip): the hot (kIowHot floats) and
// cold (kIowCold) records of the n objects at types (n) and rec (n * 24; any 4-byte alignment, float4 loads
// when 16-byte aligned), byte-equal to iow_records (rt_scene_build.hip), and the RI priors of iow_priors
// as ten words on the device at *d_priors (inside ws): {ri_prior, alt_vals[8], n_alt_vals as a float}, from
// a radix sort of the RIs' orderable bits and a run-length pass.  ws: 256-byte aligned,
// iow_prepare_workspace_bytes(n).  Never synchronises.
size_t iow_prepare_workspace_bytes(uint32_t n);
hipError_t iow_prepare_device(const float *types, const float *rec, uint32_t n, float *hot, float *cold, void *ws,
                              size_t ws_bytes, const uint32_t **d_priors, hipStream_t s);
// {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} of k_iow_prepare with float4 loads (which
// = 0) and scalar loads (1), k_iow_mode (2), k_iow_priors (3)
hipError_t update_iow_kernel_info(int which, int info[4]);
// A scene update from device-resident records (rt_build.hip).  None of these synchronises
// except inw_bin_trees_device (the level counts).
// inw_prepare_device: the hot (kInwHot floats), cold (kInwCold) and sphere (12) records of the n GeometryBuff
// records at geom (device, n * 28), byte-equal to inw_records / inw_sphere_records (rt_scene_build.hip), and
// the decision words dec (8 uint32, device; zeroed here), which inw_decisions decodes once read back.
struct InwDecisions {
    bool spheres;      // every object an unrotated sphere (inw_sphere_records returns true)
    bool moving;       // some delta is not zero
    bool textured;     // layout 4: some TextureIndex >= 1 (inw_textured)
    bool bins_finite;  // rtamd::inw_bin_boxes refuses no object
    double stick_out;  // rtamd::inw_stick_out over the caller's boxes (+inf: some value is not finite)
};
hipError_t inw_prepare_device(const float *geom, const float *aabbs, uint32_t n, int layout, float *hot, float *cold,
                              float *sph, uint32_t *dec, hipStream_t s);
InwDecisions inw_decisions(const uint32_t dec[8]);
// per object the box of rtamd::inw_bin_boxes with one bin (n * 6 floats)
hipError_t inw_swept_boxes_device(const float *geom, uint32_t n, float *out, hipStream_t s);
// The time-bin trees (rtamd::inw_wide_add_bins) over rtamd::inw_bin_boxes' boxes, computed on the device:
// tree b built by the SAH and collapse levels into tmp + b * n nodes (10 float4 each) with links of its own,
// then placed by inw_bin_place_device at node n0 + b * stride of wnodes, links rebased, the rest of each
// stride empty nodes.  ws holds inw_build_workspace_bytes(n).  hipErrorNotSupported: deeper than max_levels.
struct InwBinsDev {
    uint32_t nw[16];  // nodes of each tree
    uint32_t stride;  // the largest
    float wbound;     // largest |coordinate| of the bin boxes
};
hipError_t inw_bin_trees_device(const float *geom, uint32_t n, uint32_t bins, void *ws, size_t ws_bytes, float4 *tmp,
                                InwBinsDev &out, hipStream_t s, int max_levels = 0);
hipError_t inw_bin_place_device(const float4 *tmp, uint32_t n, uint32_t bins, const InwBinsDev &t, uint32_t n0,
                                float4 *wnodes, hipStream_t s);
// {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} of k_inw_prepare (which = 0), k_bin_boxes
// (1), k_swept_boxes (2), k_bin_place (3)
hipError_t update_kernel_info(int which, int info[4]);
// the quantised form of nw wide nodes (InwScene::qnodes): 4 float4 per node, planes rounded
// outward by at least `margin` beyond the wide node's (rt_build.hip)
hipError_t inw_quantize_wnodes(const float4 *wnodes, uint32_t nw, float4 *qnodes, float margin, hipStream_t s);
// InwScene::cnodes from the wide nodes (rt_build.hip)
hipError_t inw_compact_wnodes(const float4 *wnodes, uint32_t nw, float4 *cnodes, hipStream_t s);
// the surrounding-RI grid on the device (rtamd::ri_grid_build's cells and ids) over the extent
// inw_wide_build_device returned: per-cell counts scanned into cells[0..nc] with the total and an
// over-64 flag read back (synchronises), then the ids
size_t ri_scan_temp_bytes(size_t cells);
hipError_t ri_count_device(const float4 *leafbox, uint32_t n, void *ws, const double lo[3], const double inv[3],
                           const int dim[3], uint32_t *cells, void *tmp, size_t tmp_bytes, uint32_t *total,
                           uint32_t *over, hipStream_t s);
hipError_t ri_fill_device(const float4 *leafbox, uint32_t n, const double lo[3], const double inv[3], const int dim[3],
                          const uint32_t *cells, uint32_t *fill, uint32_t *ids, hipStream_t s);
// Texture producers (rt_texture.hip): noise textures (MakeTexture, utility.h:69-192) and the
// Mercator <-> cubic re-projection (utility.cpp:266-463).  noise_batches_exact(W): the
// reference's 4 column batches tile [0, W) (other widths index out of bounds there).
bool noise_batches_exact(uint32_t W);
size_t noise_workspace_bytes(int W, int H);
hipError_t noise_texture(int W, int H, int type, const float *grad, int n_grad, float freq, float lac, float gain,
                         int octaves, uint8_t *d_rgb, void *d_ws, hipStream_t s);
// Display pass (rt_display.hip): RGBA32F colour or R32F depth -> RGBA8 framebuffer texels
hipError_t display_rgba8(const float *rgba, const float *depth, uint32_t n, int use_depth, uint8_t *out,
                         hipStream_t s);
size_t remap_workspace_bytes(int W, int H);
hipError_t texture_remap(const uint8_t *d_in, int W, int H, int C, int load_as, uint8_t *d_out, void *d_ws,
                         hipStream_t s);
hipError_t spec_hist(const uint4 *ctr, size_t n, unsigned long long *d_out, hipStream_t s);  // diagnostics
hipError_t spec_list_stale(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *list, const unsigned *count,
                           unsigned long long *d_out,
                           hipStream_t s);  // diagnostics
hipError_t spec_list_hist(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *list, const unsigned *count,
                          unsigned long long *d_out,
                          hipStream_t s);  // diagnostics
hipError_t spec_pixels(const uint4 *ctr, uint32_t P, uint32_t S, const uint32_t *order, uint32_t *d_out,
                       hipStream_t s);  // diagnostics
// after the kSpecFirst pass: assumptions for samples 1.. and the per-pixel ordering keys
// checkpoint rounds: advance each pixel's frontier over finished, valid samples and
// queue a finished sample at the frontier whose assumption was wrong for an exact re-run
// (appended to cont as a restart, at most cap entries in all); then make parked samples at the
// frontier exact (patch unread entries, or restart)
hipError_t launch_iow03_frontier(const Frame &f, const SpecRecs &R, float4 *cont, unsigned *count, uint32_t cap,
                                 hipStream_t s);
hipError_t launch_iow03_fixf(const Frame &f, const SpecRecs &R, float4 *cont, const unsigned *count, int max_lanes,
                             hipStream_t s);
// heavy-first enumeration: per sample index cost from the probe pixels' records and the parked
// lanes' progress -> R.sorder; per pixel cost of its heavy samples -> key (sort -> R.order)
hipError_t launch_iow03_sample_order(const Frame &f, const SpecRecs &R, const float4 *cont, const unsigned *count,
                                     int max_lanes, unsigned long long *fcost, uint32_t *sorder, hipStream_t s);
hipError_t launch_iow03_pixel_key(const Frame &f, const SpecRecs &R, const float4 *cont, const unsigned *count,
                                  int max_lanes, unsigned *key, hipStream_t s);
// rt_math.hpp's shortened sequences against the compiler's for all 2^32 x (k_check_fastmath):
// mismatch count, lowest bad x
hipError_t launch_check_fastmath(int which, unsigned long long *bad, unsigned *first, hipStream_t s);
hipError_t launch_iow03_altspawn(const Frame &f, const SpecRecs &R, float4 *cont, unsigned *count, uint32_t cap,
                                 hipStream_t s);
hipError_t launch_iow03_prep(const Frame &f, const SpecRecs &R, unsigned *key, float prior, uint32_t prior_from,
                             hipStream_t s);
// replay each pixel's samples: re-queue wrong assumptions; final: write clean pixels, hand
// the rest (with their resume state in `state`) to the sequential kernel via R.fb_list
hipError_t launch_iow03_resolve(const Frame &f, const SpecRecs &R, bool final_pass, float4 *state, hipStream_t s);

// INW with the on-chip End() folds (k_inw_probe + k_inw_pm / k_inw_sm); ring:
// blocks * (kBlock / 64) * max(ring_pm, ring_sm) float4 (powers of two >= 64); counter: 2 queue
// counters 64 B apart; mode: 2 uints; force: 0 = probe decides, 1 = pixel-major, 2 = sample-major
// blocks_ln > 0: the fold kernels run as blocks_ln 768-lane blocks with the top of the wide BVH
// staged in LDS (ring: max(blocks * 4, blocks_ln * 12) waves)
hipError_t launch_inw_fold(const Frame &f, const InwScene &sc, float4 *ring, uint32_t ring_pm, uint32_t ring_sm,
                           unsigned *counter, uint32_t *mode, uint32_t force, int blocks, int blocks_ln,
                           uint32_t *cost, bool sky, const BeamPrune &bp, hipStream_t s);
// cost: the claim order's workspace, inw_cost_uints(blocks of 8x8 units) uints; its sky-block
// bookkeeping (rt_debug_sky_blocks) starts at inw_sky_info_at(blocks): flagged, rendered at + 1, + 2
size_t inw_cost_uints(uint32_t nblk);
size_t inw_sky_info_at(uint32_t nblk);
// the pixel beams of a pixel-major frame (sc.beam*; exits when the probe picks sample-major); bp:
// which leaves the lists drop (rt_beam_prune.hpp)
hipError_t launch_inw_beam(const Frame &f, const InwScene &sc, const BeamPrune &bp, const uint32_t *mode, uint32_t force,
                           hipStream_t s);
// rt_trace.hip: n_rays closest-hit queries (rt_ray / rt_hit as 2 float4 each) on a persistent grid
// of at most cus * inw_trace_blocks_per_cu blocks; queue: one u32 (zeroed here); counters: 6 x u64
// added to (slots 0, 1, 2, 4), or null.  sc.fused picks the fused-cull instance.
hipError_t launch_inw_trace(const InwScene &sc, const float4 *rays, uint32_t n_rays, bool invert, bool any,
                            float4 *hits, unsigned long long *counters, unsigned *queue, int cus, hipStream_t s);
int inw_trace_blocks_per_cu(bool any, bool fused);
// k_inw_trace's {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} (hipFuncGetAttributes)
hipError_t inw_trace_kernel_info(bool any, bool fused, int info[4]);
// rt_trace_iow.hip: n_rays closest-hit queries on an IOW-03 scene, same persistent grid and buffers
// (counters: slots 0, 1, 2).  iow_lds(sc) picks the LDS-staged instance; sc.nodes == null runs the
// linear loop; leaf_batch = rt_options.iow_leaf_batch.
hipError_t launch_iow_trace(const IowScene &sc, int leaf_batch, const float4 *rays, uint32_t n_rays, bool any,
                            float4 *hits, unsigned long long *counters, unsigned *queue, int cus, hipStream_t s);
int iow_trace_blocks_per_cu(bool any, bool ln);
// k_iow_trace's {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} (hipFuncGetAttributes)
hipError_t iow_trace_kernel_info(bool any, bool ln, int info[4]);
// rt_paths.hip: n_rays path queries (rt_path_ray / rt_path_out as 2 float4 each) on a persistent grid
// of at most cus * inw_paths_blocks_per_cu blocks with persistent lanes; queue: one u32 (zeroed
// here); counters: 6 x u64 added to, or null.  sc.layout picks INW-01 / INW-04, sc.fused the
// fused-cull instance; spp: the length of sc.sunflower / 2.
hipError_t launch_inw_paths(const InwScene &sc, const float4 *rays, uint32_t n_rays, int spp, int max_bounces,
                            bool invert, float4 *out, unsigned long long *counters, unsigned *queue, int cus,
                            hipStream_t s);
int inw_paths_blocks_per_cu(bool lights, bool fused);
// k_inw_paths' {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} (hipFuncGetAttributes)
hipError_t inw_paths_kernel_info(bool lights, bool fused, int info[4]);
int inw_paths_max_blocks(int blocks);  // rt_debug_paths_max_blocks: cap the grid (0 = off); the previous cap
// rt_path_iow.hip: n_rays path queries on an IOW-03 scene (rt_path_iow_ray / rt_path_iow_out as 3 float4
// each) in chains of `chain` (>= 1) consecutive queries, one chain per persistent lane of a grid of at
// most cus * iow_paths_blocks_per_cu blocks; queue: one u32 (zeroed here); counters: 6 x u64 added to
// (slots 0, 1, 2, 4, 5), or null.  iow_lds(sc) picks the LDS-staged instance; sc.nodes == null runs
// the linear loop; spp: the length of sc.fib / 4; leaf_batch = rt_options.iow_leaf_batch.
hipError_t launch_iow_paths(const IowScene &sc, int leaf_batch, int max_bounces, const float4 *rays, uint32_t n_rays,
                            uint32_t chain, int spp, float4 *out, unsigned long long *counters, unsigned *queue,
                            int cus, hipStream_t s);
int iow_paths_blocks_per_cu(bool ln);
// k_iow_paths' {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} (hipFuncGetAttributes)
hipError_t iow_paths_kernel_info(bool ln, int info[4]);
int iow_paths_max_blocks(int blocks);  // rt_debug_path_iow_max_blocks: cap the grid (0 = off); the previous cap
// rt_pixels.hip: the camera rays of samples [s0, s0 + ns) of `pixels` (x, y pairs) as path-query
// records, record k * ns + j = pixel k, sample s0 + j; n = pixels * ns <= 2^31 records (2 float4 each
// on an INW scene, 3 on an IOW-03 one).  f: make_frame's (W, H, spp, the camera, screen_dist).
hipError_t launch_camera_rays(const Frame &f, const InwScene &sc, const int2 *pixels, uint32_t n, uint32_t s0,
                              uint32_t ns, float4 *rays, hipStream_t s);
hipError_t launch_camera_rays(const Frame &f, const IowScene &sc, const int2 *pixels, uint32_t n, uint32_t s0,
                              uint32_t ns, float4 *rays, hipStream_t s);
// ... and the fold of f.spp path answers per pixel (samples: pixel-major) into one rt_pixel_out (2 float4) each
hipError_t launch_pixel_fold(const Frame &f, bool iow, const int2 *pixels, uint32_t n_pixels, const float4 *samples,
                             float4 *out, hipStream_t s);
// {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} of k_camera_rays (which = 0 INW, 1
// IOW-03) and k_pixel_fold (2 INW, 3 IOW-03)
hipError_t pixels_kernel_info(int which, int info[4]);
// rt_passes.hip, IOW-03: samples [s0, s1) of every pixel of f's rectangle (rect mode; f.out_rgba and
// f.out_depth may be null, f.counters is added to) on a persistent grid of at most cus * resident
// blocks, a lane per pixel; state: 2 float4 per pixel of the W x H image (rt_pass_state), read when
// s0 > 0 and left as the state after sample s1 - 1; queue: one u32 (zeroed here).  s1 <= the scene's
// s_stop, f.leaf_batch set, iow_lds(sc) picks the LDS-staged instance.
hipError_t launch_iow_pass(const Frame &f, const IowScene &sc, uint32_t s0, uint32_t s1, float4 *state,
                           unsigned *queue, int cus, hipStream_t s);
// rt_passes.hip, INW: the two ends of a pass around launch_inw_paths.  The camera rays of samples
// [s0, s0 + ns) of every unit of f's rectangle as path queries, record u * ns + j = unit u, sample
// s0 + j (units_of(f) * ns <= 2^31 records of 2 float4); and End()'s fold of the answers into the state
// (the first float4 of a pixel's rt_pass_state; read when s0 > 0), with the image acc * RN(1 / k) and
// the depth written when k > 0.
hipError_t launch_pass_rays(const Frame &f, const InwScene &sc, uint32_t s0, uint32_t ns, float4 *rays,
                            hipStream_t s);
hipError_t launch_pass_fold(const Frame &f, uint32_t s0, uint32_t ns, uint32_t k, const float4 *out, float4 *state,
                            hipStream_t s);
// {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} of k_pass_rays (which = 0), k_pass_fold
// (1) and k_iow_pass (2 nodes staged in LDS, 3 not); 4..7: the same four for a packed tile list.  The
// three launches above pick the tile-list instance when f.tiles is set (units, state and image by slot).
hipError_t pass_kernel_info(int which, int info[4]);
int pass_max_blocks_now();        // the cap rt_debug_pass_max_blocks set (0 = none)
int pass_max_blocks(int blocks);  // rt_debug_pass_max_blocks: cap the grid (0 = off); the previous cap
// rt_adaptive.hip: a pass over the list `pixels` (x, y pairs; an entry outside the image is skipped) in
// which every pixel renders samples [count, min(count + ns, stop)), count = its rt_pass_aux's (aux: one
// float4 per pixel of the W x H image: even.xyz, the count's bits).
// INW: the two ends of a chunk around launch_inw_paths.  Record k * ns + j = entry k, sample count + j
// (the invalid sample past stop; n_pixels * ns <= 2^31 records of 2 float4); and the fold of the answers
// into state and aux, which advances the count, with the image acc * RN(1 / count) and the depth written
// when `last`.
hipError_t launch_adapt_rays(const Frame &f, const InwScene &sc, const int2 *pixels, uint32_t n_pixels,
                             const float4 *aux, uint32_t stop, uint32_t ns, float4 *rays, hipStream_t s);
hipError_t launch_adapt_fold(const Frame &f, const int2 *pixels, uint32_t n_pixels, uint32_t stop, uint32_t ns,
                             bool last, const float4 *out, float4 *state, float4 *aux, hipStream_t s);
// The same pair over a slot list of f's packed tile list (f.tiles set; a slot = tile * T * T + iy * T + ix, one
// that is 0xffffffff, past the list's slots or outside the image is skipped): state, aux, image and answers by slot.
hipError_t launch_adapt_rays(const Frame &f, const InwScene &sc, const uint32_t *slots, uint32_t n_slots,
                             const float4 *aux, uint32_t stop, uint32_t ns, float4 *rays, hipStream_t s);
hipError_t launch_adapt_fold(const Frame &f, const uint32_t *slots, uint32_t n_slots, uint32_t stop, uint32_t ns,
                             bool last, const float4 *out, float4 *state, float4 *aux, hipStream_t s);
// IOW-03: launch_iow_pass's persistent grid over the list (queue: one u32, zeroed here; pass_max_blocks caps
// the grid).
hipError_t launch_iow_adapt(const Frame &f, const IowScene &sc, const int2 *pixels, uint32_t n_pixels, uint32_t stop,
                            uint32_t ns, float4 *state, float4 *aux, unsigned *queue, int cus, hipStream_t s);
hipError_t launch_iow_adapt(const Frame &f, const IowScene &sc, const uint32_t *slots, uint32_t n_slots, uint32_t stop,
                            uint32_t ns, float4 *state, float4 *aux, unsigned *queue, int cus, hipStream_t s);
// The stable partition of the units of f's rectangle into the active pixels, in unit order, and a tail of
// {-1, -1} up to the rectangle's pixel count; *n_active = the active count; err (W x H, may be null): the
// estimate of the rectangle's pixels.  part: select_blocks(f) + 1 uint2 of scratch.  Three launches.
uint32_t select_blocks(const Frame &f);
hipError_t launch_pass_select(const Frame &f, const float4 *state, const float4 *aux, float tol, uint32_t min_samples,
                              uint32_t stop, int2 *list, uint32_t *n_active, float *err, uint2 *part, hipStream_t s);
// The same over the units of f's packed tile list (f.tiles set): the active slots in unit order, a tail of
// 0xffffffff up to the number of slots inside the image; state, aux and err by slot.
hipError_t launch_pass_select(const Frame &f, const float4 *state, const float4 *aux, float tol, uint32_t min_samples,
                              uint32_t stop, uint32_t *slots, uint32_t *n_active, float *err, uint2 *part, hipStream_t s);
// {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} of k_adapt_rays (which = 0), k_adapt_fold
// (1), k_iow_adapt (2 nodes staged in LDS, 3 not), k_select_count (4), k_select_scan (5), k_select_scatter (6);
// 7..12: the tile-list instances of 0..4 and 6 (the scan is shared)
hipError_t adaptive_kernel_info(int which, int info[4]);
int adaptive_chunk_cap_now();          // the cap rt_debug_adaptive_chunk set (0 = none)
int adaptive_chunk_cap(int samples);   // rt_debug_adaptive_chunk: cap an INW chunk's samples (0 = off); the previous cap
// What the units that own kernels share on the launch side.
// Resident blocks per CU of `kernel` at `block` lanes (2 if the query fails): each unit answers
// resident_blocks_per_cu and its *_blocks_per_cu for the kernels it owns.
template <class K>
int occupancy_of(K kernel, int block) {
    int nb = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, 0);
    return (e == hipSuccess && nb > 0) ? nb : 2;
}
// A kernel's {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} (hipFuncGetAttributes and the
// unit's own occupancy answer): what every *_kernel_info returns.
template <class K>
hipError_t kernel_info(K kernel, int blocks_per_cu, int info[4]) {
    hipFuncAttributes a;
    const hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(kernel));
    if (e != hipSuccess) return e;
    info[0] = a.numRegs;
    info[1] = (int)a.localSizeBytes;
    info[2] = (int)a.sharedSizeBytes;
    info[3] = blocks_per_cu;
    return hipSuccess;
}
// The launch rule of a persistent grid of kBlock-lane blocks over n work items, whose waves claim
// 64 * rounds consecutive items with one atomic: at most cus * blocks_per_cu blocks (the resident grid;
// max_blocks > 0: a debug cap below it), and as many 64s per claim, kClaimRounds at most, as leave every
// wave of the grid at least four claims (the tail of a batch stays balanced; a small batch claims 64 at a
// time).
constexpr uint32_t kClaimRounds = 16;  // measured on C2 (k_iow_trace): 1 -> 5.5, 4 -> 20.9, 16 -> 32.6 G primary queries/s
struct ClaimGrid { uint32_t grid, rounds; };
inline ClaimGrid claim_grid(uint32_t n, int cus, int blocks_per_cu, int max_blocks) {
    const uint32_t need = (n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock;
    uint32_t cap = (uint32_t)(cus > 0 ? cus : 1) * (uint32_t)blocks_per_cu;
    if (max_blocks > 0 && (uint32_t)max_blocks < cap) cap = (uint32_t)max_blocks;
    const uint32_t grid = need < cap ? need : cap;
    const uint32_t per_wave = grid ? n / (64u * grid * (uint32_t)(kBlock / 64) * 4u) : 0u;  // (n = 0: no grid)
    return ClaimGrid{grid, per_wave < 1u ? 1u : (per_wave > kClaimRounds ? kClaimRounds : per_wave)};
}
// The persistent render kernels, by name, and the resident blocks per CU of each (occupancy query;
// 2 if it fails).  The kernels are private to their units, so resident_blocks_per_cu
// (rt_iow_render.hip) asks the unit that owns the kernel.
enum class RenderKernel {
    Iow03,         // k_iow03
    Iow03Narrow,   // k_iow03n
    Iow03Lds,      // k_iow03L (768-lane blocks)
    Iow03Spec,     // k_iow03s
    Iow03SpecLds,  // k_iow03sL (768-lane blocks)
    Inw01,         // k_inw<false>
    Inw04,         // k_inw<true>
    InwPm01,       // k_inw_pm<false>
    InwPm04,       // k_inw_pm<true>
    InwPmLn01,     // k_inw_pm<false, true> (768-lane blocks)
    InwPmLn04,     // k_inw_pm<true, true> (768-lane blocks)
    InwPmGq,       // k_inw_pm<false, true, true, true, true> (kGqSub * 256-lane blocks)
};
int resident_blocks_per_cu(RenderKernel k);
int iow_render_blocks_per_cu(RenderKernel k);  // rt_iow_render.hip: Iow03, Iow03Narrow, Iow03Lds
int iow_spec_blocks_per_cu(RenderKernel k);    // rt_iow_spec.hip: Iow03Spec, Iow03SpecLds
int inw_render_blocks_per_cu(RenderKernel k);  // rt_inw_render.hip: Inw01, Inw04
int inw_fold_blocks_per_cu(RenderKernel k);    // rt_inw_fold.hip: InwPm*
// IOW-03 kernel variant for this frame: narrow (byte bounce counts, 12-deep BVH stack, 4 waves
// per SIMD with spills) when rt_options.iow_narrow and u_NumOfBounce <= 255; wide otherwise
bool iow_narrow(const Frame &f);
bool iow_lds(const IowScene &sc);  // k_iow03L / k_iow03sL (BVH in LDS) apply (sc.lds_on and it fits); their blocks_cap counts 256-lane slots
// order[i] = unit ids sorted by cost, most expensive first (hipcub radix sort)
hipError_t sort_units_by_cost(const unsigned *cost, unsigned *keys_tmp, const unsigned *iota, unsigned *order,
                              uint32_t n, void *temp, size_t temp_bytes, hipStream_t s);
size_t sort_temp_bytes(uint32_t n);
// descending key/value radix sort over bits [0, end_bit)
size_t sort_pairs_temp_bytes(size_t n, int end_bit);
hipError_t sort_pairs_desc(const unsigned *keys_in, unsigned *keys_out, const unsigned *vals_in, unsigned *vals_out,
                           size_t n, void *temp, size_t temp_bytes, int end_bit, hipStream_t s);
// keys for ordering the re-execution list longest-first: the ray count of each listed unit's
// previous execution (0 beyond the list's count)
hipError_t spec_list_keys(const SpecRecs &R, unsigned *keys, size_t n, hipStream_t s);

}  // namespace rtk
