// rt_dev_scene.hpp -- the device scene behind the C ABI (opaque to its callers), the kernels'
// views of it, the compaction-round loop its launches share, and what the host units
// (rt_scene_build.hip, rt_launch.hip, rt_launch_spec.hip, rt_capi.hip, rt_capi_debug.hip) call in
// each other.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/rt_hip.h"
#include "../../include/rt_hip_debug.h"
#include "rt_device.hpp"
#include "rt_host.hpp"
#include "rt_kernels.hpp"

// process-wide state, each defined by the unit that sets it
extern rt_options g_opt;               // rt_options_set (rt_capi.hip); scenes copy it at creation
extern unsigned long long *g_dbg;      // rt_debug_counters(): lane-occupancy diagnostics (rt_capi_debug.hip)
extern unsigned *g_px_rays;            // rt_debug_pixel_rays(): rays per work unit
extern int g_build_levels;             // rt_debug_build_level_cap(): the device build's level cap (0 = 256)
extern bool g_time_kernels;            // rt_debug_time_kernels
extern uint32_t g_sky_blocking[3];     // rt_debug_sky_blocks(NULL): the last blocking render's sky blocks

// IOW-03: the culling BVH beside the shared node buffer, and the RI values of its materials
struct IowCullPriors {
    int root_link = 0;       // culling BVH: leftData of the root
    uint32_t n_wide = 0;     // culling BVH: 4-wide nodes
    DevBuf obox;             // per-object culling boxes (2 float4 each) for wave-cooperative queries
    float ri_prior = 1.0f;   // most common refractive index (sample-parallel guess)
    // alternative runs: the values a stale ray-stack RI can hold (0 for a never-written
    // entry, 1 for the camera ray, every material RI; 03...glsl:285-356), up to 8, else none
    float alt_vals[8] = {};
    int n_alt_vals = 0;
    int depth = 0;           // culling BVH: levels of the 4-wide tree
    // rt_dev_scene_iow03_update (update_iow03)
    uint32_t built = 0;      // where the culling BVH was built: 0 host, 1 device, 2 host after the device build ran
                             // past its level cap, 3 host because a box was not finite (rt_debug_iow_info info[3])
    uint32_t updates = 0;    // successful updates so far
    DevBuf build_ws;         // the device build's workspace (rt_build.hip)
};

// INW: the wide walk's structures and the surrounding-RI grid (make_inw_wide, make_inw_wide_device)
struct InwWalk {
    DevBuf wnodes, wrank, wleaf;  // culling BVH, depth-first ranks, LBVH leaf boxes
    DevBuf qnodes;                // ... the culling BVH quantised (4 float4 per node, rtk::inw_quantize_wnodes)
    DevBuf cnodes;                // ... without the repeated low planes (7 float4 per node, rtk::inw_compact_wnodes)
    DevBuf ri_cells, ri_ids;      // surrounding-RI grid (cell offsets, object ids)
    float ri_lo[3] = {}, ri_hi[3] = {}, ri_inv[3] = {};
    int ri_dim[3] = {};
    int wdepth = 0;               // levels of the 4-wide culling BVH
    uint32_t n_wnodes = 0;        // its nodes (every tree)
    uint32_t n_wtree0 = 0;        // ... of the tree over the swept boxes (the first ones)
    uint32_t wbins = 1, wbin_stride = 0;  // time-bin trees after it (rtamd::InwWide::bins)
    bool ri_ok = false;           // the RI grid applies (ri_cells / ri_ids hold it)
    float wbound = 0.0f;          // largest |coordinate| of the culling boxes (the fused cull's condition)
    uint32_t dfs_high = 0;        // the reference walk's stack high-water mark (0: no walkable LBVH)
    bool sl_ok = false;           // the node buffer has the stackless walks' layout (lbvh_walk_info)
    uint32_t wbuild = 0;          // where the walk structures were built: 0 host, 1 device, 2 host after the
                                  // device build ran past its level cap (rt_debug_wide_info info[7])
    DevBuf lbvh_ws, aabb, lcnt;   // rt_dev_scene_inw_update: device LBVH workspace, object boxes, leaf counts
    DevBuf build_ws, ri_fill, ri_tmp;  // ... and the device build of the wide walk and RI grid (rt_build.hip)
    DevBuf dec, wbin_tmp;         // rt_dev_scene_inw_update_device: k_inw_prepare's decision words, the bin trees as built
    // no structures: the state both builders start from (the buffers keep their capacity)
    void reset() {
        dfs_high = 0;
        sl_ok = false;
        n_wnodes = n_wtree0 = 0;
        wbins = 1;
        wbin_stride = 0;
        ri_ok = false;
    }
};

// INW: what the fold launch keeps between frames (launch_scene_inw_fold)
struct InwFold {
    DevBuf ring;             // k_inw_pm / k_inw_sm: the waves' fold rings
    uint32_t ring_frame = 0; // frames rendered with the current fold rings (their tag epoch)
    DevBuf mode;             // k_inw_probe's verdict (2 uints)
    DevBuf cost;             // claim order: block cost keys, the order, 256 bucket offsets
    DevBuf beam, beam_n;     // pixel beams: beam_cap (id, entry t) per unit; count + cut per unit
    DevBuf gstk;             // k_inw_pm's GQ instance: the reference's 40-float stacks, 160 B per lane
};

// chunked-render workspace, sized for `units` pixel units (grown on demand), and the
// tail-compaction continuation buffers (ping-pong), blocks_cap*kBlock slots each
struct SeqWorkspace {
    uint32_t units = 0;
    size_t temp_bytes = 0;
    DevBuf state, cost, keys, iota, order, temp;
    DevBuf cont[2], cont_count;
};

// sample-parallel IOW-03 (launch_scene_spec): the records, sized for `cap` (pixel units x samples)
struct SpecState {
    size_t cap = 0, units = 0;
    uint32_t P = 0, S = 0;  // the last sample-parallel render's P and S (its record layout, SpecRecs::ix)
    DevBuf col, fin, ctr, assume, list, fb, counts;
    DevBuf keys, keys2, list2, temp;  // longest-first ordering of the re-execution list
    size_t temp_bytes = 0;
    DevBuf pstate;  // asynchronous windows: per-pixel frontier state
    DevBuf front;   // checkpoint rounds: per-pixel frontier (uint4)
    DevBuf sorder, fcost;  // heavy-first enumeration: sample indices by cost, their costs
    DevBuf alt, alt_hash, alt_count;  // alternative runs (sized for alt_cap records)
    uint32_t alt_cap = 0;
    unsigned epoch = 0;  // frame tag of the records (16 bits in their flags; next_spec_epoch)
    uint32_t launch_seq = 0;
    // the pipeline after sample 0: its own queue counter, continuation buffers and sort scratch
    // (rt_render_* calls on one scene must not overlap)
    DevBuf lane_counter, lane_cont[2], lane_cont_count, lane_temp;
    size_t lane_temp_bytes = 0;
    DevBuf dbg_t;             // RT_DEBUG_TIMES diagnostics: per unit start / end launch
    size_t dbg_n = 0;         // units (P * S) of the render that last wrote dbg_t
    DevBuf exact;             // RT_SPEC_ORACLE diagnostics: exact incoming state per sample
    size_t exact_n = 0;
    bool exact_valid = false;
};

// what the last render ran: each launch function fills one and stores it, the rt_debug_* entry
// points read it
struct LastRender {
    rt_path_info path{};       // rt_debug_path
    char kernel[64] = {0};     // the render's main kernel (rt_debug_launches)
    int launches = 0;          // ... and its launches
    int chunks = 0;            // sample chunks (rt_debug_chunks)
    // the INW fold launch: `kernel` names the fold kernel's instance once rt_debug_launches has
    // read the probe's verdict (fold_pending until then)
    bool fold_pending = false;
    bool ln = false;           // it used the LDS-staged kernels
    bool fu = false;           // ... their fused-fma cull instances
    uint32_t force = 0;        // ... its forced order (0: the probe's pick, read back from fold.mode)
    bool lring = false;        // ... k_inw_pm's fold ring was in LDS
    bool lring_sm = false;     // ... k_inw_sm's
    bool gq = false;           // ... k_inw_pm's GQ instance (quantised nodes, global stacks)
    uint32_t ring[2] = {0, 0}; // ... its fold windows (pixel-major, sample-major)
    bool sky = false;          // ... it ran the sky-block kernels (rt_debug_sky_blocks)
    uint32_t sky_blocks = 0;   // ... the frame's 8x8 blocks
    uint32_t beam_lists = 0;   // ... its beam lists, units x time bins (0: none; rt_debug_beam_lists)
    uint32_t beam_cap = 0;     // ... entries a list can hold
    bool beam16 = false;       // ... entries of 32 bits (InwScene::beam16)
};

// A prepared scene: device-resident records, LBVH nodes, lights and sample tables.
struct rt_dev_scene {
    rt_options opt = g_opt;  // the options current when the scene was created (rt_dev_scene_set_options)
    int kind = 0;  // 3 = IOW-03, 11/14 = INW layout 1/4
    int device = 0;
    int spp = 0;
    uint32_t n = 0, n_lights = 0;
    int layout = 0;
    int s_stop = 0;      // IOW-03: samples before the ring schedule's early return (== spp in practice)
    int blocks_cap = 0;  // persistent grid size: resident blocks the device can hold (max over variants)
    int cus = 0;
    int n_focus = 0;        // INW-01 MULTIFOCUS lens chain (0 = the reference's single focus)
    float focus[9] = {};
    DevBuf hot, cold, nodes, lights, sunflower, fib, ring, counter;
    float sf_max = 0.0f;  // largest |x| + |y| of the sunflower lens table
    DevBuf sph;           // INW sphere scenes: 2 float4 per object (rtk::InwScene::sph)
    bool sph_ok = false;
    DevBuf tex, tex_info;  // INW-04 material textures (float4 texels, (first, w, h, 0) per texture)
    uint32_t n_tex = 0;
    DevBuf pass_ws;        // INW progressive passes: the camera rays and answers of one chunk of samples
    DevBuf select_ws;      // rt_pass_select_async: the block partials of the rectangle's units (8 B a block)
    DevBuf walk_ctr;       // the last frame's closest-hit queries handed to the LBVH walks (u64)
    bool broken = false;   // a failed rt_dev_scene_inw_update / rt_dev_scene_iow03_update left the buffers
                           // inconsistent: no renders, no queries
    bool tex_missing = false;  // rt_dev_scene_inw_update_device met a textured object and the scene has no texture
                               // bound: renders and queries return RT_E_UNSUPPORTED until a later update
    IowCullPriors iow;
    InwWalk walk;
    InwFold fold;
    SeqWorkspace ws;
    SpecState sp;
    LastRender last;
    // rt_debug_time_kernels: HIP events around every launch of the render's main kernel
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kt_ev;
    size_t kt_used = 0;
};

// ---------------------------------------------------------------- the kernels' scene views
// root_link says whether the scene has a culling BVH: after an update to a scene without one the node
// and box buffers still hold the old tree (they keep their capacity), so the kernels get null then,
// which is what they read as "the linear loop".
inline rtk::IowScene iow_view(const rt_dev_scene &s) {
    const bool bvh = s.iow.root_link != 0;
    return rtk::IowScene{s.hot.as<float>(), s.cold.as<float>(), s.n, bvh ? s.nodes.as<float4>() : nullptr,
                         s.sunflower.as<float>(), s.fib.as<float>(), s.ring.as<int>(), s.iow.root_link,
                         bvh ? s.iow.obox.as<float4>() : nullptr, bvh ? s.iow.n_wide : 0u, s.opt.iow_lds_bvh};
}

// INW wide walk (DESIGN.md "INW wide walk").  The reference finds the closest hit by a
// depth-first walk of its LBVH (01_BVH...glsl:431-473); the result is the nearest hit, ties to
// the object the walk meets first, among the objects whose LBVH leaf box the ray crosses.  The
// kernels find the same object with an ordered walk of a 4-wide culling BVH over the leaf boxes
// (inflated to stay conservative), the reference's exact test on the leaf box, and a (t, rank)
// rule with each object's rank in the reference's depth-first order.  That equivalence needs
// the reference walk to drop no push on its shared 40-float stack: dfs_high is the walk's
// stack high-water mark, and the kernels use the wide walk only while size + dfs_high <= 40.
inline rtk::InwScene inw_view(const rt_dev_scene &s) {
    rtk::InwScene sc{s.hot.as<float4>(), s.cold.as<float4>(), s.nodes.as<float4>(),
                     s.lights.as<float>(), s.n, s.n_lights, s.layout, s.sunflower.as<float>(),
                     s.tex.as<float4>(), s.tex_info.as<int4>(), s.n_tex};
    const InwWalk &w = s.walk;
    if (!w.dfs_high) return sc;
    sc.dfs_high = w.dfs_high;
    sc.sl = w.sl_ok && s.opt.inw_stackless ? 1u : 0u;  // stackless LBVH walks (rt_options.inw_stackless)
    if (!w.n_wnodes) return sc;  // no wide walk
    sc.wnodes = w.wnodes.as<float4>();
    sc.wroot = 1;
    if (w.wbins > 1 && s.opt.inw_time_bins > 1) {  // (built at scene creation; 0 / 1 later: unused)
        sc.wbin_base = w.n_wtree0; sc.wbin_stride = w.wbin_stride;
        if (s.opt.inw_walk_bins) sc.wbins = w.wbins;  // the wide closest-hit walks (set_beam: the beam lists)
    }
    sc.rank = w.wrank.as<uint32_t>();
    sc.leafbox = w.wleaf.as<float4>();
    if (s.sph_ok && s.opt.inw_sphere_records) sc.sph = s.sph.as<float4>();
    if (s.opt.inw_compact_nodes) sc.cnodes = w.cnodes.as<float4>();
    sc.n_wnodes = w.n_wnodes;
    if (w.ri_ok && s.opt.inw_ri_grid) {
        sc.ri_cells = w.ri_cells.as<uint32_t>();
        sc.ri_ids = w.ri_ids.as<uint32_t>();
        for (int a = 0; a < 3; a++) {
            sc.ri_lo[a] = w.ri_lo[a]; sc.ri_hi[a] = w.ri_hi[a]; sc.ri_inv[a] = w.ri_inv[a]; sc.ri_dim[a] = w.ri_dim[a];
        }
    }
    return sc;
}

// ---------------------------------------------------------------- compaction rounds
// A queue of compaction rounds: its stream and work-queue counter, the two continuation buffers
// (ping-pong) and the round counts, 64 B apart (separate cache lines; rt_debug_rounds).
struct RoundQueue {
    hipStream_t st;
    unsigned *counter;
    const DevBuf *cont;
    unsigned *cnt;
    float4 *buf(int r) const { return cont[r & 1].as<float4>(); }  // round r writes it, round r + 1 reads it
    unsigned *count(int r) const { return cnt + 16 * r; }          // lanes parked by round r
};

// park lanes only while at least this many units remain (rt_options.park_min; -1: cap / 8 waves)
inline uint32_t park_min_of(const rt_dev_scene *s, int cap) {
    return uint32_t(s->opt.park_min >= 0 ? s->opt.park_min : cap * rtk::kBlock / 8);
}

// One compacted pass as 1 + `rounds` launches (rounds <= 14: rt_options): the first takes n0
// units, each later one resumes the lanes the previous one parked.  Counts stay on the device
// (no host round trip): a resume launch with nothing parked exits at once.  Parking stops below
// park_min units, where compaction can no longer shorten the critical path; the last round never
// parks, and with `spread` gives its long units a wave each.  solo_first: the first launch takes
// its sorted head one unit per wave (Cont.solo_n).  launch(ct, n_units) enqueues one round.
template <class Launch>
hipError_t run_rounds(const RoundQueue &q, int rounds, uint32_t n0, int cap, uint32_t park_min, bool spread,
                      uint32_t solo_first, Launch &&launch) {
    hipError_t e = hipSuccess;
    for (int r = 0; r <= rounds && e == hipSuccess; r++) {
        rtk::Cont ct{};
        uint32_t n_units = n0;
        if (r > 0) {
            ct.in = q.buf(r - 1);
            ct.in_count = q.count(r - 1);
            n_units = uint32_t(cap) * rtk::kBlock;
        }
        if (r < rounds) {
            ct.out = q.buf(r);
            ct.out_count = q.count(r);
            ct.park_min = park_min;
            e = hipMemsetAsync(ct.out_count, 0, sizeof(unsigned), q.st);
            if (e != hipSuccess) break;
        } else if (r > 0 && spread) ct.spread = 1;
        if (r == 0) ct.solo_n = solo_first;
        e = launch(ct, n_units);
    }
    return e;
}

// ---------------------------------------------------------------- across the units
// rt_scene_build.hip
int make_iow03(rt_dev_scene *s, const float *types, const float *rec, uint32_t n, int spp);
int make_inw(rt_dev_scene *s, const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
             uint32_t n_lights, const rt_texture *tex, int n_tex, int spp);
int update_inw(rt_dev_scene *s, const float *geom, uint32_t n, const float *nodes, const float *aabbs,
               const float *lights, uint32_t n_lights, double *ms);
int update_inw_device(rt_dev_scene *s, const float *d_geom, uint32_t n, const float *d_aabbs, const float *d_lights,
                      uint32_t n_lights, int flags, hipStream_t st, double *ms);
int update_iow03(rt_dev_scene *s, const float *types, const float *rec, uint32_t n, int flags, double *ms);
int update_iow03_device(rt_dev_scene *s, const float *d_types, const float *d_rec, uint32_t n, int flags, hipStream_t st,
                        double *ms);
// make_iow03's hot / cold records (n * kIowHot, n * kIowCold floats; either may be null) and RI priors
// of host records, no device; the priors as {ri_prior, alt_vals[8] (0 past the count), n_alt_vals}
void iow_prepare_host(const float *types, const float *rec, uint32_t n, float *hot, float *cold, float priors[10]);
void iow_priors_out(const IowCullPriors &q, float priors[10]);
bool inw_sphere_records(const float *geom, uint32_t n, int layout, std::vector<float> &out);
bool inw_textured(const float *geom, uint32_t n, int layout);
bool textures_ok(const rt_texture *tex, int n_tex);
// rt_launch.hip
bool params_ok(const rt_params *p);
rtk::Frame make_frame(const rt_camera *cam, const rt_params *p);
int ensure_workspace(rt_dev_scene *s, uint32_t units);
int ensure_cont(rt_dev_scene *s);
int launch_scene(rt_dev_scene *s, rtk::Frame &f, hipStream_t st);
// rt_debug_sky_blocks of a scene's last render (synchronises when the sky-block kernels ran)
int sky_blocks_of(rt_dev_scene *s, uint32_t out[3]);
int render_blocking(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, float *rgba, float *depth,
                    rt_stats *st);
// rt_launch_spec.hip
bool ensure_spec(rt_dev_scene *s, uint32_t P, uint32_t S);
int launch_scene_spec(rt_dev_scene *s, rtk::Frame &f, hipStream_t st);
