// rt_launch.hip -- enqueues a render of a device scene: the frame uniforms, the sequential
// (chunked, tail-compacted) kernels of both families, the INW fold launch, and the blocking
// render into host buffers.  The sample-parallel IOW-03 pipeline is rt_launch_spec.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_dev_scene.hpp"

bool params_ok(const rt_params *p) {
    return p && p->width > 0 && p->height > 0 && p->spp >= 1 && p->max_bounces >= 0;
}

// Uniforms of one dispatch.  screen_dist = 1/(2 tan(FOV/2)) is evaluated on the host in
// double and rounded (contract: transcendentals only on the host).
rtk::Frame make_frame(const rt_camera *cam, const rt_params *p) {
    rtk::Frame f;
    std::memset(&f, 0, sizeof(f));
    f.W = p->width; f.H = p->height; f.spp = p->spp; f.max_bounces = p->max_bounces;
    f.show_normal = p->show_normal;
    if (p->tile_w > 0 && p->tile_h > 0) { f.x0 = p->tile_x0; f.y0 = p->tile_y0; f.tw = p->tile_w; f.th = p->tile_h; }
    else { f.x0 = 0; f.y0 = 0; f.tw = p->width; f.th = p->height; }
    if (cam) {
        std::memcpy(f.pos, cam->pos, sizeof(f.pos));
        std::memcpy(f.dir, cam->dir, sizeof(f.dir));
        f.aperture = cam->aperture;
        f.focus = cam->focus_dist;
        f.screen_dist = 1.0f / (2.0f * (float)std::tan((double)(cam->fov_y_rad * 0.5f)));
    }
    f.inv_spp = 1.0f / (float)p->spp;
    f.dbg = g_dbg;
    f.px_rays = g_px_rays;
    // leaf_batch / coop_max / narrow come from the scene's options (launch_scene)
#ifdef RT_DIAG  // diagnostic builds only (make variant VDEFS=-DRT_DIAG)
    const char *fs = std::getenv("RT_DEBUG_FIRST_STALE");
    f.dbg_first_stale = (fs && fs[0] == '1') ? 1 : 0;
#endif
    return f;
}

int ensure_workspace(rt_dev_scene *s, uint32_t units) {
    SeqWorkspace &w = s->ws;
    if (units <= w.units) return RT_OK;
    HIP_OK(w.state.alloc(size_t(units) * 32));
    HIP_OK(w.cost.alloc(size_t(units) * 4));
    HIP_OK(w.keys.alloc(size_t(units) * 4));
    HIP_OK(w.order.alloc(size_t(units) * 4));
    std::vector<unsigned> iota(units);
    for (uint32_t i = 0; i < units; i++) iota[i] = i;
    HIP_OK(w.iota.upload(iota.data(), size_t(units) * 4));
    w.temp_bytes = rtk::sort_temp_bytes(units);
    HIP_OK(w.temp.alloc(w.temp_bytes));
    w.units = units;
    return RT_OK;
}

int ensure_cont(rt_dev_scene *s) {
    if (s->ws.cont_count.p) return RT_OK;
    const size_t slots = size_t(s->blocks_cap) * rtk::kBlock;
    for (auto &b : s->ws.cont) HIP_OK(b.alloc(slots * rtk::kContSlots * sizeof(float4)));
    HIP_OK(s->ws.cont_count.alloc(64 * 16));  // one count per round, 64 B apart (rt_debug_rounds)
    return RT_OK;
}

namespace {

// Sample ranges of the render.  Default: one range (tail compaction keeps the SIMDs full).
// rt_options.iow_chunks_lpt: a short first chunk measures every pixel's cost and the rest run
// longest-first (LPT) -- kept as an A/B switch; with compaction it measured slower.
std::vector<std::pair<int, int>> chunk_plan(int spp, bool lpt) {
    std::vector<std::pair<int, int>> plan;
    if (spp <= 2 || !lpt) { plan.push_back({0, spp}); return plan; }
    const int first = std::max(1, spp / 20);
    const int step = std::max(1, (spp - first + 7) / 8);
    plan.push_back({0, first});
    for (int b = first; b < spp; b += step) plan.push_back({b, std::min(spp, b + step)});
    return plan;
}

// Pixel beams (DESIGN.md §5 "Pixel beams"; rt_options.inw_beams = 0 turns them off).  Sample s of a pixel
// starts its primary ray one unit behind tip = C0 + rr * ox + ru * oy (C0 = co + cd, |rr|, |ru|
// <= 1, |ox| + |oy| <= aperture / 2 * sf_max) and aims it at F = co + cd * focus.  With
// L = |F - C0| = focus - 1, the point of that ray at fraction u of the way from tip to F is
// within delta0 * |1 - u| of the point C0 + u * L * cd of the central ray, so over the central
// parameter range [tmin, tfar] that covers the scene, every primary ray lies within
// R = delta0 * max |1 - t / L| (+ rounding slack) of the central ray.  A sample ray's hit at t
// has central parameter <= t * kappa, kappa = L / (L - delta0).
// bp: what k_inw_beam drops from the lists (rt_options.inw_beam_prune; rt_beam_prune.hpp).
int set_beam(rt_dev_scene *s, const rtk::Frame &f, rtk::InwScene &sc, rtk::BeamPrune &bp) {
    const uint32_t cap = 32;
    const InwWalk &w = s->walk;
    DevBuf &beam = s->fold.beam, &beam_n = s->fold.beam_n;
    const double units = double(rtk::units_of(f));
    rtk::BeamGeom g;
    if (!s->opt.inw_beams || !sc.wnodes || f.n_focus > 0 ||
        units * cap * 8.0 * std::max<uint32_t>(1u, w.wbins) > 8.0e9 ||  // list capacity; each list is packed
        !rtk::beam_geom(f.pos, f.aperture, f.focus, s->sf_max, w.wbound, g))
        return RT_OK;
    const double R = g.R, tmin = g.tmin, tfar = g.tfar;
    // object ids below 2^16: one uint32 per entry (the id, t's high half), else (id, t)
    const bool b16 = s->n <= 65536u && s->opt.inw_beams != 2;  // inw_beams = 2: the pairs (A/B)
    // one list per unit and time bin when the scene has time-bin trees (rt_options.inw_time_bins)
    const uint32_t nb = w.wbins > 1 && s->opt.inw_time_bins > 1 && s->opt.inw_beam_bins ? w.wbins : 1u;
    const size_t need = size_t(units) * nb * cap * (b16 ? sizeof(uint32_t) : sizeof(uint2)),
                 need_n = size_t(units) * nb * 2 * sizeof(uint32_t);
    // the lists are an optional speed-up: on a device short of memory the frame runs without them
    size_t free_b = 0, total_b = 0;
    const size_t grow = (beam.bytes < need ? need : 0) + (beam_n.bytes < need_n ? need_n : 0);
    if (grow && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || grow > free_b / 2)) return RT_OK;
    // (bytes = 0 after a failure: `grow` above counts the buffer again next frame)
    if (beam.reserve(need) != hipSuccess) { (void)hipGetLastError(); beam.bytes = 0; return RT_OK; }
    if (beam_n.reserve(need_n) != hipSuccess) { (void)hipGetLastError(); beam_n.bytes = 0; return RT_OK; }
    sc.beam = beam.as<uint2>();
    sc.beam_n = beam_n.as<uint32_t>();
    sc.beam_cut = reinterpret_cast<const float *>(beam_n.as<uint32_t>() + size_t(units) * nb);
    sc.beam_cap = cap;
    sc.beam_bins = nb > 1 ? nb : 0u;
    sc.beam_units = uint32_t(units);
    if (nb > 1) { sc.wbin_base = w.n_wtree0; sc.wbin_stride = w.wbin_stride; }
    sc.beam16 = b16 ? 1u : 0u;
    sc.beam_R = float(R);
    sc.beam_tmin = float(tmin);
    sc.beam_tfar = float(tfar);
    sc.beam_kappa = float(g.kappa);
    bp = rtk::beam_prune_of(g, s->opt.inw_beam_prune, nb);
    return RT_OK;
}

// INW with on-chip End() folds (DESIGN.md §5 "INW: on-chip End() folds"): the probe, then
// k_inw_pm and k_inw_sm (one of them exits at once), persistent launches of one frame.  The
// launches are bracketed by HIP events on their stream when kernel timing is on
// (rt_debug_kernel_time).  rt_options.inw_order = 1 / 2 forces pixel- / sample-major (tests, A/B);
// inw_ring_pm / inw_ring_sm set the fold windows (samples per wave, powers of two).
int launch_scene_inw_fold(rt_dev_scene *s, rtk::Frame &f, hipStream_t st) {
    const rt_options &o = s->opt;
    const InwWalk &w = s->walk;
    InwFold &fold = s->fold;
    const int blocks = s->cus * rtk::resident_blocks_per_cu(s->layout == 4 ? rtk::RenderKernel::InwPm04 : rtk::RenderKernel::InwPm01);
    // the top of the wide BVH staged in LDS (768-lane blocks, 3 waves per SIMD);
    // inw_lds_nodes = 0: 256-lane blocks reading every node from L1 / L2 (A/B)
    // (without the wide walk the stackless LBVH walks read the top of the LBVH from that LDS; the
    // stack walks run in the same 768-lane instances, with nothing staged)
    const int blocks_ln = o.inw_lds_nodes && (w.n_wnodes || w.dfs_high)
                              ? s->cus * rtk::resident_blocks_per_cu(s->layout == 4 ? rtk::RenderKernel::InwPmLn04
                                                                                    : rtk::RenderKernel::InwPmLn01)
                              : 0;
    // inw_ring_pm = 0: k_inw_pm's fold ring in LDS (768-lane blocks), else a global
    // ring of that many entries per wave (1024 for the 256-lane blocks)
    const bool lring = o.inw_ring_pm == 0 && blocks_ln > 0;
    const uint32_t ring_pm = lring ? rtk::kPmLdsRing : uint32_t(o.inw_ring_pm ? o.inw_ring_pm : 1024);
    // inw_ring_sm = 0: k_inw_sm's ring in LDS too when the staging keeps every node it would stage
    // anyway (a BVH top of at most kPmLdsNodes wide nodes: INW-04's rooms), else a global ring of
    // 256 entries; a power of two: the global ring of that size
    const bool fits5 = w.n_wnodes ? w.n_wtree0 <= rtk::kPmLdsNodes
                                  : (w.sl_ok && 2 * size_t(s->n) - 1 <= size_t(rtk::kPmLdsNodes) * 10 / 2);
    const bool lring_sm = o.inw_ring_sm == 0 && blocks_ln > 0 && fits5;
    const uint32_t ring_sm = lring_sm ? rtk::kPmLdsRing : uint32_t(o.inw_ring_sm ? o.inw_ring_sm : 256);
    const size_t waves = std::max(size_t(blocks) * (rtk::kBlock / 64), size_t(blocks_ln) * (3 * rtk::kBlock / 64));
    const size_t ring_bytes = waves * std::max(lring ? 0u : ring_pm, lring_sm ? 0u : ring_sm) * sizeof(float4);
    if (!fold.ring.p || fold.ring.bytes < ring_bytes) {
        if (fold.ring.reserve(ring_bytes) != hipSuccess) return RT_E_HIP;
        fold.ring_frame = 0;  // fresh memory: clear it before the first frame
    }
    // ring tags carry the frame's epoch (rtk::ring_tag); the rings are cleared only when it wraps.
    // ring_frame advances only once this frame's clear (epoch 0) is enqueued, and any failure
    // below resets it, so the next frame clears the rings before it uses them
    const uint32_t epoch = fold.ring_frame % 63u;
    fold.ring_frame = 0;
    rtk::InwScene sc = inw_view(*s);
    sc.ring_epoch = epoch << 26;
    sc.lring = lring ? 1u : 0u;
    sc.lring_sm = lring_sm ? 1u : 0u;
    sc.xcdq = o.inw_claim_xcd ? 1u : 0u;
    // the fused cull (cull4nf<true>: one fma per plane) while every ray origin -- the camera (+ lens and the unit step
    // of the primary ray), hit points inside the scene's boxes -- lies within 1000 of the origin
    // (DESIGN.md §2); not with the MULTIFOCUS lens chain, whose lens points are farther out
    {
        const float cam = std::fmax(std::fabs(f.pos[0]), std::fmax(std::fabs(f.pos[1]), std::fabs(f.pos[2]))) +
                          2.0f + std::fabs(f.aperture);
        sc.fused = (o.inw_fused_cull && f.n_focus == 0 && std::fmax(cam, w.wbound) <= 1000.0f) ? 1 : 0;
    }
    // GQ: k_inw_pm over the quantised nodes with the reference's stacks in global
    // memory -- INW-01, the LDS ring instances, the fused cull's error bound (the quantised decode
    // is argued under it)
    if (o.inw_qnodes && s->layout != 4 && lring && sc.fused && sc.wnodes && w.qnodes.p) {
        const uint32_t gb = uint32_t(s->cus * rtk::resident_blocks_per_cu(rtk::RenderKernel::InwPmGq));
        const size_t need = size_t(gb) * rtk::kGqSub * rtk::kBlock * (rtk::kFStack / 4) * sizeof(float4);
        if (fold.gstk.reserve(need) != hipSuccess) return RT_E_HIP;
        sc.qnodes = w.qnodes.as<float4>();
        sc.gstk = fold.gstk.as<float4>();
        sc.gq_blocks = gb;
    }
    const uint32_t force = (o.inw_order == 1 || o.inw_order == 2) ? uint32_t(o.inw_order) : 0u;
    s->kt_used = 0;
    std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
    hipError_t e = hipSuccess;
    if (g_time_kernels) {
        if (s->kt_ev.empty()) {
            std::pair<hipEvent_t, hipEvent_t> p{nullptr, nullptr};
            if (hipEventCreate(&p.first) != hipSuccess || hipEventCreate(&p.second) != hipSuccess) return RT_E_HIP;
            s->kt_ev.push_back(p);
        }
        ev = &s->kt_ev[0];
        s->kt_used = 1;
    }
    // the rings are cleared first (when the epoch wraps), so the events bracket the probe and the
    // two fold kernels
    // claim order, costliest blocks first (inw_claim_order = 0: unit order)
    uint32_t *cost = nullptr;
    if (o.inw_claim_order) {
        const size_t need = rtk::inw_cost_uints(rtk::units_of(f) / 64) * sizeof(uint32_t);
        if (fold.cost.reserve(need) != hipSuccess) return RT_E_HIP;
        cost = fold.cost.as<uint32_t>();
    }
    rtk::BeamPrune bp;
    if (int rc = set_beam(s, f, sc, bp); rc != RT_OK) return rc;
    // sky blocks (inw_sky_blocks = 0: off): INW-01 frames with beam lists and the claim
    // order, the single-focus camera, a fresh sample's stack below the wide walk's condition, no
    // per-pixel ray count or occupancy hook; the pixel-major verdict is read on the device
    const bool sky = o.inw_sky_blocks && s->layout != 4 && s->n_lights == 0 && f.n_focus == 0 && sc.beam && cost &&
                     rtk::units_of(f) >= 64u && force != 2 && 8u + w.dfs_high <= uint32_t(rtk::kFStack) &&
                     !f.px_rays && !f.dbg;
    {  // what this frame runs (the fold order, and with it the kernel's name, is resolved at query time)
        LastRender last;
        std::snprintf(last.kernel, sizeof(last.kernel), "%s", s->layout == 4 ? "k_inw_fold<true>" : "k_inw_fold<false>");
        last.fold_pending = true;
        last.launches = 1;
        last.chunks = 1;
        last.gq = sc.gstk != nullptr;
        last.force = force;
        last.ring[0] = ring_pm;
        last.ring[1] = ring_sm;
        last.lring = lring;
        last.lring_sm = lring_sm;
        last.ln = blocks_ln > 0;
        last.fu = last.ln && sc.fused;
        last.sky = sky;
        last.sky_blocks = rtk::units_of(f) / 64;
        last.beam_lists = sc.beam ? sc.beam_units * (sc.beam_bins > 1u ? sc.beam_bins : 1u) : 0u;
        last.beam_cap = sc.beam_cap;
        last.beam16 = sc.beam16 != 0;
        rt_path_info &P = last.path;
        P.launches = 1;
        P.order_forced = force != 0;
        P.order = int(force);
        P.wide_walk = sc.wnodes != nullptr;
        P.beams = sc.beam != nullptr;
        P.ri_grid = sc.ri_cells != nullptr;
        P.fused_cull = last.fu && sc.wnodes ? 1 : 0;  // the fused cull is the wide walk's
        P.lds_nodes = last.ln ? int(std::min<uint32_t>(w.n_wtree0, uint32_t(rtk::kInwLdsNodes))) : 0;
        P.stackless = sc.sl ? 1 : 0;
        // the LBVH nodes the stackless walks read from LDS (LN kernels without the wide walk)
        P.lbvh_lds_nodes = last.ln && sc.sl && !sc.wnodes
                               ? int(std::min<uint32_t>(2 * s->n - 1, uint32_t(rtk::kInwLdsNodes * 10 / 2))) : 0;
        P.claim_order = cost != nullptr;
        P.qnodes = sc.qnodes != nullptr;
        P.global_stack = sc.gstk != nullptr;
        P.walk_stack = sc.gstk ? rtk::kWStack : rtk::kFStack - 3;
        if (sc.gstk) P.lds_nodes = int(std::min<uint32_t>(w.n_wtree0, uint32_t(rtk::kQLdsNodes)));
        P.time_bins = sc.wnodes && !sc.gstk ? int(sc.wbins) : 0;  // the GQ walks read the staged (swept) tree
        P.beam_bins = sc.beam ? int(sc.beam_bins) : 0;
        P.sphere_records = sc.sph ? 1 : 0;
        P.beam_prune = sc.beam ? int(bp.mode >= 2u && !sc.sph ? 1u : bp.mode) : 0;  // step 2 needs the sphere records
        s->last = last;
    }
    if (epoch == 0) e = hipMemsetAsync(fold.ring.p, 0xff, fold.ring.bytes, st);
    if (e == hipSuccess) fold.ring_frame = epoch + 1;
    if (e == hipSuccess && ev) e = hipEventRecord(ev->first, st);
    if (e == hipSuccess)
        e = rtk::launch_inw_fold(f, sc, fold.ring.as<float4>(), ring_pm, ring_sm, s->counter.as<unsigned>(),
                                 fold.mode.as<uint32_t>(), force, blocks, blocks_ln, cost, sky, bp, st);
    if (e == hipSuccess && ev) e = hipEventRecord(ev->second, st);
    if (e != hipSuccess) {
        fold.ring_frame = 0;
        return launch_failed(e);
    }
    return RT_OK;
}

}  // namespace

// Enqueue a whole render (all chunks) on `st`.  The first call for a given frame size
// allocates the chunk workspace; later calls allocate nothing.
int launch_scene(rt_dev_scene *s, rtk::Frame &f, hipStream_t st) {
    if (s->broken) return RT_E_ARG;  // a failed rt_dev_scene_inw_update (update_inw)
    if (s->tex_missing) return RT_E_UNSUPPORTED;  // a textured object and no texture bound (update_inw_device)
    f.n_focus = (s->kind != 3 && s->layout == 1) ? s->n_focus : 0;
    std::memcpy(f.focus_list, s->focus, sizeof(f.focus_list));
    f.leaf_batch = s->opt.iow_leaf_batch;
    f.coop_max = s->opt.iow_coop_max;
    f.narrow = s->opt.iow_narrow;
    if (s->kind != 3) {  // the frame's closest-hit queries that fell back to the LBVH walks (rt_debug_path)
        HIP_OK(s->walk_ctr.reserve(sizeof(unsigned long long)));
        HIP_OK(hipMemsetAsync(s->walk_ctr.p, 0, sizeof(unsigned long long), st));
        f.walk_ctr = s->walk_ctr.as<unsigned long long>();
    }
    if (s->kind == 3 && s->opt.iow_spec && !rtk::iow_narrow(f) && s->s_stop > 0 &&
        ensure_spec(s, rtk::units_of(f), uint32_t(s->s_stop)))
        return launch_scene_spec(s, f, st);
    // INW: the on-chip fold kernels; inw_order = -1 runs the per-pixel sequential kernel k_inw
    // (a second restatement of End()'s loop, kept for the strategy-exactness tests)
    if (s->kind != 3 && s->opt.inw_order >= 0) return launch_scene_inw_fold(s, f, st);
    const std::vector<std::pair<int, int>> plan = chunk_plan(f.spp, s->opt.iow_chunks_lpt != 0);
    const uint32_t units = rtk::units_of(f);
    const int rounds = s->opt.rounds_seq;
    const rtk::IowScene iow = iow_view(*s);
    const rtk::InwScene inw = inw_view(*s);
    // grid of this frame's kernel variant
    int cap = s->kind == 3 ? s->cus * rtk::resident_blocks_per_cu(rtk::iow_narrow(f) ? rtk::RenderKernel::Iow03Narrow
                                                                                         : rtk::RenderKernel::Iow03)
                           : s->blocks_cap;
    LastRender last;
    const char *kernel = s->kind == 3 ? (rtk::iow_narrow(f) ? "k_iow03n" : "k_iow03") : (s->layout == 4 ? "k_inw<true>" : "k_inw<false>");
    last.launches = int(plan.size()) * (1 + rounds);
    last.chunks = int(plan.size());
    last.path.order = s->kind == 3 ? 5 : 3;
    last.path.wide_walk = s->kind != 3 && s->walk.n_wnodes != 0;
    last.path.stackless = s->kind != 3 && s->walk.dfs_high != 0 && s->walk.sl_ok && s->opt.inw_stackless;
    if (s->kind == 3 && !rtk::iow_narrow(f)) {
        if (rtk::iow_lds(iow)) {
            cap = s->cus * 3 * rtk::resident_blocks_per_cu(rtk::RenderKernel::Iow03Lds);  // 256-lane slots of the 768-lane blocks
            kernel = "k_iow03L";
        }
        last.path.iow_bvh = s->iow.root_link ? (rtk::iow_lds(iow) ? 2 : 1) : 0;
    }
    std::snprintf(last.kernel, sizeof(last.kernel), "%s", kernel);
    s->last = last;
    if (plan.size() > 1) {
        int rc = ensure_workspace(s, units);
        if (rc != RT_OK) return rc;
    }
    if (rounds > 0) {
        int rc = ensure_cont(s);
        if (rc != RT_OK) return rc;
    }
    // each chunk runs as one compacted pass (run_rounds) on the scene's queue
    const SeqWorkspace &w = s->ws;
    const RoundQueue q{st, s->counter.as<unsigned>(), w.cont, w.cont_count.as<unsigned>()};
    const uint32_t park_min = park_min_of(s, cap);
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < plan.size() && e == hipSuccess; k++) {
        rtk::Chunk ch{};
        ch.s_begin = plan[k].first;
        ch.s_end = plan[k].second;
        ch.final_chunk = k + 1 == plan.size();
        ch.state = plan.size() > 1 ? w.state.as<float4>() : nullptr;
        ch.order = k > 0 ? w.order.as<unsigned>() : nullptr;
        ch.cost = ch.final_chunk ? nullptr : w.cost.as<unsigned>();
        e = run_rounds(q, rounds, units, cap, park_min, false, 0, [&](const rtk::Cont &ct, uint32_t n_units) {
            return s->kind == 3 ? rtk::launch_iow03(f, iow, ch, ct, n_units, q.counter, s->s_stop, cap, st)
                                : rtk::launch_inw(f, inw, ch, ct, n_units, q.counter, s->blocks_cap, st);
        });
        if (e == hipSuccess && !ch.final_chunk)
            e = rtk::sort_units_by_cost(w.cost.as<unsigned>(), w.keys.as<unsigned>(), w.iota.as<unsigned>(),
                                        w.order.as<unsigned>(), units, w.temp.p, w.temp_bytes, st);
    }
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

// rt_debug_sky_blocks of the scene's last render: (flagged, rendered by k_inw_sky, blocks of the frame)
int sky_blocks_of(rt_dev_scene *s, uint32_t out[3]) {
    const LastRender &L = s->last;
    out[0] = out[1] = 0;
    out[2] = L.sky_blocks;
    if (!L.sky) return RT_OK;
    uint32_t info[3] = {0, 0, 0};  // (blocks k_inw_pm skips, flagged, rendered)
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(info, s->fold.cost.as<uint32_t>() + rtk::inw_sky_info_at(L.sky_blocks), sizeof(info),
                     hipMemcpyDeviceToHost));
    out[0] = info[1];
    out[1] = info[2];
    return RT_OK;
}

// blocking render of one scene into host buffers
int render_blocking(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, float *rgba, float *depth,
                    rt_stats *st) {
    rtk::Frame f = make_frame(cam, p);
    const size_t npx = size_t(p->width) * p->height;
    DevBuf d_rgba, d_depth, d_ctr;
    HIP_OK(d_rgba.alloc(npx * 16));
    HIP_OK(hipMemcpy(d_rgba.p, rgba, npx * 16, hipMemcpyHostToDevice));  // untouched pixels keep their value
    if (depth) {
        HIP_OK(d_depth.alloc(npx * 4));
        HIP_OK(hipMemcpy(d_depth.p, depth, npx * 4, hipMemcpyHostToDevice));
    }
    HIP_OK(d_ctr.alloc(6 * sizeof(unsigned long long)));
    HIP_OK(hipMemset(d_ctr.p, 0, 6 * sizeof(unsigned long long)));
    f.out_rgba = d_rgba.as<float>();
    f.out_depth = depth ? d_depth.as<float>() : nullptr;
    f.counters = d_ctr.as<unsigned long long>();
    double ms = 0.0;
    const int rc = timed([&] { return launch_scene(s, f, nullptr); }, &ms);
    if (rc != RT_OK) return rc;
    HIP_OK(hipDeviceSynchronize());
    if (int rs = sky_blocks_of(s, g_sky_blocking); rs != RT_OK) return rs;
    HIP_OK(hipMemcpy(rgba, d_rgba.p, npx * 16, hipMemcpyDeviceToHost));
    if (depth) HIP_OK(hipMemcpy(depth, d_depth.p, npx * 4, hipMemcpyDeviceToHost));
    return st ? read_stats(d_ctr.p, ms, st) : RT_OK;
}
