// rt_launch_spec.hip -- the sample-parallel IOW-03 pipeline: its records, the frame tags and
// the launches of one render (DESIGN.md "Sample-parallel IOW-03").
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "rt_dev_scene.hpp"

namespace {

#ifdef RT_DIAG  // diagnostic builds only: switches of the diagnostics (never of the render path)
int env_int(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : dflt;
}
#endif

constexpr int kCountSlots = 160;  // round counts of the pipeline's lane, 64 B apart

// the lane of the pipeline after sample 0; temp_bytes = sort scratch it needs
int ensure_lane(rt_dev_scene *s, size_t temp_bytes) {
    SpecState &sp = s->sp;
    if (!sp.lane_cont_count.p) {
        const size_t slots = size_t(s->blocks_cap) * rtk::kBlock;
        HIP_OK(sp.lane_counter.alloc(64));
        // 2x: parked lanes (<= resident lanes) plus restarts queued between checkpoint rounds
        for (auto &b : sp.lane_cont) HIP_OK(b.alloc(2 * slots * rtk::kContSlots * sizeof(float4)));
        HIP_OK(sp.lane_cont_count.alloc(kCountSlots * 64));
    }
    if (sp.lane_temp_bytes < temp_bytes) {
        HIP_OK(sp.lane_temp.alloc(temp_bytes));
        sp.lane_temp_bytes = temp_bytes;
    }
    return RT_OK;
}

// Frame tag of the sample-parallel records: a record is "done" for a frame when its flags carry
// the frame's tag (16 bits).  The tags are process-wide, so a new scene whose record buffers
// reuse a freed scene's memory never takes that scene's records for its own (the same render of
// the full frame, then of one tile alone, found the full frame's records at its own indices and
// returned their colours), and a scene clears its flags when its tag comes round again.
// The clear goes on the render's stream st, ordered after the scene's earlier frames on that stream
// (a null-stream memset would not wait for a non-blocking caller stream).
unsigned next_spec_epoch(rt_dev_scene *s, hipStream_t st) {
    static std::atomic<unsigned> g{0};
    unsigned v;
    do v = (g.fetch_add(1u) + 1u) & 0xffffu; while (v == 0u);
    if (v <= s->sp.epoch && s->sp.col.p)  // wrapped since this scene's last frame: forget its tags
        (void)hipMemsetAsync(s->sp.col.p, 0, s->sp.col.bytes, st);
    s->sp.epoch = v;
    return v;
}

// k_iow03s(L) launch, bracketed by events on its stream when kernel timing is on
hipError_t spec_launch(rt_dev_scene *s, const rtk::Frame &f, const rtk::IowScene &sc, const rtk::SpecRecs &R, int mode,
                       const rtk::Cont &ct, uint32_t n, unsigned *counter, int cap, hipStream_t st) {
    std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
    if (g_time_kernels) {
        if (s->kt_used == s->kt_ev.size()) {
            std::pair<hipEvent_t, hipEvent_t> p{nullptr, nullptr};
            if (hipEventCreate(&p.first) != hipSuccess || hipEventCreate(&p.second) != hipSuccess) return hipErrorUnknown;
            s->kt_ev.push_back(p);
        }
        ev = &s->kt_ev[s->kt_used++];
        hipError_t e = hipEventRecord(ev->first, st);
        if (e != hipSuccess) return e;
    }
    rtk::Cont c2 = ct;
    c2.launch_id = s->sp.launch_seq++;
    hipError_t e = rtk::launch_iow03_spec(f, sc, R, mode, c2, n, counter, cap, st);
    if (e == hipSuccess && ev) e = hipEventRecord(ev->second, st);
    return e;
}

}  // namespace

// Sample-parallel records for P pixel units x S samples; false if they do not fit.
bool ensure_spec(rt_dev_scene *s, uint32_t P, uint32_t S) {
    SpecState &sp = s->sp;
    const size_t n = size_t(P) * S;
    const size_t bytes = n * (4 * sizeof(float4) + 4 * sizeof(uint32_t)) + size_t(P) * (4 + 32);
    if (double(bytes) > s->opt.spec_max_gb * 1e9) return false;
    if (n <= sp.cap && P <= sp.units) return true;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 2) return false;
    sp.temp_bytes = rtk::sort_pairs_temp_bytes(n, 24);
    const std::pair<DevBuf *, size_t> want[] = {
        {&sp.col, n * sizeof(float4)}, {&sp.fin, n * sizeof(float4)}, {&sp.ctr, n * sizeof(uint4)},
        {&sp.assume, n * sizeof(float4)}, {&sp.list, n * sizeof(uint32_t)}, {&sp.fb, size_t(P) * 4},
        {&sp.counts, 64 * 64}, {&sp.keys, n * 4}, {&sp.keys2, n * 4}, {&sp.list2, n * 4},
        {&sp.pstate, size_t(P) * 3 * sizeof(uint4)}, {&sp.front, size_t(P) * 2 * sizeof(uint4)},
        {&sp.sorder, size_t(S) * sizeof(uint32_t)}, {&sp.fcost, size_t(S) * sizeof(unsigned long long)},
        {&sp.temp, sp.temp_bytes}};
    sp.cap = sp.units = 0;
    for (const auto &w : want) w.first->reset();  // every buffer is dropped before the first is allocated anew
    for (const auto &w : want)
        if (w.first->alloc(w.second) != hipSuccess) return false;
    if (hipMemset(sp.col.p, 0, sp.col.bytes) != hipSuccess) return false;  // no flags: no record is done
    sp.cap = n;
    sp.units = P;
    return true;
}

// Sample-parallel IOW-03: speculate every (pixel, sample) at once, then resolve / re-run the
// samples whose assumed incoming stack state was wrong (RT_SPEC_ITERS passes), and hand any
// pixel still unresolved to the sequential kernel from its first unresolved sample.  All
// launches are enqueued on `st`; counts stay on the device.
int launch_scene_spec(rt_dev_scene *s, rtk::Frame &f, hipStream_t st) {
    SpecState &sp = s->sp;
    const SeqWorkspace &ws = s->ws;
    const uint32_t P = rtk::units_of(f), S = uint32_t(s->s_stop);
    s->kt_used = 0;
    int rc = ensure_workspace(s, P);
    if (rc != RT_OK) return rc;
    const rt_options &o = s->opt;
    const int rounds = o.rounds_spec;
    const int iters = o.spec_iters;
    // A render of at most half the frame (one rank's tiles of a partition) has less parallel work
    // per sample chain, and its time becomes the longest dependent chain of its heaviest pixel
    // (north star): the automatic settings then spend more on the long samples,
    // twice the heavy-first indices and alternative runs from 2048 segments on (north-star 8-way
    // shares 5.87x -> 6.09x; whole frames keep (S - 1) / 20 and 16384: C2 +2.3% otherwise).
    const bool partial = uint64_t(P) * 2u <= uint64_t((f.W + 7) / 8 * 8) * uint64_t((f.H + 7) / 8 * 8);
    const int heavy_auto = int(S - 1) / (partial ? 10 : 20);
    const int alt_seg = o.spec_alt_seg > 0 ? o.spec_alt_seg : (partial ? 2048 : 16384);
    if ((rc = ensure_cont(s)) != RT_OK) return rc;
    // one pipeline for every pixel (a stream per pixel group measured slower: 8.8 s with 4 groups)
    if ((rc = ensure_lane(s, rtk::sort_pairs_temp_bytes((size_t(P) + 1) * S, 24))) != RT_OK) return rc;
    unsigned *sc = sp.counts.as<unsigned>();  // [0] list count, [16] fallback count
    rtk::SpecRecs R{sp.col.as<float4>(), sp.fin.as<float4>(), sp.ctr.as<uint4>(),
                          sp.assume.as<float4>(), P, S, sp.list.as<uint32_t>(), sc, sp.fb.as<uint32_t>(),
                          sc + 16, ws.order.as<uint32_t>(), 0, 0, sp.pstate.as<uint4>(), next_spec_epoch(s, st),
                          sp.front.as<uint4>(), sp.sorder.as<uint32_t>(),
                          uint32_t(o.spec_probe),
                          S > 2 ? uint32_t(std::min(int(S) - 2, o.spec_heavy >= 0 ? o.spec_heavy : heavy_auto)) : 0u};
    R.pmag = rtk::spec_pmag(P);
    sp.P = P;
    sp.S = S;
    sp.launch_seq = 0;
#ifdef RT_DIAG
    if (env_int("RT_DEBUG_TIMES", 0) != 0) {  // diagnostic builds only (rt_debug_spec_times)
        const size_t n = size_t(P) * S * 2 * sizeof(uint32_t);
        HIP_OK(sp.dbg_t.reserve(n));
        HIP_OK(hipMemsetAsync(sp.dbg_t.p, 0, n, st));
        R.dbg_start = sp.dbg_t.as<uint32_t>();
        R.dbg_end = R.dbg_start + size_t(P) * S;
        sp.dbg_n = size_t(P) * S;
    }
#endif
    const bool alt_on = o.spec_alt != 0 && s->iow.n_alt_vals > 1 && S > 1;
    if (alt_on) {  // alternative runs (DESIGN.md "Alternative runs")
        // slots pack as first | count << 24 in the hash (alt_find): the cap stays below 2^24
        const uint32_t cap = uint32_t(o.spec_alt_cap);
        if (sp.alt_cap != cap) {
            HIP_OK(sp.alt.alloc(size_t(cap) * sizeof(rtk::AltRec)));
            HIP_OK(sp.alt_hash.alloc(size_t(cap) * 2 * sizeof(uint2)));
            HIP_OK(sp.alt_count.alloc(64));
            sp.alt_cap = cap;
        }
        HIP_OK(hipMemsetAsync(sp.alt_hash.p, 0, size_t(cap) * 2 * sizeof(uint2), st));
        HIP_OK(hipMemsetAsync(sp.alt_count.p, 0, 64, st));
        R.alt = sp.alt.as<rtk::AltRec>();
        R.alt_hash = sp.alt_hash.as<uint2>();
        R.alt_count = sp.alt_count.as<unsigned>();
        R.alt_cap = cap;
        R.alt_hcap = cap * 2;
        R.alt_min_seg = uint32_t(alt_seg);
        for (int v = 0; v < 8; v++) R.alt_vals[v] = s->iow.alt_vals[v];
        R.n_alt_vals = s->iow.n_alt_vals;
    }
    // alternatives are spawned after the checkpoint rounds and, with spec_alt_every = k > 0,
    // after every k-th budgeted tail round too (measured: once is best on the bench frame)
    const int alt_every = o.spec_alt_every;
    R.front2 = sp.front.as<uint4>() + P;  // the anchored scan's secondary frontier
    R.scan_max = uint32_t(o.spec_scan);
    if (R.scan_max == 0) R.front2 = nullptr;
#ifdef RT_DIAG  // diagnostic builds only: copy one render's exact per-sample state into the next
    if (env_int("RT_SPEC_ORACLE", 0) != 0) {  // (see SpecRecs::exact)
        const size_t n = size_t(P) * S;
        if (sp.exact_n != n) {
            HIP_OK(sp.exact.alloc(n * sizeof(float4)));
            sp.exact_n = n;
            sp.exact_valid = false;
        }
        R.exact = sp.exact.as<float4>();
        R.exact_mode = 1 | (sp.exact_valid ? 2 : 0);
        sp.exact_valid = true;
    }
#endif
    const rtk::IowScene scene = iow_view(*s);
    // caps in 256-lane slots; the LDS-BVH kernels run 768-lane blocks
    const bool lds = rtk::iow_lds(scene);
    const int cap_s = s->cus * (lds ? 3 * rtk::resident_blocks_per_cu(rtk::RenderKernel::Iow03SpecLds)
                                     : rtk::resident_blocks_per_cu(rtk::RenderKernel::Iow03Spec));
    const int cap_q = s->cus * (lds ? 3 * rtk::resident_blocks_per_cu(rtk::RenderKernel::Iow03Lds)
                                     : rtk::resident_blocks_per_cu(rtk::RenderKernel::Iow03));
    hipError_t e = hipSuccess;
    const bool spread_last = o.spec_spread != 0;
    // one compacted pass (run_rounds) of the speculative kernel over n0 units on queue q
    auto spec_pass = [&](const RoundQueue &q, const rtk::SpecRecs &RR, int mode, uint32_t n0, uint32_t solo_first) {
        return run_rounds(q, rounds, n0, cap_s, park_min_of(s, cap_s), spread_last, solo_first,
                          [&](const rtk::Cont &ct, uint32_t n) {
                              return spec_launch(s, f, scene, RR, mode, ct, n, q.counter, cap_s, q.st);
                          });
    };
    // Checkpoint rounds (spec_rounds = k > 0): the speculative pass over samples 1.. runs as k
    // launches, each taking the lanes the previous one parked plus the next slice of fresh units
    // and parking every lane once its queue drains; between launches the pixel frontiers advance
    // and mispredicted samples at a frontier are re-run at once (k_iow03_frontier,
    // k_iow03_fixf).  The tail then runs as before (compaction rounds).
    const int ckpt = S > 1 ? std::min(kCountSlots - 16, o.spec_rounds) : 0;
    // Heavy-first (R.n_heavy = K > 0): round 0 runs every sample of every R.probe_stride-th pixel;
    // the measured cost per sample index orders the indices (k_sample_rank); the next rounds run
    // the K costliest indices for every pixel (sample-major, so the long samples start first);
    // the pixels are then re-sorted by the rays of those samples and the remaining indices run
    // pixel-major (so each heavy pixel's frontier reaches its long samples early).
    // Budgeted tail rounds (spec_tail_rounds, spec_tail_budget segments each; DESIGN.md
    // "Budgeted tail"): the frontier advances between them, so mispredicted samples re-run while
    // the long ones still run instead of in a re-run pass after them.
    // exact restarts go on down their pixel's chain of mispredicted samples (spec_chain)
    const int chain = o.spec_chain != 0 ? 1 : 0;
    const int tail_budgeted = ckpt > 0 ? std::max(0, std::min(kCountSlots - 16 - ckpt - rounds, o.spec_tail_rounds)) : 0;
    auto ckpt_pass = [&](const RoundQueue &q, const rtk::SpecRecs &RG, uint32_t n_fresh) {
        const uint32_t slots = uint32_t(s->blocks_cap) * rtk::kBlock, cap_cont = 2 * slots;
        struct Rnd { int mode; uint32_t lo, hi; };
        std::vector<Rnd> plan;
        const uint32_t n_px = RG.order_n ? RG.order_n : RG.P, K = RG.n_heavy;
        int r_heavy_end = -1;  // last round of the heavy phase
        if (K > 0 && ckpt >= 3) {
            const uint32_t n_probe = (n_px + RG.probe_stride - 1) / RG.probe_stride * (S - 1);
            plan.push_back({1, 0, n_probe});
            const int rest = ckpt - 1;
            const int ra = std::max(1, std::min(rest - 1, int(std::lround(double(rest) * K / (S - 1)))));
            const uint64_t nh = uint64_t(K) * n_px, nr = uint64_t(S - 1 - K) * n_px;
            for (int r = 0; r < ra; r++) plan.push_back({2, uint32_t(nh * r / ra), uint32_t(nh * (r + 1) / ra)});
            r_heavy_end = ra;
            for (int r = 0; r < rest - ra; r++)
                plan.push_back({3, uint32_t(nr * r / (rest - ra)), uint32_t(nr * (r + 1) / (rest - ra))});
        } else {
            for (int r = 0; r < ckpt; r++)
                plan.push_back({0, uint32_t(uint64_t(n_fresh) * r / ckpt), uint32_t(uint64_t(n_fresh) * (r + 1) / ckpt)});
        }
        for (int r = 0; r < ckpt && e == hipSuccess; r++) {
            rtk::Cont ct{};
            if (r > 0) { ct.in = q.buf(r - 1); ct.in_count = q.count(r - 1); }
            ct.out = q.buf(r);
            ct.out_count = q.count(r);
            ct.mixed = 1;
            ct.chain = chain;
            ct.park_below = 65;  // park every busy lane once the queue drains
            ct.fresh_mode = plan[size_t(r)].mode;
            ct.fresh_lo = plan[size_t(r)].lo;
            ct.fresh_hi = plan[size_t(r)].hi;
            if (r == ckpt - 1) ct.park_below = 0;  // the last round compacts as the tail rounds do
            ct.park_min = r == ckpt - 1 ? park_min_of(s, cap_s) : 0u;
            e = hipMemsetAsync(ct.out_count, 0, sizeof(unsigned), q.st);
            if (e == hipSuccess) e = spec_launch(s, f, scene, RG, rtk::kSpecRest, ct, uint32_t(cap_s) * rtk::kBlock,
                                                 q.counter, cap_s, q.st);
            if (e == hipSuccess) e = rtk::launch_iow03_frontier(f, RG, ct.out, ct.out_count, cap_cont, q.st);
            if (e == hipSuccess) e = rtk::launch_iow03_fixf(f, RG, ct.out, ct.out_count, int(cap_cont), q.st);
            if (e == hipSuccess && RG.alt && r == ckpt - 1)
                e = rtk::launch_iow03_altspawn(f, RG, ct.out, ct.out_count, cap_cont, q.st);
            if (e == hipSuccess && r == 0 && r_heavy_end > 0)
                e = rtk::launch_iow03_sample_order(f, RG, ct.out, ct.out_count, int(cap_cont),
                                                   sp.fcost.as<unsigned long long>(), sp.sorder.as<uint32_t>(), q.st);
            if (e == hipSuccess && r == r_heavy_end) {
                e = rtk::launch_iow03_pixel_key(f, RG, ct.out, ct.out_count, int(cap_cont), ws.cost.as<unsigned>(), q.st);
                if (e == hipSuccess)
                    e = rtk::sort_units_by_cost(ws.cost.as<unsigned>(), ws.keys.as<unsigned>(), ws.iota.as<unsigned>(),
                                                ws.order.as<unsigned>(), P, ws.temp.p, ws.temp_bytes, q.st);
            }
        }
        // tail: resume rounds with compaction, numbered on from the checkpoint rounds (so round r
        // reads what round r - 1 wrote); the first `tb` of them are budgeted (every unit parks
        // after spec_tail_budget segments) and followed by the frontier, so a sample found
        // mispredicted re-runs while the long samples are still running; the last round runs to
        // completion
        const uint32_t park_min = park_min_of(s, cap_s);
        const int tb = tail_budgeted;
        const uint32_t budget = uint32_t(o.spec_tail_budget);
        const int n_tail = tb + rounds;
        for (int t = 0; t <= n_tail && e == hipSuccess; t++) {
            const int r = ckpt + t;
            rtk::Cont ct{};
            ct.chain = chain;
            ct.in = q.buf(r - 1);
            ct.in_count = q.count(r - 1);
            if (t < n_tail) {
                ct.out = q.buf(r);
                ct.out_count = q.count(r);
                ct.park_min = park_min;
                if (t < tb) {
                    ct.seg_budget = budget;
                    if (spread_last) { ct.spread = 1; ct.park_min = 0xffffffffu; }  // no compaction parking
                }
                e = hipMemsetAsync(ct.out_count, 0, sizeof(unsigned), q.st);
            }
            if (t == n_tail && spread_last) ct.spread = 1;  // the last round: long samples get a wave each
            if (e == hipSuccess) e = spec_launch(s, f, scene, RG, rtk::kSpecRest, ct, uint32_t(cap_s) * rtk::kBlock,
                                                 q.counter, cap_s, q.st);
            if (e == hipSuccess && t < tb) {
                e = rtk::launch_iow03_frontier(f, RG, ct.out, ct.out_count, cap_cont, q.st);
                if (e == hipSuccess) e = rtk::launch_iow03_fixf(f, RG, ct.out, ct.out_count, int(cap_cont), q.st);
                if (e == hipSuccess && RG.alt && alt_every > 0 && t % alt_every == alt_every - 1)
                    e = rtk::launch_iow03_altspawn(f, RG, ct.out, ct.out_count, cap_cont, q.st);
            }
        }
    };
    {
        LastRender last;
        std::snprintf(last.kernel, sizeof(last.kernel), "%s", lds ? "k_iow03sL" : "k_iow03s");
        last.path.order = 4;
        last.path.iow_bvh = s->iow.root_link ? (lds ? 2 : 1) : 0;
        last.launches = (1 + rounds) * (1 + (S > 1 ? 1 : 0) + iters) + (ckpt > 0 ? ckpt + tail_budgeted : 0);
        last.chunks = 1;
        s->last = last;
    }
    // (1) sample 0 of every pixel (exact), the guesses for the other samples, and the pixel order
    // (heaviest sample 0 first), on the scene's queue
    const RoundQueue L0{st, s->counter.as<unsigned>(), ws.cont, ws.cont_count.as<unsigned>()};
    e = hipMemsetAsync(R.assume, 0, size_t(P) * sizeof(float4), st);
    if (e == hipSuccess) e = spec_pass(L0, R, rtk::kSpecFirst, P, 0);
    if (S > 1) {
        // Sample 1 starts from sample 0's final stack (exact: its written entries, 0 elsewhere).
        // From spec_prior_from (2) on every entry is guessed as the scene's most common RI
        // The prior misses far less often (the re-run pass re-traces ~1% of the rays instead of
        // ~20% with zeros); the dependent chains it forms are cheap for the validating pass.
        const uint32_t prior_from = uint32_t(o.spec_prior_from);
        if (e == hipSuccess)
            e = rtk::launch_iow03_prep(f, R, ws.cost.as<unsigned>(), s->iow.ri_prior, prior_from, st);
        if (e == hipSuccess)
            e = rtk::sort_units_by_cost(ws.cost.as<unsigned>(), ws.keys.as<unsigned>(), ws.iota.as<unsigned>(),
                                        ws.order.as<unsigned>(), P, ws.temp.p, ws.temp_bytes, st);
    }
    // (2) the pipeline, on the same stream with the lane's queue: speculative pass over samples
    // 1.., resolve and re-run passes (the first list longest first), final resolve, sequential
    // leftovers
    const bool sort_first = o.spec_sort != 0;
    const RoundQueue L{st, sp.lane_counter.as<unsigned>(), sp.lane_cont, sp.lane_cont_count.as<unsigned>()};
    rtk::SpecRecs RG = R;
    if (S > 1) RG.order_n = P;  // every pixel, in the sorted order
    const size_t nmax = size_t(P) * S;  // list bound
    if (S > 1 && e == hipSuccess) {
        if (ckpt > 0) ckpt_pass(L, RG, P * (S - 1));
        else e = spec_pass(L, RG, rtk::kSpecRest, P * (S - 1), 0);
    }
    for (int it = 0; it < iters && e == hipSuccess; it++) {
        e = hipMemsetAsync(RG.list_count, 0, sizeof(unsigned), st);
        if (e == hipSuccess) e = rtk::launch_iow03_resolve(f, RG, false, nullptr, st);
        if (it == 0 && sort_first && e == hipSuccess) {
            // the first re-execution list holds the long samples: run it longest first (LPT),
            // keyed by each sample's ray count in its speculative run
            unsigned *k1 = sp.keys.as<unsigned>(), *k2 = sp.keys2.as<unsigned>();
            uint32_t *l2 = sp.list2.as<uint32_t>();
            e = rtk::spec_list_keys(RG, k1, nmax, st);
            if (e == hipSuccess)
                e = rtk::sort_pairs_desc(k1, k2, RG.list, l2, nmax, sp.lane_temp.p, sp.lane_temp_bytes, 24, st);
            rtk::SpecRecs R2 = RG;
            R2.list = l2;
            if (e == hipSuccess) e = spec_pass(L, R2, rtk::kSpecList, uint32_t(nmax), uint32_t(o.spec_solo));
        } else if (e == hipSuccess) e = spec_pass(L, RG, rtk::kSpecList, uint32_t(nmax), 0);
    }
    if (e == hipSuccess) e = hipMemsetAsync(RG.fb_count, 0, sizeof(unsigned), st);
    if (e == hipSuccess) e = rtk::launch_iow03_resolve(f, RG, true, ws.state.as<float4>(), st);
    // leftovers: the sequential kernel from each pixel's first unresolved sample
    rtk::Chunk ch{};
    ch.s_begin = 0;
    ch.s_end = int(S);
    ch.final_chunk = 1;
    ch.state = ws.state.as<float4>();
    ch.order = RG.fb_list;
    ch.order_count = RG.fb_count;
    ch.per_unit_begin = 1;
    if (o.spec_validate != 0) {  // reuse the records that are still exact
        ch.rec_col = R.col; ch.rec_fin = R.fin; ch.rec_assume = R.assume; ch.rec_ctr = R.ctr;
        ch.rec_P = P;
        ch.rec_S = S;
    }
    if (e == hipSuccess)
        e = run_rounds(L, rounds, P, cap_q, park_min_of(s, cap_q), spread_last, 0,
                       [&](const rtk::Cont &ct, uint32_t n) {
                           return rtk::launch_iow03(f, scene, ch, ct, n, L.counter, s->s_stop, cap_q, st);
                       });
    return e == hipSuccess ? RT_OK : launch_failed(e);
}
