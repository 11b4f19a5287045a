// rt_iow_spec.hip -- the sample-parallel IOW-03 render for gfx950 (DESIGN.md "Sample-parallel
// speculation"): the bulk pass k_iow03s / k_iow03sL, alternative runs, the checkpoint rounds
// (frontier, altspawn, fixf), the resolve, the heavy-first ordering kernels, and their launches.
// The segment step is the sequential kernels' (rt_iow_coop.hpp).
#include "rt_render_common.hpp"
#include "rt_iow_coop.hpp"

namespace rtk {

// ============================================================================ IOW-03, sample-parallel
// One unit = one sample of one pixel (u = s*P + pu), so a heavy pixel's samples run on many
// lanes at once instead of one after another.  Exactness: a sample's result is a function of
// the pixel, the sample index and the RI left in stack entries 1..3 by the samples before it
// (entry 0 is always written before any read).  The sample runs with an assumed value for
// those entries (zeros in the first pass, else what the last resolve computed) and records
// which entries it read before writing (rmask) and which it wrote (wmask); the resolve replays
// the pixel in sample order and re-queues exactly the samples whose assumption was wrong.
// ---------------------------------------------------------------- alternative runs
// The slots (first, count) of unit u's alternative runs; count 0: none.  Open addressing over
// alt_hcap entries, key u + 1.
__device__ __forceinline__ uint2 alt_find(const SpecRecs &R, uint32_t u) {
    if (!R.alt_hash) return make_uint2(0u, 0u);
    uint32_t h = (u * 2654435761u) % R.alt_hcap;
    for (uint32_t i = 0; i < R.alt_hcap; i++) {
        const uint2 e = R.alt_hash[h];
        if (e.x == 0u) break;
        if (e.x == u + 1u) return make_uint2(e.y & 0xffffffu, e.y >> 24);
        h = h + 1u == R.alt_hcap ? 0u : h + 1u;
    }
    return make_uint2(0u, 0u);
}
// A finished alternative run of u (finished in a launch other than `launch`, whose records are
// stable) whose assumption holds on the entries it read under the exact state E: copied into
// u's records, which then read as a finished exact execution (flags tagged with `tag_launch`).
// Returns its slot + 1, or 0.
__device__ uint32_t alt_adopt(const SpecRecs &R, uint32_t u, uint32_t E1, uint32_t E2, uint32_t E3, uint32_t launch,
                              uint32_t tag_launch) {
    const uint2 fk = alt_find(R, u);
    for (uint32_t i = 0; i < fk.y; i++) {
        const AltRec &A = R.alt[fk.x + i];
        const uint32_t st = __hip_atomic_load(&A.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st == 0u || st == launch + 1u || A.u != u) continue;  // (A.u: a record of this unit only)
        const unsigned fl = __float_as_uint(A.col.w), rm = fl & 15u;
        if (((rm & 2u) && __float_as_uint(A.assume.x) != E1) || ((rm & 4u) && __float_as_uint(A.assume.y) != E2) ||
            ((rm & 8u) && __float_as_uint(A.assume.z) != E3))
            continue;
        R.assume[R.ix(u)] = A.assume;
        R.fin[R.ix(u)] = A.fin;
        R.ctr[R.ix(u)] = A.ctr;
        R.col[R.ix(u)] = make_float4(A.col.x, A.col.y, A.col.z,
                               __uint_as_float((fl & ~(63u << 10)) | ((tag_launch & 63u) << 10)));
        return fk.x + i + 1u;
    }
    return 0u;
}

template <bool NARROW, int SUB, bool LN>
__device__ __forceinline__ void iow03s_body(const Frame &f, const IowScene &S, const SpecRecs &R, int mode,
                                            const Cont &ct, unsigned *counter) {
    using Stack = IowStack<NARROW>;
    using Cfg = IowCfg<NARROW, SUB, LN>;
    constexpr int kFl = kIowStack * Stack::kSlot;
    constexpr int BCAP = Cfg::BS - 3;
    __shared__ float lds[SUB * kFl * kBlock];
    __shared__ unsigned char lds_b[NARROW ? SUB * kIowStack * kBlock : 1];
    __shared__ short lds_bvh[SUB * Cfg::BS * kBlock];
    __shared__ unsigned long long s_dbg[SUB * kBlock / 64][kDbgSlots];
    __shared__ float4 s_nodes[LN ? kIowLdsNodes * 7 : 1];
    const int sb = (int)(threadIdx.x / kBlock), tl = (int)(threadIdx.x % kBlock);
    short *bstk = lds_bvh + sb * Cfg::BS * kBlock + tl;  // bslot's layout
    const float4 *nodes = iow_stage_nodes<LN>(S, s_nodes);
    Ctr c;  // per unit here: written to the unit's record, never flushed
    if (f.dbg) {
        c.wdbg = s_dbg[threadIdx.x >> 6];
        if ((threadIdx.x & 63) < kDbgSlots) c.wdbg[threadIdx.x & 63] = 0;
    }
    Stack K{lds + sb * kFl * kBlock + tl, lds_b + (NARROW ? sb * kIowStack * kBlock + tl : 0), 0};
    // units: the parked lanes of ct.in first, then fresh units of the mode ([fresh_lo, fresh_hi)
    // in a mixed launch; all of them in a first launch; none in a plain resume launch)
    const uint32_t nin = ct.in ? *ct.in_count : 0u;
    const uint32_t f_lo = ct.mixed ? ct.fresh_lo : 0u;
    const uint32_t f_n = ct.mixed ? ct.fresh_hi - ct.fresh_lo
                       : (ct.in ? 0u : (mode == kSpecList ? *R.list_count
                                                          : (mode == kSpecFirst ? R.P : R.order_n * (R.S - 1))));
    const uint32_t total = nin + f_n;
    const bool may_park = ct.out != nullptr && total >= ct.park_min;
    const int park_below = ct.park_below ? ct.park_below : kParkBelow;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t wcap = ct.spread ? max(1u, (total + n_waves - 1u) / n_waves) : 64u;
    const int W = f.W, H = f.H, spp = f.spp;
    int grid = 1;
    while (grid * grid < spp) grid++;
    const float aspect = (float)W * rcp((float)H);
    const float dsx = iow_px_dsx(aspect, W, grid);
    const float dsy = iow_px_dsy(H, grid);
    bool live = true, busy = false;
    bool solo = false;  // wave-uniform: the wave holds one unit from the sorted head
    const uint32_t solo_n = min(min(ct.solo_n, n_waves), total);
    bool solo_open = solo_n != 0;  // wave-uniform: the queue head may still be below solo_n
    uint32_t u = 0, urays = 0;
    int skip = 0;
    f3 sample = f3{0, 0, 0};
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    const unsigned started_tag = (1u << 9) | ((R.epoch & 0xffffu) << 16);  // heavy-first: taken, unfinished
    uint32_t useg = 0;  // segments of the current unit in this launch (ct.seg_budget)
    // exact: the unit was (re)started with its exact incoming state (a frontier or fixf restart),
    // so the state after it is exact too and the lane may go on down its pixel's chain
    bool exact = false;
    uint32_t alt_slot = 0;  // an alternative run: its slot + 1 (its record goes to R.alt)
    // the lane's state at a segment boundary -> a continuation slot (13 float4)
    auto park = [&](float4 *p) {
        p[0] = make_float4(ubits(u), ibits(skip), ibits(K.size), ubits(K.wmask | (K.rmask << 4)));
        p[1] = make_float4(sample.x, sample.y, sample.z, ubits(urays));
        p[2] = make_float4(ubits(c.seg), ubits(c.nodes), ubits(c.prims), ubits(c.drops));
        // .y: restart flag (k_iow03_fixf), .z: exact, .w: alternative slot + 1 (bits)
        p[12] = make_float4(ubits(c.nans), 0.0f, exact ? 1.0f : 0.0f, ubits(alt_slot));
        float *fl = reinterpret_cast<float *>(p + 3);
        for (int k = 0; k < kFl; k++) fl[k] = K.base[k * kBlock];
        if constexpr (NARROW)
            for (int e = 0; e < kIowStack; e++) fl[kFl + e] = ibits(K.bounced(e));
    };
    // start unit u (sample s of pixel pu) with assumed stack RI a.xyz in entries 1..3
    auto begin = [&](uint32_t u_, float4 a) {
        u = u_;
#ifdef RT_DIAG
        if (R.dbg_start) R.dbg_start[u] = (ct.launch_id & 0xffffu) | ((R.dbg_start[u] >> 16) + 1u) << 16;
#endif
        const uint32_t pu = u % R.P;
        const int s = (int)(u / R.P);
        const UnitPix px = unit_pixel(f, pu);
        busy = true;
        c.seg = c.nodes = c.prims = c.drops = c.nans = 0;
        urays = 0;
        useg = 0;
        skip = 0;
        sample = f3{0, 0, 0};
        K.size = 0; K.wmask = 0; K.rmask = 0;
        K.at(0, 7) = 0.0f; K.at(1, 7) = a.x; K.at(2, 7) = a.y; K.at(3, 7) = a.z;
        const float sx = iow_px_sx(aspect, px.x, W);
        const float sy = iow_px_sy(px.y, H);
        f3 ro, rd;
        iow_camera_ray(S, f, sx, sy, dsx, dsy, s, ro, rd);
        if (f.show_normal) {  // one ray, no stack: the normal is the sample
            sample = iow_launch_ray<BCAP, Cfg::NS>(S, f, ro, rd, 32000.0f, 1.0f, c, bstk, nodes).normal;
            urays = 1;
        } else K.push(ro, rd, 1.0f, 1.0f, 0, c);
    };
    for (;;) {
        // spread: a wave holds at most wcap units, so a few long samples get a wave each (and the
        // wave-cooperative closest hits) instead of sharing one
        bool want = live && !busy;
        if (wcap < 64u) {
            const int room = (int)wcap - __popcll(__ballot(busy));
            want = want && (int)lanes_below(__ballot(want)) < room;
        }
        // solo head: the queue is read only while this wave has not yet seen it pass solo_n (the
        // counter only grows), so the check costs a load per wave at the start of a launch
        if (solo) {
            if (__ballot(busy) != 0) want = false;  // keep the head unit alone
            else solo = false;
        }
        if (!solo && solo_open && __ballot(want) != 0) {
            const uint32_t head = __builtin_amdgcn_readfirstlane(__hip_atomic_load(
                counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (head >= solo_n) solo_open = false;
            else want = want && __ballot(busy) == 0 && lanes_below(__ballot(want)) == 0;
        }
        const uint32_t q = fetch_unit(counter, want);
        if (solo_open && __ballot(want && q < solo_n) != 0) solo = true;
        if (want) {
            if (q >= total) live = false;
            else if (q < nin && ct.in[(size_t)q * kContSlots + 12].y == 3.0f) {  // an alternative run
                const uint32_t slot = __float_as_uint(ct.in[(size_t)q * kContSlots + 12].z);
                u = __float_as_uint(ct.in[(size_t)q * kContSlots].x);
                begin(u, R.alt[slot].assume);
                exact = false;
                alt_slot = slot + 1u;
            } else if (q < nin && ct.in[(size_t)q * kContSlots + 12].y != 0.0f) {  // doomed while parked: restart exact
                u = __float_as_uint(ct.in[(size_t)q * kContSlots].x);
                begin(u, R.assume[R.ix(u)]);
                exact = ct.chain != 0;
                alt_slot = 0;
            } else if (q < nin) {  // resume a parked lane
                const float4 *p = ct.in + (size_t)q * kContSlots;
                const float4 m = p[0], a = p[1], b = p[2];
                u = __float_as_uint(m.x); skip = __float_as_int(m.y); K.size = __float_as_int(m.z);
                K.wmask = __float_as_uint(m.w) & 15u; K.rmask = __float_as_uint(m.w) >> 4;
                sample = f3{a.x, a.y, a.z}; urays = __float_as_uint(a.w);
                c.seg = __float_as_uint(b.x); c.nodes = __float_as_uint(b.y); c.prims = __float_as_uint(b.z);
                c.drops = __float_as_uint(b.w); c.nans = __float_as_uint(p[12].x);
                exact = p[12].z != 0.0f;
                alt_slot = __float_as_uint(p[12].w);
                const float *fl = reinterpret_cast<const float *>(p + 3);
                for (int k = 0; k < kFl; k++) K.base[k * kBlock] = fl[k];
                if constexpr (NARROW)
                    for (int e = 0; e < kIowStack; e++) K.set_bounced(e, __float_as_int(fl[kFl + e]));
                useg = 0;
                busy = true;
            } else {
                // kSpecFirst: sample 0 of every pixel; kSpecRest: samples 1.. pixel-major, pixels
                // in R.order (heaviest sample 0 first); kSpecList: the re-execution list
                const uint32_t qf = f_lo + (q - nin);
                bool fresh = true;
                if (ct.fresh_mode == 0) {
                    u = mode == kSpecList ? R.list[qf]
                        : (mode == kSpecFirst ? qf : (1u + qf % (R.S - 1)) * R.P + R.order[R.order_base + qf / (R.S - 1)]);
                } else {  // heavy-first enumerations of kSpecRest (a unit may come up twice: run it once)
                    const uint32_t n_px = R.order_n ? R.order_n : R.P, nr = R.S - 1u - R.n_heavy;
                    uint32_t s_, rank;
                    if (ct.fresh_mode == 1) { rank = (qf / (R.S - 1u)) * R.probe_stride; s_ = 1u + qf % (R.S - 1u); }
                    else if (ct.fresh_mode == 2) { s_ = R.sorder[qf / n_px]; rank = qf % n_px; }
                    else { s_ = R.sorder[R.n_heavy + qf % nr]; rank = qf / nr; }
                    u = s_ * R.P + R.order[R.order_base + rank];
                    const uint32_t tag = __float_as_uint(R.col[R.ix(u)].w);
                    fresh = !((tag >> 16) == (R.epoch & 0xffffu) && (tag & 0x300u) != 0u);
                }
                if (fresh && unit_pixel(f, u % R.P).in_image) {
                    if (ct.fresh_mode != 0) R.col[R.ix(u)].w = ubits(started_tag);
                    begin(u, mode == kSpecFirst ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : R.assume[R.ix(u)]);
                    exact = false;
                    alt_slot = 0;
                }
            }
        }
        if (__ballot(live) == 0) break;
        if (may_park && __ballot(!live) != 0 && __popcll(__ballot(busy)) < park_below) {
            const uint32_t slot = park_slot(ct.out_count, busy);
            if (busy) park(ct.out + (size_t)slot * kContSlots);
            break;
        }
        DBG_TALLY(f, c, kDbgOuter, busy);
        DBG_TALLY(f, c, kDbgSeg, busy && K.size > 0);
        DBG_T0(f, t_seg);
        {
            const bool seg = busy && K.size > 0;
            iow_seg_step<NARROW, Cfg::BS, Cfg::NS>(S, f, K, skip, sample, (int)(u / R.P), c, bstk, nodes, seg);
            if (seg) { urays++; useg++; }
        }
        DBG_CYC(f, c, kDbgCycSeg, t_seg);
        if (ct.seg_budget) {  // budgeted round: a unit that used its segments parks (per lane)
            const bool over = busy && K.size > 0 && useg >= ct.seg_budget;
            if (__ballot(over) != 0) {
                const uint32_t slot = park_slot(ct.out_count, over);
                if (over) { park(ct.out + (size_t)slot * kContSlots); busy = false; }
            }
        }
        if (busy && K.size == 0 && alt_slot) {  // an alternative run done: its own record
            AltRec &A = R.alt[alt_slot - 1u];
            A.col = make_float4(sample.x, sample.y, sample.z, ubits(K.rmask | (K.wmask << 4) | done_tag));
            A.fin = make_float4(K.at(1, 7), K.at(2, 7), K.at(3, 7), ubits(c.prims));
            A.ctr = make_uint4(c.seg, c.drops, c.nans, c.nodes);
            __threadfence();
            __hip_atomic_store(&A.state, ct.launch_id + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            busy = false;
            alt_slot = 0;
        }
        if (busy && K.size == 0) {  // sample done: record it
            R.col[R.ix(u)] = make_float4(sample.x, sample.y, sample.z,
                                   ubits(K.rmask | (K.wmask << 4) | done_tag | ((ct.launch_id & 63u) << 10)));
            R.fin[R.ix(u)] = make_float4(K.at(1, 7), K.at(2, 7), K.at(3, 7), ubits(c.prims));
            R.ctr[R.ix(u)] = make_uint4(c.seg, c.drops, c.nans, c.nodes);
#ifdef RT_DIAG
            if (R.dbg_end) R.dbg_end[u] = ct.launch_id;
#endif
            busy = false;
            if (exact) {
                // Chain following: the stack this exact sample left is the exact incoming state of
                // the next sample.  Walk the pixel's following finished samples while their
                // assumptions hold on the entries they read; re-run the first one that does not,
                // here and now, with the exact state.  A pixel whose samples all mispredict (each
                // reads the entry its predecessor wrote) then runs down its chain on one lane,
                // not one sample per frontier round.  Stops at an unfinished sample (running or
                // queued elsewhere), which the frontier handles.
                // Other lanes of this launch may write these records, so only records finished in
                // an earlier launch (stable since that kernel boundary) are read, with
                // device-coherent loads; a record is claimed for a re-run by a compare-and-swap of
                // its flags, and a read whose flags changed meanwhile stops the walk.
                const uint32_t pu = u % R.P;
                uint32_t E1 = __float_as_uint(K.at(1, 7)), E2 = __float_as_uint(K.at(2, 7)),
                         E3 = __float_as_uint(K.at(3, 7));
                auto ld = [](const float *p) {
                    return __hip_atomic_load(reinterpret_cast<const unsigned *>(p), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
                };
                for (uint32_t t = u / R.P + 1u; t < R.S; t++) {
                    const uint32_t v = t * R.P + pu;
                    unsigned *flp = reinterpret_cast<unsigned *>(&R.col[R.ix(v)].w);
                    const unsigned fl = ld(&R.col[R.ix(v)].w);
                    if ((fl & 0xffff0100u) != done_tag || ((fl >> 10) & 63u) == (ct.launch_id & 63u)) break;
                    const unsigned rm = fl & 15u, wm = (fl >> 4) & 15u;
                    const unsigned a1 = ld(&R.assume[R.ix(v)].x), a2 = ld(&R.assume[R.ix(v)].y), a3 = ld(&R.assume[R.ix(v)].z);
                    const unsigned f1 = ld(&R.fin[R.ix(v)].x), f2 = ld(&R.fin[R.ix(v)].y), f3v = ld(&R.fin[R.ix(v)].z);
                    __atomic_thread_fence(__ATOMIC_ACQUIRE);
                    if (ld(&R.col[R.ix(v)].w) != fl) break;
                    if (((rm & 2u) && a1 != E1) || ((rm & 4u) && a2 != E2) || ((rm & 8u) && a3 != E3)) {
                        unsigned expect = fl;
                        if (!__hip_atomic_compare_exchange_strong(flp, &expect, started_tag, __ATOMIC_ACQ_REL,
                                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                            break;
                        const uint32_t got = alt_adopt(R, v, E1, E2, E3, ct.launch_id, ct.launch_id);
                        if (got) {  // an alternative run already holds its exact execution
                            const AltRec &A = R.alt[got - 1u];
                            const unsigned awm = (__float_as_uint(A.col.w) >> 4) & 15u;
                            if (awm & 2u) E1 = __float_as_uint(A.fin.x);
                            if (awm & 4u) E2 = __float_as_uint(A.fin.y);
                            if (awm & 8u) E3 = __float_as_uint(A.fin.z);
                            continue;
                        }
                        const float4 e = make_float4(__uint_as_float(E1), __uint_as_float(E2), __uint_as_float(E3), 0.0f);
                        R.assume[R.ix(v)] = e;
                        begin(v, e);
                        break;
                    }
                    if (wm & 2u) E1 = f1;
                    if (wm & 4u) E2 = f2;
                    if (wm & 8u) E3 = f3v;
                }
                exact = busy;
            }
        }
    }
    if (c.wdbg && (threadIdx.x & 63) == 0)
        for (int i = 0; i < kDbgSlots; i++) atomicAdd(f.dbg + i, c.wdbg[i]);
}

__global__ __launch_bounds__(kBlock) void k_iow03s(Frame f, IowScene S, SpecRecs R, int mode, Cont ct,
                                                   unsigned *counter) {
    iow03s_body<false, 1, false>(f, S, R, mode, ct, counter);
}
__global__ __launch_bounds__(3 * kBlock) void k_iow03sL(Frame f, IowScene S, SpecRecs R, int mode, Cont ct,
                                                        unsigned *counter) {
    iow03s_body<false, 3, true>(f, S, R, mode, ct, counter);
}

// After the sample-0 pass: every later sample of a pixel assumes, for each stack entry 1..3,
// the RI sample 0 left there, or `prior` where sample 0 never wrote it (a guess, checked by
// the resolve; `prior` is the scene's most common refractive index, the value such entries
// almost always hold once any sample has pushed there).  Pixels are keyed by sample 0's ray
// count so the rest run heaviest first.
__global__ __launch_bounds__(kBlock) void k_iow03_prep(Frame f, SpecRecs R, unsigned *key, float prior,
                                                       uint32_t prior_from) {
    const uint32_t pu = blockIdx.x * kBlock + threadIdx.x;
    if (pu >= R.P) return;  // no cross-lane work in this kernel
    const UnitPix px = unit_pixel(f, pu);
    if (!px.in_image) { key[pu] = 0; return; }
    const uint32_t wm = (__float_as_uint(R.col[R.ix(pu)].w) >> 4) & 15u;
    const float4 fn = R.fin[R.ix(pu)];
    const float4 e0 = make_float4((wm & 2u) ? fn.x : 0.0f, (wm & 4u) ? fn.y : 0.0f, (wm & 8u) ? fn.z : 0.0f, 0.0f);
    // From prior_from on every entry is guessed as the prior: sample 0 starts from the all-zero
    // stack no later sample sees (a stale 0 makes target_RI 0 and forces TIR, 03...glsl:316-327),
    // so the values it leaves are a worse guess of the steady state than the scene's most common
    // RI (tests/analysis/fork_stats.py: mispredicted rays 2.6% -> 0.8% on C2).
    const float4 e1 = make_float4(prior, prior, prior, 0.0f);
    for (uint32_t s = 1; s < R.S; s++) R.assume[R.ix((size_t)s * R.P + pu)] = s >= prior_from ? e1 : e0;
#ifdef RT_DIAG
    if (R.exact && (R.exact_mode & 2))
        for (uint32_t s = 1; s < R.S; s++) R.assume[R.ix((size_t)s * R.P + pu)] = R.exact[(size_t)s * R.P + pu];
#endif
    if (R.front)  // sample 0 is exact: the frontier starts at sample 1 with its final entries
        R.front[pu] = make_uint4(1u, __float_as_uint(e0.x), __float_as_uint(e0.y), __float_as_uint(e0.z));
    if (R.front2) R.front2[pu] = make_uint4(0xffffffffu, 0u, 0u, 0u);
    key[pu] = R.ctr[R.ix(pu)].x;
}

// ---------------------------------------------------------------- checkpoint rounds
// Between the rounds of the speculative pass (kernel boundaries, so every finished record is
// visible), each pixel's frontier advances over its finished samples in sample order while
// their assumptions match the exact state E.  The first finished sample whose assumption was
// wrong gets E and is queued at once for an exact re-run in the next round (its record is
// marked unfinished until then), so a mispredicted sample -- long ones especially -- is re-run
// while the pass still has other work, not in a re-execution pass after it.  Samples behind the
// frontier keep speculating; the resolve after the pass checks everything again.
__global__ __launch_bounds__(kBlock) void k_iow03_frontier(Frame f, SpecRecs R, float4 *cont, unsigned *count,
                                                           uint32_t cap) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = R.order_n ? R.order_n : R.P;
    if (i >= n) return;  // no cross-lane work in this kernel
    const uint32_t pu = R.order_n ? R.order[R.order_base + i] : i;
    if (!unit_pixel(f, pu).in_image) return;
    uint4 st = R.front[pu];
    if (st.x >= R.S) return;
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    // queue sample u for an exact re-run with incoming state E (its record is marked unfinished)
    auto requeue = [&](size_t u, uint32_t e1, uint32_t e2, uint32_t e3) {
        const uint32_t slot = atomicAdd(count, 1u);
        if (slot >= cap) { atomicSub(count, 1u); return; }  // full: leave it to the resolve after the pass
        R.assume[R.ix(u)] = make_float4(__uint_as_float(e1), __uint_as_float(e2), __uint_as_float(e3), 0.0f);
        R.col[R.ix(u)].w = __uint_as_float((1u << 9) | ((R.epoch & 0xffffu) << 16));  // queued: unfinished
        float4 *p = cont + (size_t)slot * kContSlots;
        p[0] = make_float4(__uint_as_float((uint32_t)u), 0.0f, 0.0f, 0.0f);
        p[12] = make_float4(0.0f, 1.0f, 0.0f, 0.0f);  // restart with the (now exact) assumption
    };
    uint32_t s = st.x;
    bool queued = false;
    for (; s < R.S; s++) {
        const size_t u = (size_t)s * R.P + pu;
        unsigned fl = __float_as_uint(R.col[R.ix(u)].w);
        if ((fl & 0xffff0100u) != done_tag) {  // still running (or queued): an alternative may hold it
            if (!R.alt || !alt_adopt(R, (uint32_t)u, st.y, st.z, st.w, 0xffffffffu, 0u)) break;
            fl = __float_as_uint(R.col[R.ix(u)].w);
        }
        const float4 a = R.assume[R.ix(u)];
        const unsigned rm = fl & 15u, wm = (fl >> 4) & 15u;
        if (((rm & 2u) && __float_as_uint(a.x) != st.y) || ((rm & 4u) && __float_as_uint(a.y) != st.z) ||
            ((rm & 8u) && __float_as_uint(a.z) != st.w)) {
            if (R.alt && alt_adopt(R, (uint32_t)u, st.y, st.z, st.w, 0xffffffffu, 0u)) {
                fl = __float_as_uint(R.col[R.ix(u)].w);  // the adopted alternative is exact: go on
            } else {
                requeue(u, st.y, st.z, st.w);
                queued = true;
                break;
            }
        }
        const unsigned wm2 = (fl >> 4) & 15u;
        (void)wm;
        const float4 fn = R.fin[R.ix(u)];
        if (wm2 & 2u) st.y = __float_as_uint(fn.x);
        if (wm2 & 4u) st.z = __float_as_uint(fn.y);
        if (wm2 & 8u) st.w = __float_as_uint(fn.z);
    }
    st.x = s;
    R.front[pu] = st;
    // Anchored scan past the blocked sample s.  A finished sample that read no entry it had not
    // written (rmask 0) is exact whatever came before it, and so are the entries it wrote; a
    // finished sample whose reads are all of known entries is exact if its assumption matches
    // them.  Knowledge of entries 1..3 is tracked from s + 1 on (none known at first); once all
    // three are known, a mispredicted finished sample is re-queued at once with the exact state,
    // and the first unfinished one is handed to k_iow03_fixf (front2).  The scan goes on past
    // unfinished and mispredicted samples (knowledge restarts at the next anchor) up to
    // scan_max samples past the frontier.  So a misprediction
    // behind a long running sample is repaired without waiting for that sample (anchors --
    // samples with rmask 0 that write all three entries -- are 18% of the samples of the bench
    // scene, tests/analysis/fork_stats.py).
    if (!R.front2) return;
    uint4 f2 = make_uint4(0xffffffffu, 0u, 0u, 0u);
    if (!queued && s < R.S) {
        unsigned known = 0;
        uint32_t E[4] = {0u, 0u, 0u, 0u};
        const uint32_t k_end = min(R.S, s + 1u + R.scan_max);
        for (uint32_t k = s + 1u; k < k_end; k++) {
            const size_t u = (size_t)k * R.P + pu;
            const unsigned fl = __float_as_uint(R.col[R.ix(u)].w);
            if ((fl & 0xffff0100u) != done_tag) {  // unfinished: fixf may patch the first one
                if (known == 14u && f2.x == 0xffffffffu) f2 = make_uint4(k, E[1], E[2], E[3]);
                known = 0;  // its outputs are unknown; later anchors restore knowledge
                continue;
            }
            const unsigned rm = fl & 14u, wm = (fl >> 4) & 14u;
            if (rm & ~known) { known &= ~wm; continue; }  // read an unknown entry: its writes are unknown
            const float4 a = R.assume[R.ix(u)];
            const bool bad = ((rm & 2u) && __float_as_uint(a.x) != E[1]) ||
                             ((rm & 4u) && __float_as_uint(a.y) != E[2]) ||
                             ((rm & 8u) && __float_as_uint(a.z) != E[3]);
            unsigned wmx = wm;
            if (bad) {  // mispredicted: adopt an alternative, or re-run it now if the whole state is known
                if (known == 14u && R.alt && alt_adopt(R, (uint32_t)u, E[1], E[2], E[3], 0xffffffffu, 0u)) {
                    wmx = (__float_as_uint(R.col[R.ix(u)].w) >> 4) & 14u;
                } else {
                    if (known == 14u) requeue(u, E[1], E[2], E[3]);
                    known = 0;
                    continue;
                }
            }
            const float4 fn = R.fin[R.ix(u)];
            if (wmx & 2u) E[1] = __float_as_uint(fn.x);
            if (wmx & 4u) E[2] = __float_as_uint(fn.y);
            if (wmx & 8u) E[3] = __float_as_uint(fn.z);
            known |= wmx;
        }
    }
    R.front2[pu] = f2;
}
// Alternative runs (RT_SPEC_ALT, between tail rounds): for each pixel, every finished sample
// past the frontier that read exactly one stale entry before writing it, traced at least
// alt_min_seg segments and has no alternatives yet gets one run per other value that entry can
// hold (R.alt_vals), queued as restart records with flag 3.  Such a sample is where a dependent
// chain forms: if its guess was wrong, the frontier adopts the matching alternative instead of
// re-running a long sample once the samples before it are done.
__global__ __launch_bounds__(kBlock) void k_iow03_altspawn(Frame f, SpecRecs R, float4 *cont, unsigned *count,
                                                           uint32_t cap) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = R.order_n ? R.order_n : R.P;
    if (i >= n) return;  // no cross-lane work in this kernel
    const uint32_t pu = R.order_n ? R.order[R.order_base + i] : i;
    if (!unit_pixel(f, pu).in_image) return;
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    for (uint32_t s = R.front[pu].x; s < R.S; s++) {
        const uint32_t u = s * R.P + pu;
        const unsigned fl = __float_as_uint(R.col[R.ix(u)].w);
        if ((fl & 0xffff0100u) != done_tag) continue;
        const unsigned rm = fl & 14u;
        if (rm == 0u || (rm & (rm - 1u)) != 0u) continue;  // exactly one stale entry read
        if (R.ctr[R.ix(u)].x < R.alt_min_seg) continue;
        if (alt_find(R, u).y != 0u) continue;
        const int e = rm == 2u ? 0 : (rm == 4u ? 1 : 2);
        const float4 a = R.assume[R.ix(u)];
        const float ae = e == 0 ? a.x : (e == 1 ? a.y : a.z);
        uint32_t k = 0;
        for (int v = 0; v < R.n_alt_vals; v++) k += __float_as_uint(R.alt_vals[v]) != __float_as_uint(ae);
        if (k == 0u) continue;
        const uint32_t first = atomicAdd(R.alt_count, k);
        if (first + k > R.alt_cap) { atomicSub(R.alt_count, k); return; }
        const uint32_t slot = atomicAdd(count, k);
        if (slot + k > cap) { atomicSub(count, k); return; }  // leaves the claimed alt slots unused
        uint32_t j = 0;
        for (int v = 0; v < R.n_alt_vals; v++) {
            if (__float_as_uint(R.alt_vals[v]) == __float_as_uint(ae)) continue;
            AltRec &A = R.alt[first + j];
            A.u = u;
            A.state = 0u;
            float4 b = a;
            if (e == 0) b.x = R.alt_vals[v]; else if (e == 1) b.y = R.alt_vals[v]; else b.z = R.alt_vals[v];
            A.assume = b;
            float4 *p = cont + (size_t)(slot + j) * kContSlots;
            p[0] = make_float4(__uint_as_float(u), 0.0f, 0.0f, 0.0f);
            p[12] = make_float4(0.0f, 3.0f, __uint_as_float(first + j), 0.0f);  // start an alternative run
            j++;
        }
        // publish u -> (first, k) in the hash (open addressing, key u + 1)
        uint32_t h = (u * 2654435761u) % R.alt_hcap;
        for (uint32_t t = 0; t < R.alt_hcap; t++) {
            const unsigned prev = atomicCAS(&R.alt_hash[h].x, 0u, u + 1u);
            if (prev == 0u) { R.alt_hash[h].y = first | (k << 24); break; }
            h = h + 1u == R.alt_hcap ? 0u : h + 1u;
        }
    }
}

// Parked samples at their pixel's frontier: the exact incoming state E is known.  Entries the
// sample neither read nor wrote get E (exact: it would have started with them); if an entry it
// already read differs from E it restarts with E.  Either way its assumption becomes exact, so
// long samples stop waiting for a later resolve pass to find them wrong.
__global__ __launch_bounds__(kBlock) void k_iow03_fixf(Frame f, SpecRecs R, float4 *cont, const unsigned *count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= *count) return;  // no cross-lane work in this kernel
    float4 *p = cont + (size_t)i * kContSlots;
    if (p[12].y != 0.0f || __float_as_uint(p[12].w) != 0u) return;  // a restart already / an alternative run
    const uint32_t u = __float_as_uint(p[0].x);
    const uint32_t pu = u % R.P, s = u / R.P;
    uint4 st = R.front[pu];
    if (st.x != s) {  // not at the frontier: past it, its exact state may come from the anchored scan
        if (!R.front2) return;
        st = R.front2[pu];
        if (st.x != s) return;
    }
    const unsigned E[3] = {st.y, st.z, st.w};
    const unsigned masks = __float_as_uint(p[0].w), wm = masks & 15u, rm = masks >> 4;
    float4 a = R.assume[R.ix(u)];
    float *av = &a.x;
    bool doomed = false;
    for (int k = 1; k <= 3; k++)
        if (((rm >> k) & 1u) && __float_as_uint(av[k - 1]) != E[k - 1]) doomed = true;
    if (doomed) {
        R.assume[R.ix(u)] = make_float4(__uint_as_float(E[0]), __uint_as_float(E[1]), __uint_as_float(E[2]), 0.0f);
        p[12].y = 1.0f;
        return;
    }
    float *fl = reinterpret_cast<float *>(p + 3);  // parked stack, [entry*9 + field], RI = field 7
    for (int k = 1; k <= 3; k++)
        if (!((wm >> k) & 1u) && !((rm >> k) & 1u)) {
            fl[k * 9 + 7] = __uint_as_float(E[k - 1]);
            av[k - 1] = __uint_as_float(E[k - 1]);
        }
    R.assume[R.ix(u)] = a;
}

// Replay of each pixel's samples in order (one lane per pixel unit; records are [s][pu], so
// consecutive lanes read consecutive records).
__global__ __launch_bounds__(kBlock) void k_iow03_resolve(Frame f, SpecRecs R, int final_pass, float4 *state) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // pixel i of the group (or of all units)
    const bool valid = R.order_n ? i < R.order_n : i < R.P;
    const uint32_t pu = valid ? (R.order_n ? R.order[R.order_base + i] : i) : 0;
    const UnitPix px = unit_pixel(f, valid ? pu : 0);
    bool work = valid && px.in_image;
    uint32_t E1 = 0, E2 = 0, E3 = 0;  // exact RI bits of entries 1..3 before sample s
    f3 fc = f3{0, 0, 0};
    unsigned long long seg = 0, drops = 0, nans = 0, nodes = 0, prims = 0;
    int first_bad = -1;
    uint32_t s = 0;
    for (; work && s < R.S; s++) {
        const size_t u = (size_t)s * R.P + pu;
        float4 cl = R.col[R.ix(u)];
        uint32_t fl = __float_as_uint(cl.w), rm = fl & 15u, wm = (fl >> 4) & 15u;
        float4 a = R.assume[R.ix(u)];
#ifdef RT_DIAG
        if (final_pass && R.exact && (R.exact_mode & 1) && first_bad < 0)
            R.exact[u] = make_float4(__uint_as_float(E1), __uint_as_float(E2), __uint_as_float(E3), 0.0f);
#endif
        bool bad = ((rm & 2u) && __float_as_uint(a.x) != E1) || ((rm & 4u) && __float_as_uint(a.y) != E2) ||
                   ((rm & 8u) && __float_as_uint(a.z) != E3);
        if (bad && first_bad < 0 && R.alt && alt_adopt(R, (uint32_t)u, E1, E2, E3, 0xffffffffu, 0u)) {
            cl = R.col[R.ix(u)];  // an alternative run under the exact state: adopted
            fl = __float_as_uint(cl.w); rm = fl & 15u; wm = (fl >> 4) & 15u;
            a = R.assume[R.ix(u)];
            bad = false;
        }
        if (bad) {
            if (first_bad < 0) first_bad = (int)s;
            if (final_pass) break;  // the sequential kernel takes over from here
            R.assume[R.ix(u)] = make_float4(__uint_as_float(E1), __uint_as_float(E2), __uint_as_float(E3), 0.0f);
            R.list[atomicAdd(R.list_count, 1u)] = (uint32_t)u;
        }
        if (first_bad < 0) {  // still exact: accumulate in sample order
            fc = fc + f3{cl.x, cl.y, cl.z};
            const uint4 ct4 = R.ctr[R.ix(u)];
            seg += ct4.x; drops += ct4.y; nans += ct4.z; nodes += ct4.w;
            prims += __float_as_uint(R.fin[R.ix(u)].w);
        }
        const float4 fn = R.fin[R.ix(u)];  // the record's own outputs (a guess while it is queued)
        if (wm & 2u) E1 = __float_as_uint(fn.x);
        if (wm & 4u) E2 = __float_as_uint(fn.y);
        if (wm & 8u) E3 = __float_as_uint(fn.z);
    }
    if (final_pass && valid && !px.in_image) write_px(f, px, f3{0, 0, 0}, 0.0f);  // tile padding
    if (final_pass && work) {
        if (first_bad < 0) {
            write_px(f, px, fc * rcp((float)R.S), 0.0f);
            if (f.px_rays) f.px_rays[pu] = (unsigned)seg;
        } else {  // resume state for the sequential kernel: colour sum, first sample, stack RI
            state[2 * (size_t)pu] = make_float4(fc.x, fc.y, fc.z, __int_as_float(first_bad));
            state[2 * (size_t)pu + 1] = make_float4(0.0f, __uint_as_float(E1), __uint_as_float(E2), __uint_as_float(E3));
            R.fb_list[atomicAdd(R.fb_count, 1u)] = pu;
        }
    }
    if (final_pass && f.counters) {
        const unsigned long long v[5] = {seg, nodes, prims, drops, nans};
        const int slot[5] = {0, 1, 2, 4, 5};
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const unsigned long long t = wave_sum(v[i]);
            if ((threadIdx.x & 63) == 0 && t) atomicAdd(f.counters + slot[i], t);
        }
    }
}

// ============================================================================ launch
int iow_spec_blocks_per_cu(RenderKernel k) {
    return k == RenderKernel::Iow03SpecLds ? occupancy_of(k_iow03sL, 3 * kBlock) : occupancy_of(k_iow03s, kBlock);
}
hipError_t launch_iow03_spec(const Frame &f, const IowScene &sc, const SpecRecs &R, int mode, const Cont &ct,
                             uint32_t n_units, unsigned *counter, int blocks_cap, hipStream_t s) {
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    if (iow_lds(sc))
        hipLaunchKernelGGL(k_iow03sL, dim3(grid_of((n_units + 2) / 3, blocks_cap / 3)), dim3(3 * kBlock), 0, s, f, sc, R,
                           mode, ct, counter);
    else
        hipLaunchKernelGGL(k_iow03s, dim3(grid_of(n_units, blocks_cap)), dim3(kBlock), 0, s, f, sc, R, mode, ct,
                           counter);
    return hipGetLastError();
}
__global__ void k_spec_list_keys(SpecRecs R, unsigned *keys, size_t n) {
    const unsigned cnt = *R.list_count;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        keys[i] = i < cnt ? min(R.ctr[R.ix(R.list[i])].x, 0xffffffu) : 0u;
}
hipError_t spec_list_keys(const SpecRecs &R, unsigned *keys, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_list_keys, dim3(4096), dim3(256), 0, s, R, keys, n);
    return hipGetLastError();
}
// ---------------------------------------------------------------- heavy-first enumeration
// cost of sample index s (1..S-1) over the probe pixels: finished records (block s-1)
__global__ __launch_bounds__(kBlock) void k_sample_cost(SpecRecs R, unsigned long long *fcost) {
    __shared__ unsigned long long part[kBlock / 64];
    const uint32_t s = blockIdx.x + 1u;
    const uint32_t n_px = R.order_n ? R.order_n : R.P;
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    unsigned long long acc = 0;
    for (uint32_t i = threadIdx.x; (size_t)i * R.probe_stride < n_px; i += kBlock) {
        const size_t u = (size_t)s * R.P + R.order[R.order_base + i * R.probe_stride];
        if ((__float_as_uint(R.col[R.ix(u)].w) & 0xffff0100u) == done_tag) acc += R.ctr[R.ix(u)].x;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kBlock / 64; w++) t += part[w];
        atomicAdd(fcost + s, t);
    }
}
// progress of the parked lanes (the long samples still running) counts toward their index
__global__ __launch_bounds__(kBlock) void k_sample_cost_parked(SpecRecs R, const float4 *cont, const unsigned *count,
                                                               unsigned long long *fcost) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= *count) return;  // no cross-lane work in this kernel
    const float4 *p = cont + (size_t)i * kContSlots;
    if (p[12].y != 0.0f) return;
    const uint32_t u = __float_as_uint(p[0].x);
    atomicAdd(fcost + u / R.P, (unsigned long long)__float_as_uint(p[2].x));
}
// rank the indices 1..S-1 by cost, most expensive first (ties: lower index first)
__global__ __launch_bounds__(1024) void k_sample_rank(SpecRecs R, const unsigned long long *fcost, uint32_t *sorder) {
    for (uint32_t s = 1u + threadIdx.x; s < R.S; s += 1024u) {
        const unsigned long long c = fcost[s];
        uint32_t rank = 0;
        for (uint32_t t = 1; t < R.S; t++) rank += (fcost[t] > c || (fcost[t] == c && t < s)) ? 1u : 0u;
        sorder[rank] = s;
    }
}
// per pixel: the most rays among its heavy samples (finished records), for the re-sort
__global__ __launch_bounds__(kBlock) void k_pixel_key(Frame f, SpecRecs R, unsigned *key) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n_px = R.order_n ? R.order_n : R.P;
    if (i >= n_px) return;  // no cross-lane work in this kernel
    const uint32_t pu = R.order[R.order_base + i];
    const unsigned done_tag = (1u << 8) | ((R.epoch & 0xffffu) << 16);
    unsigned k = R.ctr[R.ix(pu)].x;  // sample 0
    for (uint32_t j = 0; j < R.n_heavy; j++) {
        const size_t u = (size_t)R.sorder[j] * R.P + pu;
        if ((__float_as_uint(R.col[R.ix(u)].w) & 0xffff0100u) == done_tag) k = max(k, R.ctr[R.ix(u)].x);
    }
    key[pu] = unit_pixel(f, pu).in_image ? k : 0u;
}
__global__ __launch_bounds__(kBlock) void k_pixel_key_parked(SpecRecs R, const float4 *cont, const unsigned *count,
                                                             unsigned *key) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= *count) return;  // no cross-lane work in this kernel
    const float4 *p = cont + (size_t)i * kContSlots;
    if (p[12].y != 0.0f) return;
    const uint32_t u = __float_as_uint(p[0].x);
    atomicMax(key + u % R.P, __float_as_uint(p[2].x));
}
hipError_t launch_iow03_sample_order(const Frame &f, const SpecRecs &R, const float4 *cont, const unsigned *count,
                                     int max_lanes, unsigned long long *fcost, uint32_t *sorder, hipStream_t s) {
    hipError_t e = hipMemsetAsync(fcost, 0, sizeof(unsigned long long) * R.S, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sample_cost, dim3(R.S - 1u), dim3(kBlock), 0, s, R, fcost);
    const unsigned blocks = (unsigned)((max_lanes + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_sample_cost_parked, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, R, cont, count, fcost);
    hipLaunchKernelGGL(k_sample_rank, dim3(1), dim3(1024), 0, s, R, fcost, sorder);
    return hipGetLastError();
}
hipError_t launch_iow03_pixel_key(const Frame &f, const SpecRecs &R, const float4 *cont, const unsigned *count,
                                  int max_lanes, unsigned *key, hipStream_t s) {
    const uint32_t n_px = R.order_n ? R.order_n : R.P;
    hipLaunchKernelGGL(k_pixel_key, dim3((n_px + kBlock - 1) / kBlock), dim3(kBlock), 0, s, f, R, key);
    const unsigned blocks = (unsigned)((max_lanes + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_pixel_key_parked, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, R, cont, count, key);
    return hipGetLastError();
}
hipError_t launch_iow03_frontier(const Frame &f, const SpecRecs &R, float4 *cont, unsigned *count, uint32_t cap,
                                 hipStream_t s) {
    const uint32_t n = R.order_n ? R.order_n : R.P;
    hipLaunchKernelGGL(k_iow03_frontier, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, f, R, cont, count, cap);
    return hipGetLastError();
}
hipError_t launch_iow03_altspawn(const Frame &f, const SpecRecs &R, float4 *cont, unsigned *count, uint32_t cap,
                                 hipStream_t s) {
    const uint32_t n = R.order_n ? R.order_n : R.P;
    const unsigned blocks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_iow03_altspawn, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, f, R, cont, count, cap);
    return hipGetLastError();
}
hipError_t launch_iow03_fixf(const Frame &f, const SpecRecs &R, float4 *cont, const unsigned *count, int max_lanes,
                             hipStream_t s) {
    const unsigned blocks = (unsigned)((max_lanes + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_iow03_fixf, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, f, R, cont, count);
    return hipGetLastError();
}
hipError_t launch_iow03_prep(const Frame &f, const SpecRecs &R, unsigned *key, float prior, uint32_t prior_from,
                             hipStream_t s) {
    const unsigned blocks = (R.P + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_iow03_prep, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, f, R, key, prior, prior_from);
    return hipGetLastError();
}
hipError_t launch_iow03_resolve(const Frame &f, const SpecRecs &R, bool final_pass, float4 *state, hipStream_t s) {
    const unsigned blocks = ((R.order_n ? R.order_n : R.P) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_iow03_resolve, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, f, R, final_pass ? 1 : 0, state);
    return hipGetLastError();
}

}  // namespace rtk
