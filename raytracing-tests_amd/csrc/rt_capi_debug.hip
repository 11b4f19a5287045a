// rt_capi_debug.hip -- the rt_debug_* entry points of include/rt_hip_debug.h: diagnostics and
// what the tests ask about the last render.  No exception crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_dev_scene.hpp"

unsigned long long *g_dbg = nullptr;
unsigned *g_px_rays = nullptr;
bool g_time_kernels = false;
uint32_t g_sky_blocking[3] = {0, 0, 0};

namespace {

// a histogram of n u64 over the scene's sample-parallel records: zeroed, filled by fn on the
// device, copied to out
template <class F> int spec_hist_out(rt_dev_scene *s, uint64_t *out, size_t n, F &&fn) {
    if (!s || !out) return RT_E_ARG;
    std::memset(out, 0, n * sizeof(uint64_t));
    if (!s->sp.cap) return RT_OK;
    DevBuf d;
    HIP_OK(d.alloc(n * sizeof(uint64_t)));
    HIP_OK(hipMemset(d.p, 0, n * sizeof(uint64_t)));
    HIP_OK(fn(d.as<unsigned long long>()));
    HIP_OK(hipMemcpy(out, d.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_debug_build_level_cap(int levels) {
    if (levels < 0) return RT_E_ARG;
    g_build_levels = levels;
    return RT_OK;
}

int rt_debug_wide_info(rt_dev_scene *s, uint32_t info[8], uint32_t *rank_out) {
    if (!s || s->kind == 3 || !info) return RT_E_ARG;
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipDeviceSynchronize());
    const InwWalk &w = s->walk;
    const uint32_t cells = w.ri_ok ? uint32_t(w.ri_dim[0]) * uint32_t(w.ri_dim[1]) * uint32_t(w.ri_dim[2]) : 0u;
    const uint32_t v[8] = {w.n_wtree0, w.dfs_high, uint32_t(w.wdepth), w.ri_ok ? 1u : 0u, cells,
                           w.sl_ok ? 1u : 0u, s->n, w.wbuild};
    std::memcpy(info, v, sizeof(v));
    if (rank_out && w.n_wnodes)
        HIP_OK(hipMemcpy(rank_out, w.wrank.p, size_t(s->n) * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_path(rt_dev_scene *s, rt_path_info *out) {
    if (!s || !out) return RT_E_ARG;
    char name[64] = {0};
    const int n = rt_debug_launches(s, name, int(sizeof(name)));  // resolves the fold kernel (synchronises)
    if (n < 0) return n;
    const LastRender &L = s->last;
    const uint32_t n_wtree0 = s->walk.n_wtree0;
    rt_path_info P = L.path;
    std::memcpy(P.kernel, name, sizeof(P.kernel));
    P.launches = n;
    P.ref_walks = 0;
    if (s->kind != 3 && s->walk_ctr.p) {
        unsigned long long v = 0;
        HIP_OK(hipMemcpy(&v, s->walk_ctr.p, sizeof(v), hipMemcpyDeviceToHost));
        P.ref_walks = v;
    }
    if (std::strncmp(name, "k_inw_pm", 8) == 0) {
        P.order = 1;
        P.ring_entries = int(L.ring[0]);
        P.ring_lds = L.lring ? 1 : 0;
        if (L.lring && !L.gq) { P.lds_nodes = 0; P.lbvh_lds_nodes = 0; }  // the FStack ring instances stage no nodes
        if (L.ln && !L.lring) P.time_bins = 0;  // the global-ring LN instance walks the staged swept tree
    }
    else if (std::strncmp(name, "k_inw_sm", 8) == 0) {
        P.order = 2;
        P.ring_entries = int(L.ring[1]);
        P.ring_lds = L.lring_sm ? 1 : 0;
        if (L.lring_sm) P.lds_nodes = std::min(P.lds_nodes, int(rtk::kPmLdsNodes));
        if (L.lring_sm) P.lbvh_lds_nodes = std::min(P.lbvh_lds_nodes, int(rtk::kPmLdsNodes * 10 / 2));
        if (L.ln) P.time_bins = 0;  // its walks read the staged top of the swept tree
        if (L.gq) {  // the GQ instance is pixel-major only: k_inw_sm ran the 236-node FStack kernel
            P.qnodes = 0; P.global_stack = 0; P.walk_stack = rtk::kFStack - 3;
            P.lds_nodes = L.lring_sm ? std::min(n_wtree0, rtk::kPmLdsNodes) : std::min(n_wtree0, uint32_t(rtk::kInwLdsNodes));
        }
    }
    if (P.order != 1) { P.beams = 0; P.claim_order = 0; P.beam_bins = 0; P.beam_prune = 0; }  // both serve the pixel-major kernel only
    *out = P;
    return RT_OK;
}

// Diagnostics (not part of the reference's surface): pass a device buffer of 8 u64 to make
// the kernels tally lane occupancy per phase; NULL turns it off.
int rt_debug_counters(uint64_t *d_buf) {
    g_dbg = reinterpret_cast<unsigned long long *>(d_buf);
    return RT_OK;
}

int rt_debug_pixel_rays(uint32_t *d_buf) {
    g_px_rays = d_buf;
    return RT_OK;
}

int rt_debug_rounds(rt_dev_scene *s, uint32_t *out, int cap) {
    if (!s || !out || cap <= 0) return RT_E_ARG;
    if (!s->ws.cont_count.p) return 0;
    std::vector<unsigned> v(16 * 16);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(v.data(), s->ws.cont_count.p, v.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    const int n = std::min(cap, 16);
    for (int r = 0; r < n; r++) out[r] = v[size_t(16) * r];
    return n;
}

int rt_debug_spec_hist(rt_dev_scene *s, uint64_t *out) {
    return spec_hist_out(s, out, 66, [&](unsigned long long *d) {
        return rtk::spec_hist(s->sp.ctr.as<uint4>(), s->sp.cap, d, nullptr);
    });
}

int rt_debug_spec_list_hist(rt_dev_scene *s, uint64_t *out) {
    return spec_hist_out(s, out, 66, [&](unsigned long long *d) {
        return rtk::spec_list_hist(s->sp.ctr.as<uint4>(), s->sp.P, s->sp.S, s->sp.list.as<uint32_t>(),
                                   s->sp.counts.as<unsigned>(), d, nullptr);
    });
}

int rt_debug_spec_list_stale(rt_dev_scene *s, uint64_t *out) {
    return spec_hist_out(s, out, 32, [&](unsigned long long *d) {
        return rtk::spec_list_stale(s->sp.ctr.as<uint4>(), s->sp.P, s->sp.S, s->sp.list.as<uint32_t>(),
                                    s->sp.counts.as<unsigned>(), d, nullptr);
    });
}

int rt_debug_spec_pixels(rt_dev_scene *s, uint32_t *out, uint32_t cap_units) {
    if (!s || !out) return RT_E_ARG;
    if (!s->sp.cap || !s->sp.P || s->sp.P > cap_units) return RT_E_ARG;
    const uint32_t P = s->sp.P, S = s->sp.S;  // the last render's record layout
    DevBuf d;
    HIP_OK(d.alloc(size_t(P) * 16));
    HIP_OK(rtk::spec_pixels(s->sp.ctr.as<uint4>(), P, S, s->ws.order.as<uint32_t>(), d.as<uint32_t>(), nullptr));
    HIP_OK(hipMemcpy(out, d.p, size_t(P) * 16, hipMemcpyDeviceToHost));
    return int(P);
}

int rt_debug_spec_dump(rt_dev_scene *s, uint32_t *rays_out, size_t cap, uint32_t *list_out, uint32_t list_cap,
                       uint32_t *dims) {
    if (!s || !rays_out || !dims) return RT_E_ARG;
    if (!s->sp.cap || !s->sp.P) return RT_E_ARG;
    const uint32_t P = s->sp.P, S = s->sp.S;  // the last render's record layout (SpecRecs::ix)
    if (size_t(P) * S > cap) return RT_E_ARG;
    std::vector<uint4> h(size_t(P) * S);
    HIP_OK(hipMemcpy(h.data(), s->sp.ctr.p, h.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    for (size_t u = 0; u < h.size(); u++) rays_out[u] = h[rtk::spec_rec_ix(u, P, S)].x;  // in unit order s * P + pu
    unsigned cnt[32] = {};
    HIP_OK(hipMemcpy(cnt, s->sp.counts.p, sizeof(cnt), hipMemcpyDeviceToHost));
    const uint32_t nl = std::min(cnt[0], list_cap);
    if (list_out && nl) HIP_OK(hipMemcpy(list_out, s->sp.list.p, size_t(nl) * 4, hipMemcpyDeviceToHost));
    dims[0] = P; dims[1] = S; dims[2] = cnt[0]; dims[3] = cnt[16];
    return RT_OK;
}

int rt_debug_spec_times(rt_dev_scene *s, uint32_t *start_out, uint32_t *end_out, size_t cap) {
    if (!s || !start_out || !end_out || !s->sp.dbg_n || !s->sp.dbg_t.p) return RT_E_ARG;
    const size_t n = s->sp.dbg_n;  // the last render's P * S: its end times start at offset n
    if (n > cap || s->sp.dbg_t.bytes < 2 * n * sizeof(uint32_t)) return RT_E_ARG;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(start_out, s->sp.dbg_t.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(end_out, static_cast<char *>(s->sp.dbg_t.p) + n * 4, n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_launches(rt_dev_scene *s, char *name_out, int name_cap) {
    if (!s) return RT_E_ARG;
    LastRender &L = s->last;
    if (L.fold_pending) {
        // the probe picked the fold kernel on the device: read its verdict (synchronises)
        uint32_t m[2] = {0, 0};
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(m, s->fold.mode.p, sizeof(m), hipMemcpyDeviceToHost));
        const uint32_t ord = L.force;  // the order the launch used (0: the probe's verdict)
        const bool sm = ord == 2 || (ord != 1 && m[0] > 0 && 2 * m[1] >= m[0]);
        // the template instance's name as rocprofv3 prints it, every template argument:
        // <LIGHTS, LN (LDS-staged BVH top), FU (fused cull), LRING (the fold ring in LDS)[, GQ (k_inw_pm)]>
        auto tf = [](bool b) { return b ? "true" : "false"; };
        const bool lights = s->layout == 4;
        if (sm)
            std::snprintf(L.kernel, sizeof(L.kernel), "k_inw_sm<%s, %s, %s, %s>", tf(lights), tf(L.ln), tf(L.fu),
                          tf(L.lring_sm));
        else
            std::snprintf(L.kernel, sizeof(L.kernel), "k_inw_pm<%s, %s, %s, %s, %s>", tf(lights), tf(L.ln), tf(L.fu),
                          tf(L.lring || L.gq), tf(L.gq));
        L.fold_pending = false;
    }
    if (name_out && name_cap > 0) {
        std::strncpy(name_out, L.kernel, size_t(name_cap) - 1);
        name_out[name_cap - 1] = 0;
    }
    return L.launches;
}

int rt_debug_sky_blocks(rt_dev_scene *s, uint32_t out[3]) {
    if (!out) return RT_E_ARG;
    if (!s) {  // the last blocking render (its scene is gone)
        std::memcpy(out, g_sky_blocking, sizeof(g_sky_blocking));
        return RT_OK;
    }
    return sky_blocks_of(s, out);
}
int rt_debug_beam_lists(rt_dev_scene *s, uint64_t totals[8], uint32_t *n_out, float *cut_out, uint64_t *entries_out,
                        uint32_t cap_lists) {
    if (!s || !totals || s->kind == 3) return RT_E_ARG;
    std::memset(totals, 0, 8 * sizeof(uint64_t));
    char name[64] = {0};
    if (rt_debug_launches(s, name, int(sizeof(name))) < 0) return RT_E_ARG;  // resolves the fold order (synchronises)
    const LastRender &L = s->last;
    if (!L.beam_lists || !L.beam_cap || std::strncmp(name, "k_inw_pm", 8) != 0) return RT_OK;
    const size_t lists = L.beam_lists, cap = L.beam_cap, esz = L.beam16 ? sizeof(uint32_t) : sizeof(uint2);
    if ((n_out || cut_out || entries_out) && cap_lists < lists) return RT_E_ARG;
    if (s->fold.beam_n.bytes < lists * 8 || s->fold.beam.bytes < lists * cap * esz) return RT_E_ARG;
    try {
        HIP_OK(hipSetDevice(s->device));
        HIP_OK(hipDeviceSynchronize());
        std::vector<uint32_t> nc(lists * 2);  // the counts, then the cuts
        HIP_OK(hipMemcpy(nc.data(), s->fold.beam_n.p, lists * 8, hipMemcpyDeviceToHost));
        std::vector<uint32_t> raw;
        if (entries_out) {
            raw.resize(lists * cap * esz / sizeof(uint32_t));
            HIP_OK(hipMemcpy(raw.data(), s->fold.beam.p, lists * cap * esz, hipMemcpyDeviceToHost));
            std::memset(entries_out, 0, lists * cap * sizeof(uint64_t));
        }
        uint64_t nonempty = 0, entries = 0, cuts = 0, offs = 0;
        for (size_t l = 0; l < lists; l++) {
            const uint32_t nw = nc[l];
            const bool off = nw == rtk::kBeamOff;
            const uint32_t cnt = off ? 0u : (nw & 0xffu);
            float cut;
            std::memcpy(&cut, &nc[lists + l], sizeof(cut));
            if (n_out) n_out[l] = off ? rtk::kBeamOff : cnt;
            if (cut_out) cut_out[l] = cut;
            offs += off;
            nonempty += cnt > 0;
            entries += cnt;
            cuts += !off && std::isfinite(cut);  // +inf: every leaf that passed the tests is listed
            if (!entries_out || cnt == 0) continue;
            // the block's 64 lists share its region of 64 * cap entries (k_inw_beam)
            const size_t base = (l & ~size_t(63)) * cap + (nw >> 8);
            if (cnt > cap || base + cnt > lists * cap) return RT_E_ARG;
            for (uint32_t j = 0; j < cnt; j++) {
                uint64_t id, key;
                if (L.beam16) { const uint32_t e = raw[base + j]; id = e & 0xffffu; key = e & 0xffff0000u; }
                else { id = raw[2 * (base + j)]; key = raw[2 * (base + j) + 1]; }
                entries_out[l * cap + j] = id | (key << 32);
            }
        }
        const uint64_t v[8] = {lists, nonempty, entries, cuts, offs, cap, 0, 0};
        std::memcpy(totals, v, sizeof(v));
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

int rt_beam_keep_host(const float cam_pos[3], const float cd[3], float aperture, float focus, float sf_max,
                      float wbound, const float box[6], const float *sph, uint32_t bin, uint32_t bins, int prune,
                      int *candidate) {
    if (!cam_pos || !cd || !box || prune < 0 || prune > 2 || bin >= std::max(1u, bins)) return RT_E_ARG;
    rtk::BeamGeom g;
    if (!rtk::beam_geom(cam_pos, aperture, focus, sf_max, wbound, g)) return RT_E_UNSUPPORTED;
    const rtk::BeamPrune P = rtk::beam_prune_of(g, prune, bins);
    // k_inw_beam's central ray: from co + cd along cd, the reciprocals correctly rounded
    const float o[3] = {cam_pos[0] + cd[0], cam_pos[1] + cd[1], cam_pos[2] + cd[2]};
    const float id[3] = {1.0f / cd[0], 1.0f / cd[1], 1.0f / cd[2]};
    if (candidate) *candidate = 0;
    if (!(std::isfinite(id[0]) && std::isfinite(id[1]) && std::isfinite(id[2]))) return 0;  // the list is switched off
    const bool neg[3] = {cd[0] < 0.0f, cd[1] < 0.0f, cd[2] < 0.0f};
    float nr[3], fr[3], te, tx;
    for (int a = 0; a < 3; a++) { nr[a] = neg[a] ? box[3 + a] : box[a]; fr[a] = neg[a] ? box[a] : box[3 + a]; }
    rtk::beam_slab(nr, fr, o, id, neg, P.R, te, tx);
    if (!(std::fmax(te, P.tmin) <= std::fmin(tx, P.tfar))) return 0;
    if (candidate) *candidate = 1;
    if (P.mode == 0) return 1;
    if (!rtk::beam_box_keep(P, nr, fr, o, id, neg, te, tx)) return 0;
    if (P.mode >= 2 && sph && !rtk::beam_sphere_keep(P, o, cd, sph, sph + 4, bin)) return 0;
    return 1;
}

int rt_debug_chunks(rt_dev_scene *s) {
    if (!s) return RT_E_ARG;
    return s->last.chunks;
}

int rt_debug_check_fastmath(int which, uint64_t *mismatches, uint32_t *first_bad) {
    if (!mismatches || !first_bad || which != 0) return RT_E_ARG;
    DevBuf d;
    HIP_OK(d.alloc(16));
    HIP_OK(hipMemset(d.p, 0, 8));
    HIP_OK(hipMemset(static_cast<char *>(d.p) + 8, 0xff, 4));
    HIP_OK(rtk::launch_check_fastmath(which, d.as<unsigned long long>(), reinterpret_cast<unsigned *>(static_cast<char *>(d.p) + 8),
                                 nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(mismatches, d.p, 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(first_bad, static_cast<char *>(d.p) + 8, 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_time_kernels(int on) {
    g_time_kernels = on != 0;
    return RT_OK;
}

int rt_debug_kernel_time(rt_dev_scene *s, double *ms_total, int *launches) {
    if (!s || !ms_total || !launches) return RT_E_ARG;
    double t = 0.0;
    for (size_t i = 0; i < s->kt_used; i++) {
        HIP_OK(hipEventSynchronize(s->kt_ev[i].second));
        float ms = 0.0f;
        HIP_OK(hipEventElapsedTime(&ms, s->kt_ev[i].first, s->kt_ev[i].second));
        t += ms;
    }
    *ms_total = t;
    *launches = int(s->kt_used);
    return RT_OK;
}

int rt_debug_time_bins(const float *nodes, const float *geom, uint32_t n, uint32_t bins, float *wnodes_out,
                       uint32_t wnodes_cap, uint32_t info[4]) {
    if (!nodes || !geom || n == 0 || !info) return RT_E_ARG;
    try {
        rtamd::InwWide w;
        if (!rtamd::inw_wide_build(nodes, n, w)) { std::memset(info, 0, 4 * sizeof(uint32_t)); return RT_OK; }
        rtamd::inw_wide_add_bins(geom, n, bins, w);
        const uint32_t total = uint32_t(w.wnodes.size() / 40);
        const uint32_t v[4] = {w.n_tree0, w.bins, w.bin_stride, total};
        std::memcpy(info, v, sizeof(v));
        if (wnodes_out && wnodes_cap >= total) std::memcpy(wnodes_out, w.wnodes.data(), w.wnodes.size() * sizeof(float));
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

int rt_debug_bin_boxes(const float *geom, uint32_t n, uint32_t bins, uint32_t b, float *boxes_out) {
    if (!geom || !boxes_out || n == 0 || bins == 0 || b >= bins) return RT_E_ARG;
    try {
        std::vector<float> boxes;
        float wb = 0.0f;
        if (!rtamd::inw_bin_boxes(geom, n, bins, b, boxes, wb)) return RT_E_ARG;
        std::memcpy(boxes_out, boxes.data(), boxes.size() * sizeof(float));
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

int rt_debug_sphere_records(const float *geom, uint32_t n, int layout, float *out) {
    if (!geom || !out || n == 0 || (layout != 1 && layout != 4)) return RT_E_ARG;
    try {
        std::vector<float> r;
        if (!inw_sphere_records(geom, n, layout, r)) return 0;
        std::memcpy(out, r.data(), r.size() * sizeof(float));
    } catch (...) {
        return RT_E_ARG;
    }
    return 1;
}

int rt_debug_inw_stick_out(const float *geom, uint32_t n, const float *nodes, const float *aabbs, double *worst_out) {
    if (!geom || n == 0 || (!nodes && !aabbs) || !worst_out) return RT_E_ARG;
    *worst_out = nodes ? rtamd::inw_stick_out(geom, n, nodes, 0) : rtamd::inw_stick_out(geom, n, aabbs, 6);
    return RT_OK;
}

int rt_debug_walk_dump(rt_dev_scene *s, int what, void *out, size_t cap_bytes, uint64_t info[8]) {
    if (!s || s->kind == 3 || s->broken || !info) return RT_E_ARG;
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipDeviceSynchronize());
    const InwWalk &w = s->walk;
    uint64_t v[8] = {};
    const DevBuf *src = nullptr;
    const void *host = nullptr;  // RI frame and wbound live in the scene, not in a device buffer
    struct { float f[9]; int32_t dim[3]; } frame{};
    const size_t nw = w.n_wnodes, n = s->n;
    const size_t cells = w.ri_ok ? size_t(w.ri_dim[0]) * size_t(w.ri_dim[1]) * size_t(w.ri_dim[2]) : 0;
    switch (what) {
    case RT_WALK_WNODES:
        src = &w.wnodes; v[0] = nw * 10 * sizeof(float4); v[1] = nw; v[2] = w.n_wtree0; v[3] = w.wbins;
        v[4] = w.wbin_stride; v[5] = uint64_t(w.wdepth);
        break;
    case RT_WALK_CNODES: src = &w.cnodes; v[0] = nw * 7 * sizeof(float4); v[1] = nw; break;
    case RT_WALK_QNODES: src = &w.qnodes; v[0] = nw * rtk::kQNodeF4 * sizeof(float4); v[1] = nw; v[2] = rtk::kQNodeF4; break;
    case RT_WALK_LEAFBOX: src = &w.wleaf; v[0] = nw ? n * 2 * sizeof(float4) : 0; v[1] = nw ? n : 0; break;
    case RT_WALK_LBVH: src = &s->nodes; v[0] = n ? (2 * n - 1) * 2 * sizeof(float4) : 0; v[1] = n ? 2 * n - 1 : 0; break;
    case RT_WALK_RI_CELLS: src = &w.ri_cells; v[0] = cells ? (cells + 1) * sizeof(uint32_t) : 0; v[1] = cells; v[2] = w.ri_ok; break;
    case RT_WALK_RI_IDS: {
        src = &w.ri_ids;
        uint32_t total = 0;
        if (cells) {
            if (w.ri_cells.bytes < (cells + 1) * sizeof(uint32_t)) return RT_E_ARG;
            HIP_OK(hipMemcpy(&total, w.ri_cells.as<uint32_t>() + cells, sizeof(total), hipMemcpyDeviceToHost));
        }
        v[0] = size_t(total) * sizeof(uint32_t); v[1] = total;
        break;
    }
    case RT_WALK_RI_FRAME:
        for (int a = 0; a < 3; a++) {
            frame.f[a] = w.ri_lo[a]; frame.f[3 + a] = w.ri_hi[a]; frame.f[6 + a] = w.ri_inv[a]; frame.dim[a] = w.ri_dim[a];
        }
        host = &frame; v[0] = w.ri_ok ? sizeof(frame) : 0;
        break;
    case RT_WALK_WBOUND: host = &w.wbound; v[0] = nw ? sizeof(float) : 0; break;
    case RT_WALK_HOT: src = &s->hot; v[0] = n * rtk::kInwHot * sizeof(float); v[1] = n; v[2] = rtk::kInwHot; break;
    case RT_WALK_COLD: src = &s->cold; v[0] = n * rtk::kInwCold * sizeof(float); v[1] = n; v[2] = rtk::kInwCold; break;
    case RT_WALK_SPH: src = &s->sph; v[0] = s->sph_ok ? n * 12 * sizeof(float) : 0; v[1] = s->sph_ok ? n : 0; v[2] = 12; break;
    default: return RT_E_ARG;
    }
    std::memcpy(info, v, sizeof(v));
    if (!out || !v[0]) return RT_OK;
    if (cap_bytes < v[0]) return RT_E_ARG;
    if (host) { std::memcpy(out, host, size_t(v[0])); return RT_OK; }
    if (!src->p || src->bytes < v[0]) return RT_E_ARG;  // never read past the allocation
    HIP_OK(hipMemcpy(out, src->p, size_t(v[0]), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_inw_host_dump(const float *nodes, uint32_t n, uint32_t info[8], float *wnodes, float *leafbox,
                           uint32_t *rank, uint32_t *ri_cells, uint32_t *ri_ids, float ri_frame[9], int32_t ri_dim[3]) {
    if (!nodes || n == 0 || !info) return RT_E_ARG;
    try {
        std::memset(info, 0, 8 * sizeof(uint32_t));
        rtamd::InwWide w;
        if (!rtamd::inw_wide_build(nodes, n, w)) return RT_OK;
        const rtamd::RiGrid g = rtamd::ri_grid_build(w.leafbox.data(), n);
        uint32_t wb = 0;
        std::memcpy(&wb, &w.wbound, sizeof(wb));
        const uint32_t v[8] = {uint32_t(w.wnodes.size() / 40), w.dfs_high, uint32_t(w.depth), g.ok ? 1u : 0u,
                               g.ok ? uint32_t(g.cells.size() - 1) : 0u, uint32_t(g.ids.size()), wb, 0u};
        std::memcpy(info, v, sizeof(v));
        if (wnodes) std::memcpy(wnodes, w.wnodes.data(), w.wnodes.size() * sizeof(float));
        if (leafbox) std::memcpy(leafbox, w.leafbox.data(), w.leafbox.size() * sizeof(float));
        if (rank) std::memcpy(rank, w.rank.data(), w.rank.size() * sizeof(uint32_t));
        if (g.ok) {
            if (ri_cells) std::memcpy(ri_cells, g.cells.data(), g.cells.size() * sizeof(uint32_t));
            if (ri_ids && !g.ids.empty()) std::memcpy(ri_ids, g.ids.data(), g.ids.size() * sizeof(uint32_t));
            for (int a = 0; a < 3; a++) {
                if (ri_frame) { ri_frame[a] = g.lo[a]; ri_frame[3 + a] = g.hi[a]; ri_frame[6 + a] = g.inv[a]; }
                if (ri_dim) ri_dim[a] = g.dim[a];
            }
        }
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

int rt_debug_iow_host_dump(const float *types, const float *records, uint32_t n, uint32_t info[4], float *wide,
                           float *obox) {
    if (!types || !records || n == 0 || !info) return RT_E_ARG;
    try {
        std::memset(info, 0, 4 * sizeof(uint32_t));
        rtamd::IowCull c;
        if (!rtamd::iow_cull_build(types, records, n, c)) return RT_OK;
        info[0] = c.n_wide;
        if (wide) std::memcpy(wide, c.wide.data(), c.wide.size() * sizeof(float));
        if (obox) std::memcpy(obox, c.obox.data(), c.obox.size() * sizeof(float));
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

int rt_debug_iow_info(rt_dev_scene *s, uint32_t info[8]) {
    if (!s || s->kind != 3 || !info) return RT_E_ARG;
    const IowCullPriors &q = s->iow;
    const rtk::IowScene sc = iow_view(*s);
    const uint32_t v[8] = {s->n, sc.n_nodes, uint32_t(q.depth), q.built, rtk::iow_lds(sc) ? 1u : 0u, q.updates, 0u, 0u};
    std::memcpy(info, v, sizeof(v));
    return RT_OK;
}

int rt_debug_iow_dump(rt_dev_scene *s, uint32_t info[4], float *wide, float *obox) {
    if (!s || s->kind != 3 || s->broken || !info) return RT_E_ARG;
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipDeviceSynchronize());
    std::memset(info, 0, 4 * sizeof(uint32_t));
    const rtk::IowScene sc = iow_view(*s);
    if (!sc.nodes) return RT_OK;
    const size_t wb = size_t(sc.n_nodes) * 32 * sizeof(float), ob = size_t(s->n) * 6 * sizeof(float);
    if (s->nodes.bytes < wb || !s->iow.obox.p || s->iow.obox.bytes < ob) return RT_E_ARG;  // never read past the allocation
    info[0] = sc.n_nodes;
    if (wide) HIP_OK(hipMemcpy(wide, s->nodes.p, wb, hipMemcpyDeviceToHost));
    if (obox) HIP_OK(hipMemcpy(obox, s->iow.obox.p, ob, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_iow_prepare_host(const float *types, const float *records, uint32_t n, float *hot, float *cold,
                              float priors[10]) {
    if (!types || !records || n == 0) return RT_E_ARG;
    try {
        iow_prepare_host(types, records, n, hot, cold, priors);
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

int rt_debug_iow_records(rt_dev_scene *s, float *hot, float *cold, float priors[10]) {
    if (!s || s->kind != 3 || s->broken) return RT_E_ARG;
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipDeviceSynchronize());
    const size_t hb = size_t(s->n) * rtk::kIowHot * sizeof(float), cb = size_t(s->n) * rtk::kIowCold * sizeof(float);
    if (s->hot.bytes < hb || s->cold.bytes < cb) return RT_E_ARG;  // never read past the allocation
    if (hot) HIP_OK(hipMemcpy(hot, s->hot.p, hb, hipMemcpyDeviceToHost));
    if (cold) HIP_OK(hipMemcpy(cold, s->cold.p, cb, hipMemcpyDeviceToHost));
    if (priors) iow_priors_out(s->iow, priors);
    return RT_OK;
}

int rt_debug_update_iow_kernel(int which, int info[4]) {
    if (!info || which < 0 || which > 3) return RT_E_ARG;
    HIP_OK(rtk::update_iow_kernel_info(which, info));
    return RT_OK;
}

int rt_debug_trace_kernel(int any, int fused, int info[4]) {
    if (!info) return RT_E_ARG;
    HIP_OK(rtk::inw_trace_kernel_info(any != 0, fused != 0, info));
    return RT_OK;
}

int rt_debug_trace_iow_kernel(int any, int lds, int info[4]) {
    if (!info) return RT_E_ARG;
    HIP_OK(rtk::iow_trace_kernel_info(any != 0, lds != 0, info));
    return RT_OK;
}

int rt_debug_paths_kernel(int lights, int fused, int info[4]) {
    if (!info) return RT_E_ARG;
    HIP_OK(rtk::inw_paths_kernel_info(lights != 0, fused != 0, info));
    return RT_OK;
}

int rt_debug_paths_max_blocks(int blocks) { return rtk::inw_paths_max_blocks(blocks); }

int rt_debug_path_iow_kernel(int lds_nodes, int info[4]) {
    if (!info) return RT_E_ARG;
    HIP_OK(rtk::iow_paths_kernel_info(lds_nodes != 0, info));
    return RT_OK;
}

int rt_debug_path_iow_max_blocks(int blocks) { return rtk::iow_paths_max_blocks(blocks); }

int rt_debug_pixels_kernel(int which, int info[4]) {
    if (!info || which < 0 || which > 3) return RT_E_ARG;
    HIP_OK(rtk::pixels_kernel_info(which, info));
    return RT_OK;
}

int rt_debug_pass_kernel(int which, int info[4]) {
    if (!info || which < 0 || (which > 3 && which < 8) || which == 15 || (which > 19 && which < 24) || which == 29 ||
        which > 30)
        return RT_E_ARG;
    // rt_adaptive.hip's tile-list instances: an adaptive kernel's `which` + 16 (the scan, 13, serves both)
    if (which >= 24) HIP_OK(rtk::adaptive_kernel_info(which == 30 ? 12 : which - 17, info));
    else if (which >= 16) HIP_OK(rtk::pass_kernel_info(which - 12, info));  // the tile-list instances
    else if (which >= 8) HIP_OK(rtk::adaptive_kernel_info(which - 8, info));  // rt_adaptive.hip's
    else HIP_OK(rtk::pass_kernel_info(which, info));
    return RT_OK;
}

int rt_debug_update_kernel(int which, int info[4]) {
    if (!info || which < 0 || which > 3) return RT_E_ARG;
    HIP_OK(rtk::update_kernel_info(which, info));
    return RT_OK;
}

int rt_debug_pass_max_blocks(int blocks) { return rtk::pass_max_blocks(blocks); }

int rt_debug_adaptive_chunk(int samples) { return rtk::adaptive_chunk_cap(samples); }

}  // extern "C"
