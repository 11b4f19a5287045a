// rt_scene_build.hip -- scene construction: converts the reference's record layouts into the
// kernels' device layouts (hot/cold split, per-object reciprocals hoisted under the numerics
// contract), builds the sample tables, the walk structures (host and device builds) and the
// textures, and redoes that per redraw (update_inw, update_inw_device, update_iow03, update_iow03_device).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_dev_scene.hpp"

int g_build_levels = 0;

namespace {

int build_tables(rt_dev_scene *s, int spp) {
    std::vector<float> sf(size_t(spp) * 2), fib3(size_t(spp) * 3), fib4(size_t(spp) * 4, 0.0f);
    std::vector<int> ring(size_t(spp) * 2);
    rtamd::sample_tables(spp, sf.data(), fib3.data(), ring.data());
    for (int i = 0; i < spp; i++)
        for (int k = 0; k < 3; k++) fib4[size_t(i) * 4 + k] = fib3[size_t(i) * 3 + k];
    HIP_OK(s->sunflower.upload(sf.data(), sf.size() * sizeof(float)));
    s->sf_max = 0.0f;
    for (int i = 0; i < spp; i++)
        s->sf_max = std::fmax(s->sf_max, std::fabs(sf[size_t(i) * 2]) + std::fabs(sf[size_t(i) * 2 + 1]));
    HIP_OK(s->fib.upload(fib4.data(), fib4.size() * sizeof(float)));
    HIP_OK(s->ring.upload(ring.data(), ring.size() * sizeof(int)));
    s->spp = spp;
    s->s_stop = spp;
    for (int i = 0; i < spp; i++)
        if (ring[size_t(i) * 2] < 0) { s->s_stop = i; break; }
    HIP_OK(s->counter.alloc(1024));  // queue counters 64 B apart (the INW fold launches: two, + 8 XCD queues)
    HIP_OK(s->fold.mode.alloc(64));
    return RT_OK;
}

// Persistent grid = the blocks the device keeps resident (a work-queue kernel gains nothing
// from more: extra blocks would only start after the queue ran dry).
void set_residency(rt_dev_scene *s) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    s->cus = cus;
    using rtk::RenderKernel;
    const RenderKernel own = s->kind == 3 ? RenderKernel::Iow03 : (s->kind == 14 ? RenderKernel::Inw04 : RenderKernel::Inw01);
    s->blocks_cap = cus * rtk::resident_blocks_per_cu(own);
    if (s->kind == 3)  // continuation buffers serve every IOW-03 variant
        s->blocks_cap = std::max({s->blocks_cap, cus * rtk::resident_blocks_per_cu(RenderKernel::Iow03Narrow),
                                  cus * rtk::resident_blocks_per_cu(RenderKernel::Iow03Spec)});
    else  // and the INW-01 per-pixel kernel
        s->blocks_cap = std::max(s->blocks_cap, cus * rtk::resident_blocks_per_cu(RenderKernel::Inw01));
}

// u_MaterialTextures[0..n_tex) (04...glsl:10; bound by GeometryData_04::BindExtraData,
// lights.cpp:22): unorm8 texels -> float (c / 255, the GL conversion) once, on the host
int upload_textures(rt_dev_scene *s, const rt_texture *tex, int n_tex) {
    s->n_tex = 0;
    if (n_tex == 0) {
        HIP_OK(s->tex.alloc(16));
        HIP_OK(s->tex_info.alloc(16));
        return RT_OK;
    }
    size_t total = 0;
    std::vector<int> info(size_t(n_tex) * 4, 0);
    for (int k = 0; k < n_tex; k++) {
        info[4 * k] = int(total);
        info[4 * k + 1] = tex[k].width;
        info[4 * k + 2] = tex[k].height;
        total += size_t(tex[k].width) * size_t(tex[k].height);
    }
    if (total > (size_t(1) << 31)) return RT_E_ARG;
    std::vector<float> texels(total * 4, 0.0f);
    for (int k = 0; k < n_tex; k++) {
        const size_t m = size_t(tex[k].width) * size_t(tex[k].height);
        const int ch = tex[k].channels;
        float *o = texels.data() + size_t(info[4 * k]) * 4;
        for (size_t i = 0; i < m; i++) {
            for (int c = 0; c < 3; c++) o[4 * i + c] = float(tex[k].texels[i * ch + c]) / 255.0f;
            o[4 * i + 3] = ch == 4 ? float(tex[k].texels[i * ch + 3]) / 255.0f : 1.0f;
        }
    }
    HIP_OK(s->tex.upload(texels.data(), texels.size() * sizeof(float)));
    HIP_OK(s->tex_info.upload(info.data(), info.size() * sizeof(int)));
    s->n_tex = uint32_t(n_tex);
    return RT_OK;
}

// Whether a scene takes the wide walk: rt_options.inw_wide_walk, and every object inside its leaf box
// up to the margin of rtamd::inw_stick_out (DESIGN.md §2 "Objects inside their leaf boxes").  A scene
// with caller boxes that an object sticks out of is built as with inw_wide_walk = 0: the reference's
// LBVH walks, no beam lists, no RI grid.  boxes / stride as inw_stick_out takes them.
bool inw_wide_ok(const rt_dev_scene *s, const float *geom, uint32_t n, const float *boxes, uint32_t stride) {
    return s->opt.inw_wide_walk && n >= 2 && rtamd::inw_stick_out(geom, n, boxes, stride) <= 1.0;
}

// The quantised culling BVH (DESIGN.md §5.2 "Quantised nodes") from the scene's wide nodes, on the
// device: planes rounded outward by kQMargin beyond the wide nodes' own (the error bound of the
// walk's decode is below it while every coordinate lies within 1000 of the origin, the fused
// cull's condition, which the launch checks per frame).  The two kernels run on `st` (the null stream
// for every entry point but rt_dev_scene_inw_update_device); the wait at the end makes the derived
// nodes complete before any caller returns the scene, so a render enqueued at once on a non-blocking
// stream reads finished nodes.
constexpr float kQMargin = 2e-3f;
int make_qnodes(InwWalk &w, hipStream_t st = nullptr) {
    if (!w.n_wnodes) return RT_OK;
    HIP_OK(w.cnodes.reserve(size_t(w.n_wnodes) * 7 * sizeof(float4)));
    HIP_OK(rtk::inw_compact_wnodes(w.wnodes.as<float4>(), w.n_wnodes, w.cnodes.as<float4>(), st));
    HIP_OK(w.qnodes.reserve(size_t(w.n_wnodes) * rtk::kQNodeF4 * sizeof(float4)));
    HIP_OK(rtk::inw_quantize_wnodes(w.wnodes.as<float4>(), w.n_wnodes, w.qnodes.as<float4>(), kQMargin, st));
    HIP_OK(hipStreamSynchronize(st));
    return RT_OK;
}

// The wide walk's structures and the RI grid, built on the host (rtamd::inw_wide_build,
// rtamd::ri_grid_build) and uploaded.
// ms (may be null): host time of the builds, then of the uploads
// geom (may be null): the reference's GeometryBuff records, for the time-bin trees
// wide: the scene takes the wide walk (inw_wide_ok)
int make_inw_wide(rt_dev_scene *s, const float *nodes, uint32_t n, bool wide, double *ms = nullptr,
                  const float *geom = nullptr) {
    InwWalk &d = s->walk;
    d.reset();
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t high = 0;
    bool sl = false;
    const bool walkable = rtamd::lbvh_walk_info(nodes, n, high, sl);
    rtamd::InwWide w;
    rtamd::RiGrid g;
    const bool ok = walkable && wide && rtamd::inw_wide_build(nodes, n, w);
    if (ok) g = rtamd::ri_grid_build(w.leafbox.data(), n);
    if (ok && geom && s->opt.inw_time_bins > 1) rtamd::inw_wide_add_bins(geom, n, uint32_t(s->opt.inw_time_bins), w);
    const auto t1 = std::chrono::steady_clock::now();
    if (ms) ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (!ok) {  // the reference walk only (stackless where it cannot drop a push)
        if (walkable) { d.dfs_high = high; d.sl_ok = sl; }
        return RT_OK;
    }
    HIP_OK(d.wnodes.store(w.wnodes.data(), w.wnodes.size() * sizeof(float)));
    HIP_OK(d.wrank.store(w.rank.data(), w.rank.size() * sizeof(uint32_t)));
    HIP_OK(d.wleaf.store(w.leafbox.data(), w.leafbox.size() * sizeof(float)));
    if (g.ok) {
        HIP_OK(d.ri_cells.store(g.cells.data(), g.cells.size() * sizeof(uint32_t)));
        HIP_OK(d.ri_ids.store(g.ids.data(), std::max<size_t>(1, g.ids.size()) * sizeof(uint32_t)));
        d.ri_ok = true;
        for (int a = 0; a < 3; a++) {
            d.ri_lo[a] = g.lo[a]; d.ri_hi[a] = g.hi[a]; d.ri_inv[a] = g.inv[a]; d.ri_dim[a] = g.dim[a];
        }
    }
    d.n_wnodes = uint32_t(w.wnodes.size() / 40);
    d.n_wtree0 = w.n_tree0;
    d.wbins = w.bins;
    d.wbin_stride = w.bin_stride;
    d.dfs_high = w.dfs_high;
    d.sl_ok = sl;
    d.wdepth = w.depth;
    d.wbound = w.wbound;
    if (int rc = make_qnodes(d); rc != RT_OK) return rc;
    if (ms) ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    return RT_OK;
}

// The same structures built on the device from the scene's device LBVH (rt_build.hip, DESIGN.md
// "Device build"; rt_options.inw_device_build): no host build, no upload.  Two steps, both on `st`:
// the swept tree, ranks, leaf boxes and high-water mark (RT_E_UNSUPPORTED: deeper than the level cap,
// the caller builds on the host), then, for a scene that takes the wide walk, the RI grid and the
// walk's counts (the derived nodes follow: make_qnodes).
int inw_swept_build_device(rt_dev_scene *s, uint32_t n, rtk::InwWideDev &out, hipStream_t st) {
    InwWalk &d = s->walk;
    HIP_OK(d.wnodes.reserve(size_t(n) * 40 * sizeof(float)));
    HIP_OK(d.wrank.reserve(size_t(n) * 2 * sizeof(uint32_t)));
    HIP_OK(d.wleaf.reserve(size_t(n) * 8 * sizeof(float)));
    const size_t wsb = rtk::inw_build_workspace_bytes(n);
    HIP_OK(d.build_ws.reserve(wsb));
    out = rtk::InwWideDev{d.wnodes.as<float4>(), d.wrank.as<uint32_t>(), d.wleaf.as<float4>(), 0, 0, 0, 0.0f, {}, {}};
    const hipError_t be = rtk::inw_wide_build_device(s->nodes.as<float4>(), d.lcnt.as<uint32_t>(), n,
                                                     d.build_ws.p, d.build_ws.bytes, out, st, g_build_levels);
    if (be == hipErrorNotSupported) return RT_E_UNSUPPORTED;  // deeper than its level cap: the caller builds on the host
    HIP_OK(be);
    return RT_OK;
}
int inw_swept_commit_device(rt_dev_scene *s, uint32_t n, const rtk::InwWideDev &out, hipStream_t st) {
    InwWalk &d = s->walk;
    double dlo[3], dhi[3], inv[3];
    int dim[3];
    for (int a = 0; a < 3; a++) { dlo[a] = out.ri_lo[a]; dhi[a] = out.ri_hi[a]; }
    if (rtamd::ri_grid_dims(dlo, dhi, n, dim, inv)) {
        const size_t nc = size_t(dim[0]) * dim[1] * dim[2];
        HIP_OK(d.ri_cells.reserve((nc + 1) * sizeof(uint32_t)));
        const size_t tb = rtk::ri_scan_temp_bytes(nc + 1);
        HIP_OK(d.ri_tmp.reserve(tb));
        uint32_t total = 0, over = 0;
        HIP_OK(rtk::ri_count_device(d.wleaf.as<float4>(), n, d.build_ws.p, dlo, inv, dim, d.ri_cells.as<uint32_t>(),
                                    d.ri_tmp.p, tb, &total, &over, st));
        if (!over) {
            HIP_OK(d.ri_ids.reserve(std::max<size_t>(1, total) * sizeof(uint32_t)));
            HIP_OK(d.ri_fill.reserve(std::max<size_t>(1, nc) * sizeof(uint32_t)));
            HIP_OK(rtk::ri_fill_device(d.wleaf.as<float4>(), n, dlo, inv, dim, d.ri_cells.as<uint32_t>(),
                                       d.ri_fill.as<uint32_t>(), d.ri_ids.as<uint32_t>(), st));
            for (int a = 0; a < 3; a++) {
                d.ri_lo[a] = float(dlo[a]); d.ri_hi[a] = float(dhi[a]); d.ri_inv[a] = float(inv[a]);
                d.ri_dim[a] = dim[a];
            }
            d.ri_ok = true;
        }
    }
    d.n_wnodes = d.n_wtree0 = out.n_wnodes;
    d.wdepth = out.depth;
    d.wbound = out.wbound;
    return RT_OK;
}

// rt_dev_scene_inw_update's device build: the two steps on the null stream.  ms: host wall time of
// the build (its level loop and the RI grid read counts back) in ms[0], 0 in ms[1].
int make_inw_wide_device(rt_dev_scene *s, uint32_t n, bool wide, double *ms) {
    InwWalk &d = s->walk;
    d.reset();
    const auto t0 = std::chrono::steady_clock::now();
    rtk::InwWideDev out{};
    if (int rc = inw_swept_build_device(s, n, out, nullptr); rc != RT_OK) return rc;
    if (wide) {
        if (int rc = inw_swept_commit_device(s, n, out, nullptr); rc != RT_OK) return rc;
        if (int rc = make_qnodes(d); rc != RT_OK) return rc;
    }
    HIP_OK(hipDeviceSynchronize());  // the build kernels too
    d.dfs_high = out.dfs_high;
    d.sl_ok = true;  // the device LBVH has the stackless layout by construction (rt_lbvh.hip)
    if (ms) {
        ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ms[1] = 0.0;
    }
    return RT_OK;
}

// The time-bin trees of a device-built scene (rtamd::inw_wide_add_bins' trees and layout, built by
// rtk::inw_bin_trees_device from the records at d_geom) appended to the swept tree the scene's walk
// holds.  RT_E_UNSUPPORTED: a tree ran past the level cap (the caller builds on the host).  The scene
// keeps the swept tree alone (RT_OK) when the trees would not fit the walkers' ids: the buffer-load
// walk multiplies node ids with __umul24 and counts records in 32 bits, so all trees together stay
// below 2^24 nodes and 2^32 bytes.
int add_bins_device(rt_dev_scene *s, const float *d_geom, uint32_t n, uint32_t bins, hipStream_t st) {
    InwWalk &d = s->walk;
    constexpr uint64_t kMaxNodes = uint64_t(1) << 24, kMaxBytes = uint64_t(1) << 32, kNodeBytes = 10 * sizeof(float4);
    auto fits = [&](uint64_t nodes) { return nodes < kMaxNodes && nodes * kNodeBytes < kMaxBytes; };
    // (a 4-wide tree over n objects has at least (n - 1) / 3 nodes: scenes that cannot fit build nothing)
    if (!fits(uint64_t(d.n_wtree0) + uint64_t(bins) * ((n - 1) / 3))) return RT_OK;
    HIP_OK(d.wbin_tmp.reserve(size_t(bins) * n * kNodeBytes));
    rtk::InwBinsDev t{};
    const hipError_t be = rtk::inw_bin_trees_device(d_geom, n, bins, d.build_ws.p, d.build_ws.bytes,
                                                    d.wbin_tmp.as<float4>(), t, st, g_build_levels);
    if (be == hipErrorNotSupported) return RT_E_UNSUPPORTED;
    HIP_OK(be);
    const uint64_t total = uint64_t(d.n_wtree0) + uint64_t(bins) * t.stride;
    if (!fits(total)) return RT_OK;
    if (d.wnodes.bytes < total * kNodeBytes) {  // a larger node array that keeps the swept tree (with room to grow)
        DevBuf grown;
        HIP_OK(grown.alloc(size_t(total + total / 8) * kNodeBytes));
        HIP_OK(hipMemcpyAsync(grown.p, d.wnodes.p, size_t(d.n_wtree0) * kNodeBytes, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
        std::swap(grown.p, d.wnodes.p);
        std::swap(grown.bytes, d.wnodes.bytes);
    }
    HIP_OK(rtk::inw_bin_place_device(d.wbin_tmp.as<float4>(), n, bins, t, d.n_wtree0, d.wnodes.as<float4>(), st));
    d.n_wnodes = uint32_t(total);
    d.wbins = bins;
    d.wbin_stride = t.stride;
    d.wbound = std::fmax(d.wbound, t.wbound);
    return RT_OK;
}

// The kernels' hot / cold records from the reference's GeometryBuff(_04) records (28 floats).
void inw_records(const float *geom, uint32_t n, int layout, std::vector<float> &hot, std::vector<float> &cold) {
    hot.assign(size_t(n) * rtk::kInwHot, 0.0f);
    cold.assign(size_t(n) * rtk::kInwCold, 0.0f);
    for (uint32_t j = 0; j < n; j++) {
        const float *f = geom + size_t(j) * 28;
        float *h = hot.data() + size_t(j) * rtk::kInwHot;
        float *c = cold.data() + size_t(j) * rtk::kInwCold;
        for (int k = 0; k < 20; k++) h[k] = f[k];  // pos R scale delta type extra
        bool ident = true;  // the rotation exactly the identity (entries 1 and +-0): type + 0.5 (rtk::Xf::ident)
        for (int k = 0; k < 9; k++) ident = ident && f[3 + k] == ((k % 4) == 0 ? 1.0f : 0.0f);
        if (ident && (f[18] == 1.0f || f[18] == 2.0f)) h[18] = f[18] + 0.5f;
        for (int k = 0; k < 3; k++) {
            h[20 + k] = 1.0f / f[12 + k];                  // a / scale  -> a * RN(1/scale)
            h[23 + k] = 1.0f / (f[12 + k] * f[12 + k]);    // a / (s*s)  -> a * RN(1/RN(s*s))
        }
        h[26] = layout == 4 ? f[19] : f[20];  // RI accumulated by the surrounding-RI walk
        if (layout == 1) {  // BVH.h:6-19
            c[0] = f[21]; c[1] = f[22]; c[2] = f[23]; c[3] = f[24];
            c[4] = f[25]; c[5] = f[26]; c[6] = f[27]; c[7] = f[20];
        } else {            // lights.h:6-21
            c[0] = f[20]; c[1] = f[21]; c[2] = f[22]; c[3] = f[23];
            c[4] = f[24]; c[5] = f[25]; c[6] = f[26];
            // TextureIndex = uint(texel 6.w + 0.1) (04...glsl:414), as uint bits; the RI (f[19])
            // reaches the kernel as IntersectRay's extra data instead
            const float ti = f[27] + 0.1f;
            const uint32_t tu = ti <= 0.0f ? 0u : (ti >= 4294967040.0f ? 0xffffffffu : uint32_t(ti));
            std::memcpy(&c[7], &tu, 4);
        }
    }
}

}  // namespace

bool inw_textured(const float *geom, uint32_t n, int layout) {
    if (layout != 4) return false;
    for (uint32_t g = 0; g < n; g++)
        if (geom[size_t(g) * 28 + 27] + 0.1f >= 1.0f) return true;
    return false;
}

bool textures_ok(const rt_texture *tex, int n_tex) {
    if (n_tex < 0 || (n_tex > 0 && !tex)) return false;
    for (int k = 0; k < n_tex; k++)
        if (!tex[k].texels || tex[k].width <= 0 || tex[k].height <= 0 || (tex[k].channels != 3 && tex[k].channels != 4) ||
            size_t(tex[k].width) * size_t(tex[k].height) > (size_t(1) << 31))
            return false;
    return true;
}

// The kernels' hot / cold records from the reference's IOW-03 records (24 floats) and types.
static void iow_records(const float *types, const float *rec, uint32_t n, std::vector<float> &hot, std::vector<float> &cold) {
    hot.assign(size_t(n) * rtk::kIowHot, 0.0f);
    cold.assign(size_t(n) * rtk::kIowCold, 0.0f);
    for (uint32_t j = 0; j < n; j++) {
        const float *r = rec + size_t(j) * 24;
        float *h = hot.data() + size_t(j) * rtk::kIowHot;
        float *c = cold.data() + size_t(j) * rtk::kIowCold;
        h[0] = r[0]; h[1] = r[1]; h[2] = r[2];
        h[3] = types[j];
        for (int k = 0; k < 9; k++) h[4 + k] = r[3 + k];
        for (int k = 0; k < 3; k++) { h[13 + k] = r[12 + k]; h[16 + k] = 1.0f / r[12 + k]; }
        for (int k = 0; k < 3; k++) { c[k] = r[15 + k]; c[3 + k] = r[18 + k]; }
        c[6] = r[21]; c[7] = r[22];
        // glm::mat3(1) bit pattern (+0 off-diagonal): the kernel may reuse the ray's
        // identity-transformed direction, which is bit-identical to transforming it here
        static const float kI[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        h[19] = std::memcmp(r + 3, kI, sizeof(kI)) == 0 ? 1.0f : 0.0f;
    }
}

// The RI priors of the sample-parallel pipeline: the most common RefractiveIndex (record float 20,
// Geometry::FillBuffer materials.h:48-76) and the values a stale ray-stack RI can hold.
static void iow_priors(const float *rec, uint32_t n, IowCullPriors &q) {
    std::vector<float> ri(n);
    for (uint32_t j = 0; j < n; j++) ri[j] = rec[size_t(j) * 24 + 20];
    std::sort(ri.begin(), ri.end());
    size_t best = 0;
    for (size_t i = 0; i < ri.size();) {
        size_t k = i;
        while (k < ri.size() && ri[k] == ri[i]) k++;
        if (k - i > best) { best = k - i; q.ri_prior = ri[i]; }
        i = k;
    }
    std::vector<float> vals{0.0f, 1.0f};
    vals.insert(vals.end(), ri.begin(), ri.end());
    std::sort(vals.begin(), vals.end());
    vals.erase(std::unique(vals.begin(), vals.end(), [](float a, float b) {
        return std::memcmp(&a, &b, sizeof(a)) == 0; }), vals.end());
    q.n_alt_vals = 0;
    if (vals.size() <= 8) {
        for (size_t v = 0; v < vals.size(); v++) q.alt_vals[v] = vals[v];
        q.n_alt_vals = int(vals.size());
    }
}

int make_iow03(rt_dev_scene *s, const float *types, const float *rec, uint32_t n, int spp) {
    std::vector<float> hot, cold;
    iow_records(types, rec, n, hot, cold);
    s->kind = 3; s->n = n;
    IowCullPriors &q = s->iow;
    iow_priors(rec, n, q);
    HIP_OK(s->hot.upload(hot.data(), hot.size() * sizeof(float)));
    HIP_OK(s->cold.upload(cold.data(), cold.size() * sizeof(float)));
    // Culling BVH over the objects (the reference loops linearly; rtk::iow_launch_ray keeps its
    // exact result); iow_linear: the reference's linear loop (A/B)
    rtamd::IowCull cull;
    if (!s->opt.iow_linear && rtamd::iow_cull_build(types, rec, n, cull)) {
        HIP_OK(s->nodes.upload(cull.wide.data(), cull.wide.size() * sizeof(float)));
        q.root_link = 1;
        q.n_wide = cull.n_wide;
        q.depth = cull.depth;
        HIP_OK(q.obox.upload(cull.obox.data(), cull.obox.size() * sizeof(float)));
    }
    set_residency(s);
    return build_tables(s, spp);
}

// Objects from which the library's choice (flags = 0) builds the culling BVH on the device, read from
// the measured rows of DESIGN.md §5.12: the device build beats the host build at every measured size
// (0.35 against 0.48 ms at 485 objects, 0.38 against 1.03 ms at 1024), but at the C2 scene (486
// objects) its binned tree costs the frame more than the build saves (+6.8% node visits, +2.1% frame
// time), so that size keeps the host build and the next measured one is the threshold.
constexpr uint32_t kIowDeviceBuildMin = 1024;

namespace {

// The two IOW-03 updates' clock: ms[0..2] by laps, ms[3] the whole call.
struct UpdateClock {
    using clk = std::chrono::steady_clock;
    clk::time_point t_call = clk::now(), t = t_call;
    double lap() {
        const auto now = clk::now();
        const double v = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return v;
    }
    double total() const { return std::chrono::duration<double, std::milli>(clk::now() - t_call).count(); }
};

// Where the records of an IOW-03 update live.  types / rec: on the host (rt_dev_scene_iow03_update), or
// null with d_types / d_rec on the device and the priors' ten words at d_priors
// (rt_dev_scene_iow03_update_device; the host builder then gets one copy-back, n * 25 floats).
struct IowUpdateSrc {
    const float *types, *rec;
    const float *d_types, *d_rec;
    const uint32_t *d_priors;
};

void set_priors(IowCullPriors &q, const uint32_t w[10]) {
    q.ri_prior = __builtin_bit_cast(float, w[0]);
    for (int v = 0; v < 8; v++) q.alt_vals[v] = __builtin_bit_cast(float, w[1 + v]);
    q.n_alt_vals = int(__builtin_bit_cast(float, w[9]));
}

// What both updates do once the scene's hot and cold records are in place (enqueued on `st` or stored):
// the object boxes and the culling BVH -- on the device (rtk::iow_cull_build_device) or
// by rtamd::iow_cull_build as make_iow03 builds it, which is also the fallback of a device build that
// ran past its level cap or met a box that is not finite -- then, for records on the device, the
// priors' words (in the build's own read-back where the device build succeeded), the wait, and the
// commit of the new sizes.  ms[1], ms[2], ms[3] as the two callers document them.
int iow_update_finish(rt_dev_scene *s, const IowUpdateSrc &src, uint32_t n, int flags, hipStream_t st, UpdateClock &ck,
                      double *ms) {
    IowCullPriors &q = s->iow;
    // a scene created with iow_linear keeps the linear loop; n < 2 or n >= 16384 has no BVH, as
    // rtamd::iow_cull_build decides
    const bool bvh = !s->opt.iow_linear && n >= 2 && n < 16384;
    const bool device_build = flags == RT_UPDATE_DEVICE_BUILD || (flags == 0 && n >= kIowDeviceBuildMin);
    uint32_t n_wide = 0, built = 0;
    int depth = 0;
    bool host_build = bvh && !device_build, have_priors = !src.d_priors;
    uint32_t pw[10];
    if (bvh && device_build) {
        HIP_OK(s->nodes.reserve(size_t(n) * 8 * sizeof(float4)));
        HIP_OK(q.obox.reserve(size_t(n) * 6 * sizeof(float)));
        HIP_OK(q.build_ws.reserve(rtk::inw_build_workspace_bytes(n)));
        rtk::IowCullDev out{};
        const hipError_t be = rtk::iow_cull_build_device(s->hot.as<float>(), n, q.build_ws.p, q.build_ws.bytes,
                                                         s->nodes.as<float4>(), q.obox.as<float4>(), out, st,
                                                         g_build_levels, src.d_priors);
        // deeper than the level cap (a chain-like scene), or a box that is not finite (the binned
        // splits mean nothing then): the host builder, whose scene equals a fresh one by construction
        if (be == hipErrorNotSupported) { built = 2; host_build = true; }
        else {
            HIP_OK(be);
            if (out.nonfinite) { built = 3; host_build = true; }
            else { built = 1; n_wide = out.n_wide; depth = out.depth; }
            if (src.d_priors) { std::memcpy(pw, out.priors, sizeof(pw)); have_priors = true; }
        }
    }
    double t_build = ck.lap(), t_up = 0.0;
    if (!have_priors) HIP_OK(hipMemcpyAsync(pw, src.d_priors, sizeof(pw), hipMemcpyDeviceToHost, st));
    if (host_build) {
        const float *types = src.types, *rec = src.rec;
        std::vector<float> back;
        if (!rec) {  // the one copy-back: types, then records
            back.resize(size_t(n) * 25);
            HIP_OK(hipMemcpyAsync(back.data(), src.d_types, size_t(n) * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(back.data() + n, src.d_rec, size_t(n) * 24 * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            types = back.data();
            rec = back.data() + n;
            t_up += ck.lap();
        }
        rtamd::IowCull cull;
        if (!rtamd::iow_cull_build(types, rec, n, cull)) return RT_E_ARG;  // (bvh: it builds)
        t_build += ck.lap();
        HIP_OK(s->nodes.store(cull.wide.data(), cull.wide.size() * sizeof(float)));
        HIP_OK(q.obox.store(cull.obox.data(), cull.obox.size() * sizeof(float)));
        n_wide = cull.n_wide;
        depth = cull.depth;
        t_up += ck.lap();
    }
    // every copy and build kernel: a render on any stream may follow
    if (src.d_priors) HIP_OK(hipStreamSynchronize(st));
    else HIP_OK(hipDeviceSynchronize());
    if (src.d_priors) set_priors(q, pw);
    q.root_link = bvh ? 1 : 0;
    q.n_wide = n_wide;
    q.depth = depth;
    q.built = built;
    q.updates++;
    s->n = n;
    s->broken = false;
    if (ms) { ms[1] = t_build; ms[2] = t_up; ms[3] = ck.total(); }
    return RT_OK;
}

}  // namespace

// The next edit of an IOW-03 scene on its existing device buffers (rt_dev_scene_iow03_update; the
// reference's CopyObjBuffer per ImGui edit, 03_Shadows_and_Materials/materials.cpp:329-364): new hot
// and cold records and the RI priors from the host's arrays, then the object boxes and the culling BVH
// (iow_update_finish).  The sample tables, workspaces and speculation records stay.  ms[4]: host time of
// the records and priors with their uploads, the boxes and the BVH, the upload of host-built structures,
// the call.
int update_iow03(rt_dev_scene *s, const float *types, const float *rec, uint32_t n, int flags, double *ms) {
    UpdateClock ck;
    if (ms) ms[0] = ms[1] = ms[2] = ms[3] = 0.0;
    // Until every step below has succeeded the buffers may hold a mix of the old and the new scene:
    // the scene refuses renders and queries and keeps its old n and counts, so nothing indexes past
    // a buffer.  The new sizes are committed at the end.
    s->broken = true;
    std::vector<float> hot, cold;
    iow_records(types, rec, n, hot, cold);
    iow_priors(rec, n, s->iow);
    HIP_OK(s->hot.store(hot.data(), hot.size() * sizeof(float)));
    HIP_OK(s->cold.store(cold.data(), cold.size() * sizeof(float)));
    const double t0 = ck.lap();
    if (ms) ms[0] = t0;
    return iow_update_finish(s, IowUpdateSrc{types, rec, nullptr, nullptr, nullptr}, n, flags, nullptr, ck, ms);
}

// update_iow03 for types and records that live on the scene's device (rt_dev_scene_iow03_update_device,
// DESIGN.md §5.18): the hot and cold records by k_iow_prepare, the priors by a sort of the RI keys and a
// run-length pass, all on `st` in the scene's build workspace (the BVH build's pieces first, the
// prepare's after them), then iow_update_finish on `st`.  With the device build no record byte crosses
// to the host: ten words of priors come back with the build's counts.  ms[4]: host time of the records
// and priors (their enqueue), the boxes and the BVH, the copy-back plus the upload of host-built
// structures, the call.
int update_iow03_device(rt_dev_scene *s, const float *d_types, const float *d_rec, uint32_t n, int flags, hipStream_t st,
                        double *ms) {
    UpdateClock ck;
    if (ms) ms[0] = ms[1] = ms[2] = ms[3] = 0.0;
    s->broken = true;  // (as update_iow03: the new sizes are committed at the end)
    IowCullPriors &q = s->iow;
    HIP_OK(s->hot.reserve(size_t(n) * rtk::kIowHot * sizeof(float)));
    HIP_OK(s->cold.reserve(size_t(n) * rtk::kIowCold * sizeof(float)));
    const size_t build_bytes = rtk::inw_build_workspace_bytes(n), prep_bytes = rtk::iow_prepare_workspace_bytes(n);
    HIP_OK(q.build_ws.reserve(build_bytes + prep_bytes));
    const uint32_t *d_priors = nullptr;
    HIP_OK(rtk::iow_prepare_device(d_types, d_rec, n, s->hot.as<float>(), s->cold.as<float>(),
                                   static_cast<char *>(q.build_ws.p) + build_bytes, prep_bytes, &d_priors, st));
    const double t0 = ck.lap();
    if (ms) ms[0] = t0;
    return iow_update_finish(s, IowUpdateSrc{nullptr, nullptr, d_types, d_rec, d_priors}, n, flags, st, ck, ms);
}

void iow_prepare_host(const float *types, const float *rec, uint32_t n, float *hot, float *cold, float priors[10]) {
    std::vector<float> h, c;
    iow_records(types, rec, n, h, c);
    IowCullPriors q;
    iow_priors(rec, n, q);
    if (hot) std::memcpy(hot, h.data(), h.size() * sizeof(float));
    if (cold) std::memcpy(cold, c.data(), c.size() * sizeof(float));
    if (priors) iow_priors_out(q, priors);
}

void iow_priors_out(const IowCullPriors &q, float priors[10]) {
    priors[0] = q.ri_prior;
    for (int v = 0; v < 8; v++) priors[1 + v] = v < q.n_alt_vals ? q.alt_vals[v] : 0.0f;  // (slots past the count are stale)
    priors[9] = float(q.n_alt_vals);
}

// Sphere records (rtk::InwScene::sph) when every object is an ellipsoid with equal scales and the
// identity rotation (entries exactly 1 and +-0): (position, RN(1/scale)), (position - last_position,
// RI), (RN(1/RN(scale^2)) per axis, extra).  false: some object is not.
bool inw_sphere_records(const float *geom, uint32_t n, int layout, std::vector<float> &out) {
    out.assign(size_t(n) * 12, 0.0f);
    for (uint32_t j = 0; j < n; j++) {
        const float *f = geom + size_t(j) * 28;
        if (int(f[18] + 0.1f) != 1 || !(f[12] == f[13] && f[13] == f[14]) || !std::isfinite(f[12])) return false;
        for (int k = 0; k < 9; k++)
            if (f[3 + k] != ((k % 4) == 0 ? 1.0f : 0.0f)) return false;
        float *o = out.data() + size_t(j) * 12;
        o[0] = f[0]; o[1] = f[1]; o[2] = f[2]; o[3] = 1.0f / f[12];  // the hot record's is (RN(1/scale))
        o[4] = f[15]; o[5] = f[16]; o[6] = f[17];
        o[7] = layout == 4 ? f[19] : f[20];  // the RI the surrounding-RI walk adds (the hot record's)
        for (int k = 0; k < 3; k++) o[8 + k] = 1.0f / (f[12 + k] * f[12 + k]);  // the hot record's is2
        o[11] = f[19];  // its extra data
    }
    return n > 0;
}

int make_inw(rt_dev_scene *s, const float *geom, uint32_t n, int layout, const float *nodes,
             const float *lights, uint32_t n_lights, const rt_texture *tex, int n_tex, int spp) {
    if (int rc = upload_textures(s, layout == 4 ? tex : nullptr, layout == 4 ? n_tex : 0); rc != RT_OK) return rc;
    std::vector<float> hot, cold;
    inw_records(geom, n, layout, hot, cold);
    s->kind = layout == 4 ? 14 : 11;
    s->n = n; s->layout = layout; s->n_lights = layout == 4 ? n_lights : 0;
    HIP_OK(s->hot.store(hot.data(), hot.size() * sizeof(float)));
    HIP_OK(s->cold.store(cold.data(), cold.size() * sizeof(float)));
    {
        std::vector<float> sph;
        s->sph_ok = inw_sphere_records(geom, n, layout, sph);
        if (s->sph_ok) HIP_OK(s->sph.store(sph.data(), sph.size() * sizeof(float)));
    }
    HIP_OK(s->nodes.store(nodes, size_t(2 * n - 1) * 8 * sizeof(float)));
    if (int rc = make_inw_wide(s, nodes, n, inw_wide_ok(s, geom, n, nodes, 0), nullptr, geom); rc != RT_OK) return rc;
    if (s->n_lights) HIP_OK(s->lights.store(lights, size_t(s->n_lights) * 7 * sizeof(float)));
    else HIP_OK(s->lights.store(nullptr, 0));
    set_residency(s);
    return build_tables(s, spp);
}

// RT_Base<>::OnUpdateBase's per-redraw work on an existing device scene (In-Next-Week/base.h:
// 96-175): new records, the LBVH (the caller's, or built on the device from the boxes), the wide
// walk and RI grid rebuilt on the host, every upload into the scene's buffers.  ms[4]: host time
// of the records, the LBVH (upload + device build + read-back), the host structures, their upload.
int update_inw(rt_dev_scene *s, const float *geom, uint32_t n, const float *nodes, const float *aabbs,
               const float *lights, uint32_t n_lights, double *ms) {
    using clk = std::chrono::steady_clock;
    auto t = clk::now();
    auto lap = [&](int k) {
        const auto now = clk::now();
        if (ms) ms[k] = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    };
    if (n > (1u << 24)) return RT_E_UNSUPPORTED;  // node / object ids are stored as floats (exact to 2^24)
    // the wide walk's structures and the RI grid built on the device from the device LBVH
    // (rt_options.inw_device_build; a caller's host LBVH keeps the host builders)
    const bool device_build = s->opt.inw_device_build && !nodes && n >= 2;
    const float *const caller_nodes = nodes;
    // Until every step below has succeeded the buffers may hold a mix of the old and the new
    // scene (sizes included): the scene refuses renders (launch_scene) and keeps its old n and
    // counts, so nothing indexes past a buffer.  The new sizes are committed at the end.
    s->broken = true;
    std::vector<float> hot, cold;
    inw_records(geom, n, s->layout, hot, cold);
    const uint32_t nl = s->layout == 4 ? n_lights : 0;
    HIP_OK(s->hot.store(hot.data(), hot.size() * sizeof(float)));
    HIP_OK(s->cold.store(cold.data(), cold.size() * sizeof(float)));
    {
        std::vector<float> sph;
        s->sph_ok = false;  // (the scene is marked broken until the update completes)
        if (inw_sphere_records(geom, n, s->layout, sph)) {
            HIP_OK(s->sph.store(sph.data(), sph.size() * sizeof(float)));
            s->sph_ok = true;
        }
    }
    if (nl) HIP_OK(s->lights.store(lights, size_t(nl) * 7 * sizeof(float)));
    lap(0);
    InwWalk &d = s->walk;
    const size_t nbytes = size_t(2 * n - 1) * 8 * sizeof(float);
    std::vector<float> host_nodes;
    if (!nodes) {  // ConstructLBVH_Buff on the device (rt_lbvh_build_async), read back for the host builders
        HIP_OK(s->nodes.reserve(nbytes));
        HIP_OK(d.aabb.store(aabbs, size_t(n) * 6 * sizeof(float)));
        const size_t ws = rtk::lbvh_workspace_bytes(n);
        HIP_OK(d.lbvh_ws.reserve(ws));
        if (device_build) HIP_OK(d.lcnt.reserve(size_t(2 * n - 1) * sizeof(uint32_t)));
        HIP_OK(rtk::lbvh_build_device(d.aabb.as<float>(), n, s->nodes.as<float>(), d.lbvh_ws.p, ws, nullptr,
                                      device_build ? d.lcnt.as<uint32_t>() : nullptr));
        if (!device_build) {  // the host builders read it
            host_nodes.resize(nbytes / sizeof(float));
            HIP_OK(hipMemcpy(host_nodes.data(), s->nodes.p, nbytes, hipMemcpyDeviceToHost));
            nodes = host_nodes.data();
        }
    } else {
        HIP_OK(s->nodes.store(nodes, nbytes));
    }
    lap(1);
    double w[2] = {0.0, 0.0};
    // (the leaf boxes: the caller's nodes', or with nodes = NULL the caller's boxes themselves)
    const bool wide = caller_nodes ? inw_wide_ok(s, geom, n, caller_nodes, 0) : inw_wide_ok(s, geom, n, aabbs, 6);
    if (device_build) {
        int rc = make_inw_wide_device(s, n, wide, w);
        d.wbuild = 1;
        if (rc == RT_E_UNSUPPORTED) {
            // the binned SAH tree ran past the device build's level cap (a chain-like scene: a split
            // can peel one object off per level); the host builders have no such limit, so read the
            // device LBVH back and build the walk structures there, as rt_dev_scene_inw does
            host_nodes.resize(nbytes / sizeof(float));
            HIP_OK(hipMemcpy(host_nodes.data(), s->nodes.p, nbytes, hipMemcpyDeviceToHost));
            rc = make_inw_wide(s, host_nodes.data(), n, wide, w, geom);
            d.wbuild = 2;
        }
        if (rc != RT_OK) return rc;
    } else {
        if (int rc = make_inw_wide(s, nodes, n, wide, w, geom); rc != RT_OK) return rc;
        d.wbuild = 0;
    }
    if (ms) { ms[2] = w[0]; ms[3] = w[1]; }
    s->n = n;
    s->n_lights = nl;
    s->tex_missing = false;  // (rt_dev_scene_inw_update refuses such records before it gets here)
    s->broken = false;
    return RT_OK;
}

// The library's choice for rt_dev_scene_inw_update_device's flags = 0, from the measured rows of DESIGN.md
// §5.15 (profiles/update_dev_c3.json): on the C3 scene the bin trees add 1.25 ms to the update (2.35
// against 1.10 ms) and take 1.74 ms off the frame that follows (146.30 against 148.04 ms), so update +
// frame is 148.63 [148.05, 148.86] ms with them and 149.12 [148.73, 149.82] ms without; neither median
// lies inside the other's spread.
constexpr int kInwUpdateDefault = RT_UPDATE_BINS;

// update_inw with nodes = NULL for records, boxes and lights that live on the scene's device
// (rt_dev_scene_inw_update_device): the records and the decisions by k_inw_prepare, the LBVH from the
// caller's boxes, the swept tree, the RI grid, the time-bin trees and the derived nodes, all on `st`;
// the decision words are read back after the swept build's own reads.  No geometry crosses to the host
// unless the host builders are needed (the level cap, inw_device_build = 0, one object): then the records
// and the device LBVH are copied back once and make_inw_wide builds as it does for update_inw.
// ms[4]: host time of the records and decisions, the LBVH, the swept tree + RI grid + derived nodes
// (or the host build), the time-bin trees.
int update_inw_device(rt_dev_scene *s, const float *d_geom, uint32_t n, const float *d_aabbs, const float *d_lights,
                      uint32_t n_lights, int flags, hipStream_t st, double *ms) {
    using clk = std::chrono::steady_clock;
    auto t = clk::now();
    auto lap = [&]() {
        const auto now = clk::now();
        const double v = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return v;
    };
    if (ms) ms[0] = ms[1] = ms[2] = ms[3] = 0.0;
    const bool want_bins = (flags ? flags : kInwUpdateDefault) == RT_UPDATE_BINS;
    s->broken = true;  // (as update_inw: the new sizes are committed at the end)
    s->sph_ok = false;
    InwWalk &d = s->walk;
    const uint32_t nl = s->layout == 4 ? n_lights : 0;
    HIP_OK(s->hot.reserve(size_t(n) * rtk::kInwHot * sizeof(float)));
    HIP_OK(s->cold.reserve(size_t(n) * rtk::kInwCold * sizeof(float)));
    HIP_OK(s->sph.reserve(size_t(n) * 12 * sizeof(float)));
    HIP_OK(d.dec.reserve(8 * sizeof(uint32_t)));
    HIP_OK(rtk::inw_prepare_device(d_geom, d_aabbs, n, s->layout, s->hot.as<float>(), s->cold.as<float>(),
                                   s->sph.as<float>(), d.dec.as<uint32_t>(), st));
    if (nl) {
        HIP_OK(s->lights.reserve(size_t(nl) * 7 * sizeof(float)));
        HIP_OK(hipMemcpyAsync(s->lights.p, d_lights, size_t(nl) * 7 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (ms) ms[0] = lap();
    const bool device_build = s->opt.inw_device_build && n >= 2;
    const size_t nbytes = size_t(2 * n - 1) * 8 * sizeof(float);
    HIP_OK(s->nodes.reserve(nbytes));
    const size_t ws = rtk::lbvh_workspace_bytes(n);
    HIP_OK(d.lbvh_ws.reserve(ws));
    if (device_build) HIP_OK(d.lcnt.reserve(size_t(2 * n - 1) * sizeof(uint32_t)));
    HIP_OK(rtk::lbvh_build_device(d_aabbs, n, s->nodes.as<float>(), d.lbvh_ws.p, ws, st,
                                  device_build ? d.lcnt.as<uint32_t>() : nullptr));
    if (ms) ms[1] = lap();
    d.reset();
    rtk::InwWideDev out{};
    bool host_build = !device_build;
    if (device_build) {
        const int rc = inw_swept_build_device(s, n, out, st);
        if (rc == RT_E_UNSUPPORTED) host_build = true;
        else if (rc != RT_OK) return rc;
    }
    uint32_t dec[8];
    HIP_OK(hipMemcpyAsync(dec, d.dec.p, sizeof(dec), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const rtk::InwDecisions dcs = rtk::inw_decisions(dec);
    const bool wide = s->opt.inw_wide_walk && n >= 2 && dcs.stick_out <= 1.0;  // inw_wide_ok
    const uint32_t K = s->opt.inw_time_bins > 1 ? uint32_t(s->opt.inw_time_bins) : 0u;
    double bins_ms = 0.0;
    if (!host_build) {
        if (wide) {
            if (int rc = inw_swept_commit_device(s, n, out, st); rc != RT_OK) return rc;
            if (want_bins && K >= 2 && K <= 16 && dcs.moving && dcs.bins_finite) {  // inw_wide_add_bins' conditions
                const auto tb = clk::now();
                const int rc = add_bins_device(s, d_geom, n, K, st);
                if (rc == RT_E_UNSUPPORTED) host_build = true;
                else if (rc != RT_OK) return rc;
                bins_ms = std::chrono::duration<double, std::milli>(clk::now() - tb).count();
            }
        }
        if (!host_build) {
            if (wide)
                if (int rc = make_qnodes(d, st); rc != RT_OK) return rc;
            d.dfs_high = out.dfs_high;
            d.sl_ok = true;  // the device LBVH has the stackless layout by construction (rt_lbvh.hip)
            d.wbuild = 1;
        }
    }
    if (host_build) {
        std::vector<float> geom(size_t(n) * 28), host_nodes(nbytes / sizeof(float));
        HIP_OK(hipMemcpyAsync(geom.data(), d_geom, geom.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(host_nodes.data(), s->nodes.p, nbytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        double w[2] = {0.0, 0.0};
        if (int rc = make_inw_wide(s, host_nodes.data(), n, wide, w, want_bins ? geom.data() : nullptr); rc != RT_OK)
            return rc;
        d.wbuild = device_build ? 2 : 0;
        bins_ms = 0.0;
    }
    HIP_OK(hipStreamSynchronize(st));  // every copy and kernel of this call: a render on any stream may follow
    if (ms) {
        ms[2] = lap() - bins_ms;
        ms[3] = bins_ms;
    }
    s->sph_ok = dcs.spheres;
    s->tex_missing = dcs.textured && s->n_tex == 0;  // renders and queries return RT_E_UNSUPPORTED
    s->n = n;
    s->n_lights = nl;
    s->broken = false;
    return RT_OK;
}
