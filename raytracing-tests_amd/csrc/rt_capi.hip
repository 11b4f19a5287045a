// rt_capi.hip -- the extern "C" surface of include/rt_hip.h and include/rt_scene.h: the options,
// argument checks and forwarding to the scene (rt_scene_build.hip) and launch units
// (rt_launch.hip, rt_launch_spec.hip).  The rt_debug_* entry points are rt_capi_debug.hip.  No
// exception crosses the ABI.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/rt_scene.h"
#include "rt_dev_scene.hpp"

namespace {

// rt_options (include/rt_hip.h): the library-wide options; scenes copy them at creation
rt_options default_options() {
    rt_options o;
    std::memset(&o, 0, sizeof(o));
    o.size = sizeof(rt_options);
    o.inw_wide_walk = 1; o.inw_order = 0; o.inw_beams = 1; o.inw_ri_grid = 1; o.inw_lds_nodes = 1;
    o.inw_fused_cull = 1; o.inw_claim_order = 1; o.inw_ring_pm = 0; o.inw_ring_sm = 0; o.inw_stackless = 1;
    o.inw_device_build = 1; o.inw_claim_xcd = 1; o.inw_qnodes = 0; o.inw_time_bins = 2;
    o.inw_walk_bins = 1; o.inw_beam_bins = 1; o.inw_sphere_records = 1; o.inw_compact_nodes = 1;
    o.iow_spec = 1; o.iow_linear = 0; o.iow_narrow = 0; o.iow_lds_bvh = 1;
    o.iow_leaf_batch = 32;  // 32 measured 2.5% faster on the bench frame than 65 (round 2)
    o.iow_coop_max = 4; o.iow_chunks_lpt = 0;
    o.rounds_seq = 6; o.rounds_spec = 1; o.park_min = -1;
    o.spec_iters = 1; o.spec_probe = 64; o.spec_heavy = -1; o.spec_rounds = 24; o.spec_tail_rounds = 60;
    o.spec_tail_budget = 3072; o.spec_scan = 128; o.spec_chain = 1; o.spec_alt = 1; o.spec_alt_cap = 1 << 17;
    o.spec_alt_seg = 0; o.spec_alt_every = 0; o.spec_spread = 1; o.spec_prior_from = 2; o.spec_sort = 1;
    o.spec_solo = 4096; o.spec_validate = 1; o.spec_max_gb = 96.0;
    o.inw_sky_blocks = 1;
    o.inw_beam_prune = 2;
    return o;
}
bool options_ok(const rt_options *o) {
    auto pow2 = [](int r) { return r >= 64 && r <= (1 << 16) && (r & (r - 1)) == 0; };
    return o && o->size == sizeof(rt_options) && o->inw_order >= -1 && o->inw_order <= 2 && (o->inw_ring_pm == 0 || pow2(o->inw_ring_pm)) &&
           (o->inw_ring_sm == 0 || pow2(o->inw_ring_sm)) && o->iow_leaf_batch >= 1 && o->iow_leaf_batch <= 65 && o->iow_coop_max >= 0 &&
           o->rounds_seq >= 0 && o->rounds_seq <= 14 && o->rounds_spec >= 0 && o->rounds_spec <= 14 &&
           o->park_min >= -1 && o->spec_iters >= 0 && o->spec_probe >= 1 && o->spec_heavy >= -1 &&
           o->spec_rounds >= 0 && o->spec_tail_rounds >= 0 && o->spec_tail_budget >= 1 && o->spec_scan >= 0 &&
           o->spec_alt_cap >= 1024 && o->spec_alt_cap <= (1 << 24) && o->spec_alt_seg >= 0 && o->spec_alt_every >= 0 &&
           o->spec_prior_from >= 1 && o->spec_solo >= 0 && o->spec_max_gb > 0.0 && o->inw_time_bins >= 0 &&
           o->inw_time_bins <= 16 && o->inw_beam_prune >= 0 && o->inw_beam_prune <= 2;
}

bool noise_args_ok(int width, int height, int type, const float *gradient, int n_grad, int octaves) {
    return width > 0 && height > 0 && size_t(width) * size_t(height) < (size_t(1) << 31) && type >= 0 && type <= 2 &&
           octaves >= 0 && n_grad >= 0 && n_grad <= 64 && (n_grad == 0 || gradient) &&
           rtk::noise_batches_exact(uint32_t(width));
}
bool remap_args_ok(int width, int height, int channels, int load_as, int map_to) {
    return width > 0 && height > 0 && size_t(width) * size_t(height) < (size_t(1) << 31) &&
           (channels == 3 || channels == 4) && load_as >= 0 && load_as <= 1 && map_to >= 0 && map_to <= 1 &&
           (load_as == map_to || rtk::noise_batches_exact(uint32_t(width)));
}

// a scene of this call alone, on the current device
std::unique_ptr<rt_dev_scene> temp_scene() {
    std::unique_ptr<rt_dev_scene> s(new (std::nothrow) rt_dev_scene());
    if (s) (void)hipGetDevice(&s->device);
    return s;
}

// The blocking scene renders: a temporary scene from make(scene), rendered into host buffers.
template <class Make>
int render_temp(const rt_camera *cam, const rt_params *p, float *rgba, float *depth, rt_stats *st, Make &&make) {
    int rc = check_device(p->device);
    if (rc != RT_OK) return rc;
    std::unique_ptr<rt_dev_scene> s = temp_scene();
    if (!s) return RT_E_ARG;
    if ((rc = make(s.get())) != RT_OK) return rc;
    return render_blocking(s.get(), cam, p, rgba, depth, st);
}

// The blocking ray and path queries: a temporary scene from make(scene), the rays up, trace(scene,
// rays, hits, counters) timed on the null stream, the hits and the counters back.  Ray / Hit: the
// query and answer records, whole float4s of one size (rt_ray / rt_hit, rt_path_ray / rt_path_out: 32
// bytes; rt_path_iow_ray / rt_path_iow_out: 48).
template <class Ray, class Hit, class Make, class Trace>
int trace_blocking(int flags, int allowed, const Ray *rays, uint32_t n_rays, Hit *hits, int device, rt_stats *st,
                   Make &&make, Trace &&trace) {
    static_assert(sizeof(Ray) == sizeof(Hit) && sizeof(Ray) % 16 == 0, "queries and answers are as many float4 each");
    if ((flags & ~allowed) || n_rays > (1u << 31)) return RT_E_ARG;
    if (n_rays > 0 && (!rays || !hits)) return RT_E_ARG;
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    std::unique_ptr<rt_dev_scene> s = temp_scene();
    if (!s) return RT_E_ARG;
    try {  // the host builders allocate: no exception crosses the ABI
        rc = make(s.get());
    } catch (...) {
        return RT_E_ARG;
    }
    if (rc != RT_OK) return rc;
    if (st) std::memset(st, 0, sizeof(*st));
    if (n_rays == 0) return RT_OK;
    DevBuf d_rays, d_hits, d_ctr;
    const size_t bytes = size_t(n_rays) * sizeof(Ray);
    HIP_OK(d_rays.alloc(bytes));
    HIP_OK(d_hits.alloc(bytes));
    HIP_OK(d_ctr.alloc(6 * sizeof(unsigned long long)));
    HIP_OK(hipMemcpy(d_rays.p, rays, bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_ctr.p, 0, 6 * sizeof(unsigned long long)));
    double ms = 0.0;
    rc = timed([&] { return trace(s.get(), d_rays.as<Ray>(), d_hits.as<Hit>(), d_ctr.as<uint64_t>()); }, &ms);
    if (rc != RT_OK) return rc;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(hits, d_hits.p, bytes, hipMemcpyDeviceToHost));
    return st ? read_stats(d_ctr.p, ms, st) : RT_OK;
}

// Pixel queries: the bytes of one path query / answer record of the scene's family, and the
// workspace of n_pixels pixels: their spp rays plus their spp answers.
size_t pixel_record_bytes(const rt_dev_scene *s) { return s->kind == 3 ? sizeof(rt_path_iow_ray) : sizeof(rt_path_ray); }
size_t pixel_ws_bytes(const rt_dev_scene *s, uint32_t n_pixels) {
    return size_t(n_pixels) * size_t(s->spp) * pixel_record_bytes(s) * 2;
}
bool pixels_args_ok(const rt_params *p, const rt_pixel *pixels, uint32_t n_pixels, const rt_pixel_out *pixels_out) {
    return uint64_t(n_pixels) * uint32_t(p->spp) <= (uint64_t(1) << 31) && (n_pixels == 0 || (pixels && pixels_out));
}

// The blocking pixel queries: a temporary scene from make(scene), the pixels up, rt_pixel_query_async
// timed on the null stream, the pixels (and, when asked for, the rays and the samples, both left in
// the workspace) and the counters back.
template <class Ray, class Out, class Make>
int pixels_blocking(const rt_camera *cam, const rt_params *p, const rt_pixel *pixels, uint32_t n_pixels, Ray *rays_out,
                    Out *samples_out, rt_pixel_out *pixels_out, int device, rt_stats *st, Make &&make) {
    static_assert(sizeof(Ray) == sizeof(Out), "queries and answers are as many float4 each");
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    std::unique_ptr<rt_dev_scene> s = temp_scene();
    if (!s) return RT_E_ARG;
    try {  // the host builders allocate: no exception crosses the ABI
        rc = make(s.get());
    } catch (...) {
        return RT_E_ARG;
    }
    if (rc != RT_OK) return rc;
    if (st) std::memset(st, 0, sizeof(*st));
    if (n_pixels == 0) return RT_OK;
    DevBuf d_px, d_out, d_ws, d_ctr;
    const size_t rec_bytes = size_t(n_pixels) * size_t(p->spp) * sizeof(Ray);
    HIP_OK(d_px.upload(pixels, size_t(n_pixels) * sizeof(rt_pixel)));
    HIP_OK(d_out.alloc(size_t(n_pixels) * sizeof(rt_pixel_out)));
    HIP_OK(d_ws.alloc(pixel_ws_bytes(s.get(), n_pixels)));
    HIP_OK(d_ctr.alloc(6 * sizeof(unsigned long long)));
    HIP_OK(hipMemset(d_ctr.p, 0, 6 * sizeof(unsigned long long)));
    double ms = 0.0;
    rc = timed([&] {
        return rt_pixel_query_async(s.get(), cam, p, d_px.as<rt_pixel>(), n_pixels, d_out.as<rt_pixel_out>(), nullptr,
                                    d_ws.p, d_ws.bytes, d_ctr.as<uint64_t>(), nullptr);
    }, &ms);
    if (rc != RT_OK) return rc;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(pixels_out, d_out.p, size_t(n_pixels) * sizeof(rt_pixel_out), hipMemcpyDeviceToHost));
    if (rays_out) HIP_OK(hipMemcpy(rays_out, d_ws.p, rec_bytes, hipMemcpyDeviceToHost));
    if (samples_out) HIP_OK(hipMemcpy(samples_out, d_ws.as<char>() + rec_bytes, rec_bytes, hipMemcpyDeviceToHost));
    return st ? read_stats(d_ctr.p, ms, st) : RT_OK;
}

// The scene view of the INW queries and passes: as in the renders, only layout-1 walks read the sphere records,
// and the fused cull needs the scene's culling boxes within 1000 of the origin (the kernels check each query's).
rtk::InwScene inw_query_view(const rt_dev_scene *s) {
    rtk::InwScene sc = inw_view(*s);
    if (s->layout == 4) sc.sph = nullptr;
    sc.fused = (s->opt.inw_fused_cull && sc.wnodes && s->walk.wbound <= 1000.0f) ? 1 : 0;
    return sc;
}

// The samples a pass's shader runs: IOW-03 stops at the ring schedule's early return (k_iow03's s_stop).
uint32_t pass_stop(const rt_dev_scene *s) { return uint32_t(s->kind == 3 ? s->s_stop : s->spp); }

// A pass's frame: make_frame's with the caller's outputs and counters.
rtk::Frame make_pass_frame(const rt_dev_scene *s, const rt_camera *cam, const rt_params *p, float *d_rgba,
                           float *d_depth, uint64_t *d_counters) {
    rtk::Frame f = make_frame(cam, p);
    f.out_rgba = d_rgba; f.out_depth = d_depth;
    f.counters = reinterpret_cast<unsigned long long *>(d_counters);
    f.dbg = nullptr; f.px_rays = nullptr;  // the renders' diagnostics hooks do not apply
    f.leaf_batch = s->opt.iow_leaf_batch;
    return f;
}

// rt_debug_pass_max_blocks caps the paths' grid while one of these lives; the paths' own cap is back after it.
struct PassBlockCap {
    const int prev = rtk::inw_paths_max_blocks(rtk::pass_max_blocks_now());
    ~PassBlockCap() { (void)rtk::inw_paths_max_blocks(prev); }
};

// The INW half of a pass, `total` samples of each of n pixels (units or list entries): per chunk [c0, c0 + nsc)
// of them, the camera rays into the scene's pass workspace (rays_of), the path queries on them
// (rt_path_rays_async's launch: its scene view, its queue word, its fused-cull rule) and the fold (fold_of).
// A chunk is as many samples as keep the rays and answers (64 B a sample and pixel) within kPassRecords records,
// chunk_cap > 0 at most; the first pass of a frame size and chunk grows the workspace, later ones allocate none.
template <class Rays, class Fold>
int pass_inw_chunks(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, uint32_t n, uint32_t total,
                    int chunk_cap, uint64_t *d_counters, hipStream_t st, Rays &&rays_of, Fold &&fold_of) {
    constexpr uint64_t kPassRecords = uint64_t(1) << 25;
    uint32_t chunk = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(total, kPassRecords / n)));
    if (chunk_cap > 0) chunk = std::min(chunk, uint32_t(chunk_cap));
    HIP_OK(s->pass_ws.reserve(size_t(n) * chunk * 2 * sizeof(rt_path_ray)));
    float4 *rays = s->pass_ws.as<float4>(), *out = rays + size_t(n) * chunk * 2;
    const rtk::InwScene sc = inw_query_view(s);
    // the frame's child order: dot(dir, (1, 1, 1)) > 0 in binary32, the shader's order (inw_segment)
    const float dsum = (cam->dir[0] * 1.0f + cam->dir[1] * 1.0f) + cam->dir[2] * 1.0f;
    unsigned *queue = s->counter.as<unsigned>() + 224;
    const PassBlockCap cap;
    hipError_t e = hipSuccess;
    for (uint32_t c0 = 0; c0 < total && e == hipSuccess; c0 += chunk) {
        const uint32_t nsc = std::min(chunk, total - c0);
        e = rays_of(sc, c0, nsc, rays);
        if (e == hipSuccess)
            e = rtk::launch_inw_paths(sc, rays, n * nsc, s->spp, p->max_bounces, dsum > 0.0f, out,
                                      reinterpret_cast<unsigned long long *>(d_counters), queue, s->cus, st);
        if (e == hipSuccess) e = fold_of(c0, nsc, c0 + nsc == total, out);
    }
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

// Progressive passes: cuts is strictly increasing from cuts[0] > 0 to at most spp.
bool cuts_ok(const rt_params *p, const uint32_t *cuts, int n_cuts) {
    if (!cuts || n_cuts < 1 || cuts[0] == 0 || cuts[n_cuts - 1] > uint32_t(p->spp)) return false;
    for (int i = 1; i < n_cuts; i++)
        if (cuts[i] <= cuts[i - 1]) return false;
    return true;
}

// A packed tile list of the adaptive calls: rt_render_pass_tiles_async's rule, at most 2^31 slots.
bool tile_list_ok(const int *d_tiles, int n_tiles, int tile_size) {
    if (!d_tiles || n_tiles <= 0 || tile_size <= 0 || tile_size % 16 != 0) return false;
    return uint64_t(n_tiles) * uint64_t(tile_size) * uint64_t(tile_size) <= (uint64_t(1) << 31);
}

// The blocking passes: a temporary scene from make(scene), the host buffers up (pixels outside the
// rectangle keep their bytes), pass i = samples [cuts[i - 1], cuts[i]) into image i, timed together
// on the null stream, the images, the last state and the counters back.
template <class Make>
int passes_blocking(const rt_camera *cam, const rt_params *p, const uint32_t *cuts, int n_cuts, float *rgba,
                    float *depth, rt_pass_state *state_out, int device, rt_stats *st, Make &&make) {
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    std::unique_ptr<rt_dev_scene> s = temp_scene();
    if (!s) return RT_E_ARG;
    try {  // the host builders allocate: no exception crosses the ABI
        rc = make(s.get());
    } catch (...) {
        return RT_E_ARG;
    }
    if (rc != RT_OK) return rc;
    if (st) std::memset(st, 0, sizeof(*st));
    const size_t npx = size_t(p->width) * size_t(p->height);
    DevBuf d_state, d_rgba, d_depth, d_ctr;
    if (state_out) HIP_OK(d_state.upload(state_out, npx * sizeof(rt_pass_state)));
    else HIP_OK(d_state.alloc(npx * sizeof(rt_pass_state)));
    HIP_OK(d_rgba.upload(rgba, size_t(n_cuts) * npx * 16));
    if (depth) HIP_OK(d_depth.upload(depth, size_t(n_cuts) * npx * 4));
    HIP_OK(d_ctr.alloc(6 * sizeof(unsigned long long)));
    HIP_OK(hipMemset(d_ctr.p, 0, 6 * sizeof(unsigned long long)));
    double ms = 0.0;
    rc = timed([&] {
        uint32_t s0 = 0;
        for (int i = 0; i < n_cuts; i++) {
            const int r = rt_render_pass_async(s.get(), cam, p, s0, cuts[i] - s0, d_state.as<rt_pass_state>(),
                                               d_rgba.as<float>() + size_t(i) * npx * 4,
                                               depth ? d_depth.as<float>() + size_t(i) * npx : nullptr,
                                               d_ctr.as<uint64_t>(), nullptr);
            if (r != RT_OK) return r;
            s0 = cuts[i];
        }
        return int(RT_OK);
    }, &ms);
    if (rc != RT_OK) return rc;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(rgba, d_rgba.p, size_t(n_cuts) * npx * 16, hipMemcpyDeviceToHost));
    if (depth) HIP_OK(hipMemcpy(depth, d_depth.p, size_t(n_cuts) * npx * 4, hipMemcpyDeviceToHost));
    if (state_out) HIP_OK(hipMemcpy(state_out, d_state.p, npx * sizeof(rt_pass_state), hipMemcpyDeviceToHost));
    return st ? read_stats(d_ctr.p, ms, st) : RT_OK;
}

// The blocking adaptive passes: a temporary scene from make(scene), the host buffers up (pixels outside the
// rectangle keep their bytes), the aux buffer zeroed and every pixel of the rectangle listed (a select that
// finds every pixel active), then rounds of one listed pass of `batch` samples and one select, with the
// active count read back, while pixels are active and rounds remain (max_rounds == 0: no limit).  The
// rounds are timed on the null stream and summed.
template <class Make>
int adaptive_blocking(const rt_camera *cam, const rt_params *p, uint32_t batch, float tol, uint32_t min_samples,
                      uint32_t max_rounds, float *rgba, float *depth, uint32_t *count, float *err,
                      rt_pass_state *state_out, rt_pass_aux *aux_out, uint32_t *rounds_out, int device, rt_stats *st,
                      Make &&make) {
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    std::unique_ptr<rt_dev_scene> s = temp_scene();
    if (!s) return RT_E_ARG;
    try {  // the host builders allocate: no exception crosses the ABI
        rc = make(s.get());
    } catch (...) {
        return RT_E_ARG;
    }
    if (rc != RT_OK) return rc;
    if (st) std::memset(st, 0, sizeof(*st));
    if (rounds_out) *rounds_out = 0;
    const size_t npx = size_t(p->width) * size_t(p->height);
    const rtk::Frame f = make_frame(cam, p);
    const size_t cap = size_t(f.tw > 0 ? f.tw : 0) * size_t(f.th > 0 ? f.th : 0);  // the list's capacity
    DevBuf d_state, d_aux, d_rgba, d_depth, d_err, d_list, d_n, d_ctr;
    if (state_out) HIP_OK(d_state.upload(state_out, npx * sizeof(rt_pass_state)));
    else HIP_OK(d_state.alloc(npx * sizeof(rt_pass_state)));
    HIP_OK(d_aux.alloc(npx * sizeof(rt_pass_aux)));
    HIP_OK(hipMemset(d_aux.p, 0, npx * sizeof(rt_pass_aux)));
    HIP_OK(d_rgba.upload(rgba, npx * 16));
    if (depth) HIP_OK(d_depth.upload(depth, npx * 4));
    if (err) HIP_OK(d_err.upload(err, npx * 4));
    HIP_OK(d_list.alloc(cap * sizeof(rt_pixel)));
    HIP_OK(d_n.alloc(sizeof(uint32_t)));
    HIP_OK(d_ctr.alloc(6 * sizeof(unsigned long long)));
    HIP_OK(hipMemset(d_ctr.p, 0, 6 * sizeof(unsigned long long)));
    auto select = [&](float t, uint32_t m, float *e, uint32_t *n_active) -> int {
        const int r = rt_pass_select_async(s.get(), p, d_state.as<rt_pass_state>(), d_aux.as<rt_pass_aux>(), t, m,
                                           d_list.as<rt_pixel>(), d_n.as<uint32_t>(), e, nullptr);
        if (r != RT_OK) return r;
        HIP_OK(hipMemcpy(n_active, d_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        return int(RT_OK);
    };
    uint32_t n_active = 0, rounds = 0;
    if ((rc = select(-1.0f, 0, nullptr, &n_active)) != RT_OK) return rc;  // every pixel has 0 samples: all active
    double total_ms = 0.0;
    while (n_active > 0 && (max_rounds == 0 || rounds < max_rounds)) {
        double ms = 0.0;
        rc = timed([&]() -> int {
            const int r = rt_render_pass_pixels_async(s.get(), cam, p, d_list.as<rt_pixel>(), n_active, batch,
                                                      d_state.as<rt_pass_state>(), d_aux.as<rt_pass_aux>(),
                                                      d_rgba.as<float>(), depth ? d_depth.as<float>() : nullptr,
                                                      d_ctr.as<uint64_t>(), nullptr);
            return r != RT_OK ? r : select(tol, min_samples, err ? d_err.as<float>() : nullptr, &n_active);
        }, &ms);
        if (rc != RT_OK) return rc;
        total_ms += ms;
        rounds++;
    }
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(rgba, d_rgba.p, npx * 16, hipMemcpyDeviceToHost));
    if (depth) HIP_OK(hipMemcpy(depth, d_depth.p, npx * 4, hipMemcpyDeviceToHost));
    if (err) HIP_OK(hipMemcpy(err, d_err.p, npx * 4, hipMemcpyDeviceToHost));
    if (state_out) HIP_OK(hipMemcpy(state_out, d_state.p, npx * sizeof(rt_pass_state), hipMemcpyDeviceToHost));
    if (count || aux_out) {  // the rectangle's pixels of the aux buffer (the others were never the frame's)
        std::vector<rt_pass_aux> aux(npx);
        HIP_OK(hipMemcpy(aux.data(), d_aux.p, npx * sizeof(rt_pass_aux), hipMemcpyDeviceToHost));
        for (int y = std::max(f.y0, 0); y < std::min(f.y0 + f.th, f.H); y++)
            for (int x = std::max(f.x0, 0); x < std::min(f.x0 + f.tw, f.W); x++) {
                const size_t i = size_t(y) * size_t(f.W) + size_t(x);
                if (count) count[i] = aux[i].count;
                if (aux_out) aux_out[i] = aux[i];
            }
    }
    if (rounds_out) *rounds_out = rounds;
    return st ? read_stats(d_ctr.p, total_ms, st) : RT_OK;
}

}  // namespace

rt_options g_opt = default_options();

int rtamd::scene_device(const rt_dev_scene *s) { return s ? s->device : -1; }

int rtamd::scene_pass_check(const rt_dev_scene *s, int spp) {
    if (!s || s->spp != spp || s->broken) return RT_E_ARG;
    return s->tex_missing ? RT_E_UNSUPPORTED : RT_OK;
}

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

// rt_hip_debug.h: the fused-cull decision of the query and pass launches (inw_query_view's)
int rt_debug_query_fused(rt_dev_scene *s) {
    if (!s || s->kind == 3) return RT_E_ARG;
    return inw_query_view(s).fused;
}

void rt_options_default(rt_options *o) {
    if (o) *o = default_options();
}

int rt_options_set(const rt_options *o) {
    if (!options_ok(o)) return RT_E_ARG;
    g_opt = *o;
    return RT_OK;
}

int rt_options_get(rt_options *o) {
    if (!o) return RT_E_ARG;
    *o = g_opt;
    return RT_OK;
}

int rt_dev_scene_inw_update(rt_dev_scene *s, const float *geom, uint32_t n, const float *nodes, const float *aabbs,
                            const float *lights, uint32_t n_lights, double timing_ms[4]) {
    if (!s || s->kind == 3 || !geom || n == 0 || (!nodes && !aabbs)) return RT_E_ARG;
    if (s->layout == 4 && n_lights > 0 && !lights) return RT_E_ARG;
    if (s->n_tex == 0 && inw_textured(geom, n, s->layout)) return RT_E_UNSUPPORTED;
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipDeviceSynchronize());  // the scene's last frame may still read the buffers being replaced
    try {  // the host builders allocate: no exception crosses the ABI
        return update_inw(s, geom, n, nodes, aabbs, lights, n_lights, timing_ms);
    } catch (...) {
        s->broken = true;
        return RT_E_ARG;
    }
}

int rt_dev_scene_inw_update_device(rt_dev_scene *s, const float *d_geom, uint32_t n, const float *d_aabbs,
                                   const float *d_lights, uint32_t n_lights, int flags, void *stream, double timing_ms[4]) {
    // argument errors come back before a device is touched, the scene untouched and still valid
    if (!s || !d_geom || !d_aabbs || n == 0) return RT_E_ARG;
    if ((flags & ~(RT_UPDATE_BINS | RT_UPDATE_NO_BINS)) || flags == (RT_UPDATE_BINS | RT_UPDATE_NO_BINS)) return RT_E_ARG;
    if (s->kind != 3 && s->layout == 4 && n_lights > 0 && !d_lights) return RT_E_ARG;
    if (s->kind == 3 || n > (1u << 24)) return RT_E_UNSUPPORTED;  // (node / object ids are stored as floats, exact to 2^24)
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipDeviceSynchronize());  // the scene's last frame may still read the buffers being replaced
    try {  // the host builders of the fallback allocate: no exception crosses the ABI
        return update_inw_device(s, d_geom, n, d_aabbs, d_lights, n_lights, flags, static_cast<hipStream_t>(stream),
                                 timing_ms);
    } catch (...) {
        s->broken = true;
        return RT_E_ARG;
    }
}

int rt_inw_swept_boxes_async(const float *d_geom, uint32_t n, float *d_aabbs_out, void *stream) {
    if (!d_geom || !d_aabbs_out) return RT_E_ARG;
    if (n == 0) return RT_OK;
    const hipError_t e = rtk::inw_swept_boxes_device(d_geom, n, d_aabbs_out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

int rt_dev_scene_iow03_update(rt_dev_scene *s, const float *types, const float *records, uint32_t n, int flags,
                              double timing_ms[4]) {
    // argument errors come back before a device is touched, the scene untouched and still valid
    if (!s || !types || !records || n == 0) return RT_E_ARG;
    if ((flags & ~(RT_UPDATE_HOST_BUILD | RT_UPDATE_DEVICE_BUILD)) || flags == (RT_UPDATE_HOST_BUILD | RT_UPDATE_DEVICE_BUILD))
        return RT_E_ARG;
    if (s->kind != 3) return RT_E_UNSUPPORTED;
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipDeviceSynchronize());  // the scene's last frame may still read the buffers being replaced
    try {  // the host builders allocate: no exception crosses the ABI
        return update_iow03(s, types, records, n, flags, timing_ms);
    } catch (...) {
        s->broken = true;
        return RT_E_ARG;
    }
}

int rt_dev_scene_iow03_update_device(rt_dev_scene *s, const float *d_types, const float *d_records, uint32_t n, int flags,
                                     void *stream, double timing_ms[4]) {
    // argument errors come back before a device is touched, the scene untouched and still valid
    if (!s || !d_types || !d_records || n == 0) return RT_E_ARG;
    if ((flags & ~(RT_UPDATE_HOST_BUILD | RT_UPDATE_DEVICE_BUILD)) || flags == (RT_UPDATE_HOST_BUILD | RT_UPDATE_DEVICE_BUILD))
        return RT_E_ARG;
    if (s->kind != 3) return RT_E_UNSUPPORTED;
    if (n > 0x7fffffffu) return RT_E_ARG;  // (the sort counts in an int)
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipDeviceSynchronize());  // the scene's last frame may still read the buffers being replaced
    try {  // the host builder of the fallback allocates: no exception crosses the ABI
        return update_iow03_device(s, d_types, d_records, n, flags, static_cast<hipStream_t>(stream), timing_ms);
    } catch (...) {
        s->broken = true;
        return RT_E_ARG;
    }
}

int rt_dev_scene_set_options(rt_dev_scene *s, const rt_options *o) {
    if (!s || !options_ok(o)) return RT_E_ARG;
    const int wide = s->opt.inw_wide_walk, linear = s->opt.iow_linear;  // [build] options stay
    s->opt = *o;
    s->opt.inw_wide_walk = wide;
    s->opt.iow_linear = linear;
    return RT_OK;
}

int rt_device_info(int device, char *name_out, int name_cap, int *cu_count) {
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    int cur = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&cur) != hipSuccess || hipGetDeviceProperties(&prop, cur) != hipSuccess) return RT_E_HIP;
    if (name_out && name_cap > 0) std::snprintf(name_out, size_t(name_cap), "%s (%s)", prop.name, prop.gcnArchName);
    if (cu_count) *cu_count = prop.multiProcessorCount;
    return RT_OK;
}

int rt_render_iow01(const rt_camera *cam, const float sphere[4], const rt_params *p, float *rgba, rt_stats *st) {
    if (!cam || !sphere || !params_ok(p) || !rgba) return RT_E_ARG;
    int rc = check_device(p->device);
    if (rc != RT_OK) return rc;
    rtk::Frame f = make_frame(cam, p);
    std::memcpy(f.sphere, sphere, sizeof(f.sphere));
    const size_t npx = size_t(p->width) * p->height;
    DevBuf d_rgba;
    HIP_OK(d_rgba.alloc(npx * 16));
    HIP_OK(hipMemcpy(d_rgba.p, rgba, npx * 16, hipMemcpyHostToDevice));
    f.out_rgba = d_rgba.as<float>();
    double ms = 0.0;
    rc = timed([&] { HIP_OK(rtk::launch_iow01(f, nullptr)); return RT_OK; }, &ms);
    if (rc != RT_OK) return rc;
    HIP_OK(hipMemcpy(rgba, d_rgba.p, npx * 16, hipMemcpyDeviceToHost));
    if (st) {
        std::memset(st, 0, sizeof(*st));
        st->segments = uint64_t(f.tw) * uint64_t(f.th);
        st->ms = ms;
    }
    return RT_OK;
}

int rt_render_iow03(const float *types, const float *records, uint32_t n, const rt_camera *cam,
                    const rt_params *p, float *rgba, rt_stats *st) {
    if (!types || !records || !cam || !params_ok(p) || !rgba) return RT_E_ARG;
    return render_temp(cam, p, rgba, nullptr, st,
                       [&](rt_dev_scene *s) { return make_iow03(s, types, records, n, p->spp); });
}

int rt_render_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                  uint32_t n_lights, const rt_camera *cam, const rt_params *p, float *rgba, float *depth,
                  rt_stats *st) {
    return rt_render_inw_tex(geom, n, layout, nodes, lights, n_lights, nullptr, 0, cam, p, rgba, depth, st);
}

int rt_render_inw_tex(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                      uint32_t n_lights, const rt_texture *tex, int n_tex, const rt_camera *cam, const rt_params *p,
                      float *rgba, float *depth, rt_stats *st) {
    if (!geom || !nodes || n == 0 || !cam || !params_ok(p) || !rgba) return RT_E_ARG;
    if (layout != 1 && layout != 4) return RT_E_ARG;
    if (layout == 4 && n_lights > 0 && !lights) return RT_E_ARG;
    if (!textures_ok(tex, n_tex)) return RT_E_ARG;
    if (n_tex == 0 && inw_textured(geom, n, layout)) return RT_E_UNSUPPORTED;  // no texture bound
    return render_temp(cam, p, rgba, depth, st, [&](rt_dev_scene *s) {
        return make_inw(s, geom, n, layout, nodes, lights, n_lights, tex, n_tex, p->spp);
    });
}

int rt_inw_host_build(const float *nodes, uint32_t n, uint32_t info[8], double *ms) {
    if (!nodes || n == 0) return RT_E_ARG;
    try {
        const auto t0 = std::chrono::steady_clock::now();
        rtamd::InwWide w;
        rtamd::RiGrid g;
        const bool ok = rtamd::inw_wide_build(nodes, n, w);
        if (ok) g = rtamd::ri_grid_build(w.leafbox.data(), n);
        const auto t1 = std::chrono::steady_clock::now();
        if (ms) *ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        if (info) {
            const uint32_t v[8] = {uint32_t(w.wnodes.size() / 40), w.dfs_high, uint32_t(w.depth), g.ok ? 1u : 0u,
                                   g.ok ? uint32_t(g.cells.size() - 1) : 0u, uint32_t(g.ids.size()), 0u, 0u};
            std::memcpy(info, v, sizeof(v));
        }
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

int rt_iow_host_build(const float *types, const float *records, uint32_t n, uint32_t info[4], double *ms) {
    if (!types || !records || n == 0) return RT_E_ARG;
    try {
        const auto t0 = std::chrono::steady_clock::now();
        rtamd::IowCull c;
        const bool ok = rtamd::iow_cull_build(types, records, n, c);
        const auto t1 = std::chrono::steady_clock::now();
        if (ms) *ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        if (info) {
            const uint32_t v[4] = {ok ? c.n_wide : 0u, 0u, 0u, 0u};
            std::memcpy(info, v, sizeof(v));
        }
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

int rt_lbvh_build(const float *aabbs, uint32_t n, float *nodes_out) {
    if (!aabbs || !nodes_out || n == 0) return RT_E_ARG;
    try {
        std::vector<float> v = rtamd::lbvh_build(aabbs, n);
        std::memcpy(nodes_out, v.data(), v.size() * sizeof(float));
    } catch (...) {
        return RT_E_ARG;
    }
    return RT_OK;
}

size_t rt_lbvh_workspace_bytes(uint32_t n) { return rtk::lbvh_workspace_bytes(n); }

int rt_lbvh_build_async(const float *d_aabbs, uint32_t n, float *d_nodes_out, void *d_ws, size_t ws_bytes,
                        void *stream) {
    if (!d_aabbs || !d_nodes_out || n == 0 || (n > 1 && (!d_ws || ws_bytes < rtk::lbvh_workspace_bytes(n))))
        return RT_E_ARG;
    if (n > (1u << 24)) return RT_E_UNSUPPORTED;  // node / object ids are stored as floats (exact to 2^24)
    const hipError_t e = rtk::lbvh_build_device(d_aabbs, n, d_nodes_out, d_ws, ws_bytes, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : hip_failed("lbvh build failed", e);
}

int rt_lbvh_build_gpu(const float *aabbs, uint32_t n, float *nodes_out, int device, double *ms) {
    if (!aabbs || !nodes_out || n == 0) return RT_E_ARG;
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    const size_t total = 2 * size_t(n) - 1;
    DevBuf d_in, d_out, d_ws;
    HIP_OK(d_in.upload(aabbs, size_t(n) * 6 * sizeof(float)));
    HIP_OK(d_out.alloc(total * 8 * sizeof(float)));
    HIP_OK(d_ws.alloc(rtk::lbvh_workspace_bytes(n)));
    rc = timed([&] { return rt_lbvh_build_async(d_in.as<float>(), n, d_out.as<float>(), d_ws.p, d_ws.bytes, nullptr); },
               ms);
    if (rc != RT_OK) return rc;
    HIP_OK(hipMemcpy(nodes_out, d_out.p, total * 8 * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

size_t rt_noise_workspace_bytes(int width, int height) {
    return width > 0 && height > 0 ? rtk::noise_workspace_bytes(width, height) : 0;
}

int rt_noise_texture_async(int width, int height, int type, const float *gradient, int n_grad, float freq,
                           float lac, float gain, int octaves, uint8_t *d_rgb_out, void *d_ws, size_t ws_bytes,
                           void *stream) {
    if (!noise_args_ok(width, height, type, gradient, n_grad, octaves) || !d_rgb_out || !d_ws ||
        ws_bytes < rtk::noise_workspace_bytes(width, height))
        return RT_E_ARG;
    const hipError_t e = rtk::noise_texture(width, height, type, gradient, n_grad, freq, lac, gain, octaves, d_rgb_out,
                                            d_ws, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : hip_failed("noise texture failed", e);
}

int rt_noise_texture(int width, int height, int type, const float *gradient, int n_grad, float freq, float lac,
                     float gain, int octaves, uint8_t *rgb_out, int device, double *ms) {
    if (!noise_args_ok(width, height, type, gradient, n_grad, octaves) || !rgb_out) return RT_E_ARG;
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    const size_t bytes = size_t(width) * size_t(height) * 3;
    DevBuf d_out, d_ws;
    HIP_OK(d_out.alloc(bytes));
    HIP_OK(d_ws.alloc(rtk::noise_workspace_bytes(width, height)));
    rc = timed([&] {
        return rt_noise_texture_async(width, height, type, gradient, n_grad, freq, lac, gain, octaves,
                                      d_out.as<uint8_t>(), d_ws.p, d_ws.bytes, nullptr);
    }, ms);
    if (rc != RT_OK) return rc;
    uint32_t status = 0;
    HIP_OK(hipMemcpy(&status, d_ws.as<uint32_t>() + 2, sizeof(status), hipMemcpyDeviceToHost));
    if (status) return RT_E_ARG;  // degenerate value range (the reference divides by zero)
    HIP_OK(hipMemcpy(rgb_out, d_out.p, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

size_t rt_remap_workspace_bytes(int width, int height) {
    return width > 0 && height > 0 ? rtk::remap_workspace_bytes(width, height) : 0;
}

int rt_texture_remap_async(const uint8_t *d_in, int width, int height, int channels, int load_as, int map_to,
                           uint8_t *d_out, void *d_ws, size_t ws_bytes, void *stream) {
    if (!remap_args_ok(width, height, channels, load_as, map_to) || !d_in || !d_out) return RT_E_ARG;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (load_as == map_to) {
        e = hipMemcpyAsync(d_out, d_in, size_t(width) * height * channels, hipMemcpyDeviceToDevice, st);
    } else {
        if (!d_ws || ws_bytes < rtk::remap_workspace_bytes(width, height)) return RT_E_ARG;
        e = rtk::texture_remap(d_in, width, height, channels, load_as, d_out, d_ws, st);
    }
    return e == hipSuccess ? RT_OK : hip_failed("texture remap failed", e);
}

int rt_texture_remap(const uint8_t *in, int width, int height, int channels, int load_as, int map_to, uint8_t *out,
                     int device, double *ms) {
    if (!remap_args_ok(width, height, channels, load_as, map_to) || !in || !out) return RT_E_ARG;
    int rc = check_device(device);
    if (rc != RT_OK) return rc;
    const size_t bytes = size_t(width) * size_t(height) * channels;
    DevBuf d_in, d_out, d_ws;
    HIP_OK(d_in.upload(in, bytes));
    HIP_OK(d_out.alloc(bytes));
    HIP_OK(d_ws.alloc(rtk::remap_workspace_bytes(width, height)));
    rc = timed([&] {
        return rt_texture_remap_async(d_in.as<uint8_t>(), width, height, channels, load_as, map_to,
                                      d_out.as<uint8_t>(), d_ws.p, d_ws.bytes, nullptr);
    }, ms);
    if (rc != RT_OK) return rc;
    HIP_OK(hipMemcpy(out, d_out.p, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_tile_spiral(int width, int height, int tile_w, int tile_h, int *out, int cap) {
    if (width <= 0 || height <= 0 || tile_w <= 0 || tile_h <= 0 || cap < 0 || (cap > 0 && !out)) return RT_E_ARG;
    if (width / tile_w > 32766 || height / tile_h > 32766) return RT_E_ARG;  // int16 tile indices
    const std::vector<rtamd::SpiralTile> t = rtamd::tile_spiral(width, height, tile_w, tile_h);
    for (size_t i = 0; i < t.size() && int(i) < cap; i++) {
        out[4 * i] = t[i].tx; out[4 * i + 1] = t[i].ty; out[4 * i + 2] = t[i].w; out[4 * i + 3] = t[i].h;
    }
    return int(t.size());
}

int rt_render_spiral_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, int tile_w, int tile_h,
                           int first, int count, float *d_rgba, float *d_depth, uint64_t *d_counters,
                           void *stream) {
    if (!s || !cam || !params_ok(p) || !d_rgba || tile_w <= 0 || tile_h <= 0 || first < 0 || count < 0)
        return RT_E_ARG;
    if (p->width / tile_w > 32766 || p->height / tile_h > 32766) return RT_E_ARG;
    const std::vector<rtamd::SpiralTile> t = rtamd::tile_spiral(p->width, p->height, tile_w, tile_h);
    int i = std::min(first, int(t.size()));
    const int end = int(std::min<size_t>(t.size(), size_t(i) + size_t(count)));
    for (; i < end; i++) {
        if (t[size_t(i)].w <= 0 || t[size_t(i)].h <= 0) continue;  // a zero-size dispatch draws nothing
        rt_params q = *p;
        q.tile_x0 = t[size_t(i)].tx * tile_w;
        q.tile_y0 = t[size_t(i)].ty * tile_h;
        q.tile_w = t[size_t(i)].w;
        q.tile_h = t[size_t(i)].h;
        const int rc = rt_render_image_async(s, cam, &q, d_rgba, d_depth, d_counters, stream);
        if (rc != RT_OK) return rc;
    }
    return end;
}

int rt_display_rgba8_async(const float *d_rgba, const float *d_depth, int width, int height, int use_depth,
                           uint8_t *d_out, void *stream) {
    if (width <= 0 || height <= 0 || !d_out || (use_depth ? !d_depth : !d_rgba)) return RT_E_ARG;
    const hipError_t e = rtk::display_rgba8(d_rgba, d_depth, uint32_t(size_t(width) * size_t(height)), use_depth,
                                            d_out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : hip_failed("display pass failed", e);
}

rt_dev_scene *rt_dev_scene_iow03(const float *types, const float *records, uint32_t n, int spp, int device) {
    if (!types || !records || spp < 1) return nullptr;
    if (check_device(device) != RT_OK) return nullptr;
    std::unique_ptr<rt_dev_scene> s = temp_scene();
    if (!s || make_iow03(s.get(), types, records, n, spp) != RT_OK) return nullptr;
    return s.release();
}

rt_dev_scene *rt_dev_scene_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                               uint32_t n_lights, int spp, int device) {
    return rt_dev_scene_inw_tex(geom, n, layout, nodes, lights, n_lights, nullptr, 0, spp, device);
}

rt_dev_scene *rt_dev_scene_inw_tex(const float *geom, uint32_t n, int layout, const float *nodes,
                                   const float *lights, uint32_t n_lights, const rt_texture *tex, int n_tex,
                                   int spp, int device) {
    if (!geom || !nodes || n == 0 || spp < 1 || (layout != 1 && layout != 4)) return nullptr;
    if (layout == 4 && n_lights > 0 && !lights) return nullptr;
    if (!textures_ok(tex, n_tex)) return nullptr;
    if (n_tex == 0 && inw_textured(geom, n, layout)) return nullptr;
    if (check_device(device) != RT_OK) return nullptr;
    std::unique_ptr<rt_dev_scene> s = temp_scene();
    if (!s || make_inw(s.get(), geom, n, layout, nodes, lights, n_lights, tex, n_tex, spp) != RT_OK) return nullptr;
    return s.release();
}

void rt_dev_scene_free(rt_dev_scene *s) {
    if (!s) return;
    (void)hipDeviceSynchronize();  // the scene's last frame may still run
    delete s;
}

int rt_render_tiles_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, const int *d_tiles,
                          int n_tiles, int tile_size, float *d_out_packed, float *d_out_depth_packed,
                          uint64_t *d_counters, void *stream) {
    if (!s || !cam || !params_ok(p) || !d_tiles || n_tiles <= 0 || !d_out_packed) return RT_E_ARG;
    if (tile_size <= 0 || tile_size % 16 != 0) return RT_E_ARG;
    if (p->spp != s->spp) return RT_E_ARG;  // tables are built for the scene's spp
    rtk::Frame f = make_frame(cam, p);
    f.tiles = d_tiles; f.n_tiles = n_tiles; f.tile_size = tile_size;
    f.out_rgba = d_out_packed; f.out_depth = d_out_depth_packed;
    f.counters = reinterpret_cast<unsigned long long *>(d_counters);
    return launch_scene(s, f, static_cast<hipStream_t>(stream));
}

int rt_render_image_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, float *d_rgba, float *d_depth,
                          uint64_t *d_counters, void *stream) {
    if (!s || !cam || !params_ok(p) || !d_rgba) return RT_E_ARG;
    if (p->spp != s->spp) return RT_E_ARG;
    rtk::Frame f = make_frame(cam, p);
    f.out_rgba = d_rgba; f.out_depth = d_depth;
    f.counters = reinterpret_cast<unsigned long long *>(d_counters);
    return launch_scene(s, f, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------ ray queries
int rt_trace_rays_async(rt_dev_scene *s, const rt_ray *d_rays, uint32_t n_rays, int flags, rt_hit *d_hits,
                        uint64_t *d_counters, void *stream) {
    static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 32, "rt_ray / rt_hit are 2 float4 each");
    if (!s || (flags & ~(RT_TRACE_INVERT | RT_TRACE_ANY))) return RT_E_ARG;
    if (s->kind == 3) return RT_E_UNSUPPORTED;
    if (s->broken || n_rays > (1u << 31)) return RT_E_ARG;
    if (n_rays == 0) return RT_OK;
    if (!d_rays || !d_hits) return RT_E_ARG;
    const rtk::InwScene sc = inw_query_view(s);
    // its own queue counter, past the fold kernels' (two queues 64 B apart and 8 XCD queues from byte 256)
    unsigned *queue = s->counter.as<unsigned>() + 240;
    const hipError_t e = rtk::launch_inw_trace(sc, reinterpret_cast<const float4 *>(d_rays), n_rays,
                                               (flags & RT_TRACE_INVERT) != 0, (flags & RT_TRACE_ANY) != 0,
                                               reinterpret_cast<float4 *>(d_hits),
                                               reinterpret_cast<unsigned long long *>(d_counters), queue, s->cus,
                                               static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

int rt_trace_inw(const float *geom, uint32_t n, int layout, const float *nodes, const rt_ray *rays, uint32_t n_rays,
                 int flags, rt_hit *hits, int device, rt_stats *st) {
    if (!geom || !nodes || n == 0 || (layout != 1 && layout != 4)) return RT_E_ARG;
    return trace_blocking(
        flags, RT_TRACE_INVERT | RT_TRACE_ANY, rays, n_rays, hits, device, st,
        [&](rt_dev_scene *s) { return make_inw(s, geom, n, layout, nodes, nullptr, 0, nullptr, 0, 1); },
        [&](rt_dev_scene *s, const rt_ray *d_rays, rt_hit *d_hits, uint64_t *d_ctr) {
            return rt_trace_rays_async(s, d_rays, n_rays, flags, d_hits, d_ctr, nullptr);
        });
}

int rt_trace_iow_rays_async(rt_dev_scene *s, const rt_ray *d_rays, uint32_t n_rays, int flags, rt_hit *d_hits,
                            uint64_t *d_counters, void *stream) {
    if (!s || (flags & ~RT_TRACE_ANY)) return RT_E_ARG;
    if (s->kind != 3) return RT_E_UNSUPPORTED;
    if (s->broken || n_rays > (1u << 31)) return RT_E_ARG;
    if (n_rays == 0) return RT_OK;
    if (!d_rays || !d_hits) return RT_E_ARG;
    const rtk::IowScene sc = iow_view(*s);  // the sample tables stay unread
    // the ray queries' own queue counter (rt_trace_rays_async: past the fold kernels')
    unsigned *queue = s->counter.as<unsigned>() + 240;
    const hipError_t e = rtk::launch_iow_trace(sc, s->opt.iow_leaf_batch, reinterpret_cast<const float4 *>(d_rays),
                                               n_rays, (flags & RT_TRACE_ANY) != 0,
                                               reinterpret_cast<float4 *>(d_hits),
                                               reinterpret_cast<unsigned long long *>(d_counters), queue, s->cus,
                                               static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

int rt_trace_iow03(const float *types, const float *records, uint32_t n, const rt_ray *rays, uint32_t n_rays,
                   int flags, rt_hit *hits, int device, rt_stats *st) {
    if (!types || !records || n == 0) return RT_E_ARG;
    return trace_blocking(
        flags, RT_TRACE_ANY, rays, n_rays, hits, device, st,
        [&](rt_dev_scene *s) { return make_iow03(s, types, records, n, 1); },  // spp = 1: the sample tables are unused
        [&](rt_dev_scene *s, const rt_ray *d_rays, rt_hit *d_hits, uint64_t *d_ctr) {
            return rt_trace_iow_rays_async(s, d_rays, n_rays, flags, d_hits, d_ctr, nullptr);
        });
}

// ------------------------------------------------------------------------ path queries
int rt_path_rays_async(rt_dev_scene *s, const rt_path_ray *d_rays, uint32_t n_rays, int max_bounces, int flags,
                       rt_path_out *d_out, uint64_t *d_counters, void *stream) {
    static_assert(sizeof(rt_path_ray) == 32 && sizeof(rt_path_out) == 32, "rt_path_ray / rt_path_out are 2 float4 each");
    if (!s || (flags & ~RT_TRACE_INVERT) || max_bounces < 0) return RT_E_ARG;
    if (s->kind == 3) return RT_E_UNSUPPORTED;  // an IOW-03 sample starts from its pixel's previous one
    if (s->broken || n_rays > (1u << 31)) return RT_E_ARG;
    if (s->tex_missing) return RT_E_UNSUPPORTED;  // a textured object and no texture bound (rt_dev_scene_inw_update_device)
    if (n_rays == 0) return RT_OK;
    if (!d_rays || !d_out) return RT_E_ARG;
    const rtk::InwScene sc = inw_query_view(s);
    // its own queue counter: clear of the fold kernels' (bytes 0..767) and the ray queries' (word 240)
    unsigned *queue = s->counter.as<unsigned>() + 224;
    const hipError_t e = rtk::launch_inw_paths(sc, reinterpret_cast<const float4 *>(d_rays), n_rays, s->spp,
                                               max_bounces, (flags & RT_TRACE_INVERT) != 0,
                                               reinterpret_cast<float4 *>(d_out),
                                               reinterpret_cast<unsigned long long *>(d_counters), queue, s->cus,
                                               static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

int rt_path_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights, uint32_t n_lights,
                const rt_texture *tex, int n_tex, int spp, int max_bounces, const rt_path_ray *rays, uint32_t n_rays,
                int flags, rt_path_out *out, int device, rt_stats *st) {
    if (!geom || !nodes || n == 0 || (layout != 1 && layout != 4) || spp < 1 || max_bounces < 0) return RT_E_ARG;
    if (layout == 4 && n_lights > 0 && !lights) return RT_E_ARG;
    if (!textures_ok(tex, n_tex)) return RT_E_ARG;
    if ((flags & ~RT_TRACE_INVERT) || n_rays > (1u << 31) || (n_rays > 0 && (!rays || !out))) return RT_E_ARG;
    if (n_tex == 0 && inw_textured(geom, n, layout)) return RT_E_UNSUPPORTED;  // no texture bound
    return trace_blocking(
        flags, RT_TRACE_INVERT, rays, n_rays, out, device, st,
        // the scene of rt_render_inw_tex: the sunflower table is spp long
        [&](rt_dev_scene *s) { return make_inw(s, geom, n, layout, nodes, lights, n_lights, tex, n_tex, spp); },
        [&](rt_dev_scene *s, const rt_path_ray *d_rays, rt_path_out *d_out, uint64_t *d_ctr) {
            return rt_path_rays_async(s, d_rays, n_rays, max_bounces, flags, d_out, d_ctr, nullptr);
        });
}

// ------------------------------------------------------------------------ path queries, IOW-03
int rt_path_iow_rays_async(rt_dev_scene *s, const rt_path_iow_ray *d_rays, uint32_t n_rays, uint32_t chain,
                           int max_bounces, int flags, rt_path_iow_out *d_out, uint64_t *d_counters, void *stream) {
    static_assert(sizeof(rt_path_iow_ray) == 48 && sizeof(rt_path_iow_out) == 48,
                  "rt_path_iow_ray / rt_path_iow_out are 3 float4 each");
    if (!s || flags != 0 || chain == 0 || max_bounces < 0) return RT_E_ARG;
    if (s->kind != 3) return RT_E_UNSUPPORTED;
    if (s->broken || n_rays > (1u << 31)) return RT_E_ARG;
    if (n_rays == 0) return RT_OK;
    if (!d_rays || !d_out) return RT_E_ARG;
    const rtk::IowScene sc = iow_view(*s);
    // its own queue counter: clear of the renders' (word 0; the speculative pipeline's second queue is a
    // buffer of its own), the INW path queries' (word 224) and the ray queries' (word 240)
    unsigned *queue = s->counter.as<unsigned>() + 208;
    const hipError_t e = rtk::launch_iow_paths(sc, s->opt.iow_leaf_batch, max_bounces,
                                               reinterpret_cast<const float4 *>(d_rays), n_rays, chain, s->spp,
                                               reinterpret_cast<float4 *>(d_out),
                                               reinterpret_cast<unsigned long long *>(d_counters), queue, s->cus,
                                               static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

int rt_path_iow03(const float *types, const float *records, uint32_t n, int spp, int max_bounces,
                  const rt_path_iow_ray *rays, uint32_t n_rays, uint32_t chain, int flags, rt_path_iow_out *out,
                  int device, rt_stats *st) {
    if (!types || !records || n == 0 || spp < 1 || max_bounces < 0 || chain == 0) return RT_E_ARG;
    return trace_blocking(
        flags, 0, rays, n_rays, out, device, st,
        // the scene of rt_render_iow03: the scatter table is spp long
        [&](rt_dev_scene *s) { return make_iow03(s, types, records, n, spp); },
        [&](rt_dev_scene *s, const rt_path_iow_ray *d_rays, rt_path_iow_out *d_out, uint64_t *d_ctr) {
            return rt_path_iow_rays_async(s, d_rays, n_rays, chain, max_bounces, flags, d_out, d_ctr, nullptr);
        });
}

// ------------------------------------------------------------------------ pixel queries
int rt_camera_rays_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, const rt_pixel *d_pixels,
                         uint32_t n_pixels, uint32_t s0, uint32_t ns, void *d_rays, void *stream) {
    static_assert(sizeof(rt_pixel) == 8 && sizeof(rt_pixel) == sizeof(int2), "rt_pixel is an (x, y) int pair");
    if (!s || !cam || !params_ok(p) || p->spp != s->spp || s->broken) return RT_E_ARG;
    const uint64_t n = uint64_t(n_pixels) * ns;
    if (n > (uint64_t(1) << 31)) return RT_E_ARG;
    if (n == 0) return RT_OK;
    if (!d_pixels || !d_rays) return RT_E_ARG;
    const rtk::Frame f = make_frame(cam, p);
    const int2 *px = reinterpret_cast<const int2 *>(d_pixels);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t e = s->kind == 3 ? rtk::launch_camera_rays(f, iow_view(*s), px, uint32_t(n), s0, ns,
                                                                static_cast<float4 *>(d_rays), st)
                                      : rtk::launch_camera_rays(f, inw_view(*s), px, uint32_t(n), s0, ns,
                                                                static_cast<float4 *>(d_rays), st);
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

size_t rt_pixel_workspace_bytes(const rt_dev_scene *s, uint32_t n_pixels) {
    return s ? pixel_ws_bytes(s, n_pixels) : 0;
}

int rt_pixel_query_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, const rt_pixel *d_pixels,
                         uint32_t n_pixels, rt_pixel_out *d_pixels_out, void *d_samples_out, void *d_ws,
                         size_t ws_bytes, uint64_t *d_counters, void *stream) {
    static_assert(sizeof(rt_pixel_out) == 32, "rt_pixel_out is 2 float4");
    if (!s || !cam || !params_ok(p) || p->spp != s->spp || s->broken) return RT_E_ARG;
    if (s->tex_missing) return RT_E_UNSUPPORTED;  // a textured object and no texture bound (rt_dev_scene_inw_update_device)
    const uint64_t n = uint64_t(n_pixels) * uint32_t(p->spp);
    if (n > (uint64_t(1) << 31)) return RT_E_ARG;
    if (n_pixels > 0 && (!d_pixels || !d_pixels_out || !d_ws || ws_bytes < pixel_ws_bytes(s, n_pixels))) return RT_E_ARG;
    if (p->show_normal) return RT_E_UNSUPPORTED;  // one normal per sample, no path
    if (n_pixels == 0) return RT_OK;
    const bool iow = s->kind == 3;
    void *samples = d_samples_out ? d_samples_out : static_cast<char *>(d_ws) + size_t(n) * pixel_record_bytes(s);
    int rc = rt_camera_rays_async(s, cam, p, d_pixels, n_pixels, 0, uint32_t(p->spp), d_ws, stream);
    if (rc != RT_OK) return rc;
    if (iow) {
        rc = rt_path_iow_rays_async(s, static_cast<const rt_path_iow_ray *>(d_ws), uint32_t(n), uint32_t(p->spp),
                                    p->max_bounces, 0, static_cast<rt_path_iow_out *>(samples), d_counters, stream);
    } else {
        // the frame's child order: dot(dir, (1, 1, 1)) > 0 in binary32, the shader's order (inw_segment)
        const float dsum = (cam->dir[0] * 1.0f + cam->dir[1] * 1.0f) + cam->dir[2] * 1.0f;
        rc = rt_path_rays_async(s, static_cast<const rt_path_ray *>(d_ws), uint32_t(n), p->max_bounces,
                                dsum > 0.0f ? RT_TRACE_INVERT : 0, static_cast<rt_path_out *>(samples), d_counters,
                                stream);
    }
    if (rc != RT_OK) return rc;
    const hipError_t e = rtk::launch_pixel_fold(make_frame(cam, p), iow, reinterpret_cast<const int2 *>(d_pixels),
                                                n_pixels, static_cast<const float4 *>(samples),
                                                reinterpret_cast<float4 *>(d_pixels_out),
                                                static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

int rt_pixels_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                  uint32_t n_lights, const rt_texture *tex, int n_tex, const rt_camera *cam, const rt_params *p,
                  const rt_pixel *pixels, uint32_t n_pixels, rt_path_ray *rays_out, rt_path_out *samples_out,
                  rt_pixel_out *pixels_out, int device, rt_stats *st) {
    if (!geom || !nodes || n == 0 || (layout != 1 && layout != 4) || !cam || !params_ok(p)) return RT_E_ARG;
    if (layout == 4 && n_lights > 0 && !lights) return RT_E_ARG;
    if (!textures_ok(tex, n_tex)) return RT_E_ARG;
    if (!pixels_args_ok(p, pixels, n_pixels, pixels_out)) return RT_E_ARG;
    if (n_tex == 0 && inw_textured(geom, n, layout)) return RT_E_UNSUPPORTED;  // no texture bound
    if (p->show_normal) return RT_E_UNSUPPORTED;
    return pixels_blocking(cam, p, pixels, n_pixels, rays_out, samples_out, pixels_out, device, st, [&](rt_dev_scene *s) {
        return make_inw(s, geom, n, layout, nodes, lights, n_lights, tex, n_tex, p->spp);
    });
}

int rt_pixels_iow03(const float *types, const float *records, uint32_t n, const rt_camera *cam, const rt_params *p,
                    const rt_pixel *pixels, uint32_t n_pixels, rt_path_iow_ray *rays_out, rt_path_iow_out *samples_out,
                    rt_pixel_out *pixels_out, int device, rt_stats *st) {
    if (!types || !records || n == 0 || !cam || !params_ok(p)) return RT_E_ARG;
    if (!pixels_args_ok(p, pixels, n_pixels, pixels_out)) return RT_E_ARG;
    if (p->show_normal) return RT_E_UNSUPPORTED;
    return pixels_blocking(cam, p, pixels, n_pixels, rays_out, samples_out, pixels_out, device, st,
                           [&](rt_dev_scene *s) { return make_iow03(s, types, records, n, p->spp); });
}

// ------------------------------------------------------------------------ progressive passes
int rt_render_pass_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, uint32_t s0, uint32_t ns,
                         rt_pass_state *d_state, float *d_rgba, float *d_depth, uint64_t *d_counters, void *stream) {
    static_assert(sizeof(rt_pass_state) == 32, "rt_pass_state is 2 float4");
    if (!s || !cam || !params_ok(p) || !d_state || p->spp != s->spp || s0 >= uint32_t(p->spp) || s->broken)
        return RT_E_ARG;
    if (s->tex_missing) return RT_E_UNSUPPORTED;  // a textured object and no texture bound (rt_dev_scene_inw_update_device)
    if (p->show_normal) return RT_E_UNSUPPORTED;  // one normal per sample, no fold state
    if (ns == 0) return RT_OK;
    const uint32_t s1 = uint32_t(std::min<uint64_t>(uint64_t(s0) + ns, pass_stop(s)));
    const rtk::Frame f = make_pass_frame(s, cam, p, d_rgba, d_depth, d_counters);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    float4 *state = reinterpret_cast<float4 *>(d_state);
    if (s->kind == 3) {
        // its own queue counter: clear of the fold kernels' (bytes 0..767) and the queries' (words 208, 224, 240)
        unsigned *queue = s->counter.as<unsigned>() + 192;
        const hipError_t e = rtk::launch_iow_pass(f, iow_view(*s), s0, s1, state, queue, s->cus, st);
        return e == hipSuccess ? RT_OK : launch_failed(e);
    }
    const uint32_t units = rtk::units_of(f);
    if (units == 0 || units > (1u << 31)) return RT_E_ARG;
    return pass_inw_chunks(s, cam, p, units, s1 - s0, 0, d_counters, st,
        [&](const rtk::InwScene &sc, uint32_t c0, uint32_t nsc, float4 *rays) {
            return rtk::launch_pass_rays(f, sc, s0 + c0, nsc, rays, st);
        },
        [&](uint32_t c0, uint32_t nsc, bool last, const float4 *out) {
            return rtk::launch_pass_fold(f, s0 + c0, nsc, last ? s1 : 0u, out, state, st);
        });
}

int rt_render_passes_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                         uint32_t n_lights, const rt_texture *tex, int n_tex, const rt_camera *cam, const rt_params *p,
                         const uint32_t *cuts, int n_cuts, float *rgba, float *depth, rt_pass_state *state_out,
                         int device, rt_stats *st) {
    if (!geom || !nodes || n == 0 || (layout != 1 && layout != 4) || !cam || !params_ok(p) || !rgba) return RT_E_ARG;
    if (layout == 4 && n_lights > 0 && !lights) return RT_E_ARG;
    if (!textures_ok(tex, n_tex) || !cuts_ok(p, cuts, n_cuts)) return RT_E_ARG;
    if (n_tex == 0 && inw_textured(geom, n, layout)) return RT_E_UNSUPPORTED;  // no texture bound
    if (p->show_normal) return RT_E_UNSUPPORTED;
    return passes_blocking(cam, p, cuts, n_cuts, rgba, depth, state_out, device, st, [&](rt_dev_scene *s) {
        return make_inw(s, geom, n, layout, nodes, lights, n_lights, tex, n_tex, p->spp);
    });
}

int rt_render_passes_iow03(const float *types, const float *records, uint32_t n, const rt_camera *cam,
                           const rt_params *p, const uint32_t *cuts, int n_cuts, float *rgba,
                           rt_pass_state *state_out, int device, rt_stats *st) {
    if (!types || !records || n == 0 || !cam || !params_ok(p) || !rgba || !cuts_ok(p, cuts, n_cuts)) return RT_E_ARG;
    if (p->show_normal) return RT_E_UNSUPPORTED;
    return passes_blocking(cam, p, cuts, n_cuts, rgba, nullptr, state_out, device, st,
                           [&](rt_dev_scene *s) { return make_iow03(s, types, records, n, p->spp); });
}

// A pass over a packed tile list: rt_render_pass_async's launches on rt_render_tiles_async's frame; the pass
// kernels' tile-list instances index state and image by slot.
int rt_render_pass_tiles_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, const int *d_tiles,
                               int n_tiles, int tile_size, uint32_t s0, uint32_t ns, rt_pass_state *d_state_packed,
                               float *d_out_packed, float *d_out_depth_packed, uint64_t *d_counters, void *stream) {
    if (!s || !cam || !params_ok(p) || !d_state_packed || p->spp != s->spp || s0 >= uint32_t(p->spp) || s->broken)
        return RT_E_ARG;
    if (!d_tiles || n_tiles <= 0 || tile_size <= 0 || tile_size % 16 != 0) return RT_E_ARG;
    if (uint64_t(n_tiles) * uint64_t(tile_size) * uint64_t(tile_size) > (uint64_t(1) << 31)) return RT_E_ARG;
    if (s->tex_missing) return RT_E_UNSUPPORTED;  // a textured object and no texture bound (rt_dev_scene_inw_update_device)
    if (p->show_normal) return RT_E_UNSUPPORTED;  // one normal per sample, no fold state
    if (ns == 0) return RT_OK;
    const uint32_t s1 = uint32_t(std::min<uint64_t>(uint64_t(s0) + ns, pass_stop(s)));
    rt_params whole = *p;
    whole.tile_x0 = whole.tile_y0 = whole.tile_w = whole.tile_h = 0;  // the list says which pixels
    rtk::Frame f = make_pass_frame(s, cam, &whole, d_out_packed, d_out_depth_packed, d_counters);
    f.tiles = d_tiles; f.n_tiles = n_tiles; f.tile_size = tile_size;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    float4 *state = reinterpret_cast<float4 *>(d_state_packed);
    if (s->kind == 3) {
        unsigned *queue = s->counter.as<unsigned>() + 192;  // the passes' own: calls on one scene do not overlap
        const hipError_t e = rtk::launch_iow_pass(f, iow_view(*s), s0, s1, state, queue, s->cus, st);
        return e == hipSuccess ? RT_OK : launch_failed(e);
    }
    return pass_inw_chunks(s, cam, p, rtk::units_of(f), s1 - s0, 0, d_counters, st,
        [&](const rtk::InwScene &sc, uint32_t c0, uint32_t nsc, float4 *rays) {
            return rtk::launch_pass_rays(f, sc, s0 + c0, nsc, rays, st);
        },
        [&](uint32_t c0, uint32_t nsc, bool last, const float4 *out) {
            return rtk::launch_pass_fold(f, s0 + c0, nsc, last ? s1 : 0u, out, state, st);
        });
}

// ------------------------------------------------------------------------ adaptive sample passes
int rt_render_pass_pixels_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, const rt_pixel *d_pixels,
                                uint32_t n_pixels, uint32_t ns, rt_pass_state *d_state, rt_pass_aux *d_aux,
                                float *d_rgba, float *d_depth, uint64_t *d_counters, void *stream) {
    static_assert(sizeof(rt_pass_aux) == 16, "rt_pass_aux is a float4");
    if (!s || !cam || !params_ok(p) || !d_state || !d_aux || p->spp != s->spp || s->broken) return RT_E_ARG;
    if (s->tex_missing) return RT_E_UNSUPPORTED;  // a textured object and no texture bound (rt_dev_scene_inw_update_device)
    if (n_pixels > (1u << 31) || (n_pixels > 0 && !d_pixels)) return RT_E_ARG;
    if (p->show_normal) return RT_E_UNSUPPORTED;  // one normal per sample, no fold state
    if (n_pixels == 0 || ns == 0) return RT_OK;
    const uint32_t stop = pass_stop(s);
    ns = std::min(ns, stop);  // no pixel has more samples left
    rt_params whole = *p;
    whole.tile_w = whole.tile_h = 0;  // the list says which pixels
    const rtk::Frame f = make_pass_frame(s, cam, &whole, d_rgba, d_depth, d_counters);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    float4 *state = reinterpret_cast<float4 *>(d_state), *aux = reinterpret_cast<float4 *>(d_aux);
    const int2 *px = reinterpret_cast<const int2 *>(d_pixels);
    if (s->kind == 3) {
        unsigned *queue = s->counter.as<unsigned>() + 192;  // the passes' own: calls on one scene do not overlap
        const hipError_t e = rtk::launch_iow_adapt(f, iow_view(*s), px, n_pixels, stop, ns, state, aux, queue, s->cus, st);
        return e == hipSuccess ? RT_OK : launch_failed(e);
    }
    // every chunk's fold advances the counts the next chunk's rays start from; rt_debug_adaptive_chunk caps it
    return pass_inw_chunks(s, cam, p, n_pixels, ns, rtk::adaptive_chunk_cap_now(), d_counters, st,
        [&](const rtk::InwScene &sc, uint32_t, uint32_t nsc, float4 *rays) {
            return rtk::launch_adapt_rays(f, sc, px, n_pixels, aux, stop, nsc, rays, st);
        },
        [&](uint32_t, uint32_t nsc, bool last, const float4 *out) {
            return rtk::launch_adapt_fold(f, px, n_pixels, stop, nsc, last, out, state, aux, st);
        });
}

int rt_pass_select_async(rt_dev_scene *s, const rt_params *p, const rt_pass_state *d_state, const rt_pass_aux *d_aux,
                         float tol, uint32_t min_samples, rt_pixel *d_list, uint32_t *d_n_active, float *d_err,
                         void *stream) {
    if (!s || !params_ok(p) || !d_state || !d_aux || !d_list || !d_n_active || p->spp != s->spp || s->broken)
        return RT_E_ARG;
    const rtk::Frame f = make_frame(nullptr, p);
    const uint32_t units = rtk::units_of(f);
    if (units == 0 || units > (1u << 31)) return RT_E_ARG;
    HIP_OK(s->select_ws.reserve((size_t(rtk::select_blocks(f)) + 1) * sizeof(uint2)));
    const hipError_t e = rtk::launch_pass_select(f, reinterpret_cast<const float4 *>(d_state),
                                                 reinterpret_cast<const float4 *>(d_aux), tol, min_samples, pass_stop(s),
                                                 reinterpret_cast<int2 *>(d_list), d_n_active, d_err,
                                                 s->select_ws.as<uint2>(), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

// The adaptive pair on a packed tile list: the same launches with the list entries slots and everything
// indexed by slot (the kernels' tile-list instances).
int rt_render_pass_slots_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, const int *d_tiles,
                               int n_tiles, int tile_size, const uint32_t *d_slots, uint32_t n_slots, uint32_t ns,
                               rt_pass_state *d_state_packed, rt_pass_aux *d_aux_packed, float *d_out_packed,
                               float *d_out_depth_packed, uint64_t *d_counters, void *stream) {
    if (!s || !cam || !params_ok(p) || !d_state_packed || !d_aux_packed || p->spp != s->spp || s->broken)
        return RT_E_ARG;
    if (!tile_list_ok(d_tiles, n_tiles, tile_size)) return RT_E_ARG;
    if (n_slots > (1u << 31) || (n_slots > 0 && !d_slots)) return RT_E_ARG;
    if (s->tex_missing) return RT_E_UNSUPPORTED;  // a textured object and no texture bound (rt_dev_scene_inw_update_device)
    if (p->show_normal) return RT_E_UNSUPPORTED;  // one normal per sample, no fold state
    if (n_slots == 0 || ns == 0) return RT_OK;
    const uint32_t stop = pass_stop(s);
    ns = std::min(ns, stop);  // no slot has more samples left
    rt_params whole = *p;
    whole.tile_x0 = whole.tile_y0 = whole.tile_w = whole.tile_h = 0;  // the list says which pixels
    rtk::Frame f = make_pass_frame(s, cam, &whole, d_out_packed, d_out_depth_packed, d_counters);
    f.tiles = d_tiles; f.n_tiles = n_tiles; f.tile_size = tile_size;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    float4 *state = reinterpret_cast<float4 *>(d_state_packed), *aux = reinterpret_cast<float4 *>(d_aux_packed);
    if (s->kind == 3) {
        unsigned *queue = s->counter.as<unsigned>() + 192;  // the passes' own: calls on one scene do not overlap
        const hipError_t e = rtk::launch_iow_adapt(f, iow_view(*s), d_slots, n_slots, stop, ns, state, aux, queue, s->cus, st);
        return e == hipSuccess ? RT_OK : launch_failed(e);
    }
    return pass_inw_chunks(s, cam, p, n_slots, ns, rtk::adaptive_chunk_cap_now(), d_counters, st,
        [&](const rtk::InwScene &sc, uint32_t, uint32_t nsc, float4 *rays) {
            return rtk::launch_adapt_rays(f, sc, d_slots, n_slots, aux, stop, nsc, rays, st);
        },
        [&](uint32_t, uint32_t nsc, bool last, const float4 *out) {
            return rtk::launch_adapt_fold(f, d_slots, n_slots, stop, nsc, last, out, state, aux, st);
        });
}

int rt_pass_select_tiles_async(rt_dev_scene *s, const rt_params *p, const int *d_tiles, int n_tiles, int tile_size,
                               const rt_pass_state *d_state_packed, const rt_pass_aux *d_aux_packed, float tol,
                               uint32_t min_samples, uint32_t *d_slots, uint32_t *d_n_active, float *d_err_packed,
                               void *stream) {
    if (!s || !params_ok(p) || !d_state_packed || !d_aux_packed || !d_slots || !d_n_active || p->spp != s->spp ||
        s->broken)
        return RT_E_ARG;
    if (!tile_list_ok(d_tiles, n_tiles, tile_size)) return RT_E_ARG;
    if (s->tex_missing) return RT_E_UNSUPPORTED;  // a textured object and no texture bound (rt_dev_scene_inw_update_device)
    if (p->show_normal) return RT_E_UNSUPPORTED;  // one normal per sample, no fold state
    rtk::Frame f = make_frame(nullptr, p);
    f.tiles = d_tiles; f.n_tiles = n_tiles; f.tile_size = tile_size;
    HIP_OK(s->select_ws.reserve((size_t(rtk::select_blocks(f)) + 1) * sizeof(uint2)));
    const hipError_t e = rtk::launch_pass_select(f, reinterpret_cast<const float4 *>(d_state_packed),
                                                 reinterpret_cast<const float4 *>(d_aux_packed), tol, min_samples,
                                                 pass_stop(s), d_slots, d_n_active, d_err_packed,
                                                 s->select_ws.as<uint2>(), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : launch_failed(e);
}

int rt_render_adaptive_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                           uint32_t n_lights, const rt_texture *tex, int n_tex, const rt_camera *cam, const rt_params *p,
                           uint32_t batch, float tol, uint32_t min_samples, uint32_t max_rounds, float *rgba,
                           float *depth, uint32_t *count, float *err, rt_pass_state *state_out, rt_pass_aux *aux_out,
                           uint32_t *rounds_out, int device, rt_stats *st) {
    if (!geom || !nodes || n == 0 || (layout != 1 && layout != 4) || !cam || !params_ok(p) || !rgba || batch == 0)
        return RT_E_ARG;
    if (layout == 4 && n_lights > 0 && !lights) return RT_E_ARG;
    if (!textures_ok(tex, n_tex)) return RT_E_ARG;
    if (n_tex == 0 && inw_textured(geom, n, layout)) return RT_E_UNSUPPORTED;  // no texture bound
    if (p->show_normal) return RT_E_UNSUPPORTED;
    return adaptive_blocking(cam, p, batch, tol, min_samples, max_rounds, rgba, depth, count, err, state_out, aux_out,
                             rounds_out, device, st, [&](rt_dev_scene *s) {
        return make_inw(s, geom, n, layout, nodes, lights, n_lights, tex, n_tex, p->spp);
    });
}

int rt_render_adaptive_iow03(const float *types, const float *records, uint32_t n, const rt_camera *cam,
                             const rt_params *p, uint32_t batch, float tol, uint32_t min_samples, uint32_t max_rounds,
                             float *rgba, uint32_t *count, float *err, rt_pass_state *state_out, rt_pass_aux *aux_out,
                             uint32_t *rounds_out, int device, rt_stats *st) {
    if (!types || !records || n == 0 || !cam || !params_ok(p) || !rgba || batch == 0) return RT_E_ARG;
    if (p->show_normal) return RT_E_UNSUPPORTED;
    return adaptive_blocking(cam, p, batch, tol, min_samples, max_rounds, rgba, nullptr, count, err, state_out,
                             aux_out, rounds_out, device, st,
                             [&](rt_dev_scene *s) { return make_iow03(s, types, records, n, p->spp); });
}

// ------------------------------------------------------------------------ rt_scene.h
int rt_scene_preset(int preset, uint32_t seed, int n_hint, rt_geom_desc *out, int cap, rt_cam_desc *cam,
                    rt_params *params) {
    try {
        std::vector<rt_geom_desc> v;
        rt_cam_desc c;
        rt_params p;
        int n = rtamd::scene_preset(preset, seed, n_hint, v, c, p);
        if (n < 0) return n;
        if (out) {
            if (cap < n) return RT_E_ARG;
            std::memcpy(out, v.data(), v.size() * sizeof(rt_geom_desc));
        }
        if (cam) *cam = c;
        if (params) *params = p;
        return n;
    } catch (...) {
        return RT_E_ARG;
    }
}

int rt_camera_from_desc(const rt_cam_desc *d, int stage, rt_camera *out) {
    if (!d || !out) return RT_E_ARG;
    const bool iow = stage == RT_STAGE_IOW01 || stage == RT_STAGE_IOW02 || stage == RT_STAGE_IOW03;
    if (!iow && stage != RT_STAGE_INW01 && stage != RT_STAGE_INW04) return RT_E_ARG;
    rtamd::Vec3 fr = rtamd::front_from_pitch_yaw(d->pitch_deg, d->yaw_deg, iow);
    std::memcpy(out->pos, d->position, sizeof(out->pos));
    out->dir[0] = fr.x; out->dir[1] = fr.y; out->dir[2] = fr.z;
    out->fov_y_rad = rtamd::radians(d->fov_y_deg);
    out->aperture = d->aperture;
    out->focus_dist = d->focus_dist;
    return RT_OK;
}

int rt_pack_iow03(const rt_geom_desc *g, uint32_t n, float *types, float *records) {
    if (!g || !types || !records) return RT_E_ARG;
    for (uint32_t k = 0; k < n; k++) {
        rtamd::IowGeometry geo = rtamd::to_iow(g[k]);
        geo.fill_buffer(records + size_t(k) * 24);
        types[k] = float(geo.type);
    }
    return RT_OK;
}

// Groups::Geometry::FillBuffer (groups.h:45-64) packs the same position / inverse rotation /
// scale / colour as the IOW-03 Geometry::FillBuffer (materials.h:48-76): its first 18 floats.
int rt_pack_iow02(const rt_geom_desc *g, uint32_t n, float *types, float *records) {
    if (!g || !types || !records) return RT_E_ARG;
    float r24[24];
    for (uint32_t k = 0; k < n; k++) {
        rtamd::IowGeometry geo = rtamd::to_iow(g[k]);
        geo.fill_buffer(r24);
        std::memcpy(records + size_t(k) * 18, r24, 18 * sizeof(float));
        types[k] = float(geo.type);
    }
    return RT_OK;
}

int rt_pack_inw(const rt_geom_desc *g, uint32_t n, int layout, float *geom, float *aabbs, float *lights,
                uint32_t *n_lights) {
    if (!g || (layout != 1 && layout != 4)) return RT_E_ARG;
    uint32_t nl = 0;
    for (uint32_t k = 0; k < n; k++) {
        std::pair<rtamd::Vec3, rtamd::Vec3> bb;
        if (layout == 1) {
            rtamd::GeometryData d = rtamd::to_inw01(g[k]);
            if (geom) d.fill_buffer(geom + size_t(k) * 28);
            bb = d.bb_min_max();
        } else {
            rtamd::GeometryData04 d = rtamd::to_inw04(g[k]);
            if (geom) d.fill_buffer(geom + size_t(k) * 28);
            bb = d.bb_min_max();
            if (d.emissive) {  // Lights::FillBuffer, lights.cpp:261-264
                if (lights) {
                    float *L = lights + size_t(nl) * 7;
                    L[0] = bb.first.x; L[1] = bb.first.y; L[2] = bb.first.z;
                    L[3] = bb.second.x; L[4] = bb.second.y; L[5] = bb.second.z;
                    uint32_t idx = k;
                    std::memcpy(L + 6, &idx, 4);
                }
                nl++;
            }
        }
        if (aabbs) {
            float *b = aabbs + size_t(k) * 6;
            b[0] = bb.first.x; b[1] = bb.first.y; b[2] = bb.first.z;
            b[3] = bb.second.x; b[4] = bb.second.y; b[5] = bb.second.z;
        }
    }
    if (n_lights) *n_lights = nl;
    return RT_OK;
}

int rt_sample_tables(int spp, float *sunflower, float *fib, int *ring) {
    if (spp < 1) return RT_E_ARG;
    rtamd::sample_tables(spp, sunflower, fib, ring);
    return RT_OK;
}

int rt_render_iow00(const rt_params *p, float *rgba) {
    if (!p || p->width <= 0 || p->height <= 0 || !rgba) return RT_E_ARG;
    int rc = check_device(p->device);
    if (rc != RT_OK) return rc;
    const size_t npx = size_t(p->width) * p->height;
    DevBuf d_rgba;
    HIP_OK(d_rgba.alloc(npx * 16));
    HIP_OK(rtk::launch_iow00(p->width, p->height, d_rgba.as<float>(), nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(rgba, d_rgba.p, npx * 16, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_render_iow02(const float *types, const float *records, uint32_t n, const rt_camera *cam, const rt_params *p,
                    int cull_front, int cull_back, float *rgba, rt_stats *st) {
    if ((n > 0 && (!types || !records)) || !cam || !params_ok(p) || !rgba) return RT_E_ARG;
    int rc = check_device(p->device);
    if (rc != RT_OK) return rc;
    rtk::Frame f = make_frame(cam, p);
    const size_t npx = size_t(p->width) * p->height;
    // host tables: the ring schedule (02.glsl:146-157) and pow(0.4, i) (02.glsl:206), double -> float
    std::vector<int> ring(size_t(p->spp) * 2);
    rtamd::sample_tables(p->spp, nullptr, nullptr, ring.data());
    std::vector<float> pw(size_t(std::max(1, p->max_bounces)));
    for (int i = 0; i < p->max_bounces; i++) pw[size_t(i)] = float(std::pow(double(0.4f), double(i)));
    DevBuf d_rgba, d_types, d_rec, d_ring, d_pw, d_ctr;
    HIP_OK(d_rgba.alloc(npx * 16));
    HIP_OK(hipMemcpy(d_rgba.p, rgba, npx * 16, hipMemcpyHostToDevice));  // untouched pixels keep their value
    if (n > 0) {
        HIP_OK(d_types.upload(types, size_t(n) * sizeof(float)));
        HIP_OK(d_rec.upload(records, size_t(n) * 18 * sizeof(float)));
    }
    HIP_OK(d_ring.upload(ring.data(), ring.size() * sizeof(int)));
    HIP_OK(d_pw.upload(pw.data(), pw.size() * sizeof(float)));
    HIP_OK(d_ctr.alloc(6 * sizeof(unsigned long long)));
    HIP_OK(hipMemset(d_ctr.p, 0, 6 * sizeof(unsigned long long)));
    f.out_rgba = d_rgba.as<float>();
    f.counters = d_ctr.as<unsigned long long>();
    double ms = 0.0;
    rc = timed([&] {
        HIP_OK(rtk::launch_iow02(f, d_types.as<float>(), d_rec.as<float>(), n, d_ring.as<int>(), d_pw.as<float>(),
                                 cull_front, cull_back, nullptr));
        return RT_OK;
    }, &ms);
    if (rc != RT_OK) return rc;
    HIP_OK(hipMemcpy(rgba, d_rgba.p, npx * 16, hipMemcpyDeviceToHost));
    if (st) {  // this stage counts its rays and primitive tests only
        rt_stats all;
        if ((rc = read_stats(d_ctr.p, ms, &all)) != RT_OK) return rc;
        std::memset(st, 0, sizeof(*st));
        st->segments = all.segments;
        st->prim_tests = all.prim_tests;
        st->ms = all.ms;
    }
    return RT_OK;
}

int rt_render_inw_mf(const float *geom, uint32_t n, const float *nodes, const rt_camera *cam, const float *focus,
                     int n_focus, const rt_params *p, float *rgba, float *depth, rt_stats *st) {
    if (!geom || !nodes || n == 0 || !cam || !params_ok(p) || !rgba || !focus || n_focus < 1 || n_focus > 9)
        return RT_E_ARG;
    return render_temp(cam, p, rgba, depth, st, [&](rt_dev_scene *s) {
        s->n_focus = n_focus;
        std::memcpy(s->focus, focus, sizeof(float) * size_t(n_focus));
        return make_inw(s, geom, n, 1, nodes, nullptr, 0, nullptr, 0, p->spp);
    });
}

}  // extern "C"
