// rt_multi.hip -- the multi-GPU partition behind the C ABI (BASELINE configs[3]):
// one host thread drives several devices of this process (SURVEY 8b "one host thread drives
// all devices"), the frame's tiles are dealt across them, every device renders its share with
// rt_render_tiles_async on a stream of its own, and the packed tiles travel to device 0 in one
// RCCL exchange (grouped ncclSend / ncclRecv over xGMI), where one kernel unpacks them into the
// W x H image.  This generalises the reference's per-tile dispatch loop
// (In-One-Weekend/03_Shadows_and_Materials/materials.cpp:98-152) to devices and replaces the
// single-device dispatch of RT_Base<>::OnUpdateBase (In-Next-Week/base.h:148-173) for a C++ host.
// bench.py's one-process-per-GPU torchrun path (the driver's scaling run) deals the same tiles
// (rt_tile_deal == bench.deal_order) and gathers them with torch.distributed on RCCL.
// Progressive frames (rt_render_pass_multi_async): every device keeps the fold state of its share's slots
// and continues it with rt_render_pass_tiles_async; a pass that is asked for an image ends in the same
// exchange and unpack, one that is not sends its counters alone.
// Adaptive frames (rt_render_adaptive_multi_async): beside the states every device keeps the aux records, a
// slot list and packed image buffers of the adaptive frame; a round is rt_render_pass_slots_async over the
// list, rt_pass_select_tiles_async for the next list, the active count to pinned host memory behind an event,
// and the same exchange.  The next round waits for the counts on the host and sizes its launches by them.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_host.hpp"

namespace {

// ------------------------------------------------------------------ unpack + counter sum
// recv: the gathered packed tiles, device after device (device r's tiles at its slot offset,
// in its deal order); tiles: their (tx, ty) in the same order.  One thread per pixel of the
// gathered tiles; pixels outside the image (the ragged right / top tiles) are skipped.
__global__ __launch_bounds__(256) void k_unpack_tiles(const float4 *recv, const float *recv_depth, const int2 *tiles,
                                                      uint32_t n_px, int T, int W, int H, float4 *rgba, float *depth) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_px) return;  // no cross-lane work in this kernel
    const uint32_t area = uint32_t(T) * uint32_t(T);
    const int2 t = tiles[i / area];
    const uint32_t r = i % area;
    const int x = t.x * T + int(r % uint32_t(T)), y = t.y * T + int(r / uint32_t(T));
    if (x >= W || y >= H) return;
    const size_t o = size_t(y) * size_t(W) + size_t(x);
    rgba[o] = recv[i];
    if (depth) depth[o] = recv_depth[i];
}

// The sample counts of a share's slots out of its aux records (rt_pass_aux: even.xyz, count), one thread a slot.
__global__ __launch_bounds__(256) void k_aux_counts(const uint4 *aux, uint32_t n, uint32_t *counts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;  // no cross-lane work in this kernel
    counts[i] = aux[i].w;
}

// k_unpack_tiles for the gathered counts: d_count[y * W + x] of the slots inside the image.
__global__ __launch_bounds__(256) void k_unpack_counts(const uint32_t *recv, const int2 *tiles, uint32_t n_px, int T,
                                                       int W, int H, uint32_t *count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_px) return;  // no cross-lane work in this kernel
    const uint32_t area = uint32_t(T) * uint32_t(T);
    const int2 t = tiles[i / area];
    const uint32_t r = i % area;
    const int x = t.x * T + int(r % uint32_t(T)), y = t.y * T + int(r / uint32_t(T));
    if (x >= W || y >= H) return;
    count[size_t(y) * size_t(W) + size_t(x)] = recv[i];
}

// d_counters[k] += sum over devices of their 6 counters (one 64-lane block)
__global__ __launch_bounds__(64) void k_sum_counters(const unsigned long long *all, int n_dev,
                                                     unsigned long long *out) {
    const int k = int(threadIdx.x);
    if (k >= 6) return;  // no cross-lane work in this kernel
    unsigned long long s = 0;
    for (int r = 0; r < n_dev; r++) s += all[r * 6 + k];
    out[k] += s;
}

struct Buf {  // a device allocation on a given device (freed there)
    void *p = nullptr;
    size_t bytes = 0;
    int dev = 0;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() {
        if (p) {
            int cur = 0;
            (void)hipGetDevice(&cur);
            (void)hipSetDevice(dev);
            (void)hipFree(p);
            (void)hipSetDevice(cur);
        }
    }
    // (re)allocate on the current device, `d`, when smaller than b
    hipError_t ensure(size_t b, int d) {
        if (p && bytes >= b) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; }
        dev = d;
        bytes = b;
        return hipMalloc(&p, b ? b : 16);
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

#define MULTI_HIP(expr)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            std::fprintf(stderr, "[rt_hip] %s failed: %s\n", #expr, hipGetErrorString(e_));         \
            return RT_E_HIP;                                                                       \
        }                                                                                          \
    } while (0)
#define MULTI_NCCL(expr)                                                                            \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess) {                                                                   \
            std::fprintf(stderr, "[rt_hip] %s failed: %s\n", #expr, ncclGetErrorString(r_));       \
            return RT_E_HIP;                                                                       \
        }                                                                                          \
    } while (0)

// restores the caller's current device on scope exit
struct DeviceGuard {
    int cur = 0;
    DeviceGuard() { (void)hipGetDevice(&cur); }
    ~DeviceGuard() { (void)hipSetDevice(cur); }
};

}  // namespace

struct rt_group {
    int n = 0;
    std::vector<int> dev;
    std::vector<ncclComm_t> comm;
    std::vector<hipStream_t> st;  // st[0] unused: device 0 works on the caller's stream
    struct Share {                // one device's share of the frame
        Buf tiles, packed, depth, counters;
        Buf state;  // the fold state of the share's slots (rt_pass_state, 32 B each): it never leaves its device
        int n_tiles = 0;
        // the adaptive frame (rt_render_adaptive_multi_async), allocated when the deal's first one begins:
        // the aux records beside the states, the slot list and its active count, the counts as they travel,
        // and packed image and depth buffers of its own, which rt_render_multi_async never writes
        Buf aux, slots, n_active, counts, a_packed, a_depth;
        uint32_t n_inside = 0;       // the share's slots inside the image
        hipEvent_t counted = nullptr;  // behind the copy of n_active to the group's pinned counts
    };
    std::vector<std::unique_ptr<Share>> share;
    Buf recv, recv_depth, recv_tiles, recv_ctr, recv_count;  // on device 0
    // the deal the buffers hold (re-uploaded when the frame or tile size changes)
    int W = 0, H = 0, T = 0;
    std::vector<uint32_t> off;  // device r's first tile in the gathered order
    uint32_t samples = 0;       // rt_render_pass_multi_async: the samples the states hold for this deal
    bool adaptive = false;      // the states of this deal were left by an adaptive round, and no pass ran since
    uint32_t *h_active = nullptr;  // pinned: device r's active count of the last adaptive round
    ~rt_group() {
        for (size_t r = 0; r < share.size(); r++)
            if (share[r]->counted) {
                (void)hipSetDevice(dev[r]);
                (void)hipEventDestroy(share[r]->counted);
            }
        if (h_active) (void)hipHostFree(h_active);
        share.clear();
        for (ncclComm_t c : comm)
            if (c) (void)ncclCommDestroy(c);
        for (size_t r = 0; r < st.size(); r++)
            if (st[r]) {
                (void)hipSetDevice(dev[r]);
                (void)hipStreamDestroy(st[r]);
            }
    }
};

namespace {

// the deal of a W x H frame in T x T tiles over g's devices, uploaded to every device's tile list
// and to device 0's gathered order.  The buffers are reused when large enough, so an earlier frame
// still running on the group's streams (device 0: the caller's stream s0) is waited for first: the
// API is asynchronous, and a null-stream copy does not wait for non-blocking streams
int set_deal(rt_group *g, int W, int H, int T, hipStream_t s0) {
    if (g->W == W && g->H == H && g->T == T) return RT_OK;
    g->samples = 0;  // the states of another deal are no one's
    g->adaptive = false;
    for (int r = 0; r < g->n; r++) {
        MULTI_HIP(hipSetDevice(g->dev[size_t(r)]));
        MULTI_HIP(hipStreamSynchronize(r == 0 ? s0 : g->st[size_t(r)]));
    }
    const std::vector<std::pair<int, int>> order = rtamd::tile_deal(W, H, T, g->n);
    std::vector<std::vector<int>> lists(size_t(g->n));
    for (size_t k = 0; k < order.size(); k++) {
        auto &l = lists[k % size_t(g->n)];
        l.push_back(order[k].first);
        l.push_back(order[k].second);
    }
    std::vector<int> all;
    g->off.assign(size_t(g->n) + 1, 0);
    const size_t area = size_t(T) * size_t(T);
    for (int r = 0; r < g->n; r++) {
        auto &S = *g->share[size_t(r)];
        S.n_tiles = int(lists[size_t(r)].size() / 2);
        S.n_inside = 0;
        for (int k = 0; k < S.n_tiles; k++)
            S.n_inside += uint32_t(std::min(T, W - lists[size_t(r)][size_t(2 * k)] * T)) *
                          uint32_t(std::min(T, H - lists[size_t(r)][size_t(2 * k + 1)] * T));
        g->off[size_t(r) + 1] = g->off[size_t(r)] + uint32_t(S.n_tiles);
        all.insert(all.end(), lists[size_t(r)].begin(), lists[size_t(r)].end());
        MULTI_HIP(hipSetDevice(g->dev[size_t(r)]));
        const size_t nt = size_t(std::max(S.n_tiles, 1));
        MULTI_HIP(S.tiles.ensure(nt * 2 * sizeof(int), g->dev[size_t(r)]));
        MULTI_HIP(S.packed.ensure(nt * area * 4 * sizeof(float), g->dev[size_t(r)]));
        MULTI_HIP(S.depth.ensure(nt * area * sizeof(float), g->dev[size_t(r)]));
        MULTI_HIP(S.counters.ensure(6 * sizeof(unsigned long long), g->dev[size_t(r)]));
        MULTI_HIP(S.state.ensure(nt * area * sizeof(rt_pass_state), g->dev[size_t(r)]));
        if (S.n_tiles)
            MULTI_HIP(hipMemcpy(S.tiles.p, lists[size_t(r)].data(), size_t(S.n_tiles) * 2 * sizeof(int),
                                hipMemcpyHostToDevice));
    }
    MULTI_HIP(hipSetDevice(g->dev[0]));
    const size_t total = order.size();
    MULTI_HIP(g->recv.ensure(total * area * 4 * sizeof(float), g->dev[0]));
    MULTI_HIP(g->recv_depth.ensure(total * area * sizeof(float), g->dev[0]));
    MULTI_HIP(g->recv_tiles.ensure(total * 2 * sizeof(int), g->dev[0]));
    MULTI_HIP(g->recv_ctr.ensure(size_t(g->n) * 6 * sizeof(unsigned long long), g->dev[0]));
    MULTI_HIP(hipMemcpy(g->recv_tiles.p, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
    g->W = W; g->H = H; g->T = T;
    return RT_OK;
}

// The one exchange step: every device's packed tiles (with `image`), depth (with d_depth) and counters to
// device 0 (device 0 sends to itself too, so one code path serves every group size), where one kernel
// unpacks the tiles into the W x H image and one adds the counters up.  An error inside the group still
// ends it, so later RCCL calls of this thread are not left inside an open group.
// adaptive: the packed image and depth are the adaptive frame's, and with d_count the counts travel too.
int gather(rt_group *g, const rt_params *p, int tile_size, bool image, float *d_rgba, float *d_depth,
           uint64_t *d_counters, hipStream_t s0, bool adaptive = false, uint32_t *d_count = nullptr) {
    auto stream_of = [&](int r) { return r == 0 ? s0 : g->st[size_t(r)]; };
    const size_t area = size_t(tile_size) * size_t(tile_size);
    MULTI_NCCL(ncclGroupStart());
    ncclResult_t nr = ncclSuccess;
    auto call = [&](ncclResult_t r_) { if (nr == ncclSuccess) nr = r_; };
    for (int r = 0; r < g->n && nr == ncclSuccess; r++) {
        auto &S = *g->share[size_t(r)];
        if (S.n_tiles && image) {
            call(ncclSend(adaptive ? S.a_packed.p : S.packed.p, size_t(S.n_tiles) * area * 4, ncclFloat32, 0,
                          g->comm[size_t(r)], stream_of(r)));
            if (d_depth)
                call(ncclSend(adaptive ? S.a_depth.p : S.depth.p, size_t(S.n_tiles) * area, ncclFloat32, 0,
                              g->comm[size_t(r)], stream_of(r)));
        }
        if (S.n_tiles && d_count)
            call(ncclSend(S.counts.p, size_t(S.n_tiles) * area, ncclUint32, 0, g->comm[size_t(r)], stream_of(r)));
        call(ncclSend(S.counters.p, 6, ncclUint64, 0, g->comm[size_t(r)], stream_of(r)));
    }
    for (int r = 0; r < g->n && nr == ncclSuccess; r++) {
        auto &S = *g->share[size_t(r)];
        const size_t o = g->off[size_t(r)];
        if (S.n_tiles && image) {
            call(ncclRecv(g->recv.as<float>() + o * area * 4, size_t(S.n_tiles) * area * 4, ncclFloat32, r, g->comm[0],
                          s0));
            if (d_depth)
                call(ncclRecv(g->recv_depth.as<float>() + o * area, size_t(S.n_tiles) * area, ncclFloat32, r,
                              g->comm[0], s0));
        }
        if (S.n_tiles && d_count)
            call(ncclRecv(g->recv_count.as<uint32_t>() + o * area, size_t(S.n_tiles) * area, ncclUint32, r, g->comm[0],
                          s0));
        call(ncclRecv(g->recv_ctr.as<unsigned long long>() + size_t(r) * 6, 6, ncclUint64, r, g->comm[0], s0));
    }
    const ncclResult_t ne = ncclGroupEnd();
    MULTI_NCCL(nr);
    MULTI_NCCL(ne);
    // device 0 assembles the frame
    MULTI_HIP(hipSetDevice(g->dev[0]));
    const uint32_t n_px = uint32_t(size_t(g->off[size_t(g->n)]) * area);
    if (n_px && image)
        hipLaunchKernelGGL(k_unpack_tiles, dim3((n_px + 255u) / 256u), dim3(256), 0, s0, g->recv.as<float4>(),
                           g->recv_depth.as<float>(), g->recv_tiles.as<int2>(), n_px, tile_size, p->width, p->height,
                           reinterpret_cast<float4 *>(d_rgba), d_depth);
    if (n_px && d_count)
        hipLaunchKernelGGL(k_unpack_counts, dim3((n_px + 255u) / 256u), dim3(256), 0, s0, g->recv_count.as<uint32_t>(),
                           g->recv_tiles.as<int2>(), n_px, tile_size, p->width, p->height, d_count);
    if (d_counters)
        hipLaunchKernelGGL(k_sum_counters, dim3(1), dim3(64), 0, s0, g->recv_ctr.as<unsigned long long>(), g->n,
                           reinterpret_cast<unsigned long long *>(d_counters));
    MULTI_HIP(hipGetLastError());
    return RT_OK;
}

// The adaptive frame's buffers of the current deal, the pinned counts and the events: allocated when the
// deal's first adaptive frame begins, kept while the deal stays.
int ensure_adaptive(rt_group *g) {
    if (!g->h_active) {
        MULTI_HIP(hipHostMalloc(reinterpret_cast<void **>(&g->h_active), size_t(g->n) * sizeof(uint32_t),
                                hipHostMallocPortable));  // every device of the group copies into it
        std::memset(g->h_active, 0, size_t(g->n) * sizeof(uint32_t));
    }
    const size_t area = size_t(g->T) * size_t(g->T);
    for (int r = 0; r < g->n; r++) {
        auto &S = *g->share[size_t(r)];
        const int d = g->dev[size_t(r)];
        MULTI_HIP(hipSetDevice(d));
        if (!S.counted) MULTI_HIP(hipEventCreateWithFlags(&S.counted, hipEventDisableTiming));
        const size_t slots = size_t(std::max(S.n_tiles, 1)) * area;
        MULTI_HIP(S.aux.ensure(slots * sizeof(rt_pass_aux), d));
        MULTI_HIP(S.slots.ensure(slots * sizeof(uint32_t), d));
        MULTI_HIP(S.n_active.ensure(sizeof(uint32_t), d));
        MULTI_HIP(S.counts.ensure(slots * sizeof(uint32_t), d));
        MULTI_HIP(S.a_packed.ensure(slots * 4 * sizeof(float), d));
        MULTI_HIP(S.a_depth.ensure(slots * sizeof(float), d));
    }
    MULTI_HIP(hipSetDevice(g->dev[0]));
    MULTI_HIP(g->recv_count.ensure(size_t(g->off[size_t(g->n)]) * area * sizeof(uint32_t), g->dev[0]));
    return RT_OK;
}

// every scene must live on its group device (its buffers are that device's; a scene of another
// device would launch there with this device's stream)
bool scenes_ok(const rt_group *g, rt_dev_scene *const *scenes) {
    for (int r = 0; r < g->n; r++)
        if (!scenes[r] || rtamd::scene_device(scenes[r]) != g->dev[size_t(r)]) return false;
    return true;
}

// The blocking group calls: the scene replicated on every device, a group for the call, n_img images (and
// depths, when asked) up to device 0 so that pixels nothing writes keep the caller's bytes, run(group,
// scenes, d_rgba, d_depth, d_ctr) timed on device 0's null stream, the images and the counters back.
template <class Run>
int inw_multi_blocking(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                       uint32_t n_lights, const rt_params *p, const int *devices, int n_dev, size_t n_img, float *rgba,
                       float *depth, rt_stats *st, Run &&run) {
    DeviceGuard guard;
    struct SceneDel { void operator()(rt_dev_scene *s) const { rt_dev_scene_free(s); } };
    struct GroupDel { void operator()(rt_group *g) const { rt_group_free(g); } };
    std::vector<std::unique_ptr<rt_dev_scene, SceneDel>> own;
    std::vector<rt_dev_scene *> scenes;
    for (int r = 0; r < n_dev; r++) {  // the scene replicated on every device (< 2 MB at C3)
        rt_dev_scene *s = rt_dev_scene_inw(geom, n, layout, nodes, lights, n_lights, p->spp, devices[r]);
        if (!s) return RT_E_NODEVICE;
        own.emplace_back(s);
        scenes.push_back(s);
    }
    std::unique_ptr<rt_group, GroupDel> g(rt_group_create(devices, n_dev));
    if (!g) return RT_E_NODEVICE;
    MULTI_HIP(hipSetDevice(devices[0]));
    const size_t npx = size_t(p->width) * size_t(p->height) * n_img;
    Buf d_rgba, d_depth, d_ctr;
    MULTI_HIP(d_rgba.ensure(npx * 16, devices[0]));
    MULTI_HIP(hipMemcpy(d_rgba.p, rgba, npx * 16, hipMemcpyHostToDevice));
    if (depth) {
        MULTI_HIP(d_depth.ensure(npx * 4, devices[0]));
        MULTI_HIP(hipMemcpy(d_depth.p, depth, npx * 4, hipMemcpyHostToDevice));
    }
    MULTI_HIP(d_ctr.ensure(6 * sizeof(unsigned long long), devices[0]));
    MULTI_HIP(hipMemset(d_ctr.p, 0, 6 * sizeof(unsigned long long)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    MULTI_HIP(hipEventCreate(&e0));
    MULTI_HIP(hipEventCreate(&e1));
    MULTI_HIP(hipEventRecord(e0, nullptr));
    int rc = run(g.get(), scenes.data(), d_rgba.as<float>(), depth ? d_depth.as<float>() : nullptr,
                 d_ctr.as<uint64_t>());
    (void)hipSetDevice(devices[0]);
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != RT_OK) return rc;
    MULTI_HIP(hipDeviceSynchronize());
    MULTI_HIP(hipMemcpy(rgba, d_rgba.p, npx * 16, hipMemcpyDeviceToHost));
    if (depth) MULTI_HIP(hipMemcpy(depth, d_depth.p, npx * 4, hipMemcpyDeviceToHost));
    if (st) {
        unsigned long long c[6];
        MULTI_HIP(hipMemcpy(c, d_ctr.p, sizeof(c), hipMemcpyDeviceToHost));
        st->segments = c[0]; st->node_visits = c[1]; st->prim_tests = c[2];
        st->shadow_queries = c[3]; st->stack_drops = c[4]; st->nan_drops = c[5];
        st->ms = ms;
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_tile_deal(int width, int height, int tile_size, int n_dev, int *order_out, int cap) {
    if (width <= 0 || height <= 0 || tile_size <= 0 || n_dev <= 0 || cap < 0 || (cap > 0 && !order_out))
        return RT_E_ARG;
    try {
        const std::vector<std::pair<int, int>> order = rtamd::tile_deal(width, height, tile_size, n_dev);
        for (size_t k = 0; k < order.size() && k < size_t(cap); k++) {
            order_out[2 * k] = order[k].first;
            order_out[2 * k + 1] = order[k].second;
        }
        return int(order.size());
    } catch (...) {
        return RT_E_ARG;
    }
}

rt_group *rt_group_create(const int *devices, int n_dev) {
    if (!devices || n_dev <= 0 || n_dev > 64) return nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return nullptr;
    for (int r = 0; r < n_dev; r++) {
        if (devices[r] < 0 || devices[r] >= count) return nullptr;
        for (int q = 0; q < r; q++)
            if (devices[q] == devices[r]) return nullptr;  // one rank per device (RCCL refuses duplicates)
        if (rt_device_info(devices[r], nullptr, 0, nullptr) != RT_OK) return nullptr;  // a gfx950 device
    }
    DeviceGuard guard;
    std::unique_ptr<rt_group> g(new (std::nothrow) rt_group());
    if (!g) return nullptr;
    try {
        g->n = n_dev;
        g->dev.assign(devices, devices + n_dev);
        g->comm.assign(size_t(n_dev), nullptr);
        g->st.assign(size_t(n_dev), nullptr);
        for (int r = 0; r < n_dev; r++) g->share.push_back(std::make_unique<rt_group::Share>());
    } catch (...) {
        return nullptr;
    }
    if (ncclCommInitAll(g->comm.data(), n_dev, g->dev.data()) != ncclSuccess) {
        g->comm.assign(size_t(n_dev), nullptr);
        return nullptr;
    }
    for (int r = 1; r < n_dev; r++) {
        if (hipSetDevice(devices[r]) != hipSuccess) return nullptr;
        if (hipStreamCreateWithFlags(&g->st[size_t(r)], hipStreamNonBlocking) != hipSuccess) return nullptr;
    }
    return g.release();
}

void rt_group_free(rt_group *g) {
    if (!g) return;
    DeviceGuard guard;
    for (int d : g->dev) {
        (void)hipSetDevice(d);
        (void)hipDeviceSynchronize();
    }
    delete g;
}

int rt_render_multi_async(rt_group *g, rt_dev_scene *const *scenes, const rt_camera *cam, const rt_params *p,
                          int tile_size, float *d_rgba, float *d_depth, uint64_t *d_counters, void *stream) {
    if (!g || !scenes || !cam || !p || !d_rgba || p->width <= 0 || p->height <= 0 || tile_size <= 0 ||
        tile_size % 16 != 0)
        return RT_E_ARG;
    if (!scenes_ok(g, scenes)) return RT_E_ARG;
    DeviceGuard guard;
    const hipStream_t s0 = static_cast<hipStream_t>(stream);
    if (int rc = set_deal(g, p->width, p->height, tile_size, s0); rc != RT_OK) {
        g->W = 0;  // rebuild the deal next time
        return rc;
    }
    auto stream_of = [&](int r) { return r == 0 ? s0 : g->st[size_t(r)]; };
    rt_params q = *p;
    q.tile_x0 = q.tile_y0 = q.tile_w = q.tile_h = 0;  // the whole frame
    // every device renders its share on its own stream
    for (int r = 0; r < g->n; r++) {
        auto &S = *g->share[size_t(r)];
        MULTI_HIP(hipSetDevice(g->dev[size_t(r)]));
        MULTI_HIP(hipMemsetAsync(S.counters.p, 0, 6 * sizeof(unsigned long long), stream_of(r)));
        if (S.n_tiles == 0) continue;
        const int rc = rt_render_tiles_async(scenes[r], cam, &q, S.tiles.as<int>(), S.n_tiles, tile_size,
                                             S.packed.as<float>(), d_depth ? S.depth.as<float>() : nullptr,
                                             S.counters.as<uint64_t>(), stream_of(r));
        if (rc != RT_OK) return rc;
    }
    return gather(g, p, tile_size, true, d_rgba, d_depth, d_counters, s0);
}

int rt_render_pass_multi_async(rt_group *g, rt_dev_scene *const *scenes, const rt_camera *cam, const rt_params *p,
                               int tile_size, uint32_t s0, uint32_t ns, float *d_rgba, float *d_depth,
                               uint64_t *d_counters, void *stream) {
    if (!g || !scenes || !cam || !p || p->width <= 0 || p->height <= 0 || p->spp < 1 || p->max_bounces < 0 ||
        tile_size <= 0 || tile_size % 16 != 0 || s0 >= uint32_t(p->spp))
        return RT_E_ARG;
    if (!scenes_ok(g, scenes)) return RT_E_ARG;
    // everything a device's pass could refuse is asked of every scene first, so that a refused call leaves
    // the deal, the states and their count as they were: argument errors of any scene before RT_E_UNSUPPORTED
    bool unsupported = p->show_normal != 0;
    for (int r = 0; r < g->n; r++) {
        const int rc = rtamd::scene_pass_check(scenes[r], p->spp);
        if (rc == RT_E_ARG) return RT_E_ARG;
        unsupported |= rc != RT_OK;
    }
    // the samples the states hold: none when this call changes the deal
    const uint32_t held = (g->W == p->width && g->H == p->height && g->T == tile_size) ? g->samples : 0u;
    if (s0 != 0 && s0 != held) return RT_E_ARG;
    if (unsupported) return RT_E_UNSUPPORTED;
    if (ns == 0) return RT_OK;
    DeviceGuard guard;
    const hipStream_t st0 = static_cast<hipStream_t>(stream);
    if (int rc = set_deal(g, p->width, p->height, tile_size, st0); rc != RT_OK) {
        g->W = 0;  // rebuild the deal next time
        return rc;
    }
    auto stream_of = [&](int r) { return r == 0 ? st0 : g->st[size_t(r)]; };
    const bool image = d_rgba != nullptr, want_depth = image && d_depth != nullptr;
    g->samples = 0;  // until every device has taken the pass: a failed one leaves states of no count
    g->adaptive = false;  // and no adaptive round continues them
    // every device continues the states of its share on its own stream
    for (int r = 0; r < g->n; r++) {
        auto &S = *g->share[size_t(r)];
        MULTI_HIP(hipSetDevice(g->dev[size_t(r)]));
        MULTI_HIP(hipMemsetAsync(S.counters.p, 0, 6 * sizeof(unsigned long long), stream_of(r)));
        if (S.n_tiles == 0) continue;
        const int rc = rt_render_pass_tiles_async(scenes[r], cam, p, S.tiles.as<int>(), S.n_tiles, tile_size, s0, ns,
                                                  S.state.as<rt_pass_state>(), image ? S.packed.as<float>() : nullptr,
                                                  want_depth ? S.depth.as<float>() : nullptr,
                                                  S.counters.as<uint64_t>(), stream_of(r));
        if (rc != RT_OK) return rc;
    }
    const int rc = gather(g, p, tile_size, image, d_rgba, want_depth ? d_depth : nullptr, d_counters, st0);
    if (rc == RT_OK) g->samples = uint32_t(std::min<uint64_t>(uint64_t(s0) + ns, uint64_t(p->spp)));
    return rc;
}

int rt_render_adaptive_multi_async(rt_group *g, rt_dev_scene *const *scenes, const rt_camera *cam, const rt_params *p,
                                   int tile_size, int first, uint32_t ns, float tol, uint32_t min_samples,
                                   float *d_rgba, float *d_depth, uint32_t *d_count, uint64_t *d_counters,
                                   void *stream) {
    if (!g || !scenes || !cam || !p || p->width <= 0 || p->height <= 0 || p->spp < 1 || p->max_bounces < 0 ||
        tile_size <= 0 || tile_size % 16 != 0)
        return RT_E_ARG;
    if (!scenes_ok(g, scenes)) return RT_E_ARG;
    // as in rt_render_pass_multi_async, every scene is asked before the group is touched
    bool unsupported = p->show_normal != 0;
    for (int r = 0; r < g->n; r++) {
        const int rc = rtamd::scene_pass_check(scenes[r], p->spp);
        if (rc == RT_E_ARG) return RT_E_ARG;
        unsupported |= rc != RT_OK;
    }
    // a round continues the adaptive frame of this deal, which no pass has touched since
    if (!first && !(g->adaptive && g->W == p->width && g->H == p->height && g->T == tile_size)) return RT_E_ARG;
    if (unsupported) return RT_E_UNSUPPORTED;
    if (ns == 0) return RT_OK;
    DeviceGuard guard;
    const hipStream_t st0 = static_cast<hipStream_t>(stream);
    if (int rc = set_deal(g, p->width, p->height, tile_size, st0); rc != RT_OK) {
        g->W = 0;  // rebuild the deal next time
        return rc;
    }
    auto stream_of = [&](int r) { return r == 0 ? st0 : g->st[size_t(r)]; };
    const bool image = d_rgba != nullptr, want_depth = image && d_depth != nullptr;
    g->samples = 0;  // the states are an adaptive frame's: no progressive pass continues into them
    g->adaptive = false;  // until every device has taken the round
    if (first)
        if (int rc = ensure_adaptive(g); rc != RT_OK) return rc;
    const size_t area = size_t(tile_size) * size_t(tile_size);
    for (int r = 0; r < g->n; r++) {
        auto &S = *g->share[size_t(r)];
        const hipStream_t sr = stream_of(r);
        MULTI_HIP(hipSetDevice(g->dev[size_t(r)]));
        MULTI_HIP(hipMemsetAsync(S.counters.p, 0, 6 * sizeof(unsigned long long), sr));
        if (S.n_tiles == 0) continue;
        const size_t slots = size_t(S.n_tiles) * area;
        rt_pass_state *state = S.state.as<rt_pass_state>();
        rt_pass_aux *aux = S.aux.as<rt_pass_aux>();
        uint32_t n_list = 0;
        if (first) {  // no samples anywhere, every slot inside the image listed (a select that finds all active)
            MULTI_HIP(hipMemsetAsync(S.aux.p, 0, slots * sizeof(rt_pass_aux), sr));
            MULTI_HIP(hipMemsetAsync(S.a_packed.p, 0, slots * 4 * sizeof(float), sr));
            MULTI_HIP(hipMemsetAsync(S.a_depth.p, 0, slots * sizeof(float), sr));
            const int rc = rt_pass_select_tiles_async(scenes[r], p, S.tiles.as<int>(), S.n_tiles, tile_size, state, aux,
                                                      -1.0f, 0, S.slots.as<uint32_t>(), S.n_active.as<uint32_t>(),
                                                      nullptr, sr);
            if (rc != RT_OK) return rc;
            n_list = S.n_inside;
        } else {  // the one wait: the previous round's count sizes this round's launches
            MULTI_HIP(hipEventSynchronize(S.counted));
            n_list = g->h_active[r];
        }
        if (n_list != 0) {
            int rc = rt_render_pass_slots_async(scenes[r], cam, p, S.tiles.as<int>(), S.n_tiles, tile_size,
                                                S.slots.as<uint32_t>(), n_list, ns, state, aux, S.a_packed.as<float>(),
                                                S.a_depth.as<float>(), S.counters.as<uint64_t>(), sr);
            if (rc != RT_OK) return rc;
            rc = rt_pass_select_tiles_async(scenes[r], p, S.tiles.as<int>(), S.n_tiles, tile_size, state, aux, tol,
                                            min_samples, S.slots.as<uint32_t>(), S.n_active.as<uint32_t>(), nullptr, sr);
            if (rc != RT_OK) return rc;
        }
        MULTI_HIP(hipMemcpyAsync(g->h_active + r, S.n_active.p, sizeof(uint32_t), hipMemcpyDeviceToHost, sr));
        MULTI_HIP(hipEventRecord(S.counted, sr));
        if (d_count)
            hipLaunchKernelGGL(k_aux_counts, dim3(uint32_t((slots + 255) / 256)), dim3(256), 0, sr, S.aux.as<uint4>(),
                               uint32_t(slots), S.counts.as<uint32_t>());
    }
    const int rc = gather(g, p, tile_size, image, d_rgba, want_depth ? d_depth : nullptr, d_counters, st0, true, d_count);
    if (rc == RT_OK) g->adaptive = true;
    return rc;
}

int rt_group_adaptive_active(rt_group *g, uint32_t *n_active) {
    if (!g || !n_active || !g->adaptive) return RT_E_ARG;
    DeviceGuard guard;
    uint64_t sum = 0;
    for (int r = 0; r < g->n; r++) {
        auto &S = *g->share[size_t(r)];
        if (S.n_tiles == 0) continue;
        MULTI_HIP(hipSetDevice(g->dev[size_t(r)]));
        MULTI_HIP(hipEventSynchronize(S.counted));
        sum += g->h_active[r];
    }
    *n_active = uint32_t(std::min<uint64_t>(sum, 0xffffffffu));
    return RT_OK;
}

int rt_render_inw_multi(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                        uint32_t n_lights, const rt_camera *cam, const rt_params *p, const int *devices, int n_dev,
                        int tile_size, float *rgba, float *depth, rt_stats *st) {
    if (!geom || !nodes || n == 0 || !cam || !p || p->width <= 0 || p->height <= 0 || p->spp < 1 || !rgba ||
        !devices || n_dev <= 0 || (layout != 1 && layout != 4))
        return RT_E_ARG;
    return inw_multi_blocking(geom, n, layout, nodes, lights, n_lights, p, devices, n_dev, 1, rgba, depth, st,
        [&](rt_group *g, rt_dev_scene *const *scenes, float *d_rgba, float *d_depth, uint64_t *d_ctr) {
            return rt_render_multi_async(g, scenes, cam, p, tile_size, d_rgba, d_depth, d_ctr, nullptr);
        });
}

int rt_render_passes_inw_multi(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                               uint32_t n_lights, const rt_camera *cam, const rt_params *p, const int *devices,
                               int n_dev, int tile_size, const uint32_t *cuts, int n_cuts, float *rgba, float *depth,
                               rt_stats *st) {
    if (!geom || !nodes || n == 0 || !cam || !p || p->width <= 0 || p->height <= 0 || p->spp < 1 || !rgba ||
        !devices || n_dev <= 0 || (layout != 1 && layout != 4) || tile_size <= 0 || tile_size % 16 != 0)
        return RT_E_ARG;
    if (layout == 4 && n_lights > 0 && !lights) return RT_E_ARG;
    // rt_render_passes_inw's rule: strictly increasing from cuts[0] > 0 to at most spp
    if (!cuts || n_cuts < 1 || cuts[0] == 0 || cuts[n_cuts - 1] > uint32_t(p->spp)) return RT_E_ARG;
    for (int i = 1; i < n_cuts; i++)
        if (cuts[i] <= cuts[i - 1]) return RT_E_ARG;
    if (p->show_normal) return RT_E_UNSUPPORTED;
    const size_t npx = size_t(p->width) * size_t(p->height);
    return inw_multi_blocking(geom, n, layout, nodes, lights, n_lights, p, devices, n_dev, size_t(n_cuts), rgba, depth, st,
        [&](rt_group *g, rt_dev_scene *const *scenes, float *d_rgba, float *d_depth, uint64_t *d_ctr) {
            uint32_t s0 = 0;
            for (int i = 0; i < n_cuts; i++) {  // pass i into image i
                const int rc = rt_render_pass_multi_async(g, scenes, cam, p, tile_size, s0, cuts[i] - s0,
                                                          d_rgba + size_t(i) * npx * 4,
                                                          d_depth ? d_depth + size_t(i) * npx : nullptr, d_ctr, nullptr);
                if (rc != RT_OK) return rc;
                s0 = cuts[i];
            }
            return int(RT_OK);
        });
}

int rt_render_adaptive_inw_multi(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                                 uint32_t n_lights, const rt_camera *cam, const rt_params *p, const int *devices,
                                 int n_dev, int tile_size, uint32_t batch, float tol, uint32_t min_samples,
                                 uint32_t max_rounds, float *rgba, float *depth, uint32_t *count, uint32_t *rounds_out,
                                 rt_stats *st) {
    if (!geom || !nodes || n == 0 || !cam || !p || p->width <= 0 || p->height <= 0 || p->spp < 1 ||
        p->max_bounces < 0 || !rgba || !devices || n_dev <= 0 || (layout != 1 && layout != 4) || tile_size <= 0 ||
        tile_size % 16 != 0 || batch == 0)
        return RT_E_ARG;
    if (layout == 4 && n_lights > 0 && !lights) return RT_E_ARG;
    if (p->show_normal) return RT_E_UNSUPPORTED;
    if (st) std::memset(st, 0, sizeof(*st));
    if (rounds_out) *rounds_out = 0;
    const size_t npx = size_t(p->width) * size_t(p->height);
    return inw_multi_blocking(geom, n, layout, nodes, lights, n_lights, p, devices, n_dev, 1, rgba, depth, st,
        [&](rt_group *g, rt_dev_scene *const *scenes, float *d_rgba, float *d_depth, uint64_t *d_ctr) -> int {
            Buf d_count;  // on device 0, the current device here
            if (count) {
                MULTI_HIP(d_count.ensure(npx * sizeof(uint32_t), devices[0]));
                MULTI_HIP(hipMemcpy(d_count.p, count, npx * sizeof(uint32_t), hipMemcpyHostToDevice));
            }
            // rt_render_adaptive_inw's loop: every pixel listed, then rounds while pixels are active and rounds remain
            uint32_t n_active = 1, rounds = 0;
            while (n_active > 0 && (max_rounds == 0 || rounds < max_rounds)) {
                int rc = rt_render_adaptive_multi_async(g, scenes, cam, p, tile_size, rounds == 0, batch, tol, min_samples,
                                                        d_rgba, d_depth, d_count.as<uint32_t>(), d_ctr, nullptr);
                if (rc == RT_OK) rc = rt_group_adaptive_active(g, &n_active);
                if (rc != RT_OK) return rc;
                rounds++;
            }
            if (count) {
                MULTI_HIP(hipSetDevice(devices[0]));
                MULTI_HIP(hipStreamSynchronize(nullptr));
                MULTI_HIP(hipMemcpy(count, d_count.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost));
            }
            if (rounds_out) *rounds_out = rounds;
            return RT_OK;
        });
}

}  // extern "C"
