/*
 * rt_hip.h -- C ABI of the MI355X-native render path (librt_hip.so).
 *
 * This is the drop-in boundary for the reference's per-pixel render loop.  In the
 * reference the boundary is the OpenGL compute-dispatch contract: sampler units 0/1
 * bound to the geometry / LBVH "buffer textures", a set of uniforms, an optional light
 * SSBO, then glDispatchCompute.  Each entry point below replaces one such dispatch
 * (file:line citations are relative to /root/reference/Raytracing-Sandbox/Src/):
 *
 *   rt_render_iow01  <- In_One_Weekend::Sphere::OnUpdate             01_Adding_Sphere/Sphere.cpp:51-64
 *                       (uniforms Sphere.cpp:54-61, dispatch (W,H,1) Sphere.cpp:63)
 *   rt_render_iow03  <- In_One_Weekend::Adding_Materials::OnUpdate   03_Shadows_and_Materials/materials.cpp:118-146
 *                       (uniforms :121-135, textures :137-140, per-tile dispatch :142-143)
 *   rt_render_inw    <- In_Next_Week::RT_Base<>::OnUpdateBase        In-Next-Week/base.h:148-173
 *                       (layout 1 = BVH stage, 01_BoundingVolumeHierarchy/BVH.cpp:26-43;
 *                        layout 4 = Lights stage + SSBO, 04_Lights_Camera_And_Action/lights.cpp:15-37)
 *   rt_lbvh_build    <- LBVH::ConstructLBVH_Buff                      In-Next-Week/LBVH/lbvh.h:215-269
 *                       (called from base.h:135 on every redraw)
 *
 * Conventions:
 *   - POD structs, caller-owned host memory, library-owned device memory.
 *   - int status: 0 = ok, negative = error (RT_E_*); no exceptions cross the ABI.
 *   - Output images are row-major, row y = pixel_coords.y (GL bottom row first),
 *     RGBA float32 with alpha = 1, exactly the reference's rgba32f image memory.
 *     The depth image (INW only) is one float per pixel (the reference's r32f image).
 *   - The *_async variants take DEVICE pointers (inputs already resident in HBM) and a
 *     hipStream_t passed as void*; they never allocate or synchronise (graph-capturable).
 *   - Threading: calls are reentrant per distinct output buffer.
 *
 * Numerics contract shared with the CPU oracle (DESIGN.md "Numerics contract"):
 * IEEE binary32, GLSL evaluation order, no FMA contraction, GLSL a/b == a*RN(1/b),
 * correctly rounded sqrt and reciprocal, transcendentals only in host-built double
 * precision tables.  Under this contract the GPU image is bit-identical to the oracle's.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 5

/* status codes */
#define RT_OK            0
#define RT_E_ARG        -1   /* bad argument (null pointer, non-positive size, bad layout) */
#define RT_E_HIP        -2   /* a HIP runtime call failed */
#define RT_E_NODEVICE   -3   /* no usable gfx950 device */
#define RT_E_UNSUPPORTED -4  /* a feature the call cannot serve (e.g. TextureIndex > 0 with no texture bound) */

/* Camera uniforms.
 *   IOW-01: u_CameraPosn, u_CameraDirn, u_FocusDist            (01_Adding_Sphere/computeShaderSrc.glsl:5-7)
 *   IOW-03: u_CameraPosn, u_CameraDirn, u_FOV_y, u_CamAperture, u_CamFocusDist (03...glsl:7-13)
 *   INW   : u_Camera{Position, Direction, FOV_y, FocusDist[0], Aperture} (01_BoundingVolumeHierarchy/computeShaderSrc.glsl:221-228)
 * dir is passed exactly as the reference host computes it (IOW: normalized FrontFromPitchYaw,
 * materials.cpp:321-328; INW: RT_Base::m_Camera.Front(), NOT normalized, base.h:274-281). */
typedef struct rt_camera {
    float pos[3];
    float dir[3];
    float fov_y_rad;
    float aperture;
    float focus_dist;
} rt_camera;

/* Render parameters.
 *   width, height : full image size (imageSize(img_output))
 *   spp           : IOW-03 u_NumOfSamples; INW local_size_x (samples per pixel, any value >= 1)
 *   max_bounces   : IOW-03 u_NumOfBounce; INW u_NumOfBounces
 *   tile_*        : rectangle of pixels to render (IOW-03 u_TileIndex*u_TileSize and the
 *                   per-tile dispatch size, materials.cpp:126-143).  tile_w/tile_h <= 0 => full image.
 *   show_normal   : IOW-01/IOW-03 u_ShowNormal
 *   device        : HIP device ordinal for the blocking entry points (-1 = current) */
typedef struct rt_params {
    int width, height, spp, max_bounces;
    int tile_x0, tile_y0, tile_w, tile_h;
    int show_normal;
    int device;
} rt_params;

/* Counters, identical definitions in the kernels and in the oracle (DESIGN.md "Counters"). */
typedef struct rt_stats {
    uint64_t segments;        /* rays cast (primary + secondary), i.e. closest-hit queries   */
    uint64_t node_visits;     /* LBVH nodes fetched+tested (closest-hit, shadow, RI walks)   */
    uint64_t prim_tests;      /* primitive tests (IOW linear loop, INW leaves, RI inside)    */
    uint64_t shadow_queries;  /* INW-04 shadow rays                                          */
    uint64_t stack_drops;     /* pushes silently dropped by a full stack                     */
    uint64_t nan_drops;       /* secondary directions that came out NaN                      */
    double   ms;              /* device time of the render launch(es), milliseconds          */
} rt_stats;

/* ---- options ------------------------------------------------------------------------
 * The strategy switches of the render path.  Every strategy is exact: the image, the depth
 * and the ray-level counters are bit-identical whatever the options (tests/test_gpu_bvh_exact.py);
 * only speed and the build's own node / primitive counts change.  The defaults (rt_options_default)
 * are the measured-best settings; nothing else (no environment variable) changes what the
 * library runs.  rt_options_set sets the library-wide options; a device scene copies them when
 * it is created (rt_dev_scene_*) and rt_dev_scene_set_options replaces its copy.  The blocking
 * entry points build a scene per call, so they use the options current at the call.
 * Options marked [build] shape the scene's device structures and are read at scene creation only. */
typedef struct rt_options {
    uint32_t size;          /* sizeof(rt_options), set by rt_options_default; checked by the setters */
    /* INW (In-Next-Week 01 / 04) */
    int inw_wide_walk;      /* [build] 1: 4-wide culling walk with the reference's leaf tests; 0: the LBVH walk as the shader does it
                             * (also taken, per scene, when an object sticks out of its caller-supplied leaf box: DESIGN.md §2) */
    int inw_order;          /* fold kernel: 0 = the probe picks, 1 = pixel-major, 2 = sample-major, -1 = per-pixel k_inw */
    int inw_beams;          /* per-pixel candidate lists for primary rays (pixel-major frames); 1: entries of
                               32 bits (16-bit object id, entry t rounded down) when ids fit, 2: (id, t) pairs */
    int inw_ri_grid;        /* surrounding-RI queries through the uniform grid */
    int inw_lds_nodes;      /* top of the wide BVH staged in LDS (768-lane blocks) */
    int inw_fused_cull;     /* one fma per culling plane where the error bound holds */
    int inw_claim_order;    /* pixel-major claims costliest 8x8 blocks first */
    int inw_ring_pm;        /* pixel-major fold ring: 0 (default) in LDS, 256 entries per wave, the walks
                               reading every node from L1 / L2; else a global ring of that many entries
                               per wave (power of two >= 64) beside 236 staged nodes */
    int inw_ring_sm;        /* sample-major fold ring: 0 (default) in LDS, 256 entries per wave, when the
                               scene's BVH top fits the 5 nodes staged beside it (nothing lost), else a
                               global ring of 256; else a global ring of that many entries per wave */
    int inw_stackless;      /* the reference's LBVH walks (closest hit, surrounding RI) without their stack, by
                               the node buffer's parent links, wherever no push could drop; their top
                               nodes staged in LDS when there is no wide walk (DESIGN.md "Stackless") */
    int inw_device_build;   /* rt_dev_scene_inw_update with the LBVH built on the device: the wide walk's
                               4-wide BVH (binned SAH), ranks and RI grid built on the device too (0: on
                               the host from the read-back LBVH, as rt_dev_scene_inw does) */
    int inw_claim_xcd;      /* pixel-major claims from 8 queues, one per XCD (an 8x8 block's pixels are
                               written by one XCD's L2, whole lines), idle XCDs taking from the others */
    int inw_qnodes;         /* 1: pixel-major INW-01 frames with the fused cull run k_inw_pm's GQ instance
                               (DESIGN.md §5.1): the reference's 40-float stacks in global memory with the
                               top ray in registers, the wide walk's node stack and the top of the culling
                               BVH in LDS (quantised 64-B nodes, 1,168 of them); 0 (default, measured faster):
                               the FStack instance */
    int inw_time_bins;      /* moving objects: the wide walk culls with one of this many extra culling trees,
                               each over the boxes the objects sweep in its share of the shutter interval
                               (the ray's time ratio picks it; DESIGN.md §5.2 "Time-binned culling trees");
                               0 or 1: the swept tree only.  Default 2 (4 and 8 measured slower: their trees crowd
                               the L2); scenes built on the host */
    int inw_walk_bins;      /* 1 (default): the wide closest-hit walks use the time-bin trees */
    int inw_beam_bins;      /* 1 (default): a pixel's beam lists per time bin, from the time-bin trees */
    int inw_sphere_records; /* 1 (default): in scenes of equal-scale ellipsoids with the identity rotation, the
                               wide walk, beam lists and RI grid read 3-float4 sphere records */
    int inw_compact_nodes;  /* 1 (default): the wide walk reads its nodes from global memory as 7 float4
                               (112 B) instead of 10 (the repeated low planes dropped) */
    /* IOW-03 (In-One-Weekend 03) */
    int iow_spec;           /* sample-parallel speculation (0: the sequential per-pixel kernel) */
    int iow_linear;         /* [build] the shader's linear object loop instead of the culling BVH */
    int iow_narrow;         /* byte bounce counts / 12-deep BVH stack variant (u_NumOfBounce <= 255) */
    int iow_lds_bvh;        /* culling BVH staged in LDS when it fits */
    int iow_leaf_batch;     /* test postponed leaves once this many lanes hold one (1..65) */
    int iow_coop_max;       /* wave-cooperative closest hits when at most this many lanes trace (0 = off) */
    int iow_chunks_lpt;     /* sequential kernel: a short first sample chunk, then longest-first */
    int rounds_seq;         /* tail-compaction rounds per pass, sequential kernels (0..14) */
    int rounds_spec;        /* ... sample-parallel passes (0..14) */
    int park_min;           /* park lanes only while at least this many units remain (-1: resident lanes / 8) */
    int spec_iters;         /* resolve + re-run passes */
    int spec_probe;         /* heavy-first: every spec_probe-th pixel probes all sample indices */
    int spec_heavy;         /* heavy-first: costliest sample indices run first (-1: (spp - 1) / 20,
                               (spp - 1) / 10 for a render of at most half the frame) */
    int spec_rounds;        /* checkpoint rounds of the speculative pass (0 = one launch) */
    int spec_tail_rounds;   /* budgeted tail rounds */
    int spec_tail_budget;   /* segments per unit and budgeted tail round */
    int spec_scan;          /* anchored scan past the frontier, samples (0 = off) */
    int spec_chain;         /* exact restarts follow their pixel's chain */
    int spec_alt;           /* alternative runs for long samples that read one stale entry */
    int spec_alt_cap;       /* alternative-run records */
    int spec_alt_seg;       /* segments that make a sample long enough for alternatives (0: 16384,
                               2048 for a render of at most half the frame) */
    int spec_alt_every;     /* also spawn alternatives after every k-th budgeted tail round (0 = once) */
    int spec_spread;        /* the last round of a pass gives long samples a wave each */
    int spec_prior_from;    /* first sample whose stale entries are guessed as the scene's RI prior */
    int spec_sort;          /* run the first re-execution list longest first */
    int spec_solo;          /* re-run pass: the longest samples take a wave each, up to this many */
    int spec_validate;      /* the sequential leftover pass reuses still-exact records */
    double spec_max_gb;     /* device memory cap of the speculation records, GB */
    int inw_sky_blocks;     /* INW-01, 1 (default): pixel-major frames render the 8x8 blocks whose pixels have empty,
                               complete beam lists (no primary ray can reach an object) in the lean kernel
                               k_inw_sky, outside k_inw_pm's claims (DESIGN.md §5.1 "Sky blocks") */
    int inw_beam_prune;     /* what the beam lists leave out (DESIGN.md §5.2 "Pixel beams"): 0 nothing (every leaf
                               whose box, inflated by the beam's largest radius, the central ray crosses);
                               1: leaves whose box the central ray misses once it is inflated by the beam's
                               radius over the box's own depth interval; 2 (default): also, in scenes with
                               sphere records, spheres whose swept centre stays farther from the central
                               line than their radius plus the beam's */
} rt_options;
void rt_options_default(rt_options *o);
int  rt_options_set(const rt_options *o);   /* RT_E_ARG: null, wrong size or a value out of range */
int  rt_options_get(rt_options *o);

/* ---- version / device ------------------------------------------------------------ */
int  rt_abi_version(void);
/* Returns RT_OK if a gfx950 device is visible; writes its name (<=255 chars). */
int  rt_device_info(int device, char *name_out, int name_cap, int *cu_count);

/* ---- blocking entry points (host buffers in, host buffers out) -------------------- */
int rt_render_iow01(const rt_camera *cam, const float sphere[4] /* centre xyz, radius */,
                    const rt_params *p, float *rgba /* W*H*4 */, rt_stats *st);

/* IOW-00: the base stage's default compute shader (In-One-Weekend/base.cpp:7-28, dispatched
 * W x H by 00_Image/image.cpp:46-53): rgba = (x/(W-1), y/(H-1), 0.25, 1). */
int rt_render_iow00(const rt_params *p, float *rgba /* W*H*4 */);

/* IOW-02 groups stage (02_Groups/computeShaderSrc.glsl; host groups.cpp:56-84, CopyObjBuffer
 * :250-285): records N x 18 = position, inverse rotation (glm column-major), scale, colour
 * (groups.h:11-17 GeometryBuff; the first 18 floats of an IOW-03 record), types 1 = CUBOID,
 * 2 = ELLIPSOID; u_Cull_Front / u_Cull_Back; u_NumOfBounce = p->max_bounces, u_FocusDist =
 * cam->focus_dist.  st->segments = bounce iterations (closest-hit queries). */
int rt_render_iow02(const float *types, const float *records /* N*18 */, uint32_t n, const rt_camera *cam,
                    const rt_params *p, int cull_front, int cull_back, float *rgba, rt_stats *st);

int rt_render_iow03(const float *types /* N, float(Geom_type) */,
                    const float *records /* N*24, materials.h:11-19 */, uint32_t n,
                    const rt_camera *cam, const rt_params *p, float *rgba, rt_stats *st);

int rt_render_inw(const float *geom /* N*28, layout 1 (BVH.h:12-19) or 4 (lights.h:15-21) */,
                  uint32_t n, int layout,
                  const float *nodes /* (2N-1)*8, BFS, lbvh.h:48-54 */,
                  const float *lights /* L*7: BBmin[3] BBmax[3] uint idx (bit-cast), lights.h:187-192 */,
                  uint32_t n_lights,
                  const rt_camera *cam, const rt_params *p,
                  float *rgba /* W*H*4 */, float *depth /* W*H, may be NULL */, rt_stats *st);

/* INW-01 (layout 1) with the shader's "#if MULTIFOCUS" branch compiled in
 * (01_BoundingVolumeHierarchy/computeShaderSrc.glsl:388-404, 424-428, 479-481, 505-549; the
 * reference never defines MULTIFOCUS): u_Camera.FocusDist[0..n_focus-1] = focus, 1..9 values
 * (u_NumOfFocusDist, In-Next-Week/base.h:458-473).  cam->focus_dist is not used. */
int rt_render_inw_mf(const float *geom /* N*28, layout 1 */, uint32_t n, const float *nodes, const rt_camera *cam,
                     const float *focus, int n_focus, const rt_params *p, float *rgba, float *depth, rt_stats *st);

/* ---- textures --------------------------------------------------------
 * INW-04 material textures, u_MaterialTextures[u_NumOfTexture2D]
 * (04_Lights_Camera_And_Action/computeShaderSrc.glsl:10, bound from slot 2 by
 * GeometryData_04::BindExtraData, lights.cpp:18-22).  texels: row 0 first (the GL upload
 * order; stbi flips on load, utility.cpp:217), channels 3 (GL_RGB8) or 4 (GL_RGBA8),
 * tightly packed.  An object with TextureIndex k in 1..n_tex multiplies its colour by the
 * nearest texel (GL_NEAREST, GL_REPEAT: a compute shader samples level 0 with the
 * magnification filter, utility.cpp:182-193) of its cube-projected object-space hit point
 * (04...glsl:416-464); TextureIndex > n_tex leaves the colour as is. */
typedef struct rt_texture {
    const uint8_t *texels;
    int width, height, channels;
} rt_texture;

int rt_render_inw_tex(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                      uint32_t n_lights, const rt_texture *tex, int n_tex, const rt_camera *cam,
                      const rt_params *p, float *rgba, float *depth, rt_stats *st);

/* Noise textures <- Helper::Noise::MakeTexture<glm::vec3>  Utilities/utility.h:69-192
 * (Snoise2 / Fbm2 / Turbulance, Utilities/utility.cpp:609-769; the stage UI calls it with
 * 600 x 100, gradient {0, 1}, lights.cpp:206).  rgb_out: width*height*3 bytes (GL_RGB8 texels,
 * row 0 first).  gradient: n_grad rgb triples (a list shorter than 2 gets black in front,
 * then white at the end, as MakeTexture does).  width must be one the reference's four
 * column batches tile exactly (600 is; others index out of bounds there): RT_E_ARG
 * otherwise, and for a constant noise field (the reference divides by zero). */
#define RT_NOISE_SIMPLEX    0
#define RT_NOISE_FBM        1
#define RT_NOISE_TURBULENCE 2
int rt_noise_texture(int width, int height, int type, const float *gradient, int n_grad, float freq, float lac,
                     float gain, int octaves, uint8_t *rgb_out, int device, double *ms);
size_t rt_noise_workspace_bytes(int width, int height);
/* Device pointers, never synchronises.  A constant noise field writes zeros and sets the
 * third uint32 of d_ws to 1. */
int rt_noise_texture_async(int width, int height, int type, const float *gradient, int n_grad, float freq,
                           float lac, float gain, int octaves, uint8_t *d_rgb_out, void *d_ws, size_t ws_bytes,
                           void *stream);

/* Re-projection <- TEXTURE_2D::LoadFromDiskToGPU(location, loadAs, mapTo)
 * Utilities/utility.cpp:266-463 (MercatorToCubic / CubicToMercator); load_as == map_to copies.
 * Where the reference is undefined: the output starts zeroed, the later loop position wins a
 * texel two positions store to, a load past the last texel reads the last texel. */
#define RT_MAP_MERCATOR 0
#define RT_MAP_CUBIC    1
int rt_texture_remap(const uint8_t *in, int width, int height, int channels, int load_as, int map_to,
                     uint8_t *out, int device, double *ms);
size_t rt_remap_workspace_bytes(int width, int height);
int rt_texture_remap_async(const uint8_t *d_in, int width, int height, int channels, int load_as, int map_to,
                           uint8_t *d_out, void *d_ws, size_t ws_bytes, void *stream);

/* LBVH builder: aabbs = N*(min xyz, max xyz) in geometry order -> (2N-1)*8 floats. */
int rt_lbvh_build(const float *aabbs, uint32_t n, float *nodes_out);

/* The same LBVH built on the GPU, node-for-node identical to rt_lbvh_build:
 * Morton keys + radix sort, the level merge as a Cartesian tree over the highest differing
 * bits, bottom-up boxes, breadth-first numbering.  Device pointers; d_ws holds
 * rt_lbvh_workspace_bytes(n) of scratch; never synchronises.  N <= 2^24 (ids are floats). */
size_t rt_lbvh_workspace_bytes(uint32_t n);
int rt_lbvh_build_async(const float *d_aabbs, uint32_t n, float *d_nodes_out, void *d_ws, size_t ws_bytes,
                        void *stream);
/* Blocking convenience wrapper (host buffers); *ms (may be NULL) receives the device time. */
int rt_lbvh_build_gpu(const float *aabbs, uint32_t n, float *nodes_out, int device, double *ms);

/* Host-side builds of a device scene's acceleration structures, without a device (what
 * rt_dev_scene_inw / rt_dev_scene_iow03 build on the host and upload):
 *   INW: the wide walk's 4-wide culling BVH over the LBVH leaf boxes, the depth-first ranks and
 *        leaf boxes, and the surrounding-RI grid; info = {wide nodes, dfs_high, wide depth,
 *        RI grid built, RI cells, RI ids, 0, 0} (all 0 when the wide walk does not apply);
 *   IOW-03: the culling BVH over the records; info = {wide nodes (0: linear loop), 0, 0, 0}.
 * info may be NULL; *ms (may be NULL) receives the host time. */
int rt_inw_host_build(const float *nodes /* (2N-1)*8 */, uint32_t n, uint32_t info[8], double *ms);
int rt_iow_host_build(const float *types, const float *records /* N*24 */, uint32_t n, uint32_t info[4], double *ms);

/* ---- asynchronous device entry points (bench / multi-GPU path) ---------------------
 * A prepared scene owns its device buffers (scene records, LBVH nodes, sample tables).
 * rt_scene_dev_* return an opaque handle; render calls enqueue on `stream`.
 * Counters are accumulated atomically into d_counters (6 x uint64, device memory). */
typedef struct rt_dev_scene rt_dev_scene;

rt_dev_scene *rt_dev_scene_iow03(const float *types, const float *records, uint32_t n,
                                 int spp, int device);
rt_dev_scene *rt_dev_scene_inw(const float *geom, uint32_t n, int layout, const float *nodes,
                               const float *lights, uint32_t n_lights, int spp, int device);
/* The same with material textures bound (see rt_texture); copied to the device. */
rt_dev_scene *rt_dev_scene_inw_tex(const float *geom, uint32_t n, int layout, const float *nodes,
                                   const float *lights, uint32_t n_lights, const rt_texture *tex, int n_tex,
                                   int spp, int device);
void rt_dev_scene_free(rt_dev_scene *s);
/* The next frame's geometry for an INW scene: RT_Base<>::OnUpdateBase's per-redraw work
 * (In-Next-Week/base.h:96-175: FillBuffer, LBVH::ConstructLBVH_Buff at :135-142, the texture
 * uploads) on the scene's existing device buffers.  geom: N*28 records of the scene's layout;
 * nodes: the caller's LBVH ((2N-1)*8), or NULL to build it on the device from aabbs (N*6, the
 * swept boxes rt_pack_inw writes) with rt_lbvh_build_async; lights: the layout-4 light SSBO.
 * The wide walk's structures and the RI grid are rebuilt on the device from a device-built LBVH
 * (rt_options.inw_device_build, the default), else on the host.  Synchronises the device first.
 * timing_ms (may be NULL) receives the host time of {records, LBVH (upload + device build, +
 * read-back for the host builders), the wide walk's structures (device or host build), their
 * upload (0 for the device build)}.  If any step fails the scene keeps its
 * previous object count but its buffers may be partly replaced: every render of it then returns
 * RT_E_ARG until a later update succeeds. */
int rt_dev_scene_inw_update(rt_dev_scene *s, const float *geom, uint32_t n, const float *nodes, const float *aabbs,
                            const float *lights, uint32_t n_lights, double timing_ms[4]);
/* rt_dev_scene_inw_update with nodes = NULL for inputs that live on the scene's device: the redraw of a
 * host that moves its objects on the GPU (a torch simulation step, or any producer that keeps the N*28
 * records in device memory) runs device to device, records -> update -> frame.  d_geom: N*28 records of
 * the scene's layout; d_aabbs: N*6 boxes (the caller's, or rt_inw_swept_boxes_async's); d_lights: the
 * layout-4 light SSBO (L*7).  All device pointers; d_geom is read fastest when 16-byte aligned.
 * The inputs are read in `stream` order (a producer kernel enqueued on `stream` before the call needs no
 * synchronisation) and all device work runs on `stream`, which the call synchronises (the builds read
 * counts back; the device is synchronised first, as by rt_dev_scene_inw_update).  When it returns all
 * of its device work has finished, the derived compact and quantised nodes included, so a render or
 * query on any stream may follow at once.  No geometry byte crosses to the host, except where the
 * host builders are needed: a device build that runs past its level cap (rt_debug_wide_info info[7] =
 * 2 then), a scene with inw_device_build = 0, or one object; then the records and the device LBVH are
 * copied back once and the host builders run as for rt_dev_scene_inw_update, time-bin trees included.
 * It builds everything rt_dev_scene_inw_update builds -- the hot, cold and sphere records (byte-equal
 * to the host's), the lights, the LBVH, leaf boxes, ranks, high-water mark and swept wide tree, the RI
 * grid, the compact and quantised nodes -- and, new, the time-bin trees (rt_options.inw_time_bins of
 * the scene) on the device, so the updated scene has every structure a fresh one has.  The decisions
 * follow the host's rules, from a reduction on the device: sphere records where every object is an
 * unrotated sphere; the wide walk where no object sticks out of its box by more than the margin and
 * every value is finite; bin trees where the wide walk applies, inw_time_bins >= 2, some object moves
 * and every bin box is finite.  Trees that together would reach 2^24 nodes or 2^32 bytes (the walkers'
 * ids) are not built: the scene keeps the swept tree alone.  A textured object on a scene with no
 * texture bound cannot be refused up front here: the update succeeds and every render and shading query of
 * the scene returns RT_E_UNSUPPORTED until a later update.  Frames and queries are bit-identical to a
 * fresh scene's of the same records and boxes.
 * flags: 0 is the library's choice, RT_UPDATE_BINS -- the smaller update + frame sum on the C3 scene
 * (measured, DESIGN.md §5.15: the bin trees raise the update from 1.10 to 2.35 ms and cut the 1920 x
 * 1080, 500 spp frame that follows from 148.04 to 146.30 ms; the sums, 148.63 [148.05, 148.86] against
 * 149.12 [148.73, 149.82] ms, lie outside each other's spread; at 200,000 objects 15.9 against 6.9 ms
 * buys 49 ms of a 2.9 s frame; a host that redraws small or low-sample frames may prefer
 * RT_UPDATE_NO_BINS); RT_UPDATE_BINS or RT_UPDATE_NO_BINS forces one; both together, or any other bit, is
 * RT_E_ARG.
 * timing_ms (may be NULL) receives the host time of {records and decisions; LBVH; swept tree + RI grid +
 * derived nodes (or the host build); time-bin trees}.
 * RT_E_ARG for a null scene, null d_geom or d_aabbs, n == 0, null d_lights with n_lights > 0 on a
 * layout-4 scene or bad flags, and RT_E_UNSUPPORTED for an IOW-03 scene or n > 2^24, come back before a
 * device is touched, the scene untouched and timing_ms unwritten.  A later failure leaves the scene
 * broken as rt_dev_scene_inw_update does. */
#define RT_UPDATE_BINS    4   /* build the time-bin trees (rt_options.inw_time_bins of the scene) */
#define RT_UPDATE_NO_BINS 8   /* swept tree only, as rt_dev_scene_inw_update's device build leaves it */
int rt_dev_scene_inw_update_device(rt_dev_scene *s, const float *d_geom /* N*28, device */, uint32_t n,
                                   const float *d_aabbs /* N*6, device */,
                                   const float *d_lights /* L*7, device; layout 4 */, uint32_t n_lights,
                                   int flags, void *stream, double timing_ms[4]);
/* Per object a box (lo xyz, hi xyz) that contains it over the whole shutter interval, from the records
 * alone, so a simulation that only moves positions can feed the update without computing boxes: the
 * segment of its centre from position - delta to position, widened by the object's half extent under
 * both orientation conventions of its rotation, inflated and rounded outward (the time-bin trees' box
 * formula with one bin).  These are not rt_pack_inw's boxes: that packer works from the description's
 * Euler angles and last_position, which the records do not carry.  The image of a scene updated with
 * them is the reference's image for the LBVH over these boxes.  Device pointers; never synchronises.
 * RT_E_ARG for null pointers; n == 0 returns RT_OK. */
int rt_inw_swept_boxes_async(const float *d_geom, uint32_t n, float *d_aabbs_out /* N*6 */, void *stream);
/* The next edit of an IOW-03 scene (the reference's stage is an editor: every ImGui edit of an object
 * runs CopyObjBuffer and restarts the spiral, 03_Shadows_and_Materials/materials.cpp:77-152, :329-364)
 * on the scene's existing device buffers: new hot and cold records, the RI priors, the object boxes and
 * the culling BVH.  types: n; records: n*24; n may be the same, larger or smaller.  spp, the sample
 * tables, the workspaces and the speculation records are kept.  Synchronises the device first; all of
 * its device work has finished when it returns, so a render on any stream (a non-blocking one
 * included) may follow at once.
 * After it the scene behaves as a fresh scene of the new records would: every render
 * (rt_render_image_async, rt_render_tiles_async, rt_render_spiral_async, with iow_spec 0 and 1) and
 * every query (rt_trace_iow_rays_async, rt_path_iow_rays_async, rt_camera_rays_async,
 * rt_pixel_query_async) returns, bit for bit, what rt_dev_scene_iow03(types, records, n, spp) with the
 * same options returns, for every option.  Counters [0], [4] and [5] are the fresh scene's too; [1]
 * and [2] are this build's own, as everywhere: the fresh scene's with RT_UPDATE_HOST_BUILD, possibly
 * others with the device build.
 * flags: 0 is the library's choice -- the device build from 1024 objects on, the host build below
 * (measured, DESIGN.md §5.12: the device build is the faster one from 485 objects on, 0.35 against
 * 0.48 ms there and 0.76 against 28.3 ms at 16383, but at 486 objects its binned tree slowed the C2
 * frame by 2.1%, more than the build saves; a host that renders long frames of a large scene may
 * prefer RT_UPDATE_HOST_BUILD); RT_UPDATE_HOST_BUILD or RT_UPDATE_DEVICE_BUILD forces one builder; both together,
 * or any other bit, is RT_E_ARG.  The [build] options keep the values the scene was built with: a
 * scene created with iow_linear = 1 keeps the linear loop and builds nothing.  n < 2 or n >= 16384
 * means no BVH, as for a fresh scene.  A device build that runs past its level cap, or meets a box
 * that is not finite, is redone by the host builder.
 * timing_ms (may be NULL) receives the host time of {records and priors with their uploads; boxes
 * and culling BVH; upload of host-built structures, 0 for the device build; the whole call}.
 * RT_E_ARG for a null scene, null types or records, n == 0 or bad flags, and RT_E_UNSUPPORTED for an
 * INW scene, come back before a device is touched, the scene untouched and still valid.  If a later
 * step fails the scene keeps its previous object count but its buffers may be partly replaced: every
 * render and query of it then returns RT_E_ARG until a later update succeeds.  Calls on one scene
 * must not overlap its renders or queries. */
#define RT_UPDATE_HOST_BUILD   1   /* culling BVH by rtamd::iow_cull_build, as rt_dev_scene_iow03 builds it */
#define RT_UPDATE_DEVICE_BUILD 2   /* culling BVH built on the device */
int rt_dev_scene_iow03_update(rt_dev_scene *s, const float *types, const float *records /* N*24 */,
                              uint32_t n, int flags, double timing_ms[4]);
/* rt_dev_scene_iow03_update for types and records that live on the scene's device: the edit loop of a
 * host that changes the scene on the GPU (a torch optimiser or simulation that keeps the n*24 records
 * in device memory) runs device to device, records -> update -> frame.  d_types: n; d_records: n*24,
 * read fastest when 16-byte aligned, correct at any 4-byte alignment.  n may stay, grow or shrink;
 * spp, the sample tables, the workspaces and the speculation records are kept, and so are the scene's
 * [build] options (a scene created with iow_linear = 1 builds no BVH; n < 2 or n >= 16384 means no
 * BVH).
 * The inputs are read in `stream` order (a producer kernel enqueued on `stream` before the call needs no
 * synchronisation) and all device work runs on `stream`.  The call synchronises the device first, as
 * rt_dev_scene_iow03_update does, and `stream` at the end (the build reads its counts back): when it
 * returns, a render or query on any stream, a non-blocking one included, may follow at once.
 * The hot and cold records come from a kernel (byte-equal to the host packer's: IEEE division for the
 * 1/scale values, the identity flag from the rotation's bit patterns), the RI priors from a sort of
 * the RI values on the device and a run-length pass (the host's answers for every scene whose RIs hold
 * no NaN and no -0.0; ten words of result are all that is read back).  After the call the scene
 * behaves as rt_dev_scene_iow03(types, records, n, spp) with the same options would: bit for bit for
 * every render and query rt_dev_scene_iow03_update lists, and for rt_render_pass_async,
 * rt_render_pass_pixels_async and their tile-list forms.  Counters [0], [4] and [5] are the fresh
 * scene's; [1] and [2] are the build's own.
 * flags: the two bits of rt_dev_scene_iow03_update; both together, or any other bit, is RT_E_ARG.
 * RT_UPDATE_DEVICE_BUILD: no record byte crosses to the host.  RT_UPDATE_HOST_BUILD: the types and
 * records are copied back once (n*25 floats) and rtamd::iow_cull_build runs as for a fresh scene; the
 * hot and cold records and the priors still come from the device kernels.  0 is the library's choice by
 * the same rule and the same constant as rt_dev_scene_iow03_update: the device build from 1024 objects
 * on, below that the host build with the one copy-back (under 100 KB) -- because at 486 objects the
 * device's binned tree slowed the C2 frame by 2.1%, far more than the copy costs
 * (DESIGN.md §5.18).  A device build that runs past its level cap, or meets a box that is not
 * finite, is redone by the host builder after the same copy-back (rt_debug_iow_info info[3] = 2 or 3).
 * timing_ms (may be NULL) receives the host time of {records and priors (their enqueue); boxes and
 * culling BVH; copy-back plus upload of host-built structures, 0 for the device build; the whole call}.
 * RT_E_ARG for a null scene, null d_types or d_records, n == 0 or bad flags, and RT_E_UNSUPPORTED for an
 * INW scene, come back before a device is touched, the scene untouched and still valid, timing_ms
 * unwritten.  A later failure leaves the scene broken as rt_dev_scene_iow03_update does. */
int rt_dev_scene_iow03_update_device(rt_dev_scene *s, const float *d_types /* n, device */,
                                     const float *d_records /* n*24, device */, uint32_t n,
                                     int flags, void *stream, double timing_ms[4]);
/* Replace the scene's options (the [build] ones keep the values the scene was built with). */
int rt_dev_scene_set_options(rt_dev_scene *s, const rt_options *o);

/* Render one tile list.  tiles: device int array of n_tiles (tx, ty) pairs of tile_size^2
 * tiles; out_packed: device float array n_tiles*tile_size*tile_size*4 (tile-major, row-major
 * inside a tile; pixels outside the image are written as 0).  out_depth may be NULL. */
int rt_render_tiles_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p,
                          const int *d_tiles, int n_tiles, int tile_size,
                          float *d_out_packed, float *d_out_depth_packed,
                          uint64_t *d_counters, void *stream);

/* Render the rectangle in p->tile_* into a full W*H image resident on the device. */
int rt_render_image_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p,
                          float *d_rgba, float *d_depth, uint64_t *d_counters, void *stream);

/* ---- ray queries -------------------------------------------------------------------------
 * Batched closest-hit queries on an INW device scene: what does this ray hit?  (Picking,
 * visibility and collision probes, debugging a pixel.)  A query's result is what the reference
 * shader's closest-hit walk leaves behind -- layout 1: 01_BoundingVolumeHierarchy/
 * computeShaderSrc.glsl:431-473 with IntersectRay :230-269; layout 4: 04_Lights_Camera_And_Action/
 * computeShaderSrc.glsl:524-563 -- started on an EMPTY 40-float stack with t_limiting = tmax, the
 * object positions of time ratio `ratio` (the shader's sample index / samples, 0..1 there), and the child
 * order RT_TRACE_INVERT selects (set: the order the shader takes when dot(u_Camera.Direction,
 * (1,1,1)) > 0).  The kernel runs the render path's own walk (the scene's options apply: wide
 * walk, time-bin trees, sphere records, compact nodes, stackless walks, fused cull), so results
 * are bit-identical whatever the options.
 *   - A query hits if and only if t_limiting ended below tmax.  Hit: t = the final t_limiting,
 *     id = the object's index, n = the world-space normal the shader computes (IntersectRay),
 *     extra = record float 19 (layout 4: the object's refractive index).  Miss: t = tmax exactly
 *     as passed, id = -1, n = 0, extra = 0.  pad is written as 0.
 *   - Exact ties in t go to the object the reference's depth-first order reaches first for that
 *     child order.
 *   - A push the reference's full stack would drop is dropped here too (the result is then the
 *     reference's, not the geometric closest hit) and counted in counters[4].
 *   - tmax <= 0 or NaN: a miss by the shader's own tests (t > 0 && t < t_limiting); no walk runs.
 *   - A direction with zero or non-finite components gives what the reference walk gives (its
 *     reciprocals are infinite or NaN; the box tests then follow IEEE min / max).
 *   - Any ratio is answered as the shader would: its object positions are position - delta *
 *     (1 - ratio) whatever the ratio, below 0, above 1, infinite or NaN.  A ratio outside [0, 1]
 *     (or NaN) takes the reference walk: the time-bin trees and the swept boxes cover [0, 1] only.
 *   - So does an origin farther than 1000 from the world origin on some axis, NaN included.
 *   - RT_TRACE_ANY (occlusion): id >= 0 exactly when the closest-hit query hits; id is then some
 *     accepted object and t its t, t_closest <= t < tmax; n = 0 and extra = 0.
 *   - counters (6 x u64 as rt_stats' first six fields, added to): [0] += n_rays; [1], [2] the node
 *     visits and primitive tests of the walks that ran (they depend on the options, as in the
 *     renders); [4] += dropped pushes; [3] and [5] untouched.
 * Returns RT_E_ARG for a null scene, null rays or hits with n_rays > 0, unknown flag bits,
 * n_rays > 2^31 or a scene a failed update left broken; RT_E_UNSUPPORTED for an IOW-03 scene (those
 * have rt_trace_iow_rays_async, below);
 * n_rays == 0 returns RT_OK and launches nothing.  Calls on one scene must not overlap each other
 * or its renders (they share the scene's work queue). */
typedef struct rt_ray { float o[3]; float tmax; float d[3]; float ratio; } rt_ray;                /* 32 B */
typedef struct rt_hit { float t; int32_t id; float n[3]; float extra; uint32_t pad[2]; } rt_hit;  /* 32 B */
#define RT_TRACE_INVERT 1   /* child order of the shader's walk: its dot(camDir,(1,1,1)) > 0 case */
#define RT_TRACE_ANY    2   /* occlusion query: may stop at the first accepted hit */
/* Device pointers (16-byte aligned); never allocates or synchronises (as rt_render_image_async). */
int rt_trace_rays_async(rt_dev_scene *s, const rt_ray *d_rays, uint32_t n_rays, int flags,
                        rt_hit *d_hits, uint64_t *d_counters /* 6 x u64, added to; may be NULL */, void *stream);
/* Blocking: host buffers; builds a device scene for the call (like rt_render_inw) from the
 * GeometryBuff records and LBVH nodes.  st (may be NULL): the counters and the kernel's device time.
 * RT_E_ARG also for null geom / nodes, n == 0 or a layout other than 1 and 4. */
int rt_trace_inw(const float *geom, uint32_t n, int layout, const float *nodes, const rt_ray *rays,
                 uint32_t n_rays, int flags, rt_hit *hits, int device, rt_stats *st);

/* ---- ray queries, IOW-03 ------------------------------------------------------------------
 * The same question on an IOW-03 device scene.  rt_ray and rt_hit are reused.  A query's result is
 * what the reference shader's LaunchRay (03_Shadows_and_Materials/computeShaderSrc.glsl:196-256)
 * computes for (o, d, max_t = tmax); rt_ray.ratio is ignored, any bit pattern may be in it.  The
 * kernel runs the render path's own search (the scene's options apply: iow_linear, iow_lds_bvh,
 * iow_leaf_batch), so results are bit-identical whatever the options.
 *   - A query hits if and only if min_t ended below tmax.  Hit: t = the final min_t, id = the
 *     object's index, n = RayReturnData.normal (world space, normalised), extra = record float 20
 *     (the object's refractive index, material.z).  Miss: t = tmax exactly as passed, id = -1,
 *     n = 0, extra = 0.  pad is written as 0.
 *   - What t measures: t is the shader's own min_t, a distance along normalize(M * d) in the hit
 *     object's frame, NOT the parameter of d.  The hit point is o + d * t, as the shader forms it.
 *     t equals the usual ray parameter only for unit d and an orthonormal M.
 *   - Exact ties in t go to the lowest object index (the reference's strict min_t > t).
 *   - tmax <= 0 or NaN: a miss by the shader's own test (min_t > t && t > 0); no walk runs.
 *   - A zero or NaN direction is a miss: every object's t is -1.
 *   - Directions with |d|^2 outside (0.998, 1.002) are answered by the reference's linear loop, as
 *     in the renders: exact, but n object tests per query.  Normalise directions to get the BVH.
 *   - RT_TRACE_ANY: as above (id >= 0 exactly when the closest-hit query hits, t_closest <= t <
 *     tmax, n = 0, extra = 0).  RT_TRACE_INVERT has no meaning here: any bit other than
 *     RT_TRACE_ANY is an error.
 *   - counters: [0] += n_rays; [1], [2] the node visits and object tests of the searches that ran
 *     (they depend on the options); [3], [4], [5] untouched.
 * Returns RT_E_ARG for a null scene, null rays or hits with n_rays > 0, a flag bit other than
 * RT_TRACE_ANY, n_rays > 2^31 or a scene a failed rt_dev_scene_iow03_update left broken;
 * RT_E_UNSUPPORTED for an INW scene; n_rays == 0 returns RT_OK and launches nothing.  Every
 * argument error comes back before a device is touched.  Calls on one scene must not overlap each
 * other or its renders (they share the scene's work queue). */
/* Device pointers (16-byte aligned); never allocates or synchronises. */
int rt_trace_iow_rays_async(rt_dev_scene *s, const rt_ray *d_rays, uint32_t n_rays, int flags,
                            rt_hit *d_hits, uint64_t *d_counters /* 6 x u64, added to; may be NULL */, void *stream);
/* Blocking: host buffers; builds a device scene for the call, like rt_render_iow03, from the
 * ObjectTypes and N*24 record buffers.  st (may be NULL): the counters and the kernel's device time.
 * RT_E_ARG also for null types / records or n == 0. */
int rt_trace_iow03(const float *types, const float *records /* N*24 */, uint32_t n, const rt_ray *rays,
                   uint32_t n_rays, int flags, rt_hit *hits, int device, rt_stats *st);

/* ---- path (radiance) queries --------------------------------------------------------------
 * Batched path queries on an INW device scene: what does this ray SEE?  (Light probes, reflection
 * captures, "why is sample 37 of this pixel white?".)  One query is one invocation of the reference
 * shader's out_Pixel ray loop -- layout 1: 01_BoundingVolumeHierarchy/computeShaderSrc.glsl:414-597;
 * layout 4: 04_Lights_Camera_And_Action/computeShaderSrc.glsl:510-713 -- started from the caller's
 * ray instead of the camera's: an empty 40-float stack, push_ray(o, d, contribution = 1,
 * bounced = 0), no MULTIFOCUS record, then the loop to its end with the materials and textures,
 * the surrounding-RI walks, INW-04's shadow rays, the scatter step and the stack's silent drops.
 * For the shader's own camera ray of (pixel, sample s) a query returns exactly that sample's
 * `color` and `depth`, so a frame is the End() fold of path queries, bit for bit.  The kernel runs
 * the render path's own segment (the scene's options apply), so results are bit-identical whatever
 * the options.
 *   - sample = the shader's sample index s: the time ratio is (float)s * (1.0f / spp) and the
 *     scatter offsets are sunflower[2s], [2s + 1] of the scene's table; spp is the value the scene
 *     was created with.  u_NumOfBounces = max_bounces.  pad is ignored: any bits may be in it.
 *   - The primary ray's limit is the shader's 32000; there is no per-ray tmax.
 *   - A query whose origin lies farther than 1000 from the world origin on some axis (NaN included)
 *     runs its whole path on the reference walks, with or without the fused cull: the same answer,
 *     without the culling trees.
 *   - RT_TRACE_INVERT selects the child order of the walks, as for rt_trace_rays_async.  Any other
 *     flag bit is an error.
 *   - rgb = the loop's final `color`: before End()'s sqrt, and (1, 1, 1) after INW-04's
 *     lit-geometry break.
 *   - depth = the shader's `depth`.  It is written only by a segment that MISSES, so it is 0 or that
 *     miss's t_limiting (32000 for a primary miss): the shader's behaviour, not a hit distance --
 *     rt_trace_rays_async answers that.
 *   - segments, drops, nans = this path's rays popped, pushes the full stack dropped and NaN
 *     secondary directions; status = 0.
 *   - sample >= spp: status = 1 and every other field 0; no path runs and the query is not counted.
 *   - counters (6 x u64 as rt_stats' first six fields, added to): [0] += segments, [3] += shadow
 *     queries, [4] += dropped pushes, [5] += NaN directions, all as the reference counts them;
 *     [1], [2] this build's own node visits and primitive tests (they depend on the options and on
 *     the skipped RI walks, as in the renders).
 * Returns RT_E_ARG for a null scene, null rays or out with n_rays > 0, a flag bit other than
 * RT_TRACE_INVERT, max_bounces < 0, n_rays > 2^31 or a scene a failed update left broken;
 * RT_E_UNSUPPORTED for an IOW-03 scene: an IOW-03 sample reads the RI stack the previous sample of
 * its pixel left behind, so a single ray has no defined radiance there (rt_path_iow_rays_async,
 * below, takes that stack state as an input).  n_rays == 0 returns RT_OK
 * and launches nothing.  Every argument error comes back before a device is touched.  Calls on one
 * scene must not overlap each other, its renders or its ray queries (they share its work queue). */
typedef struct rt_path_ray { float o[3]; uint32_t sample; float d[3]; uint32_t pad; } rt_path_ray;   /* 32 B */
typedef struct rt_path_out { float rgb[3]; float depth; uint32_t segments, drops, nans, status; } rt_path_out; /* 32 B */
/* Device pointers (16-byte aligned); never allocates or synchronises. */
int rt_path_rays_async(rt_dev_scene *s, const rt_path_ray *d_rays, uint32_t n_rays, int max_bounces, int flags,
                       rt_path_out *d_out, uint64_t *d_counters /* 6 x u64, added to; may be NULL */, void *stream);
/* Blocking: host buffers; builds a device scene for the call like rt_render_inw_tex (sample tables
 * of `spp` entries, lights, textures).  st (may be NULL): the counters and the kernel's device time.
 * RT_E_ARG also for null geom / nodes, n == 0, a layout other than 1 and 4, spp < 1, n_lights > 0
 * with null lights or bad textures; RT_E_UNSUPPORTED for textured objects with no texture bound. */
int rt_path_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights, uint32_t n_lights,
                const rt_texture *tex, int n_tex, int spp, int max_bounces, const rt_path_ray *rays, uint32_t n_rays,
                int flags, rt_path_out *out, int device, rt_stats *st);

/* ---- path (radiance) queries, IOW-03 ------------------------------------------------------
 * The same question on an IOW-03 device scene.  One query is one invocation of the reference
 * shader's LaunchRays (03_Shadows_and_Materials/computeShaderSrc.glsl:285-358) for (o, d): the ray
 * stack empty and skip = 0, the RI fields of its four slots holding the incoming state ri_in,
 * push(o, d, contribution = 1, RI = 1, bounced = 0), then the loop to its end.  The RI fields are
 * all a sample inherits from its pixel's previous one: the stack is empty between samples, skip is
 * local, and no other slot field is read before it is written.
 *   - sample picks the scatter table entry fib[sample] of the scene's table; spp is the value the
 *     scene was created with.  u_NumOfBounce = max_bounces, any value >= 0.  Every segment's limit is
 *     the shader's 32000; there is no per-ray tmax.  pad is ignored: any bits may be in it.
 *   - State: ri_in = {0, 0, 0, 0} is what a pixel's first sample sees.  ri_out[e] is slot e's RI
 *     field when the path ends: the last value the path pushed there, or the incoming value if it
 *     never wrote the slot.  A pixel's sample s is therefore the query of its camera ray with ri_in
 *     = the ri_out of sample s - 1, and a frame's pixel is sum(rgb) * RN(1 / spp), as out_Pixel does
 *     it, bit for bit.
 *   - stale: bit e is set iff the path used the incoming value of slot e as a parent RI (a hit from
 *     inside, cos_t > 0, whose parent index pi = size - 1 - skip is in 0..3 and names a slot this
 *     path has not written yet).  stale == 0: the answer does not depend on ri_in.  More generally,
 *     changing ri_in[e] for any e whose bit is clear changes nothing but ri_out[e] of an unwritten
 *     slot.
 *   - Chains (chain >= 1): queries [k * chain, (k + 1) * chain) form a chain; the last chain may be
 *     short.  The first query of a chain takes its own ri_in; every later one ignores its ri_in and
 *     takes its predecessor's outgoing state.  chain = 1: every query is independent.  chain = spp
 *     with a pixel's camera rays in sample order: one launch answers every sample of that pixel.
 *   - rgb = the function's return value (`sample`); segments, drops, nans = this path's popped rays,
 *     pushes dropped by the full 4-entry stack and NaN secondary directions, counted as the renders
 *     count them; status = 0.
 *   - sample >= spp: status = 1; rgb, stale and the counts are 0; ri_out is the state on entry (the
 *     chain passes through it).  No path runs and nothing is counted.
 *   - Directions are handled by the scene's own search, as in the renders and in
 *     rt_trace_iow_rays_async: |d|^2 outside (0.998, 1.002) takes the linear loop, a zero or NaN
 *     direction misses (a NaN direction's rgb is the NaN its background colour is; which NaN is not
 *     defined); bounce directions are normalised by the shader.
 *   - The scene's options apply (iow_linear, iow_lds_bvh, iow_leaf_batch); results are bit-identical
 *     whatever they are.
 *   - counters: [0] += segments, [4] += dropped pushes, [5] += NaN directions, as the reference
 *     counts them; [1], [2] this build's own node visits and object tests; [3] untouched.
 * Returns RT_E_ARG for a null scene (even with n_rays == 0), null rays or out with n_rays > 0,
 * chain == 0, flags != 0 (reserved), max_bounces < 0, n_rays > 2^31 or a scene a failed
 * rt_dev_scene_iow03_update left broken; RT_E_UNSUPPORTED for an INW scene; n_rays == 0 returns RT_OK
 * and launches nothing.  Every argument error comes back before a device is touched, with the
 * output untouched.  Calls on one scene must not overlap each other, its renders or its ray
 * queries. */
typedef struct rt_path_iow_ray { float o[3]; uint32_t sample; float d[3]; uint32_t pad; float ri_in[4]; } rt_path_iow_ray;   /* 48 B */
typedef struct rt_path_iow_out { float rgb[3]; uint32_t stale; uint32_t segments, drops, nans, status; float ri_out[4]; } rt_path_iow_out; /* 48 B */
/* Device pointers (16-byte aligned); never allocates or synchronises, so it is graph-capturable
 * like the other queries. */
int rt_path_iow_rays_async(rt_dev_scene *s, const rt_path_iow_ray *d_rays, uint32_t n_rays, uint32_t chain,
                           int max_bounces, int flags, rt_path_iow_out *d_out,
                           uint64_t *d_counters /* 6 x u64, added to; may be NULL */, void *stream);
/* Blocking: host buffers; builds a device scene for the call like rt_render_iow03 (sample tables of
 * `spp` entries).  st (may be NULL): the counters and the kernel's device time.  RT_E_ARG also for
 * null types / records, n == 0 or spp < 1. */
int rt_path_iow03(const float *types, const float *records /* N*24 */, uint32_t n, int spp, int max_bounces,
                  const rt_path_iow_ray *rays, uint32_t n_rays, uint32_t chain, int flags,
                  rt_path_iow_out *out, int device, rt_stats *st);

/* ---- pixel queries --------------------------------------------------------------------------
 * The two ends of the path queries' theorem as entry points: the shader's own camera ray of (pixel,
 * sample), and the shader's fold of a pixel's answers.  With them "what is pixel (x, y) of this
 * frame, and what did each of its samples contribute?" is one call: no W x H render, no host
 * arithmetic, nothing of out_Pixel's prologue to restate.
 *
 * rt_camera_rays_async writes the camera rays of samples [s0, s0 + ns) of n_pixels pixels as
 * path-query records: rt_path_ray (32 B) on an INW scene, rt_path_iow_ray (48 B, ri_in = 0) on an
 * IOW-03 one.  Record k * ns + j is the ray of pixel d_pixels[k], sample s0 + j, with sample = s0 + j
 * and pad = 0: pixel-major, so an IOW-03 pixel is one chain of ns consecutive records.
 *   - The rays are, bit for bit, what the render kernels push for that pixel and sample -- the
 *     kernel calls the renders' own device functions.  INW: out_Pixel's prologue
 *     (01_BoundingVolumeHierarchy/computeShaderSrc.glsl:366-410), the single-focus branch: origin
 *     tip - la, direction la.  IOW-03: 03_Shadows_and_Materials/computeShaderSrc.glsl:370-406 with
 *     the scene's sunflower and ring tables.
 *   - y is pixel_coords.y: the GL image's bottom row first, the row index of the renders' output.
 *   - p->width, p->height and p->spp are read; p->spp must equal the scene's, as for the renders.
 *     p->tile_*, p->max_bounces and p->show_normal are ignored.  The frame uniforms (screen_dist,
 *     1 / spp) are formed as the renders form them.
 *   - A pixel outside [0, W) x [0, H) and a sample index >= spp (s0 + ns may overrun) get sample =
 *     0xffffffff and every other field 0, which the path queries answer with status = 1.  So does an
 *     IOW-03 sample whose ring entry is the shader's early-return marker (03...glsl:396); with the
 *     tables rt_sample_tables builds no spp >= 1 has one.
 * Returns RT_E_ARG for a null scene, cam or p, bad params (width, height, spp < 1, max_bounces < 0),
 * p->spp != the scene's, null d_pixels or d_rays with n_pixels * ns > 0, n_pixels * ns > 2^31 or a
 * scene a failed update left broken; n_pixels == 0 or ns == 0 returns RT_OK and launches nothing.
 * Every argument error comes back before a device is touched. */
typedef struct rt_pixel { int32_t x, y; } rt_pixel;   /* 8 B; y = pixel_coords.y, GL bottom row first */
/* Device pointers (d_rays 16-byte aligned); never allocates or synchronises. */
int rt_camera_rays_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p,
                         const rt_pixel *d_pixels, uint32_t n_pixels, uint32_t s0, uint32_t ns,
                         void *d_rays, void *stream);
/* rt_pixel_query_async answers n_pixels pixels of the frame (cam, p).  It enqueues, with nothing else
 * in between: the camera rays of all spp samples into the workspace; the unchanged path kernel on
 * them (INW: max_bounces = p->max_bounces and RT_TRACE_INVERT exactly when dot(cam->dir, (1, 1, 1))
 * > 0 in binary32 in the shader's order; IOW-03: chain = spp); the fold, one rt_pixel_out per pixel:
 *   - INW: rgb = End()'s fold (01_BVH...glsl:625-675): the first sample's sqrt(colour) assigned, the
 *     others added in sample order, times RN(1 / spp); alpha = 1; depth = the depth of sample
 *     spp / 2.
 *   - IOW-03: rgb = the samples' rgb added in order from 0, times RN(1 / spp) (a pixel stops at its
 *     first status = 1 answer, sample s, and is scaled by RN(1 / s): the shader's early return);
 *     alpha = 1; depth = 0.
 *   - segments, drops, nans = the sums over the pixel's samples.
 *   - A pixel outside the image gives an all-zero record.
 * rgba and depth are, bit for bit, what rt_render_image_async writes at that pixel for the same cam
 * and p; counters [0], [3], [4], [5], added over all pixels of a frame, are the render's.
 * The per-sample answers (n_pixels * spp rt_path_out / rt_path_iow_out, pixel-major) go to
 * d_samples_out when given, else into the workspace.  d_ws: rt_pixel_workspace_bytes(s, n_pixels)
 * bytes (the rays plus the samples: one size serves both cases; 0 for a null scene).  After the call
 * the workspace's first n_pixels * spp records are the camera rays.
 * Returns RT_E_ARG as rt_camera_rays_async does (with ns = spp), for a null d_pixels_out or d_ws with
 * n_pixels > 0 and for ws_bytes too small; then RT_E_UNSUPPORTED for p->show_normal != 0 (that mode
 * is not a path).  n_pixels == 0 returns RT_OK and launches nothing.  Calls on one scene must not
 * overlap each other, its renders or its queries. */
typedef struct rt_pixel_out { float rgba[4]; float depth; uint32_t segments, drops, nans; } rt_pixel_out;  /* 32 B */
size_t rt_pixel_workspace_bytes(const rt_dev_scene *s, uint32_t n_pixels);
/* Device pointers (16-byte aligned); never allocates or synchronises, so it is graph-capturable. */
int rt_pixel_query_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p,
                         const rt_pixel *d_pixels, uint32_t n_pixels,
                         rt_pixel_out *d_pixels_out,
                         void *d_samples_out /* n_pixels * spp rt_path_out / rt_path_iow_out, may be NULL */,
                         void *d_ws, size_t ws_bytes,
                         uint64_t *d_counters /* 6 x u64, added to; may be NULL */, void *stream);
/* Blocking: host buffers; build a device scene for the call like rt_path_inw / rt_path_iow03 (sample
 * tables of p->spp entries).  rays_out and samples_out (n_pixels * p->spp records each) may be NULL.
 * st (may be NULL): the counters and the three kernels' device time. */
int rt_pixels_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                  uint32_t n_lights, const rt_texture *tex, int n_tex, const rt_camera *cam, const rt_params *p,
                  const rt_pixel *pixels, uint32_t n_pixels, rt_path_ray *rays_out, rt_path_out *samples_out,
                  rt_pixel_out *pixels_out, int device, rt_stats *st);
int rt_pixels_iow03(const float *types, const float *records /* N*24 */, uint32_t n, const rt_camera *cam,
                    const rt_params *p, const rt_pixel *pixels, uint32_t n_pixels, rt_path_iow_ray *rays_out,
                    rt_path_iow_out *samples_out, rt_pixel_out *pixels_out, int device, rt_stats *st);

/* ---- progressive sample passes ---------------------------------------------------------------
 * Refinement in samples: the host renders samples [0, 8) of every pixel and shows them, then [8, 40)
 * and shows the better image, and so on; after the last range it holds, bit for bit, the frame
 * rt_render_image_async would have written.  The folds allow it exactly: INW's End()
 * (01_BoundingVolumeHierarchy/computeShaderSrc.glsl:625-675) is a sequential float sum in sample
 * order (the first sqrt(colour) assigned, the others added, the sum times RN(1 / spp)), IOW-03's
 * out_Pixel (03_Shadows_and_Materials/computeShaderSrc.glsl:383-417) a sequential sum from 0, and an
 * IOW-03 sample inherits exactly four floats from its predecessor, the RI fields of the ray-stack
 * slots (rt_path_iow_rays_async's ri_in / ri_out).  Cutting the sample loop anywhere changes no bit.
 *
 * rt_render_pass_async renders samples [s0, min(s0 + ns, S)) of every pixel of the rectangle
 * p->tile_* (the whole frame when tile_w or tile_h is 0), exactly as rt_render_image_async reads
 * that rectangle.  S = spp on an INW scene; on an IOW-03 scene S is the first sample whose ring entry
 * is the shader's early-return marker (03...glsl:396), else spp (no table rt_sample_tables builds has
 * such a marker).
 *   - State: d_state[y * W + x] is the pixel's state after samples [0, s0); the pass leaves it as the
 *     state after [0, min(s0 + ns, S)).  INW: acc = End()'s running sum, depth = the depth of sample
 *     spp / 2 once that sample has run, else 0; ri is neither read nor written.  IOW-03: acc = the
 *     running sum, depth = 0, ri = the RI fields of the four stack slots as the last sample left
 *     them.  With s0 == 0 the incoming state is not read (no memset is needed): INW assigns the
 *     first sample, IOW-03 starts from 0 with ri = 0.  The caller issues the passes of a frame in
 *     order, with s0 equal to the samples already in the state; the call cannot check this.
 *   - Image: when d_rgba is given, the pixel's value is acc * RN(1 / k) with alpha 1, k = min(s0 +
 *     ns, S): the frame as it would be at k samples of these tables.  At k == S it is the frame
 *     rt_render_image_async writes, bit for bit; so is d_depth (INW: the state's depth; IOW-03: 0).
 *     Pixels outside the rectangle keep their state and image bytes.
 *   - counters: added to as the renders count them; summed over the passes of a frame, [0], [3], [4]
 *     and [5] (INW) or [0], [4] and [5] (IOW-03) are the render's; [1], [2] are this build's own.
 *   - The scene's options apply (wide walk, time bins, sphere records, stackless walks, fused cull,
 *     iow_linear, iow_lds_bvh, iow_leaf_batch); the result is bit-identical whatever they are.  A
 *     scene updated by rt_dev_scene_inw_update / rt_dev_scene_iow03_update behaves as a fresh one.
 *   - Never synchronises.  On an IOW-03 scene it never allocates; on an INW scene a pass is, per chunk
 *     of samples, the camera rays, rt_path_rays_async's kernel on them and the fold, in a workspace the
 *     scene owns (64 B per pixel unit and sample of a chunk, at most 2 GB unless one sample of the
 *     rectangle needs more): the first pass of a rectangle size and sample count grows it, as the
 *     first render of a frame size allocates, and later passes allocate nothing, so they are
 *     graph-capturable.  Calls on one scene must not overlap each other, its renders or its queries.
 * Returns RT_E_ARG, before a device is touched and with the buffers untouched, for a null scene, cam,
 * p or d_state, bad params as the renders judge them, p->spp != the scene's, s0 >= p->spp or a scene
 * a failed update left broken; then RT_E_UNSUPPORTED for p->show_normal != 0.  ns == 0 returns RT_OK
 * and launches nothing; s0 + ns may overrun S (the pass is clipped).  Packed tile lists and
 * device groups are served by rt_render_pass_tiles_async and rt_render_pass_multi_async in the multi-GPU
 * section.  Not covered: the MULTIFOCUS camera (no device scene has one: only rt_render_inw_mf's own).
 * Packed pixel lists, with a sample count per pixel, are served by rt_render_pass_pixels_async below;
 * "Captured graphs" there states a rule that was seen to hold for captured passes as well. */
typedef struct rt_pass_state { float acc[3]; float depth; float ri[4]; } rt_pass_state;   /* 32 B */
/* Device pointers (16-byte aligned). */
int rt_render_pass_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p,
                         uint32_t s0, uint32_t ns, rt_pass_state *d_state /* W*H */,
                         float *d_rgba /* W*H*4, may be NULL */, float *d_depth /* W*H, may be NULL */,
                         uint64_t *d_counters /* 6 x u64, added to; may be NULL */, void *stream);
/* Blocking: host buffers; build a device scene for the call like rt_pixels_inw / rt_pixels_iow03.
 * cuts is strictly increasing with cuts[0] > 0 and cuts[n_cuts - 1] <= p->spp; pass i renders
 * [cuts[i - 1], cuts[i]) (from 0 for i = 0) and image i (rgba + i * W*H*4, depth + i * W*H) is the
 * image after it; pixels outside the rectangle keep the bytes the buffers came with.  state_out (may
 * be NULL): the state after the last pass.  st (may be NULL): the counters and the passes' device
 * time.  RT_E_ARG also for null rgba or bad cuts. */
int rt_render_passes_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                         uint32_t n_lights, const rt_texture *tex, int n_tex, const rt_camera *cam,
                         const rt_params *p, const uint32_t *cuts, int n_cuts,
                         float *rgba /* n_cuts*W*H*4 */, float *depth /* n_cuts*W*H or NULL */,
                         rt_pass_state *state_out /* W*H, may be NULL */, int device, rt_stats *st);
int rt_render_passes_iow03(const float *types, const float *records /* N*24 */, uint32_t n, const rt_camera *cam,
                           const rt_params *p, const uint32_t *cuts, int n_cuts, float *rgba /* n_cuts*W*H*4 */,
                           rt_pass_state *state_out /* W*H, may be NULL */, int device, rt_stats *st);

/* ---- adaptive sample passes ------------------------------------------------------------------
 * Refinement that stops where the image has settled: a pass over a packed pixel list in which every
 * pixel continues from its own sample count, a device-side error estimate, and the ordered compaction
 * of the pixels that still need samples.  The sequential folds that make the passes above exact make
 * this exact too: a pixel that stopped after n samples holds, bit for bit, the state and image
 * rt_render_pass_async gives every pixel after n samples.
 *
 * rt_pass_aux is what a pixel keeps beside its rt_pass_state: count, the samples folded so far, and
 * even, the same fold as acc restricted to the even sample indices (0, 2, 4, ...) in sample order
 * (INW: sample 0's sqrt(colour) assigned, the later even samples added; IOW-03: a sum of rgb from
 * 0.0f).  A frame starts from a zeroed aux buffer; the state needs no memset.
 *
 * rt_render_pass_pixels_async handles every listed pixel inside the image: with c =
 * d_aux[y * W + x].count it renders samples [c, min(c + ns, S)) of that pixel, S as for
 * rt_render_pass_async, continues d_state (not read when c == 0) and aux.even, sets aux.count to the
 * new count c', writes acc * RN(1 / c') with alpha 1 to d_rgba and the state's depth to d_depth, and
 * adds to the counters as the passes do.  A listed pixel with c >= S renders nothing and has its image
 * rewritten from its state.  Unlisted pixels keep every byte of state, aux and image; an entry outside
 * [0, W) x [0, H) is skipped, so a host can launch with the list's full capacity without reading the
 * count back (rt_pass_select_async pads the list with {-1, -1}).  The list holds no pixel twice: the
 * caller's duty, unchecked.  p->tile_* is ignored.  The scene's options apply as for the passes.
 * Never synchronises; on an INW scene the first call of a list size and sample count grows the scene's
 * pass workspace (64 B per entry and sample of a chunk), later ones allocate nothing, so they are
 * graph-capturable, with the condition stated under "Captured graphs" below.  Calls on one scene must
 * not overlap each other, its passes, renders or queries.
 * Returns RT_E_ARG, before a device is touched and with the buffers untouched, for a null scene, cam,
 * p, d_state or d_aux, null d_pixels with n_pixels > 0, n_pixels > 2^31, bad params as the renders
 * judge them, p->spp != the scene's or a scene a failed update left broken; then RT_E_UNSUPPORTED for
 * p->show_normal != 0.  n_pixels == 0 or ns == 0 returns RT_OK and launches nothing.
 *
 * rt_pass_select_async works on the rectangle p->tile_* (the whole frame when 0).  With n = count,
 * h = (n + 1) / 2, a = acc * RN(1 / n) and e = even * RN(1 / h), all in binary32 in this order,
 *   err = (|a.x - e.x| + |a.y - e.y|) + |a.z - e.z|,   err = +inf for n < 2,
 * and a pixel is active iff n < S && (n < min_samples || !(err <= tol)): a NaN estimate keeps the pixel
 * sampling, and tol < 0 keeps every pixel active until S.  d_list[0 .. n_active) receives the active
 * pixels in the order of the passes' units (8x8 blocks of the rectangle row-major, pixels row-major
 * inside a block, units past the rectangle's edge left out), the remaining entries {-1, -1} up to the
 * count of the rectangle's pixels that lie inside the image (entries past that count keep their bytes:
 * a rectangle that leaves the image is clipped); *d_n_active the active count; d_err[y * W + x], when given, the
 * estimate of the rectangle's pixels (pixels outside it keep their bytes).  Three launches, no
 * synchronisation, no allocation beyond a scratch the scene owns (8 B per 256 units; the first call of
 * a rectangle size grows it); after that call it is graph-capturable, with the condition below.
 * RT_E_ARG for a null scene, p, d_state, d_aux, d_list or d_n_active, bad params, p->spp != the scene's
 * or a broken scene.
 *
 * Captured graphs: a known condition, cause unknown.  Before a graph of these calls is captured, run its
 * calls once eagerly ON THE STREAM THE GRAPH WILL BE REPLAYED ON.  Where the eager run had been on
 * another stream only, the first replay gave the eager bytes and every later replay gave wrong images:
 * the persistent kernels of the later rounds (k_inw_paths, k_iow_adapt, and k_iow_pass alike) found
 * their work-queue word used up, as if the 4-byte hipMemsetAsync node that zeroes it before each of
 * them had lost its order against them (node pair: queue memset -> persistent kernel).  This was seen
 * on graphs of rt_render_pass_pixels_async + rt_pass_select_async, of rt_render_pass_async +
 * rt_pass_select_async and, in the same probe, of three rt_render_pass_async calls alone, so it is not
 * particular to these two calls; with the eager run on the replay's stream every replay observed was
 * right (DESIGN.md 5.14 has the probes).  Nothing in the library's host or device code reads the
 * stream apart from launching on it. */
typedef struct rt_pass_aux { float even[3]; uint32_t count; } rt_pass_aux;   /* 16 B per pixel */
/* Device pointers (16-byte aligned; d_pixels and d_list 8-byte). */
int rt_render_pass_pixels_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p,
                                const rt_pixel *d_pixels, uint32_t n_pixels, uint32_t ns,
                                rt_pass_state *d_state /* W*H */, rt_pass_aux *d_aux /* W*H */,
                                float *d_rgba /* may be NULL */, float *d_depth /* may be NULL */,
                                uint64_t *d_counters /* may be NULL */, void *stream);
int rt_pass_select_async(rt_dev_scene *s, const rt_params *p,
                         const rt_pass_state *d_state, const rt_pass_aux *d_aux,
                         float tol, uint32_t min_samples,
                         rt_pixel *d_list /* one entry per pixel of the rectangle */,
                         uint32_t *d_n_active, float *d_err /* W*H, may be NULL */, void *stream);
/* Blocking: host buffers; build a device scene for the call like rt_render_passes_inw / _iow03 and run
 * the loop: zero the aux buffer and list every pixel of the rectangle; one listed pass with ns = batch;
 * select, and read n_active back; again while n_active > 0 and rounds remain (max_rounds == 0: no
 * limit; the loop ends by itself once every pixel has S samples).  rgba (and depth) hold the image of
 * the last pass each pixel was in; pixels outside the rectangle keep the bytes the buffers came with.
 * May be NULL: count (W*H, the samples per pixel), err (W*H, the last select's estimate), state_out,
 * aux_out, rounds_out (the rounds run), st (the counters and the rounds' summed device time).
 * RT_E_ARG also for null rgba or batch == 0. */
int rt_render_adaptive_inw(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                           uint32_t n_lights, const rt_texture *tex, int n_tex, const rt_camera *cam,
                           const rt_params *p, uint32_t batch, float tol, uint32_t min_samples,
                           uint32_t max_rounds, float *rgba /* W*H*4 */, float *depth /* W*H or NULL */,
                           uint32_t *count, float *err, rt_pass_state *state_out, rt_pass_aux *aux_out,
                           uint32_t *rounds_out, int device, rt_stats *st);
int rt_render_adaptive_iow03(const float *types, const float *records /* N*24 */, uint32_t n, const rt_camera *cam,
                             const rt_params *p, uint32_t batch, float tol, uint32_t min_samples,
                             uint32_t max_rounds, float *rgba /* W*H*4 */, uint32_t *count, float *err,
                             rt_pass_state *state_out, rt_pass_aux *aux_out, uint32_t *rounds_out, int device,
                             rt_stats *st);

/* ---- multi-GPU partition (BASELINE configs[3]) -----------------------------
 * One host thread drives several devices of this process: the frame's tiles are dealt
 * across the devices, each renders its share with rt_render_tiles_async on a stream of its own,
 * and one RCCL exchange over xGMI (grouped ncclSend / ncclRecv) brings the packed tiles to device
 * 0, which unpacks them into the W x H image.  This generalises the reference's per-tile
 * dispatch (In-One-Weekend/03_Shadows_and_Materials/materials.cpp:98-152) to devices, for the
 * host that replaces RT_Base<>::OnUpdateBase (In-Next-Week/base.h:148-173).
 *
 * rt_tile_deal: the frame's ceil(W/T) x ceil(H/T) tiles in deal order as (tx, ty) int pairs,
 * row-major for one device, else row-major permuted by the multiplicative hash
 * i * 2654435761 mod 2^32 (ties by i); entry k goes to device k % n_dev.  Writes up to cap pairs
 * to order_out (may be NULL) and returns the tile count. */
int rt_tile_deal(int width, int height, int tile_size, int n_dev, int *order_out, int cap);
/* A group of distinct devices with one RCCL communicator each (ncclCommInitAll) and a stream per
 * device.  NULL when a device is missing, not gfx950, repeated, or RCCL fails. */
typedef struct rt_group rt_group;
rt_group *rt_group_create(const int *devices, int n_dev);
void rt_group_free(rt_group *g);   /* synchronises the group's devices first */
/* Render the whole frame p->width x p->height (p->tile_* ignored) of scenes[r] (one device scene
 * per group device r, built from the same records and spp) in tile_size^2 tiles (a multiple of
 * 16) dealt by rt_tile_deal.  d_rgba (W*H*4 floats), d_depth (W*H, may be NULL) and d_counters
 * (6 x u64, added to; may be NULL) are device-0 pointers; stream is device 0's stream (the other
 * devices use the group's).  The first call for a frame size allocates the group's buffers. */
int rt_render_multi_async(rt_group *g, rt_dev_scene *const *scenes, const rt_camera *cam, const rt_params *p,
                          int tile_size, float *d_rgba, float *d_depth, uint64_t *d_counters, void *stream);
/* Blocking form of rt_render_inw over devices[0..n_dev): the scene replicated on every device, a
 * group, one partitioned frame, the image copied back (st->ms: device-0 time of the render). */
int rt_render_inw_multi(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                        uint32_t n_lights, const rt_camera *cam, const rt_params *p, const int *devices, int n_dev,
                        int tile_size, float *rgba, float *depth, rt_stats *st);

/* Progressive sample passes on packed tile lists and on device groups: a host that deals a frame over
 * several devices shows it after the first few samples, as a single-device host does with
 * rt_render_pass_async, and ends at the same frame, bit for bit.
 *
 * rt_render_pass_tiles_async is rt_render_pass_async over a packed tile list.  Tiles and slots are
 * rt_render_tiles_async's: tile_size is a positive multiple of 16, d_tiles holds n_tiles (tx, ty) int
 * pairs, slot = tile * T*T + iy * T + ix, and p->tile_* is ignored.
 *   - A slot inside the image behaves as its pixel does under rt_render_pass_async with the same s0 and
 *     ns: samples [s0, min(s0 + ns, S)) with the same S, the state not read at s0 == 0 and left
 *     byte-equal to that pixel's, the image acc * RN(1 / k) with alpha 1, the depth the state's (INW) or
 *     0 (IOW-03).
 *   - A slot outside the image (the ragged right and bottom tiles) runs no path; its state bytes are
 *     neither read nor written; its image slot is written as (0, 0, 0, 0) and its depth as 0 by every
 *     pass that is given the buffers, as rt_render_tiles_async writes them.  After the pass that reaches
 *     S the packed image is byte-equal to rt_render_tiles_async's for the same list, and on an INW scene
 *     so is the packed depth (an IOW-03 pass writes the depth 0 where the IOW-03 renders write nothing).
 *   - counters, options, synchronisation and allocation are the passes': [0], [3], [4], [5] (INW) or [0],
 *     [4], [5] (IOW-03), summed over a frame's passes and a partition's lists, are the render's; the
 *     scene's options change no bit; it never synchronises; an INW scene grows its pass workspace on
 *     the first call of a list size, IOW-03 allocates nothing.
 * Returns RT_E_ARG, before a device is touched and with the buffers untouched, for the passes'
 * conditions, null d_tiles, n_tiles <= 0, a bad tile_size or n_tiles * T*T > 2^31; then
 * RT_E_UNSUPPORTED for p->show_normal != 0 or a scene an update left without its textures.
 * The adaptive calls are served on tile lists and on groups by rt_render_pass_slots_async,
 * rt_pass_select_tiles_async and rt_render_adaptive_multi_async below. */
int rt_render_pass_tiles_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p,
                               const int *d_tiles, int n_tiles, int tile_size,
                               uint32_t s0, uint32_t ns,
                               rt_pass_state *d_state_packed   /* n_tiles*T*T */,
                               float *d_out_packed             /* n_tiles*T*T*4, may be NULL */,
                               float *d_out_depth_packed       /* n_tiles*T*T,   may be NULL */,
                               uint64_t *d_counters            /* may be NULL */, void *stream);
/* One pass of a group's frame: the deal, the streams and the argument rules are rt_render_multi_async's
 * (scenes of other devices are refused; a frame or tile size change synchronises before the lists
 * change).  The group owns one packed state buffer per device, 32 B per slot of the device's share,
 * allocated with the deal: fold state never leaves its device.  Every device runs
 * rt_render_pass_tiles_async on its share.  With d_rgba the grouped send / recv brings the packed image,
 * the depth (when d_depth is given) and the counters to device 0, where the W x H image is unpacked: it
 * is byte-equal to rt_render_pass_async's image and depth for the same cuts on one device, and after the
 * last pass to the frame of rt_render_multi_async and rt_render_image_async, on an INW scene depth included
 * (an IOW-03 pass writes the depth 0 where the IOW-03 renders write nothing).  With d_rgba == NULL only
 * the counters travel (d_depth is then ignored).
 * The group remembers how many samples its states hold for the current deal, min(s0 + ns, p->spp) after
 * a pass: s0 must be 0 (a new frame) or exactly that count, anything else is RT_E_ARG with nothing
 * launched, as are s0 >= p->spp, bad params, rt_render_multi_async's argument errors and any scene with
 * another spp or left broken by an update; then RT_E_UNSUPPORTED for p->show_normal or a scene an update
 * left without its textures.  Every scene is asked before the group is touched: a refused call leaves the
 * deal, the states and the count as they were.  A changed deal resets the count to 0; rt_render_multi_async calls in between leave
 * states and count alone; a pass that fails on some device leaves the count at 0.  ns == 0 returns RT_OK
 * and launches nothing.  Group passes have not been captured into graphs (a group works on several
 * streams: see "Captured graphs" above). */
int rt_render_pass_multi_async(rt_group *g, rt_dev_scene *const *scenes, const rt_camera *cam, const rt_params *p,
                               int tile_size, uint32_t s0, uint32_t ns,
                               float *d_rgba /* may be NULL */, float *d_depth /* may be NULL */,
                               uint64_t *d_counters /* may be NULL */, void *stream);
/* Blocking form: rt_render_inw_multi's scenes and group, rt_render_passes_inw's cuts and images (image i
 * at rgba + i * W*H*4, depth + i * W*H; depth may be NULL).  RT_E_ARG also for bad cuts or a bad
 * tile_size. */
int rt_render_passes_inw_multi(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                               uint32_t n_lights, const rt_camera *cam, const rt_params *p, const int *devices,
                               int n_dev, int tile_size, const uint32_t *cuts, int n_cuts,
                               float *rgba /* n_cuts*W*H*4 */, float *depth /* n_cuts*W*H or NULL */, rt_stats *st);

/* Adaptive sample passes on packed tile lists and on device groups: rt_render_pass_pixels_async and
 * rt_pass_select_async with everything indexed by slot, so that a host that deals a frame over several
 * devices stops sampling where the image has settled.  Whether a pixel is active depends only on its own
 * state and aux, so a partition's adaptive loop gives, bit for bit, the single-device loop's image, depth,
 * counts and reference counters.
 *
 * A list entry on a tile list is a slot, slot = tile * T*T + iy * T + ix as in rt_render_pass_tiles_async;
 * RT_SLOT_NONE is the padding value.  Tiles, tile_size and the packed buffers are that call's; p->tile_* is
 * ignored; T need not be a power of two (48 is legal).
 *
 * rt_render_pass_slots_async is rt_render_pass_pixels_async over slots.
 *   - A listed slot is handled when it is below n_tiles * T*T and its pixel (tiles[tile].x * T + ix,
 *     tiles[tile].y * T + iy) lies inside the image.  With c = d_aux_packed[slot].count it renders samples
 *     [c, min(c + ns, S)); the state is continued and not read when c == 0, `even` and count are continued
 *     too; the image acc * RN(1 / c') with alpha 1 and the state's depth (0 on IOW-03) are written to the
 *     slot.  A listed slot with c >= S renders nothing and has its image rewritten from its state.
 *   - Any other entry is skipped: RT_SLOT_NONE, an entry past the list's slots, a slot outside the image.
 *     So a host can launch with the list's full capacity after a select without reading the count back.
 *   - Unlisted slots keep every byte of state, aux, image and depth.  The zero image of the slots outside
 *     the image is never written here: it stays the uniform tile pass's and the tile render's business.
 *   - The list holds no slot twice: the caller's duty, unchecked.
 * A slot inside the image ends byte-equal to what rt_render_pass_pixels_async leaves for its pixel, given the
 * same starting count and ns: state, aux, image and depth.  Counters, options, allocation and
 * synchronisation are the listed passes': [0], [3], [4], [5] (INW) or [0], [4], [5] (IOW-03), summed over a
 * partition's lists and a frame's rounds, are the single-device loop's; the call never synchronises; an INW
 * scene grows its pass workspace on the first call of a list size (rt_debug_adaptive_chunk caps the chunks
 * as it does for pixel lists), IOW-03 allocates nothing.
 *
 * rt_pass_select_tiles_async applies rt_pass_select_async's rule (the same operations in the same order,
 * err = +inf for n < 2, a NaN keeps a slot active) to every slot of the list that lies inside the image.
 * d_slots[0 .. n_active) receives the active slots in the order of the tile passes' units:
 * tile-major, 8x8 blocks row-major inside a tile, pixels row-major inside a block.  The following entries are RT_SLOT_NONE,
 * up to the number of slots inside the image; entries past that keep their bytes.  d_err_packed[slot] gets
 * the estimate of the slots inside the image, the others keep their bytes.  Three launches, no
 * synchronisation; the scene's select scratch grows on the first call of a list size.
 *
 * Both return RT_E_ARG, before a device is touched and with the buffers untouched, for the conditions of
 * rt_render_pass_pixels_async and rt_pass_select_async, null d_tiles, n_tiles <= 0, a tile_size that is not a
 * positive multiple of 16, n_tiles * T*T > 2^31, n_slots > 2^31 or null d_slots with n_slots > 0; then
 * RT_E_UNSUPPORTED for p->show_normal != 0 or a scene an update left without its textures.
 * n_slots == 0 or ns == 0 returns RT_OK and launches nothing. */
#define RT_SLOT_NONE 0xffffffffu
int rt_render_pass_slots_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p,
                               const int *d_tiles, int n_tiles, int tile_size,
                               const uint32_t *d_slots, uint32_t n_slots, uint32_t ns,
                               rt_pass_state *d_state_packed /* n_tiles*T*T */, rt_pass_aux *d_aux_packed /* same */,
                               float *d_out_packed /* may be NULL */, float *d_out_depth_packed /* may be NULL */,
                               uint64_t *d_counters /* may be NULL */, void *stream);
int rt_pass_select_tiles_async(rt_dev_scene *s, const rt_params *p,
                               const int *d_tiles, int n_tiles, int tile_size,
                               const rt_pass_state *d_state_packed, const rt_pass_aux *d_aux_packed,
                               float tol, uint32_t min_samples,
                               uint32_t *d_slots /* n_tiles*T*T */, uint32_t *d_n_active,
                               float *d_err_packed /* may be NULL */, void *stream);
/* One adaptive round of a group's frame.  The deal, the streams, the scene checks and the device-0 pointers
 * are rt_render_pass_multi_async's.  Beside the states the group owns, per device, the aux records of its
 * share, a slot list with its active count, and packed image and depth buffers of the adaptive frame of their
 * own, so that an rt_render_multi_async frame between two rounds disturbs nothing; they are allocated when a
 * deal's first adaptive frame begins.
 * first != 0 begins a frame: every device zeroes its aux and lists every slot of its share that lies inside
 * the image.  A round runs, on every device and its own stream, rt_render_pass_slots_async (ns samples) over
 * the current list and rt_pass_select_tiles_async (tol, min_samples) for the next one, and copies the active
 * count to pinned host memory behind an event.  The grouped send / recv brings the packed image (with d_rgba),
 * the depth (with d_rgba and d_depth), the counts (with d_count: W*H sample counts) and the counters to device
 * 0, where the W x H buffers are unpacked.  Pixels that were not listed keep the values of the round they were
 * last in; nothing depends on slots outside the image.  Image, depth, counts and, summed over the rounds,
 * the counters [0], [3], [4], [5] are byte-equal to the single-device loop's (rt_render_pass_pixels_async +
 * rt_pass_select_async) round for round.
 * THIS CALL BLOCKS in one place: a round with first == 0 waits on the host for the previous round's counts,
 * launches no pass on a device whose list is empty and sizes each device's launches by its count.
 * rt_group_adaptive_active waits for the last round's counts too and returns their sum (RT_E_ARG when the
 * group holds no adaptive frame).
 * first == 0 is RT_E_ARG with nothing launched when the states of the current deal were not left by an
 * adaptive round: no frame was begun, the deal changed, or an rt_render_pass_multi_async pass ran since.
 * Beginning an adaptive frame sets the progressive count to 0, so rt_render_pass_multi_async refuses to
 * continue into it.  The other argument errors, RT_E_UNSUPPORTED and ns == 0 are rt_render_pass_multi_async's;
 * every scene is asked before the group is touched.  Not captured into graphs, as the group passes. */
int rt_render_adaptive_multi_async(rt_group *g, rt_dev_scene *const *scenes, const rt_camera *cam, const rt_params *p,
                                   int tile_size, int first, uint32_t ns, float tol, uint32_t min_samples,
                                   float *d_rgba /* may be NULL */, float *d_depth /* may be NULL */,
                                   uint32_t *d_count /* W*H, may be NULL */, uint64_t *d_counters /* may be NULL */,
                                   void *stream);
int rt_group_adaptive_active(rt_group *g, uint32_t *n_active);   /* waits for the last round's counts; their sum */
/* Blocking form: rt_render_passes_inw_multi's scenes and group, rt_render_adaptive_inw's loop and stopping
 * rule.  rgba, depth, count and rounds_out are byte-equal to rt_render_adaptive_inw's for the whole frame, as
 * are the stats segments, shadow_queries, stack_drops and nan_drops.  err, state_out and aux_out are not
 * offered: fold state does not leave its device.  RT_E_ARG also for batch == 0 or a bad tile_size. */
int rt_render_adaptive_inw_multi(const float *geom, uint32_t n, int layout, const float *nodes, const float *lights,
                                 uint32_t n_lights, const rt_camera *cam, const rt_params *p,
                                 const int *devices, int n_dev, int tile_size,
                                 uint32_t batch, float tol, uint32_t min_samples, uint32_t max_rounds,
                                 float *rgba, float *depth /* or NULL */, uint32_t *count /* or NULL */,
                                 uint32_t *rounds_out, rt_stats *st);

/* ---- progressive display -------------------------------------------------
 * Tile order <- Adding_Materials::OnUpdate  In-One-Weekend/03_Shadows_and_Materials/materials.cpp:84-152:
 * the drawable tiles of the centre-out square spiral over tile_w x tile_h tiles, each as
 * (tx, ty, dispatch_w, dispatch_h); the last tile index of an axis is dispatched W % tile wide
 * (materials.cpp:142-143; 0 when the tile divides W, as in the reference).  Writes up to cap
 * quadruples to out (may be NULL) and returns the number of tiles. */
int rt_tile_spiral(int width, int height, int tile_w, int tile_h, int *out, int cap);
/* One progressive update (OnUpdate with m_NumberOfTilesAtATime = count): renders tiles
 * [first, first + count) of that order into the full W*H device image (p->tile_* ignored).
 * Returns the next cursor (== rt_tile_spiral's count when the frame is complete) or an
 * error. */
int rt_render_spiral_async(rt_dev_scene *s, const rt_camera *cam, const rt_params *p, int tile_w, int tile_h,
                           int first, int count, float *d_rgba, float *d_depth, uint64_t *d_counters,
                           void *stream);
/* Display pass <- the fullscreen-quad blit into the RGBA8 framebuffer
 * (In-Next-Week/01_BoundingVolumeHierarchy/BVH.cpp:6-43; materials.cpp:154-161): the colour
 * image, or with use_depth the depth image as (d, d, d, 1), converted as GL stores unorm8
 * (clamp to [0,1], round to nearest, NaN -> 0).  d_out: W*H*4 bytes. */
int rt_display_rgba8_async(const float *d_rgba, const float *d_depth, int width, int height, int use_depth,
                           uint8_t *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
