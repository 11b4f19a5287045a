/* Diagnostics, bench and test hooks of librt_hip.so: every rt_debug_* entry point.  Not part
 * of the render ABI a host needs (rt_hip.h); the symbols, signatures and struct layouts are
 * covered by the same RT_ABI_VERSION. */
#ifndef RT_HIP_DEBUG_H
#define RT_HIP_DEBUG_H

#include "rt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The path the scene's last render took (bench line): the main kernel as
 * rocprofv3 names it and its launches per frame, the resolved fold order and which exact
 * shortcuts were on for that frame (some are decided per frame: the probe's pick, the fused
 * cull's error bound, the beam lists' memory and geometry conditions).  Synchronises when the
 * fold order was left to the device probe. */
typedef struct rt_path_info {
    char kernel[64];
    int launches;
    int order;            /* INW: 1 pixel-major, 2 sample-major, 3 per-pixel k_inw; IOW-03: 4 sample-parallel, 5 sequential */
    int order_forced;     /* 1 when rt_options.inw_order chose it, 0 when the probe did */
    int wide_walk, beams, ri_grid, fused_cull;
    int lds_nodes;        /* wide BVH nodes staged in LDS (0: none) */
    int claim_order;
    int ring_entries;     /* fold window of the kernel that ran */
    int iow_bvh;          /* IOW-03: 0 linear loop, 1 culling BVH, 2 culling BVH in LDS */
    int ring_lds;         /* 1: the fold ring was in LDS (k_inw_pm: inw_ring_pm = 0; k_inw_sm: inw_ring_sm = 0 and a BVH top of <= 5 nodes) */
    int stackless;        /* 1: the reference LBVH walks ran stackless where no push could drop */
    int lbvh_lds_nodes;   /* LBVH nodes the stackless walks read from LDS (no wide walk) */
    int qnodes;           /* 1: the wide closest-hit walks read quantised nodes (inw_qnodes) */
    int global_stack;     /* 1: the reference's 40-float stacks lived in global memory, not in LDS */
    int walk_stack;       /* entries of the wide walks' own node stack per lane (LDS) */
    uint64_t ref_walks;   /* INW: the last frame's closest-hit queries (segments + shadow rays) that the wide
                             walk or beam list handed to the reference's LBVH walks (stackless or stack) */
    int time_bins;        /* INW: time-bin culling trees the wide closest-hit walks chose from (0: the swept
                             tree; inw_time_bins, moving objects, walks that read no LDS-staged nodes) */
    int beam_bins;        /* INW: beam lists per pixel (one per time bin; 0: one list over the swept boxes) */
    int sphere_records;   /* INW: 1 when the object tests read the sphere records (inw_sphere_records) */
    int beam_prune;       /* INW: what the frame's beam lists left out (inw_beam_prune: 0, 1, or 2 with sphere records) */
} rt_path_info;
int rt_debug_path(rt_dev_scene *s, rt_path_info *out);
/* Sky blocks of the scene's last INW fold render (rt_options.inw_sky_blocks; synchronises): out[0] =
 * 8x8 blocks the classifier flagged (every pixel's beam lists empty and complete), out[1] = those of
 * them k_inw_sky rendered (the others held a ray that fails the beam lists' test and went back to
 * k_inw_pm), out[2] = the frame's blocks.  A frame the path does not apply to reports 0 flagged.
 * s == NULL: the same of the last blocking render (rt_render_inw and its kin build a scene per call). */
int rt_debug_sky_blocks(rt_dev_scene *s, uint32_t out[3]);
/* The beam lists of the scene's last INW fold render (k_inw_beam's output; synchronises): totals =
 * {lists (pixel units, padding included, x time bins), non-empty lists, entries, lists with a cut
 * (some leaf not kept), lists switched off (the wide walk answers), entries a list can hold, 0, 0}.
 * Each of n_out, cut_out (totals[0] values: a list's entry count, or 0xffffffff when switched off;
 * its cut, +infinity when nothing was cut) and entries_out (totals[0] * totals[5] uint64,
 * list l's entries at l * totals[5]: the object id in the low half, the stored key word in the high
 * one -- the float bits of the entry t, or its high 16 bits when entries are packed) may be NULL;
 * cap_lists says how many lists the others hold (RT_E_ARG when too few).  A frame without beam
 * lists, or a sample-major one (no list written), reports totals[0] = 0. */
int rt_debug_beam_lists(rt_dev_scene *s, uint64_t totals[8], uint32_t *n_out, float *cut_out, uint64_t *entries_out,
                        uint32_t cap_lists);
/* k_inw_beam's keep / drop decision for one culling box, on the host (no device; tests): the camera
 * position, the pixel's central direction cd (inw_pixel_dir), aperture and focus distance of the
 * frame, the lens table's largest |x| + |y| (sf_max) and the scene bound (wbound) give the beam as
 * set_beam derives it; box = lo xyz, hi xyz; sph = the object's sphere record (8 floats: position,
 * RN(1 / scale), position - last_position, RI) or NULL; bin of `bins` time bins (bins <= 1: one list
 * over the shutter interval); prune = rt_options.inw_beam_prune.  Returns 1 when the list keeps the
 * leaf, 0 when it does not, RT_E_ARG for a bad argument, RT_E_UNSUPPORTED when this camera gets no
 * beam lists.  *candidate (may be NULL): 1 when the leaf passes the test of prune = 0. */
int rt_beam_keep_host(const float cam_pos[3], const float cd[3], float aperture, float focus, float sf_max,
                      float wbound, const float box[6], const float *sph, uint32_t bin, uint32_t bins, int prune,
                      int *candidate);

/* ---- diagnostics ---------------------------------------------------------------------
 * d_buf: device array of 16 uint64 (or NULL to disable).  While set, the IOW-03 kernel adds
 *   [0..7]  per wave iteration of each phase (outer work loop, BVH walk, postponed-leaf tests,
 *           ray segments): 1 and the number of lanes taking part (lane occupancy);
 *   [8..13] wave shader-clock cycles in: the work loop's camera-ray part, closest-hit queries,
 *           their BVH walk, leaf tests, ray segments, (unused).
 * Diagnostics cost time; never enable them for a measured run. */
int rt_debug_counters(uint64_t *d_buf);
/* d_buf: device array with one uint32 per work unit (or NULL to disable): the IOW-03 kernel
 * writes the rays each pixel cast when the pixel completes (unit = tile-major pixel index in
 * tile mode, 8x8-block-major in rect mode).  The INW fold kernels instead ADD the rays of each
 * output pixel (index = the pixel's position in the output image: y * W + x, or the packed
 * tile index), so the buffer must be zeroed before the render. */
int rt_debug_pixel_rays(uint32_t *d_buf);
/* Lanes parked by each tail-compaction round of the scene's last render (synchronises the
 * device).  Returns the number of rounds written to out (<= cap). */
int rt_debug_rounds(rt_dev_scene *s, uint32_t *out, int cap);
/* Rays per sample over the scene's last sample-parallel IOW-03 render (synchronises):
 * out[0] = max, out[1] = samples, out[2+b] = samples with 2^b <= rays < 2^(b+1),
 * out[34+b] = rays in those samples.  66 entries. */
int rt_debug_spec_hist(rt_dev_scene *s, uint64_t *out);
/* Per pixel unit of the last sample-parallel IOW-03 render, 4 x u32: sample-0 rays, the most
 * rays of one sample, that sample's index, and (column 3 of row r) the pixel at rank r of the
 * heaviest-first order.  Returns the number of units (<= cap_units) or an error. */
int rt_debug_spec_pixels(rt_dev_scene *s, uint32_t *out, uint32_t cap_units);
/* Same 66 x u64 layout as rt_debug_spec_hist, over the samples of group 0's last re-execution
 * list (their final executions). */
int rt_debug_spec_list_hist(rt_dev_scene *s, uint64_t *out);
/* With RT_DEBUG_FIRST_STALE=1 (which repurposes the stack-drop counter): out[b] / out[16+b] =
 * samples / rays of the re-execution list whose first stale stack read came in the b-th 16th
 * of their segments. */
int rt_debug_spec_list_stale(rt_dev_scene *s, uint64_t *out);
/* Rays of every (pixel unit, sample) record of the last sample-parallel IOW-03 render
 * (rays_out[s * P + pu], cap >= P * S), group 0's last re-execution list (up to list_cap
 * units) and dims = {P, S, list count, sequential-leftover count}. */
int rt_debug_spec_dump(rt_dev_scene *s, uint32_t *rays_out, size_t cap, uint32_t *list_out, uint32_t list_cap,
                       uint32_t *dims);
/* With RT_DEBUG_TIMES=1 set before the render: per (pixel unit, sample) record of the last
 * sample-parallel IOW-03 render, start_out[s * P + pu] = launch of the sample's last start
 * (bits 0-15) and its start count (bits 16-31), end_out = launch it finished in (synchronises). */
int rt_debug_spec_times(rt_dev_scene *s, uint32_t *start_out, uint32_t *end_out, size_t cap);
/* Main render kernel of the scene's last render and how many times it was launched (the
 * bench's per-launch roofline figures divide by this).  Returns the count; writes the name. */
int rt_debug_launches(rt_dev_scene *s, char *name_out, int name_cap);
/* Sample chunks of the scene's last render: the sample-parallel paths split the samples into
 * chunks whose records fit the device's free memory (INW: RT_SPEC_MAX_GB), and the per-pixel
 * paths split them by chunk_plan.  1 = one pass over all samples. */
int rt_debug_chunks(rt_dev_scene *s);
/* Kernel timing (diagnostics / bench): with rt_debug_time_kernels(1), every launch of the main
 * sample-parallel IOW-03 kernel (rt_debug_launches' name) is bracketed by HIP events on its
 * stream; rt_debug_kernel_time returns the summed durations and the launch count of the
 * scene's last render (waits for it). */
int rt_debug_time_kernels(int on);
/* Numerics self-check of the shortened correctly rounded sequences in rt_math.hpp against the
 * compiler's, for all 2^32 float bit patterns x: which 0 = rcp_sqrt_domain(sqrtf(x)) (the
 * reciprocal normalize() uses) vs 1.0f / sqrtf(x); other values are RT_E_ARG.
 * Writes the mismatch count and the lowest mismatching x (0xffffffff if none); synchronous. */
int rt_debug_check_fastmath(int which, uint64_t *mismatches, uint32_t *first_bad);
int rt_debug_kernel_time(rt_dev_scene *s, double *ms_total, int *launches);
/* The INW scene's walk structures (synchronises): info = {wide nodes, dfs_high, wide depth, RI grid
 * built, RI cells, stackless layout, objects, where the walk structures were built: 0 host, 1 device,
 * 2 host after the device build ran past its level cap}; rank_out (2n, may be NULL) receives the objects'
 * depth-first ranks (invert 0, then 1) when the wide walk is built.  Lets the tests compare the
 * device build (rt_dev_scene_inw_update) with the host build of a fresh scene. */
int rt_debug_wide_info(rt_dev_scene *s, uint32_t info[8], uint32_t *rank_out);
/* 1 when the scene's ray, path and pixel queries and passes launch the fused-cull instance of their
 * kernel (rt_options.inw_fused_cull, a wide tree, every culling box within 1000 of the origin), else 0;
 * RT_E_ARG for a null or IOW-03 scene.  The decision the launches themselves take. */
int rt_debug_query_fused(rt_dev_scene *s);
/* Test hook: the device build of the walk structures (rt_dev_scene_inw_update) and of the IOW-03
 * culling BVH (rt_dev_scene_iow03_update) launches at most `levels` SAH / collapse levels (0 = its own
 * cap, 256); a deeper tree is built on the host instead (rt_debug_wide_info info[7] = 2,
 * rt_debug_iow_info info[3] = 2), which lets a test reach that fallback with an ordinary scene. */
int rt_debug_build_level_cap(int levels);
/* Test hooks for the host build of the time-bin culling trees and the sphere records (no device;
 * DESIGN.md §5.2).  rt_debug_time_bins builds the wide walk's trees from the reference's LBVH nodes
 * and GeometryBuff records (28 floats each) with `bins` time bins and copies the 4-wide nodes (40
 * floats each, links as int bits) into wnodes_out when wnodes_cap holds them; info = {nodes of the
 * swept tree, bins built (1: none), nodes per bin tree, all nodes}.  rt_debug_bin_boxes writes the
 * culling boxes (lo xyz, hi xyz per object) of bin b of `bins`.  rt_debug_sphere_records writes the
 * 3-float4 sphere records (12 floats per object) and returns 1, or 0 when some object does not
 * qualify. */
int rt_debug_time_bins(const float *nodes, const float *geom, uint32_t n, uint32_t bins, float *wnodes_out,
                       uint32_t wnodes_cap, uint32_t info[4]);
int rt_debug_bin_boxes(const float *geom, uint32_t n, uint32_t bins, uint32_t b, float *boxes_out);
int rt_debug_sphere_records(const float *geom, uint32_t n, int layout, float *out);
/* Objects inside their leaf boxes: how far, at most, an object of the GeometryBuff
 * records sticks out of its box over the shutter interval, as a multiple of the margin up to which
 * a scene takes the wide walk (1e-5 * max(1, largest |coordinate| of the box)); > 1: the scene is
 * built as with inw_wide_walk = 0.  The boxes are the leaves of `nodes` ((2n - 1) x 8), or with
 * nodes = NULL the rows of aabbs (n x 6).  *worst_out is +inf for a value that is not finite. */
int rt_debug_inw_stick_out(const float *geom, uint32_t n, const float *nodes, const float *aabbs, double *worst_out);
/* Read-back hooks for the culling and bookkeeping structures (tests/test_walk_structs.py,
 * tests/test_gpu_walk_structs.py check each one directly against DESIGN.md §2's "every structure is
 * conservative").  None of them changes what a render path builds or reads.
 *
 * rt_debug_walk_dump synchronises and copies one structure of an INW device scene out exactly as the
 * kernels read it.  info[0] = its size in bytes, info[1..] as listed; with out == NULL only info is
 * written, otherwise cap_bytes must hold the structure (RT_E_ARG if not).  A structure the scene does
 * not have (no wide walk, RI grid dropped) has size 0. */
#define RT_WALK_WNODES   0  /* 10 float4 per node; info = {bytes, nodes, n_wtree0, wbins, wbin_stride, depth} */
#define RT_WALK_CNODES   1  /* 7 float4 per node; info = {bytes, nodes} */
#define RT_WALK_QNODES   2  /* info[2] float4 per node; info = {bytes, nodes, float4 per node} */
#define RT_WALK_LEAFBOX  3  /* 2 float4 per object (its LBVH leaf node); info = {bytes, objects} */
#define RT_WALK_LBVH     4  /* 2 float4 per LBVH node; info = {bytes, 2 * objects - 1} */
#define RT_WALK_RI_CELLS 5  /* uint32 cell offsets (cells + 1); info = {bytes, cells, RI grid built} */
#define RT_WALK_RI_IDS   6  /* uint32 object ids; info = {bytes, ids} */
#define RT_WALK_RI_FRAME 7  /* float lo[3], hi[3], inv[3], int32 dim[3] as the kernels get them; info = {bytes} */
#define RT_WALK_WBOUND   8  /* one float; info = {bytes} (ranks and dfs_high: rt_debug_wide_info) */
#define RT_WALK_HOT      9  /* the hot records; info = {bytes, objects, floats per object} */
#define RT_WALK_COLD    10  /* the cold records; info = {bytes, objects, floats per object} */
#define RT_WALK_SPH     11  /* the sphere records (size 0 unless every object is an unrotated sphere); info as above */
int rt_debug_walk_dump(rt_dev_scene *s, int what, void *out, size_t cap_bytes, uint64_t info[8]);
/* {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} of the kernels of
 * rt_dev_scene_inw_update_device and rt_inw_swept_boxes_async: k_inw_prepare (which = 0), k_bin_boxes (1),
 * k_swept_boxes (2), k_bin_place (3). */
int rt_debug_update_kernel(int which, int info[4]);
/* The host builders' full output, no device: rtamd::inw_wide_build and ri_grid_build over the
 * reference's LBVH nodes ((2n-1) x 8).  info = {wide nodes, dfs_high, wide depth, RI grid built, RI
 * cells, RI ids, wbound as float bits, 0} (zeros when the LBVH is not walkable).  Every array may be
 * NULL; one that is not must hold what info reports (wnodes: 40 floats per node; leafbox: 8n; rank:
 * 2n; ri_cells: cells + 1; ri_ids; ri_frame: lo[3] hi[3] inv[3]; ri_dim[3]). */
int rt_debug_inw_host_dump(const float *nodes, uint32_t n, uint32_t info[8], float *wnodes, float *leafbox,
                           uint32_t *rank, uint32_t *ri_cells, uint32_t *ri_ids, float ri_frame[9], int32_t ri_dim[3]);
/* The same for rtamd::iow_cull_build: info = {wide nodes (0: linear loop), 0, 0, 0}; wide: 32 floats
 * per node (6 float4 of SoA child planes, the links as int bits, one unused float4); obox: 6n floats as
 * the kernels read them ((lo xyz, hi x) per object, then (hi y, hi z) per object). */
int rt_debug_iow_host_dump(const float *types, const float *records, uint32_t n, uint32_t info[4], float *wide,
                           float *obox);
/* The IOW-03 scene's culling structures: info = {objects, wide nodes (0 = linear loop), wide depth,
 * where built (0 host, 1 device, 2 host after the device build ran past its level cap, 3 host because
 * a box was not finite), the LDS-staged kernel instances apply (0/1), successful
 * rt_dev_scene_iow03_update calls so far, 0, 0}.  No device work. */
int rt_debug_iow_info(rt_dev_scene *s, uint32_t info[8]);
/* The scene's culling BVH and object boxes as the kernels read them (synchronises), in exactly the
 * layout of rt_debug_iow_host_dump: info = {wide nodes (0: linear loop), 0, 0, 0}; wide and obox may
 * be NULL.  (rt_debug_walk_dump keeps refusing IOW-03 scenes.) */
int rt_debug_iow_dump(rt_dev_scene *s, uint32_t info[4], float *wide, float *obox);
/* The IOW-03 record packer and RI priors as rt_dev_scene_iow03 runs them on the host, no device: hot (n *
 * 20 floats: pos3 type M9 scale3 1/scale3 identity flag), cold (n * 8: colour3 material3 scat2) and
 * priors = {ri_prior (the most common RefractiveIndex, record float 20; the smallest among equals),
 * alt_vals[8] (the ascending distinct bit patterns of {0, 1} and the RIs when there are at most 8; 0
 * past the count), n_alt_vals as a float}.  Each output may be NULL.  RT_E_ARG for null inputs or
 * n == 0.  What rt_dev_scene_iow03_update_device's kernels must reproduce byte for byte. */
int rt_debug_iow_prepare_host(const float *types, const float *records, uint32_t n, float *hot, float *cold,
                              float priors[10]);
/* The scene's current hot records, cold records and priors in the same layouts (synchronises; each
 * output may be NULL).  RT_E_ARG for a null, INW or broken scene. */
int rt_debug_iow_records(rt_dev_scene *s, float *hot, float *cold, float priors[10]);
/* {VGPRs, scratch bytes, static LDS bytes, resident blocks per CU} of the kernels of
 * rt_dev_scene_iow03_update_device: k_iow_prepare with float4 loads (which = 0) and with scalar loads
 * (1), k_iow_mode (2), k_iow_priors (3; one 64-lane block).  Needs a device. */
int rt_debug_update_iow_kernel(int which, int info[4]);
/* The ray-query kernel (rt_trace_rays_async) as the loaded code object has it: info = {VGPRs,
 * scratch bytes per lane, static LDS bytes per block, resident 256-lane blocks per CU} of the
 * closest-hit (any = 0) or RT_TRACE_ANY instance, with the fused cull or without.  Needs a device. */
int rt_debug_trace_kernel(int any, int fused, int info[4]);
/* The same for the IOW-03 ray-query kernel (rt_trace_iow_rays_async): lds = 1 the instance with
 * the BVH staged in LDS, 0 the one that reads nodes from global memory (also the linear loop's). */
int rt_debug_trace_iow_kernel(int any, int lds, int info[4]);
/* The same for the path-query kernel (rt_path_rays_async): lights = 1 the INW-04 instance, 0 the
 * INW-01 one, with the fused cull or without. */
int rt_debug_paths_kernel(int lights, int fused, int info[4]);
/* Caps the path-query kernel's grid at `blocks` 256-lane blocks (0 = the default, the resident
 * grid), so that a test can make one block answer many queries.  Returns the previous cap. */
int rt_debug_paths_max_blocks(int blocks);
/* The same pair for the IOW-03 path-query kernel (rt_path_iow_rays_async): lds_nodes = 1 the instance
 * with the BVH staged in LDS, 0 the one that reads nodes from global memory (also the linear
 * loop's); the cap counts 256-lane blocks, each lane of which owns one chain at a time. */
int rt_debug_path_iow_kernel(int lds_nodes, int info[4]);
int rt_debug_path_iow_max_blocks(int blocks);
/* The same for the pixel-query kernels (rt_camera_rays_async, rt_pixel_query_async): which = 0
 * k_camera_rays on an INW scene, 1 on an IOW-03 scene, 2 k_pixel_fold INW, 3 IOW-03 (blocks of 256
 * lanes: 256 records of rays, four pixels of the fold).  RT_E_ARG for any other `which`. */
int rt_debug_pixels_kernel(int which, int info[4]);
/* The same pair for the progressive-pass kernels (rt_render_pass_async).  An INW pass is the camera
 * rays of its samples, the path-query kernel (rt_debug_paths_kernel) and the fold: which = 0 is
 * k_pass_rays, 1 k_pass_fold, both serving INW-01 and INW-04 alike; 2 is the IOW-03 kernel with the BVH
 * staged in LDS, 3 the one that reads nodes from global memory (also the linear loop's).  RT_E_ARG for
 * any other `which`.  The cap counts 256-lane blocks of the kernels that own a lane per path or pixel
 * (INW: the path-query kernel's grid during a pass; IOW-03: k_iow_pass's); rt_debug_pass_max_blocks
 * returns the previous cap.
 *
 * The tile-list instances of these kernels (rt_render_pass_tiles_async) answer to rt_debug_pass_kernel
 * too: which = 16 is k_pass_rays, 17 k_pass_fold, 18 k_iow_pass with the BVH staged in LDS, 19 the one
 * that reads nodes from global memory.  (4..7 and 15 stay RT_E_ARG: hosts and tests rely on it.)
 * rt_debug_pass_max_blocks caps their grids as it caps the rectangle passes'. */
int rt_debug_pass_kernel(int which, int info[4]);
int rt_debug_pass_max_blocks(int blocks);
/* The adaptive-pass kernels (rt_render_pass_pixels_async, rt_pass_select_async) answer to
 * rt_debug_pass_kernel as well: which = 8 is k_adapt_rays, 9 k_adapt_fold (both INW), 10 the IOW-03 kernel
 * k_iow_adapt with the BVH staged in LDS, 11 the one that reads nodes from global memory, 12 k_select_count,
 * 13 k_select_scan, 14 k_select_scatter.  (4..7 stay RT_E_ARG, as every value past 3 was before these
 * kernels existed.)  rt_debug_pass_max_blocks also caps the grids of a listed pass.
 * rt_debug_adaptive_chunk caps the samples of one chunk of an INW listed pass (0 = the default: as many as
 * the workspace rule allows), so that a test can make a small pass run in several chunks; it returns the
 * previous cap.
 *
 * The tile-list instances of the adaptive kernels (rt_render_pass_slots_async, rt_pass_select_tiles_async)
 * are an adaptive kernel's `which` + 16, as 16..19 are 0..3 + 16: which = 24 is k_adapt_rays, 25 k_adapt_fold,
 * 26 k_iow_adapt with the BVH staged in LDS, 27 the one that reads nodes from global memory, 28
 * k_select_count, 30 k_select_scatter.  k_select_scan (13) serves both forms, so 29 is RT_E_ARG, as 20..23
 * and every value past 30 are.  Both caps apply to a listed pass over slots as to one over pixels. */
int rt_debug_adaptive_chunk(int samples);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_DEBUG_H */
