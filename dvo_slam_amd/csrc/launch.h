// launch.h -- host-callable launchers of the gfx950 kernels (one per .hip translation unit).
#pragma once

#include <hip/hip_runtime.h>

#include "device_types.h"

namespace dvo_hip {

struct RefOrderSeg;
struct RefOrderPair;
struct RefOrderPlane;   // (ref_order.h)

// pyramid_kernels.hip
// raw ingest + pyramid levels 1..3 in one pass (levels beyond the fourth: launch_pyr_down)
void launch_pyr_down(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h);
// max_workgroups > 0 caps the grid (the kernels walk the tiles with a grid stride): background build next to an alignment
// level 0 in role `role` (-1 none, 0 current, 1 reference) + pyramid levels 1..3 straight from raw planes; `strips`: through the strip
// ingest (ingest_strips.hip; the caller asks ingest_strips_supports once and counts and plans by the same answer), else in 64 x 16 tiles
// cur_flavor (role 0): which planes of the current role are written, kCurAB | kCurC (device_types.h)
// c_levels: bit l set = pyramid level l (1..3) also gets the current role's {I, Z} plane C in the same pass (with `strips` only)
// colour_channels: 0 = grey planes, 3 / 4 = every frame's colour plane (FrameBuildPtrs::colour) with that many bytes per pixel,
// kChF32 = a float image plane there; depth_f32: float depth planes (FrameBuildPtrs::depth_f32) instead of the u16 ones
// stream_nt: the strip kernels read the raw planes and write the planes of levels 0-1 with the non-temporal policy (global_ptr.h; the
// option "stream_policy" for the build stream's launches)
void launch_build_from_raw(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, float scale, int w0, int h0, int levels, int role, bool strips,
                           float ithr, float dthr, int max_workgroups, int cur_flavor = kCurAB, int c_levels = 0, int colour_channels = 0,
                           bool stream_nt = false, bool depth_f32 = false);
// ingest_strips.hip: the role planes of one level from the float planes I / Z in strips (even widths); role 1: counters zeroed before
bool derive_strips_supports(int w);
void launch_derive_strips(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h, int role, float ithr, float dthr,
                          int max_workgroups, int cur_flavor, bool stream_nt = false);
// ingest_strips.hip: the same pass with one 128 x 8 strip per wavefront, registers only (even widths, aligned planes)
// wide: every plane's address and pitch suit the strip loads (f32_strips_aligned, colour_strips_aligned; 8-bit grey and u16 depth: 4-pixel
// groups).  f32_image: the image plane is float (with float depth): every even width qualifies, the 8-bit planes want a multiple of 4
bool ingest_strips_supports(int w0, bool wide, bool f32_image = false);
// a float plane's share of `wide`: address and row pitch are 8-byte aligned (a lane loads its pixel pair in one piece)
bool f32_strips_aligned(const void* plane, size_t pitch);
// a colour plane's share of `wide`: its address and row pitch suit the strip kernel's loads for `channels` bytes per pixel
bool colour_strips_aligned(const void* colour, size_t pitch, int channels);
// colour_channels: 0 = the grey plane of every frame, 3 / 4 = the colour plane (FrameBuildPtrs::colour) with that many bytes per pixel,
// kChF32 = a float image plane there; depth_f32: the depth plane is FrameBuildPtrs::depth_f32 (always so with a float image)
void launch_ingest_strips(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, float scale, int w0, int h0, int levels, int role,
                          float ithr, float dthr, int max_workgroups, int cur_flavor, int c_levels, int colour_channels = 0, bool stream_nt = false,
                          bool depth_f32 = false);
// the role planes of one level from the float planes I / Z: the strips at even widths, launch_derive_levels over the one level at odd ones
void launch_derive_current(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h, int max_workgroups, int cur_flavor = kCurAB,
                           bool stream_nt = false);
// mode 0: A + B from C; 1: C from A; 2: R + selection count from C (the level's counters are zeroed first)
void launch_from_current_plane(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h, int mode, float ithr, float dthr,
                               int max_workgroups);
void launch_derive_reference(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h, float ithr, float dthr,
                             int max_workgroups, bool stream_nt = false);
// the role planes (role 0: current, flavours per level in span.flavor; role 1: reference, counters zeroed here) of the levels
// span.l0 .. span.l1 in one launch of 64 x 16 tiles
void launch_derive_levels(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, const LevelSpan& span, int role, float ithr, float dthr,
                          int max_workgroups);
void launch_select_pack(hipStream_t s, const float4* A, const float2* B, int n, float ithr, float dthr, float2* R, int* count, uint8_t* mask);
// the levels l0 .. l1 of a camera (w, h: indexed by level) as a span; tile0 = offsets of each level's 64 x 16 tiles (k_derive_levels), or
// with pixel_blocks of its 512-pixel blocks (k_apply_selection).  flavor: zero, the caller's to set
LevelSpan level_span(int l0, int l1, const int* w, const int* h, bool pixel_blocks = false);
// the caller selection (selection.h) over the reference planes R of levels span.l0 .. span.l1 of n frames, one launch (a pixel_blocks span)
void launch_apply_selection(hipStream_t s, const SelectionApply* tbl, int n_frames, const LevelSpan& span, int max_workgroups);
// an explicit accepted set of one level: R = {Z where accepted[i] != 0, else NaN; I}, count = accepted entries (zeroed before)
void launch_pack_accepted(hipStream_t s, const float4* A, const uint8_t* accepted, int n, float2* R, int* count);
void launch_unpack_plane(hipStream_t s, const float4* A, const float2* B, int n, int plane, float* out);

// rectify.hip: the raw planes of n frames through one lens into their float planes I / Z of level 0 (lens.h).  channels: 0 = grey8, 3 / 4 =
// a colour plane with that many bytes per pixel, kChF32 = a float image; depth_f32: float depth planes, else u16.  stream_nt: raw planes
// read and float planes written with the non-temporal policy (option "stream_policy")
void launch_rectify(hipStream_t s, const RectifyPtrs* tbl, int n_frames, const RectifyArgs& a, int channels, bool depth_f32, int max_workgroups,
                    bool stream_nt);

// depth_register.hip: the depth planes of n frames through one depth rig into their float plane Z of level 0 (depth_rig.h): a fill of
// the z-buffers with the hole pattern, then the forward scatter with an atomic minimum.  depth_f32: float depth planes, else u16.
// stream_nt: the depth planes are read with the non-temporal policy (option "stream_policy"); the z-buffer is written at the default one
void launch_depth_register(hipStream_t s, const DepthRigPtrs* tbl, int n_frames, const DepthRigArgs& a, bool depth_f32, int max_workgroups,
                           bool stream_nt);

// depth_filter.hip: the depth planes of n frames through one depth filter (depth_filter.h) into their filter planes: flying pixels and
// hole borders rejected, noise smoothed.  depth_f32: float depth planes, else u16.  stream_nt: the source planes are read and the filter
// planes written with the non-temporal policy (option "stream_policy")
void launch_depth_filter(hipStream_t s, const DepthFilterPtrs* tbl, int n_frames, const DepthFilterArgs& a, bool depth_f32, int max_workgroups,
                         bool stream_nt);

// sensor_convert.hip: the sensor planes (Bayer mosaics, YUV 4:2:2) of n frames of one size into tight planes of grey (packed false: the
// ingest's pre-pass) or of packed pixels (packed true: dvo_hip_frames_set_colour), sensor_formats.h.  a.src_dwords / a.dst_wide: what
// sensor_src_dwords and the caller's look at the destinations say.  stream_nt: planes read and written with the non-temporal policy
bool sensor_src_dwords(const void* plane, size_t pitch);
void launch_sensor_convert(hipStream_t s, const SensorPtrs* tbl, int n_frames, const SensorArgs& a, bool packed, int max_workgroups, bool stream_nt);

// the grid of a kernel that walks `total` tiles with a grid stride: a workgroup per tile, or max_workgroups of them where that cap is set
// (> 0: a background build next to an alignment) and lower
inline int capped_grid(long long total, int max_workgroups) { return int(max_workgroups > 0 && total > max_workgroups ? max_workgroups : total); }

// the grid of a kernel that walks `items` elements with a grid stride, 256 per workgroup: 1 .. 8192 workgroups
inline int stride_grid(unsigned long long items) {
  const unsigned long long blocks = (items + 255) / 256;
  return int(blocks < 1 ? 1 : blocks > 8192 ? 8192 : blocks);
}

// cloud_map.hip: the keyframe map (cloud_map.h).  tbl: n_frames entries and one more whose first_block is total_blocks, the launch's grid.
// launch_world_points: every frame's organised cloud into MapFrame::out.  launch_map_insert: every usable pixel into the table m (with the
// wavefront's run folding unless the library was built with DVO_MAP_COMBINE_RUNS=0: map_insert_combines_runs); mixed: the frames carry
// signs (MapFrame::sign), those with -1 are removed.  launch_map_extract: the occupied slots into xyzi / counts / keys / rgba (null: not
// wanted; xyzi null: count only), at most max_points; zeroes and then sets the counters kMapCntCursor (live slots seen), kMapCntOverLimit
// and -- counting only -- kMapCntVacant.  launch_map_clear: keys empty, sums and all counters zero.
// launch_map_rehash: clears `to` (its counters too) and places every live slot of `from` in it; to's kMapCntOccupied and kMapCntDropped
// (records without a slot) say how that went.
// A COLOURED map (m.colour is its side table, every MapFrame carries a plane of packed pixels; cloud_colour.h) takes the same launches:
// they carry the colour sums along, resp. handle the side table, wherever the table has one; rgba is written for a coloured map only.
void launch_world_points(hipStream_t s, const MapFrame* tbl, int n_frames, int total_blocks, float min_depth, float max_depth);
void launch_map_insert(hipStream_t s, const MapFrame* tbl, int n_frames, int total_blocks, const MapTable& m, float min_depth, float max_depth, bool mixed);
void launch_map_rehash(hipStream_t s, const MapTable& from, const MapTable& to);
bool map_insert_combines_runs();
hipError_t launch_map_extract(hipStream_t s, const MapTable& m, unsigned long long max_points, float4* xyzi, uint32_t* counts, unsigned long long* keys,
                              uint32_t* rgba, float4* normals = nullptr);
void launch_map_clear(hipStream_t s, const MapTable& m);
// A map WITH NORMALS (m.normals is its side table; cloud_normal.h) takes the same launches too: k_map_insert forms every valid pixel's
// normal and carries its sums along, clear and rehash handle the side table, `normals` (16-byte records) is written for such a map only.
// cloud_normal.hip, launch_frame_normals: every frame's organised plane of world normals {N.x, N.y, N.z, has} into MapFrame::out.
void launch_frame_normals(hipStream_t s, const MapFrame* tbl, int n_frames, int total_blocks, float min_depth, float max_depth);

// map_merge.hip: voxel tables and record arrays into and out of a map (cloud_map.h, Merge).  tbl: n_entries entries and one more whose
// first_block is total_blocks, the launch's grid.  launch_map_merge: every live record of every entry into (sign +1) or out of (-1) the
// table m, which has a side table iff the entries carry colour records; posed: under each entry's pose, binned anew with m.leaf.
// launch_map_export: the live slots of m as raw records (and colour records at the same indices, where m has a side table and colour is
// given; likewise normal records where m has normals and `normals` is given), at most max_records; records null: count only.  Zeroes and then sets kMapCntCursor (live slots seen).
void launch_map_merge(hipStream_t s, const MapMergeEntry* tbl, int n_entries, int total_blocks, const MapTable& m, bool posed);
hipError_t launch_map_export(hipStream_t s, const MapTable& m, unsigned long long max_records, MapSlot* records, MapColourSlot* colour,
                             MapNormalSlot* normals = nullptr);

// cloud_colour.hip: the colour planes of frames (cloud_colour.h).  launch_colour_pack: n_planes 8-bit colour planes of one pixel format
// into planes of packed pixels (tbl: n_planes entries and one more whose first_block is total_blocks).  launch_colour_level: the
// level-`shift` colour plane (w x h, tight) of a level-0 plane of packed pixels with rows of `pitch` dwords.
void launch_colour_pack(hipStream_t s, const ColourPlane* tbl, int n_planes, int total_blocks, int pixel_format);
void launch_colour_level(hipStream_t s, const uint32_t* plane, int pitch, int shift, int w, int h, uint32_t* out);

// map_render.hip: views of the keyframe map (map_render.h).  n_views views of `pixels` = w * h pixels each; zbuf: pixels * n_views
// elements.  launch_render_fill: every element ~0.  launch_render_splat: every voxel of the table into every view, an atomic minimum per
// covered pixel.  launch_render_resolve: the z-buffers into the planes out[view].  launch_map_render: the three, in that order.
// colour: a colour view of a coloured map (cloud_colour.h): the element's low half is the voxel's colour, out[view].I holds the address
// of the uint32 rgba plane
void launch_render_fill(hipStream_t s, unsigned long long* zbuf, long long elements);
void launch_render_splat(hipStream_t s, const MapTable& m, const MapView* views, int n_views, const RenderArgs& a, unsigned long long* zbuf, bool colour);
void launch_render_resolve(hipStream_t s, const unsigned long long* zbuf, const RenderPlanes* out, int n_views, long long pixels, bool colour);
void launch_map_render(hipStream_t s, const MapTable& m, const MapView* views, const RenderPlanes* out, int n_views, long long pixels, const RenderArgs& a,
                       unsigned long long* zbuf, bool colour);
// a normals view of a map with normals (cloud_normal.h): the element's low half is the voxel's quantised world normal, out[view].I holds
// the address of the plane of 16-byte records {n.x, n.y, n.z, has} in the view's camera coordinates.  The same three launches.
void launch_map_render_normals(hipStream_t s, const MapTable& m, const MapView* views, const RenderPlanes* out, int n_views, long long pixels,
                               const RenderArgs& a, unsigned long long* zbuf);
bool map_render_preloads();

// frame_warp.hip: frames warped under a pose (frame_warp.h).  launch_warp_inverse: n items; tbl holds 2n (+ 1) entries, entry 2i the
// raster frame with the item's transform as its pose, entry 2i + 1 the sampled frame (same w and h); the planes of item i into outs[i];
// max_pixels: the largest w * h of the items.  launch_warp_forward: n items of `pixels` = w * h pixels each (tbl[i]: the source frame, its
// pose the transform) into the z-buffers zbuf (pixels * n elements, filled by launch_render_fill, resolved by launch_render_resolve).
void launch_warp_inverse(hipStream_t s, const MapFrame* tbl, const WarpPlanes* outs, int n, long long max_pixels, float margin);
void launch_warp_forward(hipStream_t s, const MapFrame* tbl, int n, long long pixels, int mode, float min_depth, float max_depth,
                         unsigned long long* zbuf);

// covisibility.hip: keyframe covisibility (covisibility.h).  n pairs over the frame table tbl (every pair's a and b index it; no pose of
// it is read); max_pixels: the largest w * h of the pairs' a; records: n records of four 64-bit words (dvo_hip_covis_record), 8-byte
// aligned and ZEROED on the stream s before the launch, which only adds to them.
void launch_covisibility(hipStream_t s, const MapFrame* tbl, const CovisPair* pairs, int n, long long max_pixels, const dvo_hip_covis_params& par,
                         unsigned long long* records);

// keyframe_codes.hip: keyframes retrieved by appearance (keyframe_codes.h).  launch_encode_frames: the codes of the n frames of the frame
// table tbl under the m ferns at `ferns` (16-byte aligned), m / 8 words each, into codes_out (4-byte aligned).  launch_code_search: the
// n_queries x n uint16 distances of the queries (n_queries codes, 16-byte aligned) to the n stored codes (entry-major, 16-byte aligned;
// live: a byte per entry; skip: n_queries pairs {from, to}, 8-byte aligned), 0xFFFF for a dead or skipped entry; n >= 1.
// launch_code_topk: per row of that matrix the k least (distance, id) into rows (n_queries x k, padded); n may be 0.
// launch_gather_codes: the codes of entries ids[0 .. n) into out.
void launch_encode_frames(hipStream_t s, const MapFrame* tbl, int n, const dvo_hip_fern* ferns, int m, uint32_t* codes_out);
void launch_code_search(hipStream_t s, const uint32_t* codes, const unsigned char* live, uint32_t n, int m, const uint32_t* queries, int n_queries,
                        const uint32_t* skip, uint16_t* distances);
void launch_code_topk(hipStream_t s, const uint16_t* distances, uint32_t n, int n_queries, int k, dvo_hip_code_match* rows);
void launch_gather_codes(hipStream_t s, const uint32_t* codes, const uint32_t* ids, int n, int m, uint32_t* out);

// pose_graph.hip: the stages of the pose-graph optimiser (pose_graph.h), kPgBlock edges or vertices per workgroup.  *_partials: one
// double per workgroup, a subtree of the scalar's tree (rz_partials: two rows of them).  launch_pg_linearise: every edge's record at
// `poses` (with_blocks: the weighted blocks too) and the partials of the cost.  launch_pg_gather: D and b of every vertex and each
// workgroup's largest diagonal entry.  launch_pg_cg_init: the preconditioner and the start of a solve (st cleared by the caller).
// launch_pg_multiply / launch_pg_cg_update: iteration `it` of the solve; both return at once when it has ended (given: the multiply of
// the p stored at kPgP0, the test hook).  launch_pg_apply: the step into `out`.  launch_pg_reduce: out[0], out[1] = the trees over a, b.
struct PgGraph;
struct PgCgState;
void launch_pg_linearise(hipStream_t s, const PgGraph& g, const double* poses, bool with_blocks, double* cost_partials);
void launch_pg_gather(hipStream_t s, const PgGraph& g, double* max_partials);
void launch_pg_cg_init(hipStream_t s, const PgGraph& g, PgCgState* st, double lambda, double* rz_partials);
void launch_pg_multiply(hipStream_t s, const PgGraph& g, PgCgState* st, const double* rz_partials, double* pap_partials, int it, double lambda,
                        double tolerance, bool given);
void launch_pg_cg_update(hipStream_t s, const PgGraph& g, PgCgState* st, const double* pap_partials, double* rz_partials, int it);
void launch_pg_apply(hipStream_t s, const PgGraph& g, double lambda, const double* poses, double* out, double* scale_partials);
void launch_pg_reduce(hipStream_t s, const double* a, int n_a, const double* b, int n_b, double* out);
// the resident schedule: n_graphs resident-sized graphs, each optimised from start to end by one workgroup of one launch.  outs: one per
// graph; records: max_records per graph, the first of its trials; stage_bytes: the LDS a workgroup gets to keep its graph's solve in
// (pose_graph.h: pg_resident_stage_bytes of the largest graph that is to be staged, at most kPgResidentStageBytes)
struct PgResidentJob;
struct PgResidentOut;
struct PgResidentIteration;
void launch_pg_resident(hipStream_t s, const PgResidentJob* jobs, int n_graphs, PgResidentOut* outs, PgResidentIteration* records, int max_records,
                        size_t stage_bytes);

// align_kernels.hip: the sweep of one level, by the kernel its SweepChoice names (sweep_choice.h; rows_per_wave: the plan's tile height,
// choice.tile_rows where the kernel insists on one).  Same outputs whatever the kernel.
// `tail` (non-null; only where sweep_has_tail says so): the workgroup that completes the last tile of a pair runs the pair's solver step
// in the sweep's launch (solver_step.h) -- no launch_solver_step behind it
void launch_residual_reduce(hipStream_t s, const SweepChoice& choice, int rows_per_wave, bool finest_level, const LevelGeom& g, const PairPtrs* pairs,
                            const PairState* states, int n_pairs, float* partials, float2* scratch, unsigned long long* window_fallbacks = nullptr,
                            int* f16_range_flag = nullptr, const SolverStepArgs* tail = nullptr);
// align_mfma.hip: Gram accumulation on the matrix cores.  mode 0: f32 Gram (the f32 matrix instruction); 1: Gram accumulation on the f16
// matrix pipe (gram_f16.h; variant 7); 2: 1 with the contracted per-pixel arithmetic of align_fast.hip (variants 8 / 9 on the levels the
// window sweep does not take)
void launch_residual_reduce_mfma(hipStream_t s, int rows_per_wave, bool finest_level, const LevelGeom& g, const PairPtrs* pairs,
                                 const PairState* states, int n_pairs, float* partials, float2* scratch, int mode = 0,
                                 int* f16_range_flag = nullptr, const SolverStepArgs* tail = nullptr);
// align_window.hip: variants 6 (f32 Gram) and 7 (f16 hi/lo Gram) -- the current frame's {I, Z} window staged in LDS; tiled levels whose
// width is a multiple of 64 only, tile height 16 (rows_per_wave 4).  fallback_count (may be null): lanes
// whose taps fell outside the staged window and were fetched from memory.  f16_range_flag (may be null; pinned host memory): set
// to 1 by a workgroup of variant 7 whose Jacobian components left the f16 range -- the caller repeats the work with variant 6.
void launch_sweep_window(hipStream_t s, bool f16, const LevelGeom& g, const PairPtrs* pairs, const PairState* states, int n_pairs,
                         float* partials, float2* scratch, unsigned long long* fallback_count, int* f16_range_flag = nullptr);
// align_fast.hip: variants 8 / 9 -- the window sweep with contracted per-pixel arithmetic (same function, rounding differences of a few
// ulp against variants 6 / 7; window 84 x 28 cells at a pitch of 96; operand_store 2: high and low operand parts take turns in the slab,
// 1: side by side, moved with v_permlane32_swap).
void launch_sweep_fast(hipStream_t s, int operand_store, const LevelGeom& g, const PairPtrs* pairs, const PairState* states, int n_pairs,
                       float* partials, float2* scratch, unsigned long long* fallback_count, int* f16_range_flag = nullptr,
                       const SolverStepArgs* tail = nullptr);
// align_small.hip: a level small enough for the whole current plane C to live in LDS ((w + 2) x (h + 2) cells of 8 B <= 43 KB, even width:
// 80 x 60, 40 x 30 ...), walked linearly, rows_per_wave segments per wavefront and workgroup; contracted arithmetic, f16 Gram, residual pairs by pixel
void launch_sweep_small(hipStream_t s, int rows_per_wave, const LevelGeom& g, const PairPtrs* pairs, const PairState* states, int n_pairs,
                        float* partials, float2* scratch, int* f16_range_flag = nullptr);
// scratch == null: read-only (one float per workgroup goes to `sink`, which must hold a float per (8 * 256)-pixel block)
// window_planes: the planes the window sweep reads (reference 8 B + current {I, Z} 8 B) instead of the gathering sweep's 8 + 16 + 8 B
void launch_stream_mix(hipStream_t s, const PairPtrs* pairs, int n_pairs, int n_px, float2* scratch, float* sink, bool window_planes = false);
// ref_order (option "ref_order", ref_order.h): n and S of every pair from its RefOrderPair instead of the partial rows
void launch_loglik(hipStream_t s, const LevelGeom& g, const PairState* states, int n_pairs, const float* partials,
                   const float2* scratch, double* ll_partials, int blocks_per_pair, bool one_schedule = false, const RefOrderPair* ref_order = nullptr);

// ref_order.hip (option "ref_order"): behind a sweep that stored the residual pairs by pixel, the rows' records (`rows`: g.h per pair) and
// every pair's RefOrderPair; and the Q3 edit of reference planes
void launch_ref_order(hipStream_t s, const LevelGeom& g, const PairState* states, int n_pairs, const float2* scratch, RefOrderSeg* rows, RefOrderPair* out);
void launch_ref_order_drop_last(hipStream_t s, const RefOrderPlane* planes, int n_planes);
void launch_ref_order_restore(hipStream_t s, const RefOrderPlane* planes, int n_planes);   // (the pixels the edit cleared, back)

// align_resident.hip: levels first_level..last_level of every pair in one launch.  The n_pairs * group workgroups must fit the
// device at once when group > 1 (one per compute unit); `cooperative` launches them through hipLaunchCooperativeKernel.
hipError_t launch_match_resident(hipStream_t s, const ResidentArgs& args, bool cooperative);

// align_coarse.hip: levels first_level..last_level of every pair in one launch, one workgroup per pair (no workgroup waits for another).
// workgroups_per_cu: 4 (128 registers; default) or 3 (168)
bool coarse_kernel_takes(const SweepChoice& choice, const LevelGeom& g);
hipError_t launch_match_coarse(hipStream_t s, const CoarseArgs& args, int workgroups_per_cu);

// solver_kernels.hip
extern int g_solver_occupancy;   // experiment (option "solver_occupancy"): 3 / 4 = the four-wavefront solver step built for that many workgroups per compute unit
void launch_init_pairs(hipStream_t s, PairState* states, int n_pairs, SolverParams prm, const double* T_init);
// flags (may be null: every pair): which == 0 -- every pair whose flag byte is zero, which == 1 -- the flagged ones; from_level >= 0:
// of those, the pairs that have left that level
void launch_level_begin(hipStream_t s, PairState* states, int n_pairs, SolverParams prm, LevelGeom g, int level,
                        const PairPtrs* pairs, dvo_hip_level_stats* levels, const double* T_init_or_null = nullptr,
                        const unsigned char* flags = nullptr, int which = 0, int from_level = -1);
// the slow lane of a batch (capi_lane.inc::SlowLane): the pairs still active on `level` get their flag byte set, and the indices of all flagged
// pairs go into list[0 .. cap) in ascending order, -1 behind the last; LevelGeom::pair_list then makes a launch cover the list, ::skip_flags
// makes one leave the flagged pairs alone.  The flags of a batch start at zero (launch_clear_flags).
// list_only: nothing is flagged; the list gets the unflagged pairs active on the level (flags may be null) -- the active-pair list of a level's last steps
void launch_mark_stragglers(hipStream_t s, const PairState* states, int n_pairs, int level, unsigned char* flags, int* list, int cap, bool list_only = false);
void launch_clear_flags(hipStream_t s, unsigned char* flags, int n_pairs);
// ... which the sweep of the level must understand (SweepChoice::pair_list: the contracted window sweep and the gathering sweep of the default schedule do)
void launch_solver_step(hipStream_t s, PairState* states, int n_pairs, SolverParams prm, LevelGeom g,
                        const float* partials, const double* ll_partials, int ll_blocks_per_pair, const float2* scratch_for_fused_ll,
                        dvo_hip_level_stats* levels, dvo_hip_iteration_stats* iters, unsigned long long* step_tally,
                        int* host_status, bool two_waves = false, int level_slot_hint = -1, const NextLevel* next_or_null = nullptr,
                        const RefOrderPair* ref_order = nullptr);
// the serial half of a step whose wide half ran in the sweep's tail (a.pair_sums)
void launch_solver_serial(hipStream_t s, int n_pairs, LevelGeom g, const SolverStepArgs& a);
void launch_finish(hipStream_t s, const PairState* states, int n_pairs, SolverParams prm,
                   const dvo_hip_level_stats* levels, const dvo_hip_iteration_stats* iters, dvo_hip_result* results);
// single-shot linearisation for parity tests: fixed T34 / P_prev, no state machine
// measurement: every pair back on its level with the weights on (after warm-up iterations)
void launch_force_active(hipStream_t s, PairState* states, int n_pairs);
void launch_set_fixed_state(hipStream_t s, PairState* states, LevelGeom g, const float* T34_dev, const float* Pprev_dev, int first);
void launch_single_shot_out(hipStream_t s, LevelGeom g, const float* partials, const double* ll_partials, int ll_blocks_per_pair,
                            int n_selected, dvo_hip_iteration_out* out_dev, const RefOrderPair* ref_order = nullptr);

}  // namespace dvo_hip
