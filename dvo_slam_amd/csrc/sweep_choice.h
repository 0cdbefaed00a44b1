// sweep_choice.h -- which of the five sweep kernels runs a pyramid level, and everything that follows from that choice: THE statement of
// the rule.  Plain host C++17 (no HIP): the driver makes a SweepChoice per level of a batch's plan (capi_schedule.inc::make_plan) and
// every consumer -- the level's geometry and tile height, the flavour of the current role that is built, the resident / coarse / slow-lane
// plans, launch_residual_reduce -- reads it; code without a plan (frame allocation, the flavours of an ingest) calls choose_sweep itself.
// The limits the kernels impose are defined here, once, and the kernels' files read them from here.
//
//   kernel                   chosen for (the first row that applies)                          reads    walk                   tile rows
//   k_sweep_small            option "small_sweep", variant >= 8, no "ref_compat" / "ref_order":   C        linear                 driver's
//                            an even width that is walked linearly, level + border in kSmallCells
//   k_sweep_fast             variant >= 8: even widths from kFastCols on, both extents below      C        tiled                  4
//                            kWindowMaxExtent, planes and packed residuals within buffer offsets
//   k_sweep_window           variant >= 6: widths that are a multiple of 64, both extents below   C        tiled                  4
//                            kWindowMaxExtent (variants 8 / 9: what is left of them -- width 64)
//   k_residual_reduce_mfma   variant >= 5: every other level                                      A + B    linear where the width driver's
//                                                                                                          is no multiple of 64
//   k_residual_reduce        variants below 5                                                     A + B    tiled                  driver's
//
// One corner differs from the code before this header on purpose: an even width from kFastCols on that is no multiple of 64, under
// variant >= 8, whose planes -- or whose packed residuals, padded to whole tiles -- reach kBufferOffsetLimit (2^28 pixels, the padding
// counted).  The launcher always sent such a level to the gathering sweep, tiled; the driver used to build plane C alone for it and to
// fix the tile height at 4.  Now the planes follow the kernel: A + B, and the tile height is the driver's.  Nothing else differs.
//
// A second corner is kept as it was: whether a width is walked linearly is decided by the width alone, so a level of variant >= 8 with
// a fast sweep's width and a HEIGHT of kWindowMaxExtent or more stays tiled in the gathering sweep.
#pragma once

namespace dvo_hip {

constexpr int kWavesPerBlock = 4;
constexpr int kTileW = 64;           // one wavefront spans 64 consecutive pixels of a row
constexpr int kWindowRowsPerWave = 4;                   // both window sweeps: tiles of 64 x 16
constexpr int kFastCols = 84;                           // window columns in use: 64 + the taps' reach (3) + 17 of motion / parallax
constexpr int kSmallCells = 5376;                            // (w + 2) x (h + 2) cells of 8 B at most: 43 KB (80 x 60: 82 x 62 = 5084)
constexpr int kWindowMaxExtent = 32768;                 // both window sweeps: widths and heights below this
// (a pair's planes and its residual buffer are addressed through 32-bit buffer offsets: 2 GB each at most -- a 16 384 x 16 384 level)
constexpr long long kBufferOffsetLimit = 1ll << 31;
constexpr int kCompactTileEntries = 1024, kCompactWaveEntries = 256;

enum class SweepKernel { Valu, Gather, Window, Fast, Small };   // k_residual_reduce, k_residual_reduce_mfma, k_sweep_window, k_sweep_fast, k_sweep_small

// the option values that bear on the choice (the driver's sweep_options fills them from the context)
struct SweepOptions {
  int variant, small_sweep, ref_compat, ref_order, compact_residuals;
};

struct SweepChoice {
  SweepKernel kernel;
  bool linear;       // LevelGeom::linear: one row of w * h pixels in 64-pixel segments instead of 64-column tiles
  bool reads_c;      // the current role's 8-byte plane C; else the taps A + B
  int tile_rows;     // rows per wavefront the kernel insists on (kWindowRowsPerWave), 0: the driver's to pick
  bool compact;      // LevelGeom::compact: packed residual pairs
  // 0: f32 Gram, exact arithmetic; 1: f16 Gram, exact arithmetic (variant 7, and the contracted schedules under "ref_compat"); 2: f16 Gram,
  // contracted arithmetic.  The gathering sweep's MODE; the exact window sweep runs its f16 Gram from 1 on
  int mode;
  bool pair_list;    // the kernel reads LevelGeom::pair_list
  // the contracted window sweep's operand store (STORE): 2 = high and low parts take turns in the slab (variant 8, and under "ref_compat"
  // whatever the variant: "variant" 9 is the same as 8 there), 1 = side by side (variant 9, a measurement schedule)
  int operand_store;

  bool windowed() const { return kernel == SweepKernel::Window || kernel == SweepKernel::Fast; }
};

// the levels k_sweep_small takes: even widths (the plane C of a level is built in pixel pairs), the whole level + border in kSmallCells
inline bool small_level_fits(int w, int h) { return w % 2 == 0 && w >= 4 && h >= 4 && (w + 2ll) * (h + 2ll) <= kSmallCells; }

// (64-column tiles; a width that is no multiple of 64 leaves the last tile column partly empty)
inline bool fast_sweep_width(int w) { return w >= kFastCols && w % 2 == 0; }

inline SweepChoice choose_sweep(const SweepOptions& o, int w, int h) {
  const bool in_extent = w < kWindowMaxExtent && h < kWindowMaxExtent;
  const bool fast_width = o.variant >= 8 && fast_sweep_width(w) && w < kWindowMaxExtent;   // (option "ref_compat" included: the COMPAT instantiations)
  const long long tiles = ((w + kTileW - 1ll) / kTileW) * ((h + kWavesPerBlock * kWindowRowsPerWave - 1ll) / (kWavesPerBlock * kWindowRowsPerWave));
  const bool offsets_fit = 8ll * w * h < kBufferOffsetLimit && 8ll * kCompactTileEntries * tiles < kBufferOffsetLimit;
  SweepChoice c;
  c.linear = o.variant >= 5 && w % kTileW != 0 && !fast_width;
  c.mode = o.variant >= 8 && !o.ref_compat ? 2 : o.variant >= 7 ? 1 : 0;
  c.operand_store = o.variant == 8 || o.ref_compat ? 2 : 1;
  if (o.small_sweep && o.variant >= 8 && !o.ref_compat && !o.ref_order && c.linear && small_level_fits(w, h)) c.kernel = SweepKernel::Small;
  else if (fast_width && in_extent && offsets_fit) c.kernel = SweepKernel::Fast;
  else if (o.variant >= 6 && w % kTileW == 0 && in_extent) c.kernel = SweepKernel::Window;
  else c.kernel = o.variant >= 5 ? SweepKernel::Gather : SweepKernel::Valu;
  c.reads_c = c.windowed() || c.kernel == SweepKernel::Small;
  c.tile_rows = c.windowed() ? kWindowRowsPerWave : 0;
  // (not under "ref_order": its passes read the residual pairs by pixel, ref_order.hip)
  c.compact = o.compact_residuals && !o.ref_order && c.kernel == SweepKernel::Fast;
  c.pair_list = o.variant >= 8 && (c.kernel == SweepKernel::Fast || c.kernel == SweepKernel::Gather);
  return c;
}

// The sweep has an instantiation that ends with the pairs' solver steps (solver_step.h), at `rows_per_wave` rows per wavefront and
// with the level's LevelGeom::rcp_table set or not and its ::gram_hi_j: the default schedule (variant 8, every low part of the Gram
// operands, no "ref_compat") in the contracted window sweep, the contracted gathering sweep at tiles of up to 8 rows per wavefront.
inline bool sweep_has_tail(const SweepChoice& c, int rows_per_wave, bool rcp_table, bool gram_hi_j) {
  if (rcp_table) return false;
  if (c.kernel == SweepKernel::Fast) return c.operand_store == 2 && !gram_hi_j;
  return c.kernel == SweepKernel::Gather && c.mode == 2 && rows_per_wave != 16;
}

// Can any choice read plane C at this size?  (Whatever the options of the moment: a frame outlives option changes.)
inline bool any_sweep_reads_plane_c(int w, int h) { return w % kTileW == 0 || fast_sweep_width(w) || small_level_fits(w, h); }

}  // namespace dvo_hip
