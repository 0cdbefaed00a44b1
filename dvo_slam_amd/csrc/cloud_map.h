// cloud_map.h -- the keyframe map (include/dvo_hip.h, dvo_hip_map_* and dvo_hip_frames_world_points): the world point of a pixel under a
// keyframe pose, the voxel it falls into, and the per-voxel integer sums a fused, downsampled cloud is read from.  These are the semantics
// of the reference's map building -- AsyncPointCloudBuilder::BuildJob::build (dvo_core/src/visualization/async_point_cloud_builder.cpp:61-110:
// pose.cast<float>() * image.pointcloud, plus intensity) and PointCloudAggregator::build (point_cloud_aggregator.cpp:74-109: concatenate,
// then a 1 cm voxel grid) -- with an EXACT per-voxel centroid in place of PCL's ApproximateVoxelGrid.  Shared by the kernels
// (cloud_map.hip: k_world_points, k_map_insert, k_map_rehash, k_map_extract, k_map_clear; map_merge.hip: k_map_merge, k_map_export) and the host compiler of the CPU tier (tests/test_cloud_map.py),
// which is the yardstick the device results are compared with bit for bit: float32 throughout (the extraction alone is double), compiled
// without contraction (clang: the pragma below; a host compiler: -ffp-contract=off), division correctly rounded on both sides.  Every
// product, quotient and sum is rounded on its own, left to right as parenthesised.
//
// World point.  For pixel (u, v) of a level with intrinsics K = {fx, fy, ox, oy}, depth z, intensity I and the pose T = [R | t] (camera ->
// world; the row-major 4 x 4 double of dvo_hip_result::transformation, converted to float ONCE per frame, map_pose_prepare):
//   X = ((u - ox) / fx) * z,  Y = ((v - oy) / fy) * z      (RgbdCamera::buildPointCloud, include/dvo/core/rgbd_image.h)
//   P = R (X, Y, z) + t, each row as ((r0 X + r1 Y) + r2 z) + t
// The point is USABLE iff z is finite and > 0, min_depth <= z <= max_depth (0 and +INFINITY: the range is off, selection.h), and P is
// finite.
// Voxel.  leaf is a float > 0.  Per axis: f = P.x / leaf, i = floorf(f); the point is OUT OF RANGE (counted, skipped) unless
// -2^20 <= i < 2^20; q = int((f - i) * 1024.0f) clamped into [0, 1023] (both operations are exact in float; the clamp catches f - i
// rounding up to 1 for a tiny negative f).  Key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20) as uint64: at most 2^63 - 1, so
// kMapEmptyKey = ~0 is no key.  Intensity: qi = int(floorf(I * 16.0f + 0.5f)) clamped into [0, 4095], 0 for a non-finite I.
// Accumulation.  A voxel holds the point count n and the sums of qx, qy, qz, qi as unsigned 32-bit integers.  A voxel may take at most
// kMapVoxelMaxPoints = 2^20 points: up to there no sum can wrap (4095 * 2^20 < 2^32).  Whether a voxel exceeded the limit is decided
// from n alone, so the decision does not depend on the order of insertion.  All sums are integers: the table's content does not depend
// on the order of the additions, and neither does the SET of occupied slots under linear probing.
// Table.  Open addressing, capacity a power of two, slot = map_hash(key) & (capacity - 1), linear probing with the FIXED bound
// kMapMaxProbes = 128; a point that finds neither its key nor an empty slot within the bound is DROPPED and counted.
// Extraction of a voxel, in double, rounded to float once:
//   x = (double(ix) + (double(sx) / double(n) + 0.5) / 1024.0) * double(leaf)   (y, z likewise);   intensity = double(si) / double(n) / 16.0
// Each point's offset is truncated to a 1024th of the leaf and the half step is added back, so per axis the result lies within
// leaf / 2048 of the true centroid of the voxel's points (plus float32 rounding); the intensity within 1 / 32.
//
// Removal (dvo_hip_map_remove, the - half of dvo_hip_map_move; k_map_insert over a frame whose sign is -1).  A frame leaves the map by the
// road it came: usable / out of range / key / q[0..3] of every pixel are computed exactly as at insertion (map_world_point, map_key_of,
// the same pose cast, level and depth range), and the key is LOOKED UP with the insertion's probe sequence.  A lookup never claims a slot:
// one that meets an empty slot, or exhausts kMapMaxProbes, leaves the point UNMATCHED -- counted, nothing subtracted.  From a found slot
// the point is subtracted as whole words: {n, sx} and {sy, sz} take one 64-bit two's-complement add each (map_word, map_negate), si one
// 32-bit add.  That is the exact inverse of the insertion's three adds, carries between the halves included, so removing what was
// inserted restores the slot bit for bit -- also for a voxel beyond kMapVoxelMaxPoints, whose low halves have carried into the high ones.
// Additions and subtractions may interleave within a launch: every field is at all times its old total, minus some of what EARLIER
// launches added, plus some of the new points -- never negative, so no borrow crosses a half-word.
// A slot whose n returns to 0 keeps its key.  It is VACANT (map_slot_vacant): skipped by the extraction and by a render (neither is
// live, map_slot_live), still no stop on anybody's probe path -- keys never leave their slots, so bounded linear probing stays valid
// without tombstones -- and still counted in `occupied`.  The frame's unusable and out-of-range pixels leave those two counts as well:
// points, out_of_range and unusable describe the frames the map holds now.
// PRECONDITION.  Removal is exact only for points the table took, and the caller passes the same frame content, level, pose and depth
// range as at insertion; a mismatch shows up as unmatched > 0.  A mismatched point that happens to meet a voxel of other points is
// subtracted from THAT voxel -- the map cannot tell -- and a voxel that loses more than it holds wraps and reads as over the limit.  A map that has dropped points since its last clear or rehash refuses a removal: what was dropped cannot be told
// from what was taken.
// Rehash (dvo_hip_map_rehash; k_map_rehash).  A second table of a given capacity (a power of two) takes every LIVE slot of the first with
// its five sums unchanged; vacant slots stay behind.  Live keys are unique in the old table: whoever claims a slot of the new one (one
// 64-bit CAS, the same probe sequence and bound) is its only writer and stores the sums plainly.  A record that finds no slot is counted,
// and the new table replaces the old one only if there was none; else the map is unchanged.
//
// Merge (dvo_hip_map_merge, dvo_hip_map_move_submaps, dvo_hip_map_export, dvo_hip_map_merge_records; map_merge.hip: k_map_merge, k_map_export).
// A RECORD is 32 bytes with the layout of MapSlot, {key, n, sx, sy, sz, si, pad}; of a coloured map also the 16 bytes of MapColourSlot
// (cloud_colour.h) at the same index, of a map with normals the 16 bytes of MapNormalSlot (cloud_normal.h, which also says how a posed
// merge turns them).  A record with key == kMapEmptyKey or n == 0 is not live and is skipped (map_slot_live): a raw dump
// of a table is a valid record array, and so is what an export compacts out of one.
// Plain merge, sign +1.  Source and destination have the same leaf (as bits).  The record's key is probed in the destination exactly as an
// insertion probes (map_hash, linear, kMapMaxProbes, an empty slot is claimed), and the WHOLE WORDS are added: map_word(n, sx),
// map_word(sy, sz), si, and of a coloured map colour_word(sr, sg), sb.  That is the arithmetic modulo 2^64 of inserting the record's
// points one at a time: the sum of two sub-maps is, bit for bit in what an extraction and a render return, the map built from all their
// keyframes at once -- voxels beyond kMapVoxelMaxPoints included.  A record that finds no slot is DROPPED, by its n points.
// Plain merge, sign -1.  A lookup that never claims, as in a removal; the two's complement of the same words is added (map_negate).  A
// record that finds no slot is UNMATCHED by its n points.  Subtracting a sub-map restores the words as a removal of its frames does.
// Posed merge (map_pose_record).  The source lies in its own coordinates -- those of its anchor keyframe -- and enters under T = [R | t],
// the row-major 4 x 4 double cast to float once (map_pose_prepare):
//   1. c[0..2] = the voxel's centroid, map_extract_voxel with the SOURCE's leaf: double, rounded to float once;
//   2. P = R c + t, each row as ((r0 c0 + r1 c1) + r2 c2) + t in float, every operation rounded on its own (map_pose_point: the shape
//      of map_world_point);
//   3. P not finite: the record's n points are UNUSABLE;
//   4. else map_key_of(P, 0, leaf of the DESTINATION, &key2, q); false: the n points are OUT OF RANGE;
//   5. else the record added under key2 is {n, n * q[0], n * q[1], n * q[2], si}, the products in uint32 (they wrap like every other
//      sum: a source voxel beyond kMapVoxelMaxPoints makes the destination voxel one, which n reports); the colour sums go unchanged.
// The sign -1 form computes the same key2 and addends and subtracts them: a posed subtraction of what was posed-merged under the same
// float pose restores the destination bit for bit.  The source's leaf may differ from the destination's: the record is binned anew.
// ACCURACY.  A posed merge treats a source voxel's n points as n copies of their centroid: a point may land up to one source leaf from
// where a rebuild from the frames would put it, and voxels at the faces of the destination's grid differ from such a rebuild.  The
// point-weighted mean position is kept to quantisation: per axis within (leaf_src + leaf_dst) / 2048 of the source's, transformed, plus
// the float rounding of the transform.  This is the sub-map approximation (a LocalMap moves rigidly with its keyframe), not a rebuild.
// Statistics.  A plus merge adds the n of every live record in range to the usable points, a minus merge to the points being removed;
// dropped and unmatched count points, not records.  A plain merge from a MAP also adds (sign -1: takes back) the source's out-of-range
// and unusable counts: the merged map's points, out_of_range, unusable, dropped and over_limit are those of the single build.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hd_compat.h"
#include "selection.h"   // selection_range_on

namespace dvo_hip {

constexpr int kMapMaxProbes = 128;
constexpr int kMapAxisOffset = 1 << 20;                 // voxel indices -2^20 .. 2^20 - 1 per axis
constexpr uint32_t kMapVoxelMaxPoints = 1u << 20;
constexpr uint64_t kMapEmptyKey = ~0ull;
constexpr uint32_t kMapHole = 0x7FC00000u;              // x, y, z of an unusable pixel in the organised cloud: a quiet NaN

// one slot of the table, 32 bytes: {n, sx} and {sy, sz} are also addressed as two 64-bit words (cloud_map.hip: one atomic add each; a
// carry out of the low half needs more than 2^20 points in the voxel, which n -- a low half itself -- reports)
struct alignas(32) MapSlot {
  uint64_t key;
  uint32_t n, sx, sy, sz, si, pad;
};

struct MapPose {
  float r[9], t[3];
};

// the pose as the kernels use it: pose.cast<float>() of the row-major 4 x 4 double
DVO_HD MapPose map_pose_prepare(const double* T16) {
  MapPose p;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) p.r[i * 3 + j] = float(T16[i * 4 + j]);
    p.t[i] = float(T16[i * 4 + 3]);
  }
  return p;
}

DVO_HD bool map_finite(float x) { return x > -__builtin_inff() && x < __builtin_inff(); }   // (NaN: no)

// The world point of pixel (u, v), depth z: P[0..2]; true iff the point is usable.
DVO_HD bool map_world_point(const MapPose& p, const float K[4], int u, int v, float z, float min_depth, float max_depth, float P[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float X = ((float(u) - K[2]) / K[0]) * z, Y = ((float(v) - K[3]) / K[1]) * z;
  P[0] = ((p.r[0] * X + p.r[1] * Y) + p.r[2] * z) + p.t[0];
  P[1] = ((p.r[3] * X + p.r[4] * Y) + p.r[5] * z) + p.t[1];
  P[2] = ((p.r[6] * X + p.r[7] * Y) + p.r[8] * z) + p.t[2];
  if (!(z > 0.0f && z < __builtin_inff())) return false;
  if (selection_range_on(min_depth, max_depth) && !(min_depth <= z && z <= max_depth)) return false;
  return map_finite(P[0]) && map_finite(P[1]) && map_finite(P[2]);
}

// one axis: voxel index + 2^20 into *cell and the quantised offset into *q; false = out of range
DVO_HD bool map_axis(float x, float leaf, uint32_t* cell, uint32_t* q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float f = x / leaf, i = floorf(f);
  if (!(i >= -float(kMapAxisOffset) && i < float(kMapAxisOffset))) return false;
  int k = int((f - i) * 1024.0f);
  k = k < 0 ? 0 : k > 1023 ? 1023 : k;
  *cell = uint32_t(int(i) + kMapAxisOffset);
  *q = uint32_t(k);
  return true;
}

DVO_HD uint64_t map_pack_key(uint32_t cx, uint32_t cy, uint32_t cz) { return uint64_t(cx) << 42 | uint64_t(cy) << 21 | uint64_t(cz); }
DVO_HD void map_unpack_key(uint64_t key, int* ix, int* iy, int* iz) {
  *ix = int(uint32_t(key >> 42) & 0x1fffffu) - kMapAxisOffset;
  *iy = int(uint32_t(key >> 21) & 0x1fffffu) - kMapAxisOffset;
  *iz = int(uint32_t(key) & 0x1fffffu) - kMapAxisOffset;
}

DVO_HD uint32_t map_quantise_intensity(float I) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!map_finite(I)) return 0u;
  const float r = floorf(I * 16.0f + 0.5f);
  return r < 0.0f ? 0u : r > 4095.0f ? 4095u : uint32_t(int(r));
}

// Key and quantised offsets q[0..2] of the usable point P, and the quantised intensity q[3]; false = out of range.
DVO_HD bool map_key_of(const float P[3], float I, float leaf, uint64_t* key, uint32_t q[4]) {
  uint32_t c[3];
  if (!map_axis(P[0], leaf, &c[0], &q[0]) || !map_axis(P[1], leaf, &c[1], &q[1]) || !map_axis(P[2], leaf, &c[2], &q[2])) return false;
  *key = map_pack_key(c[0], c[1], c[2]);
  q[3] = map_quantise_intensity(I);
  return true;
}

// where a key's probe sequence starts: a 64-bit mixer (the finaliser of MurmurHash3), masked; capacity is a power of two
DVO_HD uint64_t map_hash(uint64_t key, uint64_t capacity) {
  key ^= key >> 33;
  key *= 0xff51afd7ed558ccdull;
  key ^= key >> 33;
  key *= 0xc4ceb9fe1a85ec53ull;
  key ^= key >> 33;
  return key & (capacity - 1);
}

// a slot that holds a voxel; and one whose points have all been removed (the key stays: Removal above)
DVO_HD bool map_slot_live(uint64_t key, uint32_t n) { return key != kMapEmptyKey && n > 0u; }
DVO_HD bool map_slot_vacant(uint64_t key, uint32_t n) { return key != kMapEmptyKey && n == 0u; }

// two neighbouring sums as the 64-bit word the table adds them in ({n, sx}: n low; {sy, sz}: sy low), and what to add to take a word back
DVO_HD uint64_t map_word(uint32_t lo, uint32_t hi) { return uint64_t(lo) | uint64_t(hi) << 32; }
DVO_HD uint64_t map_negate(uint64_t word) { return uint64_t(0) - word; }

// a voxel's record: out[0..2] the centroid, out[3] the mean intensity
DVO_HD void map_extract_voxel(uint64_t key, uint32_t n, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t si, float leaf, float out[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int ix, iy, iz;
  map_unpack_key(key, &ix, &iy, &iz);
  const double dn = double(n), dl = double(leaf);
  out[0] = float((double(ix) + (double(sx) / dn + 0.5) / 1024.0) * dl);
  out[1] = float((double(iy) + (double(sy) / dn + 0.5) / 1024.0) * dl);
  out[2] = float((double(iz) + (double(sz) / dn + 0.5) / 1024.0) * dl);
  out[3] = float(double(si) / dn / 16.0);
}

// P = R c + t in float, every operation rounded on its own, each row as ((r0 c0 + r1 c1) + r2 c2) + t (the shape of map_world_point)
DVO_HD void map_pose_point(const MapPose& p, const float c[3], float P[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  P[0] = ((p.r[0] * c[0] + p.r[1] * c[1]) + p.r[2] * c[2]) + p.t[0];
  P[1] = ((p.r[3] * c[0] + p.r[4] * c[1]) + p.r[5] * c[2]) + p.t[1];
  P[2] = ((p.r[6] * c[0] + p.r[7] * c[1]) + p.r[8] * c[2]) + p.t[2];
}

// what became of a record under a pose (Merge above)
constexpr int kMapPosePlaced = 0, kMapPoseUnusable = 1, kMapPoseOutOfRange = 2;

// The live record {key, n, sx, sy, sz, si} of a table of leaf leaf_src under the pose p, for a table of leaf leaf_dst: its key there and
// add[0..4] = {n, n q0, n q1, n q2, si}, or why it has none.
DVO_HD int map_pose_record(const MapPose& p, uint64_t key, uint32_t n, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t si, float leaf_src,
                           float leaf_dst, uint64_t* key2, uint32_t add[5]) {
  float c[4], P[3];
  uint32_t q[4];
  map_extract_voxel(key, n, sx, sy, sz, si, leaf_src, c);
  map_pose_point(p, c, P);
  if (!(map_finite(P[0]) && map_finite(P[1]) && map_finite(P[2]))) return kMapPoseUnusable;
  if (!map_key_of(P, 0.0f, leaf_dst, key2, q)) return kMapPoseOutOfRange;
  add[0] = n;
  add[1] = n * q[0];
  add[2] = n * q[1];
  add[3] = n * q[2];
  add[4] = si;
  return kMapPosePlaced;
}

}  // namespace dvo_hip
