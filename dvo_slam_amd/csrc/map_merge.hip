// map_merge.hip -- keyframe sub-maps on the device (cloud_map.h, Merge; include/dvo_hip.h, dvo_hip_map_merge, dvo_hip_map_move_submaps,
// dvo_hip_map_export and dvo_hip_map_merge_records): voxel tables and arrays of raw voxel records go into, and out of, a map without
// the frames they were built from.
//
// k_map_merge runs over sources x records in one launch: a lane owns one source record (32 B, two 16-byte loads; a table's slot or an
// element of a record array), a workgroup 256 consecutive ones; sources of different sizes share the launch, a workgroup finds its
// source by bisecting the table's first_block column, as k_map_insert finds its frame.  A source's count need not be a multiple of
// 64: a lane past the end holds no record but stays in every ballot and shuffle of its wavefront.  A live lane -- of the POSED
// instantiation: one whose record has a key under the entry's pose (map_pose_record) -- probes the destination like an insertion: a
// relaxed load of the slot's key, a 64-bit atomicCAS where it reads empty and the entry's sign is +1 (sign -1 only looks up: an empty
// slot ends it, the record is unmatched), then the record's words as return-less relaxed adds ({n, sx} and {sy, sz} as 64-bit words,
// si as a 32-bit one; COLOUR: {sr, sg} and sb on the side table, the colour record loaded by live lanes only; NORMALS: {snx, sny} and
// {snz, nn} on the normal side table, the sums turned by the entry's pose in the POSED instantiation, cloud_normal.h), negated for sign -1.
// The probe loop is a `for` over kMapMaxProbes.  No LDS, no barriers, no spinning, no floating-point atomics.  There is no run folding:
// neighbouring slots of a hashed table do not share keys, and equal keys in a caller's record array are summed by the atomics.
// Counters: slot updates and claims are lane counts (one add per wavefront: wave_count); the usable points and the points being
// removed are sums of n over the wavefront (one add per wavefront: wave_add); dropped, unmatched, unusable and out-of-range points are
// rare and take one add of n per lane.  The first lane of an entry's first workgroup adds the counts the entry carries along.
// k_map_export is the compaction of k_map_extract with the raw 32 bytes (and the side table's 16) in place of the float record.
#include "global_ptr.h"
#include "launch.h"
#include "cloud_map.h"
#include "map_device.h"

namespace dvo_hip {

namespace {

typedef unsigned GlobalU32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void counter_add(unsigned long long* counter, unsigned long long v) {
  (void)__hip_atomic_fetch_add(counter, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the sum of v over the wavefront (every lane takes part; lane 0 ends up with the total), one add
__device__ __forceinline__ void wave_add(unsigned long long* counter, unsigned long long v, int lane) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  if (lane == 0 && v != 0) counter_add(counter, v);
}

// NORMALS: the destination has a side table of normal sums (m.normals) and every entry normal records (MapMergeEntry::normals)
template <bool POSED, bool COLOUR, bool NORMALS>
__global__ __launch_bounds__(256) void k_map_merge(const MapMergeEntry* __restrict__ tbl, int n_entries, MapTable m) {
#pragma clang fp contract(off)
  const MapMergeEntry& e = tbl[map_frame_of(tbl, n_entries, int(blockIdx.x))];
  const unsigned long long i = (unsigned long long)(int(blockIdx.x) - e.first_block) * 256ull + threadIdx.x;
  const int lane = int(threadIdx.x) & 63;
  const bool minus = e.sign < 0;                             // (uniform over the workgroup)
  bool valid = false, unusable = false, out_of_range = false;
  unsigned long long key = 0;
  uint32_t add[5] = {0, 0, 0, 0, 0}, tint[3] = {0, 0, 0}, n_src = 0;
  uint32_t facing[4] = {0, 0, 0, 0};                         // NORMALS: snx sny snz nn as they are added
  if (i < e.count) {                                         // (inside the source's records)
    const auto words = (Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(e.slots + i));
    const GlobalU32x4 lo = words[0], hi = words[1];         // key | n sx, sy sz si pad
    const unsigned long long k = (unsigned long long)lo.x | (unsigned long long)lo.y << 32;
    if (map_slot_live(k, lo.z)) {
      n_src = lo.z;
      if constexpr (POSED) {
        uint64_t k2 = 0;
        const int how = map_pose_record(e.pose, k, lo.z, lo.w, hi.x, hi.y, hi.z, e.leaf_src, m.leaf, &k2, add);
        valid = how == kMapPosePlaced;
        unusable = how == kMapPoseUnusable;
        out_of_range = how == kMapPoseOutOfRange;
        key = k2;
      } else {
        valid = true;
        key = k;
        add[0] = lo.z; add[1] = lo.w; add[2] = hi.x; add[3] = hi.y; add[4] = hi.z;
      }
      if constexpr (COLOUR) {
        if (valid) {
          const GlobalU32x4 t = *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(e.colour + i));   // sr sg sb pad
          tint[0] = t.x; tint[1] = t.y; tint[2] = t.z;
        }
      }
      if constexpr (NORMALS) {
        if (valid) {
          const GlobalU32x4 t = *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(e.normals + i));   // snx sny snz nn
          facing[0] = t.x; facing[1] = t.y; facing[2] = t.z; facing[3] = t.w;
          if constexpr (POSED) {
            if (t.w != 0u) normal_pose_sums(e.pose, t.x, t.y, t.z, t.w, facing);   // (the summed normal turns with the sub-map; nn stays)
          }
        }
      }
    }
  }
  wave_add(m.counters + (minus ? kMapCntRemoving : kMapCntCandidates), valid ? (unsigned long long)n_src : 0ull, lane);
  if constexpr (POSED) {
    if (unusable) counter_add(m.counters + kMapCntUnusable, minus ? 0ull - n_src : (unsigned long long)n_src);
    if (out_of_range) counter_add(m.counters + kMapCntOutOfRange, minus ? 0ull - n_src : (unsigned long long)n_src);
  }
  if (int(blockIdx.x) == e.first_block && threadIdx.x == 0) {
    if (e.out_of_range != 0) counter_add(m.counters + kMapCntOutOfRange, e.out_of_range);
    if (e.unusable != 0) counter_add(m.counters + kMapCntUnusable, e.unusable);
  }

  bool placed = false, claimed = false;
  if (valid) {
    const unsigned long long mask = m.capacity - 1;
    unsigned long long at = map_hash(key, m.capacity);
    for (int p = 0; p < kMapMaxProbes; ++p, at = (at + 1) & mask) {
      MapSlot* slot = m.slots + at;                          // (at <= capacity - 1: inside the table)
      unsigned long long* words = reinterpret_cast<unsigned long long*>(slot);
      unsigned long long seen = __hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (seen == kMapEmptyKey) {
        if (minus) break;                                    // a lookup never claims (cloud_map.h, Removal)
        seen = atomicCAS(words, (unsigned long long)kMapEmptyKey, key);
        if (seen == kMapEmptyKey) { claimed = true; seen = key; }
      }
      if (seen != key) continue;
      const unsigned long long w1 = map_word(add[0], add[1]), w2 = map_word(add[2], add[3]);
      (void)__hip_atomic_fetch_add(words + 1, minus ? map_negate(w1) : w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(words + 2, minus ? map_negate(w2) : w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(&slot->si, minus ? 0u - add[4] : add[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if constexpr (COLOUR) {
        MapColourSlot* to = m.colour + at;                     // (the side table has the slots' capacity)
        const unsigned long long w3 = colour_word(tint[0], tint[1]);
        (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(to), minus ? map_negate(w3) : w3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(&to->sb, minus ? 0u - tint[2] : tint[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if constexpr (NORMALS) {
        if (facing[3] != 0u) {                                 // (a record none of whose points had a normal adds nothing)
          unsigned long long* to = reinterpret_cast<unsigned long long*>(m.normals + at);   // (the side table has the slots' capacity)
          const unsigned long long w4 = normal_word(facing[0], facing[1]), w5 = normal_word(facing[2], facing[3]);
          (void)__hip_atomic_fetch_add(to, minus ? map_negate(w4) : w4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          (void)__hip_atomic_fetch_add(to + 1, minus ? map_negate(w5) : w5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      placed = true;
      break;
    }
    if (!placed) counter_add(m.counters + (minus ? kMapCntUnmatched : kMapCntDropped), (unsigned long long)n_src);
  }
  wave_count(m.counters + kMapCntUpdates, __ballot(placed), lane);
  wave_count(m.counters + kMapCntOccupied, __ballot(claimed), lane);
}

// records == null: count only (live slots into the cursor).  colour (a coloured map, or null) and normals (a map with normals, or null):
// the slot's colour record resp. normal record at the index of its record
__global__ __launch_bounds__(256) void k_map_export(MapTable m, unsigned long long max_records, MapSlot* __restrict__ records,
                                                    MapColourSlot* __restrict__ colour, MapNormalSlot* __restrict__ normals) {
  const int lane = int(threadIdx.x) & 63;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  // (capacity and the stride are multiples of 64: the lanes of a wavefront leave the loop together)
  for (unsigned long long at = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; at < m.capacity; at += stride) {
    const auto words = (Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(m.slots + at));
    const GlobalU32x4 lo = words[0], hi = words[1];         // key | n sx, sy sz si pad
    const unsigned long long key = (unsigned long long)lo.x | (unsigned long long)lo.y << 32;
    const bool live = map_slot_live(key, lo.z);
    const unsigned long long mask = __ballot(live);
    unsigned long long base = 0;
    if (lane == 0 && mask != 0)
      base = __hip_atomic_fetch_add(m.counters + kMapCntCursor, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, 0);
    const unsigned long long idx = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
    if (live && records && idx < max_records) {              // (idx < max_records: inside the caller's arrays)
      const auto out = (Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(records + idx));
      const GlobalU32x4 sums = {hi.x, hi.y, hi.z, 0u};
      out[0] = lo;
      out[1] = sums;
      if (colour) {
        const GlobalU32x4 t = *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(m.colour + at));   // sr sg sb pad
        const GlobalU32x4 rec = {t.x, t.y, t.z, 0u};
        *(Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(colour + idx)) = rec;
      }
      if (normals)
        *(Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(normals + idx)) =
            *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(m.normals + at));   // snx sny snz nn
    }
  }
}

}  // namespace

void launch_map_merge(hipStream_t s, const MapMergeEntry* tbl, int n_entries, int total_blocks, const MapTable& m, bool posed) {
  const dim3 grid(total_blocks), block(256);
  if (m.normals) {
    if (posed) {
      if (m.colour) k_map_merge<true, true, true><<<grid, block, 0, s>>>(tbl, n_entries, m);
      else k_map_merge<true, false, true><<<grid, block, 0, s>>>(tbl, n_entries, m);
    } else {
      if (m.colour) k_map_merge<false, true, true><<<grid, block, 0, s>>>(tbl, n_entries, m);
      else k_map_merge<false, false, true><<<grid, block, 0, s>>>(tbl, n_entries, m);
    }
  } else if (posed) {
    if (m.colour) k_map_merge<true, true, false><<<grid, block, 0, s>>>(tbl, n_entries, m);
    else k_map_merge<true, false, false><<<grid, block, 0, s>>>(tbl, n_entries, m);
  } else {
    if (m.colour) k_map_merge<false, true, false><<<grid, block, 0, s>>>(tbl, n_entries, m);
    else k_map_merge<false, false, false><<<grid, block, 0, s>>>(tbl, n_entries, m);
  }
}

hipError_t launch_map_export(hipStream_t s, const MapTable& m, unsigned long long max_records, MapSlot* records, MapColourSlot* colour,
                             MapNormalSlot* normals) {
  const hipError_t e = hipMemsetAsync(m.counters + kMapCntCursor, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  k_map_export<<<dim3(stride_grid(m.capacity)), dim3(256), 0, s>>>(m, max_records, records, m.colour ? colour : nullptr, m.normals ? normals : nullptr);
  return hipSuccess;
}

}  // namespace dvo_hip
