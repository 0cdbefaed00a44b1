// cloud_map.hip -- the keyframe map on the device (cloud_map.h; include/dvo_hip.h, dvo_hip_map_* and dvo_hip_frames_world_points): the
// {I, Z} pairs of one pyramid level of n keyframes under their poses -> the organised world cloud of every frame (k_world_points), or one
// voxel-grid map of all of them (k_map_insert into -- and out of -- an open-addressing table of integer sums, k_map_extract out of it,
// k_map_rehash into a second table, k_map_clear).
//
// Both per-pixel kernels run over frames x pixels in one launch: a lane owns one pixel, a wavefront 64 consecutive pixels in raster order,
// a workgroup 256; frames of different sizes share the launch, a workgroup finds its frame by bisecting the table's first_block column.
// k_world_points stores one 16-byte record per lane, coalesced.
// k_map_insert reads 8 B per pixel.  Neighbouring pixels very often share a voxel, so before anything goes to memory the wavefront folds
// every run of consecutive lanes that hold the same key into the run's first lane: a segmented suffix sum over the lanes (__shfl_down,
// six steps, three packed words: a run of at most 64 points keeps every sum below 2^16 resp. 2^18).  Unusable, out-of-range and inactive
// lanes break a run.  Only a run's first lane probes the table -- a relaxed load of the slot's key, and a 64-bit atomicCAS where it reads
// empty; a key never changes once set, so a stale read can only send a lane to the CAS, which decides -- and issues the adds: three
// vector memory atomics whose return value is not used ({n, sx} and {sy, sz} as 64-bit words, si as a 32-bit one; relaxed, agent
// scope).  The probe loop is a `for` over kMapMaxProbes: it never spins and never waits for another lane; a run that finds no slot is
// counted as dropped.  All sums are integers, so the table is the same bit for bit with and without the folding, in any order of
// arrival.  DVO_MAP_COMBINE_RUNS=0 builds the plain one-lane-one-point form (profiles/keyframe_map.md has both).
// The MIXED instantiation of k_map_insert reads a sign per frame (MapFrame::sign; a workgroup, and so a wavefront and every run, lies in
// one frame): a frame with sign -1 is REMOVED (cloud_map.h, Removal) -- the same classification, keys and run folding, but the leader only
// looks its key up (a relaxed load per probe, no CAS: an empty slot ends the lookup, the run is unmatched) and adds the two's complement
// of the three words.  A move of n keyframes is one launch over 2n entries.  The instantiation without MIXED is the pure insert as it
// was.  k_map_rehash walks the old table like k_map_extract (32 B per slot) and places every live slot in a second, cleared table: the
// lane that wins the slot's CAS is its only writer (live keys are unique) and stores the 24 bytes of sums with plain vector stores.
// k_map_extract compacts the occupied slots into the caller's arrays, one atomic add of the active-lane count per wavefront on the
// output cursor, bounded by max_points; the order of the output is unspecified.  No LDS, no barriers, 256-thread workgroups.
// A COLOURED map (cloud_colour.h; MapTable::colour, a side table of 16 bytes per slot at the slot's index) runs the COLOUR instantiation
// of k_map_insert: a valid lane forms the colour of its pixel from the frame's level-0 plane of packed pixels (dword loads: the rows of
// an odd-width plane are not 16-byte aligned; 4 B per pixel at level 0, the 2^L x 2^L block above it), the run folding carries two more
// packed words through the same suffix sum (r | g << 16 and b: 64 * 255 = 16320 < 2^16, no carry between the halves), and the leader
// issues two more return-less adds on colour[at] ({sr, sg} as a 64-bit word, sb as a 32-bit one), negated for a minus frame.  Probing,
// claiming and counting are untouched, and the instantiations without COLOUR are the kernels of a grey map as they were.  k_map_clear
// zeroes the side table with the slots, k_map_rehash's winning lane copies the old index's 16 bytes to the new one, k_map_extract writes
// the colour record at the xyzi record's index where it is given an array for it.
// A map WITH NORMALS (cloud_normal.h; MapTable::normals, a second side table of 16 bytes per slot) runs the NORMALS instantiation of
// k_map_insert: a valid lane whose pixel is not on the border loads the four neighbouring depths (frame_normal, map_device.h: the left
// and right ones lie in the wavefront's own cache lines, the rows above and below were or will be read by other wavefronts), forms the
// world normal and quantises it to 10 bits a component; the run folding carries two more packed words (qx | qy << 16 and qz | 1 << 16:
// 64 * 1022 = 65408 < 2^16, no carry between the halves) and the leader issues two more return-less 64-bit adds on normals[at] ({snx,
// sny} and {snz, nn}), negated for a minus frame -- none where no point of the run has a normal.  COLOUR and NORMALS combine.  The
// instantiations without NORMALS are the kernels as they were; k_map_clear, k_map_rehash and k_map_extract treat the table like colour's.
#include "global_ptr.h"
#include "launch.h"
#include "cloud_map.h"
#include "map_device.h"

#ifndef DVO_MAP_COMBINE_RUNS
#define DVO_MAP_COMBINE_RUNS 1
#endif

namespace dvo_hip {

namespace {

typedef unsigned GlobalU32x4 __attribute__((ext_vector_type(4)));
typedef unsigned GlobalU32x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void k_world_points(const MapFrame* __restrict__ tbl, int n_frames, float min_depth, float max_depth) {
#pragma clang fp contract(off)
  const MapFrame& f = tbl[map_frame_of(tbl, n_frames, int(blockIdx.x))];
  const int i = (int(blockIdx.x) - f.first_block) * 256 + int(threadIdx.x);
  if (i >= f.w * f.h) return;
  const GlobalF32x2 iz = *(Global<const GlobalF32x2>)global_ptr(f.iz + size_t(i) * f.stride);
  const float K[4] = {f.K[0], f.K[1], f.K[2], f.K[3]};
  float P[3];
  const bool usable = map_world_point(f.pose, K, i % f.w, i / f.w, iz.y, min_depth, max_depth, P);
  const float hole = __uint_as_float(kMapHole);
  const GlobalF32x4 rec = {usable ? P[0] : hole, usable ? P[1] : hole, usable ? P[2] : hole, iz.x};
  *((Global<GlobalF32x4>)global_ptr(f.out) + i) = rec;
}

// MIXED: the frames carry signs (a remove or a move); without it every frame is inserted and MapFrame::sign is not read
// COLOUR: the map has a side table of colour sums (m.colour) and every frame a plane of packed pixels (MapFrame::colour)
// NORMALS: the map has a side table of normal sums (m.normals); a valid lane forms its pixel's normal from the four neighbouring depths
template <bool COMBINE, bool MIXED, bool COLOUR, bool NORMALS>
__global__ __launch_bounds__(256) void k_map_insert(const MapFrame* __restrict__ tbl, int n_frames, MapTable m, float min_depth, float max_depth) {
#pragma clang fp contract(off)
  const MapFrame& f = tbl[map_frame_of(tbl, n_frames, int(blockIdx.x))];
  const int i = (int(blockIdx.x) - f.first_block) * 256 + int(threadIdx.x);
  const int lane = int(threadIdx.x) & 63;
  const bool minus = MIXED && f.sign < 0;                    // (uniform over the workgroup)
  const bool active = i < f.w * f.h;
  bool unusable = false, out_of_range = false, valid = false;
  unsigned long long key = 0;
  uint32_t q[4] = {0, 0, 0, 0}, rgb = 0;
  uint32_t na = 0, nb = 0;                                   // NORMALS: {qnx | qny << 16}, {qnz | 1 << 16} of a lane whose pixel has a normal
  if (active) {
    const GlobalF32x2 iz = *(Global<const GlobalF32x2>)global_ptr(f.iz + size_t(i) * f.stride);
    const float K[4] = {f.K[0], f.K[1], f.K[2], f.K[3]};
    float P[3];
    uint64_t k = 0;
    if (!map_world_point(f.pose, K, i % f.w, i / f.w, iz.y, min_depth, max_depth, P)) unusable = true;
    else if (!map_key_of(P, iz.x, m.leaf, &k, q)) out_of_range = true;
    else valid = true;
    key = k;
    if constexpr (COLOUR) {
      // (valid: 0 <= u < w, 0 <= v < h of the level, so the block lies inside the level-0 plane, cloud_colour.h)
      if (valid) rgb = colour_level(f.colour, f.colour_pitch, i % f.w, i / f.w, f.shift);
    }
    if constexpr (NORMALS) {
      float N[3];
      if (frame_normal(f, K, i, i % f.w, i / f.w, iz.y, valid, N)) {
        na = normal_quantise(N[0]) | normal_quantise(N[1]) << 16;
        nb = normal_quantise(N[2]) | 1u << 16;
      }
    }
  }
  const unsigned long long validmask = __ballot(valid);
  if (minus) {
    wave_uncount(m.counters + kMapCntUnusable, __ballot(unusable), lane);
    wave_uncount(m.counters + kMapCntOutOfRange, __ballot(out_of_range), lane);
    wave_count(m.counters + kMapCntRemoving, validmask, lane);
  } else {
    wave_count(m.counters + kMapCntUnusable, __ballot(unusable), lane);
    wave_count(m.counters + kMapCntOutOfRange, __ballot(out_of_range), lane);
    wave_count(m.counters + kMapCntCandidates, validmask, lane);
  }

  // what this lane adds: {qx | qy << 16}, {qz | n << 16}, qi
  uint32_t a = valid ? q[0] | q[1] << 16 : 0u, b = valid ? q[2] | 1u << 16 : 0u, c = valid ? q[3] : 0u;
  // ... and to the side table of a coloured map: {r | g << 16}, b (0 from a lane that is not valid)
  uint32_t cw = colour_r(rgb) | colour_g(rgb) << 16, cb = colour_b(rgb);
  bool leader = valid;
  if constexpr (COMBINE) {
    const unsigned long long prev_key = __shfl_up(key, 1);
    const bool prev_valid = lane > 0 && ((validmask >> (lane - 1)) & 1ull) != 0;
    leader = valid && !(prev_valid && prev_key == key);
    const unsigned long long breaks = __ballot(leader) | ~validmask;   // lanes that do not continue the run of the lane before them
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t ua = __shfl_down(a, d), ub = __shfl_down(b, d), uc = __shfl_down(c, d);
      // lanes lane + 1 .. lane + d all continue this lane's run: lane + d holds the sum of the next (up to) d lanes of the same run
      const bool same_run = lane + d < 64 && ((breaks >> (lane + 1)) & ((1ull << d) - 1ull)) == 0;
      if (same_run) { a += ua; b += ub; c += uc; }
      if constexpr (COLOUR) {
        const uint32_t uw = __shfl_down(cw, d), uv = __shfl_down(cb, d);
        if (same_run) { cw += uw; cb += uv; }
      }
      if constexpr (NORMALS) {
        // (64 * 1022 = 65408 < 2^16: no carry between the halves)
        const uint32_t ux = __shfl_down(na, d), uy = __shfl_down(nb, d);
        if (same_run) { na += ux; nb += uy; }
      }
    }
  }
  const uint32_t n = b >> 16, sx = a & 0xffffu, sy = a >> 16, sz = b & 0xffffu, si = c;
  bool placed = false, claimed = false;
  if (leader) {
    const unsigned long long mask = m.capacity - 1;
    unsigned long long at = map_hash(key, m.capacity);
    for (int p = 0; p < kMapMaxProbes; ++p, at = (at + 1) & mask) {
      MapSlot* slot = m.slots + at;                          // (at <= capacity - 1: inside the table)
      unsigned long long* words = reinterpret_cast<unsigned long long*>(slot);
      unsigned long long seen = __hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (seen == kMapEmptyKey) {
        // a lookup never claims: the key was set by an earlier launch or not at all, and behind an empty slot it cannot lie
        if (minus) break;
        seen = atomicCAS(words, (unsigned long long)kMapEmptyKey, key);
        if (seen == kMapEmptyKey) { claimed = true; seen = key; }
      }
      if (seen != key) continue;
      const unsigned long long w1 = map_word(n, sx), w2 = map_word(sy, sz);
      (void)__hip_atomic_fetch_add(words + 1, minus ? map_negate(w1) : w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(words + 2, minus ? map_negate(w2) : w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(&slot->si, minus ? 0u - si : si, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if constexpr (COLOUR) {
        MapColourSlot* tint = m.colour + at;                   // (the side table has the slots' capacity)
        const unsigned long long w3 = colour_word(cw & 0xffffu, cw >> 16);
        (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(tint), minus ? map_negate(w3) : w3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(&tint->sb, minus ? 0u - cb : cb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if constexpr (NORMALS) {
        if (nb != 0u) {                                        // (a run none of whose points has a normal adds nothing)
          unsigned long long* facing = reinterpret_cast<unsigned long long*>(m.normals + at);   // (the side table has the slots' capacity)
          const unsigned long long w4 = normal_word(na & 0xffffu, na >> 16), w5 = normal_word(nb & 0xffffu, nb >> 16);
          (void)__hip_atomic_fetch_add(facing, minus ? map_negate(w4) : w4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          (void)__hip_atomic_fetch_add(facing + 1, minus ? map_negate(w5) : w5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      placed = true;
      break;
    }
    if (!placed)
      (void)__hip_atomic_fetch_add(m.counters + (minus ? kMapCntUnmatched : kMapCntDropped), (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  wave_count(m.counters + kMapCntUpdates, __ballot(placed), lane);
  wave_count(m.counters + kMapCntOccupied, __ballot(claimed), lane);
}

// xyzi == null: count only (live slots into the cursor, voxels over the limit, vacant slots).  rgba (a coloured map, or null): the
// voxel's colour record at the index of its xyzi record
__global__ __launch_bounds__(256) void k_map_extract(MapTable m, unsigned long long max_points, float4* __restrict__ xyzi, uint32_t* __restrict__ counts,
                                                     unsigned long long* __restrict__ keys, uint32_t* __restrict__ rgba, float4* __restrict__ normals) {
#pragma clang fp contract(off)
  const int lane = int(threadIdx.x) & 63;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  // (capacity and the stride are multiples of 64: the lanes of a wavefront leave the loop together)
  for (unsigned long long at = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; at < m.capacity; at += stride) {
    const auto words = (Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(m.slots + at));
    const GlobalU32x4 lo = words[0], hi = words[1];         // key | n sx, sy sz si pad
    const unsigned long long key = (unsigned long long)lo.x | (unsigned long long)lo.y << 32;
    const uint32_t n = lo.z;
    const bool occupied = map_slot_live(key, n);
    const unsigned long long mask = __ballot(occupied);
    wave_count(m.counters + kMapCntOverLimit, __ballot(occupied && n > kMapVoxelMaxPoints), lane);
    if (!xyzi) wave_count(m.counters + kMapCntVacant, __ballot(map_slot_vacant(key, n)), lane);
    unsigned long long base = 0;
    if (lane == 0 && mask != 0)
      base = __hip_atomic_fetch_add(m.counters + kMapCntCursor, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, 0);
    const unsigned long long idx = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
    if (occupied && xyzi && idx < max_points) {              // (idx < max_points: inside the caller's arrays)
      float rec[4];
      map_extract_voxel(key, n, lo.w, hi.x, hi.y, hi.z, m.leaf, rec);
      gstore((Global<float4>)global_ptr(xyzi) + idx, make_float4(rec[0], rec[1], rec[2], rec[3]));
      if (counts) counts[idx] = n;
      if (keys) keys[idx] = key;
      if (rgba) {
        const GlobalU32x4 t = *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(m.colour + at));   // sr sg sb pad
        rgba[idx] = colour_extract(n, t.x, t.y, t.z);
      }
      if (normals) {
        const GlobalU32x4 t = *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(m.normals + at));   // snx sny snz nn
        float nrec[4];
        normal_extract(t.x, t.y, t.z, t.w, nrec);
        gstore((Global<float4>)global_ptr(normals) + idx, make_float4(nrec[0], nrec[1], nrec[2], nrec[3]));
      }
    }
  }
}

// every live slot of `from` into `to` (cleared, its counters zero): to's kMapCntOccupied counts the slots claimed, its kMapCntDropped
// the records that found none within the probe bound
__global__ __launch_bounds__(256) void k_map_rehash(MapTable from, MapTable to) {
  const int lane = int(threadIdx.x) & 63;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x, mask = to.capacity - 1;
  // (capacity and the stride are multiples of 64: the lanes of a wavefront leave the loop together)
  for (unsigned long long src = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; src < from.capacity; src += stride) {
    const auto in = (Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(from.slots + src));
    const GlobalU32x4 lo = in[0], hi = in[1];               // key | n sx, sy sz si pad
    const unsigned long long key = (unsigned long long)lo.x | (unsigned long long)lo.y << 32;
    const bool live = map_slot_live(key, lo.z);
    bool placed = false;
    if (live) {
      unsigned long long at = map_hash(key, to.capacity);
      for (int p = 0; p < kMapMaxProbes; ++p, at = (at + 1) & mask) {
        MapSlot* slot = to.slots + at;                        // (at <= capacity - 1: inside the new table)
        unsigned long long* words = reinterpret_cast<unsigned long long*>(slot);
        // (every key differs from this one: a slot is this lane's iff its CAS wins it)
        if (__hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kMapEmptyKey) continue;
        if (atomicCAS(words, (unsigned long long)kMapEmptyKey, key) != kMapEmptyKey) continue;
        const GlobalU32x2 n_sx = {lo.z, lo.w};
        *(Global<GlobalU32x2>)global_ptr(reinterpret_cast<GlobalU32x2*>(words + 1)) = n_sx;
        *(Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(words + 2)) = hi;
        if (from.colour)                                       // (a coloured map: both tables have a side table)
          *(Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(to.colour + at)) =
              *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(from.colour + src));
        if (from.normals)                                      // (a map with normals: both tables have that side table)
          *(Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(to.normals + at)) =
              *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(from.normals + src));
        placed = true;
        break;
      }
    }
    wave_count(to.counters + kMapCntOccupied, __ballot(placed), lane);
    wave_count(to.counters + kMapCntDropped, __ballot(live && !placed), lane);
  }
}

__global__ __launch_bounds__(256) void k_map_clear(MapTable m) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  const GlobalU32x4 lo = {0xffffffffu, 0xffffffffu, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
  for (unsigned long long at = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; at < m.capacity; at += stride) {
    const auto words = (Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(m.slots + at));
    words[0] = lo;
    words[1] = hi;
    if (m.colour) *(Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(m.colour + at)) = hi;
    if (m.normals) *(Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(m.normals + at)) = hi;
  }
  if (blockIdx.x == 0 && threadIdx.x < kMapCounters) m.counters[threadIdx.x] = 0ull;
}

}  // namespace

void launch_world_points(hipStream_t s, const MapFrame* tbl, int n_frames, int total_blocks, float min_depth, float max_depth) {
  k_world_points<<<dim3(total_blocks), dim3(256), 0, s>>>(tbl, n_frames, min_depth, max_depth);
}

void launch_map_insert(hipStream_t s, const MapFrame* tbl, int n_frames, int total_blocks, const MapTable& m, float min_depth, float max_depth, bool mixed) {
  const dim3 grid(total_blocks), block(256);
  constexpr bool kCombine = DVO_MAP_COMBINE_RUNS != 0;
  if (m.normals) {
    if (mixed) {
      if (m.colour) k_map_insert<kCombine, true, true, true><<<grid, block, 0, s>>>(tbl, n_frames, m, min_depth, max_depth);
      else k_map_insert<kCombine, true, false, true><<<grid, block, 0, s>>>(tbl, n_frames, m, min_depth, max_depth);
    } else {
      if (m.colour) k_map_insert<kCombine, false, true, true><<<grid, block, 0, s>>>(tbl, n_frames, m, min_depth, max_depth);
      else k_map_insert<kCombine, false, false, true><<<grid, block, 0, s>>>(tbl, n_frames, m, min_depth, max_depth);
    }
  } else if (mixed) {
    if (m.colour) k_map_insert<kCombine, true, true, false><<<grid, block, 0, s>>>(tbl, n_frames, m, min_depth, max_depth);
    else k_map_insert<kCombine, true, false, false><<<grid, block, 0, s>>>(tbl, n_frames, m, min_depth, max_depth);
  } else {
    if (m.colour) k_map_insert<kCombine, false, true, false><<<grid, block, 0, s>>>(tbl, n_frames, m, min_depth, max_depth);
    else k_map_insert<kCombine, false, false, false><<<grid, block, 0, s>>>(tbl, n_frames, m, min_depth, max_depth);
  }
}

void launch_map_rehash(hipStream_t s, const MapTable& from, const MapTable& to) {
  k_map_clear<<<dim3(stride_grid(to.capacity)), dim3(256), 0, s>>>(to);
  k_map_rehash<<<dim3(stride_grid(from.capacity)), dim3(256), 0, s>>>(from, to);
}

bool map_insert_combines_runs() { return DVO_MAP_COMBINE_RUNS != 0; }

hipError_t launch_map_extract(hipStream_t s, const MapTable& m, unsigned long long max_points, float4* xyzi, uint32_t* counts, unsigned long long* keys,
                              uint32_t* rgba, float4* normals) {
  static_assert(kMapCntCursor == kMapCntOverLimit + 1 && kMapCntVacant == kMapCntOverLimit + 2, "what a pass counts lies together");
  const hipError_t e = hipMemsetAsync(m.counters + kMapCntOverLimit, 0, 3 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  k_map_extract<<<dim3(stride_grid(m.capacity)), dim3(256), 0, s>>>(m, max_points, xyzi, counts, keys, m.colour ? rgba : nullptr, m.normals ? normals : nullptr);
  return hipSuccess;
}

void launch_map_clear(hipStream_t s, const MapTable& m) { k_map_clear<<<dim3(stride_grid(m.capacity)), dim3(256), 0, s>>>(m); }

}  // namespace dvo_hip
