// covisibility.hip -- keyframe covisibility counted on the device (covisibility.h; include/dvo_hip.h, dvo_hip_frames_covisibility).
// k_covisibility reads the frames through the frame table of the keyframe-map launches (MapFrame: the {I, Z} pairs of the level, 8 B
// apart in plane C or 16 B apart in the taps A, and the level's K) -- every distinct frame stands in it ONCE, however many pairs name
// it -- and the pairs through a pair table {a, b, T} of indices into it.
//
// One launch covers all pairs, whatever mix of sizes: the pair is the grid's y, walked where there are more pairs than the grid is
// high; the grid's x strides over the pixels of a, a lane per pixel, a wavefront 64 consecutive pixels.  A lane makes one 8-byte load of
// {I_a, Z_a}, carries the point into b's camera in registers and -- only where it lands in view -- gathers b's {I, Z} with one plain
// cached 8-byte load: neighbouring lanes land on neighbouring pixels under any small motion.
// Reduction: the class of a lane's pixel becomes six wave-wide counts by ballot + popcount, summed in (wave-uniform) registers over the
// grid-stride loop; the photometric sum is kept per lane in 64 bits and reduced across the wavefront once per pair by xor shuffles.
// The four waves of a workgroup meet in 128 B of LDS, and the workgroup ends the pair with at most FOUR return-less 64-bit integer
// vector atomics (relaxed, agent scope) into the pair's record, which the driver zeroed on the same stream: {valid, in_view},
// {unknown, occluded}, {seen_through, consistent} and photo (covis_words: a count stays below 2^31, so no half carries into the other).
// No floating-point atomics, nothing waits or retries, and integer sums make the record independent of any order.  A workgroup
// whose share of a pair is empty (a smaller frame in a launch sized for a larger one) touches nothing.
//
// Expected traffic: 8 B read per pixel of a (16 B of the line where the pairs come from the taps A), at most 8 B gathered from b per
// pixel in view, and 32 B per pair (the record; 56 B of pair table read).  b's planes are shared by many pairs -- in an n x n list every
// frame is b to n pairs and a to n more -- and should hit in L2 / the Infinity Cache, so the HBM traffic of a large list should be far
// below the sum above; that is UNMEASURED until profiles/covisibility.md says otherwise.
// 256-thread workgroups, 128 B of LDS, two barriers per pair and workgroup.
#include "global_ptr.h"
#include "launch.h"
#include "covisibility.h"

namespace dvo_hip {

namespace {

__global__ __launch_bounds__(256) void k_covisibility(const MapFrame* __restrict__ tbl, const CovisPair* __restrict__ pairs, int n,
                                                      dvo_hip_covis_params par, unsigned long long* __restrict__ records) {
#pragma clang fp contract(off)
  __shared__ unsigned long long part[4][4];                      // [wave][word]
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int lane = int(threadIdx.x & 63u), wave = int(threadIdx.x >> 6);
  for (int item = int(blockIdx.y); item < n; item += int(gridDim.y)) {
    const CovisPair& pr = pairs[item];                           // (item < n: inside the pair table)
    const MapFrame& A = tbl[pr.a];                               // (0 <= a, b < the frames of the table: checked before the launch)
    const MapFrame& B = tbl[pr.b];
    const int wa = A.w, wb = B.w, hb = B.h;
    const long long pixels = (long long)wa * A.h;
    if ((long long)blockIdx.x * blockDim.x >= pixels) continue;  // (uniform over the workgroup: before any barrier)
    const size_t as = size_t(A.stride), bs = size_t(B.stride);
    const auto Ap = (Global<const float>)global_ptr(A.iz);
    const auto Bp = (Global<const float>)global_ptr(B.iz);
    const MapPose T = pr.T;
    const float Ka[4] = {A.K[0], A.K[1], A.K[2], A.K[3]}, Kb[4] = {B.K[0], B.K[1], B.K[2], B.K[3]};
    // the tap: covis_pixel asks only for 0 <= xx < wb and 0 <= yy < hb, so yy * wb + xx < wb * hb: inside B's level
    const auto tap = [&](int xx, int yy) {
      const GlobalF32x2 t = *(Global<const GlobalF32x2>)(Bp + (size_t(yy) * size_t(wb) + size_t(xx)) * bs);
      return WarpTap{t.x, t.y};
    };
    unsigned count[6] = {0u, 0u, 0u, 0u, 0u, 0u};                // wave-wide, the same in every lane
    unsigned long long photo = 0ull;                             // this lane's
    // i0: the wavefront's first pixel, so that the loop's trip count is uniform over the wavefront and every ballot sees all 64 lanes
    for (long long i0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < pixels; i0 += stride) {
      const long long i = i0 + lane;
      int c = kCovisSkipped;
      uint32_t q = 0u;
      if (i < pixels) {                                          // (i < wa * ha: inside A's level)
        const GlobalF32x2 iz = *(Global<const GlobalF32x2>)(Ap + size_t(i) * as);
        c = covis_pixel(T, Ka, Kb, wb, hb, par, int(i % wa), int(i / wa), iz.x, iz.y, tap, &q);
      }
      photo += q;
      count[0] += unsigned(__popcll(__ballot(c >= kCovisValid)));
      count[1] += unsigned(__popcll(__ballot(c >= kCovisUnknown)));
      count[2] += unsigned(__popcll(__ballot(c == kCovisUnknown)));
      count[3] += unsigned(__popcll(__ballot(c == kCovisOccluded)));
      count[4] += unsigned(__popcll(__ballot(c == kCovisSeenThrough)));
      count[5] += unsigned(__popcll(__ballot(c == kCovisConsistent)));
    }
    for (int m = 32; m > 0; m >>= 1) photo += __shfl_xor(photo, m, 64);
    if (lane == 0) {
      part[wave][0] = (unsigned long long)count[0] | (unsigned long long)count[1] << 32;
      part[wave][1] = (unsigned long long)count[2] | (unsigned long long)count[3] << 32;
      part[wave][2] = (unsigned long long)count[4] | (unsigned long long)count[5] << 32;
      part[wave][3] = photo;
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
      const unsigned long long sum = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
      // (item < n: the item's own four words of the n records)
      if (sum != 0ull) (void)__hip_atomic_fetch_add(records + size_t(item) * 4 + threadIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();                                             // (part is written again for the workgroup's next pair)
  }
}

// x: grid-stride over the pixels of the largest a, y: the pairs (at most 1024 rows; the kernel walks the rest) -- warp_grid's shape
dim3 covis_grid(long long pixels, int n) {
  long long blocks = (pixels + 255) / 256;
  const int rows = n < 1024 ? n : 1024;
  const long long cap = 8192 / rows > 64 ? 8192 / rows : 64;
  blocks = blocks < 1 ? 1 : blocks > cap ? cap : blocks;
  return dim3(unsigned(blocks), unsigned(rows));
}

}  // namespace

void launch_covisibility(hipStream_t s, const MapFrame* tbl, const CovisPair* pairs, int n, long long max_pixels, const dvo_hip_covis_params& par,
                         unsigned long long* records) {
  k_covisibility<<<covis_grid(max_pixels, n), dim3(256), 0, s>>>(tbl, pairs, n, par, records);
}

}  // namespace dvo_hip
