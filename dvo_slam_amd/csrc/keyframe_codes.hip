// keyframe_codes.hip -- keyframes retrieved by appearance on the device (keyframe_codes.h; include/dvo_hip.h, dvo_hip_codebook_*).
//
// k_encode_frames: n frames at one level in ONE launch, whatever mix of sizes and cameras.  The frames are read through the frame table of
// the keyframe-map launches (MapFrame: the {I, Z} pairs of the level, 8 B apart in plane C or 16 B apart in the taps A).  The frame is the
// grid's y (walked where there are more frames than rows), a lane makes one WORD of the code: it reads its eight ferns (128 contiguous
// bytes), gathers per fern two 8-byte {I, Z} pairs (of the second only I is used), combines the eight nibbles in registers and writes the
// word with one plain 4-byte store, coalesced over the wavefront.  No atomics, no LDS.  Traffic: 16 m bytes of ferns (shared by all
// frames: cached), 16 m bytes gathered and m / 2 bytes written per frame.  A code has at most 256 words, so one workgroup of 256 lanes
// covers a frame and only m / 8 of its lanes work (16 at m = 128): the launch is latency-bound at any size, which is all it needs.
//
// k_code_search: Q query codes against the N stored codes, distances as a Q x N uint16 matrix (0xFFFF: dead or skipped).  The stored codes
// lie entry-major and are read with 16-byte loads; LPE = code_lanes_per_entry(m) lanes share an entry (16 at m = 512), so a wavefront
// covers 64 / LPE whole entries and a lane owns the 16-byte chunks c = sub, sub + LPE, ... of its entry.  A tile of up to 16 query codes
// (at most 16 KB) is staged in LDS once per workgroup and tile; every lane compares its chunk with the same chunk of every query of the
// tile (all groups of the wavefront read the same LDS addresses: broadcasts), counting two queries in the two halves of one register
// (a distance is at most 2048).  The counts are reduced across the LPE lanes of the group by xor shuffles, and lane `sub` of the group
// stores the distances of queries sub, sub + LPE, ...  Grid: x strides over the entries (walked beyond kSearchMaxBlocks workgroups), y
// is the query tile (at most 4096 queries / 16 = 256 tiles: one grid row each), so the stored codes are read once per tile of 16
// queries: once per launch for up to 16 queries, from L2 / the Infinity Cache for further tiles where the book fits.
//
// k_code_topk: one workgroup per query selects the k least (distance, id) of its matrix row by a radix select on the 36-bit key
// code_key(distance, id) -- three digits of 12 bits, each a histogram of 4096 bins in LDS (integer LDS atomics: counts, the same in any
// order) -- then collects the keys at or below the k-th and orders those (at most 64) by rank.  That READS THE ROW THREE TIMES (the
// distance digit, the high id digit, the collection) and 4096 entries of it once more (the low id digit: the ids the second digit left).
// Keys are unique, so the row is the stated one whatever order anything ran in; nothing waits or retries.
//
// k_gather_codes copies the book's own entries into the query buffer (dvo_hip_codebook_query_ids).
//
// Expected traffic of a search: N m / 2 bytes of codes read per tile of queries, 2 Q N bytes of distances written and read back three
// times by k_code_topk (from L2 / the Infinity Cache up to a few million entries), 8 k bytes of results per query.  By that model ONE
// query is bound by HBM (256 B per entry at m = 512) and a full tile of 16 queries by VALU (about six integer operations per word and
// query: xor, two shift-ors, and, popcount, add).  Both are DERIVED, not measured; k_code_topk uses one CU per query and is expected to
// dominate few queries against a very large book (profiles/keyframe_codes.md).
#include "global_ptr.h"
#include "launch.h"
#include "keyframe_codes.h"

namespace dvo_hip {

namespace {

typedef unsigned GlobalU32x4 __attribute__((ext_vector_type(4)));

constexpr int kSearchTile = 16;                // queries staged in LDS at a time
constexpr int kSearchMaxBlocks = 4096;
constexpr int kEncodeRows = 1024;

__global__ __launch_bounds__(256) void k_encode_frames(const MapFrame* __restrict__ tbl, int n, const Fern* __restrict__ ferns, int words,
                                                       uint32_t* __restrict__ out) {
  const int j = int(blockIdx.x * blockDim.x + threadIdx.x);     // the word of the code
  if (j >= words) return;
  Fern f[8];
  const auto fp = (Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(ferns));
  for (int i = 0; i < 8; ++i) {                                  // (8 j + i < 8 words = m: inside the table)
    const GlobalU32x4 r = fp[8 * j + i];
    f[i].u = uint16_t(r.x & 0xFFFFu);
    f[i].v = uint16_t(r.x >> 16);
    f[i].u2 = uint16_t(r.y & 0xFFFFu);
    f[i].v2 = uint16_t(r.y >> 16);
    f[i].t_i = __uint_as_float(r.z);
    f[i].t_z = __uint_as_float(r.w);
  }
  for (int item = int(blockIdx.y); item < n; item += int(gridDim.y)) {
    const MapFrame& F = tbl[item];                               // (item < n: inside the frame table)
    const int w = F.w, h = F.h;
    const size_t stride = size_t(F.stride);
    const auto P = (Global<const float>)global_ptr(F.iz);
    // the tap: code_position gives 0 <= x < w and 0 <= y < h, so y * w + x < w * h: inside the level
    const auto tap = [&](int x, int y) {
      const GlobalF32x2 t = *(Global<const GlobalF32x2>)(P + (size_t(y) * size_t(w) + size_t(x)) * stride);
      return CodeTap{t.x, t.y};
    };
    uint32_t word = 0u;
    for (int i = 0; i < 8; ++i) word |= fern_nibble(f[i], w, h, tap) << (4 * i);
    out[size_t(item) * size_t(words) + size_t(j)] = word;        // (item < n, j < words: inside the n codes)
  }
}

// NQ: the queries a tile holds (1, 4 or 16); LPE: lanes per entry (4, 8 or 16)
template <int LPE, int NQ>
__global__ __launch_bounds__(256) void k_code_search(const uint32_t* __restrict__ codes, const unsigned char* __restrict__ live, uint32_t n,
                                                     int chunks, const uint32_t* __restrict__ queries, int n_queries,
                                                     const uint2* __restrict__ skip, uint16_t* __restrict__ distances) {
  constexpr int kPairs = (NQ + 1) / 2;
  constexpr uint32_t kGroups = 256u / LPE;                       // entries a workgroup covers per step
  __shared__ GlobalU32x4 tile[NQ * 64];                          // [query][chunk], chunks <= 64
  const auto C = (Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(codes));
  const auto Qp = (Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(queries));
  const uint32_t sub = threadIdx.x % LPE, group = threadIdx.x / LPE;
  {
    const int q0 = int(blockIdx.y) * NQ, nq = n_queries - q0 < NQ ? n_queries - q0 : NQ;   // (a grid row per tile: q0 < n_queries)
    // (q0 + nq <= n_queries: inside the query buffer; i < nq * chunks <= NQ * 64: inside the tile)
    for (int i = int(threadIdx.x); i < nq * chunks; i += 256) tile[i] = Qp[size_t(q0) * size_t(chunks) + size_t(i)];
    __syncthreads();
    // the trip count is uniform over the workgroup: every lane reaches every shuffle
    for (uint32_t e0 = blockIdx.x * kGroups; e0 < n; e0 += gridDim.x * kGroups) {
      const uint32_t e = e0 + group;
      const bool inside = e < n;
      uint32_t acc[kPairs];
      for (int p = 0; p < kPairs; ++p) acc[p] = 0u;
      for (int c = int(sub); c < chunks; c += LPE) {
        // (e < n, c < chunks: inside the n stored codes)
        const GlobalU32x4 s = inside ? C[size_t(e) * size_t(chunks) + size_t(c)] : GlobalU32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const GlobalU32x4 r = tile[q * chunks + c];            // (q >= nq reads LDS nothing wrote: counted, never stored)
          const uint32_t d = (code_word_distance(s.x, r.x) + code_word_distance(s.y, r.y)) + (code_word_distance(s.z, r.z) + code_word_distance(s.w, r.w));
          acc[q >> 1] += d << (16 * (q & 1));
        }
      }
      for (int p = 0; p < kPairs; ++p)
        for (int m = LPE / 2; m > 0; m >>= 1) acc[p] += uint32_t(__shfl_xor(int(acc[p]), m, 64));   // (m < LPE: within the group)
      const bool alive = inside && live[e] != 0;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q % LPE == int(sub) && q < nq && inside) {
          const uint2 sk = skip[q0 + q];
          const uint32_t d = (acc[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
          // (q0 + q < n_queries, e < n: inside the n_queries x n matrix)
          distances[size_t(q0 + q) * size_t(n) + size_t(e)] = alive && !code_skipped(e, sk.x, sk.y) ? uint16_t(d) : kCodeMasked;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_code_topk(const uint16_t* __restrict__ distances, uint32_t n, int k, CodeMatch* __restrict__ rows) {
  __shared__ uint32_t hist[4096];
  __shared__ uint32_t part[256];
  __shared__ unsigned long long list[kCodeMaxK];
  __shared__ uint32_t found[2];                                  // the digit of the k-th key and how many keys are still wanted in it
  __shared__ uint32_t held;
  const uint32_t tid = threadIdx.x;
  const uint16_t* row = distances + size_t(blockIdx.x) * size_t(n);
  CodeMatch* out = rows + size_t(blockIdx.x) * size_t(k);
  unsigned long long prefix = 0ull;                              // the digits of the k-th key found so far
  uint32_t need = uint32_t(k);
  for (int pass = 0; pass < 3 && need > 0u; ++pass) {            // (need is the same in every thread)
    const int shift = 24 - 12 * pass;
    // the third pass: the ids with the twelve high bits found in the second
    const uint32_t lo = pass == 2 ? uint32_t(prefix & 0xFFFull) << 12 : 0u;
    const uint32_t hi = pass == 2 ? (lo + 4096u < n ? lo + 4096u : n) : n;
    for (uint32_t i = tid; i < 4096u; i += 256u) hist[i] = 0u;
    __syncthreads();
    for (uint32_t i = lo + tid; i < hi; i += 256u) {             // (i < n: inside the row)
      const uint32_t d = row[i];
      if (d == kCodeMasked) continue;
      const unsigned long long key = code_key(d, i);
      if (key >> (shift + 12) == prefix) atomicAdd(&hist[uint32_t(key >> shift) & 0xFFFu], 1u);
    }
    __syncthreads();
    uint32_t mine = 0u;
    for (uint32_t j = 0; j < 16u; ++j) mine += hist[tid * 16u + j];
    part[tid] = mine;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (uint32_t j = 0; j < 256u; ++j) {
      if (j == tid) before = total;
      total += part[j];
    }
    if (pass == 0 && total < need) need = total;                 // fewer than k qualify: all of them
    if (need > 0u && before < need && need <= before + mine) {   // exactly one thread: the k-th key lies in its sixteen bins
      uint32_t c = before;
      for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t here = hist[tid * 16u + j];
        if (c + here >= need) {
          found[0] = tid * 16u + j;
          found[1] = need - c;
          break;
        }
        c += here;
      }
    }
    __syncthreads();
    if (need > 0u) {
      prefix = prefix << 12 | found[0];
      need = found[1];
    }
    __syncthreads();                                             // (hist, part and found are written again)
  }
  // prefix is the k-th key (need ended at 1: keys are unique), or nothing qualifies
  const bool any = need > 0u;
  if (tid == 0u) held = 0u;
  __syncthreads();
  if (any) {
    const uint32_t last_d = uint32_t(prefix >> 24);
    for (uint32_t i = tid; i < n; i += 256u) {
      const uint32_t d = row[i];
      if (d == kCodeMasked || d > last_d) continue;
      const unsigned long long key = code_key(d, i);
      if (key <= prefix) {
        const uint32_t at = atomicAdd(&held, 1u);
        if (at < uint32_t(kCodeMaxK)) list[at] = key;            // (at most k <= 64 keys lie at or below the k-th)
      }
    }
  }
  __syncthreads();
  const uint32_t count = held < uint32_t(k) ? held : uint32_t(k);
  if (tid < count) {
    const unsigned long long key = list[tid];
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < count; ++j) rank += list[j] < key ? 1u : 0u;
    out[rank] = CodeMatch{uint32_t(key & 0xFFFFFFull), uint32_t(key >> 24)};   // (rank < count <= k: inside the row)
  }
  if (tid >= count && tid < uint32_t(k)) out[tid] = CodeMatch{kCodeNone, kCodeNone};
}

__global__ __launch_bounds__(256) void k_gather_codes(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ ids, int n, int words,
                                                      uint32_t* __restrict__ out) {
  const size_t total = size_t(n) * size_t(words);
  for (size_t i = size_t(blockIdx.x) * 256u + threadIdx.x; i < total; i += size_t(gridDim.x) * 256u) {
    const size_t q = i / size_t(words), j = i % size_t(words);   // (q < n; ids[q] < the book's size: checked before the launch)
    out[i] = codes[size_t(ids[q]) * size_t(words) + j];
  }
}

template <int LPE>
void search_tile(hipStream_t s, dim3 grid, int tile, const uint32_t* codes, const unsigned char* live, uint32_t n, int chunks, const uint32_t* queries,
                 int n_queries, const uint2* skip, uint16_t* distances) {
  if (tile == 1) k_code_search<LPE, 1><<<grid, dim3(256), 0, s>>>(codes, live, n, chunks, queries, n_queries, skip, distances);
  else if (tile == 4) k_code_search<LPE, 4><<<grid, dim3(256), 0, s>>>(codes, live, n, chunks, queries, n_queries, skip, distances);
  else k_code_search<LPE, kSearchTile><<<grid, dim3(256), 0, s>>>(codes, live, n, chunks, queries, n_queries, skip, distances);
}

}  // namespace

void launch_encode_frames(hipStream_t s, const MapFrame* tbl, int n, const dvo_hip_fern* ferns, int m, uint32_t* codes_out) {
  const int words = code_words(m);
  k_encode_frames<<<dim3(unsigned((words + 255) / 256), unsigned(n < kEncodeRows ? n : kEncodeRows)), dim3(256), 0, s>>>(tbl, n, ferns, words,
                                                                                                                       codes_out);
}

void launch_code_search(hipStream_t s, const uint32_t* codes, const unsigned char* live, uint32_t n, int m, const uint32_t* queries, int n_queries,
                        const uint32_t* skip, uint16_t* distances) {
  const int lpe = code_lanes_per_entry(m), chunks = m / 32;
  const int tile = n_queries == 1 ? 1 : n_queries <= 4 ? 4 : kSearchTile;
  const int tiles = (n_queries + tile - 1) / tile;
  const uint32_t per_block = 256u / uint32_t(lpe);
  const uint32_t blocks = (n + per_block - 1) / per_block;
  const dim3 grid(blocks < uint32_t(kSearchMaxBlocks) ? blocks : uint32_t(kSearchMaxBlocks), unsigned(tiles));   // (tiles <= 4096 / 16 = 256)
  const uint2* sk = reinterpret_cast<const uint2*>(skip);
  if (lpe == 16) search_tile<16>(s, grid, tile, codes, live, n, chunks, queries, n_queries, sk, distances);
  else if (lpe == 8) search_tile<8>(s, grid, tile, codes, live, n, chunks, queries, n_queries, sk, distances);
  else search_tile<4>(s, grid, tile, codes, live, n, chunks, queries, n_queries, sk, distances);
}

void launch_code_topk(hipStream_t s, const uint16_t* distances, uint32_t n, int n_queries, int k, dvo_hip_code_match* rows) {
  k_code_topk<<<dim3(unsigned(n_queries)), dim3(256), 0, s>>>(distances, n, k, rows);
}

void launch_gather_codes(hipStream_t s, const uint32_t* codes, const uint32_t* ids, int n, int m, uint32_t* out) {
  const size_t total = size_t(n) * size_t(code_words(m));
  const size_t blocks = (total + 255) / 256;
  k_gather_codes<<<dim3(unsigned(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s>>>(codes, ids, n, code_words(m), out);
}

}  // namespace dvo_hip
