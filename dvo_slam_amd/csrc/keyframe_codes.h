// keyframe_codes.h -- keyframes retrieved by APPEARANCE: randomised fern codes and their search (include/dvo_hip.h, dvo_hip_codebook_*;
// Glocker, Shotton, Criminisi, Izadi: "Real-Time RGB-D Camera Relocalization via Randomized Ferns for Keyframe Encoding", TVCG 2015).
// The reference has no such routine: NearestNeighborConstraintSearch::findPossibleConstraints (dvo_slam/src/keyframe_constraint_search.cpp:41-72)
// radius-searches the keyframes' translations, and dvo_hip_frames_covisibility (covisibility.h) classifies pixels under a transform the
// caller supplies -- both need a pose to start from.  A lost tracker, a loop that closes after drift and two sessions without common
// coordinates have none.  This header states what answers them, once, for the kernels (keyframe_codes.hip) and for the host compiler of
// the CPU tier (tests/test_keyframe_codes.py): comparisons and integer counts only -- NO arithmetic is done on a sample -- so the device
// codes, distances and result rows EQUAL the host build's, in any order.
//
// A FERN is {uint16 u, v, u2, v2; float t_i, t_z}, 16 bytes.  The positions are fractions of the image, so one table serves every frame
// size and camera: on a level of w x h pixels  x = (u * w) >> 16, y = (v * h) >> 16, and likewise x2, y2 from u2, v2 -- always inside the
// level (u < 2^16).  The NIBBLE of a fern on the level's planes {I, Z}:
//   bit 0   I(x, y) > t_i
//   bit 1   I(x, y) > I(x2, y2)           (holds under a change of exposure)
//   bit 2   Z(x, y) is finite and > t_z
//   bit 3   Z(x, y) is finite
// A comparison with NaN is false.  The CODE of a frame is m nibbles packed eight to a 32-bit word, fern 8 j + i in bits 4 i .. 4 i + 3 of
// word j; m is a multiple of 128, 128 <= m <= 2048: a code is a multiple of 64 bytes and at most 1 KB.
//
// The default table is fern_table(seed, m, z_lo, z_hi): a splitmix64 stream started at `seed`, two draws per fern.  Draw 1 gives the
// positions, 16 bits each from the low end: u, v, u2, v2.  Draw 2 gives t_i = float(32 + (low 32 bits) % 192) grey levels and, with r16 =
// bits 32 .. 47, t_z = z_lo + ((z_hi - z_lo) * float(r16)) / 65536 in float.  The table is computed on the host and uploaded.
//
// The DISTANCE of two codes is the number of ferns whose nibbles differ in any bit (Glocker's BlockHD times m): per word, with x = a ^ b,
// popcount((x | x >> 1 | x >> 2 | x >> 3) & 0x11111111).  0 .. m.
//
// The ANSWER to a query is the k live entries, outside the query's skipped id interval [skip_from, skip_to), of least (distance, id): a
// tie in distance goes to the lower id.  A row is k records {uint32 id, uint32 distance}, ascending, padded with {0xFFFFFFFF, 0xFFFFFFFF}
// where fewer than k qualify.  In the distance matrix (uint16, queries x entries) a dead or skipped entry is 0xFFFF.  codes_topk_host
// produces both: the yardstick.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hd_compat.h"
#include "../../include/dvo_hip.h"

namespace dvo_hip {

typedef dvo_hip_fern Fern;                     // {u, v, u2, v2, t_i, t_z}
typedef dvo_hip_code_match CodeMatch;          // {id, distance}
static_assert(sizeof(Fern) == 16, "a fern is 16 bytes");
static_assert(sizeof(CodeMatch) == 8, "a result record is 8 bytes");

constexpr int kCodeMinFerns = 128, kCodeMaxFerns = 2048, kCodeFernStep = 128;
constexpr int kCodeMaxK = 64, kCodeMaxQueries = 4096, kCodeMaxCapacity = 1 << 24;
constexpr uint32_t kCodeNone = 0xFFFFFFFFu;    // the id and the distance of a padding record
constexpr uint16_t kCodeMasked = 0xFFFFu;      // a dead or skipped entry in the distance matrix

DVO_HD bool code_ferns_ok(int m) { return m >= kCodeMinFerns && m <= kCodeMaxFerns && m % kCodeFernStep == 0; }
DVO_HD int code_words(int m) { return m / 8; }

// one sample of a level: what a fern reads
struct CodeTap {
  float I, Z;
};

// finite: neither NaN nor an infinity (a comparison, no arithmetic)
DVO_HD bool code_finite(float z) { return fabsf(z) <= 3.402823466e+38f; }

// x = (u * w) >> 16: 0 <= x < w for 0 <= u < 2^16 and 1 <= w < 2^15
DVO_HD int code_position(uint32_t u, int extent) { return int((u * uint32_t(extent)) >> 16); }

// The nibble of fern f on a level of w x h pixels; tap(x, y) returns the CodeTap of pixel (x, y), 0 <= x < w, 0 <= y < h.
template <class Tap>
DVO_HD uint32_t fern_nibble(const Fern& f, int w, int h, const Tap& tap) {
  const CodeTap a = tap(code_position(f.u, w), code_position(f.v, h));
  const CodeTap b = tap(code_position(f.u2, w), code_position(f.v2, h));
  const bool known = code_finite(a.Z);
  return (a.I > f.t_i ? 1u : 0u) | (a.I > b.I ? 2u : 0u) | (known && a.Z > f.t_z ? 4u : 0u) | (known ? 8u : 0u);
}

// word j of a frame's code: ferns 8 j .. 8 j + 7
template <class Tap>
DVO_HD uint32_t fern_word(const Fern* ferns, int j, int w, int h, const Tap& tap) {
  uint32_t word = 0u;
  for (int i = 0; i < 8; ++i) word |= fern_nibble(ferns[8 * j + i], w, h, tap) << (4 * i);
  return word;
}

// the ferns of two words whose nibbles differ
DVO_HD uint32_t code_word_distance(uint32_t a, uint32_t b) {
  const uint32_t x = a ^ b;
  return uint32_t(__builtin_popcount((x | x >> 1 | x >> 2 | x >> 3) & 0x11111111u));
}

DVO_HD uint32_t code_distance(const uint32_t* a, const uint32_t* b, int words) {
  uint32_t d = 0u;
  for (int j = 0; j < words; ++j) d += code_word_distance(a[j], b[j]);
  return d;
}

// id in [from, to): left out of this query's answer (from >= to: nothing is)
DVO_HD bool code_skipped(uint32_t id, uint32_t from, uint32_t to) { return id >= from && id < to; }

// (distance, id) as one ascending key: the distance above the 24 bits of an id (ids stay below 2^24: kCodeMaxCapacity)
DVO_HD uint64_t code_key(uint32_t distance, uint32_t id) { return uint64_t(distance) << 24 | uint64_t(id); }

// ---- host only: the table's generator, the encoding of one frame and the yardstick of a query ---------------------------------------------

inline uint64_t code_splitmix64(uint64_t* state) {
  uint64_t z = (*state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the default fern table: m ferns into out
inline void fern_table(uint64_t seed, int m, float z_lo, float z_hi, Fern* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  uint64_t state = seed;
  for (int i = 0; i < m; ++i) {
    const uint64_t p = code_splitmix64(&state), t = code_splitmix64(&state);
    out[i].u = uint16_t(p & 0xFFFFu);
    out[i].v = uint16_t((p >> 16) & 0xFFFFu);
    out[i].u2 = uint16_t((p >> 32) & 0xFFFFu);
    out[i].v2 = uint16_t((p >> 48) & 0xFFFFu);
    out[i].t_i = float(32u + uint32_t(t & 0xFFFFFFFFu) % 192u);
    const float span = z_hi - z_lo, r16 = float(uint32_t((t >> 32) & 0xFFFFu));
    const float scaled = span * r16;
    out[i].t_z = z_lo + scaled / 65536.0f;
  }
}

// the code of one frame over tight planes I, Z of w x h pixels: m / 8 words into out
inline void encode_frame_host(const float* I, const float* Z, int w, int h, const Fern* ferns, int m, uint32_t* out) {
  const auto tap = [&](int x, int y) { return CodeTap{I[size_t(y) * size_t(w) + size_t(x)], Z[size_t(y) * size_t(w) + size_t(x)]}; };
  for (int j = 0; j < code_words(m); ++j) out[j] = fern_word(ferns, j, w, h, tap);
}

// The rows of n_queries queries against n stored codes (entry-major, m / 8 words each; live[i] != 0: entry i is alive).  skip_from /
// skip_to: per query, or null (nothing skipped).  rows: n_queries x k records; distances (may be null): n_queries x n.
inline void codes_topk_host(const uint32_t* codes, const unsigned char* live, int n, int m, const uint32_t* queries, int n_queries,
                            const uint32_t* skip_from, const uint32_t* skip_to, int k, CodeMatch* rows, uint16_t* distances) {
  const int words = code_words(m);
  for (int q = 0; q < n_queries; ++q) {
    CodeMatch* row = rows + size_t(q) * size_t(k);
    int held = 0;
    const uint32_t from = skip_from ? skip_from[q] : 0u, to = skip_to ? skip_to[q] : 0u;
    for (int i = 0; i < n; ++i) {
      const bool out = !live[i] || code_skipped(uint32_t(i), from, to);
      const uint32_t d = out ? kCodeNone : code_distance(queries + size_t(q) * size_t(words), codes + size_t(i) * size_t(words), words);
      if (distances) distances[size_t(q) * size_t(n) + size_t(i)] = out ? kCodeMasked : uint16_t(d);
      if (out) continue;
      // ids ascend, so an entry goes behind every held record of its distance: insertion keeps (distance, id) ascending
      int at = held;
      while (at > 0 && row[at - 1].distance > d) --at;
      if (at >= k) continue;
      for (int j = (held < k ? held : k - 1); j > at; --j) row[j] = row[j - 1];
      row[at] = CodeMatch{uint32_t(i), d};
      if (held < k) ++held;
    }
    for (int j = held; j < k; ++j) row[j] = CodeMatch{kCodeNone, kCodeNone};
  }
}

// ---- what the kernels of keyframe_codes.hip take (the launches: below) ---------------------------------------------------------------------

// lanes that share one stored code in k_code_search: the largest power of two that divides the code's 16-byte chunks (m / 32), at most
// 16 -- 16 at m = 512, 4 at m = 128 and m = 384
DVO_HD int code_lanes_per_entry(int m) {
  const int chunks = m / 32;
  return chunks % 16 == 0 ? 16 : chunks % 8 == 0 ? 8 : 4;
}

}  // namespace dvo_hip
