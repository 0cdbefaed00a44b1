// cache_policy.hip -- does any cache policy of a streaming kernel keep its lines from displacing a table that another kernel re-reads
// out of the 256 MB Infinity Cache?  (The frame build beside the coarse levels: DESIGN.md section 10.)
//
// A: one pass over a 160 MB table (16 B per lane, default policy), the coarse levels' taps.
// B: a copy of 1 GiB into another 1 GiB, 256 workgroups of 256 lanes (the build's grid), with the cache policy of its loads and its
//    stores set per variant: the buffer instructions' `aux` operand (bit 0 = sc0, bit 1 = nt, bit 4 = sc1 on gfx950: the disassembly
//    of this file prints them as `sc0` / `nt` / `sc1`), or __builtin_nontemporal_load / _store on global pointers.
//
// Modes:
//   serial      per variant: (A, B over CHUNK bytes) x PASSES on one stream; A's time per pass from events around each A launch.
//               "A alone" = A behind A.  This is also the form for a separate --pmc FETCH_SIZE run: A is instantiated per variant,
//               so the counter rows of k_table<V> are those of the A passes behind variant V.
//   concurrent  per variant: B (long, on a lowest-priority stream) and 200 back-to-back A passes on a highest-priority stream beside it.
//
// usage: cache_policy serial [chunk_mb=320] [passes=20] | concurrent [passes=200]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                         \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      std::printf("%s failed: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);     \
      std::exit(1);                                                                      \
    }                                                                                    \
  } while (0)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int kUnroll = 4;
constexpr int kThreads = 256;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// A: one pass over the table; V only names the instantiation (the variant of B in front of it)
template <int V>
__global__ __launch_bounds__(kThreads) void k_table(const u32x4* table, unsigned n16, unsigned* out) {
  const __amdgpu_buffer_rsrc_t t = rsrc(table, n16 * 16u);
  unsigned s = 0;
  for (unsigned i = blockIdx.x * kThreads * kUnroll + threadIdx.x; i < n16; i += gridDim.x * kThreads * kUnroll) {
    u32x4 v[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) v[k] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(t, (i + k * kThreads) * 16u, 0, 0));
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) s ^= v[k].x + v[k].y + v[k].z + v[k].w;
  }
  if (s == 0x9e3779b9u) out[0] = s;   // never true for the zero-filled table: keeps the loads
}

// B: copy n16 elements, reps times; buffer out-of-range loads read 0 and stores are dropped, the i < n16 guard keeps it in range anyway
template <int LAUX, int SAUX, bool NTB>
__global__ __launch_bounds__(kThreads) void k_stream(const u32x4* src, u32x4* dst, unsigned n16, int reps) {
  const __amdgpu_buffer_rsrc_t s = rsrc(src, n16 * 16u), d = rsrc(dst, n16 * 16u);
  for (int r = 0; r < reps; ++r)
    for (unsigned i = blockIdx.x * kThreads * kUnroll + threadIdx.x; i < n16; i += gridDim.x * kThreads * kUnroll) {
      u32x4 v[kUnroll];
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const unsigned j = i + k * kThreads;
        if (NTB) v[k] = j < n16 ? __builtin_nontemporal_load(src + j) : u32x4{0, 0, 0, 0};
        else v[k] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(s, j * 16u, 0, LAUX));
      }
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const unsigned j = i + k * kThreads;
        if (j >= n16) break;
        if (NTB) __builtin_nontemporal_store(v[k], dst + j);
        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v[k]), d, j * 16u, 0, SAUX);
      }
    }
}

struct Variant {
  const char* name;
  void (*stream)(const u32x4*, u32x4*, unsigned, int, hipStream_t);
  void (*table)(const u32x4*, unsigned, unsigned*, hipStream_t);
};

template <int LAUX, int SAUX, bool NTB>
static void launch_stream(const u32x4* s, u32x4* d, unsigned n16, int reps, hipStream_t st) {
  k_stream<LAUX, SAUX, NTB><<<256, kThreads, 0, st>>>(s, d, n16, reps);
}
template <int V>
static void launch_table(const u32x4* t, unsigned n16, unsigned* out, hipStream_t st) {
  k_table<V><<<2048, kThreads, 0, st>>>(t, n16, out);
}

#define VARIANT(v, name, l, s, ntb) Variant{name, launch_stream<l, s, ntb>, launch_table<v>}
static const Variant kVariants[] = {
    VARIANT(1, "default (aux 0 / 0)", 0, 0, false),
    VARIANT(2, "nt (aux 2 / 2)", 2, 2, false),
    VARIANT(3, "sc0 (aux 1 / 1)", 1, 1, false),
    VARIANT(4, "sc1 (aux 16 / 16)", 16, 16, false),
    VARIANT(5, "sc0 sc1 (aux 17 / 17)", 17, 17, false),
    VARIANT(6, "sc0 nt (aux 3 / 3)", 3, 3, false),
    VARIANT(7, "sc1 nt (aux 18 / 18)", 18, 18, false),
    VARIANT(8, "sc0 sc1 nt (aux 19 / 19)", 19, 19, false),
    VARIANT(9, "loads nt, stores default (2 / 0)", 2, 0, false),
    VARIANT(10, "loads default, stores nt (0 / 2)", 0, 2, false),
    VARIANT(11, "__builtin_nontemporal_load/store", 0, 0, true),
};

static float elapsed(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  CHECK(hipEventElapsedTime(&ms, a, b));
  return ms;
}

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char** argv) {
  const bool serial = argc < 2 || std::strcmp(argv[1], "concurrent") != 0;
  const size_t table_bytes = size_t(160) << 20;    // 168 MB
  const size_t big_bytes = size_t(1) << 30;
  const unsigned table16 = unsigned(table_bytes / 16), big16 = unsigned(big_bytes / 16);
  u32x4 *table, *src, *dst, *flush;
  unsigned* out;
  CHECK(hipMalloc(&table, table_bytes));
  CHECK(hipMalloc(&src, big_bytes));
  CHECK(hipMalloc(&dst, big_bytes));
  CHECK(hipMalloc(&flush, big_bytes));
  CHECK(hipMalloc(&out, 4));
  CHECK(hipMemset(table, 0, table_bytes));
  CHECK(hipMemset(src, 0, big_bytes));
  CHECK(hipMemset(dst, 0, big_bytes));
  CHECK(hipMemset(flush, 0, big_bytes));
  int lo, hi;
  CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  hipStream_t sa, sb;
  CHECK(hipStreamCreateWithPriority(&sa, hipStreamNonBlocking, hi));
  CHECK(hipStreamCreateWithPriority(&sb, hipStreamNonBlocking, lo));
  hipEvent_t e0, e1, e2, e3;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  CHECK(hipEventCreate(&e2));
  CHECK(hipEventCreate(&e3));
  const double table_mb = table_bytes / 1e6;

  if (serial) {
    const size_t chunk_mb = argc > 2 ? std::atoi(argv[2]) : 320;
    const int passes = argc > 3 ? std::atoi(argv[3]) : 20;
    const unsigned chunk16 = unsigned(std::min(chunk_mb * 1000000 / 32, size_t(big16)));   // read chunk/2, write chunk/2
    std::printf("# serial: A = one pass over a %.0f MB table, B = copy of %.0f MB into %.0f MB (%.0f MB streamed) between two A passes, "
                "%d passes per variant; medians\n", table_mb, chunk16 * 16 / 1e6, chunk16 * 16 / 1e6, chunk16 * 32 / 1e6, passes);
    std::printf("%-36s %10s %10s %12s\n", "B's policy (loads / stores)", "A us/pass", "A TB/s", "B TB/s");
    // A alone: A behind A (the table's second and later passes)
    {
      std::vector<double> ta;
      for (int p = 0; p < passes + 2; ++p) {
        CHECK(hipEventRecord(e0, sa));
        launch_table<0>(table, table16, out, sa);
        CHECK(hipEventRecord(e1, sa));
        CHECK(hipEventSynchronize(e1));
        if (p >= 2) ta.push_back(1e3 * elapsed(e0, e1));
      }
      const double a = median(ta);
      std::printf("%-36s %10.1f %10.2f %12s\n", "A alone (A behind A)", a, table_bytes / a / 1e6, "-");
    }
    // A cold: behind a 1 GiB default-policy copy
    {
      std::vector<double> ta;
      for (int p = 0; p < passes; ++p) {
        launch_stream<0, 0, false>(src, flush, big16, 1, sa);
        CHECK(hipEventRecord(e0, sa));
        launch_table<0>(table, table16, out, sa);
        CHECK(hipEventRecord(e1, sa));
        CHECK(hipEventSynchronize(e1));
        ta.push_back(1e3 * elapsed(e0, e1));
      }
      const double a = median(ta);
      std::printf("%-36s %10.1f %10.2f %12s\n", "A cold (behind a 2 GiB default copy)", a, table_bytes / a / 1e6, "-");
    }
    for (const Variant& v : kVariants) {
      std::vector<double> ta, tb;
      v.table(table, table16, out, sa);
      for (int p = 0; p < passes; ++p) {
        CHECK(hipEventRecord(e2, sa));
        v.stream(src, dst, chunk16, 1, sa);
        CHECK(hipEventRecord(e0, sa));
        v.table(table, table16, out, sa);
        CHECK(hipEventRecord(e1, sa));
        CHECK(hipEventSynchronize(e1));
        ta.push_back(1e3 * elapsed(e0, e1));
        tb.push_back(1e3 * elapsed(e2, e0));
      }
      const double a = median(ta), b = median(tb);
      std::printf("%-36s %10.1f %10.2f %12.2f\n", v.name, a, table_bytes / a / 1e6, chunk16 * 32.0 / b / 1e6);
    }
  } else {
    const int passes = argc > 2 ? std::atoi(argv[2]) : 200;
    std::printf("# concurrent: B = 256-workgroup copy of 1 GiB into 1 GiB, repeated, on the lowest-priority stream; A = %d back-to-back "
                "passes over a %.0f MB table on the highest-priority stream beside it\n", passes, table_mb);
    std::printf("%-36s %10s %10s %12s %10s\n", "B's policy (loads / stores)", "A us/pass", "A TB/s", "B TB/s", "B outlasts");
    for (int p = 0; p < 3; ++p) launch_table<0>(table, table16, out, sa);
    CHECK(hipEventRecord(e0, sa));
    for (int p = 0; p < passes; ++p) launch_table<0>(table, table16, out, sa);
    CHECK(hipEventRecord(e1, sa));
    CHECK(hipEventSynchronize(e1));
    const double alone = 1e3 * elapsed(e0, e1) / passes;
    std::printf("%-36s %10.1f %10.2f %12s %10s\n", "A alone", alone, table_bytes / alone / 1e6, "-", "-");
    for (const Variant& v : kVariants) {
      // B's reps sized to outlast A's loop: a copy pass of 2 GiB takes >= 0.35 ms
      const int reps = std::max(4, int(passes * alone * 1.5 / 350.0) + 4);
      CHECK(hipEventRecord(e2, sb));
      v.stream(src, dst, big16, reps, sb);
      CHECK(hipEventRecord(e3, sb));
      for (int p = 0; p < 3; ++p) v.table(table, table16, out, sa);
      CHECK(hipEventRecord(e0, sa));
      for (int p = 0; p < passes; ++p) v.table(table, table16, out, sa);
      CHECK(hipEventRecord(e1, sa));
      CHECK(hipStreamSynchronize(sa));
      CHECK(hipStreamSynchronize(sb));
      const double a = 1e3 * elapsed(e0, e1) / passes, b = elapsed(e2, e3);
      const bool outlasts = elapsed(e2, e3) > elapsed(e2, e1);
      std::printf("%-36s %10.1f %10.2f %12.2f %10s\n", v.name, a, table_bytes / a / 1e6, reps * 2.0 * big_bytes / b / 1e9, outlasts ? "yes" : "NO");
    }
  }
  CHECK(hipDeviceSynchronize());
  return 0;
}
