// capi_codes.inc -- keyframes retrieved by appearance behind the C-ABI (include/dvo_hip.h, dvo_hip_codebook_* and dvo_hip_frames_encode;
// semantics: keyframe_codes.h; kernels: keyframe_codes.hip).  A book owns its codes, its fern table and a byte per entry that says whether
// it is alive.  The encoding calls read frames at a level (capi_frame_calls.inc); a query's codes lie in the context's scratch words, its
// skipped intervals (and, before them, the ids of dvo_hip_codebook_query_ids) in the side table, its distance matrix in front of the
// staged results.  Arguments are checked before anything is launched or changed.  Textually included by capi.hip inside its extern "C" block.
struct dvo_hip_codebook {
  dvo_hip_context* ctx = nullptr;
  int m = 0, capacity = 0, size = 0, live_count = 0;
  std::vector<Fern> ferns_host;
  std::vector<unsigned char> live_host;
  DevBuf codes, ferns, live;
};

namespace {

constexpr int kCodeMaxFrames = 1 << 20;                    // frames one encoding call takes

size_t code_bytes(const dvo_hip_codebook* b) { return size_t(code_words(b->m)) * sizeof(uint32_t); }

// the book, and -- out: the call's mandatory pointer beside it (codes, ids, an output), named in the message when it is missing
int check_book(dvo_hip_context* ctx, const dvo_hip_codebook* b, const char* who, const void* out = "", const char* out_name = "") {
  if (!ctx || !b) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null context or book");
  if (!out) return fail(ctx, DVO_HIP_ERR_INVALID, who, out_name);
  if (b->ctx != ctx) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a book of another context");
  return DVO_HIP_OK;
}

// the frames and the level of an encoding call
int check_code_frames(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, int level, const char* who) {
  int rc = check_frame_count(ctx, n, frames, who);
  if (rc != DVO_HIP_OK) return rc;
  if (n > kCodeMaxFrames) return fail(ctx, DVO_HIP_ERR_INVALID, who, "more than 2^20 frames");
  return check_frames_at_level(ctx, n, frames, level, 1, kMaxPixelBlocks, /*budget_early=*/true, who, [&](int, const dvo_hip_frame* f) -> int {
    if (f->lv[level].w <= 32767 && f->lv[level].h <= 32767) return DVO_HIP_OK;
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "the level is wider or higher than 32767 pixels");
  });
}

// what the three queries share; the room for n more entries
int check_query(dvo_hip_context* ctx, int n_queries, int k, const uint32_t* skip_from, const uint32_t* skip_to,
                const dvo_hip_code_match* results, const uint16_t* distances, int out_on_device, const char* who) {
  if (n_queries < 1 || !results) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (n_queries > kCodeMaxQueries) return fail(ctx, DVO_HIP_ERR_INVALID, who, "more than 4096 queries");
  if (k < 1 || k > kCodeMaxK) return fail(ctx, DVO_HIP_ERR_INVALID, who, "k must be 1 .. 64");
  if ((skip_from == nullptr) != (skip_to == nullptr)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "skip_from and skip_to go together");
  if (out_on_device && !aligned_to(results, 8)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "device result rows must be 8-byte aligned");
  if (out_on_device && distances && !aligned_to(distances, 2)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "device distances must be 2-byte aligned");
  return DVO_HIP_OK;
}
int check_room(dvo_hip_context* ctx, const dvo_hip_codebook* b, int n, const char* who) {
  if (n > b->capacity - b->size) return fail(ctx, DVO_HIP_ERR_CAPACITY, who, "the book is full");
  return DVO_HIP_OK;
}

// the codes of n checked frames into device memory `dst` (one launch on the main stream; not waited for)
int encode_frames(dvo_hip_context* ctx, const dvo_hip_codebook* b, int n, dvo_hip_frame* const* frames, int level, uint32_t* dst) {
  int blocks = 0;
  const int rc = upload_frames(ctx, n, frames, nullptr, level, nullptr, &blocks);
  if (rc != DVO_HIP_OK) return rc;
  launch_encode_frames(ctx->stream, ctx->frame_tbl.as<MapFrame>(), n, b->ferns.as<dvo_hip_fern>(), b->m, dst);
  DVO_HIP_TRY(ctx, hipGetLastError());
  ctx->codebook_encoded += n;
  return DVO_HIP_OK;
}

// n entries more, alive, their codes already in place (or on their way on the main stream); ids_out may be null
int book_grow(dvo_hip_context* ctx, dvo_hip_codebook* b, int n, uint32_t* ids_out) {
  std::fill(b->live_host.begin() + b->size, b->live_host.begin() + b->size + n, static_cast<unsigned char>(1));
  DVO_HIP_TRY(ctx, hipMemsetAsync(b->live.as<unsigned char>() + b->size, 1, size_t(n), ctx->stream));
  for (int i = 0; i < n && ids_out; ++i) ids_out[i] = uint32_t(b->size + i);
  b->size += n;
  b->live_count += n;
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
}

uint32_t* book_slot(const dvo_hip_codebook* b, int id) { return b->codes.as<uint32_t>() + size_t(id) * size_t(code_words(b->m)); }

// a query's table into the side table, through the ring of pinned slots like every other table there (at most 48 KB)
int upload_query_table(dvo_hip_context* ctx, const std::vector<uint32_t>& table) {
  const size_t bytes = table.size() * sizeof(uint32_t);
  DVO_HIP_TRY(ctx, ctx->side_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->side_tbl.p, table.data(), bytes));
  return DVO_HIP_OK;
}

// The query all three entry points end in: n_queries codes lie at the start of the scratch words.  The distances of a round of
// queries go straight into the caller's device matrix, else into the staging area, as many queries at a time as option
// "codebook_round_kb" holds (every offset below is the round's first query q0 times a row).
int run_query(dvo_hip_context* ctx, dvo_hip_codebook* b, int n_queries, int k, const uint32_t* skip_from, const uint32_t* skip_to,
              dvo_hip_code_match* results_out, uint16_t* distances_out, int out_on_device) {
  const uint32_t n = uint32_t(b->size);
  const uint32_t* queries = ctx->scratch_words.as<uint32_t>();
  std::vector<uint32_t> skip(size_t(n_queries) * 2, 0u);
  for (int q = 0; q < n_queries && skip_from; ++q) {
    skip[size_t(q) * 2] = skip_from[q];
    skip[size_t(q) * 2 + 1] = skip_to[q];
  }
  int rc = upload_query_table(ctx, skip);
  if (rc != DVO_HIP_OK) return rc;
  const size_t row_bytes = size_t(n) * sizeof(uint16_t), rows_bytes = size_t(n_queries) * size_t(k) * sizeof(dvo_hip_code_match);
  const bool direct = out_on_device && distances_out;            // the caller's matrix takes every round
  const size_t budget = size_t(ctx->opt_codebook_round_kb) * 1024;   // (option "codebook_round_kb")
  int per_round = n_queries;
  if (!direct && row_bytes * size_t(n_queries) > budget) {
    per_round = int(std::max<size_t>(budget / row_bytes, 1));    // (fewer than n_queries; at least one query, whatever the budget)
    if (per_round >= 16) per_round -= per_round % 16;            // whole tiles of 16 queries
  }
  // staging: the rounds' matrix, then the host-bound result rows
  const std::vector<ResultArray> results = {{results_out, rows_bytes, 8}};
  std::vector<void*> dev;
  rc = stage_results(ctx, results, out_on_device, &dev, /*scratch=*/direct ? 0 : row_bytes * size_t(per_round));
  if (rc != DVO_HIP_OK) return rc;
  dvo_hip_code_match* rows = static_cast<dvo_hip_code_match*>(dev[0]);
  for (int q0 = 0; q0 < n_queries; q0 += per_round) {
    const int nq = std::min(per_round, n_queries - q0);
    uint16_t* matrix = direct ? distances_out + size_t(q0) * size_t(n) : ctx->result_stage.as<uint16_t>();
    if (n > 0u)
      launch_code_search(ctx->stream, b->codes.as<uint32_t>(), b->live.as<unsigned char>(), n, b->m, queries + size_t(q0) * size_t(code_words(b->m)),
                         nq, ctx->side_tbl.as<uint32_t>() + size_t(q0) * 2, matrix);
    launch_code_topk(ctx->stream, matrix, n, nq, k, rows + size_t(q0) * size_t(k));
    DVO_HIP_TRY(ctx, hipGetLastError());
    if (distances_out && !direct && n > 0u)
      DVO_HIP_TRY(ctx, hipMemcpyAsync(distances_out + size_t(q0) * size_t(n), matrix, row_bytes * size_t(nq),
                                      out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  }
  ctx->codebook_queries += n_queries;
  return finish_results(ctx, results, out_on_device, dev);
}

}  // namespace

int dvo_hip_codebook_create(dvo_hip_context* ctx, int m, int capacity, uint64_t seed, const dvo_hip_fern* ferns_or_null, float z_lo, float z_hi,
                            dvo_hip_codebook** book_out) {
  DVO_LOCK(ctx);
  const char* who = "codebook_create";
  if (!ctx || !book_out) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (!code_ferns_ok(m)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "m must be a multiple of 128, 128 .. 2048");
  if (capacity < 1 || capacity > kCodeMaxCapacity) return fail(ctx, DVO_HIP_ERR_INVALID, who, "capacity must be 1 .. 2^24");
  if (!ferns_or_null && !(std::isfinite(z_lo) && std::isfinite(z_hi) && z_lo <= z_hi))
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "need finite z_lo <= z_hi");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<dvo_hip_codebook> b(new dvo_hip_codebook());
  b->ctx = ctx;
  b->m = m;
  b->capacity = capacity;
  b->ferns_host.resize(size_t(m));
  if (ferns_or_null) std::memcpy(b->ferns_host.data(), ferns_or_null, size_t(m) * sizeof(Fern));
  else fern_table(seed, m, z_lo, z_hi, b->ferns_host.data());
  b->live_host.assign(size_t(capacity), static_cast<unsigned char>(0));
  hipError_t e = b->codes.reserve(size_t(capacity) * code_bytes(b.get()));
  if (e == hipSuccess) e = b->ferns.reserve(size_t(m) * sizeof(Fern));
  if (e == hipSuccess) e = b->live.reserve(size_t(capacity));
  if (e == hipSuccess) e = hipMemcpyAsync(b->ferns.p, b->ferns_host.data(), size_t(m) * sizeof(Fern), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(b->live.p, 0, size_t(capacity), ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    for (DevBuf* d : {&b->codes, &b->ferns, &b->live}) d->release();
    DVO_HIP_TRY(ctx, e);
  }
  *book_out = b.release();
  return DVO_HIP_OK;
}

void dvo_hip_codebook_destroy(dvo_hip_context* ctx, dvo_hip_codebook* book) {
  DVO_LOCK(ctx);
  if (!book) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* d : {&book->codes, &book->ferns, &book->live}) d->release();
  delete book;
}

int dvo_hip_codebook_clear(dvo_hip_context* ctx, dvo_hip_codebook* book) {
  DVO_LOCK(ctx);
  const int rc = check_book(ctx, book, "codebook_clear");
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, hipMemsetAsync(book->live.p, 0, size_t(book->capacity), ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::fill(book->live_host.begin(), book->live_host.end(), static_cast<unsigned char>(0));
  book->size = 0;
  book->live_count = 0;
  return DVO_HIP_OK;
}

int dvo_hip_codebook_info(dvo_hip_context* ctx, const dvo_hip_codebook* book, int* m, int* capacity, int* size, int* live) {
  DVO_LOCK(ctx);
  const int rc = check_book(ctx, book, "codebook_info");
  if (rc != DVO_HIP_OK) return rc;
  if (m) *m = book->m;
  if (capacity) *capacity = book->capacity;
  if (size) *size = book->size;
  if (live) *live = book->live_count;
  return DVO_HIP_OK;
}

int dvo_hip_codebook_ferns(dvo_hip_context* ctx, const dvo_hip_codebook* book, dvo_hip_fern* ferns_out) {
  DVO_LOCK(ctx);
  const int rc = check_book(ctx, book, "codebook_ferns", ferns_out, "null ferns_out");
  if (rc != DVO_HIP_OK) return rc;
  std::memcpy(ferns_out, book->ferns_host.data(), size_t(book->m) * sizeof(Fern));
  return DVO_HIP_OK;
}

int dvo_hip_frames_encode(dvo_hip_context* ctx, const dvo_hip_codebook* book, int n, dvo_hip_frame* const* frames, int level,
                          uint32_t* codes_out, int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "frames_encode";
  int rc = check_book(ctx, book, who, codes_out, "null codes_out");
  if (rc == DVO_HIP_OK) rc = check_code_frames(ctx, n, frames, level, who);
  if (rc != DVO_HIP_OK) return rc;
  const std::vector<ResultArray> results = {{codes_out, size_t(n) * code_bytes(book), 4}};
  rc = check_results(ctx, results, out_on_device, who, "null codes_out", "device codes must be 4-byte aligned");
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<void*> dev;
  rc = stage_results(ctx, results, out_on_device, &dev);
  if (rc == DVO_HIP_OK) rc = encode_frames(ctx, book, n, frames, level, static_cast<uint32_t*>(dev[0]));
  if (rc != DVO_HIP_OK) return rc;
  return finish_results(ctx, results, out_on_device, dev);
}

int dvo_hip_codebook_add_frames(dvo_hip_context* ctx, dvo_hip_codebook* book, int n, dvo_hip_frame* const* frames, int level,
                                uint32_t* ids_out_or_null) {
  DVO_ENTER(ctx);
  const char* who = "codebook_add_frames";
  int rc = check_book(ctx, book, who);
  if (rc == DVO_HIP_OK) rc = check_code_frames(ctx, n, frames, level, who);
  if (rc == DVO_HIP_OK) rc = check_room(ctx, book, n, who);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = encode_frames(ctx, book, n, frames, level, book_slot(book, book->size));
  if (rc != DVO_HIP_OK) return rc;
  return book_grow(ctx, book, n, ids_out_or_null);
}

int dvo_hip_codebook_add_codes(dvo_hip_context* ctx, dvo_hip_codebook* book, int n, const uint32_t* codes, int on_device,
                               uint32_t* ids_out_or_null) {
  DVO_ENTER(ctx);
  const char* who = "codebook_add_codes";
  int rc = check_book(ctx, book, who, codes, "null codes");
  if (rc != DVO_HIP_OK) return rc;
  if (n < 1) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (on_device && !aligned_to(codes, 4)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "device codes must be 4-byte aligned");
  rc = check_room(ctx, book, n, who);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, hipMemcpyAsync(book_slot(book, book->size), codes, size_t(n) * code_bytes(book),
                                  on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  return book_grow(ctx, book, n, ids_out_or_null);
}

int dvo_hip_codebook_remove(dvo_hip_context* ctx, dvo_hip_codebook* book, int n, const uint32_t* ids) {
  DVO_ENTER(ctx);
  const char* who = "codebook_remove";
  const int rc = check_book(ctx, book, who, ids, "null ids");
  if (rc != DVO_HIP_OK) return rc;
  if (n < 1) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  for (int i = 0; i < n; ++i)
    if (ids[i] >= uint32_t(book->size)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "an id beyond the book's size");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < n; ++i) {
    if (!book->live_host[ids[i]]) continue;
    book->live_host[ids[i]] = 0;
    book->live_count -= 1;
  }
  // the entries' flags as a whole: one copy, whatever the number of ids
  DVO_HIP_TRY(ctx, hipMemcpyAsync(book->live.p, book->live_host.data(), size_t(book->size), hipMemcpyHostToDevice, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
}

int dvo_hip_codebook_read_codes(dvo_hip_context* ctx, const dvo_hip_codebook* book, int first, int n, uint32_t* codes_out, int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "codebook_read_codes";
  const int rc = check_book(ctx, book, who, codes_out, "null codes_out");
  if (rc != DVO_HIP_OK) return rc;
  if (n < 1 || first < 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (first > book->size || n > book->size - first) return fail(ctx, DVO_HIP_ERR_INVALID, who, "entries beyond the book's size");
  if (out_on_device && !aligned_to(codes_out, 4)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "device codes must be 4-byte aligned");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, hipMemcpyAsync(codes_out, book_slot(book, first), size_t(n) * code_bytes(book),
                                  out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
}

int dvo_hip_codebook_query_frames(dvo_hip_context* ctx, dvo_hip_codebook* book, int n_queries, dvo_hip_frame* const* frames, int level, int k,
                                  const uint32_t* skip_from_or_null, const uint32_t* skip_to_or_null, dvo_hip_code_match* results_out,
                                  uint16_t* distances_out_or_null, int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "codebook_query_frames";
  int rc = check_book(ctx, book, who);
  if (rc == DVO_HIP_OK) rc = check_query(ctx, n_queries, k, skip_from_or_null, skip_to_or_null, results_out, distances_out_or_null, out_on_device, who);
  if (rc == DVO_HIP_OK) rc = check_code_frames(ctx, n_queries, frames, level, who);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, ctx->scratch_words.reserve(size_t(n_queries) * code_bytes(book)));
  rc = encode_frames(ctx, book, n_queries, frames, level, ctx->scratch_words.as<uint32_t>());
  if (rc != DVO_HIP_OK) return rc;
  return run_query(ctx, book, n_queries, k, skip_from_or_null, skip_to_or_null, results_out, distances_out_or_null, out_on_device);
}

int dvo_hip_codebook_query_codes(dvo_hip_context* ctx, dvo_hip_codebook* book, int n_queries, const uint32_t* codes, int codes_on_device, int k,
                                 const uint32_t* skip_from_or_null, const uint32_t* skip_to_or_null, dvo_hip_code_match* results_out,
                                 uint16_t* distances_out_or_null, int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "codebook_query_codes";
  int rc = check_book(ctx, book, who, codes, "null codes");
  if (rc == DVO_HIP_OK) rc = check_query(ctx, n_queries, k, skip_from_or_null, skip_to_or_null, results_out, distances_out_or_null, out_on_device, who);
  if (rc != DVO_HIP_OK) return rc;
  if (codes_on_device && !aligned_to(codes, 4)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "device codes must be 4-byte aligned");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t bytes = size_t(n_queries) * code_bytes(book);
  DVO_HIP_TRY(ctx, ctx->scratch_words.reserve(bytes));
  // (the kernel stages its queries with 16-byte loads: they go through the scratch whatever the caller's alignment)
  DVO_HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_words.p, codes, bytes, codes_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  if (!codes_on_device) DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the caller's host array)
  return run_query(ctx, book, n_queries, k, skip_from_or_null, skip_to_or_null, results_out, distances_out_or_null, out_on_device);
}

int dvo_hip_codebook_query_ids(dvo_hip_context* ctx, dvo_hip_codebook* book, int n_queries, const uint32_t* ids, int k,
                               const uint32_t* skip_from_or_null, const uint32_t* skip_to_or_null, dvo_hip_code_match* results_out,
                               uint16_t* distances_out_or_null, int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "codebook_query_ids";
  int rc = check_book(ctx, book, who, ids, "null ids");
  if (rc == DVO_HIP_OK) rc = check_query(ctx, n_queries, k, skip_from_or_null, skip_to_or_null, results_out, distances_out_or_null, out_on_device, who);
  if (rc != DVO_HIP_OK) return rc;
  for (int q = 0; q < n_queries; ++q)
    if (ids[q] >= uint32_t(book->size)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "an id beyond the book's size");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, ctx->scratch_words.reserve(size_t(n_queries) * code_bytes(book)));
  // the ids go through the side table as a table of their own; run_query's table replaces it behind the gather, on the same stream
  // (reserved for that larger table now, so that nothing is reallocated between the two)
  DVO_HIP_TRY(ctx, ctx->side_tbl.reserve(size_t(n_queries) * 2 * sizeof(uint32_t)));
  rc = upload_query_table(ctx, std::vector<uint32_t>(ids, ids + n_queries));
  if (rc != DVO_HIP_OK) return rc;
  const uint32_t* dev_ids = ctx->side_tbl.as<uint32_t>();
  launch_gather_codes(ctx->stream, book->codes.as<uint32_t>(), dev_ids, n_queries, book->m, ctx->scratch_words.as<uint32_t>());
  DVO_HIP_TRY(ctx, hipGetLastError());
  return run_query(ctx, book, n_queries, k, skip_from_or_null, skip_to_or_null, results_out, distances_out_or_null, out_on_device);
}
