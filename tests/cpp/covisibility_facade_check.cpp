// The C++ facade's loop-closure proposal by covisibility (include/dvo_slam/keyframe_covisibility.h, dvo_slam::CovisibilityConstraintSearch;
// include/dvo_hip.h, dvo_hip_frames_covisibility): usage: covisibility_facade_check <output file>.
//  1. five keyframes of 64 x 48 (the formulas of tests/test_gpu_frame_warp.py::facade_frame) under poses that are translations by
//     dyadic fractions: the inverse and the product of two poses are exact in double, so the transforms equal the Python wrappers';
//  2. with minOverlap == 0 the search returns the reference's radius set in the order of `all`, the query itself included;
//  3. with minOverlap > 0 the set comes back filtered and ranked;
//  4. compute() returns the raw records of a pair list; a pair that names no keyframe is refused through the error handler;
//  5. the records go to the output file (32 bytes each) and the candidate ids to the standard output ("radius: ...", "ranked: ...") for
//     the test to compare with dvo_slam_amd.covisibility_batch and loop_closure_candidates.
// Prints "ok" last, or the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dvo_slam/keyframe_covisibility.h"

using namespace dvo::core;

namespace {

const int W = 64, H = 48, LEVEL = 1, N = 5;
const double POSITIONS[N][3] = {{0.0, 0.0, 0.0}, {0.0625, 0.0, 0.0}, {0.125, 0.03125, 0.0}, {4.0, 0.0, 0.0}, {0.0, -0.0625, -0.25}};
int refusals = 0;

void count_refusal(const char*, const char*) { ++refusals; }

void frame(int k, dvo::compat::ImageMat& I, dvo::compat::ImageMat& Z) {
  I = dvo::compat::image_create(H, W);
  Z = dvo::compat::image_create(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      i[y * W + x] = float((x * 7 + y * 13 + k * 5) % 256);
      z[y * W + x] = (x / 2 + 2 * (y / 2) + k) % 29 == 0 ? NAN : float(1000 + (x * 3 + y * 5 + k * 11) % 512) * 0.001f;
    }
}

void print_ids(const char* label, const dvo_slam::KeyframeVector& v) {
  std::printf("%s:", label);
  for (size_t i = 0; i < v.size(); ++i) std::printf(" %d", int(v[i]->id()));
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: covisibility_facade_check <file>\n"); return 2; }
  const IntrinsicMatrix K = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, K);
  camera.build(3);
  dvo_slam::KeyframeVector all;
  for (int k = 0; k < N; ++k) {
    dvo::compat::ImageMat I, Z;
    frame(k, I, Z);
    RgbdImagePyramidPtr image = camera.create(I, Z);
    image->build(3);
    AffineTransformd pose;
    pose.setIdentity();
    for (int r = 0; r < 3; ++r) pose.matrix()(r, 3) = POSITIONS[k][r];
    dvo_slam::KeyframePtr keyframe(new dvo_slam::Keyframe());
    keyframe->id(short(k)).image(image).pose(pose);
    all.push_back(keyframe);
  }

  // 2. the reference's radius set
  dvo_slam::CovisibilityConstraintSearch search(1.0f);
  if (search.maxDistance() != 1.0f || search.minOverlap() != 0.0f || search.level() != 2) { std::printf("the accessors\n"); return 1; }
  search.level(LEVEL);
  dvo_slam::KeyframeVector radius;
  search.findPossibleConstraints(all, all[0], radius);
  if (radius.size() != 4 || radius[0] != all[0] || radius[1] != all[1] || radius[2] != all[2] || radius[3] != all[4]) {
    print_ids("the radius set is", radius);
    return 1;
  }
  dvo_slam::KeyframeVector far;
  search.findPossibleConstraints(all, all[3], far);
  if (far.size() != 1 || far[0] != all[3]) { print_ids("the far keyframe's radius set is", far); return 1; }
  search.maxDistance(4.0f);                                      // (keyframe 0 is 4 m away: a distance equal to the radius is inside)
  far.clear();
  search.findPossibleConstraints(all, all[3], far);
  if (far.size() != 4 || far[0] != all[0] || far[1] != all[1] || far[2] != all[2] || far[3] != all[3]) {
    print_ids("at radius 4 the set is", far);
    return 1;
  }
  search.maxDistance(1.0f);
  print_ids("radius", radius);

  // 3. filtered and ranked
  search.minOverlap(0.05f);
  dvo_slam::KeyframeVector ranked;
  search.findPossibleConstraints(all, all[0], ranked);
  if (ranked.empty() || ranked[0] != all[0] || ranked.size() > radius.size()) { print_ids("ranked", ranked); return 1; }
  print_ids("ranked", ranked);
  search.minOverlap(0.999f);
  dvo_slam::KeyframeVector best;
  search.findPossibleConstraints(all, all[0], best);
  if (best.size() != 1 || best[0] != all[0]) { print_ids("only the query overlaps itself entirely, got", best); return 1; }

  // 4. raw records
  typedef dvo_slam::CovisibilityConstraintSearch::Pair Pair;
  std::vector<Pair> pairs = {Pair(0, 1), Pair(1, 0), Pair(0, 0), Pair(2, 4), Pair(4, 2), Pair(3, 0)};
  std::vector<dvo_slam::CovisibilityConstraintSearch::Record> records;
  if (!dvo_slam::CovisibilityConstraintSearch::compute(all, pairs, LEVEL, 0, records) || records.size() != pairs.size()) {
    std::printf("compute failed\n");
    return 1;
  }
  for (size_t k = 0; k < records.size(); ++k) {
    const dvo_hip_covis_record& r = records[k];
    if (r.in_view != r.unknown + r.occluded + r.seen_through + r.consistent || r.in_view > r.valid || r.valid == 0) {
      std::printf("record %zu breaks the invariant\n", k);
      return 1;
    }
  }
  if (records[2].valid != records[2].consistent || records[2].photo != 0 || records[5].in_view != 0 || records[0].consistent == 0) {
    std::printf("the self pair or the far pair\n");
    return 1;
  }
  if (dvo_slam::CovisibilityConstraintSearch::overlap(records[2], records[2]) != 1.0) { std::printf("overlap of the self pair\n"); return 1; }
  DeviceContext::setErrorHandler(count_refusal);
  std::vector<dvo_slam::CovisibilityConstraintSearch::Record> none;
  const bool refused = !dvo_slam::CovisibilityConstraintSearch::compute(all, std::vector<Pair>(1, Pair(0, N)), LEVEL, 0, none) &&
                       !dvo_slam::CovisibilityConstraintSearch::compute(all, pairs, 7, 0, none);
  DeviceContext::setErrorHandler(0);
  if (!refused || refusals != 2 || !none.empty()) { std::printf("bad pairs or levels were not refused\n"); return 1; }

  std::FILE* f = std::fopen(argv[1], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[1]); return 1; }
  std::fwrite(records.data(), sizeof records[0], records.size(), f);
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
