// The C++ facade's loop-closure proposal by appearance (include/dvo_slam/keyframe_appearance.h, dvo_slam::AppearanceConstraintSearch;
// include/dvo_hip.h, dvo_hip_codebook_*): usage: appearance_facade_check <output file>.
//  1. six keyframes of 64 x 48 (the formulas of tests/test_gpu_keyframe_codes.py::facade_frame) enter the book at the first call;
//  2. a keyframe of `all` as the query: its own entry is skipped, with window 1 its neighbours in time too;
//  3. a query keyframe that is not in `all` -- keyframe 2 with a few pixels changed -- finds keyframe 2 first; its records go to the
//     output file (8 bytes each) and to the standard output ("query: id:distance ...") for the test to compare with KeyframeCodebook;
//  4. maxCodeDistance cuts the list; k < 1 is refused through the error handler;
//  5. 300 more keyframes (the same six images again and again) take the book past its first capacity: same ids, same answer, and among
//     equal codes the lowest id comes first;
//  6. a keyframe that has left `all` is proposed no more.
// Prints "ok" last, or the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dvo_slam/keyframe_appearance.h"

using namespace dvo::core;

namespace {

const int W = 64, H = 48, LEVEL = 1, N = 6, K = 3, M = 256;
int refusals = 0;

void count_refusal(const char*, const char*) { ++refusals; }

void frame(int k, bool changed, dvo::compat::ImageMat& I, dvo::compat::ImageMat& Z) {
  I = dvo::compat::image_create(H, W);
  Z = dvo::compat::image_create(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      i[y * W + x] = float((x * (7 + 2 * k) + y * (13 + 4 * k) + k * 37) % 256);
      z[y * W + x] = (x / 2 + 2 * (y / 2) + k) % 29 == 0 ? NAN : float(1000 + (x * (3 + k) + y * 5 + k * 111) % 4096) * 0.001f;
      if (changed && (x / 4 + y / 4) % 5 == 0) i[y * W + x] = 255.0f - i[y * W + x];
    }
}

dvo_slam::KeyframePtr keyframe(RgbdCameraPyramid& camera, int id, int k, bool changed) {
  dvo::compat::ImageMat I, Z;
  frame(k, changed, I, Z);
  RgbdImagePyramidPtr image = camera.create(I, Z);
  image->build(3);
  AffineTransformd pose;
  pose.setIdentity();
  dvo_slam::KeyframePtr out(new dvo_slam::Keyframe());
  out->id(short(id)).image(image).pose(pose);
  return out;
}

void print_matches(const char* label, const std::vector<dvo_hip_code_match>& v) {
  std::printf("%s:", label);
  for (size_t i = 0; i < v.size(); ++i) std::printf(" %u:%u", v[i].id, v[i].distance);
  std::printf("\n");
}

bool has(const dvo_slam::KeyframeVector& v, const dvo_slam::KeyframePtr& k) { return std::find(v.begin(), v.end(), k) != v.end(); }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: appearance_facade_check <file>\n"); return 2; }
  const IntrinsicMatrix Kc = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, Kc);
  camera.build(3);
  dvo_slam::KeyframeVector all;
  for (int k = 0; k < N; ++k) all.push_back(keyframe(camera, k, k, false));

  dvo_slam::AppearanceConstraintSearch search(K, 512, LEVEL, M, 5);
  if (search.k() != K || search.maxCodeDistance() != 512 || search.level() != LEVEL || search.ferns() != M || search.window() != 0 || search.size() != 0) {
    std::printf("the accessors\n");
    return 1;
  }
  // 2. a keyframe of `all`
  dvo_slam::KeyframeVector own;
  search.findPossibleConstraints(all, all[2], own);
  if (search.size() != size_t(N) || own.size() != size_t(K) || has(own, all[2])) { std::printf("the query's own entry was not skipped\n"); return 1; }
  search.window(1);
  own.clear();
  search.findPossibleConstraints(all, all[2], own);
  if (own.size() != size_t(K) || has(own, all[1]) || has(own, all[2]) || has(own, all[3])) { std::printf("the window was not skipped\n"); return 1; }
  search.window(0);

  // 3. a query from outside
  dvo_slam::KeyframePtr query = keyframe(camera, 100, 2, true);
  dvo_slam::KeyframeVector found;
  search.findPossibleConstraints(all, query, found);
  const std::vector<dvo_hip_code_match> first = search.lastMatches();
  if (found.size() != size_t(K) || found[0] != all[2] || first.size() != size_t(K) || first[0].id != 2u || first[0].distance == 0u ||
      first[0].distance + 8u > first[1].distance || search.size() != size_t(N)) {
    print_matches("the query found", first);
    return 1;
  }
  for (int i = 0; i < K; ++i)
    if (found[size_t(i)] != all[first[size_t(i)].id]) { std::printf("candidate %d is not the record's keyframe\n", i); return 1; }
  print_matches("query", first);

  // 4. the cut, and a refusal
  search.maxCodeDistance(int(first[0].distance));
  dvo_slam::KeyframeVector cut;
  search.findPossibleConstraints(all, query, cut);
  if (cut.size() != 1 || cut[0] != all[2]) { std::printf("maxCodeDistance did not cut the list to one\n"); return 1; }
  search.maxCodeDistance(int(first[0].distance) - 1);
  cut.clear();
  search.findPossibleConstraints(all, query, cut);
  if (!cut.empty()) { std::printf("maxCodeDistance below the best distance left candidates\n"); return 1; }
  search.maxCodeDistance(512);
  DeviceContext::setErrorHandler(count_refusal);
  search.k(0);
  search.findPossibleConstraints(all, query, cut);
  search.k(65);
  search.findPossibleConstraints(all, query, cut);
  DeviceContext::setErrorHandler(0);
  search.k(K);
  if (refusals != 2 || !cut.empty()) { std::printf("k = 0 or k = 65 was not refused\n"); return 1; }

  // 5. past the first capacity
  for (int round = 0; round < 2; ++round) {
    const int more = round == 0 ? 250 : 50;
    for (int j = 0; j < more; ++j) all.push_back(keyframe(camera, int(all.size()), int(all.size()) % N, false));
    found.clear();
    search.findPossibleConstraints(all, query, found);
    const std::vector<dvo_hip_code_match>& now = search.lastMatches();
    // keyframes 2, 8, 14 hold the same image: equal codes, the lowest id first
    if (search.size() != all.size() || found.size() != size_t(K) || found[0] != all[2] || now[0].distance != first[0].distance || now[1].id != 8u ||
        now[2].id != 14u || now[1].distance != first[0].distance) {
      print_matches("after growth the query found", now);
      return 1;
    }
  }

  // 6. a keyframe that has left
  const dvo_slam::KeyframePtr left = all[2];
  all.erase(all.begin() + 2);
  found.clear();
  search.findPossibleConstraints(all, query, found);
  if (found.size() != size_t(K) || has(found, left) || search.lastMatches()[0].id != 8u || search.size() != size_t(N + 300)) {
    print_matches("after keyframe 2 left the query found", search.lastMatches());
    return 1;
  }

  std::FILE* f = std::fopen(argv[1], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[1]); return 1; }
  std::fwrite(first.data(), sizeof first[0], first.size(), f);
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
