// The C++ facade's point selection with caller-defined predicates (include/dvo/core/point_selection.h) on a synthetic textured scene:
//   1. a subclass of ValidPointAndGradientThresholdPredicate that adds z <= 2.5 gives records bit-identical to the stock predicate on a
//      pyramid with the device depth range [0, 2.5];
//   2. a subclass that adds the level-local region test x < 40 gives records bit-identical to explicit selections handed to the engine
//      (dvo_hip_frame_set_level_selection) computed from dvo_hip_frame_select's masks;
//   3. the stock predicate through match(PointSelection&) gives the records of match(RgbdImagePyramid&);
//   4. getDebugIndex returns the selection of a level (the count select() returned), also after a stock match with debug on;
//   5. a pyramid matched with a custom predicate and then with the stock one gives the stock records of a fresh pyramid.
// Prints "ok" or the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dvo/dense_tracking.h"

using dvo::DenseTracker;
using namespace dvo::core;

namespace {

const int W = 320, H = 240;

struct DepthCap : ValidPointAndGradientThresholdPredicate {
  bool isPointOk(const size_t& x, const size_t& y, const float& z, const float& idx, const float& idy, const float& zdx,
                 const float& zdy) const override {
    return ValidPointAndGradientThresholdPredicate::isPointOk(x, y, z, idx, idy, zdx, zdy) && z <= 2.5f;
  }
};

struct LeftBand : ValidPointAndGradientThresholdPredicate {
  bool isPointOk(const size_t& x, const size_t& y, const float& z, const float& idx, const float& idy, const float& zdx,
                 const float& zdy) const override {
    return ValidPointAndGradientThresholdPredicate::isPointOk(x, y, z, idx, idy, zdx, zdy) && x < 40;
  }
};

RgbdImagePyramidPtr frame(RgbdCameraPyramid& camera, float shift) {
  dvo::compat::ImageMat I = dvo::compat::image_create(H, W), Z = dvo::compat::image_create(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const float u = float(x) + shift;
      i[y * W + x] = 128.0f + 60.0f * std::sin(u * 0.21f) * std::cos(float(y) * 0.17f) + 30.0f * std::sin((u + float(y)) * 0.05f);
      z[y * W + x] = (x > 250 && y < 30) ? NAN : 1.2f + 2.4f * float(x) / W + 0.4f * float(y) / H;
    }
  return camera.create(I, Z);
}

// every field of a record, as bytes
std::vector<double> fingerprint(const DenseTracker::Result& r) {
  std::vector<double> f;
  double T[16];
  dvo::compat::affine_to_rowmajor(r.Transformation, T);
  f.insert(f.end(), T, T + 16);
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) f.push_back(r.Information(a, b));
  f.push_back(r.LogLikelihood);
  for (const auto& L : r.Statistics.Levels) {
    f.push_back(double(L.Id)); f.push_back(double(L.MaxValidPixels)); f.push_back(double(L.ValidPixels));
    f.push_back(double(L.TerminationCriterion)); f.push_back(double(L.Iterations.size()));
    for (const auto& it : L.Iterations) {
      f.push_back(double(it.ValidConstraints));
      f.push_back(it.TDistributionLogLikelihood);
      for (int a = 0; a < 6; ++a) f.push_back(it.EstimateIncrement(a));
    }
  }
  return f;
}

bool same(const std::vector<double>& a, const std::vector<double>& b, const char* what) {
  if (a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0) return true;
  std::printf("%s: records differ (%zu / %zu values)\n", what, a.size(), b.size());
  return false;
}

}  // namespace

int main() {
  RgbdCameraPyramid camera(W, H, IntrinsicMatrix::create(260.0f, 260.0f, 159.5f, 119.5f));
  camera.build(4);
  DenseTracker::Config cfg = DenseTracker::getDefaultConfig();
  cfg.FirstLevel = 3;
  cfg.LastLevel = 0;
  DenseTracker tracker(cfg);

  // 3. the stock predicate, both overloads
  RgbdImagePyramidPtr ref = frame(camera, 0.0f), cur = frame(camera, 1.5f);
  DenseTracker::Result plain, stock;
  tracker.match(*ref, *cur, plain);
  ValidPointAndGradientThresholdPredicate stock_pred;
  PointSelection stock_sel(*ref, stock_pred);
  tracker.match(stock_sel, *cur, stock);
  if (!same(fingerprint(plain), fingerprint(stock), "stock predicate")) return 1;
  if (stock.Statistics.Levels.empty() || plain.Statistics.Levels[0].ValidPixels == 0) { std::printf("empty selection\n"); return 1; }

  // 1. z <= 2.5 on the host against the device range [0, 2.5]
  DenseTracker::Result capped, ranged;
  {
    RgbdImagePyramidPtr r1 = frame(camera, 0.0f);
    DepthCap cap;
    PointSelection sel(*r1, cap);
    tracker.match(sel, *cur, capped);
    RgbdImagePyramidPtr r2 = frame(camera, 0.0f);
    r2->setSelectionDepthRange(0.0f, 2.5f);
    tracker.match(*r2, *cur, ranged);
  }
  if (!same(fingerprint(capped), fingerprint(ranged), "z <= 2.5 against the device range")) return 1;
  if (capped.Statistics.Levels.back().ValidPixels >= plain.Statistics.Levels.back().ValidPixels) { std::printf("range removed nothing\n"); return 1; }

  // 2. x < 40 on the host against explicit sets made from dvo_hip_frame_select's masks
  DenseTracker::Result band, explicit_sets;
  {
    RgbdImagePyramidPtr r1 = frame(camera, 0.0f);
    LeftBand left;
    PointSelection sel(*r1, left);
    sel.debug(true);
    tracker.match(sel, *cur, band);
    // 4. getDebugIndex holds the level's accepted set
    for (int l = cfg.LastLevel; l <= cfg.FirstLevel; ++l) {
      std::vector<uint8_t> dbg;
      if (!sel.getDebugIndex(size_t(l), dbg)) { std::printf("no debug index at level %d\n", l); return 1; }
      size_t n = 0;
      for (uint8_t v : dbg) n += v != 0;
      if (n != sel.select(size_t(l))) { std::printf("debug index of level %d: %zu points\n", l, n); return 1; }
    }
    // 5. the same pyramid matched afterwards with the stock predicate -- through match(pyramid), match(PointSelection) and matchBatch --
    //    gives the records of a fresh pyramid: the custom predicate's accepted sets do not stand in for the thresholds' selection
    DenseTracker::Result after, after_sel, after_batch, again1, again2;
    tracker.match(*r1, *cur, after);
    if (!same(fingerprint(after), fingerprint(plain), "stock match after a custom-predicate match")) return 1;
    tracker.match(sel, *cur, again1);                            // (the custom sets again)
    if (!same(fingerprint(again1), fingerprint(band), "custom predicate again")) return 1;
    PointSelection stock_again(*r1, stock_pred);
    tracker.match(stock_again, *cur, after_sel);
    if (!same(fingerprint(after_sel), fingerprint(plain), "stock PointSelection after a custom-predicate match")) return 1;
    tracker.match(sel, *cur, again2);
    std::vector<RgbdImagePyramid*> rs(1, r1.get()), cs(1, cur.get());
    std::vector<DenseTracker::Result*> os(1, &after_batch);
    tracker.matchBatch(rs, cs, os);
    if (!same(fingerprint(after_batch), fingerprint(plain), "matchBatch after a custom-predicate match")) return 1;
    RgbdImagePyramidPtr r2 = frame(camera, 0.0f);
    r2->build(4);
    for (int l = cfg.LastLevel; l <= cfg.FirstLevel; ++l) {
      const int w = W >> l, h = H >> l;
      std::vector<uint8_t> m(size_t(w) * h);
      int n = 0;
      dvo_hip_frame_select(r2->device_context(), r2->device_frame(), l, 0.0f, 0.0f, &n, m.data());
      for (int y = 0; y < h; ++y)
        for (int x = 40; x < w; ++x) m[size_t(y) * w + x] = 0;
      dvo_hip_frame_set_level_selection(r2->device_context(), r2->device_frame(), l, m.data());
    }
    tracker.match(*r2, *cur, explicit_sets);
  }
  if (!same(fingerprint(band), fingerprint(explicit_sets), "x < 40 against explicit sets")) return 1;

  // 4. with the stock predicate and debug on, a match fills the index of every level it aligns (the device's own masks)
  {
    RgbdImagePyramidPtr r3 = frame(camera, 0.0f);
    PointSelection sel(*r3, stock_pred);
    sel.debug(true);
    DenseTracker::Result dbg_run;
    tracker.match(sel, *cur, dbg_run);
    if (!same(fingerprint(dbg_run), fingerprint(plain), "stock match with debug on")) return 1;
    for (int l = cfg.LastLevel; l <= cfg.FirstLevel; ++l) {
      std::vector<uint8_t> dbg;
      if (!sel.getDebugIndex(size_t(l), dbg)) { std::printf("no debug index after a stock match, level %d\n", l); return 1; }
      size_t k = 0;
      for (uint8_t v : dbg) k += v != 0;
      if (k != dbg_run.Statistics.Levels[size_t(cfg.FirstLevel - l)].ValidPixels) { std::printf("debug index of level %d: %zu\n", l, k); return 1; }
    }
  }
  {
    PointSelection sel(*ref, stock_pred);
    sel.debug(true);
    const size_t n = sel.select(1);
    std::vector<uint8_t> dbg;
    size_t k = 0;
    if (!sel.getDebugIndex(1, dbg)) { std::printf("no debug index (stock)\n"); return 1; }
    for (uint8_t v : dbg) k += v != 0;
    if (k != n || n != plain.Statistics.Levels[2].ValidPixels) { std::printf("stock debug index: %zu / %zu\n", k, n); return 1; }
  }
  std::printf("ok\n");
  return 0;
}
