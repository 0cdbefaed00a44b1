// The C++ facade's depth filter (RgbdImagePyramid::setDepthFilter / clearDepthFilter; include/dvo_hip.h,
// dvo_hip_frames_set_depth_filter): update() of a pyramid that carries a filter conditions its depth matrix on the device first.
//  1. a filter that changes no pixel (radius 0, no edge rejection, no erosion) keeps every bit: a match on pyramids updated under it
//     returns the same Result, bit for bit, as freshly created pyramids of the same matrices;
//  2. the default filter changes the Result, keeps the frame handles, and level(0).depth is no longer the caller's matrix;
//  3. an invalid filter is refused (the error handler runs, setDepthFilter returns false) and changes nothing;
//  4. clearDepthFilter: the next update is the plain one again.
// Prints "ok" or the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dvo/core/rgbd_image.h"
#include "dvo/dense_tracking.h"

using dvo::DenseTracker;
using namespace dvo::core;

namespace {

const int W = 320, H = 240;

// a slanted plane with a foreground box (a depth step on four sides), holes and a ripple of a millimetre
void planes(float shift, dvo::compat::ImageMat& I, dvo::compat::ImageMat& Z) {
  I = dvo::compat::image_create(H, W);
  Z = dvo::compat::image_create(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const float u = float(x) + shift;
      i[y * W + x] = 128.0f + 60.0f * std::sin(u * 0.21f) * std::cos(float(y) * 0.17f) + 30.0f * std::sin((u + float(y)) * 0.05f);
      const bool box = u > 90.0f && u < 170.0f && y > 60 && y < 150;
      const float surface = box ? 1.1f + 0.1f * float(y) / H : 1.9f + 1.4f * float(x) / W + 0.4f * float(y) / H;
      z[y * W + x] = (x > 250 && y < 30) || (x % 37 == 5 && y % 11 == 3) ? NAN : surface + 0.001f * std::sin(u * 1.7f + float(y) * 2.3f);
    }
}

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

int g_errors = 0;
void count_error(const char*, const char*) { ++g_errors; }

int main() {
  const IntrinsicMatrix Kc = IntrinsicMatrix::create(260.0f, 260.0f, 159.5f, 119.5f);
  RgbdCameraPyramid camera(W, H, Kc);
  camera.build(4);
  DenseTracker::Config cfg = DenseTracker::getDefaultConfig();
  cfg.FirstLevel = 3;
  cfg.LastLevel = 0;
  DenseTracker tracker(cfg);

  dvo::compat::ImageMat Ia, Za, Ib, Zb, Ic, Zc, Id, Zd;
  planes(0.0f, Ia, Za);
  planes(1.5f, Ib, Zb);
  planes(7.0f, Ic, Zc);
  planes(8.0f, Id, Zd);

  DenseTracker::Result fresh;
  {
    RgbdImagePyramidPtr r = camera.create(Ic, Zc), c = camera.create(Id, Zd);
    tracker.match(*r, *c, fresh);
  }
  if (fresh.Statistics.Levels.empty() || fresh.Statistics.Levels[0].ValidPixels == 0) { std::printf("empty selection\n"); return 1; }

  // 1. a filter that changes no pixel
  dvo_hip_depth_filter keep = dvo_hip_depth_filter_default();
  keep.radius = 0;
  keep.edge_radius = 0;
  keep.hole_radius = 0;
  RgbdImagePyramidPtr ref = camera.create(Ia, Za), cur = camera.create(Ib, Zb);
  DenseTracker::Result first, kept, filtered, refused, cleared;
  tracker.match(*ref, *cur, first);
  dvo_hip_frame* ref_handle = ref->device_frame();
  dvo_hip_frame* cur_handle = cur->device_frame();
  if (!ref->setDepthFilter(keep) || !cur->setDepthFilter(keep) || !ref->hasDepthFilter()) { std::printf("the filter was refused\n"); return 1; }
  ref->update(Ic, Zc);
  cur->update(Id, Zd);
  tracker.match(*ref, *cur, kept);
  if (!same(fingerprint(fresh), fingerprint(kept), "a filter that keeps every pixel")) return 1;

  // 2. the default filter
  const dvo_hip_depth_filter usual = dvo_hip_depth_filter_default();
  if (!ref->setDepthFilter(usual) || !cur->setDepthFilter(usual)) { std::printf("the default filter was refused\n"); return 1; }
  ref->update(Ic, Zc);
  cur->update(Id, Zd);
  if (ref->device_frame() != ref_handle || cur->device_frame() != cur_handle) { std::printf("update changed a frame handle\n"); return 1; }
  if (!dvo::compat::image_empty(ref->level(0).depth) && dvo::compat::image_ptr(ref->level(0).depth) == dvo::compat::image_ptr(Zc)) {
    std::printf("level 0 of a filtered pyramid is bound to the unfiltered matrix\n");
    return 1;
  }
  tracker.match(*ref, *cur, filtered);
  if (fingerprint(filtered) == fingerprint(fresh)) { std::printf("the filter changed nothing\n"); return 1; }

  // 3. invalid filters: refused, the frame keeps the filter it has
  dvo_hip_depth_filter wide = usual, nan_gate = usual, no_noise = usual;
  wide.radius = 4;
  nan_gate.gate = NAN;
  no_noise.noise_a = no_noise.noise_b = 0.0f;
  DeviceContext::setErrorHandler(count_error);
  const bool a = ref->setDepthFilter(wide), b = ref->setDepthFilter(nan_gate), c = ref->setDepthFilter(no_noise);
  DeviceContext::setErrorHandler(0);
  if (a || b || c || g_errors != 3) { std::printf("an invalid filter was accepted (%d errors)\n", g_errors); return 1; }
  ref->update(Ic, Zc);
  tracker.match(*ref, *cur, refused);
  if (!same(fingerprint(filtered), fingerprint(refused), "after a refused filter")) return 1;

  // 4. cleared
  ref->clearDepthFilter();
  cur->clearDepthFilter();
  if (ref->hasDepthFilter()) { std::printf("clearDepthFilter left the filter\n"); return 1; }
  ref->update(Ic, Zc);
  cur->update(Id, Zd);
  if (dvo::compat::image_ptr(ref->level(0).depth) != dvo::compat::image_ptr(Zc)) { std::printf("level 0 is not rebound after clearDepthFilter\n"); return 1; }
  tracker.match(*ref, *cur, cleared);
  if (!same(fingerprint(fresh), fingerprint(cleared), "filter cleared")) return 1;
  std::printf("ok\n");
  return 0;
}
