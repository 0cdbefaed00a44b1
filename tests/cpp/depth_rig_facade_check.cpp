// The C++ facade's depth rig (RgbdImagePyramid::setDepthRig / clearDepthRig; include/dvo_hip.h, dvo_hip_frames_set_depth_rig): update() of
// a pyramid that carries a rig takes its depth matrix as the depth sensor's own image and registers it into the colour camera on the
// device.
//  1. the identity rig (depth_K = K, the identity transform) maps every pixel onto itself: a match on pyramids updated under it returns
//     the same Result, bit for bit, as freshly created pyramids of the same matrices;
//  2. a real rig changes the Result, keeps the frame handles, and level(0).depth is no longer the caller's matrix;
//  3. an invalid rig is refused (the error handler runs, setDepthRig returns false) and changes nothing; a rig and a lens that
//     rectifies depth exclude each other, in either order;
//  4. clearDepthRig: the next update is the rig-less one again.
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

void planes(float shift, dvo::compat::ImageMat& I, dvo::compat::ImageMat& Z) {
  I = dvo::compat::image_create(H, W);
  Z = dvo::compat::image_create(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const float u = float(x) + shift;
      i[y * W + x] = 128.0f + 60.0f * std::sin(u * 0.21f) * std::cos(float(y) * 0.17f) + 30.0f * std::sin((u + float(y)) * 0.05f);
      z[y * W + x] = (x > 250 && y < 30) || (x % 37 == 5 && y % 11 == 3) ? NAN : 1.2f + 2.4f * float(x) / W + 0.4f * float(y) / H;
    }
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

  dvo::compat::Affine3d identity_T, kinect_T;
  kinect_T.matrix()(0, 3) = -0.025;
  kinect_T.matrix()(1, 3) = 0.001;
  kinect_T.matrix()(2, 3) = 0.003;
  const IntrinsicMatrix Kd = IntrinsicMatrix::create(286.0f, 286.0f, 160.25f, 118.75f);

  // 1. the identity rig
  RgbdImagePyramidPtr ref = camera.create(Ia, Za), cur = camera.create(Ib, Zb);
  DenseTracker::Result first, identity, rigged, refused, cleared;
  tracker.match(*ref, *cur, first);
  dvo_hip_frame* ref_handle = ref->device_frame();
  dvo_hip_frame* cur_handle = cur->device_frame();
  if (!ref->setDepthRig(Kc, identity_T) || !cur->setDepthRig(Kc, identity_T) || !ref->hasDepthRig()) { std::printf("the identity rig was refused\n"); return 1; }
  ref->update(Ic, Zc);
  cur->update(Id, Zd);
  tracker.match(*ref, *cur, identity);
  if (!same(fingerprint(fresh), fingerprint(identity), "identity rig")) return 1;

  // 2. a real rig
  if (!ref->setDepthRig(Kd, kinect_T) || !cur->setDepthRig(Kd, kinect_T)) { std::printf("the rig was refused\n"); return 1; }
  ref->update(Ic, Zc);
  cur->update(Id, Zd);
  if (ref->device_frame() != ref_handle || cur->device_frame() != cur_handle) { std::printf("update changed a frame handle\n"); return 1; }
  if (!dvo::compat::image_empty(ref->level(0).depth) && dvo::compat::image_ptr(ref->level(0).depth) == dvo::compat::image_ptr(Zc)) {
    std::printf("level 0 of a rigged pyramid is bound to the depth sensor's matrix\n");
    return 1;
  }
  tracker.match(*ref, *cur, rigged);
  if (fingerprint(rigged) == fingerprint(fresh)) { std::printf("the rig changed nothing\n"); return 1; }

  // 3. an invalid rig: refused, the frame keeps the rig it has; a lens that rectifies depth and a rig exclude each other
  const float K_raw[4] = {258.5f, 259.0f, 160.25f, 118.75f};
  const float fr1[8] = {0.2624f, -0.9531f, -0.0054f, 0.0026f, 1.1633f, 0.0f, 0.0f, 0.0f};
  dvo::compat::Affine3d nan_T;
  nan_T.matrix()(1, 2) = NAN;
  DeviceContext::setErrorHandler(count_error);
  const bool accepted = ref->setDepthRig(IntrinsicMatrix::create(0.0f, 286.0f, 160.0f, 120.0f), kinect_T);
  const bool accepted_nan = ref->setDepthRig(Kd, nan_T);
  const bool accepted_lens = ref->setLens(K_raw, fr1, /*rectify_depth=*/true);
  DeviceContext::setErrorHandler(0);
  if (accepted || accepted_nan || accepted_lens || g_errors != 3) { std::printf("an invalid rig or lens was accepted (%d errors)\n", g_errors); return 1; }
  ref->update(Ic, Zc);
  tracker.match(*ref, *cur, refused);
  if (!same(fingerprint(rigged), fingerprint(refused), "after a refused rig")) return 1;
  {
    RgbdImagePyramidPtr lensed = camera.create(Ia, Za);
    if (!lensed->setLens(K_raw, fr1, /*rectify_depth=*/true)) { std::printf("the lens was refused\n"); return 1; }
    DeviceContext::setErrorHandler(count_error);
    const bool both = lensed->setDepthRig(Kd, kinect_T);
    DeviceContext::setErrorHandler(0);
    if (both || g_errors != 4 || lensed->hasDepthRig()) { std::printf("a rig was accepted beside a lens that rectifies depth\n"); return 1; }
    if (!lensed->setLens(K_raw, fr1, /*rectify_depth=*/false) || !lensed->setDepthRig(Kd, kinect_T)) {
      std::printf("a rig was refused beside a lens that leaves depth alone\n");
      return 1;
    }
    lensed->update(Ic, Zc);
  }

  // 4. cleared
  ref->clearDepthRig();
  cur->clearDepthRig();
  if (ref->hasDepthRig()) { std::printf("clearDepthRig left the rig\n"); return 1; }
  ref->update(Ic, Zc);
  cur->update(Id, Zd);
  if (dvo::compat::image_ptr(ref->level(0).depth) != dvo::compat::image_ptr(Zc)) { std::printf("level 0 is not rebound after clearDepthRig\n"); return 1; }
  tracker.match(*ref, *cur, cleared);
  if (!same(fingerprint(fresh), fingerprint(cleared), "rig cleared")) return 1;
  std::printf("ok\n");
  return 0;
}
