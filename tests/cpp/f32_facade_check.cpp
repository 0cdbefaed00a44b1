// The C++ facade's float re-ingest (RgbdImagePyramid::update) and device-plane construction (RgbdCameraPyramid::createFromFloatDevice).
//  1. update() before the first build only swaps the matrices; after it, it keeps the device frame's handle and the caller selection,
//     rebinds level(0).intensity / depth, and a DenseTracker::match on the updated pyramids returns the same Result, bit for bit, as a
//     freshly created pyramid pair of the same matrices -- without and with a depth-range selection on the reference;
//  2. createFromFloatDevice: the frame holds the planes it was given and, with host mirrors on, level 0's host matrices are filled.
// Prints "ok" or the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

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

bool same_plane(const float* a, const float* b, size_t n, const char* what) {
  if (std::memcmp(a, b, n * sizeof(float)) == 0) return true;
  std::printf("%s: planes differ\n", what);
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

  dvo::compat::ImageMat Ia, Za, Ib, Zb, Ic, Zc, Id, Zd;
  planes(0.0f, Ia, Za);
  planes(1.5f, Ib, Zb);
  planes(7.0f, Ic, Zc);
  planes(8.0f, Id, Zd);

  // the yardstick: freshly created pyramids of (c, d), without and with a selection on the reference
  DenseTracker::Result fresh, fresh_ranged;
  {
    RgbdImagePyramidPtr r = camera.create(Ic, Zc), c = camera.create(Id, Zd);
    tracker.match(*r, *c, fresh);
    RgbdImagePyramidPtr r2 = camera.create(Ic, Zc);
    r2->setSelectionDepthRange(0.0f, 2.5f);
    tracker.match(*r2, *c, fresh_ranged);
  }
  if (fresh.Statistics.Levels.empty() || fresh.Statistics.Levels[0].ValidPixels == 0) { std::printf("empty selection\n"); return 1; }
  if (fingerprint(fresh) == fingerprint(fresh_ranged)) { std::printf("the depth range selects nothing away\n"); return 1; }

  // 1a. before the first build: update only swaps the matrices
  RgbdImagePyramidPtr ref = camera.create(Ia, Za), cur = camera.create(Ib, Zb);
  ref->update(Ic, Zc);
  DenseTracker::Result swapped;
  {
    RgbdImagePyramidPtr c = camera.create(Id, Zd);
    tracker.match(*ref, *c, swapped);
  }
  if (!same(fingerprint(fresh), fingerprint(swapped), "update before build")) return 1;

  // 1b. pyramids that have matched (a, b) are updated to (c, d): same handles, same Result as the fresh pair
  ref = camera.create(Ia, Za);
  DenseTracker::Result first, updated, updated_ranged, updated_again;
  tracker.match(*ref, *cur, first);
  dvo_hip_frame* ref_handle = ref->device_frame();
  dvo_hip_frame* cur_handle = cur->device_frame();
  ref->update(Ic, Zc);
  cur->update(Id, Zd);
  if (ref->device_frame() != ref_handle || cur->device_frame() != cur_handle) { std::printf("update changed a frame handle\n"); return 1; }
  if (dvo::compat::image_ptr(ref->level(0).intensity) != dvo::compat::image_ptr(Ic) || dvo::compat::image_ptr(ref->level(0).depth) != dvo::compat::image_ptr(Zc)) {
    std::printf("level 0 is not rebound to the new matrices\n");
    return 1;
  }
  tracker.match(*ref, *cur, updated);
  if (!same(fingerprint(fresh), fingerprint(updated), "match after update")) return 1;
  if (fingerprint(first) == fingerprint(updated)) { std::printf("the update changed nothing\n"); return 1; }

  // 1c. the caller selection is kept across update()
  ref->setSelectionDepthRange(0.0f, 2.5f);
  ref->update(Ia, Za);
  ref->update(Ic, Zc);
  tracker.match(*ref, *cur, updated_ranged);
  if (!same(fingerprint(fresh_ranged), fingerprint(updated_ranged), "selection across update")) return 1;
  ref->clearSelection();
  tracker.match(*ref, *cur, updated_again);
  if (!same(fingerprint(fresh), fingerprint(updated_again), "selection cleared after update")) return 1;

  // 1d. host mirrors of the other levels are refreshed
  RgbdImage::hostMirrors(true);
  {
    RgbdImagePyramidPtr p = camera.create(Ia, Za), q = camera.create(Ic, Zc);
    p->build(3);
    q->build(3);
    p->level(1).syncHostMirrors(RgbdImage::MirrorPlanes);
    q->level(1).syncHostMirrors(RgbdImage::MirrorPlanes);
    const size_t n1 = size_t(W / 2) * (H / 2);
    if (std::memcmp(dvo::compat::image_ptr(p->level(1).intensity), dvo::compat::image_ptr(q->level(1).intensity), n1 * sizeof(float)) == 0) {
      std::printf("level 1 of two different frames is the same\n");
      return 1;
    }
    p->update(Ic, Zc);
    if (dvo::compat::image_empty(p->level(1).intensity) ||
        !same_plane(dvo::compat::image_ptr(p->level(1).intensity), dvo::compat::image_ptr(q->level(1).intensity), n1, "level 1 mirror after update") ||
        !same_plane(dvo::compat::image_ptr(p->level(1).depth), dvo::compat::image_ptr(q->level(1).depth), n1, "level 1 depth mirror after update"))
      return 1;
  }

  // 2. device planes: the frame holds them, level 0's host mirrors are filled (mirrors are on)
  {
    const size_t n = size_t(W) * H;
    float* dev = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&dev), n * 2 * sizeof(float)) != hipSuccess) { std::printf("hipMalloc failed\n"); return 1; }
    if (hipMemcpy(dev, dvo::compat::image_ptr(Ic), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dev + n, dvo::compat::image_ptr(Zc), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      std::printf("hipMemcpy failed\n");
      return 1;
    }
    RgbdImagePyramidPtr p = camera.createFromFloatDevice(dev, dev + n);
    p->build(3);
    RgbdImage& l0 = p->level(0);
    if (dvo::compat::image_empty(l0.intensity) || dvo::compat::image_empty(l0.depth) || dvo::compat::image_rows(l0.intensity) != H ||
        dvo::compat::image_cols(l0.intensity) != W) {
      std::printf("createFromFloatDevice: level 0 has no host intensity / depth\n");
      return 1;
    }
    if (!same_plane(dvo::compat::image_ptr(l0.intensity), dvo::compat::image_ptr(Ic), n, "createFromFloatDevice intensity") ||
        !same_plane(dvo::compat::image_ptr(l0.depth), dvo::compat::image_ptr(Zc), n, "createFromFloatDevice depth"))
      return 1;
    DenseTracker::Result from_device;
    RgbdImagePyramidPtr c = camera.create(Id, Zd);
    RgbdImage::hostMirrors(false);
    tracker.match(*p, *c, from_device);
    if (!same(fingerprint(fresh), fingerprint(from_device), "match on a pyramid of device planes")) return 1;
    p.reset();
    (void)hipFree(dev);
  }
  std::printf("ok\n");
  return 0;
}
