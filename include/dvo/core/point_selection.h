// dvo/core/point_selection.h -- PointSelection and its predicates (dvo_core/include/dvo/core/point_selection.h:40-127).
// The compacted point list of the reference (48 B per selected point) never exists here: the predicate is folded
// into the reference-side device plane, so select() returns only the count.
//
// Predicates are dispatched on their EXACT dynamic type (typeid):
//  * ValidPointPredicate and ValidPointAndGradientThresholdPredicate run on the device as thresholds (intensityThreshold() /
//    depthThreshold()), the path every match takes by default.  ValidPointPredicate maps to thresholds of 0, which rejects a pixel whose
//    four gradients are all exactly zero where the reference accepts it (kept: existing behaviour).
//  * any other type -- a subclass of either included -- is evaluated on the HOST with the reference's argument order and level-local
//    coordinates (point_selection.cpp:119-152): select() downloads Z, Idx, Idy, Zdx, Zdy of the level (20 B per pixel, device to host),
//    calls isPointOk once per pixel, and hands the accepted set to the device (1 B per pixel, dvo_hip_frame_set_level_selection), where
//    it serves the matches that pass this PointSelection (a match through a stock predicate, matchBatch or computeIntensityErrorImage drops it
//    first: RgbdImagePyramid::reference_frame).  DenseTracker::match does this for every level of every match: slow (a few milliseconds
//    per 640 x 480 frame, host-bound) but exact.  Restrictions that a mask or a depth range can express run on the device at no such
//    cost: RgbdImagePyramid::setSelectionMask / setSelectionDepthRange.
#pragma once

#include <typeinfo>
#include <vector>

#include "rgbd_image.h"

namespace dvo {
namespace core {

class PointSelectionPredicate {
 public:
  virtual ~PointSelectionPredicate() {}
  virtual bool isPointOk(const size_t& x, const size_t& y, const float& z, const float& idx, const float& idy, const float& zdx,
                         const float& zdy) const = 0;
  virtual float intensityThreshold() const { return 0.0f; }
  virtual float depthThreshold() const { return 0.0f; }
};

class ValidPointPredicate : public PointSelectionPredicate {
 public:
  virtual ~ValidPointPredicate() {}
  virtual bool isPointOk(const size_t& x, const size_t& y, const float& z, const float& idx, const float& idy, const float& zdx,
                         const float& zdy) const {
    (void)x; (void)y; (void)idx; (void)idy;
    return z == z && zdx == zdx && zdy == zdy;
  }
};

class ValidPointAndGradientThresholdPredicate : public PointSelectionPredicate {
 public:
  float intensity_threshold;
  float depth_threshold;
  ValidPointAndGradientThresholdPredicate() : intensity_threshold(0.0f), depth_threshold(0.0f) {}
  virtual ~ValidPointAndGradientThresholdPredicate() {}
  virtual bool isPointOk(const size_t& x, const size_t& y, const float& z, const float& idx, const float& idy, const float& zdx,
                         const float& zdy) const {
    (void)x; (void)y;
    return z == z && zdx == zdx && zdy == zdy &&
           (std::abs(idx) > intensity_threshold || std::abs(idy) > intensity_threshold || std::abs(zdx) > depth_threshold ||
            std::abs(zdy) > depth_threshold);
  }
  virtual float intensityThreshold() const { return intensity_threshold; }
  virtual float depthThreshold() const { return depth_threshold; }
};

class PointSelection {
 public:
  explicit PointSelection(const PointSelectionPredicate& predicate) : pyramid_(0), predicate_(predicate), debug_(false) {}
  PointSelection(RgbdImagePyramid& pyramid, const PointSelectionPredicate& predicate) : pyramid_(&pyramid), predicate_(predicate), debug_(false) {}
  RgbdImagePyramid& getRgbdImagePyramid() {
    assert(pyramid_ != 0);
    return *pyramid_;
  }
  void setRgbdImagePyramid(RgbdImagePyramid& pyramid) { pyramid_ = &pyramid; }   // the device cache is keyed by (frame, level, thresholds)
  void recycle(RgbdImagePyramid& pyramid) { setRgbdImagePyramid(pyramid); }
  size_t getMaximumNumberOfPoints(const size_t& level) {   // point_selection.cpp:68-71
    const RgbdCamera& c = pyramid_->cameraPyramid().level(0);
    double n = double(c.width() * c.height());
    for (size_t l = 0; l < level; ++l) n *= 0.25;
    return size_t(n);
  }
  // point_selection.cpp:56-86: with debug on, select() keeps the selection mask of every level it selects
  bool getDebug() const { return debug_; }
  void debug(bool v) { debug_ = v; }
  // the selection mask (1 = selected) of a level select() ran on with debug on -- DenseTracker::match(PointSelection&, ...) selects every
  // level of the match then; false if there is none
  bool getDebugIndex(const size_t& level, std::vector<uint8_t>& dbg_idx) const {
    if (!debug_ || level >= debug_idx_.size() || debug_idx_[level].empty()) return false;
    dbg_idx = debug_idx_[level];
    return true;
  }
  // The same as an image.  Differs from the reference, whose index is a CV_8UC1 matrix: dvo::compat::ImageMat is a one-channel FLOAT
  // image here (CV_32FC1 with OpenCV), holding 0.0f / 1.0f; the byte mask is the overload above.
  bool getDebugIndex(const size_t& level, dvo::compat::ImageMat& dbg_idx) const {
    std::vector<uint8_t> m;
    if (!getDebugIndex(level, m)) return false;
    const RgbdCamera& c = pyramid_->cameraPyramid().level(level);
    dbg_idx = dvo::compat::image_create(int(c.height()), int(c.width()));
    float* out = dvo::compat::image_ptr_mut(dbg_idx);
    for (size_t i = 0; i < m.size(); ++i) out[i] = m[i] ? 1.0f : 0.0f;
    return true;
  }
  // true: the predicate is one of the two stock classes, which run on the device as thresholds
  bool deviceThresholds() const {
    return typeid(predicate_) == typeid(ValidPointAndGradientThresholdPredicate) || typeid(predicate_) == typeid(ValidPointPredicate);
  }
  // number of selected reference pixels at `level` (point_selection.cpp:89-117)
  size_t select(const size_t& level) {
    assert(pyramid_ != 0);
    pyramid_->compute(level + 1);
    if (!deviceThresholds()) return selectOnHost(level);
    int n = 0;
    uint8_t* mask = 0;
    if (debug_) {
      std::vector<uint8_t>& m = debugSlot(level);
      mask = m.data();
    }
    dvo_hip_check(pyramid_->device_context(), dvo_hip_frame_select(pyramid_->device_context(), pyramid_->device_frame(), int(level),
                  predicate_.intensityThreshold(), predicate_.depthThreshold(), &n, mask), "dvo_hip_frame_select");
    return size_t(n);
  }
  const PointSelectionPredicate& predicate() const { return predicate_; }

 private:
  std::vector<uint8_t>& debugSlot(size_t level) {
    if (debug_idx_.size() <= level) debug_idx_.resize(level + 1);
    const RgbdCamera& c = pyramid_->cameraPyramid().level(level);
    debug_idx_[level].assign(size_t(c.width()) * c.height(), 0);
    return debug_idx_[level];
  }
  // a caller-defined predicate: evaluated here, the accepted set (with the pyramid's caller selection) handed to the device
  size_t selectOnHost(size_t level) {
    dvo_hip_context* ctx = pyramid_->device_context();
    dvo_hip_frame* frame = pyramid_->device_frame();
    const RgbdCamera& c = pyramid_->cameraPyramid().level(level);
    const size_t w = c.width(), h = c.height(), n = w * h;
    std::vector<float> planes(5 * n);
    for (int k = 0; k < 5; ++k)   // depth, intensity_dx, intensity_dy, depth_dx, depth_dy
      if (!dvo_hip_check(ctx, dvo_hip_frame_download_plane(ctx, frame, int(level), k + 1, &planes[k * n]), "dvo_hip_frame_download_plane")) return 0;
    const float *z = &planes[0], *idx = &planes[n], *idy = &planes[2 * n], *zdx = &planes[3 * n], *zdy = &planes[4 * n];
    std::vector<uint8_t> accepted(n, 0);
    size_t count = 0;
    for (size_t y = 0; y < h; ++y)
      for (size_t x = 0; x < w; ++x) {
        const size_t i = y * w + x;
        if (predicate_.isPointOk(x, y, z[i], idx[i], idy[i], zdx[i], zdy[i]) && pyramid_->selectionKeeps(level, x, y, z[i])) {
          accepted[i] = 1;
          ++count;
        }
      }
    dvo_hip_check(ctx, dvo_hip_frame_set_level_selection(ctx, frame, int(level), accepted.data()), "dvo_hip_frame_set_level_selection");
    pyramid_->noteExplicitSelection(level);
    if (debug_) debugSlot(level) = accepted;
    return count;
  }

  RgbdImagePyramid* pyramid_;
  const PointSelectionPredicate& predicate_;
  bool debug_;
  std::vector<std::vector<uint8_t> > debug_idx_;
};

}  // namespace core
}  // namespace dvo
