// dvo_slam/keyframe_covisibility.h -- which keyframes a new keyframe is validated against, by what the two cameras both SEE.
//
// The reference proposes loop closures by distance alone: NearestNeighborConstraintSearch::findPossibleConstraints
// (dvo_slam/src/keyframe_constraint_search.cpp:41-72, called from dvo_slam/src/keyframe_graph.cpp:233 and :456) radius-searches the
// keyframes' translations and hands every hit to the validator.  Two keyframes a metre apart that look at opposite walls then cost two
// multi-level alignments each.  CovisibilityConstraintSearch has the reference's interface (maxDistance, findPossibleConstraints with
// the same signature) and applies the same radius test first; the survivors are then counted against the new keyframe on the device,
// both directions of every survivor in ONE dvo_hip_frames_covisibility call (32 bytes come back per direction), and only those whose
// overlap reaches minOverlap are proposed, the best first.
//
//   overlap(a, b) = min(consistent_ab / valid_a, consistent_ba / valid_b): the share of each keyframe's surface the other one confirms
//   (dvo_slam_amd/csrc/covisibility.h states the counts), 0 where a keyframe has no valid pixel.
//
// With minOverlap == 0 nothing is counted and the result IS the reference's radius set, in the order of `all` (the reference's
// unsorted kd-tree search promises no order).  As in the reference the query keyframe itself is in that set when it is in `all`
// (its distance is 0; keyframe_graph.cpp:238 drops it afterwards as a "self constraint"), and a distance equal to maxDistance is inside.
// Poses are taken as rigid (Affine3d::inverse).  This header deliberately does not declare KeyframeConstraintSearchInterface or
// NearestNeighborConstraintSearch: a drop-in build keeps compiling the reference's own keyframe_constraint_search.{h,cpp} unchanged.
#pragma once

#include <algorithm>
#include <utility>
#include <vector>

#include "dvo/core/rgbd_image.h"
#include "dvo_slam/keyframe.h"

namespace dvo_slam {

class CovisibilityConstraintSearch {
 public:
  typedef dvo_hip_covis_record Record;
  typedef std::pair<int, int> Pair;                              // (a, b): indices into the keyframes of a compute() call

  explicit CovisibilityConstraintSearch(float max_distance, float min_overlap = 0.0f, int level = 2)
      : max_distance_(max_distance), min_overlap_(min_overlap), level_(level), params_(dvo_hip_covis_params_default()) {}
  virtual ~CovisibilityConstraintSearch() {}

  float maxDistance() const { return max_distance_; }
  void maxDistance(const float& d) { max_distance_ = d; }
  float minOverlap() const { return min_overlap_; }
  void minOverlap(const float& v) { min_overlap_ = v; }
  int level() const { return level_; }
  void level(int v) { level_ = v; }
  // depth tolerances and the depth range of the counts (dvo_hip_covis_params)
  const dvo_hip_covis_params& params() const { return params_; }
  void params(const dvo_hip_covis_params& p) { params_ = p; }

  // the reference's radius test: float translations, squared distance <= maxDistance squared; indices into `all`, ascending
  std::vector<int> radiusSet(const KeyframeVector& all, const KeyframePtr& keyframe) const {
    std::vector<int> out;
    double q[16], m[16];
    dvo::compat::affine_to_rowmajor(keyframe->pose(), q);
    for (size_t i = 0; i < all.size(); ++i) {
      dvo::compat::affine_to_rowmajor(all[i]->pose(), m);
      const float dx = float(m[3]) - float(q[3]), dy = float(m[7]) - float(q[7]), dz = float(m[11]) - float(q[11]);
      if ((dx * dx + dy * dy) + dz * dz <= float(double(max_distance_) * double(max_distance_))) out.push_back(int(i));
    }
    return out;
  }

  virtual void findPossibleConstraints(const KeyframeVector& all, const KeyframePtr& keyframe, KeyframeVector& candidates) {
    const std::vector<int> near = radiusSet(all, keyframe);
    if (!(min_overlap_ > 0.0f) || near.empty()) {
      for (size_t i = 0; i < near.size(); ++i) candidates.push_back(all[size_t(near[i])]);
      return;
    }
    // the frames of the call: the survivors, and the query behind them; pairs: query -> survivor, then survivor -> query
    KeyframeVector used;
    for (size_t i = 0; i < near.size(); ++i) used.push_back(all[size_t(near[i])]);
    used.push_back(keyframe);
    const int q = int(used.size()) - 1, m = int(near.size());
    std::vector<Pair> pairs;
    for (int i = 0; i < m; ++i) pairs.push_back(Pair(q, i));
    for (int i = 0; i < m; ++i) pairs.push_back(Pair(i, q));
    std::vector<Record> records;
    if (!compute(used, pairs, level_, &params_, records)) return;
    std::vector<std::pair<double, int> > ranked;                 // (-overlap, index into all): ascending = best first, ties by index
    for (int i = 0; i < m; ++i) {
      const double share = overlap(records[size_t(i)], records[size_t(m + i)]);
      if (share >= double(min_overlap_)) ranked.push_back(std::make_pair(-share, near[size_t(i)]));
    }
    std::sort(ranked.begin(), ranked.end());
    for (size_t i = 0; i < ranked.size(); ++i) candidates.push_back(all[size_t(ranked[i].second)]);
  }

  // min(consistent_ab / valid_a, consistent_ba / valid_b); 0 where either keyframe has no valid pixel
  static double overlap(const Record& ab, const Record& ba) {
    if (ab.valid == 0 || ba.valid == 0) return 0.0;
    return std::min(double(ab.consistent) / double(ab.valid), double(ba.consistent) / double(ba.valid));
  }

  // The raw records of a pair list: records[k] is keyframes[pairs[k].first]'s surface as keyframes[pairs[k].second] sees it at `level`,
  // under T = pose_b^-1 * pose_a.  One device call; false (through the error handler) when the library refuses it.
  static bool compute(const KeyframeVector& keyframes, const std::vector<Pair>& pairs, int level, const dvo_hip_covis_params* params_or_null,
                      std::vector<Record>& records) {
    records.clear();
    if (keyframes.empty() || pairs.empty()) {
      dvo::core::DeviceContext::fail("CovisibilityConstraintSearch::compute", "no keyframes or no pairs");
      return false;
    }
    std::vector<dvo_hip_frame*> frames;
    for (size_t i = 0; i < keyframes.size(); ++i) {
      if (!keyframes[i] || !keyframes[i]->image()) {
        dvo::core::DeviceContext::fail("CovisibilityConstraintSearch::compute", "a keyframe without an image");
        return false;
      }
      frames.push_back(keyframes[i]->image()->device_frame());
    }
    std::vector<int32_t> a(pairs.size()), b(pairs.size());
    std::vector<double> transforms(pairs.size() * 16);
    for (size_t k = 0; k < pairs.size(); ++k) {
      a[k] = pairs[k].first;
      b[k] = pairs[k].second;
      if (a[k] < 0 || b[k] < 0 || size_t(a[k]) >= keyframes.size() || size_t(b[k]) >= keyframes.size()) {
        dvo::core::DeviceContext::fail("CovisibilityConstraintSearch::compute", "a pair names no keyframe");
        return false;
      }
      dvo::compat::affine_to_rowmajor(keyframes[size_t(b[k])]->pose().inverse() * keyframes[size_t(a[k])]->pose(), &transforms[k * 16]);
    }
    records.resize(pairs.size());
    dvo_hip_context* ctx = keyframes[0]->image()->device_context();
    if (!dvo::core::dvo_hip_check(ctx, dvo_hip_frames_covisibility(ctx, int(frames.size()), frames.data(), int(pairs.size()), a.data(), b.data(),
                                                                   transforms.data(), level, params_or_null, records.data(), 0),
                                  "dvo_hip_frames_covisibility")) {
      records.clear();
      return false;
    }
    return true;
  }

 private:
  float max_distance_, min_overlap_;
  int level_;
  dvo_hip_covis_params params_;
};

}  // namespace dvo_slam
