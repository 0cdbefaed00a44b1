// dvo_slam/keyframe_appearance.h -- which keyframes a new keyframe is validated against, by what the two images LOOK like.
//
// The reference proposes loop closures by distance alone: NearestNeighborConstraintSearch::findPossibleConstraints
// (dvo_slam/src/keyframe_constraint_search.cpp:41-72) radius-searches the keyframes' translations, and CovisibilityConstraintSearch
// (keyframe_covisibility.h) counts what two keyframes both see UNDER their poses.  Both need poses that can be trusted.  After drift the
// true neighbour of a keyframe lies outside maxDistance of its pose and is never proposed; a lost tracker has no pose at all.
// AppearanceConstraintSearch has the reference's findPossibleConstraints(all, keyframe, candidates) signature and asks no pose: it keeps
// a code book (dvo_hip_codebook; dvo_slam_amd/csrc/keyframe_codes.h: keyframe encoding by randomised ferns, Glocker et al., TVCG 2015) in
// step with `all` -- a keyframe it has not seen is encoded at `level` and added, one it no longer finds in `all` is removed -- and
// proposes the k stored keyframes whose codes are nearest to the query keyframe's, those within maxCodeDistance ferns, the best first.
// The query keyframe itself and its neighbours in time (the keyframes added within `window` entries of it) are skipped: they are
// trivially similar.  The recipe behind it: align against the candidates from the identity, accept by covisibility under the pose found.
//
// This header deliberately does not declare KeyframeConstraintSearchInterface or NearestNeighborConstraintSearch: a drop-in build keeps
// compiling the reference's own keyframe_constraint_search.{h,cpp} unchanged, and a maintainer who wants this search behind the
// reference's interface derives a three-line adapter from both.
#pragma once

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "dvo/core/rgbd_image.h"
#include "dvo_slam/keyframe.h"

namespace dvo_slam {

class AppearanceConstraintSearch {
 public:
  typedef dvo_hip_code_match Match;

  explicit AppearanceConstraintSearch(int k = 4, int max_code_distance = 512, int level = 2, int m = 512, unsigned long long seed = 0)
      : k_(k), max_code_distance_(max_code_distance), level_(level), m_(m), window_(0), seed_(seed), ctx_(0), book_(0), capacity_(0) {}
  virtual ~AppearanceConstraintSearch() { release(); }

  int k() const { return k_; }
  void k(int v) { k_ = v; }
  int maxCodeDistance() const { return max_code_distance_; }
  void maxCodeDistance(int v) { max_code_distance_ = v; }
  int window() const { return window_; }
  void window(int v) { window_ = v; }
  int level() const { return level_; }
  int ferns() const { return m_; }
  // entries of the book so far (ids given), and the keyframe behind an id (null once removed)
  size_t size() const { return entries_.size(); }
  // the last query's records, padding included: what findPossibleConstraints chose from
  const std::vector<Match>& lastMatches() const { return last_; }

  virtual void findPossibleConstraints(const KeyframeVector& all, const KeyframePtr& keyframe, KeyframeVector& candidates) {
    last_.clear();
    if (!keyframe || !keyframe->image() || k_ < 1) {
      dvo::core::DeviceContext::fail("AppearanceConstraintSearch::findPossibleConstraints", "no keyframe image, or k < 1");
      return;
    }
    if (!sync(all, keyframe->image()->device_context())) return;
    if (entries_.empty()) return;
    dvo_hip_frame* frame[1] = {keyframe->image()->device_frame()};
    // the query's own entry and its neighbours in time
    uint32_t from = 0, to = 0;
    const std::map<const Keyframe*, uint32_t>::const_iterator own = ids_.find(keyframe.get());
    if (own != ids_.end()) {
      from = own->second > uint32_t(window_) ? own->second - uint32_t(window_) : 0u;
      to = own->second + uint32_t(window_) + 1u;
    }
    last_.resize(size_t(k_));
    if (!dvo::core::dvo_hip_check(ctx_, dvo_hip_codebook_query_frames(ctx_, book_, 1, frame, level_, k_, &from, &to, last_.data(), 0, 0),
                                  "dvo_hip_codebook_query_frames")) {
      last_.clear();
      return;
    }
    for (size_t i = 0; i < last_.size(); ++i)
      if (last_[i].id != 0xFFFFFFFFu && last_[i].distance <= uint32_t(max_code_distance_ < 0 ? 0 : max_code_distance_))
        candidates.push_back(entries_[last_[i].id]);
  }

 private:
  AppearanceConstraintSearch(const AppearanceConstraintSearch&);
  AppearanceConstraintSearch& operator=(const AppearanceConstraintSearch&);

  void release() {
    if (book_) dvo_hip_codebook_destroy(ctx_, book_);
    book_ = 0;
  }

  // room for n more entries: a book of twice the capacity takes the codes over (read_codes + add_codes) and the dead stay dead
  bool reserve(size_t n) {
    if (book_ && entries_.size() + n <= capacity_) return true;
    size_t capacity = capacity_ ? capacity_ : 256;
    while (capacity < entries_.size() + n) capacity *= 2;
    dvo_hip_codebook* grown = 0;
    if (!dvo::core::dvo_hip_check(ctx_, dvo_hip_codebook_create(ctx_, m_, int(capacity), seed_, 0, 0.5f, 5.0f, &grown), "dvo_hip_codebook_create"))
      return false;
    if (book_ && !entries_.empty()) {
      std::vector<uint32_t> codes(entries_.size() * size_t(m_ / 8)), dead;
      for (size_t i = 0; i < entries_.size(); ++i)
        if (!entries_[i]) dead.push_back(uint32_t(i));
      bool ok = dvo::core::dvo_hip_check(ctx_, dvo_hip_codebook_read_codes(ctx_, book_, 0, int(entries_.size()), codes.data(), 0), "dvo_hip_codebook_read_codes") &&
                dvo::core::dvo_hip_check(ctx_, dvo_hip_codebook_add_codes(ctx_, grown, int(entries_.size()), codes.data(), 0, 0), "dvo_hip_codebook_add_codes");
      if (ok && !dead.empty()) ok = dvo::core::dvo_hip_check(ctx_, dvo_hip_codebook_remove(ctx_, grown, int(dead.size()), dead.data()), "dvo_hip_codebook_remove");
      if (!ok) {
        dvo_hip_codebook_destroy(ctx_, grown);
        return false;
      }
    }
    release();
    book_ = grown;
    capacity_ = capacity;
    return true;
  }

  // the book in step with `all`: what is new is encoded and added in ONE call, what has left is removed
  bool sync(const KeyframeVector& all, dvo_hip_context* ctx) {
    if (!ctx_) ctx_ = ctx;
    KeyframeVector fresh;
    std::vector<dvo_hip_frame*> frames;
    std::map<const Keyframe*, uint32_t> present;
    for (size_t i = 0; i < all.size(); ++i) {
      if (!all[i] || !all[i]->image()) {
        dvo::core::DeviceContext::fail("AppearanceConstraintSearch::findPossibleConstraints", "a keyframe without an image");
        return false;
      }
      const std::map<const Keyframe*, uint32_t>::const_iterator at = ids_.find(all[i].get());
      if (at != ids_.end()) {
        present.insert(*at);
      } else if (present.find(all[i].get()) == present.end()) {
        present[all[i].get()] = uint32_t(entries_.size() + fresh.size());
        fresh.push_back(all[i]);
        frames.push_back(all[i]->image()->device_frame());
      }
    }
    std::vector<uint32_t> gone;
    for (std::map<const Keyframe*, uint32_t>::const_iterator it = ids_.begin(); it != ids_.end(); ++it)
      if (present.find(it->first) == present.end()) gone.push_back(it->second);
    if (!fresh.empty()) {
      if (!reserve(fresh.size())) return false;
      if (!dvo::core::dvo_hip_check(ctx_, dvo_hip_codebook_add_frames(ctx_, book_, int(frames.size()), frames.data(), level_, 0),
                                    "dvo_hip_codebook_add_frames"))
        return false;
      entries_.insert(entries_.end(), fresh.begin(), fresh.end());
    }
    if (!gone.empty()) {
      if (!dvo::core::dvo_hip_check(ctx_, dvo_hip_codebook_remove(ctx_, book_, int(gone.size()), gone.data()), "dvo_hip_codebook_remove")) return false;
      for (size_t i = 0; i < gone.size(); ++i) entries_[gone[i]].reset();
    }
    ids_.swap(present);
    return true;
  }

  int k_, max_code_distance_, level_, m_, window_;
  unsigned long long seed_;
  dvo_hip_context* ctx_;
  dvo_hip_codebook* book_;
  size_t capacity_;
  KeyframeVector entries_;                                        // by id; null: removed
  std::map<const Keyframe*, uint32_t> ids_;
  std::vector<Match> last_;
};

}  // namespace dvo_slam
