// dvo/visualization/point_cloud_aggregator.h -- the downsampled map of the registered keyframes, fused on the device.
// Stands in for dvo::visualization::PointCloudAggregator (dvo_core/include/dvo/visualization/point_cloud_aggregator.h:36-52,
// dvo_core/src/visualization/point_cloud_aggregator.cpp:49-109).  The reference registers cloud builders by name and, on build(),
// concatenates every step-th cloud (step = max(size / 50, 1), in name order) and filters the sum with a 1 cm voxel grid.  Here a
// keyframe is registered as its device pyramid and its pose; build() clears a device map (include/dvo_hip.h, dvo_hip_map_*), inserts
// the same subset in ONE launch and returns one point per voxel, sorted by voxel key.  An empty aggregator returns one default point,
// as the reference does.  The voxel's point is the exact centroid quantised to leaf / 1024 -- NOT PCL's ApproximateVoxelGrid, whose
// output depends on the order of insertion.
// Not in the reference: setIncremental(true) keeps the device map between builds and makes it FOLLOW the registered keyframes instead of
// rebuilding it: build() then issues at most one dvo_hip_map_remove (keyframes that left, or whose pyramid was replaced), one
// dvo_hip_map_move (keyframes whose pose changed: a pose-graph optimisation) and one dvo_hip_map_insert (new ones) for the difference to
// what the map holds, and rehashes the table at its capacity when the vacated slots outnumber the live voxels.  All sums are integers,
// so the cloud is the one the rebuild gives, bit for bit.  It falls back to the rebuild while the every-step-th subsampling is active
// (step > 1: from 100 keyframes on), when a call reports a lack of capacity or unmatched points, and when the context changed.  A
// registered pyramid must keep its content while it is in the map (update() it only after remove(), or add() it again afterwards).
// Also not in the reference: render() and renderInto() give the map built last as a model view -- an RgbdImagePyramid seen from a pose
// (include/dvo_hip.h, dvo_hip_map_render / dvo_hip_map_render_frames) -- that a DenseTracker can align a new frame against.
// setColour(true) makes the map a COLOURED one, as the reference's is (it voxel-filters PointXYZRGB clouds): build() attaches level(0).rgb
// of every registered pyramid that hasRgb() and does not carry colour yet (RgbdImagePyramid::setColourFromRgb), creates the device map
// with DVO_HIP_MAP_COLOUR and fills the cloud's rgba (0xFFRRGGBB per voxel, include/dvo_hip.h, dvo_hip_map_extract_colour).  If some
// registered pyramid has neither colour nor rgb, the build falls back to the grey map and says so (DeviceContext::warn); rgba stays empty.
// setNormals(true) makes the map one WITH NORMALS (include/dvo_hip.h, DVO_HIP_MAP_NORMALS; combines with setColour): the device map fuses
// the surface normal of every point that has one, the cloud gains normal_x / normal_y / normal_z and the agreement of the fused normals
// per voxel (dvo_hip_map_extract_normals), and renderNormals() gives the map as a view of normals.  In the sub-map calls below such
// a map merges with its like, and its records have a third array (VoxelNormalRecord; dvo_hip_map_export_ex, dvo_hip_map_merge_records_ex).
// merge() / subtract() / moveSubmaps() / exportRecords() / absorbRecords() work on the device maps themselves (include/dvo_hip.h,
// dvo_hip_map_merge ...): an aggregator built in the coordinates of an anchor keyframe is a SUB-MAP that enters another aggregator's map
// under the anchor's pose and follows a pose-graph optimisation without its keyframes' pyramids (see "sub-maps" below).
#pragma once

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "dvo/visualization/async_point_cloud_builder.h"

namespace dvo {
namespace visualization {

class PointCloudAggregator {
 public:
  typedef AsyncPointCloudBuilder::PointCloud PointCloud;

  // capacity_slots: the device table (32 bytes per slot); keep it at least four times the voxels of the map
  explicit PointCloudAggregator(size_t capacity_slots = size_t(1) << 22) : capacity_(capacity_slots), ctx_(0), map_(0), incremental_(false), colour_(false), map_coloured_(false), normals_(false), map_normals_(false) {}
  ~PointCloudAggregator() {
    if (map_) dvo_hip_map_destroy(ctx_, map_);
  }

  void add(const std::string& name, const dvo::core::RgbdImagePyramidPtr& pyramid, const dvo::compat::Affine3d& pose) {
    Entry e;
    e.pyramid = pyramid;
    e.pose = pose;
    clouds_[name] = e;
  }
  void remove(const std::string& name) { clouds_.erase(name); }
  size_t size() const { return clouds_.size(); }
  // off (the default): every build() clears the map and inserts every keyframe.  on: build() updates the map by the difference
  void setIncremental(bool on) {
    incremental_ = on;
    if (!on) held_.clear();
  }
  bool incremental() const { return incremental_; }
  // off (the default): a grey map.  on: build() fuses the pyramids' colour (see above)
  void setColour(bool on) { colour_ = on; }
  bool colour() const { return colour_; }
  // off (the default): no normals.  on: build() fuses the points' surface normals (see above)
  void setNormals(bool on) { normals_ = on; }
  bool normals() const { return normals_; }

  PointCloud::Ptr build() {
    PointCloud::Ptr cloud(new PointCloud);
    if (clouds_.empty()) {
      cloud->push_back_default();
      return cloud;
    }
    const bool coloured = colour_ && attachColour();
    if (map_ && (coloured != map_coloured_ || normals_ != map_normals_)) {   // (a map is of one kind for life: another kind is made anew)
      dvo_hip_map_destroy(ctx_, map_);
      map_ = 0;
      held_.clear();
    }
    if (incremental_ && clouds_.size() / size_t(50) <= size_t(1)) {
      dvo_hip_context* now = clouds_.begin()->second.pyramid->device_context();
      if (map_ && now == ctx_ && !held_.empty() && update()) return extract(cloud);
    }
    held_.clear();
    std::vector<dvo_hip_frame*> frames;
    std::vector<double> poses;
    const size_t step = std::max(clouds_.size() / size_t(50), size_t(1));
    size_t k = 0;
    for (std::map<std::string, Entry>::iterator it = clouds_.begin(); it != clouds_.end(); ++it, ++k) {
      if ((k % step) != 0) continue;
      frames.push_back(it->second.pyramid->device_frame());
      double T[16];
      dvo::compat::affine_to_rowmajor(it->second.pose, T);
      poses.insert(poses.end(), T, T + 16);
    }
    dvo_hip_context* ctx = clouds_.begin()->second.pyramid->device_context();
    if (map_ && ctx != ctx_) {
      dvo_hip_map_destroy(ctx_, map_);
      map_ = 0;
    }
    ctx_ = ctx;
    using dvo::core::dvo_hip_check;
    if (!map_) {
      const unsigned flags = (coloured ? DVO_HIP_MAP_COLOUR : 0u) | (normals_ ? DVO_HIP_MAP_NORMALS : 0u);
      if (!dvo_hip_check(ctx_, dvo_hip_map_create_ex(ctx_, 0.01f, capacity_, flags, &map_), "dvo_hip_map_create_ex")) return cloud;
      map_coloured_ = coloured;
      map_normals_ = normals_;
    }
    if (!dvo_hip_check(ctx_, dvo_hip_map_clear(ctx_, map_), "dvo_hip_map_clear")) return cloud;
    if (!dvo_hip_check(ctx_, dvo_hip_map_insert(ctx_, map_, int(frames.size()), frames.data(), poses.data(), 0, 0.0f, INFINITY), "dvo_hip_map_insert"))
      return cloud;
    if (incremental_ && step == 1) held_ = clouds_;
    return extract(cloud);
  }

  // A view of the map build() made last, as a pyramid of `camera` seen from `pose` (camera -> world): intensity 0 and depth NaN where
  // the map shows nothing.  The planes come to the host once, as the pyramid's own matrices.  Null before the first build().
  dvo::core::RgbdImagePyramidPtr render(dvo::core::RgbdCameraPyramid& camera, const dvo::compat::Affine3d& pose,
                                        const dvo_hip_render_params& params = dvo_hip_render_params_default()) {
    if (!map_) return dvo::core::RgbdImagePyramidPtr();
    const dvo::core::RgbdCamera& c0 = camera.level(0);
    const int w = int(c0.width()), h = int(c0.height());
    const float K[4] = {c0.intrinsics().fx(), c0.intrinsics().fy(), c0.intrinsics().ox(), c0.intrinsics().oy()};
    double T[16];
    dvo::compat::affine_to_rowmajor(pose, T);
    dvo::compat::ImageMat I = dvo::compat::image_create(h, w), Z = dvo::compat::image_create(h, w);
    float* i[1] = {dvo::compat::image_ptr_mut(I)};
    float* z[1] = {dvo::compat::image_ptr_mut(Z)};
    if (!dvo::core::dvo_hip_check(ctx_, dvo_hip_map_render(ctx_, map_, 1, w, h, K, T, &params, i, z, 0), "dvo_hip_map_render"))
      return dvo::core::RgbdImagePyramidPtr();
    dvo::core::DeviceContext::Scope scope(ctx_);   // (the pyramid belongs to the map's context)
    return camera.create(I, Z);
  }
  // The streaming form: the view goes straight into `pyramid`'s existing device frame (its own size and intrinsics), without leaving
  // the device; the pyramid then behaves as after RgbdImagePyramid::update() with the rendered planes.
  bool renderInto(dvo::core::RgbdImagePyramid& pyramid, const dvo::compat::Affine3d& pose,
                  const dvo_hip_render_params& params = dvo_hip_render_params_default()) {
    if (!map_ || pyramid.device_context() != ctx_) return false;
    double T[16];
    dvo::compat::affine_to_rowmajor(pose, T);
    dvo_hip_frame* one[1] = {pyramid.device_frame()};
    if (!dvo::core::dvo_hip_check(ctx_, dvo_hip_map_render_frames(ctx_, map_, 1, one, T, &params, -1, 0, 0u), "dvo_hip_map_render_frames")) return false;
    pyramid.deviceFrameChanged();
    return true;
  }

  // A view of the normals of the map build() made last (setNormals(true)) from `pose` (camera -> world) through level 0 of `camera`:
  // normals = width * height records {n.x, n.y, n.z, has} in the VIEW'S CAMERA coordinates (zeros where nothing was seen or the voxel has
  // no normal), depth = the view's depth plane, bit for bit render()'s (NaN where nothing was seen).  false before the first build(), for
  // a map without normals, and on an error.
  bool renderNormals(dvo::core::RgbdCameraPyramid& camera, const dvo::compat::Affine3d& pose, std::vector<float>& normals, std::vector<float>& depth,
                     const dvo_hip_render_params& params = dvo_hip_render_params_default()) {
    if (!map_ || !map_normals_) return false;
    const dvo::core::RgbdCamera& c0 = camera.level(0);
    const int w = int(c0.width()), h = int(c0.height());
    const float K[4] = {c0.intrinsics().fx(), c0.intrinsics().fy(), c0.intrinsics().ox(), c0.intrinsics().oy()};
    double T[16];
    dvo::compat::affine_to_rowmajor(pose, T);
    normals.assign(size_t(w) * size_t(h) * 4, 0.0f);
    depth.assign(size_t(w) * size_t(h), 0.0f);
    float* n[1] = {normals.data()};
    float* z[1] = {depth.data()};
    return dvo::core::dvo_hip_check(ctx_, dvo_hip_map_render_normals(ctx_, map_, 1, w, h, K, T, &params, n, z, 0), "dvo_hip_map_render_normals");
  }

  // ---- sub-maps (include/dvo_hip.h, dvo_hip_map_merge / _move_submaps / _export / _merge_records) ----
  // An aggregator whose keyframes were added under poses RELATIVE to an anchor keyframe (T_anchor^-1 * T_i) and built is a sub-map; the
  // calls below put the device maps of such aggregators into this one's, take them out again and re-pose them, from the voxel tables
  // alone.  They work on the map build() made last (an aggregator without keyframes gets an empty map of the first source's context and
  // kind) and last until the next build() that rebuilds; cloud() returns the map as it stands.  All return false on a refusal or an error
  // (dvo_hip_last_error says which) and, unlike build(), do not go through DeviceContext::fail: a refusal is an answer, not a fault.
  struct VoxelRecord {       // 32 bytes: a slot of the device table
    uint64_t key;
    uint32_t n, sx, sy, sz, si, pad;
  };
  struct VoxelColourRecord {  // 16 bytes: the slot's colour sums (a coloured map)
    uint32_t sr, sg, sb, pad;
  };

  struct VoxelNormalRecord {  // 16 bytes: the slot's normal sums (a map with normals)
    uint32_t snx, sny, snz, nn;
  };

  // plain: the sum is, bit for bit, the map built from the keyframes of both
  bool merge(const PointCloudAggregator& other) { return mergeOne(other, 1, 0); }
  bool subtract(const PointCloudAggregator& other) { return mergeOne(other, -1, 0); }
  // posed: `pose` takes the sub-map's coordinates to this map's (the anchor keyframe's pose)
  bool merge(const PointCloudAggregator& other, const dvo::compat::Affine3d& pose) { return mergeOne(other, 1, &pose); }
  bool subtract(const PointCloudAggregator& other, const dvo::compat::Affine3d& pose) { return mergeOne(other, -1, &pose); }
  // after a pose-graph optimisation: every sub-map from its old anchor pose to its new one, in one launch
  bool moveSubmaps(const std::vector<const PointCloudAggregator*>& submaps, const std::vector<dvo::compat::Affine3d>& poses_old,
                   const std::vector<dvo::compat::Affine3d>& poses_new) {
    if (!map_ || submaps.size() != poses_old.size() || submaps.size() != poses_new.size()) return false;
    std::vector<dvo_hip_map*> maps;
    std::vector<double> from(16 * submaps.size()), to(16 * submaps.size());
    for (size_t i = 0; i < submaps.size(); ++i) {
      if (!submaps[i] || !submaps[i]->map_) return false;
      maps.push_back(submaps[i]->map_);
      dvo::compat::affine_to_rowmajor(poses_old[i], &from[16 * i]);
      dvo::compat::affine_to_rowmajor(poses_new[i], &to[16 * i]);
    }
    return dvo_hip_map_move_submaps(ctx_, map_, int(maps.size()), maps.data(), from.data(), to.data()) == DVO_HIP_OK;
  }
  // the live voxels as raw records (colour: filled for a coloured map, else emptied), in no particular order; *leaf = the map's leaf
  bool exportRecords(std::vector<VoxelRecord>& records, std::vector<VoxelColourRecord>& colour, float* leaf = 0) const {
    if (!map_) return false;
    size_t n = 0, got = 0;
    if (dvo_hip_map_export(ctx_, map_, 0, 0, 0, 0, &n) != DVO_HIP_OK) return false;
    if (leaf && dvo_hip_map_info(ctx_, map_, leaf, 0, 0) != DVO_HIP_OK) return false;
    records.resize(n);
    colour.resize(map_coloured_ ? n : size_t(0));
    if (n == 0) return true;
    return dvo_hip_map_export(ctx_, map_, n, records.data(), map_coloured_ ? colour.data() : 0, 0, &got) == DVO_HIP_OK && got == n;
  }
  // records (of another context, another process, a file) into or out of the map; pose null: plain, leaf must be the map's
  bool absorbRecords(const std::vector<VoxelRecord>& records, const std::vector<VoxelColourRecord>& colour, float leaf = 0.01f, int sign = 1,
                     const dvo::compat::Affine3d* pose = 0) {
    if (!map_ || (map_coloured_ && colour.size() != records.size()) || (!map_coloured_ && !colour.empty())) return false;
    double T[16];
    if (pose) dvo::compat::affine_to_rowmajor(*pose, T);
    return dvo_hip_map_merge_records(ctx_, map_, records.size(), records.data(), map_coloured_ ? colour.data() : 0, 0, leaf, sign, pose ? T : 0) == DVO_HIP_OK;
  }
  // ... with the normal records of a map with normals (filled for such a map, else emptied) ...
  bool exportRecords(std::vector<VoxelRecord>& records, std::vector<VoxelColourRecord>& colour, std::vector<VoxelNormalRecord>& normals, float* leaf = 0) const {
    if (!map_) return false;
    size_t n = 0, got = 0;
    if (dvo_hip_map_export_ex(ctx_, map_, 0, 0, 0, 0, 0, &n) != DVO_HIP_OK) return false;
    if (leaf && dvo_hip_map_info(ctx_, map_, leaf, 0, 0) != DVO_HIP_OK) return false;
    records.resize(n);
    colour.resize(map_coloured_ ? n : size_t(0));
    normals.resize(map_normals_ ? n : size_t(0));
    if (n == 0) return true;
    return dvo_hip_map_export_ex(ctx_, map_, n, records.data(), map_coloured_ ? colour.data() : 0, map_normals_ ? normals.data() : 0, 0, &got) == DVO_HIP_OK &&
           got == n;
  }
  // ... and back: a map with normals takes records WITH normal records, one without takes none
  bool absorbRecords(const std::vector<VoxelRecord>& records, const std::vector<VoxelColourRecord>& colour, const std::vector<VoxelNormalRecord>& normals,
                     float leaf = 0.01f, int sign = 1, const dvo::compat::Affine3d* pose = 0) {
    if (!map_ || (map_coloured_ && colour.size() != records.size()) || (!map_coloured_ && !colour.empty())) return false;
    if ((map_normals_ && normals.size() != records.size()) || (!map_normals_ && !normals.empty())) return false;
    double T[16];
    if (pose) dvo::compat::affine_to_rowmajor(*pose, T);
    return dvo_hip_map_merge_records_ex(ctx_, map_, records.size(), records.data(), map_coloured_ ? colour.data() : 0, map_normals_ ? normals.data() : 0, 0,
                                        leaf, sign, pose ? T : 0) == DVO_HIP_OK;
  }
  // the map as it stands -- after merges -- one point per voxel, sorted by voxel key (build() without rebuilding)
  PointCloud::Ptr cloud() {
    PointCloud::Ptr out(new PointCloud);
    if (!map_) {
      out->push_back_default();
      return out;
    }
    return extract(out);
  }

 private:
  struct Entry {
    dvo::core::RgbdImagePyramidPtr pyramid;
    dvo::compat::Affine3d pose;
  };
  static_assert(sizeof(VoxelRecord) == 32 && sizeof(VoxelColourRecord) == 16 && sizeof(VoxelNormalRecord) == 16,
                "the records of include/dvo_hip.h, dvo_hip_map_export_ex");

  bool mergeOne(const PointCloudAggregator& other, int sign, const dvo::compat::Affine3d* pose) {
    if (!other.map_) return false;
    using dvo::core::dvo_hip_check;
    if (!map_) {                               // an aggregator that only collects sub-maps: an empty map like the first one
      ctx_ = other.ctx_;
      const unsigned flags = (other.map_coloured_ ? DVO_HIP_MAP_COLOUR : 0u) | (other.map_normals_ ? DVO_HIP_MAP_NORMALS : 0u);
      if (!dvo_hip_check(ctx_, dvo_hip_map_create_ex(ctx_, 0.01f, capacity_, flags, &map_), "dvo_hip_map_create_ex")) return false;
      map_coloured_ = other.map_coloured_;
      map_normals_ = other.map_normals_;
    }
    double T[16];
    if (pose) dvo::compat::affine_to_rowmajor(*pose, T);
    dvo_hip_map* src[1] = {other.map_};
    const int signs[1] = {sign};
    return dvo_hip_map_merge(ctx_, map_, 1, src, signs, pose ? T : 0) == DVO_HIP_OK;
  }
  PointCloudAggregator(const PointCloudAggregator&);
  PointCloudAggregator& operator=(const PointCloudAggregator&);

  // every registered pyramid carries colour, attached now from level(0).rgb where it did not; false (and a warning): one has neither
  bool attachColour() {
    for (std::map<std::string, Entry>::iterator it = clouds_.begin(); it != clouds_.end(); ++it) {
      dvo::core::RgbdImagePyramid& p = *it->second.pyramid;
      if (p.hasColour()) continue;
      if (!p.level(0).hasRgb() || !p.setColourFromRgb()) {
        dvo::core::DeviceContext::warn("PointCloudAggregator::build", ("keyframe " + it->first + " has no rgb: the map is built grey").c_str());
        return false;
      }
    }
    return true;
  }

  // the map's live voxels into `cloud`, sorted by key
  PointCloud::Ptr extract(PointCloud::Ptr cloud) {
    using dvo::core::dvo_hip_check;
    struct dvo_hip_map_stats stats;
    if (!dvo_hip_check(ctx_, dvo_hip_map_stats(ctx_, map_, &stats), "dvo_hip_map_stats")) return cloud;
    const size_t n = size_t(stats.occupied - stats.vacant);
    std::vector<float> xyzi(4 * std::max(n, size_t(1)));
    std::vector<uint64_t> keys(std::max(n, size_t(1)));
    std::vector<uint32_t> rgba(map_coloured_ ? std::max(n, size_t(1)) : size_t(0));
    std::vector<float> normals(map_normals_ ? 4 * std::max(n, size_t(1)) : size_t(0));
    size_t got = 0;
    if (map_normals_) {
      if (!dvo_hip_check(ctx_, dvo_hip_map_extract_normals(ctx_, map_, n, xyzi.data(), normals.data(), map_coloured_ ? rgba.data() : 0, 0, keys.data(), 0, &got),
                         "dvo_hip_map_extract_normals"))
        return cloud;
    } else if (map_coloured_) {
      if (!dvo_hip_check(ctx_, dvo_hip_map_extract_colour(ctx_, map_, n, xyzi.data(), rgba.data(), 0, keys.data(), 0, &got), "dvo_hip_map_extract_colour"))
        return cloud;
    } else if (!dvo_hip_check(ctx_, dvo_hip_map_extract(ctx_, map_, n, xyzi.data(), 0, keys.data(), 0, &got), "dvo_hip_map_extract")) {
      return cloud;
    }
    std::vector<size_t> order(got);
    std::iota(order.begin(), order.end(), size_t(0));
    std::sort(order.begin(), order.end(), [&keys](size_t a, size_t b) { return keys[a] < keys[b]; });
    cloud->resize(got);
    cloud->rgba.resize(map_coloured_ ? got : size_t(0));
    for (std::vector<float>* v : {&cloud->normal_x, &cloud->normal_y, &cloud->normal_z, &cloud->agreement}) v->resize(map_normals_ ? got : size_t(0));
    cloud->width = got;
    cloud->height = 1;
    for (size_t i = 0; i < got; ++i) {
      const float* p = &xyzi[4 * order[i]];
      cloud->x[i] = p[0];
      cloud->y[i] = p[1];
      cloud->z[i] = p[2];
      cloud->intensity[i] = p[3];
      if (map_coloured_) cloud->rgba[i] = rgba[order[i]];
      if (map_normals_) {
        const float* m = &normals[4 * order[i]];
        cloud->normal_x[i] = m[0];
        cloud->normal_y[i] = m[1];
        cloud->normal_z[i] = m[2];
        cloud->agreement[i] = m[3];
      }
    }
    return cloud;
  }

  // The difference between what the map holds (held_) and what is registered (clouds_, all of it: no subsampling), as at most one
  // remove, one move and one insert; false: the map is in doubt and is to be rebuilt.
  bool update() {
    std::vector<dvo_hip_frame*> gone, moved, fresh;
    std::vector<double> gone_poses, moved_from, moved_to, fresh_poses;
    double T[16], U[16];
    for (std::map<std::string, Entry>::iterator it = held_.begin(); it != held_.end(); ++it) {
      std::map<std::string, Entry>::iterator now = clouds_.find(it->first);
      dvo::compat::affine_to_rowmajor(it->second.pose, T);
      if (now == clouds_.end() || now->second.pyramid != it->second.pyramid) {
        gone.push_back(it->second.pyramid->device_frame());
        gone_poses.insert(gone_poses.end(), T, T + 16);
        continue;
      }
      dvo::compat::affine_to_rowmajor(now->second.pose, U);
      if (std::equal(T, T + 16, U)) continue;
      moved.push_back(it->second.pyramid->device_frame());
      moved_from.insert(moved_from.end(), T, T + 16);
      moved_to.insert(moved_to.end(), U, U + 16);
    }
    for (std::map<std::string, Entry>::iterator it = clouds_.begin(); it != clouds_.end(); ++it) {
      std::map<std::string, Entry>::iterator was = held_.find(it->first);
      if (was != held_.end() && was->second.pyramid == it->second.pyramid) continue;
      if (it->second.pyramid->device_context() != ctx_) return false;
      dvo::compat::affine_to_rowmajor(it->second.pose, T);
      fresh.push_back(it->second.pyramid->device_frame());
      fresh_poses.insert(fresh_poses.end(), T, T + 16);
    }
    // (a call that fails -- capacity, unmatched points, a map that has dropped points -- leaves the rebuild to put things right)
    if (!gone.empty() && dvo_hip_map_remove(ctx_, map_, int(gone.size()), gone.data(), gone_poses.data(), 0, 0.0f, INFINITY) != DVO_HIP_OK) return false;
    if (!moved.empty() &&
        dvo_hip_map_move(ctx_, map_, int(moved.size()), moved.data(), moved_from.data(), moved_to.data(), 0, 0.0f, INFINITY) != DVO_HIP_OK)
      return false;
    if (!fresh.empty() && dvo_hip_map_insert(ctx_, map_, int(fresh.size()), fresh.data(), fresh_poses.data(), 0, 0.0f, INFINITY) != DVO_HIP_OK) return false;
    held_ = clouds_;
    struct dvo_hip_map_stats stats;
    if (dvo_hip_map_stats(ctx_, map_, &stats) != DVO_HIP_OK) return false;
    if (stats.vacant > stats.occupied - stats.vacant && dvo_hip_map_rehash(ctx_, map_, 0) != DVO_HIP_OK) return false;
    return true;
  }

  std::map<std::string, Entry> clouds_;
  std::map<std::string, Entry> held_;   // incremental mode: what the device map holds, as inserted (empty: nothing is known, rebuild)
  size_t capacity_;
  dvo_hip_context* ctx_;
  dvo_hip_map* map_;
  bool incremental_;
  bool colour_;          // setColour
  bool map_coloured_;    // what map_ was created as
  bool normals_;         // setNormals
  bool map_normals_;     // what map_ was created as
};

}  // namespace visualization
}  // namespace dvo
