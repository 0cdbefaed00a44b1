// dvo/core/rgbd_image.h -- RgbdCamera / RgbdCameraPyramid / RgbdImage / RgbdImagePyramid with the public surface of
// dvo_core/include/dvo/core/rgbd_image.h:90-262, backed by device-resident pyramids of libdvo_hip (include/dvo_hip.h).
//
// What a caller of the reference can rely on here:
//  * Same class names, constructors, methods, smart-pointer typedefs (boost::shared_ptr when boost is installed) and the same
//    PUBLIC FIELDS of RgbdImage (intensity, depth, *_dx, *_dy, rgb, normals, angles, pointcloud, acceleration, width, height,
//    timestamp): the reference's callers read and write them directly (dvo_benchmark/src/benchmark_slam.cpp:90, 334-339).
//  * The derived planes live on the GPU.  The fields are HOST MIRRORS: level 0 `intensity` / `depth` are the caller's own
//    matrices (no copy), `rgb` is whatever the caller stores; everything else is filled when the method that produces it in the
//    reference is called AND host mirrors are enabled (RgbdImage::hostMirrors(true), off by default), or on demand with
//    RgbdImage::syncHostMirrors().  Nothing on the alignment path reads them, and LocalTracker calls buildPointCloud() /
//    buildAccelerationStructure() on every level of every frame (dvo_slam/src/local_tracker.cpp:163-169): a download per call
//    would put a PCIe round trip on the tracking path for planes nobody looks at.
//  * calculateDerivatives() / buildPointCloud() are by-products of the device kernels; buildAccelerationStructure() starts the
//    asynchronous device build of the level's sampling planes, so local_tracker.cpp:163-169 compiles and behaves unchanged.
//  * No exceptions, like the reference: a device failure prints the library's message and aborts (the reference asserts on
//    misuse), unless an error handler is installed with DeviceContext::setErrorHandler (tests install one that throws).
#pragma once

#include <cassert>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../dvo_hip.h"
#include "datatypes.h"
#include "intrinsic_matrix.h"

namespace dvo {
namespace core {

// One engine context per (device, host thread group).  current() is what new pyramids are bound to: the calling thread's
// context if one was set (set_current / Scope), else the process-wide context of device 0.  forDevice(i) hands out the
// process-wide context of device i (created on first use), so that a caller can spread independent frame pairs over the GPUs
// of a node inside one process, the reference's own model (dvo_slam/src/keyframe_graph.cpp:576-593 runs them on a TBB pool).
// The C library serialises concurrent calls on one context, so trackers on several threads may share it.
class DeviceContext {
 public:
  typedef void (*ErrorHandler)(const char* what, const char* message);

  static dvo_hip_context* current() {
    dvo_hip_context*& c = slot();
    return c ? c : forDevice(0);
  }
  static void set_current(dvo_hip_context* c) { slot() = c; }
  static dvo_hip_context* forDevice(int device) {
    std::lock_guard<std::mutex> lock(registry_mutex());
    std::vector<dvo_hip_context*>& r = registry();
    if (device < 0) device = 0;
    if (size_t(device) >= r.size()) r.resize(size_t(device) + 1, 0);
    if (!r[size_t(device)]) {
      const int rc = dvo_hip_context_create(device, &r[size_t(device)]);
      if (rc != DVO_HIP_OK) fail("dvo_hip_context_create", dvo_hip_last_error(0));
    }
    return r[size_t(device)];
  }
  static int deviceCount() { return dvo_hip_device_count(); }
  // a further, independent context on `device` (own streams and workspace), owned by the caller: dvo_hip_context_destroy
  static dvo_hip_context* createAdditional(int device) {
    dvo_hip_context* c = 0;
    if (dvo_hip_context_create(device, &c) != DVO_HIP_OK) fail("dvo_hip_context_create", dvo_hip_last_error(0));
    return c;
  }
  // binds the calling thread to a device (or to one particular context) for the lifetime of the object
  class Scope {
   public:
    explicit Scope(int device) : previous_(slot()) { slot() = forDevice(device); }
    explicit Scope(dvo_hip_context* context) : previous_(slot()) { slot() = context; }
    ~Scope() { slot() = previous_; }

   private:
    dvo_hip_context* previous_;
  };
  static void setErrorHandler(ErrorHandler h) { handler() = h; }
  // something the caller should know that is no failure (PointCloudAggregator falling back to a grey map): to the handler if there is
  // one, else to stderr; never aborts
  static void warn(const char* what, const char* message) {
    if (handler()) handler()(what, message);
    else std::fprintf(stderr, "dvo (MI355X engine): %s: %s\n", what, message ? message : "?");
  }
  static void fail(const char* what, const char* message) {
    if (handler()) {
      handler()(what, message);
      return;
    }
    std::fprintf(stderr, "dvo (MI355X engine): %s: %s\n", what, message ? message : "?");
    std::abort();
  }

 private:
  static dvo_hip_context*& slot() {
    static thread_local dvo_hip_context* ctx = 0;
    return ctx;
  }
  static std::vector<dvo_hip_context*>& registry() {
    static std::vector<dvo_hip_context*> r;
    return r;
  }
  static std::mutex& registry_mutex() {
    static std::mutex m;
    return m;
  }
  static ErrorHandler& handler() {
    static ErrorHandler h = 0;
    return h;
  }
};

// true when the call succeeded; otherwise the error handler has run (default: message + abort)
inline bool dvo_hip_check(dvo_hip_context* ctx, int rc, const char* what) {
  if (rc == DVO_HIP_OK) return true;
  DeviceContext::fail(what, dvo_hip_last_error(ctx));
  return false;
}

typedef dvo::compat::PointCloud PointCloud;

class RgbdImage;
typedef dvo::compat::shared_ptr<RgbdImage> RgbdImagePtr;
class RgbdImagePyramid;
typedef dvo::compat::shared_ptr<RgbdImagePyramid> RgbdImagePyramidPtr;

class RgbdCamera {
 public:
  RgbdCamera(size_t width, size_t height, const IntrinsicMatrix& intrinsics) : width_(width), height_(height), intrinsics_(intrinsics) {}
  ~RgbdCamera() {}
  size_t width() const { return width_; }
  size_t height() const { return height_; }
  const IntrinsicMatrix& intrinsics() const { return intrinsics_; }
  // a free-standing image of this camera (rgbd_image.cpp:206-232): host fields only, no device pyramid behind it
  inline RgbdImagePtr create(const dvo::compat::ImageMat& intensity, const dvo::compat::ImageMat& depth) const;
  inline RgbdImagePtr create() const;
  // p = ((x - ox) / fx, (y - oy) / fy, 1, 0) * z with w = 1  (rgbd_image.cpp:186-204, 245-262)
  void buildPointCloud(const dvo::compat::ImageMat& depth, PointCloud& pointcloud) const {
    assert(size_t(dvo::compat::image_rows(depth)) == height_ && size_t(dvo::compat::image_cols(depth)) == width_);
    dvo::compat::pointcloud_resize(pointcloud, width_ * height_);
    const float* z = dvo::compat::image_ptr(depth);
    float* out = dvo::compat::pointcloud_ptr(pointcloud);
    for (size_t y = 0; y < height_; ++y) {
      const float ty = (float(y) - intrinsics_.oy()) / intrinsics_.fy();
      for (size_t x = 0; x < width_; ++x, ++z, out += 4) {
        const float tx = (float(x) - intrinsics_.ox()) / intrinsics_.fx();
        out[0] = tx * *z;
        out[1] = ty * *z;
        out[2] = *z;
        out[3] = 1.0f;
      }
    }
  }

 private:
  size_t width_, height_;
  IntrinsicMatrix intrinsics_;
};
typedef dvo::compat::shared_ptr<RgbdCamera> RgbdCameraPtr;
typedef dvo::compat::shared_ptr<const RgbdCamera> RgbdCameraConstPtr;

class RgbdCameraPyramid {
 public:
  RgbdCameraPyramid(const RgbdCamera& base) { levels_.push_back(RgbdCameraPtr(new RgbdCamera(base))); }
  RgbdCameraPyramid(size_t base_width, size_t base_height, const IntrinsicMatrix& base_intrinsics) {
    levels_.push_back(RgbdCameraPtr(new RgbdCamera(base_width, base_height, base_intrinsics)));
  }
  ~RgbdCameraPyramid() {}
  // rgbd_image.cpp:283-296: halves width, height and the whole intrinsic matrix per level
  void build(size_t levels) {
    for (size_t idx = levels_.size(); idx < levels; ++idx) {
      IntrinsicMatrix k(levels_[idx - 1]->intrinsics());
      k.scale(0.5f);
      levels_.push_back(RgbdCameraPtr(new RgbdCamera(levels_[idx - 1]->width() / 2, levels_[idx - 1]->height() / 2, k)));
    }
  }
  const RgbdCamera& level(size_t level) {
    build(level + 1);
    return *levels_[level];
  }
  const RgbdCamera& level(size_t level) const { return *levels_[level]; }
  size_t numLevels() const { return levels_.size(); }
  // intensity CV_32FC1 0..255, depth CV_32FC1 metres with NaN = invalid (asserts at rgbd_image.cpp:350, 356)
  inline RgbdImagePyramidPtr create(const dvo::compat::ImageMat& base_intensity, const dvo::compat::ImageMat& base_depth);
  // not in the reference: the pyramid of a colour frame as a camera delivers it -- an 8-bit colour plane (host memory, DVO_HIP_PIXEL_*
  // format, row pitch in bytes, 0 = tight) and the u16 depth plane (tight).  The CV_BGR2GRAY conversion the reference's callers run
  // before create (dvo_benchmark/src/benchmark_slam.cpp:55-69) and the depth scaling happen on the device (dvo_hip_frame_create_colour);
  // the device frame is built here, with every level the size admits.  Level 0's host intensity / depth matrices are downloaded from
  // the device like those of the other levels: when the pyramid is built with host mirrors on, else by syncHostMirrors().
  // pixel_format may also be a raw sensor format -- DVO_HIP_PIXEL_BAYER_{RGGB8, BGGR8, GBRG8, GRBG8} (1 byte per pixel) or
  // DVO_HIP_PIXEL_YUYV8 / _UYVY8 (2, even width): the plane a camera driver publishes as image_raw, demosaicked / converted on the device.
  inline RgbdImagePyramidPtr createFromColour(const void* colour, int pixel_format, size_t colour_pitch, const uint16_t* raw_depth,
                                              float depth_scale = 1.0f / 5000.0f);
  // not in the reference: the pyramid of two float planes that already live in DEVICE memory (both tight; intensity 0..255, depth in
  // metres with NaN = invalid -- a filtered, rendered or predicted depth image), without a trip through the host
  // (dvo_hip_frame_create_f32_device).  The build is asynchronous: the planes must stay valid until the pyramid's first use has been
  // waited for.  Host matrices as after createFromColour: downloaded when host mirrors are on, else by syncHostMirrors().
  inline RgbdImagePyramidPtr createFromFloatDevice(const void* intensity_dev, const void* depth_dev);

 private:
  std::vector<RgbdCameraPtr> levels_;
};
typedef dvo::compat::shared_ptr<RgbdCameraPyramid> RgbdCameraPyramidPtr;
typedef dvo::compat::shared_ptr<const RgbdCameraPyramid> RgbdCameraPyramidConstPtr;

class RgbdImage {
 public:
  typedef dvo::core::PointCloud PointCloud;
  typedef dvo::compat::Vec8f Vec8f;

  RgbdImage(const RgbdCamera& camera) : width(camera.width()), height(camera.height()), timestamp(0), owner_(0), level_(0), camera_(camera) {}
  virtual ~RgbdImage() {}
  const RgbdCamera& camera() const { return camera_; }

  // rgbd_image.h:161-179 -- host mirrors, see the header comment
  dvo::compat::ImageMat intensity, intensity_dx, intensity_dy;
  dvo::compat::ImageMat depth, depth_dx, depth_dy;
  dvo::compat::ImageMat normals, angles;
  dvo::compat::ImageMat rgb;
  PointCloud pointcloud;
  dvo::compat::AccelerationMat acceleration;
  size_t width, height;
  double timestamp;

  bool hasIntensity() const { return !dvo::compat::image_empty(intensity); }
  bool hasDepth() const { return !dvo::compat::image_empty(depth); }
  bool hasRgb() const { return !dvo::compat::image_empty(rgb); }
  void initialize() {}
  // derivatives and the 3-D points are by-products of the device kernels
  void calculateDerivatives() { if (hostMirrors()) syncHostMirrors(MirrorDerivatives); }
  bool calculateIntensityDerivatives() { calculateDerivatives(); return true; }
  void calculateDepthDerivatives() { calculateDerivatives(); }
  void calculateNormals() {}
  void buildPointCloud() { if (hostMirrors()) syncHostMirrors(MirrorPlanes | MirrorPointCloud); }
  // rgbd_image.cpp:534-543.  On the device: the current-frame sampling planes of this level, built asynchronously on the
  // context's build stream (dvo_hip_frames_prepare) -- what LocalTracker does with a new image before handing it to its
  // trackers (local_tracker.cpp:163-169).  Optional: match() builds whatever is missing.
  inline void buildAccelerationStructure();
  bool inImage(const float& x, const float& y) const { return x >= 0 && x < float(width) && y >= 0 && y < float(height); }
  // rgbd_image.h:199-213, rgbd_image.cpp:545-781 -- the image warps, on the device (dvo_hip_frames_warp_inverse / _forward; the semantics
  // and the deviations from the reference's loops: include/dvo_hip.h, "frames warped under a pose").  For images that belong to a
  // pyramid; on a free-standing image they fail through the error handler.  The transformation is the double one of the rest of this
  // facade (the library rounds it to float once, as the reference's cast does).  All fill result.intensity and result.depth (host
  // matrices of this level's size); result may be any RgbdImage, this one included.
  // warpIntensity: this image seen in `reference`'s raster under `transformation` (reference's camera -> this camera).  The reference
  // passes the host point cloud of the raster image; here the image that owns it stands in (same level size).
  inline void warpIntensity(const AffineTransformd& transformation, const RgbdImage& reference, RgbdImage& result);
  // the forward warps into a target of this image's own size; `intrinsics` must equal the level's own (the library projects with them).
  // warpIntensityForward and warpDepthForward draw one pixel per source pixel (DVO_HIP_WARP_NEAREST), warpDepthForwardAdvanced the
  // reference's footprint (DVO_HIP_WARP_SPLAT)
  void warpIntensityForward(const AffineTransformd& transformation, const IntrinsicMatrix& intrinsics, RgbdImage& result) {
    warpForward(transformation, intrinsics, DVO_HIP_WARP_NEAREST, result);
  }
  void warpDepthForward(const AffineTransformd& transformation, const IntrinsicMatrix& intrinsics, RgbdImage& result) {
    warpForward(transformation, intrinsics, DVO_HIP_WARP_NEAREST, result);
  }
  void warpDepthForwardAdvanced(const AffineTransformd& transformation, const IntrinsicMatrix& intrinsics, RgbdImage& result) {
    warpForward(transformation, intrinsics, DVO_HIP_WARP_SPLAT, result);
  }

  // ---- not in the reference: control over the host mirrors ---------------------------------------------------------
  enum { MirrorPlanes = 1, MirrorDerivatives = 2, MirrorPointCloud = 4, MirrorAcceleration = 8, MirrorAll = 15 };
  static bool& hostMirrors() {   // process-wide; off = the fields of levels > 0 stay empty until syncHostMirrors()
    static bool enabled = false;
    return enabled;
  }
  static void hostMirrors(bool on) { hostMirrors() = on; }
  inline void syncHostMirrors(unsigned what = MirrorAll);

 private:
  friend class RgbdImagePyramid;
  RgbdImage(RgbdImagePyramid* owner, int level, const RgbdCamera& camera)
      : width(camera.width()), height(camera.height()), timestamp(0), owner_(owner), level_(level), camera_(camera) {}
  inline void download(int plane, dvo::compat::ImageMat& m);
  inline void warpForward(const AffineTransformd& transformation, const IntrinsicMatrix& intrinsics, int mode, RgbdImage& result);
  RgbdImagePyramid* owner_;   // null for free-standing images (RgbdCamera::create)
  int level_;
  const RgbdCamera& camera_;
};

class RgbdImagePyramid {
 public:
  typedef dvo::compat::shared_ptr<dvo::core::RgbdImagePyramid> Ptr;

  RgbdImagePyramid(RgbdCameraPyramid& camera, const dvo::compat::ImageMat& intensity, const dvo::compat::ImageMat& depth)
      : camera_(camera), intensity_(intensity), depth_(depth), frame_(0), timestamp_(0) {
    assert(dvo::compat::image_is_float1(intensity) && dvo::compat::image_is_float1(depth));
    assert(dvo::compat::image_rows(intensity) == dvo::compat::image_rows(depth) && dvo::compat::image_cols(intensity) == dvo::compat::image_cols(depth));
    ctx_ = DeviceContext::current();
  }
  // (RgbdCameraPyramid::createFromColour: a device frame built already, adopted)
  RgbdImagePyramid(RgbdCameraPyramid& camera, dvo_hip_context* ctx, dvo_hip_frame* frame)
      : camera_(camera), ctx_(ctx), frame_(frame), timestamp_(0) {}
  virtual ~RgbdImagePyramid() { if (frame_) dvo_hip_frame_destroy(ctx_, frame_); }
  RgbdImagePyramid(const RgbdImagePyramid&) = delete;
  RgbdImagePyramid& operator=(const RgbdImagePyramid&) = delete;

  void compute(const size_t num_levels) { build(num_levels); }   // deprecated alias in the reference too
  // rgbd_image.cpp:156-172: idempotent, only ever grows.  The device frame is created once, with every level the image size
  // admits (a quarter of a level each: the pyramid above what a caller asks for is a few per cent of the frame), so asking for
  // more levels later neither re-uploads anything nor invalidates a handle a PointSelection holds; RgbdImage& references
  // returned by level() stay valid (the vector only grows and holds pointers).
  void build(const size_t num_levels) {
    camera_.build(num_levels);
    if (!frame_) {
      const RgbdCamera& c0 = camera_.level(0);
      int all = 1;
      while (all < DVO_HIP_MAX_LEVELS && (c0.width() >> all) >= 2 && (c0.height() >> all) >= 2) ++all;
      if (size_t(all) < num_levels) all = int(num_levels);   // frame_create rejects it with a message
      const float K[4] = {c0.intrinsics().fx(), c0.intrinsics().fy(), c0.intrinsics().ox(), c0.intrinsics().oy()};
      if (!dvo_hip_check(ctx_, dvo_hip_frame_create_f32(ctx_, int(c0.width()), int(c0.height()), K, dvo::compat::image_ptr(intensity_),
                                                        dvo::compat::image_ptr(depth_), all, &frame_), "dvo_hip_frame_create_f32"))
        frame_ = 0;
    }
    for (size_t l = levels_.size(); l < num_levels; ++l) {
      levels_.push_back(RgbdImagePtr(new RgbdImage(this, int(l), camera_.level(l))));
      levels_[l]->timestamp = timestamp_;
      if (l == 0 && !dvo::compat::image_empty(intensity_)) {   // the caller's own matrices: valid without a download
        levels_[0]->intensity = intensity_;
        levels_[0]->depth = depth_;
      } else if (l == 0 && frame_ && RgbdImage::hostMirrors()) {   // (createFromColour: the grey the device converted)
        levels_[0]->syncHostMirrors(RgbdImage::MirrorPlanes);
      }
    }
  }
  RgbdImage& level(size_t idx) {
    build(idx + 1);
    return *levels_[idx];
  }
  // not in the reference: new float matrices into this pyramid's EXISTING device frame (dvo_hip_frames_update_f32_as_ex) -- the
  // streaming form of RgbdCameraPyramid::create for every camera image.  No new frame, the handle stays (a PointSelection keeps it), and
  // so does the caller selection.  level(0).intensity / depth are rebound to the new matrices; whatever other host mirrors a level held
  // is dropped and, with host mirrors on, downloaded again.  Before the first build() it only swaps the matrices.  Returns once the
  // matrices' pixels have left the host (they may be reused).
  void update(const dvo::compat::ImageMat& intensity, const dvo::compat::ImageMat& depth) {
    assert(dvo::compat::image_is_float1(intensity) && dvo::compat::image_is_float1(depth));
    assert(dvo::compat::image_rows(intensity) == dvo::compat::image_rows(depth) && dvo::compat::image_cols(intensity) == dvo::compat::image_cols(depth));
    intensity_ = intensity;
    depth_ = depth;
    if (!frame_) return;
    const float* i[1] = {dvo::compat::image_ptr(intensity_)};
    const float* z[1] = {dvo::compat::image_ptr(depth_)};
    dvo_hip_frame* one[1] = {frame_};
    if (dvo_hip_check(ctx_, dvo_hip_frames_update_f32_as_ex(ctx_, 1, one, i, 0, z, 0, 1.0f, -1, nullptr, 0u), "dvo_hip_frames_update_f32_as_ex"))
      dvo_hip_check(ctx_, dvo_hip_upload_wait(ctx_), "dvo_hip_upload_wait");
    refreshMirrors(has_lens_ || has_rig_ || has_filter_);
  }
  // the device frame's pixels were replaced on the device (PointCloudAggregator::renderInto): the host matrices are dropped, every
  // level is mirrored from the device like the levels above 0
  void deviceFrameChanged() {
    intensity_ = dvo::compat::ImageMat();
    depth_ = dvo::compat::ImageMat();
    refreshMirrors(true);
  }

 private:
  // after new pixels: raw_planes = level 0 is not the caller's matrices
  void refreshMirrors(const bool raw_planes) {
    explicit_levels_ = 0u;   // (new pixels: the device dropped every accepted set)
    for (size_t l = 0; l < levels_.size(); ++l) {
      RgbdImage& image = *levels_[l];
      unsigned had = 0u;
      if ((l > 0 || raw_planes) && !dvo::compat::image_empty(image.intensity)) had |= RgbdImage::MirrorPlanes;
      if (!dvo::compat::image_empty(image.intensity_dx)) had |= RgbdImage::MirrorDerivatives;
      if (image.pointcloud.cols() > 0) had |= RgbdImage::MirrorPointCloud;
      if (image.acceleration.rows > 0) had |= RgbdImage::MirrorAcceleration;
      // (with a lens or a depth rig the matrices are RAW sensor planes: level 0 is what the device rectified / registered, mirrored like
      // every other level)
      image.intensity = l == 0 && !raw_planes ? intensity_ : dvo::compat::ImageMat();
      image.depth = l == 0 && !raw_planes ? depth_ : dvo::compat::ImageMat();
      image.intensity_dx = image.intensity_dy = image.depth_dx = image.depth_dy = dvo::compat::ImageMat();
      image.pointcloud = RgbdImage::PointCloud();
      image.acceleration = dvo::compat::AccelerationMat();
      if (had != 0u && RgbdImage::hostMirrors()) image.syncHostMirrors(had);
    }
  }

 public:
  double timestamp() const { return levels_.empty() ? timestamp_ : levels_[0]->timestamp; }   // rgbd_image.cpp: level(0).timestamp
  void timestamp(double t) { timestamp_ = t; for (size_t l = 0; l < levels_.size(); ++l) levels_[l]->timestamp = t; }

  // ---- extension over the reference API: the caller selection of this frame's reference points (include/dvo_hip.h,
  // dvo_hip_frames_set_selection).  A pixel of level l is selected as a reference point iff the predicate accepts it, the level-0 mask
  // byte (x << l, y << l) is non-zero and its depth lies in [min, max].  Kept until replaced or cleared, across re-ingests; works with
  // DenseTracker::match / matchBatch, LocalTracker and the validator unchanged.  The mask is copied at once (host memory).
  void setSelectionMask(const uint8_t* mask, size_t pitch) {
    const RgbdCamera& c0 = camera_.level(0);
    const size_t w = c0.width(), h = c0.height(), p = pitch ? pitch : w;
    selection_mask_.assign(w * h, 0);
    for (size_t y = 0; y < h; ++y) std::memcpy(&selection_mask_[y * w], mask + y * p, w);
    has_selection_mask_ = true;
    pushSelection();
  }
  void setSelectionDepthRange(float min_depth, float max_depth) {
    selection_min_ = min_depth;
    selection_max_ = max_depth;
    pushSelection();
  }
  void clearSelection() {
    selection_mask_.clear();
    has_selection_mask_ = false;
    selection_min_ = 0.0f;
    selection_max_ = INFINITY;
    dvo_hip_frame* one[1] = {device_frame()};
    dvo_hip_check(ctx_, dvo_hip_frames_clear_selection(ctx_, 1, one), "dvo_hip_frames_clear_selection");
  }
  // ---- extension over the reference API: the lens of this frame's camera (include/dvo_hip.h, dvo_hip_frames_set_lens; the reference's
  // nodes sit behind a CPU rectifier, dvo_ros/src/camera_base.cpp:30-31).  K_raw = fx fy ox oy of the raw image, D = k1 k2 p1 p2 k3 k4
  // k5 k6 (OpenCV / ROS plumb_bob, rational_polynomial; zeros switch terms off).  Every later update() takes its matrices as raw camera
  // planes and rectifies them on the device first; the matrices the pyramid was created from were ingested as they are.  Kept until
  // replaced or cleared.  rectify_depth false: the depth matrix is taken pixel for pixel.  Returns false where the engine refuses the lens.
  // Host mirrors: update() under a lens does NOT rebind level(0).intensity / depth to the caller's matrices (they are raw camera planes,
  // not the frame's pixels).  With host mirrors on, level 0 is downloaded like every other level that held a mirror; with host mirrors
  // off, level(0).intensity / depth are EMPTY matrices after such an update -- ask for them with syncHostMirrors -- and they stay so after
  // clearLens() until the next update() binds the caller's matrices again.
  bool setLens(const float K_raw[4], const float D[8], bool rectify_depth = true) {
    dvo_hip_lens lens;
    std::memcpy(lens.K_raw, K_raw, sizeof lens.K_raw);
    std::memcpy(lens.D, D, sizeof lens.D);
    lens.rectify_depth = rectify_depth ? 1 : 0;
    lens.reserved = 0;
    dvo_hip_frame* one[1] = {device_frame()};
    if (!dvo_hip_check(ctx_, dvo_hip_frames_set_lens(ctx_, 1, one, &lens), "dvo_hip_frames_set_lens")) return false;
    has_lens_ = true;
    return true;
  }
  void clearLens() {
    dvo_hip_frame* one[1] = {device_frame()};
    dvo_hip_check(ctx_, dvo_hip_frames_clear_lens(ctx_, 1, one), "dvo_hip_frames_clear_lens");
    has_lens_ = false;
  }
  bool hasLens() const { return has_lens_; }
  // ---- extension over the reference API: the depth rig of this frame's sensors (include/dvo_hip.h, dvo_hip_frames_set_depth_rig; the
  // reference's nodes subscribe to depth_registered topics behind a CPU depth_image_proc/register stage, dvo_ros/src/camera_base.cpp:30-33).
  // depth_K = the intrinsics of the depth sensor's image, colour_from_depth = the rigid transform from depth-sensor to colour-camera
  // coordinates in metres (Eigen::Affine3f, Eigen::Affine3d or dvo::compat::Affine3d: anything whose matrix()(i, j) reads a 4 x 4).  Every
  // later update() takes its depth matrix as the depth sensor's own image and registers it on the device first; the matrices the pyramid
  // was created from were ingested as they are.  Kept until replaced or cleared.  Returns false where the engine refuses the rig (a
  // non-finite value, a focal length <= 0, a lens that rectifies depth).  Host mirrors: as under a lens, update() under a rig does NOT
  // rebind level(0).intensity / depth to the caller's matrices (the depth matrix is the depth sensor's image, not the frame's depth):
  // level 0 is mirrored from the device like every other level, and is empty with host mirrors off until syncHostMirrors asks for it.
  template <typename Transform>
  bool setDepthRig(const IntrinsicMatrix& depth_K, const Transform& colour_from_depth) {
    dvo_hip_depth_rig rig;
    rig.K_depth[0] = depth_K.fx(); rig.K_depth[1] = depth_K.fy(); rig.K_depth[2] = depth_K.ox(); rig.K_depth[3] = depth_K.oy();
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) rig.T[i * 4 + j] = float(colour_from_depth.matrix()(i, j));
    rig.reserved[0] = rig.reserved[1] = 0;
    dvo_hip_frame* one[1] = {device_frame()};
    if (!dvo_hip_check(ctx_, dvo_hip_frames_set_depth_rig(ctx_, 1, one, &rig), "dvo_hip_frames_set_depth_rig")) return false;
    has_rig_ = true;
    return true;
  }
  void clearDepthRig() {
    dvo_hip_frame* one[1] = {device_frame()};
    dvo_hip_check(ctx_, dvo_hip_frames_clear_depth_rig(ctx_, 1, one), "dvo_hip_frames_clear_depth_rig");
    has_rig_ = false;
  }
  bool hasDepthRig() const { return has_rig_; }
  // ---- extension over the reference API: the depth filter of this frame (include/dvo_hip.h, dvo_hip_frames_set_depth_filter; the
  // reference has no such pass, SurfacePyramid::convertRawDepthImage only scales and maps 0 to NaN).  Every later update() conditions its
  // depth matrix on the device first, behind the depth rig and the lens: flying pixels at depth edges and hole borders become NaN, the
  // noise of kept pixels is smoothed.  The matrices the pyramid was created from were ingested as they are.  Kept until replaced or
  // cleared.  Returns false where the engine refuses the filter (a field out of range or not finite).  dvo_hip_depth_filter_default()
  // gives a filter to start from.  Host mirrors: as under a lens or a rig, update() under a filter does NOT rebind level(0).intensity /
  // depth to the caller's matrices (the depth matrix is the unfiltered image): level 0 is mirrored from the device like every other level.
  bool setDepthFilter(const dvo_hip_depth_filter& filter) {
    dvo_hip_frame* one[1] = {device_frame()};
    if (!dvo_hip_check(ctx_, dvo_hip_frames_set_depth_filter(ctx_, 1, one, &filter), "dvo_hip_frames_set_depth_filter")) return false;
    has_filter_ = true;
    return true;
  }
  void clearDepthFilter() {
    dvo_hip_frame* one[1] = {device_frame()};
    dvo_hip_check(ctx_, dvo_hip_frames_clear_depth_filter(ctx_, 1, one), "dvo_hip_frames_clear_depth_filter");
    has_filter_ = false;
  }
  bool hasDepthFilter() const { return has_filter_; }
  // ---- the colour of this frame (include/dvo_hip.h, dvo_hip_frames_set_colour; the reference keeps the camera image in level(0).rgb,
  // dvo_benchmark/src/benchmark_slam.cpp:89-90, and AsyncPointCloudBuilder reads it, async_point_cloud_builder.cpp:72-104).  setColour:
  // an 8-bit plane of the frame's level-0 size, rows `pitch` bytes apart (0 = tight), format DVO_HIP_PIXEL_{BGR8, RGB8, BGRA8, RGBA8} or a
  // raw sensor format (DVO_HIP_PIXEL_BAYER_*, DVO_HIP_PIXEL_YUYV8 / _UYVY8: the colour of its BGR8 image); copied at once.  What a coloured PointCloudAggregator fuses.  Kept until replaced or cleared, across update(): re-attach after an
  // update() with other content.  Returns false where the engine refuses (a pyramid with a lens: its colour must be attached rectified).
  bool setColour(const uint8_t* bgr, size_t pitch = 0, int format = DVO_HIP_PIXEL_BGR8) {
    dvo_hip_frame* one[1] = {device_frame()};
    const void* planes[1] = {bgr};
    if (!dvo_hip_check(ctx_, dvo_hip_frames_set_colour(ctx_, 1, one, planes, format, pitch, 0), "dvo_hip_frames_set_colour")) return false;
    has_colour_ = true;
    return true;
  }
  // ... from level(0).rgb where it is a three-channel float image (hasRgb()): converted on the host the way the reference's
  // p.b = intensity_ptr[0], p.g = ..[1], p.r = ..[2] does -- channel order B, G, R, each float truncated to uint8 and saturated (a NaN
  // gives 0).  False if level 0 has no such image.
  bool setColourFromRgb() {
    RgbdImage& l0 = level(0);
    const int w = int(camera_.level(0).width()), h = int(camera_.level(0).height());
    if (!l0.hasRgb() || dvo::compat::image_channels(l0.rgb) != 3 || !dvo::compat::image_is_float3(l0.rgb) ||
        dvo::compat::image_rows(l0.rgb) != h || dvo::compat::image_cols(l0.rgb) != w)
      return false;
    const float* src = dvo::compat::image_ptr(l0.rgb);
    std::vector<uint8_t> bgr(size_t(w) * h * 3);
    for (size_t i = 0; i < bgr.size(); ++i) bgr[i] = src[i] >= 255.0f ? uint8_t(255) : src[i] >= 0.0f ? uint8_t(src[i]) : uint8_t(0);
    return setColour(bgr.data(), 0, DVO_HIP_PIXEL_BGR8);
  }
  void clearColour() {
    dvo_hip_frame* one[1] = {device_frame()};
    dvo_hip_check(ctx_, dvo_hip_frames_clear_colour(ctx_, 1, one), "dvo_hip_frames_clear_colour");
    has_colour_ = false;
  }
  bool hasColour() const { return has_colour_; }
  // the caller selection's verdict on a point of level `level` (host side: PointSelection with a caller-defined predicate)
  bool selectionKeeps(size_t level, size_t x, size_t y, float z) const {
    if (has_selection_mask_ && selection_mask_[(y << level) * size_t(camera_.level(0).width()) + (x << level)] == 0) return false;
    const bool range_on = selection_min_ > 0.0f || !(selection_max_ >= 3.402823466e+38f);
    return !range_on || (selection_min_ <= z && z <= selection_max_);
  }

  // engine handles (not in the reference API)
  dvo_hip_frame* device_frame() { build(1); return frame_; }
  // The frame for a match whose reference points a stock predicate selects (thresholds): the accepted sets a caller-defined predicate
  // left on the device (PointSelection, point_selection.h) are dropped first, so that they never stand in for the thresholds' selection.
  dvo_hip_frame* reference_frame() {
    dvo_hip_frame* f = device_frame();
    for (int l = 0; explicit_levels_ != 0u && l < DVO_HIP_MAX_LEVELS; ++l)
      if (explicit_levels_ >> l & 1u) dvo_hip_check(ctx_, dvo_hip_frame_set_level_selection(ctx_, f, l, nullptr), "dvo_hip_frame_set_level_selection");
    explicit_levels_ = 0u;
    return f;
  }
  // (PointSelection with a caller-defined predicate: level `level` holds an accepted set handed to the device)
  void noteExplicitSelection(size_t level) { explicit_levels_ |= 1u << level; }
  size_t builtLevels() const { return levels_.size(); }
  dvo_hip_context* device_context() { return ctx_; }
  RgbdCameraPyramid& cameraPyramid() { return camera_; }

 private:
  void pushSelection() {
    dvo_hip_frame* one[1] = {device_frame()};
    const uint8_t* masks[1] = {has_selection_mask_ ? selection_mask_.data() : nullptr};
    dvo_hip_check(ctx_, dvo_hip_frames_set_selection(ctx_, 1, one, masks, 0, 0, selection_min_, selection_max_), "dvo_hip_frames_set_selection");
  }

  RgbdCameraPyramid& camera_;
  dvo::compat::ImageMat intensity_, depth_;
  dvo_hip_context* ctx_;
  dvo_hip_frame* frame_;
  std::vector<RgbdImagePtr> levels_;
  double timestamp_;
  std::vector<uint8_t> selection_mask_;
  bool has_selection_mask_ = false;
  bool has_lens_ = false;
  bool has_rig_ = false;
  bool has_filter_ = false;
  bool has_colour_ = false;
  float selection_min_ = 0.0f, selection_max_ = INFINITY;
  unsigned explicit_levels_ = 0u;
};

inline RgbdImagePtr RgbdCamera::create(const dvo::compat::ImageMat& intensity, const dvo::compat::ImageMat& depth) const {
  RgbdImagePtr result(new RgbdImage(*this));
  result->intensity = intensity;
  result->depth = depth;
  return result;
}

inline RgbdImagePtr RgbdCamera::create() const { return RgbdImagePtr(new RgbdImage(*this)); }

inline RgbdImagePyramidPtr RgbdCameraPyramid::create(const dvo::compat::ImageMat& base_intensity, const dvo::compat::ImageMat& base_depth) {
  return RgbdImagePyramidPtr(new RgbdImagePyramid(*this, base_intensity, base_depth));
}

inline RgbdImagePyramidPtr RgbdCameraPyramid::createFromColour(const void* colour, int pixel_format, size_t colour_pitch, const uint16_t* raw_depth,
                                                               float depth_scale) {
  const RgbdCamera& c0 = level(0);
  int all = 1;
  while (all < DVO_HIP_MAX_LEVELS && (c0.width() >> all) >= 2 && (c0.height() >> all) >= 2) ++all;
  const float K[4] = {c0.intrinsics().fx(), c0.intrinsics().fy(), c0.intrinsics().ox(), c0.intrinsics().oy()};
  dvo_hip_context* ctx = DeviceContext::current();
  dvo_hip_frame* frame = 0;
  if (!dvo_hip_check(ctx, dvo_hip_frame_create_colour(ctx, int(c0.width()), int(c0.height()), K, colour, pixel_format, colour_pitch, raw_depth,
                                                      depth_scale, all, &frame), "dvo_hip_frame_create_colour"))
    frame = 0;
  return RgbdImagePyramidPtr(new RgbdImagePyramid(*this, ctx, frame));
}

inline RgbdImagePyramidPtr RgbdCameraPyramid::createFromFloatDevice(const void* intensity_dev, const void* depth_dev) {
  const RgbdCamera& c0 = level(0);
  int all = 1;
  while (all < DVO_HIP_MAX_LEVELS && (c0.width() >> all) >= 2 && (c0.height() >> all) >= 2) ++all;
  const float K[4] = {c0.intrinsics().fx(), c0.intrinsics().fy(), c0.intrinsics().ox(), c0.intrinsics().oy()};
  dvo_hip_context* ctx = DeviceContext::current();
  dvo_hip_frame* frame = 0;
  if (!dvo_hip_check(ctx, dvo_hip_frame_create_f32_device(ctx, int(c0.width()), int(c0.height()), K, intensity_dev, depth_dev, all, &frame),
                     "dvo_hip_frame_create_f32_device"))
    frame = 0;
  return RgbdImagePyramidPtr(new RgbdImagePyramid(*this, ctx, frame));
}

inline void RgbdImage::buildAccelerationStructure() {
  if (!owner_) return;
  // The callers walk the levels of a new image (dvo_slam/src/local_tracker.cpp:163-169): the first call prepares every level that has
  // been built from this one upwards in ONE background launch, the calls for the other levels find their planes in place.  The
  // reference role is prepared along with it, speculatively (negative thresholds: the selection thresholds of the context's last
  // match, and only if the image holds no selection yet -- a key frame that was selected for a tracker's thresholds keeps it):
  // in a tracking front end every image is the odometry tracker's reference one frame later (local_tracker.cpp:198-206), and
  // deriving it then would sit inside that match.
  dvo_hip_config c = {};
  c.last_level = level_;
  c.first_level = int(owner_->builtLevels()) > level_ ? int(owner_->builtLevels()) - 1 : level_;
  c.max_iterations_per_level = 1;
  dvo_hip_frame* one[1] = {owner_->device_frame()};
  dvo_hip_check(owner_->device_context(), dvo_hip_frames_prepare(owner_->device_context(), 1, one, DVO_HIP_ROLE_CURRENT, &c), "dvo_hip_frames_prepare");
  c.intensity_derivative_threshold = c.depth_derivative_threshold = -1.0f;
  dvo_hip_check(owner_->device_context(), dvo_hip_frames_prepare(owner_->device_context(), 1, one, DVO_HIP_ROLE_REFERENCE, &c), "dvo_hip_frames_prepare");
  if (hostMirrors()) syncHostMirrors(MirrorAcceleration);
}

inline void RgbdImage::download(int plane, dvo::compat::ImageMat& m) {
  m = dvo::compat::image_create(int(height), int(width));
  dvo_hip_check(owner_->device_context(), dvo_hip_frame_download_plane(owner_->device_context(), owner_->device_frame(), level_, plane,
                                                                       dvo::compat::image_ptr_mut(m)), "dvo_hip_frame_download_plane");
}

inline void RgbdImage::warpIntensity(const AffineTransformd& transformation, const RgbdImage& reference, RgbdImage& result) {
  if (!owner_ || !reference.owner_) {
    DeviceContext::fail("RgbdImage::warpIntensity", "both images must belong to a pyramid");
    return;
  }
  double m[16];
  dvo::compat::affine_to_rowmajor(transformation, m);
  dvo::compat::ImageMat I = dvo::compat::image_create(int(reference.height), int(reference.width));
  dvo::compat::ImageMat Z = dvo::compat::image_create(int(reference.height), int(reference.width));
  dvo_hip_frame* raster[1] = {reference.owner_->device_frame()};
  dvo_hip_frame* sampled[1] = {owner_->device_frame()};
  float* i[1] = {dvo::compat::image_ptr_mut(I)};
  float* z[1] = {dvo::compat::image_ptr_mut(Z)};
  if (level_ != reference.level_) {
    DeviceContext::fail("RgbdImage::warpIntensity", "the images are of different pyramid levels");
    return;
  }
  if (!dvo_hip_check(owner_->device_context(), dvo_hip_frames_warp_inverse(owner_->device_context(), 1, raster, sampled, m, level_, nullptr, i, z,
                                                                           nullptr, 0), "dvo_hip_frames_warp_inverse"))
    return;
  result.intensity = I;
  result.depth = Z;
  result.initialize();
}

inline void RgbdImage::warpForward(const AffineTransformd& transformation, const IntrinsicMatrix& intrinsics, int mode, RgbdImage& result) {
  if (!owner_) {
    DeviceContext::fail("RgbdImage::warpForward", "the image must belong to a pyramid");
    return;
  }
  const IntrinsicMatrix& own = camera_.intrinsics();
  if (intrinsics.fx() != own.fx() || intrinsics.fy() != own.fy() || intrinsics.ox() != own.ox() || intrinsics.oy() != own.oy()) {
    DeviceContext::fail("RgbdImage::warpForward", "the intrinsics must be those of the image's own level");
    return;
  }
  double m[16];
  dvo::compat::affine_to_rowmajor(transformation, m);
  dvo::compat::ImageMat I = dvo::compat::image_create(int(height), int(width)), Z = dvo::compat::image_create(int(height), int(width));
  dvo_hip_frame* one[1] = {owner_->device_frame()};
  float* i[1] = {dvo::compat::image_ptr_mut(I)};
  float* z[1] = {dvo::compat::image_ptr_mut(Z)};
  dvo_hip_warp_params params = dvo_hip_warp_params_default();
  params.mode = mode;
  if (!dvo_hip_check(owner_->device_context(), dvo_hip_frames_warp_forward(owner_->device_context(), 1, one, m, level_, &params, i, z, 0),
                     "dvo_hip_frames_warp_forward"))
    return;
  result.intensity = I;
  result.depth = Z;
  result.initialize();
}

// fills the requested host fields from the device planes (bit-identical to what the reference computes on the host:
// tests/test_gpu_parity.py compares every plane with the oracle)
inline void RgbdImage::syncHostMirrors(unsigned what) {
  if (!owner_) {   // free-standing image: only the point cloud can be derived, on the host
    if ((what & MirrorPointCloud) && hasDepth()) camera_.buildPointCloud(depth, pointcloud);
    return;
  }
  const bool need_planes = (what & (MirrorPlanes | MirrorPointCloud | MirrorAcceleration)) != 0;
  // (level 0 of a pyramid built from the caller's float matrices has them already; one built from a colour plane downloads its grey)
  if (need_planes && dvo::compat::image_empty(intensity)) {
    download(0, intensity);
    download(1, depth);
  }
  if ((what & (MirrorDerivatives | MirrorAcceleration)) && dvo::compat::image_empty(intensity_dx)) {
    download(2, intensity_dx);
    download(3, intensity_dy);
    download(4, depth_dx);
    download(5, depth_dy);
  }
  if (what & MirrorPointCloud) camera_.buildPointCloud(depth, pointcloud);
  if (what & MirrorAcceleration) {   // {I, Z, Idx, Idy, Zdx, Zdy, 0, 0} interleaved (rgbd_image.cpp:534-543)
    const dvo::compat::ImageMat* planes[6] = {&intensity, &depth, &intensity_dx, &intensity_dy, &depth_dx, &depth_dy};
    dvo::compat::acceleration_fill(acceleration, int(height), int(width), planes);
  }
}

}  // namespace core
}  // namespace dvo
