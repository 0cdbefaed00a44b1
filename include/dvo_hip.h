/*
 * dvo_hip.h -- C-ABI of libdvo_hip.so: the MI355X (gfx950) implementation of the dense RGB-D
 * alignment hot path of tum-vision/dvo_slam (dvo::DenseTracker::match and the image data model
 * that feeds it).
 *
 * The reference has no plugin / FFI layer: the drop-in boundary is the C++ class API of dvo_core
 * (SURVEY.md section 8b).  This header is the thin C layer underneath the header-only C++ facade
 * `include/dvo/` that reproduces that class API; every entry point cites the reference interface
 * it replaces (paths relative to /root/reference).  Plain C types only, caller-allocated outputs,
 * int status return (0 = ok, negative = error, see dvo_hip_last_error), no exceptions cross the
 * ABI.  A context is thread-compatible (one thread at a time); use one context per host thread,
 * mirroring "one DenseTracker per thread" (dvo_slam/src/local_tracker.cpp:69-70).
 *
 * There is NO CPU fallback: every compute entry point fails with DVO_HIP_ERR_NO_DEVICE when no
 * gfx950 device is usable.
 */
#ifndef DVO_HIP_H_
#define DVO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVO_HIP_MAX_LEVELS 8

enum {
  DVO_HIP_OK = 0,
  DVO_HIP_ERR_NO_DEVICE = -1,
  DVO_HIP_ERR_INVALID = -2,
  DVO_HIP_ERR_HIP = -3,
  DVO_HIP_ERR_CAPACITY = -4
};

/* dvo::DenseTracker::TerminationCriteria::Enum, dvo_core/include/dvo/dense_tracking.h:71-81 */
enum {
  DVO_HIP_ITERATIONS_EXCEEDED = 0,
  DVO_HIP_INCREMENT_TOO_SMALL = 1,
  DVO_HIP_LOGLIKELIHOOD_DECREASED = 2,
  DVO_HIP_TOO_FEW_CONSTRAINTS = 3,
  DVO_HIP_TERMINATION_UNSET = -1
};

/* The fields of dvo::DenseTracker::Config that match() reads (dense_tracking.h:42-69; defaults
 * dvo_core/src/dense_tracking_config.cpp:27-42).  UseWeighting / UseParallel / InfluenceFunction* /
 * ScaleEstimator* are dead for match() and live only in the C++ facade. */
typedef struct {
  int32_t first_level;               /* FirstLevel, default 3 */
  int32_t last_level;                /* LastLevel, default 1 */
  int32_t max_iterations_per_level;  /* default 100 */
  int32_t use_initial_estimate;      /* default 0 */
  double precision;                  /* default 5e-7 */
  double mu;                         /* default 0 */
  float intensity_derivative_threshold; /* default 0 */
  float depth_derivative_threshold;     /* default 0 */
} dvo_hip_config;

/* dvo::DenseTracker::IterationStats, dense_tracking.h:83-101 */
typedef struct {
  int32_t id;
  int32_t valid_constraints;
  double tdist_loglik;               /* TDistributionLogLikelihood (= -ll) */
  double tdist_mean[2];              /* always 0 */
  double tdist_precision[4];         /* row-major 2x2 */
  double prior_loglik;
  double increment[6];               /* EstimateIncrement, twist (v, omega) */
  double information[36];            /* EstimateInformation, row-major 6x6, includes mu*I */
} dvo_hip_iteration_stats;

/* dvo::DenseTracker::LevelStats, dense_tracking.h:104-117 */
typedef struct {
  int32_t id;
  int32_t max_valid_pixels;
  int32_t valid_pixels;
  int32_t termination;
  int32_t n_iterations;
  int32_t first_iteration_index;     /* index of this level's first record in the iteration array */
} dvo_hip_level_stats;

/* dvo::DenseTracker::Result, dense_tracking.h:125-140 (Statistics are returned separately) */
typedef struct {
  double transformation[16];         /* row-major 4x4. in: initial guess when use_initial_estimate;
                                        out: estimate^-1 = current -> reference (dense_tracking.cpp:371) */
  double information[36];            /* A_last * 0.008^2 (dense_tracking.cpp:372) */
  double loglik;                     /* dense_tracking.cpp:373 */
  int32_t n_levels;
  int32_t n_iterations_total;
  /* Keyframe-selection statistics, by-products of the last normal equations (what the reference's front-end derives on
   * the host from Information / Statistics for every frame): */
  double entropy;                    /* log det(information): EntropyRatioTrackingResultEvaluation::value,
                                        dvo_slam/src/tracking_result_evaluation.cpp:52-55 */
  double condition_number;           /* |lambda_max / lambda_min| of information, dvo_slam/src/keyframe_tracker.cpp:170-196;
                                        NaN unless dvo_hip_set_option(ctx, "condition_number", 1) */
  double constraint_ratio;           /* ValidConstraints(last iteration) / ValidPixels(last level), keyframe_tracker.cpp:165-168 */
  double constraint_ratio_accepted;  /* same for LastIterationWithIncrement, 0 if there is none
                                        (dvo_slam/src/constraints/constraint_proposal_voter.cpp:136-140) */
} dvo_hip_result;

/* the two roles of a frame in an alignment (dvo_hip_frames_prepare, dvo_hip_frames_update_raw*_as) */
#define DVO_HIP_ROLE_CURRENT 0
#define DVO_HIP_ROLE_REFERENCE 1

typedef struct dvo_hip_context dvo_hip_context;
typedef struct dvo_hip_frame dvo_hip_frame;

/* ---- context -------------------------------------------------------------------------------- */
/* One context = one device + one HIP stream + scratch.  Replaces the per-tracker scratch vectors
 * (dense_tracking.h:205-212) and nothing else. */
int dvo_hip_context_create(int device, dvo_hip_context** out);
void dvo_hip_context_destroy(dvo_hip_context* ctx);
/* last error text of this context (or of context creation when ctx == NULL) */
const char* dvo_hip_last_error(const dvo_hip_context* ctx);
/* the hipStream_t all work of this context is enqueued on (for HIP-event timing by the caller) */
void* dvo_hip_context_stream(dvo_hip_context* ctx);
/* the device index the context was created on (-1 for a null context) */
int dvo_hip_context_device(const dvo_hip_context* ctx);
int dvo_hip_device_count(void);

/* ---- frames: RgbdCameraPyramid::create + RgbdImagePyramid::build + buildAccelerationStructure --
 * (dvo_core/include/dvo/core/rgbd_image.h:127-147,242-262; rgbd_image.cpp:156-172,283-296,419-543)
 * Builds the whole device-resident pyramid: 2x2-mean intensity, subsampled depth, halved
 * intrinsics, clamped central-difference derivatives, interleaved sampling planes.
 * K = {fx, fy, ox, oy} of level 0.  `levels` = Config::getNumLevels() = FirstLevel + 1.
 * Every dvo_hip_frame_create_* refuses a K that is not finite or has fx <= 0 or fy <= 0 with DVO_HIP_ERR_INVALID, before it allocates. */
int dvo_hip_frame_create_f32(dvo_hip_context* ctx, int width, int height, const float K[4],
                             const float* intensity /* 0..255 */, const float* depth /* metres, NaN invalid */,
                             int levels, dvo_hip_frame** out);
/* Ingest of raw sensor planes (dvo_benchmark/src/benchmark_slam.cpp:46-93 after BGR2GRAY;
 * SurfacePyramid::convertRawDepthImageSse, dvo_core/src/core/surface_pyramid.cpp:65-105):
 * grey u8 -> float 0..255, depth u16 * depth_scale, 0 -> NaN, converted on the device. */
int dvo_hip_frame_create_raw(dvo_hip_context* ctx, int width, int height, const float K[4],
                             const uint8_t* grey, const uint16_t* raw_depth, float depth_scale,
                             int levels, dvo_hip_frame** out);
/* Same, but the two raw planes are already resident in device memory (HBM). */
int dvo_hip_frame_create_raw_device(dvo_hip_context* ctx, int width, int height, const float K[4],
                                    const void* grey_dev, const void* raw_depth_dev, float depth_scale,
                                    int levels, dvo_hip_frame** out);
/* Re-ingest new raw planes (device pointers) into an existing frame: no allocation, asynchronous on the
 * context's build stream.  The streaming use of RgbdCameraPyramid::create for every camera frame
 * (dvo_ros/src/camera_dense_tracking.cpp:243); invalidates the frame's cached point selection. */
int dvo_hip_frame_update_raw_device(dvo_hip_context* ctx, dvo_hip_frame* frame, const void* grey_dev,
                                    const void* raw_depth_dev, float depth_scale);
/* The same for n frames of one camera in one launch per pyramid level (blockIdx.z = frame). */
int dvo_hip_frames_update_raw_device(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                     const void* const* grey_dev, const void* const* raw_depth_dev, float depth_scale);
/* Update + dvo_hip_frames_prepare(role, cfg) in ONE pass over the raw planes: the frames are about to be used in that role
 * (DVO_HIP_ROLE_*), so level 0 is written straight into the role's planes instead of float planes that the prepare step would
 * have to read back (40 instead of 56 B of traffic per pixel for a current frame, 33 instead of 45 for a reference).
 * A frame can still be used in the other role later. */
int dvo_hip_frames_update_raw_device_as(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                        const void* const* grey_dev, const void* const* raw_depth_dev, float depth_scale,
                                        int role, const dvo_hip_config* cfg);
/* The same from HOST memory: the raw planes are transferred on an upload stream of the context (DMA), the build follows on
 * the build stream; the call returns at once.  With planes in pinned memory (dvo_hip_host_alloc) the transfer of the next
 * batch overlaps the build and the alignment of earlier ones.  A frame whose grey plane directly follows its depth plane
 * (grey == (uint8_t*)(raw_depth + w*h)) moves in one transfer, and so does a run of such frames that follow each other in
 * host memory at a stride of 3*w*h bytes rounded up to even (one 0.9 MB transfer per 640x480 frame reaches ~30 GB/s, a
 * whole batch per transfer the link rate).  The host planes must stay unchanged until
 * dvo_hip_upload_wait() returns (or until a dvo_hip_match* call that uses the frames has returned).
 * Replaces the per-frame cv::imread -> convert -> RgbdCameraPyramid::create hand-over (dvo_benchmark/src/benchmark_slam.cpp:46-93,
 * dvo_ros/src/camera_dense_tracking.cpp:243) for a stream of frames. */
int dvo_hip_frames_update_raw(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                              const uint8_t* const* grey, const uint16_t* const* raw_depth, float depth_scale);
int dvo_hip_frames_update_raw_as(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                 const uint8_t* const* grey, const uint16_t* const* raw_depth, float depth_scale,
                                 int role, const dvo_hip_config* cfg);
/* The two role-aware ingests with PER-CALL behaviour instead of the context-wide options "defer_ingest" / "keep_raw_copy" (a caller
 * that shares its context with other host threads must not toggle options around a call): flags = DVO_HIP_INGEST_DEFER (device
 * planes only: the request is recorded -- pointer arrays copied, the raw planes must stay valid -- and carried out right behind the
 * first launches of the next dvo_hip_match_batch, or by whatever entry point comes first, or by dvo_hip_flush_deferred) |
 * DVO_HIP_INGEST_NO_RAW_COPY (a frame ingested into the REFERENCE role keeps no copy of its raw planes: it serves as a reference with
 * cfg's thresholds until it is ingested again, anything else fails with DVO_HIP_ERR_INVALID and leaves every frame as it was).
 * dvo_slam_amd/apps/stream_pipeline.cpp (the loop bench.py times) uses these. */
#define DVO_HIP_INGEST_DEFER 1u
#define DVO_HIP_INGEST_NO_RAW_COPY 2u
int dvo_hip_frames_update_raw_device_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                           const void* const* grey_dev, const void* const* raw_depth_dev, float depth_scale,
                                           int role, const dvo_hip_config* cfg, unsigned flags);
int dvo_hip_frames_update_raw_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                    const uint8_t* const* grey, const uint16_t* const* raw_depth, float depth_scale,
                                    int role, const dvo_hip_config* cfg, unsigned flags);
/* ---- colour ingest: an 8-bit colour plane + the u16 depth plane, converted to grey on the device ----------------------------
 * Real frame sources deliver colour: the PNGs under a TUM sequence's rgb/ are RGB, OpenCV's imread hands over BGR, ROS cameras publish "bgr8" / "rgb8", camera
 * SDKs emit 4-byte BGRA / RGBA surfaces.  The reference's callers convert on the host before RgbdCameraPyramid::create
 * (dvo_benchmark/src/benchmark_slam.cpp:55-69, dvo_ros/src/camera_dense_tracking.cpp:222-224,
 * dvo_slam/src/camera_keyframe_tracking.cpp:227-229); these entry points take the colour plane itself.  The grey value is OpenCV's
 * CV_BGR2GRAY fixed point, (B*1868 + G*9617 + R*4899 + 8192) >> 14, and then goes through the grey ingest's pipeline unchanged: the
 * same planes, bit for bit, as the grey entry points fed that grey plane.  The frame's copy of its raw planes stays grey u8 + depth u16
 * (3 B per pixel), so a later role, a reselection and dvo_hip_frames_prepare work as after a grey ingest.
 * colour_pitch = bytes from one row of the colour plane to the next, 0 = tight (width * channels); the depth plane is tight.
 * DVO_HIP_ERR_INVALID, every frame left as it was: an unknown format, a null pointer or entry, 0 < colour_pitch < width * channels,
 * colour_pitch >= 2^31. */
#define DVO_HIP_PIXEL_BGR8 1  /* OpenCV imread, ROS "bgr8" */
#define DVO_HIP_PIXEL_RGB8 2  /* TUM rgb PNGs, ROS "rgb8" */
#define DVO_HIP_PIXEL_BGRA8 3 /* 4-byte pixels, alpha ignored */
#define DVO_HIP_PIXEL_RGBA8 4
/* ---- raw sensor planes: Bayer mosaics and YUV 4:2:2, as a camera driver publishes them (image_raw) ----------------------------------
 * RGB-D sensors do not deliver BGR: the Kinect / OpenNI driver publishes a Bayer GRBG mosaic (1 B per pixel), Xtion, RealSense and UVC
 * cameras YUV 4:2:2 (2 B per pixel); the reference's nodes sit behind image_proc, which debayers and rectifies on the CPU
 * (dvo_ros/src/camera_base.cpp:30 subscribes to camera/rgb/image_rect).  Every entry point that takes a pixel_format takes these six
 * too -- dvo_hip_frame_create_colour*, dvo_hip_frames_update_colour*_as_ex, dvo_hip_frames_update_colour_f32depth*,
 * dvo_hip_frames_set_colour -- with everything the ingest combines: host or device planes, a pitch, a role, DVO_HIP_INGEST_DEFER (the
 * request records the sensor planes and they are converted at the flush), DVO_HIP_INGEST_NO_RAW_COPY, a lens, a depth rig.
 *   semantics   dvo_slam_amd/csrc/sensor_formats.h, integer only.  A sensor format is DEFINED by its BGR8 image -- a bilinear demosaic in
 *               OpenCV's arithmetic with neighbours outside the image read by reflection (the interior is OpenCV's COLOR_Bayer*2BGR, the
 *               one-pixel border is ours), or BT.601 limited range in 20-bit fixed point (meant to be OpenCV's COLOR_YUV2BGR_YUY2 /
 *               _UYVY; that equality is not verified) -- and the frame is then a BGR8 frame: bit for bit the frame fed that BGR8 image,
 *               or its CV_BGR2GRAY grey plane through the grey entry points, in every plane of every level, and
 *               dvo_hip_frames_set_colour stores the 0x00RRGGBB of that image.  For YUV the grey is therefore NOT the Y byte.
 *   planes      1 byte per pixel (Bayer) or 2 (YUV); colour_pitch 0 = tight, else at least width * bytes; any byte alignment of pointer
 *               and pitch.  A Bayer plane needs width >= 2 and height >= 2, a YUV plane an even width: DVO_HIP_ERR_INVALID otherwise, like
 *               every value in 6..15 and from 22 on, before anything is touched.
 *   pipeline    one conversion pass on the build stream at the head of the ingest (k_sensor_convert, sensor_convert.hip) writes the
 *               grey plane into the frame's own u8 staging plane; the rig pass, the lens pass and the ingest then run as for a grey8
 *               source at that address.  From host memory the upload buffers carry the sensor plane itself: 1 or 2 B per pixel.
 *   raw copy    the staging plane the pass wrote IS the grey half of the frame's raw copy: with u16 depth the ingest stores the depth
 *               half beside it (and rewrites the grey bytes with the values it read), with float depth the copy is the float planes as
 *               for any float-depth ingest.  keep_raw_copy, another role, a reselection and a download behave as after a grey ingest.
 *   counters    "sensor_ingests" counts the frames; "colour_ingests" does not count them. */
#define DVO_HIP_PIXEL_BAYER_RGGB8 16   /* named by the 2 x 2 block at the image's top-left corner, row-major: R G / G B */
#define DVO_HIP_PIXEL_BAYER_BGGR8 17
#define DVO_HIP_PIXEL_BAYER_GBRG8 18
#define DVO_HIP_PIXEL_BAYER_GRBG8 19
#define DVO_HIP_PIXEL_YUYV8       20   /* bytes Y0 U Y1 V per pixel pair (ROS "yuv422_yuy2") */
#define DVO_HIP_PIXEL_UYVY8       21   /* bytes U Y0 V Y1 per pixel pair (ROS "yuv422") */
/* the counterpart of dvo_hip_frame_create_raw: host planes (staged through the context's upload buffers) */
int dvo_hip_frame_create_colour(dvo_hip_context* ctx, int width, int height, const float K[4], const void* colour, int pixel_format,
                                size_t colour_pitch, const uint16_t* raw_depth, float depth_scale, int levels, dvo_hip_frame** out);
/* the counterpart of dvo_hip_frame_create_raw_device: both planes in device memory */
int dvo_hip_frame_create_colour_device(dvo_hip_context* ctx, int width, int height, const float K[4], const void* colour_dev,
                                       int pixel_format, size_t colour_pitch, const void* raw_depth_dev, float depth_scale, int levels,
                                       dvo_hip_frame** out);
/* The counterparts of dvo_hip_frames_update_raw_device_as_ex / dvo_hip_frames_update_raw_as_ex.  role = DVO_HIP_ROLE_*, or -1 with
 * cfg NULL for a plain update (dvo_hip_frames_update_raw_device / dvo_hip_frames_update_raw).  flags as there (DVO_HIP_INGEST_DEFER:
 * device planes only, the request records the format and pitch).  From host memory a frame whose colour plane directly follows its depth
 * plane (colour == (char*)(raw_depth + w*h), tight pitch) moves in one transfer, and so does a run of such frames that follow each other
 * at a stride of (2 + channels)*w*h bytes rounded up to even. */
int dvo_hip_frames_update_colour_device_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                              const void* const* colour_dev, int pixel_format, size_t colour_pitch,
                                              const void* const* raw_depth_dev, float depth_scale, int role, const dvo_hip_config* cfg,
                                              unsigned flags);
int dvo_hip_frames_update_colour_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* colour,
                                       int pixel_format, size_t colour_pitch, const uint16_t* const* raw_depth, float depth_scale,
                                       int role, const dvo_hip_config* cfg, unsigned flags);
/* ---- float planes: a float32 intensity and / or depth plane, host or device, into existing frames --------------------------------
 * The reference's class API hands over float matrices (RgbdCameraPyramid::create(intensity, depth)), ROS drivers publish registered depth
 * as "32FC1" metres with NaN holes next to a "bgr8" / "mono8" image (dvo_ros/src/camera_dense_tracking.cpp:231-240), and a filtered,
 * rendered or predicted depth image is a float tensor in device memory.  These entry points are the streaming ingest for such planes:
 * they re-ingest into existing frames, build level 0 straight into `role`, can be deferred, and take the same strip kernels.
 *   image plane  DVO_HIP_PIXEL_F32: one float per pixel, 0..255, taken as is (no clamp, no rounding); its pitch follows the colour
 *                pitch rules, in bytes, 0 = tight (width * 4).  Or an 8-bit plane: DVO_HIP_PIXEL_GREY8 (one byte per pixel) or one of
 *                the four colour formats, converted as by the colour ingest.
 *   scale        "taken as is" includes the scale: a float image in [0, 1], a dim or low-contrast frame and depths in other units than
 *                the test scenes' 0.4-12 m are legal.  The f32-Gram schedules (option "variant" 0, 5, 6) do not depend on the
 *                intensity's scale by one bit.  The default schedule forms its normal equations from f16 high + low parts, which have
 *                an absolute floor: measured on an MI355X, with the grey levels x 2^ki and the depths x 2^kz against 8-bit levels at
 *                those depths, it keeps every documented bound for ki >= -16 and ki - kz >= -16 -- a [0, 1] image
 *                is ki = -8 -- and for depth scales of 1/64 ... 256 at 8-bit levels.  Outside that range nothing is flagged and no pair
 *                is repeated (the "f16_range_repeats" guard is for components too LARGE for f16): residuals, constraints, precision
 *                matrix and log-likelihood keep their accuracy, the normal equations lose about a factor of four of it per factor of
 *                four in scale (1.3e-4 instead of 1e-5 at ki = -16, kz = 4).  Rescale such planes, or run them under "variant" 6.
 *   depth plane  DVO_HIP_DEPTH_F32: one float per pixel, metres, NaN = hole, with a pitch of its own in bytes, 0 = tight (width * 4).
 *                The stored depth is z * depth_scale, one rounding of its own (depth_scale 1 is exact; float millimetres are
 *                depth_scale 1e-3f).  Nothing else is done to a value: NaN stays NaN (a hole); 0, negative values and +-infinity are
 *                stored as they are (times depth_scale), exactly as dvo_hip_frame_create_f32 stores them -- 0 is NOT a hole here (it is
 *                in a u16 plane, DVO_HIP_DEPTH_U16).  Such pixels then behave as in the reference: an infinite depth or depth
 *                difference fails the selection's finiteness test or warps out of the image, a depth <= 0 warps behind the camera.
 *   supported    F32 image + F32 depth; GREY8 / BGR8 / RGB8 / BGRA8 / RGBA8 image + F32 depth.  F32 image + U16 depth: DVO_HIP_ERR_INVALID.
 *   alignment    float planes and their pitches must be multiples of 4 bytes (DVO_HIP_ERR_INVALID otherwise).  The strip kernel takes
 *                frames of even width whose float rows are 8-byte aligned (address and pitch; an 8-bit image plane under the colour
 *                ingest's rules, width a multiple of 4); everything else takes the tile kernel.  Same planes either way.
 *   raw copy     every frame owns float planes I and Z of level 0; after an ingest with float depth THEY are the frame's raw copy (I holds
 *                the converted grey as float after an 8-bit image), the u8 / u16 staging area is not used.  A later role, other
 *                thresholds, dvo_hip_frame_select, dvo_hip_frames_prepare, a caller selection and dvo_hip_frame_download_plane work as
 *                after any other ingest, and a frame may alternate between u8 / u16 and float ingests.  DVO_HIP_INGEST_NO_RAW_COPY and
 *                option "keep_raw_copy" mean what they mean above: no copy, the other role is refused with DVO_HIP_ERR_INVALID.
 * role = DVO_HIP_ROLE_*, or -1 with cfg NULL for a plain update.  flags: DVO_HIP_INGEST_DEFER (device planes only -- the host entry
 * points refuse it; the request records both formats and both pitches) | DVO_HIP_INGEST_NO_RAW_COPY.  Host planes go through the upload
 * buffers in slots of [depth][image]; a frame whose tight image plane directly follows its tight depth plane moves in one transfer, a run
 * of such frames at a stride of the two planes' bytes rounded up to 8 in one, and padded pitches are repacked by a 2-D transfer.
 * DVO_HIP_ERR_INVALID, every frame and counter left as it was: an unknown format, F32 image + U16 depth, a null array or entry, a pitch
 * below width * 4 (or width * channels), a pitch above 2^31 - 1, a misaligned float plane, frames of differing cameras or level
 * counts, DVO_HIP_INGEST_DEFER with host planes. */
#define DVO_HIP_PIXEL_GREY8 0 /* one byte per pixel; the float-depth entry points only (the colour entry points refuse it) */
#define DVO_HIP_PIXEL_F32 5   /* one float per pixel, 0..255 (other scales: "scale" above) */
#define DVO_HIP_DEPTH_U16 0   /* 0 -> NaN, else value * depth_scale */
#define DVO_HIP_DEPTH_F32 1   /* metres * depth_scale, NaN = hole */
/* the device counterpart of dvo_hip_frame_create_f32 (both planes tight): asynchronous on the build stream like
 * dvo_hip_frame_create_raw_device; the planes must stay valid until the frame's first use has been waited for */
int dvo_hip_frame_create_f32_device(dvo_hip_context* ctx, int width, int height, const float K[4], const void* intensity_dev,
                                    const void* depth_dev, int levels, dvo_hip_frame** out);
int dvo_hip_frames_update_f32_device_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                           const void* const* intensity_dev, size_t intensity_pitch, const void* const* depth_dev,
                                           size_t depth_pitch, float depth_scale, int role, const dvo_hip_config* cfg, unsigned flags);
int dvo_hip_frames_update_f32_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const float* const* intensity,
                                    size_t intensity_pitch, const float* const* depth, size_t depth_pitch, float depth_scale, int role,
                                    const dvo_hip_config* cfg, unsigned flags);
/* an 8-bit image plane (DVO_HIP_PIXEL_GREY8 or a colour format) + a float depth plane: a ROS "bgr8" + "32FC1" pair */
int dvo_hip_frames_update_colour_f32depth_device_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                                       const void* const* colour_dev, int pixel_format, size_t colour_pitch,
                                                       const void* const* depth_dev, size_t depth_pitch, float depth_scale, int role,
                                                       const dvo_hip_config* cfg, unsigned flags);
int dvo_hip_frames_update_colour_f32depth_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames,
                                                const void* const* colour, int pixel_format, size_t colour_pitch,
                                                const float* const* depth, size_t depth_pitch, float depth_scale, int role,
                                                const dvo_hip_config* cfg, unsigned flags);
/* carries out every recorded ingest now; returns the first failure */
int dvo_hip_flush_deferred(dvo_hip_context* ctx);
int dvo_hip_upload_wait(dvo_hip_context* ctx);
/* pinned (page-locked) host memory for raw planes: decoders / camera drivers write here, uploads from it are asynchronous */
int dvo_hip_host_alloc(dvo_hip_context* ctx, size_t bytes, void** out);
void dvo_hip_host_free(dvo_hip_context* ctx, void* p);
/* Build the role planes of n frames ahead of time, asynchronously: role CURRENT = the sampling planes of
 * RgbdImage::buildAccelerationStructure (dvo_core/src/core/rgbd_image.cpp:534-543), role REFERENCE = the point selection of
 * PointSelection::select for cfg's thresholds (dvo_core/src/core/point_selection.cpp:89-152), levels cfg->last_level ..
 * cfg->first_level.  This is what the reference's LocalTracker does with a new image BEFORE handing it to its trackers
 * (dvo_slam/src/local_tracker.cpp:159-170).  Optional: dvo_hip_match* builds whatever is missing.
 * Role REFERENCE with a NEGATIVE threshold in cfg is a speculative preparation, for a caller that does not know the tracker the
 * frame will meet: the selection thresholds of the context's last match are used, and frames that already hold a selection (for
 * whatever thresholds) are left alone.
 * Frame construction (create / update / prepare) runs on a stream of its own, concurrently with an alignment that was
 * started afterwards on other frames -- build the next batch, then align the current one, and the two overlap.  A frame
 * must not be updated while a match that uses it is in progress (matches are blocking calls, so this only concerns other
 * host threads). */
int dvo_hip_frames_prepare(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, int role, const dvo_hip_config* cfg);
void dvo_hip_frame_destroy(dvo_hip_context* ctx, dvo_hip_frame* frame);
int dvo_hip_frame_info(const dvo_hip_frame* frame, int level, int* width, int* height, float K[4]);
/* where the tight float planes I / Z of one level lie in device memory (width * height floats each; either pointer may be NULL): what
 * the aliasing rules of the float, lens and depth-rig ingests speak of.  They hold the frame's pixels only where the frame keeps its
 * raw copy in them (a frame built from float planes); the engine writes them on the build stream.  A diagnostic aid for tests and tools
 * that probe those rules, not a data path: the planes stay the engine's, and their layout may change with it. */
int dvo_hip_frame_device_planes(const dvo_hip_frame* frame, int level, void** intensity_dev, void** depth_dev);
/* host mirror of one plane of one level (RgbdImage public fields, rgbd_image.h:161-179):
 * plane 0=intensity 1=depth 2=intensity_dx 3=intensity_dy 4=depth_dx 5=depth_dy */
int dvo_hip_frame_download_plane(dvo_hip_context* ctx, dvo_hip_frame* frame, int level, int plane, float* out);
/* PointSelection::select (dvo_core/src/core/point_selection.cpp:89-152): number of reference
 * pixels that pass ValidPointAndGradientThresholdPredicate (point_selection.h:49-67) and the frame's
 * caller selection (dvo_hip_frames_set_selection).  Builds and caches the reference-side packed
 * plane of that level; optional w*h uint8 mask. */
int dvo_hip_frame_select(dvo_hip_context* ctx, dvo_hip_frame* frame, int level,
                         float intensity_threshold, float depth_threshold, int* n_selected, uint8_t* mask_or_null);

/* ---- caller selection of reference points (an extension over the reference's PointSelectionPredicate,
 * dvo_core/include/dvo/core/point_selection.h:32-36, point_selection.cpp:119-152) ----------------------------------------------
 * A frame can carry a CALLER SELECTION: an optional level-0 mask (uint8, mask_pitch bytes per row, 0 = tight) and an optional depth
 * range [min_depth, max_depth] in metres (0 and +INFINITY = off: a range is on when min_depth > 0 or max_depth is finite).  At level l,
 * pixel (x, y) of a frame in the REFERENCE role is selected iff
 *   1. the threshold predicate of the match holds (ValidPointAndGradientThresholdPredicate, unchanged),
 *   2. mask0[(y << l) * mask_pitch + (x << l)] != 0 -- the level-0 pixel whose depth the coarse pixel carries (the depth pyramid
 *      subsamples, rgbd_image.cpp:128-140, 169); no mask pyramid is stored,
 *   3. min_depth <= Z_l(x, y) <= max_depth (when the range is on).
 * The per-level count (LevelStats::ValidPixels -- the reference's selected-point count --, dvo_hip_frame_select's count and mask)
 * counts exactly these pixels.  Under option
 * "ref_order" the Q3 edit (an odd selection loses its last selected pixel) applies after the caller selection.  The current role of the
 * frame is untouched: a selection restricts only which reference points enter an alignment.
 * The selection persists across re-ingests of the frame's pixels (like the intrinsics) until it is replaced or cleared.  Setting,
 * replacing or clearing one invalidates the frame's reference-role selection at every level -- also one a speculative
 * dvo_hip_frames_prepare made -- so that the next use rebuilds it; a frame ingested into the reference role without a copy of its raw
 * planes (DVO_HIP_INGEST_NO_RAW_COPY) cannot be rebuilt: set its selection BEFORE that ingest.
 * The mask is copied into memory the frame owns when it is set: a host mask (masks_on_device 0) may be reused as soon as the call returns
 * (the call waits for the context's pending frame builds); a device mask follows the stream contract of
 * dvo_hip_frames_update_raw_device (the copy runs asynchronously on the context's build stream: keep the plane unchanged until a later
 * call that uses the frames has returned).  masks may be NULL, and so may any entry (that frame: no mask).
 * Cost: one pass (k_apply_selection) behind every build of a plane R of a frame that carries a selection -- ~9 B per level-0 pixel, a
 * third more for levels 1-3; nothing for frames without one. */
int dvo_hip_frames_set_selection(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const uint8_t* const* masks,
                                 size_t mask_pitch, int masks_on_device, float min_depth, float max_depth);
int dvo_hip_frames_clear_selection(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames);
/* Explicit selection of one level, for an arbitrary predicate evaluated by the caller: `accepted` (host memory, w x h bytes of that
 * level) is the exact accepted set.  The reference-role plane selects Z where accepted != 0, and the count is the number of non-zero
 * entries -- what the reference counts, points with a NaN depth included; the sweeps reject those as they reject any NaN depth.  It
 * replaces the threshold predicate and the caller selection at that level, whatever thresholds a match asks for, until the frame's
 * pixels change, its caller selection is set or cleared, dvo_hip_frame_select asks for a selection of that level, or the set is dropped
 * (accepted = NULL: the level selects by the thresholds of its next use again; nothing happens where the level holds no explicit set).  Under "ref_order"
 * the Q3 edit then drops the last selected pixel of FINITE depth where the reference may drop a NaN-depth point. */
int dvo_hip_frame_set_level_selection(dvo_hip_context* ctx, dvo_hip_frame* frame, int level, const uint8_t* accepted);

/* ---- lens distortion: raw camera frames, rectified on the device at ingest (an extension: the reference's nodes subscribe to
 * image_rect topics, dvo_ros/src/camera_base.cpp:30-31, behind a CPU image_proc stage) -------------------------------------------
 * A frame can carry a LENS: the intrinsics K_raw = {fx, fy, ox, oy} of the raw camera image and the coefficients
 * D = {k1, k2, p1, p2, k3, k4, k5, k6} of OpenCV's / ROS' "plumb_bob" (k4 = k5 = k6 = 0) or "rational_polynomial" model; zeros switch
 * terms off.  Every later dvo_hip_frames_update_* / dvo_hip_frame_update_* of such a frame takes its planes as RAW camera planes and
 * rectifies them first, before anything else happens to them: the rectified pixel (u, v) of the frame -- whose own K stays the pinhole
 * model every alignment uses -- is looked up at
 *   x = (u - ox) / fx,  y = (v - oy) / fy,  r2 = x x + y y,  radial = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
 *   sx = fx_raw (x radial + 2 p1 x y + p2 (r2 + 2 x^2)) + ox_raw,   sy = fy_raw (y radial + p1 (r2 + 2 y^2) + 2 p2 x y) + oy_raw
 * (closed form, float32, operation order fixed in dvo_slam_amd/csrc/lens.h; D = 0 with K_raw = K maps every pixel exactly onto itself).
 * The pixel is valid iff 0 <= sx <= w - 1 and 0 <= sy <= h - 1.  A valid pixel's intensity is the float bilinear blend of the four
 * source taps (an 8-bit colour tap converted to grey first, the result NOT rounded back to 8 bits: a float intensity taken as is,
 * like DVO_HIP_PIXEL_F32); its depth is the converted depth (u16: 0 -> NaN, else value * depth_scale; float: value * depth_scale) of the
 * NEAREST source pixel (int(sx + 0.5), int(sy + 0.5)) -- never a blend, so that no surface is invented across a depth edge -- or, with
 * rectify_depth = 0, of pixel (u, v) itself (depth that is rendered, or rectified already).  An invalid pixel has I = 0 and Z = NaN
 * (also with rectify_depth = 0): it is selected by no reference and matched by no current frame.
 *   ownership    the lens belongs to the FRAME, like the caller selection: it persists across re-ingests until it is replaced or
 *                cleared, and it is no part of the frame's camera -- frames with and without a lens, and with different lenses, align
 *                with each other in one dvo_hip_match_batch as long as they share K.
 *   scope        every dvo_hip_frames_update_* / dvo_hip_frame_update_* entry point, every format, host or device planes, role-aware or
 *                plain, DVO_HIP_INGEST_DEFER and DVO_HIP_INGEST_NO_RAW_COPY included.  dvo_hip_frame_create_* ingests its planes as
 *                they are: there is no frame yet that could carry a lens (create, set the lens, update).
 *   pending      setting or clearing a lens first carries out every recorded ingest (DVO_HIP_INGEST_DEFER), so a recorded ingest runs
 *                with the lens its frames carried when it was recorded.
 *   batches      the frames of ONE ingest call carry bytewise equal lenses (rectify_depth compared as 0 / 1, reserved ignored), or none:
 *                anything else is DVO_HIP_ERR_INVALID and leaves every frame as it was.  So does setting a NULL lens, a non-finite
 *                value, or fx_raw <= 0 or fy_raw <= 0.
 *   aliasing     the pass writes the frame's own float planes of level 0 while it gathers taps from the caller's planes, so a frame that
 *                carries a lens cannot be ingested from planes that overlap its own level-0 planes I / Z (the in-place float ingest of
 *                a lens-less frame): DVO_HIP_ERR_INVALID, every frame left as it was.  Planes that overlap ANOTHER frame's level-0 planes
 *                of the same call are not checked and must not be passed.
 *   raw copy     after a lens ingest the frame is in the state of a frame WITHOUT a lens that was fed the rectified float pair through
 *                dvo_hip_frames_update_f32* with depth_scale 1, bit for bit: its raw copy is the rectified float planes I / Z of
 *                level 0, and a later role, other thresholds, dvo_hip_frame_select, dvo_hip_frames_prepare,
 *                dvo_hip_frame_download_plane, DVO_HIP_INGEST_NO_RAW_COPY and the caller selection work as there.  The selection mask
 *                is in rectified coordinates.
 *   counters     "lens_ingests" counts the frames rectified.  The ingest behind the pass is a float ingest and is counted as one:
 *                "f32_ingests" counts such a frame (whatever its source formats), "strip_ingests" counts it where the strip kernel
 *                takes float planes (even widths), "colour_ingests" does not count it.
 *   cost         one pass (k_rectify, rectify.hip) at the head of the ingest, on the build stream: the map is computed per pixel in
 *                registers (no table), the pass reads the caller's planes and writes 8 B per pixel into the frame's own level-0 planes,
 *                which the float ingest then reads in place; no staging memory.  Frames without a lens take the path they always
 *                took: nothing is launched or allocated for them (profiles/lens_ingest.md). */
typedef struct {
  float K_raw[4];        /* fx, fy, ox, oy of the raw camera image */
  float D[8];            /* k1 k2 p1 p2 k3 k4 k5 k6 */
  int32_t rectify_depth; /* 0: only the image plane is rectified, the depth plane is taken pixel for pixel */
  int32_t reserved;      /* 0 */
} dvo_hip_lens;
int dvo_hip_frames_set_lens(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const dvo_hip_lens* lens);
int dvo_hip_frames_clear_lens(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames);

/* ---- depth rig: raw depth from a second sensor, registered into the colour camera on the device at ingest (an extension: the
 * reference's nodes subscribe to camera/depth_registered/image_rect_raw, dvo_ros/src/camera_base.cpp:30-33, behind a CPU
 * depth_image_proc/register stage) ----------------------------------------------------------------------------------------------
 * A frame can carry a DEPTH RIG: the intrinsics K_depth = {fx_d, fy_d, ox_d, oy_d} of the depth sensor's image (same width x height as
 * the frame) and T = [R | t], the row-major 3 x 4 transform from depth-sensor coordinates to colour-camera coordinates in metres.
 * Every later dvo_hip_frames_update_* / dvo_hip_frame_update_* of such a frame takes its DEPTH plane as the depth sensor's own image
 * and registers it first, before anything else happens: for every source pixel (u, v) of converted depth z (u16: 0 -> NaN, else
 * value * depth_scale; float: value * depth_scale) that is finite and > 0,
 *   X = (u - ox_d) / fx_d * z,  Y = (v - oy_d) / fy_d * z,  P' = R (X, Y, z) + t;   skipped unless P'.z is finite and > 0
 *   u' = fx P'.x / P'.z + ox,   v' = fy P'.y / P'.z + oy  (the frame's own K);      skipped unless -0.5 <= u' < w - 0.5, -0.5 <= v' < h - 0.5
 *   Z[int(floor(v' + 0.5))][int(floor(u' + 0.5))] = min(that element, P'.z)
 * into a plane that starts as NaN everywhere (float32, operation order fixed in dvo_slam_amd/csrc/depth_rig.h; the result does not
 * depend on the order of the pixels).  These are the semantics of ROS' depth_image_proc/register WITHOUT hole filling: a nearest-pixel
 * forward scatter, the nearest surface wins, target pixels that nothing lands on stay holes (NaN).  R is not checked for
 * orthonormality.  The image plane is taken as it comes.
 *   ownership    the rig belongs to the FRAME, like the lens and the caller selection: it persists across re-ingests until it is
 *                replaced or cleared, and it is no part of the frame's camera -- frames with and without a rig align with each other
 *                in one dvo_hip_match_batch as long as they share K.
 *   scope        every dvo_hip_frames_update_* / dvo_hip_frame_update_* entry point in the format combinations it accepts today, host
 *                or device planes, role-aware or plain, DVO_HIP_INGEST_DEFER and DVO_HIP_INGEST_NO_RAW_COPY included.
 *                dvo_hip_frame_create_* ingests its planes as they are: create, set the rig, then update.
 *   pending      setting or clearing a rig first carries out every recorded ingest (DVO_HIP_INGEST_DEFER), so a recorded ingest runs
 *                with the rig its frames carried when it was recorded.
 *   batches      the frames of ONE ingest call carry bytewise equal rigs, or none: anything else is DVO_HIP_ERR_INVALID and leaves
 *                every frame as it was.  So does setting a NULL rig, a non-finite value, fx_d <= 0 or fy_d <= 0, or a non-zero reserved.
 *   lens         registration projects into the frame's rectified pinhole K, so its output is rectified depth already: a frame carries a
 *                rig and a lens only if the lens has rectify_depth = 0.  Setting a rig on a frame whose lens has rectify_depth != 0, or
 *                such a lens on a frame with a rig, is DVO_HIP_ERR_INVALID and changes nothing.  The order is: register, then the
 *                lens pass on the image plane; pixels the lens leaves invalid still end with Z = NaN.
 *   aliasing     the pass fills and scatters into the frame's own float plane Z of level 0, so a depth plane or an image plane that
 *                overlaps that plane is DVO_HIP_ERR_INVALID, every frame left as it was.  Planes that overlap ANOTHER frame's level-0 planes of the same call
 *                are not checked and must not be passed.
 *   raw copy     after a rig ingest the frame is in the state of a frame WITHOUT a rig that was fed the same image plane and the
 *                registered plane through the float-depth entry point of that image format (dvo_hip_frames_update_f32* /
 *                dvo_hip_frames_update_colour_f32depth*, depth_scale 1), bit for bit: its raw copy is its float planes I / Z of level
 *                0, and a later role, dvo_hip_frame_select, dvo_hip_frame_download_plane, DVO_HIP_INGEST_NO_RAW_COPY and the caller
 *                selection work as there.
 *   counters     "depth_registrations" counts the frames registered.  The ingest behind the pass is a float-depth ingest and is
 *                counted as one: "f32_ingests" counts such a frame, "strip_ingests" and "colour_ingests" count as for that ingest.
 *   cost         two launches (k_depth_fill, k_depth_register, depth_register.hip) at the head of the ingest, on the build stream, ahead
 *                of the lens pass: 4 B per pixel filled, 2-4 B read and one 4-byte atomic minimum per valid pixel, no staging memory.
 *                Device times of the two kernels are NOT MEASURED yet (profiles/depth_registration.md says how to take them).
 *                Frames without a rig take the path they always took: nothing is launched or allocated for them (DESIGN.md section
 *                3, profiles/depth_registration.md). */
typedef struct {
  float K_depth[4];    /* fx, fy, ox, oy of the depth sensor's image (same width x height as the frame) */
  float T[12];         /* row-major 3x4 [R | t]: depth-sensor coordinates -> colour-camera coordinates, metres */
  int32_t reserved[2]; /* 0 */
} dvo_hip_depth_rig;
int dvo_hip_frames_set_depth_rig(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const dvo_hip_depth_rig* rig);
int dvo_hip_frames_clear_depth_rig(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames);

/* ---- depth filter: raw depth conditioned on the device at ingest -- flying pixels and hole borders rejected, axial noise smoothed (an
 * extension: the reference has no such pass, SurfacePyramid::convertRawDepthImage only scales and maps 0 to NaN; users of
 * camera/depth/image_raw run cv::bilateralFilter, PCL's fast bilateral filter or an edge erosion on the CPU) ------------------------
 * A frame can carry a DEPTH FILTER.  Every later dvo_hip_frames_update_* / dvo_hip_frame_update_* of such a frame conditions its depth
 * plane LAST of the ingest's pre-passes (sensor format -> depth rig -> lens -> depth filter), so in the frame's own raster.  With z_c
 * the converted depth of a pixel (u16: 0 -> NaN, else value * depth_scale; float: value * depth_scale; behind a rig or a lens: what that
 * pass left), valid iff finite and > 0, every output pixel is a function of the INPUT window alone:
 *   hole     an invalid input gives the canonical quiet NaN 0x7FC00000;
 *   edge     a valid pixel is rejected (that NaN) if any in-image valid tap within Chebyshev distance edge_radius has
 *            |z_n - z_c| > edge_abs + edge_rel * z_c: both sides of a step go, each by its own threshold, and the mixed pixels between;
 *   erosion  a valid pixel is rejected if any in-image tap within Chebyshev distance hole_radius is invalid (the image border erodes
 *            nothing);
 *   smooth   a kept pixel becomes z_c + sum(w d) / sum(w) over the valid in-image taps of the (2 radius + 1)^2 window, row-major,
 *            d = z_n - z_c, t = |d| * inv, inv = 64 / (gate * (noise_a + noise_b * (z_c * z_c))), taps with t >= 64 left out,
 *            w = ws[dy][dx] * wr[int(t)], ws = exp(-(dx^2 + dy^2) / (2 sigma_space^2)), wr[b] = exp(-((b + 0.5) gate / 64)^2 / 2), both
 *            tables computed on the host in double and rounded to float once.  radius 0: a kept pixel keeps its bits.
 * float32 throughout, the operation order fixed in dvo_slam_amd/csrc/depth_filter.h, whose host build the device equals bit for bit.
 *   ownership    the filter belongs to the FRAME, like the depth rig, the lens and the caller selection: it persists across re-ingests
 *                until it is replaced or cleared, and it is no part of the frame's camera -- frames with and without a filter align
 *                with each other in one dvo_hip_match_batch as long as they share K.
 *   scope        every dvo_hip_frames_update_* / dvo_hip_frame_update_* entry point in the format combinations it accepts today, host
 *                or device planes, role-aware or plain, DVO_HIP_INGEST_DEFER and DVO_HIP_INGEST_NO_RAW_COPY included.
 *                dvo_hip_frame_create_* ingests its planes as they are: create, set the filter, then update.
 *                dvo_hip_map_render_frames refuses a frame with a filter, as it refuses one with a lens or a rig.
 *   pending      setting or clearing a filter first carries out every recorded ingest (DVO_HIP_INGEST_DEFER), so a recorded ingest
 *                runs with the filter its frames carried when it was recorded.
 *   batches      the frames of ONE ingest call carry bytewise equal filters, or none: anything else is DVO_HIP_ERR_INVALID and leaves
 *                every frame as it was.
 *   invalid      DVO_HIP_ERR_INVALID, nothing changed, for a NULL filter, a non-finite field, radius outside 0..3, edge_radius or
 *                hole_radius outside 0..2, sigma_space <= 0 with radius > 0, gate <= 0, a negative noise_* or edge_* field, noise_a
 *                and noise_b both 0 (sigma(z) not positive), or a non-zero reserved.
 *   aliasing     the pass writes the frame's filter plane (one more float plane of width x height, allocated when the filter is set
 *                and freed when it is cleared: a steady-state ingest allocates nothing) and the ingest behind it the frame's level-0
 *                planes: a caller plane, image or depth, that overlaps the frame's float planes I / Z of level 0 or its filter plane
 *                is DVO_HIP_ERR_INVALID, every frame left as it was.  Planes that overlap ANOTHER frame's planes of the same call are
 *                not checked and must not be passed.
 *   raw copy     after the ingest the frame is in the state of a frame WITHOUT a filter (same lens, same rig) that was fed the same
 *                image and the filtered float plane through the float-depth entry point of that image format, depth_scale 1, bit
 *                for bit: its raw copy is its float planes I / Z of level 0, and a later role, dvo_hip_frame_select,
 *                dvo_hip_frame_download_plane, DVO_HIP_INGEST_NO_RAW_COPY and the caller selection work as there.
 *   counters     "depth_filter_ingests" counts the frames filtered.  The ingest behind the pass is a float-depth ingest and is
 *                counted as one: "f32_ingests" counts such a frame, the other ingest counters count as for that ingest.
 *   cost         one launch (k_depth_filter, depth_filter.hip) behind the other pre-passes, on the build stream: 2-4 B read and 4 B
 *                written per pixel, the window staged in LDS (profiles/depth_filter.md).  Frames without a filter take the path they
 *                always took: nothing is launched or allocated for them.
 * dvo_hip_depth_filter_default() returns radius 2, sigma_space 1.5, noise_a 0.0012, noise_b 0.0019, gate 3, edge_radius 1, edge_abs
 * 0.01, edge_rel 0.03, hole_radius 0: values recalled from published Kinect axial-noise fits, NOT verified here. */
typedef struct {
  int32_t radius;        /* 0..3: half-size of the smoothing window; 0 = no smoothing */
  float sigma_space;     /* pixels; > 0 when radius > 0 */
  float noise_a;         /* sigma(z) = noise_a + noise_b * (z * z), metres */
  float noise_b;
  float gate;            /* > 0: taps further than gate * sigma(z_c) from z_c take no part in the mean */
  int32_t edge_radius;   /* 0..2; 0 = no edge rejection */
  float edge_abs;        /* tau(z) = edge_abs + edge_rel * z, metres */
  float edge_rel;
  int32_t hole_radius;   /* 0..2; 0 = no hole-border erosion */
  int32_t reserved[2];   /* 0 */
} dvo_hip_depth_filter;
dvo_hip_depth_filter dvo_hip_depth_filter_default(void);
int dvo_hip_frames_set_depth_filter(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const dvo_hip_depth_filter* filter);
int dvo_hip_frames_clear_depth_filter(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames);

/* ---- keyframe map: world point clouds and a voxel-grid map of n keyframes, on the device ---------------------------------------------
 * Stands in for the reference's map building: AsyncPointCloudBuilder::BuildJob::build
 * (dvo_core/src/visualization/async_point_cloud_builder.cpp:61-110: pose.cast<float>() * image.pointcloud plus intensity, every pixel of a
 * keyframe), PointCloudAggregator::build (dvo_core/src/visualization/point_cloud_aggregator.cpp:74-109: the clouds of up to ~50 keyframes
 * concatenated and downsampled with a 1 cm voxel grid) and its caller dvo_ros/src/visualization/ros_camera_trajectory_visualizer.cpp.
 * The keyframes already lie in device memory: fusing them reads 8 B per pixel, and only the finished map crosses to the host.
 *   world point  pixel (u, v) of level `level` (intrinsics K of that level), depth z, intensity I, pose T = [R | t] (camera -> world, the
 *                row-major 4 x 4 double of dvo_hip_result::transformation, converted to float once per frame):
 *                X = (u - ox) / fx * z, Y = (v - oy) / fy * z (the (u - ox) / fx template of the RgbdCamera constructor,
 *                dvo_core/src/core/rgbd_image.cpp:186-204, times z in RgbdCamera::buildPointCloud, rgbd_image.cpp:245-262), P = R (X, Y, z) + t.  USABLE iff z is finite and > 0, min_depth <= z <= max_depth (0 and +INFINITY: the range is off,
 *                as in dvo_hip_frames_set_selection) and P is finite.  I and z are exactly what dvo_hip_frame_download_plane returns for
 *                planes 0 and 1 of that level -- of a frame with a lens or a depth rig: the rectified / registered planes.
 *   voxel        leaf > 0 (float).  Per axis i = floor(P / leaf), which must lie in -2^20 .. 2^20 - 1 (else the point is OUT OF RANGE:
 *                counted, skipped); the offset inside the voxel is truncated to a 1024th of the leaf, the intensity rounded to a 16th
 *                and clamped into [0, 4095 / 16].  key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20).
 *   sums         a voxel holds its point count n and the integer sums of the quantised offsets and intensities (uint32 each).  Up to
 *                2^20 points per voxel no sum can wrap; a voxel with more is reported (over_limit, and by dvo_hip_map_extract), decided
 *                from n alone.  Integer sums do not depend on the order of the additions: the map is the same BIT FOR BIT whatever
 *                order the device visits the pixels in, however the frames are split over calls -- and equal to the host build of
 *                dvo_slam_amd/csrc/cloud_map.h, where the operation order of all of this is fixed.
 *   table        open addressing, capacity a power of two, linear probing with a fixed bound of 128 probes.  A point that finds neither
 *                its voxel nor a free slot within the bound is DROPPED and counted; nothing ever waits or retries.
 *   extraction   per voxel x = (ix + (sx / n + 0.5) / 1024) * leaf in double, rounded to float once (y, z likewise), intensity =
 *                si / n / 16: per axis within leaf / 2048 of the true centroid of the voxel's points, the intensity within 1 / 32.
 *                This is NOT PCL's ApproximateVoxelGrid, whose output depends on the order of insertion and on a 2048-entry hash
 *                history.
 *   streams      every call runs on the context's main stream behind the build-stream work that wrote the frames, and carries out every
 *                recorded ingest first (DVO_HIP_INGEST_DEFER), as a match does.  Calls return when their result is complete.
 *   refusals     a null or foreign frame or map, a level a frame does not have, a null pose or output, min_depth > max_depth or NaN:
 *                DVO_HIP_ERR_INVALID, nothing launched, nothing changed.
 *   updates      the map follows the pose graph without being rebuilt: dvo_hip_map_remove takes a keyframe's points out again,
 *                dvo_hip_map_move re-poses keyframes (a loop closure) in one launch, dvo_hip_map_rehash reclaims the slots they vacated
 *                and resizes the table.  All sums are integers filled by integer adds, so subtracting what a keyframe added restores
 *                the table's words BIT FOR BIT: after a removal the extraction and every render equal those of a map that never held
 *                the keyframe (dvo_slam_amd/csrc/cloud_map.h, Removal and Rehash).
 *   cost         profiles/keyframe_map.md, profiles/keyframe_map_update.md. */
typedef struct dvo_hip_map dvo_hip_map;
/* (a struct tag beside the function of the same name, like stat(2): `struct dvo_hip_map_stats s; dvo_hip_map_stats(ctx, map, &s);`) */
struct dvo_hip_map_stats {
  uint64_t occupied;      /* slots that hold a key: the voxels in the table, vacant ones included */
  uint64_t points;        /* points the table holds: those it took less those removed */
  uint64_t dropped;       /* usable points in range that found no slot within the probe bound */
  uint64_t out_of_range;  /* usable points beyond +-2^20 voxels on some axis (of the frames the map holds: a removal takes its own back) */
  uint64_t unusable;      /* pixels without a usable point (likewise) */
  uint64_t over_limit;    /* voxels that hold more than 2^20 points */
  uint64_t capacity;      /* slots */
  uint64_t updates;       /* slot updates issued, additions and subtractions: runs of neighbouring pixels that share a voxel go to the table as one */
  uint64_t vacant;        /* slots whose points have all been removed: they keep their key until dvo_hip_map_rehash (occupied - vacant voxels are live) */
  uint64_t removed;       /* points subtracted by dvo_hip_map_remove / dvo_hip_map_move */
  uint64_t unmatched;     /* points a removal did not find in the table: nothing was subtracted for them */
  uint64_t reserved[5];   /* 0 */
};
/* capacity_slots is rounded up to a power of two, at least 64 (32 bytes per slot); a leaf that is not finite and > 0 is
 * DVO_HIP_ERR_INVALID.  Keep the table at most a quarter full (dvo_hip_map_stats): probe sequences then stay far below the bound.
 * A map belongs to its context and is destroyed before it. */
int dvo_hip_map_create(dvo_hip_context* ctx, float leaf, size_t capacity_slots, dvo_hip_map** out);
void dvo_hip_map_destroy(dvo_hip_context* ctx, dvo_hip_map* map);
/* every slot empty, every sum and statistic zero (after a pose-graph optimisation there is no need to: dvo_hip_map_move) */
int dvo_hip_map_clear(dvo_hip_context* ctx, dvo_hip_map* map);
/* PointCloudAggregator::build's concatenate + filter for n frames (point_cloud_aggregator.cpp:95-106) in one launch: every usable point
 * of level `level` of every frame, under poses[16 * i ..], into the map.  Frames of different sizes and cameras may share a call.
 * DVO_HIP_ERR_CAPACITY if the call dropped a point -- the map keeps what it took, the statistics say how many -- else DVO_HIP_OK.
 * To answer that, the call WAITS for the main stream (one read-back of the map's counters behind the launch; dvo_hip_map_stats and
 * dvo_hip_map_extract wait likewise): it drains whatever was queued before it, so it does not belong between pipelined matches. */
int dvo_hip_map_insert(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, const double* poses /* n x 16 */,
                       int level, float min_depth, float max_depth);
/* The inverse of dvo_hip_map_insert: every usable point of level `level` of every frame, under poses[16 * i ..], out of the map again.
 * The caller passes what it passed to the insertion -- the same frame CONTENT (a frame re-ingested since is another frame), level, pose and
 * depth range: every point then finds its voxel and is subtracted from it, exactly (integer sums), and the map is, bit for bit in what
 * dvo_hip_map_extract and dvo_hip_map_render give, the map that never held the frames.  A voxel that loses all its points becomes VACANT:
 * no longer extracted or rendered, but its slot keeps the key (dvo_hip_map_stats: vacant) until dvo_hip_map_rehash.  A point that does
 * not find its voxel is UNMATCHED: counted, nothing subtracted; a call that leaves any returns DVO_HIP_ERR_INVALID with the count in
 * dvo_hip_last_error -- the map keeps what the call did, the statistics say how many.  Streams, waiting and refusals as for
 * dvo_hip_map_insert, and one more: a map that has DROPPED points since its last clear or rehash does not know what it holds of a
 * frame and refuses (DVO_HIP_ERR_INVALID, nothing launched, nothing changed). */
int dvo_hip_map_remove(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, const double* poses /* n x 16 */,
                       int level, float min_depth, float max_depth);
/* After a pose-graph optimisation: the frames leave the map under poses_old and enter it under poses_new, in ONE launch over 2 n
 * entries -- bit for bit dvo_hip_map_remove(poses_old) followed by dvo_hip_map_insert(poses_new).  A frame whose two poses are equal
 * once converted to float is left out of the launch (a call in which every frame is returns DVO_HIP_OK and launches nothing).
 * DVO_HIP_ERR_CAPACITY if the call dropped a point (its insertions can), else DVO_HIP_ERR_INVALID if it left unmatched points, else
 * DVO_HIP_OK; refusals as for dvo_hip_map_remove. */
int dvo_hip_map_move(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, const double* poses_old /* n x 16 */,
                     const double* poses_new /* n x 16 */, int level, float min_depth, float max_depth);
/* Rebuilds the table with capacity_slots slots (a power of two, 64 .. 2^32; 0: as many as it has; anything else is
 * DVO_HIP_ERR_INVALID): every live voxel moves with its sums unchanged, vacant slots are reclaimed.  Afterwards occupied = the live
 * voxels, vacant = 0, dropped = 0 (a map that dropped points takes removals again; the dropped points themselves stay lost), points
 * and the other statistics are as before.  DVO_HIP_ERR_CAPACITY if a voxel finds no slot in the new table within the probe bound: the
 * map is then unchanged.  A second table exists during the call: the old one is freed on success, the new one on failure.  Runs on the
 * main stream and waits for it, like dvo_hip_map_insert. */
int dvo_hip_map_rehash(dvo_hip_context* ctx, dvo_hip_map* map, size_t capacity_slots);
int dvo_hip_map_stats(dvo_hip_context* ctx, dvo_hip_map* map, struct dvo_hip_map_stats* out);
/* The downsampled cloud (what point_cloud_aggregator.cpp:105-108 returns): one record {x, y, z, intensity} per voxel into xyzi, its point
 * count and key into counts / keys where those are not NULL; host arrays, or device arrays (xyzi 16-byte aligned) with out_on_device.
 * The ORDER is unspecified and may differ from call to call: sort by key to compare.  *n_points = records written (<= max_points).
 * DVO_HIP_ERR_CAPACITY if the map holds more voxels than max_points -- the first max_points found are written, nothing beyond -- or if
 * a voxel is over the 2^20 limit (everything is written; that voxel's record is unreliable). */
int dvo_hip_map_extract(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_points, float* xyzi, uint32_t* counts_or_null,
                        uint64_t* keys_or_null, int out_on_device, size_t* n_points);
/* AsyncPointCloudBuilder::BuildJob::build for n frames (async_point_cloud_builder.cpp:61-110): the ORGANISED cloud, w x h records
 * {P.x, P.y, P.z, I} per frame in raster order into out[i] (host, or device and 16-byte aligned with out_on_device); an unusable pixel
 * has a quiet NaN (0x7FC00000) in x, y and z and its I as it is. */
int dvo_hip_frames_world_points(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const double* poses /* n x 16 */,
                                int level, float min_depth, float max_depth, float* const* out, int out_on_device);

/* ---- views of the keyframe map: model images to track against ---------------------------------------------------------------------------
 * Not in the reference, which only draws its map in a PCL window.  The map is projected into a pinhole camera at a pose, the nearest
 * surface per pixel, and comes back as tight float planes I (0..255) and Z (metres, NaN = hole) -- the planes the float ingest above
 * takes ("a filtered, rendered or predicted depth image").  With them a caller tracks a frame against the fused model instead of one
 * noisy keyframe (with the parameters "tracking" below names, not the defaults), checks a loop closure against the model, tests a new depth image for outliers, or looks at the map from any pose
 * without hauling a cloud to the host.
 *   view         width, height, K = {fx, fy, ox, oy} and a pose T = [R | t] (camera -> world, the row-major 4 x 4 double of
 *                dvo_hip_result::transformation, as everywhere in the map API); its inverse (R^T, -R^T t) is formed once per view in
 *                double and rounded to float once.
 *   source       every voxel of the map with min_points <= n <= 2^20 points; its record {x, y, z, I} is exactly what
 *                dvo_hip_map_extract reports.  p = R^T P - R^T t; the voxel is skipped unless p.z is finite and > 0 and lies within
 *                [min_depth, max_depth] (0 and +INFINITY: the range is off).  u' = fx p.x / p.z + ox, v' = fy p.y / p.z + oy.
 *   footprint    a flat square of the voxel's size times `splat`: hx = splat * 0.5 * leaf * fx / p.z (hy with fy); the voxel covers
 *                the pixel centres u in [ceil(u' - hx), floor(u' + hx)], v likewise; an axis on which that range is empty takes the one
 *                nearest pixel floor(u' + 0.5).  Each range is then cut to at most max_splat pixels centred on the nearest pixel and
 *                clipped to the image.  splat is a float in (0, 4], max_splat an odd integer in 1 .. 15.
 *   z-buffer     per pixel the minimum of uint64(bits(p.z)) << 32 | bits(max(I, 0)) over the voxels that cover it: the nearest voxel,
 *                and of voxels at the same depth the one with the LOWER intensity.  A minimum over integers: the planes are the same BIT
 *                FOR BIT whatever order the device visits the voxels in and whatever order the map was filled in -- and equal to the
 *                host build of dvo_slam_amd/csrc/map_render.h, where the operation order of all of this is fixed.
 *   planes       a pixel no voxel covers is a hole: Z = NaN (0x7FC00000), I = 0.  Else Z = p.z of the winning voxel and I its intensity.
 *                The depth is constant across a footprint (no surface normal), a foreground silhouette grows by up to splat * leaf / 2,
 *                and nothing fills holes.  With the default splat (2) a fronto-parallel surface whose voxels are all occupied has no
 *                hole as long as 2 hx + 1 <= max_splat, wherever the centroids lie inside their voxels.
 *   tracking     the defaults favour a view without holes, NOT tracking: grown silhouettes put foreground depth on background pixels,
 *                and where near objects stand before a far background that misleads the alignment.  On the project's 128 x 96 scene
 *                (objects at 0.3 m before a background metres away, leaf 0.02; profiles/map_render.md) a frame aligned against the
 *                default view ends 0.054 from the true relative pose (twist, max-abs) where the keyframe itself gives 0.0089 and the
 *                motion is 0.021; with max_splat = 1 the view gives 0.0088, with splat = 1 and min_depth = 0.6 0.0071.  For model
 *                views to track against use max_splat = 1 (one pixel per voxel: needs a leaf of about a pixel or less at the depths
 *                seen) or a splat <= 1 with a depth range that drops the near field.
 *   streams      a render runs on the context's main stream, behind every insert and clear of the map (they run there too), and
 *                carries out every recorded ingest first, as dvo_hip_map_insert does.  dvo_hip_map_render reads nothing but the
 *                table, which only the main stream writes, so unlike an insert it makes no wait on the build stream.  The z-buffers are scratch of the context, grown
 *                on demand and reused.  dvo_hip_map_render to HOST planes returns when they are complete; to DEVICE planes it returns
 *                at once and the planes are ordered on the context's stream (dvo_hip_context_stream).  dvo_hip_map_render_frames makes
 *                the build stream wait for the render and ingests there: the frames are ordered like after any other device ingest.
 *   refusals     DVO_HIP_ERR_INVALID, nothing launched, nothing changed, no counter moved: a null or foreign map, frame, pose or
 *                output; n <= 0; a size that is not positive, above 2^24 on a side or above 2^31 - 1 pixels for the views of one
 *                call; a K that is not finite or has fx or fy <= 0; splat outside (0, 4]; max_splat even or outside 1 .. 15;
 *                min_points of 0; min_depth > max_depth or a NaN bound; a reserved field that is not 0; a device plane that is not
 *                16-byte aligned; for dvo_hip_map_render_frames also DVO_HIP_INGEST_DEFER, frames of differing cameras, and a frame
 *                that carries a lens or a depth rig (the planes are rectified and registered already).
 *   cost         profiles/map_render.md: 8 B per pixel filled, 8 B per slot and 32 B per voxel read, one 8-byte atomic per covered
 *                pixel, 16 B per pixel resolved; per VIEW, so 16 views cost 16 times one.  Counter "map_renders" counts views. */
typedef struct {
  float min_depth, max_depth; /* of p.z; 0 and +INFINITY: off */
  float splat;                /* footprint in voxel sizes, (0, 4] */
  int32_t max_splat;          /* pixels per axis at most: odd, 1 .. 15 */
  uint32_t min_points;        /* voxels with fewer points are not drawn; >= 1 */
  uint32_t reserved[3];       /* 0 */
} dvo_hip_render_params;
/* min_depth 0, max_depth +INFINITY, splat 2, max_splat 7, min_points 1 */
dvo_hip_render_params dvo_hip_render_params_default(void);
/* n_views views of width x height under K, view i at poses[16 * i ..]: plane I into intensity_out[i], Z into depth_out[i], width *
 * height floats each, tight; host arrays, or device arrays (16-byte aligned) with out_on_device.  params NULL: the defaults. */
int dvo_hip_map_render(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float K[4],
                       const double* poses /* n x 16 */, const dvo_hip_render_params* params, float* const* intensity_out,
                       float* const* depth_out, int out_on_device);
/* The same straight into frames: frame i's own level-0 size and K are view i (all frames of a call share a camera, as the ingest
 * demands), and the rendered planes go through the float-depth device ingest -- the code path of dvo_hip_frames_update_f32_device_as_ex
 * with depth_scale 1; role, cfg and DVO_HIP_INGEST_NO_RAW_COPY mean what they mean there, DVO_HIP_INGEST_DEFER is refused.
 * Afterwards a frame is, bit for bit, a frame that was fed the planes dvo_hip_map_render gives for the same view. */
int dvo_hip_map_render_frames(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames,
                              const double* poses /* n x 16 */, const dvo_hip_render_params* params, int role, const dvo_hip_config* cfg,
                              unsigned flags);
/* measurement (scripts/map_render_rate.py): renders the views `reps` times into scratch planes of the context with HIP events around each
 * kernel; ms[0..2] = the medians of k_render_fill, k_map_render and k_render_resolve in milliseconds.  Counts nothing. */
int dvo_hip_time_map_render(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float K[4],
                            const double* poses /* n x 16 */, const dvo_hip_render_params* params, int reps, float ms[3]);

/* ---- frames warped under a pose: the reference's image warps --------------------------------------------------------------------------------
 * RgbdImage::warpIntensity, warpIntensityForward, warpDepthForward and warpDepthForwardAdvanced (dvo_core/include/dvo/core/rgbd_image.h:199-213,
 * dvo_core/src/core/rgbd_image.cpp:545-781, dvo_core/src/core/interpolation.cpp:55-110) for n frames in one launch, on the planes the
 * frames hold on the device.  The INVERSE warp shows one image in another image's raster -- the picture a user of a direct method checks an
 * alignment with, and its difference image.  The FORWARD warp predicts the depth (and intensity) image at a new pose from one frame, without
 * a map: the planes the float ingest above takes ("a filtered, rendered or predicted depth image").  All arithmetic is float32 and stated
 * once in dvo_slam_amd/csrc/frame_warp.h, whose host build the device planes equal BIT FOR BIT; every NaN stored is 0x7FC00000.
 *   transform    the row-major 4 x 4 double of dvo_hip_result::transformation, rounded to float once per item; the linear part is applied
 *                as given (no orthonormality check), each row as ((r0 X + r1 Y) + r2 z) + t.
 *   inverse      (warpIntensity, rgbd_image.cpp:564-597, with Interpolation::bilinearWithDepthBuffer, interpolation.cpp:55-110.)  Item i:
 *                a RASTER frame R (the owner of the reference's reference_pointcloud), a SAMPLED frame S (the reference's `this`) and T,
 *                R's camera -> S's camera, at a level where both have the same size; K_R back-projects, K_S projects.  Per raster pixel
 *                with depth z: p = T (((x - ox) / fx) z, ((y - oy) / fy) z, z); u = (p.x fx) / p.z + ox, v likewise.  I_w = Z_w = NaN where
 *                z is not finite, p.z is not finite or <= 0, or (u, v) is outside 0 <= u < w, 0 <= v < h.  Else Z_w = p.z, and I_w is the
 *                bilinear sample of I_S at (u, v) over the taps whose Z_S is finite and > p.z - occlusion_margin (the reference's 0.05),
 *                renormalised by their weights; NaN when no tap counts, and NaN (Z_w stays) in the last row and column, where a tap
 *                would lie outside.  The optional difference plane is D = I_w - I_R, NaN where I_w is NaN.
 *                dvo_hip_result::transformation is current -> reference: to see the current image in the reference's raster pass its inverse
 *                with R = the reference frame and S = the current one.
 *   forward      (warpIntensityForward rgbd_image.cpp:654-721, warpDepthForward :604-652, warpDepthForwardAdvanced :723-781.)  Item i: a
 *                source frame F and T, F's camera -> the target camera; the target has F's size and K at the level.  A source pixel is
 *                skipped unless z is finite and > 0 and within [min_depth, max_depth] (0 and +INFINITY: off), and p.z is finite and > 0.
 *                DVO_HIP_WARP_NEAREST: the pixel (floor(u), floor(v)) when it lies in the image.  DVO_HIP_WARP_SPLAT: the reference's
 *                footprint (rgbd_image.cpp:734-763), xlen = ceil(zf1 + xf1 (X / z)) + 1 by ylen pixels from (floor(u), floor(v)), clipped
 *                to the image, each length cut to 8.  Every covered pixel takes the unsigned minimum of bits(p.z) << 32 | bits(max(I, 0)),
 *                the z-buffer element of the map views: the nearest surface wins, the intensity is that surface's, and the planes do not
 *                depend on the order of the source pixels.  A pixel nothing covers is a hole: Z = NaN, I = 0.
 *   deviations   the inverse warp refuses points behind the camera (the reference tests only finiteness).  The reference's
 *                warpDepthForward keeps an order-dependent 5 cm hysteresis and stores the UNTRANSFORMED depth, warpIntensityForward lets
 *                the last writer win and returns the source's depth: neither is followed, both modes give p.z of the nearest surface and
 *                its intensity.  rotation() of an Eigen Affine is a decomposition; here the linear part is used.  The Z plane of SPLAT is,
 *                for rigid T and footprints within the cap, exactly the reference's (its `!isfinite(*v) || *v > z` is a minimum).
 *   streams      as dvo_hip_frames_world_points: the launches run on the context's main stream behind the builds of the frames, recorded
 *                (deferred) ingests are carried out first, and the call waits for that stream: host AND device planes are complete on
 *                return (device planes are thereby ordered before anything issued later on any stream of the context).  The forward
 *                warp's z-buffers are the render scratch of the context, filled and resolved on the main stream like a map render's.
 *   refusals     DVO_HIP_ERR_INVALID, nothing launched, no output touched, no counter moved: null or foreign handles, null outputs, a
 *                null transforms; n <= 0; a level the frames do not have; a pair whose sizes differ at the level; a transform that is
 *                not finite; an unknown mode; a margin that is negative or NaN; min_depth > max_depth or a NaN bound; a reserved field
 *                that is not 0; a device plane that is not 16-byte aligned.
 *   cost         profiles/frame_warp.md.  Counter "frame_warps" counts items. */
#define DVO_HIP_WARP_NEAREST 0 /* warpDepthForward / warpIntensityForward: one pixel per source pixel */
#define DVO_HIP_WARP_SPLAT 1   /* warpDepthForwardAdvanced: the reference's footprint, no holes on a surface that comes nearer */
typedef struct {
  int32_t mode;               /* forward: DVO_HIP_WARP_NEAREST or DVO_HIP_WARP_SPLAT; the inverse warp checks it and uses nothing of it */
  float occlusion_margin;     /* inverse: a tap nearer than p.z - margin is left out; >= 0 */
  float min_depth, max_depth; /* forward: of the source depth; 0 and +INFINITY: off */
  uint32_t reserved[4];       /* 0 */
} dvo_hip_warp_params;
/* DVO_HIP_WARP_SPLAT, margin 0.05f, min_depth 0, max_depth +INFINITY */
dvo_hip_warp_params dvo_hip_warp_params_default(void);
/* Item i: raster_frames[i] and sampled_frames[i] under transforms[16 * i ..] (raster camera -> sampled camera) at `level`: I_w into
 * intensity_out[i], Z_w into depth_out[i] and -- where difference_out_or_null is not NULL -- D into difference_out_or_null[i]; w_L * h_L
 * floats each, tight; host arrays, or device arrays (16-byte aligned) with out_on_device.  params NULL: the defaults. */
int dvo_hip_frames_warp_inverse(dvo_hip_context* ctx, int n, dvo_hip_frame* const* raster_frames, dvo_hip_frame* const* sampled_frames,
                                const double* transforms /* n x 16 */, int level, const dvo_hip_warp_params* params_or_null,
                                float* const* intensity_out, float* const* depth_out, float* const* difference_out_or_null, int out_on_device);
/* Item i: frames[i] under transforms[16 * i ..] (its camera -> the target camera) at `level`: the predicted planes I into intensity_out[i]
 * and Z into depth_out[i], as above. */
int dvo_hip_frames_warp_forward(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const double* transforms /* n x 16 */, int level,
                                const dvo_hip_warp_params* params_or_null, float* const* intensity_out, float* const* depth_out,
                                int out_on_device);

/* ---- keyframe covisibility: loop-closure candidates counted on the device ---------------------------------------------------------------------
 * Which keyframes a new keyframe should be validated against.  The reference asks only how far apart the cameras stand:
 * NearestNeighborConstraintSearch::findPossibleConstraints (dvo_slam/src/keyframe_constraint_search.cpp:41-72, called from
 * dvo_slam/src/keyframe_graph.cpp:233 and :456) radius-searches the keyframes' translations and hands every hit to the validator.  This
 * call counts, for many ordered keyframe pairs in ONE launch, how much of one frame's surface the other frame also sees, and downloads
 * nothing but a 32-byte record per pair: a proposal (dvo_slam::CovisibilityConstraintSearch, include/dvo_slam/keyframe_covisibility.h), a
 * ranking of relocalisation candidates, which sub-maps overlap before a dvo_hip_map_merge, which keyframes are redundant.  All arithmetic
 * is float32 and stated once in dvo_slam_amd/csrc/covisibility.h, whose host build the device records EQUAL (every output is an integer).
 *   pair         (a, b, T): a = frames[pair_a[k]], b = frames[pair_b[k]], T = transforms[16 k ..], the row-major 4 x 4 double that carries
 *                a's camera into b's camera, rounded to float once per pair, its linear part applied as given.  a and b are taken at
 *                `level` with their own sizes and intrinsics: the two need not agree in size or camera.  a == b is allowed.
 *   per pixel    of a with depth z and intensity I_a: skipped unless z is finite and > 0 and within [min_depth, max_depth] (0 and
 *                +INFINITY: off); else `valid`.  p = T (((x - ox_a) / fx_a) z, ((y - oy_a) / fy_a) z, z); nothing more unless p.z is
 *                finite and > 0.  u = (p.x fx_b) / p.z + ox_b, v likewise; the NEAREST pixel (floor(u + 0.5), floor(v + 0.5)) -- integer
 *                coordinates are pixel centres -- and nothing more unless it lies in b's image; else `in_view`.  Z_b there not finite:
 *                `unknown`.  Else with tol = depth_tolerance + depth_tolerance_rel p.z and d = Z_b - p.z: d < -tol `occluded` (b sees
 *                a nearer surface), d > tol `seen_through` (b sees past the point: a free-space conflict -- a pose error or something that
 *                moved), else `consistent` and photo += q(|I_a - I_b|), q(e) = (uint32)(e 16 + 0.5) for e < 4096, else (NaN too) 65535.
 *   record       in_view == unknown + occluded + seen_through + consistent, in_view <= valid.  consistent / valid is the share of a's
 *                surface b confirms; photo / (16 consistent) the mean absolute intensity difference over it, in grey levels.
 *   streams      as dvo_hip_frames_world_points: one launch on the context's main stream behind the builds of the frames, recorded
 *                (deferred) ingests are carried out first, and the call waits for that stream: host AND device records are complete
 *                on return.  Every distinct frame is uploaded once, whatever the number of pairs.
 *   refusals     DVO_HIP_ERR_INVALID, nothing launched, no output touched, no counter moved: null pointers; n_frames or n_pairs <= 0; more
 *                than 2^22 pairs (checked before any pair is read); a null or foreign frame; a level a frame does not have; too many
 *                pixels for one call (the blocks of 256 pixels of the listed frames exceed 2^31 / 256); an index outside [0, n_frames);
 *                a transform that is not finite; a tolerance that is negative or NaN; min_depth > max_depth or a NaN bound; a reserved
 *                field that is not 0; device records that are not 8-byte aligned.
 *   cost         profiles/covisibility.md.  Counter "covisibility_pairs" counts pairs. */
typedef struct dvo_hip_covis_params {
  float depth_tolerance;      /* metres; >= 0 */
  float depth_tolerance_rel;  /* added per metre of p.z; >= 0 */
  float min_depth, max_depth; /* of a's depth; 0 and +INFINITY: off */
  uint32_t reserved[4];       /* 0 */
} dvo_hip_covis_params;       /* 32 B */
typedef struct dvo_hip_covis_record {
  uint32_t valid, in_view, unknown, occluded, seen_through, consistent;
  uint64_t photo;
} dvo_hip_covis_record;       /* 32 B */
/* depth_tolerance 0.05f, depth_tolerance_rel 0, min_depth 0, max_depth +INFINITY */
dvo_hip_covis_params dvo_hip_covis_params_default(void);
/* Pair k: frames[pair_a[k]] seen by frames[pair_b[k]] under transforms[16 k ..] at `level` into records_out[k]; host memory, or device
 * memory (8-byte aligned) with out_on_device.  params NULL: the defaults. */
int dvo_hip_frames_covisibility(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, int n_pairs, const int32_t* pair_a,
                                const int32_t* pair_b, const double* transforms /* n_pairs x 16 */, int level,
                                const dvo_hip_covis_params* params_or_null, dvo_hip_covis_record* records_out, int out_on_device);

/* ---- keyframes retrieved by appearance: fern codes and their search on the device -----------------------------------------------------------
 * Which keyframes a frame should be aligned against when NO pose can be trusted.  The reference's proposal
 * (NearestNeighborConstraintSearch::findPossibleConstraints, dvo_slam/src/keyframe_constraint_search.cpp:41-72) and
 * dvo_hip_frames_covisibility both start from a pose; a lost tracker, a loop that closes after drift and two sessions without common
 * coordinates have none, and the reference has no answer to them.  These calls go beyond it with keyframe encoding by randomised ferns
 * (Glocker et al., TVCG 2015): a frame becomes m 4-bit tests on a coarse pyramid level (a CODE of m / 2 bytes), similar views have codes
 * that differ in few ferns, and retrieval is a search over all stored codes.  Everything is comparisons and integer counts, stated once
 * in dvo_slam_amd/csrc/keyframe_codes.h, whose host build the device results EQUAL.
 *   fern         {u, v, u2, v2, t_i, t_z}: on a level of w x h pixels x = (u w) >> 16, y = (v h) >> 16, likewise x2, y2.  Nibble: bit 0
 *                I(x, y) > t_i; bit 1 I(x, y) > I(x2, y2); bit 2 Z(x, y) finite and > t_z; bit 3 Z(x, y) finite.  NaN compares false.
 *   code         m nibbles, eight to a 32-bit word, fern 8 j + i in bits 4 i .. 4 i + 3 of word j.  m: a multiple of 128, 128 .. 2048.
 *   distance     the number of ferns whose nibbles differ in any bit, 0 .. m.
 *   book         dvo_hip_codebook: a device-resident set of codes under ONE fern table.  A slot's id is its index; ids are given in the
 *                order of adding and are not reused before dvo_hip_codebook_clear; a removed slot stays dead.  The codes of `capacity`
 *                entries (capacity m / 2 bytes) are allocated when the book is created.
 *   answer       per query the k live entries outside its skipped id interval [skip_from, skip_to) of least (distance, id), ascending, a
 *                tie in distance to the lower id; padded with {0xFFFFFFFF, 0xFFFFFFFF} where fewer than k qualify.
 *   streams      every launch runs on the context's main stream behind the builds of the frames, recorded (deferred) ingests are carried
 *                out first, and every call waits for that stream: host AND device outputs are complete on return.
 *   refusals     DVO_HIP_ERR_INVALID, nothing launched, no book, output or counter touched: a null context, book or pointer; a book of
 *                another context; m that is no multiple of 128 in 128 .. 2048; capacity outside 1 .. 2^24; z_lo or z_hi not finite or
 *                z_lo > z_hi (without a table of the caller's); n <= 0; n_queries > 4096; k outside 1 .. 64; a null or foreign frame; a
 *                level a frame does not have; a level wider or higher than 32767 pixels; more than 2^20 frames, or too many pixels for one
 *                call (the blocks of 256 pixels of the listed frames exceed 2^31 / 256); an id (or first + n) beyond the book's size;
 *                device codes that are not 4-byte aligned, device result rows that are not 8-byte aligned, device distances that are not
 *                2-byte aligned.  A book too full for the call: DVO_HIP_ERR_CAPACITY, nothing added.
 *   cost         profiles/keyframe_codes.md.  Counters "codebook_encoded" (frames encoded, into a book or not) and "codebook_queries". */
typedef struct dvo_hip_fern {
  uint16_t u, v, u2, v2;      /* positions as fractions of the level, / 65536 */
  float t_i, t_z;             /* thresholds: grey levels, metres */
} dvo_hip_fern;               /* 16 B */
typedef struct dvo_hip_code_match {
  uint32_t id, distance;
} dvo_hip_code_match;         /* 8 B */
typedef struct dvo_hip_codebook dvo_hip_codebook;
/* A book of at most `capacity` codes of m ferns.  ferns_or_null: the caller's table of m ferns, else the stated generator's
 * (keyframe_codes.h, fern_table) for `seed` with depth thresholds uniform in [z_lo, z_hi) (0.5 and 5 metres are the usual choice). */
int dvo_hip_codebook_create(dvo_hip_context* ctx, int m, int capacity, uint64_t seed, const dvo_hip_fern* ferns_or_null, float z_lo, float z_hi,
                            dvo_hip_codebook** book_out);
void dvo_hip_codebook_destroy(dvo_hip_context* ctx, dvo_hip_codebook* book);
/* forgets every entry: size 0, ids start at 0 again; the fern table stays */
int dvo_hip_codebook_clear(dvo_hip_context* ctx, dvo_hip_codebook* book);
/* any of the outputs may be NULL.  size: ids given so far; live: of those, not removed */
int dvo_hip_codebook_info(dvo_hip_context* ctx, const dvo_hip_codebook* book, int* m, int* capacity, int* size, int* live);
/* the book's m ferns into host memory */
int dvo_hip_codebook_ferns(dvo_hip_context* ctx, const dvo_hip_codebook* book, dvo_hip_fern* ferns_out);
/* The codes of n frames at `level` under the book's ferns, m / 8 words each, into codes_out (host, or device with out_on_device); the
 * book is not changed.  Frames of different sizes and cameras share the call (one launch). */
int dvo_hip_frames_encode(dvo_hip_context* ctx, const dvo_hip_codebook* book, int n, dvo_hip_frame* const* frames, int level,
                          uint32_t* codes_out, int out_on_device);
/* ... encoded straight into the book's next n slots; ids_out_or_null (host): the ids given */
int dvo_hip_codebook_add_frames(dvo_hip_context* ctx, dvo_hip_codebook* book, int n, dvo_hip_frame* const* frames, int level,
                                uint32_t* ids_out_or_null);
/* n raw codes (host, or device with on_device) into the next n slots: codes of another context's book, or of a saved one */
int dvo_hip_codebook_add_codes(dvo_hip_context* ctx, dvo_hip_codebook* book, int n, const uint32_t* codes, int on_device,
                               uint32_t* ids_out_or_null);
/* the listed entries die (an id may be listed twice, or be dead already); their slots are not given again */
int dvo_hip_codebook_remove(dvo_hip_context* ctx, dvo_hip_codebook* book, int n, const uint32_t* ids);
/* the stored codes of entries first .. first + n - 1, dead ones included */
int dvo_hip_codebook_read_codes(dvo_hip_context* ctx, const dvo_hip_codebook* book, int first, int n, uint32_t* codes_out, int out_on_device);
/* Three entry points over one query: the queries are frames encoded at `level`, raw codes, or the book's own entries `ids` (dead ones
 * may ask too).  skip_from_or_null / skip_to_or_null (host, n_queries each, both or neither): ids skip_from[q] <= id < skip_to[q] are
 * left out of query q -- the query itself and its neighbours in time, which are trivially similar.  results_out: n_queries x k records.
 * distances_out_or_null: n_queries x size uint16, 0xFFFF for a dead or skipped entry -- the matrix of an all-against-all comparison.
 * out_on_device: where results_out and distances_out lie. */
int dvo_hip_codebook_query_frames(dvo_hip_context* ctx, dvo_hip_codebook* book, int n_queries, dvo_hip_frame* const* frames, int level, int k,
                                  const uint32_t* skip_from_or_null, const uint32_t* skip_to_or_null, dvo_hip_code_match* results_out,
                                  uint16_t* distances_out_or_null, int out_on_device);
int dvo_hip_codebook_query_codes(dvo_hip_context* ctx, dvo_hip_codebook* book, int n_queries, const uint32_t* codes, int codes_on_device, int k,
                                 const uint32_t* skip_from_or_null, const uint32_t* skip_to_or_null, dvo_hip_code_match* results_out,
                                 uint16_t* distances_out_or_null, int out_on_device);
int dvo_hip_codebook_query_ids(dvo_hip_context* ctx, dvo_hip_codebook* book, int n_queries, const uint32_t* ids, int k,
                               const uint32_t* skip_from_or_null, const uint32_t* skip_to_or_null, dvo_hip_code_match* results_out,
                               uint16_t* distances_out_or_null, int out_on_device);

/* ---- colour in the keyframe map: frames keep RGB, voxels fuse it -------------------------------------------------------------------------
 * The reference's map is coloured: dvo_benchmark/src/benchmark_slam.cpp:89-90 keeps the camera image in level(0).rgb,
 * AsyncPointCloudBuilder::BuildJob::build (dvo_core/src/visualization/async_point_cloud_builder.cpp:72-104) writes p.b, p.g, p.r from it
 * whenever hasRgb(), and PointCloudAggregator::build voxel-filters PointXYZRGB clouds.  Here a frame may CARRY colour beside what it was
 * ingested from, a map created with DVO_HIP_MAP_COLOUR fuses it per voxel, and the extraction and the views return it.  Tracking stays on
 * intensity; a grey map, and every entry point above, behaves as it did.  All of it is integer arithmetic, stated once in
 * dvo_slam_amd/csrc/cloud_colour.h, whose host build the device results equal BIT FOR BIT.
 *   packed pixel  a uint32 0x00RRGGBB (PCL's PointXYZRGB::rgba layout with A = 0), from BGR8 / RGB8 / BGRA8 / RGBA8 bytes; alpha is ignored.
 *   frame colour  dvo_hip_frames_set_colour packs n planes in one launch into frame-owned planes of level-0 size.  The colour is a frame
 *                 PROPERTY like a lens or a selection: it stays until replaced or cleared, and a re-ingest does NOT touch it -- a caller
 *                 that re-ingests other content into the frame re-attaches the colour that belongs to it.  The colour of level L at (u, v)
 *                 is, per channel, the rounded mean of the 2^L x 2^L block of level 0 at (u << L, v << L):
 *                 (sum + (1 << (2 L - 1))) >> 2 L; level sizes are w0 >> L, so every block lies inside level 0.
 *                 dvo_hip_frame_download_colour returns that plane, exactly as an insertion sees it.
 *   sums          a coloured map has a side table beside its slots (16 more bytes per slot): per voxel the sums of the three 8-bit
 *                 channels of its points, uint32 each (255 * 2^20 < 2^28: nothing wraps up to the 2^20-point limit).  Insert, remove,
 *                 move and rehash carry them like the other sums: integer adds, a removal subtracts exactly what the insertion added.
 *   extraction    per channel c = (2 s + n) / (2 n) in unsigned 64-bit integer division (the mean, rounded half up), clamped to 255; the
 *                 record is 0xFF000000 | r << 16 | g << 8 | b, at the index of the voxel's xyzi record.
 *   views         the z-buffer element is uint64(bits(p.z)) << 32 | r << 16 | g << 8 | b: the nearest voxel, and of voxels at the same
 *                 depth the one with the LOWER packed colour.  The depth plane equals dvo_hip_map_render's bit for bit.  A hole is
 *                 Z = NaN (0x7FC00000) and colour word 0; a covered pixel has A = 0xFF.
 *   streams       like the map calls: the main stream, behind earlier work, recorded ingests first.  dvo_hip_frames_set_colour returns
 *                 when the caller's planes, host or device, may be reused.
 *   refusals      DVO_HIP_ERR_INVALID, nothing launched, nothing changed: an unknown pixel format, a null entry, 0 < colour_pitch <
 *                 width * channels, a frame of another context, the same frame twice in a call, and a frame that carries a LENS -- such a
 *                 frame takes raw sensor planes, so its colour would have to be rectified first (a depth rig is fine: depth is
 *                 registered INTO the colour camera); dvo_hip_frame_download_colour of a frame without colour or at a level it lacks;
 *                 dvo_hip_map_insert / _remove / _move of a frame without colour into a COLOURED map (a grey map ignores attached
 *                 colour); dvo_hip_map_extract_colour and dvo_hip_map_render_colour on a grey map; an unknown flag.
 *   cost          profiles/keyframe_map_colour.md. */
/* colour: n planes of frame i's level-0 size, pixel_format one of DVO_HIP_PIXEL_{BGR8, RGB8, BGRA8, RGBA8}, rows colour_pitch bytes
 * apart (0 = tight); host memory, or device memory with on_device.  Or one of the six sensor formats (DVO_HIP_PIXEL_BAYER_*,
 * DVO_HIP_PIXEL_YUYV8 / _UYVY8; their plane rules above): the plane stored is the packed BGR8 image of sensor_formats.h. */
int dvo_hip_frames_set_colour(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* colour, int pixel_format,
                              size_t colour_pitch, int on_device);
int dvo_hip_frames_clear_colour(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames);
/* the colour plane of `level` as packed pixels into out (host, w_L * h_L words, tight) */
int dvo_hip_frame_download_colour(dvo_hip_context* ctx, dvo_hip_frame* frame, int level, uint32_t* out);
#define DVO_HIP_MAP_COLOUR 1u /* dvo_hip_map_create_ex: the map fuses colour */
/* dvo_hip_map_create with flags: 0 is dvo_hip_map_create itself; DVO_HIP_MAP_COLOUR adds the side table (48 bytes per slot in all) */
int dvo_hip_map_create_ex(dvo_hip_context* ctx, float leaf, size_t capacity_slots, unsigned flags, dvo_hip_map** out);
/* dvo_hip_map_extract of a coloured map with the colour records into rgba (max_points words; host, or device with out_on_device).
 * dvo_hip_map_extract itself returns of a coloured map what it returns of a grey one fed the same frames. */
int dvo_hip_map_extract_colour(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_points, float* xyzi, uint32_t* rgba, uint32_t* counts_or_null,
                               uint64_t* keys_or_null, int out_on_device, size_t* n_points);
/* dvo_hip_map_render of a coloured map: the colour words into rgba_out[i], Z into depth_out[i], width * height elements each, tight; host
 * arrays, or device arrays (16-byte aligned) with out_on_device.  View preparation, footprint, parameters and refusals are the grey view's. */
int dvo_hip_map_render_colour(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float K[4],
                              const double* poses /* n x 16 */, const dvo_hip_render_params* params, uint32_t* const* rgba_out,
                              float* const* depth_out, int out_on_device);

/* ---- keyframe sub-maps: merge, subtract, re-pose and export voxel tables -------------------------------------------------------------
 * The reference's LocalMap (dvo_slam/include/dvo_slam/local_map.h) is a keyframe with a handful of frames around it; the pose graph moves
 * keyframes and everything attached to one moves rigidly with it.  A SUB-MAP is a dvo_hip_map built in the coordinates of its anchor
 * keyframe (insertion poses T_anchor^-1 * T_i); the global map is the sum of the sub-maps under their anchors' poses, and follows
 * dvo_hip_graph_optimize from the voxel tables alone -- 32 bytes per voxel (48 with colour) -- so the frames can be destroyed.
 *   record      32 bytes, the layout of a slot: {uint64 key; uint32 n, sx, sy, sz, si, pad} (dvo_slam_amd/csrc/cloud_map.h, MapSlot); of a
 *               coloured map also 16 bytes {uint32 sr, sg, sb, pad} at the same index of a second array.  A record whose key is ~0 or
 *               whose n is 0 is not live and is skipped.
 *   plain       sources of the destination's leaf (equal as bits).  Sign +1: a record's key is probed like an inserted point's and the
 *               record's integer sums are ADDED to the voxel's as whole words, which is the arithmetic of inserting its points one at a
 *               time: the sum of two sub-maps is, BIT FOR BIT in what dvo_hip_map_extract and dvo_hip_map_render give, the map built from all
 *               their keyframes at once.  Sign -1: a lookup that claims nothing, the same words subtracted, as dvo_hip_map_remove does: what
 *               was merged leaves exactly.  A record without a slot is dropped (+1) or unmatched (-1), counted by its n points.
 *   posed       the source enters under a pose T (source coordinates -> destination coordinates, row-major 4 x 4 double cast to float
 *               once): a source voxel's centroid (what dvo_hip_map_extract returns for it) is transformed in float, binned with the
 *               DESTINATION's leaf, and added there as n points at that position with the voxel's intensity (and colour) sums unchanged.
 *               Deterministic and equal to the host build of cloud_map.h (map_pose_record) bit for bit; subtracting under the same pose
 *               restores the destination bit for bit.  The leaves may differ.
 *   accuracy    a posed merge treats a source voxel's points as n copies of their centroid: a point may land up to one source leaf from
 *               where a rebuild from the frames would put it.  The point-weighted mean position is kept to quantisation, per axis
 *               (leaf_src + leaf_dst) / 2048 plus float rounding of the transform.  It is the sub-map approximation, not a rebuild.
 *   statistics  a plus merge adds the points it placed to `points`, a minus merge takes them back (and adds them to `removed`); dropped and
 *               unmatched count points.  A posed merge counts a record whose transformed centroid is not finite as n unusable points,
 *               one beyond +-2^20 voxels as n out of range.  A plain merge from a map adds (-1: takes back) the source's out_of_range
 *               and unusable: points, out_of_range, unusable, dropped and over_limit of a merged map are those of the single build.
 *   returns     as dvo_hip_map_move: DVO_HIP_ERR_CAPACITY if the call dropped points, else DVO_HIP_ERR_INVALID if it left unmatched
 *               points, else DVO_HIP_OK; the map keeps what the call did.  Every call runs on the main stream and waits for it, as
 *               dvo_hip_map_insert does.
 *   refusals    DVO_HIP_ERR_INVALID, nothing launched, nothing changed: a source that is the destination; a null map or one of another
 *               context (that way leads through dvo_hip_map_export and dvo_hip_map_merge_records); coloured against grey, or a coloured
 *               destination given records without colour records; a plain merge whose source leaf is not the destination's; a sign
 *               other than +1 and -1; a pose with an entry that is not finite; a minus entry into a destination that has dropped
 *               points since its last clear or rehash; n_src < 0; more than 2^32 records; device records not 16-byte aligned.
 *   cost        profiles/keyframe_map_merge.md. */
/* leaf, flags (DVO_HIP_MAP_COLOUR | DVO_HIP_MAP_NORMALS, or 0) and slots of a map; any of the three may be NULL */
int dvo_hip_map_info(dvo_hip_context* ctx, dvo_hip_map* map, float* leaf, unsigned* flags, uint64_t* capacity);
/* n_src source maps into (sign +1) or out of (-1) dst in ONE launch.  signs_or_null NULL: +1 for every source.  poses_or_null NULL: a
 * plain merge of every source; else a posed merge of source i under poses[16 * i ..].  A source may appear more than once. */
int dvo_hip_map_merge(dvo_hip_context* ctx, dvo_hip_map* dst, int n_src, dvo_hip_map* const* src, const int* signs_or_null,
                      const double* poses_or_null /* n x 16 */);
/* After a pose-graph optimisation: every sub-map leaves dst under poses_old and enters it under poses_new, in ONE launch over 2 n
 * entries -- bit for bit the posed subtraction followed by the posed merge.  A sub-map whose two poses are equal once cast to float is
 * left out (a call in which every one is launches nothing and returns DVO_HIP_OK). */
int dvo_hip_map_move_submaps(dvo_hip_context* ctx, dvo_hip_map* dst, int n_src, dvo_hip_map* const* src, const double* poses_old /* n x 16 */,
                             const double* poses_new /* n x 16 */);
/* The live voxels of a map as raw records, in unspecified order: records (max_records x 32 bytes) and, of a coloured map, their colour
 * records into colour_records_or_null (max_records x 16 bytes) where that is not NULL; host arrays, or device arrays (16-byte aligned) with
 * out_on_device.  *n_records = records written.  DVO_HIP_ERR_CAPACITY if the map holds more live voxels than max_records (the first
 * max_records found are written).  records NULL with max_records 0 only counts: *n_records = the live voxels, DVO_HIP_OK.  With the leaf and the flags (dvo_hip_map_info) the
 * records are the whole map: save them, or hand them to another context or device. */
int dvo_hip_map_export(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_records, void* records, void* colour_records_or_null, int out_on_device,
                       size_t* n_records);
/* dvo_hip_map_merge of one source given as n_records records (and colour records) in host memory -- staged on the main stream -- or in
 * device memory (on_device, 16-byte aligned), binned with leaf_src.  pose_or_null NULL: plain.  Equal keys in the array are summed. */
int dvo_hip_map_merge_records(dvo_hip_context* ctx, dvo_hip_map* dst, size_t n_records, const void* records, const void* colour_or_null,
                              int on_device, float leaf_src, int sign, const double* pose_or_null /* 16 */);

/* ---- surface normals in the keyframe map: frames give them, voxels fuse them ------------------------------------------------------------
 * The reference's map is a PointXYZRGB cloud; whoever meshes it, shades it from a new pose or feeds a point-to-plane consumer needs the
 * PointXYZRGBNormal, and would otherwise estimate normals on the host from the organised cloud.  Here every frame yields an organised plane
 * of normals on the device, a map created with DVO_HIP_MAP_NORMALS fuses them per voxel, and an extraction and a view return them.  A map
 * without the flag, and every entry point above, behaves as it did.  The arithmetic is stated once in dvo_slam_amd/csrc/cloud_normal.h,
 * whose host build the device results equal BIT FOR BIT.
 *   pixel normal  from the level's own depth plane (what dvo_hip_frame_download_plane returns) and K: the cross product of the central
 *                 differences of the back-projected 4-neighbourhood, in float; normalised in double; facing the camera.  A pixel has a
 *                 normal iff it is not on the level's border, it is usable as a map point (depth range included), its four neighbours
 *                 have a finite depth > 0, and the surface is seen at a cosine of at least 0.1 (about 84 degrees) -- which also drops a
 *                 stencil across a depth step above roughly 4 % of the depth at level 0.  That constant is a definition with no knob.
 *                 It is NOT PCL's k-neighbour PCA, and there is no viewpoint ambiguity to resolve.
 *   world normal  N = R n in float under the frame's pose: no translation, no renormalisation.  dvo_hip_frames_normals returns the plane
 *                 of records {N.x, N.y, N.z, has}, has 1.0f or 0.0f (then N = 0), exactly as an insertion sees it.
 *   sums          a map with normals has a side table beside its slots (16 more bytes per slot): per voxel the sums of the three components
 *                 quantised to 10 bits with a bias (q = floor(N * 511 + 0.5) + 511 in [0, 1022]) and nn, the number of its points that
 *                 had a normal; uint32 each, 1022 * 2^20 < 2^30.  A point without a normal is inserted as ever and adds nothing there.
 *                 Insert, remove, move, rehash and clear carry the table: integer adds, a removal subtracts exactly what was added.
 *   extraction    in double, rounded once: m = s - 511 nn per component, the record is {m / |m|, |m| / (511 nn)} -- the unit normal and the
 *                 AGREEMENT of the fused normals, about 1 on a flat patch, low on a crease or a thin wall seen from both sides -- or
 *                 {0, 0, 0, 0} where nn = 0 or m = 0; at the index of the voxel's xyzi record.
 *   views         the z-buffer element is uint64(bits(p.z)) << 32 | payload, payload = 1 << 30 | qx << 20 | qy << 10 | qz of the voxel's
 *                 extracted world normal, 0 for a voxel without one: the nearest voxel, and of voxels at the same depth the LOWER payload.
 *                 The depth plane equals dvo_hip_map_render's bit for bit.  A pixel's record is the dequantised normal rotated into the
 *                 VIEW'S CAMERA coordinates and 1.0f; {0, 0, 0, 0} for a hole (Z = NaN) and for a voxel without a normal.  It is not
 *                 renormalised: its length is within the quantisation of 1.
 *   sub-maps      dvo_hip_map_merge and dvo_hip_map_move_submaps take maps with normals without a change of signature (source and
 *                 destination must agree in the flag).  A RECORD of such a map has 16 more bytes {uint32 snx, sny, snz, nn} at the same
 *                 index of a third array: dvo_hip_map_export_ex and dvo_hip_map_merge_records_ex are the two record calls with that
 *                 array.  A plain merge adds the sums as whole words: the sum of two sub-maps is bit for bit the single build.  A posed
 *                 merge turns a voxel's SUMMED normal: m = s - 511 nn, M = R m in double, s' = clamp(rint(M) + 511 nn, 0, 1022 nn), nn
 *                 unchanged; deterministic, and a posed subtraction under the same pose restores the words.  The old
 *                 dvo_hip_map_export of a map with normals writes what it always wrote, without them; the old
 *                 dvo_hip_map_merge_records into a map with normals is REFUSED: it cannot supply them.
 *   other calls   dvo_hip_map_extract, dvo_hip_map_render and their colour forms return of a map with normals what they return of one
 *                 without, fed the same frames.  DVO_HIP_MAP_COLOUR and DVO_HIP_MAP_NORMALS combine.
 *   refusals      DVO_HIP_ERR_INVALID, nothing launched, nothing changed: dvo_hip_map_extract_normals and dvo_hip_map_render_normals on a
 *                 map without the flag; a null output; a device array that is not 16-byte aligned; rgba given for a map without colour;
 *                 what dvo_hip_frames_world_points, dvo_hip_map_extract_colour and dvo_hip_map_render refuse.
 *   cost          profiles/keyframe_map_normals.md. */
/* The value is 4, not 2: flags = 2 has been an unknown flag that is refused since the flags exist, callers may rely on that, and it stays
 * refused.  DVO_HIP_MAP_NORMALS adds the normal side table (16 more bytes per slot); dvo_hip_map_info reports the bit. */
#define DVO_HIP_MAP_NORMALS 4u /* dvo_hip_map_create_ex: the map fuses surface normals */
/* The twin of dvo_hip_frames_world_points: w_L x h_L records of 4 floats {N.x, N.y, N.z, has} per frame into out[i]; host arrays, or device
 * arrays (16-byte aligned) with out_on_device.  Streams, deferred ingests and refusals as there. */
int dvo_hip_frames_normals(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const double* poses /* n x 16 */, int level,
                           float min_depth, float max_depth, float* const* out, int out_on_device);
/* dvo_hip_map_extract of a map with normals with the normal records (4 floats per voxel) into normals; rgba_or_null: the colour records
 * of a map that also has colour, NULL for one without.  Otherwise as dvo_hip_map_extract_colour. */
int dvo_hip_map_extract_normals(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_points, float* xyzi, float* normals, uint32_t* rgba_or_null,
                                uint32_t* counts_or_null, uint64_t* keys_or_null, int out_on_device, size_t* n_points);
/* dvo_hip_map_render of a map with normals: width * height records of 4 floats into normals_out[i], Z into depth_out[i], tight; host
 * arrays, or device arrays (16-byte aligned) with out_on_device.  View preparation, footprint, parameters and refusals are the grey view's. */
int dvo_hip_map_render_normals(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float K[4],
                               const double* poses /* n x 16 */, const dvo_hip_render_params* params, float* const* normals_out,
                               float* const* depth_out, int out_on_device);
/* dvo_hip_map_export with one more array: the normal records (max_records x 16 bytes, {uint32 snx, sny, snz, nn}) of a map with normals
 * into normal_records_or_null where that is not NULL (refused for a map without normals).  Otherwise as dvo_hip_map_export. */
int dvo_hip_map_export_ex(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_records, void* records, void* colour_records_or_null,
                          void* normal_records_or_null, int out_on_device, size_t* n_records);
/* dvo_hip_map_merge_records with one more array: a destination with normals takes records WITH normal records, one without takes none.
 * Otherwise as dvo_hip_map_merge_records. */
int dvo_hip_map_merge_records_ex(dvo_hip_context* ctx, dvo_hip_map* dst, size_t n_records, const void* records, const void* colour_or_null,
                                 const void* normals_or_null, int on_device, float leaf_src, int sign, const double* pose_or_null /* 16 */);

/* ---- the hot path --------------------------------------------------------------------------- */
/* DenseTracker::match(RgbdImagePyramid& reference, RgbdImagePyramid& current, Result&)
 * (dvo_core/src/dense_tracking.cpp:123-376).  `levels`/`iters` may be NULL (no statistics).
 * Always returns DVO_HIP_OK on a completed run, like the reference's `return true` (Q16): failure
 * is signalled by NaNs in the result and by the termination criteria. */
int dvo_hip_match(dvo_hip_context* ctx, dvo_hip_frame* reference, dvo_hip_frame* current,
                  const dvo_hip_config* cfg, dvo_hip_result* result,
                  dvo_hip_level_stats* levels, int cap_levels,
                  dvo_hip_iteration_stats* iters, int cap_iters);

/* n independent matches in one batched launch sequence (grid = tiles x pairs): the multi-hypothesis
 * shape of KeyframeGraph::validateKeyframeConstraintsParallel (dvo_slam/src/keyframe_graph.cpp:576-593)
 * and of LocalTracker::update's two trackers (dvo_slam/src/local_tracker.cpp:180-184).
 * results[i].transformation is in/out.  Optional stats: levels[i*cap_levels + l],
 * iters[i*cap_iters + k].  All frames must share width/height/levels. */
int dvo_hip_match_batch(dvo_hip_context* ctx, int n_pairs,
                        dvo_hip_frame* const* references, dvo_hip_frame* const* currents,
                        const dvo_hip_config* cfg, dvo_hip_result* results,
                        dvo_hip_level_stats* levels, int cap_levels,
                        dvo_hip_iteration_stats* iters, int cap_iters);

/* One Gauss-Newton linearisation at a given estimate: passes 1-5 of dense_tracking.cpp:271-343
 * (computeResidualsSse + computeWeightsSse + computeScaleSse + computeCompleteDataLogLikelihood +
 * NormalEquationsLeastSquares::update) for parity tests against the oracle. */
typedef struct {
  int32_t n;                 /* valid constraints */
  int32_t n_selected;        /* selected reference pixels of the level */
  float scale_cov[3];        /* C00 C01 C11 = sum w r r^T / (n-3) */
  float precision[4];        /* P = C^-1, row-major */
  double neg_loglik;         /* -ll */
  double A[36];              /* J^T (w P) J, row-major, without mu */
  double b[6];               /* -J^T (w P) r */
  double sum_w;              /* reserved (0) */
} dvo_hip_iteration_out;

int dvo_hip_level_iteration(dvo_hip_context* ctx, dvo_hip_frame* reference, dvo_hip_frame* current, int level,
                            float intensity_threshold, float depth_threshold,
                            const float T34[12] /* row-major 3x4 float estimate: reference -> current */,
                            const float P_prev[4], int first_iteration_on_level,
                            dvo_hip_iteration_out* out,
                            float* residuals_or_null /* w*h*2 floats, NaN where invalid */);

/* ---- measurement ---------------------------------------------------------------------------- */
/* Launches the dominant kernel (fused warp + residual + weight + Jacobian + reduce) `reps` times for
 * the given pairs at `level`, bracketed by HIP events on the context stream; returns the average duration of one launch in
 * milliseconds.  `warm_iterations` Gauss-Newton steps are taken on that level first, so that the timed launches run where
 * the sweeps of a match run: at the transform the solver moved to, with the t-distribution weights on.  0 = at the identity
 * with unit weights (the first sweep of a level). */
int dvo_hip_time_residual_kernel(dvo_hip_context* ctx, int n_pairs,
                                 dvo_hip_frame* const* references, dvo_hip_frame* const* currents,
                                 int level, int warm_iterations, int reps, float* avg_ms);

/* The yardstick for that number: a kernel that only streams the planes the level's sweep reads, of the same pairs, in pixel order
 * (window sweep, the default where the level's width is a multiple of 64: reference {Zsel, I} 8 B + current {I, Z} 8 B per pixel;
 * gathering sweep: 8 + 16 + 8 B; with_write != 0: plus the 8 B per pixel the sweep writes for the log-likelihood pass) -- no
 * gather, no arithmetic, no reduction.  What the memory system needs for the bytes the sweep moves on this part. */
int dvo_hip_time_stream_mix(dvo_hip_context* ctx, int n_pairs,
                            dvo_hip_frame* const* references, dvo_hip_frame* const* currents,
                            int level, int with_write, int reps, float* avg_ms);

/* Tunables (0 = library default).  key: "rows_per_wave" (1,2,4,8,16: tile height of the sweep kernel),
 * "iters_per_sync" (host polling cadence of the batched Gauss-Newton loop), "variant" (schedule of the sweep
 * kernel: 8 (default) = the current frame's {I, Z} window staged in LDS, contracted per-pixel arithmetic (fused multiply-adds,
 * v_rcp_f32 in the projection, separable blends: the same function as 7 to a few ulp of the tap coordinate -- residuals within 2e-5,
 * constraint counts equal except at pixels on a bound) + Gram accumulation on the f16 matrix pipe, on every level of even width >= 84
 * (a width that is no multiple of 64 leaves the last tile column partly empty) and the gathering sweep with the same arithmetic on
 * narrower ones; 9 = 8 with another way of storing the matrix operands (v_permlane32_swap; measurement); 7 = the window sweep
 * whose residuals and constraint counts equal the oracle's MATH mode BIT FOR BIT (no contraction, correctly rounded divisions), f16
 * Gram; 6 = the same with the f32 Gram (bit-identical to 5); 5 = gathered taps, f32 Gram accumulation on the matrix cores; 0 =
 * all-VALU with the DPP + LDS reduction),
 * "gram_lo_parts" (default 1 since round 6: every matrix operand is an exact f16 high + low pair on every level -- 22-bit operands, f32
 * accumulation: what the reference's f32 accumulation, dvo_core/src/core/math_sse.cpp:82-178, is compared with at 1e-5; 0: on levels of
 * 150 000 pixels and more the default schedule forms its operands from the f16 HIGH parts of the twelve Jacobian components alone -- the
 * two residual components keep both parts -- which is 3.5 % of the finest-level sweep; a component is then off by <= 2^-12 of itself,
 * at random, the normal equations by ~3e-6 of their largest entry at 190 000 constraints and `b` by up to 3e-5.
 * Never under options "deterministic", "ref_compat" and "variant" 9),
 * "compact_residuals" (default 1: the contracted window sweep stores only the residual pairs of constraints, packed per wavefront
 * slot, for the log-likelihood pass to read half the bytes; 0: one pair per pixel at its pixel's place like every other schedule --
 * the same normal equations bit for bit, the log-likelihood the same sum in another order),
 * "ll_blocks" (workgroups per pair of the log-likelihood pass, 1..32; 0 = by batch size: 32, 16 from 48 pairs, 8 from 256),
 * "tail_speculation" (measurement: 1 = the step ahead of the host's poll is always enqueued, also on the tail of a level whose empty
 * step is costly; n >= 2: costly means n workgroups or more per step; 0 = 131072),
 * "solver_waves" (wavefronts of a solver-step workgroup, 2 or 4; 0 = two on the smallest levels of a batch of more than two
 * workgroups per compute unit, four otherwise -- the records do not depend on it),
 * "solver_occupancy" (experiment: 3 = the four-wavefront solver step built for three workgroups per compute unit, 168 registers and part
 * of the serial lane's state in scratch, instead of the compiler's 184 = two; 0 = default.  Level on the boxes of round 6),
 * "min_workgroups" (tile-height heuristic: smallest launch that counts as filling the chip; 0 = built-in table),
 * "defer_ingest" (default 0; 1: dvo_hip_frames_update_raw_device_as only RECORDS its request -- the pointer arrays are copied, the
 * raw planes must stay valid as for any asynchronous ingest -- and the next dvo_hip_match_batch carries it out right behind the first
 * launches of its first level, so that the host's work for the ingest of batch k + 1 (0.1-0.5 ms) does not keep the alignment of batch k
 * from starting; any other entry point, a match that aligns the very frames, or switching the option off carries it out at once, and
 * returns its status if it fails; counter "deferred_ingests".  dvo_slam_amd/apps/stream_pipeline.cpp switches it on around its step),
 * "keep_raw_copy" (default 1: a frame ingested from raw planes straight into the REFERENCE role keeps a copy of them, 3 bytes per
 * pixel, from which its other role -- or a selection with other thresholds -- is derived later; 0: no copy: such a frame serves as a
 * reference with the thresholds it was ingested for until it is ingested again, anything else fails with DVO_HIP_ERR_INVALID.  The
 * value in effect when the ingest is requested counts; dvo_slam_amd/apps/stream_pipeline.cpp switches it off for its reference frames),
 * "stream_policy" (default 1: the strip kernels of a build on the build stream -- the ingest of raw planes and the role planes derived
 * there -- read the raw planes and write the planes of levels 0-1 and the raw copy with the non-temporal cache policy, so that a
 * background build does not push the planes of the coarse levels a running match re-reads out of the device's last-level cache; levels
 * 2-3 keep the default policy.  Planes and records are the same bit for bit either way; 0: the default policy everywhere, for A/B runs),
 * "table_cache" (default 1: a small table -- plane pointers of the frames to build or the pairs to align, initial guesses -- is not sent
 * to the device again when the very bytes were last sent to the very address on the same stream and no device memory was freed since:
 * a streaming caller hands over the same frame sets step after step; counter "table_uploads_skipped"; 0 for measurement),
 * "fused_ll_pixels" (largest level, in pixels, whose log-likelihood sweep runs inside the solver
 * workgroup instead of a launch of its own; 0 = 160x120, and 320x240 for batches of 512 pairs and more),
 * "condition_number" (1: results carry the condition number of the information
 * matrix, ~20 us of extra serial work per batch; default 0),
 * "deterministic" (1: a pair's record -- transform, information matrix, log-likelihood, every statistic -- is bit-identical whatever
 * batch the pair is aligned in and however many GPUs the batch is spread over, like the reference's result for a pair never depends on
 * its neighbours: one tile height on every level, one log-likelihood schedule, every level on the launch path.  By default the tile
 * height and the latency path follow the batch size and records agree to the precision of the stopping rule (1e-8 per pass) instead.
 * Price: a lone pair takes the launch path's 0.50 ms instead of 0.36 ms; large batches are unaffected; default 0),
 * "ref_compat" (1: the projection and the t-distribution weights multiply with the HOST CPU's approximate reciprocal _mm_rcp_ps, like
 * the reference's SSE path does (dvo_core/src/dense_tracking_impl.cpp:192, :700), instead of dividing exactly -- the one quirk of the
 * reference that separates its trajectories from the exact arithmetic's; the instruction is dumped into a table
 * when the option is first switched on; the latency path (option "resident") carries the same arithmetic; also switched on by the environment variable
 * DVO_HIP_REF_COMPAT=1 when a context is created; default 0.  The schedules keep their meaning in this mode: under "variant" 8 (the
 * default) the contracted window sweep runs with the table in place of v_rcp_f32 -- residuals within 2e-5 of the oracle's MATH + Q1
 * mode, the same constraints except at pixels on a bound; under "variant" 7 residuals and constraint counts equal that oracle mode
 * bit for bit.  2 = as 1 with the table read through memory by every sweep -- the path of a CPU whose table has no 16-bit copy for
 * the contracted sweep to keep in LDS; test and measurement),
 * "ref_order" (1: the reference's rank-dependent quirks -- Q3: an odd selection loses its last selected pixel (ValidPixels still
 * counts it); Q6: the scale matrix pairs the constraints in raster order and uses the first residual of each pair twice; Q7: the
 * log-likelihood sum drops its last n mod 50 terms -- so that Information and LogLikelihood follow the reference's own code.  With
 * "ref_compat" 1, under "variant" 8 (the default: what DVO_HIP_REF_COMPAT=1 DVO_HIP_REF_ORDER=1 give) and 7 alike, Information lands
 * 1e-4 ... 1.3e-2 of its largest entry from the reference's (median 1.8e-3 over 32 pairs), LogLikelihood 1e-6 ... 1.6e-4 -- as close
 * as the oracle's float64 rendering of these quirks gets; without the option 20 %, and in the default mode about 6 times the
 * reference's (README "What agrees with what").  Independent of "ref_compat"; "variant" 7 or 8 only.  Every level runs on the launch
 * path with two extra passes per step (ref_order.hip); "resident", "coarse", "small_sweep", "sweep_tail", "overlap_tails",
 * "tail_lists" and "batch_groups" are ignored.  Also switched on by DVO_HIP_REF_ORDER=1 when a context is created; default 0;
 * cost: profiles/ref_order.txt),
 * "resident" (-1 default: small batches and coarse levels run in ONE launch per match, each pair owned by a group of resident
 * workgroups -- the latency path, DESIGN.md section 4: up to compute units / 4 pairs the coarse levels, up to 7/16 of the compute
 * units -- and from compute units / 8 pairs on when the current frames hold plane C without the taps, as a role-aware ingest of that
 * many frames leaves them -- the coarsest one (DVO_HIP_TRACE_PLAN in the environment prints the plan of every batch to stderr); 0: one to three launches per Gauss-Newton step always; 1: every level resident), "resident_rows" (a level runs resident when a sweeping wavefront gets at most this many 64-pixel segments per
 * pass; default 24), "resident_group" (workgroups per pair, a power of two <= 64; 0 = as many as fit the device),
 * "resident_cooperative" (1: groups are launched with hipLaunchCooperativeKernel), "resident_flags" (measurement / test hooks).
 * "small_sweep" (default 0; 1: under the default schedule a pyramid level small enough for its whole current plane {I, Z} to live in LDS --
 * even width, (w + 2) x (h + 2) cells of 8 B within 43 KB: 80 x 60, 40 x 30 -- is swept by dvo_slam_amd/csrc/align_small.hip: a workgroup
 * copies the level into LDS once and finds every tap there, one memory round trip per pixel row instead of the gathering sweep's two.  Same
 * function, rounding differences of a few ulp in the blended gradients.  Off by default: measured level with the gathering sweep -- 45-50 us
 * against 46-48 per 1024-pair launch -- DESIGN.md section 10), "small_tiles" (its workgroups per pair; 0 = by batch size, 3 .. 8),
 * "batch_groups" (default 0 = one group; 2 .. 4: a batch is aligned as that many sub-batches AT ONCE (of at least 64 pairs each) -- the
 * caller's thread runs the first on this context, helper threads the others on twin contexts of the same device (own stream, own
 * scratch; created when first needed), the way the reference spreads independent match() calls over the workers of a
 * tbb::parallel_reduce (dvo_slam/src/keyframe_graph.cpp:576-593).  A pair's record is what its sub-batch gives it: bit-identical to the
 * ungrouped batch's where both fall into the same batch-size class of the schedule, equal to the precision of the stopping rule
 * otherwise.  Off by default: groups that start together stay in phase -- 1024 pairs 11.75 -> 11.1-11.9 ms per streaming step with two
 * groups; what several contexts on one GPU gain, they gain by running OUT of phase, which a streaming caller gets from the lanes of
 * dvo_slam_amd/apps/stream_pipeline.cpp (dvo_stream_lanes_*: 11.3 -> 10.8 ms).  Not under "deterministic" or "ref_compat"; counter
 * "grouped_batches"),
 * "sweep_tail" (default 0; 1: on the levels whose log-likelihood pass runs inside the solver step -- up to 160 x 120 pixels, 320 x 240
 * in batches of 512 pairs and more -- under the default schedule, the workgroup of the sweep that completes the LAST tile of a pair
 * runs the pair's Gauss-Newton step right there: one launch per iteration instead of two (dvo_slam_amd/csrc/solver_step.h; the
 * reference's loop body follows its residual pass without leaving the thread either, dvo_core/src/dense_tracking.cpp:240-357).  The
 * records are the two-launch form's bit for bit; 2: only the WIDE half of the step -- reduction and log-likelihood -- in the tail, the serial
 * half in a one-wavefront launch behind it.  Off by default: both forms measured slower (128 pairs 1.8 -> 2.2 / 2.3 ms per step, 1024
 * pairs 11.6 -> 14.4 / 13.6): every workgroup of the sweep waits ~5 us for its write-through stores before it can take the pair's
 * ticket, as long as its tile takes -- profiles/r06_sweep_tail.txt; counter "tail_steps"),
 * "overlap_tails" (1: once at most 1 / "overlap_fraction" -- default 8 -- of a batch's pairs is still on a pyramid level, those pairs
 * leave the batch's launch chain: the chain goes on to the next level without them, and a SLOW LANE -- a second stream with buffers of
 * its own -- runs them to the end of the match with launches over a list of pairs, level after level behind the chain, taking up the
 * stragglers of the later levels on the way; the batch ends when both are through.  Every pair runs its levels on its own, as in the
 * reference (dvo_core/src/dense_tracking.cpp:200-357), instead of the whole batch waiting for its slowest pair on every level.
 * Batches beyond the solver steps' hand-over (more than one pair per compute unit), the default schedule; the last level sheds
 * nothing.  The records are the synchronous chain's bit for bit; counters "overlapped_tails", "overlapped_steps", "tail_drains",
 * "tail_wait_us"),
 * "defer_ingest_pixels" (0; n: an ingest recorded under "defer_ingest" is not carried out before the launch chain has reached a pyramid
 * level of at least n pixels -- the memory-bound frame build slows the latency-bound kernels of the small levels by 30-50 %, the
 * issue-bound sweeps of the large ones by 2 %.  Measured on the 1024-pair streaming step: 11.21 against 11.04 ms with the ingest behind
 * the first step of the 320 x 240 level, 11.35 behind that of the finest -- the build then no longer ends before the match does),
 * "tail_lists" (1: where a step that finds no pair is expensive -- 131 072 workgroups and more per sweep, "tail_speculation" -- and at
 * most an eighth of the pairs is left on a level, the steps that follow are launched over the LIST of those pairs: tiles x active
 * workgroups instead of tiles x pairs of which all but a few leave at once; the same records; counter "listed_steps"),
 * "coarse" (default 0; 1: wherever the levels admit it -- the default schedule, no "ref_compat", levels of up to 160 x 120 pixels --
 * the leading pyramid levels run in ONE launch, a workgroup per pair from the level's begin to its termination, level after level,
 * like one thread runs one match() in the reference (dvo_core/src/dense_tracking.cpp:200-357, dvo_slam/src/keyframe_graph.cpp:576-593):
 * dvo_slam_amd/csrc/align_coarse.hip, in place of the resident kernel too.  No workgroup waits for another one: no residency
 * requirement, no time-out, any batch size; built from the launch path's own device functions on its data layout, so the records are
 * the launch path's bit for bit at the tile height 2 the kernel sweeps gathering levels with ("rows_per_wave" 2 on the launch path).
 * Off by default: slower than the launch path up to 1024 pairs per batch -- a workgroup walks the tiles of an iteration one after the
 * other, and with no more pairs than workgroup slots the launch lasts as long as its slowest pair),
 * "coarse_pixels" (the largest level it takes, in pixels; 0 = 160 x 120.  Above that the launch path's log-likelihood schedule differs
 * and the records agree to the stopping rule's precision only), "coarse_workgroups" (its workgroups per compute unit: 4 with 128
 * registers, the default, or 3 with 168).
 * "codebook_round_kb" (default 262144 = 256 MB; >= 1): the staging the dvo_hip_codebook_query_* calls may take for the distance matrix of
 * one round of queries when the caller gives no device matrix -- more queries than fit are answered in rounds of as many as fit (at
 * least one); the results do not depend on it.
 * "rendezvous" (default 1): two dvo_hip_match calls from two host threads with the SAME current frame and configuration -- the
 * reference's LocalTracker, dvo_slam/src/local_tracker.cpp:180-184 -- leave as one two-pair batch: the second caller's thread runs
 * it, the first waits at most 60 microseconds for a partner, and only on a context where concurrent callers have been seen
 * (counter "rendezvous_pairs").  A pair's record in a two-pair batch can differ from the single match's in the last bits (another
 * split of the sweep over workgroups), unless "deterministic" or a pinned "resident_group" makes records independent of the batch.
 * "build_workgroups" (default 0 = no cap): the largest grid a frame-build kernel of a batched (re-)ingest is launched with; the build
 * stream has the lowest priority, and a streaming caller that ingests the next batch while a match runs keeps the match's short
 * kernels moving by capping the background build at about one workgroup per compute unit (bench.py: 256, 14.23 -> 13.77 ms per step). */
int dvo_hip_set_option(dvo_hip_context* ctx, const char* key, int value);

/* Event counters of a context.  key: "resident_launches" (matches, or coarse-level runs, done by the resident kernel),
 * "resident_levels" (pyramid levels those launches ran, summed),
 * "grouped_batches" (batches aligned as concurrent sub-batches, option "batch_groups"),
 * "compute_units" (of the context's device), "defer_ingest_max_pairs" and "background_build_workgroups" (not events: what the library's
 * batch-size policy, dvo_slam_amd/csrc/batch_policy.h, says for that device -- the largest batch whose re-ingest a streaming caller
 * should defer behind the alignment's first launches, and the grid a background frame build should be capped at with option
 * "build_workgroups": one pair / one workgroup per compute unit),
 * "tail_steps" (Gauss-Newton steps of a batch enqueued as ONE launch, the sweep with the solver step in its tail, option "sweep_tail"),
 * "coarse_launches" / "coarse_levels" (the same for the fused coarse-level kernel, option "coarse"),
 * "ref_order_passes" (Gauss-Newton steps ENQUEUED with the scale passes of option "ref_order" -- including the steps enqueued ahead of a
 * poll, which do nothing for the pairs that have left the level -- and linearisations of dvo_hip_level_iteration under it),
 * "listed_steps" (Gauss-Newton steps launched over an active-pair list, option "tail_lists"),
 * "overlapped_tails" (levels that shed their last pairs to the slow lane, option "overlap_tails"), "overlapped_steps" (the
 * Gauss-Newton steps enqueued on the lane), "tail_drains" (batches that ended with a lane) and "tail_wait_us" (how long the host
 * waited for the lane behind the chain's last step, summed),
 * "resident_timeouts" (batches repeated on the launch-per-step path because a workgroup group of the resident kernel waited
 * in vain for its peers -- the device was shared with another such kernel; the results are those of the repeat),
 * "window_fallbacks" (lanes of the window sweep whose bilinear taps fell outside the staged window and were fetched from memory),
 * "f16_range_repeats" (PAIRS that ran a second time with the f32 Gram because a Jacobian component of some pixel was beyond the f16
 * range of the default schedule's matrix operands, +-65504: depth steps of metres right in front of the camera.  Only the pairs
 * concerned are repeated, as a batch of their own -- unless they are half of the batch or more: then the whole batch is, and the 32
 * batches that follow on this context start on the f32 Gram (a tracking sequence that keeps meeting such a step does not pay twice
 * per frame).  That hold makes the arithmetic of those batches -- f32 instead of f16 hi + lo Gram operands, 1e-6 apart in the
 * normal equations -- depend on what the context aligned before; setting option "variant" clears it, option "deterministic" never
 * enters it),
 * "deferred_ingests" (ingests carried out behind the first launches of a match, see option "defer_ingest"),
 * "table_uploads_skipped" (small host-to-device table uploads answered from the cache, see option "table_cache"),
 * "rendezvous_pairs" (two-pair batches formed from concurrent single matches, see option "rendezvous"),
 * "strip_ingests" (frames whose raw planes went through the strip ingest, one 128 x 8 strip per wavefront -- even-width rows and
 * 4 / 8-byte aligned planes; the others take the tile kernel),
 * "colour_ingests" (frames ingested from an 8-bit colour plane, dvo_hip_frame_create_colour* / dvo_hip_frames_update_colour*),
 * "sensor_ingests" (frames ingested from a raw sensor plane, DVO_HIP_PIXEL_BAYER_* / _YUYV8 / _UYVY8, through the same entry points;
 * "colour_ingests" does not count them, "strip_ingests" counts those whose grey-plane ingest took the strip kernel),
 * "f32_ingests" (frames ingested from a float depth plane, dvo_hip_frame_create_f32_device / dvo_hip_frames_update_f32* /
 * dvo_hip_frames_update_colour_f32depth*; "strip_ingests" counts those of them that took the strip kernel),
 * "lens_ingests" (frames rectified at ingest because they carry a lens, dvo_hip_frames_set_lens; each is also one of "f32_ingests"),
 * "depth_filter_ingests" (frames whose depth plane was conditioned at ingest because they carry a depth filter,
 * dvo_hip_frames_set_depth_filter; each is also one of "f32_ingests"),
 * "depth_registrations" (frames whose depth plane was registered at ingest because they carry a depth rig,
 * dvo_hip_frames_set_depth_rig; each is also one of "f32_ingests") and "depth_rig_table_bytes" (the size of that pass's pointer table:
 * 0 until the first such frame is ingested),
 * "map_inserts" (frames dvo_hip_map_insert and dvo_hip_map_move have launched into a map of this context), "map_points" (the points those
 * maps took) and "map_dropped" (the points they dropped for want of a slot; a call that drops any returns DVO_HIP_ERR_CAPACITY),
 * "map_removes" (frames dvo_hip_map_remove and dvo_hip_map_move have launched out of a map; a frame whose pose a move leaves as it is
 * counts in neither) and "map_rehashes" (tables dvo_hip_map_rehash has replaced).  Refused calls count nothing, dvo_hip_map_clear resets
 * none of them,
 * "map_renders" (views dvo_hip_map_render and dvo_hip_map_render_frames have rendered; a refused call counts nothing),
 * "frame_warps" (items dvo_hip_frames_warp_inverse and dvo_hip_frames_warp_forward have warped; a refused call counts nothing),
 * "covisibility_pairs" (pairs dvo_hip_frames_covisibility has counted; a refused call counts nothing),
 * "codebook_encoded" (frames dvo_hip_frames_encode, dvo_hip_codebook_add_frames and dvo_hip_codebook_query_frames have encoded) and
 * "codebook_queries" (queries the three dvo_hip_codebook_query_* have answered; a refused call counts nothing),
 * "warmup_wait_us" (the longest of the nine stream waits dvo_hip_context_create makes on trivial commands to warm up the runtime's wait
 * path, in microseconds: the first GPU process on a fresh box has been seen to spend 14-24 ms in its first wait),
 * "host_batches" and "host_ns_prepare" / "host_ns_enqueue" / "host_ns_wait" / "host_ns_finish" (nanoseconds the calling thread spent
 * in dvo_hip_match_batch before its first launch, enqueueing, waiting for the device and afterwards; accumulated). */
int dvo_hip_get_counter(dvo_hip_context* ctx, const char* key, long long* value);

/* ---- multi-GPU: one process per GPU, the records of a sharded batch gathered over RCCL (xGMI) --------------------------------
 * The reference runs independent match() calls on the workers of a tbb::parallel_reduce and concatenates their results
 * (dvo_slam/src/keyframe_graph.cpp:576-593; dvo_slam/src/local_tracker.cpp:180-184).  Spread over the GPUs of a node -- pair i on rank
 * i mod N, no communication while aligning -- the only exchange is an all-gather of fixed-size result records
 * afterwards.  These entry points are that exchange for a C++ host (inside ONE process dvo::DenseTracker::matchBatch over several
 * contexts needs none).  RCCL is loaded when the first of them is called (librccl.so.1; DVO_HIP_RCCL_LIBRARY overrides the name):
 * without it they return DVO_HIP_ERR_NO_DEVICE and nothing else in this header is affected.
 *   rank 0: dvo_hip_comm_get_unique_id(id) -> the caller carries the DVO_HIP_COMM_ID_BYTES bytes to every rank (a file, a socket, MPI,
 *           torch.distributed's store: the reference has no process launcher of its own, so none is prescribed here);
 *   every rank: dvo_hip_comm_create(ctx, id, rank, n_ranks, &comm)   -- collective (ncclCommInitRank) on the context's device;
 *   per batch:  dvo_hip_gather_records_begin(comm, mine, bytes_mine, bytes_per_rank, &ticket)   -- returns at once: the block is staged
 *               in pinned memory, copied to the device, ncclAllGather and the copy back are enqueued on the communicator's OWN stream
 *               (the context's stream is busy aligning the next batch by then); bytes_per_rank, a multiple of 8, is the same on every
 *               rank -- a rank with a smaller share is padded with zeros;
 *               dvo_hip_gather_records_end(comm, ticket, all, all_bytes)   -- waits for that gather: n_ranks blocks in rank order.
 *               Two gathers may be in flight (the records of step k travel while step k + 1 is aligned).
 *   dvo_hip_gather_records = begin + end.  Every rank must make the same sequence of calls (a collective).
 * The record layout a batch of alignments travels in -- 32 doubles per pair: twist (6) | upper triangle of the information matrix (21) |
 * log-likelihood | flag | padding (3) -- is dvo_stream_pack_records' (dvo_slam_amd/apps/stream_pipeline.cpp). */
typedef struct dvo_hip_comm dvo_hip_comm;
#define DVO_HIP_COMM_ID_BYTES 128
int dvo_hip_comm_get_unique_id(void* id /* DVO_HIP_COMM_ID_BYTES bytes */);
int dvo_hip_comm_create(dvo_hip_context* ctx, const void* id, int rank, int n_ranks, dvo_hip_comm** out);
void dvo_hip_comm_destroy(dvo_hip_comm* comm);
int dvo_hip_comm_rank(const dvo_hip_comm* comm);
int dvo_hip_comm_size(const dvo_hip_comm* comm);
const char* dvo_hip_comm_last_error(const dvo_hip_comm* comm /* null: the calling thread's last failed comm call */);
int dvo_hip_gather_records_begin(dvo_hip_comm* comm, const void* mine, size_t bytes_mine, size_t bytes_per_rank, int* ticket);
int dvo_hip_gather_records_end(dvo_hip_comm* comm, int ticket, void* all, size_t all_bytes);
int dvo_hip_gather_records(dvo_hip_comm* comm, const void* mine, size_t bytes_mine, size_t bytes_per_rank, void* all, size_t all_bytes);

/* ---- the keyframe pose graph, optimised on the device -----------------------------------------------------------------------------
 * The reference's back end builds a g2o graph of VertexSE3 / EdgeSE3 with an optional Cauchy kernel and runs Levenberg-Marquardt on it
 * after every keyframe and at the end of a sequence (dvo_slam/src/keyframe_graph.cpp:256-285, 475-489, 840-845; the local map's:
 * dvo_slam/src/local_map.cpp:79-88, 208-213).  A dvo_hip_graph is that problem and that step: Levenberg-Marquardt with g2o's
 * defaults around a block-Jacobi preconditioned conjugate-gradient solve, all in float64 (definitions, schedule and the order of every
 * sum: dvo_slam_amd/csrc/pose_graph.h).  The result is deterministic: a function of the vertices and of the edges
 * in the order given -- not independent of that order -- and the same bits run after run.  The optimised poses are what dvo_hip_map_move
 * takes as new_poses.
 * Poses and measurements: row-major 4 x 4 doubles, camera -> world, n x 16 / m x 16 like the map's.  Information: m x 36, row-major,
 * rows and columns translation first, then rotation, taken AS GIVEN: the reference hands Result.Information (twist order) straight to
 * setInformation (keyframe_graph.cpp:628); hand dvo_hip_result::information over the same way to get what it gets.
 * Limits: n <= 2^20 vertices, m <= 2^22 edges; an edge costs about 1 KB of device memory, a vertex about 1 KB.
 * Two schedules, the same bits.  The launch path (dvo_hip_graph_optimize by default) enqueues every stage of a trial as a launch of its
 * own over all vertices or edges: any size, but two launch latencies per conjugate-gradient iteration however small the graph.  The
 * resident path optimises a RESIDENT-SIZED graph -- at most 1024 vertices and at most 4096 edges -- from start to end inside ONE launch
 * by ONE workgroup, and a batch of such graphs (many trackers' local maps, several edge subsets of one graph) by one workgroup each in
 * the same launch: dvo_hip_graph_optimize_batch.  A graph whose solve fits 144 KB of LDS (114 n + 36 m doubles: about 100 vertices with
 * 125 edges) is solved out of LDS; a larger resident-sized one from memory, where a single graph is slower than on the launch path
 * (profiles/pose_graph.md).  Option "graph_resident" (dvo_hip_set_option; default 0): 1 = dvo_hip_graph_optimize
 * takes the resident path for a resident-sized graph, as a batch of one; a larger graph takes the launch path as before.  Counter
 * "graph_resident_solves" (dvo_hip_get_counter): graphs optimised by the resident path.
 * Errors: DVO_HIP_ERR_INVALID for from == to, an index out of range, a non-finite entry, delta < 0, n <= 0, or a graph of another
 * context -- checked before anything is launched or changed; DVO_HIP_ERR_NO_DEVICE without a gfx950, as everywhere else. */
typedef struct dvo_hip_graph dvo_hip_graph;

/* status of an optimisation (dvo_hip_graph_report::status) */
#define DVO_HIP_GRAPH_CONVERGED 0          /* an accepted step lowered the cost by less than min_relative_decrease, or the gradient is zero */
#define DVO_HIP_GRAPH_ITERATION_CAP 1
#define DVO_HIP_GRAPH_DAMPING_OVERFLOW 2
#define DVO_HIP_GRAPH_STALLED 3            /* ten rejected trials in a row (g2o's maxTrialsAfterFailure) */
#define DVO_HIP_GRAPH_NOTHING_TO_DO 4      /* no free vertex or no edge: the graph optimises to itself */
/* status of one conjugate-gradient solve (dvo_hip_graph_iteration::cg_status) */
#define DVO_HIP_GRAPH_CG_CONVERGED 1
#define DVO_HIP_GRAPH_CG_BREAKDOWN 2       /* p^T A p or r^T z not positive and finite: the trial is rejected, no pose takes a NaN */
#define DVO_HIP_GRAPH_CG_CHOLESKY 3        /* a vertex's diagonal block plus damping has no Cholesky factor */
#define DVO_HIP_GRAPH_CG_ZERO_RHS 4
#define DVO_HIP_GRAPH_CG_ITERATION_CAP 5   /* the step the cap left is used, as g2o uses it */

typedef struct dvo_hip_graph_params {
  int32_t max_iterations;          /* Levenberg-Marquardt trials, accepted or not (default 50) */
  int32_t cg_max_iterations;       /* default 200 */
  double cg_tolerance;             /* relative residual in the M^-1 norm, sqrt(r^T M^-1 r / b^T M^-1 b) (default 1e-8) */
  double min_relative_decrease;    /* default 1e-9 */
  double initial_damping_scale;    /* g2o's tau: lambda_0 = tau * the largest diagonal entry of H (default 1e-5) */
  double reserved[3];
} dvo_hip_graph_params;

typedef struct dvo_hip_graph_iteration {
  double cost_before, cost_after;  /* sum of rho at the estimate and at the stepped poses */
  double damping;                  /* lambda of this trial */
  int32_t cg_iterations, cg_status, accepted, reserved;
} dvo_hip_graph_iteration;

typedef struct dvo_hip_graph_report {
  int32_t status, iterations, accepted, cg_iterations;
  double initial_cost, final_cost, final_damping;
  double reserved[4];
} dvo_hip_graph_report;

int dvo_hip_graph_create(dvo_hip_context* ctx, dvo_hip_graph** out);
void dvo_hip_graph_destroy(dvo_hip_context* ctx, dvo_hip_graph* graph);
/* The vertices (g2o: addVertex + setEstimate + setFixed, keyframe_graph.cpp:702-739, local_map.cpp:88-98).  fixed: n bytes, non-zero =
 * held, or null.  Drops the edges of an earlier set. */
int dvo_hip_graph_set_vertices(dvo_hip_context* ctx, dvo_hip_graph* graph, int n, const double* poses, const unsigned char* fixed_or_null);
/* a new estimate for the same n vertices and the same edges (setEstimate, local_map.cpp:153-168) */
int dvo_hip_graph_set_poses(dvo_hip_context* ctx, dvo_hip_graph* graph, int n, const double* poses);
/* The edges, replacing all earlier ones (addEdge, keyframe_graph.cpp:620-636; local_map.cpp:104-116).  delta: the Cauchy kernel's
 * width per edge, 0 = no kernel; null = none has one.  m = 0 removes them all.  The per-vertex incidence lists are built here. */
int dvo_hip_graph_set_edges(dvo_hip_context* ctx, dvo_hip_graph* graph, int m, const int32_t* from, const int32_t* to, const double* measurements,
                            const double* information, const double* delta_or_null);
dvo_hip_graph_params dvo_hip_graph_params_default(void);
/* initializeOptimization + optimize (keyframe_graph.cpp:475-489, local_map.cpp:208-213).  params null = the defaults.  records (may be
 * null): one per trial, the first max_records of them.  The estimate becomes the last accepted one. */
int dvo_hip_graph_optimize(dvo_hip_context* ctx, dvo_hip_graph* graph, const dvo_hip_graph_params* params, dvo_hip_graph_report* out,
                           dvo_hip_graph_iteration* records_or_null, int max_records);
/* n_graphs resident-sized graphs of this context, each given once, optimised in ONE launch, one workgroup each; every graph is left as
 * dvo_hip_graph_optimize with its parameters would have left it, bit for bit, whatever its place in the batch.  params: n_graphs of
 * them, null = the defaults for all.  reports: n_graphs.  records (may be null): graph i's at records[i * max_records ...], the first
 * max_records of its trials.  DVO_HIP_ERR_INVALID, before anything is launched or changed: n_graphs <= 0, a null entry, a graph of
 * another context, the same graph twice, a graph without vertices or beyond 1024 vertices / 4096 edges, a parameter set
 * dvo_hip_graph_optimize would refuse, null reports, max_records < 0, max_records > 0 without records. */
int dvo_hip_graph_optimize_batch(dvo_hip_context* ctx, int n_graphs, dvo_hip_graph* const* graphs, const dvo_hip_graph_params* params_or_null,
                                 dvo_hip_graph_report* reports, dvo_hip_graph_iteration* records_or_null, int max_records);
int dvo_hip_graph_get_poses(dvo_hip_context* ctx, dvo_hip_graph* graph, int n, double* poses_out);
/* chi2 = e^T Omega e and the kernel's weight (1 without a kernel) of every edge at the current estimate: what
 * removeOutlierConstraints thresholds (keyframe_graph.cpp:643-674) */
int dvo_hip_graph_edge_stats(dvo_hip_context* ctx, dvo_hip_graph* graph, int m, double* chi2_out, double* weight_out);
/* One stage each, results to the host -- the test hooks, as dvo_hip_level_iteration is for match().  Every output may be null.
 * linearise: per edge the error (m x 6), chi2, weight, the blocks w Ji^T Omega Ji | w Ji^T Omega Jj | w Jj^T Omega Jj (m x 108, row-major
 * 6 x 6 each), the gradient parts -w Ji^T Omega e | -w Jj^T Omega e (m x 12), and the cost.  multiply: linearises, gathers, factorises
 * D_v + damping I, then y = (H + damping I) p over the free vertices for the given p (n x 6): y (n x 6), p^T y, the gathered diagonal
 * blocks (n x 36), right-hand side (n x 6) and block inverses (n x 36). */
int dvo_hip_graph_linearise(dvo_hip_context* ctx, dvo_hip_graph* graph, double* error_out, double* chi2_out, double* weight_out, double* blocks_out,
                            double* gradient_out, double* cost_out);
int dvo_hip_graph_multiply(dvo_hip_context* ctx, dvo_hip_graph* graph, double damping, const double* p, double* y_out, double* pty_out,
                           double* diagonal_out, double* rhs_out, double* inverse_out);

const char* dvo_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DVO_HIP_H_ */
