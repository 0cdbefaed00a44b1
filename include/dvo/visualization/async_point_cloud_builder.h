// dvo/visualization/async_point_cloud_builder.h -- the world cloud of one keyframe, computed on the device.
// Stands in for dvo::visualization::AsyncPointCloudBuilder (dvo_core/include/dvo/visualization/async_point_cloud_builder.h:39-68,
// dvo_core/src/visualization/async_point_cloud_builder.cpp:61-110): BuildJob(image, pose).build() returns pose.cast<float>() * pointcloud
// plus intensity for every pixel of the image -- the ORGANISED cloud of level 0, NaN in x, y, z where the pixel has no usable depth
// (include/dvo_hip.h, dvo_hip_frames_world_points).  There is no PCL here: the cloud is dvo::compat::IntensityPointCloud, and the job
// holds the device pyramid instead of a host image.  Where the pyramid carries colour (RgbdImagePyramid::setColour; the reference's
// hasRgb() branch, async_point_cloud_builder.cpp:72-104) the cloud's rgba is filled with the level-0 colour of every pixel, 0xFFRRGGBB.
#pragma once

#include <vector>

#include "dvo/core/rgbd_image.h"

namespace dvo {
namespace visualization {

class AsyncPointCloudBuilder {
 public:
  typedef dvo::compat::IntensityPointCloud PointCloud;

  struct BuildJob {
    dvo::core::RgbdImagePyramid& image;
    const dvo::compat::Affine3d pose;

    BuildJob(dvo::core::RgbdImagePyramid& image_, const dvo::compat::Affine3d& pose_ = identity()) : image(image_), pose(pose_) {}

    PointCloud::Ptr build() {
      PointCloud::Ptr cloud(new PointCloud);
      dvo_hip_frame* one[1] = {image.device_frame()};
      int w = 0, h = 0;
      if (dvo_hip_frame_info(one[0], 0, &w, &h, 0) != DVO_HIP_OK) return cloud;
      double T[16];
      dvo::compat::affine_to_rowmajor(pose, T);
      std::vector<float> xyzi(size_t(w) * h * 4);
      float* out[1] = {xyzi.data()};
      if (!dvo::core::dvo_hip_check(image.device_context(),
                                    dvo_hip_frames_world_points(image.device_context(), 1, one, T, 0, 0.0f, INFINITY, out, 0),
                                    "dvo_hip_frames_world_points"))
        return cloud;
      cloud->resize(size_t(w) * h);
      cloud->width = size_t(w);
      cloud->height = size_t(h);
      for (size_t i = 0; i < cloud->size(); ++i) {
        cloud->x[i] = xyzi[4 * i];
        cloud->y[i] = xyzi[4 * i + 1];
        cloud->z[i] = xyzi[4 * i + 2];
        cloud->intensity[i] = xyzi[4 * i + 3];
      }
      if (image.hasColour()) {
        cloud->rgba.resize(cloud->size());
        if (!dvo::core::dvo_hip_check(image.device_context(), dvo_hip_frame_download_colour(image.device_context(), one[0], 0, cloud->rgba.data()),
                                      "dvo_hip_frame_download_colour")) {
          cloud->rgba.clear();
          return cloud;
        }
        for (size_t i = 0; i < cloud->size(); ++i) cloud->rgba[i] |= 0xFF000000u;   // (the frame's packed pixels have A = 0)
      }
      return cloud;
    }

   private:
    static dvo::compat::Affine3d identity() {
      dvo::compat::Affine3d T;
      T.setIdentity();
      return T;
    }
  };
};

}  // namespace visualization
}  // namespace dvo
