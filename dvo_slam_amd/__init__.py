"""dvo_slam_amd -- MI355X-native dense RGB-D alignment (the DenseTracker::match hot path of tum-vision/dvo_slam).

The product is libdvo_hip.so (hand-written HIP for gfx950 behind the C-ABI in include/dvo_hip.h);
this package is the thin Python mirror of the reference's class API used by the tests and bench.
"""
from ._lib import DvoHipError, build, lib, LIB_PATH  # noqa: F401
from .tracker import (Config, Context, DenseTracker, IterationStats, LevelStats, PointSelection, Result,  # noqa: F401
                      RgbdCameraPyramid, RgbdImage, RgbdImagePyramid, Stats, TERMINATION, default_context,
                      update_raw_device_batch, prepare_roles_batch, update_raw_host_batch, update_colour_device_batch, update_colour_host_batch, update_f32_device_batch, update_f32_host_batch, upload_wait, PinnedRawPlanes, FrameSet, device_pointer_array,
                      set_selection_batch, clear_selection_batch, set_level_selection, set_lens_batch, clear_lens_batch, lens_struct,
                      set_depth_rig_batch, clear_depth_rig_batch, depth_rig_struct, set_depth_filter_batch, clear_depth_filter_batch, depth_filter_struct, depth_filter_default, set_colour_batch, clear_colour_batch, KeyframeMap, world_points_batch, normals_batch,render_params_struct, warp_inverse_batch,
                      warp_forward_batch, warp_params_struct, COVIS_DTYPE, covis_params_struct, covisibility_batch, covisibility_matrix, overlap, radius_set,
                      loop_closure_candidates, FERN_DTYPE, CODE_MATCH_DTYPE, CODE_NONE, CODE_MASKED, CodebookLogic, KeyframeCodebook,
                      relocalisation_candidates, loop_closure_candidates_by_appearance, PoseGraph, graph_params_struct)
