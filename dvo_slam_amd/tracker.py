"""Host-side mirror of the reference's dvo_core class API for the alignment hot path.

Same names, argument meaning and error behaviour as
  dvo::DenseTracker / Config / Result / Stats      dvo_core/include/dvo/dense_tracking.h:36-215
  dvo::core::RgbdCameraPyramid / RgbdImagePyramid  dvo_core/include/dvo/core/rgbd_image.h:99-262
  dvo::core::PointSelection                         dvo_core/include/dvo/core/point_selection.h:69-99
but every pixel operation runs on the MI355X through libdvo_hip.so (include/dvo_hip.h).  The
C++ facade with the identical role for C++ callers lives in include/dvo/.

This file only imports.  The code lives in one module per subject, each importing only from those listed before it.
"""
# flake8: noqa: F401
from ._lib import DvoHipError
from .context import Context, default_context
from .api_types import Config, IterationStats, LevelStats, Result, Stats, TERMINATION, _RESULT_DTYPE
from .planes import FrameSet, PinnedRawPlanes, device_pointer_array, _handles
from .attachments import (clear_colour_batch, clear_depth_filter_batch, clear_depth_rig_batch, clear_lens_batch, clear_selection_batch, depth_filter_default,
                          depth_filter_struct, depth_rig_struct, lens_struct, set_colour_batch, set_depth_filter_batch, set_depth_rig_batch, set_lens_batch,
                          set_level_selection, set_selection_batch, _colour_sources)
from .frames import RgbdCameraPyramid, RgbdImage, RgbdImagePyramid
from .ingest import (prepare_roles_batch, update_colour_device_batch, update_colour_host_batch, update_f32_device_batch, update_f32_host_batch,
                     update_raw_device_batch, update_raw_host_batch, upload_wait)
from .frame_calls import (COVIS_DTYPE, COVIS_MAX_PAIRS, covis_params_struct, covisibility_batch, covisibility_matrix, loop_closure_candidates, normals_batch,
                          overlap, radius_set, warp_forward_batch, warp_inverse_batch, warp_params_struct, world_points_batch, _covis_args, _map_frames_args,
                          _warp_args)
from .codebook import (CODE_MASKED, CODE_MATCH_DTYPE, CODE_MAX_CAPACITY, CODE_MAX_K, CODE_MAX_QUERIES, CODE_NONE, CodebookLogic, FERN_DTYPE,
                       KeyframeCodebook, loop_closure_candidates_by_appearance, relocalisation_candidates)
from .keyframe_map import KeyframeMap, RENDER_DEFAULTS, render_params_struct, _render_view_args, _rehash_capacity
from .pose_graph import GRAPH_DEFAULTS, PoseGraph, graph_params_struct, select_outliers
from .dense_tracker import DenseTracker, PointSelection
