"""ctypes binding of libdvo_hip.so (the C-ABI declared in include/dvo_hip.h).

There is no CPU fallback: if the shared library is missing or no gfx950 device is usable, every
entry point raises.  The library is built in-tree by `dvo_slam_amd.build()` (hipcc, gfx950).
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DVO_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libdvo_hip.so")   # override: A/B measurements of two builds
CSRC = os.path.join(_HERE, "csrc")

MAX_LEVELS = 8

OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_CAPACITY = 0, -1, -2, -3, -4


class DvoHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libdvo_hip error %d: %s" % (code, message))
        self.code = code


class Config(C.Structure):
    """dvo_hip_config <-> dvo::DenseTracker::Config (dvo_core/include/dvo/dense_tracking.h:42-69)."""
    _fields_ = [
        ("first_level", C.c_int32), ("last_level", C.c_int32),
        ("max_iterations_per_level", C.c_int32), ("use_initial_estimate", C.c_int32),
        ("precision", C.c_double), ("mu", C.c_double),
        ("intensity_derivative_threshold", C.c_float), ("depth_derivative_threshold", C.c_float),
    ]


class IterationStats(C.Structure):
    _fields_ = [
        ("id", C.c_int32), ("valid_constraints", C.c_int32),
        ("tdist_loglik", C.c_double), ("tdist_mean", C.c_double * 2), ("tdist_precision", C.c_double * 4),
        ("prior_loglik", C.c_double), ("increment", C.c_double * 6), ("information", C.c_double * 36),
    ]


class LevelStats(C.Structure):
    _fields_ = [("id", C.c_int32), ("max_valid_pixels", C.c_int32), ("valid_pixels", C.c_int32),
                ("termination", C.c_int32), ("n_iterations", C.c_int32), ("first_iteration_index", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("information", C.c_double * 36), ("loglik", C.c_double),
                ("n_levels", C.c_int32), ("n_iterations_total", C.c_int32),
                ("entropy", C.c_double), ("condition_number", C.c_double), ("constraint_ratio", C.c_double),
                ("constraint_ratio_accepted", C.c_double)]


class IterationOut(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_selected", C.c_int32), ("scale_cov", C.c_float * 3), ("precision", C.c_float * 4),
                ("neg_loglik", C.c_double), ("A", C.c_double * 36), ("b", C.c_double * 6), ("sum_w", C.c_double)]


class Lens(C.Structure):
    """dvo_hip_lens: K_raw = fx fy ox oy of the raw image, D = k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV / ROS plumb_bob, rational_polynomial)."""
    _fields_ = [("K_raw", C.c_float * 4), ("D", C.c_float * 8), ("rectify_depth", C.c_int32), ("reserved", C.c_int32)]


class DepthRig(C.Structure):
    """dvo_hip_depth_rig: K_depth = fx fy ox oy of the depth sensor's image, T = row-major 3 x 4 [R | t], depth sensor -> colour camera."""
    _fields_ = [("K_depth", C.c_float * 4), ("T", C.c_float * 12), ("reserved", C.c_int32 * 2)]


class MapStats(C.Structure):
    """struct dvo_hip_map_stats: the statistics of a keyframe map (dvo_hip_map_stats)."""
    _fields_ = [("occupied", C.c_uint64), ("points", C.c_uint64), ("dropped", C.c_uint64), ("out_of_range", C.c_uint64),
                ("unusable", C.c_uint64), ("over_limit", C.c_uint64), ("capacity", C.c_uint64), ("updates", C.c_uint64),
                ("vacant", C.c_uint64), ("removed", C.c_uint64), ("unmatched", C.c_uint64), ("reserved", C.c_uint64 * 5)]


class RenderParams(C.Structure):
    """dvo_hip_render_params: how a view of a keyframe map is rendered (dvo_hip_map_render)."""
    _fields_ = [("min_depth", C.c_float), ("max_depth", C.c_float), ("splat", C.c_float), ("max_splat", C.c_int32),
                ("min_points", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class WarpParams(C.Structure):
    """dvo_hip_warp_params: how frames are warped under a pose (dvo_hip_frames_warp_inverse, dvo_hip_frames_warp_forward)."""
    _fields_ = [("mode", C.c_int32), ("occlusion_margin", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("reserved", C.c_uint32 * 4)]


# DVO_HIP_WARP_*: the footprint of a forward warp
WARP_MODES = {"nearest": 0, "splat": 1}


class CovisParams(C.Structure):
    """dvo_hip_covis_params: how the pixels of a keyframe pair are classified (dvo_hip_frames_covisibility)."""
    _fields_ = [("depth_tolerance", C.c_float), ("depth_tolerance_rel", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("reserved", C.c_uint32 * 4)]


class GraphParams(C.Structure):
    """dvo_hip_graph_params: the schedule of a pose-graph optimisation (dvo_hip_graph_optimize)."""
    _fields_ = [("max_iterations", C.c_int32), ("cg_max_iterations", C.c_int32), ("cg_tolerance", C.c_double),
                ("min_relative_decrease", C.c_double), ("initial_damping_scale", C.c_double), ("reserved", C.c_double * 3)]


class GraphIteration(C.Structure):
    """dvo_hip_graph_iteration: one Levenberg-Marquardt trial."""
    _fields_ = [("cost_before", C.c_double), ("cost_after", C.c_double), ("damping", C.c_double), ("cg_iterations", C.c_int32),
                ("cg_status", C.c_int32), ("accepted", C.c_int32), ("reserved", C.c_int32)]


class GraphReport(C.Structure):
    """dvo_hip_graph_report: what an optimisation did."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("accepted", C.c_int32), ("cg_iterations", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_damping", C.c_double), ("reserved", C.c_double * 4)]


# DVO_HIP_GRAPH_*: the status of an optimisation, and DVO_HIP_GRAPH_CG_*: of one conjugate-gradient solve
GRAPH_STATUS = {0: "converged", 1: "iteration_cap", 2: "damping_overflow", 3: "stalled", 4: "nothing_to_do"}
GRAPH_CG_STATUS = {1: "converged", 2: "breakdown", 3: "cholesky", 4: "zero_rhs", 5: "iteration_cap"}
GRAPH_MAX_VERTICES, GRAPH_MAX_EDGES = 1 << 20, 1 << 22
# a resident-sized graph (pose_graph.h: kPgResidentMaxVertices, kPgResidentMaxEdges): what dvo_hip_graph_optimize_batch takes
GRAPH_RESIDENT_MAX_VERTICES, GRAPH_RESIDENT_MAX_EDGES = 1024, 4096

class DepthFilter(C.Structure):
    """dvo_hip_depth_filter: smoothing window (radius, sigma_space), noise model sigma(z) = noise_a + noise_b z^2 and its gate, edge
    rejection (edge_radius, tau(z) = edge_abs + edge_rel z), hole-border erosion (hole_radius)."""
    _fields_ = [("radius", C.c_int32), ("sigma_space", C.c_float), ("noise_a", C.c_float), ("noise_b", C.c_float), ("gate", C.c_float),
                ("edge_radius", C.c_int32), ("edge_abs", C.c_float), ("edge_rel", C.c_float), ("hole_radius", C.c_int32),
                ("reserved", C.c_int32 * 2)]


# every symbol include/dvo_hip.h declares (tests check that the library exports all of them)
EXPORTS = [
    "dvo_hip_context_create", "dvo_hip_context_destroy", "dvo_hip_last_error", "dvo_hip_context_stream",
    "dvo_hip_device_count", "dvo_hip_frame_create_f32", "dvo_hip_frame_create_raw", "dvo_hip_frame_create_raw_device",
    "dvo_hip_frame_update_raw_device", "dvo_hip_frames_update_raw_device", "dvo_hip_frames_update_raw", "dvo_hip_frames_update_raw_device_as", "dvo_hip_frames_update_raw_as", "dvo_hip_upload_wait",
    "dvo_hip_host_alloc", "dvo_hip_host_free", "dvo_hip_frames_prepare", "dvo_hip_frame_destroy", "dvo_hip_frame_info", "dvo_hip_frame_device_planes", "dvo_hip_frame_download_plane", "dvo_hip_frame_select",
    "dvo_hip_match", "dvo_hip_match_batch", "dvo_hip_level_iteration", "dvo_hip_time_residual_kernel", "dvo_hip_time_stream_mix",
    "dvo_hip_set_option", "dvo_hip_get_counter", "dvo_hip_version",
    "dvo_hip_frames_update_raw_device_as_ex", "dvo_hip_frames_update_raw_as_ex", "dvo_hip_flush_deferred", "dvo_hip_context_device",
    "dvo_hip_frame_create_colour", "dvo_hip_frame_create_colour_device", "dvo_hip_frames_update_colour_device_as_ex",
    "dvo_hip_frames_update_colour_as_ex", "dvo_hip_frames_set_selection", "dvo_hip_frames_clear_selection", "dvo_hip_frame_set_level_selection",
    "dvo_hip_comm_get_unique_id", "dvo_hip_comm_create", "dvo_hip_comm_destroy", "dvo_hip_comm_rank", "dvo_hip_comm_size",
    "dvo_hip_comm_last_error", "dvo_hip_gather_records_begin", "dvo_hip_gather_records_end", "dvo_hip_gather_records",
    "dvo_hip_frame_create_f32_device", "dvo_hip_frames_update_f32_device_as_ex", "dvo_hip_frames_update_f32_as_ex",
    "dvo_hip_frames_update_colour_f32depth_device_as_ex", "dvo_hip_frames_update_colour_f32depth_as_ex",
    "dvo_hip_frames_set_lens", "dvo_hip_frames_clear_lens",
    "dvo_hip_frames_set_depth_rig", "dvo_hip_frames_clear_depth_rig",
    "dvo_hip_frames_set_depth_filter", "dvo_hip_frames_clear_depth_filter", "dvo_hip_depth_filter_default",
    "dvo_hip_map_create", "dvo_hip_map_destroy", "dvo_hip_map_clear", "dvo_hip_map_insert", "dvo_hip_map_stats", "dvo_hip_map_extract",
    "dvo_hip_frames_world_points", "dvo_hip_map_remove", "dvo_hip_map_move", "dvo_hip_map_rehash",
    "dvo_hip_render_params_default", "dvo_hip_map_render", "dvo_hip_map_render_frames", "dvo_hip_time_map_render",
    "dvo_hip_frames_set_colour", "dvo_hip_frames_clear_colour", "dvo_hip_frame_download_colour", "dvo_hip_map_create_ex",
    "dvo_hip_map_extract_colour", "dvo_hip_map_render_colour",
    "dvo_hip_map_info", "dvo_hip_map_merge", "dvo_hip_map_move_submaps", "dvo_hip_map_export", "dvo_hip_map_merge_records",
    "dvo_hip_frames_normals", "dvo_hip_map_extract_normals", "dvo_hip_map_render_normals", "dvo_hip_map_export_ex",
    "dvo_hip_map_merge_records_ex",
    "dvo_hip_warp_params_default", "dvo_hip_frames_warp_inverse", "dvo_hip_frames_warp_forward",
    "dvo_hip_covis_params_default", "dvo_hip_frames_covisibility",
    "dvo_hip_codebook_create", "dvo_hip_codebook_destroy", "dvo_hip_codebook_clear", "dvo_hip_codebook_info", "dvo_hip_codebook_ferns",
    "dvo_hip_frames_encode", "dvo_hip_codebook_add_frames", "dvo_hip_codebook_add_codes", "dvo_hip_codebook_remove",
    "dvo_hip_codebook_read_codes", "dvo_hip_codebook_query_frames", "dvo_hip_codebook_query_codes", "dvo_hip_codebook_query_ids",
    "dvo_hip_graph_create", "dvo_hip_graph_destroy", "dvo_hip_graph_set_vertices", "dvo_hip_graph_set_poses", "dvo_hip_graph_set_edges",
    "dvo_hip_graph_params_default", "dvo_hip_graph_optimize", "dvo_hip_graph_get_poses", "dvo_hip_graph_edge_stats",
    "dvo_hip_graph_linearise", "dvo_hip_graph_multiply", "dvo_hip_graph_optimize_batch",
]

ROLE_CURRENT, ROLE_REFERENCE = 0, 1
INGEST_DEFER, INGEST_NO_RAW_COPY = 1, 2
# DVO_HIP_PIXEL_*: the formats of an 8-bit colour plane, and their bytes per pixel
PIXEL_FORMATS = {"bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4}
PIXEL_CHANNELS = {"bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}
# ... and of the image plane that comes with a float depth plane (dvo_hip_frames_update_colour_f32depth*): grey8 as well
MIXED_PIXEL_FORMATS = dict(PIXEL_FORMATS, grey8=0)
MIXED_PIXEL_CHANNELS = dict(PIXEL_CHANNELS, grey8=1)
# the raw sensor formats every pixel_format argument takes as well (dvo_hip.h, DVO_HIP_PIXEL_BAYER_* / _YUYV8 / _UYVY8): Bayer mosaics,
# named by the 2 x 2 block at the image's top-left corner, and YUV 4:2:2; their bytes per pixel
SENSOR_PIXEL_FORMATS = {"bayer_rggb8": 16, "bayer_bggr8": 17, "bayer_gbrg8": 18, "bayer_grbg8": 19, "yuyv8": 20, "uyvy8": 21}
SENSOR_PIXEL_CHANNELS = {"bayer_rggb8": 1, "bayer_bggr8": 1, "bayer_gbrg8": 1, "bayer_grbg8": 1, "yuyv8": 2, "uyvy8": 2}
PIXEL_F32 = 5
DEPTH_U16, DEPTH_F32 = 0, 1
DEPTH_FORMATS = {"u16": DEPTH_U16, "f32": DEPTH_F32}
MAP_COLOUR = 1   # DVO_HIP_MAP_COLOUR
MAP_NORMALS = 4  # DVO_HIP_MAP_NORMALS (2 stays an unknown flag)
# a voxel record of dvo_hip_map_export / dvo_hip_map_merge_records (32 bytes: cloud_map.h, MapSlot) and its colour record (16: MapColourSlot)
MAP_RECORD = [("key", "<u8"), ("n", "<u4"), ("sx", "<u4"), ("sy", "<u4"), ("sz", "<u4"), ("si", "<u4"), ("pad", "<u4")]
MAP_COLOUR_RECORD = [("sr", "<u4"), ("sg", "<u4"), ("sb", "<u4"), ("pad", "<u4")]
# ... and its normal record (16: cloud_normal.h, MapNormalSlot; dvo_hip_map_export_ex / dvo_hip_map_merge_records_ex)
MAP_NORMAL_RECORD = [("snx", "<u4"), ("sny", "<u4"), ("snz", "<u4"), ("nn", "<u4")]
# the record of one keyframe pair (32 bytes: dvo_hip_covis_record; dvo_hip_frames_covisibility)
COVIS_RECORD = [("valid", "<u4"), ("in_view", "<u4"), ("unknown", "<u4"), ("occluded", "<u4"), ("seen_through", "<u4"), ("consistent", "<u4"),
                ("photo", "<u8")]
# a fern and a result record of a keyframe code book (16 and 8 bytes: dvo_hip_fern, dvo_hip_code_match; dvo_hip_codebook_*)
FERN_RECORD = [("u", "<u2"), ("v", "<u2"), ("u2", "<u2"), ("v2", "<u2"), ("t_i", "<f4"), ("t_z", "<f4")]
CODE_MATCH_RECORD = [("id", "<u4"), ("distance", "<u4")]
COMM_ID_BYTES = 128


def build(force=False):
    """Compile libdvo_hip.so for gfx950 with the committed Makefile (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-s", "-j4"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(cmd)
    # the replay driver (g++ only) links the library just built
    subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(CSRC), "apps"), "-s"])
    return LIB_PATH


_lib = None


def lib():
    """Load libdvo_hip.so. Raises if it has not been built -- never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DvoHipError(ERR_NO_DEVICE, "%s not built; run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.dvo_hip_context_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.dvo_hip_context_destroy.argtypes = [vp]
    L.dvo_hip_context_destroy.restype = None
    L.dvo_hip_last_error.argtypes = [vp]
    L.dvo_hip_last_error.restype = C.c_char_p
    L.dvo_hip_context_stream.argtypes = [vp]
    L.dvo_hip_context_stream.restype = vp
    L.dvo_hip_device_count.restype = C.c_int
    L.dvo_hip_frame_create_f32.argtypes = [vp, C.c_int, C.c_int, fp, fp, fp, C.c_int, C.POINTER(vp)]
    L.dvo_hip_frame_create_raw.argtypes = [vp, C.c_int, C.c_int, fp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.c_float,
                                           C.c_int, C.POINTER(vp)]
    L.dvo_hip_frame_create_raw_device.argtypes = [vp, C.c_int, C.c_int, fp, vp, vp, C.c_float, C.c_int, C.POINTER(vp)]
    L.dvo_hip_frame_update_raw_device.argtypes = [vp, vp, vp, vp, C.c_float]
    L.dvo_hip_frames_update_raw_device.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_float]
    L.dvo_hip_frames_update_raw.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_float]
    L.dvo_hip_frames_update_raw_device_as.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_float, C.c_int, C.POINTER(Config)]
    L.dvo_hip_frames_update_raw_as.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_float, C.c_int, C.POINTER(Config)]
    L.dvo_hip_upload_wait.argtypes = [vp]
    L.dvo_hip_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.dvo_hip_host_free.argtypes = [vp, vp]
    L.dvo_hip_host_free.restype = None
    L.dvo_hip_frames_prepare.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_int, C.POINTER(Config)]
    L.dvo_hip_frame_destroy.argtypes = [vp, vp]
    L.dvo_hip_frame_destroy.restype = None
    L.dvo_hip_frame_info.argtypes = [vp, C.c_int, ip, ip, fp]
    if hasattr(L, "dvo_hip_frame_device_planes"):
        L.dvo_hip_frame_device_planes.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.dvo_hip_frame_download_plane.argtypes = [vp, vp, C.c_int, C.c_int, fp]
    L.dvo_hip_frame_select.argtypes = [vp, vp, C.c_int, C.c_float, C.c_float, ip, C.POINTER(C.c_uint8)]
    L.dvo_hip_match.argtypes = [vp, vp, vp, C.POINTER(Config), C.POINTER(Result), C.POINTER(LevelStats), C.c_int,
                                C.POINTER(IterationStats), C.c_int]
    L.dvo_hip_match_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(Config), C.POINTER(Result),
                                      C.POINTER(LevelStats), C.c_int, C.POINTER(IterationStats), C.c_int]
    L.dvo_hip_level_iteration.argtypes = [vp, vp, vp, C.c_int, C.c_float, C.c_float, fp, fp, C.c_int,
                                          C.POINTER(IterationOut), fp]
    L.dvo_hip_time_residual_kernel.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, fp]
    L.dvo_hip_time_stream_mix.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, fp]
    L.dvo_hip_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.dvo_hip_get_counter.argtypes = [vp, C.c_char_p, C.POINTER(C.c_longlong)]
    L.dvo_hip_version.restype = C.c_char_p
    L.dvo_hip_frames_update_raw_device_as_ex.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_float, C.c_int, C.POINTER(Config), C.c_uint]
    L.dvo_hip_frames_update_raw_as_ex.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_float, C.c_int, C.POINTER(Config), C.c_uint]
    L.dvo_hip_frame_create_colour.argtypes = [vp, C.c_int, C.c_int, fp, vp, C.c_int, C.c_size_t, C.POINTER(C.c_uint16), C.c_float, C.c_int,
                                              C.POINTER(vp)]
    L.dvo_hip_frame_create_colour_device.argtypes = [vp, C.c_int, C.c_int, fp, vp, C.c_int, C.c_size_t, vp, C.c_float, C.c_int, C.POINTER(vp)]
    L.dvo_hip_frames_update_colour_device_as_ex.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_size_t, C.POINTER(vp),
                                                            C.c_float, C.c_int, C.POINTER(Config), C.c_uint]
    L.dvo_hip_frames_update_colour_as_ex.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_size_t, C.POINTER(vp), C.c_float,
                                                     C.c_int, C.POINTER(Config), C.c_uint]
    L.dvo_hip_frame_create_f32_device.argtypes = [vp, C.c_int, C.c_int, fp, vp, vp, C.c_int, C.POINTER(vp)]
    L.dvo_hip_frames_update_f32_device_as_ex.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_size_t, C.POINTER(vp), C.c_size_t,
                                                         C.c_float, C.c_int, C.POINTER(Config), C.c_uint]
    L.dvo_hip_frames_update_f32_as_ex.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_size_t, C.POINTER(vp), C.c_size_t, C.c_float,
                                                  C.c_int, C.POINTER(Config), C.c_uint]
    L.dvo_hip_frames_update_colour_f32depth_device_as_ex.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_size_t,
                                                                     C.POINTER(vp), C.c_size_t, C.c_float, C.c_int, C.POINTER(Config), C.c_uint]
    L.dvo_hip_frames_update_colour_f32depth_as_ex.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_size_t, C.POINTER(vp),
                                                              C.c_size_t, C.c_float, C.c_int, C.POINTER(Config), C.c_uint]
    L.dvo_hip_flush_deferred.argtypes = [vp]
    L.dvo_hip_frames_set_selection.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_size_t, C.c_int, C.c_float, C.c_float]
    L.dvo_hip_frames_clear_selection.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.dvo_hip_frame_set_level_selection.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_uint8)]
    if hasattr(L, "dvo_hip_frames_set_lens"):   # (DVO_HIP_LIBRARY may name an older build for an A/B: it has no lens, a call raises AttributeError)
        L.dvo_hip_frames_set_lens.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(Lens)]
        L.dvo_hip_frames_clear_lens.argtypes = [vp, C.c_int, C.POINTER(vp)]
    if hasattr(L, "dvo_hip_frames_set_depth_rig"):   # (likewise: an older build has no depth rig)
        L.dvo_hip_frames_set_depth_rig.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(DepthRig)]
        L.dvo_hip_frames_clear_depth_rig.argtypes = [vp, C.c_int, C.POINTER(vp)]
    if hasattr(L, "dvo_hip_frames_set_depth_filter"):   # (likewise: an older build has no depth filter)
        L.dvo_hip_frames_set_depth_filter.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(DepthFilter)]
        L.dvo_hip_frames_clear_depth_filter.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.dvo_hip_depth_filter_default.argtypes = []
        L.dvo_hip_depth_filter_default.restype = DepthFilter
    if hasattr(L, "dvo_hip_map_create"):   # (likewise: an older build has no keyframe map)
        dp = C.POINTER(C.c_double)
        L.dvo_hip_map_create.argtypes = [vp, C.c_float, C.c_size_t, C.POINTER(vp)]
        L.dvo_hip_map_destroy.argtypes = [vp, vp]
        L.dvo_hip_map_destroy.restype = None
        L.dvo_hip_map_clear.argtypes = [vp, vp]
        L.dvo_hip_map_insert.argtypes = [vp, vp, C.c_int, C.POINTER(vp), dp, C.c_int, C.c_float, C.c_float]
        L.dvo_hip_map_stats.argtypes = [vp, vp, C.POINTER(MapStats)]
        L.dvo_hip_map_extract.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
        L.dvo_hip_frames_world_points.argtypes = [vp, C.c_int, C.POINTER(vp), dp, C.c_int, C.c_float, C.c_float, C.POINTER(vp), C.c_int]
    if hasattr(L, "dvo_hip_map_remove"):   # (likewise: an older build's map can only grow)
        L.dvo_hip_map_remove.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_double), C.c_int, C.c_float, C.c_float]
        L.dvo_hip_map_move.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_float, C.c_float]
        L.dvo_hip_map_rehash.argtypes = [vp, vp, C.c_size_t]
    if hasattr(L, "dvo_hip_map_render"):   # (likewise: an older build renders no views)
        dp, rp = C.POINTER(C.c_double), C.POINTER(RenderParams)
        L.dvo_hip_render_params_default.argtypes = []
        L.dvo_hip_render_params_default.restype = RenderParams
        L.dvo_hip_map_render.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, fp, dp, rp, C.POINTER(vp), C.POINTER(vp), C.c_int]
        L.dvo_hip_map_render_frames.argtypes = [vp, vp, C.c_int, C.POINTER(vp), dp, rp, C.c_int, C.POINTER(Config), C.c_uint]
        L.dvo_hip_time_map_render.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, fp, dp, rp, C.c_int, fp]
    if hasattr(L, "dvo_hip_frames_set_colour"):   # (likewise: an older build's map is grey)
        dp, rp = C.POINTER(C.c_double), C.POINTER(RenderParams)
        L.dvo_hip_frames_set_colour.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_size_t, C.c_int]
        L.dvo_hip_frames_clear_colour.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.dvo_hip_frame_download_colour.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_uint32)]
        L.dvo_hip_map_create_ex.argtypes = [vp, C.c_float, C.c_size_t, C.c_uint, C.POINTER(vp)]
        L.dvo_hip_map_extract_colour.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
        L.dvo_hip_map_render_colour.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, fp, dp, rp, C.POINTER(vp), C.POINTER(vp), C.c_int]
    if hasattr(L, "dvo_hip_map_merge"):   # (likewise: an older build's maps do not merge)
        dp, mp = C.POINTER(C.c_double), C.POINTER(vp)
        L.dvo_hip_map_info.argtypes = [vp, vp, fp, C.POINTER(C.c_uint), C.POINTER(C.c_uint64)]
        L.dvo_hip_map_merge.argtypes = [vp, vp, C.c_int, mp, ip, dp]
        L.dvo_hip_map_move_submaps.argtypes = [vp, vp, C.c_int, mp, dp, dp]
        L.dvo_hip_map_export.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
        L.dvo_hip_map_merge_records.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_int, C.c_float, C.c_int, dp]
    if hasattr(L, "dvo_hip_frames_normals"):   # (likewise: an older build's map holds no normals)
        dp, rp = C.POINTER(C.c_double), C.POINTER(RenderParams)
        L.dvo_hip_frames_normals.argtypes = [vp, C.c_int, C.POINTER(vp), dp, C.c_int, C.c_float, C.c_float, C.POINTER(vp), C.c_int]
        L.dvo_hip_map_extract_normals.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
        L.dvo_hip_map_render_normals.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, fp, dp, rp, C.POINTER(vp), C.POINTER(vp), C.c_int]
        L.dvo_hip_map_export_ex.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
        L.dvo_hip_map_merge_records_ex.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_int, C.c_float, C.c_int, dp]
    if hasattr(L, "dvo_hip_frames_warp_inverse"):   # (likewise: an older build warps no frames)
        dp, wp, pp = C.POINTER(C.c_double), C.POINTER(WarpParams), C.POINTER(vp)
        L.dvo_hip_warp_params_default.argtypes = []
        L.dvo_hip_warp_params_default.restype = WarpParams
        L.dvo_hip_frames_warp_inverse.argtypes = [vp, C.c_int, pp, pp, dp, C.c_int, wp, pp, pp, pp, C.c_int]
        L.dvo_hip_frames_warp_forward.argtypes = [vp, C.c_int, pp, dp, C.c_int, wp, pp, pp, C.c_int]
    if hasattr(L, "dvo_hip_frames_covisibility"):   # (likewise: an older build counts no covisibility)
        dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L.dvo_hip_covis_params_default.argtypes = []
        L.dvo_hip_covis_params_default.restype = CovisParams
        L.dvo_hip_frames_covisibility.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_int, i32p, i32p, dp, C.c_int, C.POINTER(CovisParams), vp, C.c_int]
    if hasattr(L, "dvo_hip_codebook_create"):   # (likewise: an older build keeps no code book)
        ip, u32p = C.POINTER(C.c_int), C.POINTER(C.c_uint32)
        L.dvo_hip_codebook_create.argtypes = [vp, C.c_int, C.c_int, C.c_uint64, vp, C.c_float, C.c_float, C.POINTER(vp)]
        L.dvo_hip_codebook_destroy.argtypes = [vp, vp]
        L.dvo_hip_codebook_destroy.restype = None
        L.dvo_hip_codebook_clear.argtypes = [vp, vp]
        L.dvo_hip_codebook_info.argtypes = [vp, vp, ip, ip, ip, ip]
        L.dvo_hip_codebook_ferns.argtypes = [vp, vp, vp]
        L.dvo_hip_frames_encode.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.c_int, vp, C.c_int]
        L.dvo_hip_codebook_add_frames.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.c_int, u32p]
        L.dvo_hip_codebook_add_codes.argtypes = [vp, vp, C.c_int, vp, C.c_int, u32p]
        L.dvo_hip_codebook_remove.argtypes = [vp, vp, C.c_int, u32p]
        L.dvo_hip_codebook_read_codes.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int]
        L.dvo_hip_codebook_query_frames.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.c_int, C.c_int, u32p, u32p, vp, vp, C.c_int]
        L.dvo_hip_codebook_query_codes.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, u32p, u32p, vp, vp, C.c_int]
        L.dvo_hip_codebook_query_ids.argtypes = [vp, vp, C.c_int, u32p, C.c_int, u32p, u32p, vp, vp, C.c_int]
    if hasattr(L, "dvo_hip_graph_create"):   # (likewise: an older build optimises no pose graph)
        dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L.dvo_hip_graph_create.argtypes = [vp, C.POINTER(vp)]
        L.dvo_hip_graph_destroy.argtypes = [vp, vp]
        L.dvo_hip_graph_destroy.restype = None
        L.dvo_hip_graph_set_vertices.argtypes = [vp, vp, C.c_int, dp, C.POINTER(C.c_uint8)]
        L.dvo_hip_graph_set_poses.argtypes = [vp, vp, C.c_int, dp]
        L.dvo_hip_graph_set_edges.argtypes = [vp, vp, C.c_int, i32p, i32p, dp, dp, dp]
        L.dvo_hip_graph_params_default.argtypes = []
        L.dvo_hip_graph_params_default.restype = GraphParams
        L.dvo_hip_graph_optimize.argtypes = [vp, vp, C.POINTER(GraphParams), C.POINTER(GraphReport), C.POINTER(GraphIteration), C.c_int]
        L.dvo_hip_graph_optimize_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(GraphParams), C.POINTER(GraphReport), C.POINTER(GraphIteration),
                                                   C.c_int]
        L.dvo_hip_graph_get_poses.argtypes = [vp, vp, C.c_int, dp]
        L.dvo_hip_graph_edge_stats.argtypes = [vp, vp, C.c_int, dp, dp]
        L.dvo_hip_graph_linearise.argtypes = [vp, vp, dp, dp, dp, dp, dp, dp]
        L.dvo_hip_graph_multiply.argtypes = [vp, vp, C.c_double, dp, dp, dp, dp, dp, dp]
    L.dvo_hip_context_device.argtypes = [vp]
    L.dvo_hip_comm_get_unique_id.argtypes = [vp]
    L.dvo_hip_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.dvo_hip_comm_destroy.argtypes = [vp]
    L.dvo_hip_comm_destroy.restype = None
    L.dvo_hip_comm_rank.argtypes = [vp]
    L.dvo_hip_comm_size.argtypes = [vp]
    L.dvo_hip_comm_last_error.argtypes = [vp]
    L.dvo_hip_comm_last_error.restype = C.c_char_p
    L.dvo_hip_gather_records_begin.argtypes = [vp, vp, C.c_size_t, C.c_size_t, ip]
    L.dvo_hip_gather_records_end.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.dvo_hip_gather_records.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t]
    _lib = L
    return L
