"""ctypes binding of librelpose_hip.so (the C ABI in include/relpose.h).

The product path has no CPU fallback: if the library is missing or a call is
made without a GPU, it raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RELPOSE_LIB_PATH") or os.path.join(HERE, "librelpose_hip.so")     # (override: an A/B build, tools/build_variant.py)

c_void_p, c_int, c_int64, c_size_t, c_double, c_char_p = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_double, C.c_char_p


class Params(C.Structure):
    _fields_ = [("distThre", c_double), ("distSepThre", c_double), ("angleThre", c_double),
                ("sigmaAngle1", c_double), ("sigmaAngle2", c_double), ("sigmaDist", c_double),
                ("sigmaFeat", c_double), ("mu", c_double), ("topK", c_int), ("method", c_int)]


class Keypoints(C.Structure):
    _fields_ = [("B", c_int), ("ns_max", c_int), ("nt_max", c_int),
                ("ns", c_void_p), ("nt", c_void_p),
                ("pc_s", c_void_p), ("normal_s", c_void_p), ("feat_s", c_void_p), ("weight_s", c_void_p),
                ("pc_t", c_void_p), ("normal_t", c_void_p), ("feat_t", c_void_p), ("weight_t", c_void_p)]


class MatchDebug(C.Structure):
    _fields_ = [("wij", c_void_p), ("corres_j", c_void_p), ("corres_w", c_void_p),
                ("counts", c_void_p), ("trace", c_void_p), ("eig_iters", c_void_p)]


class ForwardArgs(C.Structure):
    """RelposeForwardArgs (include/relpose.h): the argument block of relpose_scnet_forward_ex."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", c_int), ("x", c_void_p), ("out", c_void_p),
                ("n_images", c_int), ("H", c_int), ("W", c_int), ("reserved0", c_int),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p), ("tail_stream", c_void_p),
                ("self_tag", C.c_uint64), ("workspace_generation", C.c_uint64), ("reserved1", c_void_p),
                ("sample_pts", c_void_p), ("sample_npts", c_void_p), ("sample_npts_max", c_int), ("reserved2", c_int)]


class SCNetConfig(C.Structure):
    """RelposeSCNetConfig (include/relpose.h): the reference constructor's switches, relpose_scnet_create_ex."""
    _fields_ = [("struct_size", C.c_uint32), ("snumclass", c_int), ("use_tanh", c_int), ("batchnorm", c_int), ("skip_layer", c_int),
                ("output_mask", c_int)]


class MatchArgs(C.Structure):
    """RelposeMatchArgs (include/relpose.h): the argument block of relpose_match_pairs_ex -- the per-call choices travel with the call."""
    _fields_ = [("struct_size", C.c_uint32), ("fit_cluster", c_int), ("params_host", C.POINTER(Params)), ("kp_host", C.POINTER(Keypoints)),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("max_edges", c_int64), ("pose", c_void_p), ("status", c_void_p),
                ("debug_host", C.POINTER(MatchDebug)), ("stream", c_void_p), ("affinity_kernel", c_int), ("reserved0", c_int)]


class SiftArgs(C.Structure):
    """RelposeSiftArgs (include/relpose.h): the argument block of relpose_sift_detect."""
    _fields_ = [("struct_size", C.c_uint32), ("n_views", c_int), ("images", c_void_p), ("img_h", c_int), ("img_w", c_int), ("channels", c_int),
                ("crop_x", c_int), ("crop_y", c_int), ("crop_w", c_int), ("crop_h", c_int), ("max_kp", c_int), ("xy", c_void_p), ("size", c_void_p),
                ("angle", c_void_p), ("gray", c_void_p), ("count", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("stream", c_void_p)]


SIFT_OVERFLOW = -3                  # include/relpose.h RELPOSE_SIFT_OVERFLOW
SIFT_MAX_SIDE = 2048                # RELPOSE_SIFT_MAX_SIDE


class FgrArgs(C.Structure):
    """RelposeFgrArgs (include/relpose.h): the argument block of relpose_fgr."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs", c_int), ("n_points", c_int), ("max_points", c_int), ("pc", c_void_p), ("valid", c_void_p),
                ("seed", C.c_uint64), ("pose", c_void_p), ("status", c_void_p), ("down_points", c_void_p), ("down_count", c_void_p),
                ("nbr_index", c_void_p), ("nbr_count", c_void_p), ("normals", c_void_p), ("fpfh", c_void_p), ("corr", c_void_p),
                ("n_corr", c_void_p), ("tuple_corr", c_void_p), ("n_tuples", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("stream", c_void_p)]


FGR_OVERFLOW = -4                   # RELPOSE_FGR_OVERFLOW
FGR_MAX_POINTS = 32768              # RELPOSE_FGR_MAX_POINTS
FGR_MAX_POINTS_LIMIT = 65536        # RELPOSE_FGR_MAX_POINTS_LIMIT
FGR_MAX_TUPLES = 1000


class RansacArgs(C.Structure):
    """RelposeRansacArgs (include/relpose.h): the argument block of relpose_ransac."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs", c_int), ("n_points", c_int), ("max_points", c_int), ("pc", c_void_p), ("valid", c_void_p),
                ("seed", C.c_uint64), ("max_iterations", c_int), ("max_validations", c_int), ("pose", c_void_p), ("status", c_void_p),
                ("fitness", c_void_p), ("inlier_rmse", c_void_p), ("n_iterations", c_void_p), ("n_validations", c_void_p), ("best_index", c_void_p),
                ("down_points", c_void_p), ("down_count", c_void_p), ("fpfh", c_void_p), ("nn", c_void_p), ("val_iter", c_void_p),
                ("val_inliers", c_void_p), ("val_err", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p)]


RANSAC_OVERFLOW = -5                # RELPOSE_RANSAC_OVERFLOW
RANSAC_MAX_ITERATIONS = 4000000     # RELPOSE_RANSAC_MAX_ITERATIONS
RANSAC_MAX_VALIDATIONS = 500        # RELPOSE_RANSAC_MAX_VALIDATIONS
RANSAC_MAX_ITERATIONS_LIMIT = 16777216
RANSAC_MAX_VALIDATIONS_LIMIT = 4096


class CicpArgs(C.Structure):
    """RelposeCicpArgs (include/relpose.h): the argument block of relpose_cicp."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs", c_int), ("n_points", c_int), ("max_points", c_int), ("pc", c_void_p), ("valid", c_void_p),
                ("color", c_void_p), ("init", c_void_p), ("lambda_geometric", c_double), ("pose", c_void_p), ("status", c_void_p),
                ("fitness", c_void_p), ("inlier_rmse", c_void_p), ("n_iterations", c_void_p), ("level_pose", c_void_p),
                ("down_points", c_void_p), ("down_colors", c_void_p), ("down_count", c_void_p), ("normals", c_void_p), ("gradient", c_void_p),
                ("iter_pose", c_void_p), ("iter_ncorr", c_void_p), ("iter_rmse", c_void_p), ("iter_corr", c_void_p), ("iter_x", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p)]


CICP_OVERFLOW = -6                  # RELPOSE_CICP_OVERFLOW
CICP_LEVELS = 3                     # RELPOSE_CICP_LEVELS
CICP_TRACE_SLOTS = 94               # RELPOSE_CICP_TRACE_SLOTS
CICP_LAMBDA_GEOMETRIC = 0.968       # RELPOSE_CICP_LAMBDA_GEOMETRIC


class DenseNnArgs(C.Structure):
    """RelposeDenseNnArgs (include/relpose.h): the argument block of relpose_dense_nn."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs", c_int), ("n_points", c_int), ("n_query", c_int), ("h", c_int), ("reserved0", c_int),
                ("pc", c_void_p), ("valid", c_void_p), ("to_world", c_void_p), ("query", c_void_p), ("max_dist", c_double),
                ("nn_index", c_void_p), ("nn_dist", c_void_p), ("hit", c_void_p), ("idx_src", c_void_p), ("idx_tgt", c_void_p),
                ("stream", c_void_p)]


class DescRankArgs(C.Structure):
    """RelposeDescRankArgs (include/relpose.h): the argument block of relpose_descriptor_rank."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs", c_int), ("h", c_int), ("total_channels", c_int), ("feat_off", c_int),
                ("n_channels", c_int), ("n_corres", c_int), ("n_slots", c_int), ("f", c_void_p), ("idx_src", c_void_p), ("idx_tgt", c_void_p),
                ("sel", c_void_p), ("pair_valid", c_void_p), ("mask", c_void_p), ("count", c_void_p), ("thr", c_void_p), ("type", c_void_p),
                ("stream", c_void_p)]


DESC_MAX_CHANNELS = 64              # RELPOSE_DESC_MAX_CHANNELS


class SiftDescArgs(C.Structure):
    """RelposeSiftDescArgs (include/relpose.h): the argument block of relpose_sift_describe."""
    _fields_ = [("struct_size", C.c_uint32), ("n_views", c_int), ("images", c_void_p), ("img_h", c_int), ("img_w", c_int), ("channels", c_int),
                ("crop_x", c_int), ("crop_y", c_int), ("crop_w", c_int), ("crop_h", c_int), ("n_kp", c_int), ("grid_step", c_int),
                ("reserved0", c_int), ("kp", c_void_p), ("kp_count", c_void_p), ("desc", c_void_p), ("desc_f32", c_void_p), ("base", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p)]


class SiftRankArgs(C.Structure):
    """RelposeSiftRankArgs (include/relpose.h): the argument block of relpose_sift_rank."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs", c_int), ("n_slots", c_int), ("n_points", c_int), ("src", c_void_p), ("tgt", c_void_p),
                ("dense", c_void_p), ("pair_valid", c_void_p), ("thr", c_void_p), ("count", c_void_p), ("stream", c_void_p)]


class CompletionLossArgs(C.Structure):
    """RelposeCompletionLossArgs (include/relpose.h): the argument block of relpose_completion_loss."""
    _fields_ = [("struct_size", C.c_uint32), ("n_images", c_int), ("H", c_int), ("W", c_int), ("total_channels", c_int), ("n_classes", c_int),
                ("f", c_void_p), ("complete", c_void_p), ("label", c_void_p), ("mask", c_void_p), ("weight", c_void_p), ("sums", c_void_p),
                ("ce_mag", c_void_p), ("ce_cross", c_void_p), ("n_bad_label", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("stream", c_void_p)]


class ContrastLossArgs(C.Structure):
    """RelposeContrastLossArgs (include/relpose.h): the argument block of relpose_contrast_loss."""
    _fields_ = [("struct_size", C.c_uint32), ("n_pairs", c_int), ("h", c_int), ("total_channels", c_int), ("feat_off", c_int),
                ("n_channels", c_int), ("n_corres", c_int), ("n_neg", c_int), ("margin", C.c_float), ("reserved0", c_int), ("f", c_void_p),
                ("idx_src", c_void_p), ("idx_tgt", c_void_p), ("pair_valid", c_void_p), ("neg", c_void_p), ("pos_sum", c_void_p),
                ("neg_sum", c_void_p), ("n_active", c_void_p), ("n_skipped", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("stream", c_void_p)]


class DepthNormalsArgs(C.Structure):
    """RelposeDepthNormalsArgs (include/relpose.h): the argument block of relpose_depth_normals."""
    _fields_ = [("struct_size", C.c_uint32), ("n_views", c_int), ("h", c_int), ("dataset", c_int), ("radius", c_int), ("min_neighbors", c_int),
                ("gate_scale", C.c_float), ("reserved0", c_int), ("depth", c_void_p), ("normal", c_void_p), ("valid", c_void_p),
                ("count", c_void_p), ("moments", c_void_p), ("stream", c_void_p)]


class FramesToPanoArgs(C.Structure):
    """RelposeFramesToPanoArgs (include/relpose.h): the argument block of relpose_frames_to_pano."""
    _fields_ = [("struct_size", C.c_uint32), ("n_views", c_int), ("n_frames", c_int), ("frame_h", c_int), ("frame_w", c_int), ("h", c_int),
                ("dataset", c_int), ("gate", C.c_float), ("box", c_int * 4), ("depth", c_void_p), ("rgb", c_void_p), ("scale", c_void_p),
                ("pose", c_void_p), ("out_depth", c_void_p), ("out_rgb", c_void_p), ("out_valid", c_void_p), ("zmin", c_void_p),
                ("count", c_void_p), ("sum_z", c_void_p), ("sum_rgb", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("stream", c_void_p)]


class OverlapArgs(C.Structure):
    """RelposeOverlapArgs (include/relpose.h): the argument block of relpose_overlap."""
    _fields_ = [("struct_size", C.c_uint32), ("n_clouds", c_int), ("n_points", c_int), ("n_queries", c_int), ("pc", c_void_p), ("valid", c_void_p),
                ("query_cloud_host", c_void_p), ("ref_cloud_host", c_void_p), ("pose", c_void_p), ("max_dist", c_double), ("hits", c_void_p),
                ("nn_min", c_void_p), ("n_valid", c_void_p), ("hit", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("stream", c_void_p)]


OVERLAP_EXTENT = -7                 # RELPOSE_OVERLAP_EXTENT


class VisibilityArgs(C.Structure):
    """RelposeVisibilityArgs (include/relpose.h): the argument block of relpose_visibility."""
    _fields_ = [("struct_size", C.c_uint32), ("n_clouds", c_int), ("n_points", c_int), ("n_views", c_int), ("h", c_int), ("n_queries", c_int),
                ("dataset", c_int), ("radius", c_int), ("pc", c_void_p), ("valid", c_void_p), ("depth", c_void_p),
                ("query_cloud_host", c_void_p), ("ref_view_host", c_void_p), ("pose", c_void_p), ("tol_abs", c_double), ("tol_rel", c_double),
                ("counts", c_void_p), ("margin_sum", c_void_p), ("cls", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("stream", c_void_p)]


class TsdfFuseArgs(C.Structure):
    """RelposeTsdfFuseArgs (include/relpose.h): the argument block of relpose_tsdf_fuse."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("n_views", c_int), ("h", c_int), ("dataset", c_int), ("nx", c_int),
                ("ny", c_int), ("nz", c_int), ("accumulate", c_int), ("reserved0", c_int), ("depth", c_void_p), ("rgb", c_void_p),
                ("pose", c_void_p), ("view_begin_host", c_void_p), ("origin_host", c_void_p), ("voxel", c_double), ("trunc", c_double),
                ("tsdf_sum", c_void_p), ("weight", c_void_p), ("color_sum", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("stream", c_void_p)]


class TsdfSurfaceArgs(C.Structure):
    """RelposeTsdfSurfaceArgs (include/relpose.h): the argument block of relpose_tsdf_surface."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("nx", c_int), ("ny", c_int), ("nz", c_int), ("min_weight", c_int),
                ("cap", c_int), ("reserved0", c_int), ("tsdf_sum", c_void_p), ("weight", c_void_p), ("color_sum", c_void_p),
                ("origin_host", c_void_p), ("voxel", c_double), ("points", c_void_p), ("normals", c_void_p), ("colors", c_void_p),
                ("valid", c_void_p), ("n_points", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p)]


class TsdfMeshArgs(C.Structure):
    """RelposeTsdfMeshArgs (include/relpose.h): the argument block of relpose_tsdf_mesh."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("nx", c_int), ("ny", c_int), ("nz", c_int), ("min_weight", c_int),
                ("cap", c_int), ("cap_tri", c_int), ("tsdf_sum", c_void_p), ("weight", c_void_p), ("color_sum", c_void_p),
                ("origin_host", c_void_p), ("voxel", c_double), ("points", c_void_p), ("normals", c_void_p), ("colors", c_void_p),
                ("valid", c_void_p), ("n_points", c_void_p), ("triangles", c_void_p), ("n_triangles", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t), ("stream", c_void_p)]


class MeshComponentsArgs(C.Structure):
    """RelposeMeshComponentsArgs (include/relpose.h): the argument block of relpose_mesh_components."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("cap", c_int), ("cap_tri", c_int), ("cap_comp", c_int), ("max_rounds", c_int),
                ("triangles", c_void_p), ("n_triangles", c_void_p), ("n_points", c_void_p), ("points", c_void_p), ("area_scale", c_double),
                ("vertex_label", c_void_p), ("tri_label", c_void_p), ("n_components", c_void_p), ("bad_triangles", c_void_p),
                ("comp_root", c_void_p), ("comp_vertices", c_void_p), ("comp_triangles", c_void_p), ("comp_area", c_void_p),
                ("rounds_host", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p)]


class MeshFilterArgs(C.Structure):
    """RelposeMeshFilterArgs (include/relpose.h): the argument block of relpose_mesh_filter."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("cap", c_int), ("cap_tri", c_int), ("cap_comp", c_int), ("drop_unused", c_int),
                ("points", c_void_p), ("normals", c_void_p), ("colors", c_void_p), ("n_points", c_void_p), ("triangles", c_void_p),
                ("n_triangles", c_void_p), ("vertex_label", c_void_p), ("tri_label", c_void_p), ("keep", c_void_p), ("out_points", c_void_p),
                ("out_normals", c_void_p), ("out_colors", c_void_p), ("out_valid", c_void_p), ("out_n_points", c_void_p),
                ("out_triangles", c_void_p), ("out_n_triangles", c_void_p), ("vertex_map", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t), ("stream", c_void_p)]


class MeshDecimateArgs(C.Structure):
    """RelposeMeshDecimateArgs (include/relpose.h): the argument block of relpose_mesh_decimate."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("cap", c_int), ("cap_tri", c_int), ("gx", c_int), ("gy", c_int), ("gz", c_int),
                ("dedupe", c_int), ("points", c_void_p), ("normals", c_void_p), ("colors", c_void_p), ("n_points", c_void_p),
                ("triangles", c_void_p), ("n_triangles", c_void_p), ("origin_host", c_void_p), ("cell", c_double), ("out_points", c_void_p),
                ("out_normals", c_void_p), ("out_colors", c_void_p), ("out_valid", c_void_p), ("out_n_points", c_void_p), ("out_count", c_void_p),
                ("out_triangles", c_void_p), ("out_n_triangles", c_void_p), ("vertex_map", c_void_p), ("tri_map", c_void_p),
                ("bad_triangles", c_void_p), ("outside_triangles", c_void_p), ("degenerate_triangles", c_void_p),
                ("duplicate_triangles", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p)]


class TsdfAlignArgs(C.Structure):
    """RelposeTsdfAlignArgs (include/relpose.h): the argument block of relpose_tsdf_align."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("n_views", c_int), ("h", c_int), ("dataset", c_int), ("nx", c_int),
                ("ny", c_int), ("nz", c_int), ("min_weight", c_int), ("iters", c_int), ("stride", c_int), ("reserved0", c_int),
                ("tsdf_sum", c_void_p), ("weight", c_void_p), ("depth", c_void_p), ("pose", c_void_p), ("origin_host", c_void_p),
                ("scene_of_view_host", c_void_p), ("voxel", c_double), ("eig_min", c_double), ("pose_out", c_void_p), ("eig", c_void_p),
                ("held", c_void_p), ("sums", c_void_p), ("rms", c_void_p), ("trace_pose", c_void_p), ("trace_sums", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p)]


class TsdfRenderArgs(C.Structure):
    """RelposeTsdfRenderArgs (include/relpose.h): the argument block of relpose_tsdf_render."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("n_views", c_int), ("h", c_int), ("dataset", c_int), ("nx", c_int),
                ("ny", c_int), ("nz", c_int), ("min_weight", c_int), ("n_steps", c_int), ("skip", c_int), ("reserved0", c_int),
                ("tsdf_sum", c_void_p), ("weight", c_void_p), ("color_sum", c_void_p), ("pose", c_void_p), ("origin_host", c_void_p),
                ("scene_of_view_host", c_void_p), ("voxel", c_double), ("d_min", c_double), ("step", c_double), ("depth", c_void_p),
                ("cls", c_void_p), ("normal", c_void_p), ("color", c_void_p), ("n_evaluated", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t), ("stream", c_void_p)]


class PoseSyncArgs(C.Structure):
    """RelposePoseSyncArgs (include/relpose.h): the argument block of relpose_pose_sync."""
    _fields_ = [("struct_size", C.c_uint32), ("n_scenes", c_int), ("n_views", c_int), ("n_edges", c_int), ("n_final", c_int), ("robust", c_int),
                ("reserved0", c_int), ("reserved1", c_int), ("view_begin_host", c_void_p), ("edge_begin_host", c_void_p), ("src", c_void_p),
                ("dst", c_void_p), ("T", c_void_p), ("w0", c_void_p), ("sigma_r", c_double), ("sigma_t", c_double), ("mu0", c_double),
                ("div", c_double), ("pose", c_void_p), ("component", c_void_p), ("tree", c_void_p), ("edge_state", c_void_p),
                ("confidence", c_void_p), ("res_rot", c_void_p), ("res_trans", c_void_p), ("n_components", c_void_p), ("cost", c_void_p),
                ("last_step", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("stream", c_void_p)]


SYNC_MAX_VIEWS = 64                 # RELPOSE_SYNC_MAX_VIEWS, per scene
SYNC_MAX_EDGES = 4096               # RELPOSE_SYNC_MAX_EDGES, per scene
TSDF_MAX_VIEWS = 4096               # per scene per relpose_tsdf_fuse call
TSDF_MAX_WEIGHT = 65535             # the caller's bound on a voxel's weight across accumulating calls
TSDF_ALIGN_EIG_MIN = 0.0043         # relpose_tsdf_align's eigenvalue floor: between the two ranges measured in DESIGN.md 4.19
TSDF_RENDER_MAX_STEPS = 65536        # relpose_tsdf_render's bound on n_steps
MESH_EROUNDS = -3                   # RELPOSE_EROUNDS: relpose_mesh_components ran out of max_rounds
TSDF_ALIGN_SUMS = 32                # 21 JtJ + 6 Jtr + r^2 + the counts of outside, unknown, saturated and used points


# name -> (restype, argtypes); must list every symbol declared in include/relpose.h
SIGNATURES = {
    "relpose_default_params": (None, [C.POINTER(Params)]),
    "relpose_version": (c_char_p, []),
    "relpose_set_tuning": (c_int, [c_int, c_int]),
    "relpose_match_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int64]),
    "relpose_match_pairs": (c_int, [C.POINTER(Params), C.POINTER(Keypoints), c_void_p, c_size_t, c_int64,
                                    c_void_p, c_void_p, C.POINTER(MatchDebug), c_void_p]),
    "relpose_match_pairs_ex": (c_int, [C.POINTER(MatchArgs)]),
    "relpose_affinity_topk": (c_int, [C.POINTER(Params), C.POINTER(Keypoints), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "relpose_apply_mask": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "relpose_build_view": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "relpose_pano2pc": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "relpose_warp_workspace_bytes": (c_size_t, [c_int, c_int]),
    "relpose_warp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "relpose_warp_pairs": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "relpose_warp_pairs2": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "relpose_pose_inverse": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "relpose_sample_primitives": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                          c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "relpose_get_pixel": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "relpose_interpolate": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "relpose_observed_points": (c_int, [c_int, c_int]),
    "relpose_depth2pc": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "relpose_depth2pc_full": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "relpose_nn_dist": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "relpose_feature_distance_map": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "relpose_nms_sampling": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "relpose_keypoints_reference_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "relpose_keypoints_reference": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                            c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "relpose_sift_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "relpose_sift_stage_capacity": (c_int, [c_int]),
    "relpose_sift_detect": (c_int, [C.POINTER(SiftArgs)]),
    "relpose_fgr_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "relpose_fgr": (c_int, [C.POINTER(FgrArgs)]),
    "relpose_ransac_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "relpose_ransac": (c_int, [C.POINTER(RansacArgs)]),
    "relpose_cicp_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "relpose_cicp": (c_int, [C.POINTER(CicpArgs)]),
    "relpose_dense_nn": (c_int, [C.POINTER(DenseNnArgs)]),
    "relpose_descriptor_rank": (c_int, [C.POINTER(DescRankArgs)]),
    "relpose_sift_describe_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "relpose_sift_describe": (c_int, [C.POINTER(SiftDescArgs)]),
    "relpose_sift_rank": (c_int, [C.POINTER(SiftRankArgs)]),
    "relpose_completion_loss_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "relpose_completion_loss": (c_int, [C.POINTER(CompletionLossArgs)]),
    "relpose_contrast_loss_workspace_bytes": (c_size_t, [c_int, c_int]),
    "relpose_contrast_loss": (c_int, [C.POINTER(ContrastLossArgs)]),
    "relpose_depth_normals": (c_int, [C.POINTER(DepthNormalsArgs)]),
    "relpose_frames_to_pano_workspace_bytes": (c_size_t, [c_int, c_int]),
    "relpose_frames_to_pano": (c_int, [C.POINTER(FramesToPanoArgs)]),
    "relpose_overlap_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "relpose_overlap": (c_int, [C.POINTER(OverlapArgs)]),
    "relpose_visibility_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "relpose_visibility": (c_int, [C.POINTER(VisibilityArgs)]),
    "relpose_tsdf_fuse_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "relpose_tsdf_fuse": (c_int, [C.POINTER(TsdfFuseArgs)]),
    "relpose_tsdf_surface_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "relpose_tsdf_surface": (c_int, [C.POINTER(TsdfSurfaceArgs)]),
    "relpose_tsdf_mesh_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "relpose_tsdf_mesh": (c_int, [C.POINTER(TsdfMeshArgs)]),
    "relpose_mesh_components_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "relpose_mesh_components": (c_int, [C.POINTER(MeshComponentsArgs)]),
    "relpose_mesh_filter_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "relpose_mesh_filter": (c_int, [C.POINTER(MeshFilterArgs)]),
    "relpose_mesh_decimate_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "relpose_mesh_decimate": (c_int, [C.POINTER(MeshDecimateArgs)]),
    "relpose_tsdf_align_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "relpose_tsdf_align": (c_int, [C.POINTER(TsdfAlignArgs)]),
    "relpose_tsdf_render_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "relpose_tsdf_render": (c_int, [C.POINTER(TsdfRenderArgs)]),
    "relpose_pose_sync_workspace": (c_size_t, [c_int, c_int, c_int]),
    "relpose_pose_sync": (c_int, [C.POINTER(PoseSyncArgs)]),
    "relpose_scnet_create": (c_void_p, [c_int, c_int]),
    "relpose_scnet_create_ex": (c_void_p, [C.POINTER(SCNetConfig)]),
    "relpose_scnet_destroy": (None, [c_void_p]),
    "relpose_scnet_set_param": (c_int, [c_void_p, c_char_p, c_void_p, c_size_t]),
    "relpose_scnet_finalize": (c_int, [c_void_p]),
    "relpose_scnet_set_precision": (c_int, [c_void_p, c_int]),
    "relpose_scnet_num_params": (c_int64, [c_void_p]),
    "relpose_scnet_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "relpose_scnet_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "relpose_scnet_forward_ex": (c_int, [c_void_p, C.POINTER(ForwardArgs)]),
    "relpose_scnet_plan_macs": (c_int, [c_void_p, c_int, c_int, c_int, C.POINTER(c_double)]),
    "relpose_scnet_layer_kernel": (c_int, [c_void_p, c_char_p, c_int]),
    "relpose_scnet_zero_tiles": (c_int, [c_void_p, c_void_p, c_void_p, C.POINTER(c_int64)]),
    "relpose_scnet_last_tail": (c_int, [c_void_p]),
    "relpose_scnet_conv1_zero": (c_int, [c_void_p, c_void_p, c_void_p, C.POINTER(c_int64), c_void_p]),
    "relpose_scnet_conv4_rows": (c_int, [c_void_p, c_void_p, c_void_p, C.POINTER(c_int64)]),
    "relpose_scnet_read_tap": (c_int64, [c_void_p, c_char_p, c_void_p, c_void_p, c_void_p]),
    "relpose_scnet_profile": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_int,
                                      C.POINTER(c_double), C.POINTER(c_double), C.POINTER(c_int64), c_void_p]),
}

_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            _build_locked()          # a fresh checkout on a box with hipcc: compile the HIP library once (no CPU fallback exists)
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `python -m relativepose_amd.build` "
                               "(or __graft_entry__.build()). There is no CPU fallback.")
        # torch ships its own libamdhip64; import it first so this library binds to the SAME HIP runtime
        # (loading ours first pulls in /opt/rocm's copy and the second runtime then sees no device).
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        missing = [name for name in SIGNATURES if not hasattr(l, name)]
        if missing:
            raise RuntimeError(f"{LIB_PATH} is stale, missing symbols: {missing}")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def _build_locked():
    """Compile librelpose_hip.so with hipcc if it is missing; one process builds, concurrent ranks wait on the lock."""
    import fcntl
    from . import build as _b
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        return
    with open(LIB_PATH + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            if not os.path.exists(LIB_PATH):
                _b.build(verbose=False)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)


# relpose_set_tuning keys (include/relpose.h RELPOSE_TUNE_*)
TUNE_KEYS = {"affinity_kernel": 0, "fit_max_products": 1, "fit_cluster": 2, "fit_global_vectors": 3, "fit_fixed_checks": 4,
             "heads_kernel": 5, "deconv_strip": 6, "zero_tiles": 7, "conv1_zero": 8, "conv4_rows": 9}
AFFINITY_KERNELS = {"auto": 0, "rows": 1, "tile": 2, "lds": 3, "pool": 4}


class tuning:
    """``with tuning(affinity_kernel="tile"): ...`` -- force a kernel variant for the calls inside (process-wide knob of the
    library, restored on exit).  Every variant produces the same results; the parity tests use this to check each one."""

    def __init__(self, **kw):
        self.kw = {k: (AFFINITY_KERNELS[v] if k == "affinity_kernel" and isinstance(v, str) else int(v)) for k, v in kw.items()}
        self.old = {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = lib().relpose_set_tuning(TUNE_KEYS[k], v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            lib().relpose_set_tuning(TUNE_KEYS[k], v)
        return False


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}" + (" (HIP error %d)" % (-rc - 1000) if rc <= -1000 else ""))


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("relativepose_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
