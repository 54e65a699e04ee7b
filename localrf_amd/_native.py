"""ctypes binding of liblrf_hip.so (C ABI in include/lrf.h), and the one calling convention of the package:

  call(name, *args)                    the symbol, checked: a non-zero return raises NativeError under the symbol's name
  launch(name, dev, *args, guard=...)  call() with the device's current stream appended as the trailing ABI argument
  stream(dev) / torch_stream(dev)      that stream's handle / its torch object
  workspace(name, dev, *shape)         the <name>_workspace_bytes protocol -> uint8 device tensor
  require_gpu(t, name, feature)        "is a tensor, lives on the GPU", else TypeError / NativeError
  conform(t, dtype)                    t itself when it is already dtype + contiguous, else converted

There is no fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRF_LIB", os.path.join(_HERE, "csrc", "liblrf_hip.so"))   # LRF_LIB: experiment builds

LRF_FLAG_WHITE_BG = 1
LRF_FLAG_RELU_DENS = 2
LRF_FLAG_MLP_VALU = 4
LRF_FLAG_MLP_F32 = 8
LRF_FLAG_ROWS_SAVED = 16
LRF_FLAG_SORT_RAYS = 32
LRF_FLAG_PE_OFF = 64
LRF_FLAG_PLANE_EVENTS = 128
LRF_FLAG_DETERMINISTIC = 256
LRF_FLAG_ALL = 511

_f = C.c_void_p  # device float*


class LrfParams(C.Structure):
    _fields_ = [("density_plane", _f * 3), ("density_line", _f * 3),
                ("app_plane", _f * 3), ("app_line", _f * 3),
                ("basis", _f), ("w1", _f), ("b1", _f), ("w2", _f), ("b2", _f), ("w3", _f), ("b3", _f),
                ("grid", C.c_int32 * 3), ("fea_pe", C.c_int32), ("view_pe", C.c_int32), ("feature_c", C.c_int32)]


class LrfField(C.Structure):
    _fields_ = [("cache", C.c_void_p), ("alpha_vol", _f), ("alpha_dim", C.c_int32 * 3),
                ("alpha_aabb", C.c_float * 6), ("aabb", C.c_float * 6), ("grid", C.c_int32 * 3),
                ("density_shift", C.c_float), ("distance_scale", C.c_float), ("weight_thres", C.c_float),
                ("term_T", C.c_float),
                ("basis", _f), ("w1", _f), ("b1", _f), ("w2", _f), ("b2", _f), ("w3", _f), ("b3", _f),
                ("fea_pe", C.c_int32), ("view_pe", C.c_int32), ("feature_c", C.c_int32)]


class LrfSceneField(C.Structure):
    _fields_ = [("field", C.POINTER(LrfField)), ("z", _f), ("S", C.c_int32), ("flags", C.c_uint32),
                ("workspace", C.c_void_p)]


class LrfGrads(C.Structure):
    _fields_ = [("density_plane", _f * 3), ("density_line", _f * 3),
                ("app_plane", _f * 3), ("app_line", _f * 3),
                ("basis", _f), ("w1", _f), ("b1", _f), ("w2", _f), ("b2", _f), ("w3", _f), ("b3", _f),
                ("zero_base", _f), ("zero_floats", C.c_int64)]


LRF_ADAM_MAX = 64
LRF_POSE_MAX = 64


class LrfAdamTensor(C.Structure):
    _fields_ = [("p", _f), ("g", _f), ("m", _f), ("v", _f), ("n", C.c_int64),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float)]


class LrfTvSeg(C.Structure):
    _fields_ = [("x", _f), ("g", _f), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("scale", C.c_float)]


class LrfFlowLoss(C.Structure):
    _fields_ = [("cam2world", _f), ("frame", C.c_void_p), ("fwd_off", C.c_void_p), ("dirs", _f), ("depth", _f), ("ij", C.c_void_p),
                ("fwd_flow", _f), ("fwd_mask", _f), ("bwd_flow", _f), ("bwd_mask", _f), ("focal", _f), ("center", _f),
                ("F", C.c_int32), ("V", C.c_int32), ("n", C.c_int32), ("quantile", C.c_float)]


LRF_LOSS_MAX_PER_VIEW = 4096
LRF_LOSS_TERMS_MAX = 8


class LrfBatchGather(C.Structure):
    _fields_ = [("images", _f), ("fwd_flow", _f), ("bwd_flow", _f), ("invdepths", _f), ("view_ids", C.c_void_p), ("pix", C.c_void_p),
                ("V", C.c_int32), ("n", C.c_int32), ("HW", C.c_int32), ("n_images", C.c_int32)]


class LrfLossTerms(C.Structure):
    _fields_ = [("x", _f * LRF_LOSS_TERMS_MAX), ("n", C.c_int32 * LRF_LOSS_TERMS_MAX), ("a", C.c_float * LRF_LOSS_TERMS_MAX),
                ("b", C.c_float * LRF_LOSS_TERMS_MAX), ("count", C.c_int32), ("s", _f)]


class LrfImageMetrics(C.Structure):
    _fields_ = [("img0", _f), ("img1", _f), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("filter_size", C.c_int32),
                ("max_val", C.c_double), ("filter_sigma", C.c_double), ("k1", C.c_double), ("k2", C.c_double)]


LRF_FRAMES_ERR_NOT_RESIDENT = 1


class LrfFrameWindow(C.Structure):
    _fields_ = [("rgb", _f), ("loss_weight", _f), ("invdepth", _f), ("fwd_flow", _f), ("fwd_mask", _f), ("bwd_flow", _f),
                ("bwd_mask", _f), ("slot_of", C.c_void_p), ("status", C.c_void_p),
                ("capacity", C.c_int32), ("n_px", C.c_int32), ("num_images", C.c_int32)]


LRF_SELECT_QUANTILE = 0
LRF_SELECT_MEDIAN = 1
LRF_SELECT_MAX_ROWS = 256
LRF_EVAL_MAX_VIEWS = 64


class LrfFlowComparison(C.Structure):
    _fields_ = [("cam2world", _f), ("depth", _f), ("dirs", _f), ("ij", C.c_void_p), ("fwd_flow", _f), ("fwd_mask", _f),
                ("bwd_flow", _f), ("bwd_mask", _f), ("focal", _f), ("center", _f),
                ("F", C.c_int32), ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("idx", C.c_int32 * LRF_EVAL_MAX_VIEWS)]


LRF_POINTS_MAX_NEIGH = 8


class LrfPointsFuse(C.Structure):
    _fields_ = [("depth", _f), ("rgb8", C.c_void_p), ("cam2world", _f), ("focal", _f), ("center", _f),
                ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("fov360", C.c_int32), ("stride", C.c_int32),
                ("d_min", C.c_float), ("d_max", C.c_float), ("n_neigh", C.c_int32), ("neigh", C.c_int32 * LRF_POINTS_MAX_NEIGH),
                ("rel_tol", C.c_float), ("min_consistent", C.c_int32)]


class LrfTsdfVolume(C.Structure):
    _fields_ = [("tsdf", _f), ("weight", _f), ("rgb", _f), ("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32),
                ("origin", C.c_float * 3), ("voxel", C.c_float), ("trunc", C.c_float)]


class LrfMeshExtract(C.Structure):
    _fields_ = [("value", _f), ("weight", _f), ("rgb", _f), ("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32),
                ("origin", C.c_float * 3), ("voxel", C.c_float), ("level", C.c_float), ("min_weight", C.c_float)]


class LrfMeshFilter(C.Structure):
    _fields_ = [("vertices", _f), ("rgb8", C.c_void_p), ("faces", C.c_void_p), ("labels", C.c_void_p), ("faces_of", C.c_void_p),
                ("Nv", C.c_int64), ("Nf", C.c_int64)]


class LrfMeshSimplify(C.Structure):
    _fields_ = [("vertices", _f), ("rgb8", C.c_void_p), ("faces", C.c_void_p), ("Nv", C.c_int64), ("Nf", C.c_int64),
                ("origin", C.c_double * 3), ("cell", C.c_double), ("lo", C.c_int32 * 3), ("dims", C.c_int32 * 3),
                ("dedupe", C.c_int32), ("reserved", C.c_int32)]


class LrfMeshSimplifyQuadric(C.Structure):
    _fields_ = [("mesh", LrfMeshSimplify), ("regularize", C.c_double)]


class LrfMeshSmooth(C.Structure):
    _fields_ = [("vertices", _f), ("faces", C.c_void_p), ("Nv", C.c_int64), ("Nf", C.c_int64),
                ("lo", C.c_double * 3), ("lam", C.c_double), ("mu", C.c_double),
                ("s", C.c_int32), ("iterations", C.c_int32), ("pin_boundary", C.c_int32), ("reserved", C.c_int32)]


class LrfMeshHoles(C.Structure):
    _fields_ = [("vertices", _f), ("rgb8", C.c_void_p), ("faces", C.c_void_p), ("Nv", C.c_int64), ("Nf", C.c_int64),
                ("lo", C.c_double * 3), ("max_edges", C.c_int32), ("s", C.c_int32)]


LRF_AGREEMENT_MAX_TOLS = 8


class LrfMeshRaster(C.Structure):
    _fields_ = [("vertices", _f), ("rgb8", C.c_void_p), ("faces", C.c_void_p), ("cam2world", _f), ("focal", _f), ("center", _f),
                ("Nv", C.c_int64), ("Nf", C.c_int64), ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("cull", C.c_int32),
                ("d_min", C.c_float), ("d_max", C.c_float)]


LRF_DISTANCE_MAX_THRESHOLDS = 8


class LrfMeshIndex(C.Structure):
    _fields_ = [("vertices", _f), ("faces", C.c_void_p), ("grid", C.c_void_p), ("list", C.c_void_p),
                ("Nv", C.c_int64), ("Nf", C.c_int64), ("entries", C.c_int64),
                ("lo", C.c_double * 3), ("cell", C.c_double), ("dims", C.c_int32 * 3), ("reserved", C.c_int32)]


LRF_CLOUD_MAX_K = 8


class LrfCloudIndex(C.Structure):
    _fields_ = [("points", _f), ("grid", C.c_void_p), ("records", C.c_void_p), ("M", C.c_int64), ("entries", C.c_int64),
                ("lo", C.c_double * 3), ("cell", C.c_double), ("dims", C.c_int32 * 3), ("reserved", C.c_int32)]


class LrfCloudVoxel(C.Structure):
    _fields_ = [("points", _f), ("rgb8", C.c_void_p), ("M", C.c_int64), ("origin", C.c_double * 3), ("cell", C.c_double),
                ("lo", C.c_int32 * 3), ("dims", C.c_int32 * 3)]


class LrfAlignFrame(C.Structure):
    _fields_ = [("c", C.c_double * 3), ("h", C.c_double)]


class LrfAlignPlane(C.Structure):
    _fields_ = [("vertices", _f), ("faces", C.c_void_p), ("points", _f), ("closest", _f), ("face", C.c_void_p), ("distance", _f),
                ("Nv", C.c_int64), ("Nf", C.c_int64), ("N", C.c_int64), ("c", C.c_double * 3), ("u", C.c_double),
                ("gate", C.c_float), ("reserved", C.c_int32)]


class LrfAlignPlaneCloud(C.Structure):
    _fields_ = [("points", _f), ("closest", _f), ("index", C.c_void_p), ("distance", _f), ("normals", _f),
                ("N", C.c_int64), ("M", C.c_int64), ("c", C.c_double * 3), ("u", C.c_double),
                ("gate", C.c_float), ("reserved", C.c_int32)]


class LrfMeshTexture(C.Structure):
    _fields_ = [("vertices", _f), ("rgb8", C.c_void_p), ("faces", C.c_void_p), ("frames", C.c_void_p), ("mesh_depth", _f),
                ("cam2world", _f), ("focal", _f), ("center", _f), ("Nv", C.c_int64), ("Nf", C.c_int64),
                ("patch", C.c_int32), ("cols", C.c_int32), ("blend", C.c_int32), ("two_sided", C.c_int32),
                ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("vis_tol", C.c_float), ("min_cos", C.c_float),
                ("reserved", C.c_int32)]


class LrfTsdfBlocks(C.Structure):
    _fields_ = [("marks", C.c_void_p), ("table", C.c_void_p), ("coords", C.c_void_p), ("tsdf", _f), ("weight", _f), ("rgb", _f),
                ("Bx", C.c_int32), ("By", C.c_int32), ("Bz", C.c_int32), ("n_blocks", C.c_int32),
                ("origin", C.c_float * 3), ("voxel", C.c_float), ("trunc", C.c_float)]


# every symbol include/lrf.h and include/lrf_debug.h declare: (restype, argtypes)
SYMBOLS = {
    "lrf_abi_version": (C.c_int, []),
    "lrf_last_error": (C.c_char_p, []),
    "lrf_error_slot": (C.c_void_p, []),
    "lrf_debug_set_dump": (None, [C.c_void_p]),
    "lrf_debug_march_phases": (None, [C.c_void_p]),
    "lrf_debug_set_lds_lines": (None, [C.c_int]),
    "lrf_debug_set_pipe_chunk": (None, [C.c_int]),
    "lrf_debug_set_scene_fuse": (None, [C.c_int]),
    "lrf_debug_set_march_rays": (None, [C.c_int]),
    "lrf_debug_set_lds_toff": (None, [C.c_int]),
    "lrf_debug_tile_ranges": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_debug_tile_reduce": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_debug_block_reduce": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_debug_saved_row_offset":(C.c_int64, [C.c_int, C.c_uint64, C.c_int]),
    "lrf_debug_scatter_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "lrf_debug_forward_plan": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "lrf_debug_workspace_vmax_bwd": (None, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "lrf_debug_set_bwd_overlap": (None, [C.c_int]),
    "lrf_debug_set_train_fwd_engine": (None, [C.c_int]),
    "lrf_debug_set_scatter_wgs": (None, [C.c_int]),
    "lrf_workspace_layout_bwd": (None, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "lrf_cache_bytes": (C.c_size_t, [C.POINTER(C.c_int32)]),
    "lrf_pack_field": (C.c_int, [C.POINTER(LrfParams), C.c_void_p, C.c_void_p]),
    "lrf_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lrf_render_fwd": (C.c_int, [C.POINTER(LrfField), _f, _f, C.c_int32, C.c_int32, C.c_uint32, C.c_float,
                                 _f, _f, _f, _f, C.c_void_p, C.c_void_p]),
    "lrf_render_fwd_profile": (C.c_int, [C.POINTER(LrfField), _f, _f, C.c_int32, C.c_int32, C.c_uint32,
                                         C.c_float, _f, _f, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "lrf_render_fwd_train": (C.c_int, [C.POINTER(LrfField), _f, _f, C.c_int32, C.c_int32, C.c_uint32, _f, _f,
                                       C.c_void_p, C.c_void_p]),
    "lrf_workspace_bytes_bwd": (C.c_size_t, [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "lrf_workspace_bytes_bwd_cfg": (C.c_size_t, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_uint32]),
    "lrf_render_bwd": (C.c_int, [C.POINTER(LrfField), C.POINTER(LrfParams), _f, _f, C.c_int32, C.c_int32,
                                 C.c_uint32, _f, _f, C.POINTER(LrfGrads), _f, C.c_void_p, C.c_void_p]),
    "lrf_render_bwd_wait": (C.c_int, [C.c_int32, C.c_void_p]),
    "lrf_density_feature": (C.c_int, [C.POINTER(LrfField), _f, C.c_int32, _f, C.c_void_p]),
    "lrf_app_feature": (C.c_int, [C.POINTER(LrfField), _f, C.c_int32, _f, C.c_void_p]),
    "lrf_sample_ray_aabb": (C.c_int, [_f, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, _f,
                                      C.c_int32, C.c_int32, _f, _f, C.c_void_p, C.c_void_p]),
    "lrf_sample_ray_contracted": (C.c_int, [_f, _f, _f, C.c_int32, C.c_int32, _f, C.c_void_p]),
    "lrf_z_schedule": (C.c_int, [C.c_int32, _f, _f, _f, C.c_void_p]),
    "lrf_adam_step": (C.c_int, [C.POINTER(LrfAdamTensor), C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "lrf_adam_step_pack": (C.c_int, [C.POINTER(LrfAdamTensor), C.c_int32, _f, C.c_float, C.c_float, C.c_float, C.POINTER(LrfParams), C.c_void_p, C.c_void_p]),
    "lrf_photo_loss_fwd": (C.c_int, [_f, _f, _f, _f, C.c_int32, _f, _f, C.c_void_p]),
    "lrf_photo_loss_bwd": (C.c_int, [_f, _f, _f, _f, _f, C.c_int32, _f, C.c_void_p]),
    "lrf_batch_gather": (C.c_int, [C.POINTER(LrfBatchGather), _f, _f, _f, _f, _f, _f, C.c_void_p]),
    "lrf_loss_combine_fwd": (C.c_int, [C.POINTER(LrfLossTerms), _f, _f, C.c_void_p]),
    "lrf_loss_combine_bwd": (C.c_int, [_f, _f, C.c_int32, _f, C.c_void_p]),
    "lrf_rows_gather": (C.c_int, [_f, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f, C.c_void_p]),
    "lrf_rows_gather_bwd": (C.c_int, [_f, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f, C.c_void_p]),
    "lrf_adam_step_dev": (C.c_int, [C.POINTER(LrfAdamTensor), C.c_int32, _f, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "lrf_density_l1_workspace": (C.c_size_t, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lrf_density_l1_fwd": (C.c_int, [C.POINTER(_f), C.POINTER(_f), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.c_float, C.c_int32, C.c_void_p, _f, C.c_void_p]),
    "lrf_density_l1_bwd": (C.c_int, [C.POINTER(_f), C.POINTER(_f), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.c_void_p, _f, C.POINTER(_f), C.POINTER(_f), C.c_void_p]),
    "lrf_density_l1_bwd_acc": (C.c_int, [C.POINTER(_f), C.POINTER(_f), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.c_void_p, _f, C.POINTER(_f), C.POINTER(_f), C.c_void_p]),
    "lrf_pose_assemble": (C.c_int, [C.POINTER(_f), C.POINTER(_f), C.c_int32, C.c_int32, _f, C.c_void_p]),
    "lrf_pose_assemble_bwd": (C.c_int, [C.POINTER(_f), C.c_int32, C.c_int32, _f, _f, _f, C.c_void_p]),
    "lrf_dense_alpha": (C.c_int, [C.POINTER(LrfField), _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                  C.c_uint32, _f, C.c_void_p]),
    "lrf_alpha_pool_threshold": (C.c_int, [_f, C.c_int32, C.c_int32, C.c_int32, C.c_float, _f, C.c_void_p]),
    "lrf_tv_workspace": (C.c_size_t, [C.POINTER(LrfTvSeg), C.c_int32]),
    "lrf_tv_loss_fwd": (C.c_int, [C.POINTER(LrfTvSeg), C.c_int32, C.c_float, C.c_void_p, _f, C.c_void_p]),
    "lrf_tv_loss_bwd": (C.c_int, [C.POINTER(LrfTvSeg), C.c_int32, C.c_float, _f, C.c_void_p]),
    "lrf_upsample_bilinear": (C.c_int, [_f, C.c_int32, C.c_int32, C.c_int32, _f, C.c_int32, C.c_int32, C.c_void_p]),
    "lrf_flow_loss_fwd": (C.c_int, [C.POINTER(LrfFlowLoss), _f, _f, C.c_void_p]),
    "lrf_flow_loss_bwd": (C.c_int, [C.POINTER(LrfFlowLoss), _f, _f, C.c_float, _f, _f, _f, _f, _f, C.c_void_p]),
    "lrf_depth_loss_fwd": (C.c_int, [_f, _f, C.c_int32, C.c_int32, C.c_float, _f, _f, _f, C.c_void_p]),
    "lrf_depth_loss_bwd": (C.c_int, [_f, _f, C.c_int32, C.c_int32, _f, _f, _f, C.c_float, _f, C.c_void_p]),
    "lrf_scene_rays": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f, _f, C.c_int32, _f, _f, C.c_int32,
                                 C.c_int32, C.c_int32, _f, _f, C.c_void_p, C.c_void_p]),
    "lrf_scene_rays_bwd": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f, C.c_int32, _f, _f, C.c_int32,
                                     C.c_int32, C.c_int32, _f, _f, _f, _f, _f, C.c_void_p]),
    "lrf_scene_blend": (C.c_int, [_f, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, _f, _f, _f, C.c_void_p]),
    "lrf_scene_fwd": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f, _f, C.c_int32, _f, _f, C.c_int32, C.c_int32,
                                C.c_int32, C.POINTER(LrfSceneField), C.c_float, C.c_int32, _f, _f,
                                _f, _f, _f, _f, C.c_void_p, _f, _f, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lrf_image_metrics_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lrf_image_metrics": (C.c_int, [C.POINTER(LrfImageMetrics), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_frames_gather": (C.c_int, [C.POINTER(LrfFrameWindow), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    _f, _f, _f, _f, _f, _f, _f, C.c_void_p]),
    "lrf_decode_flow": (C.c_int, [C.POINTER(LrfFrameWindow), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_double, C.c_void_p]),
    "lrf_frame_sharpness_workspace_bytes": (C.c_size_t, []),
    "lrf_frame_sharpness": (C.c_int, [C.POINTER(LrfFrameWindow), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "lrf_select_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "lrf_select": (C.c_int, [_f, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, C.c_float, _f, C.c_void_p,
                             C.c_void_p]),
    "lrf_flow_comparison_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "lrf_flow_comparison": (C.c_int, [C.POINTER(LrfFlowComparison), _f, _f, _f, _f, _f, C.c_void_p, C.c_void_p]),
    "lrf_depth_comparison_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "lrf_depth_comparison": (C.c_int, [_f, _f, C.c_int32, C.c_int32, C.c_int32, _f, _f, C.c_void_p, C.c_void_p]),
    "lrf_encode_frames_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "lrf_encode_frames": (C.c_int, [_f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.c_void_p,
                                    C.c_void_p, C.c_void_p, _f, C.c_void_p, C.c_void_p]),
    "lrf_points_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lrf_points_fuse": (C.c_int, [C.POINTER(LrfPointsFuse), C.c_int64, _f, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "lrf_tsdf_integrate": (C.c_int, [C.POINTER(LrfTsdfVolume), _f, C.c_void_p, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_float, C.c_float, C.c_void_p]),
    "lrf_mesh_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "lrf_mesh_extract": (C.c_int, [C.POINTER(LrfMeshExtract), C.c_int64, C.c_int64, _f, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "lrf_tsdf_blocks_touch": (C.c_int, [C.POINTER(LrfTsdfBlocks), _f, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                        C.c_float, C.c_void_p]),
    "lrf_tsdf_blocks_assign_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "lrf_tsdf_blocks_assign": (C.c_int, [C.POINTER(LrfTsdfBlocks), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_tsdf_blocks_integrate": (C.c_int, [C.POINTER(LrfTsdfBlocks), _f, C.c_void_p, _f, _f, _f, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_float, C.c_float, C.c_void_p]),
    "lrf_mesh_extract_blocks_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "lrf_mesh_extract_blocks": (C.c_int, [C.POINTER(LrfTsdfBlocks), C.c_float, C.c_float, C.c_int64, C.c_int64, _f, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_mesh_components_init": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "lrf_mesh_components_round": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "lrf_mesh_components_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "lrf_mesh_filter_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "lrf_mesh_filter": (C.c_int, [C.POINTER(LrfMeshFilter), C.c_int32, _f, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "lrf_mesh_simplify_bounds": (C.c_int, [_f, C.c_int64, C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_void_p]),
    "lrf_mesh_simplify_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "lrf_mesh_simplify": (C.c_int, [C.POINTER(LrfMeshSimplify), _f, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_mesh_simplify_quadric_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "lrf_mesh_simplify_quadric": (C.c_int, [C.POINTER(LrfMeshSimplifyQuadric), _f, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "lrf_mesh_incidence_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "lrf_mesh_incidence": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_mesh_topology": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_mesh_vertex_normals": (C.c_int, [_f, C.c_void_p, C.c_int64, C.c_int64, _f, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_debug_mesh_vertex_normals": (C.c_int, [_f, C.c_void_p, C.c_int64, C.c_int64, _f, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "lrf_mesh_smooth_bounds": (C.c_int, [_f, C.c_int64, C.c_void_p, C.c_void_p]),
    "lrf_mesh_smooth_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "lrf_mesh_smooth": (C.c_int, [C.POINTER(LrfMeshSmooth), _f, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_mesh_holes_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "lrf_mesh_holes": (C.c_int, [C.POINTER(LrfMeshHoles), C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_mesh_fill": (C.c_int, [C.POINTER(LrfMeshHoles), _f, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "lrf_mesh_rasterize_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "lrf_mesh_rasterize": (C.c_int, [C.POINTER(LrfMeshRaster), _f, C.c_void_p, C.c_void_p, _f, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "lrf_debug_mesh_rasterize": (C.c_int, [C.POINTER(LrfMeshRaster), _f, C.c_void_p, C.c_void_p, _f, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p]),
    "lrf_depth_agreement": (C.c_int, [_f, _f, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.c_float,
                                      C.c_float, C.c_void_p, _f, C.c_void_p]),
    "lrf_mesh_index_bounds": (C.c_int, [_f, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "lrf_mesh_index_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "lrf_mesh_index_build": (C.c_int, [C.POINTER(LrfMeshIndex), C.c_void_p, C.c_void_p]),
    "lrf_mesh_closest": (C.c_int, [C.POINTER(LrfMeshIndex), _f, C.c_int64, C.c_double, _f, C.c_void_p, _f, C.c_void_p]),
    "lrf_mesh_sample_count": (C.c_int, [_f, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_mesh_sample_emit": (C.c_int, [_f, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_int64, _f, C.c_void_p,
                                       C.c_void_p]),
    "lrf_distance_summary": (C.c_int, [_f, C.c_int64, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "lrf_align_transform": (C.c_int, [C.POINTER(C.c_double), _f, C.c_int64, _f, C.c_void_p]),
    "lrf_align_pairs": (C.c_int, [C.POINTER(LrfAlignFrame), _f, _f, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "lrf_align_plane": (C.c_int, [C.POINTER(LrfAlignPlane), C.c_void_p, C.c_void_p]),
    "lrf_align_plane_cloud": (C.c_int, [C.POINTER(LrfAlignPlaneCloud), C.c_void_p, C.c_void_p]),
    "lrf_cloud_index_bounds": (C.c_int, [_f, C.c_int64, C.c_void_p, C.c_void_p]),
    "lrf_cloud_index_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "lrf_cloud_index_build": (C.c_int, [C.POINTER(LrfCloudIndex), C.c_void_p]),
    "lrf_cloud_closest": (C.c_int, [C.POINTER(LrfCloudIndex), _f, C.c_int64, C.c_double, _f, C.c_void_p, _f, C.c_void_p]),
    "lrf_cloud_knn": (C.c_int, [C.POINTER(LrfCloudIndex), _f, C.c_int64, C.c_int32, C.c_double, C.c_int64, _f, C.c_void_p, C.c_void_p]),
    "lrf_cloud_radius_count": (C.c_int, [C.POINTER(LrfCloudIndex), _f, C.c_int64, C.c_double, C.c_int64, C.c_void_p, C.c_void_p]),
    "lrf_cloud_normals": (C.c_int, [C.POINTER(LrfCloudIndex), _f, C.c_int64, C.c_double, C.c_double, C.c_int32, _f, C.c_int64, _f, _f,
                                    C.c_void_p, C.c_void_p]),
    "lrf_cloud_voxel_bounds": (C.c_int, [_f, C.c_int64, C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_void_p]),
    "lrf_cloud_voxel_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "lrf_cloud_voxel": (C.c_int, [C.POINTER(LrfCloudVoxel), _f, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrf_mesh_texture_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "lrf_mesh_texture_bake": (C.c_int, [C.POINTER(LrfMeshTexture), _f, C.c_void_p]),
    "lrf_mesh_texture_resolve": (C.c_int, [C.POINTER(LrfMeshTexture), _f, C.POINTER(C.c_uint8), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "lrf_density_gradient": (C.c_int, [C.POINTER(LrfField), _f, C.c_int64, _f, _f, C.c_void_p]),
    "lrf_normals_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lrf_render_normals": (C.c_int, [C.POINTER(LrfField), _f, _f, C.c_int32, C.c_int32, C.c_uint32, C.c_float, _f, C.c_int32,
                                     C.c_int32, _f, _f, C.c_void_p, C.c_void_p]),
    "lrf_quantile_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lrf_render_depth_quantiles": (C.c_int, [C.POINTER(LrfField), _f, _f, C.c_int32, C.c_int32, C.c_uint32, C.c_float,
                                             C.POINTER(C.c_float), C.c_int32, _f, C.c_int32, C.c_int32, _f, _f, C.c_void_p, _f,
                                             C.c_void_p, C.c_void_p]),
    "lrf_depth_quantiles_from_weights": (C.c_int, [_f, _f, _f, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32, _f,
                                                   C.c_void_p, C.c_void_p]),
    "lrf_scene_blend_bwd": (C.c_int, [_f, _f, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, _f, _f, _f,
                                      C.c_void_p]),
}

_lib = None


class NativeError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"localrf_amd: {LIB_PATH} not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback for the render path.")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(h, name)          # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if h.lrf_abi_version() != 7:
            raise NativeError("localrf_amd: ABI version mismatch")
        _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        raise NativeError(f"{what} failed: {lib().lrf_last_error().decode()}")


def call(name, *args):
    """lib().<name>(*args); a non-zero return raises NativeError naming the symbol, with lrf_last_error()."""
    check(getattr(lib(), name)(*args), name)


def torch_stream(dev=None):
    """The current torch stream of dev (None: of the current device), for events, waits and synchronize()."""
    return torch.cuda.current_stream(dev)


def stream(dev):
    """The hipStream_t of dev's current stream: the trailing argument of nearly every entry point."""
    return torch.cuda.current_stream(dev).cuda_stream


def launch(name, dev, *args, guard=False):
    """call(name, *args, stream(dev)).  guard=True makes dev the current device for the duration of the call.
    Who guards: the evaluation-side features that take arbitrary caller tensors (frames, metrics, diagnostics, novel_views,
    pointcloud), so that they work on a device other than the current one.  The training path (field, scene_ops, losses,
    optim) does not: it runs ~70 launches per iteration on the device the scene was built on, and a torch.cuda.device
    context around each would cost host time nobody has measured."""
    if guard:
        with torch.cuda.device(dev):
            call(name, *args, stream(dev))
    else:                                    # spelled out, not call(..., stream(dev)): the training path comes through here
        check(getattr(_lib or lib(), name)(*args, torch.cuda.current_stream(dev).cuda_stream), name)


def workspace(name, dev, *shape):
    """The scratch buffer of entry point family `name`: <name>_workspace_bytes(*shape) bytes of uint8 on dev.  A size of 0
    is the library refusing the shape."""
    nbytes = getattr(lib(), name + "_workspace_bytes")(*shape)
    if nbytes == 0:
        raise NativeError(f"{name}: refused shape {shape}")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def require_gpu(t, name, feature):
    """t is a tensor on the GPU, or this raises.  name: the argument's; feature: whose kernels would have run ("metrics",
    "the render path", ...).  Only t.device is read (anything that carries a torch.device counts as a tensor), so the
    check costs the hot path an attribute read."""
    dev = getattr(t, "device", None)
    if not isinstance(dev, torch.device):
        raise TypeError(f"{name} must be a torch tensor")
    if dev.type != "cuda":
        raise NativeError(f"localrf_amd: {name} lives on {dev}; {feature} can run only on an AMD GPU (HIP kernels). "
                          "There is no CPU fallback.")


def conform(t, dtype=torch.float32):
    """Contiguous `dtype` form of t for a native call.  Only data_ptr() is taken, so an already conforming tensor comes
    back as is: detach() alone costs ~4 us, 70 of them per training iteration."""
    if t.dtype is dtype and t.is_contiguous():
        return t
    return t.detach().to(dtype).contiguous()


def ptr(t):
    """Device pointer of a contiguous fp32 torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "native call needs contiguous tensors"
    return C.c_void_p(t.data_ptr())
