"""ctypes declarations for libpcpx.so (include/pcpx.h).  Fails loudly if the library is missing:
there is no Python or CPU fallback for the compute path."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCPX_LIB") or os.path.join(HERE, "libpcpx.so")  # PCPX_LIB: tuning variants (tools/)

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)

ABI_VERSION = 5  # include/pcpx.h PCPX_ABI_VERSION
PCPX_OK = 0
PCPX_ERR_INVALID = -1
PCPX_ERR_DEVICE = -2
PCPX_ERR_ALLOC = -3
PCPX_ERR_CAPACITY = -4
PCPX_ERR_UNSUPPORTED = -5
PCPX_BUILD_USE_GRID = 1
PCPX_BUILD_COARSE_ORDER = 2
PCPX_BUILD_SHARD = 4
PCPX_BUILD_BORROW_CLOUD = 8
PCPX_BUILD_SHARD_RANGE = 16
UINT64_MAX = 0xFFFFFFFFFFFFFFFF


class BuildParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("grid_min", C.c_float * 3),
                ("grid_max", C.c_float * 3), ("shard_rank", C.c_uint32), ("shard_world", C.c_uint32),
                ("shard_k_hint", C.c_uint32), ("reserved", C.c_uint32), ("shard_first", C.c_uint64), ("shard_count", C.c_uint64)]


class Profile(C.Structure):
    _fields_ = [("launches", C.c_uint32 * 5), ("total_ms", C.c_float * 5)]


class Grid3d(C.Structure):
    """pcpx_grid3d ~ pcp::common::regular_grid3d_t<float>: origin, voxel size, voxels per axis."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float),
                ("sx", C.c_uint64), ("sy", C.c_uint64), ("sz", C.c_uint64)]


class HierarchyParams(C.Structure):
    """pcpx_hierarchy_params ~ pcp::algorithm::hierarchy::params_t (struct_size first)."""
    _fields_ = [("struct_size", C.c_uint32), ("cluster_size", C.c_uint64), ("var_max", C.c_double)]


class PlaneParams(C.Structure):
    """pcpx_plane_params (include/pcpx_planes.h)."""
    _fields_ = [("hypotheses", C.c_uint64), ("seed", C.c_uint32), ("flags", C.c_uint32), ("max_distance", C.c_float),
                ("min_normal_cos", C.c_float), ("axis", C.c_float * 3), ("min_axis_cos", C.c_float), ("origin_row", C.c_uint32),
                ("min_inliers", C.c_uint32), ("max_planes", C.c_uint32), ("reserved", C.c_uint32)]


class ShapeParams(C.Structure):
    """pcpx_shape_params (include/pcpx_shapes.h)."""
    _fields_ = [("hypotheses", C.c_uint64), ("kind", C.c_uint32), ("seed", C.c_uint32), ("flags", C.c_uint32), ("max_distance", C.c_float),
                ("min_radius", C.c_float), ("max_radius", C.c_float), ("min_normal_sin", C.c_float), ("min_normal_cos", C.c_float),
                ("axis", C.c_float * 3), ("min_axis_cos", C.c_float), ("origin_row", C.c_uint32), ("reserved", C.c_uint32)]


class VoxelParams(C.Structure):
    """pcpx_voxel_params (include/pcpx_voxel.h)."""
    _fields_ = [("leaf", C.c_float * 3), ("origin", C.c_float * 3), ("flags", C.c_uint32), ("attr_columns", C.c_uint32), ("reserved", C.c_uint32)]


class FpsParams(C.Structure):
    """pcpx_fps_params (include/pcpx_fps.h)."""
    _fields_ = [("flags", C.c_uint32), ("start", C.c_uint32), ("stop_radius", C.c_float), ("reserved", C.c_uint32)]


class ObjectsParams(C.Structure):
    """pcpx_objects_params (include/pcpx_objects.h)."""
    _fields_ = [("flags", C.c_uint32), ("none_label", C.c_uint32), ("min_size", C.c_uint32), ("max_size", C.c_uint32), ("reserved", C.c_uint32)]


K_BUILD, K_KNN, K_NORMALS, K_RANGE, K_QUERY_PREP = range(5)


class PcpxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("pcpx status %d: %s" % (status, message))
        self.status = status


# name -> (restype, argtypes); every symbol declared in include/pcpx.h
SIGNATURES = {
    "pcpx_abi_version": (C.c_int, []),
    "pcpx_last_error": (C.c_char_p, []),
    "pcpx_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "pcpx_index_create": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(BuildParams), C.c_int, C.POINTER(C.c_void_p)]),
    "pcpx_index_create_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(BuildParams), C.c_int, C.c_void_p,
                                        C.POINTER(C.c_void_p)]),
    "pcpx_index_rebuild": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BuildParams)]),
    "pcpx_index_rebuild_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BuildParams)]),
    "pcpx_index_destroy": (None, [C.c_void_p]),
    "pcpx_index_size": (C.c_int, [C.c_void_p, u64p]),
    "pcpx_index_trim": (C.c_int, [C.c_void_p]),
    "pcpx_index_shard_info": (C.c_int, [C.c_void_p, u64p]),
    "pcpx_knn_self_curve_order_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "pcpx_index_perm_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_estimate_normals_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "pcpx_index_bbox": (C.c_int, [C.c_void_p, f32p]),
    "pcpx_bounding_box": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, f32p]),
    "pcpx_bounding_box_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    "pcpx_knn_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_knn_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "pcpx_knn_self_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "pcpx_knn_self_strided_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "pcpx_normals_knn_self_strided_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                                    C.c_void_p, C.c_void_p]),
    "pcpx_knn_group_costs_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_uint64, u64p]),
    "pcpx_shard_cuts_by_cost": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, u64p]),
    "pcpx_debug_set": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "pcpx_debug_get": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "pcpx_debug_group_times": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "pcpx_knn_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "pcpx_range_count_self": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p]),
    "pcpx_range_count_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p]),
    "pcpx_range_count_self_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pcpx_range_count_self_curve_order_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p]),
    "pcpx_range_lists_self_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "pcpx_range_sphere_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint64, C.c_void_p,
                                          C.c_void_p, C.c_uint64]),
    "pcpx_range_aabb_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "pcpx_normals_knn_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_normals_knn_self_curve_order": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_normals_knn_self_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "pcpx_tangent_planes_knn_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
    "pcpx_mean_knn_distance_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "pcpx_neighbourhoods_self_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "pcpx_propagate_normal_orientations": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                     u64p]),
    "pcpx_propagate_normal_orientations_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                         C.c_int, C.c_void_p, u64p, C.POINTER(C.c_uint32)]),
    "pcpx_orient_normals_knn_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, u64p]),
    "pcpx_oriented_normals_knn_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, u64p]),
    "pcpx_normals_from_knn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                        C.c_void_p]),
    "pcpx_estimate_normal": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, f32p]),
    "pcpx_shard_range": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, u64p, u64p]),
    "pcpx_bilateral_filter_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int, C.c_void_p]),
    "pcpx_bilateral_filter_normals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int, C.c_void_p]),
    "pcpx_bilateral_filter_points_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int,
                                                   C.c_void_p, C.c_void_p]),
    "pcpx_bilateral_filter_normals_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int,
                                                    C.c_void_p, C.c_void_p]),
    "pcpx_wlop": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int, C.c_int, C.c_void_p]),
    "pcpx_wlop_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p]),
    "pcpx_device_malloc": (C.c_int, [C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]),
    "pcpx_device_free": (None, [C.c_void_p, C.c_int]),
    "pcpx_device_trim": (C.c_int, [C.c_int]),
    "pcpx_device_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "pcpx_device_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "pcpx_comm_unique_id": (C.c_int, [C.c_char_p]),
    "pcpx_comm_init_rank": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "pcpx_comm_wrap": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "pcpx_comm_destroy": (None, [C.c_void_p]),
    "pcpx_comm_allgather_boxes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_comm_global_grid_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, f32p]),
    "pcpx_index_synchronize": (C.c_int, [C.c_void_p]),
    "pcpx_debug_knn_stats": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, u64p, C.c_uint64]),
    "pcpx_debug_eps_test_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "pcpx_debug_sort_keys": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]),
    "pcpx_debug_tree": (C.c_int, [C.c_void_p, u64p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u32p]),
    "pcpx_profile_begin": (C.c_int, [C.c_void_p]),
    "pcpx_profile_end": (C.c_int, [C.c_void_p, C.POINTER(Profile)]),
    "pcpx_kd_create": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "pcpx_kd_destroy": (None, [C.c_void_p]),
    "pcpx_kd_size": (C.c_uint64, [C.c_void_p]),
    "pcpx_kd_dims": (C.c_uint32, [C.c_void_p]),
    "pcpx_kd_knn_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_regular_grid_containing": (C.c_int, [f32p, f32p, u64p, C.POINTER(Grid3d)]),
    "pcpx_surface_nets_dev": (C.c_int, [C.c_void_p, C.POINTER(Grid3d), C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_uint64, u64p, u64p]),
    "pcpx_surface_nets_timed_dev": (C.c_int, [C.c_void_p, C.POINTER(Grid3d), C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64,
                                              C.c_void_p, C.c_uint64, u64p, u64p, f32p]),
    "pcpx_surface_nets": (C.c_int, [C.c_void_p, C.POINTER(Grid3d), C.c_float, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                    u64p, u64p]),
    "pcpx_surface_nets_hint_dev": (C.c_int, [C.c_void_p, C.POINTER(Grid3d), C.c_float, f32p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_uint64, C.c_void_p, C.c_uint64, u64p, u64p, u64p]),
    "pcpx_surface_nets_hint_timed_dev": (C.c_int, [C.c_void_p, C.POINTER(Grid3d), C.c_float, f32p, C.c_uint64, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, u64p, u64p, f32p, u32p]),
    "pcpx_surface_nets_hint": (C.c_int, [C.c_void_p, C.POINTER(Grid3d), C.c_float, f32p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_uint64, u64p, u64p, u64p]),
    "pcpx_surface_nets_search_order": (C.c_int, [C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.POINTER(C.c_int)]),
    "pcpx_tangent_plane_sdf_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Grid3d), C.c_float, C.c_void_p]),
    "pcpx_reconstruct_surface": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, u64p, C.c_float, C.c_void_p, C.c_uint64, C.c_void_p,
                                           C.c_uint64, u64p, u64p, C.c_void_p, C.c_void_p, C.POINTER(Grid3d)]),
    "pcpx_reconstruct_surface_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, u64p, C.c_float, C.c_void_p, C.c_uint64, C.c_void_p,
                                               C.c_uint64, u64p, u64p, C.c_void_p, C.c_void_p, C.POINTER(Grid3d)]),
    "pcpx_kd_range_aabb_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "pcpx_hierarchy_simplification": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(HierarchyParams), C.c_int, C.c_void_p, C.c_void_p, C.c_uint64,
                                                u64p]),
    "pcpx_hierarchy_simplification_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(HierarchyParams), C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_uint64, u64p]),
}

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so (soname libamdhip64.so.7, the soname libpcpx.so
    needs).  Device pointers and streams can only be exchanged with torch (bench.py, multi-GPU path) if
    both sit on ONE HIP runtime, so when torch is installed its copy is loaded first -- without
    importing torch -- and libpcpx.so then binds to it by soname.  PCPX_HIP_RUNTIME=system skips this."""
    if os.environ.get("PCPX_HIP_RUNTIME", "") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # fall back to the RUNPATH copy under /opt/rocm


# name -> (restype, argtypes); every symbol declared in include/pcpx_radius.h (the fixed-radius neighbourhoods)
RADIUS_SIGNATURES = {
    "pcpx_range_neighbourhoods_self_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    "pcpx_range_neighbourhoods_self": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_range_neighbourhoods_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
}


# name -> (restype, argtypes); every symbol declared in include/pcpx_cluster.h (radius-connected components and DBSCAN)
PCPX_CLUSTER_NOISE = 0xFFFFFFFF
PCPX_CLUSTER_COMPACT = 1
CLUSTER_SIGNATURES = {
    "pcpx_cluster_self_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_cluster_self": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, u64p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_subsample.h (Poisson-disk subsampling)
PCPX_SUBSAMPLE_NONE = 0xFFFFFFFF
PCPX_SUBSAMPLE_ROUND_BATCH = 4
SUBSAMPLE_SIGNATURES = {
    "pcpx_subsample_self_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u32p]),
    "pcpx_subsample_self": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, u64p, u32p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_segment.h (smooth-surface segmentation)
PCPX_SEGMENT_NOISE = 0xFFFFFFFF
PCPX_SEGMENT_COMPACT = 1
PCPX_SEGMENT_ORIENTED = 2
SEGMENT_SIGNATURES = {
    "pcpx_segment_self_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "pcpx_segment_self": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_void_p, u64p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_features.h (local shape features)
FEATURES_SIGNATURES = {
    "pcpx_shape_features_self_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "pcpx_shape_features_self": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_shape_features_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_keypoints.h (local maxima over a radius, ISS keypoints)
KEYPOINTS_SIGNATURES = {
    "pcpx_local_maxima_self_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "pcpx_local_maxima_self": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, u64p]),
    "pcpx_iss_keypoints_self_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_iss_keypoints_self": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          u64p, C.c_void_p]),
}
# name -> (restype, argtypes); every symbol declared in include/pcpx_descriptors.h (FPFH descriptors)
DESCRIPTORS_SIGNATURES = {
    "pcpx_fpfh_self_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_fpfh_self": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
}
# name -> (restype, argtypes); every symbol declared in include/pcpx_match.h (descriptor matching)
PCPX_MATCH_MAX_DIMS = 64
PCPX_MATCH_NONE = 0xFFFFFFFF
PCPX_MATCH_SKIP_ZERO_ROWS = 1
PCPX_MATCH_MUTUAL = 2
MATCH_SIGNATURES = {
    "pcpx_match_plan": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, u32p, u32p, u64p, u64p]),
    "pcpx_match_nearest_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_match_nearest": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "pcpx_match_correspondences_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_uint32, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_match_correspondences": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_uint32, C.c_int,
                                             C.c_void_p, C.c_void_p, u64p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_register.h (rigid registration from correspondences)
PCPX_RANSAC_REFIT = 1
REGISTER_SIGNATURES = {
    "pcpx_ransac_plan": (C.c_int, [C.c_uint64, C.c_uint64, u32p, u64p, u64p]),
    "pcpx_ransac_rigid_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.c_float, C.c_float, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_ransac_rigid": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_float,
                                    C.c_float, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_rigid_fit_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_rigid_fit": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                 C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_icp.h (nearest partners under a pose, the ICP loop)
PCPX_ICP_NONE = 0xFFFFFFFF
PCPX_ICP_POINT_TO_PLANE = 1
PCPX_ICP_MAX_ITERATIONS = 1024
PCPX_ICP_EXHAUSTED, PCPX_ICP_CONVERGED, PCPX_ICP_STARVED, PCPX_ICP_DEGENERATE = range(4)
ICP_SIGNATURES = {
    "pcpx_nearest_posed_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "pcpx_nearest_posed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "pcpx_icp_rigid_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_icp_rigid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_gicp.h (Generalized ICP: the loop with a plane-to-plane step)
PCPX_GICP_COVARIANCES = 1
PCPX_GICP_ON_DEVICE = 2
_GICP_ARGS = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
GICP_SIGNATURES = {
    "pcpx_gicp_rigid": (C.c_int, list(_GICP_ARGS)),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_planes.h (plane detection)
PCPX_PLANE_REFIT = 1
PCPX_PLANE_NORMALS = 2
PCPX_PLANE_AXIS = 4
PCPX_PLANE_NONE = 0xFFFFFFFF
PCPX_PLANE_ORIGIN_FIRST = 0xFFFFFFFF
PCPX_PLANES_MAX = 64
_ppp = C.POINTER(PlaneParams)
PLANES_SIGNATURES = {
    "pcpx_plane_plan": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, u32p, u64p, u64p]),
    "pcpx_plane_ransac_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, _ppp, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_plane_ransac": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _ppp, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_plane_fit_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_plane_fit": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    "pcpx_extract_planes_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, _ppp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "pcpx_extract_planes": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, _ppp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_voxel.h (voxel-grid downsampling)
PCPX_VOXEL_ORIGIN = 1
PCPX_VOXEL_NONE = 0xFFFFFFFF
PCPX_VOXEL_ATTRS_MAX = 16
_pvp = C.POINTER(VoxelParams)
VOXEL_SIGNATURES = {
    "pcpx_voxel_plan": (C.c_int, [C.c_uint64, C.c_uint64, u64p, u64p]),
    "pcpx_voxel_grid_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, _pvp, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_voxel_grid": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, _pvp, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_mls.h (moving least squares projection)
PCPX_MLS_PIVOT_MIN = 1.0 / 4096.0
MLS_SIGNATURES = {
    "pcpx_mls_project_self_dev": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_mls_project_self": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "pcpx_mls_project_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_outliers.h (outlier removal: resolution, statistical, radius, density)
PCPX_OUTLIERS_ON_DEVICE = 1
OUTLIERS_SIGNATURES = {
    "pcpx_outliers_resolution_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pcpx_outliers_statistical_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    "pcpx_outliers_radius_self": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_outliers_density_self": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_boundary.h (boundary points: the largest empty angle)
PCPX_BOUNDARY_ON_DEVICE = 1
BOUNDARY_SIGNATURES = {
    "pcpx_boundary_self": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_objects.h (objects from labels)
PCPX_OBJECTS_ON_DEVICE = 1
PCPX_OBJECTS_SKIP = 2
PCPX_OBJECTS_NONE = 0xFFFFFFFF
PCPX_OBJECTS_CHUNK = 64
_pop = C.POINTER(ObjectsParams)
OBJECTS_SIGNATURES = {
    "pcpx_objects_plan": (C.c_int, [C.c_uint64, C.c_uint64, u64p, u64p]),
    "pcpx_label_objects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, _pop, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_fps.h (farthest point sampling)
PCPX_FPS_ON_DEVICE = 1
PCPX_FPS_NONE = 0xFFFFFFFF
PCPX_FPS_START_LOWEST = 0xFFFFFFFF
FPS_SIGNATURES = {
    "pcpx_farthest_points_self": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(FpsParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
}

# name -> (restype, argtypes); every symbol declared in include/pcpx_shapes.h (sphere and cylinder detection)
PCPX_SHAPE_SPHERE = 1
PCPX_SHAPE_CYLINDER = 2
PCPX_SHAPE_REFIT = 1
PCPX_SHAPE_NORMALS = 2
PCPX_SHAPE_AXIS = 4
PCPX_SHAPE_ON_DEVICE = 8
PCPX_SHAPE_ORIGIN_FIRST = 0xFFFFFFFF
PCPX_SHAPE_FIT_OK = 0
PCPX_SHAPE_FIT_DEGENERATE = 1
_psp = C.POINTER(ShapeParams)
SHAPES_SIGNATURES = {
    "pcpx_shape_plan": (C.c_int, [C.c_uint64, C.c_uint64, u32p, u64p, u64p]),
    "pcpx_shape_ransac": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, _psp, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pcpx_shape_fit": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
}


def load():
    """Load libpcpx.so; raises if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libpcpx.so is missing at %s: build it with `python __graft_entry__.py` (hipcc, gfx950). "
            "There is no CPU fallback for the pcpx compute path." % LIB_PATH)
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(RADIUS_SIGNATURES.items()) + list(CLUSTER_SIGNATURES.items())\
            + list(SUBSAMPLE_SIGNATURES.items()) + list(SEGMENT_SIGNATURES.items()) + list(FEATURES_SIGNATURES.items())\
            + list(KEYPOINTS_SIGNATURES.items()) + list(DESCRIPTORS_SIGNATURES.items()) + list(MATCH_SIGNATURES.items())\
            + list(REGISTER_SIGNATURES.items()) + list(ICP_SIGNATURES.items()) + list(GICP_SIGNATURES.items()) + list(PLANES_SIGNATURES.items())\
            + list(VOXEL_SIGNATURES.items()) + list(MLS_SIGNATURES.items()) + list(OUTLIERS_SIGNATURES.items())\
            + list(BOUNDARY_SIGNATURES.items()) + list(OBJECTS_SIGNATURES.items()) + list(FPS_SIGNATURES.items())\
            + list(SHAPES_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    if lib.pcpx_abi_version() != ABI_VERSION:
        raise ImportError("libpcpx.so ABI version mismatch")
    _lib = lib
    return lib


def check(status):
    if status != PCPX_OK:
        msg = load().pcpx_last_error()
        raise PcpxError(status, msg.decode("utf-8", "replace") if msg else "")
