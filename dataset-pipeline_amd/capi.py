"""ctypes binding of libe3dhip.so -- one Python method per C-ABI entry point of include/e3d_hip.h.

Array arguments may be numpy arrays (host) or torch CUDA tensors (device pointers are passed through;
the library detects them).  There is deliberately NO fallback path: if the shared library is missing the
import of any entry point fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class E3DError(RuntimeError):
    pass


def lib_path():
    return os.path.join(_HERE, "lib", "libe3dhip.so")


class PairRecord(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("src", C.c_int32), ("tgt", C.c_int32),
                ("count", C.c_int64), ("distance_sum", C.c_double)]


class UndistortPlan(C.Structure):
    """e3d_undistort_plan: a PINHOLE camera, (0, 0) = the centre of the top-left pixel."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]

    def astuple(self):
        return (self.width, self.height, self.fx, self.fy, self.cx, self.cy)


class StereoPlan(C.Structure):
    """e3d_stereo_plan: the common PINHOLE camera of a rectified pair, its baseline, the two rectified poses and source_T_rect rotations."""
    _fields_ = [("camera", UndistortPlan), ("baseline", C.c_float), ("q_rect", C.c_float * 4), ("t_left", C.c_float * 3),
                ("t_right", C.c_float * 3), ("S_left", C.c_float * 9), ("S_right", C.c_float * 9)]


UNDISTORT_U8, UNDISTORT_RGB, UNDISTORT_MASK, UNDISTORT_NEAREST = 0, 1, 2, 3
_UNDISTORT_PIXEL = {0: (np.uint8, ()), 1: (np.uint8, (3,)), 2: (np.uint8, ()), 3: (np.float32, ())}


class IterRecord(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("inner_iterations", C.c_int32), ("full_passes", C.c_int32),
                ("cost_passes", C.c_int32), ("multi_cost_passes", C.c_int32), ("multi_cost_poses", C.c_int32),
                ("correspondences", C.c_int64), ("queries", C.c_int64),
                ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("t_transform_ms", C.c_double), ("t_nn_ms", C.c_double), ("t_lm_ms", C.c_double),
                ("t_lm_kernel_ms", C.c_double), ("t_nn_query_ms", C.c_double), ("t_lm_full_kernel_ms", C.c_double),
                ("t_nn_certify_ms", C.c_double), ("t_nn_bounded_ms", C.c_double), ("t_nn_search_ms", C.c_double),
                ("nn_certify_queries", C.c_int64), ("nn_bounded_queries", C.c_int64), ("nn_search_queries", C.c_int64),
                ("nn_certify_launches", C.c_int32), ("nn_bounded_launches", C.c_int32), ("nn_search_launches", C.c_int32),
                ("lm_passes_skipped", C.c_int32), ("t_nn_sort_ms", C.c_double), ("t_nn_scan_ms", C.c_double), ("t_nn_compact_ms", C.c_double),
                ("corr_rows_rewritten", C.c_int64), ("corr_rows_walked", C.c_int64),
                ("nn_update_launches", C.c_int32), ("nn_kernel_launches", C.c_int32), ("nn_batches", C.c_int32), ("nn_sort_calls", C.c_int32)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_size_t, C.c_void_p)
ALLREDUCE_DEVICE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)

# name -> (restype, argtypes); also the list of symbols include/e3d_hip.h declares
SIGNATURES = {
    "e3d_abi_version": (C.c_int, []),
    "e3d_init": (C.c_int, [C.c_int]),
    "e3d_last_error": (C.c_char_p, []),
    "e3d_set_nn_mode": (C.c_int, [C.c_int]),
    "e3d_icp_create": (C.c_void_p, []),
    "e3d_icp_destroy": (None, [C.c_void_p]),
    "e3d_icp_add_cloud": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    "e3d_icp_run": (C.c_int, [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int]),
    "e3d_icp_get_pose": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "e3d_icp_set_max_inner_iterations": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_icp_set_sequential_distance_sum": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_icp_set_resident_rows": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_icp_num_pair_records": (C.c_size_t, [C.c_void_p]),
    "e3d_icp_pair_records": (C.POINTER(PairRecord), [C.c_void_p]),
    "e3d_icp_num_iter_records": (C.c_size_t, [C.c_void_p]),
    "e3d_icp_iter_records": (C.POINTER(IterRecord), [C.c_void_p]),
    "e3d_icp_clear_records": (None, [C.c_void_p]),
    "e3d_icp_set_shard": (C.c_int, [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]),
    "e3d_comm_unique_id": (C.c_int, [C.c_void_p]),
    "e3d_comm_create": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "e3d_comm_create_all": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_comm_destroy": (None, [C.c_void_p]),
    "e3d_comm_abort": (C.c_int, [C.c_void_p]),
    "e3d_comm_get_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "e3d_comm_rank": (C.c_int, [C.c_void_p]),
    "e3d_comm_world_size": (C.c_int, [C.c_void_p]),
    "e3d_icp_set_comm": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_set_comm": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_kernel_times": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "e3d_reg_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]),
    "e3d_find_correspondences": (C.c_int64, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float,
                                             C.c_void_p, C.c_void_p]),
    "e3d_transform_cloud": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "e3d_icp_pair_system": (C.c_int, [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 7),
    "e3d_libm_eval": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "e3d_normals_knn": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_normals_radius": (C.c_int, [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_release_workspaces": (C.c_int, []),
    "e3d_local_outlier_removal": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]),
    # (B) image registration kernels
    "e3d_reg_create": (C.c_void_p, [C.c_void_p]),
    "e3d_reg_destroy": (None, [C.c_void_p]),
    "e3d_reg_set_params": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_set_point_scale": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_variable_descriptors": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_get_variable_descriptors": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_camera_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "e3d_reg_set_depth_maps": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "e3d_reg_set_depth_map_level0": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "e3d_reg_get_depth_map": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "e3d_reg_set_rig_depth_residuals": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_reg_depth_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_depth_cost": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_intrinsics": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "e3d_reg_get_intrinsics_level": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_image": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_image_pose": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_splat_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "e3d_reg_add_occlusion_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]),
    "e3d_reg_clear_occlusion_meshes": (C.c_int, [C.c_void_p]),
    "e3d_reg_set_occlusion_options": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int]),
    "e3d_reg_occlusion_edge_count": (C.c_int64, [C.c_void_p, C.c_int]),
    "e3d_reg_render_depth": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "e3d_reg_observe": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "e3d_reg_get_observations": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_observations": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_pass1": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_cost": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_color_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_reg_color_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "e3d_reg_color_finish": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_reg_get_image_pose": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_update_observations": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_reg_set_scan_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "e3d_reg_count_scan_observations": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "e3d_reg_get_scan_observation_counts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_set_scan_observation_counts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_scan_colors_begin": (C.c_int, [C.c_void_p]),
    "e3d_reg_scan_colors_add_image": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "e3d_reg_scan_colors_get_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_scan_colors_set_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_scan_colors_finish": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_ground_truth_depth": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_scan_rendering": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "e3d_reg_mask_transfer_source": (C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "e3d_reg_mask_transfer_target": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_pick_scan_points": (C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_image_bearings": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "e3d_reg_project_points": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "e3d_reg_undistort_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p]),
    "e3d_reg_undistort": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_undistort_kernel_ms": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_stereo_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_void_p]),
    "e3d_reg_stereo_rectify": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_stereo_kernel_ms": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_stereo_ground_truth": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_pose_from_bearings": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_cache_observations": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_reg_determine_observed_indices": (C.c_int, [C.c_void_p]),
    "e3d_reg_get_observed_indices": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "e3d_reg_set_observed_indices": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "e3d_reg_color_update": (C.c_int, [C.c_void_p]),
    "e3d_reg_compute_cost": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_reg_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_reg_run_on_current_scale": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_set_rig": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_get_rig": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_reg_add_rig_images": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "e3d_determine_point_neighbors": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "e3d_reg_point_radius_minmax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "e3d_merge_close_points": (C.c_int64, [C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "e3d_reg_set_shard": (C.c_int, [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, ALLREDUCE_DEVICE_FN, C.c_void_p]),
    "e3d_reg_image_owner": (C.c_int, [C.c_void_p, C.c_int]),
    "e3d_mesh_squared_distance": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float,
                                            C.c_void_p, C.c_void_p]),
    "e3d_create_splats": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float,
                                      C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_render_cube_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_cube_map_timings": (C.c_int, [C.c_void_p]),
    # PointCloudEditor: selections and edits of one object's points
    "e3d_edit_create": (C.c_void_p, [C.c_void_p, C.c_size_t]),
    "e3d_edit_destroy": (None, [C.c_void_p]),
    "e3d_edit_size": (C.c_int64, [C.c_void_p]),
    "e3d_edit_get_points": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_edit_get_selection": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_edit_set_selection": (C.c_int64, [C.c_void_p, C.c_void_p]),
    "e3d_edit_selection_count": (C.c_int64, [C.c_void_p]),
    "e3d_edit_lasso": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "e3d_edit_beyond_plane": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "e3d_edit_pick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "e3d_edit_delete_selected": (C.c_int64, [C.c_void_p]),
    "e3d_edit_extract_selected": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "e3d_edit_kernel_ms": (C.c_int, [C.c_void_p, C.c_void_p]),
    # SurfaceReconstructor: an occlusion mesh from an oriented point cloud
    "e3d_surface_reconstruct": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float]),
    "e3d_surface_destroy": (None, [C.c_void_p]),
    "e3d_surface_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_surface_get_corners": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_surface_get_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_surface_kernel_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "e3d_surface_reconstruct_csg": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p, C.c_size_t]),
    "e3d_surface_reconstruct_filled": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_size_t]),
    "e3d_surface_get_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    # ReconstructionEvaluator: accuracy and completeness of a reconstruction against the scans
    "e3d_evaluate_reconstruction": (C.c_void_p, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int]),
    "e3d_eval_destroy": (None, [C.c_void_p]),
    "e3d_eval_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_eval_get_scores": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_eval_get_classes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_eval_get_voxels": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "e3d_eval_kernel_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "e3d_evaluate_disparity": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "e3d_disp_eval_destroy": (None, [C.c_void_p]),
    "e3d_disp_eval_get_counts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_disp_eval_get_sums": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_disp_eval_get_quantiles": (C.c_int, [C.c_void_p, C.c_void_p]),
    "e3d_disp_eval_kernel_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
}


ABI_VERSION = 5          # E3D_ABI_VERSION of include/e3d_hip.h


def lib():
    """Load libe3dhip.so (raises E3DError if it has not been built -- no fallback)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise E3DError("HIP extension missing: %s (run `python dataset-pipeline_amd/build.py`)" % p)
        # One HIP runtime per process: the ROCm torch wheel carries its own libamdhip64.  If torch is imported AFTER this
        # library has pulled in the system runtime, torch.cuda sees no device; imported first, both bind to the same copy
        # (measured on the MI355X box, tools/probe_hip_runtime.py).  torch is optional -- only tests / bench.py / dist.py use it.
        if os.environ.get("E3D_NO_TORCH_PRELOAD", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:  # noqa: BLE001
                pass
        L = C.CDLL(p)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        if L.e3d_abi_version() != ABI_VERSION:      # the structures below mirror include/e3d_hip.h of that version
            raise E3DError("libe3dhip.so has ABI version %d, this binding expects %d: rebuild (python dataset-pipeline_amd/build.py)"
                           % (L.e3d_abi_version(), ABI_VERSION))
        _LIB = L
    return _LIB


def _err(prefix, code=None):
    msg = lib().e3d_last_error()
    raise E3DError("%s: %s%s" % (prefix, msg.decode() if msg else "unknown error",
                                 "" if code is None else " (code %d)" % code))


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _ptr(a, dtype, keep):
    """Pointer of a numpy array / torch tensor with the given numpy dtype (contiguous); None passes through."""
    if a is None:
        return None
    if _is_torch(a):
        import torch
        want = {np.float32: torch.float32, np.int32: torch.int32, np.float64: torch.float64, np.uint8: torch.uint8}[dtype]
        t = a.contiguous()
        if t.dtype != want:
            t = t.to(want)
        keep.append(t)
        if t.is_cuda:
            # the library reads device memory on its own (non-blocking) stream: wait for the work torch queued on the
            # tensor's device before handing the pointer over
            torch.cuda.current_stream(t.device).synchronize()
        return C.c_void_p(t.data_ptr())
    arr = np.ascontiguousarray(a, dtype=dtype)
    keep.append(arr)
    return C.c_void_p(arr.ctypes.data)


def _pose12(T):
    T = np.asarray(T, dtype=np.float32)
    return np.ascontiguousarray(T[:3, :4])


class PointToPlaneICP:
    """Host-side mirror of icp::PointToPlaneICP (src/icp/icp_point_to_plane.h:39-80) on the HIP library."""

    def __init__(self, device=None):
        L = lib()
        if device is not None and L.e3d_init(int(device)) < 0:
            _err("e3d_init")
        self._h = L.e3d_icp_create()
        if not self._h:
            _err("e3d_icp_create")
        self._cb = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().e3d_icp_destroy(h)
            self._h = None

    # int AddPointCloud(cloud, global_T_cloud, fixed)
    def add_point_cloud(self, xyz, normals, global_T_cloud, fixed):
        keep = []
        n = int(xyz.shape[0])
        T = _pose12(global_T_cloud)
        r = lib().e3d_icp_add_cloud(self._h, _ptr(xyz, np.float32, keep), _ptr(normals, np.float32, keep), n,
                                    C.c_void_p(T.ctypes.data), int(bool(fixed)))
        if r < -1:
            _err("e3d_icp_add_cloud", r)
        return r

    # bool Run(max_correspondence_distance, initial_iteration, max_num_iterations, thr, print_progress)
    def run(self, max_correspondence_distance, initial_iteration, max_num_iterations,
            convergence_threshold_max_movement, print_progress=False):
        r = lib().e3d_icp_run(self._h, float(np.float32(max_correspondence_distance)), int(initial_iteration),
                              int(max_num_iterations), float(np.float32(convergence_threshold_max_movement)),
                              int(bool(print_progress)))
        if r < 0:
            _err("e3d_icp_run", r)
        return bool(r)

    # Eigen::Affine3f GetResultGlobalTCloud(int)
    def get_result_global_T_cloud(self, cloud_index):
        T = np.zeros((3, 4), np.float32)
        r = lib().e3d_icp_get_pose(self._h, int(cloud_index), C.c_void_p(T.ctypes.data))
        if r < 0:
            if r == -5:
                raise IndexError(cloud_index)
            _err("e3d_icp_get_pose", r)
        out = np.eye(4, dtype=np.float32)
        out[:3] = T
        return out

    def set_sequential_distance_sum(self, enable):
        if lib().e3d_icp_set_sequential_distance_sum(self._h, int(bool(enable))) < 0:
            _err("e3d_icp_set_sequential_distance_sum")

    def set_resident_rows(self, enable):
        """Resident correspondence rows (default) or rows compacted afresh every outer iteration (include/e3d_hip.h)."""
        if lib().e3d_icp_set_resident_rows(self._h, int(bool(enable))) < 0:
            _err("e3d_icp_set_resident_rows")

    def set_max_inner_iterations(self, n):
        if lib().e3d_icp_set_max_inner_iterations(self._h, int(n)) < 0:
            _err("e3d_icp_set_max_inner_iterations")

    def set_comm(self, comm):
        """Native multi-GPU mode: `comm` is a Comm (the library's RCCL communicator); replaces set_shard."""
        self._comm = comm
        if lib().e3d_icp_set_comm(self._h, comm.handle if comm is not None else None) < 0:
            _err("e3d_icp_set_comm")

    def set_shard(self, rank, world_size, allreduce=None):
        """allreduce(np.ndarray float64, in place) -> None; called from inside run()."""
        if allreduce is not None:
            def _cb(buf, count, _user):
                try:
                    arr = np.ctypeslib.as_array(buf, shape=(count,))
                    allreduce(arr)
                    return 0
                except Exception:  # noqa: BLE001 -- must not propagate through C
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = ALLREDUCE_FN(_cb)
        else:
            self._cb = ALLREDUCE_FN()
        if lib().e3d_icp_set_shard(self._h, int(rank), int(world_size), self._cb, None) < 0:
            _err("e3d_icp_set_shard")

    def pair_records(self):
        n = lib().e3d_icp_num_pair_records(self._h)
        p = lib().e3d_icp_pair_records(self._h)
        return [(p[i].iteration, p[i].src, p[i].tgt, p[i].count, p[i].distance_sum) for i in range(n)]

    def iter_records(self):
        n = lib().e3d_icp_num_iter_records(self._h)
        p = lib().e3d_icp_iter_records(self._h)
        names = [f[0] for f in IterRecord._fields_]
        return [{k: getattr(p[i], k) for k in names} for i in range(n)]

    def clear_records(self):
        lib().e3d_icp_clear_records(self._h)


def find_correspondences(source_xyz, target_xyz, max_correspondence_distance):
    """FindCorrespondencesFast: returns (match_index[n_src] int32 (-1 = none), sq_distance[n_src], count)."""
    keep = []
    ns, nt = int(source_xyz.shape[0]), int(target_xyz.shape[0])
    idx = np.full(max(ns, 1), -1, np.int32)
    d2 = np.zeros(max(ns, 1), np.float32)
    c = lib().e3d_find_correspondences(_ptr(source_xyz, np.float32, keep), ns, _ptr(target_xyz, np.float32, keep), nt,
                                       float(np.float32(max_correspondence_distance)),
                                       C.c_void_p(idx.ctypes.data), C.c_void_p(d2.ctypes.data))
    if c < 0:
        _err("e3d_find_correspondences", c)
    return idx[:ns], d2[:ns], int(c)


def transform_cloud(xyz, normals, T):
    keep = []
    n = int(xyz.shape[0])
    T = _pose12(T)
    oxyz = np.zeros((n, 3), np.float32)
    onrm = np.zeros((n, 3), np.float32)
    bmin = np.zeros(3, np.float32)
    bmax = np.zeros(3, np.float32)
    r = lib().e3d_transform_cloud(_ptr(xyz, np.float32, keep), _ptr(normals, np.float32, keep), n,
                                  C.c_void_p(T.ctypes.data), C.c_void_p(oxyz.ctypes.data),
                                  C.c_void_p(onrm.ctypes.data), C.c_void_p(bmin.ctypes.data),
                                  C.c_void_p(bmax.ctypes.data))
    if r < 0:
        _err("e3d_transform_cloud", r)
    return oxyz, onrm, bmin, bmax


def icp_pair_system(sxyz, snrm, txyz, tnrm, iq, im, sq, st, tq, tt):
    keep = []
    H = np.zeros((12, 12)); b = np.zeros(12); cost = np.zeros(1)
    r = lib().e3d_icp_pair_system(
        _ptr(sxyz, np.float32, keep), _ptr(snrm, np.float32, keep), _ptr(txyz, np.float32, keep),
        _ptr(tnrm, np.float32, keep), _ptr(iq, np.int32, keep), _ptr(im, np.int32, keep), int(len(iq)),
        _ptr(sq, np.float32, keep), _ptr(st, np.float32, keep), _ptr(tq, np.float32, keep),
        _ptr(tt, np.float32, keep), C.c_void_p(H.ctypes.data), C.c_void_p(b.ctypes.data),
        C.c_void_p(cost.ctypes.data))
    if r < 0:
        _err("e3d_icp_pair_system", r)
    return H, b, float(cost[0])


class Comm:
    """The library's RCCL communicator (include/e3d_hip.h: e3d_comm_*).  One rank per GPU.

    Processes: rank 0 calls Comm.unique_id(), ships the 128 bytes through the launcher's rendezvous, every rank builds
    Comm(id_bytes, rank, world, device).  Threads of one process: Comm.create_all(n_devices)."""

    def __init__(self, id_bytes=None, rank=0, world_size=1, device=0, _handle=None):
        if _handle is not None:
            self.handle = _handle
        else:
            if id_bytes is None:
                id_bytes = Comm.unique_id()
            buf = C.create_string_buffer(bytes(id_bytes), 128)
            self.handle = lib().e3d_comm_create(buf, int(rank), int(world_size), int(device))
            if not self.handle:
                _err("e3d_comm_create")
        self.rank = lib().e3d_comm_rank(self.handle)
        self.world_size = lib().e3d_comm_world_size(self.handle)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        if lib().e3d_comm_unique_id(buf) < 0:
            _err("e3d_comm_unique_id")
        return buf.raw

    @staticmethod
    def create_all(n_devices, devices=None):
        out = (C.c_void_p * n_devices)()
        dev = (C.c_int * n_devices)(*(devices if devices is not None else range(n_devices)))
        if lib().e3d_comm_create_all(int(n_devices), dev, out) < 0:
            _err("e3d_comm_create_all")
        return [Comm(_handle=out[i]) for i in range(n_devices)]

    def stats(self, reset=False):
        """(all-reduce milliseconds by HIP events, calls, payload bytes) of this rank since creation / the last reset."""
        ms, calls, nbytes = C.c_double(0), C.c_int64(0), C.c_int64(0)
        if lib().e3d_comm_get_stats(self.handle, C.byref(ms), C.byref(calls), C.byref(nbytes), int(bool(reset))) < 0:
            _err("e3d_comm_get_stats")
        return ms.value, calls.value, nbytes.value

    def destroy(self):
        if self.handle:
            lib().e3d_comm_destroy(self.handle)
            self.handle = None


def release_workspaces():
    """Free the device workspaces e3d_normals_knn / e3d_local_outlier_removal parked for their next call."""
    lib().e3d_release_workspaces()


def libm_eval(fn, x, y=None):
    """include/e3d_libm.h evaluated by a HIP kernel; fn in {"atanf", "atan2f", "sinf", "cosf", "tanf", "log2f"}."""
    code = {"atanf": 0, "atan2f": 1, "sinf": 2, "cosf": 3, "tanf": 4, "log2f": 5}[fn]
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), np.float32)
    out = np.zeros_like(x)
    r = lib().e3d_libm_eval(code, C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), x.size, C.c_void_p(out.ctypes.data))
    if r < 0:
        _err("e3d_libm_eval", r)
    return out


def normals_knn(xyz, k, viewpoint=(0.0, 0.0, 0.0), return_knn=False):
    """NormalEstimationTwoPassOMP with setKSearch(k): returns (normals[n,3], curvature[n][, knn_idx[n,k]])."""
    keep = []
    n = int(xyz.shape[0])
    vp = np.ascontiguousarray(viewpoint, np.float32)
    on = np.zeros((n, 3), np.float32)
    oc = np.zeros(n, np.float32)
    knn = np.zeros((n, k), np.int32) if return_knn else None
    r = lib().e3d_normals_knn(_ptr(xyz, np.float32, keep), n, int(k), C.c_void_p(vp.ctypes.data),
                              C.c_void_p(on.ctypes.data), C.c_void_p(oc.ctypes.data),
                              C.c_void_p(knn.ctypes.data) if knn is not None else None)
    if r < 0:
        _err("e3d_normals_knn", r)
    return (on, oc, knn) if return_knn else (on, oc)


def normals_radius(xyz, radius, viewpoint=(0.0, 0.0, 0.0), return_counts=False):
    """NormalEstimationTwoPassOMP with setRadiusSearch(radius): (normals[n,3], curvature[n][, neighbour counts[n]])."""
    keep = []
    n = int(xyz.shape[0])
    vp = np.ascontiguousarray(viewpoint, np.float32)
    on = np.zeros((n, 3), np.float32)
    oc = np.zeros(n, np.float32)
    cnt = np.zeros(n, np.int32) if return_counts else None
    r = lib().e3d_normals_radius(_ptr(xyz, np.float32, keep), n, float(radius), C.c_void_p(vp.ctypes.data), C.c_void_p(on.ctypes.data),
                                 C.c_void_p(oc.ctypes.data), C.c_void_p(cnt.ctypes.data) if cnt is not None else None)
    if r < 0:
        _err("e3d_normals_radius", r)
    return (on, oc, cnt) if return_counts else (on, oc)


def local_outlier_removal(xyz, mean_k, distance_factor_threshold, negative=False, return_distances=False):
    """pcl::LocalStatisticalOutlierRemoval: bool mask of the points the filter keeps [, first-pass mean neighbour distances].
    1 <= mean_k <= 1023; the neighbour lists take n x (mean_k + 1) x 4 bytes of device memory."""
    keep = []
    n = int(xyz.shape[0])
    inl = np.zeros(n, np.uint8)
    md = np.zeros(n, np.float32) if return_distances else None
    r = lib().e3d_local_outlier_removal(_ptr(xyz, np.float32, keep), n, int(mean_k), float(distance_factor_threshold), int(bool(negative)),
                                        C.c_void_p(inl.ctypes.data), C.c_void_p(md.ctypes.data) if md is not None else None)
    if r < 0:
        _err("e3d_local_outlier_removal", r)
    return (inl.astype(bool), md) if return_distances else inl.astype(bool)


def _mesh_arrays(vertices, triangles, keep):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3) if not _is_torch(vertices) else vertices
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    keep.append(t)
    return _ptr(v, np.float32, keep), int(v.shape[0]), C.c_void_p(t.ctypes.data), int(t.shape[0])


def mesh_squared_distance(points, vertices, triangles, max_sq_distance=float("inf")):
    """igl::AABB::squared_distance over a triangle mesh -> (squared distance[n] (+inf above max_sq_distance), closest triangle[n])."""
    keep = []
    n = int(points.shape[0])
    vp, nv, tp, nt = _mesh_arrays(vertices, triangles, keep)
    d = np.zeros(n, np.float32)
    ids = np.zeros(n, np.int32)
    r = lib().e3d_mesh_squared_distance(_ptr(points, np.float32, keep), n, vp, nv, tp, nt, float(max_sq_distance),
                                        C.c_void_p(d.ctypes.data), C.c_void_p(ids.ctypes.data))
    if r < 0:
        _err("e3d_mesh_squared_distance", r)
    return d, ids


def create_splats(xyz, normals, vertices, triangles, distance_threshold=0.02, max_splat_size=float("inf"), timings=None):
    """SplatCreator -> (vertices[4m,3], faces[2m,3], add_splat[n] bool, radius[n]).  timings: a dict that receives the index
    build and splat pass times (ms)."""
    keep = []
    n = int(xyz.shape[0])
    vp, nv, tp, nt = _mesh_arrays(vertices, triangles, keep)
    out = np.empty((max(n, 1), 12), np.float32)           # room for a splat per point (pages are only touched where written)
    flag = np.zeros(n, np.uint8)
    rad = np.zeros(n, np.float32)
    tm = np.zeros(2, np.float32)
    m = lib().e3d_create_splats(_ptr(xyz, np.float32, keep), _ptr(normals, np.float32, keep), n, vp, nv, tp, nt, float(distance_threshold),
                                float(max_splat_size), C.c_void_p(out.ctypes.data), n, C.c_void_p(flag.ctypes.data), C.c_void_p(rad.ctypes.data),
                                C.c_void_p(tm.ctypes.data))
    if m < 0:
        _err("e3d_create_splats", m)
    if timings is not None:
        timings["index_ms"] = float(tm[0]); timings["splat_ms"] = float(tm[1])
    s = np.arange(m, dtype=np.int32)[:, None] * 4
    faces = np.concatenate([np.concatenate([s + 2, s + 1, s], 1), np.concatenate([s, s + 3, s + 2], 1)], 1).reshape(-1, 3)
    return out[:m].reshape(-1, 3).copy(), faces, flag.astype(bool), rad


class SurfaceSolid(C.Structure):
    """e3d_surface_solid_t"""
    _fields_ = [("kind", C.c_int32), ("centre", C.c_double * 3), ("rotation", C.c_double * 9), ("half_extent", C.c_double * 3)]


SURFACE_SOLID_KINDS = {"union": 0, "subtract": 1}      # E3D_SURFACE_UNION, E3D_SURFACE_SUBTRACT


def _surface_solids(solids):
    ops = (SurfaceSolid * max(len(solids), 1))()
    for op, (kind, centre, rotation, half_extent) in zip(ops, solids):
        if isinstance(kind, str):
            if kind not in SURFACE_SOLID_KINDS:
                raise E3DError("reconstruct_surface: the kind of a solid is 'union' or 'subtract', not %r" % (kind,))
            kind = SURFACE_SOLID_KINDS[kind]
        op.kind = int(kind)                                  # a number goes to the library as it is
        op.centre[:] = np.asarray(centre, np.float64).reshape(3).tolist()
        op.rotation[:] = np.asarray(rotation, np.float64).reshape(9).tolist()
        op.half_extent[:] = np.asarray(half_extent, np.float64).reshape(3).tolist()
    return ops


def reconstruct_surface(xyz, normals, voxel_size, support_radius=None, return_corners=False, timings=None, solids=None, fill_iterations=0):
    """SurfaceReconstructor (include/e3d_hip.h, e3d_surface_reconstruct) -> (vertices[v, 3] f32, triangles[t, 3] uint32), and with
    return_corners a dict of the defined corners in ascending (k, j, i): ijk[c, 3] int32, f[c], weight[c] f64, count[c] int32, plus
    the vertices' cells cell_ijk[v, 3] int32.  support_radius defaults to 2 x voxel_size (in f32).  timings: a dict that receives the
    HIP-event time of every kernel group as <group>_ms.  solids: a list of (kind, centre[3], rotation[3, 3], half_extent[3]) with kind
    "union" or "subtract", applied in order to the scan field (e3d_surface_reconstruct_csg); None calls e3d_surface_reconstruct.
    fill_iterations = N > 0: N iterations of hole filling before the solids (e3d_surface_reconstruct_filled); the dict of
    return_corners then also holds corner_filled[c] and vertex_filled[v] (bool)."""
    keep = []
    n = int(xyz.shape[0])
    h = np.float32(voxel_size)
    r = np.float32(2) * h if support_radius is None else np.float32(support_radius)
    px, pn = (_ptr(xyz, np.float32, keep), _ptr(normals, np.float32, keep)) if n else (None, None)
    fill_iterations = int(fill_iterations)
    if fill_iterations != 0:
        solids = list(solids or ())
        ops = _surface_solids(solids)
        handle = lib().e3d_surface_reconstruct_filled(px, pn, n, float(h), float(r), fill_iterations, C.cast(ops, C.c_void_p), len(solids))
    elif solids is None:
        handle = lib().e3d_surface_reconstruct(px, pn, n, float(h), float(r))
    else:
        solids = list(solids)
        ops = _surface_solids(solids)
        handle = lib().e3d_surface_reconstruct_csg(px, pn, n, float(h), float(r), C.cast(ops, C.c_void_p), len(solids))
    if not handle:
        _err("e3d_surface_reconstruct")
    try:
        nc, nv, nt = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        lib().e3d_surface_counts(handle, C.byref(nc), C.byref(nv), C.byref(nt))
        vertices = np.zeros((nv.value, 3), np.float32)
        cells = np.zeros((nv.value, 3), np.int32)
        triangles = np.zeros((nt.value, 3), np.uint32)
        if lib().e3d_surface_get_mesh(handle, C.c_void_p(vertices.ctypes.data), C.c_void_p(cells.ctypes.data), C.c_void_p(triangles.ctypes.data)) < 0:
            _err("e3d_surface_get_mesh")
        corners = None
        if return_corners:
            corners = {"ijk": np.zeros((nc.value, 3), np.int32), "f": np.zeros(nc.value, np.float64), "weight": np.zeros(nc.value, np.float64),
                       "count": np.zeros(nc.value, np.int32), "cell_ijk": cells}
            if lib().e3d_surface_get_corners(handle, *(C.c_void_p(corners[k].ctypes.data) for k in ("ijk", "f", "weight", "count"))) < 0:
                _err("e3d_surface_get_corners")
            if fill_iterations != 0:
                corners["corner_filled"] = np.zeros(nc.value, np.uint8)
                corners["vertex_filled"] = np.zeros(nv.value, np.uint8)
                if lib().e3d_surface_get_fill(handle, C.c_void_p(corners["corner_filled"].ctypes.data), C.c_void_p(corners["vertex_filled"].ctypes.data)) < 0:
                    _err("e3d_surface_get_fill")
                corners["corner_filled"] = corners["corner_filled"].astype(bool)
                corners["vertex_filled"] = corners["vertex_filled"].astype(bool)
        if timings is not None:
            ms = (C.c_float * 16)()
            names = (C.c_char_p * 16)()
            g = lib().e3d_surface_kernel_ms(handle, ms, names, 16)
            for i in range(min(g, 16)):
                timings[names[i].decode() + "_ms"] = float(ms[i])
    finally:
        lib().e3d_surface_destroy(handle)
    return (vertices, triangles, corners) if return_corners else (vertices, triangles)


def evaluate_reconstruction(rec, scans, origins, tolerances=(0.01, 0.02, 0.05, 0.1, 0.2, 0.5), voxel_size=0.01, cube_map_size=2048,
                            return_classes=False, return_voxels=False, timings=None):
    """ReconstructionEvaluator (include/e3d_hip.h, e3d_evaluate_reconstruction).  rec[n, 3] f32 (numpy or torch, host or device); scans:
    a sequence of [n_s, 3] f32 arrays in the global frame; origins[S, 3] f32: the scanner positions.  Returns a dict: tolerances[T] f32,
    completeness[T], accuracy[T], f1[T] f64, n_scan_voxels, n_rec_voxels, evaluated_voxels[T] int64; with return_classes near_rec[n],
    free[n], near_scan[sum n_s] uint8 (255 = ignored point); with return_voxels scan_voxels and rec_voxels: dicts of ijk[v, 3],
    n_points[v], count_a[v, T] (# complete / # accurate), count_b[v, T] (# inaccurate) int32 in ascending (k, j, i).  timings: a dict
    that receives the HIP-event time of every kernel group as <group>_ms."""
    keep = []
    scans = [s.detach().cpu().numpy() if _is_torch(s) else s for s in scans]
    parts = [np.ascontiguousarray(s, np.float32).reshape(-1, 3) for s in scans]
    scan_xyz = np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)
    offsets = np.zeros(len(parts) + 1, np.int64)
    offsets[1:] = np.cumsum([len(p) for p in parts])
    origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    if len(origins) != len(parts):
        raise E3DError("evaluate_reconstruction: %d scans but %d origins" % (len(parts), len(origins)))
    tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
    T = len(tol)
    n = int(rec.shape[0])
    handle = lib().e3d_evaluate_reconstruction(_ptr(rec, np.float32, keep) if n else None, n, C.c_void_p(scan_xyz.ctypes.data) if len(scan_xyz) else None,
                                               C.c_void_p(offsets.ctypes.data), C.c_void_p(origins.ctypes.data), len(parts), C.c_void_p(tol.ctypes.data), T,
                                               float(np.float32(voxel_size)), int(cube_map_size))
    if not handle:
        _err("e3d_evaluate_reconstruction")
    try:
        nsv, nrv = C.c_int64(0), C.c_int64(0)
        evaluated = np.zeros(T, np.int64)
        scores = np.zeros((3, T), np.float64)
        if lib().e3d_eval_counts(handle, C.byref(nsv), C.byref(nrv), C.c_void_p(evaluated.ctypes.data)) < 0:
            _err("e3d_eval_counts")
        if lib().e3d_eval_get_scores(handle, C.c_void_p(scores.ctypes.data)) < 0:
            _err("e3d_eval_get_scores")
        out = {"tolerances": tol, "completeness": scores[0], "accuracy": scores[1], "f1": scores[2], "n_scan_voxels": nsv.value,
               "n_rec_voxels": nrv.value, "evaluated_voxels": evaluated}
        if return_classes:
            out["near_rec"] = np.zeros(n, np.uint8); out["free"] = np.zeros(n, np.uint8); out["near_scan"] = np.zeros(len(scan_xyz), np.uint8)
            if lib().e3d_eval_get_classes(handle, *(C.c_void_p(out[k].ctypes.data) for k in ("near_rec", "free", "near_scan"))) < 0:
                _err("e3d_eval_get_classes")
        if return_voxels:
            for kind, name, nv in ((0, "scan_voxels", nsv.value), (1, "rec_voxels", nrv.value)):
                v = {"ijk": np.zeros((nv, 3), np.int32), "n_points": np.zeros(nv, np.int32), "count_a": np.zeros((nv, T), np.int32),
                     "count_b": np.zeros((nv, T), np.int32)}
                if lib().e3d_eval_get_voxels(handle, kind, *(C.c_void_p(v[k].ctypes.data) for k in ("ijk", "n_points", "count_a", "count_b"))) < 0:
                    _err("e3d_eval_get_voxels")
                out[name] = v
        if timings is not None:
            ms = (C.c_float * 16)()
            names = (C.c_char_p * 16)()
            g = lib().e3d_eval_kernel_ms(handle, ms, names, 16)
            for i in range(min(g, 16)):
                timings[names[i].decode() + "_ms"] = float(ms[i])
    finally:
        lib().e3d_eval_destroy(handle)
    return out


def disparity_scores(counts, sums):
    """Rule 7 of e3d_evaluate_disparity from counts[..., 2 + T] and sums[..., 2] alone: a dict of f64 arrays coverage, avgerr, rms [...]
    and bad, bad_or_missing [..., T]; each is 0 where its denominator is 0."""
    counts = np.asarray(counts, np.int64)
    sums = np.asarray(sums, np.float64)
    n_region, n_valid, n_bad = counts[..., 0], counts[..., 1], counts[..., 2:]

    def ratio(a, b):
        a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
        out = np.zeros(a.shape, np.float64)
        np.divide(a, b, out=out, where=b != 0)
        return out

    return {"coverage": ratio(n_valid, n_region), "bad": ratio(n_bad, n_valid[..., None]),
            "bad_or_missing": ratio(n_bad + (n_region - n_valid)[..., None], n_region[..., None]),
            "avgerr": ratio(sums[..., 0], n_valid), "rms": np.sqrt(ratio(sums[..., 1], n_valid))}


def evaluate_disparity(gt, mask, estimates, thresholds=(0.5, 1, 2, 4), percentiles=(50, 90, 95, 99), error_maps=False, timings=None):
    """StereoEvaluator (include/e3d_hip.h, e3d_evaluate_disparity).  gt[H, W] f32 (+inf = unknown), mask[H, W] uint8 or None, estimates
    [H, W] or [n_est, H, W] f32, each numpy or torch, host or device (a sequence of [H, W] arrays is stacked on the host).  Returns a
    dict: thresholds[T] f32, percentiles[P] int32, counts[n_est, 2, 2 + T] int64 (per region all / nocc: n_region, n_valid, n_bad[T]),
    sums[n_est, 2, 2] f64 (sum1, sum2), quantiles[n_est, 2, P] f32, the derived scores of rule 7 (coverage, avgerr, rms [n_est, 2];
    bad, bad_or_missing [n_est, 2, T]) and with error_maps the colour-coded maps [n_est, H, W, 3] uint8.  timings: a dict that receives
    the HIP-event time of every kernel group as <group>_ms."""
    keep = []
    if isinstance(estimates, (list, tuple)):
        estimates = np.stack([np.asarray(e.detach().cpu().numpy() if _is_torch(e) else e, np.float32) for e in estimates]) if len(estimates) else np.zeros((0,) + tuple(gt.shape), np.float32)
    if len(gt.shape) != 2:
        raise E3DError("evaluate_disparity: gt must be [H, W]")
    H, W = int(gt.shape[0]), int(gt.shape[1])
    shape = tuple(int(v) for v in estimates.shape)
    if shape == (H, W):
        n_est = 1
    elif len(shape) == 3 and shape[1:] == (H, W):
        n_est = shape[0]
    else:
        raise E3DError("evaluate_disparity: estimates of shape %s against a ground truth of %d x %d" % (shape, H, W))
    if mask is not None and tuple(int(v) for v in mask.shape) != (H, W):
        raise E3DError("evaluate_disparity: mask of shape %s against a ground truth of %d x %d" % (tuple(mask.shape), H, W))
    thr = np.ascontiguousarray(thresholds, np.float32).reshape(-1)
    pct = np.ascontiguousarray(percentiles, np.int32).reshape(-1)
    T, P = len(thr), len(pct)
    maps = np.zeros((n_est, H, W, 3), np.uint8) if error_maps else None
    handle = lib().e3d_evaluate_disparity(_ptr(gt, np.float32, keep), _ptr(mask, np.uint8, keep), W, H, _ptr(estimates, np.float32, keep) if n_est else None, n_est,
                                          C.c_void_p(thr.ctypes.data) if T else None, T, C.c_void_p(pct.ctypes.data) if P else None, P,
                                          C.c_void_p(maps.ctypes.data) if error_maps and maps.size else None)
    if not handle:
        _err("e3d_evaluate_disparity")
    try:
        counts = np.zeros((n_est, 2, 2 + T), np.int64)
        sums = np.zeros((n_est, 2, 2), np.float64)
        quantiles = np.zeros((n_est, 2, P), np.float32)
        if lib().e3d_disp_eval_get_counts(handle, C.c_void_p(counts.ctypes.data)) < 0:
            _err("e3d_disp_eval_get_counts")
        if lib().e3d_disp_eval_get_sums(handle, C.c_void_p(sums.ctypes.data)) < 0:
            _err("e3d_disp_eval_get_sums")
        if lib().e3d_disp_eval_get_quantiles(handle, C.c_void_p(quantiles.ctypes.data) if P else None) < 0:
            _err("e3d_disp_eval_get_quantiles")
        out = {"thresholds": thr, "percentiles": pct, "counts": counts, "sums": sums, "quantiles": quantiles}
        out.update(disparity_scores(counts, sums))
        if error_maps:
            out["error_maps"] = maps
        if timings is not None:
            ms = (C.c_float * 16)()
            names = (C.c_char_p * 16)()
            g = lib().e3d_disp_eval_kernel_ms(handle, ms, names, 16)
            for i in range(min(g, 16)):
                timings[names[i].decode() + "_ms"] = float(ms[i])
    finally:
        lib().e3d_disp_eval_destroy(handle)
    return out


CUBE_MAP_FACES = ("front", "left", "back", "right", "down", "up")


def render_cube_map(xyz, rgb, size, fill=True, timings=None):
    """CubeMapRenderer -> (color[6, size, size, 3] uint8 (R, G, B), depth[6, size, size] float32 (+inf: none), sweeps[6]).
    Faces in the order of CUBE_MAP_FACES.  fill=False: the raw z-buffer.  timings: a dict that receives the phase times (ms)."""
    keep = []
    n = int(xyz.shape[0])
    size = int(size)
    color = np.zeros((6, max(size, 0), max(size, 0), 3), np.uint8)
    depth = np.zeros((6, max(size, 0), max(size, 0)), np.float32)
    sweeps = np.zeros(6, np.int32)
    r = lib().e3d_render_cube_map(_ptr(xyz, np.float32, keep) if n else None, _ptr(rgb, np.uint8, keep) if n else None, n, size,
                                  1 if fill else 0, C.c_void_p(color.ctypes.data), C.c_void_p(depth.ctypes.data), C.c_void_p(sweeps.ctypes.data))
    if r < 0:
        _err("e3d_render_cube_map", r)
    if timings is not None:
        tm = np.zeros(8, np.float32)
        lib().e3d_cube_map_timings(C.c_void_p(tm.ctypes.data))
        timings.update(points_ms=float(tm[0]), resolve_ms=float(tm[1]), fill_ms=float(tm[2]), dilation_ms=float(tm[3]),
                       batches=int(tm[4]), sweeps_launched=int(tm[5]))
    return color, depth, sweeps


# ---- PointCloudEditor --------------------------------------------------------------------------------------------------
class EditView(C.Structure):
    """e3d_view -- the editor's view: pinhole camera, camera_T_object (row-major 3 x 4, rotation * scale | translation), depth range."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("camera_T_object", C.c_float * 12), ("min_depth", C.c_float), ("max_depth", C.c_float)]


def edit_view(width, height, camera_T_object=None, min_depth=0.1, max_depth=100.0, fx=None, fy=None, cx=None, cy=None):
    """An EditView; the intrinsics default to RenderWidget::SetFreeOrbitViewport's (fx = fy = height, principal point at the centre)."""
    T = np.eye(4, dtype=np.float32)[:3] if camera_T_object is None else _pose12(camera_T_object)
    return EditView(int(width), int(height), float(height if fx is None else fx), float(height if fy is None else fy),
                    float(np.float32(0.5 * width - 0.5) if cx is None else cx), float(np.float32(0.5 * height - 0.5) if cy is None else cy),
                    (C.c_float * 12)(*[float(v) for v in T.ravel()]), float(min_depth), float(max_depth))


class PointCloudEdit:
    """One object's points and their selection on the device (include/e3d_hip.h: e3d_edit_*) -- the PointCloudEditor's lasso,
    beyond-plane selection, picking, delete and move.  Colours, labels and faces stay with the caller."""
    REPLACE, ADD, REMOVE = 0, 1, 2
    _MODES = {"replace": 0, "add": 1, "remove": 2}

    def __init__(self, xyz):
        keep = []
        n = int(xyz.shape[0])
        self._h = lib().e3d_edit_create(_ptr(xyz, np.float32, keep) if n else None, n)
        if not self._h:
            _err("e3d_edit_create")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().e3d_edit_destroy(h)
            self._h = None

    def _chk(self, r, what):
        if r < 0:
            _err(what, r)
        return int(r)

    def __len__(self):
        return self._chk(lib().e3d_edit_size(self._h), "e3d_edit_size")

    def points(self):
        out = np.zeros((len(self), 3), np.float32)
        self._chk(lib().e3d_edit_get_points(self._h, C.c_void_p(out.ctypes.data)), "e3d_edit_get_points")
        return out

    def selection(self):
        """bool flag per point."""
        out = np.zeros(len(self), np.uint8)
        self._chk(lib().e3d_edit_get_selection(self._h, C.c_void_p(out.ctypes.data)), "e3d_edit_get_selection")
        return out.astype(bool)

    def set_selection(self, flags):
        keep = []
        flags = np.ascontiguousarray(flags).astype(np.uint8) if not _is_torch(flags) else flags
        if int(flags.shape[0]) != len(self):
            raise E3DError("set_selection: %d flags for %d points" % (int(flags.shape[0]), len(self)))
        return self._chk(lib().e3d_edit_set_selection(self._h, _ptr(flags, np.uint8, keep)), "e3d_edit_set_selection")

    def selection_count(self):
        return self._chk(lib().e3d_edit_selection_count(self._h), "e3d_edit_selection_count")

    def lasso(self, view, polygon, mode="replace", depth=None):
        """polygon: (m, 2) pixel positions, not closed.  depth: (height, width) f32 rendering of the object, for meshes.
        Returns the number of selected points."""
        keep = []
        poly = np.ascontiguousarray(polygon, np.float64).reshape(-1, 2)
        if depth is not None and tuple(depth.shape) != (view.height, view.width):
            raise E3DError("lasso: depth image %s for a %d x %d view" % (tuple(depth.shape), view.width, view.height))
        return self._chk(lib().e3d_edit_lasso(self._h, C.byref(view), C.c_void_p(poly.ctypes.data), poly.shape[0], self._MODES.get(mode, mode),
                                              _ptr(depth, np.float32, keep)), "e3d_edit_lasso")

    def beyond_plane(self, view, points, camera_position_object, limit_to_visible=False):
        """points: (3, 3), the plane; the side of camera_position_object stays unselected.  Returns the number of selected points."""
        p = np.ascontiguousarray(points, np.float32).reshape(3, 3)
        c = np.ascontiguousarray(camera_position_object, np.float32).reshape(3)
        return self._chk(lib().e3d_edit_beyond_plane(self._h, C.byref(view), C.c_void_p(p.ctypes.data), C.c_void_p(c.ctypes.data),
                                                     int(bool(limit_to_visible))), "e3d_edit_beyond_plane")

    def pick(self, view, clicks):
        """clicks: (m <= 8, 2) pixel positions -> (index[m] int64, -1 where no point is in range; squared pixel distance[m] f32)."""
        ck = np.ascontiguousarray(clicks, np.float64).reshape(-1, 2)
        idx = np.full(ck.shape[0], -1, np.int64)
        d = np.full(ck.shape[0], np.inf, np.float32)
        self._chk(lib().e3d_edit_pick(self._h, C.byref(view), C.c_void_p(ck.ctypes.data), ck.shape[0], C.c_void_p(idx.ctypes.data),
                                      C.c_void_p(d.ctypes.data)), "e3d_edit_pick")
        return idx, d

    def delete_selected(self):
        """Removes the selected points (the others keep their order) and clears the selection; returns the new point count."""
        return self._chk(lib().e3d_edit_delete_selected(self._h), "e3d_edit_delete_selected")

    def extract_selected(self):
        """Coordinates of the selected points, in index order."""
        m = self.selection_count()
        out = np.zeros((m, 3), np.float32)
        self._chk(lib().e3d_edit_extract_selected(self._h, C.c_void_p(out.ctypes.data), m), "e3d_edit_extract_selected")
        return out

    def kernel_ms(self):
        ms = C.c_float(0)
        self._chk(lib().e3d_edit_kernel_ms(self._h, C.byref(ms)), "e3d_edit_kernel_ms")
        return ms.value


# ---- (B) image registration kernels ------------------------------------------------------------------------------------
CAMERA_PINHOLE, CAMERA_OPENCV, CAMERA_THIN_PRISM_FISHEYE, CAMERA_OPENCV_FISHEYE, CAMERA_FOV = 0, 1, 2, 3, 4
DEPTH_HOLES_AVERAGE, DEPTH_HOLES_STRICT = 0, 1      # e3d_reg_set_depth_map_level0


def determine_point_neighbors(xyz, neighbor_count, candidate_count, scan_indices=None, scan_count=1):
    """Problem::DeterminePointNeighbors -> (n, neighbor_count) uint32."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    out = np.zeros((xyz.shape[0], neighbor_count), np.uint32)
    si = np.ascontiguousarray(scan_indices, np.uint8) if scan_indices is not None else None
    r = lib().e3d_determine_point_neighbors(C.c_void_p(xyz.ctypes.data), xyz.shape[0], C.c_void_p(si.ctypes.data) if si is not None else None,
                                            scan_count, 1 if si is not None else 0, neighbor_count, candidate_count, C.c_void_p(out.ctypes.data))
    if r < 0:
        _err("e3d_determine_point_neighbors", r)
    return out


def merge_close_points(merge_distance, num_scans, xyz, colors, scan_indices, max_radius):
    """MergeClosePoints -> (xyz, colours, scan indices, max_radius) of the merged points, in centre order."""
    xyz = np.ascontiguousarray(xyz, np.float32); colors = np.ascontiguousarray(colors, np.float32)
    scan_indices = np.ascontiguousarray(scan_indices, np.uint8); max_radius = np.ascontiguousarray(max_radius, np.float32)
    n = xyz.shape[0]
    ox = np.zeros((max(n, 1), 3), np.float32); oc = np.zeros(max(n, 1), np.float32); osc = np.zeros(max(n, 1), np.uint8); om = np.zeros(max(n, 1), np.float32)
    m = lib().e3d_merge_close_points(float(merge_distance), int(num_scans), *[C.c_void_p(a.ctypes.data) for a in (xyz, colors, scan_indices, max_radius)], n,
                                     *[C.c_void_p(a.ctypes.data) for a in (ox, oc, osc, om)])
    if m < 0:
        _err("e3d_merge_close_points", m)
    return ox[:m].copy(), oc[:m].copy(), osc[:m].copy(), om[:m].copy()


def pose_from_bearings(points, bearings, q, t):
    """Host only (no device needed): the pose image_T_global that minimises sum |f_i - (R p_i + t) / |R p_i + t||^2 over >= 6 pairs of
    global points ((n, 3) float64) and unit bearings ((n, 3) float64), by Levenberg-Marquardt from (q, t) -> (q (4,) float32 unit, w >= 0;
    t (3,) float32; stats = (RMS angle before, after, iterations, converged))."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3); f = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    if len(p) != len(f):
        raise E3DError("pose_from_bearings: %d points, %d bearings" % (len(p), len(f)))
    q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
    assert q.shape == (4,) and t.shape == (3,)
    qo = np.zeros(4, np.float32); to = np.zeros(3, np.float32); stats = np.zeros(4, np.float64)
    r = lib().e3d_pose_from_bearings(C.c_void_p(p.ctypes.data), C.c_void_p(f.ctypes.data), len(p), C.c_void_p(q.ctypes.data), C.c_void_p(t.ctypes.data),
                                     C.c_void_p(qo.ctypes.data), C.c_void_p(to.ctypes.data), C.c_void_p(stats.ctypes.data))
    if r < 0:
        _err("e3d_pose_from_bearings", r)
    return qo, to, (float(stats[0]), float(stats[1]), int(stats[2]), bool(stats[3]))


class RegParams(C.Structure):
    """e3d_reg_params -- the opt::Parameters fields the device code reads (src/opt/parameters.h:40-68)."""
    _fields_ = [("point_neighbor_count", C.c_int32), ("robust_weighting_type", C.c_int32),
                ("robust_weighting_parameter", C.c_float), ("fixed_residuals_weight", C.c_float),
                ("variable_residuals_weight", C.c_float), ("maximum_valid_intensity", C.c_float),
                ("occlusion_depth_threshold", C.c_float), ("splat_radius", C.c_float),
                ("current_image_scale", C.c_int32), ("image_scale_count", C.c_int32),
                ("depth_residuals_weight", C.c_float), ("depth_robust_weighting_type", C.c_int32),
                ("depth_robust_weighting_parameter", C.c_float)]


def default_reg_params(**kw):
    p = RegParams(5, 1, float(np.float32(30 * np.sqrt(5) / np.sqrt(2))), 1.0, 1.0, 252.0, 0.01, 0.03, 0, 2, 0.0, 2, 0.02)     # parameters.h:40-68
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class RegProblem:
    """Device-resident mirror of the parts of opt::Problem the ImageRegistrator hot loops read, plus the kernel-level
    operators (render depth / observe / accumulate / cost / colour update).  One method per C-ABI entry point."""

    def __init__(self, params=None):
        self.params = params if params is not None else default_reg_params()
        self._h = lib().e3d_reg_create(C.byref(self.params))
        if not self._h:
            _err("e3d_reg_create")
        self._levels = {}
        self._nparams = {}
        self._dependent = set()
        self._image_intr = {}
        self._intr_size = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().e3d_reg_destroy(h)
            self._h = None

    def _chk(self, r, what):
        if r < 0:
            _err(what, r)
        return r

    def set_params(self, params):
        self.params = params
        self._chk(lib().e3d_reg_set_params(self._h, C.byref(params)), "e3d_reg_set_params")

    def set_point_scale(self, scale, xyz, radius, neighbor_indices, fixed_descriptors=None):
        keep = []
        xyz = np.ascontiguousarray(xyz, np.float32)
        nbr = np.ascontiguousarray(neighbor_indices, np.uint32)
        fd = np.ascontiguousarray(fixed_descriptors, np.float32) if fixed_descriptors is not None else None
        self._chk(lib().e3d_reg_set_point_scale(self._h, scale, C.c_void_p(xyz.ctypes.data), xyz.shape[0], float(radius),
                                                C.c_void_p(nbr.ctypes.data), C.c_void_p(fd.ctypes.data) if fd is not None else None),
                  "e3d_reg_set_point_scale")

    def set_variable_descriptors(self, scale, descriptors, counts):
        d = np.ascontiguousarray(descriptors, np.float32); c = np.ascontiguousarray(counts, np.int32)
        self._chk(lib().e3d_reg_set_variable_descriptors(self._h, scale, C.c_void_p(d.ctypes.data), C.c_void_p(c.ctypes.data)), "set_variable_descriptors")

    def get_variable_descriptors(self, scale, n):
        d = np.zeros((n, self.params.point_neighbor_count), np.float32); c = np.zeros(n, np.int32)
        self._chk(lib().e3d_reg_get_variable_descriptors(self._h, scale, C.c_void_p(d.ctypes.data), C.c_void_p(c.ctypes.data)), "get_variable_descriptors")
        return d, c

    def set_intrinsics(self, intrinsics_id, width, height, parameters, min_image_scale, n_levels, camera_type=0):
        p = np.ascontiguousarray(parameters, np.float32)
        self._chk(lib().e3d_reg_set_intrinsics(self._h, intrinsics_id, camera_type, width, height, C.c_void_p(p.ctypes.data), len(p),
                                               min_image_scale, n_levels), "e3d_reg_set_intrinsics")
        self._levels[intrinsics_id] = n_levels
        self._nparams[intrinsics_id] = len(p)
        self._intr_size[intrinsics_id] = (int(height), int(width))

    def intrinsics_level(self, intrinsics_id, level):
        w = C.c_int(); h = C.c_int(); p = np.zeros(self._nparams[intrinsics_id], np.float32); c = C.c_float()
        self._chk(lib().e3d_reg_get_intrinsics_level(self._h, intrinsics_id, level, C.byref(w), C.byref(h), C.c_void_p(p.ctypes.data), C.byref(c)), "get_intrinsics_level")
        return w.value, h.value, p, c.value

    def set_camera_mask(self, intrinsics_id, masks):
        """Intrinsics::camera_mask: one u8 mask per pyramid level (or None per level); masks=None removes it."""
        if masks is None:
            self._chk(lib().e3d_reg_set_camera_mask(self._h, intrinsics_id, None), "e3d_reg_set_camera_mask")
            return
        keep = [np.ascontiguousarray(m, np.uint8) if m is not None else None for m in masks]
        arr = (C.c_void_p * len(keep))(*[(m.ctypes.data if m is not None else None) for m in keep])
        self._chk(lib().e3d_reg_set_camera_mask(self._h, intrinsics_id, arr), "e3d_reg_set_camera_mask")

    def set_depth_maps(self, image_id, levels):
        """Problem::SetFixedDepthMaps for one image: one f32 map per pyramid level (None removes them)."""
        if levels is None:
            self._chk(lib().e3d_reg_set_depth_maps(self._h, image_id, None), "e3d_reg_set_depth_maps")
            return
        keep = [np.ascontiguousarray(l, np.float32) for l in levels]
        arr = (C.c_void_p * len(keep))(*[l.ctypes.data for l in keep])
        self._chk(lib().e3d_reg_set_depth_maps(self._h, image_id, arr), "e3d_reg_set_depth_maps")

    def set_depth_map_level0(self, image_id, depth, hole_mode=DEPTH_HOLES_STRICT):
        """One full-resolution (height, width) f32 depth map; the library sanitises it (invalid pixels -> 0) and builds every further
        level of the camera pyramid on the device.  hole_mode: DEPTH_HOLES_AVERAGE (plain 2x2 box mean) or DEPTH_HOLES_STRICT (a 2x2
        block with an invalid pixel gives an invalid pixel)."""
        intr = self._image_intr.get(image_id)
        d = np.ascontiguousarray(depth, np.float32)
        if intr is not None:
            w, h, _, _ = self.intrinsics_level(intr, 0)
            if d.shape != (h, w):
                raise E3DError("set_depth_map_level0: depth map %s for a %d x %d camera" % (tuple(d.shape), w, h))
        self._chk(lib().e3d_reg_set_depth_map_level0(self._h, image_id, C.c_void_p(d.ctypes.data), int(hole_mode)), "e3d_reg_set_depth_map_level0")

    def get_depth_map(self, image_id, level):
        """One level of an image's depth maps as the device holds it, (h, w) f32; an error without depth maps or beyond the pyramid."""
        intr = self._image_intr.get(image_id)
        w = h = 1                        # an unknown image or level: the library reports it before it writes
        if intr is not None and 0 <= level < self._levels[intr]:
            w, h, _, _ = self.intrinsics_level(intr, level)
        m = np.zeros((h, w), np.float32)
        self._chk(lib().e3d_reg_get_depth_map(self._h, image_id, level, C.c_void_p(m.ctypes.data)), "e3d_reg_get_depth_map")
        return m

    def get_depth_maps(self, image_id):
        """All levels: a list of (h, w) f32 arrays, one per pyramid level of the image's camera."""
        return [self.get_depth_map(image_id, l) for l in range(self._levels.get(self._image_intr.get(image_id), 1))]

    def set_rig_depth_residuals(self, enable=True):
        """Depth residuals of the non-reference images of a rig (an error by default, as the reference aborts on them); kept by set_params."""
        self._chk(lib().e3d_reg_set_rig_depth_residuals(self._h, int(bool(enable))), "e3d_reg_set_rig_depth_residuals")

    def depth_accumulate(self, image_id, point_scale):
        """(H, b, sum of robust residuals, count) of the depth residuals of one (image, point scale); V = I + 6, or I + 12 for a
        non-reference rig image (local_unknowns)."""
        V = self.local_unknowns(image_id)
        H = np.zeros((V, V), np.float64); b = np.zeros(V, np.float64)
        sm = C.c_double(0); cn = C.c_int64(0)
        self._chk(lib().e3d_reg_depth_accumulate(self._h, image_id, point_scale, C.c_void_p(H.ctypes.data), C.c_void_p(b.ctypes.data),
                                                 C.byref(sm), C.byref(cn)), "e3d_reg_depth_accumulate")
        return H, b, sm.value, cn.value

    def depth_cost(self, image_id, point_scale):
        sm = C.c_double(0); cn = C.c_int64(0)
        self._chk(lib().e3d_reg_depth_cost(self._h, image_id, point_scale, C.byref(sm), C.byref(cn)), "e3d_reg_depth_cost")
        return sm.value, cn.value

    def set_image(self, image_id, intrinsics_id, levels, masks=None):
        if levels is None:                       # an image without pixels (another rank's, or geometry only): id, intrinsics and pose
            self._chk(lib().e3d_reg_set_image(self._h, image_id, intrinsics_id, None, None), "e3d_reg_set_image")
            self._image_intr[image_id] = intrinsics_id
            return
        keep = [np.ascontiguousarray(l, np.uint8) for l in levels]
        arr = (C.c_void_p * len(keep))(*[l.ctypes.data for l in keep])
        marr = None
        if masks is not None:
            keepm = [np.ascontiguousarray(m, np.uint8) if m is not None else None for m in masks]
            marr = (C.c_void_p * len(keepm))(*[(m.ctypes.data if m is not None else None) for m in keepm])
        self._chk(lib().e3d_reg_set_image(self._h, image_id, intrinsics_id, arr, marr), "e3d_reg_set_image")
        self._image_intr[image_id] = intrinsics_id

    def set_image_pose(self, image_id, q, t):
        """image_T_global as unit quaternion (w, x, y, z) + translation."""
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        assert q.shape == (4,) and t.shape == (3,)
        self._chk(lib().e3d_reg_set_image_pose(self._h, image_id, C.c_void_p(q.ctypes.data), C.c_void_p(t.ctypes.data)), "e3d_reg_set_image_pose")

    def get_image_pose(self, image_id):
        q = np.zeros(4, np.float32); t = np.zeros(3, np.float32)
        self._chk(lib().e3d_reg_get_image_pose(self._h, image_id, C.c_void_p(q.ctypes.data), C.c_void_p(t.ctypes.data)), "e3d_reg_get_image_pose")
        return q, t

    def update_observations(self, border_size=1):
        self._chk(lib().e3d_reg_update_observations(self._h, border_size), "e3d_reg_update_observations")

    # ---- GroundTruthCreator (f4) -------------------------------------------------------------------------------------
    def set_scan_points(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32)
        self._n_scan = xyz.shape[0]
        self._chk(lib().e3d_reg_set_scan_points(self._h, C.c_void_p(xyz.ctypes.data), xyz.shape[0]), "e3d_reg_set_scan_points")

    def count_scan_observations(self, image_id, mask=None, excluded_flag=2):
        m = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        self._chk(lib().e3d_reg_count_scan_observations(self._h, image_id, C.c_void_p(m.ctypes.data) if m is not None else None, excluded_flag),
                  "e3d_reg_count_scan_observations")

    def scan_observation_counts(self):
        out = np.zeros(self._n_scan, np.int32)
        self._chk(lib().e3d_reg_get_scan_observation_counts(self._h, C.c_void_p(out.ctypes.data)), "e3d_reg_get_scan_observation_counts")
        return out

    def set_scan_observation_counts(self, counts):
        counts = np.ascontiguousarray(counts, np.int32)
        assert counts.shape[0] == self._n_scan
        self._chk(lib().e3d_reg_set_scan_observation_counts(self._h, C.c_void_p(counts.ctypes.data)), "e3d_reg_set_scan_observation_counts")

    # ---- debug point clouds (Problem::DebugWriteColoredPointCloud) ----------------------------------------------------
    def scan_colors_begin(self):
        """Zero the colour sums and observation counts of the scan points (set_scan_points)."""
        self._chk(lib().e3d_reg_scan_colors_begin(self._h), "e3d_reg_scan_colors_begin")

    def scan_colors_add_image(self, image_id, rgb):
        """rgb: (height, width, 3) uint8, R G B -- the image file as decoded, at its own size."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.ndim == 3 and rgb.shape[2] == 3
        self._chk(lib().e3d_reg_scan_colors_add_image(self._h, int(image_id), C.c_void_p(rgb.ctypes.data), rgb.shape[1], rgb.shape[0]),
                  "e3d_reg_scan_colors_add_image")

    def scan_colors_sums(self):
        """-> (sums (n, 3) float32 r g b, counts (n,) int32)."""
        sums = np.zeros((self._n_scan, 3), np.float32); counts = np.zeros(self._n_scan, np.int32)
        self._chk(lib().e3d_reg_scan_colors_get_sums(self._h, C.c_void_p(sums.ctypes.data), C.c_void_p(counts.ctypes.data)), "e3d_reg_scan_colors_get_sums")
        return sums, counts

    def scan_colors_set_sums(self, sums, counts):
        sums = np.ascontiguousarray(sums, np.float32); counts = np.ascontiguousarray(counts, np.int32)
        assert sums.shape == (self._n_scan, 3) and counts.shape == (self._n_scan,)
        self._chk(lib().e3d_reg_scan_colors_set_sums(self._h, C.c_void_p(sums.ctypes.data), C.c_void_p(counts.ctypes.data)), "e3d_reg_scan_colors_set_sums")

    def scan_colors_finish(self):
        """-> (n, 3) uint8: (uint8)(sum / count + 0.5f) per channel, 0 0 0 where count == 0."""
        rgb = np.zeros((self._n_scan, 3), np.uint8)
        self._chk(lib().e3d_reg_scan_colors_finish(self._h, C.c_void_p(rgb.ctypes.data)), "e3d_reg_scan_colors_finish")
        return rgb

    def ground_truth_depth(self, image_id, width, height, mask=None, excluded_flag=2, min_count=2):
        """-> (gt_depth, occlusion_depth), both (height, width) float32."""
        m = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        gt = np.zeros((height, width), np.float32); occ = np.zeros((height, width), np.float32)
        self._chk(lib().e3d_reg_ground_truth_depth(self._h, image_id, C.c_void_p(m.ctypes.data) if m is not None else None, excluded_flag,
                                                   min_count, C.c_void_p(gt.ctypes.data), C.c_void_p(occ.ctypes.data)), "e3d_reg_ground_truth_depth")
        return gt, occ

    def scan_rendering(self, image_id, width, height, point_radius, mask=None, excluded_flag=2, min_count=2):
        """-> (height, width) uint32: index + 1 of the last scan point whose square covers the pixel, 0 where none does."""
        win = np.zeros((height, width), np.uint32)
        m = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        self._chk(lib().e3d_reg_scan_rendering(self._h, image_id, C.c_void_p(m.ctypes.data) if m is not None else None, excluded_flag,
                                               min_count, point_radius, C.c_void_p(win.ctypes.data)), "e3d_reg_scan_rendering")
        return win

    # ---- MaskTransfer (DatasetInspector "Label transfer", gui_main_window.cc:868-1054) ----------------------------------------------
    def _level0_shape(self, image_id):
        if image_id not in self._image_intr:
            raise E3DError("image %d not set" % image_id)
        w, h, _, _ = self.intrinsics_level(self._image_intr[image_id], 0)
        return h, w

    def _mask_ptr(self, mask, shape, keep, what):
        if tuple(mask.shape) != tuple(shape):
            raise E3DError("%s has shape %s, the image's camera is %s (height, width)" % (what, tuple(mask.shape), tuple(shape)))
        return _ptr(mask, np.uint8, keep)

    def mask_transfer_source(self, image_id, mask, transfer_eval_obs=False):
        """Source half of the label transfer: mask is the (height, width) uint8 level-0 mask of image_id (0 / 1 / 2; numpy or a torch
        tensor, host or device).  Labels the scan points (set_scan_points) and returns how many carry a label."""
        image_id = int(image_id)
        keep = []
        p = self._mask_ptr(mask, self._level0_shape(image_id), keep, "mask")
        return int(self._chk(lib().e3d_reg_mask_transfer_source(self._h, image_id, p, int(bool(transfer_eval_obs))), "e3d_reg_mask_transfer_source"))

    def mask_transfer_target(self, image_id, existing=None, return_stats=False):
        """Target half (any number of times after one mask_transfer_source): -> the merged (height, width) uint8 mask of image_id, and
        with return_stats also (pixels set by the point pass, non-zero pixels after the fill-in, pixels that differ from `existing`)."""
        image_id = int(image_id)
        keep = []
        shape = self._level0_shape(image_id)
        e = self._mask_ptr(existing, shape, keep, "existing") if existing is not None else None
        out = np.zeros(shape, np.uint8)
        stats = np.zeros(3, np.int64)
        self._chk(lib().e3d_reg_mask_transfer_target(self._h, image_id, e, C.c_void_p(out.ctypes.data), C.c_void_p(stats.ctypes.data)),
                  "e3d_reg_mask_transfer_target")
        return (out, tuple(int(v) for v in stats)) if return_stats else out

    # ---- ImageLocalizer (DatasetInspector "Localize image", localize_image_tool.cc) ------------------------------------------------
    def pick_scan_points(self, image_id, clicks):
        """The scan point nearest to each of 1 .. 32 clicks ((k, 2) float32, (0, 0) = centre of the top-left pixel) among the points
        visible in image_id at its current pose -> (indices (k,) int64, -1 = none; pixels (k, 2) float32, the winners' unrounded
        positions; squared distances (k,) float32, +inf = none; number of visible points)."""
        clicks = np.ascontiguousarray(clicks, np.float32).reshape(-1, 2)
        k = len(clicks)
        index = np.zeros(k, np.int64); pixel = np.zeros((k, 2), np.float32); dist = np.zeros(k, np.float32)
        visible = self._chk(lib().e3d_reg_pick_scan_points(self._h, int(image_id), C.c_void_p(clicks.ctypes.data), k, C.c_void_p(index.ctypes.data),
                                                           C.c_void_p(pixel.ctypes.data), C.c_void_p(dist.ctypes.data)), "e3d_reg_pick_scan_points")
        return index, pixel, dist, int(visible)

    def image_bearings(self, image_id, pixels):
        """Unit bearing vectors ((k, 3) float64, camera frame) of pixel positions ((k, 2) float32) of image_id's level-0 model."""
        pixels = np.ascontiguousarray(pixels, np.float32).reshape(-1, 2)
        out = np.zeros((len(pixels), 3), np.float64)
        self._chk(lib().e3d_reg_image_bearings(self._h, int(image_id), C.c_void_p(pixels.ctypes.data), len(pixels), C.c_void_p(out.ctypes.data)),
                  "e3d_reg_image_bearings")
        return out

    def project_points(self, image_id, xyz):
        """Global points ((k, 3) float32) in image_id at its current pose -> (unrounded level-0 pixel positions (k, 2) float32, NaN behind
        the camera; states (k,) uint8: 0 = behind the camera or outside the image, 1 = visible, 2 = behind the occlusion depth)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        pixel = np.zeros((len(xyz), 2), np.float32); state = np.zeros(len(xyz), np.uint8)
        self._chk(lib().e3d_reg_project_points(self._h, int(image_id), C.c_void_p(xyz.ctypes.data), len(xyz), C.c_void_p(pixel.ctypes.data),
                                               C.c_void_p(state.ctypes.data)), "e3d_reg_project_points")
        return pixel, state

    # ---- ImageUndistorter ------------------------------------------------------------------------------------------------------------
    def undistort_plan(self, intrinsics_id, blank_pixels=0.0, max_image_size=-1):
        """The PINHOLE camera the images of a camera are resampled to (e3d_reg_undistort_plan) -> UndistortPlan."""
        plan = UndistortPlan()
        self._chk(lib().e3d_reg_undistort_plan(self._h, int(intrinsics_id), float(blank_pixels), int(max_image_size), C.byref(plan)),
                  "e3d_reg_undistort_plan")
        return plan

    def undistort(self, intrinsics_id, plan, kind, src, return_valid=False):
        """One level-0 image of the camera through the plan.  kind 0: (H, W) uint8 bilinear, 1: (H, W, 3) uint8 bilinear, 2: (H, W) uint8
        mask (bit-OR), 3: (H, W) float32 nearest (bits copied) -> the (plan.height, plan.width[, 3]) array, and with return_valid the
        uint8 validity map as well."""
        kind = int(kind)
        if kind not in _UNDISTORT_PIXEL:
            raise E3DError("e3d_reg_undistort: unknown kind %d" % kind)
        dtype, tail = _UNDISTORT_PIXEL[kind]
        src = np.ascontiguousarray(src, dtype)
        size = self._intr_size.get(int(intrinsics_id))
        if size is not None and src.shape != size + tail:
            raise E3DError("e3d_reg_undistort: the source is %s, the camera's level 0 %s" % (src.shape, size + tail))
        out = np.zeros((max(int(plan.height), 0), max(int(plan.width), 0)) + tail, dtype)
        valid = np.zeros(out.shape[:2], np.uint8) if return_valid else None
        self._chk(lib().e3d_reg_undistort(self._h, int(intrinsics_id), C.byref(plan), kind, C.c_void_p(src.ctypes.data), C.c_void_p(out.ctypes.data),
                                          C.c_void_p(valid.ctypes.data) if return_valid else None), "e3d_reg_undistort")
        return (out, valid) if return_valid else out

    def undistort_kernel_ms(self):
        """HIP-event time of the resampling kernel of the last undistort()."""
        ms = C.c_float()
        self._chk(lib().e3d_reg_undistort_kernel_ms(self._h, C.byref(ms)), "e3d_reg_undistort_kernel_ms")
        return float(ms.value)

    # ---- StereoPairCreator ------------------------------------------------------------------------------------------------------------
    def stereo_plan(self, left_image_id, right_image_id, blank_pixels=0.0, max_image_size=-1, focal_length=0.0):
        """The rectified camera, poses and rotations of a pair of images at their current poses (e3d_reg_stereo_plan) -> StereoPlan."""
        plan = StereoPlan()
        self._chk(lib().e3d_reg_stereo_plan(self._h, int(left_image_id), int(right_image_id), float(blank_pixels), int(max_image_size),
                                            float(focal_length), C.byref(plan)), "e3d_reg_stereo_plan")
        return plan

    def stereo_rectify(self, intrinsics_id, target, S, kind, src, return_valid=False):
        """undistort() with the ray of every output pixel rotated by S (9 float32, row-major source_T_rect) before the source model."""
        kind = int(kind)
        if kind not in _UNDISTORT_PIXEL:
            raise E3DError("e3d_reg_stereo_rectify: unknown kind %d" % kind)
        dtype, tail = _UNDISTORT_PIXEL[kind]
        src = np.ascontiguousarray(src, dtype)
        S = np.ascontiguousarray(S, np.float32).reshape(-1)
        if S.shape != (9,):
            raise E3DError("e3d_reg_stereo_rectify: S has %d entries, not 9" % S.size)
        size = self._intr_size.get(int(intrinsics_id))
        if size is not None and src.shape != size + tail:
            raise E3DError("e3d_reg_stereo_rectify: the source is %s, the camera's level 0 %s" % (src.shape, size + tail))
        out = np.zeros((max(int(target.height), 0), max(int(target.width), 0)) + tail, dtype)
        valid = np.zeros(out.shape[:2], np.uint8) if return_valid else None
        self._chk(lib().e3d_reg_stereo_rectify(self._h, int(intrinsics_id), C.byref(target), C.c_void_p(S.ctypes.data), kind,
                                               C.c_void_p(src.ctypes.data), C.c_void_p(out.ctypes.data),
                                               C.c_void_p(valid.ctypes.data) if return_valid else None), "e3d_reg_stereo_rectify")
        return (out, valid) if return_valid else out

    def stereo_kernel_ms(self):
        """HIP-event time of the resampling kernel of the last stereo_rectify()."""
        ms = C.c_float()
        self._chk(lib().e3d_reg_stereo_kernel_ms(self._h, C.byref(ms)), "e3d_reg_stereo_kernel_ms")
        return float(ms.value)

    def stereo_ground_truth(self, left_image_id, right_image_id, left_excluded=None, right_excluded=None, return_depth=False):
        """Disparity ground truth of the left of two rectified images (e3d_reg_stereo_ground_truth) -> (disparity float32, +inf =
        unknown; mask uint8 255 / 128 / 0 [, depth float32]), all (height, width).  Leaves the scan observation counters holding the
        counts over the two images."""
        shape = self._level0_shape(int(left_image_id))
        keep = []
        le = self._mask_ptr(left_excluded, shape, keep, "left_excluded") if left_excluded is not None else None
        re_ = self._mask_ptr(right_excluded, shape, keep, "right_excluded") if right_excluded is not None else None
        disparity = np.zeros(shape, np.float32); nocc = np.zeros(shape, np.uint8)
        depth = np.zeros(shape, np.float32) if return_depth else None
        self._chk(lib().e3d_reg_stereo_ground_truth(self._h, int(left_image_id), int(right_image_id), le, re_, C.c_void_p(disparity.ctypes.data),
                                                    C.c_void_p(nocc.ctypes.data), C.c_void_p(depth.ctypes.data) if return_depth else None),
                  "e3d_reg_stereo_ground_truth")
        return (disparity, nocc, depth) if return_depth else (disparity, nocc)

    @staticmethod
    def pose_from_bearings(points, bearings, q, t):
        """The module's pose_from_bearings (host only): the solve that follows pick_scan_points and image_bearings."""
        return pose_from_bearings(points, bearings, q, t)

    def set_cache_observations(self, enabled):
        """Optimizer::set_cache_observations: update_observations re-projects the cached point index lists."""
        self._chk(lib().e3d_reg_set_cache_observations(self._h, int(bool(enabled))), "e3d_reg_set_cache_observations")

    def determine_observed_indices(self):
        """ObservationsCache::DetermineAndSaveObservedPointIndices without the files (full visibility pass at image scale 0)."""
        self._chk(lib().e3d_reg_determine_observed_indices(self._h), "e3d_reg_determine_observed_indices")

    def get_observed_indices(self, image_id, point_scale):
        n = lib().e3d_reg_get_observed_indices(self._h, image_id, point_scale, None)
        if n < 0:
            self._chk(-1, "e3d_reg_get_observed_indices")
        out = np.zeros(n, np.uint64)
        if n:
            self._chk(int(min(0, lib().e3d_reg_get_observed_indices(self._h, image_id, point_scale, C.c_void_p(out.ctypes.data)))),
                      "e3d_reg_get_observed_indices")
        return out

    def set_observed_indices(self, image_id, point_scale, indices):
        indices = np.ascontiguousarray(indices, np.uint64)
        self._chk(lib().e3d_reg_set_observed_indices(self._h, image_id, point_scale, C.c_void_p(indices.ctypes.data), indices.size),
                  "e3d_reg_set_observed_indices")

    def color_update(self):
        self._chk(lib().e3d_reg_color_update(self._h), "e3d_reg_color_update")

    def compute_cost(self):
        c = C.c_double()
        self._chk(lib().e3d_reg_compute_cost(self._h, C.byref(c)), "e3d_reg_compute_cost")
        return c.value

    def apply(self, lam, print_progress=False):
        """IntrinsicsAndPoseOptimizer::Apply -> (applied_update, lambda, max_change)."""
        a = C.c_int(); l = C.c_float(lam); m = C.c_float()
        self._chk(lib().e3d_reg_apply(self._h, int(print_progress), C.byref(a), C.byref(l), C.byref(m)), "e3d_reg_apply")
        return bool(a.value), l.value, m.value

    def kernel_times(self, reset=True):
        """(pass 1 ms, pass 2 ms, observations, calls) of the accumulate kernels since the last reset (HIP events)."""
        out = (C.c_double * 4)()
        self._chk(lib().e3d_reg_kernel_times(self._h, out, int(bool(reset))), "e3d_reg_kernel_times")
        return tuple(out)

    def profile(self, enable):
        """Switches the phase profile of run_on_current_scale on / off; returns {phase: ms} recorded so far (e3d_reg_profile)."""
        buf = C.create_string_buffer(16384)
        self._chk(lib().e3d_reg_profile(self._h, int(bool(enable)), buf, len(buf)), "e3d_reg_profile")
        out = {}
        self.kernel_groups = {}      # {group: (HIP-event ms, launches, work units)} of the same record ("k:" entries)
        for item in buf.value.decode().split(";"):
            if "=" in item:
                k, v = item.rsplit("=", 1)
                if k.startswith("k:"):
                    ms, calls, units = v.split(",")
                    self.kernel_groups[k[2:]] = (float(ms), int(calls), float(units))
                else:
                    out[k] = float(v)
        return out

    def set_comm(self, comm):
        """Image sharding with the library's own RCCL communicator (a Comm); call before the images are set."""
        self._comm = comm
        self._chk(lib().e3d_reg_set_comm(self._h, comm.handle if comm is not None else None), "e3d_reg_set_comm")

    def set_shard(self, rank, world_size, allreduce=None, allreduce_device=None):
        """Image sharding over ranks (image id mod world_size).  allreduce(np.ndarray float64, in place);
        allreduce_device(ptr, count, dtype) sums a DEVICE buffer in place (dtype 0 = f32, 1 = i32) -- see dist.py.
        Must be called before the images are set."""
        def _wrap_host(buf, count, _user):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:  # noqa: BLE001 -- must not propagate through C
                import traceback
                traceback.print_exc()
                return 1

        def _wrap_dev(ptr, count, dtype, _user):
            try:
                allreduce_device(ptr, count, dtype)
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1
        self._cb_host = ALLREDUCE_FN(_wrap_host) if allreduce is not None else ALLREDUCE_FN()
        self._cb_dev = ALLREDUCE_DEVICE_FN(_wrap_dev) if allreduce_device is not None else ALLREDUCE_DEVICE_FN()
        self._chk(lib().e3d_reg_set_shard(self._h, int(rank), int(world_size), self._cb_host, self._cb_dev, None), "e3d_reg_set_shard")
        self._rank, self._world = int(rank), int(world_size)

    def image_owner(self, image_id):
        return self._chk(lib().e3d_reg_image_owner(self._h, int(image_id)), "e3d_reg_image_owner")

    def run_on_current_scale(self, max_num_iterations, max_change_convergence_threshold=0.0,
                             iterations_without_new_optimum_threshold=15, print_progress=False):
        """Optimizer::RunOnCurrentScale -> (converged, optimum_cost, iterations)."""
        c = C.c_double(); it = C.c_int()
        r = self._chk(lib().e3d_reg_run_on_current_scale(self._h, max_num_iterations, max_change_convergence_threshold,
                                                         iterations_without_new_optimum_threshold, int(print_progress),
                                                         C.byref(c), C.byref(it)), "e3d_reg_run_on_current_scale")
        return bool(r), c.value, it.value

    def add_occlusion_mesh(self, vertices, triangles, compute_edges=True):
        v = np.ascontiguousarray(vertices, np.float32); t = np.ascontiguousarray(triangles, np.uint32)
        return self._chk(lib().e3d_reg_add_occlusion_mesh(self._h, C.c_void_p(v.ctypes.data), v.shape[0], C.c_void_p(t.ctypes.data), t.shape[0],
                                                           1 if compute_edges else 0), "e3d_reg_add_occlusion_mesh")

    def clear_occlusion_meshes(self):
        self._chk(lib().e3d_reg_clear_occlusion_meshes(self._h), "e3d_reg_clear_occlusion_meshes")

    def set_occlusion_options(self, min_depth=0.05, max_depth=100.0, mask_occlusion_boundaries=True):
        self._chk(lib().e3d_reg_set_occlusion_options(self._h, min_depth, max_depth, 1 if mask_occlusion_boundaries else 0), "e3d_reg_set_occlusion_options")

    def occlusion_edge_count(self, mesh_index):
        return self._chk(lib().e3d_reg_occlusion_edge_count(self._h, mesh_index), "e3d_reg_occlusion_edge_count")

    def set_splat_points(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32)
        self._chk(lib().e3d_reg_set_splat_points(self._h, C.c_void_p(xyz.ctypes.data), xyz.shape[0]), "e3d_reg_set_splat_points")

    def render_depth(self, image_id, image_scale, shape=None):
        out = np.zeros(shape, np.float32) if shape is not None else None
        self._chk(lib().e3d_reg_render_depth(self._h, image_id, image_scale, C.c_void_p(out.ctypes.data) if out is not None else None), "e3d_reg_render_depth")
        return out

    def observe(self, image_id, point_scale, image_scale, border_size, indices=None):
        if indices is None:
            n = lib().e3d_reg_observe(self._h, image_id, point_scale, image_scale, border_size, None, 0)
        else:
            idx = np.ascontiguousarray(indices, np.uint32)
            n = lib().e3d_reg_observe(self._h, image_id, point_scale, image_scale, border_size, C.c_void_p(idx.ctypes.data), len(idx))
        return int(self._chk(n, "e3d_reg_observe"))

    def get_observations(self, image_id, point_scale, n):
        idx = np.zeros(n, np.uint32); x = np.zeros(n, np.float32); y = np.zeros(n, np.float32); s = np.zeros(n, np.float32); f = np.zeros(n, np.uint8)
        self._chk(lib().e3d_reg_get_observations(self._h, image_id, point_scale, *[C.c_void_p(a.ctypes.data) for a in (idx, x, y, s, f)]), "get_observations")
        return idx, x, y, s, f

    def set_observations(self, image_id, point_scale, idx, x, y, s):
        idx = np.ascontiguousarray(idx, np.uint32); x, y, s = [np.ascontiguousarray(a, np.float32) for a in (x, y, s)]
        self._chk(lib().e3d_reg_set_observations(self._h, image_id, point_scale, len(idx), *[C.c_void_p(a.ctypes.data) for a in (idx, x, y, s)]), "set_observations")

    def point_radius_minmax(self, xyz):
        """ComputeMinMaxPointRadius over the images of this problem -> (min_radius, max_radius)."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        mn = np.zeros(xyz.shape[0], np.float32); mx = np.zeros(xyz.shape[0], np.float32)
        self._chk(lib().e3d_reg_point_radius_minmax(self._h, C.c_void_p(xyz.ctypes.data), xyz.shape[0], C.c_void_p(mn.ctypes.data),
                                                    C.c_void_p(mx.ctypes.data)), "e3d_reg_point_radius_minmax")
        return mn, mx

    def set_rig(self, rig_id, image_T_rig):
        """image_T_rig: list of (q wxyz, t) per camera, camera 0 = reference."""
        q = np.ascontiguousarray([p[0] for p in image_T_rig], np.float32); t = np.ascontiguousarray([p[1] for p in image_T_rig], np.float32)
        self._chk(lib().e3d_reg_set_rig(self._h, rig_id, len(image_T_rig), C.c_void_p(q.ctypes.data), C.c_void_p(t.ctypes.data)), "e3d_reg_set_rig")

    def get_rig(self, rig_id, camera):
        q = np.zeros(4, np.float32); t = np.zeros(3, np.float32)
        self._chk(lib().e3d_reg_get_rig(self._h, rig_id, camera, C.c_void_p(q.ctypes.data), C.c_void_p(t.ctypes.data)), "e3d_reg_get_rig")
        return q, t

    def add_rig_images(self, rig_id, image_ids):
        ids = np.ascontiguousarray(image_ids, np.int32)
        self._chk(lib().e3d_reg_add_rig_images(self._h, rig_id, C.c_void_p(ids.ctypes.data), len(ids)), "e3d_reg_add_rig_images")
        for i in image_ids[1:]:
            self._dependent.add(int(i))

    def param_count(self, image_id):
        return self._nparams[self._image_intr[image_id]]

    def local_unknowns(self, image_id):
        return self.param_count(image_id) + (12 if image_id in self._dependent else 6)

    def pass1(self, image_id, point_scale, n):
        I = np.zeros(n, np.float32); ji = np.zeros((n, self.param_count(image_id)), np.float32); jp = np.zeros((n, 6), np.float32)
        self._chk(lib().e3d_reg_pass1(self._h, image_id, point_scale, *[C.c_void_p(a.ctypes.data) for a in (I, ji, jp)]), "e3d_reg_pass1")
        return I, ji, jp

    def accumulate(self, image_id, point_scale):
        V = self.local_unknowns(image_id)
        H = np.zeros((V, V)); b = np.zeros(V); sums = np.zeros(2); counts = np.zeros(2, np.int64)
        self._chk(lib().e3d_reg_accumulate(self._h, image_id, point_scale, *[C.c_void_p(a.ctypes.data) for a in (H, b, sums, counts)]), "e3d_reg_accumulate")
        return H, b, sums, counts

    def cost(self, image_id, point_scale):
        sums = np.zeros(2); counts = np.zeros(2, np.int64)
        self._chk(lib().e3d_reg_cost(self._h, image_id, point_scale, C.c_void_p(sums.ctypes.data), C.c_void_p(counts.ctypes.data)), "e3d_reg_cost")
        return sums, counts

    def color_begin(self, point_scale):
        self._chk(lib().e3d_reg_color_begin(self._h, point_scale), "e3d_reg_color_begin")

    def color_accumulate(self, image_id, point_scale):
        self._chk(lib().e3d_reg_color_accumulate(self._h, image_id, point_scale), "e3d_reg_color_accumulate")

    def color_finish(self, point_scale):
        self._chk(lib().e3d_reg_color_finish(self._h, point_scale), "e3d_reg_color_finish")
