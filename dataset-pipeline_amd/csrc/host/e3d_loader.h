// e3d_loader.h -- thin run-time loader of the C-ABI (include/e3d_hip.h) for the C++ host tools: dlopen()s
// libe3dhip.so and resolves the entry points.  There is no fallback: if the library or a symbol is missing the
// tools stop with an error message.
#pragma once

#include <dlfcn.h>
#include <libgen.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../../include/e3d_hip.h"

namespace e3d_host {

// Every entry point the tools resolve, once: X(name) becomes a member of Api and a dlsym() in api().  A new entry point goes here
// and nowhere else.
#define E3D_API_LIST(X)                                                                                                \
  X(e3d_abi_version) X(e3d_init) X(e3d_last_error)                                                                     \
  X(e3d_icp_create) X(e3d_icp_destroy) X(e3d_icp_add_cloud) X(e3d_icp_run) X(e3d_icp_get_pose)                         \
  X(e3d_transform_cloud) X(e3d_normals_knn) X(e3d_normals_radius) X(e3d_find_correspondences)                          \
  X(e3d_reg_create) X(e3d_reg_destroy) X(e3d_reg_set_params) X(e3d_reg_set_point_scale)                                \
  X(e3d_reg_set_intrinsics) X(e3d_reg_set_camera_mask) X(e3d_reg_get_intrinsics_level)                                 \
  X(e3d_reg_set_image) X(e3d_reg_set_image_pose) X(e3d_reg_get_image_pose)                                             \
  X(e3d_reg_set_rig) X(e3d_reg_get_rig) X(e3d_reg_add_rig_images) X(e3d_reg_set_rig_depth_residuals)                   \
  X(e3d_reg_set_splat_points) X(e3d_reg_run_on_current_scale) X(e3d_reg_compute_cost)                                  \
  X(e3d_determine_point_neighbors) X(e3d_reg_point_radius_minmax) X(e3d_merge_close_points)                            \
  X(e3d_reg_add_occlusion_mesh) X(e3d_reg_set_occlusion_options) X(e3d_reg_set_cache_observations)                     \
  X(e3d_reg_determine_observed_indices) X(e3d_reg_get_observed_indices) X(e3d_reg_set_observed_indices)                \
  X(e3d_local_outlier_removal) X(e3d_reg_set_scan_points) X(e3d_reg_count_scan_observations)                           \
  X(e3d_reg_get_scan_observation_counts) X(e3d_reg_ground_truth_depth) X(e3d_reg_scan_rendering)                       \
  X(e3d_comm_create_all) X(e3d_comm_destroy) X(e3d_comm_abort) X(e3d_icp_set_comm) X(e3d_reg_set_comm)                 \
  X(e3d_create_splats) X(e3d_render_cube_map)                                                                          \
  X(e3d_reg_scan_colors_begin) X(e3d_reg_scan_colors_add_image) X(e3d_reg_scan_colors_get_sums)                        \
  X(e3d_reg_scan_colors_set_sums) X(e3d_reg_scan_colors_finish)                                                        \
  X(e3d_reg_mask_transfer_source) X(e3d_reg_mask_transfer_target)                                                      \
  X(e3d_reg_pick_scan_points) X(e3d_reg_image_bearings) X(e3d_reg_project_points) X(e3d_pose_from_bearings)            \
  X(e3d_reg_render_depth) X(e3d_reg_set_depth_map_level0)                                                              \
  X(e3d_reg_undistort_plan) X(e3d_reg_undistort)                                                                       \
  X(e3d_reg_stereo_plan) X(e3d_reg_stereo_rectify) X(e3d_reg_stereo_ground_truth)                                      \
  X(e3d_edit_create) X(e3d_edit_destroy) X(e3d_edit_size) X(e3d_edit_get_points)                                       \
  X(e3d_edit_get_selection) X(e3d_edit_set_selection) X(e3d_edit_selection_count)                                      \
  X(e3d_edit_lasso) X(e3d_edit_beyond_plane) X(e3d_edit_pick)                                                          \
  X(e3d_edit_delete_selected) X(e3d_edit_extract_selected) X(e3d_edit_kernel_ms)                                       \
  X(e3d_surface_reconstruct) X(e3d_surface_destroy) X(e3d_surface_counts) X(e3d_surface_get_corners)                   \
  X(e3d_surface_get_mesh) X(e3d_surface_kernel_ms) X(e3d_surface_reconstruct_csg)                                      \
  X(e3d_surface_reconstruct_filled) X(e3d_surface_get_fill)                                                            \
  X(e3d_evaluate_reconstruction) X(e3d_eval_destroy) X(e3d_eval_counts) X(e3d_eval_get_scores)                         \
  X(e3d_eval_get_classes) X(e3d_eval_get_voxels) X(e3d_eval_kernel_ms)                                                 \
  X(e3d_evaluate_disparity) X(e3d_disp_eval_destroy) X(e3d_disp_eval_get_counts) X(e3d_disp_eval_get_sums)             \
  X(e3d_disp_eval_get_quantiles) X(e3d_disp_eval_kernel_ms)

struct Api {
  void* handle = nullptr;
  int device_count = 0;
#define E3D_MEMBER(name) decltype(&::name) name = nullptr;
  E3D_API_LIST(E3D_MEMBER)
#undef E3D_MEMBER
};

inline std::string exe_dir() {
  char buf[4096];
  const ssize_t n = readlink("/proc/self/exe", buf, sizeof buf - 1);
  if (n <= 0) return ".";
  buf[n] = 0;
  return std::string(dirname(buf));
}

inline Api& api() {
  static Api a;
  if (a.handle) return a;
  std::string tried;
  const char* env = getenv("E3D_HIP_LIBRARY");
  const std::string candidates[] = {env ? std::string(env) : std::string(), exe_dir() + "/../lib/libe3dhip.so",
                                    exe_dir() + "/libe3dhip.so", "libe3dhip.so"};
  for (const std::string& c : candidates) {
    if (c.empty()) continue;
    a.handle = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (a.handle) break;
    tried += "\n  " + c + ": " + dlerror();
  }
  if (!a.handle) {
    fprintf(stderr, "FATAL: cannot load the HIP library libe3dhip.so (set E3D_HIP_LIBRARY); tried:%s\n", tried.c_str());
    exit(EXIT_FAILURE);
  }
#define E3D_LOAD(name)                                                             \
  a.name = reinterpret_cast<decltype(a.name)>(dlsym(a.handle, #name));             \
  if (!a.name) { fprintf(stderr, "FATAL: libe3dhip.so lacks symbol %s\n", #name); exit(EXIT_FAILURE); }
  E3D_API_LIST(E3D_LOAD)
#undef E3D_LOAD
  if (a.e3d_abi_version() != E3D_ABI_VERSION) {
    fprintf(stderr, "FATAL: libe3dhip.so ABI version %d, expected %d\n", a.e3d_abi_version(), E3D_ABI_VERSION);
    exit(EXIT_FAILURE);
  }
  const char* dev = getenv("E3D_DEVICE");
  a.device_count = a.e3d_init(dev ? atoi(dev) : 0);
  if (a.device_count < 1) {
    fprintf(stderr, "FATAL: %s\n", a.e3d_last_error());
    exit(EXIT_FAILURE);
  }
  return a;
}

// --gpus N of the tools: one host thread per GPU inside the process, the library's own RCCL communicator between them
// (e3d_comm_create_all).  0 / 1 = single GPU.
inline int& gpu_count_setting() { static int n = 1; return n; }
inline bool set_gpu_count(int n) {
  if (n < 1) n = 1;
  if (n > api().device_count) {
    fprintf(stderr, "--gpus %d: only %d HIP device(s) visible\n", n, api().device_count);
    return false;
  }
  gpu_count_setting() = n;
  return true;
}

}  // namespace e3d_host
