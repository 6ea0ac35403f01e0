// scan_loader.h -- one scan of a MeshLab project into the global frame: the per-scan part of opt::LoadPointClouds
// (src/opt/util.cc) that ImageRegistrator, GroundTruthCreator, MaskTransfer, ImageLocalizer and NormalEstimator share.
// The loop over the project stays with each tool, because what differs between them is policy: whether an empty project is
// refused, whether the scans are kept apart or concatenated, when "Done." is printed and when an empty result is refused.
// Apart from io_scans.h because it needs the library (api()); io_scans.h is also used by the host-only SfMScaleEstimator.
#pragma once

#include <iostream>
#include <string>
#include <vector>

#include "e3d_loader.h"
#include "io_ply.h"
#include "io_scans.h"

namespace e3d_host {

// a mesh's file as the project names it: an absolute path as it is, any other relative to the project's directory
inline std::string scan_file_path(const std::string& project_dir, const MeshInfo& info) {
  return (!info.filename.empty() && info.filename[0] == '/') ? info.filename : join_path(project_dir, info.filename);
}

// xyz (n x 3) <- T * xyz with the row-major 3x4 matrix T (pcl::transformPointCloud, f32, on the GPU).  An empty cloud is left alone
// without a call of the library, so a project of empty scans never loads it.
inline bool transform_points(std::vector<float>& xyz, const float* T) {
  if (xyz.empty()) return true;
  std::vector<float> out(xyz.size());
  float bmin[3], bmax[3];
  if (api().e3d_transform_cloud(xyz.data(), nullptr, xyz.size() / 3, T, out.data(), nullptr, bmin, bmax) < 0) {
    std::cerr << "transform failed: " << api().e3d_last_error() << std::endl;
    return false;
  }
  xyz.swap(out);
  return true;
}

// The scan `info` in the global frame: global->xyz, and global->rgb with want_rgb (0 0 0 per point for a file without colours).
// False with the message printed.  For a file that cannot be read that is the PLY reader's own line, followed by
// "Cannot load scan point clouds." where announce_unreadable is set: every tool but NormalEstimator says so.
inline bool load_scan(const MeshInfo& info, const std::string& project_dir, bool want_rgb, bool announce_unreadable, PointCloud* global) {
  PointCloud local;
  if (loadPLYFile(scan_file_path(project_dir, info), local, want_rgb) < 0) {
    if (announce_unreadable) std::cerr << "Cannot load scan point clouds." << std::endl;
    return false;
  }
  *global = PointCloud();
  global->xyz.swap(local.xyz);
  global->rgb.swap(local.rgb);
  float T[12];
  info.global_T_mesh.matrix3x4(T);
  return transform_points(global->xyz, T);
}

}  // namespace e3d_host
