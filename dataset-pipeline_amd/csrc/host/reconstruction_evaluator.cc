// ReconstructionEvaluator -- what the ground truth is for: the ETH3D evaluation scheme of the reference's README (a point within a
// tolerance of the scans is accurate, a point in the free space between a scanner and what it measured is wrong, everything else is
// unobserved and not judged), which neither tree computes.  A reconstructed point cloud is set against the scans of a MeshLab
// project (points/scan_alignment.mlp as GroundTruthCreator reads it); the rules: include/e3d_hip.h, e3d_evaluate_reconstruction.
// The scanner of a scan sits at the origin of its own file, so its position is the translation of the scan's global_T_mesh.
//
//   ReconstructionEvaluator --reconstruction_ply_path rec.ply --ground_truth_mlp_path scan_alignment.mlp
//                           [--tolerances 0.01,0.02,0.05,0.1,0.2,0.5] [--voxel_size 0.01] [--cube_map_size 2048] [--scores_json PATH]
//                           [--accuracy_cloud_output_path P] [--completeness_cloud_output_path P] [--cloud_tolerance T] [--timings]
//
// stdout: four lines, "Tolerances:", "Completenesses:", "Accuracies:", "F1-scores:".  The clouds are the reconstruction and the scan
// points coloured at --cloud_tolerance (default: the smallest): accurate / complete 0 255 0, inaccurate / incomplete 255 0 0,
// unobserved 0 0 255; ignored (non-finite) points are left out.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "e3d_loader.h"
#include "io_ply.h"
#include "scan_loader.h"
#include "util.h"

using namespace e3d_host;

namespace {

constexpr int kMaxTolerances = 8;

// "0.01,0.02" -> floats in the order given; false for an empty item or one that is not a number
bool parse_float_list(const std::string& text, std::vector<float>* out) {
  size_t begin = 0;
  while (true) {
    const size_t end = text.find(',', begin);
    const std::string item = text.substr(begin, end == std::string::npos ? std::string::npos : end - begin);
    char* rest = nullptr;
    const float v = strtof(item.c_str(), &rest);
    if (item.empty() || *rest != 0) return false;
    out->push_back(v);
    if (end == std::string::npos) return true;
    begin = end + 1;
  }
}

int fail(const std::string& message) {
  std::cerr << "ReconstructionEvaluator: " << message << std::endl;
  return EXIT_FAILURE;
}

std::string json_list(const double* v, int n) {
  std::string s = "[";
  char buf[64];
  for (int i = 0; i < n; ++i) {
    snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", v[i]);
    s += buf;
  }
  return s + "]";
}

// the points with class != 255 and their colours
int save_coloured(const std::string& path, const std::vector<float>& xyz, const std::vector<uint8_t>& near_cls, const uint8_t* free_cls, int level) {
  std::vector<float> kept;
  std::vector<uint8_t> rgb;
  for (size_t i = 0; i < near_cls.size(); ++i) {
    if (near_cls[i] == 255) continue;
    kept.insert(kept.end(), xyz.begin() + 3 * i, xyz.begin() + 3 * i + 3);
    const bool good = near_cls[i] <= level, bad = !good && (!free_cls || level < free_cls[i]);
    rgb.push_back(bad ? 255 : 0); rgb.push_back(good ? 255 : 0); rgb.push_back(!good && !bad ? 255 : 0);
  }
  return savePLYFileBinaryXYZRGB(path, kept, rgb);
}

int run_tool(int argc, char** argv) {
  std::string reconstruction_ply_path, ground_truth_mlp_path, tolerances_text = "0.01,0.02,0.05,0.1,0.2,0.5", scores_json;
  std::string accuracy_cloud_output_path, completeness_cloud_output_path, cloud_tolerance_text;
  parse_argument(argc, argv, "--reconstruction_ply_path", reconstruction_ply_path);
  parse_argument(argc, argv, "--ground_truth_mlp_path", ground_truth_mlp_path);
  parse_argument(argc, argv, "--tolerances", tolerances_text);
  float voxel_size = 0.01f;
  parse_argument(argc, argv, "--voxel_size", voxel_size);
  int cube_map_size = 2048;
  parse_argument(argc, argv, "--cube_map_size", cube_map_size);
  parse_argument(argc, argv, "--scores_json", scores_json);
  parse_argument(argc, argv, "--accuracy_cloud_output_path", accuracy_cloud_output_path);
  parse_argument(argc, argv, "--completeness_cloud_output_path", completeness_cloud_output_path);
  parse_argument(argc, argv, "--cloud_tolerance", cloud_tolerance_text);
  const bool timings = find_argument(argc, argv, "--timings") > 0;

  // every argument is checked before anything is loaded
  if (reconstruction_ply_path.empty() || ground_truth_mlp_path.empty()) return fail("please provide --reconstruction_ply_path and --ground_truth_mlp_path.");
  std::vector<float> tolerances;
  bool tolerances_ok = parse_float_list(tolerances_text, &tolerances) && tolerances.size() <= (size_t)kMaxTolerances;
  for (size_t i = 0; tolerances_ok && i < tolerances.size(); ++i)
    tolerances_ok = std::isfinite(tolerances[i]) && tolerances[i] > 0.f && (i == 0 || tolerances[i] > tolerances[i - 1]);
  if (!tolerances_ok) return fail("--tolerances must be 1 to 8 positive numbers in strictly ascending order, separated by commas.");
  const int T = (int)tolerances.size();
  if (!std::isfinite(voxel_size) || !(voxel_size > 0.f)) return fail("--voxel_size must be positive.");
  if (cube_map_size < 2 || cube_map_size > 8192 || cube_map_size % 2) return fail("--cube_map_size must be even, from 2 to 8192.");
  int cloud_level = 0;
  if (!cloud_tolerance_text.empty()) {
    std::vector<float> one;
    cloud_level = -1;
    if (parse_float_list(cloud_tolerance_text, &one) && one.size() == 1)
      for (int i = 0; i < T; ++i)
        if (tolerances[i] == one[0]) cloud_level = i;
    if (cloud_level < 0) return fail("--cloud_tolerance must be one of --tolerances.");
  }
  std::vector<MeshInfo> scan_infos;
  if (!ReadMeshLabProject(ground_truth_mlp_path, &scan_infos) || scan_infos.empty()) return fail("cannot read scan poses from " + ground_truth_mlp_path);

  std::cerr << "Loading the reconstruction ..." << std::endl;
  PointCloud reconstruction;
  if (loadPLYFile(reconstruction_ply_path, reconstruction) < 0) return EXIT_FAILURE;
  std::cerr << "Loading scans ..." << std::endl;
  const std::string project_dir = parent_path(ground_truth_mlp_path);
  std::vector<float> scan_points, origins;
  std::vector<int64_t> offsets(1, 0);
  for (const MeshInfo& info : scan_infos) {
    PointCloud global;
    if (!load_scan(info, project_dir, /*want_rgb=*/false, /*announce_unreadable=*/true, &global)) return EXIT_FAILURE;
    scan_points.insert(scan_points.end(), global.xyz.begin(), global.xyz.end());
    offsets.push_back((int64_t)(scan_points.size() / 3));
    origins.insert(origins.end(), info.global_T_mesh.t, info.global_T_mesh.t + 3);
  }

  std::cerr << "Evaluating ..." << std::endl;
  e3d_eval_t* eval = api().e3d_evaluate_reconstruction(reconstruction.xyz.data(), reconstruction.size(), scan_points.data(), offsets.data(), origins.data(),
                                                       (int)scan_infos.size(), tolerances.data(), T, voxel_size, cube_map_size);
  if (!eval) return fail(api().e3d_last_error());
  int64_t n_scan_voxels = 0, n_rec_voxels = 0, evaluated[kMaxTolerances] = {0};
  double scores[3 * kMaxTolerances] = {0};
  std::vector<uint8_t> near_rec(reconstruction.size()), free_rec(reconstruction.size()), near_scan(scan_points.size() / 3);
  int r = api().e3d_eval_counts(eval, &n_scan_voxels, &n_rec_voxels, evaluated);
  if (r >= 0) r = api().e3d_eval_get_scores(eval, scores);
  if (r >= 0) r = api().e3d_eval_get_classes(eval, near_rec.data(), free_rec.data(), near_scan.data());
  if (timings) {
    float ms[16];
    const char* names[16];
    const int groups = api().e3d_eval_kernel_ms(eval, ms, names, 16);
    for (int g = 0; g < groups && g < 16; ++g) std::cerr << "[timings] " << names[g] << " " << ms[g] << " ms" << std::endl;
  }
  api().e3d_eval_destroy(eval);
  if (r < 0) return fail(api().e3d_last_error());

  static const char* const kLines[3] = {"Completenesses:", "Accuracies:", "F1-scores:"};
  std::cout << "Tolerances:";
  for (int i = 0; i < T; ++i) std::cout << " " << tolerances[i];
  std::cout << std::endl;
  for (int k = 0; k < 3; ++k) {
    std::cout << kLines[k];
    for (int i = 0; i < T; ++i) std::cout << " " << scores[k * T + i];
    std::cout << std::endl;
  }
  if (!scores_json.empty()) {
    std::vector<double> tol(tolerances.begin(), tolerances.end()), ev(evaluated, evaluated + T);
    std::ofstream f(scores_json);
    f << "{\"tolerances\": " << json_list(tol.data(), T) << ",\n \"completeness\": " << json_list(scores, T) << ",\n \"accuracy\": " << json_list(scores + T, T)
      << ",\n \"f1\": " << json_list(scores + 2 * T, T) << ",\n \"n_scan_voxels\": " << n_scan_voxels << ", \"n_rec_voxels\": " << n_rec_voxels
      << ", \"evaluated_voxels\": " << json_list(ev.data(), T) << "}\n";
    if (!f) return fail("cannot write " + scores_json);
  }
  if (!accuracy_cloud_output_path.empty() && save_coloured(accuracy_cloud_output_path, reconstruction.xyz, near_rec, free_rec.data(), cloud_level) < 0) return EXIT_FAILURE;
  if (!completeness_cloud_output_path.empty() && save_coloured(completeness_cloud_output_path, scan_points, near_scan, nullptr, cloud_level) < 0) return EXIT_FAILURE;
  return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char** argv) { return run_main("ReconstructionEvaluator", run_tool, argc, argv); }
