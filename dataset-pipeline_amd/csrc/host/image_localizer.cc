// ImageLocalizer -- DatasetInspector's pose repair ("Pose verification and improvement" in the reference's README) as a batch step: the
// remedy for an image that SfM registered badly or not at all.  Three parts of the GUI, driven by a script instead of the mouse:
//   "Localize image"      src/dataset_inspector/localize_image_tool.cc: pairs of (scan point, image pixel), then an absolute-pose
//                         refinement on bearing vectors (:47-88); the click on a rendered scan point (:96-110) is
//                         e3d_reg_pick_scan_points on the MI355X, up to 32 clicks per pass over the scans
//   the positioning buttons   MainWindow::MoveImage (gui_main_window.cc:851-865)
//   "Distr. rel pose"     MainWindow::DistributeRelativePoseClicked (:605-655)
//
//   --state_path, --image_base_path, --script FILE, --output_folder_path DIR     required
//   --scan_alignment_path         required when the script has a `pick` or a `solve` line
//   --occlusion_mesh_path, --occlusion_splats_path, --camera_ids_to_ignore and the opt::Parameters flags: as in the other tools
//
// The script: one operation per line, `#` starts a comment.  Pixel coordinates are the reference's internal ones ((0, 0) = centre of
// the top-left pixel), what the --write_scan_renderings images show.
//   image NAME                                    the image the following lines work on (its name in images.txt, or its image id)
//   pick  SCAN_X SCAN_Y IMAGE_X IMAGE_Y           the visible scan point nearest to (SCAN_X, SCAN_Y) at the image's CURRENT pose belongs
//                                                 at (IMAGE_X, IMAGE_Y); pending picks are resolved together, at most 32 per pass, before
//                                                 the pose next changes
//   point X Y Z IMAGE_X IMAGE_Y                   a 3-D point of the global frame given directly
//   solve                                         >= 6 correspondences: sets the image's pose (e3d_pose_from_bearings from the current
//                                                 one) and clears the list; prints each correspondence's reprojection error before and after
//   move TX TY TZ YAW ROLL PITCH                  image_T_global = SE3f::exp((TX, TY, TZ, PITCH, YAW, ROLL)) * image_T_global
//   distribute_relative_pose                      the current image's pose relative to its rig's reference image goes into the rig and
//                                                 into every other image set of that rig (both branches of :627-654)
// Everything that can be refused is refused before the scans are read or the library is loaded.  A script without `pick` and `solve`
// needs neither: it runs on the host alone.  The state is written as ImageRegistrator writes its final state (cameras.txt, images.txt,
// points3D.txt, rigs.json).
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../../include/e3d_libm.h"
#include "opt_problem.h"

using namespace e3d_host;

namespace {

enum class Op { kImage, kPick, kPoint, kSolve, kMove, kDistribute };
struct ScriptLine { Op op; int line; std::string name; double v[6]; int image_id = -1; };
struct Correspondence { bool picked; float scan_xy[2]; float xyz[3]; float image_xy[2]; int64_t index; bool resolved; };

bool parse_number(const std::string& s, double* v) {
  char* end = nullptr;
  *v = strtod(s.c_str(), &end);
  return !s.empty() && end == s.c_str() + s.size() && std::isfinite(*v);
}

// the script -> operations; false (with a message) at the first line that cannot be an operation
bool parse_script(const std::string& path, std::vector<ScriptLine>* out) {
  std::ifstream f(path);
  if (!f) { std::cerr << "Cannot read the script " << path << std::endl; return false; }
  std::string text;
  int number = 0;
  bool have_image = false;
  while (std::getline(f, text)) {
    ++number;
    const size_t hash = text.find('#');
    if (hash != std::string::npos) text.resize(hash);
    std::istringstream ss(text);
    std::vector<std::string> tok;
    for (std::string t; ss >> t;) tok.push_back(t);
    if (tok.empty()) continue;
    ScriptLine l{};
    l.line = number;
    size_t want;
    if (tok[0] == "image") { l.op = Op::kImage; want = 1; }
    else if (tok[0] == "pick") { l.op = Op::kPick; want = 4; }
    else if (tok[0] == "point") { l.op = Op::kPoint; want = 5; }
    else if (tok[0] == "solve") { l.op = Op::kSolve; want = 0; }
    else if (tok[0] == "move") { l.op = Op::kMove; want = 6; }
    else if (tok[0] == "distribute_relative_pose") { l.op = Op::kDistribute; want = 0; }
    else { std::cerr << path << ":" << number << ": unknown operation '" << tok[0] << "'" << std::endl; return false; }
    if (tok.size() - 1 != want) {
      std::cerr << path << ":" << number << ": '" << tok[0] << "' takes " << want << " arguments, got " << tok.size() - 1 << std::endl;
      return false;
    }
    if (l.op == Op::kImage) { l.name = tok[1]; have_image = true; }
    else {
      if (!have_image) { std::cerr << path << ":" << number << ": '" << tok[0] << "' before any 'image' line" << std::endl; return false; }
      for (size_t k = 0; k < want; ++k)
        if (!parse_number(tok[1 + k], &l.v[k])) {
          std::cerr << path << ":" << number << ": '" << tok[1 + k] << "' is not a finite number" << std::endl;
          return false;
        }
    }
    out->push_back(l);
  }
  return true;
}

// Sophus' SE3f::exp of (upsilon | omega) in f32, sin and cos from the shared elementary functions: the rotation as a unit quaternion
// (series below theta = 1e-5), V = I + (1 - cos theta) / theta^2 W + (theta - sin theta) / theta^3 W^2 (the rotation matrix itself
// below 1e-5), translation V upsilon
Pose7 se3_exp(const float upsilon[3], const float omega[3]) {
  constexpr float kEpsilon = 1e-5f;
  const float theta_sq = omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2];
  float theta, imag, real;
  if (theta_sq < kEpsilon * kEpsilon) {
    theta = 0.f;
    const float theta_po4 = theta_sq * theta_sq;
    imag = 0.5f - (float)(1.0 / 48.0) * theta_sq + (float)(1.0 / 3840.0) * theta_po4;
    real = 1.f - (float)(1.0 / 8.0) * theta_sq + (float)(1.0 / 384.0) * theta_po4;
  } else {
    theta = std::sqrt(theta_sq);
    const float half = 0.5f * theta;
    imag = e3d_sinf(half) / theta;
    real = e3d_cosf(half);
  }
  Pose7 r;
  r.q[0] = real; r.q[1] = imag * omega[0]; r.q[2] = imag * omega[1]; r.q[3] = imag * omega[2];
  const float W[9] = {0, -omega[2], omega[1], omega[2], 0, -omega[0], -omega[1], omega[0], 0};
  float W2[9], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
  if (theta < kEpsilon) {
    double R[9];
    pose_rotation(r, R);
    for (int i = 0; i < 9; ++i) V[i] = (float)R[i];
  } else {
    const float a = (1.f - e3d_cosf(theta)) / theta_sq, b = (theta - e3d_sinf(theta)) / (theta_sq * theta);
    for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0 ? 1.f : 0.f) + a * W[i]) + b * W2[i];
  }
  for (int i = 0; i < 3; ++i) r.t[i] = V[3 * i] * upsilon[0] + V[3 * i + 1] * upsilon[1] + V[3 * i + 2] * upsilon[2];
  return r;
}

const HostRigImages* image_set_of(const Problem& problem, const HostImage& im) {
  if (im.rig_images_id < 0) return nullptr;
  for (const HostRigImages& f : problem.rig_images)
    if (f.rig_images_id == im.rig_images_id) return &f;
  return nullptr;
}

// DistributeRelativePoseClicked (:615-654) for `image_id`; the ids of the images whose pose changed go to `changed`
bool distribute_relative_pose(Problem& problem, int image_id, std::vector<int>* changed) {
  HostImage& image = problem.images[image_id];
  const HostRigImages* set = image_set_of(problem, image);
  if (!set) { std::cerr << "This image does not belong to a rig." << std::endl; return false; }
  HostRig* rig = nullptr;
  for (HostRig& r : problem.rigs) if (r.rig_id == set->rig_id) rig = &r;
  int index = -1;
  for (size_t c = 0; c < set->image_ids.size(); ++c) if (set->image_ids[c] == image_id) index = (int)c;
  if (!rig || index < 0) { std::cerr << "Internal error: cannot find the image in the rig_images set in which it is supposed to be." << std::endl; return false; }
  if (index != 0) {
    const Pose7 new_image_T_rig = pose_mul(image.image_T_global, pose_inverse(problem.images[set->image_ids[0]].image_T_global));
    rig->image_T_rig[(size_t)index] = new_image_T_rig;
    for (const HostRigImages& other : problem.rig_images) {
      if (other.rig_id != rig->rig_id) continue;
      HostImage& other_image = problem.images[other.image_ids[(size_t)index]];
      other_image.image_T_global = pose_mul(new_image_T_rig, problem.images[other.image_ids[0]].image_T_global);
      changed->push_back(other_image.image_id);
    }
  } else {
    if (set->image_ids.size() < 2) { std::cerr << "The rig has one camera only: nothing to distribute." << std::endl; return false; }
    std::vector<Pose7> new_image_T_rig(set->image_ids.size());
    const Pose7 global_T_image = pose_inverse(image.image_T_global);
    for (size_t c = 1; c < set->image_ids.size(); ++c) {
      new_image_T_rig[c] = pose_mul(problem.images[set->image_ids[c]].image_T_global, global_T_image);
      rig->image_T_rig[c] = new_image_T_rig[c];
    }
    // the reference camera's pose of every image set from the image with camera index 1 (the reference's own choice)
    for (const HostRigImages& other : problem.rig_images) {
      if (other.rig_id != rig->rig_id) continue;
      HostImage& other_image = problem.images[other.image_ids[0]];
      const Pose7 other_global_T_image = pose_mul(pose_inverse(problem.images[other.image_ids[1]].image_T_global), new_image_T_rig[1]);
      other_image.image_T_global = pose_inverse(other_global_T_image);
      changed->push_back(other_image.image_id);
    }
  }
  return true;
}

int run_tool(int argc, char** argv) {
  std::string scan_alignment_path, occlusion_mesh_path, occlusion_splats_path, image_base_path, state_path, output_folder_path, script_path;
  parse_argument(argc, argv, "--scan_alignment_path", scan_alignment_path);
  parse_argument(argc, argv, "--occlusion_mesh_path", occlusion_mesh_path);
  parse_argument(argc, argv, "--occlusion_splats_path", occlusion_splats_path);
  parse_argument(argc, argv, "--image_base_path", image_base_path);
  parse_argument(argc, argv, "--state_path", state_path);
  parse_argument(argc, argv, "--output_folder_path", output_folder_path);
  parse_argument(argc, argv, "--script", script_path);

  Problem problem;
  if (!problem.prm.SetFromArguments(argc, argv)) return EXIT_FAILURE;
  if (image_base_path.empty() || state_path.empty() || output_folder_path.empty() || script_path.empty()) {
    std::cerr << "Please specify all the required paths." << std::endl;
    return EXIT_FAILURE;
  }
  std::vector<ScriptLine> script;
  if (!parse_script(script_path, &script)) return EXIT_FAILURE;
  bool has_pick = false, needs_device = false;
  for (const ScriptLine& l : script) {
    has_pick = has_pick || l.op == Op::kPick;
    needs_device = needs_device || l.op == Op::kPick || l.op == Op::kSolve;
  }
  if (needs_device && scan_alignment_path.empty()) {
    std::cerr << "Please specify all the required paths (--scan_alignment_path: the script picks scan points or solves a pose)." << std::endl;
    return EXIT_FAILURE;
  }

  // the state; then the rest of what can be refused: image names, solve without enough correspondences, an image without a rig
  if (!problem.InitializeStateFromColmapModel(state_path, image_base_path, parse_camera_ids_to_ignore(argc, argv))) return EXIT_FAILURE;
  std::vector<ColmapRig> rig_vector;
  if (ReadColmapRigs(state_path + "/rigs.json", &rig_vector) && !problem.AssignRigs(rig_vector)) return EXIT_FAILURE;
  {
    int current = -1, pending = 0;
    for (ScriptLine& l : script) {
      if (l.op == Op::kImage) {
        current = problem.FindImage(image_base_path, l.name);
        if (current < 0) { std::cerr << script_path << ":" << l.line << ": " << l.name << " is not an image of the state." << std::endl; return EXIT_FAILURE; }
        pending = 0;
      }
      l.image_id = current;
      if (l.op == Op::kPick || l.op == Op::kPoint) ++pending;
      if (l.op == Op::kSolve) {
        if (pending < 6) {
          std::cerr << script_path << ":" << l.line << ": solve needs at least 6 correspondences, the list holds " << pending << std::endl;
          return EXIT_FAILURE;
        }
        pending = 0;
      }
      if (l.op == Op::kDistribute && !image_set_of(problem, problem.images[current])) {
        std::cerr << script_path << ":" << l.line << ": This image does not belong to a rig." << std::endl;
        return EXIT_FAILURE;
      }
    }
  }

  std::vector<float> all_points;
  if (needs_device) {
    // opt::LoadPointClouds as in MaskTransfer: concatenated (an empty scan adds nothing), a project without meshes is refused
    std::vector<MeshInfo> scan_infos;
    if (!ReadMeshLabProject(scan_alignment_path, &scan_infos) || scan_infos.empty()) {
      std::cerr << "Cannot read scan poses from " << scan_alignment_path << std::endl;
      return EXIT_FAILURE;
    }
    std::cout << "Loading point clouds ..." << std::endl;
    const std::string project_dir = parent_path(scan_alignment_path);
    for (const MeshInfo& info : scan_infos) {
      PointCloud global;
      if (!load_scan(info, project_dir, /*want_rgb=*/false, /*announce_unreadable=*/true, &global)) return EXIT_FAILURE;
      all_points.insert(all_points.end(), global.xyz.begin(), global.xyz.end());
    }
    std::cout << "Done." << std::endl;
    if (all_points.empty()) { std::cerr << "Point cloud is empty." << std::endl; return EXIT_FAILURE; }
    // the device holds every image on its own: this tool moves single images, the rig is applied by distribute_relative_pose alone
    std::vector<HostRig> rigs;
    std::vector<HostRigImages> rig_images;
    rigs.swap(problem.rigs); rig_images.swap(problem.rig_images);
    const bool initialised = problem.InitializeImages();
    rigs.swap(problem.rigs); rig_images.swap(problem.rig_images);
    if (!initialised) return EXIT_FAILURE;
    if (!problem.SetScanToolOcclusionGeometry(occlusion_mesh_path, occlusion_splats_path, all_points, nullptr)) return EXIT_FAILURE;   // no "Loading Occlusion mesh" line here
    if (has_pick && !problem.SetScanPoints(all_points)) return EXIT_FAILURE;
  }
  auto push_pose = [&](int image_id) {
    if (!needs_device) return true;
    const Pose7& T = problem.images[image_id].image_T_global;
    if (api().e3d_reg_set_image_pose(problem.reg, image_id, T.q, T.t) < 0) { std::cerr << "e3d_reg_set_image_pose: " << api().e3d_last_error() << std::endl; return false; }
    return true;
  };

  // the pose of an image with all the digits of its f32 values (the state files carry six)
  auto pose_text = [&](int image_id) {
    const Pose7& T = problem.images[image_id].image_T_global;
    std::ostringstream o;
    o.precision(9);
    o << "q " << T.q[0] << " " << T.q[1] << " " << T.q[2] << " " << T.q[3] << " t " << T.t[0] << " " << T.t[1] << " " << T.t[2];
    return o.str();
  };
  std::vector<Correspondence> list;
  // the pending picks of the list, E3D_LOCALIZE_MAX_CLICKS per pass over the scans, at the pose `image_id` has now
  auto resolve_picks = [&](int image_id) {
    std::vector<size_t> open;
    for (size_t k = 0; k < list.size(); ++k) if (list[k].picked && !list[k].resolved) open.push_back(k);
    for (size_t b = 0; b < open.size(); b += E3D_LOCALIZE_MAX_CLICKS) {
      const int n = (int)std::min<size_t>(E3D_LOCALIZE_MAX_CLICKS, open.size() - b);
      float clicks[2 * E3D_LOCALIZE_MAX_CLICKS];
      int64_t index[E3D_LOCALIZE_MAX_CLICKS];
      for (int k = 0; k < n; ++k) { clicks[2 * k] = list[open[b + k]].scan_xy[0]; clicks[2 * k + 1] = list[open[b + k]].scan_xy[1]; }
      const int64_t visible = api().e3d_reg_pick_scan_points(problem.reg, image_id, clicks, n, index, nullptr, nullptr);
      if (visible < 0) { std::cerr << "e3d_reg_pick_scan_points: " << api().e3d_last_error() << std::endl; return false; }
      for (int k = 0; k < n; ++k) {
        Correspondence& c = list[open[b + k]];
        if (index[k] < 0) {
          std::cerr << "pick " << c.scan_xy[0] << " " << c.scan_xy[1] << ": no scan point is visible in the image (" << visible << " visible points)" << std::endl;
          return false;
        }
        c.index = index[k]; c.resolved = true;
        for (int d = 0; d < 3; ++d) c.xyz[d] = all_points[3 * (size_t)index[k] + d];
      }
    }
    return true;
  };
  auto reprojection_errors = [&](int image_id, std::vector<float>* error, std::vector<uint8_t>* state) {
    std::vector<float> xyz(3 * list.size()), pixel(2 * list.size());
    state->assign(list.size(), 0); error->assign(list.size(), 0.f);
    for (size_t k = 0; k < list.size(); ++k) for (int d = 0; d < 3; ++d) xyz[3 * k + d] = list[k].xyz[d];
    if (api().e3d_reg_project_points(problem.reg, image_id, xyz.data(), list.size(), pixel.data(), state->data()) < 0) {
      std::cerr << "e3d_reg_project_points: " << api().e3d_last_error() << std::endl;
      return false;
    }
    for (size_t k = 0; k < list.size(); ++k) {
      const float dx = pixel[2 * k] - list[k].image_xy[0], dy = pixel[2 * k + 1] - list[k].image_xy[1];
      (*error)[k] = std::sqrt(dx * dx + dy * dy);
    }
    return true;
  };

  for (const ScriptLine& l : script) {
    const int id = l.image_id;
    // the pose is about to change (or to be solved for): the pending picks were made at the pose the image has now
    if ((l.op == Op::kSolve || l.op == Op::kMove || l.op == Op::kDistribute) && !list.empty() && !resolve_picks(id)) return EXIT_FAILURE;
    switch (l.op) {
      case Op::kImage:
        if (!list.empty()) std::cout << "Dropping " << list.size() << " correspondences without a solve." << std::endl;
        list.clear();
        std::cout << "Image " << id << " " << problem.images[id].file_path << std::endl;
        break;
      case Op::kPick: {
        Correspondence c{};
        c.picked = true; c.resolved = false; c.index = -1;
        c.scan_xy[0] = (float)l.v[0]; c.scan_xy[1] = (float)l.v[1]; c.image_xy[0] = (float)l.v[2]; c.image_xy[1] = (float)l.v[3];
        list.push_back(c);
        break;
      }
      case Op::kPoint: {
        Correspondence c{};
        c.picked = false; c.resolved = true; c.index = -1;
        for (int d = 0; d < 3; ++d) c.xyz[d] = (float)l.v[d];
        c.image_xy[0] = (float)l.v[3]; c.image_xy[1] = (float)l.v[4];
        list.push_back(c);
        break;
      }
      case Op::kSolve: {
        HostImage& im = problem.images[id];
        std::vector<float> before, after, pixels(2 * list.size());
        std::vector<uint8_t> state_before, state_after;
        std::vector<double> points(3 * list.size()), bearings(3 * list.size());
        if (!reprojection_errors(id, &before, &state_before)) return EXIT_FAILURE;
        for (size_t k = 0; k < list.size(); ++k) {
          pixels[2 * k] = list[k].image_xy[0]; pixels[2 * k + 1] = list[k].image_xy[1];
          for (int d = 0; d < 3; ++d) points[3 * k + d] = list[k].xyz[d];
        }
        if (api().e3d_reg_image_bearings(problem.reg, id, pixels.data(), (int)list.size(), bearings.data()) < 0) {
          std::cerr << "e3d_reg_image_bearings: " << api().e3d_last_error() << std::endl;
          return EXIT_FAILURE;
        }
        Pose7 solved;
        double stats[4];
        if (api().e3d_pose_from_bearings(points.data(), bearings.data(), (int)list.size(), im.image_T_global.q, im.image_T_global.t, solved.q, solved.t, stats) < 0) {
          std::cerr << "solve failed: " << api().e3d_last_error() << std::endl;
          return EXIT_FAILURE;
        }
        im.image_T_global = solved;
        if (!push_pose(id) || !reprojection_errors(id, &after, &state_after)) return EXIT_FAILURE;
        for (size_t k = 0; k < list.size(); ++k) {
          std::cout << "  correspondence " << k << ": ";
          if (list[k].picked) std::cout << "scan point " << list[k].index; else std::cout << "given point";
          std::cout << ", reprojection error " << before[k] << " px (state " << (int)state_before[k] << ") -> " << after[k] << " px (state "
                    << (int)state_after[k] << ")" << std::endl;
        }
        std::cout << "Solved image " << id << ": RMS bearing angle " << stats[0] << " -> " << stats[1] << " rad, " << (int)stats[2] << " iterations, "
                  << (stats[3] != 0 ? "converged" : "not converged") << ": " << pose_text(id) << std::endl;
        list.clear();
        break;
      }
      case Op::kMove: {
        const float upsilon[3] = {(float)l.v[0], (float)l.v[1], (float)l.v[2]};
        const float omega[3] = {(float)l.v[5], (float)l.v[3], (float)l.v[4]};        // (pitch, yaw, roll)
        HostImage& im = problem.images[id];
        im.image_T_global = pose_mul(se3_exp(upsilon, omega), im.image_T_global);
        if (!push_pose(id)) return EXIT_FAILURE;
        std::cout << "Moved image " << id << ": " << pose_text(id) << std::endl;
        break;
      }
      case Op::kDistribute: {
        std::vector<int> changed;
        if (!distribute_relative_pose(problem, id, &changed)) return EXIT_FAILURE;
        for (int other : changed) if (!push_pose(other)) return EXIT_FAILURE;
        std::cout << "Distributed the relative pose of image " << id << " to " << changed.size() << " images" << std::endl;
        for (int other : changed) std::cout << "  image " << other << ": " << pose_text(other) << std::endl;
        break;
      }
    }
  }
  if (!list.empty()) std::cout << "Dropping " << list.size() << " correspondences without a solve." << std::endl;

  if (!problem.ExportToColmap(image_base_path, output_folder_path)) { std::cerr << "Cannot write " << output_folder_path << std::endl; return EXIT_FAILURE; }
  if (!problem.rigs.empty() && !problem.ExportRigs(output_folder_path)) return EXIT_FAILURE;
  std::cout << "Wrote state to " << output_folder_path << std::endl;
  return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char** argv) { return run_main("ImageLocalizer", run_tool, argc, argv); }
