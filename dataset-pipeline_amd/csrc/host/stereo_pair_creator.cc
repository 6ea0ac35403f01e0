// StereoPairCreator -- the two-view stereo sets of a registered scene, the third ETH3D product next to the multi-view sets
// (GroundTruthCreator, ImageUndistorter): per pair of images a rectified image pair, its calibration, and -- with scans -- the disparity
// ground truth of the left image with the mask that tells pixels seen by both cameras from half-occluded ones.  The library chooses the
// rectified camera (e3d_reg_stereo_plan), resamples (e3d_reg_stereo_rectify) and renders the ground truth
// (e3d_reg_stereo_ground_truth) on the MI355X; decoding and encoding (io_image.h) stay on the host.  The rules are this project's own:
// include/e3d_hip.h states them.
//
//   --state_path DIR           COLMAP model (cameras.txt, images.txt; rigs.json for --camera_pair)                   required
//   --image_base_path DIR      the directory the image names of images.txt are relative to                          required
//   --output_folder_path DIR   one folder per pair is written below it                                              required
//   --pairs FILE               lines "left_name right_name [pair_name]" (names as in images.txt; text after a hash sign is a comment);
//                              the default pair name is the left image's file stem
//   --camera_pair L,R          for every frame of rigs.json (images of the rig's cameras with the same file name), the images of the COLMAP
//                              camera ids L and R, left first.  The poses are those of images.txt as they stand.
//   --blank_pixels B           0 (default): crop towards the part both images cover; 1: keep every source pixel, the rest is blank
//   --max_image_size N         scale the focal length down so that neither side exceeds N pixels; default -1
//   --focal_length F           focal length of the rectified camera in pixels; default: the mean of the two cameras' fx, fy
//   --scan_alignment_path, --occlusion_mesh_path, --occlusion_splats_path    the scans and the occlusion geometry as GroundTruthCreator
//                              takes them (without its upright rotation: the poses written are those of the input frame); with scans the
//                              ground truth is written, without them images and calibration only
//   --camera_ids_to_ignore     as in the other tools
// A pair the plan refuses as given right-then-left is swapped, with a line on stdout; every other refusal ends the run before an image
// is read or a file is written.  One GPU.
// Written below <output>/<pair_name>/:
//   im0.png, im1.png     the rectified left and right image (kind 1: bilinear, blank pixels black)
//   calib.txt            Middlebury's keys: cam0=[f 0 cx; 0 f cy; 0 0 1], cam1= (the same matrix), doffs=0, baseline=B, width=, height=; nine
//                        digits.  The principal point is in the pixel-centre convention: (0, 0) is the centre of the top-left pixel, so
//                        a sample at x in im0 matches x - disparity in im1.  The baseline is in the length unit of the scans (of the
//                        poses of images.txt), not in millimetres as in Middlebury's own files.
//   cameras.txt, images.txt   COLMAP: one PINHOLE camera (id 0, principal point + 0.5: COLMAP's pixel-corner convention), the two
//                        rectified poses (ids 0 and 1), nine digits, no 2D feature lines
//   disp0GT.pfm          with scans: the disparity of the left image; "Pf", "W H", "-1.0", rows bottom to top, little-endian f32, +inf = unknown
//   mask0nocc.png        with scans: 255 = seen by both, 128 = ground truth known but the point is hidden from the right image, 0 = unknown
// No ground truth is given where a rectified image has no data or where its own image mask (masks_for_images/..., resampled with kind 2
// through the same rotation) holds the kEvalObs bit.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "opt_problem.h"

using namespace e3d_host;

namespace {

enum Kind { kGray = 0, kRgb = 1, kMask = 2, kNearest = 3 };
constexpr int kEvalObs = 2;                                  // opt::MaskType::kEvalObs (image.h:43-47)

struct Pair {
  int left = -1, right = -1;                                 // image ids
  std::string name;
  e3d_stereo_plan plan{};
};

std::string file_stem(const std::string& path) {
  const std::string name = path_filename(path);
  const size_t dot = name.find_last_of('.');
  return dot == std::string::npos ? name : name.substr(0, dot);
}

bool write_pfm(const std::string& path, const std::vector<float>& values, int width, int height) {
  std::ofstream f(path, std::ios::binary);
  f << "Pf\n" << width << " " << height << "\n-1.0\n";
  for (int y = height - 1; y >= 0; --y) f.write(reinterpret_cast<const char*>(values.data() + (size_t)y * width), sizeof(float) * (size_t)width);
  return (bool)f;
}

bool write_calibration(const std::string& dir, const e3d_stereo_plan& plan) {
  const e3d_undistort_plan& c = plan.camera;
  std::ofstream f(join_path(dir, "calib.txt"));
  f.precision(9);
  for (int i = 0; i < 2; ++i) f << "cam" << i << "=[" << c.fx << " 0 " << c.cx << "; 0 " << c.fy << " " << c.cy << "; 0 0 1]\n";
  f << "doffs=0\nbaseline=" << plan.baseline << "\nwidth=" << c.width << "\nheight=" << c.height << "\n";
  std::ofstream cf(join_path(dir, "cameras.txt"));
  cf.precision(9);
  cf << "# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n# Number of cameras: 1\n";
  cf << "0 PINHOLE " << c.width << " " << c.height << " " << c.fx << " " << c.fy << " " << c.cx + 0.5f << " " << c.cy + 0.5f << "\n";
  std::ofstream imf(join_path(dir, "images.txt"));
  imf.precision(9);
  imf << "# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
      << "#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: 2\n";
  for (int i = 0; i < 2; ++i) {
    const float* t = i == 0 ? plan.t_left : plan.t_right;
    imf << i << " " << plan.q_rect[0] << " " << plan.q_rect[1] << " " << plan.q_rect[2] << " " << plan.q_rect[3] << " " << t[0] << " " << t[1] << " "
        << t[2] << " 0 im" << i << ".png\n\n";
  }
  return (bool)f && (bool)cf && (bool)imf;
}

}  // namespace

static int run_tool(int argc, char** argv) {
  std::string state_path, image_base_path, output_folder_path, pairs_path, camera_pair, blank_pixels_text = "0", focal_length_text = "0";
  std::string scan_alignment_path, occlusion_mesh_path, occlusion_splats_path;
  parse_argument(argc, argv, "--state_path", state_path);
  parse_argument(argc, argv, "--image_base_path", image_base_path);
  parse_argument(argc, argv, "--output_folder_path", output_folder_path);
  parse_argument(argc, argv, "--pairs", pairs_path);
  parse_argument(argc, argv, "--camera_pair", camera_pair);
  parse_argument(argc, argv, "--blank_pixels", blank_pixels_text);
  parse_argument(argc, argv, "--focal_length", focal_length_text);
  parse_argument(argc, argv, "--scan_alignment_path", scan_alignment_path);
  parse_argument(argc, argv, "--occlusion_mesh_path", occlusion_mesh_path);
  parse_argument(argc, argv, "--occlusion_splats_path", occlusion_splats_path);
  int max_image_size = -1;
  parse_argument(argc, argv, "--max_image_size", max_image_size);
  Problem problem;
  if (!problem.prm.SetFromArguments(argc, argv)) return EXIT_FAILURE;
  if (state_path.empty() || image_base_path.empty() || output_folder_path.empty()) {
    std::cerr << "Please specify all the required paths." << std::endl;
    return EXIT_FAILURE;
  }
  if (pairs_path.empty() && camera_pair.empty()) {
    std::cerr << "Please specify the pairs: --pairs FILE and / or --camera_pair L,R." << std::endl;
    return EXIT_FAILURE;
  }
  auto number = [](const char* flag, const std::string& text, double* value) {
    char* end = nullptr;
    *value = strtod(text.c_str(), &end);
    if (text.empty() || *end != 0) { std::cerr << flag << " " << text << " is not a number." << std::endl; return false; }
    return true;
  };
  double blank_pixels = 0, focal_length = 0;
  if (!number("--blank_pixels", blank_pixels_text, &blank_pixels) || !number("--focal_length", focal_length_text, &focal_length)) return EXIT_FAILURE;
  while (image_base_path.size() > 1 && image_base_path.back() == '/') image_base_path.pop_back();

  // ---- the scans (opt::LoadPointClouds, as GroundTruthCreator loads them): before the state, whose translations take the scale factor
  // the first scan's matrix fixes; without scans the poses are taken as they stand ----
  const bool with_scans = !scan_alignment_path.empty();
  std::vector<float> all_points;
  if (with_scans) {
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
    if (all_points.empty()) { std::cerr << "Point cloud is empty." << std::endl; return EXIT_FAILURE; }
  } else if (global_scale_factor() == 0) {
    global_scale_factor() = 1.f;
  }

  const std::unordered_set<int> ignore = parse_camera_ids_to_ignore(argc, argv);
  if (!problem.InitializeStateFromColmapModel(state_path, image_base_path, ignore)) return EXIT_FAILURE;

  // ---- the pairs ----
  std::vector<Pair> pairs;
  if (!pairs_path.empty()) {
    std::ifstream f(pairs_path);
    if (!f) { std::cerr << "Cannot read " << pairs_path << std::endl; return EXIT_FAILURE; }
    std::string line;
    while (std::getline(f, line)) {
      const size_t hash = line.find('#');
      if (hash != std::string::npos) line.erase(hash);
      std::istringstream s(line);
      std::string left, right, name;
      if (!(s >> left)) continue;
      if (!(s >> right)) { std::cerr << pairs_path << ": a line needs two image names: " << line << std::endl; return EXIT_FAILURE; }
      s >> name;
      Pair p;
      p.left = problem.FindImage(image_base_path, left); p.right = problem.FindImage(image_base_path, right);
      if (p.left < 0 || p.right < 0) { std::cerr << pairs_path << ": no image " << (p.left < 0 ? left : right) << " in the state" << std::endl; return EXIT_FAILURE; }
      p.name = name.empty() ? file_stem(problem.images[p.left].file_path) : name;
      pairs.push_back(p);
    }
  }
  if (!camera_pair.empty()) {
    int ids[2] = {0, 0};
    char tail = 0;
    if (sscanf(camera_pair.c_str(), "%d,%d%c", &ids[0], &ids[1], &tail) != 2 || ids[0] == ids[1]) {
      std::cerr << "--camera_pair " << camera_pair << " is not two different camera ids L,R." << std::endl;
      return EXIT_FAILURE;
    }
    std::vector<ColmapRig> rig_vector;
    if (!ReadColmapRigs(state_path + "/rigs.json", &rig_vector)) { std::cerr << "--camera_pair needs " << state_path << "/rigs.json" << std::endl; return EXIT_FAILURE; }
    size_t found = 0;
    for (const ColmapRig& rig : rig_vector) {
      std::string prefix[2];
      for (const ColmapRigCamera& c : rig.cameras)
        for (int k = 0; k < 2; ++k) if (c.camera_id == ids[k]) prefix[k] = c.image_prefix;
      if (prefix[0].empty() || prefix[1].empty()) continue;
      for (const auto& kv : problem.images) {               // ascending image id: the frames in the order of their left images
        const HostImage& left = kv.second;
        if (path_filename(path_parent(left.file_path)) != prefix[0]) continue;
        for (const auto& other : problem.images) {
          const HostImage& right = other.second;
          if (path_filename(path_parent(right.file_path)) != prefix[1] || path_filename(right.file_path) != path_filename(left.file_path)) continue;
          Pair p;
          p.left = left.image_id; p.right = right.image_id; p.name = file_stem(left.file_path);
          pairs.push_back(p);
          ++found;
          break;
        }
      }
    }
    if (!found) { std::cerr << "--camera_pair " << camera_pair << ": no frame of rigs.json has images of both cameras" << std::endl; return EXIT_FAILURE; }
  }
  if (pairs.empty()) { std::cerr << "No pairs given." << std::endl; return EXIT_FAILURE; }
  for (size_t i = 0; i < pairs.size(); ++i)
    for (size_t j = 0; j < i; ++j)
      if (pairs[i].name == pairs[j].name) { std::cerr << "Two pairs are named " << pairs[i].name << ": give pair names in --pairs" << std::endl; return EXIT_FAILURE; }

  // ---- the device problem: the cameras at full resolution, the images as poses only ----
  e3d_reg_params rp{};
  rp.point_neighbor_count = problem.prm.point_neighbor_count;
  rp.robust_weighting_type = problem.prm.robust_weighting_type;
  rp.robust_weighting_parameter = problem.prm.robust_weighting_parameter;
  rp.fixed_residuals_weight = problem.prm.fixed_residuals_weight;
  rp.variable_residuals_weight = problem.prm.variable_residuals_weight;
  rp.maximum_valid_intensity = (float)problem.prm.maximum_valid_intensity;
  rp.occlusion_depth_threshold = problem.prm.occlusion_depth_threshold;
  rp.splat_radius = problem.prm.splat_radius;
  rp.image_scale_count = 1;
  rp.depth_robust_weighting_type = problem.prm.depth_robust_weighting_type;
  rp.depth_robust_weighting_parameter = problem.prm.depth_robust_weighting_parameter;
  e3d_reg_t* reg = api().e3d_reg_create(&rp);
  if (!reg) { problem.lib_fail("e3d_reg_create"); return EXIT_FAILURE; }
  problem.regs.push_back(reg);
  problem.reg = reg;
  for (const HostIntrinsics& in : problem.intrinsics_list)
    if (api().e3d_reg_set_intrinsics(reg, in.intrinsics_id, in.model, in.width, in.height, in.params, in.n_params, 0, 1) < 0) { problem.lib_fail("e3d_reg_set_intrinsics"); return EXIT_FAILURE; }
  int next_image_id = 0;
  for (const auto& kv : problem.images) {
    const HostImage& im = kv.second;
    if (api().e3d_reg_set_image(reg, im.image_id, im.intrinsics_id, nullptr, nullptr) < 0 ||
        api().e3d_reg_set_image_pose(reg, im.image_id, im.image_T_global.q, im.image_T_global.t) < 0) { problem.lib_fail("e3d_reg_set_image"); return EXIT_FAILURE; }
    next_image_id = std::max(next_image_id, im.image_id + 1);
  }

  // ---- the plans: everything that can be refused is refused before an image is read ----
  for (Pair& p : pairs) {
    int r = api().e3d_reg_stereo_plan(reg, p.left, p.right, blank_pixels, max_image_size, focal_length, &p.plan);
    if (r < 0 && std::string(api().e3d_last_error()).find("swap") != std::string::npos) {
      std::cout << "Pair " << p.name << ": given right-then-left, swapped." << std::endl;
      std::swap(p.left, p.right);
      r = api().e3d_reg_stereo_plan(reg, p.left, p.right, blank_pixels, max_image_size, focal_length, &p.plan);
    }
    if (r < 0) {
      std::cerr << "Pair " << p.name << " (" << relative_path(image_base_path, problem.images[p.left].file_path) << ", "
                << relative_path(image_base_path, problem.images[p.right].file_path) << "): " << api().e3d_last_error() << std::endl;
      return EXIT_FAILURE;
    }
    std::cout.precision(9);
    std::cout << "Pair " << p.name << ": PINHOLE " << p.plan.camera.width << " x " << p.plan.camera.height << " f " << p.plan.camera.fx << " baseline "
              << p.plan.baseline << std::endl;
  }

  if (with_scans) {
    if (!occlusion_mesh_path.empty()) std::cout << "Loading Occlusion mesh" << std::endl;
    if (!problem.SetScanToolOcclusionGeometry(occlusion_mesh_path, occlusion_splats_path, all_points, nullptr)) return EXIT_FAILURE;
    if (!problem.SetScanPoints(all_points)) return EXIT_FAILURE;
  }

  // ---- per pair: rectify, write, ground truth ----
  int next_intrinsics_id = (int)problem.intrinsics_list.size();
  for (const Pair& p : pairs) {
    const e3d_undistort_plan& cam = p.plan.camera;
    const size_t px = (size_t)cam.width * cam.height;
    const std::string dir = join_path(output_folder_path, p.name);
    create_directories(dir);
    std::vector<uint8_t> excluded[2];
    for (int side = 0; side < 2; ++side) {
      const HostImage& im = problem.images[side == 0 ? p.left : p.right];
      const HostIntrinsics& in = problem.intrinsics_list[(size_t)im.intrinsics_id];
      const float* S = side == 0 ? p.plan.S_left : p.plan.S_right;
      std::string err;
      ColorImage src = imread_color(im.file_path, &err);
      if (src.empty()) { std::cerr << "Cannot read image: " << im.file_path << " (" << err << ")" << std::endl; return EXIT_FAILURE; }
      if (src.width != in.width || src.height != in.height) { std::cerr << "Image size differs from its camera: " << im.file_path << std::endl; return EXIT_FAILURE; }
      ColorImage dst;
      dst.width = cam.width; dst.height = cam.height;
      dst.rgb.resize(px * 3);
      excluded[side].assign(px, 0);
      if (api().e3d_reg_stereo_rectify(reg, in.intrinsics_id, &cam, S, kRgb, src.rgb.data(), dst.rgb.data(), excluded[side].data()) < 0) {
        problem.lib_fail("e3d_reg_stereo_rectify");
        return EXIT_FAILURE;
      }
      if (!imwrite_color(join_path(dir, side == 0 ? "im0.png" : "im1.png"), dst, &err)) { std::cerr << err << std::endl; return EXIT_FAILURE; }
      for (uint8_t& v : excluded[side]) v = v ? 0 : 1;          // the validity map -> no data here
      const std::string mask_path = own_image_mask_path(im);
      if (with_scans && file_exists(mask_path)) {
        GrayImage mask = imread_gray(mask_path, &err);
        if (mask.empty() || mask.width != in.width || mask.height != in.height) { std::cerr << "Cannot use mask " << mask_path << " " << err << std::endl; return EXIT_FAILURE; }
        std::vector<uint8_t> warped(px);
        if (api().e3d_reg_stereo_rectify(reg, in.intrinsics_id, &cam, S, kMask, mask.data.data(), warped.data(), nullptr) < 0) {
          problem.lib_fail("e3d_reg_stereo_rectify");
          return EXIT_FAILURE;
        }
        for (size_t i = 0; i < px; ++i) if (warped[i] & kEvalObs) excluded[side][i] = 1;
      }
    }
    if (!write_calibration(dir, p.plan)) { std::cerr << "Cannot write to " << dir << std::endl; return EXIT_FAILURE; }
    if (!with_scans) continue;
    // the rectified cameras as the library wants them registered: one PINHOLE, two images without pixels
    const float params[4] = {cam.fx, cam.fy, cam.cx, cam.cy};
    const int intr = next_intrinsics_id++, left_id = next_image_id++, right_id = next_image_id++;
    if (api().e3d_reg_set_intrinsics(reg, intr, E3D_CAMERA_PINHOLE, cam.width, cam.height, params, 4, 0, 1) < 0) { problem.lib_fail("e3d_reg_set_intrinsics"); return EXIT_FAILURE; }
    if (api().e3d_reg_set_image(reg, left_id, intr, nullptr, nullptr) < 0 || api().e3d_reg_set_image(reg, right_id, intr, nullptr, nullptr) < 0 ||
        api().e3d_reg_set_image_pose(reg, left_id, p.plan.q_rect, p.plan.t_left) < 0 ||
        api().e3d_reg_set_image_pose(reg, right_id, p.plan.q_rect, p.plan.t_right) < 0) { problem.lib_fail("e3d_reg_set_image"); return EXIT_FAILURE; }
    std::vector<float> disparity(px);
    GrayImage nocc;
    nocc.width = cam.width; nocc.height = cam.height;
    nocc.data.resize(px);
    if (api().e3d_reg_stereo_ground_truth(reg, left_id, right_id, excluded[0].data(), excluded[1].data(), disparity.data(), nocc.data.data(), nullptr) < 0) {
      problem.lib_fail("e3d_reg_stereo_ground_truth");
      return EXIT_FAILURE;
    }
    std::string err;
    if (!write_pfm(join_path(dir, "disp0GT.pfm"), disparity, cam.width, cam.height)) { std::cerr << "Cannot write to " << dir << std::endl; return EXIT_FAILURE; }
    if (!imwrite_gray(join_path(dir, "mask0nocc.png"), nocc, &err)) { std::cerr << err << std::endl; return EXIT_FAILURE; }
  }
  std::cout << "Done." << std::endl;
  return EXIT_SUCCESS;
}

int main(int argc, char** argv) { return run_main("StereoPairCreator", run_tool, argc, argv); }
