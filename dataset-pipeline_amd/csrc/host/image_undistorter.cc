// ImageUndistorter -- PINHOLE copies of a dataset's images, masks, depth maps and calibration: the step the reference's README leaves to
// COLMAP's undistorter, and the form in which the published ETH3D sets ship next to the distorted ones (*_undistorted).  Per camera
// the library chooses the output camera (e3d_reg_undistort_plan), per image it resamples on the MI355X (e3d_reg_undistort); decoding
// and encoding (io_image.h) stay on the host.  Both rules are this project's own: include/e3d_hip.h states them.
//
//   --state_path DIR           COLMAP model (cameras.txt, images.txt, optionally rigs.json)                          required
//   --image_base_path DIR      the directory the image names of images.txt are relative to                          required
//   --output_folder_path DIR   the new dataset                                                                      required
//   --blank_pixels B           0 (default): crop to the part where every pixel has data; 1: keep every source pixel, the rest is blank
//   --max_image_size N         scale the focal length down so that neither side exceeds N pixels; default -1: keep the focal length
//   --depth_maps_path DIR      GroundTruthCreator's ground_truth_depth/ (io_depth.h): every image's map is carried over as well
//   --compress_depth_maps 0|1  write the new maps gzip-compressed
//   --camera_ids_to_ignore, --gpus N    as in the other tools (images are dealt out to the GPUs by image id, one host thread each)
// Written below DIR, with <images> the last component of --image_base_path:
//   <images>/<name>                         every image under its name in images.txt, in its own format (kind 1: bilinear)
//   <images>/masks_for_images/..., <images>/masks_for_cameras/...    where Image::GetImageMaskPath / GetCameraMaskPath look for the masks of
//                                           the written images (image.cc:168-195), for every mask the input has (kind 2: bit-OR, blank = 3)
//   ground_truth_depth/<camera dir>/<name>  with --depth_maps_path (kind 3: nearest, bits copied; the maps hold z-depth, which is constant
//                                           along a ray, so every sample is exact -- for maps rendered at the new resolution run
//                                           GroundTruthCreator on the new model instead)
//   calibration/                            the model as ExportToColmap writes it, nine digits: every camera PINHOLE, images, poses and rigs
//                                           unchanged, no 2D feature lines (their positions belong to the distorted images)
// One line per camera on stdout: old model and size -> new size and parameters.
#include <atomic>
#include <cstdlib>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "opt_problem.h"

using namespace e3d_host;

namespace {

enum Kind { kGray = 0, kRgb = 1, kMask = 2, kNearest = 3 };

std::string camera_mask_path_of(const std::string& image_file_path) {     // Image::GetCameraMaskPath
  const std::string image_dir = path_parent(image_file_path);
  return replace_extension(path_parent(image_dir) + "/masks_for_cameras/" + path_filename(image_dir), "png");
}

// one mask through the plan: read, check its size, resample (kind 2), write
bool carry_mask(e3d_reg_t* reg, const HostIntrinsics& in, const e3d_undistort_plan& plan, const std::string& from, const std::string& to,
                std::string* err) {
  GrayImage mask = imread_gray(from, err);
  if (mask.empty()) { *err = "Cannot read mask " + from + " (" + *err + ")"; return false; }
  if (mask.width != in.width || mask.height != in.height) { *err = "Image and mask_ sizes differ! " + from; return false; }
  GrayImage out;
  out.width = plan.width; out.height = plan.height;
  out.data.resize((size_t)plan.width * plan.height);
  if (api().e3d_reg_undistort(reg, in.intrinsics_id, &plan, kMask, mask.data.data(), out.data.data(), nullptr) < 0) {
    *err = std::string("e3d_reg_undistort: ") + api().e3d_last_error();
    return false;
  }
  create_directories(parent_path(to));
  return imwrite_gray(to, out, err);
}

}  // namespace

static int run_tool(int argc, char** argv) {
  std::string state_path, image_base_path, output_folder_path, depth_maps_path, blank_pixels_text = "0";
  parse_argument(argc, argv, "--state_path", state_path);
  parse_argument(argc, argv, "--image_base_path", image_base_path);
  parse_argument(argc, argv, "--output_folder_path", output_folder_path);
  parse_argument(argc, argv, "--depth_maps_path", depth_maps_path);
  parse_argument(argc, argv, "--blank_pixels", blank_pixels_text);
  int max_image_size = -1, gpus = 1;
  bool compress_depth_maps = false;
  parse_argument(argc, argv, "--max_image_size", max_image_size);
  parse_argument(argc, argv, "--compress_depth_maps", compress_depth_maps);
  parse_argument(argc, argv, "--gpus", gpus);
  if (gpus > 1 && !set_gpu_count(gpus)) return EXIT_FAILURE;
  if (state_path.empty() || image_base_path.empty() || output_folder_path.empty()) {
    std::cerr << "Please specify all the required paths." << std::endl;
    return EXIT_FAILURE;
  }
  char* blank_pixels_end = nullptr;
  const double blank_pixels = strtod(blank_pixels_text.c_str(), &blank_pixels_end);
  if (blank_pixels_text.empty() || *blank_pixels_end != 0) {
    std::cerr << "--blank_pixels " << blank_pixels_text << " is not a number." << std::endl;
    return EXIT_FAILURE;
  }
  while (image_base_path.size() > 1 && image_base_path.back() == '/') image_base_path.pop_back();

  Problem problem;
  if (!problem.InitializeStateFromColmapModel(state_path, image_base_path, parse_camera_ids_to_ignore(argc, argv))) return EXIT_FAILURE;
  std::vector<ColmapRig> rig_vector;
  if (ReadColmapRigs(state_path + "/rigs.json", &rig_vector) && !problem.AssignRigs(rig_vector)) return EXIT_FAILURE;

  // one device problem per GPU, each with the cameras at full resolution only: no image is uploaded, no pyramid is built
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
  const int n_gpus = gpu_count_setting();
  for (int r = 0; r < n_gpus; ++r) {
    if (n_gpus > 1 && api().e3d_init(r) < 1) { problem.lib_fail("e3d_init"); return EXIT_FAILURE; }
    e3d_reg_t* h = api().e3d_reg_create(&rp);
    if (!h) { problem.lib_fail("e3d_reg_create"); return EXIT_FAILURE; }
    problem.regs.push_back(h);
  }
  if (n_gpus > 1) api().e3d_init(0);
  problem.reg = problem.regs[0];
  for (const HostIntrinsics& in : problem.intrinsics_list)
    if (!problem.all_regs([&](e3d_reg_t* r) { return api().e3d_reg_set_intrinsics(r, in.intrinsics_id, in.model, in.width, in.height, in.params,
                                                                                 in.n_params, 0, 1); }, "e3d_reg_set_intrinsics"))
      return EXIT_FAILURE;

  // the output cameras: everything that can be refused is refused before an image is read
  std::vector<e3d_undistort_plan> plans(problem.intrinsics_list.size());
  for (const HostIntrinsics& in : problem.intrinsics_list) {
    e3d_undistort_plan& plan = plans[(size_t)in.intrinsics_id];
    if (api().e3d_reg_undistort_plan(problem.reg, in.intrinsics_id, blank_pixels, max_image_size, &plan) < 0) {
      std::cerr << "Camera " << in.intrinsics_id << " (" << in.model_name << " " << in.width << " x " << in.height << "): " << api().e3d_last_error() << std::endl;
      return EXIT_FAILURE;
    }
    std::cout.precision(9);
    std::cout << "Camera " << in.intrinsics_id << ": " << in.model_name << " " << in.width << " x " << in.height << " -> PINHOLE " << plan.width << " x "
              << plan.height << " " << plan.fx << " " << plan.fy << " " << plan.cx + 0.5f << " " << plan.cy + 0.5f << std::endl;
  }

  const std::string out_image_base = join_path(output_folder_path, path_filename(image_base_path));
  std::vector<const HostImage*> order;
  for (const auto& kv : problem.images) order.push_back(&kv.second);
  std::vector<std::string> new_paths(order.size());
  for (size_t i = 0; i < order.size(); ++i) new_paths[i] = join_path(out_image_base, relative_path(image_base_path, order[i]->file_path));

  // camera masks: once per camera, found next to its first image
  std::vector<bool> camera_done(problem.intrinsics_list.size(), false);
  for (size_t i = 0; i < order.size(); ++i) {
    const HostIntrinsics& in = problem.intrinsics_list[(size_t)order[i]->intrinsics_id];
    if (camera_done[(size_t)in.intrinsics_id]) continue;
    camera_done[(size_t)in.intrinsics_id] = true;
    const std::string from = camera_mask_path_of(order[i]->file_path);
    if (!file_exists(from)) continue;
    std::string err;
    if (!carry_mask(problem.reg, in, plans[(size_t)in.intrinsics_id], from, camera_mask_path_of(new_paths[i]), &err)) { std::cerr << err << std::endl; return EXIT_FAILURE; }
  }

  std::cout << "Undistorting " << order.size() << " images ..." << std::endl;
  std::vector<std::string> errors((size_t)n_gpus);
  std::atomic<bool> stop{false};
  auto work = [&](int rank) {
    e3d_reg_t* reg = problem.regs[(size_t)rank];
    std::string& err = errors[(size_t)rank];
    for (size_t i = 0; i < order.size() && !stop.load(); ++i) {
      const HostImage& im = *order[i];
      if (((im.image_id % n_gpus) + n_gpus) % n_gpus != rank) continue;
      const HostIntrinsics& in = problem.intrinsics_list[(size_t)im.intrinsics_id];
      const e3d_undistort_plan& plan = plans[(size_t)in.intrinsics_id];
      bool ok = false;
      do {
        ColorImage src = imread_color(im.file_path, &err);
        if (src.empty()) { err = "Cannot read image: " + im.file_path + " (" + err + ")"; break; }
        if (src.width != in.width || src.height != in.height) { err = "Image size differs from its camera: " + im.file_path; break; }
        ColorImage dst;
        dst.width = plan.width; dst.height = plan.height;
        dst.rgb.resize((size_t)plan.width * plan.height * 3);
        if (api().e3d_reg_undistort(reg, in.intrinsics_id, &plan, kRgb, src.rgb.data(), dst.rgb.data(), nullptr) < 0) {
          err = std::string("e3d_reg_undistort: ") + api().e3d_last_error();
          break;
        }
        create_directories(parent_path(new_paths[i]));
        if (!imwrite_color(new_paths[i], dst, &err)) break;
        const std::string mask_from = own_image_mask_path(im);
        if (file_exists(mask_from)) {
          HostImage moved = im;
          moved.file_path = new_paths[i];
          if (!carry_mask(reg, in, plan, mask_from, own_image_mask_path(moved), &err)) break;
        }
        if (!depth_maps_path.empty()) {
          std::vector<float> depth;
          if (!read_depth_map(depth_maps_path, im.file_path, in.width, in.height, &depth, &err)) break;
          std::vector<float> warped((size_t)plan.width * plan.height);
          if (api().e3d_reg_undistort(reg, in.intrinsics_id, &plan, kNearest, depth.data(), warped.data(), nullptr) < 0) {
            err = std::string("e3d_reg_undistort: ") + api().e3d_last_error();
            break;
          }
          const std::string to = depth_map_path(join_path(output_folder_path, "ground_truth_depth"), im.file_path);
          create_directories(parent_path(to));
          if (!write_float_map(to, warped, compress_depth_maps)) { err = "Cannot write to " + to; break; }
        }
        ok = true;
      } while (false);
      if (!ok) { stop.store(true); return; }
    }
  };
  std::vector<std::thread> pool;
  for (int r = 1; r < n_gpus; ++r) pool.emplace_back(work, r);
  work(0);
  for (std::thread& t : pool) t.join();
  for (const std::string& e : errors)
    if (!e.empty()) { std::cerr << e << std::endl; return EXIT_FAILURE; }

  // the new model: PINHOLE cameras (pixel-centre principal points; ExportToColmap adds COLMAP's half pixel), the images under their new paths
  for (HostIntrinsics& in : problem.intrinsics_list) {
    const e3d_undistort_plan& plan = plans[(size_t)in.intrinsics_id];
    in.model = E3D_CAMERA_PINHOLE; in.model_name = camera_model_name(in.model); in.n_params = camera_param_count(in.model);
    in.width = plan.width; in.height = plan.height;
    in.params[0] = plan.fx; in.params[1] = plan.fy; in.params[2] = plan.cx; in.params[3] = plan.cy;
  }
  for (size_t i = 0; i < order.size(); ++i) problem.images[order[i]->image_id].file_path = new_paths[i];
  const std::string calibration = join_path(output_folder_path, "calibration");
  if (!problem.ExportToColmap(out_image_base, calibration, 9)) { std::cerr << "Cannot write to " << calibration << std::endl; return EXIT_FAILURE; }
  if (!problem.rigs.empty() && !problem.ExportRigs(calibration)) return EXIT_FAILURE;
  std::cout << "Done." << std::endl;
  return EXIT_SUCCESS;
}

int main(int argc, char** argv) { return run_main("ImageUndistorter", run_tool, argc, argv); }
