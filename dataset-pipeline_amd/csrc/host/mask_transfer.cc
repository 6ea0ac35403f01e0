// MaskTransfer -- DatasetInspector's "Label transfer" button (src/dataset_inspector/gui_main_window.cc:476-559, the work in
// TransferLabels, :868-1054) as a batch step: the mask drawn in one image is carried to other images through the laser scans.  The
// reference does one pair per click on one CPU thread; here the source side runs once (e3d_reg_mask_transfer_source labels the scan
// points on the MI355X) and every target after it (e3d_reg_mask_transfer_target: point pass, 5 x 5 fill-in, merge with the target's
// own mask).  Set-up as in GroundTruthCreator: scans through the MeshLab project into the global frame, COLMAP state, images,
// occlusion geometry, scan points; no multi-resolution cloud, no upright rotation.
//
//   --scan_alignment_path, --image_base_path, --state_path          required
//   --occlusion_mesh_path, --occlusion_splats_path, --camera_ids_to_ignore and the opt::Parameters flags: as in the other tools
//   --source_image NAME|ID     the image whose mask is transferred: its name as images.txt has it (dslr/img_0.png) or its image id (the
//                              position of the image in the state, from 0, as the tools write it); its mask is
//                              masks_for_images/<camera dir>/<name>.png (Image::GetImageMaskPath) and must exist
//   --target_images A,B,...    names or ids; default: every other image.  Every target is computed from the source's mask as loaded
//   --transfer_eval_obs 0|1    also transfer kEvalObs (2) labels; default 0, the GUI's unchecked box
//   --output_folder_path DIR   write DIR/masks_for_images/<camera dir>/<name>.png and leave the dataset as it is, or
//   --in_place 1               overwrite / create the targets' own mask files ("Save image mask"); exactly one of the two
// Per target one line on stdout with the three numbers of the transfer; a target whose merged mask equals its existing mask (or is
// all zero without one) is reported and not written.
#include <cstdlib>
#include <iostream>
#include <string>
#include <unordered_set>
#include <vector>

#include "opt_problem.h"

using namespace e3d_host;

// a level-0 mask file: the camera's size, values 0 / 1 / 2 (image.cc:77-97)
static bool load_mask_file(const std::string& path, const HostIntrinsics& in, GrayImage* mask) {
  std::string err;
  *mask = imread_gray(path, &err);
  if (mask->empty()) { std::cerr << "Cannot read mask " << path << " (" << err << ")" << std::endl; return false; }
  if (mask->width != in.width || mask->height != in.height) { std::cerr << "Image and mask_ sizes differ! " << path << std::endl; return false; }
  for (uint8_t v : mask->data)
    if (v > 2) { std::cerr << "Unknown mask_ value in " << path << std::endl; return false; }
  return true;
}

static int run_tool(int argc, char** argv) {
  std::string scan_alignment_path, occlusion_mesh_path, occlusion_splats_path, image_base_path, state_path, output_folder_path,
      source_image, target_images;
  parse_argument(argc, argv, "--scan_alignment_path", scan_alignment_path);
  parse_argument(argc, argv, "--occlusion_mesh_path", occlusion_mesh_path);
  parse_argument(argc, argv, "--occlusion_splats_path", occlusion_splats_path);
  parse_argument(argc, argv, "--image_base_path", image_base_path);
  parse_argument(argc, argv, "--state_path", state_path);
  parse_argument(argc, argv, "--output_folder_path", output_folder_path);
  parse_argument(argc, argv, "--source_image", source_image);
  parse_argument(argc, argv, "--target_images", target_images);
  bool transfer_eval_obs = false, in_place = false;
  parse_argument(argc, argv, "--transfer_eval_obs", transfer_eval_obs);
  parse_argument(argc, argv, "--in_place", in_place);

  Problem problem;
  if (!problem.prm.SetFromArguments(argc, argv)) return EXIT_FAILURE;
  if (scan_alignment_path.empty() || image_base_path.empty() || state_path.empty()) {
    std::cerr << "Please specify all the required paths." << std::endl;
    return EXIT_FAILURE;
  }
  if (source_image.empty()) {
    std::cerr << "Please name the image whose mask is to be transferred with --source_image." << std::endl;
    return EXIT_FAILURE;
  }
  if (output_folder_path.empty() == !in_place) {
    std::cerr << "Please give exactly one of --output_folder_path and --in_place 1." << std::endl;
    return EXIT_FAILURE;
  }

  // the state, the images of the transfer and the source's mask: everything that can be refused is refused before the scans are read
  if (!problem.InitializeStateFromColmapModel(state_path, image_base_path, parse_camera_ids_to_ignore(argc, argv))) return EXIT_FAILURE;
  const int source_id = problem.FindImage(image_base_path, source_image);
  if (source_id < 0) { std::cerr << "--source_image " << source_image << " is not an image of the state." << std::endl; return EXIT_FAILURE; }
  std::vector<int> targets;
  if (target_images.empty()) {
    for (const auto& kv : problem.images) if (kv.first != source_id) targets.push_back(kv.first);
  } else {
    size_t begin = 0;
    while (begin <= target_images.size()) {                    // in the order given; a name given twice counts once
      const size_t end = std::min(target_images.find(',', begin), target_images.size());
      const std::string key = target_images.substr(begin, end - begin);
      begin = end + 1;
      if (key.empty()) continue;
      const int id = problem.FindImage(image_base_path, key);
      if (id < 0) { std::cerr << "--target_images: " << key << " is not an image of the state." << std::endl; return EXIT_FAILURE; }
      bool seen = false;
      for (int t : targets) seen = seen || t == id;
      if (!seen) targets.push_back(id);
    }
  }
  if (targets.empty()) { std::cerr << "No target images." << std::endl; return EXIT_FAILURE; }
  const HostImage& source = problem.images[source_id];
  const std::string source_mask_path = own_image_mask_path(source);
  if (!file_exists(source_mask_path)) {
    std::cerr << "The source image " << source.file_path << " has no mask (" << source_mask_path << "): nothing to transfer." << std::endl;
    return EXIT_FAILURE;
  }
  GrayImage source_mask;
  if (!load_mask_file(source_mask_path, problem.intrinsics_list[source.intrinsics_id], &source_mask)) return EXIT_FAILURE;

  // opt::LoadPointClouds: scans in the global frame, concatenated (an empty scan adds nothing); a project without meshes is refused
  std::vector<MeshInfo> scan_infos;
  if (!ReadMeshLabProject(scan_alignment_path, &scan_infos) || scan_infos.empty()) {
    std::cerr << "Cannot read scan poses from " << scan_alignment_path << std::endl;
    return EXIT_FAILURE;
  }
  std::cout << "Loading point clouds ..." << std::endl;
  const std::string project_dir = parent_path(scan_alignment_path);
  std::vector<float> all_points;
  for (const MeshInfo& info : scan_infos) {
    PointCloud global;
    if (!load_scan(info, project_dir, /*want_rgb=*/false, /*announce_unreadable=*/true, &global)) return EXIT_FAILURE;
    all_points.insert(all_points.end(), global.xyz.begin(), global.xyz.end());
  }
  std::cout << "Done." << std::endl;
  if (all_points.empty()) { std::cerr << "Point cloud is empty." << std::endl; return EXIT_FAILURE; }

  if (!problem.InitializeImages()) return EXIT_FAILURE;
  if (!occlusion_mesh_path.empty()) std::cout << "Loading Occlusion mesh" << std::endl;
  if (!problem.SetScanToolOcclusionGeometry(occlusion_mesh_path, occlusion_splats_path, all_points, nullptr)) return EXIT_FAILURE;
  if (!problem.SetScanPoints(all_points)) return EXIT_FAILURE;

  const int64_t labelled = api().e3d_reg_mask_transfer_source(problem.reg, source_id, source_mask.data.data(), transfer_eval_obs ? 1 : 0);
  if (labelled < 0) { std::cerr << "label transfer failed: " << api().e3d_last_error() << std::endl; return EXIT_FAILURE; }
  std::cout << "Source image " << source_id << " " << source.file_path << ": " << labelled << " of " << all_points.size() / 3
            << " scan points carry a label" << std::endl;

  size_t written = 0;
  for (int target_id : targets) {
    const HostImage& im = problem.images[target_id];
    const HostIntrinsics& in = problem.intrinsics_list[im.intrinsics_id];
    const std::string existing_path = own_image_mask_path(im);
    GrayImage existing;
    if (file_exists(existing_path) && !load_mask_file(existing_path, in, &existing)) return EXIT_FAILURE;
    GrayImage merged;
    merged.width = in.width; merged.height = in.height;
    merged.data.resize((size_t)in.width * in.height);
    int64_t stats[3] = {0, 0, 0};
    if (api().e3d_reg_mask_transfer_target(problem.reg, target_id, existing.empty() ? nullptr : existing.data.data(), merged.data.data(), stats) < 0) {
      std::cerr << "label transfer failed: " << api().e3d_last_error() << std::endl;
      return EXIT_FAILURE;
    }
    std::cout << "Target image " << target_id << " " << im.file_path << ": point_pass " << stats[0] << " filled " << stats[1] << " changed " << stats[2];
    if (stats[2] == 0) { std::cout << " -- unchanged, not written" << std::endl; continue; }
    const std::string out_path = in_place ? existing_path : image_mask_path(output_folder_path, im);
    create_directories(parent_path(out_path));
    std::string err;
    if (!imwrite_gray(out_path, merged, &err)) { std::cout << std::endl; std::cerr << err << std::endl; return EXIT_FAILURE; }
    std::cout << " -> " << out_path << std::endl;
    ++written;
  }
  std::cout << "Wrote " << written << " of " << targets.size() << " masks." << std::endl;
  return EXIT_SUCCESS;
}

int main(int argc, char** argv) { return run_main("MaskTransfer", run_tool, argc, argv); }
