// SfMScaleEstimator -- drop-in replacement of the reference tool (src/exe/sfm_scale_estimator.cc:146-611): compares the depth of the
// SfM points observed in the cube map faces with the laser depth CubeMapRenderer wrote for those pixels, takes the geometric mean of
// the ratios as the scale of the SfM model, and writes the initial scan alignment (meshlab_project.mlp, the input of
// ICPScanAligner) and the scaled COLMAP model (colmap_model/, the input of ImageRegistrator).  Host only: file handling and a
// few thousand f32 operations; the GPU library is neither linked nor loaded.
//
// log and exp: include/e3d_libm.h defines atan, atan2, sin, cos, tan and log2 only, so the natural logarithm and the exponential
// are the C library's float functions (within 1 ulp), as in the reference's own build.  The 3 x 3 products follow the natural
// order (a0 b0 + a1 b1) + a2 b2; Eigen's order for them is not pinned by anything, and the outputs carry six digits.
#include <dirent.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "io_colmap.h"
#include "io_mlp.h"
#include "util.h"

using namespace e3d_host;

namespace {

enum class Direction { kFront = 0, kLeft, kBack, kRight, kUp, kDown, kInvalid };

struct CubeMapFace {
  Direction direction = Direction::kInvalid;
  std::string image_filename, depth_map_filename;
  std::vector<ColmapFeatureObservation> observations;     // those with a 3D point
  float image_R_global[9], image_t_global[3];             // row-major
  float global_R_image[9], global_t_image[3];
};

struct ScanPose {
  std::string scan_filename;
  float R[9], t[3];
};

// "image.png" -> "image.depth"
std::string DepthMapFilenameFromImageFilename(const std::string& image_filename) {
  return image_filename.substr(0, image_filename.rfind('.') + 1) + "depth";
}

// "<base>.<face>.png" -> face
Direction DirectionFromImageFilename(const std::string& image_filename) {
  if (image_filename.size() < 5) return Direction::kInvalid;
  const size_t second_last_dot_pos = image_filename.find_last_of('.', image_filename.size() - 5);
  const std::string name = image_filename.substr(second_last_dot_pos + 1, image_filename.size() - 4 - (second_last_dot_pos + 1));
  static const char* names[6] = {"front", "left", "back", "right", "up", "down"};
  for (int i = 0; i < 6; ++i)
    if (name == names[i]) return (Direction)i;
  return Direction::kInvalid;
}

// "<base>.<face>.png" -> "<base>.intrinsics.txt"
std::string IntrinsicsPathFromImagePath(const std::string& image_path) {
  const size_t second_last_dot_pos = image_path.size() < 5 ? std::string::npos : image_path.find_last_of('.', image_path.size() - 5);
  return image_path.substr(0, second_last_dot_pos + 1) + "intrinsics.txt";
}

// "dir/<scan>.ply.<face>.png" -> "<scan>.ply"
std::string ScanFilenameFromImagePath(const std::string& image_path) {
  const size_t last_slash_pos = image_path.find_last_of('/');
  const size_t ply_pos = image_path.find(".ply", last_slash_pos + 1);
  if (ply_pos == std::string::npos) return "";
  return image_path.substr(last_slash_pos + 1, ply_pos - last_slash_pos - 1 + strlen(".ply"));
}

// Eigen::Quaternionf(w, x, y, z).toRotationMatrix(), no normalisation
void quaternion_to_matrix(const float* q /*w x y z*/, float* R) {
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.f - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.f - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.f - (txx + tyy);
}

inline float dot3(const float* a, int sa, const float* b, int sb) { return (a[0] * b[0] + a[sa] * b[sb]) + a[2 * sa] * b[2 * sb]; }

bool LoadCubeMapFaces(const std::string& path, int cube_map_face_camera_id, std::vector<ColmapImageWithObservations>* images,
                      std::vector<CubeMapFace>* faces) {
  const std::string images_file_path = join_path(path, "images.txt");
  if (!ReadColmapImagesWithObservations(images_file_path, images)) {
    std::cout << "Cannot read file " << images_file_path << std::endl;
    return false;
  }
  for (const ColmapImageWithObservations& im : *images) {
    if (im.camera_id != cube_map_face_camera_id) continue;      // only cube map faces, not other images
    std::cout << "Found cube map face: " << im.file_path << std::endl;
    CubeMapFace face;
    face.image_filename = im.file_path;
    face.depth_map_filename = DepthMapFilenameFromImageFilename(im.file_path);
    face.direction = DirectionFromImageFilename(im.file_path);
    quaternion_to_matrix(im.q_from_double, face.image_R_global);
    for (int i = 0; i < 3; ++i) face.image_t_global[i] = im.t_from_double[i];
    // global_T_image: R^T and (R^T * -1) * t
    float neg[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) { face.global_R_image[3 * r + c] = face.image_R_global[3 * c + r]; neg[3 * r + c] = face.global_R_image[3 * r + c] * -1.f; }
    for (int r = 0; r < 3; ++r) face.global_t_image[r] = dot3(&neg[3 * r], 1, face.image_t_global, 1);
    for (const ColmapFeatureObservation& o : im.observations)
      if (o.point3d_id >= 0) face.observations.push_back(o);
    faces->push_back(face);
  }
  return true;
}

// the first entry of an id is kept (std::unordered_map::insert)
bool LoadPoints3D(const std::string& path, std::unordered_map<int, std::vector<float>>* points_3d) {
  const std::string points_file_path = join_path(path, "points3D.txt");
  std::ifstream f(points_file_path);
  if (!f) {
    std::cout << "Cannot read file " << points_file_path << std::endl;
    return false;
  }
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream s(line);
    int id = 0;
    std::vector<float> p(3, 0.f);
    s >> id >> p[0] >> p[1] >> p[2];
    points_3d->insert(std::make_pair(id, p));
  }
  return true;
}

// R of the scan in the frame of the face it was rendered into (cube_map_renderer.cc:165-225)
bool face_rotation(Direction d, float* R) {
  static const float M[6][9] = {
      {1, 0, 0, 0, 1, 0, 0, 0, 1},        // front
      {0, 0, 1, 0, 1, 0, -1, 0, 0},       // left
      {-1, 0, 0, 0, 1, 0, 0, 0, -1},      // back
      {0, 0, -1, 0, 1, 0, 1, 0, 0},       // right
      {1, 0, 0, 0, 0, 1, 0, -1, 0},       // up
      {1, 0, 0, 0, 0, -1, 0, 1, 0}};      // down
  if (d == Direction::kInvalid) return false;
  memcpy(R, M[(int)d], sizeof(float) * 9);
  return true;
}

bool copy_file(const std::string& from, const std::string& to) {
  std::ifstream in(from, std::ios::binary);
  if (!in) return false;
  std::ofstream out(to, std::ios::binary);
  out << in.rdbuf();
  return (bool)out || in.peek() == EOF;      // (an empty source leaves failbit on `out << rdbuf`)
}

}  // namespace

int main(int argc, char** argv) {
  std::string sfm_model_path;
  parse_argument(argc, argv, "-s", sfm_model_path);
  std::string sfm_image_path;
  parse_argument(argc, argv, "-si", sfm_image_path);
  std::string scans_path;
  parse_argument(argc, argv, "-i", scans_path);
  std::string output_path;
  parse_argument(argc, argv, "-o", output_path);
  int cube_map_face_camera_id = 1;
  parse_argument(argc, argv, "--cube_map_face_camera_id", cube_map_face_camera_id);

  if (sfm_model_path.empty() || sfm_image_path.empty() || scans_path.empty() || output_path.empty()) {
    std::cout << "Please provide input paths." << std::endl;
    return EXIT_FAILURE;
  }

  std::vector<ColmapImageWithObservations> images;
  std::vector<CubeMapFace> cube_map_faces;
  if (!LoadCubeMapFaces(sfm_model_path, cube_map_face_camera_id, &images, &cube_map_faces)) return EXIT_FAILURE;
  std::unordered_map<int, std::vector<float>> points_3d;
  if (!LoadPoints3D(sfm_model_path, &points_3d)) return EXIT_FAILURE;

  // Accumulate scaling information from each point observation at a pixel with depth (:423-494), f32, in file order.
  float geom_sum = 0.f;
  int factor_count = 0;
  for (const CubeMapFace& face : cube_map_faces) {
    int image_width = 0, image_height = 0;
    float image_fx, image_fy, image_cx, image_cy;
    const std::string intrinsics_path = join_path(sfm_image_path, IntrinsicsPathFromImagePath(face.image_filename));
    std::ifstream intrinsics_stream(intrinsics_path);
    if (!intrinsics_stream) {
      std::cout << "Cannot read file " << intrinsics_path << " (path derived from " << face.image_filename << ")" << std::endl;
      return EXIT_FAILURE;
    }
    std::string line;
    while (std::getline(intrinsics_stream, line)) {
      if (line.empty() || line[0] == '#') continue;
      std::istringstream line_stream(line);
      line_stream >> image_width >> image_height >> image_fx >> image_fy >> image_cx >> image_cy;
      break;
    }
    std::cout << "Image size: " << image_width << " " << image_height << std::endl;
    if (image_width <= 0 || image_height <= 0) {
      std::cout << "Error: No image size in " << intrinsics_path << std::endl;
      return EXIT_FAILURE;
    }

    std::vector<float> depth_image((size_t)image_width * image_height);
    FILE* file = fopen(join_path(sfm_image_path, face.depth_map_filename).c_str(), "rb");
    if (!file) {
      std::cout << "Error: Cannot read depth file " << face.depth_map_filename << std::endl;
      return EXIT_FAILURE;
    }
    const size_t got = fread(depth_image.data(), sizeof(float), depth_image.size(), file);
    fclose(file);
    if (got != depth_image.size()) {
      std::cout << "Error: Depth file " << face.depth_map_filename << " has unexpected size." << std::endl;
      return EXIT_FAILURE;
    }

    for (const ColmapFeatureObservation& observation : face.observations) {
      // Is there a laser depth measurement for this observation?  (the float is tested before the conversion: a value
      // beyond the int range converts to INT_MIN on x86 and is rejected there as well)
      if (!(observation.x > -1.f && observation.x < (float)image_width && observation.y > -1.f && observation.y < (float)image_height)) continue;
      const int ix = static_cast<int>(observation.x), iy = static_cast<int>(observation.y);
      const float measured_depth = depth_image[(size_t)iy * image_width + ix];
      if (std::isinf(measured_depth) || std::isnan(measured_depth) || measured_depth <= 0.f) continue;
      // Estimated depth: the reconstructed 3D point in the image's frame.
      const auto it = points_3d.find(observation.point3d_id);
      if (it == points_3d.end()) {
        std::cout << "Error: " << face.image_filename << " observes point " << observation.point3d_id << ", which points3D.txt lacks." << std::endl;
        return EXIT_FAILURE;
      }
      const float estimated_depth = dot3(&face.image_R_global[6], 1, it->second.data(), 1) + face.image_t_global[2];
      if (estimated_depth <= 0.f) continue;
      const float factor = measured_depth / estimated_depth;
      geom_sum += std::log(factor);
      factor_count += 1;
    }
  }

  // One pose per scan, from the first of its faces (:496-555): no averaging over the faces.
  std::vector<ScanPose> scan_poses;
  for (const CubeMapFace& face : cube_map_faces) {
    const std::string scan_filename = ScanFilenameFromImagePath(face.image_filename);
    bool have_pose = false;
    for (const ScanPose& scan_pose : scan_poses) have_pose = have_pose || scan_pose.scan_filename == scan_filename;
    if (have_pose) continue;
    ScanPose pose;
    pose.scan_filename = scan_filename;
    float R[9];
    if (!face_rotation(face.direction, R)) {
      std::cout << "Invalid cube map direction." << std::endl;
      return EXIT_FAILURE;
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) pose.R[3 * r + c] = dot3(&face.global_R_image[3 * r], 1, &R[c], 3);
    for (int i = 0; i < 3; ++i) pose.t[i] = face.global_t_image[i];
    scan_poses.push_back(pose);
  }

  const float geom_result = std::exp(geom_sum / factor_count);
  printf("Scaling factor: %.9g (from %d observations)\n", geom_result, factor_count);      // (all nine digits: the value is checked)
  fflush(stdout);

  // MeshLab project with the initial scan alignment (:244-295); paths relative to the output folder
  create_directories(output_path);
  {
    std::vector<MlpMesh> meshes;
    for (const ScanPose& pose : scan_poses) {
      MlpMesh m;
      m.label = pose.scan_filename;
      m.filename = relative_path(output_path, join_path(scans_path, pose.scan_filename));
      std::ostringstream t;
      t << std::endl;
      // The spaces at the end are important, MeshLab will crash when omitted.
      for (int r = 0; r < 3; ++r)
        t << pose.R[3 * r] << " " << pose.R[3 * r + 1] << " " << pose.R[3 * r + 2] << " " << geom_result * pose.t[r] << " " << std::endl;
      t << "0 0 0 1 " << std::endl;
      m.matrix_text = t.str();
      m.has_matrix = true;
      meshes.push_back(m);
    }
    const std::string mlp_path = join_path(output_path, "meshlab_project.mlp");
    if (!WriteMeshLabProjectXml(mlp_path, meshes)) std::cout << "Could not save MeshLab project: " << mlp_path << std::endl;
  }

  // Scaled COLMAP model (:297-385)
  const std::string scaled_model_path = join_path(output_path, "colmap_model");
  create_directories(scaled_model_path);
  bool ok = copy_file(join_path(sfm_model_path, "cameras.txt"), join_path(scaled_model_path, "cameras.txt"));
  if (!ok) std::cout << "Cannot copy " << join_path(sfm_model_path, "cameras.txt") << std::endl;
  {
    std::ifstream rigs(join_path(sfm_model_path, "rigs.json"));
    if (rigs && ok) ok = copy_file(join_path(sfm_model_path, "rigs.json"), join_path(scaled_model_path, "rigs.json"));
  }
  if (ok) {
    // image_T_global's translation times the factor; the inverse's translation scales with it and is not written
    for (ColmapImageWithObservations& im : images)
      for (int i = 0; i < 3; ++i) im.t[i] *= geom_result;
    ok = WriteColmapImages(join_path(scaled_model_path, "images.txt"), images);
  }
  ok = ok && ScaleColmapPoints3D(join_path(sfm_model_path, "points3D.txt"), join_path(scaled_model_path, "points3D.txt"), geom_result);
  if (!ok) {
    std::cout << "Scaling the COLMAP model failed." << std::endl;
    return EXIT_FAILURE;
  }

  // Warning in case not all scans got aligned (:571-607): scan<digits>.ply files of the scans folder without a face
  std::vector<std::string> non_aligned_scans;
  if (DIR* dir = opendir(scans_path.c_str())) {
    while (const dirent* e = readdir(dir)) {
      const std::string filename = e->d_name;
      if (filename.size() < 8 || filename.substr(filename.size() - 4) != ".ply" || filename.substr(0, 4) != "scan" ||
          filename.substr(4, filename.size() - 8).find_first_not_of("0123456789") != std::string::npos)
        continue;
      bool aligned = false;
      for (const CubeMapFace& face : cube_map_faces) aligned = aligned || ScanFilenameFromImagePath(face.image_filename) == filename;
      if (!aligned) non_aligned_scans.push_back(filename);
    }
    closedir(dir);
  }
  std::sort(non_aligned_scans.begin(), non_aligned_scans.end());
  if (!non_aligned_scans.empty()) {
    std::cout << "WARNING: SfM did not provide initial estimates for all scan poses." << std::endl;
    std::cout << "The following scans must be aligned manually:" << std::endl;
    for (const std::string& name : non_aligned_scans) std::cout << "  " << name << std::endl;
    std::cout << "Finished." << std::endl;
    return EXIT_FAILURE;
  }

  std::cout << "Finished!" << std::endl;
  return EXIT_SUCCESS;
}
