// SplatCreator -- drop-in replacement of the reference tool (src/exe/splat_creator.cc:75-235): for every point of a point +
// normal cloud that the surface mesh does not represent well (the centre or a corner of its splat farther than
// --distance_threshold from the mesh), a normal-aligned square splat of the 5th-neighbour radius is written as two triangles
// of a binary PLY mesh -- the --occlusion_splats_path input of ImageRegistrator.  The kNN, the point-to-mesh distances and the
// splats run on the MI355X (e3d_create_splats); splats are written in ascending point order.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "e3d_loader.h"
#include "io_ply.h"
#include "util.h"

using namespace e3d_host;

int main(int argc, char** argv) {
  std::string point_normal_cloud_path;
  parse_argument(argc, argv, "--point_normal_cloud_path", point_normal_cloud_path);
  std::string mesh_path;
  parse_argument(argc, argv, "--mesh_path", mesh_path);
  std::string output_path;
  parse_argument(argc, argv, "--output_path", output_path);
  float distance_threshold = 0.02f;
  parse_argument(argc, argv, "--distance_threshold", distance_threshold);
  float max_splat_size = std::numeric_limits<float>::infinity();
  parse_argument(argc, argv, "--max_plat_size", max_splat_size);       // (the reference's spelling)

  if (point_normal_cloud_path.empty() || mesh_path.empty() || output_path.empty()) {
    std::cout << "Please provide input / output paths." << std::endl;
    return EXIT_FAILURE;
  }

  std::cerr << "Loading point cloud ..." << std::endl;
  PointCloud cloud;
  if (loadPLYFile(point_normal_cloud_path, cloud) < 0) return EXIT_FAILURE;
  if (cloud.normals.size() != cloud.xyz.size()) {
    std::cerr << "[loadPLYFile] no normals in " << point_normal_cloud_path << std::endl;
    return EXIT_FAILURE;
  }
  std::cerr << "Loading mesh ..." << std::endl;
  std::vector<float> vertices;
  std::vector<uint32_t> triangles;
  if (loadPLYMesh(mesh_path, vertices, triangles) < 0) return EXIT_FAILURE;

  std::cerr << "Generating splats ..." << std::endl;
  const size_t n = cloud.size();
  std::vector<float> splats(12 * n);
  const int64_t m = api().e3d_create_splats(cloud.xyz.data(), cloud.normals.data(), n, vertices.data(), vertices.size() / 3,
                                            triangles.data(), triangles.size() / 3, distance_threshold, max_splat_size,
                                            splats.data(), n, nullptr, nullptr, nullptr);
  if (m < 0) {
    std::cerr << "SplatCreator: " << api().e3d_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  std::cerr << "Added " << m << " splats." << std::endl;

  // faces of splat s: (4s + 2, 4s + 1, 4s) and (4s, 4s + 3, 4s + 2) (:200-222)
  std::vector<int32_t> faces(6 * (size_t)m);
  for (int64_t s = 0; s < m; ++s) {
    const int32_t b = (int32_t)(4 * s);
    int32_t* f = &faces[6 * (size_t)s];
    f[0] = b + 2; f[1] = b + 1; f[2] = b; f[3] = b; f[4] = b + 3; f[5] = b + 2;
  }
  if (savePLYMeshBinary(output_path, splats.data(), 4 * (size_t)m, faces.data(), 2 * (size_t)m) < 0) return EXIT_FAILURE;
  std::cout << "Finished!" << std::endl;
  return EXIT_SUCCESS;
}
