// SurfaceReconstructor -- the step the reference leaves to MeshLab / PoissonRecon ("External Surface Reconstruction" of its README):
// the merged point + normal cloud becomes the strongly subdivided triangle mesh that SplatCreator (--mesh_path), ImageRegistrator,
// GroundTruthCreator, MaskTransfer and ImageLocalizer (--occlusion_mesh_path) read.  A signed field of the oriented points is
// evaluated on a lattice of --voxel_size anchored at the world origin and one vertex per cell with a sign change is written
// (e3d_surface_reconstruct; the rules: include/e3d_hip.h).  The mesh ends where the data ends: unobserved regions are not filled.
//
//   SurfaceReconstructor --point_normal_cloud_path cloud.ply --output_path surface.ply [--voxel_size 0.02] [--support_radius 2 x voxel_size]
//                        [--timings]
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "e3d_loader.h"
#include "io_ply.h"
#include "util.h"

using namespace e3d_host;

int main(int argc, char** argv) {
  std::string point_normal_cloud_path;
  parse_argument(argc, argv, "--point_normal_cloud_path", point_normal_cloud_path);
  std::string output_path;
  parse_argument(argc, argv, "--output_path", output_path);
  float voxel_size = 0.02f;                                            // the default of SplatCreator --distance_threshold
  parse_argument(argc, argv, "--voxel_size", voxel_size);
  float support_radius = 2.f * voxel_size;
  parse_argument(argc, argv, "--support_radius", support_radius);
  const bool timings = find_argument(argc, argv, "--timings") > 0;

  if (point_normal_cloud_path.empty() || output_path.empty()) {
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

  std::cerr << "Reconstructing the surface ..." << std::endl;
  e3d_surface_t* surface = api().e3d_surface_reconstruct(cloud.xyz.data(), cloud.normals.data(), cloud.size(), voxel_size, support_radius);
  if (!surface) {
    std::cerr << "SurfaceReconstructor: " << api().e3d_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  int64_t n_corners = 0, n_vertices = 0, n_triangles = 0;
  api().e3d_surface_counts(surface, &n_corners, &n_vertices, &n_triangles);
  std::vector<float> vertices(3 * (size_t)n_vertices);
  std::vector<uint32_t> triangles(3 * (size_t)n_triangles);
  const int r = api().e3d_surface_get_mesh(surface, vertices.data(), nullptr, triangles.data());
  if (timings) {
    float ms[16];
    const char* names[16];
    const int groups = api().e3d_surface_kernel_ms(surface, ms, names, 16);
    for (int g = 0; g < groups && g < 16; ++g) std::cerr << "[timings] " << names[g] << " " << ms[g] << " ms" << std::endl;
  }
  api().e3d_surface_destroy(surface);
  if (r < 0) {
    std::cerr << "SurfaceReconstructor: " << api().e3d_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  std::cerr << n_corners << " lattice corners, " << n_vertices << " vertices, " << n_triangles << " triangles." << std::endl;

  if ((uint64_t)n_vertices > (uint64_t)INT32_MAX) {
    std::cerr << "SurfaceReconstructor: " << n_vertices << " vertices do not fit the PLY face list's int32 indices" << std::endl;
    return EXIT_FAILURE;
  }
  std::vector<int32_t> faces(triangles.begin(), triangles.end());
  if (savePLYMeshBinary(output_path, vertices.data(), (size_t)n_vertices, faces.data(), (size_t)n_triangles) < 0) return EXIT_FAILURE;
  std::cout << "Finished!" << std::endl;
  return EXIT_SUCCESS;
}
