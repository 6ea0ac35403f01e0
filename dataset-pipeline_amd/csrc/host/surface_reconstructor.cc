// SurfaceReconstructor -- the step the reference leaves to MeshLab / PoissonRecon ("External Surface Reconstruction" of its README):
// the merged point + normal cloud becomes the strongly subdivided triangle mesh that SplatCreator (--mesh_path), ImageRegistrator,
// GroundTruthCreator, MaskTransfer and ImageLocalizer (--occlusion_mesh_path) read.  A signed field of the oriented points is
// evaluated on a lattice of --voxel_size anchored at the world origin and one vertex per cell with a sign change is written
// (e3d_surface_reconstruct; the rules: include/e3d_hip.h).  Without --fill_holes the mesh ends where the data ends.
//
//   SurfaceReconstructor --point_normal_cloud_path cloud.ply --output_path surface.ply [--voxel_size 0.02] [--support_radius 2 x voxel_size]
//                        [--fill_holes N] [--filled_mesh_path filled.ply] [--csg_script boxes.txt] [--print_csg_script] [--timings]
//
// --fill_holes N (0 to 32, default 0): N iterations that extend the signed field next to where the surface ends, before the boxes of
// --csg_script (e3d_surface_reconstruct_filled): holes up to about 2 (N + support_radius / voxel_size) cells wide close, and at an
// outer boundary of the data the sheet grows by up to N cells.  The value is checked with the other arguments, before anything is
// loaded.  --filled_mesh_path writes the triangles the fill made (those with a filled vertex) in the same PLY layout, all vertices
// kept, for inspection.  One line reports the numbers of filled corners, vertices and triangles.
// --csg_script: what the reference's editor does by hand with its CSG tool (src/point_cloud_editor/tool_csg.cc: a box united with or
// subtracted from the surface mesh where the scanner missed glass or dark objects), as a text file that is applied again whenever the
// surface is rebuilt (e3d_surface_reconstruct_csg).  `#` starts a comment; otherwise one operation per line, applied in order:
//   union box    CX CY CZ  QW QX QY QZ  EX EY EZ
//   subtract box CX CY CZ  QW QX QY QZ  EX EY EZ
// C is the centre, E the FULL extents in metres (the editor's object_extent_), Q a unit quaternion, world from box.  A quaternion whose
// norm n = sqrt(((w w + x x) + y y) + z z) differs from 1 by more than 1e-6 is an error; otherwise (w, x, y, z) are divided by n and
//   R = | 1 - 2 (y y + z z)   2 (x y - w z)       2 (x z + w y)     |
//       | 2 (x y + w z)       1 - 2 (x x + z z)   2 (y z - w x)     |
//       | 2 (x z - w y)       2 (y z + w x)       1 - 2 (x x + y y) |
// in f64, each entry evaluated as written.  The whole file is read and checked before the cloud is loaded; every error names file:line.
// --print_csg_script prints the operations as they go to the library (%.17g).  The cloud may hold zero points.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "e3d_loader.h"
#include "io_ply.h"
#include "util.h"

using namespace e3d_host;

namespace {

bool to_double(const std::string& s, double* v) {
  if (s.empty()) return false;
  char* end = nullptr;
  *v = strtod(s.c_str(), &end);
  return end && *end == 0;
}

// one line of the script (comment removed) -> an operation, or the reason why not
bool parse_csg_line(const std::vector<std::string>& tok, e3d_surface_solid_t* op, std::string* why) {
  if (tok[0] == "union") op->kind = E3D_SURFACE_UNION;
  else if (tok[0] == "subtract") op->kind = E3D_SURFACE_SUBTRACT;
  else { *why = "unknown operation '" + tok[0] + "' (union or subtract expected)"; return false; }
  if (tok.size() < 2 || tok[1] != "box") { *why = tok[0] + ": the only solid is 'box'"; return false; }
  if (tok.size() != 12) { *why = tok[0] + " box: 10 numbers expected (CX CY CZ QW QX QY QZ EX EY EZ), " + std::to_string(tok.size() - 2) + " given"; return false; }
  double v[10];
  for (int i = 0; i < 10; ++i) {
    if (!to_double(tok[2 + i], &v[i])) { *why = tok[0] + " box: '" + tok[2 + i] + "' is not a number"; return false; }
    if (!std::isfinite(v[i])) { *why = tok[0] + " box: '" + tok[2 + i] + "' is not finite"; return false; }
  }
  double w = v[3], x = v[4], y = v[5], z = v[6];
  const double norm = std::sqrt(((w * w + x * x) + y * y) + z * z);
  if (!(std::fabs(norm - 1.0) <= 1e-6)) {
    char buf[128];
    snprintf(buf, sizeof buf, " box: the quaternion has norm %.9g, a unit quaternion is expected", norm);
    *why = tok[0] + buf;
    return false;
  }
  w /= norm; x /= norm; y /= norm; z /= norm;
  double* R = op->rotation;
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
  for (int a = 0; a < 3; ++a) {
    op->centre[a] = v[a];
    if (!(v[7 + a] > 0.0)) { *why = tok[0] + " box: the extents must be positive"; return false; }
    op->half_extent[a] = 0.5 * v[7 + a];
  }
  return true;
}

// --fill_holes: an integer in [0, 32], nothing behind it
bool parse_fill_holes(int argc, char** argv, int* n) {
  const int at = find_argument(argc, argv, "--fill_holes");
  if (at < 0) return true;
  const char* text = at + 1 < argc ? argv[at + 1] : nullptr;
  char* end = nullptr;
  const long v = text ? strtol(text, &end, 10) : 0;
  if (!text || end == text || *end != 0 || v < 0 || v > 32) {
    std::cerr << "--fill_holes: an integer from 0 to 32 is expected, " << (text ? std::string("'") + text + "' given" : std::string("no value given")) << std::endl;
    return false;
  }
  *n = (int)v;
  return true;
}

bool read_csg_script(const std::string& path, std::vector<e3d_surface_solid_t>* ops) {
  std::ifstream f(path);
  if (!f) { std::cerr << "Cannot read the script " << path << std::endl; return false; }
  std::string line;
  int line_no = 0;
  while (std::getline(f, line)) {
    ++line_no;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    std::istringstream ls(line);
    std::vector<std::string> tok;
    std::string t;
    while (ls >> t) tok.push_back(t);
    if (tok.empty()) continue;
    e3d_surface_solid_t op{};
    std::string why;
    if (ops->size() >= 256) why = "more than 256 operations";
    if (!why.empty() || !parse_csg_line(tok, &op, &why)) { std::cerr << path << ":" << line_no << ": " << why << std::endl; return false; }
    ops->push_back(op);
  }
  return true;
}

}  // namespace

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
  std::string csg_script;
  parse_argument(argc, argv, "--csg_script", csg_script);
  int fill_holes = 0;
  if (!parse_fill_holes(argc, argv, &fill_holes)) return EXIT_FAILURE;
  std::string filled_mesh_path;
  parse_argument(argc, argv, "--filled_mesh_path", filled_mesh_path);

  if (point_normal_cloud_path.empty() || output_path.empty()) {
    std::cout << "Please provide input / output paths." << std::endl;
    return EXIT_FAILURE;
  }

  std::vector<e3d_surface_solid_t> ops;
  if (!csg_script.empty() && !read_csg_script(csg_script, &ops)) return EXIT_FAILURE;
  if (find_argument(argc, argv, "--print_csg_script") > 0)
    for (const e3d_surface_solid_t& op : ops) {
      fprintf(stderr, "[csg] %s box centre", op.kind == E3D_SURFACE_UNION ? "union" : "subtract");
      for (double v : op.centre) fprintf(stderr, " %.17g", v);
      fprintf(stderr, " rotation");
      for (double v : op.rotation) fprintf(stderr, " %.17g", v);
      fprintf(stderr, " half_extent");
      for (double v : op.half_extent) fprintf(stderr, " %.17g", v);
      fprintf(stderr, "\n");
    }

  std::cerr << "Loading point cloud ..." << std::endl;
  PointCloud cloud;
  if (loadPLYFile(point_normal_cloud_path, cloud) < 0) return EXIT_FAILURE;
  if (cloud.normals.size() != cloud.xyz.size()) {
    std::cerr << "[loadPLYFile] no normals in " << point_normal_cloud_path << std::endl;
    return EXIT_FAILURE;
  }

  std::cerr << "Reconstructing the surface ..." << std::endl;
  e3d_surface_t* surface = fill_holes > 0
                               ? api().e3d_surface_reconstruct_filled(cloud.xyz.data(), cloud.normals.data(), cloud.size(), voxel_size, support_radius,
                                                                      fill_holes, ops.data(), ops.size())
                           : csg_script.empty()
                               ? api().e3d_surface_reconstruct(cloud.xyz.data(), cloud.normals.data(), cloud.size(), voxel_size, support_radius)
                               : api().e3d_surface_reconstruct_csg(cloud.xyz.data(), cloud.normals.data(), cloud.size(), voxel_size, support_radius,
                                                                   ops.data(), ops.size());
  if (!surface) {
    std::cerr << "SurfaceReconstructor: " << api().e3d_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  int64_t n_corners = 0, n_vertices = 0, n_triangles = 0;
  api().e3d_surface_counts(surface, &n_corners, &n_vertices, &n_triangles);
  std::vector<float> vertices(3 * (size_t)n_vertices);
  std::vector<uint32_t> triangles(3 * (size_t)n_triangles);
  int r = api().e3d_surface_get_mesh(surface, vertices.data(), nullptr, triangles.data());
  std::vector<uint8_t> corner_filled((size_t)n_corners), vertex_filled((size_t)n_vertices);
  if (r >= 0 && fill_holes > 0) r = api().e3d_surface_get_fill(surface, corner_filled.data(), vertex_filled.data());
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
  if (fill_holes > 0) {
    std::vector<int32_t> filled_faces;
    for (size_t t = 0; t < (size_t)n_triangles; ++t)
      if (vertex_filled[faces[3 * t]] || vertex_filled[faces[3 * t + 1]] || vertex_filled[faces[3 * t + 2]])
        filled_faces.insert(filled_faces.end(), faces.begin() + 3 * t, faces.begin() + 3 * t + 3);
    size_t fc = 0, fv = 0;
    for (uint8_t b : corner_filled) fc += b;
    for (uint8_t b : vertex_filled) fv += b;
    std::cerr << "Filled: " << fc << " lattice corners, " << fv << " vertices, " << filled_faces.size() / 3 << " triangles." << std::endl;
    if (!filled_mesh_path.empty() &&
        savePLYMeshBinary(filled_mesh_path, vertices.data(), (size_t)n_vertices, filled_faces.data(), filled_faces.size() / 3) < 0)
      return EXIT_FAILURE;
  }
  std::cout << "Finished!" << std::endl;
  return EXIT_SUCCESS;
}
