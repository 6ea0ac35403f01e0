// PointCloudEditor -- the reference's interactive editor (src/point_cloud_editor) as a batch step: the manual clean-up of a scan
// becomes an edit script that is kept next to the scan and applied again after a re-scan.  The selections run on the MI355X
// behind e3d_edit_* (lasso, beyond-plane, pick, delete, move), the outlier selection behind e3d_local_outlier_removal, and the depth
// image that the lasso needs on a mesh comes from the occlusion renderer (e3d_reg_*).
//
//   PointCloudEditor --in a.ply [--in b.ply] [--label_definitions labels.txt] --script edits.txt [--timings]
//
// Objects are numbered in --in order.  A PLY with faces is a mesh, any other a coloured cloud.  <path with the extension replaced
// by "labels"> holds one uint8 label per point (main_window.cc:319-384, 528-536) and is read if it exists and written by `save` if
// the object has labels.  The label definition file has lines `Index Name R G B`; `#` starts a comment line.
//
// The script has one operation per line; `#` starts a comment.
//   object I                         the current object (a different one than before: the selection is cleared)
//   view W H                         the window: fx = fy = H, cx = W / 2 - 0.5, cy = H / 2 - 0.5 (SetFreeOrbitViewport); default 640 480
//   depth_range NEAR FAR             default 0.1 100; FAR > NEAR > 0
//   camera pose r00 r01 ... r22 tx ty tz      camera_T_world: the rotation row by row, then the translation
//   camera look_from x y z look_at x y z      render_widget.cc:832-843 (up is +z)
//   print_view                       the 3 x 4 camera_T_world, one row per line, %.9g
//   lasso replace|add|remove x0 y0 x1 y1 ...  (fewer than 3 vertices: nothing happens, as in the GUI)
//   pick PX PY                       the point closest to the pixel goes onto the point stack
//   point X Y Z                      a given point goes onto the point stack
//   beyond_plane [visible_only]      the plane through the last three points of the stack (they are consumed)
//   select_label L | select_outliers MEAN_K FACTOR | select_none | print_selection
//   assign_label_to_cloud L | label L | delete | move | save [I [path]]
// Every message box of the GUI is an error message and a non-zero exit here.  `delete`, `label` and `move` with an empty selection do
// nothing, as the GUI's keys.  Objects loaded from a PLY have the identity global_T_object, so camera_T_object = camera_T_world.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "e3d_loader.h"
#include "io_ply.h"
#include "util.h"

using namespace e3d_host;

namespace {

struct Fail : std::runtime_error { using std::runtime_error::runtime_error; };

struct Op { int line = 0; std::string name; std::vector<std::string> args; };

struct LabelDef { bool valid = false; std::string name; int r = 0, g = 0, b = 0; };

struct Object {
  std::string path;
  std::vector<float> xyz;
  std::vector<uint8_t> rgb, labels;
  std::vector<uint32_t> faces;                  // 3 per triangle; non-empty: a mesh
  bool is_mesh = false;
  e3d_edit_t* edit = nullptr;                   // the points on the device, made when an operation first needs them
  size_t size() const { return xyz.size() / 3; }
  bool has_labels() const { return !labels.empty(); }
};

std::string labels_path_for(const std::string& p) {
  const size_t slash = p.find_last_of('/'), dot = p.find_last_of('.');
  const std::string stem = (dot == std::string::npos || (slash != std::string::npos && dot < slash)) ? p : p.substr(0, dot);
  return stem + ".labels";
}

bool to_double(const std::string& s, double* v) {
  if (s.empty()) return false;
  char* end = nullptr;
  *v = strtod(s.c_str(), &end);
  return end && *end == 0;
}
bool to_int(const std::string& s, long* v) {
  if (s.empty()) return false;
  char* end = nullptr;
  *v = strtol(s.c_str(), &end, 10);
  return end && *end == 0;
}

// ---- the script: read and checked as a whole before anything is loaded ------------------------------------------------------------
void check_numbers(const Op& op, size_t first, size_t count) {
  if (op.args.size() != first + count) throw Fail(op.name + ": " + std::to_string(first + count) + " arguments expected, " + std::to_string(op.args.size()) + " given");
  double v;
  for (size_t i = first; i < op.args.size(); ++i)
    if (!to_double(op.args[i], &v)) throw Fail(op.name + ": '" + op.args[i] + "' is not a number");
}
long check_int(const Op& op, size_t i, long lo, long hi) {
  long v;
  if (i >= op.args.size() || !to_int(op.args[i], &v)) throw Fail(op.name + ": an integer is expected");
  if (v < lo || v > hi) throw Fail(op.name + ": " + std::to_string(v) + " is out of range");
  return v;
}
double num(const Op& op, size_t i) { double v = 0; to_double(op.args[i], &v); return v; }

void check_op(const Op& op) {
  const std::string& n = op.name;
  const size_t a = op.args.size();
  if (n == "object") { if (a != 1) throw Fail("object: one argument expected"); check_int(op, 0, 0, 1 << 20); }
  else if (n == "view") { if (a != 2) throw Fail("view: W H expected"); check_int(op, 0, 1, 65535); check_int(op, 1, 1, 65535); }
  else if (n == "depth_range") {
    check_numbers(op, 0, 2);
    if (!(num(op, 1) > num(op, 0) && num(op, 0) > 0)) throw Fail("depth_range: FAR > NEAR > 0 is required");
  } else if (n == "camera") {
    if (a >= 1 && op.args[0] == "pose") check_numbers(op, 1, 12);
    else if (a >= 1 && op.args[0] == "look_from") {
      if (a != 8 || op.args[4] != "look_at") throw Fail("camera: look_from x y z look_at x y z expected");
      double v;
      for (size_t i : {1, 2, 3, 5, 6, 7}) if (!to_double(op.args[i], &v)) throw Fail("camera: '" + op.args[i] + "' is not a number");
    } else throw Fail("camera: pose or look_from expected");
  } else if (n == "print_view" || n == "select_none" || n == "print_selection" || n == "delete" || n == "move") {
    if (a) throw Fail(n + ": no arguments expected");
  } else if (n == "lasso") {
    if (a < 1 || (op.args[0] != "replace" && op.args[0] != "add" && op.args[0] != "remove")) throw Fail("lasso: replace, add or remove expected");
    if ((a - 1) % 2) throw Fail("lasso: an odd number of coordinates");
    check_numbers(op, 1, a - 1);
  } else if (n == "pick") check_numbers(op, 0, 2);
  else if (n == "point") check_numbers(op, 0, 3);
  else if (n == "beyond_plane") { if (a > 1 || (a == 1 && op.args[0] != "visible_only")) throw Fail("beyond_plane: only visible_only may follow"); }
  else if (n == "select_label" || n == "assign_label_to_cloud" || n == "label") { if (a != 1) throw Fail(n + ": one label index expected"); check_int(op, 0, 0, 255); }
  else if (n == "select_outliers") { check_numbers(op, 0, 2); check_int(op, 0, 1, 1023); }
  else if (n == "save") { if (a > 2) throw Fail("save: at most an object index and a path"); if (a) check_int(op, 0, 0, 1 << 20); }
  else throw Fail("unknown operation '" + n + "'");
}

bool read_script(const std::string& path, std::vector<Op>* ops) {
  std::ifstream f(path);
  if (!f) { std::cerr << "Cannot read the script " << path << std::endl; return false; }
  std::string line;
  int line_no = 0;
  while (std::getline(f, line)) {
    ++line_no;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    std::istringstream ls(line);
    Op op;
    op.line = line_no;
    if (!(ls >> op.name)) continue;
    std::string tok;
    while (ls >> tok) op.args.push_back(tok);
    try { check_op(op); }
    catch (const Fail& e) { std::cerr << path << ":" << line_no << ": " << e.what() << std::endl; return false; }
    ops->push_back(op);
  }
  return true;
}

// MainWindow::LoadLabelFileClicked (main_window.cc:730-813)
bool read_label_definitions(const std::string& path, std::vector<LabelDef>* defs) {
  std::ifstream f(path);
  if (!f) { std::cerr << "Cannot read file: " << path << std::endl; return false; }
  std::string line;
  while (std::getline(f, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    std::istringstream ls(line);
    int index = -1, r = -1, g = -1, b = -1;
    std::string name;
    if (!(ls >> index >> name >> r >> g >> b)) { std::cerr << "Cannot parse the label definition: " << line << std::endl; return false; }
    if (index < 0 || index > 255 || r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255) {
      std::cerr << "Label indices and colors must be from 0 to 255." << std::endl; return false;
    }
    if ((int)defs->size() < index + 1) defs->resize(index + 1);
    LabelDef& d = (*defs)[index];
    if (d.valid) { std::cerr << "Label indices must be unique. Found two with index: " << index << std::endl; return false; }
    d.valid = true; d.name = name; d.r = r; d.g = g; d.b = b;
  }
  return true;
}

bool ply_has_faces(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::string line;
  while (std::getline(f, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::istringstream ls(line);
    std::string tok, name;
    size_t count = 0;
    ls >> tok;
    if (tok == "element" && (ls >> name >> count) && name == "face") return count > 0;
    if (tok == "end_header") break;
  }
  return false;
}

// MainWindow::ReadObjectFile (main_window.cc:322-388)
bool read_object(const std::string& path, const std::vector<LabelDef>& defs, Object* o) {
  o->path = path;
  o->is_mesh = ply_has_faces(path);
  if (o->is_mesh) {
    if (loadPLYMesh(path, o->xyz, o->faces) < 0) { std::cerr << "Cannot read file: " << path << std::endl; return false; }
    for (uint32_t v : o->faces)
      if (v >= o->size()) { std::cerr << "A face of " << path << " names vertex " << v << " of " << o->size() << std::endl; return false; }
  } else {
    PointCloud cloud;
    if (loadPLYFile(path, cloud, /*want_rgb=*/true) < 0) { std::cerr << "Cannot read file: " << path << std::endl; return false; }
    o->xyz.swap(cloud.xyz); o->rgb.swap(cloud.rgb);
  }
  if (o->size() >= ((size_t)1 << 32)) { std::cerr << path << ": 2^32 points or more" << std::endl; return false; }
  const std::string lp = labels_path_for(path);
  FILE* lf = fopen(lp.c_str(), "rb");
  if (lf) {
    o->labels.resize(o->size() + 1);                              // one more: a longer file is inconsistent too
    const size_t got = fread(o->labels.data(), 1, o->labels.size(), lf);
    fclose(lf);
    if (got != o->size()) {
      std::cerr << "Number of labels is inconsistent with the number of points for: " << path << std::endl; return false;
    }
    o->labels.resize(o->size());
    for (uint8_t l : o->labels)
      if (defs.size() <= l || !defs[l].valid) {
        std::cerr << "The following file has a label (index " << (int)l << ") for which there is no definition: " << path << std::endl; return false;
      }
  }
  return true;
}

bool save_object(const Object& o, const std::string& path) {
  const int r = o.is_mesh ? savePLYMeshBinary(path, o.xyz.data(), o.size(), reinterpret_cast<const int32_t*>(o.faces.data()), o.faces.size() / 3)
                          : savePLYFileBinaryXYZRGB(path, o.xyz, o.rgb);
  if (r < 0) { std::cerr << "Cannot write " << path << std::endl; return false; }
  if (o.has_labels()) {
    const std::string lp = labels_path_for(path);
    FILE* lf = fopen(lp.c_str(), "wb");
    if (!lf) { std::cerr << "Cannot write " << lp << std::endl; return false; }
    const size_t put = fwrite(o.labels.data(), 1, o.labels.size(), lf);
    if (fclose(lf) != 0 || put != o.labels.size()) { std::cerr << "Cannot write " << lp << std::endl; return false; }
  }
  return true;
}

// ---- the session ------------------------------------------------------------------------------------------------------------------
struct Session {
  std::vector<Object> objects;
  std::vector<LabelDef> defs;
  bool timings = false;
  int current = 0;
  int width = 640, height = 480;
  float min_depth = 0.1f, max_depth = 100.f;
  float camera_T_world[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  std::vector<float> stack;                     // picked and given points, 3 floats each
  // the selection belongs to `current`; it lives on the host, on the device (in the object's edit handle), or on both
  std::vector<uint8_t> sel;
  bool sel_on_host = true, sel_on_device = false;
  int64_t sel_count = 0;

  ~Session() { for (Object& o : objects) if (o.edit) api().e3d_edit_destroy(o.edit); }

  Object& cur() { return objects[current]; }
  void lib_fail(const char* what) { throw Fail(std::string(what) + " failed: " + api().e3d_last_error()); }

  e3d_view view() const {
    e3d_view v;
    v.width = width; v.height = height;
    v.fx = (float)height; v.fy = (float)height;
    v.cx = (float)(0.5 * width - 0.5f); v.cy = (float)(0.5 * height - 0.5f);
    memcpy(v.camera_T_object, camera_T_world, sizeof v.camera_T_object);
    v.min_depth = min_depth; v.max_depth = max_depth;
    return v;
  }

  void report(const char* what, e3d_edit_t* h) {
    if (!timings) return;
    float ms = 0;
    api().e3d_edit_kernel_ms(h, &ms);
    printf("timing %s %.4f ms\n", what, ms);
  }

  e3d_edit_t* handle() {
    Object& o = cur();
    if (!o.edit) {
      o.edit = api().e3d_edit_create(o.xyz.data(), o.size());
      if (!o.edit) lib_fail("e3d_edit_create");
      sel_on_device = false;
    }
    return o.edit;
  }
  void drop_handle(Object& o) { if (o.edit) { api().e3d_edit_destroy(o.edit); o.edit = nullptr; } }

  void select_none() { sel.assign(cur().size(), 0); sel_on_host = true; sel_on_device = false; sel_count = 0; }
  void set_host_selection(std::vector<uint8_t>&& flags) {
    sel = std::move(flags);
    sel_count = 0;
    for (uint8_t f : sel) sel_count += f != 0;
    sel_on_host = true; sel_on_device = false;
  }
  void selection_to_host() {
    if (sel_on_host) return;
    sel.resize(cur().size());
    if (api().e3d_edit_get_selection(handle(), sel.data()) < 0) lib_fail("e3d_edit_get_selection");
    sel_on_host = true;
  }
  void selection_to_device() {
    e3d_edit_t* h = handle();
    if (sel_on_device) return;
    sel.resize(cur().size());
    if (api().e3d_edit_set_selection(h, sel.data()) < 0) lib_fail("e3d_edit_set_selection");
    sel_on_device = true;
  }
  void device_selected(int64_t count) { sel_count = count; sel_on_device = true; sel_on_host = false; }

  // the mesh's depth from the view, by the occlusion renderer; "no depth" (0) becomes +inf
  std::vector<float> render_mesh_depth() {
    const Object& o = cur();
    e3d_reg_params prm;
    memset(&prm, 0, sizeof prm);
    prm.point_neighbor_count = 5; prm.robust_weighting_type = 1; prm.robust_weighting_parameter = 1.f;
    prm.fixed_residuals_weight = 1.f; prm.variable_residuals_weight = 1.f; prm.maximum_valid_intensity = 252.f;
    prm.occlusion_depth_threshold = 0.01f; prm.splat_radius = 0.03f; prm.current_image_scale = 0; prm.image_scale_count = 1;
    prm.depth_residuals_weight = 0.f; prm.depth_robust_weighting_type = 2; prm.depth_robust_weighting_parameter = 0.02f;
    e3d_reg_t* reg = api().e3d_reg_create(&prm);
    if (!reg) lib_fail("e3d_reg_create");
    struct Guard { e3d_reg_t* r; ~Guard() { api().e3d_reg_destroy(r); } } guard{reg};
    const e3d_view v = view();
    const float intr[4] = {v.fx, v.fy, v.cx, v.cy};
    if (api().e3d_reg_set_intrinsics(reg, 0, E3D_CAMERA_PINHOLE, width, height, intr, 4, 0, 1) < 0) lib_fail("e3d_reg_set_intrinsics");
    const std::vector<uint8_t> pixels((size_t)width * height, 0);
    const uint8_t* levels[1] = {pixels.data()};
    if (api().e3d_reg_set_image(reg, 0, 0, levels, nullptr) < 0) lib_fail("e3d_reg_set_image");
    float q[4], t[3] = {camera_T_world[3], camera_T_world[7], camera_T_world[11]};
    rotation_to_quaternion(q);
    if (api().e3d_reg_set_image_pose(reg, 0, q, t) < 0) lib_fail("e3d_reg_set_image_pose");
    if (api().e3d_reg_add_occlusion_mesh(reg, o.xyz.data(), o.size(), o.faces.data(), o.faces.size() / 3, 0) < 0) lib_fail("e3d_reg_add_occlusion_mesh");
    if (api().e3d_reg_set_occlusion_options(reg, min_depth, max_depth, 0) < 0) lib_fail("e3d_reg_set_occlusion_options");
    std::vector<float> depth((size_t)width * height);
    if (api().e3d_reg_render_depth(reg, 0, 0, depth.data()) < 0) lib_fail("e3d_reg_render_depth");
    for (float& d : depth) if (d == 0.f) d = INFINITY;
    return depth;
  }

  // Eigen's matrix -> quaternion conversion (w x y z) of camera_T_world's rotation
  void rotation_to_quaternion(float* q) const {
    double m[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m[3 * r + c] = camera_T_world[4 * r + c];
    double tr = m[0] + m[4] + m[8], w, v[3];
    if (tr > 0) {
      tr = std::sqrt(tr + 1.0); w = 0.5 * tr; tr = 0.5 / tr;
      v[0] = (m[7] - m[5]) * tr; v[1] = (m[2] - m[6]) * tr; v[2] = (m[3] - m[1]) * tr;
    } else {
      int i = 0;
      if (m[4] > m[0]) i = 1;
      if (m[8] > m[4 * i]) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      tr = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
      v[i] = 0.5 * tr; tr = 0.5 / tr;
      w = (m[3 * k + j] - m[3 * j + k]) * tr;
      v[j] = (m[3 * j + i] + m[3 * i + j]) * tr;
      v[k] = (m[3 * k + i] + m[3 * i + k]) * tr;
    }
    const double nrm = std::sqrt(w * w + v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    q[0] = (float)(w / nrm); q[1] = (float)(v[0] / nrm); q[2] = (float)(v[1] / nrm); q[3] = (float)(v[2] / nrm);
  }

  void set_camera_pose(const double* rt) {          // 9 rotation values row by row, then the translation
    for (int r = 0; r < 3; ++r) {
      double dot_self = 0;
      for (int c = 0; c < 3; ++c) dot_self += rt[3 * r + c] * rt[3 * r + c];
      const int r2 = (r + 1) % 3;
      double dot_next = 0;
      for (int c = 0; c < 3; ++c) dot_next += rt[3 * r + c] * rt[3 * r2 + c];
      if (std::fabs(dot_self - 1.0) > 1e-4 || std::fabs(dot_next) > 1e-4) throw Fail("camera pose: the 3 x 3 block is not a rotation");
    }
    const double det = rt[0] * (rt[4] * rt[8] - rt[5] * rt[7]) - rt[1] * (rt[3] * rt[8] - rt[5] * rt[6]) + rt[2] * (rt[3] * rt[7] - rt[4] * rt[6]);
    if (det < 0) throw Fail("camera pose: the 3 x 3 block is a reflection");
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) camera_T_world[4 * r + c] = (float)rt[3 * r + c];
      camera_T_world[4 * r + 3] = (float)rt[9 + r];
    }
  }

  // render_widget.cc:832-843 in f32: world_R_camera = [right, -up, forward], world_T_camera = (world_R_camera, look_from), inverted
  void set_camera_look_at(const float from[3], const float at[3]) {
    auto normalize = [](float* a) {
      const float n = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
      if (!(n > 0.f)) return false;
      for (int i = 0; i < 3; ++i) a[i] = a[i] / n;
      return true;
    };
    float forward[3] = {at[0] - from[0], at[1] - from[1], at[2] - from[2]};
    if (!normalize(forward)) throw Fail("camera look_from: look_from and look_at are the same point");
    float right[3] = {forward[1] * 1.f - forward[2] * 0.f, forward[2] * 0.f - forward[0] * 1.f, forward[0] * 0.f - forward[1] * 0.f};
    if (!(std::sqrt(right[0] * right[0] + right[1] * right[1]) > 1e-6f) || !normalize(right)) throw Fail("camera look_from: the viewing direction is parallel to z");
    const float up[3] = {right[1] * forward[2] - right[2] * forward[1], right[2] * forward[0] - right[0] * forward[2], right[0] * forward[1] - right[1] * forward[0]};
    // camera_R_world = world_R_camera^T: its rows are the camera axes
    const float rows[3][3] = {{right[0], right[1], right[2]}, {-up[0], -up[1], -up[2]}, {forward[0], forward[1], forward[2]}};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) camera_T_world[4 * r + c] = rows[r][c];
      camera_T_world[4 * r + 3] = -((rows[r][0] * from[0] + rows[r][1] * from[1]) + rows[r][2] * from[2]);
    }
  }

  // camera_T_world.inverse().translation() = -R^T t
  void camera_position(float c[3]) const {
    const float* T = camera_T_world;
    for (int i = 0; i < 3; ++i) c[i] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
  }

  void check_label_defined(long l) const {
    if ((long)defs.size() <= l || !defs[l].valid) throw Fail("label " + std::to_string(l) + " has no definition (--label_definitions)");
  }

  // the points with flag 0 stay, in order: colours, labels and faces on the host with the flags, coordinates on the device
  void remove_selected_points(Object& o) {
    const size_t n = o.size();
    std::vector<uint32_t> remap;
    if (o.is_mesh) remap.assign(n, 0);
    size_t out = 0;
    for (size_t i = 0; i < n; ++i) {
      if (sel[i]) continue;
      if (!o.rgb.empty()) for (int c = 0; c < 3; ++c) o.rgb[3 * out + c] = o.rgb[3 * i + c];
      if (o.has_labels()) o.labels[out] = o.labels[i];
      if (o.is_mesh) remap[i] = (uint32_t)out;
      ++out;
    }
    if (!o.rgb.empty()) o.rgb.resize(3 * out);
    if (o.has_labels()) o.labels.resize(out);
    if (o.is_mesh) {
      size_t fo = 0;
      for (size_t f = 0; f + 2 < o.faces.size(); f += 3) {
        const uint32_t a = o.faces[f], b = o.faces[f + 1], c = o.faces[f + 2];
        if (sel[a] || sel[b] || sel[c]) continue;
        o.faces[fo] = remap[a]; o.faces[fo + 1] = remap[b]; o.faces[fo + 2] = remap[c];
        fo += 3;
      }
      o.faces.resize(fo);
    }
    const int64_t kept = api().e3d_edit_delete_selected(o.edit);
    if (kept < 0) lib_fail("e3d_edit_delete_selected");
    report("delete", o.edit);
    if ((size_t)kept != out) throw Fail("delete: the device kept " + std::to_string(kept) + " points, the flags say " + std::to_string(out));
    o.xyz.resize(3 * out);
    if (api().e3d_edit_get_points(o.edit, o.xyz.data()) < 0) lib_fail("e3d_edit_get_points");
  }

  void run(const Op& op) {
    const std::string& n = op.name;
    if (n == "object") {
      const long i = check_int(op, 0, 0, (long)objects.size() - 1);
      if (i != current) { current = (int)i; select_none(); }
    } else if (n == "view") {
      width = (int)check_int(op, 0, 1, 65535); height = (int)check_int(op, 1, 1, 65535);
    } else if (n == "depth_range") {
      min_depth = (float)num(op, 0); max_depth = (float)num(op, 1);
    } else if (n == "camera") {
      if (op.args[0] == "pose") {
        double rt[12];
        for (int i = 0; i < 12; ++i) rt[i] = num(op, 1 + i);
        set_camera_pose(rt);
      } else {
        const float from[3] = {(float)num(op, 1), (float)num(op, 2), (float)num(op, 3)}, at[3] = {(float)num(op, 5), (float)num(op, 6), (float)num(op, 7)};
        set_camera_look_at(from, at);
      }
    } else if (n == "print_view") {
      for (int r = 0; r < 3; ++r) printf("%.9g %.9g %.9g %.9g\n", camera_T_world[4 * r], camera_T_world[4 * r + 1], camera_T_world[4 * r + 2], camera_T_world[4 * r + 3]);
    } else if (n == "lasso") {
      const int mode = op.args[0] == "replace" ? E3D_EDIT_REPLACE : (op.args[0] == "add" ? E3D_EDIT_ADD : E3D_EDIT_REMOVE);
      std::vector<double> poly;
      for (size_t i = 1; i < op.args.size(); ++i) poly.push_back(num(op, i));
      if (mode == E3D_EDIT_REPLACE && poly.size() >= 6) handle(); else selection_to_device();
      std::vector<float> depth;
      if (cur().is_mesh && poly.size() >= 6) depth = render_mesh_depth();
      const e3d_view v = view();
      const int64_t c = api().e3d_edit_lasso(handle(), &v, poly.data(), (int)(poly.size() / 2), mode, depth.empty() ? nullptr : depth.data());
      if (c < 0) lib_fail("e3d_edit_lasso");
      if (poly.size() >= 6) { device_selected(c); report("lasso", handle()); }
    } else if (n == "pick") {
      const e3d_view v = view();
      const double click[2] = {num(op, 0), num(op, 1)};
      int64_t index = -1;
      float distance = 0;
      if (api().e3d_edit_pick(handle(), &v, click, 1, &index, &distance) < 0) lib_fail("e3d_edit_pick");
      report("pick", handle());
      if (index < 0) throw Fail("pick: no point of the object is in the depth range");
      for (int c = 0; c < 3; ++c) stack.push_back(cur().xyz[3 * (size_t)index + c]);
      printf("picked point %lld (%.9g %.9g %.9g) at squared pixel distance %.9g\n", (long long)index, cur().xyz[3 * (size_t)index],
             cur().xyz[3 * (size_t)index + 1], cur().xyz[3 * (size_t)index + 2], distance);
    } else if (n == "point") {
      for (int c = 0; c < 3; ++c) stack.push_back((float)num(op, c));
    } else if (n == "beyond_plane") {
      if (stack.size() < 9) throw Fail("beyond_plane: three points are needed (pick, point)");
      float pts[9], c[3];
      memcpy(pts, stack.data() + stack.size() - 9, sizeof pts);
      stack.resize(stack.size() - 9);
      camera_position(c);
      const e3d_view v = view();
      const int64_t count = api().e3d_edit_beyond_plane(handle(), &v, pts, c, op.args.empty() ? 0 : 1);
      if (count < 0) lib_fail("e3d_edit_beyond_plane");
      device_selected(count);
      report("beyond_plane", handle());
    } else if (n == "select_label") {
      const long l = check_int(op, 0, 0, 255);
      check_label_defined(l);
      Object& o = cur();
      std::vector<uint8_t> flags(o.size(), 0);
      if (o.has_labels()) for (size_t i = 0; i < o.size(); ++i) flags[i] = o.labels[i] == (uint8_t)l;
      set_host_selection(std::move(flags));
    } else if (n == "select_outliers") {
      Object& o = cur();
      std::vector<uint8_t> inlier(o.size(), 1);
      if (api().e3d_local_outlier_removal(o.xyz.data(), o.size(), (int)check_int(op, 0, 1, 1023), num(op, 1), 0, inlier.data(), nullptr) < 0)
        lib_fail("e3d_local_outlier_removal");
      for (uint8_t& f : inlier) f = !f;
      set_host_selection(std::move(inlier));
    } else if (n == "select_none") {
      select_none();
    } else if (n == "print_selection") {
      printf("selection: %lld of %zu points of object %d\n", (long long)sel_count, cur().size(), current);
    } else if (n == "assign_label_to_cloud") {
      const long l = check_int(op, 0, 0, 255);
      check_label_defined(l);
      cur().labels.assign(cur().size(), (uint8_t)l);
    } else if (n == "label") {
      const long l = check_int(op, 0, 0, 255);
      if (sel_count == 0) return;
      if (!cur().has_labels()) throw Fail("The selected object does not have labels yet. Please assign an initial label to the object first.");
      check_label_defined(l);
      selection_to_host();
      for (size_t i = 0; i < cur().size(); ++i) if (sel[i]) cur().labels[i] = (uint8_t)l;
      select_none();
    } else if (n == "delete") {
      if (sel_count == 0) return;
      selection_to_host();
      selection_to_device();
      remove_selected_points(cur());
      select_none();
      sel_on_device = true;                                        // delete_selected cleared it there too
    } else if (n == "move") {
      if (sel_count == 0) return;
      if (objects.size() != 2) throw Fail("Moving points is currently only implemented for the case of exactly 2 objects (target object selection is missing).");
      Object& src = cur();
      Object& dst = objects[1 - current];
      if (src.has_labels() || dst.has_labels()) throw Fail("Moving points is currently not implemented for objects with labels.");
      if (src.is_mesh || dst.is_mesh) throw Fail("Moving points is currently not implemented for meshes.");
      selection_to_host();
      selection_to_device();
      const size_t m = (size_t)sel_count, at = dst.size();
      dst.xyz.resize(3 * (at + m));
      const int64_t got = api().e3d_edit_extract_selected(src.edit, dst.xyz.data() + 3 * at, m);
      if (got < 0) lib_fail("e3d_edit_extract_selected");
      report("move (extract)", src.edit);
      if ((size_t)got != m) throw Fail("move: the device and the host disagree about the selection");
      dst.rgb.resize(3 * at, 0);
      for (size_t i = 0; i < src.size(); ++i)
        if (sel[i]) for (int c = 0; c < 3; ++c) dst.rgb.push_back(src.rgb.empty() ? 0 : src.rgb[3 * i + c]);
      drop_handle(dst);                                            // its points changed: uploaded again when next needed
      remove_selected_points(src);
      select_none();
      sel_on_device = true;
    } else if (n == "save") {
      const long i = op.args.empty() ? current : check_int(op, 0, 0, (long)objects.size() - 1);
      if (!save_object(objects[i], op.args.size() == 2 ? op.args[1] : objects[i].path)) throw Fail("save failed");
    }
  }
};

int run_tool(int argc, char** argv) {
  std::string script_path, label_definitions_path;
  std::vector<std::string> inputs;
  for (int i = 1; i + 1 < argc; ++i)
    if (strcmp(argv[i], "--in") == 0) inputs.push_back(argv[++i]);
  parse_argument(argc, argv, "--script", script_path);
  parse_argument(argc, argv, "--label_definitions", label_definitions_path);
  if (inputs.empty() || script_path.empty()) {
    std::cerr << "Usage: " << argv[0] << " --in a.ply [--in b.ply] [--label_definitions labels.txt] --script edits.txt [--timings]" << std::endl;
    return EXIT_FAILURE;
  }
  std::vector<Op> ops;
  if (!read_script(script_path, &ops)) return EXIT_FAILURE;

  Session session;
  session.timings = find_argument(argc, argv, "--timings") > 0;
  if (!label_definitions_path.empty() && !read_label_definitions(label_definitions_path, &session.defs)) return EXIT_FAILURE;
  session.objects.resize(inputs.size());
  for (size_t i = 0; i < inputs.size(); ++i)
    if (!read_object(inputs[i], session.defs, &session.objects[i])) return EXIT_FAILURE;
  session.select_none();

  for (const Op& op : ops) {
    try { session.run(op); }
    catch (const Fail& e) { std::cerr << script_path << ":" << op.line << ": " << e.what() << std::endl; return EXIT_FAILURE; }
  }
  return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char** argv) { return run_main("PointCloudEditor", run_tool, argc, argv); }
