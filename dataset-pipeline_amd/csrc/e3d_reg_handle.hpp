// e3d_reg_handle.hpp -- the registration handle (struct e3d_reg) and the small host helpers every source that works on it uses:
// e3d_reg.hip (the optimiser), e3d_reg_depth.hip (the occlusion-depth renderer) and e3d_reg_scan.hip (the scan-side tools).
#pragma once

#include <chrono>
#include <map>
#include <memory>
#include <string>

#include "../../include/e3d_hip.h"
#include "e3d_comm.hpp"
#include "e3d_math.hpp"
#include "e3d_reg_device.hpp"

namespace e3d {

struct PointScale {
  size_t n = 0;
  float radius = 0;
  DevBuf<float4> pts;
  DevBuf<unsigned> nbr;
  DevBuf<float> fixed_desc, var_desc;
  DevBuf<int> obs_counts, row_of_point;
  bool has_fixed = false;
};
struct Intrin {
  int type = 0, min_image_scale = 0, n_params = 4;
  int width = 0, height = 0;
  float params[12] = {0};
  std::vector<CamLevel> levels;
  std::shared_ptr<std::vector<DevBuf<unsigned char>>> cam_mask;     // per level (empty buffer = none); survives parameter updates
};
struct Obs {
  bool active = false;            // false: the reference would hold no vector for this (image, scale); buffers are kept for reuse
  size_t n = 0;
  DevBuf<unsigned> idx;
  DevBuf<float> x, y, s;
  DevBuf<unsigned char> flags;
  DevBuf<int> nrow;               // K per observation: observation row of each neighbour point (-1: not observed), for pass 2
  DevBuf<float4> rows;
  bool rows_valid = false;
  DevBuf<float4> drows;           // depth residual rows (k_reg_depth_rows), recomputed per use
  // the interpolated image intensity of every observation (k_reg_intensity): a function of (x, y, s) and the image alone, so the
  // colour update and the cost that follows it at the same observations sample the pyramid once
  DevBuf<float> inten;
  bool inten_valid = false;
  int inten_w = 0, inten_h = 0, inten_min_scale = -1, inten_levels = 0;      // (the pyramid geometry they were sampled with)
  // flags / nrow describe the list `flags_src` (device pointer of an indexed re-projection's candidates) of flags_count entries:
  // a trial state of Apply that keeps every point of the visibility list visible reuses them (finish_observations skipped)
  const void* flags_src = nullptr;
  size_t flags_count = 0;
};
struct ImageDev {
  int intrinsics_id = -1;
  std::vector<DevBuf<unsigned char>> pix, mask;
  std::vector<bool> has_mask;
  Pose pose{};                    // so3().matrix() + translation of image_T_global, as the kernels read it
  SE3f pose_q;                    // image_T_global (Sophus::SE3f state)
  DevBuf<float> depth;            // last rendered occlusion depth (as float bits)
  int depth_scale = -1;
  std::vector<DevBuf<float>> depth_maps;   // Problem::depth_maps_ (fixed depth maps, one per pyramid level); empty = none
  std::map<int, Obs> obs;         // per point scale
  std::map<int, DevBuf<unsigned>> vis;   // per point scale: visibility list of the running Apply (grow-only scratch)
  // ObservationsCache::image_id_to_visibility_lists_ (observations_cache.h): per point scale, the observed point indices
  std::map<int, std::pair<DevBuf<unsigned>, size_t>> observed;
  bool has_observed = false;
  // rig membership (opt::RigImages): camera_index 0 = the frame's reference image, whose pose is the rig pose
  int rig_id = -1, camera_index = 0, ref_image_id = -1;
  bool dependent() const { return rig_id >= 0 && camera_index > 0; }
};
struct MeshEdge { unsigned v1, v2, f1, f2; int opposite; };       // f2 == 0xFFFFFFFF: boundary edge (one face)
// one occlusion mesh (OcclusionGeometry::AddMesh): vertices in the global frame, triangles, and -- if requested -- the
// silhouette-candidate edges with the normals of their two outermost faces
struct MeshDev {
  size_t n_vertices = 0, n_triangles = 0, n_edges = 0;
  DevBuf<float4> vertices, normals;
  DevBuf<unsigned> triangles;
  DevBuf<MeshEdge> edges;
};
struct RigState { std::vector<SE3f> image_T_rig; };                 // opt::Rig (rig.h:41-76)
struct RigFrame { int rig_id; std::vector<int> image_ids; };        // opt::RigImages

inline void set_pose(ImageDev& im, const SE3f& T) {
  im.pose_q = T;
  quat_to_matrix<float>(T.q.w, T.q.x, T.q.y, T.q.z, im.pose.R);
  for (int i = 0; i < 3; ++i) im.pose.t[i] = T.t[i];
}

// The occlusion geometry and the scratch of its renderer (e3d_reg_depth.hip)
struct DepthRenderer {
  DevBuf<float4> splat;
  size_t n_splat = 0;
  std::vector<std::unique_ptr<MeshDev>> meshes;
  DevBuf<float4> mesh_projected;          // per mesh vertex: pixel position and camera-space z
  DevBuf<float2> mesh_shaded;             // ... and the vertex shader output (x', y') the near-plane clipping interpolates
  DevBuf<float> depth_unmasked, ztmp_f;
  float min_occlusion_depth = 0.05f, max_occlusion_depth = 100.f;     // opt::Parameters defaults (parameters.h:60-61)
  bool mask_occlusion_boundaries = true;
  // splat depth: per-point rectangles, (tile, point) pairs (double-buffered for the sort), tile ranges
  DevBuf<uint4> rects;
  DevBuf<unsigned> sp_keys[2], sp_vals[2], sp_counter, tile_start, tile_end, zbuf, ztmp;
  DevBuf<char> sort_temp;
};

// The evaluation scans and the state of the tools that ask one image about them (e3d_reg_scan.hip)
struct ScanTools {
  DevBuf<float4> scan_pts;                // f4: evaluation scan points + their observation counts
  DevBuf<int> scan_counts;
  DevBuf<unsigned char> eval_mask;
  DevBuf<unsigned> gt_depth;
  size_t n_scan = 0;
  bool scan_points_set = false;
  // debug point clouds (e3d_reg_scan_colors_*): per scan point {r, g, b sums (f32), count (int bits)}, the colour image being sampled
  DevBuf<float4> scan_color_acc;
  DevBuf<unsigned char> scan_color_image, scan_color_rgb;
  bool scan_colors_begun = false;
  // mask transfer (e3d_reg_mask_transfer_*): the label every scan point carries from the last source call (kept between target calls),
  // the masks of the running call, {labelled points | the four counters of k_mask_fill, bad source values}
  DevBuf<unsigned char> mask_labels, mask_in, mask_result;
  DevBuf<unsigned long long> mask_counters;
  bool mask_labels_ready = false;
  int mask_transfer_eval_obs = 0;
  // ImageLocalizer (e3d_reg_pick_scan_points, _image_bearings, _project_points): {visible points | one key per click | {pxy, d} per
  // click as floats}, the clicks, and the staging of the two per-position calls
  DevBuf<unsigned long long> pick_words;
  DevBuf<float2> pick_clicks;
  DevBuf<float> localize_in, localize_out;
  DevBuf<unsigned char> localize_state;
  // ImageUndistorter (e3d_reg_undistort_plan, e3d_reg_undistort): the border samples and their normalized coordinates, the staging of
  // one source image, its resampled copy and the validity map; HIP-event time of the last resampling kernel
  DevBuf<float2> undistort_border;
  DevBuf<unsigned char> undistort_src, undistort_dst, undistort_valid;
  std::unique_ptr<EventTimer> t_undistort;
  float undistort_ms = 0.f;
  // StereoPairCreator: e3d_reg_stereo_rectify stages through the undistorter's buffers and has a timer of its own;
  // e3d_reg_stereo_ground_truth keeps the depth of the nearest point seen by both images, the disparity and the mask
  std::unique_ptr<EventTimer> t_stereo;
  float stereo_ms = 0.f;
  DevBuf<unsigned> stereo_d2;
  DevBuf<float> stereo_disparity;
  DevBuf<unsigned char> stereo_nocc;
};

}  // namespace e3d

using namespace e3d;

struct e3d_reg {
  int device = 0;
  hipStream_t stream = nullptr;
  e3d_reg_params prm{};
  std::map<int, PointScale> scales;
  std::map<int, Intrin> intr;
  std::map<int, ImageDev> images;
  std::map<int, RigState> rigs;
  std::vector<RigFrame> frames;
  DepthRenderer renderer;
  ScanTools scan;
  bool cache_observations = false;        // Optimizer::cache_observations_ (optimizer.h)
  bool rig_depth_residuals = false;       // e3d_reg_set_rig_depth_residuals: depth residuals of the non-reference rig images
  // scratch
  DevBuf<int> valid;
  DevBuf<float> tx, ty, ts;
  DevBuf<unsigned> cand, block_counts, block_offsets;
  PinBuf<unsigned char> mailbox;     // read_back
  DevBuf<double> block_d2, chunk_d2, d_total_d2, partial, red, red_all, acc_all;
  DevBuf<unsigned long long> chunk_sum, d_total;
  DevBuf<float> dummy_d2;
  DevBuf<unsigned> cut;
  // multi-GPU: image id mod world == rank -> owned
  int rank = 0, world = 1;
  e3d_allreduce_fn allreduce = nullptr;
  e3d_allreduce_device_fn allreduce_dev = nullptr;
  void* ar_user = nullptr;
  e3d_comm* comm = nullptr;                     // native RCCL collectives (e3d_reg_set_comm); not owned
  // HIP-event times of the two kernels of e3d_reg_accumulate, summed since the last e3d_reg_kernel_times(reset)
  std::unique_ptr<EventTimer> t_pass1, t_pass2;
  double pass1_ms = 0, pass2_ms = 0, pass_observations = 0, pass_calls = 0;
  DevBuf<double> comm_stage;
  // e3d_reg_profile: wall-clock time per phase of RunOnCurrentScale (the stream is synchronised at every phase boundary while
  // the profile is on, so a profiled run is slower than a plain one; the split is what it is for)
  bool profile_on = false;
  std::map<std::string, double> profile_ms;
  // ... and, while the profile is on, HIP-event time, launches and work units (points / observations / pixels: what the bench
  // prices a group's algorithmic bytes with) of every kernel group of an iteration (KT below); read lazily, no synchronisation
  struct KGroup { double ms = 0, units = 0; long long calls = 0; };
  std::map<std::string, KGroup> kgroups;
  struct KPending { hipEvent_t a, b; KGroup* g; };
  std::vector<KPending> kpending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> kfree;
  void kflush() {
    for (KPending& p : kpending) {
      float t = 0.f;
      if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) p.g->ms += (double)t;
      kfree.emplace_back(p.a, p.b);
    }
    kpending.clear();
  }
  bool owns(int image_id) const { return world <= 1 || ((image_id % world) + world) % world == rank; }
  ~e3d_reg() {
    kflush();
    for (auto& e : kfree) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace e3d {

// The environment switches of the registration host code, parsed once at first use (INTEGRATION.md lists them)
struct RegSwitches {
  bool pinned = env_default_on("E3D_REG_PINNED");              // 0: read_back through pageable memory (as rounds 1 - 5, for A / B timing)
  bool splat_order = env_default_on("E3D_REG_SPLAT_ORDER");    // 0: the splat points keep the caller's order (e3d_reg_set_splat_points)
  bool separable_min_filter = false;                           // E3D_REG_MIN_FILTER=separable: the splat depth's minimum filter in two launches
  int pass2_blocks = 1024;                                     // E3D_REG_PASS2_BLOCKS: the most workgroups of a pass-2 launch (below)
  enum Pass2 { mfma64, tile32, mfma32, valu } pass2 = mfma64;  // E3D_REG_PASS2=tile32|mfma32|valu: the pass-2 kernel (launch_pass2)
  bool pass2_mfma10 = getenv("E3D_REG_PASS2_MFMA10") != nullptr;      // experiment: the single-launch system on the matrix cores too
  enum Solver { by_size, dense, arrow } solver = by_size;      // E3D_REG_SOLVER=dense|arrow forces one solve of Apply (DampedSolver; tests)
  bool fuse_cost = env_int("E3D_REG_FUSE_COST", 1) != 0;       // 0: the separate cost pass in every iteration (e3d_reg_run_on_current_scale)
  RegSwitches() {
    const char* e = getenv("E3D_REG_MIN_FILTER");
    separable_min_filter = e && !strcmp(e, "separable");
    // pass 2: one resident round of workgroups (two of these 256-thread groups fit a CU): 512 on MI355X; measured 0.684 / 0.694 / 0.704 /
    // 0.711 ms for 512 / 1024 / 2048 / 4096 at the configs[3] shape
    int dev = 0, cus = 0;
    if ((e = getenv("E3D_REG_PASS2_BLOCKS"))) pass2_blocks = std::max(8, atoi(e));
    else if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
      pass2_blocks = 2 * cus;
    if ((e = getenv("E3D_REG_PASS2"))) pass2 = !strcmp(e, "valu") ? valu : (!strcmp(e, "tile32") ? tile32 : (!strcmp(e, "mfma32") ? mfma32 : mfma64));
    if ((e = getenv("E3D_REG_SOLVER"))) solver = !strcmp(e, "dense") ? dense : (!strcmp(e, "arrow") ? arrow : by_size);
  }
};
inline const RegSwitches& reg_switches() { static const RegSwitches sw; return sw; }

inline void rsync(e3d_reg* h) { E3D_HIP(hipStreamSynchronize(h->stream)); }
// A few words back from the device, through the handle's pinned mailbox, and the stream synchronised: hipMemcpyAsync into pageable
// memory (a stack variable) goes through the runtime's staging path and costs several times the copy into pinned memory -- an
// iteration of RunOnCurrentScale reads ~120 such results (pair counts, kept / dropped candidates, the sums of every pass).
inline void read_back(e3d_reg* h, void* dst, const void* src_dev, size_t bytes) {
  if (bytes == 0 || !reg_switches().pinned) { copy_out(dst, src_dev, bytes, h->stream); rsync(h); return; }
  if (bytes > h->mailbox.cap) h->mailbox.reserve(std::max(bytes, (size_t)65536));
  E3D_HIP(hipMemcpyAsync(h->mailbox.p, src_dev, bytes, hipMemcpyDeviceToHost, h->stream));
  E3D_HIP(hipStreamSynchronize(h->stream));
  memcpy(dst, h->mailbox.p, bytes);
}

// stop-watch of one kernel group (HIP events on the handle's stream; only while e3d_reg_profile is on)
struct KT {
  e3d_reg* h; hipEvent_t a = nullptr, b = nullptr; e3d_reg::KGroup* g = nullptr;
  KT(e3d_reg* hh, const char* name, double units) : h(hh) {
    if (!h->profile_on) return;
    if (h->kpending.size() >= 8192) h->kflush();
    if (h->kfree.empty()) { hipEvent_t x, y; E3D_HIP(hipEventCreate(&x)); E3D_HIP(hipEventCreate(&y)); h->kfree.emplace_back(x, y); }
    a = h->kfree.back().first; b = h->kfree.back().second; h->kfree.pop_back();
    g = &h->kgroups[name];
    g->calls += 1; g->units += units;
    (void)hipEventRecord(a, h->stream);
  }
  ~KT() {
    if (!g) return;
    (void)hipEventRecord(b, h->stream);
    h->kpending.push_back({a, b, g});
  }
};

struct Phase {
  e3d_reg* h; const char* name; std::chrono::steady_clock::time_point t0;
  Phase(e3d_reg* hh, const char* n) : h(hh), name(n) {
    if (h->profile_on) { (void)hipStreamSynchronize(h->stream); t0 = std::chrono::steady_clock::now(); }
  }
  ~Phase() {
    if (h->profile_on) {
      (void)hipStreamSynchronize(h->stream);
      h->profile_ms[name] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  }
};
inline unsigned nblk(size_t n) { return (unsigned)div_up(n ? n : 1, kBlock); }
inline int image_owner(const e3d_reg* h, int image_id) { return h->world <= 1 ? 0 : ((image_id % h->world) + h->world) % h->world; }
inline PointScale& get_scale(e3d_reg* h, int s) {
  auto it = h->scales.find(s);
  if (it == h->scales.end()) throw Error(E3D_ERR_INDEX, fmt("point scale %d not set", s));
  return it->second;
}
inline ImageDev& get_image(e3d_reg* h, int id) {
  auto it = h->images.find(id);
  if (it == h->images.end()) throw Error(E3D_ERR_INDEX, fmt("image %d not set", id));
  return it->second;
}
inline int best_available_scale(const e3d_reg* h, const Intrin& in) {
  // Intrinsics::best_available_image_scale(max(min_occlusion_check_image_scale (0), current_image_scale))
  const int want = std::max(0, (int)h->prm.current_image_scale);
  return std::min<int>(in.min_image_scale + (int)in.levels.size() - 1, std::max<int>(in.min_image_scale, want));
}

// ---- what crosses the files (each kernel lives in one .hip; another file reaches it through its launch function) --------------------
// e3d_reg.hip: p[0 .. n) = v and out[i] = {xyz[3 i], xyz[3 i + 1], xyz[3 i + 2], 0} on stream s (k_fill_f32, k_xyz_to_float4)
void fill_f32(float* p, size_t n, float v, hipStream_t s);
void xyz_to_float4(const float* xyz, size_t n, float4* out, hipStream_t s);
// e3d_reg_depth.hip: OcclusionGeometry::RenderDepthMap of one image at one image scale into im.depth; depth_out (host) may be null
void render_depth(e3d_reg* h, int image_id, int image_scale, float* depth_out);

}  // namespace e3d
