// e3d_reg_scan.hip -- the scan-side tools of the registration handle (e3d_reg_handle.hpp): kernels and C-ABI entries (include/e3d_hip.h)
// that ask one image about the evaluation scans -- GroundTruthCreator visibility and scan rendering, the debug point-cloud colours,
// MaskTransfer, ImageLocalizer, ImageUndistorter (its resampling kernel: e3d_undistort.hip) -- and the host-only e3d_pose_from_bearings.
// Their state is the handle's ScanTools; the occlusion depth they test against is render_depth of e3d_reg_depth.hip.
#include <algorithm>
#include <cmath>

#include "e3d_reg_handle.hpp"
#include "e3d_undistort.hpp"

#pragma clang fp contract(off)

namespace e3d {

// ==== debug point clouds (Problem::DebugWriteColoredPointCloud, problem.cc:642-704) ==============================================
// One image: every scan point that is an observation without scale test takes a bilinear sample of the colour image
// (InterpolateBilinearVec3, interpolate_bilinear.h:117-146) at its position at the camera's highest resolution
// (PointObservation::image_x_at_scale(min_image_scale), point_observation.h:84-93) and adds it to its accumulator {r, g, b sums as
// f32, count as int bits} -- one 16-byte record, one load and one store.  A point is touched by one thread per image and the images
// run one after the other on the handle's stream, so there are no atomics (as in k_point_radius).  rgb: cols x rows pixels of 3
// bytes, R G B, the file's own size -- the sample is rejected by ITS bounds, whatever the camera's size is.
template <int M>
__global__ __launch_bounds__(kBlock) void k_scan_colors(const float4* __restrict__ pts, size_t n, Pose P, CamLevel cam,
                                                        const unsigned char* __restrict__ img, const unsigned char* __restrict__ mask,
                                                        const unsigned char* __restrict__ cam_mask, const float* __restrict__ occlusion,
                                                        RadiusParams rp, const unsigned char* __restrict__ rgb, int cols, int rows,
                                                        float4* __restrict__ acc) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float ox, oy, returned_scale;
  if (!observe_no_scale<M>(pts[i], P, cam, img, mask, cam_mask, occlusion, rp, ox, oy, returned_scale)) return;
  const int smaller_scale = (int)returned_scale + 1;
  const float up = exp2f((float)(smaller_scale - rp.min_image_scale));     // exact power of two
  const float x = up * (ox + 0.5f) - 0.5f, y = up * (oy + 0.5f) - 0.5f;
  const int ix = f2i(x), iy = f2i(y);
  // (!(x >= 0) is x < 0 for the finite positions an observation has and keeps a NaN out: 0 <= ix <= cols - 2, 0 <= iy <= rows - 2 below)
  if (!(x >= 0.f) || !(y >= 0.f) || ix >= cols - 1 || iy >= rows - 1) return;
  const float fx = x - (float)ix, fx_inv = 1.f - fx, fy = y - (float)iy, fy_inv = 1.f - fy;
  const unsigned char* top = rgb + ((size_t)iy * cols + ix) * 3;
  const unsigned char* bottom = top + (size_t)cols * 3;
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    c[k] = fx_inv * fy_inv * (float)top[k] + fx * fy_inv * (float)top[3 + k] + fx_inv * fy * (float)bottom[k] + fx * fy * (float)bottom[3 + k];
  float4 a = acc[i];
  a.x += c[0]; a.y += c[1]; a.z += c[2];
  a.w = __int_as_float(__float_as_int(a.w) + 1);
  acc[i] = a;
}

// point->r = color_sums.x() / observation_counts + 0.5f (problem.cc:690-696): f32 divide, truncation to u8; never observed = 0 0 0
__global__ __launch_bounds__(kBlock) void k_scan_colors_finish(const float4* __restrict__ acc, size_t n, unsigned char* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = acc[i];
  const int count = __float_as_int(a.w);
  unsigned char r = 0, g = 0, b = 0;
  if (count > 0) {
    r = (unsigned char)(a.x / (float)count + 0.5f);
    g = (unsigned char)(a.y / (float)count + 0.5f);
    b = (unsigned char)(a.z / (float)count + 0.5f);
  }
  out[3 * i] = r; out[3 * i + 1] = g; out[3 * i + 2] = b;
}

// ==== f4: GroundTruthCreator visibility (src/exe/ground_truth_creator.cc:45-86, :152-189) =========================================
// mode 0: counts[i] += 1 for every scan point visible in the image; mode 1: ground-truth depth = min z over the visible
// points that were counted at least `min_count` times; mode 2: scan rendering (:175-187) -- the reference paints a square of
// 2 * radius + 1 pixels around every such point in point order, later points over earlier ones, so a pixel ends up with the colour of
// the LAST point whose square covers it: gt_depth[pixel] = max (point index + 1), 0 = untouched.
// "Visible" = in front of the camera, inside the image at the
// highest available resolution, not behind the occlusion depth (+ threshold), not under an eval-obs mask pixel.
template <int M>
__global__ __launch_bounds__(kBlock) void k_scan_visibility(const float4* __restrict__ pts, size_t n, Pose P, CamLevel cam,
                                                            const float* __restrict__ occlusion, float occlusion_threshold,
                                                            const unsigned char* __restrict__ mask, int excluded_flag, int mode,
                                                            int min_count, int* __restrict__ counts, unsigned* __restrict__ gt_depth,
                                                            int radius) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (mode != 0 && counts[i] < min_count) return;
  const float4 p = pts[i];
  float X, Yc, Z;
  rt(P, p.x, p.y, p.z, X, Yc, Z);
  if (!(Z > 0.f)) return;
  float ixf, iyf;
  cam_normalized_to_image<M>(cam, X / Z, Yc / Z, ixf, iyf);
  const int ix = f2i(ixf + 0.5f), iy = f2i(iyf + 0.5f);
  if (!(ix >= 0 && iy >= 0 && ix < cam.width && iy < cam.height)) return;
  const size_t px = (size_t)iy * cam.width + ix;
  if (!(occlusion[px] + occlusion_threshold >= Z)) return;
  if (mask && mask[px] == excluded_flag) return;
  if (mode == 0) counts[i] += 1;
  else if (mode == 1) atomicMin(&gt_depth[px], __float_as_uint(Z));       // Z > 0: the bit pattern orders like the value
  else {
    const int x0 = max(0, ix - radius), y0 = max(0, iy - radius), x1 = min(cam.width, ix + radius + 1), y1 = min(cam.height, iy + radius + 1);
    for (int y = y0; y < y1; ++y)
      for (int x = x0; x < x1; ++x) atomicMax(&gt_depth[(size_t)y * cam.width + x], (unsigned)i + 1u);
  }
}

// ==== MaskTransfer: DatasetInspector's "Label transfer" (src/dataset_inspector/gui_main_window.cc:868-1054) ========================
// A mask drawn in one image carried to another through the scan points.  The reference is one serial loop over the cloud that
// writes target_mask(target pixel) = source_mask(source pixel) for every point visible in both images, later points over earlier
// ones, then fills holes with a 5 x 5 vote and merges the result into the target's mask.  Here: per point the label it carries
// (k_mask_label_points, once per source), per target the highest labelled point index per pixel (k_mask_scatter, atomicMax of
// index + 1 as in the scan rendering above -- integer max, so the result is the serial loop's whatever the launch order), then one
// pass over the target's pixels (k_mask_fill).
//
// Visibility of a point in an image (:909-921, :931-943): z > 0, the rounded pixel inside the image at the highest resolution,
// occlusion + threshold >= z; returns the pixel's index or -1.  Unlike the visibility test above, the reference also asks for
// pxy + 0.5f >= 0 here: (int) truncates towards zero, so a position in (-1.5, -0.5) would otherwise land in column / row 0.
// mask_point_state is the test itself: 0 = behind the camera or outside the image, 1 = visible, 2 = inside the image but behind the
// occlusion depth; pxy is the unrounded position (NaN behind the camera) and px the pixel's index (states 1 and 2).
constexpr int kPointOutside = 0, kPointVisible = 1, kPointOccluded = 2;
template <int M>
__device__ __forceinline__ int mask_point_state(const float4 p, const Pose& P, const CamLevel& cam, const float* __restrict__ occlusion,
                                                float occlusion_threshold, float2& pxy, size_t& px) {
  float X, Yc, Z;
  rt(P, p.x, p.y, p.z, X, Yc, Z);
  pxy = make_float2(NAN, NAN);
  if (!(Z > 0.f)) return kPointOutside;
  float ixf, iyf;
  cam_normalized_to_image<M>(cam, X / Z, Yc / Z, ixf, iyf);
  pxy = make_float2(ixf, iyf);
  const float rx = ixf + 0.5f, ry = iyf + 0.5f;
  if (!(rx >= 0.f && ry >= 0.f)) return kPointOutside;
  const int ix = f2i(rx), iy = f2i(ry);
  if (!(ix >= 0 && iy >= 0 && ix < cam.width && iy < cam.height)) return kPointOutside;
  px = (size_t)iy * cam.width + ix;
  if (!(occlusion[px] + occlusion_threshold >= Z)) return kPointOccluded;
  return kPointVisible;
}
template <int M>
__device__ __forceinline__ long long mask_visible_pixel(const float4 p, const Pose& P, const CamLevel& cam, const float* __restrict__ occlusion,
                                                        float occlusion_threshold) {
  float2 pxy;
  size_t px = 0;
  return mask_point_state<M>(p, P, cam, occlusion, occlusion_threshold, pxy, px) == kPointVisible ? (long long)px : -1;
}

// bad[0] += number of mask bytes other than 0 / 1 / 2 (image.cc:87-97 aborts on them)
__global__ __launch_bounds__(kBlock) void k_mask_check_values(const unsigned char* __restrict__ mask, size_t n, unsigned long long* __restrict__ bad) {
  __shared__ unsigned sc[kBlock / kWave];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  block_count_add(i < n && mask[i] > 2, bad, sc);
}

// Source half: labels[i] = the source mask's value at the point's pixel if the point is visible there and the value is not 0 nor --
// without transfer_eval_obs -- kEvalObs (2); else 0.  labelled[0] += number of non-zero labels.
template <int M>
__global__ __launch_bounds__(kBlock) void k_mask_label_points(const float4* __restrict__ pts, size_t n, Pose P, CamLevel cam,
                                                              const float* __restrict__ occlusion, float occlusion_threshold,
                                                              const unsigned char* __restrict__ mask, int transfer_eval_obs,
                                                              unsigned char* __restrict__ labels, unsigned long long* __restrict__ labelled) {
  __shared__ unsigned sc[kBlock / kWave];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned char v = 0;
  if (i < n) {
    const long long px = mask_visible_pixel<M>(pts[i], P, cam, occlusion, occlusion_threshold);
    if (px >= 0) {
      v = mask[px];
      if (v > 2 || (v == 2 && !transfer_eval_obs)) v = 0;       // (values above 2 are refused by the caller; never a label)
    }
    labels[i] = v;
  }
  block_count_add(v != 0, labelled, sc);
}

// Target half, point pass: winner[pixel] = max (index + 1) over the labelled points visible in the target; 0 = no point.  The label
// is read first: most points of a real dataset carry none and leave without fetching their position.
template <int M>
__global__ __launch_bounds__(kBlock) void k_mask_scatter(const float4* __restrict__ pts, const unsigned char* __restrict__ labels, size_t n,
                                                         Pose P, CamLevel cam, const float* __restrict__ occlusion, float occlusion_threshold,
                                                         unsigned* __restrict__ winner) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || labels[i] == 0) return;
  const long long px = mask_visible_pixel<M>(pts[i], P, cam, occlusion, occlusion_threshold);
  if (px >= 0) atomicMax(&winner[px], (unsigned)i + 1u);
}

// Target half, per pixel: the winner's label; the numbers of kObs (1) and kEvalObs (2) labels in the 5 x 5 window around it, clipped
// at the image borders (:997-1023; the reference's integral images are its way to count, any exact count gives the same mask);
// obs >= 3 -> kObs, then with transfer_eval_obs eval_obs >= 3 -> kEvalObs (:1025-1030; so a kEvalObs pixel with >= 3 kObs but
// fewer than 3 kEvalObs pixels around it BECOMES kObs -- the reference's behaviour, kept); merge (:1034-1047): the new value
// replaces the existing one where it is not 0 and the existing one is not kEvalObs.  The window counts come from the point pass
// alone (all labels of the tile and its 2-pixel apron are staged in LDS before any pixel is decided), so the fill is not recursive.
// counters: [0] pixels set by the point pass, [1] non-zero pixels after the fill-in, [2] pixels of the merged mask that differ from
// the existing one (from 0 without one), [3] existing values other than 0 / 1 / 2.
// One block: 64 x 16 pixels, one wave per 4 rows, 4 pixels (one column of those rows) per thread: the 5-tap row sums of the 8 tile
// rows a thread's pixels see are formed once (kObs count in the low half-word, kEvalObs count in the high one) and shared by them.
constexpr int kMaskTileW = kWave, kMaskRows = 4, kMaskTileH = (kBlock / kWave) * kMaskRows, kMaskApron = 2;
__global__ __launch_bounds__(kBlock) void k_mask_fill(const unsigned* __restrict__ winner, const unsigned char* __restrict__ labels, int width,
                                                      int height, int transfer_eval_obs, const unsigned char* __restrict__ existing,
                                                      unsigned char* __restrict__ out, unsigned long long* __restrict__ counters) {
  constexpr int LW = kMaskTileW + 2 * kMaskApron, LH = kMaskTileH + 2 * kMaskApron, kWin = 2 * kMaskApron + 1;
  __shared__ unsigned char tile[LH][LW];
  __shared__ unsigned sc[kBlock / kWave][4];
  const int x0 = (int)blockIdx.x * kMaskTileW, y0 = (int)blockIdx.y * kMaskTileH;
  for (int k = threadIdx.x; k < LW * LH; k += kBlock) {
    const int ly = k / LW, lx = k - ly * LW;
    const int x = x0 + lx - kMaskApron, y = y0 + ly - kMaskApron;
    unsigned char v = 0;                        // outside the image: no label -- the window is clipped, not clamped
    if (x >= 0 && y >= 0 && x < width && y < height) {
      const unsigned w = winner[(size_t)y * width + x];
      if (w) v = labels[w - 1];
    }
    tile[ly][lx] = v;
  }
  __syncthreads();
  const int tx = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int x = x0 + tx, ly0 = wave * kMaskRows;              // the thread's pixels: column x, rows y0 + ly0 .. + kMaskRows - 1
  unsigned row_sum[kMaskRows + kWin - 1];
#pragma unroll
  for (int k = 0; k < kMaskRows + kWin - 1; ++k) {
    unsigned s = 0;
#pragma unroll
    for (int dx = 0; dx < kWin; ++dx) {
      const unsigned char t = tile[ly0 + k][tx + dx];
      s += (t == 1 ? 1u : 0u) + (t == 2 ? 0x10000u : 0u);
    }
    row_sum[k] = s;
  }
  constexpr unsigned kFillInThreshold = 3;      // (int)(0.10f * 25 + 0.5f)
  unsigned count[4] = {0, 0, 0, 0};             // (wave-uniform) set by the point pass, non-zero after the fill-in, changed, bad existing value
#pragma unroll
  for (int j = 0; j < kMaskRows; ++j) {
    const int y = y0 + ly0 + j;
    const bool inside = x < width && y < height;
    bool set_by_points = false, non_zero = false, changed = false, bad = false;
    if (inside) {
      unsigned s = 0;
#pragma unroll
      for (int k = 0; k < kWin; ++k) s += row_sum[j + k];
      const unsigned obs = s & 0xFFFFu, eval_obs = s >> 16;
      unsigned char v = tile[ly0 + j + kMaskApron][tx + kMaskApron];
      set_by_points = v != 0;
      if (obs >= kFillInThreshold) v = 1;
      if (transfer_eval_obs && eval_obs >= kFillInThreshold) v = 2;
      non_zero = v != 0;
      const size_t px = (size_t)y * width + x;
      const unsigned char e = existing ? existing[px] : (unsigned char)0;
      bad = e > 2;
      const unsigned char m = (v != 0 && e != 2) ? v : e;
      changed = m != e;
      out[px] = m;
    }
    count[0] += (unsigned)__popcll(__ballot(set_by_points));
    count[1] += (unsigned)__popcll(__ballot(non_zero));
    count[2] += (unsigned)__popcll(__ballot(changed));
    count[3] += (unsigned)__popcll(__ballot(bad));
  }
  if (tx == 0)
    for (int c = 0; c < 4; ++c) sc[wave][c] = count[c];
  __syncthreads();
  if (threadIdx.x < 4) {                        // one atomic per block and counter
    unsigned c = 0;
    for (int w = 0; w < kBlock / kWave; ++w) c += sc[w][threadIdx.x];
    if (c) atomicAdd(counters + threadIdx.x, (unsigned long long)c);
  }
}

// ==== ImageLocalizer: DatasetInspector's "Localize image" click on a scan point (src/dataset_inspector/localize_image_tool.cc:96-110) ====
// The reference keeps the projections of all visible scan points (ImageWidget::UpdateScanPoints, gui_image_widget.cc:521-556: the
// visibility test of the label transfer above) and, per click, walks them for the smallest squared pixel distance -- strict <, from
// +inf, so of equal distances the first point wins and a NaN distance never does.  Here one pass over the cloud serves up to
// E3D_LOCALIZE_MAX_CLICKS clicks: a block projects 256 points per step of a grid-stride loop (each point once, its occlusion value
// gathered once) and leaves the positions of the visible ones in LDS (NaN for the others).  The compares are then dealt out by click:
// with `group` = the click count rounded up to a power of two, lane l of a wave owns click l % group and the wave's points
// [l / group * group, + group), read from LDS as broadcasts.  So a lane carries ONE running key whatever the click count -- the
// register cost of the cloud pass does not depend on it -- and does `group` compares per step: 1 click is one compare of the lane's
// own point, 32 clicks are 32 compares per lane, the same total as a key per click and thread.  key = (f32 bits of d) << 32 | index:
// for finite d >= 0 its integer order is (d, index), the reference's order.  The launch ends with a wave minimum over the lanes of
// one click (__shfl_xor over the offsets >= group), a block minimum through LDS and one 64-bit atomicMin per block and click, none
// where the block found nothing.
constexpr int kPickMaxBlocks = 2048;            // 8 blocks of 256 threads for each of the 256 CUs
constexpr unsigned long long kPickNone = ~0ull;
// Vector2f::squaredNorm of (pxy - click), no contraction
__device__ __forceinline__ float pick_distance(float2 pxy, float2 click) {
  const float dx = pxy.x - click.x, dy = pxy.y - click.y;
  return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}
template <int M>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8))) void k_pick_scan_points(const float4* __restrict__ pts, size_t n, Pose P, CamLevel cam,
                                                             const float* __restrict__ occlusion, float occlusion_threshold,
                                                             const float2* __restrict__ clicks, int n_clicks, int group,
                                                             unsigned long long* __restrict__ keys, unsigned long long* __restrict__ n_visible) {
  __shared__ float2 positions[kBlock];
  __shared__ unsigned long long wave_best[kBlock / kWave][E3D_LOCALIZE_MAX_CLICKS];
  __shared__ unsigned sc[kBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int click_id = lane & (group - 1);                                    // group: a power of two, n_clicks <= group <= 32
  const int first = wave * kWave + (lane & ~(group - 1));                     // the lane's points of every step, as threads of the block
  const float2 click = click_id < n_clicks ? clicks[click_id] : make_float2(NAN, NAN);      // (a lane without a click never finds a key)
  unsigned long long best = kPickNone;
  unsigned visible = 0;
  for (size_t base = (size_t)blockIdx.x * kBlock; base < n; base += (size_t)gridDim.x * kBlock) {      // the same trips for the whole block
    const size_t i = base + threadIdx.x;
    float2 pxy = make_float2(NAN, NAN);
    size_t px = 0;
    const bool seen = i < n && mask_point_state<M>(pts[i], P, cam, occlusion, occlusion_threshold, pxy, px) == kPointVisible;
    visible += (unsigned)__popcll(__ballot(seen));
    positions[threadIdx.x] = seen ? pxy : make_float2(NAN, NAN);
    __syncthreads();
    for (int j = 0; j < group; ++j) {
      const float d = pick_distance(positions[first + j], click);
      if (d < INFINITY) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(base + first + j);
        best = key < best ? key : best;
      }
    }
    __syncthreads();
  }
  for (int o = kWave / 2; o >= group; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, kWave);
    best = other < best ? other : best;
  }
  if (lane < n_clicks) wave_best[wave][lane] = best;
  __syncthreads();
  if ((int)threadIdx.x < n_clicks) {
    unsigned long long b = wave_best[0][threadIdx.x];
    for (int w = 1; w < kBlock / kWave; ++w) b = wave_best[w][threadIdx.x] < b ? wave_best[w][threadIdx.x] : b;
    if (b != kPickNone) atomicMin(keys + threadIdx.x, b);
  }
  block_wave_counts_add(visible, n_visible, sc);
}
// ... and the winners once more, for the position and the distance the key has no room for: result[3 c ..] = {pxy.x, pxy.y, d},
// {NaN, NaN, +inf} without a winner
template <int M>
__global__ __launch_bounds__(kWave) void k_pick_finish(const float4* __restrict__ pts, Pose P, CamLevel cam, const float* __restrict__ occlusion,
                                                       float occlusion_threshold, const float2* __restrict__ clicks, int n_clicks,
                                                       const unsigned long long* __restrict__ keys, float* __restrict__ result) {
  const int c = (int)threadIdx.x;
  if (c >= n_clicks) return;
  const unsigned long long key = keys[c];
  float2 pxy = make_float2(NAN, NAN);
  float d = INFINITY;
  if (key != kPickNone) {
    size_t px = 0;
    mask_point_state<M>(pts[key & 0xffffffffull], P, cam, occlusion, occlusion_threshold, pxy, px);
    d = pick_distance(pxy, clicks[c]);
  }
  result[3 * c] = pxy.x; result[3 * c + 1] = pxy.y; result[3 * c + 2] = d;
}
// e3d_reg_project_points: position and state (mask_point_state) of arbitrary points, xyz packed
template <int M>
__global__ __launch_bounds__(kBlock) void k_project_points(const float* __restrict__ xyz, size_t n, Pose P, CamLevel cam,
                                                           const float* __restrict__ occlusion, float occlusion_threshold,
                                                           float2* __restrict__ pixel, unsigned char* __restrict__ state) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float2 pxy;
  size_t px = 0;
  state[i] = (unsigned char)mask_point_state<M>(make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f), P, cam, occlusion,
                                                occlusion_threshold, pxy, px);
  pixel[i] = pxy;
}

// e3d_reg_image_bearings: ImageToNormalized of n pixel positions (LocalizeImageTool, localize_image_tool.cc:58-61), the four lattice
// entries around each computed here where the model goes through the table
template <int M>
__global__ __launch_bounds__(kBlock) void k_image_bearings(CamLevel c, const float2* __restrict__ pixels, int n, float2* __restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const float2 p = pixels[i];
  out[i] = camera_image_to_normalized<M>(c, p.x, p.y, [&](int x, int y) { return undistort_lookup_entry<M>(c, x, y); });
}

}  // namespace e3d

extern "C" {

// the image of a call, checked: known, owned by this rank
static ImageDev& owned_image(e3d_reg* h, int image_id) {
  ImageDev& im = get_image(h, image_id);
  if (!h->owns(image_id)) throw Error(E3D_ERR_INVALID, fmt("image %d belongs to rank %d", image_id, image_owner(h, image_id)));
  return im;
}

// ---- f4: GroundTruthCreator -------------------------------------------------------------------------------------------------
int e3d_reg_set_scan_points(e3d_reg_t* h, const float* xyz, size_t n) {
  E3D_TRY_ON(h)
  if (!h || (n && !xyz)) throw Error(E3D_ERR_INVALID, "null argument");
  if (n >= (size_t)1 << 31) throw Error(E3D_ERR_INVALID, "more than 2^31-1 scan points");
  h->scan.n_scan = n; h->scan.scan_points_set = true; h->scan.scan_colors_begun = false; h->scan.mask_labels_ready = false;
  h->scan.scan_pts.reserve(n); h->scan.scan_counts.reserve(n);
  if (n) {
    DevBuf<float> raw;
    raw.reserve(3 * n);
    copy_in(raw.p, xyz, sizeof(float) * 3 * n, h->stream);
    xyz_to_float4(raw.p, n, h->scan.scan_pts.p, h->stream);
    E3D_HIP(hipMemsetAsync(h->scan.scan_counts.p, 0, sizeof(int) * n, h->stream));
    rsync(h);
  }
  return 0;
  E3D_CATCH()
}
// one k_scan_visibility launch against im.depth as it stands (mask_dev: device, may be null; gt_depth: the map of modes 1 and 2)
static void launch_scan_visibility(e3d_reg* h, ImageDev& im, const Intrin& in, const unsigned char* mask_dev, int excluded_flag, int mode,
                                   int min_count, unsigned* gt_depth, int radius = 0) {
  if (h->scan.n_scan)
    E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_scan_visibility<M>, dim3(nblk(h->scan.n_scan)), dim3(kBlock), 0, h->stream, h->scan.scan_pts.p,
                                               h->scan.n_scan, im.pose, in.levels[0], im.depth.p, h->prm.occlusion_depth_threshold, mask_dev,
                                               excluded_flag, mode, min_count, h->scan.scan_counts.p, gt_depth, radius));
}
static void scan_visibility(e3d_reg* h, int image_id, const uint8_t* mask, int excluded_flag, int mode, int min_count, int radius = 0) {
  ImageDev& im = get_image(h, image_id);
  const Intrin& in = h->intr.at(im.intrinsics_id);
  // RenderDepthMap(intrinsics, image, intrinsics.min_image_scale, ...) + intrinsics.model(0): the highest resolution
  render_depth(h, image_id, in.min_image_scale, nullptr);
  const CamLevel& cam = in.levels[0];
  const size_t px = (size_t)cam.width * cam.height;
  if (mask) { h->scan.eval_mask.reserve(px); copy_in(h->scan.eval_mask.p, mask, px, h->stream); }
  launch_scan_visibility(h, im, in, mask ? h->scan.eval_mask.p : nullptr, excluded_flag, mode, min_count, h->scan.gt_depth.p, radius);
}
int e3d_reg_count_scan_observations(e3d_reg_t* h, int image_id, const uint8_t* mask, int excluded_flag) {
  E3D_TRY_ON(h)
  if (!h) throw Error(E3D_ERR_INVALID, "null handle");
  scan_visibility(h, image_id, mask, excluded_flag, 0, 0);
  rsync(h);
  return 0;
  E3D_CATCH()
}
int e3d_reg_get_scan_observation_counts(e3d_reg_t* h, int32_t* counts) {
  E3D_TRY_ON(h)
  if (!h || (!counts && h->scan.n_scan)) throw Error(E3D_ERR_INVALID, "null argument");
  if (h->scan.n_scan) copy_out(counts, h->scan.scan_counts.p, sizeof(int) * h->scan.n_scan, h->stream);
  rsync(h);
  return 0;
  E3D_CATCH()
}
int e3d_reg_set_scan_observation_counts(e3d_reg_t* h, const int32_t* counts) {
  E3D_TRY_ON(h)
  if (!h || (!counts && h->scan.n_scan)) throw Error(E3D_ERR_INVALID, "null argument");
  if (h->scan.n_scan) copy_in(h->scan.scan_counts.p, counts, sizeof(int) * h->scan.n_scan, h->stream);
  rsync(h);
  return 0;
  E3D_CATCH()
}
int e3d_reg_ground_truth_depth(e3d_reg_t* h, int image_id, const uint8_t* mask, int excluded_flag, int min_count, float* gt_depth,
                               float* occlusion_depth) {
  E3D_TRY_ON(h)
  if (!h) throw Error(E3D_ERR_INVALID, "null handle");
  ImageDev& im = get_image(h, image_id);
  const CamLevel& cam = h->intr.at(im.intrinsics_id).levels[0];
  const size_t px = (size_t)cam.width * cam.height;
  h->scan.gt_depth.reserve(px);
  fill_f32(reinterpret_cast<float*>(h->scan.gt_depth.p), px, INFINITY, h->stream);
  scan_visibility(h, image_id, mask, excluded_flag, 1, min_count);
  if (gt_depth) copy_out(gt_depth, h->scan.gt_depth.p, sizeof(float) * px, h->stream);
  if (occlusion_depth) copy_out(occlusion_depth, im.depth.p, sizeof(float) * px, h->stream);
  rsync(h);
  return 0;
  E3D_CATCH()
}

/* CreateGroundTruthForImage, scan rendering part (ground_truth_creator.cc:149,175-187): which scan point ends up on top of every pixel
 * when the visible points counted at least min_count times are painted as squares in point order.  winner[pixel] = point index + 1, 0 where
 * the image keeps its own colour. */
int e3d_reg_scan_rendering(e3d_reg_t* h, int image_id, const uint8_t* mask, int excluded_flag, int min_count, int point_radius,
                           uint32_t* winner) {
  E3D_TRY_ON(h)
  if (!h || !winner) throw Error(E3D_ERR_INVALID, "null argument");
  if (point_radius < 0 || point_radius > 64) throw Error(E3D_ERR_INVALID, "scan_point_radius out of range [0, 64]");
  if (h->scan.n_scan >= 0xFFFFFFFFull) throw Error(E3D_ERR_INVALID, "too many scan points for 32-bit indices");
  ImageDev& im = get_image(h, image_id);
  const CamLevel& cam = h->intr.at(im.intrinsics_id).levels[0];
  const size_t px = (size_t)cam.width * cam.height;
  h->scan.gt_depth.reserve(px);
  E3D_HIP(hipMemsetAsync(h->scan.gt_depth.p, 0, sizeof(unsigned) * px, h->stream));
  scan_visibility(h, image_id, mask, excluded_flag, 2, min_count, point_radius);
  copy_out(winner, h->scan.gt_depth.p, sizeof(unsigned) * px, h->stream);
  rsync(h);
  return 0;
  E3D_CATCH()
}

// ---- MaskTransfer (MainWindow::TransferLabels, src/dataset_inspector/gui_main_window.cc:868-1054) ---------------------------------
int64_t e3d_reg_mask_transfer_source(e3d_reg_t* h, int source_image_id, const uint8_t* source_mask, int transfer_eval_obs) {
  E3D_TRY_ON(h)
  if (!h || !source_mask) throw Error(E3D_ERR_INVALID, "null argument");
  if (!h->scan.scan_points_set) throw Error(E3D_ERR_INVALID, "no scan points set (e3d_reg_set_scan_points)");
  ImageDev& im = owned_image(h, source_image_id);
  const Intrin& in = h->intr.at(im.intrinsics_id);
  const CamLevel& cam = in.levels[0];
  const size_t px = (size_t)cam.width * cam.height, n = h->scan.n_scan;
  h->scan.mask_labels_ready = false;
  h->scan.mask_in.reserve(px); h->scan.mask_labels.reserve(n); h->scan.mask_counters.reserve(5);
  copy_in(h->scan.mask_in.p, source_mask, px, h->stream);
  E3D_HIP(hipMemsetAsync(h->scan.mask_counters.p, 0, sizeof(unsigned long long) * 5, h->stream));
  hipLaunchKernelGGL(k_mask_check_values, dim3(nblk(px)), dim3(kBlock), 0, h->stream, h->scan.mask_in.p, px, h->scan.mask_counters.p + 4);
  if (n) {
    // RenderDepthMap(source_intrinsics, *source_image, source_intrinsics.min_image_scale, ...) + intrinsics.model(0) (:877-881)
    render_depth(h, source_image_id, in.min_image_scale, nullptr);
    KT kt(h, "mask.label_points", (double)n);
    E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_mask_label_points<M>, dim3(nblk(n)), dim3(kBlock), 0, h->stream, h->scan.scan_pts.p, n, im.pose, cam,
                                               im.depth.p, h->prm.occlusion_depth_threshold, h->scan.mask_in.p, transfer_eval_obs ? 1 : 0,
                                               h->scan.mask_labels.p, h->scan.mask_counters.p));
  }
  unsigned long long counters[5];
  read_back(h, counters, h->scan.mask_counters.p, sizeof counters);
  E3D_HIP(hipGetLastError());
  if (counters[4]) throw Error(E3D_ERR_INVALID, fmt("the source mask holds %llu values other than 0, 1, 2", counters[4]));
  h->scan.mask_labels_ready = true;
  h->scan.mask_transfer_eval_obs = transfer_eval_obs ? 1 : 0;
  return (int64_t)counters[0];
  E3D_CATCH()
}
int e3d_reg_mask_transfer_target(e3d_reg_t* h, int target_image_id, const uint8_t* existing_mask, uint8_t* mask_out, int64_t* stats) {
  E3D_TRY_ON(h)
  if (!h || !mask_out) throw Error(E3D_ERR_INVALID, "null argument");
  if (!h->scan.scan_points_set) throw Error(E3D_ERR_INVALID, "no scan points set (e3d_reg_set_scan_points)");
  if (!h->scan.mask_labels_ready) throw Error(E3D_ERR_INVALID, "call e3d_reg_mask_transfer_source first");
  ImageDev& im = owned_image(h, target_image_id);
  const Intrin& in = h->intr.at(im.intrinsics_id);
  const CamLevel& cam = in.levels[0];
  const size_t px = (size_t)cam.width * cam.height, n = h->scan.n_scan;
  h->scan.gt_depth.reserve(px); h->scan.mask_result.reserve(px);
  if (existing_mask) { h->scan.mask_in.reserve(px); copy_in(h->scan.mask_in.p, existing_mask, px, h->stream); }
  E3D_HIP(hipMemsetAsync(h->scan.mask_counters.p, 0, sizeof(unsigned long long) * 5, h->stream));
  E3D_HIP(hipMemsetAsync(h->scan.gt_depth.p, 0, sizeof(unsigned) * px, h->stream));       // the winners, blank for every target (:901-903)
  if (n) {
    render_depth(h, target_image_id, in.min_image_scale, nullptr);                     // (:882-886)
    KT kt(h, "mask.scatter", (double)n);
    E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_mask_scatter<M>, dim3(nblk(n)), dim3(kBlock), 0, h->stream, h->scan.scan_pts.p, h->scan.mask_labels.p, n,
                                               im.pose, cam, im.depth.p, h->prm.occlusion_depth_threshold, h->scan.gt_depth.p));
  }
  {
    KT kt(h, "mask.fill", (double)px);
    const dim3 grid((unsigned)div_up(cam.width, kMaskTileW), (unsigned)div_up(cam.height, kMaskTileH));
    hipLaunchKernelGGL(k_mask_fill, grid, dim3(kBlock), 0, h->stream, h->scan.gt_depth.p, h->scan.mask_labels.p, cam.width, cam.height,
                       h->scan.mask_transfer_eval_obs, existing_mask ? h->scan.mask_in.p : nullptr, h->scan.mask_result.p, h->scan.mask_counters.p);
  }
  unsigned long long counters[5];
  read_back(h, counters, h->scan.mask_counters.p, sizeof counters);
  E3D_HIP(hipGetLastError());
  if (counters[3]) throw Error(E3D_ERR_INVALID, fmt("the existing mask holds %llu values other than 0, 1, 2", counters[3]));
  copy_out(mask_out, h->scan.mask_result.p, px, h->stream);
  rsync(h);
  if (stats) for (int k = 0; k < 3; ++k) stats[k] = (int64_t)counters[k];
  return 0;
  E3D_CATCH()
}

// ---- ImageLocalizer (LocalizeImageTool, src/dataset_inspector/localize_image_tool.cc) ---------------------------------------------------
int64_t e3d_reg_pick_scan_points(e3d_reg_t* h, int image_id, const float* clicks_xy, int n_clicks, int64_t* index_out, float* pixel_out,
                                 float* distance_out) {
  E3D_TRY_ON(h)
  if (!h || !clicks_xy || !index_out) throw Error(E3D_ERR_INVALID, "null argument");
  if (n_clicks < 1 || n_clicks > E3D_LOCALIZE_MAX_CLICKS)
    throw Error(E3D_ERR_INVALID, fmt("n_clicks %d outside 1 .. %d", n_clicks, E3D_LOCALIZE_MAX_CLICKS));
  if (!h->scan.scan_points_set) throw Error(E3D_ERR_INVALID, "no scan points set (e3d_reg_set_scan_points)");
  if (h->scan.n_scan >= 0xFFFFFFFFull) throw Error(E3D_ERR_INVALID, "too many scan points for 32-bit indices");
  ImageDev& im = owned_image(h, image_id);
  const Intrin& in = h->intr.at(im.intrinsics_id);
  const CamLevel& cam = in.levels[0];
  const size_t n = h->scan.n_scan;
  constexpr int kKeys = 1, kResult = 1 + E3D_LOCALIZE_MAX_CLICKS, kWords = kResult + (3 * E3D_LOCALIZE_MAX_CLICKS * sizeof(float) + 7) / 8;
  h->scan.pick_words.reserve(kWords); h->scan.pick_clicks.reserve(E3D_LOCALIZE_MAX_CLICKS);
  copy_in(h->scan.pick_clicks.p, clicks_xy, sizeof(float2) * n_clicks, h->stream);
  E3D_HIP(hipMemsetAsync(h->scan.pick_words.p, 0, sizeof(unsigned long long), h->stream));
  E3D_HIP(hipMemsetAsync(h->scan.pick_words.p + kKeys, 0xFF, sizeof(unsigned long long) * E3D_LOCALIZE_MAX_CLICKS, h->stream));      // kPickNone
  float* result = reinterpret_cast<float*>(h->scan.pick_words.p + kResult);
  if (n) {
    render_depth(h, image_id, in.min_image_scale, nullptr);         // as the label transfer renders it for its source image
    int group = 1;
    while (group < n_clicks) group *= 2;
    const unsigned blocks = std::min<unsigned>(nblk(n), kPickMaxBlocks);
    KT kt(h, "localize.pick", (double)n);
    E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_pick_scan_points<M>, dim3(blocks), dim3(kBlock), 0, h->stream, h->scan.scan_pts.p, n, im.pose, cam,
                                               im.depth.p, h->prm.occlusion_depth_threshold, h->scan.pick_clicks.p, n_clicks, group,
                                               h->scan.pick_words.p + kKeys, h->scan.pick_words.p));
  }
  E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_pick_finish<M>, dim3(1), dim3(kWave), 0, h->stream, h->scan.scan_pts.p, im.pose, cam, im.depth.p,
                                             h->prm.occlusion_depth_threshold, h->scan.pick_clicks.p, n_clicks, h->scan.pick_words.p + kKeys, result));
  unsigned long long words[kWords];
  read_back(h, words, h->scan.pick_words.p, sizeof words);
  E3D_HIP(hipGetLastError());
  const float* r = reinterpret_cast<const float*>(words + kResult);
  for (int c = 0; c < n_clicks; ++c) {
    index_out[c] = words[kKeys + c] == kPickNone ? -1 : (int64_t)(words[kKeys + c] & 0xffffffffull);
    if (pixel_out) { pixel_out[2 * c] = r[3 * c]; pixel_out[2 * c + 1] = r[3 * c + 1]; }
    if (distance_out) distance_out[c] = r[3 * c + 2];
  }
  return (int64_t)words[0];
  E3D_CATCH()
}

int e3d_reg_image_bearings(e3d_reg_t* h, int image_id, const float* pixels_xy, int n, double* bearings_out) {
  E3D_TRY_ON(h)
  if (!h || (n > 0 && (!pixels_xy || !bearings_out))) throw Error(E3D_ERR_INVALID, "null argument");
  if (n < 0) throw Error(E3D_ERR_INVALID, "negative count");
  ImageDev& im = owned_image(h, image_id);
  if (n == 0) return 0;
  const Intrin& in = h->intr.at(im.intrinsics_id);
  const CamLevel& cam = in.levels[0];
  h->scan.localize_in.reserve(2 * (size_t)n); h->scan.localize_out.reserve(2 * (size_t)n);
  copy_in(h->scan.localize_in.p, pixels_xy, sizeof(float) * 2 * n, h->stream);
  E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_image_bearings<M>, dim3(nblk(n)), dim3(kBlock), 0, h->stream, cam,
                                             reinterpret_cast<const float2*>(h->scan.localize_in.p), n, reinterpret_cast<float2*>(h->scan.localize_out.p)));
  std::vector<float> nxy(2 * (size_t)n);
  copy_out(nxy.data(), h->scan.localize_out.p, sizeof(float) * nxy.size(), h->stream);
  rsync(h);
  E3D_HIP(hipGetLastError());
  for (int i = 0; i < n; ++i) {                       // Vector3d(nxy.x, nxy.y, 1).normalized()
    const double x = nxy[2 * i], y = nxy[2 * i + 1];
    const double norm = std::sqrt(x * x + y * y + 1.0);
    bearings_out[3 * i] = x / norm; bearings_out[3 * i + 1] = y / norm; bearings_out[3 * i + 2] = 1.0 / norm;
  }
  return 0;
  E3D_CATCH()
}

int e3d_reg_project_points(e3d_reg_t* h, int image_id, const float* xyz, size_t n, float* pixel_out, uint8_t* state_out) {
  E3D_TRY_ON(h)
  if (!h || (n > 0 && (!xyz || !pixel_out || !state_out))) throw Error(E3D_ERR_INVALID, "null argument");
  ImageDev& im = owned_image(h, image_id);
  if (n == 0) return 0;
  const Intrin& in = h->intr.at(im.intrinsics_id);
  const CamLevel& cam = in.levels[0];
  h->scan.localize_in.reserve(3 * n); h->scan.localize_out.reserve(2 * n); h->scan.localize_state.reserve(n);
  copy_in(h->scan.localize_in.p, xyz, sizeof(float) * 3 * n, h->stream);
  render_depth(h, image_id, in.min_image_scale, nullptr);
  E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_project_points<M>, dim3(nblk(n)), dim3(kBlock), 0, h->stream, h->scan.localize_in.p, n, im.pose, cam,
                                             im.depth.p, h->prm.occlusion_depth_threshold, reinterpret_cast<float2*>(h->scan.localize_out.p),
                                             h->scan.localize_state.p));
  copy_out(pixel_out, h->scan.localize_out.p, sizeof(float) * 2 * n, h->stream);
  copy_out(state_out, h->scan.localize_state.p, n, h->stream);
  rsync(h);
  E3D_HIP(hipGetLastError());
  return 0;
  E3D_CATCH()
}

// ---- ImageUndistorter -----------------------------------------------------------------------------------------------------------------
static const Intrin& undistort_intrinsics(e3d_reg* h, int intrinsics_id) {
  auto it = h->intr.find(intrinsics_id);
  if (it == h->intr.end()) throw Error(E3D_ERR_INDEX, fmt("no intrinsics with id %d (e3d_reg_set_intrinsics)", intrinsics_id));
  return it->second;
}

// the border samples of a level-0 model: ImageToNormalized of the pixel centres (0, y), (W - 1, y) of every row, then (x, 0), (x, H - 1)
// of every column, in that order (2 H + 2 W values)
static std::vector<float2> undistort_border_samples(e3d_reg* h, const Intrin& in) {
  const CamLevel& cam = in.levels[0];
  const int W = cam.width, H = cam.height, n = 2 * W + 2 * H;
  std::vector<float2> px((size_t)n);
  for (int y = 0; y < H; ++y) { px[2 * y] = make_float2(0.f, (float)y); px[2 * y + 1] = make_float2((float)(W - 1), (float)y); }
  for (int x = 0; x < W; ++x) { px[2 * H + 2 * x] = make_float2((float)x, 0.f); px[2 * H + 2 * x + 1] = make_float2((float)x, (float)(H - 1)); }
  h->scan.undistort_border.reserve(2 * (size_t)n);
  copy_in(h->scan.undistort_border.p, px.data(), sizeof(float2) * n, h->stream);
  E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_image_bearings<M>, dim3(nblk(n)), dim3(kBlock), 0, h->stream, cam, h->scan.undistort_border.p, n,
                                             h->scan.undistort_border.p + n));
  std::vector<float2> nxy((size_t)n);
  copy_out(nxy.data(), h->scan.undistort_border.p + n, sizeof(float2) * n, h->stream);
  rsync(h);
  E3D_HIP(hipGetLastError());
  return nxy;
}
// ... dealt out to the four sides {left, right, top, bottom} (appended: the stereo plan unites two cameras' samples)
static void undistort_append_sides(const std::vector<float2>& nxy, int W, int H, std::vector<float2> sides[4]) {
  for (int y = 0; y < H; ++y) { sides[0].push_back(nxy[2 * (size_t)y]); sides[1].push_back(nxy[2 * (size_t)y + 1]); }
  for (int x = 0; x < W; ++x) { sides[2].push_back(nxy[2 * (size_t)H + 2 * x]); sides[3].push_back(nxy[2 * (size_t)H + 2 * x + 1]); }
}

// the plan rule from the samples of the four sides and the focal lengths (include/e3d_hip.h, e3d_reg_undistort_plan)
static void undistort_plan_from_sides(const std::vector<float2> sides[4], float cam_fx, float cam_fy, double blank_pixels, int max_image_size,
                                      e3d_undistort_plan* out) {
  // per side: inner and outer extent of one coordinate of its samples
  struct Side { double in, out; int count = 0; };
  auto extent = [&](const std::vector<float2>& samples, bool x_coordinate, bool low_side) {
    Side s{low_side ? -INFINITY : INFINITY, low_side ? INFINITY : -INFINITY};
    for (const float2 v : samples) {
      if (!std::isfinite(v.x) || !std::isfinite(v.y)) {
        if (blank_pixels > 0.0)
          throw Error(E3D_ERR_INVALID, "a border pixel has no finite undistorted position (beyond the model's radius cut-off): "
                                       "only blank_pixels = 0 is possible for this camera");
        continue;
      }
      const double c = x_coordinate ? (double)v.x : (double)v.y;
      if (low_side) { s.in = std::max(s.in, c); s.out = std::min(s.out, c); }
      else { s.in = std::min(s.in, c); s.out = std::max(s.out, c); }
      ++s.count;
    }
    if (!s.count) throw Error(E3D_ERR_INVALID, "no border pixel of one image side has a finite undistorted position");
    return s;
  };
  const Side L = extent(sides[0], true, true), R = extent(sides[1], true, false);
  const Side T = extent(sides[2], false, true), B = extent(sides[3], false, false);
  const double b = blank_pixels;
  const double nL = b * L.out + (1.0 - b) * L.in, nR = b * R.out + (1.0 - b) * R.in;
  const double nT = b * T.out + (1.0 - b) * T.in, nB = b * B.out + (1.0 - b) * B.in;
  if (!(nL < nR) || !(nT < nB)) throw Error(E3D_ERR_INVALID, "the undistorted image is empty: its left / top extent is not below its right / bottom one");
  // a blended bound may lie up to b pixels outside its extent (the outer bounds are rounded outwards): 2 b pixels of margin
  double s = 1.0;
  const double extent_px = std::max((double)cam_fx * (nR - nL), (double)cam_fy * (nB - nT)), margin = 1.0 + 2.0 * b;
  if (max_image_size > 0 && extent_px + margin > (double)max_image_size) {
    s = ((double)max_image_size - margin) / extent_px;
    if (!(s > 0.0)) throw Error(E3D_ERR_INVALID, fmt("max_image_size = %d leaves no room for an image", max_image_size));
  }
  const float fx = (float)(s * (double)cam_fx), fy = (float)(s * (double)cam_fy);
  // inner bounds rounded inwards, outer bounds outwards, blended as integers
  auto low_bound = [&](double f, const Side& e) { return std::ceil(b * std::floor(f * e.out) + (1.0 - b) * std::ceil(f * e.in)); };
  auto high_bound = [&](double f, const Side& e) { return std::floor(b * std::ceil(f * e.out) + (1.0 - b) * std::floor(f * e.in)); };
  const double x0 = low_bound((double)fx, L), x1 = high_bound((double)fx, R);
  const double y0 = low_bound((double)fy, T), y1 = high_bound((double)fy, B);
  const double Wd = x1 - x0 + 1.0, Hd = y1 - y0 + 1.0;
  if (!(Wd >= 2.0) || !(Hd >= 2.0)) throw Error(E3D_ERR_INVALID, "the undistorted image would be smaller than 2 x 2 pixels");
  constexpr double kLimit = 16777216.0;          // integers a float holds exactly (the principal point)
  if (!(std::fabs(x0) < kLimit && std::fabs(y0) < kLimit && Wd < kLimit && Hd < kLimit))
    throw Error(E3D_ERR_INVALID, "the undistorted image would be larger than 2^24 pixels a side");
  out->width = (int32_t)Wd; out->height = (int32_t)Hd;
  out->fx = fx; out->fy = fy; out->cx = (float)(-x0); out->cy = (float)(-y0);
}

int e3d_reg_undistort_plan(e3d_reg_t* h, int intrinsics_id, double blank_pixels, int max_image_size, e3d_undistort_plan* out) {
  E3D_TRY_ON(h)
  if (!h || !out) throw Error(E3D_ERR_INVALID, "null argument");
  if (!(blank_pixels >= 0.0 && blank_pixels <= 1.0)) throw Error(E3D_ERR_INVALID, fmt("blank_pixels = %g is outside [0, 1]", blank_pixels));
  const Intrin& in = undistort_intrinsics(h, intrinsics_id);
  const CamLevel& cam = in.levels[0];
  std::vector<float2> sides[4];
  undistort_append_sides(undistort_border_samples(h, in), cam.width, cam.height, sides);
  undistort_plan_from_sides(sides, cam.fx, cam.fy, blank_pixels, max_image_size, out);
  return 0;
  E3D_CATCH()
}

// one image through a plan: e3d_reg_undistort (S null) and e3d_reg_stereo_rectify (S: the 9 entries of source_T_rect)
static void undistort_resample(e3d_reg* h, int intrinsics_id, const e3d_undistort_plan* plan, const float* S, int kind, const void* src, void* dst,
                               uint8_t* valid_out) {
  if (kind < 0 || kind >= kNumUndistortKinds) throw Error(E3D_ERR_INVALID, "unknown kind (0 = u8, 1 = u8 x 3, 2 = mask, 3 = f32 nearest)");
  const Intrin& in = undistort_intrinsics(h, intrinsics_id);
  const CamLevel& cam = in.levels[0];
  if (plan->width < 1 || plan->height < 1 || plan->width > (1 << 24) || plan->height > 65535 * 4 || !(plan->fx > 0.f) || !(plan->fy > 0.f) ||
      !std::isfinite(plan->fx) || !std::isfinite(plan->fy) || !std::isfinite(plan->cx) || !std::isfinite(plan->cy))
    throw Error(E3D_ERR_INVALID, S ? "bad plan (e3d_reg_stereo_plan fills it)" : "bad plan (e3d_reg_undistort_plan fills it)");
  StereoRotation rotation{};
  if (S)
    for (int k = 0; k < 9; ++k) {
      if (!std::isfinite(S[k])) throw Error(E3D_ERR_INVALID, "the rotation S has an entry that is not finite");
      rotation.m[k] = S[k];
    }
  const size_t px_bytes = undistort_pixel_bytes(kind);
  const size_t n_src = (size_t)cam.width * (size_t)cam.height, n_dst = (size_t)plan->width * (size_t)plan->height;
  h->scan.undistort_src.reserve(n_src * px_bytes); h->scan.undistort_dst.reserve(n_dst * px_bytes);
  if (valid_out) h->scan.undistort_valid.reserve(n_dst);
  copy_in(h->scan.undistort_src.p, src, n_src * px_bytes, h->stream);
  std::unique_ptr<EventTimer>& timer = S ? h->scan.t_stereo : h->scan.t_undistort;
  if (!timer) timer.reset(new EventTimer());
  const UndistortTarget target{plan->width, plan->height, plan->fx, plan->fy, plan->cx, plan->cy};
  uint8_t* valid = valid_out ? h->scan.undistort_valid.p : nullptr;
  timer->start(h->stream);
  if (S) rectify_launch(cam, target, rotation, kind, h->scan.undistort_src.p, h->scan.undistort_dst.p, valid, h->stream);
  else undistort_launch(cam, target, kind, h->scan.undistort_src.p, h->scan.undistort_dst.p, valid, h->stream);
  timer->stop(h->stream);
  copy_out(dst, h->scan.undistort_dst.p, n_dst * px_bytes, h->stream);
  if (valid_out) copy_out(valid_out, h->scan.undistort_valid.p, n_dst, h->stream);
  rsync(h);
  E3D_HIP(hipGetLastError());
  (S ? h->scan.stereo_ms : h->scan.undistort_ms) = timer->ms();
}

int e3d_reg_undistort(e3d_reg_t* h, int intrinsics_id, const e3d_undistort_plan* plan, int kind, const void* src, void* dst, uint8_t* valid_out) {
  E3D_TRY_ON(h)
  if (!h || !plan || !src || !dst) throw Error(E3D_ERR_INVALID, "null argument");
  undistort_resample(h, intrinsics_id, plan, nullptr, kind, src, dst, valid_out);
  return 0;
  E3D_CATCH()
}

int e3d_reg_undistort_kernel_ms(e3d_reg_t* h, float* ms) {
  E3D_TRY_ON(h)
  if (!h || !ms) throw Error(E3D_ERR_INVALID, "null argument");
  *ms = h->scan.undistort_ms;
  return 0;
  E3D_CATCH()
}

// ---- e3d_pose_from_bearings: host only ---------------------------------------------------------------------------------------------------
namespace {
struct BearingPose { double R[9], t[3]; };
void quat_to_rotation(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}
void rotation_to_quat(const double R[9], double q[4]) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0) {
    const double s = std::sqrt(tr + 1.0) * 2;
    q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
    q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
    q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
    q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
  }
  const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sign = q[0] < 0 ? -1.0 : 1.0;
  for (int k = 0; k < 4; ++k) q[k] = sign * q[k] / norm;
}
// exp of a rotation vector (Rodrigues), the series near 0
void rotation_exp(const double w[3], double E[9]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
  const double a = th < 1e-8 ? 1.0 - th2 / 6 : std::sin(th) / th, b = th < 1e-8 ? 0.5 - th2 / 24 : (1 - std::cos(th)) / th2;
  const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double kk = 0;
      for (int k = 0; k < 3; ++k) kk += K[3 * r + k] * K[3 * k + c];
      E[3 * r + c] = (r == c ? 1.0 : 0.0) + a * K[3 * r + c] + b * kk;
    }
}
// d_i = (R p_i + t) / |R p_i + t|; cost = sum |f_i - d_i|^2 and, on request, the mean squared angle between f_i and d_i
double bearing_cost(const BearingPose& T, const double* p, const double* f, int n, double* mean_squared_angle) {
  double cost = 0, angles = 0;
  for (int i = 0; i < n; ++i) {
    double x[3], d[3];
    for (int r = 0; r < 3; ++r) x[r] = T.R[3 * r] * p[3 * i] + T.R[3 * r + 1] * p[3 * i + 1] + T.R[3 * r + 2] * p[3 * i + 2] + T.t[r];
    const double len = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    for (int r = 0; r < 3; ++r) { d[r] = x[r] / len; const double e = f[3 * i + r] - d[r]; cost += e * e; }
    const double* g = f + 3 * i;
    const double cx = g[1] * d[2] - g[2] * d[1], cy = g[2] * d[0] - g[0] * d[2], cz = g[0] * d[1] - g[1] * d[0];
    const double angle = std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), g[0] * d[0] + g[1] * d[1] + g[2] * d[2]);
    angles += angle * angle;
  }
  if (mean_squared_angle) *mean_squared_angle = angles / n;
  return cost;
}
// A = L D L^T without pivoting, in place (L below the diagonal, D on it); false where a pivot is not above min_ratio * the diagonal
// entry it started from
bool ldlt6(double A[36], double min_ratio) {
  for (int j = 0; j < 6; ++j) {
    const double start = A[7 * j];
    double d = start;
    for (int k = 0; k < j; ++k) d -= A[6 * j + k] * A[6 * j + k] * A[7 * k];
    if (!(d > min_ratio * start) || !std::isfinite(d)) return false;
    A[7 * j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[6 * i + j];
      for (int k = 0; k < j; ++k) v -= A[6 * i + k] * A[6 * j + k] * A[7 * k];
      A[6 * i + j] = v / d;
    }
  }
  return true;
}
void ldlt6_solve(const double A[36], double x[6]) {
  for (int i = 0; i < 6; ++i) for (int k = 0; k < i; ++k) x[i] -= A[6 * i + k] * x[k];
  for (int i = 0; i < 6; ++i) x[i] /= A[7 * i];
  for (int i = 5; i >= 0; --i) for (int k = i + 1; k < 6; ++k) x[i] -= A[6 * k + i] * x[k];
}
}  // namespace

int e3d_pose_from_bearings(const double* points, const double* bearings, int n, const float q_in[4], const float t_in[3], float q_out[4],
                           float t_out[3], double stats[4]) {
  E3D_TRY
  if (!points || !bearings || !q_in || !t_in || !q_out || !t_out) throw Error(E3D_ERR_INVALID, "null argument");
  if (n < 6) throw Error(E3D_ERR_INVALID, fmt("%d correspondences: at least 6 are required", n));
  bool finite = true;
  for (int i = 0; i < 3 * n; ++i) finite = finite && std::isfinite(points[i]) && std::isfinite(bearings[i]);
  for (int k = 0; k < 4; ++k) finite = finite && std::isfinite(q_in[k]);
  for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(t_in[k]);
  double q[4] = {q_in[0], q_in[1], q_in[2], q_in[3]};
  const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!finite || !(qn > 0)) throw Error(E3D_ERR_INVALID, "a point, a bearing or the start pose is not finite");
  for (int k = 0; k < 4; ++k) q[k] /= qn;
  BearingPose T;
  quat_to_rotation(q, T.R);
  for (int k = 0; k < 3; ++k) T.t[k] = t_in[k];
  double msa_before = 0, msa_after = 0;
  double cost = bearing_cost(T, points, bearings, n, &msa_before);
  double lambda = 1e-4;
  int iterations = 0;
  bool converged = false;
  while (iterations < 100 && !converged) {
    ++iterations;
    // residual r_i = f_i - d_i(x), x = R p_i + t; the perturbation x -> exp(w) x + v gives dx = [-[x]x | I] (w, v) and
    // dd/dx = (I - d d^T) / |x|, so J_i = -(I - d d^T) / |x| * [-[x]x | I]
    double H[36] = {0}, g[6] = {0};
    for (int i = 0; i < n; ++i) {
      double x[3], d[3], res[3];
      for (int r = 0; r < 3; ++r) x[r] = T.R[3 * r] * points[3 * i] + T.R[3 * r + 1] * points[3 * i + 1] + T.R[3 * r + 2] * points[3 * i + 2] + T.t[r];
      const double len = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
      for (int r = 0; r < 3; ++r) { d[r] = x[r] / len; res[r] = bearings[3 * i + r] - d[r]; }
      const double dx[3][6] = {{0, x[2], -x[1], 1, 0, 0}, {-x[2], 0, x[0], 0, 1, 0}, {x[1], -x[0], 0, 0, 0, 1}};
      double J[3][6];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 6; ++c) {
          double v = 0;
          for (int k = 0; k < 3; ++k) v += ((r == k ? 1.0 : 0.0) - d[r] * d[k]) * dx[k][c];
          J[r][c] = -v / len;
        }
      for (int a = 0; a < 6; ++a) {
        for (int r = 0; r < 3; ++r) g[a] += J[r][a] * res[r];
        for (int b = 0; b < 6; ++b)
          for (int r = 0; r < 3; ++r) H[6 * a + b] += J[r][a] * J[r][b];
      }
    }
    double check[36];
    memcpy(check, H, sizeof H);
    if (!ldlt6(check, 1e-10)) throw Error(E3D_ERR_INVALID, "the correspondences do not determine the pose (LDLT of the normal matrix failed)");
    // damped steps until one lowers the cost or the step is below the stopping length
    for (;;) {
      double A[36], step[6];
      memcpy(A, H, sizeof H);
      for (int k = 0; k < 6; ++k) { A[7 * k] += lambda * H[7 * k]; step[k] = -g[k]; }
      if (!ldlt6(A, 0.0)) throw Error(E3D_ERR_INVALID, "LDLT of the damped normal matrix failed");
      ldlt6_solve(A, step);
      double norm = 0;
      for (int k = 0; k < 6; ++k) norm += step[k] * step[k];
      if (std::sqrt(norm) < 1e-12) { converged = true; break; }
      BearingPose N;
      double E[9];
      rotation_exp(step, E);
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) N.R[3 * r + c] = E[3 * r] * T.R[c] + E[3 * r + 1] * T.R[3 + c] + E[3 * r + 2] * T.R[6 + c];
        N.t[r] = E[3 * r] * T.t[0] + E[3 * r + 1] * T.t[1] + E[3 * r + 2] * T.t[2] + step[3 + r];
      }
      const double new_cost = bearing_cost(N, points, bearings, n, nullptr);
      if (new_cost < cost) { T = N; cost = new_cost; lambda = std::max(lambda * 0.1, 1e-15); break; }
      lambda *= 10;
      if (lambda > 1e15) { converged = true; break; }        // no step lowers the cost any more: a minimum to rounding
    }
  }
  bearing_cost(T, points, bearings, n, &msa_after);
  double qo[4];
  rotation_to_quat(T.R, qo);
  for (int k = 0; k < 4; ++k) q_out[k] = (float)qo[k];
  for (int k = 0; k < 3; ++k) t_out[k] = (float)T.t[k];
  if (stats) { stats[0] = std::sqrt(msa_before); stats[1] = std::sqrt(msa_after); stats[2] = iterations; stats[3] = converged ? 1.0 : 0.0; }
  return 0;
  E3D_CATCH()
}

// ---- StereoPairCreator (include/e3d_hip.h states the three rules) -----------------------------------------------------------
namespace {
// image_T_global of an image in f64: the rotation of its renormalised quaternion, row-major, and the camera centre C = -R^T t
struct StereoView { double R[9], C[3]; };
StereoView stereo_view(const ImageDev& im) {
  double w = im.pose_q.q.w, x = im.pose_q.q.x, y = im.pose_q.q.y, z = im.pose_q.q.z;
  const double n = std::sqrt(w * w + x * x + y * y + z * z);
  if (!(n > 0.0) || !std::isfinite(n)) throw Error(E3D_ERR_INVALID, "an image pose is not finite");
  w /= n; x /= n; y /= n; z /= n;
  StereoView v;
  quat_to_matrix<double>(w, x, y, z, v.R);
  const double t[3] = {im.pose_q.t[0], im.pose_q.t[1], im.pose_q.t[2]};
  for (int k = 0; k < 3; ++k) v.C[k] = -(v.R[k] * t[0] + v.R[3 + k] * t[1] + v.R[6 + k] * t[2]);
  return v;
}
void cross3(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
}  // namespace

int e3d_reg_stereo_plan(e3d_reg_t* h, int left_image_id, int right_image_id, double blank_pixels, int max_image_size, double focal_length,
                        e3d_stereo_plan* out) {
  E3D_TRY_ON(h)
  if (!h || !out) throw Error(E3D_ERR_INVALID, "null argument");
  if (!(blank_pixels >= 0.0 && blank_pixels <= 1.0)) throw Error(E3D_ERR_INVALID, fmt("blank_pixels = %g is outside [0, 1]", blank_pixels));
  const ImageDev* im[2] = {&get_image(h, left_image_id), &get_image(h, right_image_id)};
  const Intrin* in[2] = {&h->intr.at(im[0]->intrinsics_id), &h->intr.at(im[1]->intrinsics_id)};
  const StereoView v[2] = {stereo_view(*im[0]), stereo_view(*im[1])};
  // the rectified frame: x along the baseline, z the part of the mean optical axis at right angles to it
  const double b[3] = {v[1].C[0] - v[0].C[0], v[1].C[1] - v[0].C[1], v[1].C[2] - v[0].C[2]};
  const double B = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  if (!std::isfinite(B) || B < 1e-9) throw Error(E3D_ERR_INVALID, "the two images have the same camera centre: no baseline");
  const double ex[3] = {b[0] / B, b[1] / B, b[2] / B};
  const double zs[3] = {v[0].R[6] + v[1].R[6], v[0].R[7] + v[1].R[7], v[0].R[8] + v[1].R[8]};
  double c[3];
  cross3(zs, ex, c);
  const double nc = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), nzs = std::sqrt(zs[0] * zs[0] + zs[1] * zs[1] + zs[2] * zs[2]);
  if (!(nc >= 1e-6 * nzs) || !(nc > 0.0)) throw Error(E3D_ERR_INVALID, "the cameras look along the baseline: the pair cannot be rectified");
  const double ey[3] = {c[0] / nc, c[1] / nc, c[2] / nc};
  double ez[3];
  cross3(ex, ey, ez);
  const double ys[3] = {v[0].R[3] + v[1].R[3], v[0].R[4] + v[1].R[4], v[0].R[5] + v[1].R[5]};
  if (!(dot3(ey, ys) > 0.0))
    throw Error(E3D_ERR_INVALID, "the pair is given right-then-left (the rectified images would be upside down): swap the two images");
  for (int i = 0; i < 2; ++i)
    if (!(dot3(ez, v[i].R + 6) > 0.0)) throw Error(E3D_ERR_INVALID, "a camera looks away from the rectified viewing direction");
  const double Rr[9] = {ex[0], ex[1], ex[2], ey[0], ey[1], ey[2], ez[0], ez[1], ez[2]};
  e3d_stereo_plan plan{};
  float* S[2] = {plan.S_left, plan.S_right};
  for (int i = 0; i < 2; ++i)
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k)
        S[i][3 * r + k] = (float)(v[i].R[3 * r] * Rr[3 * k] + v[i].R[3 * r + 1] * Rr[3 * k + 1] + v[i].R[3 * r + 2] * Rr[3 * k + 2]);
  double q[4];
  rotation_to_quat(Rr, q);
  for (int k = 0; k < 4; ++k) plan.q_rect[k] = (float)q[k];
  for (int k = 0; k < 3; ++k) {
    const double tl = -(Rr[3 * k] * v[0].C[0] + Rr[3 * k + 1] * v[0].C[1] + Rr[3 * k + 2] * v[0].C[2]);
    plan.t_left[k] = (float)tl;
    plan.t_right[k] = (float)(k == 0 ? tl - B : tl);
  }
  plan.baseline = (float)B;
  double fd = focal_length;
  if (!(fd > 0.0)) fd = (((double)in[0]->levels[0].fx + (double)in[0]->levels[0].fy) + ((double)in[1]->levels[0].fx + (double)in[1]->levels[0].fy)) / 4.0;
  const float f = (float)fd;
  if (!(f > 0.f) || !std::isfinite(f)) throw Error(E3D_ERR_INVALID, "the focal length of the rectified camera is not positive and finite");
  // window: both cameras' border samples rotated into the rectified frame, r = S^T (nx, ny, 1) in f64 with the rounded S, united per side
  std::vector<float2> sides[4];
  for (int i = 0; i < 2; ++i) {
    const CamLevel& cam = in[i]->levels[0];
    std::vector<float2> nxy = undistort_border_samples(h, *in[i]);
    const float* s = S[i];
    for (float2& p : nxy) {
      const double nx = p.x, ny = p.y;
      const double rx = (double)s[0] * nx + (double)s[3] * ny + (double)s[6];
      const double ry = (double)s[1] * nx + (double)s[4] * ny + (double)s[7];
      const double rz = (double)s[2] * nx + (double)s[5] * ny + (double)s[8];
      const double u = rx / rz, w = ry / rz;
      if (rz > 0.0 && std::isfinite(u) && std::isfinite(w)) p = make_float2((float)u, (float)w);
      else p = make_float2(NAN, NAN);             // behind the rectified image plane, or no finite position in its own camera
    }
    undistort_append_sides(nxy, cam.width, cam.height, sides);
  }
  undistort_plan_from_sides(sides, f, f, blank_pixels, max_image_size, &plan.camera);
  *out = plan;
  return 0;
  E3D_CATCH()
}

int e3d_reg_stereo_rectify(e3d_reg_t* h, int intrinsics_id, const e3d_undistort_plan* target, const float S[9], int kind, const void* src, void* dst,
                           uint8_t* valid_out) {
  E3D_TRY_ON(h)
  if (!h || !target || !S || !src || !dst) throw Error(E3D_ERR_INVALID, "null argument");
  undistort_resample(h, intrinsics_id, target, S, kind, src, dst, valid_out);
  return 0;
  E3D_CATCH()
}

int e3d_reg_stereo_kernel_ms(e3d_reg_t* h, float* ms) {
  E3D_TRY_ON(h)
  if (!h || !ms) throw Error(E3D_ERR_INVALID, "null argument");
  *ms = h->scan.stereo_ms;
  return 0;
  E3D_CATCH()
}

int e3d_reg_stereo_ground_truth(e3d_reg_t* h, int left_rect_image_id, int right_rect_image_id, const uint8_t* left_excluded,
                                const uint8_t* right_excluded, float* disparity, uint8_t* nocc_mask, float* depth) {
  E3D_TRY_ON(h)
  if (!h || !disparity || !nocc_mask) throw Error(E3D_ERR_INVALID, "null argument");
  if (!h->scan.scan_points_set) throw Error(E3D_ERR_INVALID, "no scan points set (e3d_reg_set_scan_points)");
  ImageDev& left = owned_image(h, left_rect_image_id);
  ImageDev& right = owned_image(h, right_rect_image_id);
  if (left.intrinsics_id != right.intrinsics_id) throw Error(E3D_ERR_INVALID, "the two rectified images do not share their intrinsics");
  const Intrin& in = h->intr.at(left.intrinsics_id);
  const CamLevel& cam = in.levels[0];
  if (in.type != kPinhole || cam.fx != cam.fy) throw Error(E3D_ERR_INVALID, "the rectified camera is not PINHOLE with fx == fy");
  if (memcmp(&left.pose_q.q, &right.pose_q.q, sizeof(Quatf)) != 0)
    throw Error(E3D_ERR_INVALID, "the rotations of the two rectified images differ");
  if (memcmp(&left.pose_q.t[1], &right.pose_q.t[1], 2 * sizeof(float)) != 0)
    throw Error(E3D_ERR_INVALID, "the y or z translations of the two rectified images differ: the pair is not rectified");
  const double B = (double)left.pose_q.t[0] - (double)right.pose_q.t[0];
  if (!(B > 0.0) || !std::isfinite(B)) throw Error(E3D_ERR_INVALID, "the baseline t_left.x - t_right.x is not positive (are the images swapped?)");
  const size_t px = (size_t)cam.width * cam.height, n = h->scan.n_scan;
  h->scan.eval_mask.reserve(px); h->scan.gt_depth.reserve(px); h->scan.stereo_d2.reserve(px);
  h->scan.stereo_disparity.reserve(px); h->scan.stereo_nocc.reserve(px);
  if (n) E3D_HIP(hipMemsetAsync(h->scan.scan_counts.p, 0, sizeof(int) * n, h->stream));
  // Each image's occlusion depth is rendered once and stays in im.depth.  One mask buffer serves both images: the right image is
  // counted first (the counters do not depend on the order), the left image's mask then stays for its two depth maps.
  auto count = [&](ImageDev& im, int image_id, const uint8_t* excluded) {
    render_depth(h, image_id, in.min_image_scale, nullptr);
    if (excluded) { copy_in(h->scan.eval_mask.p, excluded, px, h->stream); stereo_normalize_mask_launch(h->scan.eval_mask.p, px, h->stream); }
    launch_scan_visibility(h, im, in, excluded ? h->scan.eval_mask.p : nullptr, 1, 0, 0, h->scan.gt_depth.p);
  };
  count(right, right_rect_image_id, right_excluded);
  count(left, left_rect_image_id, left_excluded);
  const unsigned char* left_mask = left_excluded ? h->scan.eval_mask.p : nullptr;
  fill_f32(reinterpret_cast<float*>(h->scan.gt_depth.p), px, INFINITY, h->stream);
  launch_scan_visibility(h, left, in, left_mask, 1, 1, 1, h->scan.gt_depth.p);           // D1: the nearest point the left image sees
  fill_f32(reinterpret_cast<float*>(h->scan.stereo_d2.p), px, INFINITY, h->stream);
  launch_scan_visibility(h, left, in, left_mask, 1, 1, 2, h->scan.stereo_d2.p);          // D2: the nearest point both see
  stereo_disparity_launch(h->scan.gt_depth.p, h->scan.stereo_d2.p, px, cam.fx, B, h->scan.stereo_disparity.p, h->scan.stereo_nocc.p, h->stream);
  copy_out(disparity, h->scan.stereo_disparity.p, sizeof(float) * px, h->stream);
  copy_out(nocc_mask, h->scan.stereo_nocc.p, px, h->stream);
  if (depth) copy_out(depth, h->scan.gt_depth.p, sizeof(float) * px, h->stream);
  rsync(h);
  E3D_HIP(hipGetLastError());
  return 0;
  E3D_CATCH()
}

// ---- debug point clouds (Problem::DebugWriteColoredPointCloud, src/opt/problem.cc:642-704) ---------------------------------------
int e3d_reg_scan_colors_begin(e3d_reg_t* h) {
  E3D_TRY_ON(h)
  if (!h) throw Error(E3D_ERR_INVALID, "null handle");
  if (!h->scan.scan_points_set) throw Error(E3D_ERR_INVALID, "no scan points set (e3d_reg_set_scan_points)");
  h->scan.scan_color_acc.reserve(h->scan.n_scan);
  if (h->scan.n_scan) E3D_HIP(hipMemsetAsync(h->scan.scan_color_acc.p, 0, sizeof(float4) * h->scan.n_scan, h->stream));     // 0.f sums, count 0
  rsync(h);
  h->scan.scan_colors_begun = true;
  return 0;
  E3D_CATCH()
}
int e3d_reg_scan_colors_add_image(e3d_reg_t* h, int image_id, const uint8_t* rgb, int width, int height) {
  E3D_TRY_ON(h)
  if (!h || !rgb) throw Error(E3D_ERR_INVALID, "null argument");
  if (width < 2 || height < 2) throw Error(E3D_ERR_INVALID, "a colour image needs at least 2 x 2 pixels for a bilinear sample");
  if (!h->scan.scan_points_set) throw Error(E3D_ERR_INVALID, "no scan points set (e3d_reg_set_scan_points)");
  if (!h->scan.scan_colors_begun) throw Error(E3D_ERR_INVALID, "call e3d_reg_scan_colors_begin first");
  ImageDev& im = owned_image(h, image_id);
  if (h->scan.n_scan == 0) return 0;
  const Intrin& in = h->intr.at(im.intrinsics_id);
  if (im.pix.size() != in.levels.size()) throw Error(E3D_ERR_INVALID, fmt("image %d was set without pixels", image_id));
  const int scale = best_available_scale(h, in);
  render_depth(h, image_id, scale, nullptr);
  const int lvl = std::max(0, scale - in.min_image_scale);
  const CamLevel& cam = in.levels[lvl];
  const size_t bytes = (size_t)width * height * 3;
  h->scan.scan_color_image.reserve(bytes);
  copy_in(h->scan.scan_color_image.p, rgb, bytes, h->stream);
  RadiusParams rp{};
  rp.image_scale = scale; rp.min_image_scale = in.min_image_scale;
  rp.occlusion_threshold = h->prm.occlusion_depth_threshold; rp.max_valid_intensity = h->prm.maximum_valid_intensity;
  {
    KT kt(h, "debug.scan_colors", (double)h->scan.n_scan);
    E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_scan_colors<M>, dim3(nblk(h->scan.n_scan)), dim3(kBlock), 0, h->stream, h->scan.scan_pts.p, h->scan.n_scan,
                                               im.pose, cam, im.pix[lvl].p, im.has_mask[lvl] ? im.mask[lvl].p : nullptr,
                                               (in.cam_mask && lvl < (int)in.cam_mask->size()) ? (*in.cam_mask)[lvl].p : nullptr, im.depth.p, rp,
                                               h->scan.scan_color_image.p, width, height, h->scan.scan_color_acc.p));
  }
  rsync(h);                          // (the caller's pixels may go away after the call)
  E3D_HIP(hipGetLastError());
  return 0;
  E3D_CATCH()
}
int e3d_reg_scan_colors_get_sums(e3d_reg_t* h, float* sums, int32_t* counts) {
  E3D_TRY_ON(h)
  if (!h || (h->scan.n_scan && (!sums || !counts))) throw Error(E3D_ERR_INVALID, "null argument");
  if (!h->scan.scan_colors_begun) throw Error(E3D_ERR_INVALID, "call e3d_reg_scan_colors_begin first");
  std::vector<float4> acc(h->scan.n_scan);
  if (h->scan.n_scan) copy_out(acc.data(), h->scan.scan_color_acc.p, sizeof(float4) * h->scan.n_scan, h->stream);
  rsync(h);
  for (size_t i = 0; i < h->scan.n_scan; ++i) {
    sums[3 * i] = acc[i].x; sums[3 * i + 1] = acc[i].y; sums[3 * i + 2] = acc[i].z;
    memcpy(&counts[i], &acc[i].w, sizeof(int32_t));
  }
  return 0;
  E3D_CATCH()
}
int e3d_reg_scan_colors_set_sums(e3d_reg_t* h, const float* sums, const int32_t* counts) {
  E3D_TRY_ON(h)
  if (!h || (h->scan.n_scan && (!sums || !counts))) throw Error(E3D_ERR_INVALID, "null argument");
  if (!h->scan.scan_points_set) throw Error(E3D_ERR_INVALID, "no scan points set (e3d_reg_set_scan_points)");
  std::vector<float4> acc(h->scan.n_scan);
  for (size_t i = 0; i < h->scan.n_scan; ++i) {
    acc[i].x = sums[3 * i]; acc[i].y = sums[3 * i + 1]; acc[i].z = sums[3 * i + 2];
    memcpy(&acc[i].w, &counts[i], sizeof(int32_t));
  }
  h->scan.scan_color_acc.reserve(h->scan.n_scan);
  if (h->scan.n_scan) copy_in(h->scan.scan_color_acc.p, acc.data(), sizeof(float4) * h->scan.n_scan, h->stream);
  rsync(h);
  h->scan.scan_colors_begun = true;
  return 0;
  E3D_CATCH()
}
int e3d_reg_scan_colors_finish(e3d_reg_t* h, uint8_t* rgb) {
  E3D_TRY_ON(h)
  if (!h || (h->scan.n_scan && !rgb)) throw Error(E3D_ERR_INVALID, "null argument");
  if (!h->scan.scan_colors_begun) throw Error(E3D_ERR_INVALID, "call e3d_reg_scan_colors_begin first");
  if (h->scan.n_scan) {
    h->scan.scan_color_rgb.reserve(3 * h->scan.n_scan);
    {
      KT kt(h, "debug.scan_colors_finish", (double)h->scan.n_scan);
      hipLaunchKernelGGL(k_scan_colors_finish, dim3(nblk(h->scan.n_scan)), dim3(kBlock), 0, h->stream, h->scan.scan_color_acc.p, h->scan.n_scan, h->scan.scan_color_rgb.p);
    }
    copy_out(rgb, h->scan.scan_color_rgb.p, 3 * h->scan.n_scan, h->stream);
  }
  rsync(h);
  E3D_HIP(hipGetLastError());
  return 0;
  E3D_CATCH()
}

}  // extern "C"
