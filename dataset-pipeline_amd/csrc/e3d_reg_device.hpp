// e3d_reg_device.hpp -- device-side pieces shared by the registration sources: the optimiser (e3d_reg.hip), the occlusion-depth
// renderer (e3d_reg_depth.hip) and the scan-side tools (e3d_reg_scan.hip).  Device functions and kernel argument structs only: a
// __global__ kernel is defined in exactly one .hip and reached from another through a host launch function (e3d_reg_handle.hpp).
#pragma once

#include <climits>

#include "e3d_camera.hpp"
#include "e3d_kernels.hpp"

#pragma clang fp contract(off)

namespace e3d {

struct Pose { float R[9]; float t[3]; };

constexpr int kRegMaxLevels = 16;
struct Pyramid {               // passed by value to kernels
  const unsigned char* img[kRegMaxLevels];
  const unsigned char* mask[kRegMaxLevels];
  const unsigned char* cam_mask[kRegMaxLevels];      // Intrinsics::camera_mask (intrinsics.h:104): shared by all images of the camera
  CamLevel cam[kRegMaxLevels];
  int n_levels;
  int min_image_scale;
};

// x86 cvttss2si / cvttsd2si semantics of the reference's `int ix = v + 0.5f;`
__device__ __forceinline__ int f2i(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : INT_MIN; }
__device__ __forceinline__ int d2i(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }

__device__ __forceinline__ void rt(const Pose& P, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = dot3e(P.R[0], P.R[1], P.R[2], x, y, z) + P.t[0];
  oy = dot3e(P.R[3], P.R[4], P.R[5], x, y, z) + P.t[1];
  oz = dot3e(P.R[6], P.R[7], P.R[8], x, y, z) + P.t[2];
}

// ---- interpolation (interpolate_bilinear.h:36-74, interpolate_trilinear.h:44-87) ------------------------------------------
// (pixel type T: u8 images, f32 depth maps -- InterpolateTrilinear* are templates in the reference too, interpolate_trilinear.h)
template <class T>
__device__ __forceinline__ float bilinear(const T* img, int w, float x, float y, int ix, int iy) {
  const float fx = x - ix, fxi = 1.f - fx, fy = y - iy, fyi = 1.f - fy;
  const T* r0 = img + (size_t)iy * w;
  const T* r1 = img + (size_t)(iy + 1) * w;
  return fyi * (fxi * r0[ix] + fx * r0[ix + 1]) + fy * (fxi * r1[ix] + fx * r1[ix + 1]);
}
template <class T>
__device__ __forceinline__ void bilinear_d(const T* img, int w, float x, float y, int ix, int iy, float& v,
                                           float& dx, float& dy) {
  const T* r0 = img + (size_t)iy * w;
  const T* r1 = img + (size_t)(iy + 1) * w;
  const float tl = r0[ix], tr = r0[ix + 1], bl = r1[ix], br = r1[ix + 1];
  const float fx = x - ix, fxi = 1.f - fx, fy = y - iy, fyi = 1.f - fy;
  const float top = fxi * tl + fx * tr, bottom = fxi * bl + fx * br;
  v = fyi * top + fy * bottom;
  dx = fy * (br - bl) + fyi * (tr - tl);
  dy = bottom - top;
}
template <class T>
__device__ __forceinline__ float trilinear(const T* i0, int w0, const T* i1, int w1, float x0,
                                           float y0, float z) {
  const float v0 = bilinear(i0, w0, x0, y0, (int)x0, (int)y0);
  const float x1 = 2 * (x0 + 0.5f) - 0.5f, y1 = 2 * (y0 + 0.5f) - 0.5f;
  const float v1 = bilinear(i1, w1, x1, y1, (int)x1, (int)y1);
  return (1 - z) * v0 + z * v1;
}
template <class T>
__device__ __forceinline__ void trilinear_d(const T* i0, int w0, const T* i1, int w1, float x0,
                                            float y0, float z, float& v, float& dx, float& dy, float& dz) {
  float v0, dx0, dy0, v1, dx1, dy1;
  bilinear_d(i0, w0, x0, y0, (int)x0, (int)y0, v0, dx0, dy0);
  const float x1 = 2 * (x0 + 0.5f) - 0.5f, y1 = 2 * (y0 + 0.5f) - 0.5f;
  bilinear_d(i1, w1, x1, y1, (int)x1, (int)y1, v1, dx1, dy1);
  v = (1 - z) * v0 + z * v1;
  dx = (1 - z) * dx0 + z * 2 * dx1;
  dy = (1 - z) * dy0 + z * 2 * dy1;
  dz = v1 - v0;
}
__device__ __forceinline__ float obs_intensity(const Pyramid& Y, float ox, float oy, float os) {
  const int s = f2i(os);
  const int l1 = s - Y.min_image_scale, l0 = l1 + 1;
  return trilinear(Y.img[l0], Y.cam[l0].width, Y.img[l1], Y.cam[l1].width, ox, oy, 1 - (os - (float)s));
}

// CameraBaseImpl::InitializeUndistortionLookup (camera_base_impl.h:252-268): one Undistort per pixel.  undistort_lookup_entry is the
// table's entry for the pixel (x, y): k_undistort_lookup fills the whole table with it, e3d_reg_image_bearings evaluates the four entries
// around a position and builds no table.
template <int M>
__device__ __forceinline__ float2 undistort_lookup_entry(const CamLevel& c, int x, int y) {
  const float dx = c.fx_inv * x + c.cx_inv, dy = c.fy_inv * y + c.cy_inv;
  float ux, uy;
  if constexpr (M == kPinhole || M == kSimplePinhole) { ux = dx; uy = dy; }
  else if constexpr (M == kFov) { cam_fov_undistort(c, dx, dy, ux, uy); }
  else {
    cam_iterative_undistort<M>(c, dx, dy, dx, dy, ux, uy);
    if constexpr (cam_is_fisheye(M)) {           // FisheyeBase::Undistort (camera_base_impl_fisheye.h:81-92)
      const float r = sqrtf(ux * ux + uy * uy);
      const float factor = (r < kFisheyeEpsilon) ? 1.f : ((r > (float)(M_PI / 2.f)) ? E3D_CAM_INF : e3d_tanf(r) / r);
      ux = factor * ux; uy = factor * uy;
    }
  }
  return make_float2(ux, uy);
}

// ImageToNormalized(Vector2f) through the lookup table (camera_base_impl.h:188-211); the row index y + 1 is clamped where the
// reference reads one row past the table with weight 0.  entry(x, y) is the table's value at a lattice position: a read of the
// table, or the entry computed on the spot.
template <class Entry>
__device__ __forceinline__ float2 image_to_normalized_from(const CamLevel& c, float px, float py, Entry entry) {
  float cx = px < c.width - 1.001f ? px : c.width - 1.001f;
  float cy = py < c.height - 1.00f ? py : c.height - 1.00f;
  if (!(cx > 0.f)) cx = 0.f;
  if (!(cy > 0.f)) cy = 0.f;
  const int ix = (int)cx, iy = (int)cy;
  const float fx = cx - (float)ix, fy = cy - (float)iy;
  const int iy1 = iy + 1 < c.height ? iy + 1 : c.height - 1;
  const float2 tl = entry(ix, iy), tr = entry(ix + 1, iy);
  const float2 bl = entry(ix, iy1), br = entry(ix + 1, iy1);
  return make_float2((1 - fy) * ((1 - fx) * tl.x + fx * tr.x) + fy * ((1 - fx) * bl.x + fx * br.x),
                     (1 - fy) * ((1 - fx) * tl.y + fx * tr.y) + fy * ((1 - fx) * bl.y + fx * br.y));
}
// ImageToNormalized of the camera model M: FisheyeFOVCamera and the two pinhole models have their own, without the table
template <int M, class Entry>
__device__ __forceinline__ float2 camera_image_to_normalized(const CamLevel& c, float px, float py, Entry entry) {
  if constexpr (M == kFov) {      // Undistort(ImageToDistorted(p)) (camera_fisheye_fov.h:65-74)
    float2 nxy;
    cam_fov_undistort(c, c.fx_inv * px + c.cx_inv, c.fy_inv * py + c.cy_inv, nxy.x, nxy.y);
    return nxy;
  } else if constexpr (M == kPinhole || M == kSimplePinhole) {   // ImageToDistorted (camera_pinhole.h:55-63)
    return make_float2(c.fx_inv * px + c.cx_inv, c.fy_inv * py + c.cy_inv);
  } else {
    return image_to_normalized_from(c, px, py, entry);
  }
}

struct RadiusParams { int image_scale, min_image_scale; float occlusion_threshold, max_valid_intensity; double min_scaling_factor; };

// _AppendObservationsForImageNoScale for one point (visibility_estimator.cc:297-364): in front of the camera, rounded pixel inside
// the level `cam`, not behind the occlusion depth, not under an image or camera mask pixel, not over-saturated -- all at the level
// rp.image_scale.  True: (ox, oy) is the observation's position at its smaller interpolation scale and returned_scale its scale.
template <int M>
__device__ __forceinline__ bool observe_no_scale(const float4 p, const Pose& P, const CamLevel& cam, const unsigned char* __restrict__ img,
                                                 const unsigned char* __restrict__ mask, const unsigned char* __restrict__ cam_mask,
                                                 const float* __restrict__ occlusion, const RadiusParams& rp, float& ox, float& oy,
                                                 float& returned_scale) {
  float X, Y, Z;
  rt(P, p.x, p.y, p.z, X, Y, Z);
  if (!(Z > 0.f)) return false;
  float ixf, iyf;
  cam_normalized_to_image<M>(cam, X / Z, Y / Z, ixf, iyf);
  const int ix = f2i(ixf + 0.5f), iy = f2i(iyf + 0.5f);
  if (!(ixf + 0.5f >= 0 && iyf + 0.5f >= 0 && ix >= 0 && iy >= 0 && ix < cam.width && iy < cam.height)) return false;
  if (!(occlusion[(size_t)iy * cam.width + ix] + rp.occlusion_threshold >= Z)) return false;
  if (mask && mask[(size_t)iy * cam.width + ix] != 0) return false;
  if (cam_mask && cam_mask[(size_t)iy * cam.width + ix] != 0) return false;                    // visibility_estimator.cc:335-345
  if (img[(size_t)iy * cam.width + ix] > rp.max_valid_intensity) return false;
  returned_scale = rp.image_scale - 1e-6f;
  ox = ixf; oy = iyf;
  if (returned_scale < 0.f) {
    returned_scale = 0.f;
    ox = 0.5f * (ox + 0.5f) - 0.5f;
    oy = 0.5f * (oy + 0.5f) - 0.5f;
  }
  return true;
}

// the sum of the waves' counts (every lane of a wave passes its wave's count) added to *counter: one atomic per block (every thread of
// the block calls it)
__device__ __forceinline__ void block_wave_counts_add(unsigned wave_count, unsigned long long* __restrict__ counter, unsigned* sc);
// the block's number of set flags added to *counter
__device__ __forceinline__ void block_count_add(bool flag, unsigned long long* __restrict__ counter, unsigned* sc) {
  block_wave_counts_add((unsigned)__popcll(__ballot(flag)), counter, sc);
}
__device__ __forceinline__ void block_wave_counts_add(unsigned wave_count, unsigned long long* __restrict__ counter, unsigned* sc) {
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = wave_count;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0;
    for (int w = 0; w < kBlock / kWave; ++w) c += sc[w];
    if (c) atomicAdd(counter, (unsigned long long)c);
  }
  __syncthreads();
}

}  // namespace e3d
