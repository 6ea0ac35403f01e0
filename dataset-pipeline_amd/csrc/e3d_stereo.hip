// e3d_stereo.hip -- StereoPairCreator's kernels (gfx950): k_rectify, the resampling kernel of e3d_reg_stereo_rectify (k_undistort with
// the ray of the output pixel rotated into the source camera's frame before it goes through the source model), and the per-pixel
// rules of e3d_reg_stereo_ground_truth.  The rules are this library's own (include/e3d_hip.h).  f32 without contraction,
// one output pixel per lane, no LDS, no atomics and no sums across lanes: a launch equals a serial loop over the pixels bit for bit.
#include "e3d_undistort.hpp"

#include "e3d_common.hpp"
#include "e3d_kernels.hpp"

#include "../../include/e3d_hip.h"

#pragma clang fp contract(off)

namespace e3d {

// The workgroup of k_undistort.  v = S (nx, ny, 1): each product and each sum rounded, in the order written; a ray that does not
// point into the source camera's front half space (!(vz > 0)) has no position (NaN fails the tail's interval test).
template <int M, int KIND>
__global__ __launch_bounds__(kBlock) void k_rectify(CamLevel c, UndistortTarget t, StereoRotation S, const unsigned char* __restrict__ src,
                                                    unsigned char* __restrict__ dst, unsigned char* __restrict__ valid) {
  const int x = (int)(blockIdx.x * kUndistortRun + threadIdx.x), y = (int)(blockIdx.y * kUndistortRows + threadIdx.y);
  if (x >= t.width || y >= t.height) return;
  const size_t o = (size_t)y * (size_t)t.width + (size_t)x;
  const float nx = ((float)x - t.cx) / t.fx, ny = ((float)y - t.cy) / t.fy;
  const float vx = (S.m[0] * nx + S.m[1] * ny) + S.m[2];
  const float vy = (S.m[3] * nx + S.m[4] * ny) + S.m[5];
  const float vz = (S.m[6] * nx + S.m[7] * ny) + S.m[8];
  float sx = NAN, sy = NAN;
  if (vz > 0.f) cam_normalized_to_image<M>(c, vx / vz, vy / vz, sx, sy);
  undistort_sample<KIND>(sx, sy, c.width, c.height, o, src, dst, valid);
}

template <int M>
static void rectify_launch_model(const CamLevel& cam, const UndistortTarget& t, const StereoRotation& S, int kind, const unsigned char* src,
                                 unsigned char* dst, unsigned char* valid, hipStream_t stream) {
  const dim3 grid((unsigned)div_up((size_t)t.width, kUndistortRun), (unsigned)div_up((size_t)t.height, kUndistortRows));
  const dim3 block(kUndistortRun, kUndistortRows);
  switch (kind) {
    case kUndistortGray: hipLaunchKernelGGL((k_rectify<M, kUndistortGray>), grid, block, 0, stream, cam, t, S, src, dst, valid); break;
    case kUndistortRgb: hipLaunchKernelGGL((k_rectify<M, kUndistortRgb>), grid, block, 0, stream, cam, t, S, src, dst, valid); break;
    case kUndistortMask: hipLaunchKernelGGL((k_rectify<M, kUndistortMask>), grid, block, 0, stream, cam, t, S, src, dst, valid); break;
    case kUndistortNearest: hipLaunchKernelGGL((k_rectify<M, kUndistortNearest>), grid, block, 0, stream, cam, t, S, src, dst, valid); break;
    default: throw Error(E3D_ERR_INVALID, "unknown kind (0 = u8, 1 = u8 x 3, 2 = mask, 3 = f32 nearest)");
  }
}

void rectify_launch(const CamLevel& cam, const UndistortTarget& target, const StereoRotation& S, int kind, const void* src, void* dst,
                    uint8_t* valid, hipStream_t stream) {
  if (target.width < 1 || target.height < 1 || target.height > 65535 * kUndistortRows)
    throw Error(E3D_ERR_INVALID, "rectification target size out of range");
  E3D_CAM_SWITCH(cam.model, rectify_launch_model<M>(cam, target, S, kind, static_cast<const unsigned char*>(src),
                                                    static_cast<unsigned char*>(dst), valid, stream));
}

// the exclusion maps of e3d_reg_stereo_ground_truth may hold any non-zero value; k_scan_visibility compares for equality with one flag
__global__ __launch_bounds__(kBlock) void k_stereo_normalize_mask(unsigned char* __restrict__ mask, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  mask[i] = mask[i] ? 1 : 0;
}

void stereo_normalize_mask_launch(uint8_t* mask, size_t n, hipStream_t stream) {
  if (!n) return;
  hipLaunchKernelGGL(k_stereo_normalize_mask, dim3((unsigned)div_up(n, (size_t)kBlock)), dim3(kBlock), 0, stream, mask, n);
}

// d1: the nearest scan point visible in the left image, d2: the nearest one visible in both (float bits, +inf = none; finite ones
// are > 0).  disparity = (float)(f * B / d1) in f64, +inf where unknown; the mask is 255 where both maps hold the same point's
// depth, 128 where the nearest left point is not seen from the right (half-occluded), 0 where there is no ground truth.
__global__ __launch_bounds__(kBlock) void k_stereo_disparity(const unsigned* __restrict__ d1_bits, const unsigned* __restrict__ d2_bits,
                                                             size_t n, float f, double baseline, float* __restrict__ disparity,
                                                             unsigned char* __restrict__ nocc) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned b1 = d1_bits[i], b2 = d2_bits[i];
  const float d1 = __uint_as_float(b1);
  const bool known = b1 < 0x7f800000u;                     // positive and finite
  disparity[i] = known ? (float)((double)f * baseline / (double)d1) : INFINITY;
  nocc[i] = known ? (b2 == b1 ? 255 : 128) : 0;
}

void stereo_disparity_launch(const unsigned* d1_bits, const unsigned* d2_bits, size_t n, float f, double baseline, float* disparity,
                             uint8_t* nocc_mask, hipStream_t stream) {
  if (!n) return;
  hipLaunchKernelGGL(k_stereo_disparity, dim3((unsigned)div_up(n, (size_t)kBlock)), dim3(kBlock), 0, stream, d1_bits, d2_bits, n, f, baseline,
                     disparity, nocc_mask);
}

}  // namespace e3d
