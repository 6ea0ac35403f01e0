// e3d_undistort.hpp -- the resampling kernels of e3d_reg_undistort (e3d_undistort.hip) and e3d_reg_stereo_rectify (e3d_stereo.hip) as
// e3d_reg_scan.hip launches them, and the sampling tail the two kernels share.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "e3d_camera.hpp"
#include "e3d_kernels.hpp"

#pragma clang fp contract(off)

namespace e3d {

// The output camera of e3d_undistort_plan (include/e3d_hip.h): PINHOLE, pixel-centre convention
struct UndistortTarget { int width, height; float fx, fy, cx, cy; };
// source_T_rect of e3d_stereo_plan, row-major: a ray of the rectified frame in the source camera's frame
struct StereoRotation { float m[9]; };

enum : int { kUndistortGray = 0, kUndistortRgb = 1, kUndistortMask = 2, kUndistortNearest = 3, kNumUndistortKinds = 4 };

// bytes of one source / destination pixel of a kind
constexpr size_t undistort_pixel_bytes(int kind) { return kind == kUndistortRgb ? 3 : (kind == kUndistortNearest ? 4 : 1); }

// A workgroup is four waves, each on 64 consecutive pixels of one output row (threadIdx.x is the lane): the positions the lanes of
// a wave gather from run along one source row (a gently bent curve for the distorted models), so a wave's byte loads of one tap
// fall on a few neighbouring cache lines, and the rows above and below belong to the waves next to it.
constexpr int kUndistortRun = kWave, kUndistortRows = kBlock / kWave;

// Everything after the source position (sx, sy) of the output pixel with the index o: the validity test, the value of an invalid
// pixel, and the sample of the kind from the W x H source (the rule: include/e3d_hip.h, e3d_reg_undistort).  k_undistort and
// k_rectify both end in it.
template <int KIND>
__device__ __forceinline__ void undistort_sample(float sx, float sy, int W, int H, size_t o, const unsigned char* __restrict__ src,
                                                 unsigned char* __restrict__ dst, unsigned char* __restrict__ valid) {
  // closed interval: the plan's inner extents map to exactly these borders (NaN and +-inf fail the comparisons)
  const bool ok = sx >= 0.f && sx <= (float)(W - 1) && sy >= 0.f && sy <= (float)(H - 1);
  if (valid) valid[o] = ok ? 1 : 0;
  if (!ok) {
    if constexpr (KIND == kUndistortGray) dst[o] = 0;
    else if constexpr (KIND == kUndistortRgb) { dst[3 * o] = 0; dst[3 * o + 1] = 0; dst[3 * o + 2] = 0; }
    else if constexpr (KIND == kUndistortMask) dst[o] = 3;        // kObs | kEvalObs: no data
    else reinterpret_cast<unsigned*>(dst)[o] = 0u;
    return;
  }
  if constexpr (KIND == kUndistortNearest) {
    const int ix = min((int)(sx + 0.5f), W - 1), iy = min((int)(sy + 0.5f), H - 1);
    reinterpret_cast<unsigned*>(dst)[o] = reinterpret_cast<const unsigned*>(src)[(size_t)iy * W + ix];     // copied as bits
  } else {
    const int ix = min((int)sx, W - 2), iy = min((int)sy, H - 2);
    const size_t r0 = (size_t)iy * W + ix, r1 = r0 + (size_t)W;
    if constexpr (KIND == kUndistortMask) {
      dst[o] = (unsigned char)(src[r0] | src[r0 + 1] | src[r1] | src[r1 + 1]);
    } else {
      const float ax = sx - (float)ix, ay = sy - (float)iy;
      const float bx = 1.f - ax, by = 1.f - ay;
      constexpr int C = KIND == kUndistortRgb ? 3 : 1;
      unsigned char p[4][C];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {                // all the loads first, then the arithmetic
        p[0][ch] = src[C * r0 + ch]; p[1][ch] = src[C * (r0 + 1) + ch];
        p[2][ch] = src[C * r1 + ch]; p[3][ch] = src[C * (r1 + 1) + ch];
      }
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const float v = by * (bx * (float)p[0][ch] + ax * (float)p[1][ch]) + ay * (bx * (float)p[2][ch] + ax * (float)p[3][ch]);
        dst[C * o + ch] = (unsigned char)(int)(v + 0.5f);
      }
    }
  }
}

// One launch on `stream`: every pixel of the target lattice from the source image of the level-0 model `cam` (device pointers;
// `valid` may be null).  Throws on an unknown model or kind.
void undistort_launch(const CamLevel& cam, const UndistortTarget& target, int kind, const void* src, void* dst, uint8_t* valid,
                      hipStream_t stream);
// The same with the ray of every output pixel rotated by S before it goes through the source model (e3d_reg_stereo_rectify)
void rectify_launch(const CamLevel& cam, const UndistortTarget& target, const StereoRotation& S, int kind, const void* src, void* dst,
                    uint8_t* valid, hipStream_t stream);
// e3d_reg_stereo_ground_truth, on n pixels (device pointers): bytes -> 0 / 1, and the disparity / mask rule from the two depth maps
void stereo_normalize_mask_launch(uint8_t* mask, size_t n, hipStream_t stream);
void stereo_disparity_launch(const unsigned* d1_bits, const unsigned* d2_bits, size_t n, float f, double baseline, float* disparity,
                             uint8_t* nocc_mask, hipStream_t stream);

}  // namespace e3d
