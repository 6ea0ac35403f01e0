// e3d_undistort.hip -- ImageUndistorter's resampling kernel (gfx950): the pixels of a PINHOLE lattice gathered from an image of any of
// the camera models of e3d_camera.hpp.  The remap rule is this library's own (include/e3d_hip.h, e3d_reg_undistort);
// the bilinear expression is the reference's InterpolateBilinearNoCheck (src/opt/interpolate_bilinear.h:37-50) and the mask values
// are the bit flags of src/opt/image.h:43-47.  f32 without contraction, one output pixel per lane, no atomics and no sums across
// lanes: a launch equals a serial loop over the pixels bit for bit.
#include "e3d_undistort.hpp"

#include "e3d_common.hpp"
#include "e3d_kernels.hpp"

#include "../../include/e3d_hip.h"

#pragma clang fp contract(off)

namespace e3d {

// A workgroup is four waves, each on 64 consecutive pixels of one output row (threadIdx.x is the lane): the positions the lanes of
// a wave gather from run along one source row (a gently bent curve for the distorted models), so a wave's byte loads of one tap
// fall on a few neighbouring cache lines, and the rows above and below belong to the waves next to it.
constexpr int kUndistortRun = kWave, kUndistortRows = kBlock / kWave;

template <int M, int KIND>
__global__ __launch_bounds__(kBlock) void k_undistort(CamLevel c, UndistortTarget t, const unsigned char* __restrict__ src,
                                                      unsigned char* __restrict__ dst, unsigned char* __restrict__ valid) {
  const int x = (int)(blockIdx.x * kUndistortRun + threadIdx.x), y = (int)(blockIdx.y * kUndistortRows + threadIdx.y);
  if (x >= t.width || y >= t.height) return;
  const size_t o = (size_t)y * (size_t)t.width + (size_t)x;
  const float nx = ((float)x - t.cx) / t.fx, ny = ((float)y - t.cy) / t.fy;
  float sx, sy;
  cam_normalized_to_image<M>(c, nx, ny, sx, sy);
  const int W = c.width, H = c.height;
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

template <int M>
static void undistort_launch_model(const CamLevel& cam, const UndistortTarget& t, int kind, const unsigned char* src, unsigned char* dst,
                                   unsigned char* valid, hipStream_t stream) {
  const dim3 grid((unsigned)div_up((size_t)t.width, kUndistortRun), (unsigned)div_up((size_t)t.height, kUndistortRows));
  const dim3 block(kUndistortRun, kUndistortRows);
  switch (kind) {
    case kUndistortGray: hipLaunchKernelGGL((k_undistort<M, kUndistortGray>), grid, block, 0, stream, cam, t, src, dst, valid); break;
    case kUndistortRgb: hipLaunchKernelGGL((k_undistort<M, kUndistortRgb>), grid, block, 0, stream, cam, t, src, dst, valid); break;
    case kUndistortMask: hipLaunchKernelGGL((k_undistort<M, kUndistortMask>), grid, block, 0, stream, cam, t, src, dst, valid); break;
    case kUndistortNearest: hipLaunchKernelGGL((k_undistort<M, kUndistortNearest>), grid, block, 0, stream, cam, t, src, dst, valid); break;
    default: throw Error(E3D_ERR_INVALID, "unknown kind (0 = u8, 1 = u8 x 3, 2 = mask, 3 = f32 nearest)");
  }
}

void undistort_launch(const CamLevel& cam, const UndistortTarget& target, int kind, const void* src, void* dst, uint8_t* valid,
                      hipStream_t stream) {
  if (target.width < 1 || target.height < 1 || target.height > 65535 * kUndistortRows)
    throw Error(E3D_ERR_INVALID, "undistortion target size out of range");
  E3D_CAM_SWITCH(cam.model, undistort_launch_model<M>(cam, target, kind, static_cast<const unsigned char*>(src),
                                                      static_cast<unsigned char*>(dst), valid, stream));
}

}  // namespace e3d
