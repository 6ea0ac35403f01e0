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

template <int M, int KIND>
__global__ __launch_bounds__(kBlock) void k_undistort(CamLevel c, UndistortTarget t, const unsigned char* __restrict__ src,
                                                      unsigned char* __restrict__ dst, unsigned char* __restrict__ valid) {
  const int x = (int)(blockIdx.x * kUndistortRun + threadIdx.x), y = (int)(blockIdx.y * kUndistortRows + threadIdx.y);
  if (x >= t.width || y >= t.height) return;
  const size_t o = (size_t)y * (size_t)t.width + (size_t)x;
  const float nx = ((float)x - t.cx) / t.fx, ny = ((float)y - t.cy) / t.fy;
  float sx, sy;
  cam_normalized_to_image<M>(c, nx, ny, sx, sy);
  undistort_sample<KIND>(sx, sy, c.width, c.height, o, src, dst, valid);
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
