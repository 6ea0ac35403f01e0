// e3d_undistort.hpp -- the resampling kernel of e3d_reg_undistort (e3d_undistort.hip) as e3d_reg_scan.hip launches it.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "e3d_camera.hpp"

namespace e3d {

// The output camera of e3d_undistort_plan (include/e3d_hip.h): PINHOLE, pixel-centre convention
struct UndistortTarget { int width, height; float fx, fy, cx, cy; };

enum : int { kUndistortGray = 0, kUndistortRgb = 1, kUndistortMask = 2, kUndistortNearest = 3, kNumUndistortKinds = 4 };

// bytes of one source / destination pixel of a kind
constexpr size_t undistort_pixel_bytes(int kind) { return kind == kUndistortRgb ? 3 : (kind == kUndistortNearest ? 4 : 1); }

// One launch on `stream`: every pixel of the target lattice from the source image of the level-0 model `cam` (device pointers;
// `valid` may be null).  Throws on an unknown model or kind.
void undistort_launch(const CamLevel& cam, const UndistortTarget& target, int kind, const void* src, void* dst, uint8_t* valid,
                      hipStream_t stream);

}  // namespace e3d
