// e3d_reg_depth.hip -- the occlusion-depth renderer of the image registration (OcclusionGeometry, src/opt/occlusion_geometry.cc): the
// splat and mesh kernels, render_depth for every source that works on the handle (e3d_reg_handle.hpp), and the C-ABI entries that
// load the occlusion geometry (include/e3d_hip.h).  Its state is the handle's DepthRenderer.
#include <algorithm>
#include <cmath>

#include "e3d_grid.hpp"
#include "e3d_reg_handle.hpp"

#pragma clang fp contract(off)

namespace e3d {

// ==== a24: OcclusionGeometry::_RenderDepthMapWithSplatsCPU ========================================================================
// depth(x, y) = min z over all points whose splat rectangle covers (x, y): an order-free reduction, so the result is exact
// whatever the schedule.  Splats overlap heavily (a 3 cm splat at 3 m is the 21 x 21 pixel maximum; scan points are
// millimetres apart), so instead of one global atomic per covered pixel the points are binned into 32 x 32 pixel tiles,
// radix-sorted by tile, and each tile is reduced in LDS by one workgroup and written once.
constexpr int kTile = 32;

// the reference's rectangle of one point (occlusion_geometry.cc:423-452), clipped to the image; false if empty
constexpr int kSplatMax = 10;        // max_splat_radius (occlusion_geometry.cc:417)

template <int M>
__device__ __forceinline__ bool splat_rect(const float4 p, const Pose& P, const CamLevel& cam, float point_radius, int& min_x, int& min_y,
                                           int& end_x, int& end_y, unsigned& zb, bool& full_size, int& cxi, int& cyi) {
  full_size = false;
  float X, Y, Z;
  rt(P, p.x, p.y, p.z, X, Y, Z);
  if (!(Z > 0.f)) return false;
  float px, py, d[6];
  const CamTheta th = cam_theta<M>(X / Z, Y / Z);                 // (the fisheye models' atan: once per point)
  cam_normalized_to_image<M>(cam, X / Z, Y / Z, th, px, py);
  cam_image_deriv_by_world<M>(cam, X, Y, Z, th, d);
  float rx = sqrtf(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])) * point_radius;
  float ry = sqrtf(d[3] * d[3] + (d[4] * d[4] + d[5] * d[5])) * point_radius;
  full_size = rx >= 10.f && ry >= 10.f;     // both half-extents clamped: the rectangle is exactly [ix-10, ix+10] x [iy-10, iy+10]
  rx = (10.f < rx) ? 10.f : rx;     // std::min(splat_radius, max_splat_radius)
  ry = (10.f < ry) ? 10.f : ry;
  const int ix = f2i(px + 0.5f), iy = f2i(py + 0.5f);
  cxi = ix; cyi = iy;
  min_x = d2i((double)((float)ix - rx) + 0.5); min_y = d2i((double)((float)iy - ry) + 0.5);
  end_x = d2i((double)((float)ix + rx) + 1.5); end_y = d2i((double)((float)iy + ry) + 1.5);
  min_x = max(min_x, 0); min_y = max(min_y, 0);
  end_x = min(end_x, cam.width); end_y = min(end_y, cam.height);
  zb = __float_as_uint(Z);          // Z > 0: the bit pattern is order preserving
  return min_x < end_x && min_y < end_y;
}

// one (tile, point) pair per tile a rectangle touches (<= 2 x 2: rectangles are at most 22 pixels wide); wave-aggregated append
template <int M>
__global__ __launch_bounds__(kBlock) void k_splat_bin(const float4* __restrict__ pts, size_t n, Pose P, CamLevel cam,
                                                      float point_radius, int tiles_x, uint4* __restrict__ rects,
                                                      unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                      unsigned* __restrict__ counter, unsigned* __restrict__ zbuf) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  int min_x = 0, min_y = 0, end_x = 0, end_y = 0, cxi = 0, cyi = 0;
  unsigned zb = 0;
  bool ok = false, full_size = false;
  if (i < n) ok = splat_rect<M>(pts[i], P, cam, point_radius, min_x, min_y, end_x, end_y, zb, full_size, cxi, cyi);
  if (ok && full_size) {
    // Full-size splats (the near, heavily overlapping ones) are not rasterised one by one: their union is the 21 x 21
    // MIN FILTER of the one-pixel-per-point z-buffer, computed separably afterwards (k_min_filter_h / _v).  The buffer
    // carries a 10-pixel apron because a splat centred outside the image can still reach into it.
    const int wp = cam.width + 2 * kSplatMax;
    if (cxi >= -kSplatMax && cyi >= -kSplatMax && cxi < cam.width + kSplatMax && cyi < cam.height + kSplatMax)
      atomicMin(&zbuf[(size_t)(cyi + kSplatMax) * wp + (cxi + kSplatMax)], zb);
    ok = false;
  }
  int tx0 = 0, tx1 = -1, ty0 = 0, ty1 = -1;
  if (ok) {
    tx0 = min_x / kTile; tx1 = (end_x - 1) / kTile; ty0 = min_y / kTile; ty1 = (end_y - 1) / kTile;
    rects[i] = make_uint4((unsigned)min_x | ((unsigned)min_y << 16), (unsigned)end_x | ((unsigned)end_y << 16), zb, 0u);
  }
  const unsigned count = ok ? (unsigned)((tx1 - tx0 + 1) * (ty1 - ty0 + 1)) : 0u;
  const int lane = threadIdx.x & 63;
  unsigned incl = count;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  // one append per workgroup (a single hot address serialises: one atomic per wave costs more than the whole projection)
  __shared__ unsigned wave_total[kBlock / kWave];
  __shared__ unsigned block_base;
  const int wv = threadIdx.x >> 6;
  if (lane == 63) wave_total[wv] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tot = 0;
#pragma unroll
    for (int k = 0; k < kBlock / kWave; ++k) tot += wave_total[k];
    block_base = tot ? atomicAdd(counter, tot) : 0u;
  }
  __syncthreads();
  unsigned base = block_base;
  for (int k = 0; k < wv; ++k) base += wave_total[k];
  unsigned o = base + incl - count;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) { keys[o] = (unsigned)(ty * tiles_x + tx); vals[o] = (unsigned)i; ++o; }
}

__global__ __launch_bounds__(kBlock) void k_tile_ranges(const unsigned* __restrict__ keys, size_t n, unsigned* __restrict__ start,
                                                        unsigned* __restrict__ end) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned k = keys[i];
  if (i == 0 || keys[i - 1] != k) start[k] = (unsigned)i;
  if (i + 1 == n || keys[i + 1] != k) end[k] = (unsigned)(i + 1);
}

// one workgroup per tile: z-min of the tile's rectangles in LDS (ds_min_u32), every pixel of the tile written exactly once
__global__ __launch_bounds__(kBlock) void k_splat_tiles(const uint4* __restrict__ rects, const unsigned* __restrict__ vals,
                                                        const unsigned* __restrict__ start, const unsigned* __restrict__ end,
                                                        int tiles_x, int width, int height, unsigned* __restrict__ depth_bits) {
  __shared__ unsigned tile[kTile * kTile];
  const int t = blockIdx.x;
  const int x0 = (t % tiles_x) * kTile, y0 = (t / tiles_x) * kTile;
  for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) tile[i] = 0x7f800000u;
  __syncthreads();
  const unsigned s = start[t], e = end[t];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lx = lane & 31, ly = lane >> 5;
  constexpr unsigned kStep = kBlock / kWave;
  uint4 nxt = (s + wv < e) ? rects[vals[s + wv]] : make_uint4(0, 0, 0, 0);
  for (unsigned j = s + wv; j < e; j += kStep) {
    const uint4 r = nxt;
    if (j + kStep < e) nxt = rects[vals[j + kStep]];       // fetch the next rectangle while this one is applied
    const int mx = max((int)(r.x & 0xffffu), x0) - x0, my = max((int)(r.x >> 16), y0) - y0;
    const int ex = min((int)(r.y & 0xffffu), x0 + kTile) - x0, ey = min((int)(r.y >> 16), y0 + kTile) - y0;
    const int x = mx + lx;
    if (x < ex)
      for (int y = my + ly; y < ey; y += 2) atomicMin(&tile[y * kTile + x], r.z);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {
    const int x = x0 + (i & (kTile - 1)), y = y0 + (i / kTile);
    if (x < width && y < height) depth_bits[(size_t)y * width + x] = tile[i];
  }
}

// separable 21 x 21 min filter of the apron-padded point z-buffer (positive float bits compare like unsigned integers)
__global__ __launch_bounds__(kBlock) void k_min_filter_h(const unsigned* __restrict__ zbuf, int width, int height,
                                                         unsigned* __restrict__ tmp /* (height + 20) x width */) {
  __shared__ unsigned row[kBlock + 2 * kSplatMax];
  const int wp = width + 2 * kSplatMax;
  const int y = blockIdx.y;                                   // padded row
  const int x0 = blockIdx.x * kBlock;
  for (int i = threadIdx.x; i < kBlock + 2 * kSplatMax; i += kBlock) {
    const int xp = x0 + i;                                    // padded column of output column x0 + i - 10
    row[i] = (xp < wp) ? zbuf[(size_t)y * wp + xp] : 0x7f800000u;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= width) return;
  unsigned m = 0x7f800000u;
#pragma unroll
  for (int d = 0; d <= 2 * kSplatMax; ++d) m = min(m, row[threadIdx.x + d]);
  tmp[(size_t)y * width + x] = m;
}
__global__ __launch_bounds__(kBlock) void k_min_filter_v(const unsigned* __restrict__ tmp, int width, int height,
                                                         unsigned* __restrict__ depth_bits) {
  const int x = blockIdx.x * kBlock + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= width) return;
  unsigned m = depth_bits[(size_t)y * width + x];             // what the rectangle path (smaller splats) produced
#pragma unroll
  for (int d = 0; d <= 2 * kSplatMax; ++d) m = min(m, tmp[(size_t)(y + d) * width + x]);
  depth_bits[(size_t)y * width + x] = m;
}

// The two passes in one kernel (round 4): a block owns a kMfW x kMfH tile of the image, stages the tile of the padded z-buffer with
// its 20-pixel skirt in LDS once, filters it horizontally into a second LDS tile and vertically into the depth map -- the
// intermediate image never goes to memory (two 98 MB images written and read per 24 MP depth map before: 0.22 ms; the vertical
// pass alone read 21 rows per pixel through L2).  A thread produces four neighbouring pixels of a row, then eight of a column:
// 6 + 3.5 LDS reads per pixel instead of 21 + 21.  min is associative: bit-identical to the separable passes.
// MERGE = false: no splat took the rectangle path (the usual case at room scale: every splat is full size), so the depth map holds
// nothing yet -- the filter's result is STORED instead of merged, and the pass that would have filled the map with +inf first
// (k_splat_tiles over all tiles: a 4 B store per pixel, read back here) is not launched.  min(+inf, m) = m: the same bits.
constexpr int kMfW = 64, kMfH = 32, kMfWin = 2 * kSplatMax + 1;
template <bool MERGE>
__global__ __launch_bounds__(kBlock) void k_min_filter_tile(const unsigned* __restrict__ zbuf, int width, int height,
                                                            unsigned* __restrict__ depth_bits) {
  constexpr int IW = kMfW + 2 * kSplatMax, IH = kMfH + 2 * kSplatMax;
  __shared__ unsigned tin[IH][IW];
  __shared__ unsigned th[IH][kMfW];
  const int wp = width + 2 * kSplatMax, hp = height + 2 * kSplatMax;
  const int x0 = blockIdx.x * kMfW, y0 = blockIdx.y * kMfH;           // tile origin (image = padded coordinates of its skirt's corner)
  for (int i = threadIdx.x; i < IH * IW; i += kBlock) {
    const int r = i / IW, c = i - r * IW;
    const int xp = x0 + c, yp = y0 + r;
    tin[r][c] = (xp < wp && yp < hp) ? zbuf[(size_t)yp * wp + xp] : 0x7f800000u;
  }
  __syncthreads();
  // horizontal: IH rows x kMfW columns, four columns per thread
  for (int i = threadIdx.x; i < IH * (kMfW / 4); i += kBlock) {
    const int r = i / (kMfW / 4), c = (i - r * (kMfW / 4)) * 4;
    unsigned mid = 0x7f800000u;                                        // columns c + 3 .. c + 20 are in all four windows
#pragma unroll
    for (int d = 3; d < kMfWin; ++d) mid = min(mid, tin[r][c + d]);
    const unsigned a0 = tin[r][c], a1 = tin[r][c + 1], a2 = tin[r][c + 2];
    const unsigned b0 = tin[r][c + kMfWin], b1 = tin[r][c + kMfWin + 1], b2 = tin[r][c + kMfWin + 2];
    th[r][c] = min(mid, min(a0, min(a1, a2)));
    th[r][c + 1] = min(mid, min(min(a1, a2), b0));
    th[r][c + 2] = min(mid, min(a2, min(b0, b1)));
    th[r][c + 3] = min(mid, min(b0, min(b1, b2)));
  }
  __syncthreads();
  // vertical: one column, eight rows per thread
  const int c = threadIdx.x & (kMfW - 1), r0 = (threadIdx.x / kMfW) * 8;
  const int x = x0 + c;
  unsigned mid = 0x7f800000u;                                          // rows r0 + 7 .. r0 + 20 are in all eight windows
#pragma unroll
  for (int d = 7; d < kMfWin; ++d) mid = min(mid, th[r0 + d][c]);
  unsigned lo[7], hi[7];
#pragma unroll
  for (int d = 0; d < 7; ++d) { lo[d] = th[r0 + d][c]; hi[d] = th[r0 + kMfWin + d][c]; }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    unsigned m = mid;
#pragma unroll
    for (int d = k; d < 7; ++d) m = min(m, lo[d]);
#pragma unroll
    for (int d = 0; d < k; ++d) m = min(m, hi[d]);
    const int y = y0 + r0 + k;
    if (x < width && y < height) {
      const size_t o = (size_t)y * width + x;
      if constexpr (MERGE) depth_bits[o] = min(depth_bits[o], m);      // with what the rectangle path (smaller splats) produced
      else depth_bits[o] = m;
    }
  }
}

// ==== f2: occlusion meshes (OcclusionGeometry::RenderDepthMap mesh branch, occlusion_geometry.cc:211-271; the reference
// renders with OpenGL, src/opengl/renderer.cc) ================================================================================
// Software rasteriser with the renderer's conventions: the vertex shader's distortion code per camera model
// (renderer.cc:226-262,470-495,630-653: no cut-off branch for PINHOLE, `* 99` outside the cut-off), projection
// p = f * x'/z + c (SetupProjection :919-974 maps pixel centres to integer coordinates of this code base), depth =
// perspective-correct interpolation of the camera-space z (the fragment shader writes var_depth), nearest fragment wins,
// pixels without geometry are 0 (glClearColor).  Triangles that cross the near plane z = min_depth are clipped the way OpenGL clips
// them: on the vertex shader's OUTPUT (x', y', z) -- linear interpolation along the edge from the vertex inside to the one outside,
// so the cut is shared by the triangles on both sides of an edge -- and before the perspective division; a vertex behind the camera
// goes through the distortion code like any other (its x / z is mirrored), as in the shader.  OpenGL's own rasterisation is implementation-defined at pixel-boundary ties; here: samples at integer pixel
// coordinates, edge functions in f64 (exact for f32 inputs), top-left rule.
template <int M>
__global__ __launch_bounds__(kBlock) void k_mesh_vertices(const float4* __restrict__ v, size_t n, Pose P, CamLevel cam,
                                                          float4* __restrict__ out, float2* __restrict__ out_l) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = v[i];
  float X, Y, Z;
  rt(P, p.x, p.y, p.z, X, Y, Z);
  float lx = X, ly = Y;
  if constexpr (M == kSimpleRadial) {
    // SimpleRadial shader (renderer.cc:402-413): its own r2 expression, 99 outside the cut-off
    float r2 = (X * X + Y * Y) / (Z * Z);
    if (r2 > cam.cutoff2) r2 = 99.0f; else r2 = 1.0f + r2 * cam.q[0];
    lx = r2 * X; ly = r2 * Y;
  } else if constexpr (M == kRadial || M == kPolynomial3) {
    // Radial / Polynomial shaders (renderer.cc:326-337, 288-300)
    const float nx = X / Z, ny = Y / Z;
    float r2 = nx * nx + ny * ny;
    if (r2 <= cam.cutoff2) {
      if constexpr (M == kRadial) r2 = 1.0f + r2 * (cam.q[0] + r2 * cam.q[1]);
      else r2 = 1.0f + r2 * (cam.q[0] + r2 * (cam.q[1] + r2 * cam.q[2]));
    } else {
      r2 = 99.0f;
    }
    lx = r2 * X; ly = r2 * Y;
  } else if constexpr (M == kRadialFisheye || M == kSimpleRadialFisheye) {
    // RadialFisheye / SimpleRadialFisheye shaders (renderer.cc:361-378, 434-452): r2 after the fisheye warp against the OUTER camera's cut-off
    float nx = X / Z, ny = Y / Z;
    float r2 = nx * nx + ny * ny;
    const float r = sqrtf(r2);
    if (r > 1e-6f) {
      const float theta_by_r = e3d_atan2f(r, 1.0f) / r;
      if constexpr (M == kRadialFisheye) { nx = theta_by_r * nx; ny = theta_by_r * ny; r2 = nx * nx + ny * ny; }
      else { r2 = r2 * theta_by_r * theta_by_r; nx = nx * theta_by_r; ny = ny * theta_by_r; }
    }
    if (r2 <= cam.cutoff2) {
      if constexpr (M == kRadialFisheye) r2 = 1.0f + r2 * (cam.q[0] + r2 * cam.q[1]);
      else r2 = 1.0f + r2 * cam.q[0];
    } else {
      r2 = 99.0f;
    }
    lx = Z * r2 * nx; ly = Z * r2 * ny;
  } else if constexpr (M == kFullOpenCV) {
    // FullOpenCV shader (renderer.cc:528-543)
    const float nx = X / Z, ny = Y / Z;
    const float x2 = nx * nx, xy = nx * ny, y2 = ny * ny;
    const float r2 = x2 + y2;
    if (r2 <= cam.cutoff2) {
      const float k1 = cam.q[0], k2 = cam.q[1], p1 = cam.q[2], p2 = cam.q[3], k3 = cam.q[4], k4 = cam.q[5], k5 = cam.q[6], k6 = cam.q[7];
      const float radial = (1.0f + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0f + r2 * (k4 + r2 * (k5 + r2 * k6)));
      lx = Z * (radial * nx + 2.0f * p1 * xy + p2 * (r2 + 2.0f * x2));
      ly = Z * (radial * ny + 2.0f * p2 * xy + p1 * (r2 + 2.0f * y2));
    } else {
      lx = X * 99.0f; ly = Y * 99.0f;
    }
  } else if constexpr (M != kPinhole && M != kSimplePinhole) {
    float nx = X / Z, ny = Y / Z;
    float r2 = nx * nx + ny * ny;
    if constexpr (M == kFov) {
      // FisheyeFOV shader (renderer.cc:153-160): r = length(xy) / z; r = atan(r * two_tan_omega_half) / (r * omega); xy *= r.  GLSL
      // leaves 0 / 0 on the optical axis undefined; the camera class's guard (camera_fisheye_fov.h:58-61) is used there
      const float r = sqrtf(X * X + Y * Y) / Z;
      const float f = (r < 1e-6f) ? 1.0f : e3d_atanf(r * cam.q[1]) / (r * cam.q[0]);
      lx = f * X; ly = f * Y;
    } else if constexpr (M == kOpenCVFisheye) {
      // FisheyePolynomial4 shader (renderer.cc:187-205): r2 turns into the radial factor (99 outside the cut-off)
      if (r2 <= cam.cutoff2) {
        const float r = sqrtf(r2);
        if (r > 1e-6f) { const float theta_by_r = e3d_atan2f(r, 1.0f) / r; nx = theta_by_r * nx; ny = theta_by_r * ny; r2 = theta_by_r * theta_by_r * r2; }
        r2 = 1.0f + r2 * (cam.q[0] + r2 * (cam.q[1] + r2 * (cam.q[2] + r2 * cam.q[3])));
      } else {
        r2 = 99.0f;
      }
      lx = Z * r2 * nx; ly = Z * r2 * ny;
    } else if (r2 <= cam.cutoff2) {
      if constexpr (cam_is_fisheye(M)) {           // THIN_PRISM_FISHEYE, FISHEYE_POLYNOMIAL_2_TANGENTIAL_2 (renderer.cc:236-258)
        const float r = sqrtf(r2);
        if (r > 1e-6f) { const float theta_by_r = e3d_atan2f(r, 1.0f) / r; nx = theta_by_r * nx; ny = theta_by_r * ny; }
      }
      const float x2 = nx * nx, xy = nx * ny, y2 = ny * ny;
      r2 = x2 + y2;
      const float k1 = cam.q[0], k2 = cam.q[1], p1 = cam.q[2], p2 = cam.q[3];
      if constexpr (cam_is_poly_tang(M)) {
        const float radial = 1.0f + r2 * (k1 + r2 * k2);
        lx = Z * (radial * nx + 2.0f * p1 * xy + p2 * (r2 + 2.0f * x2));
        ly = Z * (radial * ny + 2.0f * p2 * xy + p1 * (r2 + 2.0f * y2));
      } else {
        const float k3 = cam.q[4], k4 = cam.q[5], sx1 = cam.q[6], sy1 = cam.q[7];
        const float radial = 1.0f + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)));
        lx = Z * (radial * nx + 2.0f * p1 * xy + p2 * (r2 + 2.0f * x2) + sx1 * r2);
        ly = Z * (radial * ny + 2.0f * p2 * xy + p1 * (r2 + 2.0f * y2) + sy1 * r2);
      }
    } else {
      lx = X * 99.0f; ly = Y * 99.0f;
    }
  }
  out[i] = make_float4(cam.fx * (lx / Z) + cam.cx, cam.fy * (ly / Z) + cam.cy, Z, 0.f);
  out_l[i] = make_float2(lx, ly);
}

struct MeshProj { float fx, fy, cx, cy, near; };

// the point where the edge from vertex `in` (z >= near) to vertex `out` (z < near) meets the near plane, projected
__device__ __forceinline__ float4 near_cut(const float4 pin, const float2 lin, const float4 pout, const float2 lout, const MeshProj& m) {
  const float t = (m.near - pin.z) / (pout.z - pin.z);
  const float lx = lin.x + t * (lout.x - lin.x), ly = lin.y + t * (lout.y - lin.y);
  return make_float4(m.fx * (lx / m.near) + m.cx, m.fy * (ly / m.near) + m.cy, m.near, 0.f);
}
// Sub-triangle `sub` of triangle (p0 p1 p2) after near-plane clipping; returns how many sub-triangles there are (0: entirely in
// front of the plane, 1: untouched or one vertex kept, 2: one vertex cut off -- the quad is split along the diagonal from the first
// cut to the second kept vertex)
__device__ __forceinline__ int near_clip(const float4* p, const float2* l, const MeshProj& m, int sub, float4& a, float4& b, float4& c) {
  const bool in0 = p[0].z >= m.near, in1 = p[1].z >= m.near, in2 = p[2].z >= m.near;
  const int n_in = (int)in0 + (int)in1 + (int)in2;
  if (n_in == 3) { a = p[0]; b = p[1]; c = p[2]; return 1; }
  if (n_in == 0) return 0;
  if (n_in == 1) {
    const int i = in0 ? 0 : (in1 ? 1 : 2), j = (i + 1) % 3, k = (i + 2) % 3;
    a = p[i]; b = near_cut(p[i], l[i], p[j], l[j], m); c = near_cut(p[i], l[i], p[k], l[k], m);
    return 1;
  }
  const int i = !in0 ? 0 : (!in1 ? 1 : 2), j = (i + 1) % 3, k = (i + 2) % 3;
  const float4 pj = near_cut(p[j], l[j], p[i], l[i], m);
  if (sub == 0) { a = pj; b = p[j]; c = p[k]; }
  else { a = pj; b = p[k]; c = near_cut(p[k], l[k], p[i], l[i], m); }
  return 2;
}

struct TriSetup { double ax, ay, bx, by, cx, cy; float za, zb, zc; int x0, y0, x1, y1; bool ok; };

// bounding box (inclusive pixel range) and validity of one projected triangle
__device__ __forceinline__ TriSetup tri_setup(const float4 a, const float4 b, const float4 c, int width, int height, float min_depth,
                                              float max_depth) {
  TriSetup t{};
  t.ok = false;
  if (a.z > max_depth && b.z > max_depth && c.z > max_depth) return t;
  if (!(isfinite(a.x) && isfinite(a.y) && isfinite(b.x) && isfinite(b.y) && isfinite(c.x) && isfinite(c.y))) return t;
  const float fx0 = fminf(a.x, fminf(b.x, c.x)), fx1 = fmaxf(a.x, fmaxf(b.x, c.x));
  const float fy0 = fminf(a.y, fminf(b.y, c.y)), fy1 = fmaxf(a.y, fmaxf(b.y, c.y));
  if (fx1 < 0.f || fy1 < 0.f || fx0 > (float)(width - 1) || fy0 > (float)(height - 1)) return t;
  t.x0 = max(0, (int)ceilf(fx0)); t.y0 = max(0, (int)ceilf(fy0));
  t.x1 = min(width - 1, (int)floorf(fx1)); t.y1 = min(height - 1, (int)floorf(fy1));
  if (t.x0 > t.x1 || t.y0 > t.y1) return t;
  t.ax = a.x; t.ay = a.y; t.bx = b.x; t.by = b.y; t.cx = c.x; t.cy = c.y;
  t.za = a.z; t.zb = b.z; t.zc = c.z;
  const double area = (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax);
  if (area == 0.0) return t;
  if (area < 0.0) {     // orient so that interior points have positive edge functions (culling is disabled)
    double d; float f;
    d = t.bx; t.bx = t.cx; t.cx = d; d = t.by; t.by = t.cy; t.cy = d; f = t.zb; t.zb = t.zc; t.zc = f;
  }
  t.ok = true;
  return t;
}
__device__ __forceinline__ bool edge_inside(double ax, double ay, double bx, double by, double px, double py, double& e) {
  const double dx = bx - ax, dy = by - ay;
  e = dx * (py - ay) - dy * (px - ax);
  if (e > 0.0) return true;
  if (e < 0.0) return false;
  return dy < 0.0 || (dy == 0.0 && dx > 0.0);        // top-left rule for samples exactly on an edge
}
// depth of the triangle at an integer pixel, or 0 if the pixel is outside / beyond the depth range
__device__ __forceinline__ float tri_depth(const TriSetup& t, int x, int y, float min_depth, float max_depth) {
  double e0, e1, e2;
  const bool in0 = edge_inside(t.bx, t.by, t.cx, t.cy, x, y, e0);
  const bool in1 = edge_inside(t.cx, t.cy, t.ax, t.ay, x, y, e1);
  const bool in2 = edge_inside(t.ax, t.ay, t.bx, t.by, x, y, e2);
  if (!(in0 && in1 && in2)) return 0.f;
  const double area = e0 + e1 + e2;
  if (!(area > 0.0)) return 0.f;
  const double inv = (e0 / (double)t.za + e1 / (double)t.zb + e2 / (double)t.zc) / area;      // interpolated 1/z
  const float z = (float)(1.0 / inv);
  if (!(z >= min_depth && z <= max_depth)) return 0.f;
  return z;
}

__global__ __launch_bounds__(kBlock) void k_mesh_bin(const float4* __restrict__ pv, const float2* __restrict__ pl,
                                                     const unsigned* __restrict__ tris, size_t n_tris, MeshProj mp,
                                                     int width, int height, float min_depth, float max_depth, int tiles_x,
                                                     unsigned tri_offset, unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                     unsigned* __restrict__ counter, unsigned capacity) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  int tx0[2] = {0, 0}, tx1[2] = {-1, -1}, ty0[2] = {0, 0}, ty1[2] = {-1, -1};
  unsigned count = 0;
  if (i < n_tris) {
    const unsigned i0 = tris[3 * i], i1 = tris[3 * i + 1], i2 = tris[3 * i + 2];
    const float4 p[3] = {pv[i0], pv[i1], pv[i2]};
    const float2 l[3] = {pl[i0], pl[i1], pl[i2]};
    int n_sub = 1;
    for (int sub = 0; sub < n_sub; ++sub) {        // sub-triangle 1 exists only where the near plane cuts off one vertex
      float4 a, b, c;
      n_sub = near_clip(p, l, mp, sub, a, b, c);
      if (sub >= n_sub) break;
      const TriSetup t = tri_setup(a, b, c, width, height, min_depth, max_depth);
      if (t.ok) {
        tx0[sub] = t.x0 / kTile; tx1[sub] = t.x1 / kTile; ty0[sub] = t.y0 / kTile; ty1[sub] = t.y1 / kTile;
        count += (unsigned)((tx1[sub] - tx0[sub] + 1) * (ty1[sub] - ty0[sub] + 1));
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned incl = count;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o); if (lane >= o) incl += v; }
  __shared__ unsigned wave_total[kBlock / kWave];
  __shared__ unsigned block_base;
  if (lane == 63) wave_total[wv] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tot = 0;
#pragma unroll
    for (int k = 0; k < kBlock / kWave; ++k) tot += wave_total[k];
    block_base = tot ? atomicAdd(counter, tot) : 0u;
  }
  __syncthreads();
  unsigned o = block_base + incl - count;
  for (int k = 0; k < wv; ++k) o += wave_total[k];
  for (int sub = 0; sub < 2; ++sub)
    for (int ty = ty0[sub]; ty <= ty1[sub]; ++ty)
      for (int tx = tx0[sub]; tx <= tx1[sub]; ++tx) {
        if (o < capacity) { keys[o] = (unsigned)(ty * tiles_x + tx); vals[o] = (tri_offset + (unsigned)i) | ((unsigned)sub << 31); }
        ++o;
      }
}

// one workgroup per tile, one LANE per triangle (occlusion meshes are fine: a triangle covers a few pixels)
__global__ __launch_bounds__(kBlock) void k_mesh_tiles(const float4* __restrict__ pv, const float2* __restrict__ pl,
                                                       const unsigned* __restrict__ tris, MeshProj mp,
                                                       const unsigned* __restrict__ vals, const unsigned* __restrict__ start,
                                                       const unsigned* __restrict__ end, int tiles_x, int width, int height,
                                                       float min_depth, float max_depth, unsigned* __restrict__ depth_bits) {
  __shared__ unsigned tile[kTile * kTile];
  const int t = blockIdx.x;
  const int x0 = (t % tiles_x) * kTile, y0 = (t / tiles_x) * kTile;
  for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) tile[i] = 0x7f800000u;
  __syncthreads();
  const unsigned s = start[t], e = end[t];
  for (unsigned j = s + threadIdx.x; j < e; j += kBlock) {
    const unsigned f = vals[j] & 0x7fffffffu;
    const int sub = (int)(vals[j] >> 31);            // second half of a triangle whose near-plane cut is a quad
    const unsigned i0 = tris[3 * (size_t)f], i1 = tris[3 * (size_t)f + 1], i2 = tris[3 * (size_t)f + 2];
    const float4 p[3] = {pv[i0], pv[i1], pv[i2]};
    const float2 l[3] = {pl[i0], pl[i1], pl[i2]};
    float4 a, b, c;
    if (sub >= near_clip(p, l, mp, sub, a, b, c)) continue;
    const TriSetup ts = tri_setup(a, b, c, width, height, min_depth, max_depth);
    if (!ts.ok) continue;
    const int bx0 = max(ts.x0, x0), by0 = max(ts.y0, y0), bx1 = min(ts.x1, x0 + kTile - 1), by1 = min(ts.y1, y0 + kTile - 1);
    for (int y = by0; y <= by1; ++y)
      for (int x = bx0; x <= bx1; ++x) {
        const float z = tri_depth(ts, x, y, min_depth, max_depth);
        if (z > 0.f) atomicMin(&tile[(y - y0) * kTile + (x - x0)], __float_as_uint(z));
      }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {
    const int x = x0 + (i & (kTile - 1)), y = y0 + (i / kTile);
    if (x < width && y < height) depth_bits[(size_t)y * width + x] = (tile[i] == 0x7f800000u) ? 0u : tile[i];     // no geometry: 0
  }
}

// ---- occlusion boundaries (ComputeEdgeNormalsList / FilterEdgeList :488-645, MaskOutOcclusionBoundaries :284-402) -------------

__global__ __launch_bounds__(kBlock) void k_face_normals(const float4* __restrict__ v, const unsigned* __restrict__ tris, size_t n_tris,
                                                         float4* __restrict__ normals, unsigned long long* __restrict__ keys,
                                                         unsigned* __restrict__ vals) {
  const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_tris) return;
  const unsigned i0 = tris[3 * f], i1 = tris[3 * f + 1], i2 = tris[3 * f + 2];
  const float4 p0 = v[i0], p1 = v[i1], p2 = v[i2];
  const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z, bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
  const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const float len = sqrtf(nx * nx + (ny * ny + nz * nz));
  normals[f] = (len > 0.f) ? make_float4(nx / len, ny / len, nz / len, 0.f) : make_float4(nx, ny, nz, 0.f);     // Eigen normalized()
  const unsigned e[3][2] = {{i0, i1}, {i1, i2}, {i2, i0}};
#pragma unroll
  for (int k = 0; k < 3; ++k) {       // AddHalfEdge :466-487: key (smaller, larger) vertex, value (face, swapped)
    const bool swap = e[k][0] > e[k][1];
    const unsigned lo = swap ? e[k][1] : e[k][0], hi = swap ? e[k][0] : e[k][1];
    keys[3 * f + k] = ((unsigned long long)lo << 32) | hi;
    vals[3 * f + k] = ((unsigned)f << 1) | (swap ? 1u : 0u);
  }
}

// one thread per group of equal keys (sorted; stable: faces in increasing index like the reference's insertion order)
__global__ __launch_bounds__(kBlock) void k_filter_edges(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                         size_t n, const float4* __restrict__ v, const float4* __restrict__ normals,
                                                         MeshEdge* __restrict__ edges, unsigned* __restrict__ n_edges) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  if (i > 0 && keys[i - 1] == key) return;                       // not the head of its group
  size_t j = i + 1;
  while (j < n && keys[j] == key) ++j;
  const size_t cnt = j - i;
  MeshEdge E;
  E.v1 = (unsigned)(key >> 32); E.v2 = (unsigned)key;
  E.f1 = vals[i] >> 1; E.f2 = 0xFFFFFFFFu; E.opposite = 0;
  bool keep = true;
  if (cnt >= 2) {
    const float kEpsilon = 1e-4f;
    float factor1 = (vals[i] & 1u) ? -1.f : 1.f, factor2 = (vals[i + 1] & 1u) ? -1.f : 1.f;
    const float4 s0 = v[E.v1], s1 = v[E.v2];
    const float ex = s1.x - s0.x, ey = s1.y - s0.y, ez = s1.z - s0.z;
    const float4 nA = normals[E.f1];
    const float n1x = nA.x * factor1, n1y = nA.y * factor1, n1z = nA.z * factor1;
    E.f2 = vals[i + 1] >> 1;
    const float4 nB = normals[E.f2];
    const float n2x = nB.x * factor2, n2y = nB.y * factor2, n2z = nB.z * factor2;
    E.opposite = (factor1 * factor2 > 0) ? 1 : 0;
    const float l1 = sqrtf(n1x * n1x + (n1y * n1y + n1z * n1z));
    const float bxx = n1x / l1, bxy = n1y / l1, bxz = n1z / l1;                                   // base_x = first_normal.normalized()
    float cyx = bxy * ez - bxz * ey, cyy = bxz * ex - bxx * ez, cyz = bxx * ey - bxy * ex;        // base_x x edge
    const float l2 = sqrtf(cyx * cyx + (cyy * cyy + cyz * cyz));
    cyx /= l2; cyy /= l2; cyz /= l2;
    float n1_2x = 1.f, n1_2y = 0.f;
    float n2_2x = bxx * n2x + (bxy * n2y + bxz * n2z), n2_2y = cyx * n2x + (cyy * n2y + cyz * n2z);
    if (n2_2x < 0 && fabsf(n2_2y) < kEpsilon) keep = false;                                        // coplanar faces: no edge
    else if (cnt > 2) {
      const float cross_n1n2 = n2_2y;
      for (size_t k = i + 2; k < j && keep; ++k) {
        const unsigned f3 = vals[k] >> 1;
        const float factor3 = (vals[k] & 1u) ? -1.f : 1.f;
        const float4 nC = normals[f3];
        const float cx = nC.x * factor3, cy = nC.y * factor3, cz = nC.z * factor3;
        const float n3x = bxx * cx + (bxy * cy + bxz * cz), n3y = cyx * cx + (cyy * cy + cyz * cz);
        const float cross_n1n3 = n1_2x * n3y - n1_2y * n3x;
        const float cross_n2n3 = n2_2x * n3y - n2_2y * n3x;
        const bool sign1 = cross_n1n3 * cross_n1n2 > 0;
        const bool sign2 = cross_n2n3 * cross_n1n2 < 0;
        if (sign1 && !sign2) { n2_2x = n3x; n2_2y = n3y; E.f2 = f3; factor2 = factor3; E.opposite = (factor1 * factor3 != 1) ? 1 : 0; }
        else if (sign2 && !sign1) { n1_2x = n3x; n1_2y = n3y; E.f1 = f3; factor1 = factor3; E.opposite = (factor3 * factor2 != 1) ? 1 : 0; }
        else if (!sign2 && !sign2) keep = false;              // [sic] the reference tests !sign2 twice (:631)
      }
    }
  }
  if (keep) edges[atomicAdd(n_edges, 1u)] = E;
}

// MaskOutOcclusionBoundaries: every silhouette (or boundary) edge that is visible splats -1 over the pixels it is not clearly
// behind.  The reference runs its edge loop under `omp parallel for` while reading the map it writes (:305-334), so its result
// depends on thread timing; here visibility and the per-pixel test read the UNMASKED depth map, which makes the result
// deterministic (a superset of any reference run's mask).
template <int M>
__global__ __launch_bounds__(kBlock) void k_mask_boundaries(const MeshEdge* __restrict__ edges, size_t n_edges, const float4* __restrict__ v,
                                                            const float4* __restrict__ normals, Pose P, float3 image_position,
                                                            CamLevel cam, float splat_radius, const float* __restrict__ depth_in,
                                                            float* __restrict__ depth_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_edges) return;
  const MeshEdge E = edges[i];
  const float4 p1 = v[E.v1], p2 = v[E.v2];
  if (E.f2 != 0xFFFFFFFFu) {
    const float tx = image_position.x - p1.x, ty = image_position.y - p1.y, tz = image_position.z - p1.z;
    const float4 na = normals[E.f1], nb = normals[E.f2];
    const bool face1 = (na.x * tx + (na.y * ty + na.z * tz)) > 0, face2 = (nb.x * tx + (nb.y * ty + nb.z * tz)) > 0;
    if (!((E.opposite && (face1 == face2)) || (face1 != face2 && !E.opposite))) return;
  }
  float a0, a1, a2, b0, b1, b2;
  rt(P, p1.x, p1.y, p1.z, a0, a1, a2);
  if (a2 <= 0) return;
  rt(P, p2.x, p2.y, p2.z, b0, b1, b2);
  if (b2 <= 0) return;
  const float d0 = b0 - a0, d1 = b1 - a1, d2 = b2 - a2;
  const int splat_point_count = 1 + min((int)(sqrtf(d0 * d0 + (d1 * d1 + d2 * d2)) / splat_radius + 0.5f), 150);
  const float kOcclusionDepthThreshold = 0.05f;
  for (int k = 0; k < splat_point_count; ++k) {
    const float factor = k / (splat_point_count - 1.0f);        // 0/0 = NaN for a single point, like the reference
    const float X = a0 + factor * d0, Y = a1 + factor * d1, Z = a2 + factor * d2;
    if (!(Z > 0)) continue;
    float px, py;
    const CamTheta th = cam_theta<M>(X / Z, Y / Z);
    cam_normalized_to_image<M>(cam, X / Z, Y / Z, th, px, py);
    const int ix = f2i(px + 0.5f), iy = f2i(py + 0.5f);
    if (!(px + 0.5f >= 0 && py + 0.5f >= 0 && ix >= 0 && iy >= 0 && ix < cam.width && iy < cam.height)) continue;
    if (!(depth_in[(size_t)iy * cam.width + ix] + kOcclusionDepthThreshold >= Z)) continue;
    float d[6];
    cam_image_deriv_by_world<M>(cam, X, Y, Z, th, d);
    const float rx = sqrtf(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])) * splat_radius;
    const float ry = sqrtf(d[3] * d[3] + (d[4] * d[4] + d[5] * d[5])) * splat_radius;
    const int min_x = max(0, d2i((double)((float)ix - rx) + 0.5)), min_y = max(0, d2i((double)((float)iy - ry) + 0.5));
    const int end_x = min(cam.width, d2i((double)((float)ix + rx) + 1.5)), end_y = min(cam.height, d2i((double)((float)iy + ry) + 1.5));
    for (int y = min_y; y < end_y; ++y)
      for (int x = min_x; x < end_x; ++x) {
        const float old_depth = depth_in[(size_t)y * cam.width + x];
        if (old_depth == 0 || old_depth + kOcclusionDepthThreshold > Z) depth_out[(size_t)y * cam.width + x] = -1.f;
      }
  }
}

// p[0 .. n) = v with 16-byte stores (p from hipMalloc: 256-byte aligned); the last n % 4 entries one by one
__global__ __launch_bounds__(kBlock) void k_fill_f32x4(float* __restrict__ p, size_t n, float v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n4 = n / 4;
  if (i < n4) reinterpret_cast<float4*>(p)[i] = make_float4(v, v, v, v);
  if (i < (n & 3)) p[4 * n4 + i] = v;
}
// nearest of two mesh depth maps; 0 = no geometry
__global__ __launch_bounds__(kBlock) void k_depth_merge(float* __restrict__ a, const float* __restrict__ b, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = a[i], y = b[i];
  a[i] = (x == 0.f) ? y : ((y == 0.f) ? x : fminf(x, y));
}

// 30-bit Morton code of a point in a 1024^3 lattice over the bounding box (NaN / out of range: clamped) -- only an ORDER for the
// splat points: the depth map is a minimum over them, whatever their order
__device__ __forceinline__ unsigned morton_spread10(unsigned v) {
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu; v = (v | (v << 8)) & 0x0300F00Fu; v = (v | (v << 4)) & 0x030C30C3u; v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__global__ __launch_bounds__(kBlock) void k_morton_keys(const float* __restrict__ xyz, size_t n, float ox, float oy, float oz, float inv,
                                                        unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float fx = (xyz[3 * i] - ox) * inv, fy = (xyz[3 * i + 1] - oy) * inv, fz = (xyz[3 * i + 2] - oz) * inv;
  const unsigned qx = (unsigned)fminf(fmaxf(fx, 0.f), 1023.f), qy = (unsigned)fminf(fmaxf(fy, 0.f), 1023.f), qz = (unsigned)fminf(fmaxf(fz, 0.f), 1023.f);
  keys[i] = morton_spread10(qx) | (morton_spread10(qy) << 1) | (morton_spread10(qz) << 2);
  vals[i] = (unsigned)i;
}
__global__ __launch_bounds__(kBlock) void k_gather_xyz_to_float4(const float* __restrict__ xyz, const unsigned* __restrict__ order, size_t n,
                                                                 float4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = order[i];
  out[i] = make_float4(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], 0.f);
}

// OcclusionGeometry::RenderDepthMap, mesh branch (:211-271): rasterise all meshes, then mask the occlusion boundaries
static void render_depth_meshes(e3d_reg* h, ImageDev& im, const Intrin& in, const CamLevel& cam) {
  hipStream_t s = h->stream;
  const size_t px = (size_t)cam.width * cam.height;
  const int tiles_x = (int)div_up(cam.width, kTile), tiles_y = (int)div_up(cam.height, kTile);
  const size_t n_tiles = (size_t)tiles_x * tiles_y;
  size_t total_tris = 0, max_vertices = 0;
  for (auto& m : h->renderer.meshes) { total_tris += m->n_triangles; max_vertices = std::max(max_vertices, m->n_vertices); }
  if (total_tris >= ((size_t)1 << 31)) throw Error(E3D_ERR_INVALID, "more than 2^31 occlusion triangles");
  h->renderer.sp_counter.reserve(1); h->renderer.tile_start.reserve(n_tiles); h->renderer.tile_end.reserve(n_tiles);
  // depth of all meshes = min over meshes; each mesh is binned, sorted and reduced on its own into im.depth
  DevBuf<float>& D = (h->renderer.mask_occlusion_boundaries ? h->renderer.depth_unmasked : im.depth);
  D.reserve(px);
  bool first = true;
  for (auto& m : h->renderer.meshes) {
    h->renderer.mesh_projected.reserve(m->n_vertices); h->renderer.mesh_shaded.reserve(m->n_vertices);
    E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_mesh_vertices<M>, dim3(nblk(m->n_vertices)), dim3(kBlock), 0, s, m->vertices.p,
                                               m->n_vertices, im.pose, cam, h->renderer.mesh_projected.p, h->renderer.mesh_shaded.p));
    const MeshProj mp{cam.fx, cam.fy, cam.cx, cam.cy, h->renderer.min_occlusion_depth};
    // capacity: most triangles touch one tile; retried with the exact count if the first guess was too small
    size_t capacity = m->n_triangles + m->n_triangles / 2 + 1024;
    unsigned n_pairs = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      for (int k = 0; k < 2; ++k) { h->renderer.sp_keys[k].reserve(capacity); h->renderer.sp_vals[k].reserve(capacity); }
      E3D_HIP(hipMemsetAsync(h->renderer.sp_counter.p, 0, sizeof(unsigned), s));
      hipLaunchKernelGGL(k_mesh_bin, dim3(nblk(m->n_triangles)), dim3(kBlock), 0, s, h->renderer.mesh_projected.p, h->renderer.mesh_shaded.p, m->triangles.p,
                         m->n_triangles, mp, cam.width, cam.height, h->renderer.min_occlusion_depth, h->renderer.max_occlusion_depth, tiles_x, 0u, h->renderer.sp_keys[0].p,
                         h->renderer.sp_vals[0].p, h->renderer.sp_counter.p, (unsigned)std::min<size_t>(capacity, 0xFFFFFFFFu));
      read_back(h, &n_pairs, h->renderer.sp_counter.p, sizeof n_pairs);
      if ((size_t)n_pairs <= capacity) break;
      capacity = n_pairs;
    }
    E3D_HIP(hipMemsetAsync(h->renderer.tile_start.p, 0, sizeof(unsigned) * n_tiles, s));
    E3D_HIP(hipMemsetAsync(h->renderer.tile_end.p, 0, sizeof(unsigned) * n_tiles, s));
    if (n_pairs) {
      int bits = 1;
      while (((size_t)1 << bits) < n_tiles) ++bits;
      sort_pairs_u32_u32(h->renderer.sp_keys[0].p, h->renderer.sp_keys[1].p, h->renderer.sp_vals[0].p, h->renderer.sp_vals[1].p, n_pairs, bits, h->renderer.sort_temp, s);
      hipLaunchKernelGGL(k_tile_ranges, dim3(nblk(n_pairs)), dim3(kBlock), 0, s, h->renderer.sp_keys[1].p, (size_t)n_pairs, h->renderer.tile_start.p, h->renderer.tile_end.p);
    }
    DevBuf<float>& target = first ? D : h->renderer.ztmp_f;
    target.reserve(px);
    hipLaunchKernelGGL(k_mesh_tiles, dim3((unsigned)n_tiles), dim3(kBlock), 0, s, h->renderer.mesh_projected.p, h->renderer.mesh_shaded.p, m->triangles.p, mp,
                       h->renderer.sp_vals[1].p,
                       h->renderer.tile_start.p, h->renderer.tile_end.p, tiles_x, cam.width, cam.height, h->renderer.min_occlusion_depth, h->renderer.max_occlusion_depth,
                       reinterpret_cast<unsigned*>(target.p));
    if (!first) hipLaunchKernelGGL(k_depth_merge, dim3(nblk(px)), dim3(kBlock), 0, s, D.p, h->renderer.ztmp_f.p, px);
    first = false;
  }
  if (h->renderer.mask_occlusion_boundaries) {
    E3D_HIP(hipMemcpyAsync(im.depth.p, D.p, sizeof(float) * px, hipMemcpyDeviceToDevice, s));
    // image position = global_T_image.translation() = -R^T t
    const float* R = im.pose.R; const float* t = im.pose.t;
    float3 pos;
    pos.x = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]); pos.y = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]); pos.z = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
    for (auto& m : h->renderer.meshes)
      if (m->n_edges)
        E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_mask_boundaries<M>, dim3(nblk(m->n_edges)), dim3(kBlock), 0, s, m->edges.p, m->n_edges,
                                                   m->vertices.p, m->normals.p, im.pose, pos, cam, h->prm.splat_radius, D.p, im.depth.p));
  }
}

// OcclusionGeometry::RenderDepthMap of one image at one image scale into im.depth: the meshes, or the splat points as squares
// (z-buffer of the points, tiles of the small splats, minimum filter); depth_out (host, may be null) gets a copy
void render_depth(e3d_reg* h, int image_id, int image_scale, float* depth_out) {
  ImageDev& im = get_image(h, image_id);
  if (!h->owns(image_id)) throw Error(E3D_ERR_INVALID, fmt("image %d belongs to rank %d", image_id, image_owner(h, image_id)));
  const Intrin& in = h->intr.at(im.intrinsics_id);
  const int lvl = std::max(0, image_scale - in.min_image_scale);
  if (lvl >= (int)in.levels.size()) throw Error(E3D_ERR_INDEX, "image scale beyond the pyramid");
  const CamLevel& cam = in.levels[lvl];
  const size_t px = (size_t)cam.width * cam.height;
  im.depth.reserve(px);
  if (h->renderer.n_splat == 0 && !h->renderer.meshes.empty()) {
    double tris = 0;
    for (auto& m : h->renderer.meshes) tris += (double)m->n_triangles;
    KT kt(h, "depth.mesh_raster", tris);
    render_depth_meshes(h, im, in, cam);
  } else if (h->renderer.n_splat == 0) {
    // no occlusion geometry: everything is visible (occlusion_geometry.cc:272-281)
    fill_f32(im.depth.p, px, INFINITY, h->stream);
  } else {
    hipStream_t s = h->stream;
    const size_t n = h->renderer.n_splat;
    const int tiles_x = (int)div_up(cam.width, kTile), tiles_y = (int)div_up(cam.height, kTile);
    const size_t n_tiles = (size_t)tiles_x * tiles_y;
    if (cam.width > 65535 || cam.height > 65535) throw Error(E3D_ERR_INVALID, "image too large");
    h->renderer.rects.reserve(n);
    for (int k = 0; k < 2; ++k) { h->renderer.sp_keys[k].reserve(4 * n); h->renderer.sp_vals[k].reserve(4 * n); }
    h->renderer.sp_counter.reserve(1); h->renderer.tile_start.reserve(n_tiles); h->renderer.tile_end.reserve(n_tiles);
    E3D_HIP(hipMemsetAsync(h->renderer.sp_counter.p, 0, sizeof(unsigned), s));
    E3D_HIP(hipMemsetAsync(h->renderer.tile_start.p, 0, sizeof(unsigned) * n_tiles, s));
    E3D_HIP(hipMemsetAsync(h->renderer.tile_end.p, 0, sizeof(unsigned) * n_tiles, s));
    unsigned n_pairs = 0;
    const bool separable = reg_switches().separable_min_filter;
    const size_t zpx = (size_t)(cam.width + 2 * kSplatMax) * (cam.height + 2 * kSplatMax);
    h->renderer.zbuf.reserve(zpx);
    {
      KT kt(h, "depth.zbuffer_clear", (double)zpx);
      hipLaunchKernelGGL(k_fill_f32x4, dim3(nblk(zpx / 4 + 4)), dim3(kBlock), 0, s, reinterpret_cast<float*>(h->renderer.zbuf.p), zpx, INFINITY);
    }
    if (n) {
      {
        KT kt(h, "depth.splat_bin", (double)n);
        E3D_CAM_SWITCH(in.type, hipLaunchKernelGGL(k_splat_bin<M>, dim3(nblk(n)), dim3(kBlock), 0, s, h->renderer.splat.p, n, im.pose, cam,
                                                   h->prm.splat_radius, tiles_x, h->renderer.rects.p, h->renderer.sp_keys[0].p, h->renderer.sp_vals[0].p,
                                                   h->renderer.sp_counter.p, h->renderer.zbuf.p));
      }
      read_back(h, &n_pairs, h->renderer.sp_counter.p, sizeof n_pairs);
    }
    {
      KT kt(h, "depth.small_splat_tiles", (double)n_pairs);
      if (n_pairs) {
        int bits = 1;
        while (((size_t)1 << bits) < n_tiles) ++bits;
        sort_pairs_u32_u32(h->renderer.sp_keys[0].p, h->renderer.sp_keys[1].p, h->renderer.sp_vals[0].p, h->renderer.sp_vals[1].p, n_pairs, bits, h->renderer.sort_temp, s);
        hipLaunchKernelGGL(k_tile_ranges, dim3(nblk(n_pairs)), dim3(kBlock), 0, s, h->renderer.sp_keys[1].p, (size_t)n_pairs, h->renderer.tile_start.p,
                           h->renderer.tile_end.p);
      }
      if (n_pairs || separable)
      hipLaunchKernelGGL(k_splat_tiles, dim3((unsigned)n_tiles), dim3(kBlock), 0, s, h->renderer.rects.p, h->renderer.sp_vals[1].p, h->renderer.tile_start.p,
                         h->renderer.tile_end.p, tiles_x, cam.width, cam.height, reinterpret_cast<unsigned*>(im.depth.p));
    }
    {
      KT kt(h, "depth.min_filter", (double)px);
      if (separable) {
        h->renderer.ztmp.reserve((size_t)cam.width * (cam.height + 2 * kSplatMax));
        hipLaunchKernelGGL(k_min_filter_h, dim3((unsigned)div_up(cam.width, kBlock), (unsigned)(cam.height + 2 * kSplatMax)), dim3(kBlock), 0, s,
                           h->renderer.zbuf.p, cam.width, cam.height, h->renderer.ztmp.p);
        hipLaunchKernelGGL(k_min_filter_v, dim3((unsigned)div_up(cam.width, kBlock), (unsigned)cam.height), dim3(kBlock), 0, s, h->renderer.ztmp.p,
                           cam.width, cam.height, reinterpret_cast<unsigned*>(im.depth.p));
      } else {
        const dim3 mf_grid((unsigned)div_up(cam.width, kMfW), (unsigned)div_up(cam.height, kMfH));
        if (n_pairs) hipLaunchKernelGGL(k_min_filter_tile<true>, mf_grid, dim3(kBlock), 0, s, h->renderer.zbuf.p, cam.width, cam.height, reinterpret_cast<unsigned*>(im.depth.p));
        else hipLaunchKernelGGL(k_min_filter_tile<false>, mf_grid, dim3(kBlock), 0, s, h->renderer.zbuf.p, cam.width, cam.height, reinterpret_cast<unsigned*>(im.depth.p));
      }
    }
  }
  if (depth_out) { copy_out(depth_out, im.depth.p, sizeof(float) * px, h->stream); rsync(h); }     // (else: every reader runs on the stream)
  im.depth_scale = image_scale;
}

}  // namespace e3d

extern "C" {

/* OcclusionGeometry::AddMesh / AddSplats (occlusion_geometry.cc:64-182): one more triangle mesh (vertices already in the
 * global frame).  compute_edges != 0 also extracts the edges used for masking occlusion boundaries (meshes: yes, splat
 * geometry: no). */
int e3d_reg_add_occlusion_mesh(e3d_reg_t* h, const float* vertices, size_t n_vertices, const uint32_t* triangles, size_t n_triangles,
                               int compute_edges) {
  E3D_TRY_ON(h)
  if (!h || !vertices || !triangles || !n_vertices || !n_triangles) throw Error(E3D_ERR_INVALID, "empty mesh");
  if (n_triangles >= ((size_t)1 << 31) || n_vertices >= ((size_t)1 << 32)) throw Error(E3D_ERR_INVALID, "mesh too large");
  hipStream_t s = h->stream;
  std::unique_ptr<MeshDev> m(new MeshDev());
  m->n_vertices = n_vertices; m->n_triangles = n_triangles;
  DevBuf<float> tmp; tmp.reserve(3 * n_vertices);
  copy_in(tmp.p, vertices, sizeof(float) * 3 * n_vertices, s);
  m->vertices.reserve(n_vertices);
  xyz_to_float4(tmp.p, n_vertices, m->vertices.p, s);
  m->triangles.reserve(3 * n_triangles);
  copy_in(m->triangles.p, triangles, sizeof(unsigned) * 3 * n_triangles, s);
  rsync(h);
  for (size_t i = 0; i < 3 * n_triangles; ++i) if (triangles[i] >= n_vertices) throw Error(E3D_ERR_INDEX, "triangle refers to a missing vertex");
  if (compute_edges) {
    const size_t ne = 3 * n_triangles;
    DevBuf<unsigned long long> ka, kb;
    DevBuf<unsigned> va, vb, cnt;
    ka.reserve(ne); kb.reserve(ne); va.reserve(ne); vb.reserve(ne); cnt.reserve(1);
    m->normals.reserve(n_triangles);
    hipLaunchKernelGGL(k_face_normals, dim3(nblk(n_triangles)), dim3(kBlock), 0, s, m->vertices.p, m->triangles.p, n_triangles, m->normals.p,
                       ka.p, va.p);
    sort_pairs_u64_u32(ka.p, kb.p, va.p, vb.p, ne, 64, h->renderer.sort_temp, s);
    m->edges.reserve(ne);
    E3D_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_filter_edges, dim3(nblk(ne)), dim3(kBlock), 0, s, kb.p, vb.p, ne, m->vertices.p, m->normals.p, m->edges.p, cnt.p);
    unsigned n_edges = 0;
    copy_out(&n_edges, cnt.p, sizeof n_edges, s);
    rsync(h);
    m->n_edges = n_edges;
  }
  h->renderer.meshes.push_back(std::move(m));
  for (auto& kv : h->images) kv.second.depth_scale = -1;
  return (int)h->renderer.meshes.size();
  E3D_CATCH()
}
int e3d_reg_clear_occlusion_meshes(e3d_reg_t* h) {
  E3D_TRY_ON(h)
  if (!h) throw Error(E3D_ERR_INVALID, "null handle");
  h->renderer.meshes.clear();
  for (auto& kv : h->images) kv.second.depth_scale = -1;
  return 0;
  E3D_CATCH()
}
/* min_occlusion_depth / max_occlusion_depth (near / far plane of the mesh renderer) and mask_occlusion_boundaries of
 * OcclusionGeometry::RenderDepthMap (occlusion_geometry.h:80-86); defaults 0.05, 100, true */
int e3d_reg_set_occlusion_options(e3d_reg_t* h, float min_depth, float max_depth, int mask_occlusion_boundaries) {
  E3D_TRY_ON(h)
  if (!h || !(min_depth > 0) || !(max_depth > min_depth)) throw Error(E3D_ERR_INVALID, "bad occlusion depth range");
  h->renderer.min_occlusion_depth = min_depth; h->renderer.max_occlusion_depth = max_depth; h->renderer.mask_occlusion_boundaries = mask_occlusion_boundaries != 0;
  return 0;
  E3D_CATCH()
}
int64_t e3d_reg_occlusion_edge_count(e3d_reg_t* h, int mesh_index) {
  E3D_TRY_ON(h)
  if (!h || mesh_index < 0 || mesh_index >= (int)h->renderer.meshes.size()) throw Error(E3D_ERR_INDEX, "no such mesh");
  return (int64_t)h->renderer.meshes[mesh_index]->n_edges;
  E3D_CATCH()
}

int e3d_reg_set_splat_points(e3d_reg_t* h, const float* xyz, size_t n) {
  E3D_TRY_ON(h)
  if (!h || (!xyz && n)) throw Error(E3D_ERR_INVALID, "null argument");
  DevBuf<float> tmp; tmp.reserve(3 * n);
  copy_in(tmp.p, xyz, sizeof(float) * 3 * n, h->stream);
  h->renderer.splat.reserve(n);
  // The splat points are only ever reduced to a depth map (a minimum: order free), so the library keeps them in Morton order of
  // their positions: neighbouring threads of k_splat_bin then hit neighbouring pixels, and the one atomicMin per point lands in
  // cache lines other lanes of the wave touch too (measured: 0.41 -> see DESIGN 10.3 ms per 10 M points of a 24 MP image with the
  // points in random order before).  E3D_REG_SPLAT_ORDER=0 keeps the caller's order.
  if (reg_switches().splat_order && n > 1 && n < ((size_t)1 << 32)) {
    hipStream_t s = h->stream;
    DevBuf<float> bbp, bbo;
    bbp.reserve(6 * (size_t)kMaxBboxBlocks); bbo.reserve(6);
    launch_bbox_aos(tmp.p, n, bbp.p, bbo.p, s);
    float bb[6];
    copy_out(bb, bbo.p, sizeof bb, s);
    rsync(h);
    float ext = 0.f;
    for (int k = 0; k < 3; ++k) ext = std::max(ext, bb[3 + k] - bb[k]);
    const float inv = (ext > 0.f && std::isfinite(ext)) ? 1023.f / ext : 0.f;
    for (int k = 0; k < 2; ++k) { h->renderer.sp_keys[k].reserve(n); h->renderer.sp_vals[k].reserve(n); }
    hipLaunchKernelGGL(k_morton_keys, dim3(nblk(n)), dim3(kBlock), 0, s, tmp.p, n, std::isfinite(bb[0]) ? bb[0] : 0.f, std::isfinite(bb[1]) ? bb[1] : 0.f,
                       std::isfinite(bb[2]) ? bb[2] : 0.f, inv, h->renderer.sp_keys[0].p, h->renderer.sp_vals[0].p);
    sort_pairs_u32_u32(h->renderer.sp_keys[0].p, h->renderer.sp_keys[1].p, h->renderer.sp_vals[0].p, h->renderer.sp_vals[1].p, n, 30, h->renderer.sort_temp, s);
    hipLaunchKernelGGL(k_gather_xyz_to_float4, dim3(nblk(n)), dim3(kBlock), 0, s, tmp.p, h->renderer.sp_vals[1].p, n, h->renderer.splat.p);
  } else {
    xyz_to_float4(tmp.p, n, h->renderer.splat.p, h->stream);
  }
  rsync(h);
  h->renderer.n_splat = n;
  return 0;
  E3D_CATCH()
}

int e3d_reg_render_depth(e3d_reg_t* h, int image_id, int image_scale, float* depth_out) {
  E3D_TRY_ON(h)
  if (!h) throw Error(E3D_ERR_INVALID, "null handle");
  render_depth(h, image_id, image_scale, depth_out);
  return 0;
  E3D_CATCH()
}

}  // extern "C"
