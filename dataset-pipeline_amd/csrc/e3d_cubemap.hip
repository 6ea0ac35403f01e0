// e3d_cubemap.hip -- CubeMapRenderer (src/exe/cube_map_renderer.cc:161-373): the six pinhole faces of a coloured laser scan,
// z-buffered, slightly filled in, and the colour dilated until every pixel has one.  DESIGN.md section 15.
//
// Every result equals a serial execution bit for bit: the arithmetic is f32 with a fixed operation order (this file is built
// with -ffp-contract=off and the correctly rounded divide), integer sums and comparisons.
//
// Point pass (:238-258).  One read of the cloud serves all six faces.  The rows of the face matrices are signed unit vectors, so
// for a finite point R p is a signed permutation of p (exact; the sign of a zero plays no part: a zero depth is skipped and
// fx * (+-0) / z + cx = cx).  The reference's strict `<` against the stored depth, applied in file order, keeps per pixel the
// lowest depth and among equal depths the lowest point index: exactly the minimum of (bits of depth) << 32 | index -- positive
// floats order as their bits -- which one 64-bit unsigned atomic minimum per accepted (point, face) pair computes in any
// arrival order.  All ones = no point.
//
// Fill-in pass 1 (:260-319), then the colour dilation (:321-373) as Jacobi sweeps over two buffers of packed pixels
// (R | G << 8 | B << 16 | valid << 24).  A sweep writes every pixel of its face, so after a sweep that validated nothing both
// buffers hold the same face.  Every sweep leaves a word per face: "validated at least one pixel"; the blocks of the next sweep
// read the word of the one before and return at once when it is zero.  A face therefore stops on the device, on its own, and
// the host may launch sweeps in batches and look at the words once per batch.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/e3d_hip.h"
#include "e3d_common.hpp"

namespace e3d {

constexpr unsigned long long kNoPoint = ~0ull;
constexpr unsigned kValidBit = 0x01000000u, kRgbMask = 0x00ffffffu;
constexpr int kSweepTileX = 64, kSweepTileY = 4;      // one row segment of 256 B per wave
constexpr int kSweepWords = 8;                         // words per sweep in the flag array (six used)

// r = R_face p (:165-225): front, left, back, right, down, up
__device__ __forceinline__ void face_coords(int face, float x, float y, float z, float& rx, float& ry, float& rz) {
  switch (face) {
    case 0: rx = x; ry = y; rz = z; break;
    case 1: rx = z; ry = y; rz = -x; break;
    case 2: rx = -x; ry = y; rz = -z; break;
    case 3: rx = -z; ry = y; rz = x; break;
    case 4: rx = x; ry = -z; rz = y; break;
    default: rx = x; ry = z; rz = -y; break;
  }
}

__global__ __launch_bounds__(256) void k_cube_points(const float* __restrict__ xyz, unsigned n, int size, float half,
                                                     unsigned long long* __restrict__ keys) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
  // a non-finite coordinate makes every component of R p NaN in the reference (0 * inf): the point lands nowhere
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
  const float fsize = (float)size;
  const size_t face_px = (size_t)size * size;
#pragma unroll
  for (int face = 0; face < 6; ++face) {
    float rx, ry, rz;
    face_coords(face, x, y, z, rx, ry, rz);
    if (rz <= 0.f) continue;
    const float px = (half * rx) / rz + half;
    const float py = (half * ry) / rz + half;
    // (int) truncates toward zero: (-1, 0) is column 0.  The test is on the float -- the conversion of an out-of-range or
    // NaN value is not INT_MIN on this chip
    if (!(px > -1.f && px < fsize && py > -1.f && py < fsize)) continue;
    const int ix = (int)px, iy = (int)py;
    const unsigned long long key = ((unsigned long long)__float_as_uint(rz) << 32) | i;
    atomicMin(&keys[face * face_px + (size_t)iy * size + ix], key);
  }
}

// keys -> depth (+inf where empty) and packed colour (0 where empty; no valid bit yet)
__global__ __launch_bounds__(256) void k_cube_resolve(const unsigned long long* __restrict__ keys, const unsigned char* __restrict__ rgb,
                                                      size_t n_px, float* __restrict__ depth, unsigned* __restrict__ color) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_px) return;
  const unsigned long long k = keys[p];
  float d = INFINITY;
  unsigned c = 0;
  if (k != kNoPoint) {
    d = __uint_as_float((unsigned)(k >> 32));
    const size_t i = (size_t)(unsigned)k;
    c = (unsigned)rgb[3 * i] | ((unsigned)rgb[3 * i + 1] << 8) | ((unsigned)rgb[3 * i + 2] << 16);
  }
  depth[p] = d;
  color[p] = c;
}

__device__ __forceinline__ void cswap(float& a, float& b) { const float lo = fminf(a, b), hi = fmaxf(a, b); a = lo; b = hi; }

// (uint8)(sum / (1.f * m) + 0.5f) per channel
__device__ __forceinline__ unsigned mean_color(int r, int g, int b, int m) {
  const float fm = 1.f * (float)m;
  const unsigned cr = (unsigned)(unsigned char)((float)r / fm + 0.5f);
  const unsigned cg = (unsigned)(unsigned char)((float)g / fm + 0.5f);
  const unsigned cb = (unsigned)(unsigned char)((float)b / fm + 0.5f);
  return cr | (cg << 8) | (cb << 16);
}

// :260-319 and the validity map of :321-327.  One thread per pixel; grid (x tiles, y tiles, 6).
__global__ __launch_bounds__(kSweepTileX* kSweepTileY) void k_cube_fill(const float* __restrict__ depth, const unsigned* __restrict__ color, int size,
                                                                        float* __restrict__ fdepth, unsigned* __restrict__ fcolor,
                                                                        unsigned* __restrict__ flags) {
  const int x = blockIdx.x * kSweepTileX + threadIdx.x, y = blockIdx.y * kSweepTileY + threadIdx.y, face = blockIdx.z;
  const size_t base = (size_t)face * size * size;
  bool no_color = false;
  if (x < size && y < size) {
    const size_t p = base + (size_t)y * size + x;
    float d = INFINITY;          // border pixels: +inf even where a point was rendered
    unsigned c = 0;              // ... and black (the reference leaves them uninitialised)
    if (x >= 1 && y >= 1 && x < size - 1 && y < size - 1) {
      d = depth[p];
      c = color[p];
      if (isinf(d)) {
        float buf[7] = {INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY};
        int m = 0, r = 0, g = 0, b = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const size_t q = base + (size_t)(y + dy) * size + (x + dx);
            const float nd = depth[q];
            if (!isinf(nd)) {
              const unsigned nc = color[q];
              // the first seven in row-major order (the eighth is never used)
#pragma unroll
              for (int s = 0; s < 7; ++s) if (s == m) buf[s] = nd;
              r += nc & 0xff; g += (nc >> 8) & 0xff; b += (nc >> 16) & 0xff;
              ++m;
            }
          }
        if (m >= 2) {
          // 2: the smaller; 3-4 / 5-6 / 7-8: the median of the first 3 / 5 / 7.  Unused slots are set to +inf and the
          // seven values sorted (odd-even transposition): the median of the first k = 2 j + 1 is element j
          const int used = (m == 2) ? 2 : (m <= 4 ? 3 : (m <= 6 ? 5 : 7));
#pragma unroll
          for (int s = 0; s < 7; ++s) if (s >= used) buf[s] = INFINITY;
#pragma unroll
          for (int round = 0; round < 7; ++round)
#pragma unroll
            for (int s = round & 1; s + 1 < 7; s += 2) cswap(buf[s], buf[s + 1]);
          const int pick = (m == 2) ? 0 : used / 2;
          float v = buf[0];
#pragma unroll
          for (int s = 1; s < 4; ++s) if (s == pick) v = buf[s];
          d = v;
        }
        if (m > 0) c = mean_color(r, g, b, m);
        else no_color = true;
      }
    }
    fdepth[p] = d;
    fcolor[p] = (c & kRgbMask) | (isinf(d) ? 0u : kValidBit);
  }
  if (__syncthreads_or(no_color) && threadIdx.x == 0 && threadIdx.y == 0) flags[face] = 1u;      // "have_invalid_color_pixels"
}

// One Jacobi sweep (:328-373) of the faces whose previous sweep (sweep 0: pass 1) left its word set.
__global__ __launch_bounds__(kSweepTileX* kSweepTileY) void k_cube_sweep(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int size,
                                                                         const unsigned* __restrict__ prev_flags, unsigned* __restrict__ flags) {
  const int face = blockIdx.z;
  if (prev_flags[face] == 0u) return;
  const int x = blockIdx.x * kSweepTileX + threadIdx.x, y = blockIdx.y * kSweepTileY + threadIdx.y;
  const size_t base = (size_t)face * size * size;
  bool validated = false;
  if (x < size && y < size) {
    const size_t p = base + (size_t)y * size + x;
    unsigned c = src[p];
    if (!(c & kValidBit)) {
      int m = 0, r = 0, g = 0, b = 0;
      const int y0 = max(0, y - 1), y1 = min(size - 1, y + 1), x0 = max(0, x - 1), x1 = min(size - 1, x + 1);
      for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) {
          if (xx == x && yy == y) continue;
          const unsigned nc = src[base + (size_t)yy * size + xx];
          if (nc & kValidBit) { r += nc & 0xff; g += (nc >> 8) & 0xff; b += (nc >> 16) & 0xff; ++m; }
        }
      if (m > 0) { c = mean_color(r, g, b, m) | kValidBit; validated = true; }
    }
    dst[p] = c;
  }
  if (__syncthreads_or(validated) && threadIdx.x == 0 && threadIdx.y == 0) flags[face] = 1u;
}

// packed pixels -> R, G, B bytes; four pixels (three words) per thread
__global__ __launch_bounds__(256) void k_cube_unpack(const unsigned* __restrict__ color, size_t n_px, unsigned char* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t p = 4 * t;
  if (p >= n_px) return;
  if (p + 4 <= n_px) {
    const unsigned a = color[p] & kRgbMask, b = color[p + 1] & kRgbMask, c = color[p + 2] & kRgbMask, d = color[p + 3] & kRgbMask;
    unsigned* o = reinterpret_cast<unsigned*>(out + 3 * p);       // 12 t bytes: word aligned
    o[0] = a | (b << 24);
    o[1] = (b >> 8) | (c << 16);
    o[2] = (c >> 16) | (d << 8);
  } else {
    for (size_t q = p; q < n_px; ++q) {
      const unsigned a = color[q];
      out[3 * q] = (unsigned char)a; out[3 * q + 1] = (unsigned char)(a >> 8); out[3 * q + 2] = (unsigned char)(a >> 16);
    }
  }
}

static thread_local float g_cube_timings[E3D_CUBE_MAP_TIMINGS] = {0};

static int sweep_batch_setting() {
  // sweeps launched per look at the flag words (1: one synchronisation per sweep, for A / B timing)
  static const int b = [] { const char* e = getenv("E3D_CUBEMAP_BATCH"); const int v = e ? atoi(e) : 32; return std::min(std::max(v, 1), 1024); }();
  return b;
}

}  // namespace e3d

using namespace e3d;

extern "C" int e3d_render_cube_map(const float* xyz, const uint8_t* rgb, size_t n, int size, int fill, uint8_t* color_out,
                                   float* depth_out, int32_t* sweeps_out) {
  E3D_TRY
  if ((!xyz && n) || (!rgb && n) || !color_out || !depth_out) throw Error(E3D_ERR_INVALID, "e3d_render_cube_map: null argument");
  if (size < 3) throw Error(E3D_ERR_INVALID, fmt("e3d_render_cube_map: size %d, need at least 3", size));
  if (size > 16384) throw Error(E3D_ERR_INVALID, fmt("e3d_render_cube_map: size %d, at most 16384", size));
  if (n >= ((size_t)1 << 31)) throw Error(E3D_ERR_INVALID, "e3d_render_cube_map: more than 2^31-1 points");
  require_device();
  OwnedStream stream;
  hipStream_t s = stream.s;

  const size_t face_px = (size_t)size * size, n_px = 6 * face_px;
  const int batch = sweep_batch_setting();
  const int max_sweeps = size;                 // the largest Chebyshev distance inside a face is size - 1; one more sweep finds nothing
  const size_t n_flag_words = (size_t)kSweepWords * ((size_t)max_sweeps + batch + 2);
  DevBuf<float> X, D, FD;
  DevBuf<unsigned char> C, OUT;
  DevBuf<unsigned long long> K;
  DevBuf<unsigned> P0, P1, FL;
  EventTimer t_points, t_resolve, t_fill, t_sweeps;
  X.reserve(3 * n); C.reserve(3 * n); K.reserve(n_px); D.reserve(n_px); P0.reserve(n_px); OUT.reserve(3 * n_px + 16);
  copy_in(X.p, xyz, sizeof(float) * 3 * n, s);
  copy_in(C.p, rgb, 3 * n, s);

  t_points.start(s);
  E3D_HIP(hipMemsetAsync(K.p, 0xFF, sizeof(unsigned long long) * n_px, s));
  if (n) hipLaunchKernelGGL(k_cube_points, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, X.p, (unsigned)n, size, (float)(size / 2), K.p);
  t_points.stop(s);
  t_resolve.start(s);
  hipLaunchKernelGGL(k_cube_resolve, dim3((unsigned)div_up(n_px, 256)), dim3(256), 0, s, K.p, C.p, n_px, D.p, P0.p);
  t_resolve.stop(s);
  E3D_HIP(hipGetLastError());

  int32_t sweeps[6] = {0, 0, 0, 0, 0, 0};
  int n_batches = 0, n_launched = 0;
  const float* depth_final = D.p;
  const unsigned* color_final = P0.p;
  if (fill) {
    FD.reserve(n_px); P1.reserve(n_px); FL.reserve(n_flag_words);
    K.release();                                                     // the keys are resolved
    DevBuf<unsigned> P2;
    P2.reserve(n_px);
    E3D_HIP(hipMemsetAsync(FL.p, 0, sizeof(unsigned) * n_flag_words, s));
    const dim3 grid((unsigned)div_up(size, kSweepTileX), (unsigned)div_up(size, kSweepTileY), 6), block(kSweepTileX, kSweepTileY);
    t_fill.start(s);
    hipLaunchKernelGGL(k_cube_fill, grid, block, 0, s, D.p, P0.p, size, FD.p, P1.p, FL.p);
    t_fill.stop(s);
    E3D_HIP(hipGetLastError());
    // sweep k (1-based) reads buffer (k - 1) & 1 and writes k & 1 of {P1, P2}; its word row is k
    unsigned* buf[2] = {P1.p, P2.p};
    PinBuf<unsigned> mailbox;
    mailbox.reserve((size_t)kSweepWords * (batch + 1));
    t_sweeps.start(s);
    int done = 0;                               // sweeps launched and looked at
    bool more = true;
    // row 0 (pass 1) decides whether anything is launched at all
    E3D_HIP(hipMemcpyAsync(mailbox.p, FL.p, sizeof(unsigned) * kSweepWords, hipMemcpyDeviceToHost, s));
    E3D_HIP(hipStreamSynchronize(s));
    more = false;
    for (int f = 0; f < 6; ++f) more = more || mailbox.p[f] != 0u;
    while (more && done < max_sweeps) {
      for (int k = done + 1; k <= done + batch; ++k)
        hipLaunchKernelGGL(k_cube_sweep, grid, block, 0, s, buf[(k - 1) & 1], buf[k & 1], size, FL.p + (size_t)kSweepWords * (k - 1),
                           FL.p + (size_t)kSweepWords * k);
      E3D_HIP(hipGetLastError());
      E3D_HIP(hipMemcpyAsync(mailbox.p, FL.p + (size_t)kSweepWords * (done + 1), sizeof(unsigned) * kSweepWords * batch, hipMemcpyDeviceToHost, s));
      E3D_HIP(hipStreamSynchronize(s));
      ++n_batches; n_launched += batch;
      more = false;
      for (int f = 0; f < 6; ++f) {
        for (int k = 0; k < batch; ++k) sweeps[f] += mailbox.p[(size_t)kSweepWords * k + f] != 0u;
        more = more || mailbox.p[(size_t)kSweepWords * (batch - 1) + f] != 0u;
      }
      done += batch;
    }
    // sweep k validates the pixels at Chebyshev distance k from a valid one, and no distance reaches `size`
    if (more) throw Error(E3D_ERR_INVALID, "e3d_render_cube_map: the dilation did not settle");
    t_sweeps.stop(s);
    depth_final = FD.p;
    // a face that swept ends with both buffers equal (its last sweep validated nothing and copied); one that never swept
    // lives in P1 only
    color_final = buf[0];
    hipLaunchKernelGGL(k_cube_unpack, dim3((unsigned)div_up(div_up(n_px, 4), 256)), dim3(256), 0, s, color_final, n_px, OUT.p);
    E3D_HIP(hipGetLastError());
    copy_out(color_out, OUT.p, 3 * n_px, s);
    copy_out(depth_out, depth_final, sizeof(float) * n_px, s);
    E3D_HIP(hipStreamSynchronize(s));
    g_cube_timings[2] = t_fill.ms(); g_cube_timings[3] = t_sweeps.ms();
  } else {
    hipLaunchKernelGGL(k_cube_unpack, dim3((unsigned)div_up(div_up(n_px, 4), 256)), dim3(256), 0, s, color_final, n_px, OUT.p);
    E3D_HIP(hipGetLastError());
    copy_out(color_out, OUT.p, 3 * n_px, s);
    copy_out(depth_out, depth_final, sizeof(float) * n_px, s);
    E3D_HIP(hipStreamSynchronize(s));
    g_cube_timings[2] = 0.f; g_cube_timings[3] = 0.f;
  }
  g_cube_timings[0] = t_points.ms(); g_cube_timings[1] = t_resolve.ms();
  g_cube_timings[4] = (float)n_batches; g_cube_timings[5] = (float)n_launched;
  if (sweeps_out) for (int f = 0; f < 6; ++f) sweeps_out[f] = sweeps[f];
  return 0;
  E3D_CATCH()
}

extern "C" int e3d_cube_map_timings(float* out) {
  if (!out) { e3d::set_last_error("e3d_cube_map_timings: null argument"); return E3D_ERR_INVALID; }
  for (int i = 0; i < E3D_CUBE_MAP_TIMINGS; ++i) out[i] = g_cube_timings[i];
  return 0;
}
