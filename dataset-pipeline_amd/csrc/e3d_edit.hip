// e3d_edit.hip -- the selections and edits of the reference's PointCloudEditor (src/point_cloud_editor) as batch operations on
// one object's points, which stay on the MI355X for the whole session (include/e3d_hip.h, e3d_edit_*):
//   k_edit_lasso         LassoSelectionTool::applySelection        tool_select_lasso.cc:104-230
//   k_edit_beyond_plane  BeyondPlaneSelectionTool::PerformSelection tool_select_beyond_plane.cc:43-102
//   k_edit_pick          ...::mousePressEvent (closest point)       tool_select_beyond_plane.cc:108-155
//   compaction           Key_Delete / Key_M                         render_widget.cc:570-732
// The selection is one byte (0 / 1) per point.  The three selection kernels stream the points once: every thread takes four
// consecutive points (three 16-byte loads, one 4-byte flag word), blocks stride over the cloud, and a launch ends with one atomic
// per wave (the count of selected points; for the pick one 64-bit minimum per click).  All f32 / f64 expressions are written in the
// reference's order and the file is built without contraction, so the flags are the reference's.
#include "../../include/e3d_hip.h"
#include "e3d_common.hpp"

#include <cfloat>
#include <cmath>
#include <memory>

namespace e3d {

constexpr int kEditBlock = 256;
constexpr int kEditMaxBlocks = 2048;           // 8 blocks of 256 threads for each of the 256 CUs
constexpr int kSegment = 512;                  // points one wave compacts: 8 steps of 64

struct EditView {
  float r[12];
  float fx, fy, cx, cy, min_depth, max_depth, width_f, height_f;
  int width, height;
};
struct EditPlane { float nx, ny, nz, offset; };
struct EditClicks { double x[E3D_EDIT_MAX_CLICKS], y[E3D_EDIT_MAX_CLICKS]; int n; };
struct EditEdge { double x1, y1, y2, slope; };  // y1 < y2

// camera_point = Rs * p + t as Eigen evaluates it, the depth test (both ends inclusive, NaN fails), the pixel of
// NormalizedToImage + 0.5f
__device__ __forceinline__ bool edit_project(const EditView& v, float x, float y, float z, float& px, float& py, float& cz) {
  const float cx = ((v.r[0] * x + v.r[1] * y) + v.r[2] * z) + v.r[3];
  const float cy = ((v.r[4] * x + v.r[5] * y) + v.r[6] * z) + v.r[7];
  cz = ((v.r[8] * x + v.r[9] * y) + v.r[10] * z) + v.r[11];
  if (!(cz >= v.min_depth && cz <= v.max_depth)) return false;
  px = (v.fx * (cx / cz) + v.cx) + 0.5f;
  py = (v.fy * (cy / cz) + v.cy) + 0.5f;
  return true;
}

__device__ __forceinline__ void edit_load_quad(const float4* __restrict__ X4, size_t q, float p[12]) {
  const float4 a = ld_stream(X4 + 3 * q), b = ld_stream(X4 + 3 * q + 1), c = ld_stream(X4 + 3 * q + 2);
  p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
  p[8] = c.x; p[9] = c.y; p[10] = c.z; p[11] = c.w;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void add_wave_count(unsigned local, unsigned long long* __restrict__ counter) {
  const unsigned s = wave_sum(local);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(counter, (unsigned long long)s);
}

// MODE 0 replace, 1 add, 2 remove.  The polygon's non-horizontal edges, ordered so that y1 < y2 and with their f64 slopes, sit in
// LDS; every lane reads the same edge at the same time (a broadcast).  [ymin, ymax) is the union of the edges' y ranges: a pixel
// outside it meets the condition of no edge, so skipping the loop for it changes nothing.  (There is no such early-out in x: the
// rounded x1 + slope * (y - y1) may lie slightly outside [x1, x2].)
template <int MODE, bool DEPTH>
__global__ __launch_bounds__(kEditBlock) void k_edit_lasso(const float4* __restrict__ X4, unsigned* __restrict__ F4, size_t n, size_t n_quads,
                                                           EditView v, const EditEdge* __restrict__ edges, int n_edges, double ymin, double ymax,
                                                           const float* __restrict__ depth, unsigned long long* __restrict__ counter) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  EditEdge* s_edges = reinterpret_cast<EditEdge*>(s_raw);
  for (int e = threadIdx.x; e < n_edges; e += kEditBlock) s_edges[e] = edges[e];
  __syncthreads();
  unsigned local = 0;
  for (size_t q = (size_t)blockIdx.x * kEditBlock + threadIdx.x; q < n_quads; q += (size_t)gridDim.x * kEditBlock) {
    float p[12];
    edit_load_quad(X4, q, p);
    const unsigned old = MODE == 0 ? 0u : F4[q];
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = 4 * q + k < n;
      float px, py, cz;
      bool inside = false;
      if (valid && edit_project(v, p[3 * k], p[3 * k + 1], p[3 * k + 2], px, py, cz)) {
        const double x = (double)px, y = (double)py;
        if (y >= ymin && y < ymax) {
          unsigned parity = 0;
          for (int e = 0; e < n_edges; ++e) {
            const EditEdge E = s_edges[e];
            parity ^= (unsigned)(y >= E.y1 && y < E.y2 && E.x1 + E.slope * (y - E.y1) <= x);
          }
          inside = parity != 0;
          if (DEPTH && inside) {
            // tool_select_lasso.cc:177-190: the pixel truncated, then clamped to the image (float -> int saturates here)
            const int ix = min(max((int)px, 0), v.width - 1), iy = min(max((int)py, 0), v.height - 1);
            const float d = depth[(size_t)iy * v.width + ix];
            if (isfinite(d) && d < 0.99f * cz) inside = false;
          }
        }
      }
      const unsigned was = ((old >> (8 * k)) & 0xffu) ? 1u : 0u;
      unsigned f = MODE == 0 ? (unsigned)inside : (MODE == 1 ? (was | (unsigned)inside) : (was & (unsigned)!inside));
      if (!valid) f = 0;
      out |= f << (8 * k);
      local += f;
    }
    F4[q] = out;
  }
  add_wave_count(local, counter);
}

__global__ __launch_bounds__(kEditBlock) void k_edit_beyond_plane(const float4* __restrict__ X4, unsigned* __restrict__ F4, size_t n, size_t n_quads,
                                                                  EditView v, EditPlane pl, int limit_to_visible,
                                                                  unsigned long long* __restrict__ counter) {
  unsigned local = 0;
  for (size_t q = (size_t)blockIdx.x * kEditBlock + threadIdx.x; q < n_quads; q += (size_t)gridDim.x * kEditBlock) {
    float p[12];
    edit_load_quad(X4, q, p);
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x = p[3 * k], y = p[3 * k + 1], z = p[3 * k + 2];
      const float dist = ((pl.nx * x + pl.ny * y) + pl.nz * z) + pl.offset;     // Hyperplane::signedDistance
      bool sel = 4 * q + k < n && dist < 0.f;
      if (sel && limit_to_visible) {
        float px, py, cz;
        sel = edit_project(v, x, y, z, px, py, cz) && px >= 0.f && py >= 0.f && px < v.width_f && py < v.height_f;
      }
      out |= (unsigned)sel << (8 * k);
      local += (unsigned)sel;
    }
    F4[q] = out;
  }
  add_wave_count(local, counter);
}

// The closest point to each click: the key is (bits of the f32 squared pixel distance) << 32 | index.  The distance is >= 0 where
// it can win, so its bits order as the values do, and the smaller index wins a tie.  A distance that is not < +inf (inf, NaN) makes
// no key: the reference's strict `<` from +inf never takes it.
__global__ __launch_bounds__(kEditBlock) void k_edit_pick(const float4* __restrict__ X4, size_t n, size_t n_quads, EditView v, EditClicks clicks,
                                                          unsigned long long* __restrict__ keys) {
  unsigned long long best[E3D_EDIT_MAX_CLICKS];
#pragma unroll
  for (int c = 0; c < E3D_EDIT_MAX_CLICKS; ++c) best[c] = ~0ull;
  for (size_t q = (size_t)blockIdx.x * kEditBlock + threadIdx.x; q < n_quads; q += (size_t)gridDim.x * kEditBlock) {
    float p[12];
    edit_load_quad(X4, q, p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float px, py, cz;
      if (!(4 * q + k < n) || !edit_project(v, p[3 * k], p[3 * k + 1], p[3 * k + 2], px, py, cz)) continue;
      const double x = (double)px, y = (double)py;
#pragma unroll
      for (int c = 0; c < E3D_EDIT_MAX_CLICKS; ++c) {
        if (c >= clicks.n) continue;
        const double dx = x - clicks.x[c], dy = y - clicks.y[c];
        const float d = (float)(dx * dx + dy * dy);
        if (d < INFINITY) {
          const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(4 * q + k);
          best[c] = key < best[c] ? key : best[c];
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < E3D_EDIT_MAX_CLICKS; ++c) {
    if (c >= clicks.n) continue;
    unsigned long long b = best[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(b, o, 64);
      b = other < b ? other : b;
    }
    if ((threadIdx.x & 63) == 0 && b != ~0ull) atomicMin(keys + c, b);
  }
}

// flags as a caller gave them -> 0 / 1, and their count
__global__ __launch_bounds__(kEditBlock) void k_edit_normalise(unsigned* __restrict__ F4, size_t n, size_t n_quads, unsigned long long* __restrict__ counter) {
  unsigned local = 0;
  for (size_t q = (size_t)blockIdx.x * kEditBlock + threadIdx.x; q < n_quads; q += (size_t)gridDim.x * kEditBlock) {
    const unsigned old = F4[q];
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned f = (4 * q + k < n && ((old >> (8 * k)) & 0xffu)) ? 1u : 0u;
      out |= f << (8 * k);
      local += f;
    }
    F4[q] = out;
  }
  add_wave_count(local, counter);
}

// ---- stable compaction: one wave per segment of kSegment consecutive points -----------------------------------------------------------
// 1. selected points per segment (flags are 0 / 1: a word's byte sum is its count)
__global__ __launch_bounds__(kEditBlock) void k_edit_segment_counts(const unsigned* __restrict__ F4, size_t n_quads, size_t n_segments,
                                                                    unsigned* __restrict__ seg_selected) {
  const size_t seg = (size_t)blockIdx.x * (kEditBlock / 64) + (threadIdx.x >> 6);
  if (seg >= n_segments) return;                                   // whole waves leave
  const int lane = threadIdx.x & 63;
  unsigned local = 0;
#pragma unroll
  for (int step = 0; step < kSegment / 256; ++step) {
    const size_t w = seg * (kSegment / 4) + (size_t)step * 64 + lane;
    const unsigned f = w < n_quads ? F4[w] : 0u;
    local += (f * 0x01010101u) >> 24;
  }
  const unsigned s = wave_sum(local);
  if (lane == 0) seg_selected[seg] = s;
}

// 2. exclusive prefix of the kept points per segment (kept = selected, or with `invert` the others), by one block: every thread
//    sums a contiguous run of segments, the 1024 run sums are scanned in LDS, every thread writes its run's prefixes
__global__ __launch_bounds__(1024) void k_edit_segment_scan(const unsigned* __restrict__ seg_selected, size_t n_segments, size_t n, int invert,
                                                            unsigned* __restrict__ seg_offset, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_sum[1024];
  const size_t per = (n_segments + 1023) / 1024;
  const size_t b0 = per * threadIdx.x, b = b0 < n_segments ? b0 : n_segments, e = b + per < n_segments ? b + per : n_segments;
  auto kept = [&](size_t seg) -> unsigned {
    const unsigned sel = seg_selected[seg];
    if (!invert) return sel;
    const size_t left = n - seg * kSegment;
    return (unsigned)(left < (size_t)kSegment ? left : (size_t)kSegment) - sel;
  };
  unsigned long long mine = 0;
  for (size_t s = b; s < e; ++s) mine += kept(s);
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long add = (int)threadIdx.x >= o ? s_sum[threadIdx.x - o] : 0ull;
    __syncthreads();
    s_sum[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned long long run = s_sum[threadIdx.x] - mine;              // exclusive
  for (size_t s = b; s < e; ++s) { seg_offset[s] = (unsigned)run; run += kept(s); }
  if (threadIdx.x == 1023) *total = s_sum[1023];
}

// 3. every wave copies the kept points of its segment, in order, to their places
__global__ __launch_bounds__(kEditBlock) void k_edit_compact(const float* __restrict__ X, const unsigned char* __restrict__ F, size_t n, size_t n_segments,
                                                             int invert, const unsigned* __restrict__ seg_offset, float* __restrict__ Y, size_t capacity) {
  const size_t seg = (size_t)blockIdx.x * (kEditBlock / 64) + (threadIdx.x >> 6);
  if (seg >= n_segments) return;
  const int lane = threadIdx.x & 63;
  size_t base = seg_offset[seg];
  for (int step = 0; step < kSegment / 64; ++step) {
    const size_t i = seg * kSegment + (size_t)step * 64 + lane;
    const bool valid = i < n;
    const bool keep = valid && ((F[valid ? i : 0] != 0) != (invert != 0));
    const unsigned long long m = __ballot(keep);
    const size_t o = base + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && o < capacity) {                                    // (the host checks the total against its own count afterwards)
      Y[3 * o] = X[3 * i]; Y[3 * o + 1] = X[3 * i + 1]; Y[3 * o + 2] = X[3 * i + 2];
    }
    base += __popcll(m);
  }
}

static inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

}  // namespace e3d

using namespace e3d;

struct e3d_edit {
  int device = 0;
  hipStream_t stream = nullptr;
  size_t n = 0;                       // points
  int64_t selected = 0;               // of them selected
  // X: xyz of round4(n) points (the tail is never used), F: round4(n) flags (the tail is 0), Y: the other coordinate buffer
  DevBuf<float> X, Y, depth;
  DevBuf<unsigned char> F;
  DevBuf<unsigned> seg_selected, seg_offset;
  DevBuf<unsigned long long> words;   // [0] a count, [1..8] pick keys
  DevBuf<EditEdge> edges;
  PinBuf<unsigned long long> host_words;
  PinBuf<EditEdge> host_edges;
  std::unique_ptr<EventTimer> timer;
  float last_ms = 0.f;
  ~e3d_edit() {
    if (stream) { (void)hipStreamSynchronize(stream); }
    timer.reset();
    if (stream) (void)hipStreamDestroy(stream);
  }
  size_t n_quads() const { return round4(n) / 4; }
  size_t n_segments() const { return div_up(n, (size_t)kSegment); }
  unsigned stream_blocks() const { return (unsigned)std::min<size_t>(std::max<size_t>(div_up(n_quads(), (size_t)kEditBlock), 1), kEditMaxBlocks); }
};

namespace {

void need(e3d_edit* h, const char* what) { if (!h) throw Error(E3D_ERR_INVALID, std::string(what) + ": null handle"); }

EditView make_view(const e3d_view* view, const char* what) {
  if (!view) throw Error(E3D_ERR_INVALID, std::string(what) + ": null view");
  if (view->width < 1 || view->height < 1) throw Error(E3D_ERR_INVALID, std::string(what) + ": the view has no pixels");
  EditView v;
  for (int i = 0; i < 12; ++i) v.r[i] = view->camera_T_object[i];
  v.fx = view->fx; v.fy = view->fy; v.cx = view->cx; v.cy = view->cy;
  v.min_depth = view->min_depth; v.max_depth = view->max_depth;
  v.width = view->width; v.height = view->height;
  v.width_f = (float)view->width; v.height_f = (float)view->height;
  return v;
}

// the count word of a selection kernel, after the kernel: the one synchronisation of a selection call
int64_t read_count(e3d_edit* h) {
  h->host_words.reserve(1 + E3D_EDIT_MAX_CLICKS);
  E3D_HIP(hipMemcpyAsync(h->host_words.p, h->words.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  E3D_HIP(hipStreamSynchronize(h->stream));
  h->last_ms = h->timer->ms();
  return (int64_t)h->host_words.p[0];
}

// count, scan and copy of the points whose flag is set (invert: is not set) into `out`; their number goes to words[0]
void compact(e3d_edit* h, int invert, float* out, size_t capacity) {
  const size_t S = h->n_segments();
  if (S == 0) return;
  hipStream_t s = h->stream;
  h->seg_selected.reserve(S); h->seg_offset.reserve(S);
  const unsigned blocks = (unsigned)div_up(S, (size_t)(kEditBlock / 64));
  hipLaunchKernelGGL(k_edit_segment_counts, dim3(blocks), dim3(kEditBlock), 0, s, reinterpret_cast<const unsigned*>(h->F.p), h->n_quads(), S,
                     h->seg_selected.p);
  hipLaunchKernelGGL(k_edit_segment_scan, dim3(1), dim3(1024), 0, s, h->seg_selected.p, S, h->n, invert, h->seg_offset.p, h->words.p);
  hipLaunchKernelGGL(k_edit_compact, dim3(blocks), dim3(kEditBlock), 0, s, h->X.p, h->F.p, h->n, S, invert, h->seg_offset.p, out, capacity);
  E3D_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

e3d_edit_t* e3d_edit_create(const float* xyz, size_t n) {
  e3d_edit* h = nullptr;
  E3D_TRY
  if (!xyz && n) throw Error(E3D_ERR_INVALID, "e3d_edit_create: null points");
  if (n >= ((size_t)1 << 32)) throw Error(E3D_ERR_INVALID, "e3d_edit_create: 2^32 points or more");
  require_device();
  h = new e3d_edit();
  E3D_HIP(hipGetDevice(&h->device));
  E3D_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->timer.reset(new EventTimer());
  h->n = n;
  h->X.reserve(3 * round4(n) + 4); h->F.reserve(round4(n) + 4); h->words.reserve(1 + E3D_EDIT_MAX_CLICKS);
  E3D_HIP(hipMemsetAsync(h->X.p, 0, sizeof(float) * (3 * round4(n) + 4), h->stream));
  E3D_HIP(hipMemsetAsync(h->F.p, 0, round4(n) + 4, h->stream));
  copy_in(h->X.p, xyz, sizeof(float) * 3 * n, h->stream);
  E3D_HIP(hipStreamSynchronize(h->stream));
  return h;
  E3D_CATCH_NEW(h)
}

void e3d_edit_destroy(e3d_edit_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  delete h;
}

int64_t e3d_edit_size(e3d_edit_t* h) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_size");
  return (int64_t)h->n;
  E3D_CATCH()
}

int e3d_edit_get_points(e3d_edit_t* h, float* xyz) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_get_points");
  if (!xyz && h->n) throw Error(E3D_ERR_INVALID, "e3d_edit_get_points: null argument");
  copy_out(xyz, h->X.p, sizeof(float) * 3 * h->n, h->stream);
  E3D_HIP(hipStreamSynchronize(h->stream));
  return 0;
  E3D_CATCH()
}

int e3d_edit_get_selection(e3d_edit_t* h, uint8_t* flags) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_get_selection");
  if (!flags && h->n) throw Error(E3D_ERR_INVALID, "e3d_edit_get_selection: null argument");
  copy_out(flags, h->F.p, h->n, h->stream);
  E3D_HIP(hipStreamSynchronize(h->stream));
  return 0;
  E3D_CATCH()
}

int64_t e3d_edit_set_selection(e3d_edit_t* h, const uint8_t* flags) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_set_selection");
  if (!flags && h->n) throw Error(E3D_ERR_INVALID, "e3d_edit_set_selection: null argument");
  hipStream_t s = h->stream;
  copy_in(h->F.p, flags, h->n, s);
  E3D_HIP(hipMemsetAsync(h->words.p, 0, sizeof(unsigned long long), s));
  h->timer->start(s);
  if (h->n) hipLaunchKernelGGL(k_edit_normalise, dim3(h->stream_blocks()), dim3(kEditBlock), 0, s, reinterpret_cast<unsigned*>(h->F.p), h->n, h->n_quads(), h->words.p);
  h->timer->stop(s);
  E3D_HIP(hipGetLastError());
  h->selected = read_count(h);
  return h->selected;
  E3D_CATCH()
}

int64_t e3d_edit_selection_count(e3d_edit_t* h) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_selection_count");
  return h->selected;
  E3D_CATCH()
}

int64_t e3d_edit_lasso(e3d_edit_t* h, const e3d_view* view, const double* polygon_xy, int n_vertices, int mode, const float* depth) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_lasso");
  const EditView v = make_view(view, "e3d_edit_lasso");
  if (mode < E3D_EDIT_REPLACE || mode > E3D_EDIT_REMOVE) throw Error(E3D_ERR_INVALID, fmt("e3d_edit_lasso: mode %d", mode));
  if (n_vertices < 0 || (n_vertices && !polygon_xy)) throw Error(E3D_ERR_INVALID, "e3d_edit_lasso: null polygon");
  if (n_vertices > E3D_EDIT_MAX_POLYGON) throw Error(E3D_ERR_INVALID, fmt("e3d_edit_lasso: %d polygon vertices, at most %d", n_vertices, E3D_EDIT_MAX_POLYGON));
  if (n_vertices < 3) return h->selected;                          // tool_select_lasso.cc:105: nothing happens
  hipStream_t s = h->stream;
  // the closed polygon's edges: horizontal ones never count, the others are ordered upwards and carry their slope
  h->host_edges.reserve(E3D_EDIT_MAX_POLYGON);
  int n_edges = 0;
  double ymin = INFINITY, ymax = -INFINITY;
  for (int i = 0; i < n_vertices; ++i) {
    const int j = i + 1 == n_vertices ? 0 : i + 1;
    double x1 = polygon_xy[2 * i], y1 = polygon_xy[2 * i + 1], x2 = polygon_xy[2 * j], y2 = polygon_xy[2 * j + 1];
    if (y1 == y2) continue;
    if (y2 < y1) { std::swap(x1, x2); std::swap(y1, y2); }
    h->host_edges.p[n_edges++] = EditEdge{x1, y1, y2, (x2 - x1) / (y2 - y1)};
    if (y1 < ymin) ymin = y1;
    if (y2 > ymax) ymax = y2;
  }
  h->edges.reserve(E3D_EDIT_MAX_POLYGON);
  if (n_edges) E3D_HIP(hipMemcpyAsync(h->edges.p, h->host_edges.p, sizeof(EditEdge) * n_edges, hipMemcpyHostToDevice, s));
  if (depth) {
    const size_t px = (size_t)v.width * v.height;
    h->depth.reserve(px);
    copy_in(h->depth.p, depth, sizeof(float) * px, s);
  }
  E3D_HIP(hipMemsetAsync(h->words.p, 0, sizeof(unsigned long long), s));
  h->timer->start(s);
  if (h->n) {
    const dim3 grid(h->stream_blocks()), block(kEditBlock);
    const size_t lds = sizeof(EditEdge) * (size_t)std::max(n_edges, 1);
    const float4* X4 = reinterpret_cast<const float4*>(h->X.p);
    unsigned* F4 = reinterpret_cast<unsigned*>(h->F.p);
#define E3D_LASSO(MODE, DEPTH) \
    hipLaunchKernelGGL((k_edit_lasso<MODE, DEPTH>), grid, block, lds, s, X4, F4, h->n, h->n_quads(), v, h->edges.p, n_edges, ymin, ymax, \
                       (const float*)(DEPTH ? h->depth.p : nullptr), h->words.p)
    if (depth) { if (mode == 0) E3D_LASSO(0, true); else if (mode == 1) E3D_LASSO(1, true); else E3D_LASSO(2, true); }
    else       { if (mode == 0) E3D_LASSO(0, false); else if (mode == 1) E3D_LASSO(1, false); else E3D_LASSO(2, false); }
#undef E3D_LASSO
  }
  h->timer->stop(s);
  E3D_HIP(hipGetLastError());
  h->selected = read_count(h);                                     // (the pinned edge list is free again: its copy has run)
  return h->selected;
  E3D_CATCH()
}

int64_t e3d_edit_beyond_plane(e3d_edit_t* h, const e3d_view* view, const float points[9], const float camera_position_object[3],
                              int limit_to_visible) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_beyond_plane");
  const EditView v = make_view(view, "e3d_edit_beyond_plane");
  if (!points || !camera_position_object) throw Error(E3D_ERR_INVALID, "e3d_edit_beyond_plane: null argument");
  // Eigen::Hyperplane<float, 3>::Through(p0, p1, p2) without its SVD branch
  const float* p0 = points; const float* p1 = points + 3; const float* p2 = points + 6;
  const float v0[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]}, v1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  float nrm[3] = {v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]};
  auto norm3 = [](const float* a) { return sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); };
  const float norm = norm3(nrm);
  if (!(norm > norm3(v0) * norm3(v1) * FLT_EPSILON))
    throw Error(E3D_ERR_INVALID, "e3d_edit_beyond_plane: the three points lie on one line (or are not finite)");
  for (int i = 0; i < 3; ++i) nrm[i] = nrm[i] / norm;
  EditPlane pl;
  pl.nx = nrm[0]; pl.ny = nrm[1]; pl.nz = nrm[2];
  pl.offset = -((p0[0] * nrm[0] + p0[1] * nrm[1]) + p0[2] * nrm[2]);
  const float* c = camera_position_object;
  if (((pl.nx * c[0] + pl.ny * c[1]) + pl.nz * c[2]) + pl.offset < 0.f) { pl.nx = -pl.nx; pl.ny = -pl.ny; pl.nz = -pl.nz; pl.offset = -pl.offset; }
  hipStream_t s = h->stream;
  E3D_HIP(hipMemsetAsync(h->words.p, 0, sizeof(unsigned long long), s));
  h->timer->start(s);
  if (h->n)
    hipLaunchKernelGGL(k_edit_beyond_plane, dim3(h->stream_blocks()), dim3(kEditBlock), 0, s, reinterpret_cast<const float4*>(h->X.p),
                       reinterpret_cast<unsigned*>(h->F.p), h->n, h->n_quads(), v, pl, limit_to_visible ? 1 : 0, h->words.p);
  h->timer->stop(s);
  E3D_HIP(hipGetLastError());
  h->selected = read_count(h);
  return h->selected;
  E3D_CATCH()
}

int e3d_edit_pick(e3d_edit_t* h, const e3d_view* view, const double* clicks_xy, int n_clicks, int64_t* index_out, float* distance_out) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_pick");
  const EditView v = make_view(view, "e3d_edit_pick");
  if (n_clicks < 0 || n_clicks > E3D_EDIT_MAX_CLICKS) throw Error(E3D_ERR_INVALID, fmt("e3d_edit_pick: %d clicks, at most %d", n_clicks, E3D_EDIT_MAX_CLICKS));
  if (n_clicks == 0) return 0;
  if (!clicks_xy || !index_out) throw Error(E3D_ERR_INVALID, "e3d_edit_pick: null argument");
  EditClicks clicks;
  clicks.n = n_clicks;
  for (int c = 0; c < E3D_EDIT_MAX_CLICKS; ++c) { clicks.x[c] = c < n_clicks ? clicks_xy[2 * c] : 0.0; clicks.y[c] = c < n_clicks ? clicks_xy[2 * c + 1] : 0.0; }
  hipStream_t s = h->stream;
  E3D_HIP(hipMemsetAsync(h->words.p + 1, 0xFF, sizeof(unsigned long long) * E3D_EDIT_MAX_CLICKS, s));
  h->timer->start(s);
  if (h->n)
    hipLaunchKernelGGL(k_edit_pick, dim3(h->stream_blocks()), dim3(kEditBlock), 0, s, reinterpret_cast<const float4*>(h->X.p), h->n, h->n_quads(), v,
                       clicks, h->words.p + 1);
  h->timer->stop(s);
  E3D_HIP(hipGetLastError());
  h->host_words.reserve(1 + E3D_EDIT_MAX_CLICKS);
  E3D_HIP(hipMemcpyAsync(h->host_words.p + 1, h->words.p + 1, sizeof(unsigned long long) * E3D_EDIT_MAX_CLICKS, hipMemcpyDeviceToHost, s));
  E3D_HIP(hipStreamSynchronize(s));
  h->last_ms = h->timer->ms();
  for (int c = 0; c < n_clicks; ++c) {
    const unsigned long long key = h->host_words.p[1 + c];
    const uint32_t bits = key == ~0ull ? 0x7f800000u : (uint32_t)(key >> 32);
    index_out[c] = key == ~0ull ? -1 : (int64_t)(key & 0xffffffffull);
    if (distance_out) memcpy(distance_out + c, &bits, sizeof bits);
  }
  return 0;
  E3D_CATCH()
}

int64_t e3d_edit_extract_selected(e3d_edit_t* h, float* xyz_out, size_t capacity) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_extract_selected");
  const size_t m = (size_t)h->selected;
  if (m > capacity) throw Error(E3D_ERR_INVALID, fmt("e3d_edit_extract_selected: %zu points selected, room for %zu", m, capacity));
  if (m == 0) return 0;
  if (!xyz_out) throw Error(E3D_ERR_INVALID, "e3d_edit_extract_selected: null argument");
  hipStream_t s = h->stream;
  h->Y.reserve(3 * round4(m) + 4);
  h->timer->start(s);
  compact(h, 0, h->Y.p, m);
  h->timer->stop(s);
  if (read_count(h) != (int64_t)m) throw Error(E3D_ERR_INVALID, "e3d_edit_extract_selected: the selection count and the flags disagree");
  copy_out(xyz_out, h->Y.p, sizeof(float) * 3 * m, s);
  E3D_HIP(hipStreamSynchronize(s));
  return (int64_t)m;
  E3D_CATCH()
}

int64_t e3d_edit_delete_selected(e3d_edit_t* h) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_delete_selected");
  if (h->selected == 0) return (int64_t)h->n;
  hipStream_t s = h->stream;
  const size_t kept = h->n - (size_t)h->selected;
  h->Y.reserve(3 * round4(h->n) + 4);                                   // as large as X: the buffers change places
  h->timer->start(s);
  compact(h, 1, h->Y.p, h->n);
  h->timer->stop(s);
  if (read_count(h) != (int64_t)kept) throw Error(E3D_ERR_INVALID, "e3d_edit_delete_selected: the selection count and the flags disagree");
  std::swap(h->X, h->Y);
  h->n = kept;
  h->selected = 0;
  E3D_HIP(hipMemsetAsync(h->F.p, 0, h->F.cap, s));
  E3D_HIP(hipStreamSynchronize(s));
  return (int64_t)kept;
  E3D_CATCH()
}

int e3d_edit_kernel_ms(e3d_edit_t* h, float* ms) {
  E3D_TRY_ON(h)
  need(h, "e3d_edit_kernel_ms");
  if (!ms) throw Error(E3D_ERR_INVALID, "e3d_edit_kernel_ms: null argument");
  *ms = h->last_ms;
  return 0;
  E3D_CATCH()
}

}  // extern "C"
