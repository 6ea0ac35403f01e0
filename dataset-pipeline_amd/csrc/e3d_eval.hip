// e3d_eval.hip -- ReconstructionEvaluator: accuracy and completeness of a reconstruction against the scans on the MI355X (DESIGN.md 20;
// the rules: include/e3d_hip.h, e3d_evaluate_reconstruction).  Neither tree of the reference computes this; nothing is restated.
//
//  grid     per cloud (the reconstruction, all scans together) and search level a hashed grid of its non-ignored points (HashEntry /
//           cell_key / launch_build_table) whose cell is a little larger than the level's tolerance.  The level-0 order of a cloud is
//           also the order its points are searched in, so neighbouring queries walk the same cells
//  search   k_eval_search: the tolerances in ascending order over the queries still open.  A wave takes 64 open queries, one after the
//           other: 27 lanes look up the 27 cells around the query (its own first), the wave walks the non-empty ones 64 points at a
//           time and stops at the first cell with a point within the level's threshold.  Only the class is public, so any such point
//           will do.  The queries without one are compacted (stable) into the next level's list
//  range    one N x N x 6 buffer of f32 bit patterns, reused scan after scan: cleared, atomicMin of the scan's ranges, then one pass
//           over the reconstruction that raises free[r]
//  voxels   per kind: voxel keys, pair sort, one thread per voxel counts its points per tolerance, f64 ratios summed in a fixed tree
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/e3d_hip.h"
#include "e3d_grid.hpp"

#pragma clang fp contract(off)

namespace e3d {

constexpr int kEvalBlock = 256;
constexpr int kEvalMaxT = 8;
constexpr int kEvalVoxelBias = 1 << 20;            // |c| / h < 2^20: v + bias is the 21-bit field of the voxel key
constexpr unsigned kEvalClassifyBlocks = 2048;
constexpr int kEvalReduceChunk = 8 * kEvalBlock;   // voxels per block of k_eval_reduce (fixed: the sums' order depends on the count alone)
constexpr int kEvalGroups = 4;
static const char* const kEvalGroupNames[kEvalGroups] = {"grid", "search", "range", "voxels"};

struct EvalTolerances { float t[kEvalMaxT]; float thr[kEvalMaxT]; int T; };

// a level's grid over one cloud's non-ignored points
struct EvalGrid {
  const float4* P4;                                // the points in cell order (w = input index as bits)
  const HashEntry* table;
  unsigned mask;
  double org[3], cell;
};

__device__ __forceinline__ bool eval_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// The grid cell of a coordinate: ONE monotone function for the stored points and for the queries.  A stored point lands in
// [0, 2^20]; a query far outside is clamped to a cell whose neighbours hold nothing.
__device__ __forceinline__ int eval_grid_coord(float v, double org, double cell) {
  const double q = floor(((double)v - org) / cell);
  return (int)fmin(fmax(q, -2.0), 2097153.0);
}

// order-preserving map of a finite f32 to unsigned
__device__ __forceinline__ unsigned eval_ordered(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Per point: is it ignored; sets its classes to their start values (near = T, free = 0; 255 for an ignored point).  The bounding
// box of the others as ordered f32 in box[0..5] (min xyz, max xyz), box[6] = a point with |c| / h >= 2^20, box[7] = their number.
// A fixed grid strides over the points and every block ends in one set of atomics.
__global__ __launch_bounds__(kEvalBlock) void k_eval_classify(const float* __restrict__ xyz, size_t n, float h, unsigned char T,
                                                              unsigned char* __restrict__ near_cls, unsigned char* __restrict__ free_cls,
                                                              unsigned* __restrict__ box) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  unsigned bad = 0, count = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float c[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    const bool ok = eval_finite(c[0], c[1], c[2]);
    near_cls[i] = ok ? T : (unsigned char)255;
    if (free_cls) free_cls[i] = ok ? (unsigned char)0 : (unsigned char)255;
    if (!ok) continue;
    ++count;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (fabsf(c[a]) / h >= 1048576.f) bad = 1;
      lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]);
    }
  }
  __shared__ unsigned part[kEvalBlock / kWave][8];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { bad |= __shfl_xor(bad, o, 64); count += __shfl_xor(count, o, 64); }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { part[wv][a] = eval_ordered(lo[a]); part[wv][3 + a] = eval_ordered(hi[a]); }
    part[wv][6] = bad; part[wv][7] = count;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int t = threadIdx.x;
    unsigned v = part[0][t];
    for (int k = 1; k < kEvalBlock / kWave; ++k) v = t < 3 ? min(v, part[k][t]) : t < 6 ? max(v, part[k][t]) : t == 6 ? (v | part[k][t]) : v + part[k][t];
    if (t < 3) atomicMin(&box[t], v);
    else if (t < 6) atomicMax(&box[t], v);
    else if (t == 6) { if (v) atomicOr(&box[6], 1u); }
    else if (v) atomicAdd(&box[7], v);
  }
}

// sort keys of a level's grid (vals = point index); kEmptyKey for an ignored point, which the sort moves to the end
__global__ __launch_bounds__(kEvalBlock) void k_eval_grid_keys(const float* __restrict__ xyz, size_t n, EvalGrid G, unsigned long long* __restrict__ keys,
                                                               unsigned* __restrict__ vals) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  keys[i] = eval_finite(x, y, z) ? cell_key(eval_grid_coord(x, G.org[0], G.cell), eval_grid_coord(y, G.org[1], G.cell), eval_grid_coord(z, G.org[2], G.cell))
                                 : kEmptyKey;
  vals[i] = (unsigned)i;
}

// One level of the class search.  open: positions in Q4 of the queries still open (nullptr: all n_open of them); a wave takes 64,
// one per lane, and searches them one after the other.  A query with a point of G within thr gets the level as its class and
// leaves the list (still_open = 0).
__global__ __launch_bounds__(kEvalBlock) void k_eval_search(const float4* __restrict__ Q4, const unsigned* __restrict__ open, size_t n_open, EvalGrid G, float thr,
                                                            unsigned char level, unsigned char* __restrict__ cls, unsigned char* __restrict__ still_open) {
  const int lane = threadIdx.x & 63;
  const size_t base = ((size_t)blockIdx.x * (kEvalBlock / kWave) + (threadIdx.x >> 6)) * 64;
  if (base >= n_open) return;
  const size_t j = base + lane;
  const bool valid = j < n_open;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) q = Q4[open ? open[j] : (unsigned)j];
  const int c0 = eval_grid_coord(q.x, G.org[0], G.cell), c1 = eval_grid_coord(q.y, G.org[1], G.cell), c2 = eval_grid_coord(q.z, G.org[2], G.cell);
  // lane l < 27 looks up neighbour (l + 13) % 27 of every query: lane 0 the query's own cell
  const int o = lane + 13 >= 27 ? lane - 14 : lane + 13;
  const int ox = o % 3 - 1, oy = (o / 3) % 3 - 1, oz = o / 9 - 1;
  const int nq = (int)min((size_t)64, n_open - base);
  unsigned long long hit = 0;
  for (int t = 0; t < nq; ++t) {
    const float qx = __shfl(q.x, t, 64), qy = __shfl(q.y, t, 64), qz = __shfl(q.z, t, 64);
    const int cx = __shfl(c0, t, 64), cy = __shfl(c1, t, 64), cz = __shfl(c2, t, 64);
    unsigned s = 0, e = 0;
    if (lane < 27) hash_cell_range(G.table, G.mask, cx + ox, cy + oy, cz + oz, s, e);
    unsigned long long nonempty = __ballot(e > s);
    bool found = false;
    while (nonempty) {
      const int src = __ffsll((long long)nonempty) - 1;
      nonempty &= nonempty - 1;
      const unsigned cs = __shfl(s, src, 64), ce = __shfl(e, src, 64);
      for (unsigned m = cs + lane; m < ce && !found; m += 64) {
        const float4 p = G.P4[m];
        found = sqdist_l2(qx, qy, qz, p.x, p.y, p.z) <= thr;
      }
      if (__ballot(found)) { hit |= 1ull << t; break; }
    }
  }
  if (valid) {
    const bool h = (hit >> lane) & 1ull;
    if (h) cls[__float_as_uint(q.w)] = level;
    still_open[j] = h ? 0 : 1;
  }
}

// the open queries of the next level: a stable compaction of this level's list
__global__ __launch_bounds__(kEvalBlock) void k_eval_compact(const unsigned* __restrict__ open, const unsigned char* __restrict__ flags,
                                                             const unsigned* __restrict__ offsets, size_t n, unsigned* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n && flags[j]) out[offsets[j]] = open ? open[j] : (unsigned)j;
}

// rule 3: the pixel and the range of p seen from o; false if there is no pixel
__device__ __forceinline__ bool eval_pixel(float px, float py, float pz, float ox, float oy, float oz, int N, unsigned& pixel, float& range) {
  const float dx = px - ox, dy = py - oy, dz = pz - oz;
  if (!eval_finite(dx, dy, dz)) return false;
  const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
  const float m = fmaxf(ax, fmaxf(ay, az));
  if (m == 0.f) return false;
  const int axis = ax == m ? 0 : (ay == m ? 1 : 2);
  const float d = axis == 0 ? dx : (axis == 1 ? dy : dz);
  const float a = axis == 0 ? dy : (axis == 1 ? dz : dx);
  const float b = axis == 0 ? dz : (axis == 1 ? dx : dy);
  const int face = 2 * axis + (d < 0.f ? 1 : 0);
  const float half = (float)(N / 2);
  const int col = min(N - 1, (int)floorf((a / m + 1.0f) * half));
  const int row = min(N - 1, (int)floorf((b / m + 1.0f) * half));
  pixel = ((unsigned)face * (unsigned)N + (unsigned)row) * (unsigned)N + (unsigned)col;
  range = sqrtf(sqdist_l2(px, py, pz, ox, oy, oz));
  return true;
}

// rmin of one scan: the bit pattern of a range >= 0 orders as the range does; 0xFFFFFFFF = empty
__global__ __launch_bounds__(kEvalBlock) void k_eval_range_min(const float* __restrict__ xyz, size_t n, float ox, float oy, float oz, int N, unsigned* __restrict__ rmin) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned pixel; float range;
  if (eval_pixel(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ox, oy, oz, N, pixel, range)) atomicMin(&rmin[pixel], __float_as_uint(range));
}

// rule 4 for one scan: free[r] = max(free[r], free_s[r]) (an ignored r has no pixel and keeps 255)
__global__ __launch_bounds__(kEvalBlock) void k_eval_free(const float* __restrict__ xyz, size_t n, float ox, float oy, float oz, int N, const unsigned* __restrict__ rmin,
                                                          EvalTolerances tol, unsigned char* __restrict__ free_cls) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned pixel; float range;
  if (!eval_pixel(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ox, oy, oz, N, pixel, range)) return;
  const unsigned bits = rmin[pixel];
  if (bits == 0xFFFFFFFFu) return;
  const float nearest = __uint_as_float(bits);
  int count = 0;
#pragma unroll
  for (int k = 0; k < kEvalMaxT; ++k)
    if (k < tol.T && range + tol.t[k] < nearest) ++count;
  if (count > (int)free_cls[i]) free_cls[i] = (unsigned char)count;
}

// voxel keys of rule 6 (vals = point index); kEmptyKey for an ignored point
__global__ __launch_bounds__(kEvalBlock) void k_eval_voxel_keys(const float* __restrict__ xyz, size_t n, float h, unsigned long long* __restrict__ keys,
                                                                unsigned* __restrict__ vals) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  keys[i] = eval_finite(x, y, z) ? cell_key((int)floorf(x / h) + kEvalVoxelBias, (int)floorf(y / h) + kEvalVoxelBias, (int)floorf(z / h) + kEvalVoxelBias) : kEmptyKey;
  vals[i] = (unsigned)i;
}

// the position of the first point of every voxel: the flags of launch_flag_run_starts, compacted
__global__ __launch_bounds__(kEvalBlock) void k_eval_voxel_starts(const unsigned char* __restrict__ flags, const unsigned* __restrict__ offsets, size_t n,
                                                                  unsigned* __restrict__ starts) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n && flags[j]) starts[offsets[j]] = (unsigned)j;
}

// One voxel per thread: its key, its number of points and per tolerance count_a = # complete or accurate, count_b = # inaccurate
// (free_cls == nullptr, the scan voxels: zeros), and the voxel's ratio of rule 7 (0 and evaluated = 0 without a denominator).
__global__ __launch_bounds__(kEvalBlock) void k_eval_voxel_counts(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ order,
                                                                  const unsigned* __restrict__ starts, size_t n_voxels, size_t n_points,
                                                                  const unsigned char* __restrict__ near_cls, const unsigned char* __restrict__ free_cls, int T,
                                                                  int* __restrict__ ijk, int* __restrict__ npts, int* __restrict__ count_a, int* __restrict__ count_b,
                                                                  double* __restrict__ ratio, unsigned char* __restrict__ evaluated) {
  const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_voxels) return;
  const unsigned s = starts[v], e = v + 1 < n_voxels ? starts[v + 1] : (unsigned)n_points;
  int a[kEvalMaxT], b[kEvalMaxT];
#pragma unroll
  for (int k = 0; k < kEvalMaxT; ++k) { a[k] = 0; b[k] = 0; }
  for (unsigned m = s; m < e; ++m) {
    const unsigned i = order[m];
    const int nr = near_cls[i], fr = free_cls ? (int)free_cls[i] : 0;
#pragma unroll
    for (int k = 0; k < kEvalMaxT; ++k) {
      a[k] += nr <= k ? 1 : 0;
      b[k] += (nr > k && k < fr) ? 1 : 0;
    }
  }
  const unsigned long long key = keys[s];
  ijk[3 * v] = (int)(key & 0x1FFFFF) - kEvalVoxelBias;
  ijk[3 * v + 1] = (int)((key >> 21) & 0x1FFFFF) - kEvalVoxelBias;
  ijk[3 * v + 2] = (int)((key >> 42) & 0x1FFFFF) - kEvalVoxelBias;
  npts[v] = (int)(e - s);
#pragma unroll
  for (int k = 0; k < kEvalMaxT; ++k) {
    if (k >= T) break;
    const int den = free_cls ? a[k] + b[k] : (int)(e - s);
    count_a[(size_t)T * v + k] = a[k];
    count_b[(size_t)T * v + k] = b[k];
    ratio[(size_t)T * v + k] = den > 0 ? (double)a[k] / (double)den : 0.0;
    evaluated[(size_t)T * v + k] = den > 0 ? 1 : 0;
  }
}

// Sums of n rows of T values in a fixed order: block b takes rows [b chunk, (b + 1) chunk), thread t of it rows t, t + 256, ... in
// turn, then a binary tree over the threads.  out_sum / out_count [T b + k].  With rows = the blocks' results and one block this is
// the last step as well (count_in then holds the counts to add, else the 0 / 1 flags).
template <typename CountT>
__global__ __launch_bounds__(kEvalBlock) void k_eval_reduce(const double* __restrict__ ratio, const CountT* __restrict__ count_in, size_t n, int T,
                                                            size_t chunk, double* __restrict__ out_sum, unsigned long long* __restrict__ out_count) {
  __shared__ double ssum[kEvalBlock];
  __shared__ unsigned long long scount[kEvalBlock];
  const size_t begin = (size_t)blockIdx.x * chunk, end = min(n, begin + chunk);
  for (int k = 0; k < T; ++k) {
    double sum = 0.0;
    unsigned long long count = 0;
    for (size_t r = begin + threadIdx.x; r < end; r += kEvalBlock) { sum += ratio[(size_t)T * r + k]; count += (unsigned long long)count_in[(size_t)T * r + k]; }
    ssum[threadIdx.x] = sum; scount[threadIdx.x] = count;
    __syncthreads();
    for (int w = kEvalBlock / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) { ssum[threadIdx.x] += ssum[threadIdx.x + w]; scount[threadIdx.x] += scount[threadIdx.x + w]; }
      __syncthreads();
    }
    if (threadIdx.x == 0) { out_sum[(size_t)T * blockIdx.x + k] = ssum[0]; out_count[(size_t)T * blockIdx.x + k] = scount[0]; }
    __syncthreads();
  }
}

}  // namespace e3d

using namespace e3d;

struct e3d_eval {
  int T = 0;
  std::vector<uint8_t> near_rec, free_rec, near_scan;
  struct Voxels { std::vector<int32_t> ijk, npts, count_a, count_b; } vox[2];      // 0: scan, 1: reconstruction
  int64_t evaluated[kEvalMaxT] = {0};
  double scores[3 * kEvalMaxT] = {0};
  float ms[kEvalGroups] = {0, 0, 0, 0};
};

namespace {

float ordered_to_float(unsigned u) {
  const unsigned b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  float f; memcpy(&f, &b, sizeof f); return f;
}

// one cloud on the device: the reconstruction or all scans together
struct EvalCloud {
  size_t n = 0, m = 0;                             // points, of them not ignored
  DevBuf<float> xyz;
  DevBuf<unsigned char> near_cls, free_cls;
  double lo[3] = {0, 0, 0}, span = 0;              // bounding box of the m points: its minimum and largest extent
  DevBuf<float4> Q4;                               // level-0 grid order = search order
  DevBuf<HashEntry> table0;
  EvalGrid grid0{};
  // the level being searched (levels >= 1)
  DevBuf<float4> P4;
  DevBuf<HashEntry> table;
  // open queries
  DevBuf<unsigned> open_a, open_b;
  const unsigned* open = nullptr;                  // nullptr: all m
  size_t n_open = 0;
};

struct EvalRun : Compactor {
  DevBuf<unsigned> vals_a, vals_b, counter;
  DevBuf<unsigned long long> keys_a, keys_b;
  GroupTimer timer[kEvalGroups];
  using Compactor::Compactor;

  static dim3 blocks(size_t n) { return dim3((unsigned)div_up(n, kEvalBlock)); }

  void upload(EvalCloud& c, const float* xyz, size_t n, float h, int T, bool with_free, const char* what) {
    c.n = n;
    if (n == 0) return;
    c.xyz.reserve(3 * n); c.near_cls.reserve(n);
    if (with_free) c.free_cls.reserve(n);
    copy_in(c.xyz.p, xyz, sizeof(float) * 3 * n, s);
    counter.reserve(8);
    const unsigned box0[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0, 0};
    unsigned hb[8];
    E3D_HIP(hipMemcpyAsync(counter.p, box0, sizeof box0, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_eval_classify, dim3((unsigned)std::min<size_t>(div_up(n, kEvalBlock), kEvalClassifyBlocks)), dim3(kEvalBlock), 0, s, c.xyz.p, n, h,
                       (unsigned char)T, c.near_cls.p, with_free ? c.free_cls.p : nullptr, counter.p);
    copy_out(hb, counter.p, sizeof hb, s);
    E3D_HIP(hipStreamSynchronize(s));
    E3D_HIP(hipGetLastError());
    if (hb[6]) throw Error(E3D_ERR_INVALID, fmt("e3d_evaluate_reconstruction: a %s point lies at |coordinate| / voxel size >= 2^20", what));
    c.m = hb[7];
    if (c.m == 0) return;
    for (int a = 0; a < 3; ++a) {
      c.lo[a] = (double)ordered_to_float(hb[a]);
      c.span = std::max(c.span, (double)ordered_to_float(hb[3 + a]) - c.lo[a]);
    }
  }

  // The grid of cloud c for tolerance t.  The cell exceeds t by 1e-3 of it: d2(a, b) <= thr bounds every |a.x - b.x| by t (1 + 2^-22)
  // (+ 1e-20 where the squares underflow), so the cell coordinates of a and b, one monotone function, differ by one at most.  It
  // also keeps the cloud within 2^20 cells.
  EvalGrid build_grid(EvalCloud& c, double t, DevBuf<float4>& P4, DevBuf<HashEntry>& table) {
    EvalGrid G{};
    G.cell = std::max(t * 1.001 + 1e-20, c.span * 1.001 / 1048576.0);
    for (int a = 0; a < 3; ++a) G.org[a] = c.lo[a];
    keys_a.reserve(c.n); keys_b.reserve(c.n); vals_a.reserve(c.n); vals_b.reserve(c.n);
    hipLaunchKernelGGL(k_eval_grid_keys, blocks(c.n), dim3(kEvalBlock), 0, s, c.xyz.p, c.n, G, keys_a.p, vals_a.p);
    G.mask = sort_into_cells(keys_a.p, keys_b.p, vals_a.p, vals_b.p, c.n, c.m, 64, c.xyz.p, nullptr, P4, nullptr, temp, counter, table, s).mask;
    G.P4 = P4.p; G.table = table.p;
    return G;
  }

  // one level: the open queries of `q` against grid G of the other cloud; leaves the next level's list
  void search_level(EvalCloud& q, const EvalGrid& G, float thr, int level) {
    flags.reserve(q.n_open);
    hipLaunchKernelGGL(k_eval_search, blocks(q.n_open), dim3(kEvalBlock), 0, s, q.Q4.p, q.open, q.n_open, G, thr, (unsigned char)level, q.near_cls.p, flags.p);
    const size_t left = scan(q.n_open);
    DevBuf<unsigned>& out = q.open == q.open_a.p ? q.open_b : q.open_a;
    if (left) {
      out.reserve(left);
      hipLaunchKernelGGL(k_eval_compact, blocks(q.n_open), dim3(kEvalBlock), 0, s, q.open, flags.p, offsets.p, q.n_open, out.p);
    }
    q.open = out.p; q.n_open = left;
  }

  // rules 6 and 7 for one kind of voxel: the per-voxel record into `out`, sums[k] and counts[k] of the ratios
  void voxels(EvalCloud& c, bool with_free, float h, int T, e3d_eval::Voxels& out, double* sums, unsigned long long* counts) {
    for (int k = 0; k < T; ++k) { sums[k] = 0.0; counts[k] = 0; }
    if (c.m == 0) return;
    keys_a.reserve(c.n); keys_b.reserve(c.n); vals_a.reserve(c.n); vals_b.reserve(c.n); flags.reserve(c.m);
    timer[3].start(s);                              // the group's time leaves out the allocations and the copies of the result
    hipLaunchKernelGGL(k_eval_voxel_keys, blocks(c.n), dim3(kEvalBlock), 0, s, c.xyz.p, c.n, h, keys_a.p, vals_a.p);
    sort_pairs_u64_u32(keys_a.p, keys_b.p, vals_a.p, vals_b.p, c.n, 64, temp, s);
    launch_flag_run_starts(keys_b.p, c.m, flags.p, s);
    const size_t nv = scan(c.m);
    timer[3].stop(s);
    DevBuf<unsigned> starts;
    DevBuf<int> ijk, npts, ca, cb;
    DevBuf<double> ratio, psum, fsum;
    DevBuf<unsigned char> evaluated;
    DevBuf<unsigned long long> pcount, fcount;
    const size_t nb = div_up(nv, kEvalReduceChunk);
    starts.reserve(nv); ijk.reserve(3 * nv); npts.reserve(nv); ca.reserve(T * nv); cb.reserve(T * nv); ratio.reserve(T * nv); evaluated.reserve(T * nv);
    psum.reserve(T * nb); pcount.reserve(T * nb); fsum.reserve(T); fcount.reserve(T);
    timer[3].start(s);
    hipLaunchKernelGGL(k_eval_voxel_starts, blocks(c.m), dim3(kEvalBlock), 0, s, flags.p, offsets.p, c.m, starts.p);
    hipLaunchKernelGGL(k_eval_voxel_counts, blocks(nv), dim3(kEvalBlock), 0, s, keys_b.p, vals_b.p, starts.p, nv, c.m, c.near_cls.p,
                       with_free ? c.free_cls.p : nullptr, T, ijk.p, npts.p, ca.p, cb.p, ratio.p, evaluated.p);
    hipLaunchKernelGGL(k_eval_reduce<unsigned char>, dim3((unsigned)nb), dim3(kEvalBlock), 0, s, ratio.p, evaluated.p, nv, T, (size_t)kEvalReduceChunk, psum.p, pcount.p);
    hipLaunchKernelGGL(k_eval_reduce<unsigned long long>, dim3(1), dim3(kEvalBlock), 0, s, psum.p, pcount.p, nb, T, nb, fsum.p, fcount.p);
    timer[3].stop(s);
    out.ijk.resize(3 * nv); out.npts.resize(nv); out.count_a.resize(T * nv); out.count_b.resize(T * nv);
    copy_out(out.ijk.data(), ijk.p, sizeof(int32_t) * 3 * nv, s);
    copy_out(out.npts.data(), npts.p, sizeof(int32_t) * nv, s);
    copy_out(out.count_a.data(), ca.p, sizeof(int32_t) * T * nv, s);
    copy_out(out.count_b.data(), cb.p, sizeof(int32_t) * T * nv, s);
    copy_out(sums, fsum.p, sizeof(double) * T, s);
    copy_out(counts, fcount.p, sizeof(unsigned long long) * T, s);
    E3D_HIP(hipStreamSynchronize(s));
    E3D_HIP(hipGetLastError());
  }
};

void evaluate(e3d_eval& out, const float* rec_xyz, size_t n_rec, const float* scan_xyz, const int64_t* scan_offsets, const float* scan_origins, int S,
              const float* tolerances, int T, float h, int N) {
  const char* const fn = "e3d_evaluate_reconstruction";
  if (S < 1) throw Error(E3D_ERR_INVALID, fmt("%s: at least one scan is needed", fn));
  if (!scan_offsets || !scan_origins || !tolerances) throw Error(E3D_ERR_INVALID, fmt("%s: null argument", fn));
  if (T < 1 || T > kEvalMaxT) throw Error(E3D_ERR_INVALID, fmt("%s: %d tolerances, 1 to %d are supported", fn, T, kEvalMaxT));
  EvalTolerances tol{};
  tol.T = T;
  for (int k = 0; k < T; ++k) {
    const float t = tolerances[k];
    if (!std::isfinite(t) || !(t > 0.f) || (k > 0 && !(t > tolerances[k - 1])))
      throw Error(E3D_ERR_INVALID, fmt("%s: the tolerances must be finite, positive and strictly ascending", fn));
    tol.t[k] = t;
    tol.thr[k] = (float)((double)t * (double)t);
  }
  if (!std::isfinite(h) || !(h > 0.f)) throw Error(E3D_ERR_INVALID, fmt("%s: the voxel size must be positive and finite", fn));
  if (N < 2 || N > 8192 || (N & 1)) throw Error(E3D_ERR_INVALID, fmt("%s: cube map size %d, an even size from 2 to 8192 is needed", fn, N));
  if (scan_offsets[0] != 0) throw Error(E3D_ERR_INVALID, fmt("%s: scan_offsets must start at 0", fn));
  for (int k = 0; k < S; ++k)
    if (scan_offsets[k + 1] < scan_offsets[k]) throw Error(E3D_ERR_INVALID, fmt("%s: scan_offsets must not descend", fn));
  const size_t n_scan = (size_t)scan_offsets[S];
  if (n_rec >= (size_t)1 << 31 || n_scan >= (size_t)1 << 31) throw Error(E3D_ERR_INVALID, fmt("%s: more than 2^31-1 points", fn));
  if ((n_rec && !rec_xyz) || (n_scan && !scan_xyz)) throw Error(E3D_ERR_INVALID, fmt("%s: null argument", fn));
  require_device();

  out.T = T;
  OwnedStream stream;
  hipStream_t s = stream.s;
  EvalRun run(s);
  EvalCloud rec, scan;
  run.upload(rec, rec_xyz, n_rec, h, T, true, "reconstruction");
  run.upload(scan, scan_xyz, n_scan, h, T, false, "scan");

  // ---- near classes: level by level, both directions -------------------------------------------------------------------------------------
  size_t closed[2][kEvalMaxT + 1] = {{0}};
  if (rec.m && scan.m) {
    rec.n_open = rec.m; scan.n_open = scan.m;
    for (int level = 0; level < T && (rec.n_open || scan.n_open); ++level) {
      EvalCloud* cl[2] = {&rec, &scan};
      EvalGrid G[2];
      run.timer[0].start(s);
      for (int k = 0; k < 2; ++k) {
        // the level-0 grids stay: their order is the search order.  A later level's grid is built only if the other cloud has open queries
        if (level == 0) G[k] = cl[k]->grid0 = run.build_grid(*cl[k], (double)tol.t[0], cl[k]->Q4, cl[k]->table0);
        else if (cl[1 - k]->n_open) G[k] = run.build_grid(*cl[k], (double)tol.t[level], cl[k]->P4, cl[k]->table);
      }
      run.timer[0].stop(s);
      run.timer[1].start(s);
      for (int k = 0; k < 2; ++k) {
        const size_t before = cl[k]->n_open;
        if (before) run.search_level(*cl[k], G[1 - k], tol.thr[level], level);
        closed[k][level] = before - cl[k]->n_open;
      }
      run.timer[1].stop(s);
    }
    E3D_HIP(hipGetLastError());
    for (EvalCloud* c : {&rec, &scan}) { c->Q4.release(); c->table0.release(); c->P4.release(); c->table.release(); c->open_a.release(); c->open_b.release(); }
  }

  // ---- free classes: one range image at a time ---------------------------------------------------------------------------------------------
  if (rec.m && scan.m) {
    DevBuf<unsigned> rmin;
    const size_t pixels = (size_t)6 * N * N;
    rmin.reserve(pixels);
    run.timer[2].start(s);
    for (int k = 0; k < S; ++k) {
      const size_t b = (size_t)scan_offsets[k], cnt = (size_t)scan_offsets[k + 1] - b;
      if (cnt == 0) continue;
      const float* o = scan_origins + 3 * k;
      E3D_HIP(hipMemsetAsync(rmin.p, 0xFF, sizeof(unsigned) * pixels, s));
      hipLaunchKernelGGL(k_eval_range_min, EvalRun::blocks(cnt), dim3(kEvalBlock), 0, s, scan.xyz.p + 3 * b, cnt, o[0], o[1], o[2], N, rmin.p);
      hipLaunchKernelGGL(k_eval_free, EvalRun::blocks(rec.n), dim3(kEvalBlock), 0, s, rec.xyz.p, rec.n, o[0], o[1], o[2], N, rmin.p, tol, rec.free_cls.p);
    }
    run.timer[2].stop(s);
    E3D_HIP(hipStreamSynchronize(s));            // rmin is freed on leaving the block
    E3D_HIP(hipGetLastError());
  }

  // ---- voxels and scores ----------------------------------------------------------------------------------------------------------------------
  double sums[2][kEvalMaxT];
  unsigned long long counts[2][kEvalMaxT];
  run.voxels(scan, false, h, T, out.vox[0], sums[0], counts[0]);
  run.voxels(rec, true, h, T, out.vox[1], sums[1], counts[1]);
  for (int k = 0; k < T; ++k) {
    const double c = counts[0][k] ? sums[0][k] / (double)counts[0][k] : 0.0;
    const double a = counts[1][k] ? sums[1][k] / (double)counts[1][k] : 0.0;
    out.scores[k] = c;
    out.scores[T + k] = a;
    out.scores[2 * T + k] = (a + c) > 0.0 ? ((2.0 * a) * c) / (a + c) : 0.0;
    out.evaluated[k] = (int64_t)counts[1][k];
  }

  out.near_rec.resize(n_rec); out.free_rec.resize(n_rec); out.near_scan.resize(n_scan);
  copy_out(out.near_rec.data(), rec.near_cls.p, n_rec, s);
  copy_out(out.free_rec.data(), rec.free_cls.p, n_rec, s);
  copy_out(out.near_scan.data(), scan.near_cls.p, n_scan, s);
  E3D_HIP(hipStreamSynchronize(s));
  E3D_HIP(hipGetLastError());
  for (int g = 0; g < kEvalGroups; ++g) out.ms[g] = run.timer[g].ms();
  static const bool trace = env_default_off("E3D_EVAL_TRACE");
  if (trace) {
    fprintf(stderr, "[evaluate] %zu reconstruction points (%zu not ignored), %zu scan points (%zu), %zu + %zu voxels\n", n_rec, rec.m, n_scan, scan.m,
            out.vox[0].npts.size(), out.vox[1].npts.size());
    for (int k = 0; k < T; ++k) fprintf(stderr, "[evaluate] level %d (%g): %zu reconstruction and %zu scan queries close\n", k, (double)tol.t[k], closed[0][k], closed[1][k]);
  }
}

}  // namespace

extern "C" {

e3d_eval_t* e3d_evaluate_reconstruction(const float* rec_xyz, size_t n_rec, const float* scan_xyz, const int64_t* scan_offsets, const float* scan_origins,
                                        int n_scans, const float* tolerances, int n_tolerances, float voxel_size, int cube_map_size) {
  e3d_eval* h = nullptr;
  E3D_TRY
  h = new e3d_eval;
  evaluate(*h, rec_xyz, n_rec, scan_xyz, scan_offsets, scan_origins, n_scans, tolerances, n_tolerances, voxel_size, cube_map_size);
  return h;
  E3D_CATCH_NEW(h)
}

void e3d_eval_destroy(e3d_eval_t* h) { delete h; }

int e3d_eval_counts(e3d_eval_t* h, int64_t* n_scan_voxels, int64_t* n_rec_voxels, int64_t* evaluated_voxels) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_eval_counts: null handle");
  if (n_scan_voxels) *n_scan_voxels = (int64_t)h->vox[0].npts.size();
  if (n_rec_voxels) *n_rec_voxels = (int64_t)h->vox[1].npts.size();
  if (evaluated_voxels) memcpy(evaluated_voxels, h->evaluated, sizeof(int64_t) * h->T);
  return 0;
  E3D_CATCH()
}

int e3d_eval_get_scores(e3d_eval_t* h, double* scores) {
  E3D_TRY
  if (!h || !scores) throw Error(E3D_ERR_INVALID, "e3d_eval_get_scores: null argument");
  memcpy(scores, h->scores, sizeof(double) * 3 * h->T);
  return 0;
  E3D_CATCH()
}

int e3d_eval_get_classes(e3d_eval_t* h, uint8_t* near_rec, uint8_t* free_class, uint8_t* near_scan) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_eval_get_classes: null handle");
  if (near_rec && !h->near_rec.empty()) memcpy(near_rec, h->near_rec.data(), h->near_rec.size());
  if (free_class && !h->free_rec.empty()) memcpy(free_class, h->free_rec.data(), h->free_rec.size());
  if (near_scan && !h->near_scan.empty()) memcpy(near_scan, h->near_scan.data(), h->near_scan.size());
  return 0;
  E3D_CATCH()
}

int e3d_eval_get_voxels(e3d_eval_t* h, int kind, int32_t* ijk, int32_t* n_points, int32_t* count_a, int32_t* count_b) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_eval_get_voxels: null handle");
  if (kind != 0 && kind != 1) throw Error(E3D_ERR_INVALID, "e3d_eval_get_voxels: kind must be 0 (scan) or 1 (reconstruction)");
  const e3d_eval::Voxels& v = h->vox[kind];
  if (v.npts.empty()) return 0;
  if (ijk) memcpy(ijk, v.ijk.data(), sizeof(int32_t) * v.ijk.size());
  if (n_points) memcpy(n_points, v.npts.data(), sizeof(int32_t) * v.npts.size());
  if (count_a) memcpy(count_a, v.count_a.data(), sizeof(int32_t) * v.count_a.size());
  if (count_b) memcpy(count_b, v.count_b.data(), sizeof(int32_t) * v.count_b.size());
  return 0;
  E3D_CATCH()
}

int e3d_eval_kernel_ms(e3d_eval_t* h, float* ms, const char** names, int capacity) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_eval_kernel_ms: null handle");
  for (int g = 0; g < kEvalGroups && g < capacity; ++g) {
    if (ms) ms[g] = h->ms[g];
    if (names) names[g] = kEvalGroupNames[g];
  }
  return kEvalGroups;
  E3D_CATCH()
}

}  // extern "C"
