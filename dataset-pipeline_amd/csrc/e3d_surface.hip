// e3d_surface.hip -- SurfaceReconstructor: an occlusion mesh from an oriented point cloud on the MI355X.
//
// The reference leaves this step to MeshLab / PoissonRecon.  Here a signed field f = sum w n.(x - p) / sum w with the compact weight
// w = (1 - d^2 / R^2)^2 is evaluated at the corners of a lattice of edge h that is anchored at the world origin, and one vertex per
// cell with a sign change plus one quad per crossing lattice edge are written (the rules: include/e3d_hip.h, e3d_surface_reconstruct).
// Everything the result depends on is f64; f32 only carries the input and the final vertices.
//
//  grid        the contributing points sorted into a hashed grid of cell max(R, h) (HashEntry / cell_key / launch_build_table)
//  candidates  the occupied h-voxels (sort + unique), dilated to BRICKS of 4 x 4 x 4 corners (sort + unique).  A brick is the unit of
//              the field kernel: any superset of the defined corners is correct, corners where no point counts drop out
//  field       k_surf_field: one wave per brick, one corner per lane.  The grid cells that can hold a counting point of the brick are
//              looked up 64 at a time (one per lane); each non-empty cell's run of points is staged through LDS as f64, 64 points per
//              step, and every lane adds the staged points that count for its corner.  A corner's sums live in one lane and are
//              formed in grid order: no atomics, and the launch order cannot show
//  fill        (e3d_surface_reconstruct_filled with N > 0 only) N Jacobi iterations that extend the field into undefined corners next to
//              where the surface ends, on a brick list enlarged by floor((N + 9) / 4) face steps: per iteration k_surf_fill_x,
//              k_surf_fill_x1 and k_surf_fill_update, one wave per brick, neighbours by __shfl and from the six face-neighbour bricks
//  solids      (with operations only) oriented boxes united with or subtracted from the field before the corners are
//              compacted: k_surf_solid_brick_keys adds the bricks of every union box's band to the candidates, k_surf_apply_solids
//              applies the operation list per candidate corner and writes the defined flag
//  corners     the defined corners compacted and sorted by (k, j, i)
//  extract     crossing flags per (corner, axis) from a brick lookup, stable compaction to the edge list (= quad order); the four
//              cells of every edge sorted + unique = the vertices in (k, j, i); vertex positions and triangles
#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "../../include/e3d_hip.h"
#include "e3d_grid.hpp"

#pragma clang fp contract(off)

namespace e3d {

constexpr int kSurfBlock = 256;
constexpr int kSurfOrgMargin = 16;                 // lattice units kept free below the lowest occupied voxel: dilation (<= 9) + a cell
constexpr int kSurfGridBias = 1 << 20;             // grid-cell coordinates are in [-2^20, 2^20): cell >= h and |p| / h < 2^20
constexpr int kSurfGroups = 5;                     // of a plain call; with solids one more, "solids", and with hole filling "fill", last
constexpr int kSurfMaxGroups = 7;
static const char* const kSurfGroupNames[kSurfGroups] = {"grid", "candidates", "field", "corners", "extract"};
constexpr int kSurfMaxOps = 256;
constexpr int kSurfMaxFill = 32;                   // iterations of the hole filling
constexpr int kSurfFillMargin = 4;                 // lattice steps beyond them that the range and span limits keep free

struct SurfParams {
  double h, R, R2;
  double cell, pad;                                // point grid: cell edge max(R, h) (1 + 1e-6); slack of a brick's search bounds
  int org[3];                                      // lattice coordinate of relative coordinate 0 (a multiple of 4)
  int D;                                           // ceil(R / h)
  unsigned mask;                                   // point grid's hash table size - 1
};

// the grid cell of a coordinate: ONE monotone function for the points and for the bounds of a brick's search
__device__ __forceinline__ int surf_grid_coord(double v, double cell) { return (int)floor(v / cell); }

__device__ __forceinline__ bool surf_contributes(const float* __restrict__ xyz, const float* __restrict__ nrm, size_t i) {
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2], a = nrm[3 * i], b = nrm[3 * i + 1], c = nrm[3 * i + 2];
  const bool finite = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(a) && isfinite(b) && isfinite(c);
  return finite && !(a == 0.f && b == 0.f && c == 0.f);
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// Per point: does it contribute, is it in range, its h-voxel; the voxels' bounding box in box[0..5] (min xyz, max xyz), box[6] =
// a contributing point out of range, box[7] = number of contributing points.  A fixed grid strides over the points and every block
// ends in one set of atomics (one per wave took 25 ms for 20 M points: 2 M atomics on eight words).
constexpr unsigned kSurfClassifyBlocks = 2048;
__global__ __launch_bounds__(kSurfBlock) void k_surf_classify(const float* __restrict__ xyz, const float* __restrict__ nrm, size_t n, double h,
                                                              int* __restrict__ box) {
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  int bad = 0, count = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (!surf_contributes(xyz, nrm, i)) continue;
    ++count;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double q = (double)xyz[3 * i + a] / h;
      if (!(fabs(q) < 1048576.0)) bad = 1;
      else { const int v = (int)floor(q); lo[a] = min(lo[a], v); hi[a] = max(hi[a], v); }
    }
  }
  __shared__ int part[kSurfBlock / kWave][8];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) { lo[a] = wave_min_i(lo[a]); hi[a] = wave_max_i(hi[a]); }
  bad = wave_max_i(bad);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { part[wv][a] = lo[a]; part[wv][3 + a] = hi[a]; }
    part[wv][6] = bad; part[wv][7] = count;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int t = threadIdx.x;
    int v = part[0][t];
    for (int k = 1; k < kSurfBlock / kWave; ++k) v = t < 3 ? min(v, part[k][t]) : t < 7 ? max(v, part[k][t]) : v + part[k][t];
    if (t < 3) { if (v != INT_MAX) atomicMin(&box[t], v); }
    else if (t < 6) { if (v != INT_MIN) atomicMax(&box[t], v); }
    else if (t == 6) { if (v) atomicOr(&box[6], 1); }
    else if (v) atomicAdd(&box[7], v);
  }
}

// Sort keys of the points: the point grid's cell (vals = point index) and the h-voxel relative to org; kEmptyKey for a point that
// does not contribute, which the sorts move to the end.
__global__ __launch_bounds__(kSurfBlock) void k_surf_point_keys(const float* __restrict__ xyz, const float* __restrict__ nrm, size_t n, SurfParams P,
                                                                unsigned long long* __restrict__ grid_keys, unsigned* __restrict__ vals,
                                                                unsigned long long* __restrict__ voxel_keys) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long gk = kEmptyKey, vk = kEmptyKey;
  if (surf_contributes(xyz, nrm, i)) {
    const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = (double)xyz[3 * i + 2];
    gk = cell_key(surf_grid_coord(x, P.cell) + kSurfGridBias, surf_grid_coord(y, P.cell) + kSurfGridBias, surf_grid_coord(z, P.cell) + kSurfGridBias);
    vk = cell_key((int)floor(x / P.h) - P.org[0], (int)floor(y / P.h) - P.org[1], (int)floor(z / P.h) - P.org[2]);
  }
  grid_keys[i] = gk;
  vals[i] = (unsigned)i;
  voxel_keys[i] = vk;
}

// the unique keys of sorted keys: those flagged by launch_flag_run_starts, compacted
__global__ __launch_bounds__(kSurfBlock) void k_surf_scatter_keys(const unsigned long long* __restrict__ keys, const unsigned char* __restrict__ flags,
                                                                  const unsigned* __restrict__ offsets, size_t n, unsigned long long* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n && flags[j]) out[offsets[j]] = keys[j];
}

// Every brick a voxel's corners can fall into: corners [v - D, v + D + 1] per axis count a point of voxel v at most (one step of
// margin each side for the rounding of p / h), M bricks per axis at most; slots beyond the range repeat its last brick.
__global__ __launch_bounds__(kSurfBlock) void k_surf_brick_keys(const unsigned long long* __restrict__ voxels, size_t n_voxels, int D, int M,
                                                                unsigned long long* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per = (size_t)M * M * M;
  if (t >= n_voxels * per) return;
  const unsigned long long v = voxels[t / per];
  const int slot = (int)(t % per);
  const int s[3] = {slot % M, (slot / M) % M, slot / (M * M)};
  int b[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int c = (int)((v >> (21 * a)) & 0x1FFFFF);
    const int lo = (c - D) >> 2, hi = (c + D + 1) >> 2;
    b[a] = min(lo + s[a], hi);
  }
  out[t] = cell_key(b[0], b[1], b[2]);
}

// The field at the 64 corners of one brick per wave (block = one wave, so the barriers are the wave's own).
__global__ __launch_bounds__(64) void k_surf_field(const unsigned long long* __restrict__ bricks, const float4* __restrict__ P4, const float4* __restrict__ N4,
                                                   const HashEntry* __restrict__ table, SurfParams P, double* __restrict__ f_out, double* __restrict__ w_out,
                                                   int* __restrict__ count_out) {
  __shared__ double stage[64][6];
  const int lane = threadIdx.x;
  const unsigned long long bk = bricks[blockIdx.x];
  const int b[3] = {(int)(bk & 0x1FFFFF), (int)((bk >> 21) & 0x1FFFFF), (int)((bk >> 42) & 0x1FFFFF)};
  const double x = P.h * (double)(P.org[0] + 4 * b[0] + (lane & 3));
  const double y = P.h * (double)(P.org[1] + 4 * b[1] + ((lane >> 2) & 3));
  const double z = P.h * (double)(P.org[2] + 4 * b[2] + (lane >> 4));
  // grid cells that can hold a point within R of a corner of the brick
  int c0[3], nc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = P.h * (double)(P.org[a] + 4 * b[a]) - P.R - P.pad, hi = P.h * (double)(P.org[a] + 4 * b[a] + 3) + P.R + P.pad;
    c0[a] = surf_grid_coord(lo, P.cell) + kSurfGridBias;
    nc[a] = surf_grid_coord(hi, P.cell) + kSurfGridBias - c0[a] + 1;
  }
  const int ncell = nc[0] * nc[1] * nc[2];
  double S = 0.0, W = 0.0;
  int cnt = 0;
  for (int base = 0; base < ncell; base += 64) {
    const int idx = base + lane;
    unsigned s = 0, e = 0;
    if (idx < ncell) hash_cell_range(table, P.mask, c0[0] + idx % nc[0], c0[1] + (idx / nc[0]) % nc[1], c0[2] + idx / (nc[0] * nc[1]), s, e);
    unsigned long long nonempty = __ballot(e > s);
    while (nonempty) {
      const int src = __ffsll((long long)nonempty) - 1;
      nonempty &= nonempty - 1;
      const unsigned cs = __shfl(s, src, 64), ce = __shfl(e, src, 64);
      for (unsigned m = cs; m < ce; m += 64) {
        __syncthreads();
        if (m + lane < ce) {
          const float4 p = P4[m + lane], q = N4[m + lane];
          stage[lane][0] = (double)p.x; stage[lane][1] = (double)p.y; stage[lane][2] = (double)p.z;
          stage[lane][3] = (double)q.x; stage[lane][4] = (double)q.y; stage[lane][5] = (double)q.z;
        }
        __syncthreads();
        const int chunk = (int)min(64u, ce - m);
        for (int t = 0; t < chunk; ++t) {
          const double dx = x - stage[t][0], dy = y - stage[t][1], dz = z - stage[t][2];
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          if (d2 < P.R2) {
            const double om = 1.0 - d2 / P.R2;
            const double w = om * om;
            S += w * ((stage[t][3] * dx + stage[t][4] * dy) + stage[t][5] * dz);
            W += w;
            ++cnt;
          }
        }
      }
    }
  }
  const size_t o = (size_t)blockIdx.x * 64 + lane;
  f_out[o] = cnt ? S / W : 0.0;
  w_out[o] = W;
  count_out[o] = cnt;
}

// The function of an oriented box at x: negative inside, 0 on its surface, 1-Lipschitz (the rules: include/e3d_hip.h).  An operation
// is 16 doubles on the device (128 B): o[0] kind, o[1..3] centre, o[4..12] rotation (row-major), o[13..15] half extents.
__device__ __forceinline__ double surf_box_g(const double* o, double x, double y, double z) {
  const double d0 = x - o[1], d1 = y - o[2], d2 = z - o[3];
  const double q0 = fabs((o[4] * d0 + o[7] * d1) + o[10] * d2) - o[13];
  const double q1 = fabs((o[5] * d0 + o[8] * d1) + o[11] * d2) - o[14];
  const double q2 = fabs((o[6] * d0 + o[9] * d1) + o[12] * d2) - o[15];
  const double m = q0 >= q1 ? q0 : q1;                               // max: the first argument on equality
  return m >= q2 ? m : q2;
}

// The lattice box of a union solid's band |g| <= 2 h in bricks relative to org, and where its bricks start in the one list of all
// union solids' bricks.
struct SurfSolidBox {
  unsigned long long first;
  int b0[3], nb[3];
  int op;
  int pad;
};

// Candidates of the union solids: one thread per brick of every band's lattice box.  A brick is kept iff |g(brick centre)| <= thr =
// 2 h + 1.5 sqrt(3) h (1 + 1e-6): g is 1-Lipschitz and no corner of a brick is farther than 1.5 sqrt(3) h from its centre, so every
// corner with |g| <= 2 h lies in a kept brick.  out == nullptr: write the flags; otherwise scatter the kept bricks' keys.
__global__ __launch_bounds__(kSurfBlock) void k_surf_solid_brick_keys(const SurfSolidBox* __restrict__ boxes, int n_boxes, const double* __restrict__ ops,
                                                                      size_t n_total, SurfParams P, double thr, unsigned char* __restrict__ flags,
                                                                      const unsigned* __restrict__ offsets, unsigned long long* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_total) return;
  if (out && !flags[t]) return;
  int lo = 0, hi = n_boxes - 1;                                       // the last box that starts at or before t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (boxes[mid].first <= t) lo = mid; else hi = mid - 1;
  }
  const SurfSolidBox B = boxes[lo];
  const size_t r = t - B.first;
  const int b[3] = {B.b0[0] + (int)(r % (size_t)B.nb[0]), B.b0[1] + (int)((r / (size_t)B.nb[0]) % (size_t)B.nb[1]),
                    B.b0[2] + (int)(r / ((size_t)B.nb[0] * (size_t)B.nb[1]))};
  if (out) { out[offsets[t]] = cell_key(b[0], b[1], b[2]); return; }
  const double x = P.h * ((double)(P.org[0] + 4 * b[0]) + 1.5), y = P.h * ((double)(P.org[1] + 4 * b[1]) + 1.5),
               z = P.h * ((double)(P.org[2] + 4 * b[2]) + 1.5);
  flags[t] = fabs(surf_box_g(ops + 16 * (size_t)B.op, x, y, z)) <= thr ? 1 : 0;
}

// The operation list applied to every candidate corner, in order: one lane per corner, the list staged once per block in LDS (16
// doubles per operation; every lane reads the same entry, a broadcast).  f and the defined flag of a corner depend on that corner
// alone: no atomics, no dependence on the launch order.
__global__ __launch_bounds__(kSurfBlock) void k_surf_apply_solids(const unsigned long long* __restrict__ bricks, size_t n_slots, const double* __restrict__ ops,
                                                                  int n_ops, SurfParams P, const int* __restrict__ count, double* __restrict__ f,
                                                                  unsigned char* __restrict__ defined) {
  extern __shared__ double surf_ops[];
  for (int t = threadIdx.x; t < 16 * n_ops; t += kSurfBlock) surf_ops[t] = ops[t];
  __syncthreads();
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_slots) return;
  const unsigned long long bk = bricks[j >> 6];
  const int l = (int)(j & 63);
  const double x = P.h * (double)(P.org[0] + 4 * (int)(bk & 0x1FFFFF) + (l & 3));
  const double y = P.h * (double)(P.org[1] + 4 * (int)((bk >> 21) & 0x1FFFFF) + ((l >> 2) & 3));
  const double z = P.h * (double)(P.org[2] + 4 * (int)((bk >> 42) & 0x1FFFFF) + (l >> 4));
  const double band = 2.0 * P.h;
  bool def = count[j] > 0;
  double v = f[j];
  for (int o = 0; o < n_ops; ++o) {
    const double* op = surf_ops + 16 * o;
    const double g = surf_box_g(op, x, y, z);
    if (op[0] == (double)E3D_SURFACE_UNION) {
      if (def) v = g < v ? g : v;                                      // min: the first argument on equality
      else if (fabs(g) <= band) { def = true; v = g; }
    } else if (def) {
      const double ng = -g;
      v = ng > v ? ng : v;                                             // max
    }
  }
  f[j] = v;
  defined[j] = def ? 1 : 0;
}

// which candidate corners are defined: without solids those where a point counts
__global__ __launch_bounds__(kSurfBlock) void k_surf_corner_flags(const int* __restrict__ count, size_t n_slots, unsigned char* __restrict__ flags) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_slots) flags[j] = count[j] > 0 ? 1 : 0;
}
// keys (k, j, i) of the defined corners and their slots
__global__ __launch_bounds__(kSurfBlock) void k_surf_corner_keys(const unsigned long long* __restrict__ bricks, const unsigned char* __restrict__ flags,
                                                                 const unsigned* __restrict__ offsets, size_t n_slots, unsigned long long* __restrict__ keys,
                                                                 unsigned* __restrict__ slots) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_slots || !flags[j]) return;
  const unsigned long long bk = bricks[j >> 6];
  const int l = (int)(j & 63);
  const unsigned o = offsets[j];
  keys[o] = cell_key(4 * (int)(bk & 0x1FFFFF) + (l & 3), 4 * (int)((bk >> 21) & 0x1FFFFF) + ((l >> 2) & 3), 4 * (int)((bk >> 42) & 0x1FFFFF) + (l >> 4));
  slots[o] = (unsigned)j;
}

// position of a key in a sorted array of unique keys, or -1
__device__ __forceinline__ long long surf_find(const unsigned long long* __restrict__ keys, size_t n, unsigned long long key) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && keys[lo] == key) ? (long long)lo : -1;
}
// slot of a corner (relative coordinates) in the field arrays, or -1 if no brick holds it
__device__ __forceinline__ long long surf_corner_slot(const unsigned long long* __restrict__ bricks, size_t n_bricks, int i, int j, int k) {
  if (i < 0 || j < 0 || k < 0) return -1;
  const long long b = surf_find(bricks, n_bricks, cell_key(i >> 2, j >> 2, k >> 2));
  return b < 0 ? -1 : b * 64 + ((k & 3) << 4 | (j & 3) << 2 | (i & 3));
}

struct SurfField {
  const unsigned long long* bricks; size_t n_bricks;
  const double* f; const int* count;
  const unsigned char* defined;                    // per slot: with solids a corner can be defined where no point counts
};
// does the edge from corner a (defined, field fa) along axis d cross; its parameter t
__device__ __forceinline__ bool surf_edge(const SurfField& F, int i, int j, int k, int d, double& t, bool& a_negative) {
  const long long sa = surf_corner_slot(F.bricks, F.n_bricks, i, j, k);
  if (sa < 0 || !F.defined[sa]) return false;
  const long long sb = surf_corner_slot(F.bricks, F.n_bricks, i + (d == 0), j + (d == 1), k + (d == 2));
  if (sb < 0 || !F.defined[sb]) return false;
  const double fa = F.f[sa], fb = F.f[sb];
  a_negative = fa < 0.0;
  if (a_negative == (fb < 0.0)) return false;
  t = fa / (fa - fb);
  return true;
}

// the sorted corners' public record and the crossing flags of their three edges
__global__ __launch_bounds__(kSurfBlock) void k_surf_corner_out(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ slots, size_t n_corners,
                                                                SurfParams P, SurfField F, const double* __restrict__ w, int* __restrict__ ijk,
                                                                double* __restrict__ f_out, double* __restrict__ w_out, int* __restrict__ count_out,
                                                                unsigned char* __restrict__ cross) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_corners) return;
  const unsigned long long key = keys[c];
  const int i = (int)(key & 0x1FFFFF), j = (int)((key >> 21) & 0x1FFFFF), k = (int)((key >> 42) & 0x1FFFFF);
  const unsigned s = slots[c];
  ijk[3 * c] = i + P.org[0]; ijk[3 * c + 1] = j + P.org[1]; ijk[3 * c + 2] = k + P.org[2];
  f_out[c] = F.f[s]; w_out[c] = w[s]; count_out[c] = F.count[s];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double t; bool neg;
    cross[3 * c + d] = surf_edge(F, i, j, k, d, t, neg) ? 1 : 0;
  }
}

// the four cells around edge (a, d): offsets (-1, -1), (0, -1), (0, 0), (-1, 0) in (u, v) = ((d + 1) % 3, (d + 2) % 3)
__device__ __forceinline__ unsigned long long surf_quad_cell(int i, int j, int k, int d, int q) {
  int c[3] = {i, j, k};
  const int u = (d + 1) % 3, v = (d + 2) % 3;
  c[u] += (q == 0 || q == 3) ? -1 : 0;
  c[v] += (q == 0 || q == 1) ? -1 : 0;
  return cell_key(c[0], c[1], c[2]);
}

// crossing edges in quad order (compacted from the flags): edge e = (corner, axis), and the keys of its four cells
__global__ __launch_bounds__(kSurfBlock) void k_surf_edges(const unsigned long long* __restrict__ corner_keys, const unsigned char* __restrict__ cross,
                                                           const unsigned* __restrict__ offsets, size_t n_flags, unsigned* __restrict__ edges,
                                                           unsigned long long* __restrict__ cell_keys) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_flags || !cross[t]) return;
  const unsigned e = offsets[t];
  edges[e] = (unsigned)t;
  const unsigned long long key = corner_keys[t / 3];
  const int i = (int)(key & 0x1FFFFF), j = (int)((key >> 21) & 0x1FFFFF), k = (int)((key >> 42) & 0x1FFFFF), d = (int)(t % 3);
#pragma unroll
  for (int q = 0; q < 4; ++q) cell_keys[4 * (size_t)e + q] = surf_quad_cell(i, j, k, d, q);
}

// one vertex per active cell: the mean of the crossing points of its 12 edges (axis, then v, then u), rounded to f32 at the end
__global__ __launch_bounds__(kSurfBlock) void k_surf_vertices(const unsigned long long* __restrict__ cells, size_t n_cells, SurfParams P, SurfField F,
                                                              float* __restrict__ vertices, int* __restrict__ cell_ijk) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  const unsigned long long key = cells[c];
  const int o[3] = {(int)(key & 0x1FFFFF), (int)((key >> 21) & 0x1FFFFF), (int)((key >> 42) & 0x1FFFFF)};
  double sum[3] = {0.0, 0.0, 0.0};
  int m = 0;
  for (int d = 0; d < 3; ++d) {
    const int u = (d + 1) % 3, v = (d + 2) % 3;
    for (int dv = 0; dv < 2; ++dv)
      for (int du = 0; du < 2; ++du) {
        int a[3] = {o[0], o[1], o[2]};
        a[u] += du; a[v] += dv;
        double t; bool neg;
        if (!surf_edge(F, a[0], a[1], a[2], d, t, neg)) continue;
        double p[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) p[x] = P.h * (double)(a[x] + P.org[x]);
        p[d] = p[d] + t * P.h;
        sum[0] += p[0]; sum[1] += p[1]; sum[2] += p[2];
        ++m;
      }
  }
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    vertices[3 * c + x] = (float)(sum[x] / (double)m);
    cell_ijk[3 * c + x] = o[x] + P.org[x];
  }
}

// two triangles per crossing edge: (q0, q1, q2), (q0, q2, q3) of the cells' vertices, the four in reverse if a is not negative
__global__ __launch_bounds__(kSurfBlock) void k_surf_triangles(const unsigned* __restrict__ edges, size_t n_edges, const unsigned long long* __restrict__ corner_keys,
                                                               const unsigned* __restrict__ slots, const double* __restrict__ f,
                                                               const unsigned long long* __restrict__ cells, size_t n_cells, unsigned* __restrict__ tri) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const unsigned t = edges[e];
  const unsigned long long key = corner_keys[t / 3];
  const int i = (int)(key & 0x1FFFFF), j = (int)((key >> 21) & 0x1FFFFF), k = (int)((key >> 42) & 0x1FFFFF), d = (int)(t % 3);
  const bool a_negative = f[slots[t / 3]] < 0.0;
  unsigned q[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) q[a_negative ? x : 3 - x] = (unsigned)surf_find(cells, n_cells, surf_quad_cell(i, j, k, d, x));
  unsigned* o = tri + 6 * e;
  o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[0]; o[4] = q[2]; o[5] = q[3];
}

// ---- hole filling (e3d_surface_reconstruct_filled; the rules: include/e3d_hip.h) ---------------------------------------------------------
// A corner's state is one byte: defined, source (defined by the scan field), negative (f < 0, so that the X pass reads no f).  One
// wave per brick, one corner per lane as in k_surf_field.  A face neighbour inside the brick is read from the neighbouring lane's
// register (__shfl), one across a face from the neighbour brick's arrays (16 lanes per direction).  An iteration is three passes
// with a reach of one cell each -- X, X1, then growth and smoothing -- so only the six face-neighbour bricks are ever read, and
// every pass reads state t - 1 and writes other arrays: no atomics, no dependence on the launch order.
constexpr unsigned kFillDefined = 1, kFillSource = 2, kFillNegative = 4;

// which bricks hold a defined corner of the scan field: the seeds of the candidate set
__global__ __launch_bounds__(64) void k_surf_fill_seed_flags(const int* __restrict__ count, unsigned char* __restrict__ flags) {
  const bool any = __any(count[(size_t)blockIdx.x * 64 + threadIdx.x] > 0);
  if (threadIdx.x == 0) flags[blockIdx.x] = any ? 1 : 0;
}

// the face neighbour `d` (-x, +x, -y, +y, -z, +z) of a brick, or the brick itself where the neighbour leaves the 19 bits per axis
__device__ __forceinline__ unsigned long long surf_fill_neighbour_key(unsigned long long key, int d) {
  int b[3] = {(int)(key & 0x1FFFFF), (int)((key >> 21) & 0x1FFFFF), (int)((key >> 42) & 0x1FFFFF)};
  const int v = b[d >> 1] + ((d & 1) ? 1 : -1);
  if (v >= 0 && v < (1 << 19)) b[d >> 1] = v;
  return cell_key(b[0], b[1], b[2]);
}

// one step of the dilation: every brick and its six face neighbours (sorted + unique afterwards)
__global__ __launch_bounds__(kSurfBlock) void k_surf_fill_dilate(const unsigned long long* __restrict__ bricks, size_t n, unsigned long long* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 7 * n) return;
  const unsigned long long key = bricks[t / 7];
  const int slot = (int)(t % 7);
  out[t] = slot ? surf_fill_neighbour_key(key, slot - 1) : key;
}

// f, W and count re-laid onto the enlarged brick list (zero where the old list has no such brick, as k_surf_field writes where no
// point counts), the corners' first state and the per-brick flag "holds a defined corner"
__global__ __launch_bounds__(64) void k_surf_fill_relay(const unsigned long long* __restrict__ bricks, const unsigned long long* __restrict__ old_bricks, size_t n_old,
                                                        const double* __restrict__ f_old, const double* __restrict__ w_old, const int* __restrict__ count_old,
                                                        double* __restrict__ f, double* __restrict__ w, int* __restrict__ count, unsigned char* __restrict__ state,
                                                        unsigned char* __restrict__ holds) {
  const int lane = threadIdx.x;
  const long long ob = surf_find(old_bricks, n_old, bricks[blockIdx.x]);
  double fv = 0.0, wv = 0.0;
  int c = 0;
  if (ob >= 0) { const size_t so = (size_t)ob * 64 + lane; fv = f_old[so]; wv = w_old[so]; c = count_old[so]; }
  const size_t o = (size_t)blockIdx.x * 64 + lane;
  f[o] = fv; w[o] = wv; count[o] = c;
  state[o] = (unsigned char)(c > 0 ? (kFillDefined | kFillSource | (fv < 0.0 ? kFillNegative : 0u)) : 0u);
  const bool any = __any(c > 0);
  if (lane == 0) holds[blockIdx.x] = any ? 1 : 0;
}

// the six face-neighbour bricks of every brick as indices into the sorted list, -1 where there is none
__global__ __launch_bounds__(kSurfBlock) void k_surf_fill_neighbours(const unsigned long long* __restrict__ bricks, size_t n, int* __restrict__ nbr) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * n) return;
  const unsigned long long key = bricks[t / 6], nk = surf_fill_neighbour_key(key, (int)(t % 6));
  nbr[t] = nk == key ? -1 : (int)surf_find(bricks, n, nk);
}

// Nothing can change in a brick while neither it nor a face neighbour holds a defined corner: wave-uniform, before any value is read
__device__ __forceinline__ bool surf_fill_active(const int* __restrict__ nbr, const unsigned char* __restrict__ holds, int lane) {
  const int q = lane < 6 ? nbr[6 * (size_t)blockIdx.x + lane] : lane == 6 ? (int)blockIdx.x : -1;
  return __any(q >= 0 && holds[q] != 0);
}

// the value of the face neighbour d of this lane's corner: `own` of the neighbouring lane, or a[] of the neighbour brick's corner
template <class T>
__device__ __forceinline__ T surf_fill_gather(const T* __restrict__ a, int nb, int lane, T own, int d, bool wanted = true) {
  const int shift = 2 * (d >> 1), stride = 1 << shift, c = (lane >> shift) & 3;
  const bool up = d & 1;
  const bool edge = up ? c == 3 : c == 0;
  T v = __shfl(own, (up ? lane + stride : lane - stride) & 63, 64);
  if (edge) v = (nb >= 0 && wanted) ? a[(size_t)nb * 64 + (up ? lane - 3 * stride : lane + 3 * stride)] : T(0);
  return v;
}

// X(y): y is defined and has a defined neighbour of the other sign
__global__ __launch_bounds__(64) void k_surf_fill_x(const int* __restrict__ nbr, const unsigned char* __restrict__ holds, const unsigned char* __restrict__ state,
                                                    unsigned char* __restrict__ x) {
  const int lane = threadIdx.x;
  if (!surf_fill_active(nbr, holds, lane)) return;
  const size_t o = (size_t)blockIdx.x * 64 + lane;
  const unsigned own = state[o];
  bool hit = false;
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    const unsigned s = surf_fill_gather<unsigned char>(state, nbr[6 * (size_t)blockIdx.x + d], lane, (unsigned char)own, d);
    hit = hit || ((s & kFillDefined) && ((s ^ own) & kFillNegative));
  }
  x[o] = (own & kFillDefined) && hit ? 1 : 0;
}

// X1(y): y is defined and X holds for y or for one of its neighbours
__global__ __launch_bounds__(64) void k_surf_fill_x1(const int* __restrict__ nbr, const unsigned char* __restrict__ holds, const unsigned char* __restrict__ state,
                                                     const unsigned char* __restrict__ x, unsigned char* __restrict__ x1) {
  const int lane = threadIdx.x;
  if (!surf_fill_active(nbr, holds, lane)) return;
  const size_t o = (size_t)blockIdx.x * 64 + lane;
  const unsigned char own = x[o];
  unsigned hit = own;
#pragma unroll
  for (int d = 0; d < 6; ++d) hit |= surf_fill_gather<unsigned char>(x, nbr[6 * (size_t)blockIdx.x + d], lane, own, d);
  x1[o] = (state[o] & kFillDefined) && hit ? 1 : 0;
}

// growth and smoothing: state and f of iteration t from those of t - 1
__global__ __launch_bounds__(64) void k_surf_fill_update(const int* __restrict__ nbr, const unsigned char* __restrict__ holds, const unsigned char* __restrict__ state,
                                                         const unsigned char* __restrict__ x1, const double* __restrict__ f, unsigned char* __restrict__ state_out,
                                                         double* __restrict__ f_out, unsigned char* __restrict__ holds_out) {
  const int lane = threadIdx.x;
  if (!surf_fill_active(nbr, holds, lane)) return;
  const size_t o = (size_t)blockIdx.x * 64 + lane;
  const unsigned char own = state[o], own_x1 = x1[o];
  const double own_f = f[o];
  bool near = false;
  double s = 0.0;
  int c = 0;
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    const int nb = nbr[6 * (size_t)blockIdx.x + d];
    const unsigned ns = surf_fill_gather<unsigned char>(state, nb, lane, own, d);
    const unsigned nx1 = surf_fill_gather<unsigned char>(x1, nb, lane, own_x1, d);   // (every lane takes part in the gather's __shfl)
    near = near || nx1 != 0;
    const double nf = surf_fill_gather<double>(f, nb, lane, own_f, d, (ns & kFillDefined) != 0);
    if (ns & kFillDefined) { s += nf; ++c; }
  }
  unsigned st = own;
  double v = own_f;
  if (!(own & kFillDefined)) {
    if (near) { v = s / (double)c; st = kFillDefined | (v < 0.0 ? kFillNegative : 0u); }
  } else if (!(own & kFillSource)) {
    s += own_f; ++c;
    v = s / (double)c;
    st = kFillDefined | (v < 0.0 ? kFillNegative : 0u);
  }
  state_out[o] = (unsigned char)st;
  f_out[o] = v;
  const bool any = __any((st & kFillDefined) != 0);
  if (lane == 0) holds_out[blockIdx.x] = any ? 1 : 0;
}

// After the last iteration: the defined flag the extraction reads, and the number the solids' kernel takes for "a point counts"
// (k_surf_apply_solids starts from count > 0): a filled corner enters it as an ordinary defined corner.  Its public count stays 0.
__global__ __launch_bounds__(kSurfBlock) void k_surf_fill_finish(const unsigned char* __restrict__ state, const int* __restrict__ count, size_t n_slots,
                                                                 unsigned char* __restrict__ defined, int* __restrict__ defined_count) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_slots) return;
  const bool def = (state[j] & kFillDefined) != 0;
  defined[j] = def ? 1 : 0;
  defined_count[j] = def ? max(count[j], 1) : 0;
}

__device__ __forceinline__ bool surf_fill_filled(const unsigned char* __restrict__ state, long long slot) {
  return (state[slot] & (kFillDefined | kFillSource)) == kFillDefined;
}
// the flag `filled` of the sorted corners
__global__ __launch_bounds__(kSurfBlock) void k_surf_fill_corner_flags(const unsigned* __restrict__ slots, size_t n_corners, const unsigned char* __restrict__ state,
                                                                       unsigned char* __restrict__ out) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n_corners) out[c] = surf_fill_filled(state, slots[c]) ? 1 : 0;
}
// a vertex is filled iff a crossing edge of its cell has a filled endpoint (the 12 edges as k_surf_vertices visits them)
__global__ __launch_bounds__(kSurfBlock) void k_surf_fill_vertex_flags(const unsigned long long* __restrict__ cells, size_t n_cells, SurfField F,
                                                                       const unsigned char* __restrict__ state, unsigned char* __restrict__ out) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  const unsigned long long key = cells[c];
  const int o[3] = {(int)(key & 0x1FFFFF), (int)((key >> 21) & 0x1FFFFF), (int)((key >> 42) & 0x1FFFFF)};
  bool filled = false;
  for (int d = 0; d < 3; ++d) {
    const int u = (d + 1) % 3, v = (d + 2) % 3;
    for (int dv = 0; dv < 2; ++dv)
      for (int du = 0; du < 2; ++du) {
        int a[3] = {o[0], o[1], o[2]};
        a[u] += du; a[v] += dv;
        double t; bool neg;
        if (!surf_edge(F, a[0], a[1], a[2], d, t, neg)) continue;
        filled = filled || surf_fill_filled(state, surf_corner_slot(F.bricks, F.n_bricks, a[0], a[1], a[2])) ||
                 surf_fill_filled(state, surf_corner_slot(F.bricks, F.n_bricks, a[0] + (d == 0), a[1] + (d == 1), a[2] + (d == 2)));
      }
  }
  out[c] = filled ? 1 : 0;
}

static int bits_for(unsigned v) { int b = 0; while (b < 32 && (v >> b)) ++b; return b; }

}  // namespace e3d

using namespace e3d;

struct e3d_surface {
  std::vector<int32_t> corner_ijk, corner_count, cell_ijk;
  std::vector<double> corner_f, corner_w;
  std::vector<float> vertices;
  std::vector<uint32_t> triangles;
  std::vector<uint8_t> corner_filled, vertex_filled;  // all zero unless the call filled holes
  float ms[kSurfMaxGroups] = {0, 0, 0, 0, 0, 0, 0};
  const char* names[kSurfMaxGroups] = {kSurfGroupNames[0], kSurfGroupNames[1], kSurfGroupNames[2], kSurfGroupNames[3], kSurfGroupNames[4], nullptr, nullptr};
  int groups = kSurfGroups;
};

namespace {

// The operation list checked on the host: the operations as the kernels read them (16 doubles each: kind, centre, rotation, half
// extents) and the lattice bounding box of every solid's band |g| <= 2 h (corner coordinates, one step of margin each side).
struct SurfSolids {
  std::vector<double> ops;
  std::vector<int> lo, hi;                          // 3 per solid
  bool any_union = false;
  size_t size() const { return ops.size() / 16; }
};

void check_solids(SurfSolids& S, const e3d_surface_solid_t* ops, size_t n_ops, double h) {
  if (n_ops > (size_t)kSurfMaxOps) throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_csg: %zu operations, at most %d", n_ops, kSurfMaxOps));
  if (n_ops && !ops) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct_csg: null argument");
  for (size_t o = 0; o < n_ops; ++o) {
    const e3d_surface_solid_t& B = ops[o];
    if (B.kind != E3D_SURFACE_UNION && B.kind != E3D_SURFACE_SUBTRACT)
      throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_csg: operation %zu has the unknown kind %d", o, (int)B.kind));
    bool finite = true;
    for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(B.centre[a]) && std::isfinite(B.half_extent[a]);
    for (int a = 0; a < 9; ++a) finite = finite && std::isfinite(B.rotation[a]);
    if (!finite) throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_csg: operation %zu has a centre, rotation or extent that is not finite", o));
    for (int a = 0; a < 3; ++a)
      if (!(B.half_extent[a] > 0.0)) throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_csg: operation %zu has a half extent <= 0", o));
    const double* Q = B.rotation;
    double dev = 0.0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double dot = (Q[a] * Q[b] + Q[3 + a] * Q[3 + b]) + Q[6 + a] * Q[6 + b];
        dev = std::max(dev, std::fabs(dot - (a == b ? 1.0 : 0.0)));
      }
    const double det = Q[0] * (Q[4] * Q[8] - Q[5] * Q[7]) - Q[1] * (Q[3] * Q[8] - Q[5] * Q[6]) + Q[2] * (Q[3] * Q[7] - Q[4] * Q[6]);
    if (dev > 1e-9 || det < 0.0)
      throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_csg: the rotation of operation %zu is not a proper rotation (max |Q^T Q - I| = %g, det = %g)", o, dev, det));
    // the band lies in the box's world bounding box grown by 2 h: |d_r| <= sum_m |Q[r][m]| (a_m + 2 h)
    for (int r = 0; r < 3; ++r) {
      double e = 0.0;
      for (int m = 0; m < 3; ++m) e += std::fabs(Q[3 * r + m]) * (B.half_extent[m] + 2.0 * h);
      if (!((std::fabs(B.centre[r]) + e) / h + 2.0 < 1048576.0))
        throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_csg: the band of operation %zu reaches |coordinate| / voxel size >= 2^20", o));
      S.lo.push_back((int)std::floor((B.centre[r] - e) / h) - 1);
      S.hi.push_back((int)std::ceil((B.centre[r] + e) / h) + 1);
    }
    S.ops.push_back((double)B.kind);
    S.ops.insert(S.ops.end(), B.centre, B.centre + 3);
    S.ops.insert(S.ops.end(), B.rotation, B.rotation + 9);
    S.ops.insert(S.ops.end(), B.half_extent, B.half_extent + 3);
    S.any_union = S.any_union || B.kind == E3D_SURFACE_UNION;
  }
}

void reconstruct(e3d_surface& out, const float* xyz, const float* normals, size_t n, float voxel_size, float support_radius,
                 int fill_iterations, const e3d_surface_solid_t* ops, size_t n_ops) {
  const double h = (double)voxel_size, R = (double)support_radius;
  const int N = fill_iterations;
  if (!std::isfinite(h) || !(h > 0.0)) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: the voxel size must be positive and finite");
  if (!std::isfinite(R) || !(R > 0.0)) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: the support radius must be positive and finite");
  if (R / h > 8.0) throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct: support radius / voxel size = %g, at most 8", R / h));
  if (n && (!xyz || !normals)) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: null argument");
  if (n >= (size_t)1 << 31) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: more than 2^31-1 points");
  if (N < 0 || N > kSurfMaxFill)
    throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_filled: fill_iterations = %d, 0 to %d are possible", N, kSurfMaxFill));
  SurfSolids solids;
  check_solids(solids, ops, n_ops, h);
  if (n_ops) out.names[out.groups++] = "solids";
  if (N) out.names[out.groups++] = "fill";
  require_device();
  // without a union nothing can be defined where no point counts: subtracting from nothing gives nothing
  if (n == 0 && !solids.any_union) return;

  OwnedStream stream;
  hipStream_t s = stream.s;
  Compactor run(s);
  EventTimer timer[kSurfGroups];
  const auto blocks = [](size_t m) { return dim3((unsigned)div_up(m, kSurfBlock)); };
  const auto scatter_keys = [&](const unsigned long long* sorted, size_t count, unsigned long long* unique) {
    hipLaunchKernelGGL(k_surf_scatter_keys, blocks(count), dim3(kSurfBlock), 0, s, sorted, run.flags.p, run.offsets.p, count, unique);
  };
  const size_t kMaxItems = ((size_t)1 << 32) - 64;        // the compactions use 32-bit offsets

  // ---- grid ----------------------------------------------------------------------------------------------------------------------
  DevBuf<float> d_xyz, d_nrm;
  DevBuf<int> box;
  int hb[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
  if (n) {
    d_xyz.reserve(3 * n); d_nrm.reserve(3 * n); box.reserve(8);
    copy_in(d_xyz.p, xyz, sizeof(float) * 3 * n, s);
    copy_in(d_nrm.p, normals, sizeof(float) * 3 * n, s);
    E3D_HIP(hipMemcpyAsync(box.p, hb, sizeof hb, hipMemcpyHostToDevice, s));
  }
  timer[0].start(s);                                                   // behind the copies of the cloud
  if (n) {
    hipLaunchKernelGGL(k_surf_classify, dim3((unsigned)std::min<size_t>(div_up(n, kSurfBlock), kSurfClassifyBlocks)), dim3(kSurfBlock), 0, s, d_xyz.p, d_nrm.p, n, h, box.p);
    copy_out(hb, box.p, sizeof hb, s);
    E3D_HIP(hipStreamSynchronize(s));
    E3D_HIP(hipGetLastError());
    if (hb[6]) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: a point lies at |coordinate| / voxel size >= 2^20");
  }
  const size_t m = (size_t)hb[7];
  if (m == 0 && !solids.any_union) return;
  // the fill can define corners up to N steps beyond the scan field's: the limits hold for the voxels' box grown by N + 4
  if (N && m)
    for (int a = 0; a < 3; ++a) {
      hb[a] -= N + kSurfFillMargin; hb[3 + a] += N + kSurfFillMargin;
      if (hb[a] < -(1 << 20) || hb[3 + a] >= (1 << 20))
        throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_filled: a point lies within fill_iterations + %d voxels of |coordinate| / voxel size = 2^20", kSurfFillMargin));
    }

  SurfParams P{};
  P.h = h; P.R = R; P.R2 = R * R;
  P.cell = std::max(R, h) * (1.0 + 1e-6);
  P.pad = 1e-6 * P.cell;
  P.D = (int)std::ceil(R / h);
  // the occupied voxels and the bands of the solids together
  int lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = m ? hb[a] : INT_MAX; hi[a] = m ? hb[3 + a] : INT_MIN;
    for (size_t o = 0; o < solids.size(); ++o) { lo[a] = std::min(lo[a], solids.lo[3 * o + a]); hi[a] = std::max(hi[a], solids.hi[3 * o + a]); }
  }
  unsigned ext[3];
  for (int a = 0; a < 3; ++a) {
    P.org[a] = (int)(std::floor((double)(lo[a] - kSurfOrgMargin) / 4.0) * 4.0);
    ext[a] = (unsigned)(hi[a] - P.org[a] + kSurfOrgMargin);
    if (ext[a] >= (1u << 21))
      throw Error(E3D_ERR_INVALID, N ? "e3d_surface_reconstruct_filled: the cloud grown by fill_iterations + 4 voxels on every side (and the solids) spans more than 2^21 - 36 voxels along an axis"
                                   : n_ops ? "e3d_surface_reconstruct: the cloud and the solids span more than 2^21 - 36 voxels along an axis"
                                           : "e3d_surface_reconstruct: the cloud spans more than 2^21 - 36 voxels along an axis");
  }
  const int key_bits = 42 + bits_for(ext[2]);

  DevBuf<unsigned long long> ka, kb, vk;
  DevBuf<unsigned> va, vb, counter;
  DevBuf<float4> P4, N4;
  DevBuf<HashEntry> table;
  P4.reserve(m); N4.reserve(m);
  if (m) {
    ka.reserve(n); kb.reserve(n); vk.reserve(n); va.reserve(n); vb.reserve(n);
    hipLaunchKernelGGL(k_surf_point_keys, blocks(n), dim3(kSurfBlock), 0, s, d_xyz.p, d_nrm.p, n, P, ka.p, va.p, vk.p);
  }
  const CellTable grid = sort_into_cells(ka.p, kb.p, va.p, vb.p, n, m, 64, d_xyz.p, d_nrm.p, P4, &N4, run.temp, counter, table, s);
  const size_t n_grid_cells = grid.n_cells;
  P.mask = grid.mask;
  timer[0].stop(s);

  // ---- solids: the bricks of the union solids' bands ---------------------------------------------------------------------------------
  GroupTimer solid_timer;
  DevBuf<double> d_ops;
  DevBuf<SurfSolidBox> d_boxes;
  DevBuf<unsigned long long> solid_keys;
  size_t n_solid_keys = 0;
  if (n_ops) {
    d_ops.reserve(solids.ops.size());
    copy_in(d_ops.p, solids.ops.data(), sizeof(double) * solids.ops.size(), s);
    std::vector<SurfSolidBox> boxes;
    size_t total = 0;
    for (size_t o = 0; o < solids.size(); ++o) {
      if (solids.ops[16 * o] != (double)E3D_SURFACE_UNION) continue;
      SurfSolidBox B{};
      B.first = total; B.op = (int)o;
      size_t count = 1;
      for (int a = 0; a < 3; ++a) {
        B.b0[a] = (solids.lo[3 * o + a] - P.org[a]) >> 2;
        B.nb[a] = ((solids.hi[3 * o + a] - P.org[a]) >> 2) - B.b0[a] + 1;
        count *= (size_t)B.nb[a];                                        // at most 2^19 per axis
      }
      total += count;
      if (total > kMaxItems) throw Error(E3D_ERR_INVALID, fmt("e3d_surface_reconstruct_csg: the solids up to operation %zu cover too many bricks for one call", o));
      boxes.push_back(B);
    }
    solid_timer.start(s);
    if (total) {
      d_boxes.reserve(boxes.size());
      copy_in(d_boxes.p, boxes.data(), sizeof(SurfSolidBox) * boxes.size(), s);
      const double thr = 2.0 * h + 1.5 * std::sqrt(3.0) * h * (1.0 + 1e-6);
      run.flags.reserve(total);
      hipLaunchKernelGGL(k_surf_solid_brick_keys, blocks(total), dim3(kSurfBlock), 0, s, d_boxes.p, (int)boxes.size(), d_ops.p, total, P, thr, run.flags.p,
                         (const unsigned*)nullptr, (unsigned long long*)nullptr);
      n_solid_keys = run.scan(total);
      solid_keys.reserve(n_solid_keys);
      if (n_solid_keys)
        hipLaunchKernelGGL(k_surf_solid_brick_keys, blocks(total), dim3(kSurfBlock), 0, s, d_boxes.p, (int)boxes.size(), d_ops.p, total, P, thr, run.flags.p,
                           run.offsets.p, solid_keys.p);
    }
    solid_timer.stop(s);
    E3D_HIP(hipStreamSynchronize(s));                                    // `boxes` is read by the copy above
  }

  // ---- candidates: occupied voxels -> bricks, with the solids' bricks --------------------------------------------------------------
  timer[1].start(s);
  DevBuf<unsigned long long> voxels, bricks;
  size_t n_voxels = 0;
  if (m) {
    // (the sort moves the keys of the points that do not contribute, kEmptyKey, behind the m others only with all 64 bits)
    const size_t n_sorted_voxels = run.sort_unique(vk, ka, voxels, n, 64, scatter_keys);
    n_voxels = n_sorted_voxels - (m < n ? 1 : 0);                      // kEmptyKey is the last unique key if any point was dropped
  }
  const int M = ((2 * P.D + 4) >> 2) + 1;
  const size_t n_brick_keys = n_voxels * (size_t)M * M * M;
  if (n_brick_keys > kMaxItems) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: too many occupied voxels for one call");
  if (n_brick_keys + n_solid_keys > kMaxItems) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct_csg: too many candidate bricks of the cloud and the solids for one call");
  kb.reserve(n_brick_keys + n_solid_keys);
  if (n_brick_keys) hipLaunchKernelGGL(k_surf_brick_keys, blocks(n_brick_keys), dim3(kSurfBlock), 0, s, voxels.p, n_voxels, P.D, M, kb.p);
  if (n_solid_keys) E3D_HIP(hipMemcpyAsync(kb.p + n_brick_keys, solid_keys.p, sizeof(unsigned long long) * n_solid_keys, hipMemcpyDeviceToDevice, s));
  size_t n_bricks = run.sort_unique(kb, ka, bricks, n_brick_keys + n_solid_keys, key_bits, scatter_keys);
  timer[1].stop(s);
  size_t n_slots = n_bricks * 64;
  if (n_slots > kMaxItems) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: too many candidate corners for one call");
  if (n_bricks == 0) { E3D_HIP(hipStreamSynchronize(s)); return; }

  // ---- field -------------------------------------------------------------------------------------------------------------------------
  DevBuf<double> f, w;
  DevBuf<int> count;
  f.reserve(n_slots); w.reserve(n_slots); count.reserve(n_slots);
  timer[2].start(s);
  hipLaunchKernelGGL(k_surf_field, dim3((unsigned)n_bricks), dim3(64), 0, s, bricks.p, P4.p, N4.p, table.p, P, f.p, w.p, count.p);
  timer[2].stop(s);
  E3D_HIP(hipGetLastError());

  // ---- fill: N iterations that extend the scan field next to where the surface ends ------------------------------------------------
  GroupTimer fill_timer;
  DevBuf<unsigned char> defined, fill_state;
  DevBuf<int> defined_count;                                           // what the solids' kernel reads as "a point counts" after a fill
  bool filled = false;
  if (N) {
    fill_timer.start(s);
    // the seeds: the bricks that hold a defined corner
    run.flags.reserve(n_bricks);
    hipLaunchKernelGGL(k_surf_fill_seed_flags, dim3((unsigned)n_bricks), dim3(64), 0, s, count.p, run.flags.p);
    size_t n_grown = run.scan(n_bricks);
    filled = n_grown > 0;
    if (filled) {
      // Candidates: every brick within floor((N + 9) / 4) face steps of a seed.  A corner defined in iteration t has a defined
      // neighbour in t - 1, so it lies within N lattice steps of a source; n steps along an axis cross at most ceil(n / 4) brick
      // faces, over three axes at most (N + 9) / 4.  Bricks beyond them stay empty, so which bricks are candidates shows nowhere.
      DevBuf<unsigned long long> grown, next;
      grown.reserve(n_grown);
      scatter_keys(bricks.p, n_bricks, grown.p);
      for (int step = 0; step < (N + 9) / 4; ++step) {
        if (7 * n_grown > kMaxItems) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct_filled: too many candidate bricks of the fill for one call");
        kb.reserve(7 * n_grown);
        hipLaunchKernelGGL(k_surf_fill_dilate, blocks(7 * n_grown), dim3(kSurfBlock), 0, s, grown.p, n_grown, kb.p);
        n_grown = run.sort_unique(kb, ka, next, 7 * n_grown, key_bits, scatter_keys);
        std::swap(grown, next);
      }
      // ... together with the candidates so far (those of the solids among them): f, W and count move to the enlarged list
      if (n_grown + n_bricks > kMaxItems) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct_filled: too many candidate bricks of the fill for one call");
      kb.reserve(n_grown + n_bricks);
      E3D_HIP(hipMemcpyAsync(kb.p, grown.p, sizeof(unsigned long long) * n_grown, hipMemcpyDeviceToDevice, s));
      E3D_HIP(hipMemcpyAsync(kb.p + n_grown, bricks.p, sizeof(unsigned long long) * n_bricks, hipMemcpyDeviceToDevice, s));
      const size_t n_all = run.sort_unique(kb, ka, next, n_grown + n_bricks, key_bits, scatter_keys);
      if (n_all * 64 > kMaxItems) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct_filled: too many candidate corners of the fill for one call");
      const size_t all_slots = n_all * 64;
      DevBuf<double> f2, w2, f_next;
      DevBuf<int> count2, nbr;
      DevBuf<unsigned char> state_next, holds, holds_next, x, x1;
      f2.reserve(all_slots); w2.reserve(all_slots); count2.reserve(all_slots); f_next.reserve(all_slots); nbr.reserve(6 * n_all);
      fill_state.reserve(all_slots); state_next.reserve(all_slots); x.reserve(all_slots); x1.reserve(all_slots); holds.reserve(n_all); holds_next.reserve(n_all);
      hipLaunchKernelGGL(k_surf_fill_relay, dim3((unsigned)n_all), dim3(64), 0, s, next.p, bricks.p, n_bricks, f.p, w.p, count.p, f2.p, w2.p, count2.p, fill_state.p, holds.p);
      hipLaunchKernelGGL(k_surf_fill_neighbours, blocks(6 * n_all), dim3(kSurfBlock), 0, s, next.p, n_all, nbr.p);
      // a brick that is not active in an iteration writes nothing: it holds no defined corner, in either copy
      E3D_HIP(hipMemsetAsync(state_next.p, 0, all_slots, s));
      E3D_HIP(hipMemsetAsync(x.p, 0, all_slots, s));
      E3D_HIP(hipMemsetAsync(x1.p, 0, all_slots, s));
      E3D_HIP(hipMemsetAsync(holds_next.p, 0, n_all, s));               // (f of an undefined corner is never read)
      std::swap(bricks, next); std::swap(f, f2); std::swap(w, w2); std::swap(count, count2);
      n_bricks = n_all; n_slots = all_slots;
      for (int t = 0; t < N; ++t) {
        hipLaunchKernelGGL(k_surf_fill_x, dim3((unsigned)n_bricks), dim3(64), 0, s, nbr.p, holds.p, fill_state.p, x.p);
        hipLaunchKernelGGL(k_surf_fill_x1, dim3((unsigned)n_bricks), dim3(64), 0, s, nbr.p, holds.p, fill_state.p, x.p, x1.p);
        hipLaunchKernelGGL(k_surf_fill_update, dim3((unsigned)n_bricks), dim3(64), 0, s, nbr.p, holds.p, fill_state.p, x1.p, f.p, state_next.p, f_next.p, holds_next.p);
        std::swap(fill_state, state_next); std::swap(f, f_next); std::swap(holds, holds_next);
      }
      defined.reserve(n_slots); defined_count.reserve(n_slots);
      hipLaunchKernelGGL(k_surf_fill_finish, blocks(n_slots), dim3(kSurfBlock), 0, s, fill_state.p, count.p, n_slots, defined.p, defined_count.p);
      E3D_HIP(hipStreamSynchronize(s));                                  // the buffers of this block are freed
    }
    fill_timer.stop(s);
    E3D_HIP(hipGetLastError());
  }

  // ---- solids: the operation list at every candidate corner ---------------------------------------------------------------------------
  defined.reserve(n_slots);
  if (n_ops) {
    solid_timer.start(s);
    hipLaunchKernelGGL(k_surf_apply_solids, blocks(n_slots), dim3(kSurfBlock), sizeof(double) * 16 * n_ops, s, bricks.p, n_slots, d_ops.p, (int)n_ops, P,
                       filled ? defined_count.p : count.p, f.p, defined.p);
    solid_timer.stop(s);
    E3D_HIP(hipGetLastError());
  }

  // ---- corners: the defined ones in (k, j, i) ------------------------------------------------------------------------------------------
  timer[3].start(s);
  if (!n_ops && !filled) hipLaunchKernelGGL(k_surf_corner_flags, blocks(n_slots), dim3(kSurfBlock), 0, s, count.p, n_slots, defined.p);
  const size_t n_corners = run.scan(defined.p, n_slots);
  if (3 * n_corners > kMaxItems) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: too many corners for one call");
  DevBuf<unsigned long long> ck;
  DevBuf<unsigned> cs;
  DevBuf<int> o_ijk, o_count;
  DevBuf<double> o_f, o_w;
  DevBuf<unsigned char> cross;
  const SurfField F{bricks.p, n_bricks, f.p, count.p, defined.p};
  if (n_corners) {
    ka.reserve(n_corners); ck.reserve(n_corners); va.reserve(n_corners); cs.reserve(n_corners);
    hipLaunchKernelGGL(k_surf_corner_keys, blocks(n_slots), dim3(kSurfBlock), 0, s, bricks.p, defined.p, run.offsets.p, n_slots, ka.p, va.p);
    sort_pairs_u64_u32(ka.p, ck.p, va.p, cs.p, n_corners, key_bits, run.temp, s);
    o_ijk.reserve(3 * n_corners); o_count.reserve(n_corners); o_f.reserve(n_corners); o_w.reserve(n_corners); cross.reserve(3 * n_corners);
    hipLaunchKernelGGL(k_surf_corner_out, blocks(n_corners), dim3(kSurfBlock), 0, s, ck.p, cs.p, n_corners, P, F, w.p, o_ijk.p, o_f.p, o_w.p, o_count.p,
                       cross.p);
  }
  timer[3].stop(s);
  out.corner_ijk.resize(3 * n_corners); out.corner_count.resize(n_corners); out.corner_f.resize(n_corners); out.corner_w.resize(n_corners);
  copy_out(out.corner_ijk.data(), o_ijk.p, sizeof(int32_t) * 3 * n_corners, s);
  copy_out(out.corner_count.data(), o_count.p, sizeof(int32_t) * n_corners, s);
  copy_out(out.corner_f.data(), o_f.p, sizeof(double) * n_corners, s);
  copy_out(out.corner_w.data(), o_w.p, sizeof(double) * n_corners, s);

  // ---- extract -------------------------------------------------------------------------------------------------------------------------
  timer[4].start(s);
  size_t n_edges = 0, n_cells = 0;
  DevBuf<unsigned> edges, tri;
  DevBuf<unsigned long long> cells;
  DevBuf<float> vertices;
  DevBuf<int> cell_ijk;
  if (n_corners) {
    std::swap(run.flags, cross);                                       // the crossing flags are what is scanned next
    n_edges = run.scan(3 * n_corners);
  }
  if (n_edges) {
    if (4 * n_edges > kMaxItems) throw Error(E3D_ERR_INVALID, "e3d_surface_reconstruct: too many crossing edges for one call");
    edges.reserve(n_edges); kb.reserve(4 * n_edges);
    hipLaunchKernelGGL(k_surf_edges, blocks(3 * n_corners), dim3(kSurfBlock), 0, s, ck.p, run.flags.p, run.offsets.p, 3 * n_corners, edges.p, kb.p);
    n_cells = run.sort_unique(kb, ka, cells, 4 * n_edges, key_bits, scatter_keys);
    vertices.reserve(3 * n_cells); cell_ijk.reserve(3 * n_cells); tri.reserve(6 * n_edges);
    hipLaunchKernelGGL(k_surf_vertices, blocks(n_cells), dim3(kSurfBlock), 0, s, cells.p, n_cells, P, F, vertices.p, cell_ijk.p);
    hipLaunchKernelGGL(k_surf_triangles, blocks(n_edges), dim3(kSurfBlock), 0, s, edges.p, n_edges, ck.p, cs.p, f.p, cells.p, n_cells, tri.p);
  }
  timer[4].stop(s);
  out.vertices.resize(3 * n_cells); out.cell_ijk.resize(3 * n_cells); out.triangles.resize(6 * n_edges);
  copy_out(out.vertices.data(), vertices.p, sizeof(float) * 3 * n_cells, s);
  copy_out(out.cell_ijk.data(), cell_ijk.p, sizeof(int32_t) * 3 * n_cells, s);
  copy_out(out.triangles.data(), tri.p, sizeof(uint32_t) * 6 * n_edges, s);
  // ---- fill: which corners and vertices it made ---------------------------------------------------------------------------------------
  out.corner_filled.assign(n_corners, 0); out.vertex_filled.assign(n_cells, 0);
  DevBuf<unsigned char> corner_filled, vertex_filled;
  if (filled) {
    fill_timer.start(s);
    corner_filled.reserve(n_corners); vertex_filled.reserve(n_cells);
    if (n_corners) hipLaunchKernelGGL(k_surf_fill_corner_flags, blocks(n_corners), dim3(kSurfBlock), 0, s, cs.p, n_corners, fill_state.p, corner_filled.p);
    if (n_cells) hipLaunchKernelGGL(k_surf_fill_vertex_flags, blocks(n_cells), dim3(kSurfBlock), 0, s, cells.p, n_cells, F, fill_state.p, vertex_filled.p);
    fill_timer.stop(s);
    copy_out(out.corner_filled.data(), corner_filled.p, n_corners, s);
    copy_out(out.vertex_filled.data(), vertex_filled.p, n_cells, s);
  }
  E3D_HIP(hipStreamSynchronize(s));
  E3D_HIP(hipGetLastError());
  for (int g = 0; g < kSurfGroups; ++g) out.ms[g] = timer[g].ms();
  int group = kSurfGroups;
  if (n_ops) out.ms[group++] = solid_timer.ms();
  if (N) out.ms[group++] = fill_timer.ms();
  static const bool trace = env_default_off("E3D_SURFACE_TRACE");
  if (trace)
    fprintf(stderr, "[surface] %zu points, %zu contribute, %zu voxels, %zu bricks (%zu candidate corners), %zu grid cells, %zu corners, %zu crossing edges, %zu vertices, %zu operations, %zu bricks of solids\n",
            n, m, n_voxels, n_bricks, n_slots, n_grid_cells, n_corners, n_edges, n_cells, n_ops, n_solid_keys);
}

}  // namespace

extern "C" {

e3d_surface_t* e3d_surface_reconstruct(const float* xyz, const float* normals, size_t n, float voxel_size, float support_radius) {
  e3d_surface* h = nullptr;
  E3D_TRY
  h = new e3d_surface;
  reconstruct(*h, xyz, normals, n, voxel_size, support_radius, 0, nullptr, 0);
  return h;
  E3D_CATCH_NEW(h)
}

e3d_surface_t* e3d_surface_reconstruct_csg(const float* xyz, const float* normals, size_t n, float voxel_size, float support_radius,
                                           const e3d_surface_solid_t* ops, size_t n_ops) {
  e3d_surface* h = nullptr;
  E3D_TRY
  h = new e3d_surface;
  reconstruct(*h, xyz, normals, n, voxel_size, support_radius, 0, ops, n_ops);
  return h;
  E3D_CATCH_NEW(h)
}

e3d_surface_t* e3d_surface_reconstruct_filled(const float* xyz, const float* normals, size_t n, float voxel_size, float support_radius, int fill_iterations,
                                              const e3d_surface_solid_t* ops, size_t n_ops) {
  e3d_surface* h = nullptr;
  E3D_TRY
  h = new e3d_surface;
  reconstruct(*h, xyz, normals, n, voxel_size, support_radius, fill_iterations, ops, n_ops);
  return h;
  E3D_CATCH_NEW(h)
}

void e3d_surface_destroy(e3d_surface_t* h) { delete h; }

int e3d_surface_counts(e3d_surface_t* h, int64_t* n_corners, int64_t* n_vertices, int64_t* n_triangles) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_surface_counts: null handle");
  if (n_corners) *n_corners = (int64_t)h->corner_count.size();
  if (n_vertices) *n_vertices = (int64_t)(h->vertices.size() / 3);
  if (n_triangles) *n_triangles = (int64_t)(h->triangles.size() / 3);
  return 0;
  E3D_CATCH()
}

int e3d_surface_get_corners(e3d_surface_t* h, int32_t* ijk, double* f, double* weight, int32_t* count) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_surface_get_corners: null handle");
  const size_t c = h->corner_count.size();
  if (ijk && c) memcpy(ijk, h->corner_ijk.data(), sizeof(int32_t) * 3 * c);
  if (f && c) memcpy(f, h->corner_f.data(), sizeof(double) * c);
  if (weight && c) memcpy(weight, h->corner_w.data(), sizeof(double) * c);
  if (count && c) memcpy(count, h->corner_count.data(), sizeof(int32_t) * c);
  return 0;
  E3D_CATCH()
}

int e3d_surface_get_mesh(e3d_surface_t* h, float* vertices, int32_t* cell_ijk, uint32_t* triangles) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_surface_get_mesh: null handle");
  if ((!vertices && !h->vertices.empty()) || (!triangles && !h->triangles.empty())) throw Error(E3D_ERR_INVALID, "e3d_surface_get_mesh: null argument");
  if (!h->vertices.empty()) memcpy(vertices, h->vertices.data(), sizeof(float) * h->vertices.size());
  if (cell_ijk && !h->cell_ijk.empty()) memcpy(cell_ijk, h->cell_ijk.data(), sizeof(int32_t) * h->cell_ijk.size());
  if (!h->triangles.empty()) memcpy(triangles, h->triangles.data(), sizeof(uint32_t) * h->triangles.size());
  return 0;
  E3D_CATCH()
}

int e3d_surface_get_fill(e3d_surface_t* h, uint8_t* corner_filled, uint8_t* vertex_filled) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_surface_get_fill: null handle");
  if (corner_filled && !h->corner_filled.empty()) memcpy(corner_filled, h->corner_filled.data(), h->corner_filled.size());
  if (vertex_filled && !h->vertex_filled.empty()) memcpy(vertex_filled, h->vertex_filled.data(), h->vertex_filled.size());
  return 0;
  E3D_CATCH()
}

int e3d_surface_kernel_ms(e3d_surface_t* h, float* ms, const char** names, int capacity) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_surface_kernel_ms: null handle");
  for (int g = 0; g < h->groups && g < capacity; ++g) {
    if (ms) ms[g] = h->ms[g];
    if (names) names[g] = h->names[g];
  }
  return h->groups;
  E3D_CATCH()
}

}  // extern "C"
