// e3d_icp_device.hpp -- device functions and types that more than one of the ICP kernel files needs (e3d_icp_kernels.hip,
// e3d_icp_certify.hip, e3d_icp_rows.hip, e3d_icp_lm.hip).  What a single file uses stays in that file.
#pragma once

#include "e3d_icp_kernels.hpp"

#pragma clang fp contract(off)

namespace e3d {

// ---- half cells: every grid cell is split into 2 x 2 x 2 sub-cells and its points are stored in sub-cell order (z, y, x).  A second
// dense directory over the sub-cells (8 entries per grid cell, same construction as the cell directory) lets the bounded search
// (k_nn_bounded_half) visit only the sub-cell rows its ball touches: a 2 - 3 mm ball in 10 mm cells of 62 points touches 2 - 3
// cells but only ~7 half cells of 8 points.  The half-cell coordinate is floor((v - origin) * (2 inv_cell)); scaling by 2 is
// exact in f32, so its upper bits ARE the cell coordinate (floor(2 t) >> 1 == floor(t)), and it is monotone in v like the cell
// coordinate -- the completeness argument of the cells carries over with a cell of half the size.
__device__ __forceinline__ unsigned half_code(float x, float y, float z, const GridDesc& g) {
  const float inv_h = 2.f * g.inv_cell;
  const unsigned fx = (unsigned)cell_coord(x, g.origin[0], inv_h) & 1u;
  const unsigned fy = (unsigned)cell_coord(y, g.origin[1], inv_h) & 1u;
  const unsigned fz = (unsigned)cell_coord(z, g.origin[2], inv_h) & 1u;
  return (fz * 2u + fy) * 2u + fx;
}

// block_dist (optional): distance, in cells, from the mapped query to the nearest face of the 3 x 3 x 3 cell block around its
// cell (1 .. 1.5): every target point outside the block is at least that far away in the target's local frame.
__device__ __forceinline__ unsigned long long query_cell_key(const float4 q, const InvMap& im, const GridDesc& g,
                                                             const QueryRange& qr, int& cx, int& cy, int& cz,
                                                             float* block_dist = nullptr) {
  const float dx = q.x - im.t[0], dy = q.y - im.t[1], dz = q.z - im.t[2];
  const float lx = im.Linv[0] * dx + im.Linv[1] * dy + im.Linv[2] * dz;
  const float ly = im.Linv[3] * dx + im.Linv[4] * dy + im.Linv[5] * dz;
  const float lz = im.Linv[6] * dx + im.Linv[7] * dy + im.Linv[8] * dz;
  cx = cell_coord(lx, g.origin[0], g.inv_cell);
  cy = cell_coord(ly, g.origin[1], g.inv_cell);
  cz = cell_coord(lz, g.origin[2], g.inv_cell);
  if (block_dist) {
    const float ux = (lx - g.origin[0]) * g.inv_cell - (float)cx, uy = (ly - g.origin[1]) * g.inv_cell - (float)cy,
                uz = (lz - g.origin[2]) * g.inv_cell - (float)cz;
    const float m = fminf(fminf(fminf(ux, 1.0f - ux), fminf(uy, 1.0f - uy)), fminf(uz, 1.0f - uz));
    *block_dist = 1.0f + fminf(fmaxf(m, 0.0f), 0.5f);
  }
  const unsigned kx = (unsigned)(cx - qr.lo[0]), ky = (unsigned)(cy - qr.lo[1]), kz = (unsigned)(cz - qr.lo[2]);
  if (kx >= qr.D[0] || ky >= qr.D[1] || kz >= qr.D[2]) return kEmptyKey;   // no target cell within reach
  return ((unsigned long long)kz * qr.D[1] + ky) * qr.D[0] + kx;
}

// accumulated motion bound of query q (MotionBound, e3d_icp_kernels.hpp): a * rho + b, rho = |q - cs| widened (up) or narrowed (lo)
// by the rounding of the global coordinates and of this evaluation
__device__ __forceinline__ float motion_rho(const float4 q, const MotionBound& m) {
  const float dx = q.x - m.cs[0], dy = q.y - m.cs[1], dz = q.z - m.cs[2];
  return sqrtf(dx * dx + (dy * dy + dz * dz));
}
__device__ __forceinline__ float motion_up(const float4 q, const MotionBound& m) {
  return (m.a * (motion_rho(q, m) * 1.000002f + m.rho_err) + m.b) * 1.000001f;
}
__device__ __forceinline__ float motion_lo(const float4 q, const MotionBound& m) {
  return (m.a * fmaxf(motion_rho(q, m) * 0.999998f - m.rho_err, 0.f) + m.b) * 0.999999f;
}

// ---- a BATCH of directed pairs per launch (round 5) ---------------------------------------------------------------------------
// (the k_*_multi kernels of e3d_icp_kernels.hip, e3d_icp_certify.hip and e3d_icp_rows.hip)
// An all-pairs job runs the certificate search of 240 directed pairs per outer iteration: with one launch per pair and kernel that is
// ~2000 launches of 0.04 - 0.1 ms each, a cost that does not shrink when the job is spread over more GPUs (a rank's slices get
// shorter, its launches do not get fewer).  The kernels below walk a table of pairs instead: a block finds its pair from the
// exclusive ends of the pairs' block ranges (at most kNnBatchPairs words, block-uniform: scalar loads and compares) and runs the
// one-pair body on that pair's pointers and constants -- the same code, so the same bits.
__device__ __forceinline__ int nn_find_range(const unsigned* __restrict__ ends, int n, unsigned b) {
  int lo = 0, hi = n - 1;                                   // first index with b < ends[index]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b < ends[mid]) hi = mid; else lo = mid + 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

typedef float row_v2f __attribute__((ext_vector_type(2)));

}  // namespace e3d
