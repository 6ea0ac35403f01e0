// e3d_grid.hip -- the kernels every tool's grid build shares (gfx950 / CDNA4, wave64): transform + bounding box, cell keys,
// the permutation into cell order and the hash table of the occupied cells.  Not ICP: the host side of the build is
// build_cell_table / sort_into_cells of e3d_sort.hip, the declarations of both files are e3d_grid.hpp.
//
// Data layout in HBM (per cloud, all arrays in *grid-cell order* of the cloud's static local grid):
//   L4[n]  float4 {lx, ly, lz, bits(original index)}   local frame, written once
//   LN[n]  float4 {nx, ny, nz, 0}                      local normals, written once
//   G4[n]  float4 {gx, gy, gz, bits(original index)}   global frame, rewritten every outer iteration
//   table  HashEntry{key, start, end}                  cell -> [start,end) into the sorted arrays
//
// Reference loops covered: a3 (transform+bbox).
#include "e3d_grid.hpp"

#pragma clang fp contract(off)

namespace e3d {

// =================================================================================================
// a3: pcl::transformPointCloudWithNormals + AlignedBox::extend   (icp_point_to_plane.cc:189-205)
// =================================================================================================
// AoS variant (fixed clouds at AddPointCloud, and the stand-alone e3d_transform_cloud entry point).
__global__ __launch_bounds__(kBlock) void k_transform_aos(const float* __restrict__ xyz,
                                                          const float* __restrict__ nrm, size_t n, Affine T,
                                                          float* __restrict__ oxyz, float* __restrict__ onrm,
                                                          float* __restrict__ bbox_partial) {
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f};
  float mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const float3 p = pcl_se3(T, x, y, z);
    oxyz[3 * i] = p.x; oxyz[3 * i + 1] = p.y; oxyz[3 * i + 2] = p.z;
    if (nrm) {
      const float3 q = pcl_so3(T, nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
      onrm[3 * i] = q.x; onrm[3 * i + 1] = q.y; onrm[3 * i + 2] = q.z;
    }
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
  __shared__ float s[kBlock / kWave][6];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < 3; ++d) { mn[d] = wave_min(mn[d]); mx[d] = wave_max(mx[d]); }
  if (lane == 0) { for (int d = 0; d < 3; ++d) { s[w][d] = mn[d]; s[w][3 + d] = mx[d]; } }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = s[0][threadIdx.x];
    for (int k = 1; k < kBlock / kWave; ++k) v = (threadIdx.x < 3) ? fminf(v, s[k][threadIdx.x]) : fmaxf(v, s[k][threadIdx.x]);
    bbox_partial[6 * blockIdx.x + threadIdx.x] = v;
  }
}

// Sorted float4 variant used every outer iteration: L4 -> G4 (32 B/point of HBM traffic).
__global__ __launch_bounds__(kBlock) void k_transform_bbox(const float4* __restrict__ L4, size_t n, Affine T,
                                                           float4* __restrict__ G4,
                                                           float* __restrict__ bbox_partial) {
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f};
  float mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float4 l = ld_stream(L4 + i);
    const float3 p = pcl_se3(T, l.x, l.y, l.z);
    st_stream(G4 + i, make_float4(p.x, p.y, p.z, l.w));
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
  __shared__ float s[kBlock / kWave][6];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < 3; ++d) { mn[d] = wave_min(mn[d]); mx[d] = wave_max(mx[d]); }
  if (lane == 0) { for (int d = 0; d < 3; ++d) { s[w][d] = mn[d]; s[w][3 + d] = mx[d]; } }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = s[0][threadIdx.x];
    for (int k = 1; k < kBlock / kWave; ++k) v = (threadIdx.x < 3) ? fminf(v, s[k][threadIdx.x]) : fmaxf(v, s[k][threadIdx.x]);
    bbox_partial[6 * blockIdx.x + threadIdx.x] = v;
  }
}

// single block: reduce the per-block bbox partials to 6 floats
__global__ void k_bbox_final(const float* __restrict__ partial, int nblocks, float* __restrict__ out) {
  __shared__ float s[256][6];
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f};
  float mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
    for (int d = 0; d < 3; ++d) { mn[d] = fminf(mn[d], partial[6 * b + d]); mx[d] = fmaxf(mx[d], partial[6 * b + 3 + d]); }
  }
  for (int d = 0; d < 3; ++d) { s[threadIdx.x][d] = mn[d]; s[threadIdx.x][3 + d] = mx[d]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = s[0][threadIdx.x];
    for (int k = 1; k < (int)blockDim.x; ++k) v = (threadIdx.x < 3) ? fminf(v, s[k][threadIdx.x]) : fmaxf(v, s[k][threadIdx.x]);
    out[threadIdx.x] = v;
  }
}

// bbox only (local frame, for the grid origin)
__global__ __launch_bounds__(kBlock) void k_bbox_aos(const float* __restrict__ xyz, size_t n,
                                                     float* __restrict__ bbox_partial) {
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f};
  float mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
    mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
  }
  __shared__ float s[kBlock / kWave][6];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < 3; ++d) { mn[d] = wave_min(mn[d]); mx[d] = wave_max(mx[d]); }
  if (lane == 0) { for (int d = 0; d < 3; ++d) { s[w][d] = mn[d]; s[w][3 + d] = mx[d]; } }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = s[0][threadIdx.x];
    for (int k = 1; k < kBlock / kWave; ++k) v = (threadIdx.x < 3) ? fminf(v, s[k][threadIdx.x]) : fmaxf(v, s[k][threadIdx.x]);
    bbox_partial[6 * blockIdx.x + threadIdx.x] = v;
  }
}

// =================================================================================================
// Static grid build (replaces the per-pair FLANN kd-tree build of icp_point_to_plane.cc:46-51)
// =================================================================================================
__global__ __launch_bounds__(kBlock) void k_cell_keys(const float* __restrict__ xyz, size_t n, GridDesc g,
                                                      unsigned long long* __restrict__ keys,
                                                      unsigned* __restrict__ vals) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int cx = cell_coord(xyz[3 * i], g.origin[0], g.inv_cell);
  const int cy = cell_coord(xyz[3 * i + 1], g.origin[1], g.inv_cell);
  const int cz = cell_coord(xyz[3 * i + 2], g.origin[2], g.inv_cell);
  keys[i] = cell_key(cx, cy, cz);
  vals[i] = (unsigned)i;
}

__global__ __launch_bounds__(kBlock) void k_permute(const float* __restrict__ xyz, const float* __restrict__ nrm,
                                                    const unsigned* __restrict__ order, size_t n,
                                                    float4* __restrict__ L4, float4* __restrict__ LN) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned i = order[j];
  L4[j] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float(i));
  if (nrm) LN[j] = make_float4(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2], 0.f);
}

__global__ __launch_bounds__(kBlock) void k_count_cells(const unsigned long long* __restrict__ keys, size_t n,
                                                        unsigned* __restrict__ counter) {
  unsigned c = 0;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x)
    c += (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  __shared__ unsigned sc[kBlock / kWave];
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(counter, sc[0] + sc[1] + sc[2] + sc[3]);
}

__device__ __forceinline__ unsigned table_find_or_insert(HashEntry* table, unsigned mask, unsigned long long key) {
  unsigned h = hash_key(key) & mask;
  for (;;) {
    const unsigned long long prev = atomicCAS(&table[h].key, kEmptyKey, key);
    if (prev == kEmptyKey || prev == key) return h;
    h = (h + 1) & mask;
  }
}

__global__ __launch_bounds__(kBlock) void k_build_table(const unsigned long long* __restrict__ keys, size_t n,
                                                        HashEntry* __restrict__ table, unsigned mask) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long k = keys[j];
  const bool is_start = (j == 0) || (keys[j - 1] != k);
  const bool is_end = (j + 1 == n) || (keys[j + 1] != k);
  if (is_start || is_end) {
    const unsigned h = table_find_or_insert(table, mask, k);
    if (is_start) table[h].start = (unsigned)j;
    if (is_end) table[h].end = (unsigned)(j + 1);
  }
}

// =================================================================================================
// host-side launch helpers
// =================================================================================================
static inline int grid_for(size_t n, int cap = 4096) {
  size_t b = (n + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  if (b > (size_t)cap) b = (size_t)cap;
  return (int)b;
}

int launch_transform_aos(const float* xyz, const float* nrm, size_t n, const Affine& T, float* oxyz, float* onrm,
                         float* bbox_partial, float* bbox_out, hipStream_t s) {
  const int nb = grid_for(n, kMaxBboxBlocks);
  hipLaunchKernelGGL(k_transform_aos, dim3(nb), dim3(kBlock), 0, s, xyz, nrm, n, T, oxyz, onrm, bbox_partial);
  hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(256), 0, s, bbox_partial, nb, bbox_out);
  return nb;
}

int launch_transform_bbox(const float4* L4, size_t n, const Affine& T, float4* G4, float* bbox_partial,
                          float* bbox_out, hipStream_t s) {
  const int nb = grid_for(n, kMaxBboxBlocks);
  hipLaunchKernelGGL(k_transform_bbox, dim3(nb), dim3(kBlock), 0, s, L4, n, T, G4, bbox_partial);
  hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(256), 0, s, bbox_partial, nb, bbox_out);
  return nb;
}

void launch_bbox_aos(const float* xyz, size_t n, float* bbox_partial, float* bbox_out, hipStream_t s) {
  const int nb = grid_for(n, kMaxBboxBlocks);
  hipLaunchKernelGGL(k_bbox_aos, dim3(nb), dim3(kBlock), 0, s, xyz, n, bbox_partial);
  hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(256), 0, s, bbox_partial, nb, bbox_out);
}

void launch_cell_keys(const float* xyz, size_t n, const GridDesc& g, unsigned long long* keys, unsigned* vals,
                      hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_cell_keys, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, xyz, n, g, keys, vals);
}

void launch_permute(const float* xyz, const float* nrm, const unsigned* order, size_t n, float4* L4, float4* LN,
                    hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_permute, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, xyz, nrm, order, n, L4, LN);
}

void launch_count_cells(const unsigned long long* keys, size_t n, unsigned* counter, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_count_cells, dim3(grid_for(n, 2048)), dim3(kBlock), 0, s, keys, n, counter);
}

void launch_build_table(const unsigned long long* keys, size_t n, HashEntry* table, unsigned mask, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_build_table, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, keys, n, table, mask);
}

}  // namespace e3d
