// e3d_splats.hip -- SplatCreator (src/exe/splat_creator.cc:75-235): a device index over the triangles of a mesh, the exact
// point-to-mesh squared distance igl::AABB<MatrixXf,3>::squared_distance computes (thirdparty/igl/AABB.cpp:344-430), and the
// splat kernel.  DESIGN.md section 14.
//
// Index: triangles sorted by the 30-bit Morton code of their centroid (stable radix sort: ties keep the triangle id order),
// copied in that order as three float4 each ({a, id}, {b, 0}, {c, 0}), grouped kLeafTris to a leaf; an implicit complete
// binary tree in heap layout (node 1 the root, children 2i and 2i + 1, leaves P .. 2P - 1 for P = the power of two >= the
// leaf count) holds one box per node, computed level by level.  No cross-workgroup protocol, and the only atomics count: the
// index is a function of the input.  The traversal is stackless -- the next node is computed from the current one.
//
// Margin.  A node is pruned only when no triangle under it can produce a COMPUTED Ericson value at or below the bound.  The
// computed closest point q of the leaf function is a vertex, a point a + t e of an edge with t in [0, 1] (the edge regions
// divide a non-negative value by a larger one), or the face point (a + v ab) + w ac; for a triangle that is not nearly
// degenerate (sin^2 of its angle at a >= kRegularSin2, checked in f64 at the build) the face barycentrics leave [0, 1] only by
// rounding, so q lies within a few ulps of max|coordinate| of the triangle's box, and the computed |p - q|^2 is within 2^-22
// relative of the exact one.  The pruning test therefore uses, per axis, max(gap - delta, 0) with
// delta = 2^-16 * max(max|mesh coordinate|, max|query coordinate|) -- about 500 ulps of the largest coordinate -- and scales
// the sum of squares by (1 - 2^-20).  Triangles that are nearly degenerate or have a non-finite vertex carry no such
// bound (their face barycentrics can be anything): they are kept out of the tree in a list every query scans.  Triangles
// with two equal vertices are not in that list: their leaf function never reaches the face region.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "../../include/e3d_hip.h"
#include "e3d_grid.hpp"

namespace e3d {

constexpr int kLeafTris = 4;                       // triangles per leaf
constexpr int kSplatBlock = 256;
constexpr double kRegularSin2 = 1.0 / 65536.0;     // |ab x ac|^2 >= this * |ab|^2 |ac|^2: the triangle is in the tree
constexpr float kMarginScale = 1.0f / 65536.0f;    // delta = kMarginScale * max|coordinate|
constexpr float kBoundShrink = 1.0f - 1.0f / 1048576.0f;

struct MeshIndex {
  const float4* tri;     // 3 per triangle, tree triangles first (Morton order), then the scanned list (id order)
  const float4* lo;      // node boxes, heap order (index 0 unused)
  const float4* hi;
  unsigned n_tree;       // triangles in the tree
  unsigned n_tri;        // all triangles
  unsigned P;            // first leaf node (a power of two)
  float mag;             // max |coordinate| of the mesh's vertices
};

// ---- the leaf function: point_simplex_squared_distance (thirdparty/igl/point_simplex_squared_distance.cpp, Ericson ch. 5) ----
// f32 throughout, Eigen's 3-term order for dot products and squaredNorm (e0 + (e1 + e2)), evaluated on the original coordinates.
__device__ __forceinline__ float ericson_sq(float px, float py, float pz, float4 A, float4 B, float4 Cc) {
  const float ax = A.x, ay = A.y, az = A.z, bx = B.x, by = B.y, bz = B.z, cx = Cc.x, cy = Cc.y, cz = Cc.z;
  const float abx = bx - ax, aby = by - ay, abz = bz - az;
  const float acx = cx - ax, acy = cy - ay, acz = cz - az;
  float qx, qy, qz;
  do {
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float d1 = dot3e(abx, aby, abz, apx, apy, apz);
    const float d2 = dot3e(acx, acy, acz, apx, apy, apz);
    if (d1 <= 0.f && d2 <= 0.f) { qx = ax; qy = ay; qz = az; break; }
    const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float d3 = dot3e(abx, aby, abz, bpx, bpy, bpz);
    const float d4 = dot3e(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.f && d4 <= d3) { qx = bx; qy = by; qz = bz; break; }
    const float vc = d1 * d4 - d3 * d2;
    if ((ax != bx || ay != by || az != bz) && vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
      const float v = d1 / (d1 - d3);
      qx = ax + v * abx; qy = ay + v * aby; qz = az + v * abz;
      break;
    }
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const float d5 = dot3e(abx, aby, abz, cpx, cpy, cpz);
    const float d6 = dot3e(acx, acy, acz, cpx, cpy, cpz);
    if (d6 >= 0.f && d5 <= d6) { qx = cx; qy = cy; qz = cz; break; }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
      const float w = d2 / (d2 - d6);
      qx = ax + w * acx; qy = ay + w * acy; qz = az + w * acz;
      break;
    }
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) {
      const float w = e43 / (e43 + e56);
      qx = bx + w * (cx - bx); qy = by + w * (cy - by); qz = bz + w * (cz - bz);
      break;
    }
    // denom = 1.0 / (va + vb + vc) in f64 stored to f32: the correctly rounded f32 quotient (double rounding is innocuous
    // for division; -fhip-fp32-correctly-rounded-divide-sqrt)
    const float denom = 1.0f / ((va + vb) + vc);
    const float v = vb * denom, w = vc * denom;
    qx = (ax + abx * v) + acx * w; qy = (ay + aby * v) + acy * w; qz = (az + abz * v) + acz * w;
  } while (false);
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return dot3e(dx, dy, dz, dx, dy, dz);
}

// lower bound on every computed leaf value under a node (see the margin comment at the top)
__device__ __forceinline__ float node_lower_bound(const MeshIndex& X, unsigned node, float px, float py, float pz, float delta) {
  const float4 lo = X.lo[node], hi = X.hi[node];
  const float gx = fmaxf(fmaxf(lo.x - px, px - hi.x) - delta, 0.f);
  const float gy = fmaxf(fmaxf(lo.y - py, py - hi.y) - delta, 0.f);
  const float gz = fmaxf(fmaxf(lo.z - pz, pz - hi.z) - delta, 0.f);
  return ((gx * gx + gy * gy) + gz * gz) * kBoundShrink;      // an empty leaf (lo = +inf, hi = -inf) gives +inf
}

__device__ __forceinline__ float query_delta(const MeshIndex& X, float px, float py, float pz) {
  return kMarginScale * fmaxf(X.mag, fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz))));
}

// next node of the depth-first walk after `node` is done (pruned or a leaf): climb while it is a right child, then go to the
// right sibling; 0 = the walk is over
__device__ __forceinline__ unsigned next_node(unsigned node) {
  while (node & 1u) node >>= 1;
  return node ? node + 1u : 0u;
}

// Bounded minimum: the minimum over all triangles of the computed value if it is <= max_sq (ties: the lowest triangle id),
// else +inf and id -1.  The query must be finite.
__device__ float mesh_min_sq(const MeshIndex& X, float px, float py, float pz, float max_sq, int& best_id) {
  const float delta = query_delta(X, px, py, pz);
  float best = INFINITY;
  int bid = -1;
  auto consider = [&](unsigned t) {
    const float4 A = X.tri[3 * (size_t)t], B = X.tri[3 * (size_t)t + 1], Cc = X.tri[3 * (size_t)t + 2];
    const float v = ericson_sq(px, py, pz, A, B, Cc);
    const int id = (int)__float_as_uint(A.w);
    if (v < best || (v == best && id < bid)) { best = v; bid = id; }
  };
  unsigned node = 1;
  while (node) {
    if (node_lower_bound(X, node, px, py, pz, delta) > fminf(best, max_sq)) { node = next_node(node); continue; }
    if (node < X.P) { node <<= 1; continue; }
    const unsigned t0 = (node - X.P) * kLeafTris, t1 = min(t0 + kLeafTris, X.n_tree);
    for (unsigned t = t0; t < t1; ++t) consider(t);
    node = next_node(node);
  }
  for (unsigned t = X.n_tree; t < X.n_tri; ++t) consider(t);
  if (!(best <= max_sq)) { best = INFINITY; bid = -1; }
  best_id = bid;
  return best;
}

// Any-hit: is there a triangle whose computed value is <= thr2?  (min over triangles <= thr2 exactly when one is: NaN values
// never count, as they never win igl's `<`.)  The query must be finite.
__device__ bool mesh_any_within(const MeshIndex& X, float px, float py, float pz, float thr2) {
  const float delta = query_delta(X, px, py, pz);
  unsigned node = 1;
  while (node) {
    if (node_lower_bound(X, node, px, py, pz, delta) > thr2) { node = next_node(node); continue; }
    if (node < X.P) { node <<= 1; continue; }
    const unsigned t0 = (node - X.P) * kLeafTris, t1 = min(t0 + kLeafTris, X.n_tree);
    for (unsigned t = t0; t < t1; ++t)
      if (ericson_sq(px, py, pz, X.tri[3 * (size_t)t], X.tri[3 * (size_t)t + 1], X.tri[3 * (size_t)t + 2]) <= thr2) return true;
    node = next_node(node);
  }
  for (unsigned t = X.n_tree; t < X.n_tri; ++t)
    if (ericson_sq(px, py, pz, X.tri[3 * (size_t)t], X.tri[3 * (size_t)t + 1], X.tri[3 * (size_t)t + 2]) <= thr2) return true;
  return false;
}

// ---- index build ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned morton_spread10(unsigned v) {
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// key: bit 30 = "not in the tree" (non-finite vertex or nearly degenerate: counted in bad[1]), bits 0 - 29 the centroid's
// Morton code; an index outside the vertex array sets bad[0]
__global__ __launch_bounds__(256) void k_tri_keys(const float* __restrict__ V, size_t nv, const unsigned* __restrict__ T, size_t nt,
                                                  const float* __restrict__ bbox, unsigned* __restrict__ keys,
                                                  unsigned* __restrict__ ids, unsigned* __restrict__ bad) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  ids[t] = (unsigned)t;
  const unsigned i0 = T[3 * t], i1 = T[3 * t + 1], i2 = T[3 * t + 2];
  if (i0 >= nv || i1 >= nv || i2 >= nv) { atomicOr(bad, 1u); keys[t] = 1u << 30; atomicAdd(bad + 1, 1u); return; }
  const float ax = V[3 * (size_t)i0], ay = V[3 * (size_t)i0 + 1], az = V[3 * (size_t)i0 + 2];
  const float bx = V[3 * (size_t)i1], by = V[3 * (size_t)i1 + 1], bz = V[3 * (size_t)i1 + 2];
  const float cx = V[3 * (size_t)i2], cy = V[3 * (size_t)i2 + 1], cz = V[3 * (size_t)i2 + 2];
  const bool finite = isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz) &&
                      isfinite(cx) && isfinite(cy) && isfinite(cz);
  bool regular = finite;
  if (finite) {
    const bool ab_eq = ax == bx && ay == by && az == bz, ac_eq = ax == cx && ay == cy && az == cz, bc_eq = bx == cx && by == cy && bz == cz;
    if (!(ab_eq || ac_eq || bc_eq)) {
      const double ux = (double)bx - ax, uy = (double)by - ay, uz = (double)bz - az;
      const double wx = (double)cx - ax, wy = (double)cy - ay, wz = (double)cz - az;
      const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
      regular = (nx * nx + ny * ny + nz * nz) >= kRegularSin2 * (ux * ux + uy * uy + uz * uz) * (wx * wx + wy * wy + wz * wz);
    }
  }
  if (!regular) { keys[t] = 1u << 30; atomicAdd(bad + 1, 1u); return; }
  unsigned code = 0;
  const float c[3] = {(ax + bx + cx) / 3.f, (ay + by + cy) / 3.f, (az + bz + cz) / 3.f};
  for (int a = 0; a < 3; ++a) {
    const float ext = bbox[3 + a] - bbox[a];
    const float f = ext > 0.f ? (c[a] - bbox[a]) / ext : 0.f;
    const unsigned q = (unsigned)fminf(fmaxf(f * 1024.f, 0.f), 1023.f);
    code |= morton_spread10(q) << a;
  }
  keys[t] = code;
}

__global__ __launch_bounds__(256) void k_tri_gather(const float* __restrict__ V, const unsigned* __restrict__ T, const unsigned* __restrict__ order,
                                                    size_t nt, float4* __restrict__ tri) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  const unsigned t = order[i];
  for (int j = 0; j < 3; ++j) {
    const size_t v = T[3 * (size_t)t + j];
    tri[3 * i + j] = make_float4(V[3 * v], V[3 * v + 1], V[3 * v + 2], j == 0 ? __uint_as_float(t) : 0.f);
  }
}

__global__ __launch_bounds__(256) void k_leaf_boxes(const float4* __restrict__ tri, unsigned n_tree, unsigned P, float4* __restrict__ lo,
                                                    float4* __restrict__ hi) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= P) return;
  float4 l = make_float4(INFINITY, INFINITY, INFINITY, 0.f), h = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
  const unsigned t0 = j * kLeafTris, t1 = min(t0 + kLeafTris, n_tree);
  for (unsigned t = t0; t < t1; ++t)
    for (int v = 0; v < 3; ++v) {
      const float4 p = tri[3 * (size_t)t + v];
      l.x = fminf(l.x, p.x); l.y = fminf(l.y, p.y); l.z = fminf(l.z, p.z);
      h.x = fmaxf(h.x, p.x); h.y = fmaxf(h.y, p.y); h.z = fmaxf(h.z, p.z);
    }
  lo[P + j] = l; hi[P + j] = h;
}

// nodes [first, 2 first): the union of their children's boxes
__global__ __launch_bounds__(256) void k_node_boxes(unsigned first, float4* __restrict__ lo, float4* __restrict__ hi) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= first) return;
  const unsigned node = first + i;
  const float4 l0 = lo[2 * node], l1 = lo[2 * node + 1], h0 = hi[2 * node], h1 = hi[2 * node + 1];
  lo[node] = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.f);
  hi[node] = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.f);
}

struct MeshIndexBuffers {
  DevBuf<float> V, bbox_partial, bbox;
  DevBuf<unsigned> T, keys_a, keys_b, ids_a, ids_b, bad;
  DevBuf<char> temp;
  DevBuf<float4> tri, lo, hi;
  MeshIndex X{};
};

// Builds the index of a mesh (host or device arrays) on stream s.
static void build_mesh_index(MeshIndexBuffers& B, const float* vertices, size_t nv, const uint32_t* triangles, size_t nt, hipStream_t s) {
  if (nt >= ((size_t)1 << 31) / 3 || nv >= ((size_t)1 << 32)) throw Error(E3D_ERR_INVALID, "mesh index: too many triangles or vertices");
  B.V.reserve(3 * nv); B.T.reserve(3 * nt);
  copy_in(B.V.p, vertices, sizeof(float) * 3 * nv, s);
  copy_in(B.T.p, triangles, sizeof(unsigned) * 3 * nt, s);
  B.bbox_partial.reserve(6 * (size_t)kMaxBboxBlocks); B.bbox.reserve(6);
  float bb[6] = {0, 0, 0, 0, 0, 0};
  if (nv) {
    launch_bbox_aos(B.V.p, nv, B.bbox_partial.p, B.bbox.p, s);
    E3D_HIP(hipMemcpyAsync(bb, B.bbox.p, sizeof bb, hipMemcpyDeviceToHost, s));
  }
  B.keys_a.reserve(nt); B.keys_b.reserve(nt); B.ids_a.reserve(nt); B.ids_b.reserve(nt); B.bad.reserve(2);
  E3D_HIP(hipMemsetAsync(B.bad.p, 0, 2 * sizeof(unsigned), s));
  if (nt) {
    hipLaunchKernelGGL(k_tri_keys, dim3((unsigned)div_up(nt, 256)), dim3(256), 0, s, B.V.p, nv, B.T.p, nt, B.bbox.p, B.keys_a.p, B.ids_a.p, B.bad.p);
    sort_pairs_u32_u32(B.keys_a.p, B.keys_b.p, B.ids_a.p, B.ids_b.p, nt, 31, B.temp, s);
  }
  unsigned bad[2] = {0, 0};
  E3D_HIP(hipMemcpyAsync(bad, B.bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
  E3D_HIP(hipStreamSynchronize(s));
  if (bad[0]) throw Error(E3D_ERR_INVALID, "mesh index: a triangle references a vertex beyond n_vertices");
  const size_t n_tree = nt - bad[1];      // the tree's triangles sort first (keys below 2^30)
  const size_t n_leaves = div_up(n_tree, (size_t)kLeafTris);
  size_t P = 1;
  while (P < n_leaves) P <<= 1;
  B.tri.reserve(3 * nt + 1); B.lo.reserve(2 * P); B.hi.reserve(2 * P);
  if (nt) hipLaunchKernelGGL(k_tri_gather, dim3((unsigned)div_up(nt, 256)), dim3(256), 0, s, B.V.p, B.T.p, B.ids_b.p, nt, B.tri.p);
  hipLaunchKernelGGL(k_leaf_boxes, dim3((unsigned)div_up(P, 256)), dim3(256), 0, s, B.tri.p, (unsigned)n_tree, (unsigned)P, B.lo.p, B.hi.p);
  for (size_t first = P / 2; first >= 1; first /= 2)
    hipLaunchKernelGGL(k_node_boxes, dim3((unsigned)div_up(first, 256)), dim3(256), 0, s, (unsigned)first, B.lo.p, B.hi.p);
  E3D_HIP(hipGetLastError());
  float mag = 0.f;
  for (int a = 0; a < 6; ++a) if (std::isfinite(bb[a])) mag = std::max(mag, std::fabs(bb[a]));
  B.X = MeshIndex{B.tri.p, B.lo.p, B.hi.p, (unsigned)n_tree, (unsigned)nt, (unsigned)P, mag};
}

// ---- kernels over the queries -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSplatBlock) void k_mesh_min(MeshIndex X, const float* __restrict__ pts, size_t n, float max_sq,
                                                          float* __restrict__ out_d, int* __restrict__ out_id) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
  float d = INFINITY;
  int id = -1;
  // a non-finite query makes every leaf value NaN or +inf: none is below +inf
  if (isfinite(px) && isfinite(py) && isfinite(pz)) d = mesh_min_sq(X, px, py, pz, max_sq, id);
  out_d[i] = d;
  if (out_id) out_id[i] = id;
}

struct SplatFrame { float r, rx, ry, rz, ux, uy, uz; };

// Eigen 3.3 unitOrthogonal (3-vector selector) and n.cross(right) of splat_creator.cc:167-168; the normal is not renormalised
__device__ __forceinline__ SplatFrame splat_frame(float nx, float ny, float nz, float r) {
  SplatFrame f;
  f.r = r;
  const float prec = 1e-5f;
  if (!(fabsf(nx) <= fabsf(nz) * prec) || !(fabsf(ny) <= fabsf(nz) * prec)) {
    const float inv = 1.0f / sqrtf(nx * nx + ny * ny);
    f.rx = -ny * inv; f.ry = nx * inv; f.rz = 0.f;
  } else {
    const float inv = 1.0f / sqrtf(ny * ny + nz * nz);
    f.rx = 0.f; f.ry = -nz * inv; f.rz = ny * inv;
  }
  f.ux = ny * f.rz - nz * f.ry; f.uy = nz * f.rx - nx * f.rz; f.uz = nx * f.ry - ny * f.rx;
  return f;
}

// corner c (0 TR, 1 BR, 2 BL, 3 TL) of splat_creator.cc:170-178: p + r * (+-right +- up), per component
__device__ __forceinline__ void splat_corner(const SplatFrame& f, float px, float py, float pz, int c, float& ox, float& oy, float& oz) {
  float sx, sy, sz;
  if (c == 0) { sx = f.rx + f.ux; sy = f.ry + f.uy; sz = f.rz + f.uz; }
  else if (c == 1) { sx = f.rx - f.ux; sy = f.ry - f.uy; sz = f.rz - f.uz; }
  else if (c == 2) { sx = -f.rx - f.ux; sy = -f.ry - f.uy; sz = -f.rz - f.uz; }
  else { sx = -f.rx + f.ux; sy = -f.ry + f.uy; sz = -f.rz + f.uz; }
  ox = px + f.r * sx; oy = py + f.r * sy; oz = pz + f.r * sz;
}

// One lane per finite point, in the kNN pass's grid-cell order (neighbouring lanes walk the same nodes).  flag / radius are
// written at the point's input index; origin maps the compacted (finite) index to it (nullptr: identity).
__global__ __launch_bounds__(kSplatBlock) void k_splat_flags(MeshIndex X, const float4* __restrict__ order, const float* __restrict__ kth,
                                                             const unsigned* __restrict__ origin, size_t m, const float* __restrict__ normals,
                                                             float thr2, float max_splat, unsigned char* __restrict__ flag,
                                                             float* __restrict__ radius) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const float4 q = order[i];
  const unsigned j = __float_as_uint(q.w);
  const size_t o = origin ? (size_t)origin[j] : (size_t)j;
  const float nx = normals[3 * o], ny = normals[3 * o + 1], nz = normals[3 * o + 2];
  if (isnan(nx) || isnan(ny) || isnan(nz)) return;                  // :155-157 (flag 0, radius NaN from the fill)
  const float s = sqrtf(kth[j]);
  const float r = (max_splat < s) ? max_splat : s;                  // std::min(sqrtf(d2[4]), max_splat_size)
  const SplatFrame f = splat_frame(nx, ny, nz, r);
  // :182-198: centre, then TR, BR, BL, TL; a splat is added as soon as one is farther than the threshold.  thr2 = +inf or
  // NaN: `d > thr2` is never true, no splat.
  bool add = false;
  if (thr2 < INFINITY) {
    add = !mesh_any_within(X, q.x, q.y, q.z, thr2);
    for (int c = 0; c < 4 && !add; ++c) {
      float cx, cy, cz;
      splat_corner(f, q.x, q.y, q.z, c, cx, cy, cz);
      // a non-finite corner (a huge radius): every leaf value is NaN or +inf, none is <= thr2
      add = !(isfinite(cx) && isfinite(cy) && isfinite(cz)) || !mesh_any_within(X, cx, cy, cz, thr2);
    }
  }
  flag[o] = add ? 1 : 0;
  radius[o] = r;
}

__global__ __launch_bounds__(256) void k_fill_splat_outputs(size_t n, unsigned char* __restrict__ flag, float* __restrict__ radius) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = 0;
  radius[i] = __uint_as_float(0x7fc00000u);
}

// the corners of splat offset[i] (input order); splats beyond `capacity` are counted but not written
__global__ __launch_bounds__(256) void k_splat_write(const float* __restrict__ xyz, const float* __restrict__ normals, size_t n,
                                                     const unsigned char* __restrict__ flag, const float* __restrict__ radius,
                                                     const unsigned* __restrict__ offset, size_t capacity, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const size_t sidx = offset[i];
  if (sidx >= capacity) return;
  const SplatFrame f = splat_frame(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], radius[i]);
  for (int c = 0; c < 4; ++c) {
    float cx, cy, cz;
    splat_corner(f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], c, cx, cy, cz);
    out[12 * sidx + 3 * c] = cx; out[12 * sidx + 3 * c + 1] = cy; out[12 * sidx + 3 * c + 2] = cz;
  }
}

static void check_mesh_args(const char* what, const float* vertices, size_t nv, const uint32_t* triangles, size_t nt) {
  if ((!vertices && nv) || (!triangles && nt)) throw Error(E3D_ERR_INVALID, fmt("%s: null mesh argument", what));
}

}  // namespace e3d

using namespace e3d;

extern "C" int e3d_mesh_squared_distance(const float* points, size_t n, const float* vertices, size_t n_vertices,
                                         const uint32_t* triangles, size_t n_triangles, float max_sq_distance, float* sq_distance,
                                         int32_t* closest_triangle) {
  E3D_TRY
  if ((!points && n) || (!sq_distance && n)) throw Error(E3D_ERR_INVALID, "e3d_mesh_squared_distance: null argument");
  check_mesh_args("e3d_mesh_squared_distance", vertices, n_vertices, triangles, n_triangles);
  if (std::isnan(max_sq_distance)) throw Error(E3D_ERR_INVALID, "e3d_mesh_squared_distance: max_sq_distance is NaN");
  require_device();
  OwnedStream stream;
  hipStream_t s = stream.s;
  MeshIndexBuffers B;
  build_mesh_index(B, vertices, n_vertices, triangles, n_triangles, s);
  if (n == 0) return 0;
  DevBuf<float> P, D;
  DevBuf<int> I;
  P.reserve(3 * n); D.reserve(n);
  if (closest_triangle) I.reserve(n);
  copy_in(P.p, points, sizeof(float) * 3 * n, s);
  hipLaunchKernelGGL(k_mesh_min, dim3((unsigned)div_up(n, kSplatBlock)), dim3(kSplatBlock), 0, s, B.X, P.p, n, max_sq_distance, D.p,
                     closest_triangle ? I.p : nullptr);
  E3D_HIP(hipGetLastError());
  copy_out(sq_distance, D.p, sizeof(float) * n, s);
  if (closest_triangle) copy_out(closest_triangle, I.p, sizeof(int) * n, s);
  E3D_HIP(hipStreamSynchronize(s));
  return 0;
  E3D_CATCH()
}

extern "C" int64_t e3d_create_splats(const float* xyz, const float* normals, size_t n, const float* vertices, size_t n_vertices,
                                     const uint32_t* triangles, size_t n_triangles, float distance_threshold, float max_splat_size,
                                     float* splat_vertices, size_t capacity, uint8_t* add_splat, float* splat_radius,
                                     float* timings_ms) {
  E3D_TRY
  if ((!xyz && n) || (!normals && n)) throw Error(E3D_ERR_INVALID, "e3d_create_splats: null argument");
  if (!splat_vertices && capacity) throw Error(E3D_ERR_INVALID, "e3d_create_splats: capacity without splat_vertices");
  check_mesh_args("e3d_create_splats", vertices, n_vertices, triangles, n_triangles);
  if (n >= ((size_t)1 << 31)) throw Error(E3D_ERR_INVALID, "e3d_create_splats: more than 2^31-1 points");
  require_device();
  // the points on the host: non-finite ones are neither searched nor splatted (compacted out, as e3d_local_outlier_removal does)
  std::vector<float> hx(3 * n);
  if (n) E3D_HIP(hipMemcpy(hx.data(), xyz, sizeof(float) * 3 * n, hipMemcpyDefault));
  std::vector<float> finite;
  std::vector<unsigned> origin;
  bool all_finite = true;
  for (size_t i = 0; i < n && all_finite; ++i) all_finite = std::isfinite(hx[3 * i]) && std::isfinite(hx[3 * i + 1]) && std::isfinite(hx[3 * i + 2]);
  const float* pts = hx.data();
  size_t m = n;
  if (!all_finite) {
    for (size_t i = 0; i < n; ++i)
      if (std::isfinite(hx[3 * i]) && std::isfinite(hx[3 * i + 1]) && std::isfinite(hx[3 * i + 2])) {
        finite.insert(finite.end(), &hx[3 * i], &hx[3 * i] + 3);
        origin.push_back((unsigned)i);
      }
    pts = finite.data(); m = origin.size();
  }
  // the reference CHECKs that the k = 5 search returns 5 points (splat_creator.cc:161-163)
  if (m < 5) throw Error(E3D_ERR_INVALID, fmt("e3d_create_splats: %zu finite points, the splat radius needs at least 5", m));
  const float thr2 = distance_threshold * distance_threshold;
  int64_t count = 0;
  knn_kth_sqdist(pts, m, 5, [&](const float* kth, const float4* order, hipStream_t s) {
    EventTimer t_index, t_splat;
    t_index.start(s);
    MeshIndexBuffers B;
    build_mesh_index(B, vertices, n_vertices, triangles, n_triangles, s);
    t_index.stop(s);
    t_splat.start(s);
    DevBuf<float> X, N, R, out;
    DevBuf<unsigned char> F;
    DevBuf<unsigned> O, off;
    DevBuf<char> temp;
    X.reserve(3 * n); N.reserve(3 * n); R.reserve(n); F.reserve(n); off.reserve(n);
    copy_in(X.p, hx.data(), sizeof(float) * 3 * n, s);
    copy_in(N.p, normals, sizeof(float) * 3 * n, s);
    if (!all_finite) { O.reserve(m); copy_in(O.p, origin.data(), sizeof(unsigned) * m, s); }
    hipLaunchKernelGGL(k_fill_splat_outputs, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, n, F.p, R.p);
    hipLaunchKernelGGL(k_splat_flags, dim3((unsigned)div_up(m, kSplatBlock)), dim3(kSplatBlock), 0, s, B.X, order, kth,
                       all_finite ? nullptr : O.p, m, N.p, thr2, max_splat_size, F.p, R.p);
    E3D_HIP(hipGetLastError());
    count = (int64_t)compaction_offsets(F.p, n, off, temp, s);
    const size_t n_write = std::min((size_t)count, capacity);
    if (n_write) {
      out.reserve(12 * n_write);
      hipLaunchKernelGGL(k_splat_write, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, X.p, N.p, n, F.p, R.p, off.p, n_write, out.p);
      E3D_HIP(hipGetLastError());
      copy_out(splat_vertices, out.p, sizeof(float) * 12 * n_write, s);
    }
    t_splat.stop(s);
    if (add_splat) copy_out(add_splat, F.p, n, s);
    if (splat_radius) copy_out(splat_radius, R.p, sizeof(float) * n, s);
    E3D_HIP(hipStreamSynchronize(s));
    if (timings_ms) { timings_ms[0] = t_index.ms(); timings_ms[1] = t_splat.ms(); }
  });
  return count;
  E3D_CATCH()
}
