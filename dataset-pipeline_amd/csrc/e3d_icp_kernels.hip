// e3d_icp_kernels.hip -- ICP, the first search of a directed pair and everything built on its bodies (gfx950 / CDNA4, wave64): a
// target's half-cell and dense directories, the four generations of the 1-NN search (k_nn_query, k_nn_cells, k_nn_rows, k_nn_mfma),
// the query key kernels with the occupancy pruning, and the batch kernels that run those bodies (k_query_keys_multi,
// k_nn_rows_multi).  The certificates and the bounded search are e3d_icp_certify.hip, the grid build e3d_grid.hip, the
// correspondence rows e3d_icp_rows.hip, the LM passes e3d_icp_lm.hip.
//
// Reference loops covered: a5 (1-NN within radius).
#include <cstdlib>

#include "e3d_icp_device.hpp"

#pragma clang fp contract(off)

namespace e3d {

// first sort pass of the build: 3-bit sub-cell code per point (the stable sort by cell key that follows keeps this order
// inside every cell)
__global__ __launch_bounds__(kBlock) void k_half_keys(const float* __restrict__ xyz, size_t n, GridDesc g, unsigned* __restrict__ keys,
                                                      unsigned* __restrict__ vals) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = half_code(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g);
  vals[i] = (unsigned)i;
}
// cell keys of the points in a given order (second, stable sort pass)
__global__ __launch_bounds__(kBlock) void k_cell_keys_ordered(const float* __restrict__ xyz, const unsigned* __restrict__ order, size_t n,
                                                              GridDesc g, unsigned long long* __restrict__ keys) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const size_t i = order[j];
  keys[j] = cell_key(cell_coord(xyz[3 * i], g.origin[0], g.inv_cell), cell_coord(xyz[3 * i + 1], g.origin[1], g.inv_cell),
                     cell_coord(xyz[3 * i + 2], g.origin[2], g.inv_cell));
}
// The half-cell directory: 8 bytes per grid cell, byte k = number of the cell's points with sub-cell code <= k (an inclusive
// prefix: sub-cell k is the run [S[cell] + byte(k - 1), S[cell] + byte(k))).  Cells with more than 255 points hold 0xFF in every
// byte and are scanned whole.  Two steps: the last point of every (cell, code) run writes its end offset; the first point of every
// cell then turns the 8 bytes into a running maximum (empty sub-cells wrote nothing) and marks the overflow.
__global__ __launch_bounds__(kBlock) void k_half_ends(const unsigned long long* __restrict__ keys, const float4* __restrict__ L4, size_t n,
                                                      GridDesc g, QueryRange qr, const unsigned* __restrict__ S,
                                                      unsigned char* __restrict__ H8) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long k = keys[j];
  const float4 p = L4[j];
  const unsigned code = half_code(p.x, p.y, p.z, g);
  if (j + 1 < n && keys[j + 1] == k) {
    const float4 pn = L4[j + 1];
    if (half_code(pn.x, pn.y, pn.z, g) == code) return;       // only the last point of a run writes
  }
  const int cx = (int)(k & 0x1FFFFFull), cy = (int)((k >> 21) & 0x1FFFFFull), cz = (int)((k >> 42) & 0x1FFFFFull);
  const size_t lin = ((size_t)(unsigned)(cz - qr.lo[2]) * qr.D[1] + (unsigned)(cy - qr.lo[1])) * qr.D[0] + (unsigned)(cx - qr.lo[0]);
  const unsigned end_rel = (unsigned)(j + 1) - S[lin];
  H8[8 * lin + code] = (unsigned char)min(end_rel, 255u);
}
__global__ __launch_bounds__(kBlock) void k_half_fix(const unsigned long long* __restrict__ keys, size_t n, QueryRange qr,
                                                     const unsigned* __restrict__ S, unsigned long long* __restrict__ H8) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long k = keys[j];
  if (j > 0 && keys[j - 1] == k) return;                      // the first point of every cell
  const int cx = (int)(k & 0x1FFFFFull), cy = (int)((k >> 21) & 0x1FFFFFull), cz = (int)((k >> 42) & 0x1FFFFFull);
  const size_t lin = ((size_t)(unsigned)(cz - qr.lo[2]) * qr.D[1] + (unsigned)(cy - qr.lo[1])) * qr.D[0] + (unsigned)(cx - qr.lo[0]);
  if (S[lin + 1] - S[lin] > 255u) { H8[lin] = ~0ull; return; }
  unsigned long long w = H8[lin], out = 0ull;
  unsigned run = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    run = max(run, (unsigned)((w >> (8 * b)) & 0xFFull));
    out |= (unsigned long long)run << (8 * b);
  }
  H8[lin] = out;
}

// dense cell-start directory: ends[lin(cell)] = end index of the cell's run in the sorted arrays (written by the
// last point of each run, 0 elsewhere); an exclusive MAX scan turns it into starts, with
// starts[lin + 1] = max(starts[lin], ends[lin]) = end of the cell's run (or its start if the cell is empty).
__global__ __launch_bounds__(kBlock) void k_dense_counts(const unsigned long long* __restrict__ keys, size_t n,
                                                         QueryRange qr, unsigned* __restrict__ ends) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long k = keys[j];
  if (j + 1 < n && keys[j + 1] == k) return;          // only the last point of a run writes
  const int cx = (int)(k & 0x1FFFFFull), cy = (int)((k >> 21) & 0x1FFFFFull), cz = (int)((k >> 42) & 0x1FFFFFull);
  const size_t lin = ((size_t)(unsigned)(cz - qr.lo[2]) * qr.D[1] + (unsigned)(cy - qr.lo[1])) * qr.D[0] +
                     (unsigned)(cx - qr.lo[0]);
  ends[lin] = (unsigned)(j + 1);
}

// =================================================================================================
// a5: FindCorrespondencesFast (icp_point_to_plane.cc:42-105): exact nearest target point with
//     f32 squared distance < r2, lowest original target index on ties.
// One thread per source point (in the source cloud's cell order, so that a wave's 64 queries share
// their 27-cell neighbourhoods and the candidate reads are L1/L2 broadcast hits).
// =================================================================================================
__global__ __launch_bounds__(kBlock) void k_nn_query(const float4* __restrict__ Gsrc, size_t n_src,
                                                     const float4* __restrict__ Gtgt,
                                                     const HashEntry* __restrict__ table, GridDesc g, InvMap im,
                                                     float r2, int* __restrict__ match_pos,
                                                     float* __restrict__ match_d2) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_src) return;
  const float4 q = Gsrc[j];
  // query in the target's local frame (approximate; only selects candidate cells)
  const float dx = q.x - im.t[0], dy = q.y - im.t[1], dz = q.z - im.t[2];
  const float lx = im.Linv[0] * dx + im.Linv[1] * dy + im.Linv[2] * dz;
  const float ly = im.Linv[3] * dx + im.Linv[4] * dy + im.Linv[5] * dz;
  const float lz = im.Linv[6] * dx + im.Linv[7] * dy + im.Linv[8] * dz;
  const int cx = cell_coord(lx, g.origin[0], g.inv_cell);
  const int cy = cell_coord(ly, g.origin[1], g.inv_cell);
  const int cz = cell_coord(lz, g.origin[2], g.inv_cell);

  float best_d2 = r2;        // strict: a candidate at exactly r2 can never win (best_oi == 0)
  unsigned best_oi = 0u;
  int best_pos = -1;
  constexpr int kMaxC = (1 << 21) - 1;
  // reject early when the whole neighbourhood is outside the key range (NaN coordinates land here too)
  if (!(cx >= -1 && cy >= -1 && cz >= -1 && cx <= kMaxC + 1 && cy <= kMaxC + 1 && cz <= kMaxC + 1)) {
    match_pos[j] = -1; match_d2[j] = 0.f;
    return;
  }
  for (int oz = -1; oz <= 1; ++oz) {
    const int z = cz + oz;
    if (z < 0 || z > kMaxC) continue;
    for (int oy = -1; oy <= 1; ++oy) {
      const int y = cy + oy;
      if (y < 0 || y > kMaxC) continue;
      for (int ox = -1; ox <= 1; ++ox) {
        const int x = cx + ox;
        if (x < 0 || x > kMaxC) continue;
        const unsigned long long key = cell_key(x, y, z);
        unsigned h = hash_key(key) & g.mask;
        unsigned s = 0, e = 0;
        for (;;) {
          const HashEntry en = table[h];
          if (en.key == key) { s = en.start; e = en.end; break; }
          if (en.key == kEmptyKey) break;
          h = (h + 1) & g.mask;
        }
        for (unsigned m = s; m < e; ++m) {
          const float4 c = Gtgt[m];
          const float d2 = sqdist_l2(q.x, q.y, q.z, c.x, c.y, c.z);
          const unsigned oi = __float_as_uint(c.w);
          if (d2 < best_d2 || (d2 == best_d2 && oi < best_oi)) { best_d2 = d2; best_oi = oi; best_pos = (int)m; }
        }
      }
    }
  }
  match_pos[j] = best_pos;
  match_d2[j] = best_d2;
}

// -------------------------------------------------------------------------------------------------
// Dense-data path of a5: queries are radix-sorted by the TARGET grid cell they fall into, then one
// wave handles 64 consecutive sorted queries.  For every distinct cell in its chunk the wave stages the
// cell's 27-neighbourhood (contiguous runs of the target's cell-ordered G4 array, found with 27 parallel
// hash lookups) in LDS with coalesced loads, and the lanes -- arranged as (queries of that cell) x
// (candidate slices) -- scan the bucket with broadcast LDS reads.  Same arithmetic, same (d2, index)
// ordering and strict radius test as k_nn_query, so both kernels return identical results.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_query_keys(const float4* __restrict__ Gsrc, size_t n, GridDesc g, InvMap im,
                                                       QueryRange qr, unsigned long long* __restrict__ keys,
                                                       unsigned* __restrict__ vals) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int cx, cy, cz;
  keys[j] = query_cell_key(Gsrc[j], im, g, qr, cx, cy, cz);
  vals[j] = (unsigned)j;
}

// 32-bit variant of the sort keys (grids with fewer than 2^32 - 1 cells in the query range): 8 instead of 12
// bytes per (key, index) pair through every radix pass.
__global__ __launch_bounds__(kBlock) void k_query_keys32(const float4* __restrict__ Gsrc, size_t n, GridDesc g, InvMap im,
                                                         QueryRange qr, unsigned* __restrict__ keys,
                                                         unsigned* __restrict__ vals) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int cx, cy, cz;
  const unsigned long long k = query_cell_key(Gsrc[j], im, g, qr, cx, cy, cz);
  keys[j] = (k == kEmptyKey) ? 0xFFFFFFFFu : (unsigned)k;
  vals[j] = (unsigned)j;
}

// the same keys for a LIST of queries (the ones the certificates did not settle): vals = their source positions
__global__ __launch_bounds__(kBlock) void k_query_keys_list(const float4* __restrict__ Gsrc, const unsigned* __restrict__ list, size_t n,
                                                            GridDesc g, InvMap im, QueryRange qr, unsigned long long* __restrict__ keys,
                                                            unsigned* __restrict__ vals) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned jf = list[i], j = jf & kListIndexMask;            // (a far-list entry may carry kListNoPartner: it travels with the value)
  int cx, cy, cz;
  keys[i] = query_cell_key(Gsrc[j], im, g, qr, cx, cy, cz);
  vals[i] = jf;
}
__global__ __launch_bounds__(kBlock) void k_query_keys32_list(const float4* __restrict__ Gsrc, const unsigned* __restrict__ list, size_t n,
                                                              GridDesc g, InvMap im, QueryRange qr, unsigned* __restrict__ keys,
                                                              unsigned* __restrict__ vals) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned jf = list[i], j = jf & kListIndexMask;
  int cx, cy, cz;
  const unsigned long long k = query_cell_key(Gsrc[j], im, g, qr, cx, cy, cz);
  keys[i] = (k == kEmptyKey) ? 0xFFFFFFFFu : (unsigned)k;
  vals[i] = jf;
}

// -------------------------------------------------------------------------------------------------
// Occupancy of the 27-cell blocks (round 5).  While two scans are still centimetres apart most queries have no target point anywhere
// in the 27 cells around them; k_nn_rows keyed, sorted and visited them all the same, read the nine directory rows of their block
// and left with "no partner" (9 of the 9.4 ms of such an outer iteration at 2 x 50 M points).  One bit per cell of the dense
// directory's range says whether ANY of the 27 cells around it holds a point (k_occ_cells: the occupied cells, 64 cells per wave and
// ballot; k_occ_dilate: the OR over the 3 x 3 x 3 neighbourhood, rows padded to whole 32-bit words): 1e9 cells are 125 MB, built
// once per grid.  k_query_keys_prune tests it with ONE load per query.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_occ_cells(const unsigned* __restrict__ S, QueryRange qr, unsigned stride_w, unsigned* __restrict__ occ) {
  // one wave per 64 consecutive (padded) cells of a row
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per_row = (size_t)stride_w * 32u;
  const size_t row = t / per_row;
  if (row >= (size_t)qr.D[1] * qr.D[2]) return;                 // (per_row is a multiple of 64 or of 32: see the launch)
  const unsigned x = (unsigned)(t % per_row);
  bool on = false;
  if (x < qr.D[0]) { const size_t lin = row * qr.D[0] + x; on = S[lin + 1] > S[lin]; }
  const unsigned long long b = __ballot(on);
  const int lane = threadIdx.x & 63;
  const size_t w0 = row * stride_w + (x >> 5);
  if (lane == 0) occ[w0] = (unsigned)b;
  if (lane == 32) occ[w0] = (unsigned)(b >> 32);
}
__global__ __launch_bounds__(kBlock) void k_occ_dilate(const unsigned* __restrict__ in, unsigned D1, unsigned D2, unsigned stride_w, unsigned* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t row = t / stride_w;
  if (row >= (size_t)D1 * D2) return;
  const unsigned xw = (unsigned)(t % stride_w);
  const int y = (int)(row % D1), z = (int)(row / D1);
  unsigned acc = 0u;
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = y + dy, zz = z + dz;
      if (yy < 0 || zz < 0 || yy >= (int)D1 || zz >= (int)D2) continue;
      const unsigned* r = in + ((size_t)zz * D1 + (size_t)yy) * stride_w;
      const unsigned w = r[xw], lo = xw > 0u ? r[xw - 1] : 0u, hi = xw + 1u < stride_w ? r[xw + 1] : 0u;
      acc |= w | (w << 1) | (w >> 1) | (lo >> 31) | (hi << 31);
    }
  out[t] = acc;
}

// Keys of the queries k_nn_rows has to look at, COMPACTED: a query whose block is empty (its cell's bit in `occ` is clear, or its
// cell lies outside the directory's range) is settled here as k_nn_rows settles a query without candidates -- no partner, d2 = r2,
// the certificate of the block's faces -- and only the others are keyed for the sort.  The RESULTS (partner, distance) are those of
// k_nn_rows; the certificate STATE need not be: k_nn_rows scores a query against every candidate of its segment's span, so its
// bound can be min(sqrt(b2), faces) with a finite b2 where this kernel writes the faces' bound -- either is a valid lower bound.
// list == nullptr: all n queries.  A block takes kPruneBlock queries, kPrunePerThread per thread, and reserves its stretch of the
// output with ONE atomic (a first version with an atomic per wave on the one counter took 15 ms for 1.5 M of them).  The order of
// the kept pairs depends on the order in which blocks reach the counter; the radix sort orders them by key and k_nn_rows treats
// every query on its own, so results do not.  count[0] = number of pairs written.
constexpr int kPrunePerThread = 8, kPruneBlock = kBlock * kPrunePerThread;
static_assert((unsigned)kPruneBlock == kQueryKeysBlock, "queries per block of the key kernels");
// prune == false (a pair whose far list has stopped being mostly empty blocks, sort_query_keys_pruned): every listed query is keyed,
// none is settled -- what k_query_keys32_list does.  key_or / key_mask: the batch's key kernel puts the pair's index above the cell
// key (one sort for the far lists of a whole batch of pairs); count2: that pair's own counter.
template <typename KeyT>
__device__ __forceinline__ void query_keys_prune_body(const unsigned bx, const float4* __restrict__ Gsrc, const unsigned* __restrict__ list, size_t n,
                                                      const unsigned* __restrict__ occ, unsigned stride_w, const GridDesc& g, const InvMap& im,
                                                      const QueryRange& qr, float r2, const CertParams& cert, KeyT* __restrict__ keys,
                                                      unsigned* __restrict__ vals, unsigned* __restrict__ count, unsigned* __restrict__ count2,
                                                      const KeyT key_mask, const KeyT key_or, const bool prune,
                                                      int* __restrict__ match, int* __restrict__ match2,
                                                      float* __restrict__ match_d2, float* __restrict__ lbe, int from_state) {
  __shared__ unsigned s_cnt[kBlock / kWave][kPrunePerThread];
  __shared__ unsigned s_base;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t i0 = (size_t)bx * kPruneBlock + (size_t)w * kWave + (size_t)lane;      // step u: + u * kBlock
  KeyT kk[kPrunePerThread];
  unsigned vv[kPrunePerThread];
  unsigned long long keep_mask[kPrunePerThread];       // wave-uniform ballots
  unsigned jf[kPrunePerThread];
  float4 qq[kPrunePerThread];
#pragma unroll
  for (int u = 0; u < kPrunePerThread; ++u) {
    const size_t i = i0 + (size_t)u * kBlock;
    // from_state (all queries of a pair whose certificates were not tested this time, see certify_now in e3d_icp.hip): the flag
    // k_nn_certify would have set comes from the state itself, and so does the r2 it would have stored
    jf[u] = (i < n) ? (list ? list[i] : ((unsigned)i | ((from_state && match[i] < 0) ? kListNoPartner : 0u))) : 0u;
  }
#pragma unroll
  for (int u = 0; u < kPrunePerThread; ++u) qq[u] = Gsrc[jf[u] & kListIndexMask];
  unsigned wordv[kPrunePerThread];
  int bitv[kPrunePerThread];
  float bdist[kPrunePerThread];
#pragma unroll
  for (int u = 0; u < kPrunePerThread; ++u) {
    int cx = 0, cy = 0, cz = 0;
    bdist[u] = 2.0f;
    const unsigned long long key = query_cell_key(qq[u], im, g, qr, cx, cy, cz, &bdist[u]);
    kk[u] = ((KeyT)key & key_mask) | key_or;
    wordv[u] = 0u; bitv[u] = -1;
    if (prune && key != kEmptyKey) {
      const int kx = cx - qr.lo[0], ky = cy - qr.lo[1], kz = cz - qr.lo[2];
      wordv[u] = occ[((size_t)kz * qr.D[1] + (size_t)ky) * stride_w + (size_t)(kx >> 5)];
      bitv[u] = kx & 31;
    } else {
      bdist[u] = 2.0f;                                   // outside the directory range: two empty cells all around (k_nn_rows)
    }
  }
#pragma unroll
  for (int u = 0; u < kPrunePerThread; ++u) {
    const size_t i = i0 + (size_t)u * kBlock;
    const bool valid = i < n;
    const bool keep = valid && (!prune || (bitv[u] >= 0 && ((wordv[u] >> bitv[u]) & 1u)));
    const unsigned j = jf[u] & kListIndexMask;
    vv[u] = jf[u];
    if (valid && from_state && (jf[u] & kListNoPartner)) match_d2[j] = r2;
    if (valid && !keep) {
      if (!(jf[u] & kListNoPartner)) {                   // (see k_nn_rows: a query that had no partner holds these values already)
        match[j] = -1; match_d2[j] = r2;
        if (match2) match2[j] = -1;
      }
      const float kInf = __uint_as_float(0x7f800000u);
      const float lb_out = bdist[u] * cert.cell_scale - cert.cell_sub;
      lbe[j] = fmaxf(fminf(sqrtf(kInf), lb_out), 0.0f) * 0.999999f + motion_lo(qq[u], cert.lo);
    }
    keep_mask[u] = __ballot(keep);
    if (lane == 0) s_cnt[w][u] = (unsigned)__popcll(keep_mask[u]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tot = 0u;
    for (int ww = 0; ww < kBlock / kWave; ++ww)
      for (int u = 0; u < kPrunePerThread; ++u) tot += s_cnt[ww][u];
    s_base = tot ? atomicAdd(count, tot) : 0u;
    if (count2 && tot) atomicAdd(count2, tot);
  }
  __syncthreads();
  unsigned off = s_base;
  for (int ww = 0; ww < w; ++ww)
#pragma unroll
    for (int u = 0; u < kPrunePerThread; ++u) off += s_cnt[ww][u];
#pragma unroll
  for (int u = 0; u < kPrunePerThread; ++u) {
    if ((keep_mask[u] >> lane) & 1ull) {
      const unsigned slot = off + (unsigned)__popcll(keep_mask[u] & ((1ull << lane) - 1ull));
      keys[slot] = kk[u];
      vals[slot] = vv[u];
    }
    off += (unsigned)__popcll(keep_mask[u]);
  }
}

template <typename KeyT>
__global__ __launch_bounds__(kBlock) void k_query_keys_prune(const float4* __restrict__ Gsrc, const unsigned* __restrict__ list, size_t n,
                                                             const unsigned* __restrict__ occ, unsigned stride_w, GridDesc g, InvMap im,
                                                             QueryRange qr, float r2, CertParams cert, KeyT* __restrict__ keys,
                                                             unsigned* __restrict__ vals, unsigned* __restrict__ count,
                                                             int* __restrict__ match, int* __restrict__ match2,
                                                             float* __restrict__ match_d2, float* __restrict__ lbe, int from_state) {
  query_keys_prune_body<KeyT>(blockIdx.x, Gsrc, list, n, occ, stride_w, g, im, qr, r2, cert, keys, vals, count, nullptr, (KeyT)~(KeyT)0, (KeyT)0, true,
                              match, match2, match_d2, lbe, from_state);
}


__device__ __forceinline__ int rdlane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ unsigned rdlane_u(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }

__global__ __launch_bounds__(kBlock, 6) void k_nn_cells(const float4* __restrict__ Gsrc, const unsigned* __restrict__ order,
                                                     size_t n, const float4* __restrict__ Gtgt,
                                                     const HashEntry* __restrict__ table,
                                                     const unsigned* __restrict__ dense_start, GridDesc g, InvMap im,
                                                     QueryRange qr, float r2, int* __restrict__ match_pos,
                                                     float* __restrict__ match_d2) {
  __shared__ float4 s_c[kBlock / kWave][kNNCap];
  __shared__ int s_p[kBlock / kWave][kNNCap];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t pos = ((size_t)blockIdx.x * (kBlock / kWave) + w) * kWave + lane;
  const bool valid = pos < n;
  const unsigned j = valid ? (order[pos] & kListIndexMask) : 0u;
  const float4 q = valid ? Gsrc[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  int cx = 0, cy = 0, cz = 0;
  const unsigned long long key = valid ? query_cell_key(q, im, g, qr, cx, cy, cz) : kEmptyKey;

  float best_d2 = r2;      // strict radius: with best_oi == 0 a candidate at exactly r2 can never win
  unsigned best_oi = 0u;
  int best_pos = -1;
  constexpr int kMaxC = (1 << 21) - 1;

  unsigned long long remaining = __ballot(key != kEmptyKey);
  while (remaining) {
    const int f = __ffsll((long long)remaining) - 1;                      // first lane of the next cell group
    const unsigned klo = rdlane_u((unsigned)key, f), khi = rdlane_u((unsigned)(key >> 32), f);
    const unsigned long long cur = ((unsigned long long)khi << 32) | klo;
    const unsigned long long group = __ballot(key == cur);                // contiguous lanes (sorted input)
    const int a = __popcll(group);
    const int ccx = rdlane_i(cx, f), ccy = rdlane_i(cy, f), ccz = rdlane_i(cz, f);

    // 27 parallel cell lookups: dense cell-start directory (one coalesced round trip, runs of x-neighbours
    // are adjacent words) or, for grids too large for it, the hash table
    unsigned st = 0u, cnt = 0u;
    if (lane < 27) {
      const int x = ccx + (lane % 3) - 1, y = ccy + ((lane / 3) % 3) - 1, z = ccz + (lane / 9) - 1;
      if (dense_start) {
        const unsigned kx = (unsigned)(x - qr.lo[0]), ky = (unsigned)(y - qr.lo[1]), kz = (unsigned)(z - qr.lo[2]);
        if (kx < qr.D[0] && ky < qr.D[1] && kz < qr.D[2]) {
          const size_t lin = ((size_t)kz * qr.D[1] + ky) * qr.D[0] + kx;
          st = dense_start[lin];
          cnt = dense_start[lin + 1] - st;
        }
      } else if (x >= 0 && y >= 0 && z >= 0 && x <= kMaxC && y <= kMaxC && z <= kMaxC) {
        const unsigned long long ck = cell_key(x, y, z);
        unsigned h = hash_key(ck) & g.mask;
        for (;;) {
          const HashEntry en = table[h];
          if (en.key == ck) { st = en.start; cnt = en.end - en.start; break; }
          if (en.key == kEmptyKey) break;
          h = (h + 1) & g.mask;
        }
      }
    }
    unsigned inc = cnt;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const unsigned t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    const unsigned off = inc - cnt;
    const unsigned total = rdlane_u(inc, 26);

    // lanes = (query slot) x (candidate slice)
    int lg = 0;
    while ((1 << lg) < a) ++lg;
    const int A2 = 1 << lg, slices = kWave >> lg;
    const int qi = lane & (A2 - 1), sl = lane >> lg;
    const bool act = qi < a;
    const int owner = (f + qi) & 63;
    const float qx = __shfl(q.x, owner, 64), qy = __shfl(q.y, owner, 64), qz = __shfl(q.z, owner, 64);
    float lb_d2 = r2;
    unsigned lb_oi = 0u;
    int lb_pos = -1;

    for (unsigned base = 0; base < total; base += kNNCap) {
      const unsigned nb = min((unsigned)kNNCap, total - base);
      // stage the bucket: every lane first resolves the source positions of its kNNCap/64 slots (flat
      // candidate index -> (cell run, offset) via the 27 prefix sums), then all loads are issued
      // back-to-back, then the LDS stores -- one memory round trip per batch instead of one per run.
      static_assert(kNNCap == 4 * kWave, "staging below is written for 4 slots per lane");
      const unsigned t0 = base + (unsigned)lane, t1 = t0 + kWave, t2 = t1 + kWave, t3 = t2 + kWave;
      unsigned m0 = 0xFFFFFFFFu, m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu, m3 = 0xFFFFFFFFu;
      for (int r = 0; r < 27; ++r) {
        const unsigned c_r = rdlane_u(cnt, r);
        if (c_r == 0u) continue;
        const unsigned o_r = rdlane_u(off, r), s_r = rdlane_u(st, r);
        if (t0 - o_r < c_r) m0 = s_r + (t0 - o_r);     // unsigned wrap makes this "o_r <= t < o_r + c_r"
        if (t1 - o_r < c_r) m1 = s_r + (t1 - o_r);
        if (t2 - o_r < c_r) m2 = s_r + (t2 - o_r);
        if (t3 - o_r < c_r) m3 = s_r + (t3 - o_r);
      }
      float4 c0, c1, c2, c3;
      if (m0 != 0xFFFFFFFFu) c0 = Gtgt[m0];
      if (m1 != 0xFFFFFFFFu) c1 = Gtgt[m1];
      if (m2 != 0xFFFFFFFFu) c2 = Gtgt[m2];
      if (m3 != 0xFFFFFFFFu) c3 = Gtgt[m3];
      if (m0 != 0xFFFFFFFFu) { s_c[w][lane] = c0; s_p[w][lane] = (int)m0; }
      if (m1 != 0xFFFFFFFFu) { s_c[w][kWave + lane] = c1; s_p[w][kWave + lane] = (int)m1; }
      if (m2 != 0xFFFFFFFFu) { s_c[w][2 * kWave + lane] = c2; s_p[w][2 * kWave + lane] = (int)m2; }
      if (m3 != 0xFFFFFFFFu) { s_c[w][3 * kWave + lane] = c3; s_p[w][3 * kWave + lane] = (int)m3; }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      int lb_t = -1;
      if (act) {
#pragma unroll 4
        for (unsigned t = sl; t < nb; t += slices) {
          const float4 c = s_c[w][t];
          const float d2 = sqdist_l2(qx, qy, qz, c.x, c.y, c.z);
          const unsigned oi = __float_as_uint(c.w);
          if (d2 < lb_d2 || (d2 == lb_d2 && oi < lb_oi)) { lb_d2 = d2; lb_oi = oi; lb_t = (int)t; }
        }
        if (lb_t >= 0) lb_pos = s_p[w][lb_t];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // min over the candidate slices of each query slot
    for (int stx = A2; stx < kWave; stx <<= 1) {
      const float od2 = __shfl_xor(lb_d2, stx, 64);
      const unsigned ooi = (unsigned)__shfl_xor((int)lb_oi, stx, 64);
      const int opos = __shfl_xor(lb_pos, stx, 64);
      if (od2 < lb_d2 || (od2 == lb_d2 && ooi < lb_oi)) { lb_d2 = od2; lb_oi = ooi; lb_pos = opos; }
    }
    // hand the result to the lane that owns the query
    const int srcl = (lane - f) & 63;
    const float rd2 = __shfl(lb_d2, srcl, 64);
    const unsigned roi = (unsigned)__shfl((int)lb_oi, srcl, 64);
    const int rpos = __shfl(lb_pos, srcl, 64);
    if ((group >> lane) & 1ull) {
      if (rd2 < best_d2 || (rd2 == best_d2 && roi < best_oi)) { best_d2 = rd2; best_oi = roi; best_pos = rpos; }
    }
    remaining &= ~group;
  }
  if (valid) { match_pos[pos] = best_pos; match_d2[pos] = best_d2; }
}

// -------------------------------------------------------------------------------------------------
// Dense-directory path of a5 (the default on MI355X: 4 B per grid cell is cheap in 288 GB of HBM).
// Queries are sorted by target cell in (z, y, x) order -- the same order the target's points are stored
// in -- so the candidates of a run of cells [xa, xb] inside one neighbour ROW (y+dy, z+dz) are ONE contiguous
// run [S[lin(xa)], S[lin(xb)+1]) of the target array.  A wave handles a whole ROW SEGMENT of its 64 sorted
// queries at once (consecutive lanes in the same row, x-extent <= kRowSpan cells): 18 directory words
// (one round trip), the 9 union runs staged in LDS with all loads in flight together (second round trip),
// then lanes arranged as (query slot) x (candidate slice) scan the staged superset.  Candidates outside a
// query's own 27 cells are farther than the radius, so they can never win: results are identical to the
// other two kernels.
//
// The scan is VALU-issue bound (rocprofv3 PMC: SQ_ACTIVE_INST_VALU ~ 75 % of the kernel), so the inner loop is
// written for instruction count: candidates are staged as SoA PAIRS {x0,x1,y0,y1} {z0,z1} so that the three
// subtractions, three squares and two sums run as packed f32 ops (v_pk_add_f32 / v_pk_mul_f32, each still an
// individually rounded IEEE op in the (dx*dx + dy*dy) + dz*dz order); the bucket is padded with +inf sentinels
// so the loop is uniform and branch free with four pairs prefetched; and the (d2, index) tie rule is applied
// lazily: the fast loop tracks only (d2, slot) with a strict '<' and records whether ANY equality was seen, in
// which case (rare: lattices, duplicates) the batch is re-scanned with the full comparator.
// -------------------------------------------------------------------------------------------------
typedef float f2_t __attribute__((ext_vector_type(2)));

struct RowLds {
  float4 xy[kRowCap / 2 + 2 * kWave];   // {x0, x1, y0, y1} per candidate pair (+ sentinel padding)
  float2 z[kRowCap / 2 + 2 * kWave];    // {z0, z1}
  unsigned oi[kRowCap];             // original target index (tie rule, result)
};

// Fast scan: per QUAD of candidates (two staged pairs) only the minimum distance is compared with the running
// best -- 2 v_min + 2 v_cmp + 2 v_cndmask per four candidates instead of a compare/select chain per candidate.
// The winning quad is re-evaluated exactly afterwards (row_scan_resolve); `tie` records whether a quad minimum
// ever EQUALLED the running best (cross-quad tie), in which case the caller re-scans the batch with the full
// comparator.  trips2 = number of quads per lane; quad i of a lane covers pairs sl + 2*i*slices and
// sl + (2*i+1)*slices (sentinel padded).
__device__ __forceinline__ f2_t row_pair_d2(const float4 A, const float2 Zv, const f2_t QX, const f2_t QY, const f2_t QZ) {
  const f2_t cx = {A.x, A.y}, cy = {A.z, A.w}, cz = {Zv.x, Zv.y};
  const f2_t dx = QX - cx, dy = QY - cy, dz = QZ - cz;
  f2_t d = dx * dx;
  d = d + dy * dy;
  d = d + dz * dz;
  return d;
}

// b2 follows the second smallest value at quad granularity (a displaced best, or the minimum of a quad that did not win);
// the other members of the winning quad are folded in by row_scan_resolve, so that afterwards b2 is the exact second
// smallest squared distance among all candidates seen (the certificate bound of k_nn_certify).
__device__ __forceinline__ void row_scan_fast(const RowLds& L, int sl, int slices, int trips2, float qx, float qy,
                                              float qz, float& bd, int& bq, bool& tie, float& b2) {
  const f2_t QX = {qx, qx}, QY = {qy, qy}, QZ = {qz, qz};
  int p = sl;
  int i = 0;
#define E3D_QUAD_STEP(A0, Z0, A1, Z1, I)                                      \
  {                                                                          \
    const f2_t d0 = row_pair_d2(A0, Z0, QX, QY, QZ);                          \
    const f2_t d1 = row_pair_d2(A1, Z1, QX, QY, QZ);                          \
    const float mq = fminf(fminf(d0.x, d0.y), fminf(d1.x, d1.y));            \
    b2 = fminf(b2, fmaxf(bd, mq));                                           \
    const bool lt = mq < bd, le = mq <= bd;                                  \
    tie = tie || (le && !lt);                                                \
    bd = lt ? mq : bd;                                                       \
    bq = lt ? (I) : bq;                                                      \
  }
  for (; i + 2 <= trips2; i += 2) {
    const float4 a0 = L.xy[p], a1 = L.xy[p + slices], a2 = L.xy[p + 2 * slices], a3 = L.xy[p + 3 * slices];
    const float2 z0 = L.z[p], z1 = L.z[p + slices], z2 = L.z[p + 2 * slices], z3 = L.z[p + 3 * slices];
    E3D_QUAD_STEP(a0, z0, a1, z1, i)
    E3D_QUAD_STEP(a2, z2, a3, z3, i + 1)
    p += 4 * slices;
  }
  for (; i < trips2; ++i) {
    const float4 a0 = L.xy[p], a1 = L.xy[p + slices];
    const float2 z0 = L.z[p], z1 = L.z[p + slices];
    E3D_QUAD_STEP(a0, z0, a1, z1, i)
    p += 2 * slices;
  }
#undef E3D_QUAD_STEP
}

// exact (d2, original index) comparator over the four candidates of quad `bq` of this lane
__device__ __forceinline__ void row_scan_resolve(const RowLds& L, int sl, int slices, int bq, unsigned base, unsigned nb,
                                                 float qx, float qy, float qz, float& bd, unsigned& boi, unsigned& bt, float& b2) {
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    const int p = sl + (2 * bq + h2) * slices;
    const float4 A = L.xy[p];
    const float2 Zv = L.z[p];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const unsigned t = 2u * (unsigned)p + (unsigned)hh;
      if (t >= nb) continue;
      const float d2 = sqdist_l2(qx, qy, qz, hh ? A.y : A.x, hh ? A.w : A.z, hh ? Zv.y : Zv.x);
      const unsigned oi = L.oi[t];
      if (d2 < bd || (d2 == bd && oi < boi)) { b2 = fminf(b2, bd); bd = d2; boi = oi; bt = base + t; }
      else b2 = fminf(b2, d2);
    }
  }
}

// exact re-scan with the full (d2, original index) comparator
__device__ __forceinline__ void row_scan_exact(const RowLds& L, int sl, int slices, int trips, unsigned base, unsigned nb,
                                               float qx, float qy, float qz, float& bd, unsigned& boi, unsigned& bt, float& b2) {
  int p = sl;
  for (int i = 0; i < trips; ++i, p += slices) {
    const float4 A = L.xy[p];
    const float2 Zv = L.z[p];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const unsigned t = 2u * (unsigned)p + (unsigned)hh;
      if (t >= nb) continue;
      const float d2 = sqdist_l2(qx, qy, qz, hh ? A.y : A.x, hh ? A.w : A.z, hh ? Zv.y : Zv.x);
      const unsigned oi = L.oi[t];
      if (d2 < bd || (d2 == bd && oi < boi)) { b2 = fminf(b2, bd); bd = d2; boi = oi; bt = base + t; }
      else b2 = fminf(b2, d2);
    }
  }
}

// Results are written at the query's SOURCE position order[pos] (the queries may be a sorted sub-list of the source cloud):
// match_pos / match_d2 as before, and lbe = (distance every target point other than the partner exceeds) + cert.cum_lo, the
// state k_nn_certify tests in the following outer iterations.
__device__ __forceinline__ void nn_rows_body(const unsigned bx, const float4* __restrict__ Gsrc, const unsigned* __restrict__ order,
                                             size_t n, const float4* __restrict__ Gtgt,
                                             const unsigned* __restrict__ S, const GridDesc& g, const InvMap& im,
                                             const QueryRange& qr, float r2, int row_span, const CertParams& cert,
                                             int* __restrict__ match_pos, float* __restrict__ match_d2,
                                             float* __restrict__ lbe, int* __restrict__ match2) {
  __shared__ RowLds lds[kBlock / kWave];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  RowLds& L = lds[w];
  const size_t pos = ((size_t)bx * (kBlock / kWave) + w) * kWave + lane;
  const bool valid = pos < n;
  const unsigned jf = valid ? order[pos] : 0u, j = jf & kListIndexMask;
  const float4 q = valid ? Gsrc[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  int cx = 0, cy = 0, cz = 0;
  float block_dist = 2.0f;
  const unsigned long long key = valid ? query_cell_key(q, im, g, qr, cx, cy, cz, &block_dist) : kEmptyKey;
  if (key == kEmptyKey) block_dist = 2.0f;     // outside the directory range (occupied cells +- 2): two empty cells all around
  const int kx = cx - qr.lo[0], ky = cy - qr.lo[1], kz = cz - qr.lo[2];   // in [0, D) for valid keys

  float best_d2 = r2;      // strict radius (see k_nn_query)
  unsigned best_oi = 0u;
  int best_pos = -1;
  const float kInf = __uint_as_float(0x7f800000u);
  float best_b2 = kInf;    // second smallest squared distance among the candidates seen

  unsigned long long remaining = __ballot(key != kEmptyKey);
  while (remaining) {
    const int f = __ffsll((long long)remaining) - 1;
    const int fky = rdlane_i(ky, f), fkz = rdlane_i(kz, f), fkx = rdlane_i(kx, f);
    // segment: lanes of the same row whose cells lie within kRowSpan cells of the first (contiguous: sorted input)
    const unsigned long long seg =
        __ballot(key != kEmptyKey && ky == fky && kz == fkz && (unsigned)(kx - fkx) <= (unsigned)row_span) & remaining;
    const int a = __popcll(seg);
    const int last = 63 - __clzll((long long)seg);
    const int lkx = rdlane_i(kx, last);
    const int xa = max(fkx - 1, 0), xb = min(lkx + 1, (int)qr.D[0] - 1);

    // directory words of the 9 neighbour rows (lanes 0..8)
    unsigned dst = 0u, dcnt = 0u;
    if (lane < 9) {
      const int y = fky + (lane % 3) - 1, z = fkz + (lane / 3) - 1;
      if (y >= 0 && z >= 0 && y < (int)qr.D[1] && z < (int)qr.D[2]) {
        const size_t row = ((size_t)z * qr.D[1] + (size_t)y) * qr.D[0];
        dst = S[row + xa];
        dcnt = S[row + xb + 1] - dst;
      }
    }
    unsigned rs[9], rl[9];
    unsigned total = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) { rs[r] = rdlane_u(dst, r); rl[r] = rdlane_u(dcnt, r); total += rl[r]; }

    // lanes = (query slot) x (candidate slice)
    int lg = 0;
    while ((1 << lg) < a) ++lg;
    const int A2 = 1 << lg, slices = kWave >> lg;
    const int qi = lane & (A2 - 1), sl = lane >> lg;
    const int owner = (f + qi) & 63;
    const float qx = __shfl(q.x, owner, 64), qy = __shfl(q.y, owner, 64), qz = __shfl(q.z, owner, 64);
    float lb_d2 = r2;
    unsigned lb_oi = 0u;
    unsigned lb_t = 0xFFFFFFFFu;      // flat index into the concatenated 9 runs
    float lb_b2 = kInf;

    for (unsigned base = 0; base < total; base += kRowCap) {
      const unsigned nb = min((unsigned)kRowCap, total - base);
      const int np = (int)((nb + 1u) >> 1);
      const int trips2 = (np + 2 * slices - 1) / (2 * slices);   // quads (2 pairs) per lane
      const int trips = 2 * trips2;
      // ---- stage [base, base + nb) of the concatenated runs.  Each lane handles candidate PAIRS (2u, 2u + 1): the SoA-pair
      // layout is then one 16-byte and two 8-byte LDS stores per pair, and the flat index -> target position map
      // (position = flat + off_r for the run r that contains it, off_r wave-uniform) costs two instructions per run.
      constexpr int kPairsPerLane = kRowCap / 2 / kWave;
      unsigned pm[kPairsPerLane][2];
#pragma unroll
      for (int k = 0; k < kPairsPerLane; ++k) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const unsigned fl = base + 2u * (unsigned)(k * kWave + lane) + (unsigned)hh;
          unsigned off = rs[0];
          unsigned P = rl[0];
#pragma unroll
          for (int r = 1; r < 9; ++r) {
            off = (fl >= P) ? rs[r] - P : off;          // an empty run r is overridden by the next one (same P)
            P += rl[r];
          }
          pm[k][hh] = (fl < total) ? fl + off : 0xFFFFFFFFu;
        }
      }
      float4 cv[kPairsPerLane][2];
#pragma unroll
      for (int k = 0; k < kPairsPerLane; ++k)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
          cv[k][hh] = (pm[k][hh] != 0xFFFFFFFFu) ? Gtgt[pm[k][hh]] : make_float4(kInf, 0.f, 0.f, 0.f);
      const unsigned padded_pairs = (unsigned)(trips * slices);            // pairs incl. sentinels (<= kRowCap / 2 + 2 * 64)
      uint2* const oi2 = reinterpret_cast<uint2*>(L.oi);
#pragma unroll
      for (int k = 0; k < kPairsPerLane + 2; ++k) {
        const unsigned u = (unsigned)(k * kWave + lane);
        if (u < padded_pairs) {
          const float4 c0 = (k < kPairsPerLane) ? cv[k < kPairsPerLane ? k : 0][0] : make_float4(kInf, 0.f, 0.f, 0.f);
          const float4 c1 = (k < kPairsPerLane) ? cv[k < kPairsPerLane ? k : 0][1] : make_float4(kInf, 0.f, 0.f, 0.f);
          L.xy[u] = make_float4(c0.x, c1.x, c0.y, c1.y);    // x = +inf for slots past nb: d2 = +inf never wins and never ties
          L.z[u] = make_float2(c0.z, c1.z);
          if (2u * u < nb) oi2[u] = make_uint2(__float_as_uint(c0.w), __float_as_uint(c1.w));
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

      const float in_d2 = lb_d2, in_b2 = lb_b2;
      const unsigned in_oi = lb_oi, in_t = lb_t;
      bool tie = false;
      int bq = -1;
      float fd = lb_d2;
      row_scan_fast(L, sl, slices, trips2, qx, qy, qz, fd, bq, tie, lb_b2);
      if (__ballot(tie)) {                    // rare: cross-quad exact f32 distance tie -> full comparator for this batch
        lb_d2 = in_d2; lb_oi = in_oi; lb_t = in_t; lb_b2 = in_b2;
        row_scan_exact(L, sl, slices, trips, base, nb, qx, qy, qz, lb_d2, lb_oi, lb_t, lb_b2);
      } else if (bq >= 0) {                   // winner quad: exact (d2, index) order among its four candidates
        row_scan_resolve(L, sl, slices, bq, base, nb, qx, qy, qz, lb_d2, lb_oi, lb_t, lb_b2);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // flat index of the slice winner -> position in the target array
    int lb_pos = -1;
    {
      unsigned p = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r) {
        if (lb_t - p < rl[r]) lb_pos = (int)(rs[r] + (lb_t - p));
        p += rl[r];
      }
    }
    // min over the candidate slices of each query slot
    for (int stx = A2; stx < kWave; stx <<= 1) {
      const float od2 = __shfl_xor(lb_d2, stx, 64);
      const unsigned ooi = (unsigned)__shfl_xor((int)lb_oi, stx, 64);
      const int opos = __shfl_xor(lb_pos, stx, 64);
      const float ob2 = __shfl_xor(lb_b2, stx, 64);
      lb_b2 = fminf(fminf(lb_b2, ob2), fmaxf(lb_d2, od2));      // second smallest of the two slices together
      if (od2 < lb_d2 || (od2 == lb_d2 && ooi < lb_oi)) { lb_d2 = od2; lb_oi = ooi; lb_pos = opos; }
    }
    // hand the result to the lane that owns the query
    const int srcl = (lane - f) & 63;
    const float rd2 = __shfl(lb_d2, srcl, 64);
    const unsigned roi = (unsigned)__shfl((int)lb_oi, srcl, 64);
    const int rpos = __shfl(lb_pos, srcl, 64);
    const float rb2 = __shfl(lb_b2, srcl, 64);
    if ((seg >> lane) & 1ull) {
      best_b2 = fminf(fminf(best_b2, rb2), fmaxf(best_d2, rd2));
      if (rd2 < best_d2 || (rd2 == best_d2 && roi < best_oi)) { best_d2 = rd2; best_oi = roi; best_pos = rpos; }
    }
    remaining &= ~seg;
  }
  if (valid) {
    // A query that had no partner and still has none (kListNoPartner, set by k_nn_certify -- most queries of the first outer
    // iterations of a poorly aligned pair) holds match = match2 = -1 already, and k_nn_certify has stored r2 as its distance:
    // only the certificate changes.  Three of the four scattered 4-byte stores of this kernel, a third of its time there.
    if (!((jf & kListNoPartner) && best_pos < 0)) {
      match_pos[j] = best_pos; match_d2[j] = best_d2;
      if (match2) match2[j] = -1;               // this kernel remembers the partner only
    }
    // every candidate in the 27 cells was evaluated: the others are >= sqrt(best_b2) away (all of them, if there is no partner:
    // best_d2 stayed r2, so best_b2 is the smallest distance seen); points outside the block are >= block_dist cells away in
    // the local frame (2 cells if the query's cell lies outside the directory range, i.e. occupied cells +- 2)
    const float lb_out = block_dist * cert.cell_scale - cert.cell_sub;
    lbe[j] = fmaxf(fminf(sqrtf(best_b2), lb_out), 0.0f) * 0.999999f + motion_lo(q, cert.lo);
  }
}

__global__ __launch_bounds__(kBlock, 6) void k_nn_rows(const float4* __restrict__ Gsrc, const unsigned* __restrict__ order,
                                                       size_t n, const float4* __restrict__ Gtgt,
                                                       const unsigned* __restrict__ S, GridDesc g, InvMap im,
                                                       QueryRange qr, float r2, int row_span, CertParams cert,
                                                       int* __restrict__ match_pos, float* __restrict__ match_d2,
                                                       float* __restrict__ lbe, int* __restrict__ match2) {
  nn_rows_body(blockIdx.x, Gsrc, order, n, Gtgt, S, g, im, qr, r2, row_span, cert, match_pos, match_d2, lbe, match2);
}

// -------------------------------------------------------------------------------------------------
// MFMA-filtered variant of k_nn_rows (same segments, same staging runs, same results).
//
// The scan of a segment is a dense (queries x candidates) squared-distance matrix.  Its entries are first computed
// APPROXIMATELY on the matrix cores -- |q|^2 + |c|^2 - 2 q.c as one K = 16 f16 MFMA per 32 x 32 tile, with coordinates
// taken relative to a per-segment origin, scaled by a power of two and split into f16 hi + lo parts so that the result
// is within a PROVEN bound of the exact f32 value (host: mfma_filter_params) -- and only candidates whose approximate
// distance is within that bound of the running approximate minimum (or of the radius) are evaluated EXACTLY, with the
// very arithmetic (sqdist_l2) and the (d2, original index) order of the other kernels.  Every candidate that could be
// the exact winner passes the filter, so the output is bit-identical; the VALU work per pair drops from ~6
// instructions to ~0.02 (a min-tree over the accumulators) plus the per-candidate operand packing.
// The query's own cell row is scanned first: most queries meet their nearest neighbour there, after which the
// filter rarely fires.
//
// Operand layout (v_mfma_f32_32x32x16_f16: A = candidates as rows, B = queries as columns; lane l supplies row / column
// l & 31 and the eight k values 8 * (l >> 5) .. + 7):
//   k:   0     1     2     3    4     5     6     7   |  8     9     10    11   12    13    14    15
//   A:   chx   chy   chz   nch  clx   cly   clz   ncl |  chx   chy   chz   1    clx   cly   clz   1
//   B:  -2qhx -2qhy -2qhz  1   -2qhx -2qhy -2qhz  1   | -2qlx -2qly -2qlz  nqh -2qlx -2qly -2qlz  nql
// (h / l = f16 hi / lo part of the scaled relative coordinate, n.. = hi / lo part of |hi + lo|^2.)
// -------------------------------------------------------------------------------------------------
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef float f16_t __attribute__((ext_vector_type(16)));
typedef __fp16 fp16x2_t __attribute__((ext_vector_type(2)));

constexpr int kMfCap = 256;                     // candidates staged per wave and batch
constexpr float kMfSentinel = 60000.0f;         // |.|^2 part of padding rows / columns: never passes the filter

struct MfLds {
  uint4 a[kMfCap / 32][2][32];                  // operand A parts: [tile][k half][row]
  float4 c[kMfCap];                             // exact coordinates + original index (for the exact evaluation)
};

__device__ __forceinline__ unsigned pk_rtz(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b));
}
__device__ __forceinline__ float h_lo(unsigned w) { return (float)__builtin_bit_cast(fp16x2_t, w)[0]; }
__device__ __forceinline__ float h_hi(unsigned w) { return (float)__builtin_bit_cast(fp16x2_t, w)[1]; }

// hi / lo split of a scaled relative position: words (hx,hy) (hz,0) (lx,ly) (lz,0) and |hi + lo|^2
struct MfSplit { unsigned hxy, hz0, lxy, lz0; float n; };
__device__ __forceinline__ MfSplit mf_split(float x, float y, float z) {
  MfSplit r;
  r.hxy = pk_rtz(x, y); r.hz0 = pk_rtz(z, 0.f);
  const float hx = h_lo(r.hxy), hy = h_hi(r.hxy), hz = h_lo(r.hz0);
  const float rx = x - hx, ry = y - hy, rz = z - hz;                // exact
  r.lxy = pk_rtz(rx, ry); r.lz0 = pk_rtz(rz, 0.f);
  const float cx = hx + h_lo(r.lxy), cy = hy + h_hi(r.lxy), cz = hz + h_lo(r.lz0);   // exact sums
  r.n = cx * cx + (cy * cy + cz * cz);
  return r;
}
// (hi, lo) f16 parts of a non-negative norm as the high halves of two words whose low halves are given
__device__ __forceinline__ void mf_norm_parts(float n, unsigned lowA, unsigned lowB, unsigned& wA, unsigned& wB) {
  const unsigned nh = pk_rtz(0.f, n);                               // high half = rtz(n)
  const float rest = n - h_hi(nh);
  const unsigned nl = pk_rtz(0.f, rest);
  wA = (lowA & 0xFFFFu) | (nh & 0xFFFF0000u);
  wB = (lowB & 0xFFFFu) | (nl & 0xFFFF0000u);
}

// MfParams (e3d_icp_kernels.hpp): S = power-of-two scale of the relative coordinates, r2s = r^2 S^2, eta2 = 2 eta (eta bounds
// |mfma value - scaled exact f32 d2| apart from the coordinate representation), delta4 = 4 Delta, delta4sq = 4 Delta^2
// (Delta bounds the error of a scaled point-to-point distance caused by the hi/lo representation).
__device__ __forceinline__ float mf_threshold(float am, const MfParams& P) {
  return am + P.eta2 + P.delta4 * sqrtf(fmaxf(am, 0.f)) + P.delta4sq;
}

__device__ __forceinline__ float mf_min16(const f16_t& v) {
  const float a = fminf(fminf(v[0], v[1]), v[2]), b = fminf(fminf(v[3], v[4]), v[5]);
  const float c = fminf(fminf(v[6], v[7]), v[8]), d = fminf(fminf(v[9], v[10]), v[11]);
  const float e = fminf(fminf(v[12], v[13]), v[14]);
  return fminf(fminf(fminf(a, b), fminf(c, d)), fminf(e, v[15]));
}

// one query column group: running approximate minimum + filter threshold, exact best so far
struct MfBest {
  float am, thr;
  float qx, qy, qz;
  float bd; unsigned boi, bt;
};

__device__ __forceinline__ void mf_process(const f16_t& acc, MfBest& B, const MfLds& L, int tile, int g, unsigned base, unsigned nb,
                                           const MfParams& P) {
  const float tm = mf_min16(acc);
  if (!__ballot(tm <= B.thr)) return;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    if (acc[reg] <= B.thr) {
      const int row = (reg & 3) + 8 * (reg >> 2) + 4 * g;
      const unsigned t = (unsigned)(tile * 32 + row);
      const float4 cc = L.c[t];
      const float d2 = sqdist_l2(B.qx, B.qy, B.qz, cc.x, cc.y, cc.z);
      const unsigned oi = __float_as_uint(cc.w);
      if (t < nb && (d2 < B.bd || (d2 == B.bd && oi < B.boi))) { B.bd = d2; B.boi = oi; B.bt = base + t; }
      if (acc[reg] < B.am) { B.am = acc[reg]; B.thr = mf_threshold(B.am, P); }
    }
  }
}

__global__ __launch_bounds__(kBlock, 3) void k_nn_mfma(const float4* __restrict__ Gsrc, const unsigned* __restrict__ order,
                                                       size_t n, const float4* __restrict__ Gtgt,
                                                       const unsigned* __restrict__ S, GridDesc g, InvMap im,
                                                       QueryRange qr, float r2, int row_span, MfParams P,
                                                       int* __restrict__ match_pos, float* __restrict__ match_d2) {
  __shared__ MfLds lds[kBlock / kWave];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  MfLds& L = lds[w];
  const int col = lane & 31, gh = lane >> 5;
  const size_t pos = ((size_t)blockIdx.x * (kBlock / kWave) + w) * kWave + lane;
  const bool valid = pos < n;
  const unsigned j = valid ? (order[pos] & kListIndexMask) : 0u;
  const float4 q = valid ? Gsrc[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  int cx = 0, cy = 0, cz = 0;
  const unsigned long long key = valid ? query_cell_key(q, im, g, qr, cx, cy, cz) : kEmptyKey;
  const int kx = cx - qr.lo[0], ky = cy - qr.lo[1], kz = cz - qr.lo[2];

  float best_d2 = r2;
  unsigned best_oi = 0u;
  int best_pos = -1;
  const float kInf = __uint_as_float(0x7f800000u);
  const float thr0 = mf_threshold(P.r2s, P);
  const f16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const unsigned one_hi = 0x3C000000u;                              // f16 1.0 in the high half

  unsigned long long remaining = __ballot(key != kEmptyKey);
  while (remaining) {
    const int f = __ffsll((long long)remaining) - 1;
    const int fky = rdlane_i(ky, f), fkz = rdlane_i(kz, f), fkx = rdlane_i(kx, f);
    const unsigned long long seg =
        __ballot(key != kEmptyKey && ky == fky && kz == fkz && (unsigned)(kx - fkx) <= (unsigned)row_span) & remaining;
    const int a = __popcll(seg);
    const int last = 63 - __clzll((long long)seg);
    const int lkx = rdlane_i(kx, last);
    const int xa = max(fkx - 1, 0), xb = min(lkx + 1, (int)qr.D[0] - 1);

    // directory words of the 9 neighbour rows, the queries' own row first (lanes 0..8)
    unsigned dst = 0u, dcnt = 0u;
    if (lane < 9) {
      const int rid = (int)((0x862075314ull >> (4 * lane)) & 15ull);       // 4, 1, 3, 5, 7, 0, 2, 6, 8
      const int y = fky + (rid % 3) - 1, z = fkz + (rid / 3) - 1;
      if (y >= 0 && z >= 0 && y < (int)qr.D[1] && z < (int)qr.D[2]) {
        const size_t row = ((size_t)z * qr.D[1] + (size_t)y) * qr.D[0];
        dst = S[row + xa];
        dcnt = S[row + xb + 1] - dst;
      }
    }
    unsigned rs[9], rl[9];
    unsigned total = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) { rs[r] = rdlane_u(dst, r); rl[r] = rdlane_u(dcnt, r); total += rl[r]; }

    // segment origin: midpoint of its first and last query (wave-uniform)
    const float ox = 0.5f * (__shfl(q.x, f, 64) + __shfl(q.x, last, 64));
    const float oy = 0.5f * (__shfl(q.y, f, 64) + __shfl(q.y, last, 64));
    const float oz = 0.5f * (__shfl(q.z, f, 64) + __shfl(q.z, last, 64));

    // B operands: column group G holds query slots 32 G + col
    h8_t Bop[2];
    MfBest Q[2];
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      const int slot = 32 * G + col;
      const int owner = (f + slot) & 63;
      const float qx = __shfl(q.x, owner, 64), qy = __shfl(q.y, owner, 64), qz = __shfl(q.z, owner, 64);
      const bool qv = slot < a;
      Q[G].qx = qx; Q[G].qy = qy; Q[G].qz = qz;
      Q[G].am = P.r2s; Q[G].thr = qv ? thr0 : -kInf;
      Q[G].bd = r2; Q[G].boi = 0u; Q[G].bt = 0xFFFFFFFFu;
      const MfSplit sp = mf_split(qv ? (qx - ox) * P.S : 0.f, qv ? (qy - oy) * P.S : 0.f, qv ? (qz - oz) * P.S : 0.f);
      uint4 wv;
      if (gh == 0) {
        const unsigned w0 = pk_rtz(-2.f * h_lo(sp.hxy), -2.f * h_hi(sp.hxy));
        const unsigned w1 = (pk_rtz(-2.f * h_lo(sp.hz0), 0.f) & 0xFFFFu) | one_hi;
        wv = make_uint4(w0, w1, w0, w1);
      } else {
        const unsigned w0 = pk_rtz(-2.f * h_lo(sp.lxy), -2.f * h_hi(sp.lxy));
        const unsigned w1l = pk_rtz(-2.f * h_lo(sp.lz0), 0.f);
        unsigned w1, w3;
        mf_norm_parts(qv ? sp.n : kMfSentinel, w1l, w1l, w1, w3);
        wv = make_uint4(w0, w1, w0, w3);
      }
      Bop[G] = __builtin_bit_cast(h8_t, wv);
    }
    const bool two = a > 32;

    for (unsigned base = 0; base < total; base += kMfCap) {
      const unsigned nb = min((unsigned)kMfCap, total - base);
      const int ntiles = (int)((nb + 31u) >> 5);
      // ---- stage [base, base + nb): resolve indices, issue the loads, pack the operands ----
      unsigned m[kMfCap / kWave];
#pragma unroll
      for (int k = 0; k < kMfCap / kWave; ++k) m[k] = 0xFFFFFFFFu;
      {
        unsigned p = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
#pragma unroll
          for (int k = 0; k < kMfCap / kWave; ++k) {
            const unsigned t = base + (unsigned)(k * kWave + lane) - p;
            if (t < rl[r]) m[k] = rs[r] + t;
          }
          p += rl[r];
        }
      }
      float4 cv[kMfCap / kWave];
#pragma unroll
      for (int k = 0; k < kMfCap / kWave; ++k) cv[k] = (m[k] != 0xFFFFFFFFu) ? Gtgt[m[k]] : make_float4(kInf, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < kMfCap / kWave; ++k) {
        const unsigned t = (unsigned)(k * kWave + lane);
        if (t < (unsigned)(ntiles * 32)) {
          const bool cvd = m[k] != 0xFFFFFFFFu;
          const float4 c = cv[k];
          const MfSplit sp = mf_split(cvd ? (c.x - ox) * P.S : 0.f, cvd ? (c.y - oy) * P.S : 0.f, cvd ? (c.z - oz) * P.S : 0.f);
          unsigned w1, w3;
          mf_norm_parts(cvd ? sp.n : kMfSentinel, sp.hz0, sp.lz0, w1, w3);
          L.a[t >> 5][0][t & 31] = make_uint4(sp.hxy, w1, sp.lxy, w3);
          L.a[t >> 5][1][t & 31] = make_uint4(sp.hxy, (sp.hz0 & 0xFFFFu) | one_hi, sp.lxy, (sp.lz0 & 0xFFFFu) | one_hi);
          L.c[t] = c;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

      for (int tile = 0; tile < ntiles; ++tile) {
        const h8_t Aop = __builtin_bit_cast(h8_t, L.a[tile][gh][col]);
        const f16_t acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(Aop, Bop[0], zero16, 0, 0, 0);
        if (two) {
          const f16_t acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(Aop, Bop[1], zero16, 0, 0, 0);
          mf_process(acc0, Q[0], L, tile, gh, base, nb, P);
          mf_process(acc1, Q[1], L, tile, gh, base, nb, P);
        } else {
          mf_process(acc0, Q[0], L, tile, gh, base, nb, P);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    // per column group: flat index -> target position, combine the two row halves, hand to the owning lane
    float rd2 = r2; unsigned roi = 0u; int rpos = -1;
    const int slot_of_lane = (lane - f) & 63;
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      int lb_pos = -1;
      {
        unsigned p = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
          if (Q[G].bt - p < rl[r]) lb_pos = (int)(rs[r] + (Q[G].bt - p));
          p += rl[r];
        }
      }
      float lb_d2 = Q[G].bd; unsigned lb_oi = Q[G].boi;
      {
        const float od2 = __shfl_xor(lb_d2, 32, 64);
        const unsigned ooi = (unsigned)__shfl_xor((int)lb_oi, 32, 64);
        const int opos = __shfl_xor(lb_pos, 32, 64);
        if (od2 < lb_d2 || (od2 == lb_d2 && ooi < lb_oi)) { lb_d2 = od2; lb_oi = ooi; lb_pos = opos; }
      }
      const float sd2 = __shfl(lb_d2, slot_of_lane & 31, 64);
      const unsigned soi = (unsigned)__shfl((int)lb_oi, slot_of_lane & 31, 64);
      const int spos = __shfl(lb_pos, slot_of_lane & 31, 64);
      if ((slot_of_lane >> 5) == G) { rd2 = sd2; roi = soi; rpos = spos; }
    }
    if ((seg >> lane) & 1ull) {
      if (rd2 < best_d2 || (rd2 == best_d2 && roi < best_oi)) { best_d2 = rd2; best_oi = roi; best_pos = rpos; }
    }
    remaining &= ~seg;
  }
  if (valid) { match_pos[pos] = best_pos; match_d2[pos] = best_d2; }
}

// The FAR lists of a batch of pairs (round 6): queries without a near partner, too many for the bounded search -- the first outer
// iterations of every pair.  Round 5 keyed, sorted and searched them pair by pair: per pair a key kernel, a read-back of the kept
// count, a radix sort (six launches) and k_nn_rows -- 240 times per outer iteration of a 16-scan job, ~0.3 ms each however short a
// rank's slices are.  Now ONE key kernel walks the pairs' lists (a block finds its pair from the ends of the block ranges) and
// writes (key, query) pairs of all of them into one array, the pair's index above the cell key; ONE radix sort orders them by
// (pair, cell); ONE k_nn_rows launch walks the pairs' stretches of the sorted array.  The bodies are the one-pair kernels': the same
// results bit for bit (a query's result does not depend on its neighbours in the sorted order).
template <typename KeyT>
__global__ __launch_bounds__(kBlock) void k_query_keys_multi(const NnBatchDev* __restrict__ B, float r2, KeyT* __restrict__ keys, unsigned* __restrict__ vals,
                                                             unsigned* __restrict__ counts) {
  const int p = nn_find_range(B->far_end, B->n_pairs, blockIdx.x);
  const unsigned bx = blockIdx.x - (p ? B->far_end[p - 1] : 0u);
  const NnPairDev& P = B->pair[p];
  const GridDesc g = P.g; const InvMap im = P.im; const QueryRange qr = P.qr;
  const CertParams cert = {P.bp.cell_scale, P.bp.cell_sub, P.bp.lo};
  const int shift = B->key_shift;
  const KeyT mask = (KeyT)(((KeyT)1 << shift) - (KeyT)1), hi = (KeyT)((KeyT)p << shift);
  const int flags = __builtin_amdgcn_readfirstlane(P.far_flags);
  query_keys_prune_body<KeyT>(bx, P.Gsrc, P.far_list, (size_t)P.far_n, P.occ, P.occ_stride, g, im, qr, r2, cert, keys, vals, counts, counts + 1 + p, mask, hi,
                              (flags & 2) != 0, P.match, P.match2, P.match_d2, P.lbe, flags & 1);
}

__global__ __launch_bounds__(kBlock, 6) void k_nn_rows_multi(const NnBatchDev* __restrict__ B, const unsigned* __restrict__ order, float r2, int row_span) {
  const int p = nn_find_range(B->rows_end, B->n_pairs, blockIdx.x);
  const unsigned bx = blockIdx.x - (p ? B->rows_end[p - 1] : 0u);
  const NnPairDev& P = B->pair[p];
  const GridDesc g = P.g; const InvMap im = P.im; const QueryRange qr = P.qr;
  const CertParams cert = {P.bp.cell_scale, P.bp.cell_sub, P.bp.lo};
  nn_rows_body(bx, P.Gsrc, order + P.rows_off, (size_t)P.rows_n, P.Gtgt, P.S, g, im, qr, r2, row_span, cert, P.match, P.match_d2, P.lbe, P.match2);
}

// =================================================================================================
// host-side launch helpers
// =================================================================================================
void launch_nn_query(const float4* Gsrc, size_t n_src, const float4* Gtgt, const HashEntry* table, const GridDesc& g,
                     const InvMap& im, float r2, int* match_pos, float* match_d2, hipStream_t s) {
  if (!n_src) return;
  hipLaunchKernelGGL(k_nn_query, dim3((unsigned)div_up(n_src, kBlock)), dim3(kBlock), 0, s, Gsrc, n_src, Gtgt, table,
                     g, im, r2, match_pos, match_d2);
}

void launch_query_keys(const float4* Gsrc, size_t n, const GridDesc& g, const InvMap& im, const QueryRange& qr,
                       unsigned long long* keys, unsigned* vals, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_query_keys, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, Gsrc, n, g, im, qr, keys, vals);
}

void launch_query_keys32(const float4* Gsrc, size_t n, const GridDesc& g, const InvMap& im, const QueryRange& qr,
                         unsigned* keys, unsigned* vals, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_query_keys32, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, Gsrc, n, g, im, qr, keys, vals);
}

void launch_nn_cells(const float4* Gsrc, const unsigned* order, size_t n, const float4* Gtgt, const HashEntry* table,
                     const unsigned* dense_start, const GridDesc& g, const InvMap& im, const QueryRange& qr, float r2,
                     int* match_pos, float* match_d2, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_nn_cells, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, Gsrc, order, n, Gtgt, table,
                     dense_start, g, im, qr, r2, match_pos, match_d2);
}

static int row_span_setting() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("E3D_ROW_SPAN");      // tuning knob: x-extent (cells) of a row segment
    v = e ? atoi(e) : kRowSpan;
    if (v < 0) v = 0;
    if (v > 62) v = 62;
  }
  return v;
}

void launch_nn_rows(const float4* Gsrc, const unsigned* order, size_t n, const float4* Gtgt, const unsigned* dense_start,
                    const GridDesc& g, const InvMap& im, const QueryRange& qr, float r2, const CertParams& cert, int* match_pos,
                    float* match_d2, float* lbe, int* match2, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_nn_rows, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, Gsrc, order, n, Gtgt, dense_start,
                     g, im, qr, r2, row_span_setting(), cert, match_pos, match_d2, lbe, match2);
}

void launch_query_keys_list(const float4* Gsrc, const unsigned* list, size_t n, const GridDesc& g, const InvMap& im,
                            const QueryRange& qr, unsigned long long* keys, unsigned* vals, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_query_keys_list, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, Gsrc, list, n, g, im, qr, keys, vals);
}
void launch_query_keys32_list(const float4* Gsrc, const unsigned* list, size_t n, const GridDesc& g, const InvMap& im,
                              const QueryRange& qr, unsigned* keys, unsigned* vals, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_query_keys32_list, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, Gsrc, list, n, g, im, qr, keys, vals);
}

void launch_block_occupancy(const unsigned* dense_start, const QueryRange& qr, unsigned stride_w, unsigned* tmp, unsigned* occ, hipStream_t s) {
  const size_t rows = (size_t)qr.D[1] * qr.D[2];
  if (!rows || !stride_w) return;
  hipLaunchKernelGGL(k_occ_cells, dim3((unsigned)div_up(rows * stride_w * 32u, kBlock)), dim3(kBlock), 0, s, dense_start, qr, stride_w, tmp);
  hipLaunchKernelGGL(k_occ_dilate, dim3((unsigned)div_up(rows * stride_w, kBlock)), dim3(kBlock), 0, s, (const unsigned*)tmp, qr.D[1], qr.D[2], stride_w, occ);
}

void launch_query_keys_prune(bool keys32, const float4* Gsrc, const unsigned* list, size_t n, const unsigned* occ, unsigned stride_w, const GridDesc& g,
                             const InvMap& im, const QueryRange& qr, float r2, const CertParams& cert, void* keys, unsigned* vals, unsigned* count,
                             int* match, int* match2, float* match_d2, float* lbe, bool from_state, hipStream_t s) {
  if (!n) return;
  const dim3 grid((unsigned)div_up(n, (size_t)kPruneBlock));
  const int fs = (from_state && !list) ? 1 : 0;
  if (keys32)
    hipLaunchKernelGGL(k_query_keys_prune<unsigned>, grid, dim3(kBlock), 0, s, Gsrc, list, n, occ, stride_w, g, im, qr, r2, cert,
                       (unsigned*)keys, vals, count, match, match2, match_d2, lbe, fs);
  else
    hipLaunchKernelGGL(k_query_keys_prune<unsigned long long>, grid, dim3(kBlock), 0, s, Gsrc, list, n, occ, stride_w, g, im, qr, r2, cert,
                       (unsigned long long*)keys, vals, count, match, match2, match_d2, lbe, fs);
}

void launch_half_keys(const float* xyz, size_t n, const GridDesc& g, unsigned* keys, unsigned* vals, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_half_keys, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, xyz, n, g, keys, vals);
}
void launch_cell_keys_ordered(const float* xyz, const unsigned* order, size_t n, const GridDesc& g, unsigned long long* keys, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_cell_keys_ordered, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, xyz, order, n, g, keys);
}
void launch_half_prefix(const unsigned long long* keys, const float4* L4, size_t n, const GridDesc& g, const QueryRange& qr,
                        const unsigned* dense_start, unsigned long long* half_prefix, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_half_ends, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, keys, L4, n, g, qr, dense_start,
                     reinterpret_cast<unsigned char*>(half_prefix));
  hipLaunchKernelGGL(k_half_fix, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, keys, n, qr, dense_start, half_prefix);
}

// Filter constants of k_nn_mfma for a target grid (cell = local cell size, sigma_max = largest singular value of the
// target's local -> global linear part).  Returns false if no valid scale exists (the caller uses k_nn_rows).
// Geometry (segment origin = midpoint of the first and last query; rs = row span in cells): a candidate lies within
// sqrt((rs/2 + 2)^2 + 8) cells of the origin, a query within sqrt((rs/2 + 1)^2 + 2) cells (2 % margin for the f32 cell mapping).
bool mfma_filter_params(double cell, double sigma_max, int row_span, float r2, MfParams* P) {
  const double rs = (double)row_span;
  const double ext_c = 1.02 * sigma_max * cell * std::sqrt((0.5 * rs + 2.0) * (0.5 * rs + 2.0) + 8.0);
  const double ext_q = 1.02 * sigma_max * cell * std::sqrt((0.5 * rs + 1.0) * (0.5 * rs + 1.0) + 2.0);
  if (!(ext_c > 0) || !std::isfinite(ext_c)) return false;
  const int e = (int)std::floor(std::log2(31.0 / ext_c));
  if (e < -100 || e > 100) return false;
  const double S = std::ldexp(1.0, e);
  const double Mc = ext_c * S, Mq = ext_q * S;                     // <= 31: f16 ulp <= 2^-6 for the hi parts
  const double r2s = (double)r2 * S * S;
  if (!(r2s < 3.0e4) || !(r2s > 1e-30)) return false;
  auto ulp16 = [](double v) { return std::ldexp(1.0, (int)std::floor(std::log2(std::max(v, 1e-30))) - 10); };
  const double u = std::ldexp(1.0, -24);
  const double sum_abs = 2.0 * Mq * Mc * (1.0 + std::ldexp(1.0, -8)) + Mc * Mc + Mq * Mq;
  // accumulation of 16 products in f32 + rounding of the two norms (5 ops each) + residual of their hi/lo split
  // (rtz: below one ulp of the lo part) + f32 rounding of the exact scaled d2; factor 3 for the unspecified internal
  // rounding of the matrix core
  const double eta = 3.0 * (16.0 * u * sum_abs + 6.0 * u * (Mc * Mc + Mq * Mq) + std::ldexp(1.0, -10) * (ulp16(Mc * Mc) + ulp16(Mq * Mq)) +
                            4.0 * u * (r2s + Mc * Mc)) + 1e-6;
  // coordinate representation: f32 rounding of (p - o) (<= 2^-24 * 32) + residual of the rtz hi/lo split, at worst a
  // flushed f16 denormal (2^-14); per point sqrt(3) x that, two points
  const double delta = 2.0 * std::sqrt(3.0) * (std::ldexp(1.0, -14) + 32.0 * u + std::ldexp(1.0, -16));
  P->S = (float)S;
  P->r2s = (float)(r2s * (1.0 + 1e-6));
  P->eta2 = (float)(2.0 * eta);
  P->delta4 = (float)(4.0 * delta);
  P->delta4sq = (float)(4.0 * delta * delta);
  return true;
}

void launch_nn_mfma(const float4* Gsrc, const unsigned* order, size_t n, const float4* Gtgt, const unsigned* dense_start,
                    const GridDesc& g, const InvMap& im, const QueryRange& qr, float r2, const MfParams& P, int* match_pos,
                    float* match_d2, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_nn_mfma, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, Gsrc, order, n, Gtgt, dense_start,
                     g, im, qr, r2, row_span_setting(), P, match_pos, match_d2);
}
int nn_row_span() { return row_span_setting(); }

void launch_dense_counts(const unsigned long long* keys, size_t n, const QueryRange& qr, unsigned* counts, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_dense_counts, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, keys, n, qr, counts);
}

void launch_query_keys_multi(bool keys32, const NnBatchDev* batch, unsigned n_blocks, float r2, void* keys, unsigned* vals, unsigned* counts, hipStream_t s) {
  if (!n_blocks) return;
  if (keys32) hipLaunchKernelGGL(k_query_keys_multi<unsigned>, dim3(n_blocks), dim3(kBlock), 0, s, batch, r2, (unsigned*)keys, vals, counts);
  else hipLaunchKernelGGL(k_query_keys_multi<unsigned long long>, dim3(n_blocks), dim3(kBlock), 0, s, batch, r2, (unsigned long long*)keys, vals, counts);
}
void launch_nn_rows_multi(const NnBatchDev* batch, unsigned n_blocks, const unsigned* order, float r2, hipStream_t s) {
  if (!n_blocks) return;
  hipLaunchKernelGGL(k_nn_rows_multi, dim3(n_blocks), dim3(kBlock), 0, s, batch, order, r2, row_span_setting());
}
}  // namespace e3d
