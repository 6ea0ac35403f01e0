// e3d_icp_certify.hip -- ICP, search phase after the first outer iteration (gfx950 / CDNA4, wave64): the certificates that
// settle a query on its old partner (k_nn_certify), the bounded search around an old partner over cells and half cells
// (k_nn_bounded, k_nn_bounded_half) and the seeding key kernel of the far lists (k_query_seed_multi), each with its batch form.
// The searches these fall back on (k_nn_rows, the pruning key kernels) are e3d_icp_kernels.hip.
//
// Reference loops covered: a5 (1-NN within radius), incrementally.
#include <cstdlib>

#include "e3d_icp_device.hpp"

#pragma clang fp contract(off)

namespace e3d {

// -------------------------------------------------------------------------------------------------
// Certificates: is last outer iteration's partner provably still the unique nearest neighbour within the radius?
//
// State of query j of a directed pair (source order): match[j] = partner position m in the target arrays (or -1) and
// lbe[j] = LB + cum(s), where at the query's last search (outer iteration s) every target point other than m was at (true
// Euclidean) distance >= LB of the query in the global frame, and cum(.) is the host's running bound of how far any point of
// either cloud has moved since -- round 5: of how far THIS query has moved relative to the target, a rho + b (MotionBound; cum_up adds
// the f32 rounding of the transforms).  Triangle inequality: now every other point is at distance >= thr = lbe - cum_up.  If the partner's new f32 squared distance v
// is < thr^2 (with room for the f32 evaluation error of the others' distances) and < r2, the exact search would return (m, v):
// nothing else can be nearer or tie.  For m = -1 "no partner" stands as long as thr^2 >= r2.  All other queries are appended
// to the todo list (in source order inside a block of 2048 queries; one atomic per block) and searched by k_nn_rows, which
// renews their state.
// -------------------------------------------------------------------------------------------------
constexpr int kCertPerWave = 512;          // consecutive queries per wave (8 steps of 64): one atomic per list and block of 2048 queries
// The state may hold a second candidate match2[j] (the runner-up of the last search, lbe then bounds everything but these two).
// Lists: todo_near = queries whose old partner is within sqrt(near2) (searched by k_nn_bounded: only the cells the ball of that
// distance touches), todo_far = all others (no partner, or a far one: sorted by target cell and searched by k_nn_rows).
// counts[0] / counts[1] = list lengths.
// (bx: the block's index among the blocks of ITS pair -- blockIdx.x for the one-pair kernel, the offset inside the pair's block range
// for the kernel that walks a batch of pairs, k_nn_certify_multi)
template <int kCertUnroll>
__device__ __forceinline__ void nn_certify_body(const unsigned bx, const float4* __restrict__ Gsrc, size_t n, const float4* __restrict__ Gtgt,
                                                const MotionBound cum_up, float r2, float near2, int none_near, int* __restrict__ match,
                                                int* __restrict__ match2, const float* __restrict__ lbe,
                                                float* __restrict__ match_d2, unsigned* __restrict__ todo_near,
                                                unsigned* __restrict__ todo_far, unsigned* __restrict__ counts,
                                                unsigned* __restrict__ upd_counts = nullptr, double* __restrict__ upd_d2 = nullptr,
                                                unsigned* __restrict__ upd_groups = nullptr, unsigned char* __restrict__ upd_done = nullptr) {
  __shared__ unsigned s_list[2][kBlock / kWave][kCertPerWave];
  __shared__ unsigned s_cnt[2][kBlock / kWave];
  __shared__ unsigned s_base[2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t j0 = ((size_t)bx * (kBlock / kWave) + (size_t)w) * kCertPerWave;
  unsigned cn = 0, cf = 0;                                     // wave-uniform
  // kCertUnroll steps at a time: the state words, the queries and the partner gathers of all of them are requested before any
  // is evaluated (the kernel is a chain match[j] -> Gtgt[m] per query; kCertUnroll chains in flight per lane)
  for (int step0 = 0; step0 < kCertPerWave / kWave; step0 += kCertUnroll) {
    size_t jj[kCertUnroll];
    bool vv[kCertUnroll];
    int mm[kCertUnroll], mm2[kCertUnroll];
    float ll[kCertUnroll];
    float4 qq[kCertUnroll], c1[kCertUnroll], c2v[kCertUnroll];
#pragma unroll
    for (int u = 0; u < kCertUnroll; ++u) {
      jj[u] = j0 + (size_t)(step0 + u) * kWave + (size_t)lane;
      vv[u] = jj[u] < n;
      const size_t js = vv[u] ? jj[u] : 0;
      mm[u] = ld_stream(match + js); mm2[u] = ld_stream(match2 + js); ll[u] = ld_stream(lbe + js); qq[u] = ld_stream(Gsrc + js);
    }
#pragma unroll
    for (int u = 0; u < kCertUnroll; ++u) {
      c1[u] = Gtgt[mm[u] >= 0 ? mm[u] : 0];
      c2v[u] = Gtgt[(mm[u] >= 0 && mm2[u] >= 0) ? mm2[u] : 0];
    }
    // (round 6, upd_done != nullptr) A 256-query block of the row update whose queries are ALL settled here, none of them by its
    // runner-up, has nothing to rewrite, and its count, distance sum and active groups are known in this wave: four 64-query
    // steps = one such block, the same wave_sum over the same lanes and the same sequential sum over the four groups as
    // corr_update_body -- the same bits.  The update then skips the block on one flag instead of reading 12 B per query.
    unsigned ub_c = 0, ub_g = 0, ub_gm = 0;
    double ub_t = 0.0;
    bool ub_bad = false;
    static_assert(kCertUnroll == 4, "four steps of 64 queries = one block of the row update");
#pragma unroll
    for (int u = 0; u < kCertUnroll; ++u) {
    const size_t j = jj[u];
    const bool valid = vv[u];
    bool ok = false, near = false;
    bool swapped = false;
    float v_ok = 0.f;
    if (valid) {
      const float thr = (ll[u] - motion_up(qq[u], cum_up)) * 0.999999f;
      const float lim = thr * thr * 0.999999f;
      const int m = mm[u];
      if (m >= 0) {
        const int m2 = mm2[u];
        const float4 q = qq[u];
        const float4 c = c1[u];
        float v = sqdist_l2(q.x, q.y, q.z, c.x, c.y, c.z);
        if (m2 >= 0) {
          // two remembered candidates: the nearer one (exact (d2, original index) order) is the partner if both beat the bound
          // of everything else; the other one stays remembered
          const float4 c2 = c2v[u];
          const float v2 = sqdist_l2(q.x, q.y, q.z, c2.x, c2.y, c2.z);
          if (v2 < v || (v2 == v && __float_as_uint(c2.w) < __float_as_uint(c.w))) {
            v = v2;
            if (thr > 0.f && v < lim && v < r2) { match[j] = m2; match2[j] = m; swapped = true; }
          }
        }
        ok = (thr > 0.f) && (v < lim) && (v < r2);
        near = v < near2;
        if (ok) { st_stream(match_d2 + j, v); v_ok = v; }
      } else {
        ok = (thr > 0.f) && (lim >= r2);
        near = none_near != 0;                          // k_nn_bounded searches these beyond the radius
        st_stream(match_d2 + j, r2);                    // settled or not: what a search that finds nothing would write (k_nn_rows then skips it)
      }
    }
    const unsigned long long fn = __ballot(valid && !ok && near), ff = __ballot(valid && !ok && !near);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (valid && !ok) {
      if (near) s_list[0][w][cn + (unsigned)__popcll(fn & below)] = (unsigned)j;
      else s_list[1][w][cf + (unsigned)__popcll(ff & below)] = (unsigned)j | (mm[u] < 0 ? kListNoPartner : 0u);
    }
    cn += (unsigned)__popcll(fn); cf += (unsigned)__popcll(ff);
    if (upd_done) {
      const bool f = valid && mm[u] >= 0;
      const unsigned gc = (unsigned)__popcll(__ballot(f));
      const double gd = wave_sum((f && ok) ? (double)v_ok : 0.0);
      ub_c += gc; ub_t += gd;
      if (gc) { ++ub_g; ub_gm |= 1u << u; }
      if (__ballot(valid && (!ok || swapped))) ub_bad = true;
    }
    }
    if (upd_done) {
      const size_t blk = j0 / kBlock + (size_t)(step0 / kCertUnroll);
      if (blk < (n + kBlock - 1) / kBlock && lane == 0) {
        if (!ub_bad) { upd_counts[blk] = ub_c; upd_d2[blk] = ub_t; upd_groups[blk] = ub_g | (ub_gm << 8); }
        upd_done[blk] = ub_bad ? 0 : 1;
      }
    }
  }
  if (lane == 0) { s_cnt[0][w] = cn; s_cnt[1][w] = cf; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned tot = 0;
    for (int k = 0; k < kBlock / kWave; ++k) tot += s_cnt[threadIdx.x][k];
    s_base[threadIdx.x] = tot ? atomicAdd(&counts[threadIdx.x], tot) : 0u;
  }
  __syncthreads();
  unsigned bn = s_base[0], bf = s_base[1];
  for (int k = 0; k < w; ++k) { bn += s_cnt[0][k]; bf += s_cnt[1][k]; }
  for (unsigned i = (unsigned)lane; i < cn; i += kWave) todo_near[bn + i] = s_list[0][w][i];
  for (unsigned i = (unsigned)lane; i < cf; i += kWave) todo_far[bf + i] = s_list[1][w][i];
}

template <int kCertUnroll>
__global__ __launch_bounds__(kBlock) void k_nn_certify(const float4* __restrict__ Gsrc, size_t n, const float4* __restrict__ Gtgt,
                                                       MotionBound cum_up, float r2, float near2, int none_near, int* __restrict__ match,
                                                       int* __restrict__ match2, const float* __restrict__ lbe,
                                                       float* __restrict__ match_d2, unsigned* __restrict__ todo_near,
                                                       unsigned* __restrict__ todo_far, unsigned* __restrict__ counts) {
  nn_certify_body<kCertUnroll>(blockIdx.x, Gsrc, n, Gtgt, cum_up, r2, near2, none_near, match, match2, lbe, match_d2, todo_near, todo_far, counts);
}

__global__ __launch_bounds__(kBlock) void k_nn_certify_multi(const NnBatchDev* __restrict__ B, float r2) {
  const int p = nn_find_range(B->cert_end, B->n_pairs, blockIdx.x);
  const unsigned bx = blockIdx.x - (p ? B->cert_end[p - 1] : 0u);
  const NnPairDev& P = B->pair[p];
  nn_certify_body<4>(bx, P.Gsrc, (size_t)P.n, P.Gtgt, P.cum_up, r2, P.near2, P.none_near, P.match, P.match2, P.lbe, P.match_d2,
                     P.todo_near, P.todo_far, P.counts, P.upd_counts, P.upd_d2, P.upd_groups, P.upd_done);
}

// -------------------------------------------------------------------------------------------------
// Bounded search of the listed queries (one thread per query, no sort): the old partner at f32 squared distance d1 is still a
// candidate, so the nearest neighbour lies within d1; all target points whose squared distance is <= cover2 = (sqrt(d1) +
// margin)^2 (at most r2) lie in the cells the box [l - rho, l + rho] touches (l = query in the target's local frame, rho =
// sqrt(cover2) / sigma_min (1 + 1e-5) + slack; same completeness argument as for the 27 cells of the radius).  Those cells are
// scanned row by row -- the cells [xa, xb] of one (y, z) row are ONE run of the dense cell-start directory -- with the exact
// (d2, original index) order.  Afterwards every point other than the winner is farther than min(second smallest d2 seen,
// cover2): the next certificate.
// -------------------------------------------------------------------------------------------------
template <int LPQ>
__global__ __launch_bounds__(kBlock) void k_nn_bounded(const float4* __restrict__ Gsrc, const unsigned* __restrict__ list,
                                                       unsigned n_list, const float4* __restrict__ Gtgt, const unsigned* __restrict__ S,
                                                       GridDesc g, InvMap im, QueryRange qr, float r2, BoundParams bp,
                                                       int* __restrict__ match, int* __restrict__ match2,
                                                       float* __restrict__ match_d2, float* __restrict__ lbe) {
  // LPQ lanes per query (1 or 4): the lanes of a quad share the box and split every cell-row run -- lane k takes candidates s0 + k,
  // s0 + k + 4, ... (one 64-byte read per quad and step instead of four serial 16-byte reads per lane) -- then lane 0 merges the
  // partial top lists.  Which candidate wins does not depend on the split: distinct distances order themselves, and any exact
  // equality among the leaders (within a lane or at the merge) raises `tie`, which sends lane 0 through the exact (d2, original
  // index) scan.  Short lists are latency bound and gain from the quads (1.85 -> 1.49 ms per iteration at 2 x 50 M once the
  // poses settle); lists of millions of queries are bound by the candidate traffic and run one lane per query.
  const unsigned i = (blockIdx.x * blockDim.x + threadIdx.x) / LPQ;
  const int sub = threadIdx.x % LPQ;
  if (i >= n_list) return;
  const unsigned j = list[i] & kListIndexMask;
  const float4 q = Gsrc[j];
  const int m = match[j];
  float d1 = r2;                                     // no old partner: the whole radius (the 27 cells)
  if (m >= 0) {
    const float4 pc = Gtgt[m];
    d1 = sqdist_l2(q.x, q.y, q.z, pc.x, pc.y, pc.z);
    const int m2 = match2[j];
    if (m2 >= 0) { const float4 pc2 = Gtgt[m2]; d1 = fminf(d1, sqdist_l2(q.x, q.y, q.z, pc2.x, pc2.y, pc2.z)); }
  }
  // A query WITHOUT a partner searches radius r + np_extra: it costs little where the target is absent (a row of empty cells
  // is two directory words) and yields "nothing within r + np_extra", a certificate that outlives the next pose updates -- the
  // 27-cell block of the row kernel only certifies the distance to its faces, 1 - 1.5 cells, and most of those queries came
  // back in every outer iteration.
  const float dr = sqrtf(fminf(d1, r2)) + ((m < 0) ? bp.np_extra : bp.margin);
  const float cover2 = (d1 < r2) ? fminf(dr * dr * 1.000001f, r2) : ((m < 0) ? dr * dr * 1.000001f : r2);      // NaN distances search the whole radius too
  const float rho = sqrtf(cover2) * bp.rho_scale + bp.rho_pad;
  const float dx = q.x - im.t[0], dy = q.y - im.t[1], dz = q.z - im.t[2];
  const float lx = im.Linv[0] * dx + im.Linv[1] * dy + im.Linv[2] * dz;
  const float ly = im.Linv[3] * dx + im.Linv[4] * dy + im.Linv[5] * dz;
  const float lz = im.Linv[6] * dx + im.Linv[7] * dy + im.Linv[8] * dz;
  const int x0 = max(cell_coord(lx - rho, g.origin[0], g.inv_cell) - qr.lo[0], 0), x1 = min(cell_coord(lx + rho, g.origin[0], g.inv_cell) - qr.lo[0], (int)qr.D[0] - 1);
  const int y0 = max(cell_coord(ly - rho, g.origin[1], g.inv_cell) - qr.lo[1], 0), y1 = min(cell_coord(ly + rho, g.origin[1], g.inv_cell) - qr.lo[1], (int)qr.D[1] - 1);
  const int z0 = max(cell_coord(lz - rho, g.origin[2], g.inv_cell) - qr.lo[2], 0), z1 = min(cell_coord(lz + rho, g.origin[2], g.inv_cell) - qr.lo[2], (int)qr.D[2] - 1);
  const float kInf = __uint_as_float(0x7f800000u);
  // What the scanned box really covers: every target point outside it is at least `fd` cells away from the query in the target's
  // local frame (faces at the edge of the dense grid do not count: no point lies beyond them), i.e. at global distance >=
  // fd * cell_scale - cell_sub.  Usually more than sqrt(cover2) -- and for a query WITHOUT a partner the only way to a
  // certificate that outlives the next pose update ("nothing within more than the radius").
  float cover_box2 = 0.f;
  if (x0 <= x1 && y0 <= y1 && z0 <= z1) {
    const float ux = (lx - g.origin[0]) * g.inv_cell - (float)qr.lo[0], uy = (ly - g.origin[1]) * g.inv_cell - (float)qr.lo[1],
                uz = (lz - g.origin[2]) * g.inv_cell - (float)qr.lo[2];
    float fd = kInf;
    if (x0 > 0) fd = fminf(fd, ux - (float)x0);
    if (x1 < (int)qr.D[0] - 1) fd = fminf(fd, (float)(x1 + 1) - ux);
    if (y0 > 0) fd = fminf(fd, uy - (float)y0);
    if (y1 < (int)qr.D[1] - 1) fd = fminf(fd, (float)(y1 + 1) - uy);
    if (z0 > 0) fd = fminf(fd, uz - (float)z0);
    if (z1 < (int)qr.D[2] - 1) fd = fminf(fd, (float)(z1 + 1) - uz);
    fd = fminf(fd, 4.0f);                                   // (a box that spans the whole grid: keep the bound finite)
    const float cb = fd * bp.cell_scale - bp.cell_sub;
    cover_box2 = cb > 0.f ? cb * cb : 0.f;
  }
  const float cover_all2 = fmaxf(cover2, cover_box2);
  // fast pass over ALL scanned candidates (inside the radius or not): the two smallest distances with a strict '<' and the third
  // smallest value (`tie` is derived from the three at the end).  The radius test comes at the end.
  float bd = kInf, bd2 = kInf, b3 = kInf;
  int bpos = -1, bpos2 = -1;
  bool tie = false;
  if (x0 <= x1) {
    for (int cz = z0; cz <= z1; ++cz) {
      for (int cy = y0; cy <= y1; ++cy) {
        const size_t row = ((size_t)cz * qr.D[1] + (size_t)cy) * qr.D[0];
        const unsigned s0 = S[row + (size_t)x0], s1 = S[row + (size_t)x1 + 1];
        for (unsigned p = s0 + (unsigned)sub; p < s1; p += LPQ) {
          const float4 c = Gtgt[p];
          const float d2 = sqdist_l2(q.x, q.y, q.z, c.x, c.y, c.z);
          const bool lt1 = d2 < bd, lt2 = d2 < bd2;
          b3 = fminf(b3, fmaxf(d2, bd2));                 // the displaced runner-up, or this candidate
          bd2 = fminf(fmaxf(d2, bd), bd2);
          bpos2 = lt1 ? bpos : (lt2 ? (int)p : bpos2);
          bd = fminf(d2, bd);
          bpos = lt1 ? (int)p : bpos;
        }
      }
    }
  }
  // merge the quad's partial lists into lane 0's (the other lanes' best and second best enter like candidates, their third
  // smallest value only bounds)
#pragma unroll
  for (int l = 1; l < LPQ; ++l) {
    const float obd = __shfl(bd, l, LPQ), obd2 = __shfl(bd2, l, LPQ), ob3 = __shfl(b3, l, LPQ);
    const int opos = __shfl(bpos, l, LPQ), opos2 = __shfl(bpos2, l, LPQ);
    if (sub == 0) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float d2 = t == 0 ? obd : obd2;
        const int p = t == 0 ? opos : opos2;
        if (p >= 0) {
          const bool lt1 = d2 < bd, lt2 = d2 < bd2;
          b3 = fminf(b3, fmaxf(d2, bd2));
          bd2 = fminf(fmaxf(d2, bd), bd2);
          bpos2 = lt1 ? bpos : (lt2 ? p : bpos2);
          bd = fminf(d2, bd);
          bpos = lt1 ? p : bpos;
        }
      }
      b3 = fminf(b3, ob3);
    }
  }
  if (sub != 0) return;
  // The three smallest distances are an exact multiset (strict '<' updates keep equal values side by side), so an exact f32
  // equality that could change the winner or the runner-up shows as bd == bd2 or bd2 == b3 at the end -- no per-candidate test.
  tie = (bd == bd2 && bd < kInf) || (bd2 == b3 && bd2 < kInf);
  if (tie) {
    // rare (lattices, duplicates): the same cells again with the full (d2, original index) order
    bd = kInf; bd2 = kInf; b3 = kInf; bpos = -1; bpos2 = -1;
    unsigned boi = 0u, boi2 = 0u;
    for (int cz = z0; cz <= z1; ++cz) {
      for (int cy = y0; cy <= y1; ++cy) {
        const size_t row = ((size_t)cz * qr.D[1] + (size_t)cy) * qr.D[0];
        const unsigned s0 = S[row + (size_t)x0], s1 = S[row + (size_t)x1 + 1];
        for (unsigned p = s0; p < s1; ++p) {
          const float4 c = Gtgt[p];
          const float d2 = sqdist_l2(q.x, q.y, q.z, c.x, c.y, c.z);
          const unsigned oi = __float_as_uint(c.w);
          if (d2 < bd || (d2 == bd && oi < boi)) {
            b3 = fminf(b3, bd2); bd2 = bd; boi2 = boi; bpos2 = bpos; bd = d2; boi = oi; bpos = (int)p;
          } else if (d2 < bd2 || (d2 == bd2 && oi < boi2)) {
            b3 = fminf(b3, bd2); bd2 = d2; boi2 = oi; bpos2 = (int)p;
          } else {
            b3 = fminf(b3, d2);
          }
        }
      }
    }
  }
  const bool has1 = bd < r2, has2 = bd2 < r2;            // NaN distances compare false: no partner
  match[j] = has1 ? bpos : -1;
  match2[j] = has2 ? bpos2 : -1;
  match_d2[j] = has1 ? bd : r2;
  // everything but the remembered candidates is at least this far: the third smallest distance (two remembered), the second
  // (partner only), the smallest (no partner within the radius) -- and nothing is known beyond what the scanned box covers
  const float others2 = has2 ? b3 : (has1 ? bd2 : bd);
  lbe[j] = sqrtf(fminf(others2, cover_all2)) * 0.999999f + motion_lo(q, bp.lo);
}

// -------------------------------------------------------------------------------------------------
// The bounded search over HALF cells (targets with a half-cell directory: dense scans).  Same contract as k_nn_bounded, one lane
// per query.  The box [l - rho, l + rho] is taken in half-cell coordinates; the half cells [fxa, fxb] of sub-row (fy, fz) of one
// grid cell are ONE run, found from the cell's start and its 8 prefix bytes (one 4-byte and one 8-byte load per grid cell for
// all of its sub-rows), then the candidates -- no chain of dependent lookups.  ~55 candidates instead of ~180.
// -------------------------------------------------------------------------------------------------
constexpr int kHalfRuns = 18;     // run-list slots per lane in LDS: the 3 x 3 x 2 sub-rows a box of the unrolled path can touch
// BATCH = candidate gathers in flight per lane.  PACK: a run is its 4-byte start plus ONE length byte (runs of sub-cells come from
// prefix bytes, so they hold at most 255 points; a longer run -- a cell without prefixes -- sends the query to the whole-cell rows):
// 23 instead of 36 KB of LDS per block, six instead of four blocks per CU for a search that waits on memory.  Measured on the
// 2 x 50 M bench, launches of 100 / 82 / 54 / 47 M listed queries (profiles/round3_nn_half_variants.txt): <4, false> 10.5 / 8.1 /
// 5.4 / 4.7 ms, <4, true> 8.5 / 6.5 / 4.5 / 4.0, <8, true> 8.1 / 6.3 / 4.3 / 3.8 (the choice), <12, true> (87 VGPRs, five blocks)
// 8.8 / 6.8 / 4.5 / 4.0; a 14-slot list at 64 VGPRs (eight blocks, 7 - 13 spilled registers) 11.6 / 8.9 / 6.2 / 5.4: the queries
// whose box touches more sub-rows than slots pay whole-cell rows.
template <int BATCH>
__device__ __forceinline__ void nn_bounded_half_body(const unsigned bx, const float4* __restrict__ Gsrc, const unsigned* __restrict__ list,
                                                     unsigned n_list, const float4* __restrict__ Gtgt, const unsigned* __restrict__ S,
                                                     const unsigned long long* __restrict__ H8,
                                                     const GridDesc& g, const InvMap& im, const QueryRange& qr, float r2, const BoundParams& bp,
                                                     int* __restrict__ match, int* __restrict__ match2,
                                                     float* __restrict__ match_d2, float* __restrict__ lbe) {
  // per lane: the non-empty candidate runs of its box, a 4-byte start and ONE length byte each
  __shared__ unsigned s_runs[kHalfRuns][kBlock];
  __shared__ unsigned char s_len[kHalfRuns][kBlock];
  const unsigned i = bx * blockDim.x + threadIdx.x;
  if (i >= n_list) return;
  const unsigned j = list[i] & kListIndexMask;
  const float4 q = Gsrc[j];
  const int m = match[j];
  float d1 = r2;                                     // no old partner
  if (m >= 0) {
    const float4 pc = Gtgt[m];
    d1 = sqdist_l2(q.x, q.y, q.z, pc.x, pc.y, pc.z);
    const int m2 = match2[j];
    if (m2 >= 0) { const float4 pc2 = Gtgt[m2]; d1 = fminf(d1, sqdist_l2(q.x, q.y, q.z, pc2.x, pc2.y, pc2.z)); }
  }
  const float dr = sqrtf(fminf(d1, r2)) + ((m < 0) ? bp.np_extra : bp.margin);
  const float cover2 = (d1 < r2) ? fminf(dr * dr * 1.000001f, r2) : ((m < 0) ? dr * dr * 1.000001f : r2);      // as k_nn_bounded
  const float rho = sqrtf(cover2) * bp.rho_scale + bp.rho_pad;
  const float dx = q.x - im.t[0], dy = q.y - im.t[1], dz = q.z - im.t[2];
  const float lx = im.Linv[0] * dx + im.Linv[1] * dy + im.Linv[2] * dz;
  const float ly = im.Linv[3] * dx + im.Linv[4] * dy + im.Linv[5] * dz;
  const float lz = im.Linv[6] * dx + im.Linv[7] * dy + im.Linv[8] * dz;
  const float inv_h = 2.f * g.inv_cell;
  const int NX = 2 * (int)qr.D[0], NY = 2 * (int)qr.D[1], NZ = 2 * (int)qr.D[2];
  const int FX0 = max(cell_coord(lx - rho, g.origin[0], inv_h) - 2 * qr.lo[0], 0), FX1 = min(cell_coord(lx + rho, g.origin[0], inv_h) - 2 * qr.lo[0], NX - 1);
  const int FY0 = max(cell_coord(ly - rho, g.origin[1], inv_h) - 2 * qr.lo[1], 0), FY1 = min(cell_coord(ly + rho, g.origin[1], inv_h) - 2 * qr.lo[1], NY - 1);
  const int FZ0 = max(cell_coord(lz - rho, g.origin[2], inv_h) - 2 * qr.lo[2], 0), FZ1 = min(cell_coord(lz + rho, g.origin[2], inv_h) - 2 * qr.lo[2], NZ - 1);
  const float kInf = __uint_as_float(0x7f800000u);
  // what the scanned box covers: every target point outside it is at least `fd` HALF cells away in the target's local frame
  // (faces at the edge of the dense grid do not count), i.e. at global distance >= fd * cell_scale / 2 - cell_sub
  float cover_box2 = 0.f;
  const bool any = FX0 <= FX1 && FY0 <= FY1 && FZ0 <= FZ1;
  if (any) {
    const float ux = (lx - g.origin[0]) * inv_h - (float)(2 * qr.lo[0]), uy = (ly - g.origin[1]) * inv_h - (float)(2 * qr.lo[1]),
                uz = (lz - g.origin[2]) * inv_h - (float)(2 * qr.lo[2]);
    float fd = kInf;
    if (FX0 > 0) fd = fminf(fd, ux - (float)FX0);
    if (FX1 < NX - 1) fd = fminf(fd, (float)(FX1 + 1) - ux);
    if (FY0 > 0) fd = fminf(fd, uy - (float)FY0);
    if (FY1 < NY - 1) fd = fminf(fd, (float)(FY1 + 1) - uy);
    if (FZ0 > 0) fd = fminf(fd, uz - (float)FZ0);
    if (FZ1 < NZ - 1) fd = fminf(fd, (float)(FZ1 + 1) - uz);
    fd = fminf(fd, 8.0f);                                   // (a box that spans the whole grid: keep the bound finite)
    const float cb = fd * (bp.cell_scale * 0.5f) - bp.cell_sub;
    cover_box2 = cb > 0.f ? cb * cb : 0.f;
  }
  const float cover_all2 = fmaxf(cover2, cover_box2);
  float bd = kInf, bd2 = kInf, b3 = kInf;
  int bpos = -1, bpos2 = -1;
  // The search is latency bound, not arithmetic bound, once the candidates are few: (1) ALL directory words of the box are
  // requested before any is used -- the usual box is at most 3 x 3 half-cell rows by 2 grid cells in x, unrolled with clamped
  // addresses (larger boxes, rare, loop) -- and the non-empty runs go to a per-lane list in LDS; (2) the candidates of all runs
  // are then walked as ONE sequence, BATCH gathers in flight.
  const int cx0 = FX0 >> 1, cx1 = FX1 >> 1;
  int nr = 0;
#define RUN_S(i) s_runs[(i)][threadIdx.x]
#define RUN_LEN(i) s_len[(i)][threadIdx.x]
#define RUN_E(i) (RUN_S(i) + (unsigned)RUN_LEN(i))
  if (any) {
    const int nz = FZ1 - FZ0 + 1, ny = FY1 - FY0 + 1, nx = cx1 - cx0 + 1;
    if (nz <= 3 && ny <= 3 && nx <= 2) {
      // the (at most 2 x 2 x 2) grid cells of the box: cell start and the 8 prefix bytes, all requested at once
      const int gz0 = FZ0 >> 1, gy0 = FY0 >> 1;
      unsigned cs[8];
      unsigned long long ce[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int gz = min(gz0 + (t >> 2), FZ1 >> 1), gy = min(gy0 + ((t >> 1) & 1), FY1 >> 1), cx = min(cx0 + (t & 1), cx1);
        const size_t lin = ((size_t)gz * qr.D[1] + (size_t)gy) * qr.D[0] + (size_t)cx;
        cs[t] = S[lin];
        ce[t] = H8[lin];
      }
      // Cell by cell (compile-time cell index: no selection among the loaded words), the up to four sub-rows (z half, y half) of
      // a cell inside the box: bytes of the prefix word at compile-time positions, chosen by the x range.  A cell of more than
      // 255 points has no prefixes (all ones): the whole-cell rows below take the query.
      const int dz = (FZ1 >> 1) - gz0, dy = (FY1 >> 1) - gy0, dxc = cx1 - cx0;
      bool dense = false;
#pragma unroll
      for (int t = 0; t < 8; ++t)
        dense = dense || ((t >> 2) <= dz && ((t >> 1) & 1) <= dy && (t & 1) <= dxc && ce[t] == ~0ull);
      if (dense) {
        nr = -1;
      } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if ((t >> 2) <= dz && ((t >> 1) & 1) <= dy && (t & 1) <= dxc) {
            const int cz2 = 2 * (gz0 + (t >> 2)), cy2 = 2 * (gy0 + ((t >> 1) & 1)), cx2 = 2 * (cx0 + (t & 1));
            const bool xa = FX0 > cx2, xb = FX1 > cx2;               // the x halves [xa, xb] of this cell lie in the box
            const unsigned st = cs[t], lo = (unsigned)ce[t], hi = (unsigned)(ce[t] >> 32);
#pragma unroll
            for (int zz = 0; zz < 2; ++zz)
#pragma unroll
              for (int yy = 0; yy < 2; ++yy) {
                if (cz2 + zz >= FZ0 && cz2 + zz <= FZ1 && cy2 + yy >= FY0 && cy2 + yy <= FY1) {
                  // codes (zz, yy, 0) = kb and kb + 1; byte k of the prefix word = points of the cell with a code <= k
                  const int kb = zz * 4 + yy * 2;
                  const unsigned w = zz ? hi : lo;
                  const unsigned e_prev = kb == 0 ? 0u : (kb == 4 ? (lo >> 24) : ((w >> (8 * ((kb & 3) - 1))) & 0xFFu));
                  const unsigned e_x0 = (w >> (8 * (kb & 3))) & 0xFFu, e_x1 = (w >> (8 * ((kb & 3) + 1))) & 0xFFu;
                  const unsigned e0 = xa ? e_x0 : e_prev, e1 = xb ? e_x1 : e_x0;
                  if (e0 < e1) {                             // at most 3 x 3 x 2 sub-rows lie in the box: the list cannot overflow
                    RUN_S(nr) = st + e0;
                    RUN_LEN(nr) = (unsigned char)(e1 - e0);
                    ++nr;
                  }
                }
              }
          }
        }
      }
    } else {
      nr = -1;                                             // a large box: the plain loops below
    }
  }
  if (nr > 0) {
    // One flat walk over the candidates of all runs, BATCH gathers in flight, without a branch: the search is bound by the
    // vector instructions it issues.  Squared distances are compared as bit patterns -- non-negative floats and +inf order like
    // unsigned integers, a NaN sorts above +inf and is never taken (as with '<' on floats), and v_min_u32 / v_max_u32 need no
    // canonicalisation of their operands; a slot past the last candidate holds +inf, which changes nothing.
    const unsigned uinf = 0x7f800000u;
    unsigned ud = uinf, ud2 = uinf, u3 = uinf;
    int r = 0;
    const int last = nr - 1;
    unsigned cur = RUN_S(0), end = RUN_E(0);
    while (r < nr) {
      unsigned p[BATCH];
      bool ok[BATCH];
#pragma unroll
      for (int t = 0; t < BATCH; ++t) {
        ok[t] = r < nr;
        p[t] = cur;                                        // (beyond the last candidate: a valid address, result ignored)
        const unsigned nx = cur + 1u;
        const bool sw = ok[t] && nx == end;                // the run ends here: the next one (or, after the last, its start again)
        r += sw ? 1 : 0;
        const int rc = min(r, last);
        const unsigned ns = RUN_S(rc), ne = ns + (unsigned)RUN_LEN(rc);
        cur = sw ? ns : (ok[t] ? nx : cur);
        end = sw ? ne : end;
      }
      float4 c4[BATCH];
#pragma unroll
      for (int t = 0; t < BATCH; ++t) c4[t] = Gtgt[p[t]];
#pragma unroll
      for (int t = 0; t < BATCH; ++t) {
        const unsigned u = ok[t] ? __float_as_uint(sqdist_l2(q.x, q.y, q.z, c4[t].x, c4[t].y, c4[t].z)) : uinf;
        const bool lt1 = u < ud, lt2 = u < ud2;
        u3 = min(u3, max(u, ud2));                         // the displaced runner-up, or this candidate
        ud2 = min(max(u, ud), ud2);
        bpos2 = lt1 ? bpos : (lt2 ? (int)p[t] : bpos2);
        ud = min(u, ud);
        bpos = lt1 ? (int)p[t] : bpos;
      }
    }
    bd = __uint_as_float(ud); bd2 = __uint_as_float(ud2); b3 = __uint_as_float(u3);
  } else if (nr < 0) {
    // a large box (a query without a partner looks np_extra beyond the radius; a partner that moved far): whole grid cells, row by
    // row -- the cells [x0, x1] of one (y, z) row are ONE run of the cell directory, and an empty row costs two words.  A superset
    // of the half cells of the box: nothing is missed, and the covered region only grows.
    for (int gz = FZ0 >> 1; gz <= (FZ1 >> 1); ++gz)
      for (int gy = FY0 >> 1; gy <= (FY1 >> 1); ++gy) {
        const size_t row = ((size_t)gz * qr.D[1] + (size_t)gy) * qr.D[0];
        const unsigned s0 = S[row + (size_t)cx0], s1 = S[row + (size_t)cx1 + 1];
        for (unsigned p = s0; p < s1; ++p) {
          const float4 c = Gtgt[p];
          const float d2 = sqdist_l2(q.x, q.y, q.z, c.x, c.y, c.z);
          const bool lt1 = d2 < bd, lt2 = d2 < bd2;
          b3 = fminf(b3, fmaxf(d2, bd2));
          bd2 = fminf(fmaxf(d2, bd), bd2);
          bpos2 = lt1 ? bpos : (lt2 ? (int)p : bpos2);
          bd = fminf(d2, bd);
          bpos = lt1 ? (int)p : bpos;
        }
      }
  }
  // exact f32 equalities among the three smallest: the same candidates again with the full (d2, original index) order (rare)
  if (any && ((bd == bd2 && bd < kInf) || (bd2 == b3 && bd2 < kInf))) {
    bd = kInf; bd2 = kInf; b3 = kInf; bpos = -1; bpos2 = -1;
    unsigned boi = 0u, boi2 = 0u;
    auto exact_run = [&](unsigned s0, unsigned s1) {
      for (unsigned p = s0; p < s1; ++p) {
        const float4 c = Gtgt[p];
        const float d2 = sqdist_l2(q.x, q.y, q.z, c.x, c.y, c.z);
        const unsigned oi = __float_as_uint(c.w);
        if (d2 < bd || (d2 == bd && oi < boi)) {
          b3 = fminf(b3, bd2); bd2 = bd; boi2 = boi; bpos2 = bpos; bd = d2; boi = oi; bpos = (int)p;
        } else if (d2 < bd2 || (d2 == bd2 && oi < boi2)) {
          b3 = fminf(b3, bd2); bd2 = d2; boi2 = oi; bpos2 = (int)p;
        } else {
          b3 = fminf(b3, d2);
        }
      }
    };
    if (nr >= 0) {
      for (int r = 0; r < nr; ++r) exact_run(RUN_S(r), RUN_E(r));
    } else {
      for (int gz = FZ0 >> 1; gz <= (FZ1 >> 1); ++gz)
        for (int gy = FY0 >> 1; gy <= (FY1 >> 1); ++gy) {
          const size_t row = ((size_t)gz * qr.D[1] + (size_t)gy) * qr.D[0];
          exact_run(S[row + (size_t)cx0], S[row + (size_t)cx1 + 1]);
        }
    }
  }
#undef RUN_S
#undef RUN_E
#undef RUN_LEN
  const bool has1 = bd < r2, has2 = bd2 < r2;            // NaN distances compare false: no partner
  match[j] = has1 ? bpos : -1;
  match2[j] = has2 ? bpos2 : -1;
  match_d2[j] = has1 ? bd : r2;
  const float others2 = has2 ? b3 : (has1 ? bd2 : bd);
  lbe[j] = sqrtf(fminf(others2, cover_all2)) * 0.999999f + motion_lo(q, bp.lo);
}

template <int BATCH>
__global__ __launch_bounds__(kBlock) void k_nn_bounded_half(const float4* __restrict__ Gsrc, const unsigned* __restrict__ list,
                                                            unsigned n_list, const float4* __restrict__ Gtgt, const unsigned* __restrict__ S,
                                                            const unsigned long long* __restrict__ H8,
                                                            GridDesc g, InvMap im, QueryRange qr, float r2, BoundParams bp,
                                                            int* __restrict__ match, int* __restrict__ match2,
                                                            float* __restrict__ match_d2, float* __restrict__ lbe) {
  nn_bounded_half_body<BATCH>(blockIdx.x, Gsrc, list, n_list, Gtgt, S, H8, g, im, qr, r2, bp, match, match2, match_d2, lbe);
}

// the listed queries of a batch of pairs: one job per (pair, list) -- the near list and, when it is short, the far list of a pair
// are disjoint sets of queries and run side by side
__global__ __launch_bounds__(kBlock) void k_nn_bounded_half_multi(const NnBatchDev* __restrict__ B, float r2) {
  const int jb = nn_find_range(B->job_end, B->n_jobs, blockIdx.x);
  const unsigned bx = blockIdx.x - (jb ? B->job_end[jb - 1] : 0u);
  const int p = __builtin_amdgcn_readfirstlane(B->job_pair[jb]);
  const NnPairDev& P = B->pair[p];
  const GridDesc g = P.g; const InvMap im = P.im; const QueryRange qr = P.qr; const BoundParams bp = P.bp;      // (block-uniform: scalar registers)
  nn_bounded_half_body<8>(bx, P.Gsrc, B->job_list[jb], B->job_n[jb], P.Gtgt, P.S, P.H8, g, im, qr, r2, bp, P.match, P.match2,
                          P.match_d2, P.lbe);
}

// The far lists' key kernel WITH SEEDS (round 6).  While two scans meet, every query changes its partner: the far lists hold all
// queries, k_nn_rows scores each against the ~10^3 candidates of its row segments (12 ms per 100 M queries, after a 3.5 ms sort).
// But most of those queries have a target point a few millimetres away -- and any target point at distance s bounds the search to
// the ball of radius s, which is what the bounded search (k_nn_bounded_half) does around an OLD partner at a third of the cost.
// This kernel gives a query a partner to start from: after the occupancy test of k_query_keys_prune it probes up to eight
// points of the query's own half cell (the cell's prefix bytes; an empty half cell: points spread over the whole cell) and the old
// partner, if any.  A query with a probe (or old partner) nearer than sqrt(seed2) gets that point as match[j] and goes to the
// pair's SEEDED list -- a job of the bounded search, which treats it like any near-list query (the ball around a real target point
// at its exact f32 distance: the exact search inside it finds the nearest neighbour, ties included); the others are keyed for the
// sort and k_nn_rows as before.  Results are those of either exact search: identical.
constexpr int kSeedPerThread = 4;
static_assert((unsigned)(kBlock * kSeedPerThread) == kQuerySeedBlock, "queries per block of the seeding key kernel");
template <typename KeyT, int kSeedProbes>
__global__ __launch_bounds__(kBlock) void k_query_seed_multi(const NnBatchDev* __restrict__ B, float r2, KeyT* __restrict__ keys, unsigned* __restrict__ vals,
                                                             unsigned* __restrict__ counts) {
  __shared__ unsigned s_cnt[2][kBlock / kWave][kSeedPerThread];
  __shared__ unsigned s_base[2];
  const int p = nn_find_range(B->far_end, B->n_pairs, blockIdx.x);
  const unsigned bx = blockIdx.x - (p ? B->far_end[p - 1] : 0u);
  const NnPairDev& P = B->pair[p];
  const GridDesc g = P.g; const InvMap im = P.im; const QueryRange qr = P.qr;
  const CertParams cert = {P.bp.cell_scale, P.bp.cell_sub, P.bp.lo};
  const int shift = B->key_shift;
  const KeyT key_mask = (KeyT)(((KeyT)1 << shift) - (KeyT)1), key_or = (KeyT)((KeyT)p << shift);
  const int flags = __builtin_amdgcn_readfirstlane(P.far_flags);
  const bool from_state = (flags & 1) != 0, prune = (flags & 2) != 0, seed_on = (flags & 4) != 0;
  const float4* __restrict__ Gsrc = P.Gsrc; const float4* __restrict__ Gtgt = P.Gtgt;
  const unsigned* __restrict__ list = P.far_list; const unsigned* __restrict__ occ = P.occ; const unsigned* __restrict__ S = P.S;
  const unsigned long long* __restrict__ H8 = P.H8;
  int* __restrict__ match = P.match; int* __restrict__ match2 = P.match2; float* __restrict__ match_d2 = P.match_d2; float* __restrict__ lbe = P.lbe;
  const size_t n = (size_t)P.far_n;
  const unsigned stride_w = P.occ_stride;
  const float seed2 = P.seed2;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t i0 = (size_t)bx * (kBlock * kSeedPerThread) + (size_t)w * kWave + (size_t)lane;      // step u: + u * kBlock
  KeyT kk[kSeedPerThread];
  unsigned jf[kSeedPerThread];
  float4 qq[kSeedPerThread];
  unsigned long long keyed_mask[kSeedPerThread], seeded_mask[kSeedPerThread];       // wave-uniform ballots
#pragma unroll
  for (int u = 0; u < kSeedPerThread; ++u) {
    const size_t i = i0 + (size_t)u * kBlock;
    jf[u] = (i < n) ? (list ? list[i] : ((unsigned)i | ((from_state && match[i] < 0) ? kListNoPartner : 0u))) : 0u;
  }
#pragma unroll
  for (int u = 0; u < kSeedPerThread; ++u) qq[u] = Gsrc[jf[u] & kListIndexMask];
  unsigned wordv[kSeedPerThread];
  int bitv[kSeedPerThread];
  float bdist[kSeedPerThread];
  unsigned long long lin[kSeedPerThread];
  unsigned code[kSeedPerThread];
#pragma unroll
  for (int u = 0; u < kSeedPerThread; ++u) {
    const float4 q = qq[u];
    const float dx = q.x - im.t[0], dy = q.y - im.t[1], dz = q.z - im.t[2];
    const float lx = im.Linv[0] * dx + im.Linv[1] * dy + im.Linv[2] * dz;
    const float ly = im.Linv[3] * dx + im.Linv[4] * dy + im.Linv[5] * dz;
    const float lz = im.Linv[6] * dx + im.Linv[7] * dy + im.Linv[8] * dz;
    int cx = 0, cy = 0, cz = 0;
    bdist[u] = 2.0f;
    lin[u] = query_cell_key(q, im, g, qr, cx, cy, cz, &bdist[u]);
    code[u] = half_code(lx, ly, lz, g);
    kk[u] = ((KeyT)lin[u] & key_mask) | key_or;
    wordv[u] = 0u; bitv[u] = -1;
    if (lin[u] != kEmptyKey) {
      if (prune) {
        const int kx = cx - qr.lo[0], ky = cy - qr.lo[1], kz = cz - qr.lo[2];
        wordv[u] = occ[((size_t)kz * qr.D[1] + (size_t)ky) * stride_w + (size_t)(kx >> 5)];
        bitv[u] = kx & 31;
      }
    } else {
      bdist[u] = 2.0f;                                   // outside the directory range: two empty cells all around (k_nn_rows)
    }
  }
  // the own cell's run and prefix bytes, the old partner: requested for all steps before any is used
  bool keep[kSeedPerThread];
  unsigned s0[kSeedPerThread], s1[kSeedPerThread];
  unsigned long long h8[kSeedPerThread];
  int mm[kSeedPerThread];
#pragma unroll
  for (int u = 0; u < kSeedPerThread; ++u) {
    const size_t i = i0 + (size_t)u * kBlock;
    const bool valid = i < n;
    keep[u] = valid && (prune ? (bitv[u] >= 0 && ((wordv[u] >> bitv[u]) & 1u)) : true);
    const bool probe = keep[u] && seed_on && lin[u] != kEmptyKey;
    const size_t l = probe ? (size_t)lin[u] : 0;
    s0[u] = S[l]; s1[u] = S[l + 1];
    h8[u] = H8[l];
    mm[u] = probe ? match[jf[u] & kListIndexMask] : -1;
    if (!probe) { s0[u] = 0u; s1[u] = 0u; }
  }
#pragma unroll
  for (int u = 0; u < kSeedPerThread; ++u) {
    const size_t i = i0 + (size_t)u * kBlock;
    const bool valid = i < n;
    const unsigned j = jf[u] & kListIndexMask;
    const float4 q = qq[u];
    if (valid && from_state && (jf[u] & kListNoPartner)) match_d2[j] = r2;
    if (valid && !keep[u]) {
      if (!(jf[u] & kListNoPartner)) {                   // (see k_nn_rows: a query that had no partner holds these values already)
        match[j] = -1; match_d2[j] = r2;
        if (match2) match2[j] = -1;
      }
      const float kInf = __uint_as_float(0x7f800000u);
      const float lb_out = bdist[u] * cert.cell_scale - cert.cell_sub;
      lbe[j] = fmaxf(fminf(sqrtf(kInf), lb_out), 0.0f) * 0.999999f + motion_lo(q, cert.lo);
    }
    // probes: the own half cell's run, else the whole cell
    unsigned a = s0[u], b = s1[u];
    if (h8[u] != ~0ull && b > a) {
      const unsigned c = code[u];
      const unsigned e_hi = (unsigned)(h8[u] >> (8 * c)) & 0xFFu, e_lo = c ? ((unsigned)(h8[u] >> (8 * (c - 1))) & 0xFFu) : 0u;
      if (e_hi > e_lo) { b = a + e_hi; a = a + e_lo; }
    }
    const unsigned len = b - a;
    float4 c4[kSeedProbes];
    unsigned pp[kSeedProbes];
#pragma unroll
    for (int t = 0; t < kSeedProbes; ++t) {
      const unsigned o = len > (unsigned)kSeedProbes ? ((unsigned)t * len) / (unsigned)kSeedProbes : min((unsigned)t, len ? len - 1u : 0u);
      pp[t] = a + o;                                     // (no point in the cell: len = 0, position a = 0: a valid address, result ignored)
      c4[t] = Gtgt[pp[t]];
    }
    const float4 co = Gtgt[mm[u] >= 0 ? mm[u] : 0];
    const unsigned uinf = 0x7f800000u;
    unsigned ub = uinf;
    int bpos = -1;
#pragma unroll
    for (int t = 0; t < kSeedProbes; ++t) {
      const unsigned ud = len ? __float_as_uint(sqdist_l2(q.x, q.y, q.z, c4[t].x, c4[t].y, c4[t].z)) : uinf;     // (bit patterns: as k_nn_bounded_half)
      bpos = ud < ub ? (int)pp[t] : bpos;
      ub = min(ud, ub);
    }
    const unsigned uo = mm[u] >= 0 ? __float_as_uint(sqdist_l2(q.x, q.y, q.z, co.x, co.y, co.z)) : uinf;
    const unsigned us = __float_as_uint(seed2);
    const bool by_old = uo < us && uo <= ub;              // the old partner (and its runner-up) stay: the bounded search reads both
    const bool by_probe = !by_old && ub < us;
    if (by_probe) { match[j] = bpos; if (match2) match2[j] = -1; }
    const bool seeded = keep[u] && (by_old || by_probe);
    keyed_mask[u] = __ballot(keep[u] && !seeded);
    seeded_mask[u] = __ballot(seeded);
    if (lane == 0) { s_cnt[0][w][u] = (unsigned)__popcll(keyed_mask[u]); s_cnt[1][w][u] = (unsigned)__popcll(seeded_mask[u]); }
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int k = threadIdx.x;
    unsigned tot = 0u;
    for (int ww = 0; ww < kBlock / kWave; ++ww)
      for (int u = 0; u < kSeedPerThread; ++u) tot += s_cnt[k][ww][u];
    // counts[0]: keyed pairs of the batch (the sort's size), counts[1 + p]: of this pair, counts[1 + kNnBatchPairs + p]: seeded
    s_base[k] = 0u;
    if (tot) {
      if (k == 0) { s_base[0] = atomicAdd(counts, tot); atomicAdd(counts + 1 + p, tot); }
      else s_base[1] = atomicAdd(counts + 1 + kNnBatchPairs + p, tot);
    }
  }
  __syncthreads();
  unsigned offk = s_base[0], offs = s_base[1];
  for (int ww = 0; ww < w; ++ww)
#pragma unroll
    for (int u = 0; u < kSeedPerThread; ++u) { offk += s_cnt[0][ww][u]; offs += s_cnt[1][ww][u]; }
  unsigned* __restrict__ seed_list = P.seed_list;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int u = 0; u < kSeedPerThread; ++u) {
    if ((keyed_mask[u] >> lane) & 1ull) {
      const unsigned slot = offk + (unsigned)__popcll(keyed_mask[u] & below);
      keys[slot] = kk[u];
      vals[slot] = jf[u];
    }
    if ((seeded_mask[u] >> lane) & 1ull) seed_list[offs + (unsigned)__popcll(seeded_mask[u] & below)] = jf[u] & kListIndexMask;
    offk += (unsigned)__popcll(keyed_mask[u]);
    offs += (unsigned)__popcll(seeded_mask[u]);
  }
}

// =================================================================================================
// host-side launch helpers
// =================================================================================================
void launch_nn_certify(const float4* Gsrc, size_t n, const float4* Gtgt, const MotionBound& cum_up, float r2, float near2, bool none_near, int* match, int* match2,
                       const float* lbe, float* match_d2, unsigned* todo_near, unsigned* todo_far, unsigned* counts, hipStream_t s) {
  if (!n) return;
  // four query chains in flight per lane: 0.58 / 0.56 / 0.53 ms per 50 M queries with 1 / 2 / 4
  hipLaunchKernelGGL(k_nn_certify<4>, dim3((unsigned)div_up(n, (size_t)kCertPerWave * (kBlock / kWave))), dim3(kBlock), 0, s, Gsrc, n, Gtgt,
                     cum_up, r2, near2, none_near ? 1 : 0, match, match2, lbe, match_d2, todo_near, todo_far, counts);
}

void launch_nn_bounded(const float4* Gsrc, const unsigned* list, size_t n_list, const float4* Gtgt, const unsigned* dense_start,
                       const unsigned long long* half_prefix, bool half_always, const GridDesc& g, const InvMap& im, const QueryRange& qr, float r2,
                       const BoundParams& bp, int* match, int* match2, float* match_d2, float* lbe, hipStream_t s) {
  if (!n_list) return;
  static const size_t quad_limit = [] { const char* e = getenv("E3D_NN_QUAD_LIMIT"); return e ? (size_t)atoll(e) : (size_t)12000000; }();
  static const size_t half_min = [] { const char* e = getenv("E3D_NN_HALF_MIN"); return e ? (size_t)atoll(e) : (size_t)200000; }();
  if (half_prefix && (half_always || n_list >= half_min)) {
    // long lists are bound by the candidates they evaluate: the half-cell directory cuts those to a third
    hipLaunchKernelGGL((k_nn_bounded_half<8>), dim3((unsigned)div_up(n_list, kBlock)), dim3(kBlock), 0, s, Gsrc, list, (unsigned)n_list,
                       Gtgt, dense_start, half_prefix, g, im, qr, r2, bp, match, match2, match_d2, lbe);
    return;
  }
  if (n_list <= quad_limit)
    hipLaunchKernelGGL(k_nn_bounded<4>, dim3((unsigned)div_up(4 * n_list, kBlock)), dim3(kBlock), 0, s, Gsrc, list, (unsigned)n_list, Gtgt,
                       dense_start, g, im, qr, r2, bp, match, match2, match_d2, lbe);
  else
    hipLaunchKernelGGL(k_nn_bounded<1>, dim3((unsigned)div_up(n_list, kBlock)), dim3(kBlock), 0, s, Gsrc, list, (unsigned)n_list, Gtgt,
                       dense_start, g, im, qr, r2, bp, match, match2, match_d2, lbe);
}

void launch_nn_certify_multi(const NnBatchDev* batch, unsigned n_blocks, float r2, hipStream_t s) {
  static_assert(kNnCertBlockQueries == kCertPerWave * (kBlock / kWave), "queries per certificate block");
  if (!n_blocks) return;
  hipLaunchKernelGGL(k_nn_certify_multi, dim3(n_blocks), dim3(kBlock), 0, s, batch, r2);
}
void launch_nn_bounded_half_multi(const NnBatchDev* batch, unsigned n_blocks, float r2, hipStream_t s) {
  if (!n_blocks) return;
  hipLaunchKernelGGL(k_nn_bounded_half_multi, dim3(n_blocks), dim3(kBlock), 0, s, batch, r2);
}

void launch_query_seed_multi(bool keys32, const NnBatchDev* batch, unsigned n_blocks, float r2, void* keys, unsigned* vals, unsigned* counts, hipStream_t s) {
  if (!n_blocks) return;
  static const int probes = [] { const char* e = getenv("E3D_NN_SEED_PROBES"); return e ? atoi(e) : 8; }();      // (4 or 8 probes per query: experiments)
  if (probes == 4) {
    if (keys32) hipLaunchKernelGGL((k_query_seed_multi<unsigned, 4>), dim3(n_blocks), dim3(kBlock), 0, s, batch, r2, (unsigned*)keys, vals, counts);
    else hipLaunchKernelGGL((k_query_seed_multi<unsigned long long, 4>), dim3(n_blocks), dim3(kBlock), 0, s, batch, r2, (unsigned long long*)keys, vals, counts);
  } else {
    if (keys32) hipLaunchKernelGGL((k_query_seed_multi<unsigned, 8>), dim3(n_blocks), dim3(kBlock), 0, s, batch, r2, (unsigned*)keys, vals, counts);
    else hipLaunchKernelGGL((k_query_seed_multi<unsigned long long, 8>), dim3(n_blocks), dim3(kBlock), 0, s, batch, r2, (unsigned long long*)keys, vals, counts);
  }
}

}  // namespace e3d
