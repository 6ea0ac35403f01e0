// e3d_icp_rows.hip -- ICP, correspondence-row bookkeeping (gfx950 / CDNA4, wave64): match counts and distance sums with
// their three-step scan (launch_match_scan), the compacted rows (k_compact_corr), the source views and the resident rows with
// their group lists (k_source_view, k_corr_update, the totals), each with its batch form, and the gathers back to original order.
//
// Correspondences of all directed pairs of a rank, concatenated (three float4 planes, 48 B each):
//   A = {sp.x, sp.y, sp.z, sn.x}  B = {sn.y, sn.z, tp.x, tp.y}  C = {tp.z, tn.x, tn.y, tn.z}
// so that every LM pass is a pure coalesced 16 B/lane stream.
//
// Reference loops covered: a6 (count / distance sum).
#include "e3d_icp_device.hpp"

#pragma clang fp contract(off)

namespace e3d {

// flags -> per-block counts (first stage of the order-preserving compaction)
__global__ __launch_bounds__(kBlock) void k_match_block_counts(const int* __restrict__ match_pos, size_t n,
                                                               unsigned* __restrict__ block_counts,
                                                               double* __restrict__ block_d2,
                                                               const float* __restrict__ match_d2) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool f = (j < n) && (ld_stream(match_pos + j) >= 0);
  const unsigned long long b = __ballot(f);
  double d = (f && match_d2) ? (double)ld_stream(match_d2 + j) : 0.0;          // match_d2 == nullptr: counts only
  d = wave_sum(d);
  __shared__ unsigned sc[kBlock / kWave];
  __shared__ double sd[kBlock / kWave];
  if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = (unsigned)__popcll(b); sd[threadIdx.x >> 6] = d; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0; double t = 0;
    for (int k = 0; k < kBlock / kWave; ++k) { c += sc[k]; t += sd[k]; }
    block_counts[blockIdx.x] = c; block_d2[blockIdx.x] = t;
  }
}

// exclusive scan of the per-block counts in three small steps: chunk sums (kScanChunk entries per chunk),
// single-block scan of the chunk sums, per-chunk scan with its base.
constexpr int kScanChunk = 256;
__device__ __forceinline__ void scan_chunk_sums_body(const unsigned bx, const unsigned* __restrict__ counts, int nblocks,
                                                     const double* __restrict__ block_d2,
                                                     unsigned long long* __restrict__ chunk_sum,
                                                     double* __restrict__ chunk_d2,
                                                     const unsigned* __restrict__ groups,
                                                     unsigned* __restrict__ chunk_groups,
                                                     unsigned* __restrict__ chunk_rewritten) {
  const int b = (int)bx * kScanChunk + threadIdx.x;
  unsigned long long c = (b < nblocks) ? counts[b] : 0ull;
  double d = (b < nblocks) ? block_d2[b] : 0.0;
  const unsigned gw = (groups && b < nblocks) ? groups[b] : 0u;
  unsigned g = gw & 0xFFu, rw = gw >> 16;      // resident rows: active 64-row groups of the block, rows rewritten
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o, 64); d += __shfl_xor(d, o, 64); g += __shfl_xor(g, o, 64); rw += __shfl_xor(rw, o, 64); }
  __shared__ unsigned long long sc[kScanChunk / kWave];
  __shared__ double sd[kScanChunk / kWave];
  __shared__ unsigned sg[kScanChunk / kWave], sr[kScanChunk / kWave];
  if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = c; sd[threadIdx.x >> 6] = d; sg[threadIdx.x >> 6] = g; sr[threadIdx.x >> 6] = rw; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0; double td = 0; unsigned tg = 0, tr = 0;
    for (int k = 0; k < kScanChunk / kWave; ++k) { t += sc[k]; td += sd[k]; tg += sg[k]; tr += sr[k]; }
    chunk_sum[bx] = t; chunk_d2[bx] = td;
    if (chunk_groups) { chunk_groups[bx] = tg; chunk_rewritten[bx] = tr; }
  }
}

__global__ __launch_bounds__(kScanChunk) void k_scan_chunk_sums(const unsigned* __restrict__ counts, int nblocks,
                                                                const double* __restrict__ block_d2,
                                                                unsigned long long* __restrict__ chunk_sum,
                                                                double* __restrict__ chunk_d2,
                                                                const unsigned* __restrict__ groups = nullptr,
                                                                unsigned* __restrict__ chunk_groups = nullptr,
                                                                unsigned* __restrict__ chunk_rewritten = nullptr) {
  scan_chunk_sums_body(blockIdx.x, counts, nblocks, block_d2, chunk_sum, chunk_d2, groups, chunk_groups, chunk_rewritten);
}

// totals (and the exclusive scan of the chunk sums); chunk_groups (resident rows): scanned in place as well, total[1] = their sum
__device__ __forceinline__ void scan_chunks_body(unsigned long long* __restrict__ chunk_sum, int nchunks, const double* __restrict__ chunk_d2,
                                                 unsigned long long* __restrict__ total, double* __restrict__ total_d2,
                                                 unsigned* __restrict__ chunk_groups, const unsigned* __restrict__ chunk_rewritten) {
  __shared__ unsigned long long s[1024];
  __shared__ double sd[1024];
  __shared__ unsigned sg[1024];
  __shared__ unsigned long long sr[1024];
  const int t = threadIdx.x, T = blockDim.x;
  const int per = (nchunks + T - 1) / T;
  const int b0 = min(nchunks, t * per), b1 = min(nchunks, b0 + per);
  unsigned long long sum = 0, rs = 0; double d = 0; unsigned gs = 0;
  for (int b = b0; b < b1; ++b) { sum += chunk_sum[b]; d += chunk_d2[b]; if (chunk_groups) { gs += chunk_groups[b]; rs += chunk_rewritten[b]; } }
  s[t] = sum; sd[t] = d; sg[t] = gs; sr[t] = rs;
  __syncthreads();
  if (t == 0) {
    unsigned long long run = 0, rr = 0; double dr = 0; unsigned gr = 0;
    for (int k = 0; k < T; ++k) {
      const unsigned long long v = s[k]; s[k] = run; run += v; dr += sd[k];
      const unsigned gv = sg[k]; sg[k] = gr; gr += gv; rr += sr[k];
    }
    *total = run; *total_d2 = dr;
    if (chunk_groups) { total[1] = gr; total[2] = rr; }
  }
  __syncthreads();
  unsigned long long run = s[t];
  unsigned grun = sg[t];
  for (int b = b0; b < b1; ++b) {
    const unsigned long long v = chunk_sum[b]; chunk_sum[b] = run; run += v;
    if (chunk_groups) { const unsigned gv = chunk_groups[b]; chunk_groups[b] = grun; grun += gv; }
  }
}

__global__ void k_scan_chunks(unsigned long long* __restrict__ chunk_sum, int nchunks, const double* __restrict__ chunk_d2,
                              unsigned long long* __restrict__ total, double* __restrict__ total_d2,
                              unsigned* __restrict__ chunk_groups = nullptr, const unsigned* __restrict__ chunk_rewritten = nullptr) {
  scan_chunks_body(chunk_sum, nchunks, chunk_d2, total, total_d2, chunk_groups, chunk_rewritten);
}

__global__ __launch_bounds__(kScanChunk) void k_scan_within_chunks(const unsigned* __restrict__ counts, int nblocks,
                                                                   const unsigned long long* __restrict__ chunk_base,
                                                                   unsigned* __restrict__ offsets) {
  const int b = blockIdx.x * kScanChunk + threadIdx.x;
  const unsigned c = (b < nblocks) ? counts[b] : 0u;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __shared__ unsigned ws[kScanChunk / kWave];
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  unsigned wbase = 0;
  for (int k = 0; k < w; ++k) wbase += ws[k];
  if (b < nblocks) offsets[b] = (unsigned)chunk_base[blockIdx.x] + wbase + (inc - c);
}

// second stage: write the correspondence planes in source (cell) order
__global__ __launch_bounds__(kBlock) void k_compact_corr(const int* __restrict__ match_pos,
                                                         const unsigned* __restrict__ order, size_t n,
                                                         const unsigned* __restrict__ block_offsets,
                                                         const float4* __restrict__ Gsrc, const float4* __restrict__ LNsrc,
                                                         Affine Tsrc, const float4* __restrict__ Gtgt,
                                                         const float4* __restrict__ LNtgt, Affine Ttgt,
                                                         float4* __restrict__ A, float4* __restrict__ B,
                                                         float4* __restrict__ C, size_t out_base) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int m = (j < n) ? ld_stream(match_pos + j) : -1;
  const bool f = m >= 0;
  const unsigned long long b = __ballot(f);
  __shared__ unsigned wbase[kBlock / kWave];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wbase[w] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned base = block_offsets[blockIdx.x];
  for (int k = 0; k < w; ++k) base += wbase[k];
  if (!f) return;
  const unsigned rank = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
  const size_t o = out_base + base + rank;
  const size_t js = order ? (size_t)ld_stream(order + j) : j;     // query j of the (sorted) search order -> source position
  const float4 sp = order ? Gsrc[js] : ld_stream(Gsrc + js);
  const float4 ln = order ? LNsrc[js] : ld_stream(LNsrc + js);
  const float3 sn = pcl_so3(Tsrc, ln.x, ln.y, ln.z);
  const float4 tp = Gtgt[m];
  const float4 tl = LNtgt[m];
  const float3 tn = pcl_so3(Ttgt, tl.x, tl.y, tl.z);
  st_stream(A + o, make_float4(sp.x, sp.y, sp.z, sn.x));
  st_stream(B + o, make_float4(sn.y, sn.z, tp.x, tp.y));
  st_stream(C + o, make_float4(tp.z, tn.x, tn.y, tn.z));
}

// Resident rows (LmSet): one row per query of the pair, at its source position.  A row is twelve floats; the six of the SOURCE
// are the cloud's own point and normal at that position, the same for every pair with this cloud as source and unchanged while
// the cloud's frame stands: they live once per cloud in its source view (k_source_view), and a pair keeps the TARGET half only,
//   R0[j] = (tp.x, tp.y)   R1[j] = (tp.z, tn.xyz).
// A query without a partner carries a NaN in tp.x (kRowMark): no partner has one -- a target point with a NaN coordinate never
// compares nearer than anything in the searches -- and the LM passes turn such a row into the all-zero row whose residuals and
// Jacobian rows are exactly 0.  (Not "all zeros": a partner at the local origin with a zero normal is a correspondence.)
__device__ __forceinline__ float row_mark() { return __uint_as_float(0x7FC00000u); }
__device__ __forceinline__ void st_stream2(float2* __restrict__ p, const float2 v) {
  if constexpr (E3D_NT >= 2) { const row_v2f w = {v.x, v.y}; __builtin_nontemporal_store(w, reinterpret_cast<row_v2f*>(p)); }
  else *p = v;
}

// The source view of a cloud in its sorted order: V0[j] = (p.xyz, n.x), V1[j] = (n.y, n.z) for j < n, zeros up to cap.  A cloud
// that can move is held in its LOCAL frame (P = L4); one that never moves inside the call (impl cloud 0, fixed clouds) in the
// global frame at pose T exactly as k_compact_corr writes it (P = G4, normal = pcl_so3(T, ln)).
__global__ __launch_bounds__(kBlock) void k_source_view(const float4* __restrict__ P, const float4* __restrict__ LN, size_t n, size_t cap,
                                                        const int global, Affine T, float4* __restrict__ V0, float2* __restrict__ V1) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cap) return;
  float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f);
  float2 v1 = make_float2(0.f, 0.f);
  if (j < n) {
    const float4 sp = ld_stream(P + j);
    const float4 ln = ld_stream(LN + j);
    float3 sn = make_float3(ln.x, ln.y, ln.z);
    if (global) sn = pcl_so3(T, ln.x, ln.y, ln.z);
    v0 = make_float4(sp.x, sp.y, sp.z, sn.x);
    v1 = make_float2(sn.y, sn.z);
  }
  st_stream(V0 + j, v0); st_stream2(V1 + j, v1);
}

// The update rewrites the rows whose partner differs from the one the row encodes -- in the settled state of an alignment a handful per launch, where k_compact_corr gathered and rewrote all
// of them every outer iteration -- and produces what the progress line and the LM passes need from the match list: per-block
// match counts and squared-distance sums (the arithmetic of k_match_block_counts) and the active 64-row groups of the block
// (count in bits 0..7, mask in bits 8..11; bits 16..24: rows rewritten, a statistic -- summed without atomics: an atomic per
// wave on one counter made a launch that rewrites every row 3.5 times slower than k_compact_corr).  The half of a cloud that never
// moves (impl cloud 0, fixed clouds) is stored in the global frame exactly as k_compact_corr writes it; that of a movable cloud in
// the cloud's local frame (row_to_global).
// E3D_R0_RUN: rows per rewritten run of the float2 plane, 8 (64 B) or 16 (a whole 128-byte line; the rows of the line's other
// half gather their partner's point again).  Measured: profiles/split_rows.txt.
#ifndef E3D_R0_RUN
#define E3D_R0_RUN 8
#endif
static_assert(E3D_R0_RUN == 8 || E3D_R0_RUN == 16, "runs of the float2 plane: 8 or 16 rows");
__device__ __forceinline__ void corr_update_body(const unsigned bx, const int* __restrict__ match, int* __restrict__ plane_match,
                                                 const float* __restrict__ match_d2, size_t n, const float4* __restrict__ Ptgt,
                                                 const float4* __restrict__ LNtgt, const int tgt_global, const Affine& Ttgt,
                                                 float2* __restrict__ R0, float4* __restrict__ R1,
                                                 unsigned* __restrict__ block_counts, double* __restrict__ block_d2,
                                                 unsigned* __restrict__ block_groups, const unsigned char* __restrict__ done = nullptr) {
  if (done && done[bx]) return;      // every query settled by its certificate: nn_certify_body wrote this block's results
  const size_t j = (size_t)bx * blockDim.x + threadIdx.x;
  const bool in = j < n;
  const int m = in ? ld_stream(match + j) : -1;
  const int pm = in ? ld_stream(plane_match + j) : -1;
  const bool f = m >= 0;
  // Rows are rewritten in whole 128-byte lines (8 rows of the float4 plane): a lone 16-byte store is a partial line write all the
  // way to HBM -- measured: 3.5 ms per launch with 5 % of the rows rewritten one by one, against 1.0 ms for ALL rows in full lines.
  const unsigned long long chg = __ballot(in && m != pm);
  const bool wr = in && (((chg >> (threadIdx.x & 56)) & 0xFFull) != 0ull);
  const bool wr0 = (E3D_R0_RUN == 8) ? wr : (in && (((chg >> (threadIdx.x & 48)) & 0xFFFFull) != 0ull));
  const unsigned long long wrb = __ballot(wr);
  if (wr0) {
    float2 r0 = make_float2(row_mark(), 0.f);
    float4 r1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f) {
      const float4 tp = Ptgt[m];
      r0 = make_float2(tp.x, tp.y);
      if (wr) {
        const float4 tl = LNtgt[m];
        float3 tn = make_float3(tl.x, tl.y, tl.z);
        if (tgt_global) tn = pcl_so3(Ttgt, tl.x, tl.y, tl.z);
        r1 = make_float4(tp.z, tn.x, tn.y, tn.z);
      }
    }
    st_stream2(R0 + j, r0);
    if (wr) {
      st_stream(R1 + j, r1);
      if (m != pm) plane_match[j] = m;
    }
  }
  const unsigned long long b = __ballot(f);
  double d = f ? (double)ld_stream(match_d2 + j) : 0.0;
  d = wave_sum(d);
  __shared__ unsigned sc[kBlock / kWave], sw[kBlock / kWave];
  __shared__ double sd[kBlock / kWave];
  if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = (unsigned)__popcll(b); sw[threadIdx.x >> 6] = (unsigned)__popcll(wrb); sd[threadIdx.x >> 6] = d; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0, g = 0, gm = 0, rw = 0; double t = 0;
    for (int k = 0; k < kBlock / kWave; ++k) { c += sc[k]; t += sd[k]; rw += sw[k]; if (sc[k]) { ++g; gm |= 1u << k; } }
    block_counts[bx] = c; block_d2[bx] = t; block_groups[bx] = g | (gm << 8) | (rw << 16);    // (rw <= 256)
  }
}

__global__ __launch_bounds__(kBlock) void k_corr_update(const int* __restrict__ match, int* __restrict__ plane_match,
                                                        const float* __restrict__ match_d2, size_t n, const float4* __restrict__ Ptgt,
                                                        const float4* __restrict__ LNtgt, const int tgt_global, Affine Ttgt,
                                                        float2* __restrict__ R0, float4* __restrict__ R1,
                                                        unsigned* __restrict__ block_counts, double* __restrict__ block_d2,
                                                        unsigned* __restrict__ block_groups) {
  corr_update_body(blockIdx.x, match, plane_match, match_d2, n, Ptgt, LNtgt, tgt_global, Ttgt, R0, R1, block_counts, block_d2, block_groups);
}

// the resident rows of a batch of pairs: the per-block results of pair p go to entries [blk0(p), blk0(p) + blocks of p) of the batch's arrays
__global__ __launch_bounds__(kBlock) void k_corr_update_multi(const NnBatchDev* __restrict__ Bt, unsigned* __restrict__ block_counts,
                                                              double* __restrict__ block_d2, unsigned* __restrict__ block_groups) {
  const int p = nn_find_range(Bt->upd_end, Bt->n_pairs, blockIdx.x);
  const unsigned b0 = p ? Bt->upd_end[p - 1] : 0u;
  const NnPairDev& P = Bt->pair[p];
  const Affine Tt = P.Ttgt;
  corr_update_body(blockIdx.x - b0, P.match, P.plane_match, P.match_d2, (size_t)P.n, P.Ptgt, P.LNtgt, P.tgt_global, Tt, P.R0, P.R1,
                   block_counts + b0, block_d2 + b0, block_groups + b0, P.upd_done);
}

// ascending list of the active 64-row groups: one thread per query block (4 groups), scan inside the chunk + the chunk's base
__device__ __forceinline__ void group_list_body(const unsigned bx, const unsigned* __restrict__ block_groups, int nblocks,
                                                const unsigned* __restrict__ chunk_gbase, unsigned* __restrict__ glist) {
  const int b = (int)bx * kScanChunk + threadIdx.x;
  const unsigned w = (b < nblocks) ? block_groups[b] : 0u;
  const unsigned c = w & 0xFFu;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __shared__ unsigned ws[kScanChunk / kWave];
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  unsigned base = chunk_gbase[bx] + (inc - c);
  for (int k = 0; k < wv; ++k) base += ws[k];
  const unsigned mask = w >> 8;
#pragma unroll
  for (int k = 0; k < kBlock / kWave; ++k)
    if (mask & (1u << k)) glist[base++] = (unsigned)b * (kBlock / kWave) + (unsigned)k;
}

__global__ __launch_bounds__(kScanChunk) void k_group_list(const unsigned* __restrict__ block_groups, int nblocks,
                                                           const unsigned* __restrict__ chunk_gbase,
                                                           unsigned* __restrict__ glist) {
  group_list_body(blockIdx.x, block_groups, nblocks, chunk_gbase, glist);
}

// totals and group lists of a batch of pairs (launch_corr_totals for each of them, three launches in all): chunk c of the batch
// belongs to the pair whose chunk range holds it; pair p's totals go to totals[3 p ..], total_d2[p]
__global__ __launch_bounds__(kScanChunk) void k_scan_chunk_sums_multi(const NnBatchDev* __restrict__ Bt, const unsigned* __restrict__ block_counts,
                                                                      const double* __restrict__ block_d2, const unsigned* __restrict__ block_groups,
                                                                      unsigned long long* __restrict__ chunk_sum, double* __restrict__ chunk_d2,
                                                                      unsigned* __restrict__ chunk_groups, unsigned* __restrict__ chunk_rewritten) {
  const int p = nn_find_range(Bt->chunk_end, Bt->n_pairs, blockIdx.x);
  const unsigned c0 = p ? Bt->chunk_end[p - 1] : 0u, b0 = p ? Bt->upd_end[p - 1] : 0u;
  scan_chunk_sums_body(blockIdx.x - c0, block_counts + b0, (int)(Bt->upd_end[p] - b0), block_d2 + b0, chunk_sum + c0, chunk_d2 + c0, block_groups + b0,
                       chunk_groups + c0, chunk_rewritten + c0);
}
__global__ __launch_bounds__(1024) void k_scan_chunks_multi(const NnBatchDev* __restrict__ Bt, unsigned long long* __restrict__ chunk_sum,
                                                            const double* __restrict__ chunk_d2, unsigned long long* __restrict__ totals,
                                                            double* __restrict__ total_d2, unsigned* __restrict__ chunk_groups,
                                                            const unsigned* __restrict__ chunk_rewritten) {
  const int p = blockIdx.x;
  const unsigned c0 = p ? Bt->chunk_end[p - 1] : 0u;
  scan_chunks_body(chunk_sum + c0, (int)(Bt->chunk_end[p] - c0), chunk_d2 + c0, totals + 3 * p, total_d2 + p, chunk_groups + c0, chunk_rewritten + c0);
}
__global__ __launch_bounds__(kScanChunk) void k_group_list_multi(const NnBatchDev* __restrict__ Bt, const unsigned* __restrict__ block_groups,
                                                                 const unsigned* __restrict__ chunk_gbase) {
  const int p = nn_find_range(Bt->chunk_end, Bt->n_pairs, blockIdx.x);
  const unsigned c0 = p ? Bt->chunk_end[p - 1] : 0u, b0 = p ? Bt->upd_end[p - 1] : 0u;
  group_list_body(blockIdx.x - c0, block_groups + b0, (int)(Bt->upd_end[p] - b0), chunk_gbase + c0, Bt->pair[p].glist);
}

// gather variant for explicit (index_query, index_match) lists on unsorted AoS clouds
// (stand-alone e3d_icp_pair_system entry point)
__global__ __launch_bounds__(kBlock) void k_gather_corr(const float* __restrict__ sxyz, const float* __restrict__ snrm,
                                                        const float* __restrict__ txyz, const float* __restrict__ tnrm,
                                                        const int* __restrict__ iq, const int* __restrict__ im, size_t n,
                                                        float4* __restrict__ A, float4* __restrict__ B,
                                                        float4* __restrict__ C) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const size_t s = (size_t)iq[c], t = (size_t)im[c];
  A[c] = make_float4(sxyz[3 * s], sxyz[3 * s + 1], sxyz[3 * s + 2], snrm[3 * s]);
  B[c] = make_float4(snrm[3 * s + 1], snrm[3 * s + 2], txyz[3 * t], txyz[3 * t + 1]);
  C[c] = make_float4(txyz[3 * t + 2], tnrm[3 * t], tnrm[3 * t + 1], tnrm[3 * t + 2]);
}

// squared NN distances by ORIGINAL source index (-1 = no partner): the order the reference sums them in for its progress line
// (icp_point_to_plane.cc:226-229); e3d_icp_set_sequential_distance_sum
__global__ __launch_bounds__(kBlock) void k_match_d2_by_original(const int* __restrict__ match_pos, const float* __restrict__ match_d2,
                                                                 const unsigned* __restrict__ order, size_t n, const float4* __restrict__ Gsrc,
                                                                 float* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const size_t js = order ? (size_t)order[j] : j;
  out[__float_as_uint(Gsrc[js].w)] = (match_pos[j] >= 0) ? match_d2[j] : -1.f;
}

// un-permute NN results to original source order / original target indices
__global__ __launch_bounds__(kBlock) void k_unpermute_matches(const int* __restrict__ match_pos,
                                                              const float* __restrict__ match_d2,
                                                              const unsigned* __restrict__ order, size_t n,
                                                              const float4* __restrict__ Gsrc,
                                                              const float4* __restrict__ Gtgt,
                                                              int* __restrict__ out_idx, float* __restrict__ out_d2) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const size_t js = order ? (size_t)order[j] : j;
  const unsigned oi = __float_as_uint(Gsrc[js].w);
  const int m = match_pos[j];
  out_idx[oi] = (m >= 0) ? (int)__float_as_uint(Gtgt[m].w) : -1;
  out_d2[oi] = (m >= 0) ? match_d2[j] : 0.f;
}

// =================================================================================================
// host-side launch helpers
// =================================================================================================
void launch_match_scan(const int* match_pos, const float* match_d2, size_t n, unsigned* block_counts,
                       unsigned* block_offsets, double* block_d2, unsigned long long* chunk_sum, double* chunk_d2,
                       unsigned long long* total, double* total_d2, hipStream_t s) {
  const int nb = (int)div_up(n ? n : 1, kBlock);
  // match_pos == nullptr: block_counts / block_d2 hold the per-block sums already (their producer wrote them: k_obs_eval)
  if (match_pos) hipLaunchKernelGGL(k_match_block_counts, dim3(nb), dim3(kBlock), 0, s, match_pos, n, block_counts, block_d2,
                                    match_d2);
  const int nch = (nb + kScanChunk - 1) / kScanChunk;
  hipLaunchKernelGGL(k_scan_chunk_sums, dim3(nch), dim3(kScanChunk), 0, s, block_counts, nb, block_d2, chunk_sum, chunk_d2, (const unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr);
  hipLaunchKernelGGL(k_scan_chunks, dim3(1), dim3(1024), 0, s, chunk_sum, nch, chunk_d2, total, total_d2, (unsigned*)nullptr, (const unsigned*)nullptr);
  hipLaunchKernelGGL(k_scan_within_chunks, dim3(nch), dim3(kScanChunk), 0, s, block_counts, nb, chunk_sum, block_offsets);
}

void launch_compact_corr(const int* match_pos, const unsigned* order, size_t n, const unsigned* block_offsets, const float4* Gsrc,
                         const float4* LNsrc, const Affine& Tsrc, const float4* Gtgt, const float4* LNtgt,
                         const Affine& Ttgt, float4* A, float4* B, float4* C, size_t out_base, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_compact_corr, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, match_pos, order, n,
                     block_offsets, Gsrc, LNsrc, Tsrc, Gtgt, LNtgt, Ttgt, A, B, C, out_base);
}

void launch_source_view(const float4* P, const float4* LN, size_t n, size_t cap, bool global, const Affine& T, float4* V0, float2* V1, hipStream_t s) {
  if (!cap) return;
  hipLaunchKernelGGL(k_source_view, dim3((unsigned)div_up(cap, kBlock)), dim3(kBlock), 0, s, P, LN, n, cap, global ? 1 : 0, T, V0, V1);
}

void launch_corr_update(const int* match, int* plane_match, const float* match_d2, size_t n, const float4* Ptgt, const float4* LNtgt,
                        bool tgt_global, const Affine& Ttgt, float2* R0, float4* R1, unsigned* block_counts, double* block_d2,
                        unsigned* block_groups, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_corr_update, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, match, plane_match, match_d2, n, Ptgt, LNtgt,
                     tgt_global ? 1 : 0, Ttgt, R0, R1, block_counts, block_d2, block_groups);
}

void launch_corr_totals(size_t n, const unsigned* block_counts, const double* block_d2, const unsigned* block_groups,
                        unsigned long long* chunk_sum, double* chunk_d2, unsigned* chunk_groups, unsigned long long* totals,
                        double* total_d2, unsigned* glist, hipStream_t s) {
  const int nb = (int)div_up(n ? n : 1, kBlock);
  const int nch = (nb + kScanChunk - 1) / kScanChunk;
  unsigned* chunk_rewritten = chunk_groups + nch;        // (chunk_groups holds 2 * nch entries)
  hipLaunchKernelGGL(k_scan_chunk_sums, dim3(nch), dim3(kScanChunk), 0, s, block_counts, nb, block_d2, chunk_sum, chunk_d2, block_groups, chunk_groups, chunk_rewritten);
  hipLaunchKernelGGL(k_scan_chunks, dim3(1), dim3(1024), 0, s, chunk_sum, nch, chunk_d2, totals, total_d2, chunk_groups, (const unsigned*)chunk_rewritten);
  hipLaunchKernelGGL(k_group_list, dim3(nch), dim3(kScanChunk), 0, s, block_groups, nb, chunk_groups, glist);
}

void launch_corr_update_multi(const NnBatchDev* batch, unsigned n_blocks, unsigned* block_counts, double* block_d2, unsigned* block_groups, hipStream_t s) {
  if (!n_blocks) return;
  hipLaunchKernelGGL(k_corr_update_multi, dim3(n_blocks), dim3(kBlock), 0, s, batch, block_counts, block_d2, block_groups);
}
void launch_corr_totals_multi(const NnBatchDev* batch, int n_pairs, unsigned n_chunks, const unsigned* block_counts, const double* block_d2,
                              const unsigned* block_groups, unsigned long long* chunk_sum, double* chunk_d2, unsigned* chunk_groups,
                              unsigned* chunk_rewritten, unsigned long long* totals, double* total_d2, hipStream_t s) {
  static_assert(kNnScanChunk == kScanChunk, "blocks per chunk");
  if (!n_pairs || !n_chunks) return;
  hipLaunchKernelGGL(k_scan_chunk_sums_multi, dim3(n_chunks), dim3(kScanChunk), 0, s, batch, block_counts, block_d2, block_groups, chunk_sum, chunk_d2,
                     chunk_groups, chunk_rewritten);
  hipLaunchKernelGGL(k_scan_chunks_multi, dim3((unsigned)n_pairs), dim3(1024), 0, s, batch, chunk_sum, (const double*)chunk_d2, totals, total_d2, chunk_groups,
                     (const unsigned*)chunk_rewritten);
  hipLaunchKernelGGL(k_group_list_multi, dim3(n_chunks), dim3(kScanChunk), 0, s, batch, block_groups, (const unsigned*)chunk_groups);
}

void launch_gather_corr(const float* sxyz, const float* snrm, const float* txyz, const float* tnrm, const int* iq,
                        const int* im, size_t n, float4* A, float4* B, float4* C, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_gather_corr, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, sxyz, snrm, txyz, tnrm, iq,
                     im, n, A, B, C);
}

void launch_unpermute_matches(const int* match_pos, const float* match_d2, const unsigned* order, size_t n, const float4* Gsrc,
                              const float4* Gtgt, int* out_idx, float* out_d2, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_unpermute_matches, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, match_pos, match_d2,
                     order, n, Gsrc, Gtgt, out_idx, out_d2);
}

void launch_match_d2_by_original(const int* match_pos, const float* match_d2, const unsigned* order, size_t n, const float4* Gsrc, float* out,
                                 hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_match_d2_by_original, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, match_pos, match_d2, order, n, Gsrc, out);
}

}  // namespace e3d
