// e3d_icp_lm.hip -- ICP, LM passes (gfx950 / CDNA4, wave64): cost and Gramian blocks of the correspondence rows in one
// pass per mode (k_lm_pass), the costs of all LM tries in one pass (k_lm_cost_multi) and the fixed-order reduction of the block
// partials (k_lm_reduce).  tools/micro/lm_variants.hip includes this file for its bodies.
//
// Reference loops covered: a7 (accumulate), a8 (cost).
#include "e3d_icp_device.hpp"

#pragma clang fp contract(off)

namespace e3d {

// =================================================================================================
// a7 + a8: PointToPlaneICPImpl::compute accumulate / cost passes
//          (icp_point_to_plane_impl.h:119-211 and :240-266), fused: one pass over the
//          correspondence planes yields cost and (mode-dependent) the Gramian blocks.
// =================================================================================================
// f32 residual / Jacobian rows, literally as written in the reference (left-to-right).  (Templated on the scalar type only so that
// tools/micro/lm_variants.hip can instantiate experimental forms; the product uses T = float.  A form that pushed TWO
// correspondences through the packed v_pk_mul_f32 / v_pk_add_f32 instructions was measured and dropped: the pose entries have to
// be splatted into VGPR pairs and the pair interleaved with ~20 moves per trip, and it never beat the scalar loop -- DESIGN 4.2.)
//
// The two 12-entry rows [js ; jt] of a correspondence only hold 9 different numbers each: the translation parts are
// js[0..2] = -jt[0..2] (impl.h:162-164 / 170-172 and 188-190 / 197-199).  With m = jt[0..2], a = js[3..5], b = jt[3..5]:
//   row 1: m = sn,  a = impl.h:173-177, b = impl.h:165-168;     row 2: m = -tn, a = impl.h:200-204, b = impl.h:191-195.
template <typename T>
struct CorrRowsT {
  T r1, r2;
  T m1[3], a1[3], b1[3];
  T m2[3], a2[3], b2[3];
};

template <typename T>
__device__ __forceinline__ T dot3t(const T a0, const T a1, const T a2, const T b0, const T b1, const T b2) {
  const T e0 = a0 * b0, e1 = a1 * b1, e2 = a2 * b2;       // Eigen 3-term inner product: e0 + (e1 + e2)
  return e0 + (e1 + e2);
}
template <typename T>
__device__ __forceinline__ T rdot(const float r0, const float r1, const float r2, const T x, const T y, const T z) {
  const T e0 = r0 * x, e1 = r1 * y, e2 = r2 * z;          // row of R (block-uniform scalars) times a point
  return e0 + (e1 + e2);
}

template <typename T>
struct CorrPts { T spx, spy, spz, snx, sny, snz, tpx, tpy, tpz, tnx, tny, tnz; };

// inner poses applied with Eigen's R*p + t order (impl.h:144-151)
template <typename T>
__device__ __forceinline__ void corr_src(const float* Rs, const float* ts, const T lsx, const T lsy, const T lsz, const T lnx,
                                         const T lny, const T lnz, CorrPts<T>& P) {
  P.spx = rdot<T>(Rs[0], Rs[1], Rs[2], lsx, lsy, lsz) + ts[0];
  P.spy = rdot<T>(Rs[3], Rs[4], Rs[5], lsx, lsy, lsz) + ts[1];
  P.spz = rdot<T>(Rs[6], Rs[7], Rs[8], lsx, lsy, lsz) + ts[2];
  P.snx = rdot<T>(Rs[0], Rs[1], Rs[2], lnx, lny, lnz);
  P.sny = rdot<T>(Rs[3], Rs[4], Rs[5], lnx, lny, lnz);
  P.snz = rdot<T>(Rs[6], Rs[7], Rs[8], lnx, lny, lnz);
}
template <typename T>
__device__ __forceinline__ void corr_tgt(const float* Rt, const float* tt, const T ltx, const T lty, const T ltz, const T lmx,
                                         const T lmy, const T lmz, CorrPts<T>& P) {
  P.tpx = rdot<T>(Rt[0], Rt[1], Rt[2], ltx, lty, ltz) + tt[0];
  P.tpy = rdot<T>(Rt[3], Rt[4], Rt[5], ltx, lty, ltz) + tt[1];
  P.tpz = rdot<T>(Rt[6], Rt[7], Rt[8], ltx, lty, ltz) + tt[2];
  P.tnx = rdot<T>(Rt[0], Rt[1], Rt[2], lmx, lmy, lmz);
  P.tny = rdot<T>(Rt[3], Rt[4], Rt[5], lmx, lmy, lmz);
  P.tnz = rdot<T>(Rt[6], Rt[7], Rt[8], lmx, lmy, lmz);
}

template <bool NEED_SRC, bool NEED_TGT, typename T>
__device__ __forceinline__ void corr_rows_pts(const CorrPts<T>& P, CorrRowsT<T>& o) {
  const T spx = P.spx, spy = P.spy, spz = P.spz, snx = P.snx, sny = P.sny, snz = P.snz;
  const T tpx = P.tpx, tpy = P.tpy, tpz = P.tpz, tnx = P.tnx, tny = P.tny, tnz = P.tnz;
  o.r1 = dot3t<T>(snx, sny, snz, tpx - spx, tpy - spy, tpz - spz);                // impl.h:158
  o.r2 = dot3t<T>(tnx, tny, tnz, spx - tpx, spy - tpy, spz - tpz);                // impl.h:185
  if (NEED_SRC || NEED_TGT) {
    o.m1[0] = snx; o.m1[1] = sny; o.m1[2] = snz;                                  // impl.h:162-164 (j1s[0..2] = -m1)
    o.m2[0] = -tnx; o.m2[1] = -tny; o.m2[2] = -tnz;                               // impl.h:188-190 (j2s[0..2] = -m2 = tn)
  }
  if (NEED_TGT) {
    o.b1[0] = -sny * tpz + snz * tpy;                                             // impl.h:165-168
    o.b1[1] = snx * tpz - snz * tpx;
    o.b1[2] = -snx * tpy + sny * tpx;
    o.b2[0] = tny * tpz - tny * (tpz - spz) - tnz * tpy + tnz * (tpy - spy);      // impl.h:191-195
    o.b2[1] = -tnx * tpz + tnx * (tpz - spz) + tnz * tpx - tnz * (tpx - spx);
    o.b2[2] = tnx * tpy - tnx * (tpy - spy) - tny * tpx + tny * (tpx - spx);
  }
  if (NEED_SRC) {
    o.a1[0] = sny * spz - sny * (spz - tpz) - snz * spy + snz * (spy - tpy);      // impl.h:173-177
    o.a1[1] = -snx * spz + snx * (spz - tpz) + snz * spx - snz * (spx - tpx);
    o.a1[2] = snx * spy - snx * (spy - tpy) - sny * spx + sny * (spx - tpx);
    o.a2[0] = -tny * spz + tnz * spy;                                             // impl.h:200-204
    o.a2[1] = tnx * spz - tnz * spx;
    o.a2[2] = -tnx * spy + tny * spx;
  }
}

template <bool NEED_SRC, bool NEED_TGT, typename T, typename V4>
__device__ __forceinline__ void corr_rows(const LmSet& S, const V4& a, const V4& b, const V4& c, CorrRowsT<T>& o) {
  CorrPts<T> P;
  corr_src<T>(S.Rs, S.ts, a.x, a.y, a.z, a.w, b.x, b.y, P);
  corr_tgt<T>(S.Rt, S.tt, b.z, b.w, c.x, c.y, c.z, c.w, P);
  corr_rows_pts<NEED_SRC, NEED_TGT, T>(P, o);
}

template <int H> __device__ __forceinline__ float half_of(const float v) { return v; }

// accumulate upper triangle of J J^T (21) and r*J (6) in f64 from f32 rows cast to f64 first
// (icp_point_to_plane_impl.h:91-112,179-182: .cast<double>() before the product).  The f64 product of two numbers that
// came from f32 is exact (48 significant bits), so the fused multiply-add rounds exactly as the reference's separate
// multiplication and addition do: one v_fma_f64 instead of v_mul_f64 + v_add_f64 with the translation unit's contraction off.
__device__ __forceinline__ void acc_diag(double* H21, double* b6, const float* j, float r) {
  double J[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) J[i] = (double)j[i];
  const double R = (double)r;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int l = i; l < 6; ++l) { H21[k] = __builtin_fma(J[i], J[l], H21[k]); ++k; }
    b6[i] = __builtin_fma(R, J[i], b6[i]);
  }
}

// Both sides have variables (modes kModeTwo / kModeTwoCross).  The Gramian of the 12-entry row [js ; jt] needs 78 (+12 for
// r*J) products per row; because js[0..2] = -jt[0..2] it is determined by the Gramian of the 10 numbers u = [m a b r]:
// 45 (kModeTwo) or 54 (kModeTwoCross) products.  The f64 product of two f32 values is exact and negation commutes with
// every rounding, so sum((-m_i) a_l) = -sum(m_i a_l) bit for bit: the blocks written out below are the ones a direct
// accumulation of SS, TT, ST, bs, bt in the same order yields (icp_point_to_plane_impl.h:91-112,179-182,206-209).
//   acc layout: [0] cost, [1..6] m m^T (upper), [7..15] m a^T, [16..21] a a^T, [22..30] m b^T, [31..36] b b^T,
//               [37..39] r m, [40..42] r a, [43..45] r b, [46..54] a b^T (kModeTwoCross only)
constexpr int kAccTwo = 46, kAccCross = 55;
template <bool CROSS>
__device__ __forceinline__ void acc_reduced(double* acc, const float m0, const float m1, const float m2, const float a0,
                                            const float a1, const float a2, const float b0, const float b1, const float b2,
                                            const float r) {
  const double M[3] = {(double)m0, (double)m1, (double)m2};
  const double A[3] = {(double)a0, (double)a1, (double)a2};
  const double Bv[3] = {(double)b0, (double)b1, (double)b2};
  const double R = (double)r;
  int k = 1;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = i; l < 3; ++l) { acc[k] = __builtin_fma(M[i], M[l], acc[k]); ++k; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) acc[7 + 3 * i + l] = __builtin_fma(M[i], A[l], acc[7 + 3 * i + l]);
  k = 16;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = i; l < 3; ++l) { acc[k] = __builtin_fma(A[i], A[l], acc[k]); ++k; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) acc[22 + 3 * i + l] = __builtin_fma(M[i], Bv[l], acc[22 + 3 * i + l]);
  k = 31;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = i; l < 3; ++l) { acc[k] = __builtin_fma(Bv[i], Bv[l], acc[k]); ++k; }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    acc[37 + i] = __builtin_fma(R, M[i], acc[37 + i]); acc[40 + i] = __builtin_fma(R, A[i], acc[40 + i]); acc[43 + i] = __builtin_fma(R, Bv[i], acc[43 + i]);
  }
  if (CROSS) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int l = 0; l < 3; ++l) acc[46 + 3 * i + l] = __builtin_fma(A[i], Bv[l], acc[46 + 3 * i + l]);
  }
}

// output slot t of a block partial (layout below) = sgn[t] * acc[idx[t]] of the reduced accumulators
struct LmSlotMap { short idx[91]; signed char sgn[91]; };
constexpr int lm_tri3(int i, int l) { return i <= l ? (i == 0 ? l : i == 1 ? 2 + l : 5) : lm_tri3(l, i); }   // 00 01 02 11 12 22
constexpr LmSlotMap make_lm_slot_map() {
  LmSlotMap m{};
  m.idx[0] = 0; m.sgn[0] = 1;
  int k = 1;
  for (int i = 0; i < 6; ++i)
    for (int l = i; l < 6; ++l, ++k) {                    // SS = js js^T, js = [-m a]
      if (l < 3) { m.idx[k] = (short)(1 + lm_tri3(i, l)); m.sgn[k] = 1; }
      else if (i < 3) { m.idx[k] = (short)(7 + 3 * i + (l - 3)); m.sgn[k] = -1; }
      else { m.idx[k] = (short)(16 + lm_tri3(i - 3, l - 3)); m.sgn[k] = 1; }
    }
  for (int i = 0; i < 6; ++i) {                           // bs = r js
    if (i < 3) { m.idx[22 + i] = (short)(37 + i); m.sgn[22 + i] = -1; }
    else { m.idx[22 + i] = (short)(40 + i - 3); m.sgn[22 + i] = 1; }
  }
  k = 28;
  for (int i = 0; i < 6; ++i)
    for (int l = i; l < 6; ++l, ++k) {                    // TT = jt jt^T, jt = [m b]
      if (l < 3) { m.idx[k] = (short)(1 + lm_tri3(i, l)); m.sgn[k] = 1; }
      else if (i < 3) { m.idx[k] = (short)(22 + 3 * i + (l - 3)); m.sgn[k] = 1; }
      else { m.idx[k] = (short)(31 + lm_tri3(i - 3, l - 3)); m.sgn[k] = 1; }
    }
  for (int i = 0; i < 6; ++i) {                           // bt = r jt
    m.idx[49 + i] = (short)(i < 3 ? 37 + i : 43 + i - 3); m.sgn[49 + i] = 1;
  }
  for (int i = 0; i < 6; ++i)
    for (int l = 0; l < 6; ++l) {                         // ST = js jt^T
      const int t = 55 + 6 * i + l;
      if (i < 3 && l < 3) { m.idx[t] = (short)(1 + lm_tri3(i, l)); m.sgn[t] = -1; }
      else if (i < 3) { m.idx[t] = (short)(22 + 3 * i + (l - 3)); m.sgn[t] = -1; }
      else if (l < 3) { m.idx[t] = (short)(7 + 3 * l + (i - 3)); m.sgn[t] = 1; }
      else { m.idx[t] = (short)(46 + 3 * (i - 3) + (l - 3)); m.sgn[t] = 1; }
    }
  return m;
}
__device__ const LmSlotMap kLmSlotMap = make_lm_slot_map();

// one correspondence (T = float, H = 0) or one half of a packed pair (T = f2_t, H = 0 / 1) into the accumulators
template <int MODE, int H, typename T>
__device__ __forceinline__ void lm_accumulate(double* acc, const CorrRowsT<T>& R, const int side) {
  constexpr bool kOne = (MODE == kModeOne);
  constexpr bool kCross = (MODE == kModeTwoCross);
  const float r1 = half_of<H>(R.r1), r2 = half_of<H>(R.r2);
  if (MODE == kModeCost) {
    acc[0] += (double)(r1 * r1);
    acc[0] += (double)(r2 * r2);
  } else if (kOne) {
    // only one side of the pair has variables (the other is impl cloud 0); block-uniform branch
    float j1[6], j2[6];
    if (side == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { j1[i] = -half_of<H>(R.m1[i]); j1[3 + i] = half_of<H>(R.a1[i]); j2[i] = -half_of<H>(R.m2[i]); j2[3 + i] = half_of<H>(R.a2[i]); }
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) { j1[i] = half_of<H>(R.m1[i]); j1[3 + i] = half_of<H>(R.b1[i]); j2[i] = half_of<H>(R.m2[i]); j2[3 + i] = half_of<H>(R.b2[i]); }
    }
    acc[0] += (double)(r1 * r1);
    acc_diag(acc + 1, acc + 22, j1, r1);
    acc[0] += (double)(r2 * r2);
    acc_diag(acc + 1, acc + 22, j2, r2);
  } else {
    acc[0] += (double)(r1 * r1);
    acc_reduced<kCross>(acc, half_of<H>(R.m1[0]), half_of<H>(R.m1[1]), half_of<H>(R.m1[2]), half_of<H>(R.a1[0]), half_of<H>(R.a1[1]),
                        half_of<H>(R.a1[2]), half_of<H>(R.b1[0]), half_of<H>(R.b1[1]), half_of<H>(R.b1[2]), r1);
    acc[0] += (double)(r2 * r2);
    acc_reduced<kCross>(acc, half_of<H>(R.m2[0]), half_of<H>(R.m2[1]), half_of<H>(R.m2[2]), half_of<H>(R.a2[0]), half_of<H>(R.a2[1]),
                        half_of<H>(R.a2[2]), half_of<H>(R.b2[0]), half_of<H>(R.b2[1]), half_of<H>(R.b2[2]), r2);
  }
}

template <int MODE, typename T, typename V4>
__device__ __forceinline__ void lm_rows(const LmSet& S, const V4& a, const V4& b, const V4& c, CorrRowsT<T>& R) {
  if (MODE == kModeCost) corr_rows<false, false, T>(S, a, b, c, R);
  else if (MODE == kModeOne) {
    if (S.side == 0) corr_rows<true, false, T>(S, a, b, c, R); else corr_rows<false, true, T>(S, a, b, c, R);
  } else corr_rows<true, true, T>(S, a, b, c, R);
}

// The planes and the group list of a set are reached through pointers stored in the LmSet, which the compiler has to treat as
// generic (flat) addresses: flat loads cost an aperture check and count against both wait counters, and a flat address cannot be
// read with a scalar load.  They are HBM allocations: say so.
typedef float lm_v4f __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) lm_v4f* lm_rows_ptr;       // global
typedef const __attribute__((address_space(4))) unsigned* lm_glist_ptr;    // constant for the lifetime of the launch: s_load
__device__ __forceinline__ float4 ld_row(const lm_rows_ptr p, const long long r) {
  lm_v4f v;
  if constexpr (E3D_NT >= 1) v = __builtin_nontemporal_load(p + r); else v = p[r];
  return make_float4(v.x, v.y, v.z, v.w);
}
typedef const __attribute__((address_space(1))) row_v2f* lm_rows2_ptr;
__device__ __forceinline__ float2 ld_row2(const lm_rows2_ptr p, const long long r) {
  row_v2f v;
  if constexpr (E3D_NT >= 1) v = __builtin_nontemporal_load(p + r); else v = p[r];
  return make_float2(v.x, v.y);
}
// The twelve floats of row r.  SPLIT rows (LmSet::V1 set): the source half from the cloud's view, the target half from the pair's
// two planes -- the same 48 bytes as the three planes of a legacy row, in four loads.  Which of the two a set holds is uniform for
// the block and decided once, in front of the body (k_lm_pass, k_lm_cost_multi): each body carries the pointers of its layout only.
template <bool SPLIT>
struct LmRowPtrs {
  lm_rows_ptr pa, pb, pc;      // legacy: A, B, C; split: V0, -, R1
  lm_rows2_ptr pv1, pr0;       // split: V1, R0
  __device__ __forceinline__ explicit LmRowPtrs(const LmSet& S)
      : pa((lm_rows_ptr)S.A), pb((lm_rows_ptr)S.B), pc((lm_rows_ptr)S.C), pv1((lm_rows2_ptr)S.V1), pr0((lm_rows2_ptr)S.R0) {}
  __device__ __forceinline__ void load(const long long r, float4& a, float4& b, float4& c) const {
    a = ld_row(pa, r);
    if constexpr (SPLIT) { const float2 v = ld_row2(pv1, r), t = ld_row2(pr0, r); b = make_float4(v.x, v.y, t.x, t.y); }
    else b = ld_row(pb, r);
    c = ld_row(pc, r);
  }
  // a split row without a partner (NaN in tp.x) becomes the all-zero row, before anything is computed from it
  __device__ __forceinline__ void unmark(float4& a, float4& b, float4& c) const {
    if constexpr (SPLIT) {
      if (b.z != b.z) { a = make_float4(0.f, 0.f, 0.f, 0.f); b = a; c = a; }
    }
  }
};
__device__ __forceinline__ bool lm_block_is_split(const LmSet* __restrict__ sets, const int* __restrict__ block_set, const int gb) {
  return sets[block_set[gb]].V1 != nullptr;
}

// A resident row's local halves into the global frame of the outer iteration: pcl::transformPointCloudWithNormals' operation
// order (icp_point_to_plane.cc:192-195), i.e. the very roundings k_transform_bbox / k_compact_corr apply -- the pass then sees
// the numbers a compacted row would hold.  Block-uniform branches (S sits in SGPRs).
__device__ __forceinline__ void row_to_global(const LmSet& S, float4& a, float4& b, float4& c) {
  if (S.outer & 1) {
    const float3 p = pcl_se3(S.Tos, a.x, a.y, a.z), n = pcl_so3(S.Tos, a.w, b.x, b.y);
    a = make_float4(p.x, p.y, p.z, n.x); b.x = n.y; b.y = n.z;
  }
  if (S.outer & 2) {
    const float3 p = pcl_se3(S.Tot, b.z, b.w, c.x), n = pcl_so3(S.Tot, c.y, c.z, c.w);
    b.z = p.x; b.w = p.y; c = make_float4(p.z, n.x, n.y, n.z);
  }
}
template <typename V4>
__device__ __forceinline__ void row_to_global(const LmSet&, V4&, V4&, V4&) {}     // (packed experimental row types of tools/micro: compacted rows only)

// Output slot layout per block / per set (kLmSlot doubles):
//   [0] cost, [1..21] SS upper, [22..27] bs, [28..48] TT upper, [49..54] bt, [55..90] ST (6x6)
// Every thread walks its correspondences c, c + stride, c + 2 stride, ... in this order and adds row 1 then row 2 of each: the
// per-thread sums, and with the fixed reduction tree the block partials, are the same numbers whatever the loop shape.
// Loop shapes (tools/micro/lm_variants.hip measures them; LmCfg holds the choice per mode):
//   UNR  correspondences per trip (1 or 2);
//   PF   the next trip's float4 loads are issued before the current trip's arithmetic (at 2 - 3 waves per SIMD -- the f64
//        accumulators -- the loads in flight per lane, not the occupancy, have to cover the HBM latency).
template <int MODE, int UNR, bool PF, bool SPLIT = false>
__device__ __forceinline__ void lm_pass_body(const LmSet* __restrict__ sets, const int* __restrict__ block_set, const int block_base,
                                             double* __restrict__ partial) {
  constexpr bool kOne = (MODE == kModeOne);
  constexpr bool kCross = (MODE == kModeTwoCross);
  constexpr int NACC = (MODE == kModeCost) ? 1 : kOne ? 28 : kCross ? kAccCross : kAccTwo;
  const int gb = block_base + blockIdx.x;
  const int si = block_set[gb];
  const LmSet S = sets[si];
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;

  const long long stride = (long long)S.nblocks * kBlock;
  const LmRowPtrs<SPLIT> rows(S);
  const lm_rows_ptr pa = rows.pa, pb = rows.pb, pc = rows.pc;      // (the two-row shape: legacy rows only)
  const lm_glist_ptr gl = (lm_glist_ptr)S.glist;
  const long long lane64 = threadIdx.x & 63;
  long long c = (long long)(gb - S.block_begin) * kBlock + threadIdx.x;
  if (UNR == 2) {
    // (two rows per trip: only the micro-benchmark instantiates this shape, on compacted rows)
    float4 a0, b0, c0, a1, b1, c1;
    if (PF && c + stride < S.n) { a0 = ld_row(pa, c); b0 = ld_row(pb, c); c0 = ld_row(pc, c); a1 = ld_row(pa, c + stride); b1 = ld_row(pb, c + stride); c1 = ld_row(pc, c + stride); }
    while (c + stride < S.n) {
      if (!PF) { a0 = ld_row(pa, c); b0 = ld_row(pb, c); c0 = ld_row(pc, c); a1 = ld_row(pa, c + stride); b1 = ld_row(pb, c + stride); c1 = ld_row(pc, c + stride); }
      const float4 ua = a0, ub = b0, uc = c0, va = a1, vb = b1, vc = c1;
      c += 2 * stride;
      if (PF && c + stride < S.n) { a0 = ld_row(pa, c); b0 = ld_row(pb, c); c0 = ld_row(pc, c); a1 = ld_row(pa, c + stride); b1 = ld_row(pb, c + stride); c1 = ld_row(pc, c + stride); }
      CorrRowsT<float> R;
      lm_rows<MODE, float>(S, ua, ub, uc, R);
      lm_accumulate<MODE, 0, float>(acc, R, S.side);
      lm_rows<MODE, float>(S, va, vb, vc, R);
      lm_accumulate<MODE, 0, float>(acc, R, S.side);
    }
    if (c < S.n) {
      const float4 a = ld_row(pa, c), b = ld_row(pb, c), cc = ld_row(pc, c);
      CorrRowsT<float> R;
      lm_rows<MODE, float>(S, a, b, cc, R);
      lm_accumulate<MODE, 0, float>(acc, R, S.side);
    }
  } else {
    auto trip = [&](float4 ua, float4 ub, float4 uc) {
      rows.unmark(ua, ub, uc);
      row_to_global(S, ua, ub, uc);
      CorrRowsT<float> R;
      lm_rows<MODE, float>(S, ua, ub, uc, R);
      lm_accumulate<MODE, 0, float>(acc, R, S.side);
    };
    float4 a0, b0, c0;
    if (gl) {
      // resident rows: a wave walks whole 64-row groups, so everything that steers the walk is wave-uniform (scalar loads and
      // branches); the group id of the trip after next is requested one trip ahead of the rows it addresses, behind the current
      // trip's arithmetic like the rows themselves
      const int ng = (int)(S.n >> 6), gstride = S.nblocks * (kBlock / kWave);
      int gw = __builtin_amdgcn_readfirstlane((gb - S.block_begin) * (kBlock / kWave) + (int)(threadIdx.x >> 6));
      unsigned g0 = (gw < ng) ? gl[gw] : 0u, g1 = (gw + gstride < ng) ? gl[gw + gstride] : 0u;
      if (gw < ng) { const long long r = ((long long)g0 << 6) | lane64; rows.load(r, a0, b0, c0); }
      while (gw < ng) {
        const float4 ua = a0, ub = b0, uc = c0;
        gw += gstride;
        g0 = g1;
        if (gw + gstride < ng) g1 = gl[gw + gstride];
        if (gw < ng) { const long long r = ((long long)g0 << 6) | lane64; rows.load(r, a0, b0, c0); }
        trip(ua, ub, uc);
      }
    } else {
      if (PF && c < S.n) { rows.load(c, a0, b0, c0); }
      while (c < S.n) {
        if (!PF) { rows.load(c, a0, b0, c0); }
        const float4 ua = a0, ub = b0, uc = c0;
        c += stride;
        if (PF && c < S.n) { rows.load(c, a0, b0, c0); }
        trip(ua, ub, uc);
      }
    }
  }
  // wave reduce -> LDS -> fixed-order block sum
  __shared__ double s[kBlock / kWave][NACC];
  __shared__ double red[NACC];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const double v = wave_sum(acc[i]);
    if (lane == 0) s[w][i] = v;
  }
  __syncthreads();
  if (MODE == kModeTwo || MODE == kModeTwoCross) {
    if (threadIdx.x < NACC) {
      double v = s[0][threadIdx.x];
      for (int k = 1; k < kBlock / kWave; ++k) v += s[k][threadIdx.x];
      red[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x < kLmSlot) {
      const int t = threadIdx.x;
      double v = 0.0;
      if (t < 55 || kCross) { v = red[kLmSlotMap.idx[t]]; if (kLmSlotMap.sgn[t] < 0) v = -v; }
      partial[(size_t)gb * kLmSlot + t] = v;             // kModeTwo: the ST block is never read [QUIRK], zeros
    }
  } else if (threadIdx.x < kLmSlot) {
    double v = 0.0;
    if (threadIdx.x < NACC) {
      v = s[0][threadIdx.x];
      for (int k = 1; k < kBlock / kWave; ++k) v += s[k][threadIdx.x];
    }
    partial[(size_t)gb * kLmSlot + threadIdx.x] = v;   // unused slots of cheaper modes are zero
  }
}

// the loop shape each mode runs with.  Measured on one MI355X (tools/micro/lm_variants.hip, 1e8 correspondences in 8 sets,
// profiles/round3_lm_variants.txt): one correspondence per trip with the next one's loads in flight wins in every mode; three
// waves per SIMD (168 VGPRs) for the two-sided modes, which the 55 / 46 f64 accumulators allow.  The translation unit is built
// with -fno-slp-vectorize: left alone, the compiler packs adjacent scalar f32 operations of these expression trees into
// v_pk_mul_f32 / v_pk_add_f32 and pays for it in moves (k_lm_cost_multi 2.00 -> 1.67 ms, mode 3 0.97 -> 0.91 ms without).
template <int MODE> struct LmCfg { static constexpr int unr = 1; static constexpr bool pf = true; static constexpr int minw = 3; };
template <> struct LmCfg<kModeCost> { static constexpr int unr = 1; static constexpr bool pf = true; static constexpr int minw = 1; };
template <> struct LmCfg<kModeOne> { static constexpr int unr = 1; static constexpr bool pf = true; static constexpr int minw = 2; };

template <int MODE>
__global__ __launch_bounds__(kBlock, LmCfg<MODE>::minw) void k_lm_pass(const LmSet* __restrict__ sets, const int* __restrict__ block_set,
                                                                       int block_base, double* __restrict__ partial) {
  if (lm_block_is_split(sets, block_set, block_base + (int)blockIdx.x)) lm_pass_body<MODE, LmCfg<MODE>::unr, LmCfg<MODE>::pf, true>(sets, block_set, block_base, partial);
  else lm_pass_body<MODE, LmCfg<MODE>::unr, LmCfg<MODE>::pf, false>(sets, block_set, block_base, partial);
}

// a8, batched: the LM tries 1..9 of one inner iteration (lambda doubled each time, icp_point_to_plane_impl.h:216-283)
// only differ in the candidate poses, so their costs are evaluated in ONE pass over the correspondence planes: each
// correspondence is loaded once and pushed through up to kLmMaxPoses pose sets.  Per pose the arithmetic, the per-thread
// order of the correspondences and the reduction tree are exactly those of k_lm_pass, so every cost is bit-identical
// to the one a separate pass would return; the host then takes the first try that lowers the cost, as the
// reference's sequential loop does.  (The usual call is the last one of an outer iteration, where all nine tries fail: an
// early-out after the first few tries would not save it.)  Nine poses are 9 x 80 f32 operations per correspondence, VALU
// bound; the side of a kModeOne pair that has no variables (impl cloud 0, the same inner pose in every candidate) is transformed
// once instead of nine times.
// Round 4: the body takes U rows per trip with the POSES in the outer loop (a pose set is 24 scalar words, x 9 far more than the
// scalar registers hold, so the poses are fetched again for every trip).  Measured (tools/micro/lm_variants.hip, 1e8 rows, nine
// poses): U = 1 1.41 ms, 2 1.49 - 1.55, 3 1.52, 4 1.60 - 1.66 -- the pass is bound by its f32 instructions (0.12 ms per pose and
// 1e8 rows = the chip's f32 issue rate for the ~55 operations of a pose), not by the scalar fetches, and more rows per trip only
// cost occupancy (102 / 139 / 176 VGPRs).  U = 1 it stays.  Per pose a thread adds its rows in the order c, c + stride, ... and row
// by row r1^2 then r2^2: the same sums as k_lm_pass<kModeCost>.
constexpr int kLmCmRows = 1;

template <bool PF, int U = kLmCmRows, bool SPLIT = false>
__device__ __forceinline__ void lm_cost_multi_body(const LmSet* __restrict__ sets, const LmPose* __restrict__ poses, int n_sets,
                                                   int n_poses, const int* __restrict__ block_set, double* __restrict__ partial) {
  const int gb = blockIdx.x;
  const int si = block_set[gb];
  const LmSet S = sets[si];
  double acc[kLmMaxPoses];
#pragma unroll
  for (int k = 0; k < kLmMaxPoses; ++k) acc[k] = 0.0;
  const long long stride = (long long)S.nblocks * kBlock;
  const LmRowPtrs<SPLIT> rows(S);
  const lm_glist_ptr gl = (lm_glist_ptr)S.glist;
  const long long lane64 = threadIdx.x & 63;
  const bool fixed_tgt = (S.mode == kModeOne && S.side == 0), fixed_src = (S.mode == kModeOne && S.side == 1);
  // U rows (valid[u]: the row exists; the others were loaded from a clamped address and add +0.0, which leaves a sum of squares
  // unchanged bit for bit) through every pose
  auto trip = [&](float4* a, float4* b, float4* cc, const bool* valid) {
    CorrPts<float> F[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      rows.unmark(a[u], b[u], cc[u]);
      row_to_global(S, a[u], b[u], cc[u]);
      if (fixed_tgt) corr_tgt<float>(S.Rt, S.tt, b[u].z, b[u].w, cc[u].x, cc[u].y, cc[u].z, cc[u].w, F[u]);
      if (fixed_src) corr_src<float>(S.Rs, S.ts, a[u].x, a[u].y, a[u].z, a[u].w, b[u].x, b[u].y, F[u]);
    }
#pragma unroll
    for (int k = 0; k < kLmMaxPoses; ++k) {
      if (k < n_poses) {
        const LmPose& P = poses[(size_t)k * n_sets + si];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          CorrPts<float> Q = F[u];
          if (!fixed_src) corr_src<float>(P.Rs, P.ts, a[u].x, a[u].y, a[u].z, a[u].w, b[u].x, b[u].y, Q);
          if (!fixed_tgt) corr_tgt<float>(P.Rt, P.tt, b[u].z, b[u].w, cc[u].x, cc[u].y, cc[u].z, cc[u].w, Q);
          CorrRowsT<float> R;
          corr_rows_pts<false, false, float>(Q, R);
          acc[k] += valid[u] ? (double)(R.r1 * R.r1) : 0.0;
          acc[k] += valid[u] ? (double)(R.r2 * R.r2) : 0.0;
        }
      }
    }
  };
  float4 a[U], b[U], cc[U];
  bool valid[U];
  if (gl) {      // resident rows: whole 64-row groups per wave, wave-uniform control (lm_pass_body)
    const int ng = (int)(S.n >> 6), gstride = S.nblocks * (kBlock / kWave);
    int gw = __builtin_amdgcn_readfirstlane((gb - S.block_begin) * (kBlock / kWave) + (int)(threadIdx.x >> 6));
    while (gw < ng) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int gi = gw + u * gstride;
        valid[u] = gi < ng;
        const long long r = ((long long)gl[valid[u] ? gi : gw] << 6) | lane64;
        rows.load(r, a[u], b[u], cc[u]);
      }
      trip(a, b, cc, valid);
      gw += U * gstride;
    }
  } else {
    long long c = (long long)(gb - S.block_begin) * kBlock + threadIdx.x;
    while (c < S.n) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long ci = c + u * stride;
        valid[u] = ci < S.n;
        const long long r = valid[u] ? ci : c;
        rows.load(r, a[u], b[u], cc[u]);
      }
      trip(a, b, cc, valid);
      c += U * stride;
    }
  }
  __shared__ double s[kBlock / kWave][kLmMaxPoses];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kLmMaxPoses; ++i) {
    const double v = wave_sum(acc[i]);
    if (lane == 0) s[w][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kLmSlot) {
    double v = 0.0;
    if (threadIdx.x < kLmMaxPoses) {
      v = s[0][threadIdx.x];
      for (int k = 1; k < kBlock / kWave; ++k) v += s[k][threadIdx.x];
    }
    partial[(size_t)gb * kLmSlot + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(kBlock) void k_lm_cost_multi(const LmSet* __restrict__ sets, const LmPose* __restrict__ poses,
                                                          int n_sets, int n_poses, const int* __restrict__ block_set,
                                                          double* __restrict__ partial) {
  if (lm_block_is_split(sets, block_set, (int)blockIdx.x)) lm_cost_multi_body<true, kLmCmRows, true>(sets, poses, n_sets, n_poses, block_set, partial);
  else lm_cost_multi_body<true, kLmCmRows, false>(sets, poses, n_sets, n_poses, block_set, partial);
}

// one block per set: sum the set's block partials in a fixed order.  kRedParts threads share each of the
// kLmSlot accumulators (interleaved block ranges, 4 independent loads in flight), then a fixed-order
// LDS sum -- deterministic, and no 2048-long chain of dependent HBM loads.
constexpr int kRedParts = 8;
__global__ __launch_bounds__(kLmSlot * kRedParts) void k_lm_reduce(const double* __restrict__ partial,
                                                                   const LmSet* __restrict__ sets, int nacc,
                                                                   double* __restrict__ out) {
  const LmSet S = sets[blockIdx.x];
  const int slot = threadIdx.x % kLmSlot, part = threadIdx.x / kLmSlot;
  __shared__ double sh[kRedParts][kLmSlot];
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  const double* base = partial + (size_t)S.block_begin * kLmSlot + slot;
  int b = part;
  for (; b + 3 * kRedParts < S.nblocks; b += 4 * kRedParts) {
    const double a0 = base[(size_t)b * kLmSlot], a1 = base[(size_t)(b + kRedParts) * kLmSlot];
    const double a2 = base[(size_t)(b + 2 * kRedParts) * kLmSlot], a3 = base[(size_t)(b + 3 * kRedParts) * kLmSlot];
    v0 += a0; v1 += a1; v2 += a2; v3 += a3;
  }
  for (; b < S.nblocks; b += kRedParts) v0 += base[(size_t)b * kLmSlot];
  sh[part][slot] = (v0 + v1) + (v2 + v3);
  __syncthreads();
  if (part == 0 && slot < nacc) {
    double v = sh[0][slot];
#pragma unroll
    for (int k = 1; k < kRedParts; ++k) v += sh[k][slot];
    out[(size_t)blockIdx.x * kLmSlot + slot] = v;
  }
}

// =================================================================================================
// host-side launch helpers
// =================================================================================================
void launch_lm_pass(int mode, const LmSet* sets, const int* block_set, int block_base, int nblocks, double* partial, hipStream_t s) {
  if (nblocks <= 0) return;
  switch (mode) {
    case kModeCost:
      hipLaunchKernelGGL(k_lm_pass<kModeCost>, dim3(nblocks), dim3(kBlock), 0, s, sets, block_set, block_base, partial);
      break;
    case kModeOne:
      hipLaunchKernelGGL(k_lm_pass<kModeOne>, dim3(nblocks), dim3(kBlock), 0, s, sets, block_set, block_base, partial);
      break;
    case kModeTwo:
      hipLaunchKernelGGL(k_lm_pass<kModeTwo>, dim3(nblocks), dim3(kBlock), 0, s, sets, block_set, block_base, partial);
      break;
    default:
      hipLaunchKernelGGL(k_lm_pass<kModeTwoCross>, dim3(nblocks), dim3(kBlock), 0, s, sets, block_set, block_base, partial);
      break;
  }
}

void launch_lm_cost_multi(const LmSet* sets, const LmPose* poses, int n_sets, int n_poses, const int* block_set, int nblocks,
                          double* partial, hipStream_t s) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(k_lm_cost_multi, dim3(nblocks), dim3(kBlock), 0, s, sets, poses, n_sets, n_poses, block_set, partial);
}

void launch_lm_reduce(const double* partial, const LmSet* sets, int n_sets, int nacc, double* out, hipStream_t s) {
  if (n_sets <= 0) return;
  hipLaunchKernelGGL(k_lm_reduce, dim3(n_sets), dim3(kLmSlot * kRedParts), 0, s, partial, sets, nacc, out);
}

}  // namespace e3d
