// e3d_stereo_eval.hip -- StereoEvaluator: disparity maps against the two-view ground truth on the MI355X (the rules:
// include/e3d_hip.h, e3d_evaluate_disparity).  The reference has no such code; nothing is restated.
//
//  classify  k_disp_classify, one launch over all estimates: a pixel's class (outside region 0 / region 0 only / regions 0 and 1), its
//            err, the counts (wave ballots into scalar counters), the f64 sums (per lane, wave, block: one slot per block) and the
//            histogram of the top 11 of the 31 bits of err per estimate and class in LDS, flushed with integer atomics; the error map
//  select    radix select, no sort: the bits of a non-negative f32 order as unsigned integers.  k_disp_pick walks a histogram per
//            (estimate, region, percentile): the bin that holds rank k and the rank inside it; targets of one region that chose the
//            same prefix share a slot.  k_disp_refine reads the pixels again and builds per slot the histogram of the next 10 bits of
//            the errors with that prefix.  pick, refine, pick, refine, pick: 11 + 10 + 10 bits.  Nothing is read back in between
//  sums      k_disp_sums: one block per estimate adds the blocks' partial sums in ascending block order
#include <cmath>
#include <vector>

#include "../../include/e3d_hip.h"
#include "e3d_common.hpp"
#include "e3d_kernels.hpp"

#pragma clang fp contract(off)

namespace e3d {

constexpr int kDispBlock = 256;
constexpr int kDispRefineBlock = 1024;
constexpr unsigned kDispClassifyBlocks = 2048;      // per estimate, at most (fixed: the sums' order depends on W H alone)
constexpr unsigned kDispRefineBlocks = 512;
constexpr int kDispMaxT = 8, kDispMaxP = 8;
constexpr int kDispMaxSlots = 2 * kDispMaxP;
constexpr int kDispTopBins = 2048;                  // bits 30 .. 20 of err (bit 31 is 0)
constexpr int kDispDigitBins = 1024;                // bits 19 .. 10, then bits 9 .. 0
constexpr int kDispCounts = 2 + kDispMaxT;          // per class: n_region, n_valid, n_bad[8]
constexpr int kDispSumChunk = 512;                  // blocks whose partial sums k_disp_sums stages at a time
constexpr unsigned kDispNone = 0xFFFFFFFFu;
constexpr int kDispGroups = 3;
static const char* const kDispGroupNames[kDispGroups] = {"classify", "select", "sums"};

struct DispThresholds { float thr[kDispMaxT]; int T; };
struct DispPercentiles { int p[kDispMaxP]; int P; };
// The state of one estimate's selection between the passes.  Target q = region * P + percentile index.  A slot is a (region, prefix)
// pair some target waits for; target_slot is kDispNone for a target without valid pixels.
struct DispSelection {
  unsigned n_slots;
  unsigned slot_prefix[kDispMaxSlots], slot_region[kDispMaxSlots];
  unsigned target_slot[kDispMaxSlots], target_rank[kDispMaxSlots];
};

__device__ const unsigned char kDispPalette[9][3] = {{49, 54, 149},  {69, 117, 180}, {116, 173, 209}, {171, 217, 233}, {254, 224, 144},
                                                     {253, 174, 97}, {244, 109, 67}, {215, 48, 39},   {165, 0, 38}};

__device__ __forceinline__ bool disp_finite(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) < 0x7F800000u; }

// rule 1: -1 outside region 0, 0 in region 0 only, 1 in both regions
__device__ __forceinline__ int disp_class(float g, unsigned m) { return disp_finite(g) && m != 0 ? (m == 255 ? 1 : 0) : -1; }

// Pixel i of estimate e = blockIdx.x / blocks_per_est; every lane of a wave runs the same number of iterations, so the ballots see
// whole waves.  partial[4 blockIdx.x + {0, 1, 2, 3}] = sum1, sum2 of class 0, sum1, sum2 of class 1.
template <bool MAPS>
__global__ __launch_bounds__(kDispBlock) void k_disp_classify(const float* __restrict__ gt, const unsigned char* __restrict__ mask, const float* __restrict__ est,
                                                              size_t n, unsigned blocks_per_est, DispThresholds th, unsigned* __restrict__ ghist,
                                                              unsigned long long* __restrict__ gcounts, double* __restrict__ partial,
                                                              unsigned char* __restrict__ maps) {
  __shared__ unsigned hist[2 * kDispTopBins];
  __shared__ unsigned cnt[2 * kDispCounts];
  __shared__ double wsum[kDispBlock / kWave][4];
  const unsigned e = blockIdx.x / blocks_per_est, b = blockIdx.x % blocks_per_est;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < 2 * kDispTopBins; j += kDispBlock) hist[j] = 0;
  if (threadIdx.x < 2 * kDispCounts) cnt[threadIdx.x] = 0;
  __syncthreads();

  const float* __restrict__ x = est + (size_t)e * n;
  const size_t stride = (size_t)blocks_per_est * kDispBlock;
  const size_t iterations = (n + stride - 1) / stride;
  unsigned c_region[2] = {0, 0}, c_valid[2] = {0, 0}, c_bad[2][kDispMaxT];
#pragma unroll
  for (int t = 0; t < kDispMaxT; ++t) { c_bad[0][t] = 0; c_bad[1][t] = 0; }
  double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
  for (size_t it = 0; it < iterations; ++it) {
    const size_t i = it * stride + (size_t)b * kDispBlock + threadIdx.x;
    const bool in = i < n;
    float g = INFINITY, v = 0.f;
    unsigned m = 0;
    if (in) { g = gt[i]; v = x[i]; m = mask ? (unsigned)mask[i] : 255u; }
    const int cls = disp_class(g, m);
    const bool valid = cls >= 0 && disp_finite(v);
    const float err = fabsf(v - g);
    const unsigned long long m0 = __ballot(cls == 0), m1 = __ballot(cls == 1), mv = __ballot(valid);
    c_region[0] += __popcll(m0); c_region[1] += __popcll(m1);
    c_valid[0] += __popcll(mv & m0); c_valid[1] += __popcll(mv & m1);
    int c = 0;
#pragma unroll
    for (int t = 0; t < kDispMaxT; ++t) {
      if (t < th.T) {
        const bool bad = valid && err > th.thr[t];
        const unsigned long long mb = __ballot(bad);
        c += bad ? 1 : 0;
        c_bad[0][t] += __popcll(mb & m0); c_bad[1][t] += __popcll(mb & m1);
      }
    }
    const double d = valid ? (double)err : 0.0, dd = d * d;
    s1[0] += cls == 0 ? d : 0.0; s2[0] += cls == 0 ? dd : 0.0;
    s1[1] += cls == 1 ? d : 0.0; s2[1] += cls == 1 ? dd : 0.0;
    const unsigned bin = ((unsigned)(cls & 1) << 11) | ((__float_as_uint(err) >> 20) & (kDispTopBins - 1));
    if (valid) atomicAdd(&hist[bin], 1u);
    if (MAPS && in) {
      unsigned r = 0, gg = 0, bl = 0;
      if (cls >= 0) {
        if (valid) { const unsigned char* p = kDispPalette[(c * 8) / th.T]; r = p[0]; gg = p[1]; bl = p[2]; }
        else { r = 255; bl = 255; }
        if (cls == 0) { r >>= 1; gg >>= 1; bl >>= 1; }
      }
      unsigned char* o = maps + ((size_t)e * n + i) * 3;
      o[0] = (unsigned char)r; o[1] = (unsigned char)gg; o[2] = (unsigned char)bl;
    }
  }

#pragma unroll
  for (int k = 0; k < 2; ++k) { s1[k] = wave_sum(s1[k]); s2[k] = wave_sum(s2[k]); }
  if (lane == 0) {
    wsum[wv][0] = s1[0]; wsum[wv][1] = s2[0]; wsum[wv][2] = s1[1]; wsum[wv][3] = s2[1];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (c_region[k]) atomicAdd(&cnt[k * kDispCounts], c_region[k]);
      if (c_valid[k]) atomicAdd(&cnt[k * kDispCounts + 1], c_valid[k]);
#pragma unroll
      for (int t = 0; t < kDispMaxT; ++t)
        if (c_bad[k][t]) atomicAdd(&cnt[k * kDispCounts + 2 + t], c_bad[k][t]);
    }
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double s = wsum[0][threadIdx.x];
    for (int w = 1; w < kDispBlock / kWave; ++w) s += wsum[w][threadIdx.x];
    partial[(size_t)blockIdx.x * 4 + threadIdx.x] = s;
  }
  if (threadIdx.x < 2 * kDispCounts) {
    const unsigned v = cnt[threadIdx.x];
    if (v) atomicAdd(&gcounts[(size_t)e * (2 * kDispCounts) + threadIdx.x], (unsigned long long)v);
  }
  for (int j = threadIdx.x; j < 2 * kDispTopBins; j += kDispBlock) {
    const unsigned v = hist[j];
    if (v) atomicAdd(&ghist[(size_t)e * (2 * kDispTopBins) + j], v);
  }
}

// One block per estimate, one wave per target q = region * P + percentile index.  level 0: hist is the classify pass's
// [estimate][class][2048], the rank is rule 6's k of the region's n_valid.  level 1, 2: hist is the refine pass's
// [estimate][slot][1024], the rank is the one the level before left.  The wave's lanes each add up a run of bins, a scan over the
// lanes finds the lane whose run holds the rank, and that lane walks its run.  Thread 0 then gives the targets of one region that chose
// the same prefix one slot (levels 0 and 1); at level 2 the prefix is err's 31 bits, the quantile.  A target without valid pixels gets
// NaN at level 0 and no slot.
__global__ __launch_bounds__(kDispRefineBlock) void k_disp_pick(int level, const unsigned* __restrict__ hist, const unsigned long long* __restrict__ gcounts,
                                                                DispPercentiles pc, DispSelection* __restrict__ sel, unsigned* __restrict__ quantile_bits) {
  __shared__ unsigned new_prefix[kDispMaxSlots], new_rank[kDispMaxSlots];
  const unsigned e = blockIdx.x;
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, P = pc.P;
  if (threadIdx.x < kDispMaxSlots) { new_prefix[threadIdx.x] = kDispNone; new_rank[threadIdx.x] = 0; }
  __syncthreads();
  if (q < 2 * P) {
    const int region = q / P;
    unsigned rank = 0, old_prefix = 0;
    const unsigned* h0 = nullptr;
    const unsigned* h1 = nullptr;                  // level 0, region 0: the sum of both classes
    int bins = 0;
    if (level == 0) {
      const unsigned long long* c = gcounts + (size_t)e * (2 * kDispCounts);
      const long long n_valid = (long long)(region == 1 ? c[kDispCounts + 1] : c[1] + c[kDispCounts + 1]);
      if (n_valid > 0) {
        rank = (unsigned)(((long long)pc.p[q % P] * n_valid + 99) / 100 - 1);
        h0 = hist + (size_t)e * (2 * kDispTopBins) + kDispTopBins;
        if (region == 0) h1 = hist + (size_t)e * (2 * kDispTopBins);
        bins = kDispTopBins;
      } else if (lane == 0) {
        quantile_bits[(size_t)e * (2 * P) + q] = 0x7FC00000u;
      }
    } else {
      const unsigned slot = sel[e].target_slot[q];
      if (slot != kDispNone) {
        rank = sel[e].target_rank[q];
        old_prefix = sel[e].slot_prefix[slot];
        h0 = hist + ((size_t)e * kDispMaxSlots + slot) * kDispDigitBins;
        bins = kDispDigitBins;
      }
    }
    if (bins) {
      const int run = bins / 64, first = lane * run;
      unsigned mine = 0;
      for (int j = 0; j < run; ++j) mine += h0[first + j] + (h1 ? h1[first + j] : 0u);
      unsigned incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      unsigned cum = incl - mine;
      if (cum <= rank && rank < incl) {
        for (int j = 0; j < run; ++j) {
          const unsigned h = h0[first + j] + (h1 ? h1[first + j] : 0u);
          if (rank < cum + h) {
            new_prefix[q] = level == 0 ? (unsigned)(first + j) : ((old_prefix << 10) | (unsigned)(first + j));
            new_rank[q] = rank - cum;
            break;
          }
          cum += h;
        }
      }
    }
  }
  __syncthreads();                                 // every read of sel[e] lies before it, every write behind it
  if (level == 2) {
    if ((int)threadIdx.x < 2 * P && sel[e].target_slot[threadIdx.x] != kDispNone)
      quantile_bits[(size_t)e * (2 * P) + threadIdx.x] = new_prefix[threadIdx.x] == kDispNone ? 0x7FC00000u : new_prefix[threadIdx.x];
    return;
  }
  if (threadIdx.x == 0) {
    DispSelection& S = sel[e];
    unsigned n_slots = 0;
    for (int t = 0; t < kDispMaxSlots; ++t) {
      unsigned slot = kDispNone;
      if (t < 2 * P && new_prefix[t] != kDispNone) {
        const unsigned region = (unsigned)(t / P);
        for (unsigned s = 0; s < n_slots; ++s)
          if (S.slot_region[s] == region && S.slot_prefix[s] == new_prefix[t]) { slot = s; break; }
        if (slot == kDispNone) { slot = n_slots++; S.slot_region[slot] = region; S.slot_prefix[slot] = new_prefix[t]; }
      }
      S.target_slot[t] = slot;
      S.target_rank[t] = new_rank[t];
    }
    S.n_slots = n_slots;
  }
}

// Per slot of the estimate the histogram of bits [shift - 10, shift) of the errors whose bits from `shift` up equal the slot's prefix
// and whose pixel lies in the slot's region.  A pixel matches one slot per region at most.
__global__ __launch_bounds__(kDispRefineBlock) void k_disp_refine(const float* __restrict__ gt, const unsigned char* __restrict__ mask, const float* __restrict__ est,
                                                                  size_t n, unsigned blocks_per_est, int shift, const DispSelection* __restrict__ sel,
                                                                  unsigned* __restrict__ slot_hist) {
  __shared__ unsigned hist[kDispMaxSlots * kDispDigitBins];
  __shared__ unsigned s_prefix[kDispMaxSlots], s_region[kDispMaxSlots], s_slots;
  const unsigned e = blockIdx.x / blocks_per_est, b = blockIdx.x % blocks_per_est;
  if (threadIdx.x < kDispMaxSlots) { s_prefix[threadIdx.x] = sel[e].slot_prefix[threadIdx.x]; s_region[threadIdx.x] = sel[e].slot_region[threadIdx.x]; }
  if (threadIdx.x == 0) s_slots = min(sel[e].n_slots, (unsigned)kDispMaxSlots);
  __syncthreads();
  const unsigned n_slots = s_slots;
  if (n_slots == 0) return;
  for (unsigned j = threadIdx.x; j < n_slots * kDispDigitBins; j += kDispRefineBlock) hist[j] = 0;
  __syncthreads();
  const float* __restrict__ x = est + (size_t)e * n;
  const size_t stride = (size_t)blocks_per_est * kDispRefineBlock;
  for (size_t i = (size_t)b * kDispRefineBlock + threadIdx.x; i < n; i += stride) {
    const float g = gt[i], v = x[i];
    const int cls = disp_class(g, mask ? (unsigned)mask[i] : 255u);
    if (cls < 0 || !disp_finite(v)) continue;
    const unsigned bits = __float_as_uint(fabsf(v - g));
    const unsigned prefix = bits >> shift, digit = (bits >> (shift - 10)) & (kDispDigitBins - 1);
    for (unsigned s = 0; s < n_slots; ++s)
      if (s_prefix[s] == prefix && (s_region[s] == 0 || cls == 1)) atomicAdd(&hist[s * kDispDigitBins + digit], 1u);
  }
  __syncthreads();
  for (unsigned j = threadIdx.x; j < n_slots * kDispDigitBins; j += kDispRefineBlock) {
    const unsigned v = hist[j];
    if (v) atomicAdd(&slot_hist[(size_t)e * (kDispMaxSlots * kDispDigitBins) + j], v);
  }
}

// One block per estimate: the blocks' partial sums added in ascending block order, one thread per sum, staged through LDS a chunk
// at a time.  sums[4 e + ...] = region 0's sum1, sum2 (class 0 + class 1), region 1's sum1, sum2 (class 1).
__global__ __launch_bounds__(kDispBlock) void k_disp_sums(const double* __restrict__ partial, unsigned blocks_per_est, double* __restrict__ sums) {
  __shared__ double stage[4 * kDispSumChunk];
  __shared__ double total[4];
  const double* __restrict__ p = partial + (size_t)blockIdx.x * blocks_per_est * 4;
  double s = 0.0;
  for (unsigned begin = 0; begin < blocks_per_est; begin += kDispSumChunk) {
    const unsigned count = min((unsigned)kDispSumChunk, blocks_per_est - begin);
    for (unsigned j = threadIdx.x; j < 4 * count; j += kDispBlock) stage[j] = p[(size_t)4 * begin + j];
    __syncthreads();
    if (threadIdx.x < 4)
      for (unsigned k = 0; k < count; ++k) s += stage[4 * k + threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x < 4) total[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = sums + (size_t)blockIdx.x * 4;
    o[0] = total[0] + total[2]; o[1] = total[1] + total[3]; o[2] = total[2]; o[3] = total[3];
  }
}

}  // namespace e3d

using namespace e3d;

struct e3d_disp_eval {
  int n_est = 0, T = 0, P = 0;
  std::vector<int64_t> counts;                     // [n_est][2][2 + T]
  std::vector<double> sums;                        // [n_est][2][2]
  std::vector<float> quantiles;                    // [n_est][2][P]
  float ms[kDispGroups] = {0, 0, 0};
};

namespace {

// the caller's array on the device: as it is if it lies there, else a copy in `own`
template <typename T>
const T* on_device(const T* src, size_t count, DevBuf<T>& own, hipStream_t s) {
  if (is_device_pointer(src)) return src;
  own.reserve(count);
  copy_in(own.p, src, sizeof(T) * count, s);
  return own.p;
}

void evaluate(e3d_disp_eval& out, const float* gt, const uint8_t* mask, int width, int height, const float* estimates, int n_est, const float* thresholds, int T,
              const int32_t* percentiles, int P, uint8_t* error_maps) {
  const char* const fn = "e3d_evaluate_disparity";
  if (width < 1 || height < 1) throw Error(E3D_ERR_INVALID, fmt("%s: size %d x %d", fn, width, height));
  const size_t n = (size_t)width * (size_t)height;
  if (n >= (size_t)1 << 31) throw Error(E3D_ERR_INVALID, fmt("%s: %d x %d pixels, fewer than 2^31 are supported", fn, width, height));
  if (n_est < 1) throw Error(E3D_ERR_INVALID, fmt("%s: at least one estimate is needed", fn));
  if (T < 1 || T > kDispMaxT) throw Error(E3D_ERR_INVALID, fmt("%s: %d thresholds, 1 to %d are supported", fn, T, kDispMaxT));
  if (P < 0 || P > kDispMaxP) throw Error(E3D_ERR_INVALID, fmt("%s: %d percentiles, 0 to %d are supported", fn, P, kDispMaxP));
  if (!gt || !estimates || !thresholds || (P > 0 && !percentiles)) throw Error(E3D_ERR_INVALID, fmt("%s: null argument", fn));
  DispThresholds th{};
  th.T = T;
  for (int t = 0; t < T; ++t) {
    const float v = thresholds[t];
    if (!std::isfinite(v) || !(v >= 0.f) || (t > 0 && !(v > thresholds[t - 1])))
      throw Error(E3D_ERR_INVALID, fmt("%s: the thresholds must be finite, not negative and strictly ascending", fn));
    th.thr[t] = v;
  }
  DispPercentiles pc{};
  pc.P = P;
  for (int k = 0; k < P; ++k) {
    if (percentiles[k] < 1 || percentiles[k] > 100) throw Error(E3D_ERR_INVALID, fmt("%s: percentile %d, 1 to 100 are supported", fn, (int)percentiles[k]));
    pc.p[k] = percentiles[k];
  }
  const unsigned classify_blocks = (unsigned)std::min<size_t>(div_up(n, kDispBlock), kDispClassifyBlocks);
  const unsigned refine_blocks = (unsigned)std::min<size_t>(div_up(n, kDispRefineBlock), kDispRefineBlocks);
  const size_t E = (size_t)n_est;
  if (E * classify_blocks >= (size_t)1 << 31) throw Error(E3D_ERR_INVALID, fmt("%s: %d estimates of %zu pixels are too many for one call", fn, n_est, n));
  require_device();

  out.n_est = n_est; out.T = T; out.P = P;
  OwnedStream stream;
  hipStream_t s = stream.s;
  DevBuf<float> own_gt, own_est;
  DevBuf<unsigned char> own_mask, maps;
  DevBuf<unsigned> ghist, slot_hist, quantile_bits;
  DevBuf<unsigned long long> gcounts;
  DevBuf<double> partial, sums;
  DevBuf<DispSelection> sel;
  GroupTimer timer[kDispGroups];

  const float* d_gt = on_device(gt, n, own_gt, s);
  const unsigned char* d_mask = mask ? on_device(mask, n, own_mask, s) : nullptr;
  const float* d_est = on_device(estimates, E * n, own_est, s);
  ghist.reserve(E * 2 * kDispTopBins); gcounts.reserve(E * 2 * kDispCounts); partial.reserve(E * classify_blocks * 4); sums.reserve(E * 4);
  if (error_maps) maps.reserve(E * n * 3);
  if (P > 0) { slot_hist.reserve(E * kDispMaxSlots * kDispDigitBins); quantile_bits.reserve(E * 2 * P); sel.reserve(E); }
  E3D_HIP(hipMemsetAsync(ghist.p, 0, sizeof(unsigned) * E * 2 * kDispTopBins, s));
  E3D_HIP(hipMemsetAsync(gcounts.p, 0, sizeof(unsigned long long) * E * 2 * kDispCounts, s));
  if (P > 0) E3D_HIP(hipMemsetD32Async((hipDeviceptr_t)quantile_bits.p, 0x7FC00000, E * 2 * P, s));   // NaN until a target's last pick

  timer[0].start(s);
  if (error_maps)
    hipLaunchKernelGGL(k_disp_classify<true>, dim3((unsigned)(E * classify_blocks)), dim3(kDispBlock), 0, s, d_gt, d_mask, d_est, n, classify_blocks, th, ghist.p,
                       gcounts.p, partial.p, maps.p);
  else
    hipLaunchKernelGGL(k_disp_classify<false>, dim3((unsigned)(E * classify_blocks)), dim3(kDispBlock), 0, s, d_gt, d_mask, d_est, n, classify_blocks, th, ghist.p,
                       gcounts.p, partial.p, (unsigned char*)nullptr);
  timer[0].stop(s);

  timer[1].start(s);
  if (P > 0) {
    const dim3 pick_block((unsigned)(2 * P * kWave));
    hipLaunchKernelGGL(k_disp_pick, dim3((unsigned)E), pick_block, 0, s, 0, ghist.p, gcounts.p, pc, sel.p, quantile_bits.p);
    for (int level = 1; level <= 2; ++level) {
      E3D_HIP(hipMemsetAsync(slot_hist.p, 0, sizeof(unsigned) * E * kDispMaxSlots * kDispDigitBins, s));
      hipLaunchKernelGGL(k_disp_refine, dim3((unsigned)(E * refine_blocks)), dim3(kDispRefineBlock), 0, s, d_gt, d_mask, d_est, n, refine_blocks, 30 - 10 * level,
                         sel.p, slot_hist.p);
      hipLaunchKernelGGL(k_disp_pick, dim3((unsigned)E), pick_block, 0, s, level, slot_hist.p, gcounts.p, pc, sel.p, quantile_bits.p);
    }
  }
  timer[1].stop(s);

  timer[2].start(s);
  hipLaunchKernelGGL(k_disp_sums, dim3((unsigned)E), dim3(kDispBlock), 0, s, partial.p, classify_blocks, sums.p);
  timer[2].stop(s);

  std::vector<unsigned long long> class_counts(E * 2 * kDispCounts);
  out.sums.resize(E * 4); out.quantiles.resize(E * 2 * P);
  copy_out(class_counts.data(), gcounts.p, sizeof(unsigned long long) * class_counts.size(), s);
  copy_out(out.sums.data(), sums.p, sizeof(double) * out.sums.size(), s);
  copy_out(out.quantiles.data(), quantile_bits.p, sizeof(float) * out.quantiles.size(), s);
  if (error_maps) copy_out(error_maps, maps.p, E * n * 3, s);
  E3D_HIP(hipStreamSynchronize(s));                // the call's one synchronisation
  E3D_HIP(hipGetLastError());

  // region 0 = class 0 + class 1, region 1 = class 1
  out.counts.resize(E * 2 * (2 + T));
  for (size_t e = 0; e < E; ++e)
    for (int k = 0; k < 2 + T; ++k) {
      const unsigned long long c0 = class_counts[(e * 2) * kDispCounts + k], c1 = class_counts[(e * 2 + 1) * kDispCounts + k];
      out.counts[(e * 2) * (2 + T) + k] = (int64_t)(c0 + c1);
      out.counts[(e * 2 + 1) * (2 + T) + k] = (int64_t)c1;
    }
  for (int g = 0; g < kDispGroups; ++g) out.ms[g] = timer[g].ms();
}

}  // namespace

extern "C" {

e3d_disp_eval_t* e3d_evaluate_disparity(const float* gt, const uint8_t* mask, int width, int height, const float* estimates, int n_estimates,
                                        const float* thresholds, int n_thresholds, const int32_t* percentiles, int n_percentiles, uint8_t* error_maps) {
  e3d_disp_eval* h = nullptr;
  E3D_TRY
  h = new e3d_disp_eval;
  evaluate(*h, gt, mask, width, height, estimates, n_estimates, thresholds, n_thresholds, percentiles, n_percentiles, error_maps);
  return h;
  E3D_CATCH_NEW(h)
}

void e3d_disp_eval_destroy(e3d_disp_eval_t* h) { delete h; }

int e3d_disp_eval_get_counts(e3d_disp_eval_t* h, int64_t* counts) {
  E3D_TRY
  if (!h || !counts) throw Error(E3D_ERR_INVALID, "e3d_disp_eval_get_counts: null argument");
  memcpy(counts, h->counts.data(), sizeof(int64_t) * h->counts.size());
  return 0;
  E3D_CATCH()
}

int e3d_disp_eval_get_sums(e3d_disp_eval_t* h, double* sums) {
  E3D_TRY
  if (!h || !sums) throw Error(E3D_ERR_INVALID, "e3d_disp_eval_get_sums: null argument");
  memcpy(sums, h->sums.data(), sizeof(double) * h->sums.size());
  return 0;
  E3D_CATCH()
}

int e3d_disp_eval_get_quantiles(e3d_disp_eval_t* h, float* quantiles) {
  E3D_TRY
  if (!h || (!quantiles && !h->quantiles.empty())) throw Error(E3D_ERR_INVALID, "e3d_disp_eval_get_quantiles: null argument");
  if (!h->quantiles.empty()) memcpy(quantiles, h->quantiles.data(), sizeof(float) * h->quantiles.size());
  return 0;
  E3D_CATCH()
}

int e3d_disp_eval_kernel_ms(e3d_disp_eval_t* h, float* ms, const char** names, int capacity) {
  E3D_TRY
  if (!h) throw Error(E3D_ERR_INVALID, "e3d_disp_eval_kernel_ms: null handle");
  for (int g = 0; g < kDispGroups && g < capacity; ++g) {
    if (ms) ms[g] = h->ms[g];
    if (names) names[g] = kDispGroupNames[g];
  }
  return kDispGroups;
  E3D_CATCH()
}

}  // extern "C"
