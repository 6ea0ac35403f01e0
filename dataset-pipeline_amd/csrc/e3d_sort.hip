// e3d_sort.hip -- the library's rocPRIM primitives and the host side of the hashed grid (declarations: e3d_grid.hpp): the radix sorts
// of (key, index) pairs and of 64-bit keys, the exclusive MAX and sum scans, the stable compaction's offsets and run-start flags
// (Compactor), and the grid builders build_cell_table / sort_into_cells over the kernels of e3d_grid.hip.  The sorts
// are the library primitive (its onesweep kernel with the gfx950 tuning).  The pair sort runs at every grid build (one-off per cloud and search radius) AND on the
// per-iteration path: once per batch of directed pairs for the far lists of the first outer iterations (e3d_icp.hip: find_pairs_multi).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "e3d_grid.hpp"

namespace e3d {

// rocPRIM's temporary storage for a pair sort is a second copy of the arrays (8 - 12 B per element) plus histograms.  The far lists of an
// ICP run are sorted once per batch of pairs and outer iteration, and the number of queries that survive the pruning key kernel GROWS
// while two scans approach each other: a buffer sized for the sort at hand was re-allocated inside later, timed iterations (hipFree +
// hipMalloc of 2 GB beside 125 GB of resident rows: milliseconds as a rule, 2.8 s once in eight sessions).  n_reserve = the largest n a
// later sort of the same arrays can have (the lists' total length): the buffer is sized for that once.  E3D_ALLOC_TRACE=1 reports growth.
template <class K>
static void sort_pairs_impl(K* keys_in, K* keys_out, unsigned* vals_in, unsigned* vals_out, size_t n, int end_bit, DevBuf<char>& temp, hipStream_t s,
                            size_t n_reserve) {
  if (n == 0) return;
  size_t bytes = 0, need = 0;
  E3D_HIP(rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, n, 0u, (unsigned)end_bit, s));
  need = bytes;
  if (bytes > temp.cap && n_reserve > n)
    E3D_HIP(rocprim::radix_sort_pairs(nullptr, need, keys_in, keys_out, vals_in, vals_out, n_reserve, 0u, (unsigned)end_bit, s));
  need = std::max(need, bytes);
  static const bool trace = [] { const char* e = getenv("E3D_ALLOC_TRACE"); return e && e[0] == '1'; }();
  if (trace && need > temp.cap) fprintf(stderr, "[sort] temporary storage %zu -> %zu bytes (n = %zu, this sort needs %zu)\n", temp.cap, need, n, bytes);
  temp.reserve(need);
  E3D_HIP(rocprim::radix_sort_pairs(temp.p, bytes, keys_in, keys_out, vals_in, vals_out, n, 0u, (unsigned)end_bit, s));
}

void sort_pairs_u64_u32(unsigned long long* keys_in, unsigned long long* keys_out, unsigned* vals_in,
                        unsigned* vals_out, size_t n, int end_bit, DevBuf<char>& temp, hipStream_t s, size_t n_reserve) {
  sort_pairs_impl(keys_in, keys_out, vals_in, vals_out, n, end_bit, temp, s, n_reserve);
}

void sort_pairs_u32_u32(unsigned* keys_in, unsigned* keys_out, unsigned* vals_in, unsigned* vals_out, size_t n,
                        int end_bit, DevBuf<char>& temp, hipStream_t s, size_t n_reserve) {
  sort_pairs_impl(keys_in, keys_out, vals_in, vals_out, n, end_bit, temp, s, n_reserve);
}

void sort_keys_u64(unsigned long long* keys_in, unsigned long long* keys_out, size_t n, int end_bit, DevBuf<char>& temp, hipStream_t s) {
  if (n == 0) return;
  size_t bytes = 0;
  E3D_HIP(rocprim::radix_sort_keys(nullptr, bytes, keys_in, keys_out, n, 0u, (unsigned)end_bit, s));
  temp.reserve(bytes);
  E3D_HIP(rocprim::radix_sort_keys(temp.p, bytes, keys_in, keys_out, n, 0u, (unsigned)end_bit, s));
}

void exclusive_max_scan_u32(unsigned* data, size_t n, DevBuf<char>& temp, hipStream_t s) {
  if (n == 0) return;
  size_t bytes = 0;
  E3D_HIP(rocprim::exclusive_scan(nullptr, bytes, data, data, 0u, n, rocprim::maximum<unsigned>(), s));
  temp.reserve(bytes);
  E3D_HIP(rocprim::exclusive_scan(temp.p, bytes, data, data, 0u, n, rocprim::maximum<unsigned>(), s));
}

void exclusive_sum_u8_u32(const unsigned char* in, unsigned* out, size_t n, DevBuf<char>& temp, hipStream_t s) {
  if (n == 0) return;
  size_t bytes = 0;
  E3D_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<unsigned>(), s));
  temp.reserve(bytes);
  E3D_HIP(rocprim::exclusive_scan(temp.p, bytes, in, out, 0u, n, rocprim::plus<unsigned>(), s));
}

size_t compaction_offsets(const unsigned char* flags, size_t n, DevBuf<unsigned>& offsets, DevBuf<char>& temp, hipStream_t s) {
  if (n == 0) return 0;
  offsets.reserve(n);
  exclusive_sum_u8_u32(flags, offsets.p, n, temp, s);
  unsigned last = 0; unsigned char lf = 0;
  copy_out(&last, offsets.p + (n - 1), sizeof last, s);
  copy_out(&lf, flags + (n - 1), 1, s);
  E3D_HIP(hipStreamSynchronize(s));
  return (size_t)last + (lf ? 1 : 0);
}

CellTable build_cell_table(const unsigned long long* sorted_keys, size_t m, DevBuf<unsigned>& counter, DevBuf<HashEntry>& table, hipStream_t s) {
  unsigned n_cells = 0;
  if (m > 0) {
    counter.reserve(1);
    E3D_HIP(hipMemsetAsync(counter.p, 0, sizeof(unsigned), s));
    launch_count_cells(sorted_keys, m, counter.p, s);
    copy_out(&n_cells, counter.p, sizeof n_cells, s);
    E3D_HIP(hipStreamSynchronize(s));
  }
  size_t tsize = 64;
  while (tsize < 2 * (size_t)n_cells) tsize <<= 1;
  table.reserve(tsize);
  const unsigned mask = (unsigned)(tsize - 1);
  E3D_HIP(hipMemsetAsync(table.p, 0xFF, sizeof(HashEntry) * tsize, s));
  if (m > 0) launch_build_table(sorted_keys, m, table.p, mask, s);
  return CellTable{mask, n_cells};
}

CellTable sort_into_cells(unsigned long long* keys_a, unsigned long long* keys_b, unsigned* vals_a, unsigned* vals_b, size_t n, size_t m, int end_bit,
                          const float* xyz, const float* nrm, DevBuf<float4>& P4, DevBuf<float4>* N4, DevBuf<char>& temp,
                          DevBuf<unsigned>& counter, DevBuf<HashEntry>& table, hipStream_t s) {
  if (m > 0) {
    sort_pairs_u64_u32(keys_a, keys_b, vals_a, vals_b, n, end_bit, temp, s);
    P4.reserve(m);
    if (N4) N4->reserve(m);
    launch_permute(xyz, nrm, vals_b, m, P4.p, N4 ? N4->p : nullptr, s);
  }
  return build_cell_table(keys_b, m, counter, table, s);
}

__global__ __launch_bounds__(kBlock) void k_flag_run_starts(const unsigned long long* __restrict__ keys, size_t n, unsigned char* __restrict__ flags) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) flags[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1 : 0;
}

void launch_flag_run_starts(const unsigned long long* keys, size_t n, unsigned char* flags, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_flag_run_starts, dim3((unsigned)div_up(n, kBlock)), dim3(kBlock), 0, s, keys, n, flags);
}

}  // namespace e3d
