// e3d_grid.hpp -- the hashed grid and the device primitives every tool shares: launchers of e3d_grid.hip (bounding box, cell
// keys, permutation, cell table) and what e3d_sort.hip defines (the grid builders, rocPRIM sorts and scans, stable compaction).
#pragma once

#include <functional>

#include "e3d_common.hpp"
#include "e3d_kernels.hpp"

namespace e3d {

constexpr int kMaxBboxBlocks = 2048;
// Target-grid cell range a query must fall into to have any candidate (cells of the target's points +- 2),
// used to build dense sort keys for the queries.
struct QueryRange { int lo[3]; unsigned D[3]; };

int launch_transform_aos(const float* xyz, const float* nrm, size_t n, const Affine& T, float* oxyz, float* onrm,
                         float* bbox_partial, float* bbox_out, hipStream_t s);
int launch_transform_bbox(const float4* L4, size_t n, const Affine& T, float4* G4, float* bbox_partial,
                          float* bbox_out, hipStream_t s);
void launch_bbox_aos(const float* xyz, size_t n, float* bbox_partial, float* bbox_out, hipStream_t s);
void launch_cell_keys(const float* xyz, size_t n, const GridDesc& g, unsigned long long* keys, unsigned* vals,
                      hipStream_t s);
void launch_permute(const float* xyz, const float* nrm, const unsigned* order, size_t n, float4* L4, float4* LN,
                    hipStream_t s);
void launch_count_cells(const unsigned long long* keys, size_t n, unsigned* counter, hipStream_t s);
void launch_build_table(const unsigned long long* keys, size_t n, HashEntry* table, unsigned mask, hipStream_t s);
// The hashed grid's table over m sorted cell keys (e3d_sort.hip): counts the occupied cells (one word of `counter`, one
// synchronisation of s), sizes `table` -- the smallest power of two that is >= 64 and >= 2 x cells, so that the linear probing of
// hash_cell_range and table_find_or_insert ends at an empty slot -- fills it with 0xFF and enters the cells.  m == 0: the 64 empty
// slots, nothing counted or entered and no synchronisation.  The caller keeps its buffers; mask goes into its GridDesc.
struct CellTable { unsigned mask, n_cells; };
CellTable build_cell_table(const unsigned long long* sorted_keys, size_t m, DevBuf<unsigned>& counter, DevBuf<HashEntry>& table, hipStream_t s);
// ... with the steps before it: sorts the n (cell key, point index) pairs from keys_a / vals_a into keys_b / vals_b on key bits
// [0, end_bit), writes the first m of them in that order to P4 (and their normals to N4, where nrm and N4 are given: launch_permute;
// both are reserved here, behind the sort's launch, unless they hold m already) and builds the table over their keys.  The n - m
// pairs behind them carry a key above every cell's (points the caller's key kernel left out).
CellTable sort_into_cells(unsigned long long* keys_a, unsigned long long* keys_b, unsigned* vals_a, unsigned* vals_b, size_t n, size_t m, int end_bit,
                          const float* xyz, const float* nrm, DevBuf<float4>& P4, DevBuf<float4>* N4, DevBuf<char>& temp,
                          DevBuf<unsigned>& counter, DevBuf<HashEntry>& table, hipStream_t s);
// radix sort of (cell key, point index) pairs -- rocPRIM device primitive (e3d_sort.hip)
void sort_pairs_u64_u32(unsigned long long* keys_in, unsigned long long* keys_out, unsigned* vals_in,
                        unsigned* vals_out, size_t n, int end_bit, DevBuf<char>& temp, hipStream_t s, size_t n_reserve = 0);
// n_reserve: the temporary storage is sized for a sort of that many elements (a later sort of the same arrays; 0: for n)
void sort_pairs_u32_u32(unsigned* keys_in, unsigned* keys_out, unsigned* vals_in, unsigned* vals_out, size_t n,
                        int end_bit, DevBuf<char>& temp, hipStream_t s, size_t n_reserve = 0);
// radix sort of 64-bit keys alone (rocPRIM, e3d_sort.hip): the voxel, brick and cell lists of the surface reconstruction
void sort_keys_u64(unsigned long long* keys_in, unsigned long long* keys_out, size_t n, int end_bit, DevBuf<char>& temp, hipStream_t s);
// in-place exclusive MAX scan of n unsigned values (rocPRIM, e3d_sort.hip); one-off per grid build
void exclusive_max_scan_u32(unsigned* data, size_t n, DevBuf<char>& temp, hipStream_t s);
// exclusive prefix sum of n 0/1 flags into 32-bit offsets (rocPRIM, e3d_sort.hip): the splat compaction
void exclusive_sum_u8_u32(const unsigned char* in, unsigned* out, size_t n, DevBuf<char>& temp, hipStream_t s);
// a stable compaction's first half: the exclusive offsets of n 0/1 flags and, after a synchronisation of s, the number of flags set
size_t compaction_offsets(const unsigned char* flags, size_t n, DevBuf<unsigned>& offsets, DevBuf<char>& temp, hipStream_t s);
// flags[j] = 1 where keys[j] is the first of a run of equal keys (sorted keys): compacted, the unique keys / the runs' starts
void launch_flag_run_starts(const unsigned long long* keys, size_t n, unsigned char* flags, hipStream_t s);
// The scratch of a call's stable compactions on its stream s: flags, their offsets and rocPRIM's temporary storage
struct Compactor {
  hipStream_t s;
  DevBuf<char> temp;
  DevBuf<unsigned char> flags;
  DevBuf<unsigned> offsets;
  explicit Compactor(hipStream_t stream) : s(stream) {}

  // exclusive offsets of n flags; the number set
  size_t scan(const unsigned char* f, size_t n) { return compaction_offsets(f, n, offsets, temp, s); }
  size_t scan(size_t n) { return scan(flags.p, n); }
  // sorts keys[0, n) (into `sorted`) and leaves their unique values in `out`; the number of unique keys.  scatter(sorted, n, out)
  // launches the caller's kernel that writes sorted[j] to out[offsets[j]] where flags[j] is set.
  template <class Scatter>
  size_t sort_unique(DevBuf<unsigned long long>& keys, DevBuf<unsigned long long>& sorted, DevBuf<unsigned long long>& out, size_t n, int end_bit,
                     Scatter&& scatter) {
    if (n == 0) return 0;
    sorted.reserve(n);
    sort_keys_u64(keys.p, sorted.p, n, end_bit, temp, s);
    flags.reserve(n);
    launch_flag_run_starts(sorted.p, n, flags.p, s);
    const size_t m = scan(n);
    out.reserve(m);
    scatter(sorted.p, n, out.p);
    return m;
  }
};
// the exact kNN (e3d_normals.hip) of a finite cloud (host or device xyz) with each query's k-th squared distance (input order)
// left on the device; `use(kth, query_order, stream)` runs while the kNN workspace is held: query_order lists the queries in
// the pass's grid-cell order (w = input index as bits)
void knn_kth_sqdist(const float* xyz, size_t n, int k, const std::function<void(const float*, const float4*, hipStream_t)>& use);

}  // namespace e3d
