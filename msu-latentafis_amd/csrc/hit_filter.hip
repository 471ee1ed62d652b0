// hit_filter.hip — device code of the filtered hit lists (afis_filter.cpp: afis_rank_hits_filtered, afis_rank_subject_hits_filtered): the cells of the last search's
// matrix a query is not ELIGIBLE for — by the attribute word of the column's template (afis_labels_create) against the query's three masks, or by the query's exclusion
// list — are taken out of a COPY of the matrix, and k_rank_hits (rank_hits.hip) and k_subject_best (subject_rank.hip) rank the copy as they rank a search's, unchanged.
// The matrix itself is never written.
//
// An ineligible cell becomes kNoEntryWord (score_order.h), whose ordered word is 0.
//   templates  k_rank_hits takes thr >= 1, so the cell is neither counted nor listed, whatever min_score is
//   subjects   k_subject_best makes the composite (0 << 32 | ~position) of it: every eligible cell of the subject has an ordered word >= 1 and wins the maximum, and a
//              subject left with ineligible cells only holds a composite whose high half is 0, which k_rank_hits<subjects> never counts (w >= thr fails)
// A matrix cell that already holds that word cannot be told from an ineligible one; a search never produces such a cell (its scores are -1 or finite values >= +0.0).
//
// The label test of cell (q, t), L the label of the template at column t, (any_of, all_of, none_of) = masks[q]:
//   (any_of == 0 || (L & any_of) != 0) && (L & all_of) == all_of && (L & none_of) == 0
//
// k_filter_rows: scores[n_q][G] -> filtered[n_q][G].  Grid = (column chunks, strips of kHfRows query rows).  A thread owns one column — or, where every row starts on a
// 16-byte boundary (G % 4 == 0), four adjacent ones that travel as one 16-byte word, as in k_case_fuse — loads the labels of its columns ONCE (for a subset search through
// one more look-up, labels[d_global[p] - index_base]) and walks the rows of its strip: per cell 4 bytes in and 4 bytes out against 8 / kHfRows bytes of label.  The row
// index depends on the block index and the loop counter only, so a query's three masks are uniform over the workgroup and are read as scalars.  A whole strip's
// loads are issued before its first store, so kHfRows rows are in flight per thread; the last, shorter strip goes row by row.  No atomics, no cross-lane traffic.
// k_filter_drop: the exclusions, as (row, column) pairs the host resolved (a full search's column is idx - index_base; a subset's device order is ascending global
// index; a subject handle's ids are sorted): a 32-bit kNoEntryWord into the filtered matrix, or a 64-bit 0 ("no entry") into best[n_q][S] after k_subject_best ran.
// Duplicated pairs write the same word twice.
// Every index into the matrices is a size_t: n_q x G may pass 2^31.  A grid's second dimension holds 65 535 blocks; more strips than that are walked in a loop.
#include "afis_device.h"
#include <type_traits>

namespace afis {

constexpr int kHfThreads = 256;
constexpr int kHfRows = kFilterRows;                                        // query rows per strip (afis_device.h): the labels of a column are loaded once per strip

__device__ __forceinline__ uint32_t hf_cell(uint32_t v, u64 L, u64 any_of, u64 all_of, u64 none_of)
{
    const bool pass = (any_of == 0 || (L & any_of) != 0) && (L & all_of) == all_of && (L & none_of) == 0;
    return pass ? v : kNoEntryWord;
}

// scores, filtered [n_q][G]; labels [templates of the resident shard]; masks [n_q][3]; d_global NULL (full search: the template of position p is p) or [G] global indices
// with 0 <= d_global[p] - index_base < the labels' length.  kVec: G % 4 == 0 and both matrices 16-byte aligned
template <bool kVec>
__global__ __launch_bounds__(kHfThreads) void k_filter_rows(const uint32_t* __restrict__ scores, int n_q, int G, const u64* __restrict__ labels, const u64* __restrict__ masks,
                                                            const long long* __restrict__ d_global, long long index_base, uint32_t* __restrict__ filtered)
{
    constexpr int kCols = kVec ? 4 : 1;
    const size_t col = ((size_t)blockIdx.x * kHfThreads + threadIdx.x) * kCols;
    if (col >= (size_t)G) return;                                           // (kVec: G % 4 == 0, so col + 3 < G too)
    u64 L[kCols];
#pragma unroll
    for (int j = 0; j < kCols; ++j) L[j] = labels[d_global ? (size_t)(d_global[col + j] - index_base) : col + j];
    using W = typename std::conditional<kVec, uint4, uint32_t>::type;
    const auto filter = [&](W v, int q) -> W {                              // q is uniform over the workgroup: the masks are scalar loads
        const u64 any_of = masks[(size_t)q * 3], all_of = masks[(size_t)q * 3 + 1], none_of = masks[(size_t)q * 3 + 2];
        if constexpr (kVec) return make_uint4(hf_cell(v.x, L[0], any_of, all_of, none_of), hf_cell(v.y, L[1], any_of, all_of, none_of),
                                              hf_cell(v.z, L[2], any_of, all_of, none_of), hf_cell(v.w, L[3], any_of, all_of, none_of));
        else return hf_cell(v, L[0], any_of, all_of, none_of);
    };
    const int strips = (n_q + kHfRows - 1) / kHfRows;
    for (int st = (int)blockIdx.y; st < strips; st += (int)gridDim.y) {
        const int q0 = st * kHfRows, rows = n_q - q0 < kHfRows ? n_q - q0 : kHfRows;
        const size_t at = (size_t)q0 * (size_t)G + col;
        if (rows == kHfRows) {                                              // a whole strip: its kHfRows loads are in flight together
            W v[kHfRows];
#pragma unroll
            for (int r = 0; r < kHfRows; ++r) v[r] = *reinterpret_cast<const W*>(scores + at + (size_t)r * (size_t)G);
#pragma unroll
            for (int r = 0; r < kHfRows; ++r) *reinterpret_cast<W*>(filtered + at + (size_t)r * (size_t)G) = filter(v[r], q0 + r);
        } else
            for (int r = 0; r < rows; ++r) *reinterpret_cast<W*>(filtered + at + (size_t)r * (size_t)G) = filter(*reinterpret_cast<const W*>(scores + at + (size_t)r * (size_t)G), q0 + r);
    }
}

// pairs [n_pairs] (row, column) with row < n_rows, column < stride; buf [n_rows][stride] words of type W
template <class W>
__global__ __launch_bounds__(kHfThreads) void k_filter_drop(const int2* __restrict__ pairs, size_t n_pairs, W* __restrict__ buf, int n_rows, int stride, W word)
{
    for (size_t i = (size_t)blockIdx.x * kHfThreads + threadIdx.x; i < n_pairs; i += (size_t)gridDim.x * kHfThreads) {
        const int2 p = pairs[i];
        if (p.x >= 0 && p.x < n_rows && p.y >= 0 && p.y < stride) buf[(size_t)p.x * (size_t)stride + (size_t)p.y] = word;   // (the host resolved the pairs inside; this keeps the store there)
    }
}

hipError_t launch_filter_rows(const float* scores, int n_q, int G, const unsigned long long* labels, const unsigned long long* masks, const long long* d_global, long long index_base,
                              float* filtered, hipStream_t stream)
{
    if (n_q <= 0 || G <= 0) return hipSuccess;
    if (!scores || !labels || !masks || !filtered || scores == filtered) return hipErrorInvalidValue;
    const bool vec = rows_take_16_bytes(G, scores, filtered);
    const size_t threads = vec ? (size_t)G / 4 : (size_t)G;
    const dim3 grid((unsigned)((threads + kHfThreads - 1) / kHfThreads), grid_clamp((size_t)((n_q + kHfRows - 1) / kHfRows)));
    if (vec) hipLaunchKernelGGL(k_filter_rows<true>, grid, dim3(kHfThreads), 0, stream, (const uint32_t*)scores, n_q, G, labels, masks, d_global, index_base, (uint32_t*)filtered);
    else hipLaunchKernelGGL(k_filter_rows<false>, grid, dim3(kHfThreads), 0, stream, (const uint32_t*)scores, n_q, G, labels, masks, d_global, index_base, (uint32_t*)filtered);
    return hipGetLastError();
}

static inline unsigned hf_drop_blocks(size_t n_pairs) { return grid_clamp((n_pairs + kHfThreads - 1) / kHfThreads); }   // (a grid-stride loop walks the rest)

hipError_t launch_filter_drop_cells(const int32_t* pairs, size_t n_pairs, float* filtered, int n_q, int G, hipStream_t stream)
{
    if (n_pairs == 0) return hipSuccess;
    if (!pairs || !filtered || n_q <= 0 || G <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_filter_drop<uint32_t>, dim3(hf_drop_blocks(n_pairs)), dim3(kHfThreads), 0, stream, (const int2*)pairs, n_pairs, (uint32_t*)filtered, n_q, G, kNoEntryWord);
    return hipGetLastError();
}

hipError_t launch_filter_drop_subjects(const int32_t* pairs, size_t n_pairs, unsigned long long* best, int n_q, int S, hipStream_t stream)
{
    if (n_pairs == 0) return hipSuccess;
    if (!pairs || !best || n_q <= 0 || S <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_filter_drop<u64>, dim3(hf_drop_blocks(n_pairs)), dim3(kHfThreads), 0, stream, (const int2*)pairs, n_pairs, best, n_q, S, (u64)0);
    return hipGetLastError();
}

}  // namespace afis
