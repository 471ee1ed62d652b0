// print_cascade.hip — device code of the print cascade (afis_print_cascade.cpp: afis_search_prints_cascade): resident prints as queries, the minutiae scorer for every
// (query print, column print) cell, the texture scorer for the `keep` best columns of every query only.  Three small kernels around kernels that exist.  The queries of
// the call and the rows of parts differ: a query with something active is one PSEUDO-QUERY (afis_prints.cpp), a query with nothing active is none, so every kernel
// reaches a query's row of parts through q_row [n_q] (-1 = no pseudo-query) and its weights through q_w [n_q] (w_minu, w_tex; the host has written a zero where the
// term is not active).
//   k_print_cascade_stage1   m(q, t), the first stage's value of a cell: fold_print_cell (print_fold.h: the one expression of a print cell here) of slot 0 of the
//                            pseudo-query's parts with the texture term left out; -1.0f for an empty or removed column, and for the whole row of a query whose
//                            minutiae term is not active -> the matrix k_rank_hits (rank_hits.hip) then selects the kept columns from.  One thread per (query,
//                            column), every word written once
//   k_print_cascade_gather   one thread per kept pair of a query whose texture term is active: the pair's (pseudo-query of its launch group, shard-local template)
//                            into the pair tables of cascade_tables.h — what k_adc_pairs and k_graph_texture's pair form read.  cascade.hip's gather names the
//                            query of the group; here it is the pseudo-query's row minus the group's first row
//   k_print_cascade_finish   one thread per kept (query, rank): v_m from the stage-1 parts at (q, t), v_t from the texture pair kernel's output at the pair's slot,
//                            folded by fold_print_cell -> the word into the combined matrix at (q, t), the two parts into the kept-parts block [n_q][keep][2].  The
//                            host has filled the matrix with the "no entry" word (score_order.h) and the block with zeros before: a word is written at most twice
// A thread of the last two is a (query, rank) of the kept lists [n_q][keep] k_rank_hits left; a query's pairs stand at consecutive slots, so every access by slot — the
// tables, the pairs' parts, the kept-parts block, the lists themselves — is coalesced; only the (q, t) accesses to parts [n_pseudo][G][4] and to the matrix gather and
// scatter, through L2.  A list entry that names no template of the shard (the -1 padding: only a row of NaN keys below -inf's has fewer than n_kept entries) is routed
// to template 0 in the tables — the pair kernels stay inside the shard — and finished nowhere.  No LDS, and no word is touched by two threads of a launch.
#include "afis_device.h"
#include "print_fold.h"

namespace afis {

constexpr int kPrintCascadeThreads = 256;

// parts [n_pseudo][G] float4; q_row, q_w [n_q]; empty [G]; m [n_q][G].  Grid = (column chunks, queries): the query's row and weight depend on the block index and the
// loop counter only (scalar loads); a grid's second dimension holds 65 535 blocks, more queries than that are walked in a loop.  Every index is a size_t.
__global__ __launch_bounds__(kPrintCascadeThreads) void k_print_cascade_stage1(const float4* __restrict__ parts, const int32_t* __restrict__ q_row, const float2* __restrict__ q_w,
                                                                              const uint8_t* __restrict__ empty, int n_q, int G, float* __restrict__ m)
{
    const size_t g = (size_t)blockIdx.x * kPrintCascadeThreads + threadIdx.x;
    if (g >= (size_t)G) return;
    const bool col_empty = empty[g] != 0;
    for (int q = (int)blockIdx.y; q < n_q; q += (int)gridDim.y) {
        const int row = q_row[q];
        const float w_m = q_w[q].x;
        float r = -1.0f;
        if (row >= 0 && w_m != 0.0f && !col_empty) r = fold_print_cell(w_m, parts[(size_t)row * (size_t)G + g].x, 0.0f, 0.0f);
        m[(size_t)q * (size_t)G + g] = r;
    }
}

// kept [n_q][keep] global indices in rank order; q_slot [n_q + 1], piece_first [n_pieces + 1] (cascade_tables.h); piece_p0 [n_pieces] the first pseudo-query of the
// piece's launch group; tab (2 total + n_pieces ints)
__global__ __launch_bounds__(kPrintCascadeThreads) void k_print_cascade_gather(int n_q, int G, int keep, int n_kept, long long index_base, const long long* __restrict__ kept,
                                                                              const int32_t* __restrict__ q_slot, const int32_t* __restrict__ piece_first, int n_pieces,
                                                                              const int32_t* __restrict__ piece_p0, const int32_t* __restrict__ q_row, int32_t* __restrict__ tab)
{
    const long long u = (long long)blockIdx.x * kPrintCascadeThreads + threadIdx.x;
    if (u >= (long long)n_q * n_kept) return;
    const int qi = (int)(u / n_kept), r = (int)(u - (long long)qi * n_kept);
    const int s0 = q_slot[qi];
    if (q_slot[qi + 1] - s0 != n_kept) return;                                // a query without an active texture term has no pairs
    const int s = s0 + r;
    int lo = 0, hi = n_pieces;                                                // the piece that holds slot s: piece_first[lo] <= s < piece_first[lo + 1]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (piece_first[mid] <= s) lo = mid; else hi = mid; }
    const int p_first = piece_first[lo];
    const long long t = kept[(size_t)qi * keep + r] - index_base;
    const int gi = t >= 0 && t < G ? (int)t : 0;
    int32_t* const row = tab + 2 * (size_t)s + lo;
    if (s == p_first) row[0] = piece_first[lo + 1] - p_first;
    row[1] = q_row[qi] - piece_p0[lo];
    row[2] = gi;
}

// parts [n_pseudo][G] float4 (stage 1's); pair_parts [total] float4 (slot 3: the texture pair kernel's); out [n_q][G]; kept_parts [n_q][keep] float2
__global__ __launch_bounds__(kPrintCascadeThreads) void k_print_cascade_finish(int n_q, int G, int keep, int n_kept, long long index_base, const long long* __restrict__ kept,
                                                                              const int32_t* __restrict__ q_slot, const int32_t* __restrict__ q_row, const float2* __restrict__ q_w,
                                                                              const uint8_t* __restrict__ empty, const float4* __restrict__ parts,
                                                                              const float4* __restrict__ pair_parts, float* __restrict__ out, float2* __restrict__ kept_parts)
{
    const long long u = (long long)blockIdx.x * kPrintCascadeThreads + threadIdx.x;
    if (u >= (long long)n_q * n_kept) return;
    const int qi = (int)(u / n_kept), r = (int)(u - (long long)qi * n_kept);
    const long long t = kept[(size_t)qi * keep + r] - index_base;
    if (t < 0 || t >= G) return;
    const float2 w = q_w[qi];
    const int row = q_row[qi], s0 = q_slot[qi];
    const bool am = row >= 0 && w.x != 0.0f, at = row >= 0 && w.y != 0.0f && q_slot[qi + 1] - s0 == n_kept;
    const bool scored = (am || at) && empty[t] == 0;                         // otherwise the cell is the -1: an empty or removed column, nothing active
    const float v_m = scored && am ? parts[(size_t)row * (size_t)G + (size_t)t].x : 0.0f;
    const float v_t = scored && at ? pair_parts[s0 + r].w : 0.0f;
    out[(size_t)qi * (size_t)G + (size_t)t] = scored ? fold_print_cell(am ? w.x : 0.0f, v_m, at ? w.y : 0.0f, v_t) : -1.0f;
    kept_parts[(size_t)qi * keep + r] = make_float2(v_m, v_t);
}

hipError_t launch_print_cascade_stage1(const float* parts, const int32_t* q_row, const float* q_w, const uint8_t* empty, int n_q, int G, float* m, hipStream_t stream)
{
    if (n_q <= 0 || G <= 0) return hipSuccess;
    if (!parts || !q_row || !q_w || !empty || !m || ((uintptr_t)parts & 15) || ((uintptr_t)q_w & 7)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((size_t)G + kPrintCascadeThreads - 1) / kPrintCascadeThreads), grid_clamp((size_t)n_q));
    hipLaunchKernelGGL(k_print_cascade_stage1, grid, dim3(kPrintCascadeThreads), 0, stream, (const float4*)parts, q_row, (const float2*)q_w, empty, n_q, G, m);
    return hipGetLastError();
}

hipError_t launch_print_cascade_gather(int n_q, int G, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot, const int32_t* piece_first,
                                       int n_pieces, const int32_t* piece_p0, const int32_t* q_row, int32_t* tab, hipStream_t stream)
{
    const long long n = (long long)n_q * n_kept;
    if (n <= 0 || n_pieces <= 0) return hipSuccess;
    if (G <= 0 || n_kept > keep || n_kept > G || n > 0x7fffffffLL || !kept || !q_slot || !piece_first || !piece_p0 || !q_row || !tab) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_print_cascade_gather, dim3((unsigned)((n + kPrintCascadeThreads - 1) / kPrintCascadeThreads)), dim3(kPrintCascadeThreads), 0, stream, n_q, G, keep, n_kept,
                       index_base, kept, q_slot, piece_first, n_pieces, piece_p0, q_row, tab);
    return hipGetLastError();
}

hipError_t launch_print_cascade_finish(int n_q, int G, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot, const int32_t* q_row,
                                       const float* q_w, const uint8_t* empty, const float* parts, const float* pair_parts, float* out, float* kept_parts, hipStream_t stream)
{
    const long long n = (long long)n_q * n_kept;
    if (n <= 0) return hipSuccess;
    if (G <= 0 || n_kept > keep || n_kept > G || n > 0x7fffffffLL || !kept || !q_slot || !q_row || !q_w || !empty || !parts || !pair_parts || !out || !kept_parts ||
        (((uintptr_t)parts | (uintptr_t)pair_parts) & 15) || (((uintptr_t)q_w | (uintptr_t)kept_parts) & 7))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_print_cascade_finish, dim3((unsigned)((n + kPrintCascadeThreads - 1) / kPrintCascadeThreads)), dim3(kPrintCascadeThreads), 0, stream, n_q, G, keep, n_kept,
                       index_base, kept, q_slot, q_row, (const float2*)q_w, empty, (const float4*)parts, (const float4*)pair_parts, out, (float2*)kept_parts);
    return hipGetLastError();
}

}  // namespace afis
