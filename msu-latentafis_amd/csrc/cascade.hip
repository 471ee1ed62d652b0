// cascade.hip — device code of the cascade search (afis_cascade.cpp: afis_search_cascade): the three minutiae scorers for every (latent, print) cell, the texture scorer
// for the `keep` best prints of every latent only.  Three small kernels around kernels that exist: the first stage's fusion, and the two ends of the second stage.
//   k_fuse_stage1      m(q, t), the first stage's value of a cell: fuse_cell (fuse_cell.h: the search's own expression) with the texture score taken as +0.0f, from the
//                      cell's three minutiae parts -> the matrix k_rank_hits (rank_hits.hip) then selects the kept prints from
//   k_cascade_gather   one thread per kept pair: the pair's (query of its launch group, shard-local template) into the pair tables of cascade_tables.h — what the pair
//                      kernels of afis_score_pairs read (adc_pairs.hip, graph_pairs.hip, minu.hip::k_fuse_pairs) — and its three minutiae parts, with a texture part of
//                      +0.0f, into the pair's parts block
//   k_cascade_scatter  one thread per kept cell: the pair's fused score, or the -1 of a latent-empty query, into the combined matrix at (q, t); the host has filled the
//                      matrix with the "no entry" word (score_order.h) before, so a word is written at most twice
// A thread is a (query, rank) of the kept lists [n_q][keep] k_rank_hits left; a query's pairs stand at consecutive slots, so every access by slot — the tables, the
// parts blocks, the pair scores, the lists themselves — is coalesced; only the (q, t) accesses to parts [n_q][G][4] and to the matrix gather and scatter, through L2.
// A list entry that names no template of the shard (the -1 padding: only a row of NaN keys below -inf's has fewer than n_kept entries) is routed to template 0 in the
// tables — the pair kernels stay inside the shard — and scattered nowhere.
#include "afis_device.h"
#include "fuse_cell.h"

namespace afis {

__global__ __launch_bounds__(256) void k_fuse_stage1(QueryDev q, GalleryDev g, const float* __restrict__ parts, float* __restrict__ scores)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)q.nq * g.G;
    if (idx >= n) return;
    const int qi = (int)(idx / g.G), gi = (int)(idx - (long long)qi * g.G);
    scores[idx] = fuse_cell(q, g, qi, gi, parts + (size_t)idx * 4, 0.0f);
}

// kept [n_q][keep] global indices in rank order; q_slot [n_q + 1], piece_first [n_pieces + 1], piece_q0 [n_pieces] (cascade_tables.h); parts [n_q][G] float4;
// tab (2 total + n_pieces ints), pair_parts [total] float4
__global__ __launch_bounds__(256) void k_cascade_gather(int n_q, int G, int keep, int n_kept, long long index_base, const long long* __restrict__ kept,
                                                        const int32_t* __restrict__ q_slot, const int32_t* __restrict__ piece_first, int n_pieces,
                                                        const int32_t* __restrict__ piece_q0, const float4* __restrict__ parts, int32_t* __restrict__ tab,
                                                        float4* __restrict__ pair_parts)
{
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= (long long)n_q * n_kept) return;
    const int qi = (int)(u / n_kept), r = (int)(u - (long long)qi * n_kept);
    const int s0 = q_slot[qi];
    if (q_slot[qi + 1] - s0 != n_kept) return;                                // a latent-empty query has no pairs
    const int s = s0 + r;
    int lo = 0, hi = n_pieces;                                                // the piece that holds slot s: piece_first[lo] <= s < piece_first[lo + 1]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (piece_first[mid] <= s) lo = mid; else hi = mid; }
    const int p_first = piece_first[lo];
    const long long t = kept[(size_t)qi * keep + r] - index_base;
    const bool named = t >= 0 && t < G;
    const int gi = named ? (int)t : 0;
    int32_t* const row = tab + 2 * (size_t)s + lo;
    if (s == p_first) row[0] = piece_first[lo + 1] - p_first;
    row[1] = qi - piece_q0[lo];
    row[2] = gi;
    float4 p = parts[(size_t)qi * G + gi];
    p.w = 0.0f;
    pair_parts[s] = named ? p : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// pair_score [total]; out [n_q][G]
__global__ __launch_bounds__(256) void k_cascade_scatter(int n_q, int G, int keep, int n_kept, long long index_base, const long long* __restrict__ kept,
                                                         const int32_t* __restrict__ q_slot, const float* __restrict__ pair_score, float* __restrict__ out)
{
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= (long long)n_q * n_kept) return;
    const int qi = (int)(u / n_kept), r = (int)(u - (long long)qi * n_kept);
    const long long t = kept[(size_t)qi * keep + r] - index_base;
    if (t < 0 || t >= G) return;
    const int s0 = q_slot[qi];
    out[(size_t)qi * G + (size_t)t] = q_slot[qi + 1] - s0 == n_kept ? pair_score[s0 + r] : -1.0f;
}

hipError_t launch_fuse_stage1(const QueryDev& q, const GalleryDev& g, const float* parts, float* scores, hipStream_t stream)
{
    const long long n = (long long)q.nq * g.G;
    if (n <= 0) return hipSuccess;
    if (!parts || !scores) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fuse_stage1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, q, g, parts, scores);
    return hipGetLastError();
}

hipError_t launch_cascade_gather(int n_q, int G, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot, const int32_t* piece_first,
                                 int n_pieces, const int32_t* piece_q0, const float* parts, int32_t* tab, float* pair_parts, hipStream_t stream)
{
    const long long n = (long long)n_q * n_kept;
    if (n <= 0 || n_pieces <= 0) return hipSuccess;
    if (G <= 0 || n_kept > keep || n_kept > G || n > 0x7fffffffLL || !kept || !q_slot || !piece_first || !piece_q0 || !parts || !tab || !pair_parts) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cascade_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n_q, G, keep, n_kept, index_base, kept, q_slot, piece_first, n_pieces, piece_q0,
                       (const float4*)parts, tab, (float4*)pair_parts);
    return hipGetLastError();
}

hipError_t launch_cascade_scatter(int n_q, int G, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot, const float* pair_score,
                                  float* out, hipStream_t stream)
{
    const long long n = (long long)n_q * n_kept;
    if (n <= 0) return hipSuccess;
    if (G <= 0 || n_kept > keep || n_kept > G || n > 0x7fffffffLL || !kept || !q_slot || !pair_score || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cascade_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n_q, G, keep, n_kept, index_base, kept, q_slot, pair_score, out);
    return hipGetLastError();
}

}  // namespace afis
