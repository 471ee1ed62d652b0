// cascade_mapped.hip — the two ends of a cascade's second stage (cascade.hip: k_cascade_gather, k_cascade_scatter) for a cascade that ran over a SUB-SHARD of the resident
// shard (afis_cascade_eligible.cpp: afis_search_cascade_subset, afis_search_cascade_eligible).  There a kept global index is no column of what was searched, and the kept
// cell's place in the matrix the call leaves is not (q, t) of the sub-shard:
//   k_cascade_gather_mapped   one thread per kept pair (query, rank): the kept global index -> the template's position in the sub-shard through inv [G_res] (resident
//                             position -> sub-shard position, -1: not listed; NULL: the sub-shard is the resident shard) -> the pair's row of the pair tables
//                             (cascade_tables.h) and its three minutiae parts, from the call's parts [n_q][m][4] over the sub-shard's m templates, with a texture part of
//                             +0.0f, into the pair's parts block
//   k_cascade_scatter_mapped  one thread per kept cell: the pair's fused score, or the -1 of a latent-empty query, to out[row_of[q] * out_stride + out_col[t]] — the
//                             query's row and the template's column in the combined matrix, which the host filled with the "no entry" word before
// A thread and its coalesced accesses by slot — the lists, the tables, the parts blocks, the pair scores — are the resident pair's; only the (q, t) accesses gather
// (inv, parts) and scatter (out), through L2.  A list entry that names nothing — the -1 padding, a position outside the resident shard, a template inv does not list — is
// routed to template 0 of the sub-shard in the tables and scattered nowhere.  No LDS, no barrier: a thread that returns early leaves nobody waiting.
#include "afis_device.h"

namespace afis {

__device__ __forceinline__ int mapped_template(long long kept_global, long long index_base, int G_res, int m, const int32_t* __restrict__ inv)
{
    const long long t = kept_global - index_base;
    if (t < 0 || t >= G_res) return -1;
    const int gi = inv ? inv[t] : (int)t;
    return gi >= 0 && gi < m ? gi : -1;
}

__global__ __launch_bounds__(256) void k_cascade_gather_mapped(int n_q, int G_res, int m, int keep, int n_kept, long long index_base, const long long* __restrict__ kept,
                                                               const int32_t* __restrict__ q_slot, const int32_t* __restrict__ piece_first, int n_pieces,
                                                               const int32_t* __restrict__ piece_q0, const int32_t* __restrict__ inv, const float4* __restrict__ parts,
                                                               int32_t* __restrict__ tab, float4* __restrict__ pair_parts)
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
    const int mt = mapped_template(kept[(size_t)qi * keep + r], index_base, G_res, m, inv);
    const bool named = mt >= 0;
    const int gi = named ? mt : 0;
    int32_t* const row = tab + 2 * (size_t)s + lo;
    if (s == p_first) row[0] = piece_first[lo + 1] - p_first;
    row[1] = qi - piece_q0[lo];
    row[2] = gi;
    float4 p = parts[(size_t)qi * m + gi];
    p.w = 0.0f;
    pair_parts[s] = named ? p : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// pair_score [total]; out [out_rows][out_stride]: the kept cell (q, sub-shard template gi) is written at (row_of[q], out_col[gi]) — NULL tables: q and gi themselves —;
// a target outside the matrix is not written
__global__ __launch_bounds__(256) void k_cascade_scatter_mapped(int n_q, int G_res, int m, int keep, int n_kept, long long index_base, const long long* __restrict__ kept,
                                                                const int32_t* __restrict__ q_slot, const float* __restrict__ pair_score, const int32_t* __restrict__ inv,
                                                                const int32_t* __restrict__ row_of, const int32_t* __restrict__ out_col, long long out_rows,
                                                                long long out_stride, float* __restrict__ out)
{
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= (long long)n_q * n_kept) return;
    const int qi = (int)(u / n_kept), r = (int)(u - (long long)qi * n_kept);
    const int gi = mapped_template(kept[(size_t)qi * keep + r], index_base, G_res, m, inv);
    if (gi < 0) return;
    const long long row = row_of ? row_of[qi] : qi, col = out_col ? out_col[gi] : gi;
    if (row < 0 || row >= out_rows || col < 0 || col >= out_stride) return;
    const int s0 = q_slot[qi];
    out[(size_t)row * (size_t)out_stride + (size_t)col] = q_slot[qi + 1] - s0 == n_kept ? pair_score[s0 + r] : -1.0f;
}

hipError_t launch_cascade_gather_mapped(int n_q, int G_res, int m, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot,
                                        const int32_t* piece_first, int n_pieces, const int32_t* piece_q0, const int32_t* inv, const float* parts, int32_t* tab,
                                        float* pair_parts, hipStream_t stream)
{
    const long long n = (long long)n_q * n_kept;
    if (n <= 0 || n_pieces <= 0) return hipSuccess;
    if (G_res <= 0 || m <= 0 || (!inv && m != G_res) || n_kept > keep || n_kept > m || n > 0x7fffffffLL || !kept || !q_slot || !piece_first || !piece_q0 || !parts || !tab || !pair_parts)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cascade_gather_mapped, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n_q, G_res, m, keep, n_kept, index_base, kept, q_slot, piece_first, n_pieces,
                       piece_q0, inv, (const float4*)parts, tab, (float4*)pair_parts);
    return hipGetLastError();
}

hipError_t launch_cascade_scatter_mapped(int n_q, int G_res, int m, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot,
                                         const float* pair_score, const int32_t* inv, const int32_t* row_of, const int32_t* out_col, long long out_rows, long long out_stride,
                                         float* out, hipStream_t stream)
{
    const long long n = (long long)n_q * n_kept;
    if (n <= 0) return hipSuccess;
    if (G_res <= 0 || m <= 0 || (!inv && m != G_res) || n_kept > keep || n_kept > m || n > 0x7fffffffLL || out_rows <= 0 || out_stride <= 0 || !kept || !q_slot || !pair_score || !out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cascade_scatter_mapped, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n_q, G_res, m, keep, n_kept, index_base, kept, q_slot, pair_score, inv,
                       row_of, out_col, out_rows, out_stride, out);
    return hipGetLastError();
}

}  // namespace afis
