// template_fold.hip — device code of the weighted search (afis_weighted.cpp: afis_search_weighted): one BATCH of queries was scored as pseudo-queries — the active minutiae
// templates of a query three to a pseudo-query, its active texture templates one to a pseudo-query — and the per-part scores parts [pseudo][G][4] are folded into the
// batch's rows of the combined matrix out [queries of the batch][G]:
//   out[q][g] = -1                                   where query q has no active template (qd[q].w != 0) or rolled entry g is empty
//             = (float)acc                           otherwise: double acc = +0.0; for j < n_pq, slot 0..2 with weight w != 0: acc = acc + (double)w * (double)part;
//                                                    then for j < n_at with slot 3's weight w != 0: the same — the order include/afis_matcher.h states
// The product of two fp32 values is exact in fp64 (48 significand bits, exponents within +-254): the sum does not depend on whether the multiply-add is contracted, and
// a product may be formed before the sum has reached it.
//
// Grid = (column chunks, queries of the batch); one thread per column.  The thread walks the query's pseudo-queries: every step loads the cell's 16 bytes (float4: 1 KB
// per wave, contiguous), adds the three minutiae terms and KEEPS the texture product of the first kFoldTexKept pseudo-queries in registers; after the walk those
// products are added in order.  A query with more texture templates than that (none of the known extractors: the reference's has one) takes a second walk over the
// rest, 4 bytes per cell, from lines the first walk left in L2.  All four products of a step are formed whether used or not — that keeps the load one 16-byte word —
// and a slot of weight 0 is left out of the sum by a select, whatever its part holds.  The query's descriptor and the weight rows depend on the block index and the
// loop counter only: they are read through const __restrict__ tables as scalar loads.  One (float) conversion, one coalesced 4-byte store; every word of the batch's
// rows is written exactly once: no memset before the launch, no atomics, no LDS.  Every index into parts and out is a size_t: pseudo-queries x G x 4 may pass 2^31.
// A grid's second dimension holds 65 535 blocks; more queries than that are walked in a loop.
// Below it k_fold_print_pairs: the same fold for the pair slots of afis_score_print_pairs, one view of (minutiae, texture) per slot.
#include "afis_device.h"

namespace afis {

constexpr int kFoldThreads = 256;
constexpr int kFoldTexKept = 4;                                             // texture products kept in registers during the walk

// parts [n_pseudo][G] float4; qd [nq] (first pseudo-query, n_pq, n_at, status) with first + n_pq <= n_pseudo and n_at <= n_pq (the host checks); w [n_pseudo] float4 aligned
// to the part slots, 0 = unused; empty [G]; out [nq][G]
__global__ __launch_bounds__(kFoldThreads) void k_fold_templates(const float4* __restrict__ parts, const int4* __restrict__ qd, const float4* __restrict__ w,
                                                                 const uint8_t* __restrict__ empty, int nq, int G, float* __restrict__ out)
{
    const size_t g = (size_t)blockIdx.x * kFoldThreads + threadIdx.x;
    if (g >= (size_t)G) return;
    const bool col_empty = empty[g] != 0;
    for (int q = (int)blockIdx.y; q < nq; q += (int)gridDim.y) {
        const int4 d = qd[q];                                               // uniform over the workgroup: a scalar load
        float r = -1.0f;
        if (d.w == 0 && !col_empty) {
            double acc = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
            static_assert(kFoldTexKept == 4, "t0 .. t3");
            const float4* __restrict__ p = parts + (size_t)d.x * (size_t)G + g;
            for (int j = 0; j < d.y; ++j) {
                const float4 ww = w[d.x + j];
                const float4 v = p[(size_t)j * (size_t)G];
                const double px = (double)ww.x * (double)v.x, py = (double)ww.y * (double)v.y, pz = (double)ww.z * (double)v.z, pw = (double)ww.w * (double)v.w;
                acc = ww.x != 0.0f ? acc + px : acc;
                acc = ww.y != 0.0f ? acc + py : acc;
                acc = ww.z != 0.0f ? acc + pz : acc;
                t0 = j == 0 ? pw : t0; t1 = j == 1 ? pw : t1; t2 = j == 2 ? pw : t2; t3 = j == 3 ? pw : t3;
            }
            if (d.z > 0 && w[d.x].w != 0.0f) acc = acc + t0;
            if (d.z > 1 && w[d.x + 1].w != 0.0f) acc = acc + t1;
            if (d.z > 2 && w[d.x + 2].w != 0.0f) acc = acc + t2;
            if (d.z > 3 && w[d.x + 3].w != 0.0f) acc = acc + t3;
            for (int j = kFoldTexKept; j < d.z; ++j) {
                const float ww = w[d.x + j].w;
                if (ww != 0.0f) acc = acc + (double)ww * (double)p[(size_t)j * (size_t)G].w;
            }
            r = (float)acc;
        }
        out[(size_t)q * (size_t)G + g] = r;
    }
}

hipError_t launch_fold_templates(const float* parts, const int32_t* qd, const float* w, const uint8_t* empty, int nq, int G, float* out, hipStream_t stream)
{
    if (nq <= 0 || G <= 0) return hipSuccess;
    if (!qd || !w || !empty || !out || !parts) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((size_t)G + kFoldThreads - 1) / kFoldThreads), grid_clamp((size_t)nq));
    hipLaunchKernelGGL(k_fold_templates, grid, dim3(kFoldThreads), 0, stream, (const float4*)parts, (const int4*)qd, (const float4*)w, empty, nq, G, out);
    return hipGetLastError();
}

// The fold of a PRINT PAIR (afis_print_pairs.cpp: afis_score_print_pairs): the pair calls keep one float4 of parts per pair slot, and a print's view has its minutiae
// template in slot 0 and its texture template in slot 3.  With the slot's two weights (w_minu, w_tex) — the host has written a zero where the query print does not hold
// the template, so "active" is w != 0.0f — the score is k_fold_templates' for one pseudo-query of that view:
//   score[p] = -1                                    where nothing is active
//            = (float)acc                            otherwise: double acc = +0.0; minutiae active: acc = acc + (double)w_minu * (double)parts[p].x; then texture active:
//                                                    acc = acc + (double)w_tex * (double)parts[p].w
// and +0.0f is stored over an inactive part, so that the copy back is final.  Both products are formed whether used or not and left out by a select, as above.
// One thread per pair slot, a 16-byte and an 8-byte load, a 16-byte and a 4-byte store; per-thread data only: nothing here is uniform, so nothing goes through the scalar
// path.  No LDS, and no word is touched by two threads; every index is a size_t; a one-dimensional grid of at most 65 535 workgroups strides over longer lists.
__global__ __launch_bounds__(kFoldThreads) void k_fold_print_pairs(float4* parts, const float2* __restrict__ w, size_t n, float* __restrict__ score)
{
    const size_t stride = (size_t)gridDim.x * kFoldThreads;
    for (size_t p = (size_t)blockIdx.x * kFoldThreads + threadIdx.x; p < n; p += stride) {
        const float4 v = parts[p];
        const float2 ww = w[p];
        const bool am = ww.x != 0.0f, at = ww.y != 0.0f;
        const double pm = (double)ww.x * (double)v.x, pt = (double)ww.y * (double)v.w;
        double acc = 0.0;
        acc = am ? acc + pm : acc;
        acc = at ? acc + pt : acc;
        score[p] = am || at ? (float)acc : -1.0f;
        parts[p] = make_float4(am ? v.x : 0.0f, v.y, v.z, at ? v.w : 0.0f);
    }
}

hipError_t launch_fold_print_pairs(float* parts, const float* w, size_t n_pairs, float* score, hipStream_t stream)
{
    if (n_pairs == 0) return hipSuccess;
    if (!parts || !w || !score || ((uintptr_t)parts & 15) || ((uintptr_t)w & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fold_print_pairs, dim3(grid_clamp((n_pairs + kFoldThreads - 1) / kFoldThreads)), dim3(kFoldThreads), 0, stream, (float4*)parts, (const float2*)w, n_pairs, score);
    return hipGetLastError();
}

}  // namespace afis
