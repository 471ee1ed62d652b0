// rank_position.hip — device code of the rank positions (afis_positions.cpp: afis_rank_positions, afis_rank_subject_positions, afis_count_before): where a NAMED template
// or person stands in the list k_rank_hits (rank_hits.hip) would make of a row, without making the list.  The position of a target is the number of the row's entries
// that stand before it, and "before" is a comparison of two 64-bit composites (score_order.h) — the ordered word in the high half, ~position in the low one — so the
// whole order, tie rule included, is one unsigned comparison:
//   templates  entry e of a row of [G] floats: rank_composite(rank_key(score), e), k_topk's word and tie rule (ascending position = ascending global index)
//   subjects   slot e of best[query][0 .. S) as k_subject_best (subject_rank.hip) left it: composite_at(b, e), the raw ordered word, ties by ascending slot = ascending
//              subject id; a slot that is 0 is no entry
// A cell, or a slot, is an ENTRY when its word is >= kPosFloor, the ordered word of -inf: what k_rank_hits counts at min_score = -inf.  kNoEntryWord (a filter's or an
// exclusion's mark) and every other NaN with the sign set lie below it.
//
// Two passes.
//   k_position_targets  one thread per target (row, position): reads the target's cell — or its slot of best — and writes its composite, its status, its score's own bits
//              and, for a person, the global index of the best template; zeroes the target's counter.  A target that is no entry gets the composite ~0, which no entry
//              exceeds.  Its third form serves afis_count_before, whose composites (hypothetical score, tie position) come from the host: where the hypothetical entry's
//              index is a column of the row, that column must never count, so the counter starts at -1 when the column's own composite exceeds the target's.
//   k_count_before  the hot pass.  Grid = (column chunks, rows that have targets, workgroups that share a row's targets); the targets arrive sorted into a CSR by row.  A thread loads kCbLoads x kCols
//              entries of its row ONCE — all loads issued before the first use; kCols = 4 adjacent columns as one 16-byte word where rows_take_16_bytes, else 1 — and
//              forms their composites once, in registers (no entry: 0, which exceeds no target).  The row's targets pass through LDS in chunks of kCbTargets; the
//              entries stay in registers across the chunks, so a workgroup reads its part of the row once whatever number of targets it has.  A row with many
//              targets — a suspect list against one latent — would leave all its comparisons to G / 4096 workgroups: the grid's third dimension deals the row's
//              target chunks to up to kCbDepth workgroups per column chunk (each re-reads the part of the row, 16 KB, from the cache).  Per target (its composite read from
//              LDS at one address by every lane: a broadcast) and register entry, one 64-bit compare whose ballot is popcounted: a wave's partial is a scalar
//              sum of popcounts.  The waves' partials meet in LDS, and one thread per target adds the workgroup's sum — when it is not 0 — to the target's counter:
//              one integer add per (workgroup, target).  Integer adds commute, so the counters are the same bits on every run; there are no float atomics.
// Every barrier sits in a loop whose bounds are read from the CSR by block index: the same trip count in every thread.  Matrix indices are size_t; a workgroup counts at
// most kCbThreads x kCbLoads x 4 entries in 32 bits and the counters are 64-bit.  More than 65 535 rows with targets are walked in a loop over gridDim.y.
#include "afis_device.h"

namespace afis {

constexpr int kCbThreads = 256;
constexpr int kCbWaves = kCbThreads / 64;
constexpr int kCbLoads = kPosLoads;                                         // loads in flight per thread (afis_device.h: the chunk sizes are the host's and the tests' too)
constexpr int kCbTargets = kPosTargetChunk;                                 // targets staged in LDS at a time
constexpr int kCbDepth = 32;                                                // workgroups at most that share the target chunks of one (column chunk, row)
static_assert(kPosChunkVec == kCbThreads * kCbLoads * 4 && kPosChunkScalar == kCbThreads * kCbLoads, "a column chunk is one load round of a workgroup");
static_assert(kCbTargets <= kCbThreads, "one thread stages one target");

// the composite of template entry e holding the word v (0: no entry)
__device__ __forceinline__ u64 pos_cell(uint32_t v, uint32_t e)
{
    const uint32_t key = rank_key(__builtin_bit_cast(float, v));
    return key >= kPosFloor ? rank_composite(key, e) : (u64)0;
}
// ... of subject slot e holding the composite b of k_subject_best (0: no entry — no covered template, every template filtered out, or a best word below -inf's)
__device__ __forceinline__ u64 pos_slot(u64 b, uint32_t e)
{
    return (b != 0 && composite_word(b) >= kPosFloor) ? composite_at(b, e) : (u64)0;
}

// kMode 0 templates: pos = a column of scores [n_q][G].  1 subjects: pos = a slot of best [n_q][S]; scores is the matrix best was made of.  2 afis_count_before: comp
// [m] is the host's; pos = the column the hypothetical entry's index names, or -1.  row / pos [m] (row < n_q; pos inside the row, mode 2: or -1).
template <int kMode>
__global__ __launch_bounds__(kCbThreads) void k_position_targets(const uint32_t* __restrict__ scores, int G, const u64* __restrict__ best, int S, const int32_t* __restrict__ row,
                                                                 const int32_t* __restrict__ pos, size_t m, const long long* __restrict__ d_global, long long index_base,
                                                                 u64* __restrict__ comp, u64* __restrict__ count, int32_t* __restrict__ status, uint32_t* __restrict__ score,
                                                                 long long* __restrict__ best_idx)
{
    const size_t i = (size_t)blockIdx.x * kCbThreads + threadIdx.x;
    if (i >= m) return;
    const size_t q = (size_t)row[i];
    const int p = pos[i];
    if (kMode == 2) {
        u64 own = 0;
        if (p >= 0 && p < G) own = pos_cell(scores[q * (size_t)G + (size_t)p], (uint32_t)p);
        count[i] = own > comp[i] ? ~(u64)0 : (u64)0;                        // the column of the target itself is never counted: the hot pass will count it, this takes it back
        return;
    }
    u64 c = 0; uint32_t word = 0xff800000u; long long bi = -1;              // no entry: score -inf, best_idx -1
    if (kMode == 0) {
        if (p >= 0 && p < G) { const uint32_t v = scores[q * (size_t)G + (size_t)p]; c = pos_cell(v, (uint32_t)p); if (c) word = v; }
    } else if (p >= 0 && p < S) {
        const u64 b = best[q * (size_t)S + (size_t)p];
        const uint32_t at = composite_position(b);                          // a position of the row: k_subject_best made the composite from one
        if (at < (uint32_t)G) {
            c = pos_slot(b, (uint32_t)p);
            if (c) { word = scores[q * (size_t)G + at]; bi = d_global ? d_global[at] : index_base + (long long)at; }
        }
    }
    comp[i] = c ? c : ~(u64)0;
    count[i] = 0;
    status[i] = c ? kPosListed : kPosNoEntry;
    score[i] = word;
    if (kMode == 1) best_idx[i] = bi;
}

// scores [n_q][n] words (templates) or best [n_q][n] composites (subjects); rows [n_rows] the rows that have targets, off [n_rows + 1] their targets' ranges in
// comp / count [m]; kCols 4: n % 4 == 0 and the matrix 16-byte aligned
template <bool kSubjects, int kCols>
__global__ __launch_bounds__(kCbThreads) void k_count_before(const uint32_t* __restrict__ scores, const u64* __restrict__ best, int n, const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ off, int n_rows, const u64* __restrict__ comp, u64* __restrict__ count)
{
    constexpr int kPer = kCbLoads * kCols;
    __shared__ u64 s_tgt[kCbTargets];
    __shared__ uint32_t s_part[kCbWaves][kCbTargets];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t col0 = (size_t)blockIdx.x * (size_t)(kCbThreads * kPer);
    for (int r = (int)blockIdx.y; r < n_rows; r += (int)gridDim.y) {        // (block index and a launch argument: the same trips in every thread)
        const size_t at = (size_t)rows[r] * (size_t)n;
        const int t0 = off[r] + (int)blockIdx.z * kCbTargets, t1 = off[r + 1], t_step = (int)gridDim.z * kCbTargets;
        if (t0 >= t1) continue;                                             // this row has fewer target chunks than the grid is deep (uniform: block index and the CSR)
        u64 c[kPer];
        if constexpr (kSubjects) {
            u64 b[kCbLoads];
#pragma unroll
            for (int j = 0; j < kCbLoads; ++j) { const size_t e = col0 + (size_t)(j * kCbThreads + tid); b[j] = e < (size_t)n ? best[at + e] : (u64)0; }
#pragma unroll
            for (int j = 0; j < kCbLoads; ++j) c[j] = pos_slot(b[j], (uint32_t)(col0 + (size_t)(j * kCbThreads + tid)));
        } else if constexpr (kCols == 4) {
            uint4 v[kCbLoads];
#pragma unroll
            for (int j = 0; j < kCbLoads; ++j) {                            // (n % 4 == 0: with e inside the row, e + 3 is too)
                const size_t e = col0 + (size_t)(j * kCbThreads + tid) * 4;
                v[j] = e < (size_t)n ? *reinterpret_cast<const uint4*>(scores + at + e) : make_uint4(kNoEntryWord, kNoEntryWord, kNoEntryWord, kNoEntryWord);
            }
#pragma unroll
            for (int j = 0; j < kCbLoads; ++j) {
                const uint32_t e = (uint32_t)(col0 + (size_t)(j * kCbThreads + tid) * 4);
                c[4 * j] = pos_cell(v[j].x, e); c[4 * j + 1] = pos_cell(v[j].y, e + 1); c[4 * j + 2] = pos_cell(v[j].z, e + 2); c[4 * j + 3] = pos_cell(v[j].w, e + 3);
            }
        } else {
            uint32_t v[kCbLoads];
#pragma unroll
            for (int j = 0; j < kCbLoads; ++j) { const size_t e = col0 + (size_t)(j * kCbThreads + tid); v[j] = e < (size_t)n ? scores[at + e] : kNoEntryWord; }
#pragma unroll
            for (int j = 0; j < kCbLoads; ++j) c[j] = pos_cell(v[j], (uint32_t)(col0 + (size_t)(j * kCbThreads + tid)));
        }
        for (int tb = t0; tb < t1; tb += t_step) {                          // (t0, t1, t_step: the same in every thread)
            const int nt = t1 - tb < kCbTargets ? t1 - tb : kCbTargets;
            if (tid < nt) s_tgt[tid] = comp[tb + tid];
            __syncthreads();
            for (int t = 0; t < nt; ++t) {
                const u64 tv = s_tgt[t];                                    // one address for the whole wave: a broadcast; the value is wave-uniform
                const u64 T = ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tv >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tv);
                uint32_t w = 0;
#pragma unroll
                for (int j = 0; j < kPer; ++j) w += (uint32_t)__popcll(__ballot(c[j] > T));
                if (lane == 0) s_part[wave][t] = w;
            }
            __syncthreads();
            if (tid < nt) {
                uint32_t sum = 0;
#pragma unroll
                for (int v = 0; v < kCbWaves; ++v) sum += s_part[v][tid];
                if (sum) atomicAdd(count + tb + tid, (u64)sum);             // one integer add per (workgroup, target)
            }
            __syncthreads();                                                // the next chunk rewrites s_tgt and s_part
        }
    }
}

hipError_t launch_position_targets(int mode, const float* scores, int G, const unsigned long long* best, int S, const int32_t* row, const int32_t* pos, size_t m,
                                   const long long* d_global, long long index_base, unsigned long long* comp, unsigned long long* count, int32_t* status, float* score,
                                   long long* best_idx, hipStream_t stream)
{
    if (m == 0) return hipSuccess;
    if (!scores || G <= 0 || !row || !pos || !comp || !count || (mode != 2 && (!status || !score)) || (mode == 1 && (!best || S <= 0 || !best_idx)) || mode < 0 || mode > 2)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((m + kCbThreads - 1) / kCbThreads));
    const uint32_t* const sc = (const uint32_t*)scores;
    if (mode == 0) hipLaunchKernelGGL(k_position_targets<0>, grid, dim3(kCbThreads), 0, stream, sc, G, best, S, row, pos, m, d_global, index_base, comp, count, status, (uint32_t*)score, best_idx);
    else if (mode == 1) hipLaunchKernelGGL(k_position_targets<1>, grid, dim3(kCbThreads), 0, stream, sc, G, best, S, row, pos, m, d_global, index_base, comp, count, status, (uint32_t*)score, best_idx);
    else hipLaunchKernelGGL(k_position_targets<2>, grid, dim3(kCbThreads), 0, stream, sc, G, best, S, row, pos, m, d_global, index_base, comp, count, status, (uint32_t*)score, best_idx);
    return hipGetLastError();
}

hipError_t launch_count_before(const float* scores, const unsigned long long* best, int n, const int32_t* rows, const int32_t* off, int n_rows, int max_row_targets,
                               const unsigned long long* comp, unsigned long long* count, hipStream_t stream)
{
    if (n_rows <= 0 || n <= 0 || max_row_targets <= 0) return hipSuccess;
    if ((!scores && !best) || !rows || !off || !comp || !count) return hipErrorInvalidValue;
    const uint32_t* const sc = (const uint32_t*)scores;
    const bool vec = !best && rows_take_16_bytes(n, scores, scores);
    const size_t chunk = vec ? kPosChunkVec : kPosChunkScalar;
    const int depth = (max_row_targets + kCbTargets - 1) / kCbTargets;
    const dim3 grid((unsigned)(((size_t)n + chunk - 1) / chunk), grid_clamp((size_t)n_rows), (unsigned)(depth < kCbDepth ? depth : kCbDepth));
    if (best) hipLaunchKernelGGL((k_count_before<true, 1>), grid, dim3(kCbThreads), 0, stream, sc, best, n, rows, off, n_rows, comp, count);
    else if (vec) hipLaunchKernelGGL((k_count_before<false, 4>), grid, dim3(kCbThreads), 0, stream, sc, best, n, rows, off, n_rows, comp, count);
    else hipLaunchKernelGGL((k_count_before<false, 1>), grid, dim3(kCbThreads), 0, stream, sc, best, n, rows, off, n_rows, comp, count);
    return hipGetLastError();
}

}  // namespace afis
