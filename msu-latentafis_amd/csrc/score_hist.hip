// score_hist.hip — device code of the score distributions (afis_distribution.cpp: afis_score_histogram, afis_entries_at).  The definitions — an entry, the bin of an
// entry, one digit of the select — are score_hist.h's, shared with the host.
//
// Both hot kernels count cells into LDS bins, and real rows put most cells into one or two of them (the zeros, the -1 of empty templates; the top digits of a key):
// one LDS atomic per cell would serialise a wave on one word.  sh_count aggregates inside the wave first: up to kShRounds times, the lanes whose bin equals the first
// live lane's are balloted, the leader adds the popcount once and they retire; what is still live then — the spread-out remainder — adds 1 by itself.  A one-bin wave
// costs one atomic, a spread-out wave two rounds of scalar work on top of its own atomics.
//
// k_score_hist_rows: matrix [rows][cols] -> tab [rows][n_edges + 1] u64, zeroed by the launcher.  Grid = (column chunks, strips of kFilterRows rows), the shape of
// k_score_stats_rows.  The edge keys are staged once per workgroup in LDS.  A workgroup owns kShChunkScalar adjacent columns — kShChunkVec where every row starts on a
// 16-byte boundary (four columns as one 16-byte word) — of the rows of its strip: a thread issues the whole strip's loads, one per row, before it looks at the first
// cell (a lane past the row's end holds the no-entry word, which has no bin), finds each cell's bin by hist_bin's branch-free search in LDS and counts it into the
// row's 32-bit LDS histogram.  A strip's kFilterRows histograms stand side by side in LDS (32 bytes per bin: 32 KB at 1024 bins), so no barrier separates the rows: one
// barrier at the strip's end, then the workgroup's non-zero bins are added to the rows' u64 bins with integer atomicAdds and cleared.  Integer adds commute: the table
// does not depend on the order in which workgroups arrive.  Axis 1 is the same kernel over the transposed matrix (launch_transpose_scores).
// Why one load per row and thread: the counting chain of a cell — ballot, scalar round trip, read-lane, ballot — has nothing to overlap with inside one wave.  With four
// loads per row and thread (13 x 25 workgroups for 100 x 100 000 cells: one wave per SIMD) the kernel took 1.9 times as long, whatever was done about its loads (the next
// row fetched ahead, the whole strip in flight) or its barriers; 13 x 98 workgroups put four waves on a SIMD, whose chains hide one another.
//
// The entry at a rank: a radix select on the row's composites, 8 bits per pass from the top (the position bytes no entry differs in are skipped by the host).
//   k_select_count   grid = (column chunks, rows that have targets, workgroups that share a row's targets); the targets arrive sorted into a CSR by row, as
//                    k_count_before's.  A thread loads kSelLoads x kCols entries of its row once, all loads before the first use, and forms their composites once, in
//                    registers (no entry: 0).  The row's targets — sorted by rank by the host, so that targets with the same fixed digits are neighbours — pass through
//                    LDS in chunks of kSelTargetChunk (256 bins x 4 bytes each: 16 KB per chunk); the bins of a target depend on its row and its fixed digits only,
//                    so only the first target of a run of equal fixed digits inside a chunk counts (in the first pass: one per chunk): the entries that share
//                    its fixed digits count into its 256 bins by this pass's digit, through sh_count; the workgroup's non-zero bins are added to
//                    tab [target][256] u64 with integer adds.
//   k_select_step    one thread per target: finds the target of its chunk that counted for it, and select_step over those 256 counts fixes the digit and reduces
//                    the residual rank; a rank that is not below the total — it can only happen in the first pass, whose total is the row's number of entries —
//                    marks the target as no entry (residual ~0).  The new prefixes go to a second array (the launcher swaps the two after every pass).
//   k_select_finish  one thread per target: the fixed digits are the entry's composite, its low word the position; reads that cell and writes idx, the score's own bits
//                    and the status.
// Every barrier sits in a loop whose bounds come from block indices and launch arguments or the CSR: the same trips in every thread.  Matrix indices are size_t.
// A workgroup counts at most 256 x 4 x 4 cells per row and target in 32 bits; the tables are 64-bit.  No float atomics anywhere.
//
// Persons (afis_subject_score_histogram, afis_subject_entries_at): k_subject_keys takes the high halves of ctx->subj_best [n_q][S] into a matrix [n_q][S] of 4-byte
// person cells, and k_score_hist_rows and k_select_count run over it as they run over a score matrix — the same bodies, instantiated with score_cell.h's PersonCell,
// for which a cell is its own key; a position is a slot.  Only the last kernel differs: k_subject_select_finish names the person and the person's best template.
#include "afis_device.h"
#include "score_hist.h"
#include <type_traits>
#include <utility>

namespace afis {

constexpr int kShThreads = 256;
constexpr int kShLoads = 1;                                                 // k_score_hist_rows: loads per thread and row (a strip's kFilterRows x kShLoads are in flight together)
constexpr int kSelLoads = 4;                                                // k_select_count: loads in flight per thread
constexpr int kShRounds = 2;                                                // wave aggregation rounds before a lane counts by itself
constexpr int kSelTargets = kSelTargetChunk;                                // targets staged in LDS at a time
constexpr int kSelDepth = 32;                                               // workgroups at most that share the target chunks of one (column chunk, row)
constexpr u64 kSelDead = ~(u64)0;                                           // a target's residual once it is known to be no entry
static_assert(kShChunkScalar == kShThreads * kShLoads && kShChunkVec == 4 * kShChunkScalar && kSelChunkScalar == kShThreads * kSelLoads && kSelChunkVec == 4 * kSelChunkScalar,
              "afis_device.h names the column chunks");
static_assert(kEntryFloor == kPosFloor, "an entry is what the rank positions call one");
static_assert(kHistEdgesMax + 1 == 1024 && kSelectBins == 256, "the LDS histograms");
static_assert(kSelTargets * kSelectBins * 4 <= 16384, "a target chunk's bins take 16 KB of LDS");

// bins[bin] += 1 for every lane with bin >= 0.  Every lane of the wave calls it (wave-uniform control flow).
__device__ __forceinline__ void sh_count(uint32_t* bins, int bin, int lane)
{
    bool live = bin >= 0;
#pragma unroll
    for (int round = 0; round < kShRounds; ++round) {
        const u64 act = __ballot(live);
        if (act == 0) return;                                               // (a ballot: the same in every lane)
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)act) - 1);
        const int b = __builtin_amdgcn_readlane(bin, leader);
        const bool same = live && bin == b;
        const u64 m = __ballot(same);
        if (lane == leader) atomicAdd(bins + b, (uint32_t)__popcll(m));
        live = live && !same;
    }
    if (live) atomicAdd(bins + bin, 1u);
}

// Cell (score_cell.h): what a cell's key is — ScoreCell for a matrix of score words, PersonCell for k_subject_keys' matrix
template <bool kVec, class Cell>
__global__ __launch_bounds__(kShThreads) void k_score_hist_rows(const uint32_t* __restrict__ matrix, int rows_n, int cols, const uint32_t* __restrict__ edge_keys, int n_edges,
                                                                int top_step, u64* __restrict__ tab)
{
    constexpr int kCols = kVec ? 4 : 1;
    constexpr uint32_t kNone = Cell::kNone;
    using W = typename std::conditional<kVec, uint4, uint32_t>::type;
    __shared__ uint32_t s_edge[kHistEdgesMax + 1];
    extern __shared__ uint32_t s_hist[];                                    // a strip's histograms [kFilterRows][n_edges + 1], sized by the launcher (32 KB at 1024 bins): the rows of a strip are counted without a barrier between them
    const int tid = threadIdx.x, lane = tid & 63, n_bins = n_edges + 1;
    for (int i = tid; i <= kHistEdgesMax; i += kShThreads) s_edge[i] = i < n_edges ? edge_keys[i] : 0xffffffffu;
    for (int i = tid; i < kFilterRows * n_bins; i += kShThreads) s_hist[i] = 0;
    __syncthreads();
    const size_t col0 = (size_t)blockIdx.x * (size_t)(kShThreads * kCols * kShLoads) + (size_t)tid * kCols;
    const int strips = (rows_n + kFilterRows - 1) / kFilterRows;
    for (int st = (int)blockIdx.y; st < strips; st += (int)gridDim.y) {
        const int q0 = st * kFilterRows, rows = rows_n - q0 < kFilterRows ? rows_n - q0 : kFilterRows;
        W v[kFilterRows][kShLoads];
#pragma unroll
        for (int r = 0; r < kFilterRows; ++r) {                             // the whole strip's loads are issued before the first cell is looked at (a row past the strip's end: no entries)
            const size_t row = (size_t)(q0 + r) * (size_t)cols;
#pragma unroll
            for (int l = 0; l < kShLoads; ++l) {                            // (kVec: cols % 4 == 0, so col < cols means col + 3 < cols)
                const size_t col = col0 + (size_t)l * (size_t)(kShThreads * kCols);
                const bool in = r < rows && col < (size_t)cols;
                if constexpr (kVec) v[r][l] = in ? *reinterpret_cast<const uint4*>(matrix + row + col) : make_uint4(kNone, kNone, kNone, kNone);
                else v[r][l] = in ? matrix[row + col] : kNone;
            }
        }
#pragma unroll
        for (int r = 0; r < kFilterRows; ++r) {
            if (r >= rows) break;                                           // (uniform over the workgroup)
            int b[kShLoads * kCols];
#pragma unroll
            for (int l = 0; l < kShLoads; ++l) {                            // every search before the first count: the LDS reads of a thread's cells overlap
                if constexpr (kVec) {
                    b[4 * l] = hist_bin<Cell>(s_edge, n_edges, top_step, v[r][l].x); b[4 * l + 1] = hist_bin<Cell>(s_edge, n_edges, top_step, v[r][l].y);
                    b[4 * l + 2] = hist_bin<Cell>(s_edge, n_edges, top_step, v[r][l].z); b[4 * l + 3] = hist_bin<Cell>(s_edge, n_edges, top_step, v[r][l].w);
                } else b[l] = hist_bin<Cell>(s_edge, n_edges, top_step, v[r][l]);
            }
#pragma unroll
            for (int j = 0; j < kShLoads * kCols; ++j) sh_count(s_hist + r * n_bins, b[j], lane);
        }
        __syncthreads();                                                    // (st, strips and gridDim.y are the same in every thread: every thread reaches both barriers)
        for (int i = tid; i < rows * n_bins; i += kShThreads) {
            const uint32_t c = s_hist[i];                                   // (row r, bin b at r x n_bins + b, in LDS and — the strip's rows are adjacent — in the table)
            if (c) { atomicAdd(tab + (size_t)q0 * (size_t)n_bins + i, (u64)c); s_hist[i] = 0; }   // one integer add per (workgroup, row, non-zero bin)
        }
        __syncthreads();
    }
}

// scores [n_q][n] words; rows [n_rows] the rows that have targets, off [n_rows + 1] their targets' ranges in prefix / remain [m] and tab [m][256]; a target's prefix
// holds the digits above shift + 8 that are fixed (high_mask covers them: 0 in the first pass); kCols 4: n % 4 == 0 and the matrix 16-byte aligned
template <int kCols, class Cell>
__global__ __launch_bounds__(kShThreads) void k_select_count(const uint32_t* __restrict__ scores, int n, const int32_t* __restrict__ rows, const int32_t* __restrict__ off, int n_rows,
                                                             const u64* __restrict__ prefix, int shift, u64 high_mask, u64* __restrict__ tab)
{
    constexpr int kPer = kSelLoads * kCols;
    constexpr uint32_t kNone = Cell::kNone;
    __shared__ uint32_t s_bins[kSelTargets * kSelectBins];
    __shared__ u64 s_prefix[kSelTargets];
    __shared__ uint32_t s_counts[kSelTargets];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < kSelTargets * kSelectBins; i += kShThreads) s_bins[i] = 0;
    __syncthreads();
    const size_t col0 = (size_t)blockIdx.x * (size_t)(kShThreads * kPer);
    for (int r = (int)blockIdx.y; r < n_rows; r += (int)gridDim.y) {        // (block index and a launch argument: the same trips in every thread)
        const size_t at = (size_t)rows[r] * (size_t)n;
        const int t0 = off[r] + (int)blockIdx.z * kSelTargets, t1 = off[r + 1], t_step = (int)gridDim.z * kSelTargets;
        if (t0 >= t1) continue;                                             // this row has fewer target chunks than the grid is deep (uniform: block index and the CSR)
        u64 c[kPer];
        if constexpr (kCols == 4) {
            uint4 v[kSelLoads];
#pragma unroll
            for (int j = 0; j < kSelLoads; ++j) {                            // (n % 4 == 0: with e inside the row, e + 3 is too)
                const size_t e = col0 + (size_t)(j * kShThreads + tid) * 4;
                v[j] = e < (size_t)n ? *reinterpret_cast<const uint4*>(scores + at + e) : make_uint4(kNone, kNone, kNone, kNone);
            }
#pragma unroll
            for (int j = 0; j < kSelLoads; ++j) {
                const uint32_t e = (uint32_t)(col0 + (size_t)(j * kShThreads + tid) * 4);
                const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) { const uint32_t key = Cell::key(w[k]); c[4 * j + k] = key >= kEntryFloor ? rank_composite(key, e + k) : (u64)0; }
            }
        } else {
            uint32_t v[kSelLoads];
#pragma unroll
            for (int j = 0; j < kSelLoads; ++j) { const size_t e = col0 + (size_t)(j * kShThreads + tid); v[j] = e < (size_t)n ? scores[at + e] : kNone; }
#pragma unroll
            for (int j = 0; j < kSelLoads; ++j) {
                const uint32_t key = Cell::key(v[j]);
                c[j] = key >= kEntryFloor ? rank_composite(key, (uint32_t)(col0 + (size_t)(j * kShThreads + tid))) : (u64)0;
            }
        }
        for (int tb = t0; tb < t1; tb += t_step) {                          // (t0, t1, t_step: the same in every thread)
            const int nt = t1 - tb < kSelTargets ? t1 - tb : kSelTargets;
            if (tid < nt) {                                                 // a target whose fixed digits are its neighbour's shares that neighbour's bins: only the first of a run counts
                const u64 p = prefix[tb + tid];
                s_prefix[tid] = p; s_counts[tid] = tid == 0 || ((p ^ prefix[tb + tid - 1]) & high_mask) != 0;
            }
            __syncthreads();
            for (int t = 0; t < nt; ++t) {
                if (!__builtin_amdgcn_readfirstlane((int)s_counts[t])) continue;   // (one address for the whole wave: uniform)
                const u64 pv = s_prefix[t];
                const u64 P = ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(pv >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pv);
                uint32_t* const bins = s_bins + t * kSelectBins;
#pragma unroll
                for (int j = 0; j < kPer; ++j) {
                    const bool match = c[j] != 0 && ((c[j] ^ P) & high_mask) == 0;
                    sh_count(bins, match ? (int)((c[j] >> shift) & (u64)(kSelectBins - 1)) : -1, lane);
                }
            }
            __syncthreads();
            u64* const dst = tab + (size_t)tb * kSelectBins;
            for (int i = tid; i < nt * kSelectBins; i += kShThreads) {
                const uint32_t cnt = s_bins[i];
                if (cnt) { atomicAdd(dst + i, (u64)cnt); s_bins[i] = 0; }   // one integer add per (workgroup, target, non-zero bin)
            }
            __syncthreads();                                                // the next chunk rewrites s_prefix, s_counts and s_bins
        }
    }
}

// first [m]: where the target's row begins in the target arrays (the CSR's off of its row): the chunks k_select_count staged begin at first + a multiple of kSelTargets
__global__ __launch_bounds__(kShThreads) void k_select_step(const u64* __restrict__ tab, size_t m, int shift, u64 high_mask, const int32_t* __restrict__ first,
                                                            const u64* __restrict__ prefix, u64* __restrict__ prefix_out, u64* __restrict__ remain)
{
    const size_t i = (size_t)blockIdx.x * kShThreads + threadIdx.x;
    if (i >= m) return;
    const u64 p = prefix[i];
    prefix_out[i] = p;
    uint64_t r = remain[i];
    if (r == kSelDead) return;
    const size_t f = (size_t)first[i], chunk = f + (i - f) / kSelTargets * kSelTargets;
    size_t j = i;                                                           // the target of the chunk that counted for this one: the first of its run
    while (j > chunk && ((prefix[j - 1] ^ p) & high_mask) == 0) --j;
    const int d = select_step(reinterpret_cast<const uint64_t*>(tab + j * kSelectBins), &r);
    if (d < 0) { remain[i] = kSelDead; return; }
    prefix_out[i] = p | ((u64)d << shift);
    remain[i] = (u64)r;
}

__global__ __launch_bounds__(kShThreads) void k_select_finish(const uint32_t* __restrict__ scores, int n, const int32_t* __restrict__ row, const u64* __restrict__ prefix,
                                                              const u64* __restrict__ remain, size_t m, const long long* __restrict__ d_global, long long index_base,
                                                              long long* __restrict__ idx, uint32_t* __restrict__ score, int32_t* __restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * kShThreads + threadIdx.x;
    if (i >= m) return;
    const uint32_t p = composite_position(prefix[i]);
    const bool found = remain[i] != kSelDead && p < (uint32_t)n;
    idx[i] = found ? (d_global ? d_global[p] : index_base + (long long)p) : -1;
    score[i] = found ? scores[(size_t)row[i] * (size_t)n + p] : 0xff800000u;
    status[i] = found ? kPosListed : kPosNoEntry;
}

// The person form of k_select_finish: the fixed digits are (K, ~slot); the slot names the person, its composite in best [n_q][S] holds the score (K is its ordered
// word) and, in the low half, the position of the best template, named as k_topk_subjects names it
__global__ __launch_bounds__(kShThreads) void k_subject_select_finish(const u64* __restrict__ best, int S, int G, const int32_t* __restrict__ row, const u64* __restrict__ prefix,
                                                                      const u64* __restrict__ remain, size_t m, const long long* __restrict__ ids,
                                                                      const long long* __restrict__ d_global, long long index_base, long long* __restrict__ id,
                                                                      uint32_t* __restrict__ score, long long* __restrict__ best_idx, int32_t* __restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * kShThreads + threadIdx.x;
    if (i >= m) return;
    const uint32_t slot = composite_position(prefix[i]);
    const bool in = remain[i] != kSelDead && slot < (uint32_t)S;
    const u64 b = in ? best[(size_t)row[i] * (size_t)S + slot] : (u64)0;
    const uint32_t pos = composite_position(b);                             // < G: an entry's composite was made from a position of the row
    const bool found = in && pos < (uint32_t)G;
    id[i] = found ? ids[slot] : -1;
    score[i] = found ? score_bits_of(person_cell(b)) : 0xff800000u;
    best_idx[i] = found ? (d_global ? d_global[pos] : index_base + (long long)pos) : -1;
    status[i] = found ? kPosListed : kPosNoEntry;
}

// best [n] composites of subj_best -> keys [n] person cells (score_cell.h): one coalesced pass, 8 bytes in and 4 bytes out per cell
__global__ __launch_bounds__(kShThreads) void k_subject_keys(const u64* __restrict__ best, size_t n, uint32_t* __restrict__ keys)
{
    const size_t step = (size_t)gridDim.x * kShThreads;
    for (size_t i = (size_t)blockIdx.x * kShThreads + threadIdx.x; i < n; i += step) keys[i] = person_cell(best[i]);
}

hipError_t launch_subject_keys(const unsigned long long* best, int n_q, int S, uint32_t* keys, hipStream_t stream)
{
    if (n_q <= 0 || S <= 0) return hipSuccess;
    if (!best || !keys) return hipErrorInvalidValue;
    const size_t n = (size_t)n_q * (size_t)S, blocks = (n + kShThreads - 1) / kShThreads;
    hipLaunchKernelGGL(k_subject_keys, dim3((unsigned)(blocks < ((size_t)1 << 20) ? blocks : (size_t)1 << 20)), dim3(kShThreads), 0, stream, best, n, keys);
    return hipGetLastError();
}

template <class Cell>
static hipError_t score_hist(const uint32_t* m, int rows, int cols, const uint32_t* edge_keys, int n_edges, unsigned long long* tab, hipStream_t stream)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!m || !edge_keys || !tab || n_edges < 1 || n_edges > kHistEdgesMax) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(tab, 0, (size_t)rows * (size_t)(n_edges + 1) * 8, stream);
    if (e != hipSuccess) return e;
    const bool vec = rows_take_16_bytes(cols, m, m);
    const size_t chunk = vec ? kShChunkVec : kShChunkScalar;
    const dim3 grid((unsigned)(((size_t)cols + chunk - 1) / chunk), grid_clamp((size_t)((rows + kFilterRows - 1) / kFilterRows)));
    const int top = hist_top_step(n_edges);
    const size_t lds = (size_t)kFilterRows * (size_t)(n_edges + 1) * 4;
    if (vec) hipLaunchKernelGGL((k_score_hist_rows<true, Cell>), grid, dim3(kShThreads), lds, stream, m, rows, cols, edge_keys, n_edges, top, tab);
    else hipLaunchKernelGGL((k_score_hist_rows<false, Cell>), grid, dim3(kShThreads), lds, stream, m, rows, cols, edge_keys, n_edges, top, tab);
    return hipGetLastError();
}

hipError_t launch_score_hist(const float* matrix, int rows, int cols, const uint32_t* edge_keys, int n_edges, unsigned long long* tab, hipStream_t stream)
{
    return score_hist<ScoreCell>((const uint32_t*)matrix, rows, cols, edge_keys, n_edges, tab, stream);
}

hipError_t launch_subject_hist(const uint32_t* keys, int rows, int cols, const uint32_t* edge_keys, int n_edges, unsigned long long* tab, hipStream_t stream)
{
    return score_hist<PersonCell>(keys, rows, cols, edge_keys, n_edges, tab, stream);
}

// the digits of the select, for both forms; *prefix is left pointing at the copy that holds every target's fixed digits
template <class Cell>
static hipError_t select_digits(const uint32_t* sc, int n, const int32_t* rows, const int32_t* off, int n_rows, int max_row_targets, const int32_t* first, size_t m,
                                unsigned long long** prefix, unsigned long long* prefix_spare, unsigned long long* remain, unsigned long long* tab, hipStream_t stream)
{
    unsigned long long* p = *prefix;
    const bool vec = rows_take_16_bytes(n, sc, sc);
    const size_t chunk = vec ? kSelChunkVec : kSelChunkScalar;
    const int depth = (max_row_targets + kSelTargets - 1) / kSelTargets;
    const dim3 grid((unsigned)(((size_t)n + chunk - 1) / chunk), grid_clamp((size_t)n_rows), (unsigned)(depth < kSelDepth ? depth : kSelDepth));
    const dim3 per_target((unsigned)((m + kShThreads - 1) / kShThreads));
    const int low = select_position_digits(n);
    for (int pass = 0; pass < 4 + low; ++pass) {                            // the four bytes of the key, then the position bytes that differ
        const int shift = pass < 4 ? 56 - 8 * pass : 8 * (low - 1 - (pass - 4));
        const u64 high_mask = shift == 56 ? (u64)0 : ~(u64)0 << (shift + 8);
        const hipError_t e = hipMemsetAsync(tab, 0, m * kSelectBins * 8, stream);
        if (e != hipSuccess) return e;
        if (vec) hipLaunchKernelGGL((k_select_count<4, Cell>), grid, dim3(kShThreads), 0, stream, sc, n, rows, off, n_rows, p, shift, high_mask, tab);
        else hipLaunchKernelGGL((k_select_count<1, Cell>), grid, dim3(kShThreads), 0, stream, sc, n, rows, off, n_rows, p, shift, high_mask, tab);
        hipLaunchKernelGGL(k_select_step, per_target, dim3(kShThreads), 0, stream, tab, m, shift, high_mask, first, p, prefix_spare, remain);
        std::swap(p, prefix_spare);                                         // the step wrote the other copy: no thread reads a neighbour's prefix while it changes
    }
    *prefix = p;
    return hipGetLastError();
}

hipError_t launch_entries_at(const float* scores, int n, const int32_t* rows, const int32_t* off, int n_rows, int max_row_targets, const int32_t* row, const int32_t* first, size_t m,
                             unsigned long long* prefix, unsigned long long* prefix_spare, unsigned long long* remain, unsigned long long* tab, const long long* d_global, long long index_base,
                             long long* idx, float* score, int32_t* status, hipStream_t stream)
{
    if (m == 0 || n_rows <= 0) return hipSuccess;
    if (!scores || n <= 0 || !rows || !off || !row || !first || !prefix || !prefix_spare || !remain || !tab || !idx || !score || !status || max_row_targets <= 0) return hipErrorInvalidValue;
    const uint32_t* const sc = (const uint32_t*)scores;
    const hipError_t e = select_digits<ScoreCell>(sc, n, rows, off, n_rows, max_row_targets, first, m, &prefix, prefix_spare, remain, tab, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_select_finish, dim3((unsigned)((m + kShThreads - 1) / kShThreads)), dim3(kShThreads), 0, stream, sc, n, row, prefix, remain, m, d_global, index_base, idx,
                       (uint32_t*)score, status);
    return hipGetLastError();
}

hipError_t launch_subject_entries_at(const uint32_t* keys, const unsigned long long* best, int S, int G, const int32_t* rows, const int32_t* off, int n_rows, int max_row_targets,
                                     const int32_t* row, const int32_t* first, size_t m, unsigned long long* prefix, unsigned long long* prefix_spare, unsigned long long* remain,
                                     unsigned long long* tab, const long long* ids, const long long* d_global, long long index_base, long long* id, float* score, long long* best_idx,
                                     int32_t* status, hipStream_t stream)
{
    if (m == 0 || n_rows <= 0) return hipSuccess;
    if (!keys || !best || S <= 0 || G <= 0 || !rows || !off || !row || !first || !prefix || !prefix_spare || !remain || !tab || !ids || !id || !score || !best_idx || !status ||
        max_row_targets <= 0) return hipErrorInvalidValue;
    const hipError_t e = select_digits<PersonCell>(keys, S, rows, off, n_rows, max_row_targets, first, m, &prefix, prefix_spare, remain, tab, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_subject_select_finish, dim3((unsigned)((m + kShThreads - 1) / kShThreads)), dim3(kShThreads), 0, stream, best, S, G, row, prefix, remain, m, ids, d_global,
                       index_base, id, (uint32_t*)score, best_idx, status);
    return hipGetLastError();
}

}  // namespace afis
