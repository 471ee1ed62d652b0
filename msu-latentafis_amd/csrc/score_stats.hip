// score_stats.hip — device code of the cohort statistics and the z-normalised scores (afis_normalize.cpp: afis_score_stats, afis_normalize_scores).  The definitions —
// the three cell classes, q(v), the limb sums and their recombination, a normalised cell — are score_stats.h's, shared with the host.
//
// k_score_stats_rows (axis 0): matrix [n_q][G] -> tab [n_q][kStatWords], zeroed by the caller.  Grid = (column chunks, strips of kSsRows rows).  A workgroup owns
// kSsChunkScalar adjacent columns — kSsChunkVec where every row starts on a 16-byte boundary (G % 4 == 0: four columns travel as one 16-byte word, as in k_filter_rows)
// — and walks the rows of its strip; per row a thread issues its kSsLoads loads before it looks at the first (a lane past the row's end reads nothing and holds the
// no-entry word, which counts for nothing), classifies its cells and accumulates a row of limb sums in registers: two counts, five sums of the 18-bit limbs of q that
// cannot overflow while n <= 2^27, and the two extreme keys.  Then a wave reduction (__shfl_xor), a workgroup reduction through LDS and ONE integer atomic per word and
// workgroup into tab — adds for the seven sums, maxima for the two keys (the least key travels as its complement).  Integer adds and maxima commute: the table does not
// depend on the order in which workgroups arrive.  No float atomics.  k_score_stats_finish recombines a table row into the 48 bytes of a statistic.
// k_score_stats_cols (axis 1): a thread owns a column (four with 16-byte loads), walks ALL rows — a strip's loads in flight together, as k_filter_rows — and writes its
// columns' statistics itself: no cross-lane traffic, no atomics.
// k_normalize_scores: scores [n_q][G] -> out [n_q][G], one pass, 4 bytes in and 4 bytes out per cell, fp64 arithmetic.  Grid and row walk as k_filter_rows.  Axis 0:
// the row's (offset, scale) pair is indexed by the block index and the loop counter only, so it is a scalar load; axis 1: a thread loads its columns' pairs once.
// Persons (afis_subject_score_stats): the same two kernels over launch_subject_keys' matrix [n_q][S] of person cells, instantiated with score_cell.h's PersonCell —
// a cell stands for the score word whose ordered word it is; nothing else differs.
// Every index into the matrices is a size_t: n_q x G may pass 2^31.  A grid's second dimension holds 65 535 blocks; more strips than that are walked in a loop.
#include "afis_device.h"
#include "score_cell.h"
#include "score_stats.h"
#include <type_traits>

namespace afis {

constexpr int kSsThreads = 256;
constexpr int kSsLoads = 4;                                                 // loads in flight per thread and row
constexpr int kSsRows = kFilterRows;                                        // rows per strip
constexpr int kSsColThreads = 64;                                           // k_score_stats_cols: one wave per workgroup, so that 100 000 columns make 391 workgroups
static_assert(kSsChunkScalar == kSsThreads * kSsLoads && kSsChunkVec == 4 * kSsChunkScalar, "afis_device.h names the column chunks");

__device__ __forceinline__ void ss_zero(uint64_t* t)
{
#pragma unroll
    for (int i = 0; i < kStatWords; ++i) t[i] = 0;
}

// Cell (score_cell.h): which score word a cell stands for — ScoreCell: the cell itself; PersonCell: the word whose ordered word the cell is
template <bool kVec, class Cell>
__device__ __forceinline__ void ss_cells(uint64_t* t, typename std::conditional<kVec, uint4, uint32_t>::type v)
{
    if constexpr (kVec) { stat_limbs_cell(t, Cell::word(v.x)); stat_limbs_cell(t, Cell::word(v.y)); stat_limbs_cell(t, Cell::word(v.z)); stat_limbs_cell(t, Cell::word(v.w)); }
    else stat_limbs_cell(t, Cell::word(v));
}

template <bool kVec, class Cell>
__global__ __launch_bounds__(kSsThreads) void k_score_stats_rows(const uint32_t* __restrict__ matrix, int n_q, int G, u64* __restrict__ tab)
{
    constexpr int kCols = kVec ? 4 : 1;
    using W = typename std::conditional<kVec, uint4, uint32_t>::type;
    __shared__ uint64_t part[kSsThreads / 64][kStatWords];
    const size_t col0 = (size_t)blockIdx.x * (size_t)(kSsThreads * kCols * kSsLoads) + (size_t)threadIdx.x * kCols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strips = (n_q + kSsRows - 1) / kSsRows;
    for (int st = (int)blockIdx.y; st < strips; st += (int)gridDim.y) {
        const int q0 = st * kSsRows, rows = n_q - q0 < kSsRows ? n_q - q0 : kSsRows;
        for (int r = 0; r < rows; ++r) {                                    // (uniform over the workgroup: every thread reaches both barriers)
            const size_t row = (size_t)(q0 + r) * (size_t)G;
            W v[kSsLoads];
#pragma unroll
            for (int l = 0; l < kSsLoads; ++l) {                            // (kVec: G % 4 == 0, so col < G means col + 3 < G)
                const size_t col = col0 + (size_t)l * (size_t)(kSsThreads * kCols);
                if constexpr (kVec) v[l] = col < (size_t)G ? *reinterpret_cast<const uint4*>(matrix + row + col) : make_uint4(Cell::kNone, Cell::kNone, Cell::kNone, Cell::kNone);
                else v[l] = col < (size_t)G ? matrix[row + col] : Cell::kNone;
            }
            uint64_t t[kStatWords];
            ss_zero(t);
#pragma unroll
            for (int l = 0; l < kSsLoads; ++l) ss_cells<kVec, Cell>(t, v[l]);
#pragma unroll
            for (int i = 0; i < kStatWords; ++i)
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const uint64_t o = (uint64_t)__shfl_xor((u64)t[i], d, 64);
                    t[i] = i < 7 ? t[i] + o : (o > t[i] ? o : t[i]);
                }
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < kStatWords; ++i) part[wave][i] = t[i];
            __syncthreads();
            if (threadIdx.x < kStatWords) {
                const int i = threadIdx.x;
                uint64_t s = part[0][i];
                for (int w = 1; w < kSsThreads / 64; ++w) s = i < 7 ? s + part[w][i] : (part[w][i] > s ? part[w][i] : s);
                u64* const dst = tab + (size_t)(q0 + r) * kStatWords + i;
                if (s) { if (i < 7) atomicAdd(dst, (u64)s); else atomicMax(dst, (u64)s); }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void k_score_stats_finish(const u64* __restrict__ tab, int n, ScoreStat* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t t[kStatWords];
#pragma unroll
    for (int k = 0; k < kStatWords; ++k) t[k] = tab[(size_t)i * kStatWords + k];
    out[i] = stat_from_limbs(t);
}

template <bool kVec, class Cell>
__global__ __launch_bounds__(kSsColThreads) void k_score_stats_cols(const uint32_t* __restrict__ matrix, int n_q, int G, ScoreStat* __restrict__ out)
{
    constexpr int kCols = kVec ? 4 : 1;
    using W = typename std::conditional<kVec, uint4, uint32_t>::type;
    const size_t col = ((size_t)blockIdx.x * kSsColThreads + threadIdx.x) * kCols;
    if (col >= (size_t)G) return;                                           // (no barrier below)
    uint64_t t[kCols][kStatWords];
#pragma unroll
    for (int j = 0; j < kCols; ++j) ss_zero(t[j]);
    const auto cells = [&](W v) {
        if constexpr (kVec) { stat_limbs_cell(t[0], Cell::word(v.x)); stat_limbs_cell(t[1], Cell::word(v.y)); stat_limbs_cell(t[2], Cell::word(v.z)); stat_limbs_cell(t[3], Cell::word(v.w)); }
        else stat_limbs_cell(t[0], Cell::word(v));
    };
    int q = 0;
    for (; q + kSsRows <= n_q; q += kSsRows) {                              // a whole strip: its kSsRows loads are in flight together
        const size_t at = (size_t)q * (size_t)G + col;
        W v[kSsRows];
#pragma unroll
        for (int r = 0; r < kSsRows; ++r) v[r] = *reinterpret_cast<const W*>(matrix + at + (size_t)r * (size_t)G);
#pragma unroll
        for (int r = 0; r < kSsRows; ++r) cells(v[r]);
    }
    for (; q < n_q; ++q) cells(*reinterpret_cast<const W*>(matrix + (size_t)q * (size_t)G + col));
#pragma unroll
    for (int j = 0; j < kCols; ++j) out[col + j] = stat_from_limbs(t[j]);
}

// pair [n_q] (axis 0) or [G] (axis 1): (offset, scale) as two doubles
template <int kAxis, bool kVec>
__global__ __launch_bounds__(kSsThreads) void k_normalize_scores(const uint32_t* __restrict__ scores, int n_q, int G, const double2* __restrict__ pair, uint32_t* __restrict__ out)
{
    constexpr int kCols = kVec ? 4 : 1;
    using W = typename std::conditional<kVec, uint4, uint32_t>::type;
    const size_t col = ((size_t)blockIdx.x * kSsThreads + threadIdx.x) * kCols;
    if (col >= (size_t)G) return;
    double2 P[kCols];
#pragma unroll
    for (int j = 0; j < kCols; ++j) P[j] = kAxis == 1 ? pair[col + j] : make_double2(0.0, 0.0);
    const auto norm = [&](W v, int q) -> W {                                // q is uniform over the workgroup: axis 0's pair is a scalar load
        if constexpr (kAxis == 0) {
            const double2 p = pair[q];
            if constexpr (kVec) return make_uint4(stat_normalized_word(v.x, p.x, p.y), stat_normalized_word(v.y, p.x, p.y), stat_normalized_word(v.z, p.x, p.y), stat_normalized_word(v.w, p.x, p.y));
            else return stat_normalized_word(v, p.x, p.y);
        } else {
            if constexpr (kVec) return make_uint4(stat_normalized_word(v.x, P[0].x, P[0].y), stat_normalized_word(v.y, P[1].x, P[1].y), stat_normalized_word(v.z, P[2].x, P[2].y), stat_normalized_word(v.w, P[3].x, P[3].y));
            else return stat_normalized_word(v, P[0].x, P[0].y);
        }
    };
    const int strips = (n_q + kSsRows - 1) / kSsRows;
    for (int st = (int)blockIdx.y; st < strips; st += (int)gridDim.y) {
        const int q0 = st * kSsRows, rows = n_q - q0 < kSsRows ? n_q - q0 : kSsRows;
        const size_t at = (size_t)q0 * (size_t)G + col;
        if (rows == kSsRows) {                                              // a whole strip: its kSsRows loads are in flight together
            W v[kSsRows];
#pragma unroll
            for (int r = 0; r < kSsRows; ++r) v[r] = *reinterpret_cast<const W*>(scores + at + (size_t)r * (size_t)G);
#pragma unroll
            for (int r = 0; r < kSsRows; ++r) *reinterpret_cast<W*>(out + at + (size_t)r * (size_t)G) = norm(v[r], q0 + r);
        } else
            for (int r = 0; r < rows; ++r) *reinterpret_cast<W*>(out + at + (size_t)r * (size_t)G) = norm(*reinterpret_cast<const W*>(scores + at + (size_t)r * (size_t)G), q0 + r);
    }
}

static_assert(sizeof(ScoreStat) == 48, "a statistic is 48 bytes");

template <class Cell>
static hipError_t score_stats(int axis, const uint32_t* m, int n_q, int G, unsigned long long* tab, void* out, hipStream_t stream)
{
    if (n_q <= 0 || G <= 0) return hipSuccess;
    if (!m || !out || (axis == 0 && !tab) || (axis != 0 && axis != 1)) return hipErrorInvalidValue;
    const bool vec = rows_take_16_bytes(G, m, m);
    if (axis == 0) {
        const hipError_t e = hipMemsetAsync(tab, 0, (size_t)n_q * kStatWords * 8, stream);
        if (e != hipSuccess) return e;
        const size_t chunk = vec ? kSsChunkVec : kSsChunkScalar;
        const dim3 grid((unsigned)(((size_t)G + chunk - 1) / chunk), grid_clamp((size_t)((n_q + kSsRows - 1) / kSsRows)));
        if (vec) hipLaunchKernelGGL((k_score_stats_rows<true, Cell>), grid, dim3(kSsThreads), 0, stream, m, n_q, G, tab);
        else hipLaunchKernelGGL((k_score_stats_rows<false, Cell>), grid, dim3(kSsThreads), 0, stream, m, n_q, G, tab);
        hipLaunchKernelGGL(k_score_stats_finish, dim3((unsigned)((n_q + 255) / 256)), dim3(256), 0, stream, tab, n_q, (ScoreStat*)out);
        return hipGetLastError();
    }
    const size_t threads = vec ? (size_t)G / 4 : (size_t)G;
    const dim3 grid((unsigned)((threads + kSsColThreads - 1) / kSsColThreads));
    if (vec) hipLaunchKernelGGL((k_score_stats_cols<true, Cell>), grid, dim3(kSsColThreads), 0, stream, m, n_q, G, (ScoreStat*)out);
    else hipLaunchKernelGGL((k_score_stats_cols<false, Cell>), grid, dim3(kSsColThreads), 0, stream, m, n_q, G, (ScoreStat*)out);
    return hipGetLastError();
}

hipError_t launch_score_stats(int axis, const float* matrix, int n_q, int G, unsigned long long* tab, void* out, hipStream_t stream)
{
    return score_stats<ScoreCell>(axis, (const uint32_t*)matrix, n_q, G, tab, out, stream);
}

// keys [n_q][S] person cells as launch_subject_keys left them: axis 0 one statistic per query over the persons, axis 1 one per person over the queries
hipError_t launch_subject_stats(int axis, const uint32_t* keys, int n_q, int S, unsigned long long* tab, void* out, hipStream_t stream)
{
    return score_stats<PersonCell>(axis, keys, n_q, S, tab, out, stream);
}

hipError_t launch_normalize_scores(int axis, const float* scores, int n_q, int G, const double* pair, float* out, hipStream_t stream)
{
    if (n_q <= 0 || G <= 0) return hipSuccess;
    if (!scores || !pair || !out || scores == out || (axis != 0 && axis != 1) || ((uintptr_t)pair & 15)) return hipErrorInvalidValue;
    const bool vec = rows_take_16_bytes(G, scores, out);
    const size_t threads = vec ? (size_t)G / 4 : (size_t)G;
    const dim3 grid((unsigned)((threads + kSsThreads - 1) / kSsThreads), grid_clamp((size_t)((n_q + kSsRows - 1) / kSsRows)));
    const uint32_t* const s = (const uint32_t*)scores;
    uint32_t* const o = (uint32_t*)out;
    const double2* const p = (const double2*)pair;
    if (axis == 0 && vec) hipLaunchKernelGGL((k_normalize_scores<0, true>), grid, dim3(kSsThreads), 0, stream, s, n_q, G, p, o);
    else if (axis == 0) hipLaunchKernelGGL((k_normalize_scores<0, false>), grid, dim3(kSsThreads), 0, stream, s, n_q, G, p, o);
    else if (vec) hipLaunchKernelGGL((k_normalize_scores<1, true>), grid, dim3(kSsThreads), 0, stream, s, n_q, G, p, o);
    else hipLaunchKernelGGL((k_normalize_scores<1, false>), grid, dim3(kSsThreads), 0, stream, s, n_q, G, p, o);
    return hipGetLastError();
}

}  // namespace afis
