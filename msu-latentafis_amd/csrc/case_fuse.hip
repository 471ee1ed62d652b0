// case_fuse.hip — device code of the case lists (afis_cases.cpp: afis_rank_case_hits, afis_rank_case_subject_hits and their _filtered forms): the queries of one search that belong to one
// CASE — two encodings of an impression, several lifts of a finger, several fingers of a hand — are fused into one row, and k_rank_hits (rank_hits.hip) ranks the fused
// rows as it ranks a search's.  The host hands the cases over as a CSR: case_off[n_cases + 1] into member[n_q], the query positions of a case in ascending order.
//
// The fused value of (case, column) over the case's members m, v_m the member's value in that column:
//   a member TAKES PART when rank_key(v_m) >= rank_key(+0.0f) (score_order.h), i.e. when the sign bit of v_m + 0.0f is clear: the -1 of an empty entry or of a
//   latent-empty query, every negative value and a NaN with the sign set stay out; -0.0 is the zero it equals
//   kCaseSum  acc = +0.0f; for the members in ascending position: if the member takes part, acc = acc + v_m — one fp32 add each, in that order (the translation units
//             are built with -ffp-contract=off, and nothing here lets the compiler reassociate); -1.0f when no member takes part
//   kCaseMax  the v_m of greatest rank_key, with the bits of the first member that holds it; -1 loses by itself
//
// k_case_fuse: scores[n_q][G] -> fused[n_cases][G].  Grid = (column chunks, cases); a thread owns one column — or, where every row starts on a 16-byte boundary
// (G % 4 == 0), four adjacent ones that travel as one float4 — and walks the member rows of its case in CSR order: every load of a wave is one contiguous run of a
// row, the order of the adds is the order of the loop, and there is no atomic and no sum across lanes.  The member loop carries no dependence between its loads, so
// the unrolled loop has four rows in flight.  An odd G leaves rows unaligned: those matrices take the one-column form.
// k_case_fuse_subjects: the same over best[n_q][S], the composites k_subject_best (subject_rank.hip) made (ordered score word << 32 | ~position; 0 = none of the
// subject's templates was covered): the ordered word is turned back into the score's own bits and folded as above into a float row [n_cases][S].  A subject that was
// not covered — the same slots for every query of a search — gets kNoEntryWord (score_order.h), which k_rank_hits neither counts nor lists (include/afis_matcher.h
// states that property of the key).
// The ELIGIBLE forms (kElig; afis_rank_case_hits_filtered, afis_rank_case_subject_hits_filtered) fold a copy of the matrix from which hit_filter.hip took the cells a
// member is not eligible for, and know the state the plain forms lack — no eligible member: a member whose cell is kNoEntryWord (templates), or whose composite has a
// zero score word (subjects: k_subject_best's composite of a person's all-ineligible cells keeps a non-zero low half, a dropped or uncovered person is a plain 0), is
// not folded, and a column none of whose members was folded gets kNoEntryWord.  A column whose folded members all hold -1 is still kCaseSum's -1.0f: an entry.
// Every index into the matrices is a size_t: n_q x G may pass 2^31.  A grid's second dimension holds 65 535 blocks; more cases than that are walked in a loop.
#include "afis_device.h"

namespace afis {

constexpr int kCfThreads = 256;

struct CfAcc { float v; uint32_t key; bool any; };

__device__ __forceinline__ void cf_start(CfAcc& a) { a.v = 0.0f; a.key = 0; a.any = false; }

// one member's value into the accumulator of its column
template <int kMode>
__device__ __forceinline__ void cf_fold(CfAcc& a, float v)
{
    if (kMode == kCaseSum) {
        if (reaches_zero(v)) { a.v = a.v + v; a.any = true; }               // the member takes part
    } else {
        const uint32_t key = rank_key(v);
        if (!a.any || key > a.key) { a.v = v; a.key = key; a.any = true; }   // strictly greater: the first member of the greatest key keeps its bits
    }
}

template <int kMode>
__device__ __forceinline__ float cf_result(const CfAcc& a) { return (kMode == kCaseSum && !a.any) ? -1.0f : a.v; }

// the eligible forms: a cell the filter took out is not a member's value; seen = some member of the column was folded.  Selects, no branch: the loads of the
// unrolled member loop stay in flight together
template <int kMode>
__device__ __forceinline__ void cf_fold_eligible(CfAcc& a, bool& seen, float v)
{
    const bool there = __float_as_uint(v) != kNoEntryWord;
    seen = seen || there;
    if (kMode == kCaseSum) {
        const bool part = there && reaches_zero(v);                         // the member takes part
        a.v = part ? a.v + v : a.v; a.any = a.any || part;
    } else {
        const uint32_t key = rank_key(v);
        const bool take = there && (!a.any || key > a.key);                 // strictly greater: the first member of the greatest key keeps its bits
        a.v = take ? v : a.v; a.key = take ? key : a.key; a.any = a.any || take;
    }
}

template <int kMode>
__device__ __forceinline__ float cf_result_eligible(const CfAcc& a, bool seen) { return seen ? cf_result<kMode>(a) : __uint_as_float(kNoEntryWord); }

// scores [n_q][G]; case_off [n_cases + 1], member [case_off[n_cases]] query positions < n_q; fused [n_cases][G].  kVec: G % 4 == 0 and both matrices 16-byte aligned.
// kElig: scores is the filtered copy
template <int kMode, bool kVec, bool kElig = false>
__global__ __launch_bounds__(kCfThreads) void k_case_fuse(const float* __restrict__ scores, int G, const int32_t* __restrict__ case_off, const int32_t* __restrict__ member,
                                                          int n_cases, float* __restrict__ fused)
{
    constexpr int kCols = kVec ? 4 : 1;
    const size_t col = ((size_t)blockIdx.x * kCfThreads + threadIdx.x) * kCols;
    if (col >= (size_t)G) return;                                           // (kVec: G % 4 == 0, so col + 3 < G too)
    for (int c = (int)blockIdx.y; c < n_cases; c += (int)gridDim.y) {
        const int m0 = case_off[c], m1 = case_off[c + 1];
        CfAcc acc[kCols];
        bool seen[kCols];                                                   // (kElig only)
#pragma unroll
        for (int j = 0; j < kCols; ++j) { cf_start(acc[j]); seen[j] = false; }
#pragma unroll 4
        for (int m = m0; m < m1; ++m) {
            const float* const row = scores + (size_t)member[m] * (size_t)G + col;
            if constexpr (kVec) {
                const float4 v = *reinterpret_cast<const float4*>(row);
                if constexpr (kElig) { cf_fold_eligible<kMode>(acc[0], seen[0], v.x); cf_fold_eligible<kMode>(acc[1], seen[1], v.y); cf_fold_eligible<kMode>(acc[2], seen[2], v.z); cf_fold_eligible<kMode>(acc[3], seen[3], v.w); }
                else { cf_fold<kMode>(acc[0], v.x); cf_fold<kMode>(acc[1], v.y); cf_fold<kMode>(acc[2], v.z); cf_fold<kMode>(acc[3], v.w); }
            } else if constexpr (kElig) cf_fold_eligible<kMode>(acc[0], seen[0], row[0]);
            else cf_fold<kMode>(acc[0], row[0]);
        }
        float* const dst = fused + (size_t)c * (size_t)G + col;
        if constexpr (kVec && kElig) *reinterpret_cast<float4*>(dst) = make_float4(cf_result_eligible<kMode>(acc[0], seen[0]), cf_result_eligible<kMode>(acc[1], seen[1]), cf_result_eligible<kMode>(acc[2], seen[2]), cf_result_eligible<kMode>(acc[3], seen[3]));
        else if constexpr (kVec) *reinterpret_cast<float4*>(dst) = make_float4(cf_result<kMode>(acc[0]), cf_result<kMode>(acc[1]), cf_result<kMode>(acc[2]), cf_result<kMode>(acc[3]));
        else if constexpr (kElig) dst[0] = cf_result_eligible<kMode>(acc[0], seen[0]);
        else dst[0] = cf_result<kMode>(acc[0]);
    }
}

// best [n_q][S] as k_subject_best left it; fused [n_cases][S].  kElig: best was made from the filtered copy, and the excluded persons were dropped from it
template <int kMode, bool kElig = false>
__global__ __launch_bounds__(kCfThreads) void k_case_fuse_subjects(const u64* __restrict__ best, int S, const int32_t* __restrict__ case_off, const int32_t* __restrict__ member,
                                                                   int n_cases, float* __restrict__ fused)
{
    const size_t col = (size_t)blockIdx.x * kCfThreads + threadIdx.x;
    if (col >= (size_t)S) return;
    for (int c = (int)blockIdx.y; c < n_cases; c += (int)gridDim.y) {
        const int m0 = case_off[c], m1 = case_off[c + 1];
        CfAcc acc;
        cf_start(acc);
        bool covered = true, seen = false;                                  // (seen: kElig only)
#pragma unroll 4
        for (int m = m0; m < m1; ++m) {
            const u64 b = best[(size_t)member[m] * (size_t)S + col];
            if constexpr (kElig) {                                          // (a zero score word is the filter's 0xffffffff turned back; not b != 0: see the head of the file)
                cf_fold_eligible<kMode>(acc, seen, __uint_as_float(score_bits_of(composite_word(b))));
            } else {
                covered = covered && b != 0;
                cf_fold<kMode>(acc, __uint_as_float(score_bits_of(composite_word(b))));
            }
        }
        if constexpr (kElig) fused[(size_t)c * (size_t)S + col] = cf_result_eligible<kMode>(acc, seen);
        else fused[(size_t)c * (size_t)S + col] = covered ? cf_result<kMode>(acc) : __uint_as_float(kNoEntryWord);
    }
}

static inline dim3 cf_grid(size_t threads, int n_cases) { return dim3((unsigned)((threads + kCfThreads - 1) / kCfThreads), grid_clamp((size_t)n_cases)); }

hipError_t launch_case_fuse(const float* scores, int G, const int32_t* case_off, const int32_t* member, int n_cases, int mode, float* fused, hipStream_t stream)
{
    if (n_cases <= 0 || G <= 0) return hipSuccess;
    if (!scores || !case_off || !member || !fused || (mode != kCaseSum && mode != kCaseMax)) return hipErrorInvalidValue;
    const bool vec = rows_take_16_bytes(G, scores, fused);
    const dim3 grid = cf_grid(vec ? (size_t)G / 4 : (size_t)G, n_cases);
    if (mode == kCaseSum) {
        if (vec) hipLaunchKernelGGL((k_case_fuse<kCaseSum, true>), grid, dim3(kCfThreads), 0, stream, scores, G, case_off, member, n_cases, fused);
        else hipLaunchKernelGGL((k_case_fuse<kCaseSum, false>), grid, dim3(kCfThreads), 0, stream, scores, G, case_off, member, n_cases, fused);
    } else {
        if (vec) hipLaunchKernelGGL((k_case_fuse<kCaseMax, true>), grid, dim3(kCfThreads), 0, stream, scores, G, case_off, member, n_cases, fused);
        else hipLaunchKernelGGL((k_case_fuse<kCaseMax, false>), grid, dim3(kCfThreads), 0, stream, scores, G, case_off, member, n_cases, fused);
    }
    return hipGetLastError();
}

hipError_t launch_case_fuse_subjects(const unsigned long long* best, int S, const int32_t* case_off, const int32_t* member, int n_cases, int mode, float* fused, hipStream_t stream)
{
    if (n_cases <= 0 || S <= 0) return hipSuccess;
    if (!best || !case_off || !member || !fused || (mode != kCaseSum && mode != kCaseMax)) return hipErrorInvalidValue;
    const dim3 grid = cf_grid((size_t)S, n_cases);
    if (mode == kCaseSum) hipLaunchKernelGGL(k_case_fuse_subjects<kCaseSum>, grid, dim3(kCfThreads), 0, stream, best, S, case_off, member, n_cases, fused);
    else hipLaunchKernelGGL(k_case_fuse_subjects<kCaseMax>, grid, dim3(kCfThreads), 0, stream, best, S, case_off, member, n_cases, fused);
    return hipGetLastError();
}

hipError_t launch_case_fuse_eligible(const float* filtered, int G, const int32_t* case_off, const int32_t* member, int n_cases, int mode, float* fused, hipStream_t stream)
{
    if (n_cases <= 0 || G <= 0) return hipSuccess;
    if (!filtered || !case_off || !member || !fused || (mode != kCaseSum && mode != kCaseMax)) return hipErrorInvalidValue;
    const bool vec = rows_take_16_bytes(G, filtered, fused);
    const dim3 grid = cf_grid(vec ? (size_t)G / 4 : (size_t)G, n_cases);
    if (mode == kCaseSum) {
        if (vec) hipLaunchKernelGGL((k_case_fuse<kCaseSum, true, true>), grid, dim3(kCfThreads), 0, stream, filtered, G, case_off, member, n_cases, fused);
        else hipLaunchKernelGGL((k_case_fuse<kCaseSum, false, true>), grid, dim3(kCfThreads), 0, stream, filtered, G, case_off, member, n_cases, fused);
    } else {
        if (vec) hipLaunchKernelGGL((k_case_fuse<kCaseMax, true, true>), grid, dim3(kCfThreads), 0, stream, filtered, G, case_off, member, n_cases, fused);
        else hipLaunchKernelGGL((k_case_fuse<kCaseMax, false, true>), grid, dim3(kCfThreads), 0, stream, filtered, G, case_off, member, n_cases, fused);
    }
    return hipGetLastError();
}

hipError_t launch_case_fuse_subjects_eligible(const unsigned long long* best, int S, const int32_t* case_off, const int32_t* member, int n_cases, int mode, float* fused, hipStream_t stream)
{
    if (n_cases <= 0 || S <= 0) return hipSuccess;
    if (!best || !case_off || !member || !fused || (mode != kCaseSum && mode != kCaseMax)) return hipErrorInvalidValue;
    const dim3 grid = cf_grid((size_t)S, n_cases);
    if (mode == kCaseSum) hipLaunchKernelGGL((k_case_fuse_subjects<kCaseSum, true>), grid, dim3(kCfThreads), 0, stream, best, S, case_off, member, n_cases, fused);
    else hipLaunchKernelGGL((k_case_fuse_subjects<kCaseMax, true>), grid, dim3(kCfThreads), 0, stream, best, S, case_off, member, n_cases, fused);
    return hipGetLastError();
}

}  // namespace afis
