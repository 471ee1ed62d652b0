// subject_rank.hip — device code of the subject rank lists (afis_subjects.cpp: afis_rank_subjects): the score matrix a search left on the device, [n_q][G] over
// TEMPLATES, is grouped by enrolled person — per (query, subject) the best score among the subject's templates and where it was reached — and the k best subjects of
// every query are listed.  Two kernels; the form built is the atomic one: a maximum does not depend on the order its operands arrive in, so
// the result is the same bits on every run, and the subset case needs nothing of its own beyond one more look-up per score.
//
// k_subject_best: one coalesced pass over the matrix, grid = (chunks of kSbThreads positions, query).  A lane holds one score as k_topk's composite
// (ordered score bits << 32 | ~position: the greatest composite is the best score at the lowest position) and the slot of the subject its template belongs to
// (slot_of[position]; for a subset search slot_of[d_global[position] - index_base]).  Before anything leaves the wave, lanes that hold the same slot merge: a
// Hillis-Steele scan over the 64 lanes whose step at distance d takes the other lane's composite only when that lane holds the same slot.  Inside a run of equal
// slots the last lane then holds the run's maximum (induction over d: after the step at distance d a lane of the run holds everything the run has within 2d lanes
// before it); what a lane picks up from an equal slot beyond its own run (labels in A B A order) is that subject's too, and a maximum is idempotent.  Only the last
// lane of every run — the lane whose successor holds another slot, and lane 63 — issues a 64-bit maximum at agent scope into best[query][slot] (zeroed by the
// launcher; every real composite is > 0).  Cards enrolled one after the other, ten templates a person, cost one atomic per card (two at a wave edge); one subject
// that holds half the gallery costs one atomic per wave instead of 64 on one address.
//
// k_topk_subjects: k_topk's scheme (minu.hip) over best[query][0 .. S): one 1024-thread workgroup per query, k rounds of "the largest key below the previous round's";
// the key is (ordered score bits << 32 | ~slot), and the slots are the distinct ids in ascending order, so equal scores go by ascending subject id.  A slot that is
// still 0 belongs to a subject none of whose templates the search covered (a subset search) and is skipped.
//
// The ordered score bits are score_order.h's ordered_word, the raw word's, not k_topk's rank_key: the two agree on every fused score (k_fuse: -1, or a sum of part scores).
#include "afis_device.h"

namespace afis {

constexpr int kSbThreads = 256;          // positions per workgroup of k_subject_best (four waves; the merge never leaves a wave)
constexpr int kStThreads = 1024;         // k_topk_subjects: as k_topk

__device__ __forceinline__ u64 sr_shfl_up(u64 v, int d)
{
    return ((u64)(uint32_t)__shfl_up((int)(v >> 32), d) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, d);
}
__device__ __forceinline__ u64 sr_shfl_xor(u64 v, int d)
{
    return ((u64)(uint32_t)__shfl_xor((int)(v >> 32), d) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, d);
}

// scores [n_q][G]; slot_of [n_slot_of] int32 in [0, S); d_global NULL (full search: the template of position p is p) or [G] global indices with
// 0 <= d_global[p] - index_base < n_slot_of (a subset's positions); best [n_q][S], zeroed
__global__ __launch_bounds__(kSbThreads) void k_subject_best(const float* __restrict__ scores, int G, const int32_t* __restrict__ slot_of, const long long* __restrict__ d_global,
                                                             long long index_base, int S, u64* __restrict__ best)
{
    const int p = blockIdx.x * kSbThreads + threadIdx.x, lane = threadIdx.x & 63;
    const size_t qi = blockIdx.y;
    int slot = -1;                                                          // lanes past the end of the row: a run of their own that issues nothing
    u64 c = 0;
    if (p < G) {
        c = rank_composite(ordered_word(scores[qi * (size_t)G + p]), (uint32_t)p);
        slot = slot_of[d_global ? (int)(d_global[p] - index_base) : p];
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 oc = sr_shfl_up(c, d);
        const int os = __shfl_up(slot, d);
        if (lane >= d && os == slot && oc > c) c = oc;
    }
    const int next = __shfl_down(slot, 1);
    if (slot >= 0 && (lane == 63 || next != slot))
        (void)__hip_atomic_fetch_max(best + qi * (size_t)S + slot, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// best [n_q][S] as k_subject_best left it; ids [S] the subjects' ids in ascending order; out_* [n_q][k]
__global__ __launch_bounds__(kStThreads) void k_topk_subjects(const u64* __restrict__ best, int S, const long long* __restrict__ ids, const float* __restrict__ scores, int G,
                                                              const long long* __restrict__ d_global, long long index_base, int k,
                                                              long long* __restrict__ out_id, float* __restrict__ out_score, long long* __restrict__ out_best)
{
    __shared__ u64 s_part[kStThreads / 64];
    __shared__ u64 s_best;
    const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64* const row = best + (size_t)qi * S;
    u64 prev = ~0ull;
    for (int r = 0; r < k; ++r) {
        u64 top = 0;
        for (int e = tid; e < S; e += kStThreads) {
            const u64 b = row[e];
            const u64 key = composite_at(b, (uint32_t)e);
            if (b != 0 && key < prev && key > top) top = key;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = sr_shfl_xor(top, off);
            top = o > top ? o : top;
        }
        if (lane == 0) s_part[wave] = top;
        __syncthreads();
        if (tid == 0) {
            u64 b = 0;
#pragma unroll
            for (int w = 0; w < kStThreads / 64; ++w) b = s_part[w] > b ? s_part[w] : b;
            s_best = b;
            const size_t o = (size_t)qi * k + r;
            if (b) {
                const uint32_t slot = composite_position(b);                 // < S: a key is made from a slot of the row
                const uint32_t pos = composite_position(row[slot]);          // < G: a composite is made from a position of the row
                out_id[o] = ids[slot];
                out_score[o] = scores[(size_t)qi * G + pos];
                out_best[o] = d_global ? d_global[pos] : index_base + (long long)pos;
            } else { out_id[o] = -1; out_score[o] = -INFINITY; out_best[o] = -1; }   // k exceeds the subjects present
        }
        __syncthreads();
        prev = s_best;                                                     // 0 once the subjects are exhausted: nothing is below it
    }
}

hipError_t launch_subject_best(const float* scores, int n_q, int G, const int32_t* slot_of, const long long* d_global, long long index_base, int S,
                               unsigned long long* best, hipStream_t stream)
{
    if (n_q <= 0 || S <= 0) return hipSuccess;
    if (n_q > 65535) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(best, 0, (size_t)n_q * (size_t)S * 8, stream);
    if (e != hipSuccess || G <= 0) return e;
    hipLaunchKernelGGL(k_subject_best, dim3((unsigned)((G + kSbThreads - 1) / kSbThreads), (unsigned)n_q), dim3(kSbThreads), 0, stream, scores, G, slot_of, d_global, index_base, S, best);
    return hipGetLastError();
}

hipError_t launch_topk_subjects(const unsigned long long* best, int n_q, int S, const long long* ids, const float* scores, int G, const long long* d_global, long long index_base,
                                int k, long long* out_id, float* out_score, long long* out_best, hipStream_t stream)
{
    if (n_q <= 0 || k <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_topk_subjects, dim3(n_q), dim3(kStThreads), 0, stream, best, S, ids, scores, G, d_global, index_base, k, out_id, out_score, out_best);
    return hipGetLastError();
}

}  // namespace afis
