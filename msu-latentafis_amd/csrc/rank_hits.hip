// rank_hits.hip — device code of the hit lists (afis_hits.cpp: afis_rank_hits, afis_rank_subject_hits): of the score matrix a search left on the device, per query
// every entry whose score reaches a decision score — how many there are, and the `cap` best of them in rank-list order.  One kernel, k_rank_hits, in two
// instantiations by what a row is:
//   templates  the score row itself, [G] floats; the ordered word of an entry is k_topk's (minu.hip): rank_key(score) (score_order.h), ties by ascending position
//   subjects   best[query][0 .. S) as k_subject_best (subject_rank.hip) left it; the ordered word is the composite's high half (ordered_word of the raw score word), ties by
//              ascending slot = ascending subject id; a slot that is still 0 holds no template the search covered and is no entry
// An entry QUALIFIES when its ordered word is >= thr, the ordered word of the decision score.  The lists are sorted by that same word, so the qualifying entries are a
// prefix of k_topk's / k_topk_subjects' list whatever bits the matrix holds.
//
// One 1024-thread workgroup per query (as k_topk), at most 5 passes over the row (and a read-back of the `cap` listed scores) against k_topk's k:
//   1  count     one pass builds a 256-bin LDS histogram of the ordered word's top byte over the qualifying entries; the bins' sum is n_hits
//   2  select    only when n_hits > cap: a most-significant-digit-first radix select — the remaining three bytes, one pass each over the entries that match the digits
//                chosen so far — finds T, the ordered word of the cap-th best entry, n_gt, the entries strictly above it, and n_eq = cap - n_gt >= 1, how many of the
//                entries AT T the list still takes.  With n_hits <= cap everything that qualifies is "above" (T = thr - 1).
//   3  compact   one pass in position order: an entry above T goes to a slot below n_gt, an entry at T to slot n_gt + (its rank among the entries at T) while that rank
//                is < n_eq — ties are cut by ascending position, and with 99 % of a search's scores tied at zero the cut lies inside one huge tie as a rule.  The ranks
//                come from a workgroup-wide exclusive scan: ballot + popcount inside a wave, the wave totals through LDS, a running carry over strips of 4096 positions
//   4  sort      bitonic, descending, of the composites (ordered word << 32 | ~position) in LDS, padded with 0 to a power of two; composites are unique
//   5  write     n_hits and min(n_hits, cap) entries — the score read back from the matrix by position — then the padding (-1, -inf, -1)
// Every loop that holds a barrier runs ceil(n / 4096) trips, or a count read from LDS behind a barrier: the same number in every thread; positions past the end of the
// row contribute nothing.  All counters are 32-bit (a row holds up to INT_MAX entries).  The histograms take LDS atomics; the lanes of a wave that hold the digit of the
// wave's first entry, and then those that hold the digit of the first entry left, are counted by one add of a popcount each — inside the tie at zero that is the whole
// wave, or all of it but a few positive scores — instead of up to 64 adds to one address.  A thread takes four positions 1024 apart per trip, so that four loads are
// in flight.
#include "afis_device.h"

namespace afis {

constexpr int kRhThreads = 1024;
constexpr int kRhWaves = kRhThreads / 64;
constexpr int kRhPer = 4;                                                    // positions per thread and trip
constexpr uint32_t kRhStrip = kRhThreads * kRhPer;
static_assert((kRankHitsMax & (kRankHitsMax - 1)) == 0 && kRankHitsMax * 8 <= 48 * 1024, "the composites are sorted in LDS as a power of two");

struct RhSelect { uint32_t T, n_gt, n_eq, n_hits; };                         // the state of the selection (T: the digits chosen so far, in the end the whole word)

// the ordered word of entry e (32 bits whose unsigned order is the rank lists'), and whether e is an entry at all
template <bool kSubjects>
__device__ __forceinline__ bool rh_word(const float* __restrict__ sc, const u64* __restrict__ best, uint32_t e, uint32_t& w)
{
    if (kSubjects) { const u64 b = best[e]; w = composite_word(b); return b != 0; }
    w = rank_key(sc[e]);                                                     // k_topk's key
    return true;
}

// scores [n_q][G]; best [n_q][S] (subjects); ids [S] (subjects); d_global NULL or the subset's [G] global indices; thr >= 1; 1 <= cap <= kRankHitsMax;
// out_n [n_q], out_a / out_score / out_b [n_q][cap] (templates: out_a = global index, out_b unused; subjects: out_a = subject id, out_b = global index of the best template)
template <bool kSubjects>
__global__ __launch_bounds__(kRhThreads) void k_rank_hits(const float* __restrict__ scores, int G, const u64* __restrict__ best, int S, const long long* __restrict__ ids,
                                                          const long long* __restrict__ d_global, long long index_base, uint32_t thr, int cap,
                                                          long long* __restrict__ out_n, long long* __restrict__ out_a, float* __restrict__ out_score, long long* __restrict__ out_b)
{
    __shared__ u64 s_keys[kRankHitsMax];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[2][kRhPer][kRhWaves];                         // the compaction's wave totals: entries at T | entries above T << 16 (each <= 64)
    __shared__ RhSelect s_sel;
    const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = (uint32_t)(kSubjects ? S : G), ucap = (uint32_t)cap;
    const float* const sc = scores + (size_t)qi * (size_t)G;
    const u64* const brow = kSubjects ? best + (size_t)qi * (size_t)S : nullptr;
    const uint32_t strips = n / kRhStrip + (n % kRhStrip ? 1u : 0u);         // the same in every thread

    if (tid < 256) s_hist[tid] = 0;
    if (tid == 0) s_sel = RhSelect{0u, 0u, ucap, 0u};
    __syncthreads();

    // ---- 1, 2: count, then select while more qualify than the list holds -------------------------------------------------------------------------
    for (int pass = 0; pass < 4; ++pass) {
        const RhSelect sel = s_sel;                                         // behind a barrier: the same in every thread
        if (pass > 0 && sel.n_hits <= ucap) break;
        const int shift = 24 - 8 * pass;
        for (uint32_t st = 0; st < strips; ++st) {
            uint32_t w[kRhPer]; bool act[kRhPer];
#pragma unroll
            for (int j = 0; j < kRhPer; ++j) {
                const uint32_t e = st * kRhStrip + (uint32_t)(j * kRhThreads + tid);
                w[j] = 0;
                act[j] = e < n && rh_word<kSubjects>(sc, brow, e, w[j]) && w[j] >= thr;
            }
#pragma unroll
            for (int j = 0; j < kRhPer; ++j) {
                const bool a = act[j] && (pass == 0 || (w[j] >> (shift + 8)) == sel.T);
                const uint32_t digit = (w[j] >> shift) & 255u;
                u64 rest = __ballot(a);                                     // (wave-uniform) the lanes whose entry is still to be counted
#pragma unroll
                for (int peel = 0; peel < 2 && rest; ++peel) {              // the digit of the first such lane: one add for all lanes that hold it
                    const int first = __ffsll((long long)rest) - 1;
                    const uint32_t d0 = (uint32_t)__shfl((int)digit, first);
                    const u64 same = __ballot(a && digit == d0);
                    if (lane == first) atomicAdd(&s_hist[d0], (uint32_t)__popcll(same));
                    rest &= ~same;
                }
                if ((rest >> lane) & 1) atomicAdd(&s_hist[digit], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {                                                    // lane l takes bins 255 - 4 l .. 252 - 4 l: the scan runs from the best digit down
            uint32_t c[4], mine = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = s_hist[255 - 4 * lane - j]; s_hist[255 - 4 * lane - j] = 0; mine += c[j]; }
            uint32_t inc = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, d); if (lane >= d) inc += o; }
            const uint32_t total = (uint32_t)__shfl((int)inc, 63);
            uint32_t run = inc - mine;                                      // entries in the bins before this lane's
            if (pass == 0 && total <= ucap) {
                if (lane == 0) s_sel = RhSelect{thr - 1u, total, 0u, total};   // everything that qualifies is above thr - 1 (thr >= 1)
            } else if (run < sel.n_eq && inc >= sel.n_eq) {                 // one lane: n_eq >= 1, and the entries counted number at least n_eq
                int j = 0;
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) if (j == jj && run + c[jj] < sel.n_eq) { run += c[jj]; j = jj + 1; }
                s_sel = RhSelect{(sel.T << 8) | (uint32_t)(255 - 4 * lane - j), sel.n_gt + run, sel.n_eq - run, pass == 0 ? total : sel.n_hits};
            }
        }
        __syncthreads();
    }
    const RhSelect sel = s_sel;
    const uint32_t T = sel.T, n_gt = sel.n_gt, n_eq = sel.n_eq;
    const uint32_t count = sel.n_hits < ucap ? sel.n_hits : ucap;           // = n_gt + n_eq when the selection ran
    uint32_t P = 1;
    while (P < count) P <<= 1;

    // ---- 3: ordered compaction -----------------------------------------------------------------------------------------------------------------------
    for (uint32_t i = (uint32_t)tid; i < P; i += kRhThreads) s_keys[i] = 0;  // padding sorts last: every real composite is > 0
    __syncthreads();
    uint32_t carry_eq = 0, carry_gt = 0;
    for (uint32_t st = 0; st < strips; ++st) {
        const int par = (int)(st & 1u);
        uint32_t w[kRhPer], e[kRhPer]; bool gt[kRhPer], eq[kRhPer]; u64 b_eq[kRhPer], b_gt[kRhPer];
#pragma unroll
        for (int j = 0; j < kRhPer; ++j) {
            e[j] = st * kRhStrip + (uint32_t)(j * kRhThreads + tid);
            w[j] = 0;
            const bool q = e[j] < n && rh_word<kSubjects>(sc, brow, e[j], w[j]) && w[j] >= thr;
            gt[j] = q && w[j] > T; eq[j] = q && w[j] == T;
        }
#pragma unroll
        for (int j = 0; j < kRhPer; ++j) {
            b_eq[j] = __ballot(eq[j]); b_gt[j] = __ballot(gt[j]);
            if (lane == 0) s_wave[par][j][wave] = (uint32_t)__popcll(b_eq[j]) | ((uint32_t)__popcll(b_gt[j]) << 16);
        }
        __syncthreads();                                                    // (one barrier per strip: the next strip writes the other parity)
        const u64 below = ((u64)1 << lane) - 1;
        uint32_t before = 0;                                                // packed counts of the strip's positions before this thread's row j
#pragma unroll
        for (int j = 0; j < kRhPer; ++j) {
            uint32_t mine = 0, row = 0;
#pragma unroll
            for (int v = 0; v < kRhWaves; ++v) { const uint32_t x = s_wave[par][j][v]; row += x; if (v < wave) mine += x; }
            const uint32_t pre = before + mine;                             // (sums of at most 64 counts of at most 64: no carry between the halves)
            const uint32_t r_eq = carry_eq + (pre & 0xffffu) + (uint32_t)__popcll(b_eq[j] & below), r_gt = carry_gt + (pre >> 16) + (uint32_t)__popcll(b_gt[j] & below);
            const uint32_t slot = gt[j] ? r_gt : n_gt + r_eq;
            if ((gt[j] || (eq[j] && r_eq < n_eq)) && slot < count) s_keys[slot] = rank_composite(w[j], e[j]);   // (slot < count holds by the counts; it also keeps the store inside s_keys)
            before += row;
        }
        carry_eq += before & 0xffffu; carry_gt += before >> 16;
    }
    __syncthreads();

    // ---- 4: bitonic sort, descending ----------------------------------------------------------------------------------------------------------------
    for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = (uint32_t)tid; i < P / 2; i += kRhThreads) {
                const uint32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const u64 a = s_keys[lo], b = s_keys[hi];
                if ((lo & k2) == 0 ? a < b : a > b) { s_keys[lo] = b; s_keys[hi] = a; }
            }
            __syncthreads();
        }
    }

    // ---- 5: write -----------------------------------------------------------------------------------------------------------------------------------
    if (tid == 0) out_n[qi] = (long long)sel.n_hits;
    for (uint32_t r = (uint32_t)tid; r < ucap; r += kRhThreads) {
        const size_t o = (size_t)qi * (size_t)cap + r;
        const uint32_t e = r < count ? composite_position(s_keys[r]) : n;             // < n: a composite is made from an entry of the row
        if (e < n) {
            if (kSubjects) {
                const uint32_t pos = composite_position(brow[e]);                    // a position of the row: k_subject_best made the composite from one
                if (pos < (uint32_t)G) { out_a[o] = ids[e]; out_score[o] = sc[pos]; out_b[o] = d_global ? d_global[pos] : index_base + (long long)pos; continue; }
            } else { out_a[o] = d_global ? d_global[e] : index_base + (long long)e; out_score[o] = sc[e]; continue; }
        }
        out_a[o] = -1; out_score[o] = -INFINITY;
        if (kSubjects) out_b[o] = -1;
    }
}

hipError_t launch_rank_hits(const float* scores, int n_q, int G, const unsigned long long* best, int S, const long long* ids, const long long* d_global, long long index_base,
                            uint32_t thr, int cap, long long* out_n, long long* out_a, float* out_score, long long* out_b, hipStream_t stream)
{
    if (n_q <= 0) return hipSuccess;
    if (cap < 1 || cap > kRankHitsMax || thr == 0 || G <= 0 || (best && (S <= 0 || !ids || !out_b))) return hipErrorInvalidValue;
    if (best) hipLaunchKernelGGL(k_rank_hits<true>, dim3(n_q), dim3(kRhThreads), 0, stream, scores, G, best, S, ids, d_global, index_base, thr, cap, out_n, out_a, out_score, out_b);
    else hipLaunchKernelGGL(k_rank_hits<false>, dim3(n_q), dim3(kRhThreads), 0, stream, scores, G, best, S, ids, d_global, index_base, thr, cap, out_n, out_a, out_score, out_b);
    return hipGetLastError();
}

}  // namespace afis
