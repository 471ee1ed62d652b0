// score_hist.h — score distributions of a row of score cells, defined once for the host and the device.  Standard library only (score_order.h is): usable from g++ alone.
// The kernels (score_hist.hip), the host unit (afis_distribution.cpp) and the check program (score_hist_check.cpp) share this text.
//
// A cell (word w) is an ENTRY when rank_key(w) >= kEntryFloor, the key of -inf: what the hit lists count at min_score = -inf and the positions call an entry.  The
// no-entry word 0xffffffff and every other NaN with the sign set lie below it and are counted nowhere.
// THE BIN of an entry under n ascending edge keys is the number of edges e with key(e) <= rank_key(cell): bin 0 holds the entries below the first edge (the -1 of an
// empty template, -inf), bin n the entries that reach the last one (a NaN with the sign clear too); an edge is inclusive from below; the two zeros are one value, for
// cells and for edges, because rank_key adds + 0.0f.  So sum(bins j + 1 ..) is what a hit list counts at min_score = edge j.
// THE ENTRY AT RANK r of a row is the (r + 1)-th greatest composite rank_composite(rank_key, position) of its entries: unique inside a row, so a radix select on the
// composite needs no tie rule.  Its digits are taken from the top, 8 bits at a time; select_step is one digit's decision over the 256 counts of the entries that share
// the digits fixed so far.  The low word of a composite is ~position: the bytes of it above the highest position's are 0xff in every entry and are not counted.
// PERSONS (afis_subject_score_histogram, afis_subject_entries_at): the same three definitions over a row of person cells (score_cell.h: PersonCell) — the cell is the
// high half K of subj_best, its own key, the RAW ordered word; an edge's key is ordered_word(edge).  So -0.0 and +0.0 are two values, for cells and for edges: (-0.0,
// +0.0) is a valid pair of edges, and sum(bins j + 1 ..) is what afis_rank_subject_hits counts at min_score = edge j.  The position of a composite is the slot.
#pragma once
#include <cstdint>

#include "score_cell.h"
#include "score_order.h"

namespace afis {

constexpr uint32_t kEntryFloor = 0x007fffffu;                               // rank_key(-inf) == ordered_word(-inf)
constexpr int kHistEdgesMax = 1023;                                         // AFIS_HIST_EDGES_MAX: 1024 bins
constexpr int64_t kHistCountsMax = (int64_t)1 << 24;                        // AFIS_HIST_COUNTS_MAX: the counts one call returns
constexpr int kSelectBins = 256;                                            // one digit of the select: 8 bits

// edges [n] as keys: 0, or -1 where an edge is a NaN or the keys do not ascend strictly
template <class Cell = ScoreCell>
inline int hist_edge_keys(const float* edges, int n, uint32_t* keys)
{
    for (int j = 0; j < n; ++j) {
        if (edges[j] != edges[j]) return -1;
        keys[j] = Cell::edge_key(edges[j]);
        if (j > 0 && keys[j] <= keys[j - 1]) return -1;
    }
    return 0;
}

// the first step of the search below: the greatest power of two <= n (n >= 1)
AFIS_ORDER_FN int hist_top_step(int n)
{
    int s = 1;
    while (s * 2 <= n) s *= 2;
    return s;
}

// The bin of the cell w under keys [n] (1 <= n <= kHistEdgesMax, ascending), -1 for a cell that is no entry.  A binary search without a branch: at most 10 steps, each
// one load and one select; keys[pos + s - 1] is read only where pos + s <= n.
template <class Cell = ScoreCell>
AFIS_ORDER_FN int hist_bin(const uint32_t* keys, int n, int top_step, uint32_t w)
{
    const uint32_t key = Cell::key(w);
    int pos = 0;
    for (int s = top_step; s >= 1; s >>= 1) {
        const int at = pos + s;
        const uint32_t e = keys[(at <= n ? at : n) - 1];
        pos = (at <= n && e <= key) ? at : pos;
    }
    return key >= kEntryFloor ? pos : -1;
}

// counts [n] walked from the top with the rank *remain: the index whose count holds that rank, *remain reduced to the rank inside it; -1, *remain reduced by every
// count, where the rank is not below their total — the walk goes on in the counts below
AFIS_ORDER_FN int select_walk(const uint64_t* counts, int n, uint64_t* remain)
{
    uint64_t r = *remain;
    int found = -1;
    for (int d = n - 1; d >= 0; --d) {                                      // (no early exit: with a constant n the walk unrolls into selects over registers)
        const uint64_t c = counts[d];
        found = (found < 0 && r < c) ? d : found;
        r = found < 0 ? r - c : r;
    }
    *remain = r;
    return found;
}

// One digit of the select: counts [256] of the entries that share the digits fixed so far, by this digit; *remain the rank among them, counted from the greatest.
// Walks the counts from the top: the digit whose entries hold that rank, *remain reduced to the rank among those; -1, *remain unchanged, where it is not below the total.
// kSelectStepLoads counts are fetched before they are walked: on the device their loads are in flight together (one thread walks one target's counts).
constexpr int kSelectStepLoads = 32;
AFIS_ORDER_FN int select_step(const uint64_t* counts, uint64_t* remain)
{
    uint64_t r = *remain;
    int d = -1;
    for (int blk = kSelectBins / kSelectStepLoads - 1; blk >= 0 && d < 0; --blk) {
        uint64_t c[kSelectStepLoads];
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int k = 0; k < kSelectStepLoads; ++k) c[k] = counts[blk * kSelectStepLoads + k];
        const int at = select_walk(c, kSelectStepLoads, &r);
        if (at >= 0) d = blk * kSelectStepLoads + at;
    }
    if (d >= 0) *remain = r;
    return d;
}

// how many bytes of ~position differ among the positions 0 .. n - 1 (n >= 1): the low-word digits a select over a row of n cells counts (0 .. 4)
AFIS_ORDER_FN int select_position_digits(int64_t n)
{
    int d = 0;
    while (d < 4 && ((int64_t)1 << (8 * d)) < n) ++d;
    return d;
}

}  // namespace afis
