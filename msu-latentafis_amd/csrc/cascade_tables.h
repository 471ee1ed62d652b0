// cascade_tables.h — the STRUCTURE of the second stage of afis_search_cascade (afis_cascade.cpp), built on the host alone before anything runs: nothing here knows of a
// device, so the construction is a program of its own under the host sanitizers (cascade_tables_check.cpp, tests/test_cascade_host.py).
//
// Which prints a latent keeps is decided on the device; HOW MANY is known beforehand: every query that has pairs (has[q] != 0: the reference scores it; a latent-empty
// query has none, its kept cells are the -1) keeps exactly n_kept prints, in rank order.  So the pairs of the whole call stand in one order — query after query, rank after
// rank — and a pair's SLOT is q_slot[q] + rank.  The handle's queries lie in launch groups (group g: queries q_first[g] .. q_first[g + 1] - 1), every pair kernel is
// launched per group, and the slots are cut into CHUNKS of per_launch slots (the dense texture row maxima of one chunk are what the call holds at a time).  A PIECE is
// the part of one group's slots that lies in one chunk: pieces follow one another in slot order, piece i covering piece_first[i] .. piece_first[i + 1] - 1.
//   tab   (device; 2 total + n_pieces ints) piece i's pair table [count | (query of the group, shard-local template) x count] starts at tab + 2 piece_first[i] + i: what
//         launch_adc_pairs, launch_graph_texture_pairs and launch_fuse_pairs read, pair p of the piece at slot piece_first[i] + p.  k_cascade_gather (cascade.hip) fills it.
//   seg   the work list of k_adc_pairs (adc_pairs.hip): every latent's run of pairs INSIDE a piece cut into segments of at most seg_pairs pairs, (first pair of the
//         segment in the piece's table, pairs) each; piece i's segments are seg + 2 seg_first[i] .., seg_first[i + 1] - seg_first[i] of them
//   dev   what goes to the device, once: q_slot [n_q + 1] | piece_first [n_pieces + 1] | piece_q0 [n_pieces] (the first query of the piece's group) | seg [2 n_seg]
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace afis {

struct CascadePiece { size_t first, n; size_t group, chunk; size_t seg_first, n_seg; };

struct CascadeTables {
    size_t total = 0;                    // pairs of the call
    std::vector<size_t> q_slot;          // [n_q + 1] first slot of query q (a query without pairs: an empty range)
    std::vector<CascadePiece> pieces;    // in slot order
    std::vector<int32_t> seg;            // [2 n_seg]
    std::vector<int32_t> dev;            // the device's copy (above)
    size_t q_slot_at = 0, piece_first_at = 0, piece_q0_at = 0, seg_at = 0;   // int positions in dev
    size_t tab_ints() const { return 2 * total + pieces.size(); }
};

// has [n_q] (1 = the query has pairs), q_first [n_grp + 1] ascending from 0 to n_q, n_kept >= 0, seg_pairs >= 1, per_launch >= 1.
// false (nothing usable in t): the pairs and their tables do not fit 32-bit positions.
inline bool build_cascade_tables(size_t n_q, const uint8_t* has, size_t n_kept, size_t n_grp, const int32_t* q_first, size_t seg_pairs, size_t per_launch, CascadeTables& t)
{
    const size_t S = seg_pairs ? seg_pairs : 1, P = per_launch ? per_launch : 1;
    t = CascadeTables();
    t.q_slot.assign(n_q + 1, 0);
    for (size_t q = 0; q < n_q; ++q) t.q_slot[q + 1] = t.q_slot[q] + (has[q] ? n_kept : 0);
    t.total = t.q_slot[n_q];
    // 2 total + pieces ints of table, pieces <= groups + chunks
    if (n_kept > 0x7fffffffu || t.total > (size_t)0x3ffffff0u - n_grp - n_q) return false;
    for (size_t g = 0; g < n_grp; ++g) {
        const size_t g0 = t.q_slot[(size_t)q_first[g]], g1 = t.q_slot[(size_t)q_first[g + 1]];
        size_t q = (size_t)q_first[g];
        for (size_t a = g0; a < g1;) {
            const size_t chunk = a / P, b = (chunk + 1) * P < g1 ? (chunk + 1) * P : g1;
            CascadePiece pc{a, b - a, g, chunk, t.seg.size() / 2, 0};
            // the runs of the group's queries inside [a, b)
            while (t.q_slot[q + 1] <= a) ++q;
            for (size_t r = q; r < (size_t)q_first[g + 1] && t.q_slot[r] < b; ++r) {
                const size_t lo = t.q_slot[r] > a ? t.q_slot[r] : a, hi = t.q_slot[r + 1] < b ? t.q_slot[r + 1] : b;
                for (size_t s = lo; s < hi; s += S) {
                    t.seg.push_back((int32_t)(s - a));
                    t.seg.push_back((int32_t)(hi - s < S ? hi - s : S));
                }
            }
            pc.n_seg = t.seg.size() / 2 - pc.seg_first;
            t.pieces.push_back(pc);
            a = b;
        }
    }
    const size_t n_p = t.pieces.size();
    t.q_slot_at = 0; t.piece_first_at = n_q + 1; t.piece_q0_at = t.piece_first_at + n_p + 1; t.seg_at = t.piece_q0_at + n_p;
    t.dev.assign(t.seg_at + t.seg.size(), 0);
    for (size_t q = 0; q <= n_q; ++q) t.dev[t.q_slot_at + q] = (int32_t)t.q_slot[q];
    for (size_t i = 0; i < n_p; ++i) {
        t.dev[t.piece_first_at + i] = (int32_t)t.pieces[i].first;
        t.dev[t.piece_q0_at + i] = q_first[t.pieces[i].group];
    }
    t.dev[t.piece_first_at + n_p] = (int32_t)t.total;
    for (size_t i = 0; i < t.seg.size(); ++i) t.dev[t.seg_at + i] = t.seg[i];
    return true;
}

}  // namespace afis
