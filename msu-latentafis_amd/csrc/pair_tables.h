// pair_tables.h — the tables one chunk of a pair-list call goes to the device with (afis_pairs.cpp: PairCall), built on the host alone: nothing here knows of a device, so the
// construction is a program of its own under the host sanitizers (pair_tables_check.cpp, tests/test_score_pairs_host.py).
//
// A chunk is m pairs (position of the latent in the query handle, shard-local template).  The handle's queries lie in launch groups — contiguous runs, group g holding the
// queries q_first[g] .. q_first[g + 1] - 1 — and every kernel of the pair call is launched per group.  So the chunk's pairs are sorted (one counting sort over the queries,
// stable: the pairs of one latent keep the caller's order) by launch group and, inside a group, by latent; a pair's SLOT is its place in that order.
//   tab   group g's pair table [count | (query of the group, template) x count] starts at tab + 2 first[g] + g: what launch_minu_cands_pairs, launch_graph_minutiae_pairs,
//         launch_adc_pairs, launch_graph_texture_pairs and launch_fuse_pairs read, pair p of the group at slot first[g] + p              (2 m + n_grp ints)
//   seg   the work list of k_adc_pairs (adc_pairs.hip): every latent's run of pairs cut into segments of at most kAdcPairsSegment pairs, (first pair of the segment IN THE
//         GROUP'S TABLE, pairs) each; group g's segments are seg + 2 seg_first[g] .., seg_first[g + 1] - seg_first[g] of them          (at most 2 m ints)
//   slot_of[slot] = the chunk's pair that sits there: the way back into the caller's order
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace afis {

constexpr int kAdcPairsSegment = 64;   // S: pairs of one latent a workgroup of k_adc_pairs streams through one LUT tile at most (a latent with 4096 candidates: 64 workgroups per tile)

struct PairChunkTables {
    std::vector<size_t> first;         // [n_grp + 1] slots of group g: first[g] .. first[g + 1] - 1
    std::vector<size_t> seg_first;     // [n_grp + 1] segments of group g
    std::vector<int32_t> slot_of;      // [m]
    std::vector<size_t> run;           // scratch: [n_q + 1] the counting sort's bins
};

// query [m] in [0, n_q), tmpl [m]; q_first [n_grp + 1] ascending from 0 to n_q; tab [2 m + n_grp], seg [2 m].  Returns the number of segments.
// seg == NULL (afis_correspondences_pairs: no ADC kernel runs): no work list is written, seg_first is all zeros, 0 segments.
inline size_t build_pair_tables(size_t m, const int32_t* query, const int32_t* tmpl, size_t n_grp, const int32_t* q_first, int seg_pairs, int32_t* tab, int32_t* seg, PairChunkTables& t)
{
    const size_t n_q = n_grp ? (size_t)q_first[n_grp] : 0, S = seg_pairs > 0 ? (size_t)seg_pairs : 1;
    t.run.assign(n_q + 1, 0);
    for (size_t k = 0; k < m; ++k) ++t.run[(size_t)query[k] + 1];
    for (size_t q = 0; q < n_q; ++q) t.run[q + 1] += t.run[q];                                   // run[q] = first slot of latent q
    t.first.assign(n_grp + 1, 0); t.seg_first.assign(n_grp + 1, 0); t.slot_of.assign(m, 0);
    for (size_t g = 0; g <= n_grp; ++g) t.first[g] = n_grp ? t.run[(size_t)q_first[g]] : 0;
    size_t n_seg = 0;
    for (size_t g = 0; g < n_grp; ++g) {
        t.seg_first[g] = n_seg;
        tab[2 * t.first[g] + g] = (int32_t)(t.first[g + 1] - t.first[g]);
        for (size_t q = (size_t)q_first[g]; seg && q < (size_t)q_first[g + 1]; ++q)
            for (size_t s = t.run[q]; s < t.run[q + 1]; s += S) {
                seg[2 * n_seg] = (int32_t)(s - t.first[g]);
                seg[2 * n_seg + 1] = (int32_t)(t.run[q + 1] - s < S ? t.run[q + 1] - s : S);
                ++n_seg;
            }
    }
    t.seg_first[n_grp] = n_seg;
    // the pairs into their slots: run[q] walks latent q's run (it ends as the next latent's start)
    for (size_t k = 0; k < m; ++k) {
        const size_t q = (size_t)query[k], slot = t.run[q]++;
        size_t g = 0;
        { size_t lo = 0, hi = n_grp; while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if ((size_t)q_first[mid] <= q) lo = mid; else hi = mid; } g = lo; }
        t.slot_of[slot] = (int32_t)k;
        tab[2 * slot + g + 1] = (int32_t)(q - (size_t)q_first[g]); tab[2 * slot + g + 2] = tmpl[k];
    }
    return n_seg;
}

}  // namespace afis
