// rank_order.h — the order of a rank list, stated once for every host path that makes or merges one.  Standard library only: usable from g++ alone.
//
// A template rank list is sorted on rank_key(score) (score_order.h), descending; equal keys go by ascending GLOBAL index: the order of k_topk (afis_search*, k <= 64)
// and rank_hits.hip (afis_rank_hits, afis_rank_latent_hits), so every path lists the same entries whatever bits the scores hold — a NaN stands where its bits put it
// instead of breaking the strict weak order a float comparison needs.  On NaN-free scores key order IS float order (a > b  <=>  rank_key(a) > rank_key(b)).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "score_order.h"

namespace afis {

// "entry a stands before entry b" of a rank list: a strict total order while no global index repeats
inline bool rank_before(float score_a, int64_t idx_a, float score_b, int64_t idx_b)
{
    const uint32_t ka = rank_key(score_a), kb = rank_key(score_b);
    return ka > kb || (ka == kb && idx_a < idx_b);
}

// The k best of sc[0 .. n) in rank-list order: out_idx[r] = the global index of entry r — col[position] with a column-to-global-index table (a subset's
// columns in the caller's order), index_base + position without one — and out_score[r] its score, own bits; (-1, -inf) pads where k > n.
inline void rank_topk(const float* sc, int64_t n, int k, const int64_t* col, int64_t index_base, int64_t* out_idx, float* out_score)
{
    std::vector<uint32_t> key((size_t)n);
    for (int64_t i = 0; i < n; ++i) key[(size_t)i] = rank_key(sc[i]);
    std::vector<int32_t> ind((size_t)n);
    std::iota(ind.begin(), ind.end(), 0);
    const int kk = (int)std::min<int64_t>(k, n);
    const uint32_t* const ky = key.data();
    if (col) std::partial_sort(ind.begin(), ind.begin() + kk, ind.end(), [ky, col](int32_t a, int32_t b) { return ky[a] > ky[b] || (ky[a] == ky[b] && col[a] < col[b]); });
    else std::partial_sort(ind.begin(), ind.begin() + kk, ind.end(), [ky](int32_t a, int32_t b) { return ky[a] > ky[b] || (ky[a] == ky[b] && a < b); });
    for (int r = 0; r < k; ++r) {
        if (r < kk) { out_idx[r] = col ? col[ind[(size_t)r]] : index_base + ind[(size_t)r]; out_score[r] = sc[ind[(size_t)r]]; }
        else { out_idx[r] = -1; out_score[r] = -INFINITY; }
    }
}

// The host statement of afis_count_before (include/afis_matcher.h), and so of a rank position: how many ENTRIES of sc[0 .. n) stand before a hypothetical entry
// (score, idx) by rank_before.  Column i is template col[i], or index_base + i without a table; an entry is a column whose rank_key reaches rank_key(-inf) — the
// no-entry word of the filtered lists and every other NaN with the sign set are none — and a column whose global index is idx is the target itself, never counted.
// The position of a listed template is count_before(sc, n, col, index_base, its own score, its own index).
inline int64_t count_before(const float* sc, int64_t n, const int64_t* col, int64_t index_base, float score, int64_t idx)
{
    const uint32_t floor = rank_key(-INFINITY);
    int64_t before = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t g = col ? col[i] : index_base + i;
        if (g != idx && rank_key(sc[i]) >= floor && rank_before(sc[i], g, score, idx)) ++before;
    }
    return before;
}

// All of 0 .. n-1 in the order of afis_rank_list (include/afis_matcher.h).  ref_order 0: key descending, equal keys by ascending index.  ref_order 1:
// std::sort of the indices on rank_key(a) > rank_key(b) — the reference's statement (matcher.cpp:306-308: std::sort on scores[a] > scores[b]) with the
// comparison made on the key: the same outcome for every pair of a NaN-free column, hence the same permutation from the same libstdc++, and a strict weak
// order (defined behaviour) for every column.
inline void rank_list_order(const float* scores, int64_t n, bool ref_order, std::vector<int>& ind)
{
    std::vector<uint32_t> key((size_t)n);
    for (int64_t i = 0; i < n; ++i) key[(size_t)i] = rank_key(scores[i]);
    ind.resize((size_t)n);
    std::iota(ind.begin(), ind.end(), 0);
    const uint32_t* const ky = key.data();
    auto by_key = [ky](const int& a, const int& b) { return ky[a] > ky[b]; };
    if (ref_order) std::sort(ind.begin(), ind.end(), by_key);
    else std::stable_sort(ind.begin(), ind.end(), by_key);
}

}  // namespace afis
