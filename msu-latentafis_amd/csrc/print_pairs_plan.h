// print_pairs_plan.h — the plan of one afis_score_print_pairs / afis_correspondences_print_pairs call (afis_print_pairs.cpp), built on the host alone: nothing here
// knows of a device, so the construction is a program of its own under the host sanitizers (print_pairs_plan_check.cpp, tests/test_print_pairs_host.py; the numpy
// restatement is tests/print_pairs_model.py).
//
// A call is n_pairs pairs (a, b) of GLOBAL indices.  A pair is COVERED when both lie in [base, base + G); it is PLANNED when it is covered and wants something a holds:
// a's minutiae template (want_minu[i] and a has minutiae) or a's texture template (want_tex[i] and a has texture points).  Only planned pairs reach the device; the
// driver settles every other pair from the host's tables.
//   prints     the distinct query prints of the planned pairs (shard-local), in order of first appearance, with what of each is gathered: its minutiae template when
//              one of its pairs wants it, its texture template likewise
//   batches    consecutive runs of `prints`: at most cap_prints prints (cap_prints > 0), or (cap_prints == 0) as many as keep the views' bytes within budget_bytes —
//              392 bytes per gathered minutia and texture point, 6 144 per fragment tile of 16 minutiae — and at least one: a print larger than the budget is a batch
//              of its own.  One batch is one temporary query handle; a print's position in it is its place in the run
//   pairs      every planned pair belongs to the batch of its a: the caller's pair numbers batch after batch, inside a batch in the caller's order, each with the
//              position of its a in the batch's handle
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace afis {

constexpr int64_t kPrintViewPointBytes = 392;            // x, y (4), ori (4), 96 descriptor floats (384): a minutia's and a texture point's
constexpr int64_t kPrintViewTileBytes = 6 * 64 * 16;     // one fragment tile of 16 descriptors
constexpr int64_t kPrintPairsBatchMax = 1 << 20;         // prints of one batch at most, whatever the option and the budget say: positions and table sizes stay far inside int32

struct PrintPairsPlan {
    std::vector<int32_t> prints;       // [n_prints] shard-local
    std::vector<uint8_t> use_minu, use_tex;   // [n_prints] 1 = gathered
    std::vector<size_t> batch_first;   // [n_batches + 1] prints of batch k: batch_first[k] .. batch_first[k + 1] - 1
    std::vector<size_t> pair_first;    // [n_batches + 1] entries of pair / pos that belong to batch k
    std::vector<int64_t> pair;         // [n_planned] the caller's pair numbers
    std::vector<int32_t> pos;          // [n_planned] position of the pair's a in its batch's handle
    std::vector<int32_t> slot;         // scratch: [G] a print's place in `prints`, -1 = not a query print
    std::vector<int32_t> batch_of;     // scratch: [n_prints]
};

inline int64_t print_view_bytes(const int32_t* res_mo, const int32_t* res_to, int32_t t, bool minu, bool tex)
{
    const int64_t nm = minu ? (int64_t)res_mo[t + 1] - res_mo[t] : 0, nt = tex ? (int64_t)res_to[t + 1] - res_to[t] : 0;
    return (nm + nt) * kPrintViewPointBytes + (nm + 15) / 16 * kPrintViewTileBytes;
}

// a_idx, b_idx [n_pairs]; res_mo, res_to [G + 1]; want_minu, want_tex [n_pairs] or NULL (= no pair wants it)
inline void plan_print_pairs(int64_t n_pairs, const int64_t* a_idx, const int64_t* b_idx, int64_t base, int64_t G, const int32_t* res_mo, const int32_t* res_to,
                             const uint8_t* want_minu, const uint8_t* want_tex, int64_t cap_prints, int64_t budget_bytes, PrintPairsPlan& p)
{
    p.prints.clear(); p.use_minu.clear(); p.use_tex.clear(); p.pair.clear(); p.pos.clear(); p.batch_of.clear();
    p.batch_first.assign(1, 0); p.pair_first.assign(1, 0);
    p.slot.assign((size_t)(G > 0 ? G : 0), -1);
    auto covered = [&](int64_t g) { return g >= base && g - base < G; };    // (g - base cannot overflow once g >= base)
    // ---- the distinct query prints in order of first appearance, and what of each some pair wants
    std::vector<int64_t> planned;
    for (int64_t i = 0; i < n_pairs; ++i) {
        if (!covered(a_idx[i]) || !covered(b_idx[i])) continue;
        const size_t t = (size_t)(a_idx[i] - base);
        const bool m = want_minu && want_minu[i] && res_mo[t + 1] > res_mo[t], x = want_tex && want_tex[i] && res_to[t + 1] > res_to[t];
        if (!m && !x) continue;
        if (p.slot[t] < 0) { p.slot[t] = (int32_t)p.prints.size(); p.prints.push_back((int32_t)t); p.use_minu.push_back(0); p.use_tex.push_back(0); }
        p.use_minu[(size_t)p.slot[t]] |= m; p.use_tex[(size_t)p.slot[t]] |= x;
        planned.push_back(i);
    }
    // ---- batches: consecutive prints
    const size_t n_prints = p.prints.size();
    p.batch_of.assign(n_prints, 0);
    const int64_t cap = cap_prints > 0 && cap_prints < kPrintPairsBatchMax ? cap_prints : kPrintPairsBatchMax;
    int64_t held = 0;
    size_t first = 0;
    for (size_t k = 0; k < n_prints; ++k) {
        const int64_t bytes = print_view_bytes(res_mo, res_to, p.prints[k], p.use_minu[k] != 0, p.use_tex[k] != 0);
        const bool full = k > first && ((int64_t)(k - first) >= cap || (cap_prints <= 0 && held + bytes > budget_bytes));
        if (full) { p.batch_first.push_back(k); first = k; held = 0; }
        held += bytes;
        p.batch_of[k] = (int32_t)(p.batch_first.size() - 1);
    }
    if (n_prints > 0) p.batch_first.push_back(n_prints);
    // ---- the pairs of every batch in the caller's order (a counting sort over the batches: stable)
    const size_t n_batches = p.batch_first.size() - 1;
    p.pair_first.assign(n_batches + 1, 0);
    for (int64_t i : planned) ++p.pair_first[(size_t)p.batch_of[(size_t)p.slot[(size_t)(a_idx[i] - base)]] + 1];
    for (size_t k = 0; k < n_batches; ++k) p.pair_first[k + 1] += p.pair_first[k];
    p.pair.assign(planned.size(), 0); p.pos.assign(planned.size(), 0);
    std::vector<size_t> next(p.pair_first.begin(), p.pair_first.end() - 1);
    for (int64_t i : planned) {
        const size_t s = (size_t)p.slot[(size_t)(a_idx[i] - base)], k = (size_t)p.batch_of[s], at = next[k]++;
        p.pair[at] = i; p.pos[at] = (int32_t)(s - p.batch_first[k]);
    }
}

}  // namespace afis
