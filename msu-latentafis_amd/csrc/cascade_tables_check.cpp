// cascade_tables_check.cpp — cascade_tables.h, the host's structure of afis_search_cascade's second stage, as a program of its own: built with the host sanitizers
// (Makefile: -fsanitize=address,undefined) and run directly by tests/test_cascade_host.py.  Every case is checked against what the structure must be, stated without
// the builder's loops: the slots are the queries' runs in order; the pieces tile the slots, each inside one launch group and one chunk; the segments tile every
// latent's run inside a piece and never mix latents; and a host replay of k_cascade_gather's writes fills every int of the pair tables exactly once, inside them.
#include "cascade_tables.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <string>

using namespace afis;

static int g_cases = 0;

static bool check(const std::string& name, const std::vector<uint8_t>& has, size_t n_kept, const std::vector<int32_t>& q_first, size_t S, size_t P)
{
    ++g_cases;
    auto bad = [&](const char* what) { printf("cascade_tables_check: %s: %s\n", name.c_str(), what); return false; };
    const size_t n_q = has.size(), n_grp = q_first.size() - 1;
    CascadeTables t;
    if (!build_cascade_tables(n_q, has.data(), n_kept, n_grp, q_first.data(), S, P, t)) return bad("refused");
    // the slots
    std::vector<size_t> owner;                                               // slot -> query
    for (size_t q = 0; q < n_q; ++q) {
        if (t.q_slot[q] != owner.size()) return bad("q_slot is not the prefix sum of the queries' pairs");
        if (has[q]) owner.insert(owner.end(), n_kept, q);
    }
    if (t.q_slot[n_q] != owner.size() || t.total != owner.size()) return bad("total");
    auto group_of = [&](size_t q) { size_t g = 0; while (!((size_t)q_first[g] <= q && q < (size_t)q_first[g + 1])) ++g; return g; };
    // the pieces tile the slots; one group, one chunk each
    size_t at = 0, seg_at = 0;
    for (size_t i = 0; i < t.pieces.size(); ++i) {
        const CascadePiece& pc = t.pieces[i];
        if (pc.n == 0 || pc.first != at) return bad("the pieces do not tile the slots");
        if (pc.first / P != pc.chunk || (pc.first + pc.n - 1) / P != pc.chunk) return bad("a piece crosses a chunk boundary");
        if (pc.first - pc.chunk * P + pc.n > std::min(P, std::max<size_t>(t.total, 1))) return bad("a piece exceeds its chunk's row maxima");
        for (size_t s = pc.first; s < pc.first + pc.n; ++s) if (group_of(owner[s]) != pc.group) return bad("a piece crosses a group boundary");
        if (i > 0 && t.pieces[i - 1].group == pc.group && t.pieces[i - 1].chunk == pc.chunk) return bad("two pieces of one group and chunk");
        // its segments tile it, never mix latents, never exceed S
        if (pc.seg_first != seg_at) return bad("seg_first");
        size_t p = 0;
        for (size_t k = 0; k < pc.n_seg; ++k) {
            const int32_t f = t.seg[2 * (pc.seg_first + k)], c = t.seg[2 * (pc.seg_first + k) + 1];
            if ((size_t)f != p || c < 1 || (size_t)c > S || p + (size_t)c > pc.n) return bad("a segment is out of place");
            for (size_t j = p; j < p + (size_t)c; ++j) if (owner[pc.first + j] != owner[pc.first + p]) return bad("a segment mixes latents");
            const bool run_ends = p + (size_t)c == pc.n || owner[pc.first + p + (size_t)c] != owner[pc.first + p];
            if ((size_t)c < S && !run_ends) return bad("a short segment inside a run");
            p += (size_t)c;
        }
        if (p != pc.n) return bad("the segments do not reach the piece's end");
        seg_at += pc.n_seg;
        at += pc.n;
    }
    if (at != t.total || 2 * seg_at != t.seg.size()) return bad("pieces or segments left over");
    // the device's copy
    const size_t n_p = t.pieces.size();
    if (t.dev.size() != n_q + 1 + n_p + 1 + n_p + t.seg.size()) return bad("dev's size");
    for (size_t q = 0; q <= n_q; ++q) if ((size_t)t.dev[t.q_slot_at + q] != t.q_slot[q]) return bad("dev: q_slot");
    for (size_t i = 0; i < n_p; ++i)
        if ((size_t)t.dev[t.piece_first_at + i] != t.pieces[i].first || t.dev[t.piece_q0_at + i] != q_first[t.pieces[i].group]) return bad("dev: pieces");
    if ((size_t)t.dev[t.piece_first_at + n_p] != t.total) return bad("dev: the last piece's end");
    for (size_t i = 0; i < t.seg.size(); ++i) if (t.dev[t.seg_at + i] != t.seg[i]) return bad("dev: seg");
    // k_cascade_gather's writes, replayed: thread (q, r) -> slot, piece by binary search over dev's piece_first, three ints (the piece's first slot: the count too)
    std::vector<int32_t> tab(t.tab_ints(), 0), hits(t.tab_ints(), 0);
    const int32_t* const piece_first = t.dev.data() + t.piece_first_at;
    for (size_t q = 0; q < n_q; ++q) {
        if ((size_t)(t.dev[t.q_slot_at + q + 1] - t.dev[t.q_slot_at + q]) != n_kept) continue;
        for (size_t r = 0; r < n_kept; ++r) {
            const int s = t.dev[t.q_slot_at + q] + (int)r;
            int lo = 0, hi = (int)n_p;
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (piece_first[mid] <= s) lo = mid; else hi = mid; }
            const size_t row = 2 * (size_t)s + (size_t)lo;
            if (s == piece_first[lo]) { tab.at(row) = piece_first[lo + 1] - piece_first[lo]; ++hits.at(row); }
            tab.at(row + 1) = (int32_t)q - t.dev[t.piece_q0_at + (size_t)lo]; ++hits.at(row + 1);
            tab.at(row + 2) = (int32_t)r; ++hits.at(row + 2);
        }
    }
    if (n_kept > 0) for (size_t i = 0; i < hits.size(); ++i) if (hits[i] != 1) return bad("an int of the pair tables is not written exactly once");
    // ... and what the pair kernels then read: piece i's table [count | (query of the group, rank) x count]
    for (size_t i = 0; i < n_p && n_kept > 0; ++i) {
        const CascadePiece& pc = t.pieces[i];
        const int32_t* pt = tab.data() + 2 * pc.first + i;
        if ((size_t)pt[0] != pc.n) return bad("a piece's count word");
        for (size_t p = 0; p < pc.n; ++p) {
            const size_t q = owner[pc.first + p];
            if (pt[1 + 2 * p] != (int32_t)q - q_first[pc.group] || pt[1 + 2 * p] < 0 || pt[1 + 2 * p] >= q_first[pc.group + 1] - q_first[pc.group]) return bad("a pair's query of the group");
            if ((size_t)pt[2 + 2 * p] != pc.first + p - t.q_slot[q]) return bad("a pair's rank");
        }
    }
    return true;
}

static std::vector<int32_t> cuts(std::mt19937& rng, int n_q, int n_grp)
{
    std::vector<int32_t> f{0};
    for (int g = 1; g < n_grp; ++g) f.push_back((int32_t)(rng() % (uint32_t)(n_q + 1)));
    f.push_back(n_q);
    std::sort(f.begin(), f.end());
    return f;
}

int main()
{
    std::mt19937 rng(20261020u);
    bool ok = true;
    const size_t S = 64;
    // no query; queries without pairs only; keep of nothing
    ok &= check("no query", {}, 7, {0}, S, 50);
    ok &= check("latent-empty queries only", {0, 0, 0}, 7, {0, 2, 3}, S, 50);
    ok &= check("n_kept 0", {1, 1}, 0, {0, 1, 2}, S, 50);
    // keep of 1, 64 and 65 — one segment, a full one, a full one and one pair — over two launch groups with a latent-empty query between two others
    for (size_t keep : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)70, (size_t)128, (size_t)129, (size_t)4096})
        for (size_t P : {(size_t)1, (size_t)50, (size_t)64, (size_t)65, (size_t)1000, (size_t)16384, (size_t)1 << 20}) {
            if (keep * 3 / P > 20000) continue;
            ok &= check("3 latents, keep " + std::to_string(keep) + ", chunks of " + std::to_string(P), {1, 0, 1}, keep, {0, 2, 3}, S, P);       // the group boundary behind the latent-empty query
            ok &= check("4 latents, keep " + std::to_string(keep) + ", chunks of " + std::to_string(P), {1, 1, 0, 1}, keep, {0, 1, 4}, S, P);    // ... and before it
            ok &= check("one group, keep " + std::to_string(keep) + ", chunks of " + std::to_string(P), {1, 1, 1}, keep, {0, 3}, S, P);
            ok &= check("a group without queries, keep " + std::to_string(keep) + ", chunks of " + std::to_string(P), {1, 1, 1}, keep, {0, 2, 2, 3}, S, P);
        }
    // a chunk boundary inside a latent's run, and exactly at its end
    ok &= check("chunk boundary inside a run", {1, 1}, 70, {0, 2}, S, 100);
    ok &= check("chunk boundary at a run's end", {1, 1}, 70, {0, 2}, S, 70);
    ok &= check("chunk boundary at a group's end", {1, 1}, 70, {0, 1, 2}, S, 70);
    ok &= check("segments of one pair", {1, 0, 1, 1}, 9, {0, 2, 4}, 1, 4);
    // random shapes
    for (int it = 0; it < 300 && ok; ++it) {
        const int n_q = 1 + (int)(rng() % 24), n_grp = 1 + (int)(rng() % 6);
        std::vector<uint8_t> has((size_t)n_q);
        for (uint8_t& h : has) h = rng() % 5 != 0;
        ok &= check("random " + std::to_string(it), has, rng() % 300, cuts(rng, n_q, n_grp), 1 + rng() % 70, 1 + rng() % 900);
    }
    // what does not fit 32-bit positions is refused, not built
    {
        ++g_cases;
        std::vector<uint8_t> has(300000, 1);
        const int32_t q_first[2] = {0, 300000};
        CascadeTables t;
        if (build_cascade_tables(has.size(), has.data(), 4096, 1, q_first, S, 16384, t)) { printf("cascade_tables_check: 1.2e9 pairs were not refused\n"); ok = false; }
    }
    if (!ok) return 1;
    printf("cascade_tables_check: %d cases ok\n", g_cases);
    return 0;
}
