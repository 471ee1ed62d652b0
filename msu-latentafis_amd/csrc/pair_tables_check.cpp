// pair_tables_check.cpp — pair_tables.h::build_pair_tables as a program of its own, built with the host sanitizers (Makefile: pair_tables_check) and run directly by
// tests/test_score_pairs_host.py.  Every case hands the builder buffers of EXACTLY the sizes its contract names (2 m + n_grp and 2 m ints, heap arrays: a write beyond them
// is the sanitizer's to find) and checks what afis_score_pairs relies on:
//   - every pair of the chunk sits in exactly one slot, inside its launch group's table, with its (query of the group, template) entry, and slot_of leads back to it;
//   - a group's slots are sorted by latent, and the pairs of one latent keep the caller's order;
//   - the segments of a group cover every latent's run exactly once, in order, each inside ONE latent and of 1 .. S pairs; a latent without pairs has none.
// Every case runs a second time as afis_correspondences_pairs calls the builder — seg == NULL, no work list: the same checks of tab and slot_of, and 0 segments.
// Prints "pair_tables_check: N cases ok" and returns 0, or says what broke and returns 1.
#include "pair_tables.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>

using namespace afis;

static int g_cases = 0;

// work_list false: the form of afis_correspondences_pairs — no seg array exists at all, tab is all the builder may write —: the same tab and slot_of, no segment
static bool check_form(const std::string& name, const std::vector<int32_t>& query, const std::vector<int32_t>& tmpl, const std::vector<int32_t>& q_first, int S, bool work_list)
{
    ++g_cases;
    const size_t m = query.size(), n_grp = q_first.size() - 1;
    std::unique_ptr<int32_t[]> tab(new int32_t[2 * m + n_grp]), seg(work_list ? new int32_t[m ? 2 * m : 1] : nullptr);
    for (size_t i = 0; i < 2 * m + n_grp; ++i) tab[i] = -7;
    PairChunkTables t;
    const size_t n_seg = build_pair_tables(m, query.data(), tmpl.data(), n_grp, q_first.data(), S, tab.get(), seg.get(), t);
    auto bad = [&](const char* what) { fprintf(stderr, "pair_tables_check: %s%s: %s\n", name.c_str(), work_list ? "" : ", no work list", what); return false; };
    if (t.first.size() != n_grp + 1 || t.seg_first.size() != n_grp + 1 || t.slot_of.size() != m) return bad("table sizes");
    if (t.first[0] != 0 || t.first[n_grp] != m || t.seg_first[0] != 0 || t.seg_first[n_grp] != n_seg || n_seg > m) return bad("group ranges");
    if (!work_list && (n_seg != 0 || std::count(t.seg_first.begin(), t.seg_first.end(), (size_t)0) != (long)(n_grp + 1))) return bad("segments without a work list");
    std::vector<int> seen(m, 0);
    for (size_t g = 0; g < n_grp; ++g) {
        if (t.first[g] > t.first[g + 1] || t.seg_first[g] > t.seg_first[g + 1]) return bad("a group's range runs backwards");
        const int32_t* gt = tab.get() + 2 * t.first[g] + g;
        const size_t n = t.first[g + 1] - t.first[g];
        if (gt[0] != (int32_t)n) return bad("a group's pair count");
        int32_t prev_q = -1, prev_k = -1;
        for (size_t p = 0; p < n; ++p) {
            const size_t slot = t.first[g] + p;
            const int32_t k = t.slot_of[slot];
            if (k < 0 || (size_t)k >= m) return bad("slot_of outside the chunk");
            if (seen[(size_t)k]++) return bad("a pair sits in two slots");
            const int32_t lq = gt[1 + 2 * p], tt = gt[2 + 2 * p];
            if (lq < 0 || lq >= q_first[g + 1] - q_first[g]) return bad("a pair in the wrong group's table");
            if (lq + q_first[g] != query[(size_t)k] || tt != tmpl[(size_t)k]) return bad("a slot's entry is not its pair's");
            if (lq < prev_q) return bad("a group's slots are not sorted by latent");
            if (lq == prev_q && k < prev_k) return bad("the pairs of one latent lost the caller's order");
            prev_q = lq; prev_k = k;
        }
        if (!work_list) continue;
        // the segments: in order, back to back over the slots that hold pairs, never across two latents
        size_t at = 0;
        for (size_t s = t.seg_first[g]; s < t.seg_first[g + 1]; ++s) {
            const int32_t p0 = seg[2 * s], cnt = seg[2 * s + 1];
            if (p0 < 0 || (size_t)p0 != at) return bad("the segments do not cover the runs exactly once");
            if (cnt < 1 || cnt > S || at + (size_t)cnt > n) return bad("a segment's size");
            for (int32_t j = 1; j < cnt; ++j) if (gt[1 + 2 * (p0 + j)] != gt[1 + 2 * p0]) return bad("a segment spans two latents");
            // a segment shorter than S ends its latent's run
            if (cnt < S && at + (size_t)cnt < n && gt[1 + 2 * (p0 + cnt)] == gt[1 + 2 * p0]) return bad("a short segment inside a run");
            at += (size_t)cnt;
        }
        if (at != n) return bad("the segments do not reach the group's end");
    }
    for (size_t k = 0; k < m; ++k) if (seen[k] != 1) return bad("a pair sits in no slot");
    return true;
}

// every shape in both forms
static bool check(const std::string& name, const std::vector<int32_t>& query, const std::vector<int32_t>& tmpl, const std::vector<int32_t>& q_first, int S)
{
    const bool with = check_form(name, query, tmpl, q_first, S, true), without = check_form(name, query, tmpl, q_first, S, false);
    return with && without;
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
    std::mt19937 rng(20240611u);
    bool ok = true;
    const int S = kAdcPairsSegment;
    // nothing at all; groups without a pair; one pair
    ok &= check("empty chunk", {}, {}, {0, 3, 5}, S);
    ok &= check("one pair", {4}, {9}, {0, 3, 5}, S);
    ok &= check("one group, one pair", {0}, {0}, {0, 1}, S);
    // all pairs on one latent: n a multiple of S, and off by one either way
    for (int n : {1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 5 * S, 4096}) {
        std::vector<int32_t> q((size_t)n, 2), t((size_t)n);
        for (int i = 0; i < n; ++i) t[(size_t)i] = i;
        ok &= check("one latent x " + std::to_string(n), q, t, {0, 2, 4}, S);       // (latents 0, 1, 3 have no pair; group 0 is empty of pairs)
        ok &= check("one latent x " + std::to_string(n) + ", S = 1", q, t, {0, 4}, 1);
    }
    // a latent's run cut by a chunk boundary: the two halves are two chunks to the builder — the second starts inside the run
    {
        std::vector<int32_t> q, t;
        for (int i = 0; i < 3 * S + 5; ++i) { q.push_back(i < 2 * S + 1 ? 1 : 2); t.push_back(i); }
        const size_t cut = (size_t)S + 7;
        ok &= check("chunk boundary, first half", {q.begin(), q.begin() + (long)cut}, {t.begin(), t.begin() + (long)cut}, {0, 2, 3}, S);
        ok &= check("chunk boundary, second half", {q.begin() + (long)cut, q.end()}, {t.begin() + (long)cut, t.end()}, {0, 2, 3}, S);
    }
    // adversarial orders: descending latents, interleaved, every pair repeated
    {
        std::vector<int32_t> q, t;
        for (int i = 0; i < 300; ++i) { q.push_back(9 - i % 10); t.push_back(i % 7); }
        ok &= check("descending latents", q, t, {0, 4, 4, 10}, S);                   // (a group without queries)
        for (int i = 0; i < 300; ++i) { q.push_back(q[(size_t)i]); t.push_back(t[(size_t)i]); }
        ok &= check("repeated pairs", q, t, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 3);
    }
    // random lists over random cuts
    for (int it = 0; it < 200 && ok; ++it) {
        const int n_q = 1 + (int)(rng() % 40), n_grp = 1 + (int)(rng() % 6), m = (int)(rng() % 700), seg = 1 + (int)(rng() % 70);
        std::vector<int32_t> q((size_t)m), t((size_t)m);
        const int hot = (int)(rng() % (uint32_t)n_q);
        for (int i = 0; i < m; ++i) { q[(size_t)i] = rng() % 3 ? hot : (int32_t)(rng() % (uint32_t)n_q); t[(size_t)i] = (int32_t)(rng() % 100000u); }
        ok &= check("random " + std::to_string(it), q, t, cuts(rng, n_q, n_grp), seg);
    }
    if (!ok) return 1;
    printf("pair_tables_check: %d cases ok\n", g_cases);
    return 0;
}
