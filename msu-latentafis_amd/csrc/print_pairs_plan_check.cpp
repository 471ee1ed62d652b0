// print_pairs_plan_check.cpp — print_pairs_plan.h::plan_print_pairs as a program of its own, built with the host sanitizers (Makefile: print_pairs_plan_check) and run
// directly by tests/test_print_pairs_host.py.  Every case hands the planner heap arrays of EXACTLY the sizes its contract names (a read beyond them is the sanitizer's
// to find) and checks what afis_score_print_pairs and afis_correspondences_print_pairs rely on:
//   - the query prints are the distinct a of the planned pairs, in order of first appearance, each gathered with exactly the templates some pair of it wants and it holds;
//   - the batches are consecutive runs that cover the prints once; no batch is empty; a batch obeys the cap, or — automatic — the budget unless it is ONE print;
//     a batch could not have taken the next print as well (the cuts are greedy);
//   - every planned pair lands in exactly one batch — the batch of its a —, at the position of its a in that batch's handle, and a batch's pairs keep the caller's order;
//     no other pair lands anywhere.
// Prints "print_pairs_plan_check: N cases ok" and returns 0, or says what broke and returns 1.
#include "print_pairs_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>

using namespace afis;

static int g_cases = 0;

struct Shard {
    int64_t base;
    std::vector<int32_t> mo, to;                                            // [G + 1]
    int64_t G() const { return (int64_t)mo.size() - 1; }
};

static Shard make_shard(int64_t base, const std::vector<std::pair<int, int>>& counts)
{
    Shard s{base, {0}, {0}};
    for (const auto& c : counts) { s.mo.push_back(s.mo.back() + c.first); s.to.push_back(s.to.back() + c.second); }
    return s;
}

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v)
{
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

static bool check(const std::string& name, const Shard& sh, const std::vector<int64_t>& a, const std::vector<int64_t>& b, const std::vector<uint8_t>& wm,
                  const std::vector<uint8_t>& wt, bool give_tex, int64_t cap, int64_t budget)
{
    ++g_cases;
    const int64_t n = (int64_t)a.size(), G = sh.G(), base = sh.base;
    auto pa = exact(a), pb = exact(b); auto pm = exact(wm), pt = exact(wt); auto mo = exact(sh.mo), to = exact(sh.to);
    PrintPairsPlan p;
    plan_print_pairs(n, pa.get(), pb.get(), base, G, mo.get(), to.get(), pm.get(), give_tex ? pt.get() : nullptr, cap, budget, p);
    auto bad = [&](const char* what) { fprintf(stderr, "print_pairs_plan_check: %s: %s\n", name.c_str(), what); return false; };
    auto cov = [&](int64_t g) { return g >= base && g < base + G; };
    // the planned pairs, the prints and their uses, restated
    std::vector<int64_t> planned;
    std::vector<int32_t> prints; std::vector<uint8_t> um, ut;
    for (int64_t i = 0; i < n; ++i) {
        if (!cov(a[(size_t)i]) || !cov(b[(size_t)i])) continue;
        const int32_t t = (int32_t)(a[(size_t)i] - base);
        const bool m = wm[(size_t)i] && sh.mo[(size_t)t + 1] > sh.mo[(size_t)t], x = give_tex && wt[(size_t)i] && sh.to[(size_t)t + 1] > sh.to[(size_t)t];
        if (!m && !x) continue;
        size_t s = std::find(prints.begin(), prints.end(), t) - prints.begin();
        if (s == prints.size()) { prints.push_back(t); um.push_back(0); ut.push_back(0); }
        um[s] |= m; ut[s] |= x;
        planned.push_back(i);
    }
    if (p.prints != prints || p.use_minu != um || p.use_tex != ut) return bad("the query prints or what is gathered of them");
    const size_t np = prints.size();
    if (p.batch_first.empty() || p.batch_first[0] != 0 || p.batch_first.back() != np || p.pair_first.size() != p.batch_first.size()) return bad("batch ranges");
    if (np == 0 && p.batch_first.size() != 1) return bad("a batch without prints");
    if (p.pair_first[0] != 0 || p.pair_first.back() != planned.size() || p.pair.size() != planned.size() || p.pos.size() != planned.size()) return bad("pair ranges");
    auto bytes = [&](size_t k) { return print_view_bytes(sh.mo.data(), sh.to.data(), prints[k], um[k] != 0, ut[k] != 0); };
    std::vector<int> seen((size_t)n, 0);
    for (size_t k = 0; k + 1 < p.batch_first.size(); ++k) {
        const size_t f = p.batch_first[k], e = p.batch_first[k + 1];
        if (e <= f) return bad("an empty batch");
        int64_t held = 0;
        for (size_t s = f; s < e; ++s) held += bytes(s);
        if (cap > 0) {
            if ((int64_t)(e - f) > cap) return bad("a batch beyond the cap");
            if (e < np && (int64_t)(e - f) < cap) return bad("a batch cut before the cap");
        } else {
            if (e - f > 1 && held > budget) return bad("a batch beyond the budget");
            if (e < np && held + bytes(e) <= budget) return bad("a batch cut although the next print fits");
        }
        int64_t prev = -1;
        if (p.pair_first[k] > p.pair_first[k + 1]) return bad("a batch's pair range runs backwards");
        for (size_t at = p.pair_first[k]; at < p.pair_first[k + 1]; ++at) {
            const int64_t i = p.pair[at];
            if (i < 0 || i >= n) return bad("a pair number outside the list");
            if (i <= prev) return bad("a batch's pairs out of the caller's order");
            prev = i;
            ++seen[(size_t)i];
            const int32_t pos = p.pos[at];
            if (pos < 0 || (size_t)pos >= e - f) return bad("a handle position outside the batch");
            if ((int64_t)prints[f + (size_t)pos] != a[(size_t)i] - base) return bad("a handle position that is not the pair's query print");
        }
    }
    std::vector<int> want((size_t)n, 0);
    for (int64_t i : planned) want[(size_t)i] = 1;
    if (seen != want) return bad("a planned pair in no batch or in two, or another pair in one");
    return true;
}

int main()
{
    const Shard sh = make_shard(7000, {{1, 1}, {15, 7}, {16, 8}, {17, 9}, {64, 15}, {129, 16}, {30, 17}, {40, 33}, {80, 1000}, {0, 300}, {50, 0}, {0, 0}, {0, 0}, {70, 250}, {2000, 1000}, {90, 400}});
    const int64_t G = sh.G(), B = sh.base;
    bool ok = true;
    auto all = [&](size_t n, uint8_t v) { return std::vector<uint8_t>(n, v); };
    const int64_t big = print_view_bytes(sh.mo.data(), sh.to.data(), 14, true, true);     // the largest print: 2000 minutiae, 1000 texture points
    for (int64_t cap : {0, 1, 2, 3, 1000})
        for (int64_t budget : {(int64_t)0, (int64_t)1, big / 4, big - 1, big, 3 * big, (int64_t)1 << 40}) {
            const std::string tag = " cap " + std::to_string(cap) + " budget " + std::to_string(budget);
            ok &= check("no pairs" + tag, sh, {}, {}, {}, {}, true, cap, budget);
            ok &= check("all uncovered" + tag, sh, {-1, B - 1, B + G, B, -1, INT64_MIN, INT64_MAX}, {B, B, B, B + G, -1, B, B}, all(7, 1), all(7, 1), true, cap, budget);
            ok &= check("one print in every pair" + tag, sh, std::vector<int64_t>(130, B + 8), {[&] { std::vector<int64_t> v; for (int i = 0; i < 130; ++i) v.push_back(B + i % G); return v; }()},
                        all(130, 1), all(130, 1), true, cap, budget);
            {
                std::vector<int64_t> a, b;
                for (int64_t i = 0; i < G; ++i) { a.push_back(B + i); b.push_back(B + (G - 1 - i)); }
                ok &= check("every pair a distinct print" + tag, sh, a, b, all((size_t)G, 1), all((size_t)G, 1), true, cap, budget);
                ok &= check("minutiae only" + tag, sh, a, b, all((size_t)G, 1), all((size_t)G, 0), false, cap, budget);
                ok &= check("nothing wanted" + tag, sh, a, b, all((size_t)G, 0), all((size_t)G, 0), true, cap, budget);
            }
            ok &= check("a print larger than the budget" + tag, sh, {B + 0, B + 14, B + 1, B + 14, B + 2}, {B, B, B, B + 1, B}, all(5, 1), all(5, 1), true, cap, budget);
            ok &= check("repeats" + tag, sh, {B + 3, B + 3, B + 5, B + 3, B + 5, B + 5, B + 3}, {B + 1, B + 1, B + 2, B + 1, B + 2, B + 2, B + 9}, {1, 0, 1, 0, 0, 1, 1}, {0, 1, 0, 0, 1, 1, 0},
                        true, cap, budget);
        }
    std::mt19937_64 rng(2027);
    for (int c = 0; c < 300 && ok; ++c) {
        const size_t n = (size_t)(rng() % 200);
        std::vector<int64_t> a(n), b(n); std::vector<uint8_t> wm(n), wt(n);
        for (size_t i = 0; i < n; ++i) {
            a[i] = B - 2 + (int64_t)(rng() % (uint64_t)(G + 4)); b[i] = B - 2 + (int64_t)(rng() % (uint64_t)(G + 4));
            if (rng() % 16 == 0) a[i] = -1;
            wm[i] = rng() % 3 != 0; wt[i] = rng() % 3 != 0;
        }
        const int64_t cap = c % 3 == 0 ? 0 : (int64_t)(rng() % 5), budget = (int64_t)(rng() % (uint64_t)(2 * big));
        ok &= check("random " + std::to_string(c), sh, a, b, wm, wt, c % 5 != 0, cap, budget);
    }
    if (!ok) return 1;
    printf("print_pairs_plan_check: %d cases ok\n", g_cases);
    return 0;
}
