// gallery_splice_plan_check.cpp — gallery_splice_plan.h::plan_gallery_splice as a program of its own, built with the host sanitizers (Makefile: gallery_splice_plan_check)
// and run directly by tests/test_gallery_replace_host.py.  Every case hands the planner heap arrays of EXACTLY the sizes its contract names (a read beyond them is the
// sanitizer's to find) and checks the plan against a naive rebuild of the final template list (the old list with list[idx[i] - index_base] = staged[i]):
//   - the new CSR offsets and empty flags are the final list's;
//   - the arrays a splice makes by the source tables — every point of the new array read where k_splice_ranges reads it, from the resident or the staged array, with the
//     reads checked against those arrays' sizes — are the concatenation of the final list's points (points carry distinct labels);
//   - `first` is the first replaced entry;
//   - a refused call returns the error the contract names and leaves the output plan untouched.
// Prints "gallery_splice_plan_check: N cases ok" and returns 0, or says what broke and returns 1.
#include "gallery_splice_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <utility>

using namespace afis;

static int g_cases = 0;

typedef std::vector<std::pair<int, int>> Counts;                            // (minutiae, texture points) per template

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v)
{
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

struct Tpl { int nm, nt; uint8_t empty; int64_t label; };                   // label: resident entry t -> t, staged template j -> -1 - j

static std::vector<int64_t> points_of(const std::vector<Tpl>& list, bool minu)
{
    std::vector<int64_t> v;
    for (const Tpl& t : list) for (int k = 0; k < (minu ? t.nm : t.nt); ++k) v.push_back(t.label * 4096 + (t.label < 0 ? -k : k));
    return v;
}

// one array spliced on the host as the kernel does it: the owner of every new point by its offsets, the source by the table
static bool splice(const std::vector<int32_t>& off, const std::vector<int32_t>& src, const std::vector<int64_t>& res, const std::vector<int64_t>& stg, std::vector<int64_t>& out)
{
    const size_t G = src.size();
    out.clear();
    for (size_t t = 0; t < G; ++t)
        for (int32_t p = off[t]; p < off[t + 1]; ++p) {
            const int64_t k = p - off[t], s = src[t];
            const std::vector<int64_t>& from = s >= 0 ? res : stg;
            const int64_t at = (s >= 0 ? s : (int64_t)~(int32_t)s) + k;
            if (at < 0 || (size_t)at >= from.size()) return false;
            out.push_back(from[(size_t)at]);
        }
    return true;
}

// res: the resident shard (an entry with no points is an empty entry when `res_flag` says so or always when it has none); staged likewise; st_base: where the staged offsets start
static bool check(const std::string& name, const Counts& res, int64_t base, const std::vector<int64_t>& idx, const Counts& staged, int want, int64_t st_base_m = 0, int64_t st_base_t = 0,
                  bool null_idx = false)
{
    ++g_cases;
    auto bad = [&](const char* what) { fprintf(stderr, "gallery_splice_plan_check: %s: %s\n", name.c_str(), what); return false; };
    const int64_t G = (int64_t)res.size(), n = (int64_t)idx.size(), ns = (int64_t)staged.size();
    std::vector<int32_t> mo{0}, to{0}; std::vector<uint8_t> em;
    std::vector<Tpl> list;
    for (int64_t t = 0; t < G; ++t) {
        const auto& c = res[(size_t)t];
        mo.push_back(mo.back() + c.first); to.push_back(to.back() + c.second); em.push_back(c.first == 0 && c.second == 0);
        list.push_back({c.first, c.second, em.back(), t});
    }
    std::vector<int64_t> smo{st_base_m}, sto{st_base_t}; std::vector<uint8_t> sem;
    std::vector<Tpl> slist;
    for (int64_t j = 0; j < ns; ++j) {
        const auto& c = staged[(size_t)j];
        smo.push_back(smo.back() + c.first); sto.push_back(sto.back() + c.second); sem.push_back(c.first == 0 && c.second == 0);
        slist.push_back({c.first, c.second, sem.back(), -1 - j});
    }
    auto p_mo = exact(mo), p_to = exact(to); auto p_em = exact(em); auto p_idx = exact(idx); auto p_smo = exact(smo), p_sto = exact(sto); auto p_sem = exact(sem);
    SplicePlan p;
    p.first = -77; p.mo = {1, 2, 3};                                        // a refused call must leave these
    const int rc = plan_gallery_splice(p_mo.get(), p_to.get(), p_em.get(), G, base, null_idx ? nullptr : p_idx.get(), n, ns, p_smo.get(), p_sto.get(), p_sem.get(), p);
    if (rc != want) { fprintf(stderr, "gallery_splice_plan_check: %s: returned %d (%s), expected %d\n", name.c_str(), rc, splice_plan_message(rc), want); return false; }
    if (rc != kSpliceOk) {
        if (p.first != -77 || p.mo != std::vector<int32_t>{1, 2, 3} || !p.to.empty()) return bad("a refused call wrote the plan");
        if (!*splice_plan_message(rc)) return bad("an error without a message");
        return true;
    }
    // the naive rebuild
    const std::vector<int64_t> res_m = points_of(list, true), res_t = points_of(list, false), stg_m = points_of(slist, true), stg_t = points_of(slist, false);
    int64_t first = G;
    for (int64_t i = 0; i < n; ++i) { list[(size_t)(idx[(size_t)i] - base)] = slist[(size_t)i]; first = std::min(first, idx[(size_t)i] - base); }
    std::vector<int32_t> wmo{0}, wto{0}; std::vector<uint8_t> wem;
    for (const Tpl& t : list) { wmo.push_back(wmo.back() + t.nm); wto.push_back(wto.back() + t.nt); wem.push_back(t.empty); }
    if (p.mo != wmo || p.to != wto) return bad("the new offsets");
    if (p.empty != wem) return bad("the new empty flags");
    if (p.first != first) return bad("the first replaced entry");
    if (p.src_m.size() != (size_t)G || p.src_t.size() != (size_t)G) return bad("the source tables' sizes");
    std::vector<int64_t> got;
    if (!splice(p.mo, p.src_m, res_m, stg_m, got)) return bad("a minutiae source beyond its array");
    if (got != points_of(list, true)) return bad("the spliced minutiae");
    if (!splice(p.to, p.src_t, res_t, stg_t, got)) return bad("a texture source beyond its array");
    if (got != points_of(list, false)) return bad("the spliced texture points");
    return true;
}

int main()
{
    const Counts sh = {{1, 1}, {15, 7}, {16, 8}, {17, 9}, {64, 15}, {129, 16}, {30, 17}, {40, 33}, {80, 1000}, {0, 300}, {50, 0}, {0, 0}, {0, 0}, {70, 250}, {2000, 1000}, {90, 400}};
    const int64_t G = (int64_t)sh.size();
    bool ok = true;
    for (int64_t B : {(int64_t)0, (int64_t)7000, (int64_t)1 << 40}) {
        const std::string tag = " base " + std::to_string(B);
        // the degenerate cases of the GPU tests
        ok &= check("one in the middle, more minutiae, fewer texture points" + tag, sh, B, {B + 7}, {{55, 20}}, kSpliceOk);
        ok &= check("ends and a run, not ascending" + tag, sh, B, {B + 5, B + G - 1, B + 4, B, B + 6}, {{3, 3}, {100, 0}, {0, 41}, {2000, 2000}, {16, 32}}, kSpliceOk);
        ok &= check("tile borders" + tag, sh, B, {B + 1, B + 2, B + 3, B + 4, B + 5, B + 6}, {{15, 31}, {16, 32}, {17, 33}, {63, 63}, {64, 64}, {65, 65}}, kSpliceOk);
        ok &= check("empty onto live" + tag, sh, B, {B + 8}, {{0, 0}}, kSpliceOk);
        ok &= check("live onto empty" + tag, sh, B, {B + 11, B + 12}, {{20, 300}, {1, 1}}, kSpliceOk);
        ok &= check("empty onto empty" + tag, sh, B, {B + 12}, {{0, 0}}, kSpliceOk);
        ok &= check("minutiae-only <-> texture-only" + tag, sh, B, {B + 9, B + 10}, {{44, 0}, {0, 444}}, kSpliceOk);
        ok &= check("every count kept" + tag, sh, B, {B + 13, B + 3, B + 9}, {{70, 250}, {17, 9}, {0, 300}}, kSpliceOk);
        {
            std::vector<int64_t> all; Counts rev;
            for (int64_t i = 0; i < G; ++i) { all.push_back(B + G - 1 - i); rev.push_back({(int)(3 * i), (int)(100 - 5 * i)}); }
            ok &= check("n == G" + tag, sh, B, all, rev, kSpliceOk);
        }
        ok &= check("a shard of one entry" + tag, {{40, 400}}, B, {B}, {{41, 399}}, kSpliceOk);
        ok &= check("a shard of one entry, emptied" + tag, {{40, 400}}, B, {B}, {{0, 0}}, kSpliceOk);
        ok &= check("a shard of one empty entry" + tag, {{0, 0}}, B, {B}, {{5, 5}}, kSpliceOk);
        ok &= check("staged offsets from a slice's base" + tag, sh, B, {B + 2, B + 14}, {{9, 90}, {8, 80}}, kSpliceOk, 123456, 7654321);
        ok &= check("staged offsets beyond 32 bits" + tag, sh, B, {B + 2, B + 14}, {{9, 90}, {8, 80}}, kSpliceOk, (int64_t)5 << 32, (int64_t)9 << 32);
        // the error cases
        ok &= check("null idx" + tag, sh, B, {B + 1}, {{1, 1}}, kSpliceNullIdx, 0, 0, true);
        ok &= check("fewer indices than staged" + tag, sh, B, {B + 1}, {{1, 1}, {2, 2}}, kSpliceCount);
        ok &= check("more indices than staged" + tag, sh, B, {B + 1, B + 2}, {{1, 1}}, kSpliceCount);
        ok &= check("no index, one staged" + tag, sh, B, {}, {{1, 1}}, kSpliceCount);
        ok &= check("below the shard" + tag, sh, B, {B + 1, B - 1}, {{1, 1}, {2, 2}}, kSpliceRange);
        ok &= check("behind the shard" + tag, sh, B, {B + G}, {{1, 1}}, kSpliceRange);
        ok &= check("far outside" + tag, sh, B, {INT64_MIN}, {{1, 1}}, kSpliceRange);
        ok &= check("far outside, above" + tag, sh, B, {INT64_MAX}, {{1, 1}}, kSpliceRange);
        ok &= check("twice" + tag, sh, B, {B + 3, B + 4, B + 3}, {{1, 1}, {2, 2}, {3, 3}}, kSpliceDuplicate);
        ok &= check("nothing staged, nothing listed" + tag, sh, B, {}, {}, kSpliceOk);     // (the entry point refuses it before the plan: AFIS_ESTATE)
    }
    // the limits: 2^31 - 1 points of either kind, the bound pass's 32-point tiles (offsets only: no arrays of that size are made — `check` would; the planner is called directly)
    {
        auto limits = [&](const char* name, int32_t res_m, int32_t res_t, int64_t st_m, int64_t st_t, int64_t n_res_small, int want) {
            ++g_cases;
            // entry 0 holds res_m / res_t points, then n_res_small entries of one texture point each; staged: one template of st_m / st_t points for entry 1
            const int64_t G2 = 1 + n_res_small;
            std::vector<int32_t> mo((size_t)G2 + 1), to((size_t)G2 + 1); std::vector<uint8_t> em((size_t)G2, 0);
            mo[0] = to[0] = 0;
            for (int64_t t = 0; t < G2; ++t) { mo[(size_t)t + 1] = mo[(size_t)t] + (t == 0 ? res_m : 0); to[(size_t)t + 1] = to[(size_t)t] + (t == 0 ? res_t : 1); }
            const std::vector<int64_t> idx{1}, smo{0, st_m}, sto{0, st_t}; const std::vector<uint8_t> sem{0};
            auto p_mo = exact(mo), p_to = exact(to); auto p_em = exact(em); auto p_idx = exact(idx); auto p_smo = exact(smo), p_sto = exact(sto); auto p_sem = exact(sem);
            SplicePlan p;
            const int rc = plan_gallery_splice(p_mo.get(), p_to.get(), p_em.get(), G2, 0, p_idx.get(), 1, 1, p_smo.get(), p_sto.get(), p_sem.get(), p);
            if (rc != want) { fprintf(stderr, "gallery_splice_plan_check: %s: returned %d, expected %d\n", name, rc, want); return false; }
            if (rc == kSpliceOk && (p.mo[(size_t)G2] != (int64_t)res_m + st_m || p.to[(size_t)G2] != (int64_t)res_t + (G2 - 2) + st_t)) { fprintf(stderr, "gallery_splice_plan_check: %s: totals\n", name); return false; }
            return true;
        };
        const int32_t big = 0x7fffffff;
        ok &= limits("minutiae at the limit", big - 2000, 10, 2000, 5, 1, kSpliceOk);
        ok &= limits("minutiae beyond the limit", big - 2000, 10, 2001, 5, 1, kSpliceTooLarge);
        ok &= limits("texture points beyond the limit", 10, big - 2000, 5, 2001, 1, kSpliceTooLarge);
        ok &= limits("staged points beyond 32 bits", 10, 10, (int64_t)1 << 31, 5, 1, kSpliceTooLarge);
        ok &= limits("minutiae at the limit, several small entries", big - 2000, 5000, 2000, 2000, 100, kSpliceOk);
        // the bound pass's stream holds 32 x (2^31 - 1) / 32 points: a bound below 2^31 - 1 texture points, met first
        const int32_t tiles = big / 32;
        ok &= limits("32-point tiles at the limit", 0, 32 * (tiles - 1), 0, 32, 1, kSpliceOk);
        ok &= limits("32-point tiles beyond the limit", 0, 32 * (tiles - 1), 0, 33, 1, kSpliceTooLarge);
        ok &= limits("32-point tiles beyond the limit by the small entries", 0, 32 * (tiles - 3), 0, 32, 4, kSpliceTooLarge);
    }
    std::mt19937_64 rng(2031);
    for (int c = 0; c < 400 && ok; ++c) {
        const int64_t G2 = 1 + (int64_t)(rng() % 60), B = c % 4 == 0 ? 0 : (int64_t)(rng() % 100000);
        auto counts = [&]() -> std::pair<int, int> {
            const unsigned k = (unsigned)(rng() % 8);
            if (k == 0) return {0, 0};
            if (k == 1) return {(int)(rng() % 130), 0};
            if (k == 2) return {0, (int)(rng() % 130)};
            return {(int)(rng() % 130), (int)(rng() % 1100)};
        };
        Counts res, staged;
        for (int64_t t = 0; t < G2; ++t) res.push_back(counts());
        std::vector<int64_t> perm;
        for (int64_t t = 0; t < G2; ++t) perm.push_back(B + t);
        std::shuffle(perm.begin(), perm.end(), rng);
        const size_t n = c % 7 == 0 ? (size_t)G2 : (size_t)(rng() % (uint64_t)(G2 + 1));
        perm.resize(n);
        for (size_t i = 0; i < n; ++i) staged.push_back(rng() % 5 == 0 ? res[(size_t)(perm[i] - B)] : counts());
        int want = kSpliceOk;
        const unsigned spoil = (unsigned)(rng() % 6);
        if (spoil == 0 && n >= 2) { perm[n - 1] = perm[0]; want = kSpliceDuplicate; }
        else if (spoil == 1 && n >= 1) { perm[rng() % n] = rng() % 2 ? B + G2 : B - 1; want = kSpliceRange; }
        else if (spoil == 2) { staged.push_back({1, 1}); want = kSpliceCount; }
        ok &= check("random " + std::to_string(c), res, B, perm, staged, want, c % 3 ? 0 : (int64_t)(rng() % 1000), c % 3 ? 0 : (int64_t)(rng() % 1000));
    }
    if (!ok) return 1;
    printf("gallery_splice_plan_check: %d cases ok\n", g_cases);
    return 0;
}
