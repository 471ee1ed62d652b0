// rank_order_check — rank_order.h on score rows that hold NaNs, and score_order.h on the words of every boundary of its order, as a stand-alone program built with -fsanitize=address,undefined (csrc/Makefile): the sorts of
// afis_rank_list, of the search's host rank lists (k > 64) and of the exchange's merge must be defined behaviour and give ONE order whatever bits a row holds.
//   rank_order_check                      every function on every row kind at n = 0, 1, 2, 15, 16, 17, 1000, 5000 (either side of libstdc++'s insertion-sort
//                                         threshold, and well past it) against a model that sorts (key, index) pairs; exit 0 when all agree
//   rank_order_check -old-rank-list <f>   the statement afis_rank_list(ref_order 1) made before it compared keys — std::sort of 0 .. n-1 on scores[a] > scores[b]
//                                         (matcher.cpp:306-308) — on the score words of <f> ("n", then n hex words): prints the permutation.  For NaN-FREE columns
//                                         only: tests/test_rank_order_host.py holds the new statement against it there.
//   rank_order_check -float-compare       the same rows through the float comparators the three places used before (undefined behaviour on a NaN: run it from a
//                                         build without the sanitizers to count, with them to see the first bad read): prints per place how many rows differ
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <tuple>

#include "rank_order.h"

using namespace afis;

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }     // (the leak check needs ptrace, which a test box may refuse; nothing here is about leaks)

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static float from_bits(uint32_t w) { float f; memcpy(&f, &w, 4); return f; }
static uint32_t bits_of(float f) { uint32_t w; memcpy(&w, &f, 4); return w; }

constexpr int kKinds = 3;
// 0: infinities, both zeros, quiet NaNs of both signs among plain values; 1: small integers, one value in five a NaN; 2: finite except one NaN of either sign
static std::vector<float> make_row(int kind, int64_t n)
{
    static const uint32_t special[9] = {0x7f800000u, 0xff800000u, 0x00000000u, 0x80000000u, 0x7fc00000u, 0xffc00000u, 0x3fc00000u, 0xbf800000u, 0x40500000u};
    std::vector<float> row((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (kind == 0) row[(size_t)i] = from_bits(special[rnd() % 9]);
        else if (kind == 1) row[(size_t)i] = rnd() % 5 == 0 ? from_bits(0x7fc00000u) : (float)(rnd() % 40);
        else row[(size_t)i] = (float)(rnd() % 40) - 8.0f;
    }
    if (kind == 2 && n >= 2) {
        const size_t a = rnd() % (size_t)n; size_t b = rnd() % (size_t)n;
        if (b == a) b = (a + 1) % (size_t)n;
        row[a] = from_bits(0x7fc00000u); row[b] = from_bits(0xffc00000u);
    }
    return row;
}

// the model: positions sorted as (key descending, global index ascending) tuples — no comparator of rank_order.h
static std::vector<int> model_order(const std::vector<float>& row, const std::vector<int64_t>* col)
{
    std::vector<std::tuple<uint32_t, int64_t, int>> t;
    for (size_t i = 0; i < row.size(); ++i) t.emplace_back(~rank_key(row[i]), col ? (*col)[i] : (int64_t)i, (int)i);
    std::sort(t.begin(), t.end());
    std::vector<int> out;
    for (const auto& e : t) out.push_back(std::get<2>(e));
    return out;
}

static bool is_permutation_of_n(const std::vector<int>& ind, size_t n)
{
    if (ind.size() != n) return false;
    std::vector<char> seen(n, 0);
    for (int v : ind) { if (v < 0 || (size_t)v >= n || seen[(size_t)v]) return false; seen[(size_t)v] = 1; }
    return true;
}

static std::vector<int64_t> shuffled_globals(size_t n)
{
    std::vector<int64_t> col(n);
    for (size_t i = 0; i < n; ++i) col[i] = 5000000000ll + (int64_t)i * 3;
    for (size_t i = n; i > 1; --i) std::swap(col[i - 1], col[rnd() % i]);
    return col;
}

// per-shard top-k of a row cut into `world` contiguous shards, rank-major with (-1, -inf) padding: what the ranks hand to the exchange
static void shard_lists(const std::vector<float>& row, int world, int k, std::vector<int64_t>& idx, std::vector<float>& sc)
{
    idx.assign((size_t)world * k, -1); sc.assign((size_t)world * k, -INFINITY);
    const int64_t n = (int64_t)row.size();
    for (int r = 0; r < world; ++r) {
        const int64_t lo = n * r / world, hi = n * (r + 1) / world;
        rank_topk(row.data() + lo, hi - lo, k, nullptr, lo, idx.data() + (size_t)r * k, sc.data() + (size_t)r * k);
    }
}

template <class Before>
static void merge_lists(const std::vector<int64_t>& idx, const std::vector<float>& sc, int k_out, Before before, std::vector<int64_t>& out_i, std::vector<uint32_t>& out_w)
{
    std::vector<size_t> ord;
    for (size_t i = 0; i < idx.size(); ++i) if (idx[i] >= 0) ord.push_back(i);
    std::sort(ord.begin(), ord.end(), before);
    out_i.assign((size_t)k_out, -1); out_w.assign((size_t)k_out, 0xff800000u);
    for (size_t r = 0; r < ord.size() && r < (size_t)k_out; ++r) { out_i[r] = idx[ord[r]]; out_w[r] = bits_of(sc[ord[r]]); }
}

static const int64_t kSizes[] = {0, 1, 2, 15, 16, 17, 1000, 5000};
static const int kWorlds[] = {2, 3, 8};

static int check_all()
{
    long long failures = 0, cases = 0;
    auto expect = [&](bool ok, const char* what, int kind, int64_t n) { ++cases; if (!ok) { ++failures; fprintf(stderr, "rank_order_check: %s fails, kind %d n %lld\n", what, kind, (long long)n); } };
    for (int kind = 0; kind < kKinds; ++kind)
        for (int64_t n : kSizes)
            for (int rep = 0; rep < (n <= 17 ? 50 : 3); ++rep) {
                const std::vector<float> row = make_row(kind, n);
                const std::vector<int> want = model_order(row, nullptr);
                std::vector<int> ind, again;
                rank_list_order(row.data(), n, false, ind);
                expect(ind == want, "rank_list_order(ref_order 0) against the model", kind, n);
                rank_list_order(row.data(), n, true, ind);
                rank_list_order(row.data(), n, true, again);
                bool desc = is_permutation_of_n(ind, (size_t)n);
                for (size_t j = 1; desc && j < ind.size(); ++j) desc = rank_key(row[(size_t)ind[j - 1]]) >= rank_key(row[(size_t)ind[j]]);
                expect(desc, "rank_list_order(ref_order 1): a permutation, descending in key", kind, n);
                expect(ind == again, "rank_list_order(ref_order 1) twice", kind, n);
                const std::vector<int64_t> col = shuffled_globals((size_t)n);
                const std::vector<int> want_col = model_order(row, &col);
                for (int k : {1, 24, 64, 65, 100, (int)n + 3}) {
                    std::vector<int64_t> oi((size_t)k), ci((size_t)k); std::vector<float> os((size_t)k), cs((size_t)k);
                    rank_topk(row.data(), n, k, nullptr, 1000, oi.data(), os.data());
                    rank_topk(row.data(), n, k, col.data(), 0, ci.data(), cs.data());
                    bool ok = true, okc = true;
                    for (int r = 0; r < k; ++r) {
                        const bool in = r < n;
                        ok = ok && oi[(size_t)r] == (in ? 1000 + want[(size_t)r] : -1) && bits_of(os[(size_t)r]) == (in ? bits_of(row[(size_t)want[(size_t)r]]) : 0xff800000u);
                        okc = okc && ci[(size_t)r] == (in ? col[(size_t)want_col[(size_t)r]] : -1) && bits_of(cs[(size_t)r]) == (in ? bits_of(row[(size_t)want_col[(size_t)r]]) : 0xff800000u);
                    }
                    expect(ok, "rank_topk against the model", kind, n);
                    expect(okc, "rank_topk with a column table against the model", kind, n);
                }
                for (int world : kWorlds)
                    for (int k_out : {24, 10}) {
                        std::vector<int64_t> idx, oi; std::vector<float> sc; std::vector<uint32_t> ow;
                        shard_lists(row, world, 24, idx, sc);
                        merge_lists(idx, sc, k_out, [&](size_t a, size_t b) { return rank_before(sc[a], idx[a], sc[b], idx[b]); }, oi, ow);
                        bool ok = true;
                        for (int r = 0; r < k_out; ++r) {
                            const bool in = r < n;
                            ok = ok && oi[(size_t)r] == (in ? want[(size_t)r] : -1) && ow[(size_t)r] == (in ? bits_of(row[(size_t)want[(size_t)r]]) : 0xff800000u);
                        }
                        expect(ok, "merge of the shards' lists against the one-shard list", kind, n);
                    }
            }
    // score_order.h itself: the words either side of every boundary of the order, and a stride through all of them
    std::vector<uint32_t> words = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7fffffffu, 0xffffffffu, 0xbf800000u};
    for (uint32_t i = 0; i < 65536u; ++i) words.push_back(i * 65537u);
    bool inverse = true, increasing = true, key = true, takes_part = true, position = true;
    for (uint32_t w : words) {
        const float f = from_bits(w);
        inverse = inverse && score_bits_of(ordered_word(w)) == w && ordered_word(f) == ordered_word(w);
        key = key && rank_key(f) == ordered_word(bits_of(f + 0.0f));
        takes_part = takes_part && reaches_zero(f) == (rank_key(f) >= rank_key(+0.0f));
        for (uint32_t p : {0u, 1u, 0x7fffffffu}) {
            const uint64_t c = rank_composite(ordered_word(w), p);
            position = position && composite_position(c) == p && composite_word(c) == ordered_word(w) && composite_at(c, p ^ 1u) == rank_composite(ordered_word(w), p ^ 1u);
        }
        for (uint32_t v : {words[rnd() % words.size()], w + 1u, w ^ 0x80000000u}) {     // wherever the float order is strict, the words' is, the same way
            const float g = from_bits(v);
            if (f < g || f > g) increasing = increasing && (f < g) == (ordered_word(w) < ordered_word(v)) && ordered_word(w) != ordered_word(v);
        }
    }
    expect(inverse, "score_bits_of inverts ordered_word", -1, (int64_t)words.size());
    expect(increasing, "ordered_word increases with the float order", -1, (int64_t)words.size());
    expect(key && takes_part, "rank_key is the ordered word of s + 0.0f, reaches_zero is rank_key(s) >= rank_key(+0.0f)", -1, (int64_t)words.size());
    expect(position, "a composite gives its word and its position back", -1, (int64_t)words.size());
    expect(rank_key(-0.0f) == rank_key(+0.0f) && ordered_word(-0.0f) < ordered_word(+0.0f), "the two zeros: one rank_key, two ordered words", -1, 2);
    expect(ordered_word(kNoEntryWord) == 0u && ordered_word(from_bits(0xff800000u)) == 0x007fffffu, "the no-entry word lies below every threshold", -1, 1);
    printf("rank_order_check: %lld checks, %lld failures\n", cases, failures);
    return failures ? 1 : 0;
}

// The float comparators of the three places as they stood, on the same rows.  A NaN makes each of them something other than a strict weak order.
static int float_compare()
{
    long long rows = 0, list0 = 0, list1 = 0, list1_finite = 0, topk65 = 0, topk100 = 0, merged = 0, merges = 0;
    for (int kind = 0; kind < kKinds; ++kind)
        for (int64_t n : kSizes)
            for (int rep = 0; rep < (n <= 17 ? 50 : 3); ++rep) {
                const std::vector<float> row = make_row(kind, n);
                const float* scores = row.data();
                const std::vector<int> want = model_order(row, nullptr);
                (void)shuffled_globals((size_t)n);                                      // (keeps the generator in step with check_all: the same rows)
                ++rows;
                std::vector<int> ind((size_t)n);
                auto by_score = [scores](const int& a, const int& b) { return scores[a] > scores[b]; };
                std::iota(ind.begin(), ind.end(), 0); std::stable_sort(ind.begin(), ind.end(), by_score);
                list0 += ind != want;
                std::iota(ind.begin(), ind.end(), 0); std::sort(ind.begin(), ind.end(), by_score);
                bool desc = is_permutation_of_n(ind, (size_t)n), fin = true;
                float last = INFINITY;
                for (size_t j = 0; desc && j < ind.size(); ++j) {
                    if (j) desc = rank_key(row[(size_t)ind[j - 1]]) >= rank_key(row[(size_t)ind[j]]);
                    const float v = row[(size_t)ind[j]];
                    if (std::isfinite(v)) { fin = fin && v <= last; last = v; }
                }
                list1 += !desc; list1_finite += !fin;
                for (int k : {65, 100}) {
                    std::vector<int32_t> p((size_t)n); std::iota(p.begin(), p.end(), 0);
                    const int kk = (int)std::min<int64_t>(k, n);
                    std::partial_sort(p.begin(), p.begin() + kk, p.end(), [scores](int a, int b) { return scores[a] > scores[b] || (scores[a] == scores[b] && a < b); });
                    bool same = true;
                    for (int r = 0; r < kk; ++r) same = same && p[(size_t)r] == want[(size_t)r];
                    (k == 65 ? topk65 : topk100) += !same;
                }
                for (int world : kWorlds)
                    for (int k_out : {24, 10}) {
                        std::vector<int64_t> idx, oi; std::vector<float> sc; std::vector<uint32_t> ow;
                        shard_lists(row, world, 24, idx, sc);
                        merge_lists(idx, sc, k_out, [&](size_t a, size_t b) { return sc[a] > sc[b] || (sc[a] == sc[b] && idx[a] < idx[b]); }, oi, ow);
                        bool same = true;
                        for (int r = 0; r < k_out && r < n; ++r) same = same && oi[(size_t)r] == want[(size_t)r];
                        ++merges; merged += !same;
                    }
            }
    printf("rows %lld\n", rows);
    printf("afis_rank_list ref_order 0 (stable_sort, scores[a] > scores[b]): %lld rows differ from the key order\n", list0);
    printf("afis_rank_list ref_order 1 (sort, scores[a] > scores[b]): %lld rows not descending in key, %lld with their FINITE scores out of order\n", list1, list1_finite);
    printf("search, k = 65 (partial_sort, float compare + index): %lld rows differ; k = 100: %lld\n", topk65, topk100);
    printf("merge_topk (sort, float compare + index): %lld of %lld merges differ from the one-shard list\n", merged, merges);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 3 && !strcmp(argv[1], "-old-rank-list")) {
        std::ifstream f(argv[2]);
        long long n = 0;
        if (!(f >> n) || n < 0) { fprintf(stderr, "rank_order_check: bad file\n"); return 2; }
        std::vector<float> sc((size_t)n);
        for (auto& v : sc) { std::string w; if (!(f >> w)) { fprintf(stderr, "rank_order_check: short file\n"); return 2; } v = from_bits((uint32_t)strtoul(w.c_str(), nullptr, 16)); if (std::isnan(v)) { fprintf(stderr, "rank_order_check: a NaN: the old statement is undefined there\n"); return 2; } }
        const float* scores = sc.data();
        std::vector<int> ind((size_t)n);
        std::iota(ind.begin(), ind.end(), 0);
        std::sort(ind.begin(), ind.end(), [scores](const int& a, const int& b) { return scores[a] > scores[b]; });     // matcher.cpp:306-308, as afis_rank_list stated it
        for (int v : ind) printf("%d\n", v);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "-float-compare")) return float_compare();
    return check_all();
}
