// pq_train_plan_check.cpp — pq_train_plan.h as a program of its own, built with the host sanitizers (Makefile: pq_train_plan_check) and run directly by
// tests/test_pq_train_host.py.  Every case hands the sampler a heap array of EXACTLY 256 entries (a write beyond it is the sanitizer's to find) and checks what
// afis_pq_train_init_points relies on:
//   - the 256 indices of a sub-quantizer are distinct and lie in [0, n), at n = 256 (a permutation of all points), n = 257 and larger n up to 2^26;
//   - the same (n, seed, m) gives the same indices; the sub-quantizers of one seed differ, and so do two seeds;
//   - n < 256 is refused and writes nothing;
//   - the indices are the shuffle the header states, against a dense Fisher-Yates over a full array;
// and the CLI's selection: a template below min_points gives nothing, the others every stride-th point from the first.
// With an argument "n seed" it prints the 16 x 256 indices instead (the tests compare them with their Python restatement of the generator).
// Prints "pq_train_plan_check: N cases ok" and returns 0, or says what broke and returns 1.
#include "pq_train_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>

using namespace afis;

static int g_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("pq_train_plan_check: " __VA_ARGS__); printf("\n"); return 1; } } while (0)

static int check_indices(int64_t n, uint64_t seed)
{
    std::vector<std::vector<int64_t>> all;
    for (int m = 0; m < 16; ++m) {
        std::unique_ptr<int64_t[]> a(new int64_t[kTrainInitK]), b(new int64_t[kTrainInitK]);
        CHECK(train_init_indices(n, seed, m, a.get()) && train_init_indices(n, seed, m, b.get()), "n %lld refused", (long long)n);
        CHECK(std::equal(a.get(), a.get() + kTrainInitK, b.get()), "n %lld seed %llu m %d: two calls differ", (long long)n, (unsigned long long)seed, m);
        std::vector<int64_t> s(a.get(), a.get() + kTrainInitK);
        all.push_back(s);
        std::sort(s.begin(), s.end());
        CHECK(s.front() >= 0 && s.back() < n, "n %lld m %d: index out of range", (long long)n, m);
        CHECK(std::adjacent_find(s.begin(), s.end()) == s.end(), "n %lld m %d: an index twice", (long long)n, m);
        if (n <= 4096) {                                                       // the dense shuffle of the header's statement
            std::vector<int64_t> d((size_t)n);
            std::iota(d.begin(), d.end(), 0);
            for (int j = 0; j < kTrainInitK; ++j) std::swap(d[(size_t)j], d[(size_t)(j + (int64_t)(train_draw(seed, m, j) % (uint64_t)(n - j)))]);
            CHECK(std::equal(a.get(), a.get() + kTrainInitK, d.begin()), "n %lld m %d: not the stated shuffle", (long long)n, m);
        }
        ++g_cases;
    }
    for (int m = 1; m < 16; ++m) CHECK(all[(size_t)m] != all[0] && all[(size_t)m] != all[(size_t)m - 1], "n %lld: sub-quantizers %d and another draw alike", (long long)n, m);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3) {
        const int64_t n = atoll(argv[1]); const uint64_t seed = strtoull(argv[2], nullptr, 10);
        int64_t idx[kTrainInitK];
        for (int m = 0; m < 16; ++m) {
            if (!train_init_indices(n, seed, m, idx)) return 1;
            for (int j = 0; j < kTrainInitK; ++j) printf("%lld%c", (long long)idx[j], j + 1 < kTrainInitK ? ' ' : '\n');
        }
        return 0;
    }
    for (int64_t n : {(int64_t)256, (int64_t)257, (int64_t)258, (int64_t)300, (int64_t)511, (int64_t)4096, (int64_t)100000, (int64_t)1 << 26})
        for (uint64_t seed : {0ull, 1ull, 2ull, 0xFFFFFFFFFFFFFFFFull, 0x123456789ABCDEFull})
            if (check_indices(n, seed)) return 1;
    {
        std::unique_ptr<int64_t[]> a(new int64_t[kTrainInitK]), b(new int64_t[kTrainInitK]);
        train_init_indices(5000, 7, 3, a.get()); train_init_indices(5000, 8, 3, b.get());
        CHECK(!std::equal(a.get(), a.get() + kTrainInitK, b.get()), "seeds 7 and 8 draw alike");
        std::fill(a.get(), a.get() + kTrainInitK, (int64_t)-7);
        for (int64_t n : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)255}) CHECK(!train_init_indices(n, 0, 0, a.get()), "n %lld accepted", (long long)n);
        CHECK(std::all_of(a.get(), a.get() + kTrainInitK, [](int64_t v) { return v == -7; }), "a refused call wrote");
        g_cases += 5;
    }
    for (int64_t n = 0; n <= 260; ++n)
        for (int64_t min_points : {(int64_t)0, (int64_t)1, (int64_t)100, (int64_t)101})
            for (int64_t stride : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)7}) {
                std::vector<int64_t> got{-5};
                const int64_t k = train_take_points(n, min_points, stride, got);
                const int64_t st = stride < 1 ? 1 : stride;
                const int64_t want = (n <= 0 || n < min_points) ? 0 : (n + st - 1) / st;
                CHECK(k == want && (int64_t)got.size() == 1 + want && got[0] == -5, "take(%lld, %lld, %lld): %lld points", (long long)n, (long long)min_points, (long long)stride, (long long)k);
                for (int64_t i = 0; i < want; ++i) CHECK(got[(size_t)(1 + i)] == i * st && i * st < n, "take(%lld, %lld, %lld): entry %lld", (long long)n, (long long)min_points, (long long)stride, (long long)i);
                ++g_cases;
            }
    printf("pq_train_plan_check: %d cases ok\n", g_cases);
    return 0;
}
