// target_tables_check.cpp — target_tables.h, the targets of a matrix call as a CSR by row, and column_names.h, the column a name refers to, as a program of its own:
// built with the host sanitizers (Makefile: -fsanitize=address,undefined) and run directly by tests/test_target_tables_host.py.  Every case is checked against a
// restatement without the builders' loops: the (row, key, caller's position) triples sorted, and the names looked up by linear search.
#include "column_names.h"
#include "target_tables.h"

#include <cstdio>
#include <random>
#include <string>
#include <tuple>

using namespace afis;

static int g_cases = 0;

// query [n]; dev: the targets that go to the device (use_dev false: all n); key [n] (use_key false: none)
static bool check_tables(const std::string& name, const std::vector<int32_t>& query, bool use_dev, const std::vector<int32_t>& dev, bool use_key, const std::vector<int64_t>& key)
{
    ++g_cases;
    auto bad = [&](const char* what) { printf("target_tables_check: %s: %s\n", name.c_str(), what); return false; };
    const size_t m = use_dev ? dev.size() : query.size();
    const TargetTables t = build_target_tables(query.data(), use_dev ? dev.data() : nullptr, m, use_key ? key.data() : nullptr);
    std::vector<std::tuple<int32_t, int64_t, int32_t>> want(m);             // (row, key, place in the device list)
    for (size_t k = 0; k < m; ++k) {
        const size_t i = use_dev ? (size_t)dev[k] : k;
        want[k] = std::make_tuple(query[i], use_key ? key[i] : (int64_t)0, (int32_t)k);
    }
    std::sort(want.begin(), want.end());
    if (t.order.size() != m) return bad("order's size");
    std::vector<int32_t> rows, off(1, 0), row_of_place;
    int32_t longest = 0;
    for (size_t p = 0; p < m; ++p) {
        if (t.order[p] != std::get<2>(want[p])) return bad("order is not the sorted triples'");
        const int32_t q = std::get<0>(want[p]);
        if (rows.empty() || rows.back() != q) { rows.push_back(q); off.push_back((int32_t)p); }
        off.back() = (int32_t)p + 1;
        row_of_place.push_back(q);
    }
    for (size_t r = 0; r < rows.size(); ++r) longest = std::max(longest, off[r + 1] - off[r]);
    if (t.rows != rows) return bad("rows");
    if (t.off != off) return bad("off");
    if (t.max_row_targets != longest) return bad("max_row_targets");
    // the writer: rows | off | row [m], then the call's own column [m], untouched; the vector ends there (the sanitizer sees a write past it)
    std::vector<int32_t> tab(2 * rows.size() + 1 + 2 * m, -77), expect(rows);
    expect.insert(expect.end(), off.begin(), off.end());
    expect.insert(expect.end(), row_of_place.begin(), row_of_place.end());
    expect.insert(expect.end(), m, -77);
    if (t.write(tab.data()) != tab.data() + 2 * rows.size() + 1 + m) return bad("where the call's own column begins");
    if (tab != expect) return bad("the table written");
    return true;
}

static bool check_tables(const std::string& name, const std::vector<int32_t>& query, const std::vector<int64_t>& key = {})
{
    return check_tables(name, query, false, {}, false, {}) && (key.empty() || check_tables(name + ", keyed", query, false, {}, true, key));
}

// names: the list (by_base false), or base + 0 .. n - 1; every probe against a linear search
static bool check_names(const std::string& name, bool by_base, const std::vector<int64_t>& names, int64_t n, int64_t base, const std::vector<int64_t>& probes)
{
    ++g_cases;
    const ColumnNames c{by_base ? nullptr : names.data(), by_base ? n : (int64_t)names.size(), base};
    for (const int64_t p : probes) {
        int64_t find = -1, lower = 0;
        for (int64_t v = c.n - 1; v >= 0; --v) {
            const int64_t nm = by_base ? base + v : names[(size_t)v];
            if (c.name(v) != nm) { printf("target_tables_check: %s: name(%lld)\n", name.c_str(), (long long)v); return false; }
            if (nm == p) find = v;
            if (nm < p) ++lower;
        }
        if (c.find(p) != find || c.lower(p) != lower) {
            printf("target_tables_check: %s: probe %lld: find %lld (want %lld), lower %lld (want %lld)\n", name.c_str(), (long long)p, (long long)c.find(p), (long long)find,
                   (long long)c.lower(p), (long long)lower);
            return false;
        }
    }
    return true;
}

int main()
{
    std::mt19937 rng(20261021u);
    bool ok = true;
    // ---- the tables
    ok &= check_tables("no targets", {});
    ok &= check_tables("no targets of a device list", {3, 1}, true, {}, false, {});
    ok &= check_tables("one target", {4}, {9});
    ok &= check_tables("every target in one row", {2, 2, 2, 2, 2}, {5, 1, 4, 1, 0});
    ok &= check_tables("every row exactly one target", {0, 1, 2, 3, 4, 5}, {6, 5, 4, 3, 2, 1});
    ok &= check_tables("repeated (row, key) pairs", {1, 0, 1, 0, 1, 1}, {8, 3, 8, 3, 2, 8});        // equal pairs keep the caller's order
    ok &= check_tables("rows given in descending order", {8, 8, 5, 3, 3, 0}, {1, 0, 7, 2, 2, 9});
    ok &= check_tables("a device list that skips targets", {3, 0, 3, 1, 0, 3, 2}, true, {0, 2, 4, 5}, false, {});
    ok &= check_tables("a device list that skips targets, keyed", {3, 0, 3, 1, 0, 3, 2}, true, {0, 2, 4, 5}, true, {9, 0, 1, 0, 5, 1, 0});
    ok &= check_tables("a device list of the last target alone", {3, 0, 3}, true, {2}, false, {});
    ok &= check_tables("keys at the ends of int64", {0, 0, 0}, {INT64_MAX, INT64_MIN, 0});
    for (int it = 0; it < 400 && ok; ++it) {
        const size_t n = rng() % 65;
        const uint32_t n_rows = 1 + rng() % 9, n_keys = 1 + rng() % 6;
        std::vector<int32_t> query(n), dev;
        std::vector<int64_t> key(n);
        for (size_t i = 0; i < n; ++i) { query[i] = (int32_t)(rng() % n_rows); key[i] = (int64_t)(rng() % n_keys); if (rng() % 3) dev.push_back((int32_t)i); }
        ok &= check_tables("random " + std::to_string(it), query, it % 2 == 1, dev, it % 4 >= 2, key);
    }
    // ---- the names
    const std::vector<int64_t> sorted{3, 4, 9, 10, 40, 1000000000000};
    ok &= check_names("a sorted list: its first and last element, absent names, both sides", false, sorted, 0, 0, {3, 1000000000000, 0, 2, 5, 11, 39, 41, 999999999999, 1000000000001, 9, 10});
    ok &= check_names("a sorted list of one", false, {7}, 0, 0, {6, 7, 8, 0});
    ok &= check_names("an empty name list", false, {}, 0, 0, {0, 1, 5});
    ok &= check_names("positions of a shard: below base, base, the last, base + n, beyond", true, {}, 5, 1000, {0, 999, 1000, 1002, 1004, 1005, 1006, 99999});
    ok &= check_names("positions from 0", true, {}, 3, 0, {0, 1, 2, 3, 4});
    ok &= check_names("no position", true, {}, 0, 10, {0, 9, 10, 11});
    for (int it = 0; it < 200 && ok; ++it) {
        std::vector<int64_t> names, probes;
        int64_t v = (int64_t)(rng() % 5);
        for (size_t i = rng() % 40; i > 0; --i) { names.push_back(v); v += 1 + (int64_t)(rng() % 4); }
        for (int i = 0; i < 30; ++i) probes.push_back((int64_t)(rng() % (uint32_t)(v + 3)));
        ok &= it % 2 ? check_names("random list " + std::to_string(it), false, names, 0, 0, probes)
                     : check_names("random positions " + std::to_string(it), true, {}, (int64_t)names.size(), (int64_t)(rng() % 20), probes);
    }
    if (!ok) return 1;
    printf("target_tables_check: %d cases ok\n", g_cases);
    return 0;
}
