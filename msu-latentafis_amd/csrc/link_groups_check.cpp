// link_groups_check.cpp — the host half of link_groups.h as a program of its own, built with the host sanitizers (Makefile: link_groups_check) and run directly by
// tests/test_link_groups_host.py.  Without arguments it checks, and returns 1 with a line on stderr at the first answer that is wrong:
//   nodes     link_build_nodes: covered and uncovered names, repeated names, anonymous rows, the subject form (ids as the columns' names), a subset's sorted list
//   arrange   link_arrange: the order of members and of groups, both caps, n_listed, a prefix that stops at either cap, caps of 0
//   union     a sequential rendering of the device's steps (link_find, link_unite over LinkSeq, then link_root) against a breadth-first labelling: random graphs in
//             random edge orders, a path in ascending and in descending order, a star, a complete bipartite graph; the root of a component is its smallest node, and the
//             step budget is never reached
// With the argument "arrange" it reads from stdin, every number in decimal, `n_col base n_q row_node[n_q] n_pairs (node label)[n_pairs] cap_groups cap_members` and
// prints n_groups n_members n_listed, group_off[0 .. n_listed] and the members: the test holds that against its Python model.
#include "link_groups.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <queue>
#include <random>
#include <utility>

using namespace afis;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "link_groups_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

typedef std::vector<std::pair<int32_t, int32_t>> Edges;

static std::vector<int32_t> bfs_labels(int32_t n, const Edges& e)
{
    std::vector<std::vector<int32_t>> adj((size_t)n);
    for (const auto& x : e) { adj[(size_t)x.first].push_back(x.second); adj[(size_t)x.second].push_back(x.first); }
    std::vector<int32_t> lab((size_t)n, -1);
    for (int32_t s = 0; s < n; ++s) {                                       // ascending: a component's label is its smallest node
        if (lab[(size_t)s] >= 0) continue;
        std::queue<int32_t> q;
        q.push(s); lab[(size_t)s] = s;
        while (!q.empty()) {
            const int32_t v = q.front(); q.pop();
            for (int32_t w : adj[(size_t)v]) if (lab[(size_t)w] < 0) { lab[(size_t)w] = s; q.push(w); }
        }
    }
    return lab;
}

static int check_union(int32_t n, const Edges& e)
{
    std::vector<int32_t> parent((size_t)n);
    for (int32_t v = 0; v < n; ++v) parent[(size_t)v] = v;
    LinkSeq acc{parent.data()};
    for (const auto& x : e) {
        CHECK(link_unite(acc, x.first, x.second, link_budget(n)));
        for (int32_t v = 0; v < n; ++v) CHECK(parent[(size_t)v] <= v);      // pointers only ever point down
    }
    const std::vector<int32_t> want = bfs_labels(n, e);
    for (int32_t v = 0; v < n; ++v) CHECK(link_root(parent.data(), v, n) == want[(size_t)v]);
    return 0;
}

static int check_unions()
{
    std::mt19937 rng(7411);
    for (int rep = 0; rep < 200; ++rep) {
        const int32_t n = 1 + (int32_t)(rng() % 300);
        Edges e(rng() % (2 * (unsigned)n + 1));
        for (auto& x : e) x = {(int32_t)(rng() % (unsigned)n), (int32_t)(rng() % (unsigned)n)};   // (self loops among them: link_unite returns at once)
        if (check_union(n, e)) return 1;
    }
    const int32_t n = 2049;
    Edges path, back, star, bip;
    for (int32_t i = 0; i + 1 < n; ++i) { path.push_back({i, i + 1}); back.push_back({n - 2 - i, n - 1 - i}); star.push_back({i + 1, 777}); }
    for (int32_t a = 0; a < 40; ++a) for (int32_t b = 40; b < 100; ++b) bip.push_back({b, a});
    if (check_union(n, path) || check_union(n, back) || check_union(n, star) || check_union(100, bip)) return 1;
    std::shuffle(path.begin(), path.end(), rng);
    if (check_union(n, path)) return 1;
    // a budget that is too small is reported, not spun on
    std::vector<int32_t> parent = {0, 0, 1, 2, 3, 4, 5, 6};
    LinkSeq acc{parent.data()};
    CHECK(!link_unite(acc, 7, 0, 1));
    CHECK(link_unite(acc, 7, 0, link_budget(8)) && link_root(parent.data(), 7, 8) == 0);
    const int32_t cyc[2] = {1, 0};                                          // what cannot happen: link_root ends all the same
    CHECK(link_root(cyc, 0, 2) == -1);
    return 0;
}

static int check_nodes()
{
    {   // the template form over a full shard: names base + p; a print search with a repeated print, a latent, a print of another rank, a print below the base
        const LinkColumns cols{nullptr, 5, 1000};
        const int64_t row_node[] = {1002, -1, 1000, 2000, 1002, -1, 999, 2000, 1004};
        LinkNodes nd;
        CHECK(link_build_nodes(cols, row_node, 9, nd));
        CHECK(nd.n_col == 5 && nd.n_nodes == 5 + 2 + 2);
        CHECK((nd.extra == std::vector<int64_t>{999, 2000}) && (nd.anon == std::vector<int32_t>{1, 5}));
        CHECK((nd.row_node == std::vector<int32_t>{2, 7, 0, 6, 2, 8, 5, 6, 4}));
        CHECK((nd.first_row == std::vector<int32_t>{2, -1, 0, -1, 8, 6, 3, 1, 5}));
        CHECK(nd.name(cols, 3) == 1003 && nd.name(cols, 5) == 999 && nd.name(cols, 6) == 2000 && nd.name(cols, 7) == -2 && nd.name(cols, 8) == -6);
        CHECK(nd.order_key(cols, 5) < nd.order_key(cols, 0) && nd.order_key(cols, 4) < nd.order_key(cols, 6) && nd.order_key(cols, 6) < nd.order_key(cols, 7) &&
              nd.order_key(cols, 7) < nd.order_key(cols, 8));
    }
    {   // a NULL row_node: every row anonymous
        const LinkColumns cols{nullptr, 3, 0};
        LinkNodes nd;
        CHECK(link_build_nodes(cols, nullptr, 4, nd));
        CHECK(nd.n_nodes == 7 && nd.extra.empty() && (nd.row_node == std::vector<int32_t>{3, 4, 5, 6}) && nd.name(cols, 6) == -4 && nd.first_row[2] == -1 && nd.first_row[5] == 2);
    }
    {   // the subject form, and a subset's list: the columns' names are a sorted list
        const int64_t ids[] = {7, 20, 21, 400};
        const LinkColumns cols{ids, 4, 0};
        const int64_t row_node[] = {400, 8, 7, -1, 8, 21};
        LinkNodes nd;
        CHECK(link_build_nodes(cols, row_node, 6, nd));
        CHECK(cols.find(20) == 1 && cols.find(19) == -1 && cols.find(401) == -1);
        CHECK(nd.n_nodes == 6 && (nd.extra == std::vector<int64_t>{8}) && (nd.row_node == std::vector<int32_t>{3, 4, 0, 5, 4, 2}));
        CHECK(nd.name(cols, 1) == 20 && nd.name(cols, 4) == 8 && nd.name(cols, 5) == -4 && nd.first_row[4] == 1 && nd.first_row[1] == -1);
    }
    {   // no rows, no columns
        const LinkColumns cols{nullptr, 0, 0};
        LinkNodes nd;
        CHECK(link_build_nodes(cols, nullptr, 0, nd) && nd.n_nodes == 0 && nd.first_row.empty());
    }
    return 0;
}

static int check_arrange()
{
    const LinkColumns cols{nullptr, 6, 100};
    const int64_t row_node[] = {-1, 50, -1, 103};
    LinkNodes nd;
    CHECK(link_build_nodes(cols, row_node, 4, nd));                         // nodes: 0..5 = 100..105, 6 = 50, 7 = row 0, 8 = row 2
    // groups by label: 3 -> {103, 105, row 2}; 0 -> {100, 50, row 0}; 1 -> {101, 104}: in output order {50, 100, -1}, {101, 104}, {103, 105, -3}
    const int32_t pairs[] = {8, 3, 4, 1, 0, 0, 5, 3, 7, 0, 6, 0, 3, 3, 1, 1};
    const int64_t want_member[] = {50, 100, -1, 101, 104, 103, 105, -3}, want_off[] = {0, 3, 5, 8};
    struct Case { int64_t cg, cm, listed; } const cases[] = {{3, 8, 3}, {10, 100, 3}, {0, 0, 0}, {2, 8, 2}, {3, 7, 2}, {3, 4, 1}, {3, 2, 0}, {1, 8, 1}, {0, 8, 0}, {3, 0, 0}, {3, 5, 2}};
    for (const Case& c : cases) {
        std::vector<int64_t> off((size_t)c.cg + 1, -7), mem((size_t)c.cm, -7);   // exactly the caps: a write past them is the sanitizer's to find
        const LinkCounts got = link_arrange(cols, nd, pairs, 8, c.cg, c.cm, off.data(), mem.data());
        CHECK(got.n_groups == 3 && got.n_members == 8 && got.n_listed == c.listed);
        for (int64_t g = 0; g <= got.n_listed; ++g) CHECK(off[(size_t)g] == want_off[g]);
        for (int64_t i = 0; i < want_off[got.n_listed]; ++i) CHECK(mem[(size_t)i] == want_member[i]);
        for (size_t g = (size_t)got.n_listed + 1; g < off.size(); ++g) CHECK(off[g] == -7);
        for (size_t i = (size_t)want_off[got.n_listed]; i < mem.size(); ++i) CHECK(mem[i] == -7);
    }
    int64_t off0 = -7;
    const LinkCounts none = link_arrange(cols, nd, nullptr, 0, 0, 0, &off0, nullptr);
    CHECK(none.n_groups == 0 && none.n_members == 0 && none.n_listed == 0 && off0 == 0);
    return 0;
}

static int arrange_from_stdin()
{
    long long n_col, base, n_q, n_pairs, cg, cm;
    if (scanf("%lld %lld %lld", &n_col, &base, &n_q) != 3 || n_col < 0 || n_q < 0) return 1;
    std::vector<int64_t> row_node((size_t)n_q);
    for (int64_t& r : row_node) { long long t; if (scanf("%lld", &t) != 1) return 1; r = t; }
    if (scanf("%lld", &n_pairs) != 1 || n_pairs < 0) return 1;
    std::vector<int32_t> pairs((size_t)n_pairs * 2);
    for (int32_t& p : pairs) { long long t; if (scanf("%lld", &t) != 1) return 1; p = (int32_t)t; }
    if (scanf("%lld %lld", &cg, &cm) != 2 || cg < 0 || cm < 0) return 1;
    const LinkColumns cols{nullptr, n_col, base};
    LinkNodes nd;
    if (!link_build_nodes(cols, row_node.data(), (int)n_q, nd)) return 1;
    std::vector<int64_t> off((size_t)cg + 1), mem((size_t)cm);
    const LinkCounts c = link_arrange(cols, nd, pairs.data(), n_pairs, cg, cm, off.data(), mem.data());
    printf("%" PRId64 " %" PRId64 " %" PRId64 "\n", c.n_groups, c.n_members, c.n_listed);
    for (int64_t g = 0; g <= c.n_listed; ++g) printf("%" PRId64 " ", off[(size_t)g]);
    printf("\n");
    for (int64_t i = 0; i < off[(size_t)c.n_listed]; ++i) printf("%" PRId64 " ", mem[(size_t)i]);
    printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "arrange")) return arrange_from_stdin();
    if (check_nodes() || check_arrange() || check_unions()) return 1;
    printf("link_groups_check: ok\n");
    return 0;
}
