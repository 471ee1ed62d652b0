// link_groups.h — link groups: the connected components of the graph a score matrix makes of its rows and columns, defined once for the host and the device.
// Standard library only (score_order.h is): usable from g++ alone.  The kernels (link_groups.hip), the host unit (afis_link.cpp) and the check program
// (link_groups_check.cpp) share this text.
//
// CELLS.  A cell (word w) is an ENTRY exactly as in score_hist.h: rank_key(w) >= kLinkEntryFloor, the key of -inf.  The no-entry word 0xffffffff and every other NaN
// with the sign set lie below it and are never an edge.  A cell REACHES when rank_key(w) >= rank_key(min_score): afis_rank_hits' decision and its + 0.0f, so the two
// zeros are one value.  min_score is a number, so a cell that reaches is an entry.
// NODES.  Every column is a node: in the template form its name is its global template index, in the subject form the subject id of its template — all columns of one
// person are ONE node.  Row q is the node row_node[q] names — a global template index, or a subject id — or, at -1, a node of its own (a latent), reported as -1 - q.  A
// named row whose name is a column's name IS that column's node (a print search's identity between a row and its own column); a named row that matches no column — a
// print outside the subset's columns, a person the handle does not hold, a print of another rank — is a node with that name; several rows with one name are one node.
// EDGES, cell by cell.  kLinkAny: cell (q, c) is an edge when it reaches and row q and column c are different nodes.  kLinkMutual: and the REVERSE cell reaches too: the
// cell in the first row whose node is c's node, at the column of row q's print.  In the template form that column is the one whose name is row_node[q].  In the subject
// form row_node names only a person: the column is the FIRST column, in ascending position of the matrix as the device holds it (ascending global template index),
// whose node is q's node — a reverse cell at another print of the same person is not seen.  Where no such row or no such column exists in this matrix the cell is not an
// edge: it cannot be confirmed here.  The reverse cell is read from the same matrix, filtered or not, as the forward cell.  A cell between a node and itself is never an
// edge and never counted: a print against itself, two prints of one person, a repeated query print.  n_edges counts the cells that are edges: a mutual pair counts twice.
// GROUPS.  The connected components of that graph with at least two nodes.  The order of nodes: named nodes by ascending name, then anonymous rows by ascending q; a
// group's members stand in that order and the groups are ordered by their first member.  Every edge has a column at one end, so a group holds a named node.
// DETERMINISM.  The result is a function of the matrix and the arguments: the union below always hangs the greater root under the smaller one, so whatever order the
// device meets the edges in, the root of a component is its smallest node number; the host orders names.  No float is added anywhere.
//
// NODE NUMBERS (the device's int32): the column nodes first — position p of the matrix in the template form, slot s of the subject handle in the subject form (a slot no
// column of this matrix covers is a node without edges) —, then the named rows that are no column node by ascending name, then the anonymous rows by ascending q.
//
// THE UNION is a lock-free union-find over parent[n_nodes]: a non-root's parent is SMALLER than the node, so no cycle can form and every walk ends.  link_find walks
// to a root and halves the path (lower(): a pointer is only ever lowered, a late writer cannot raise it); link_unite hooks the greater of two roots under the smaller by
// compare-and-swap on the greater root.  Both take the memory through an accessor — atomics of agent scope on the device, plain words in the check program's sequential
// rendering — and a step budget.  THE BOUND: every step of a walk lowers the walker's node by at least one, so the walks of one link_unite from u and v together take fewer
// than u + v < 2 n_nodes steps however the other threads move; a hook fails only where another hook has just taken that root, which is then no root, so the next walk
// takes at least one step: failed hooks <= steps.  4 n_nodes + 4 is never reached by a correct run; a run that reaches it reports false and the caller raises the
// device's error word (AFIS_EDEVICE: the union did not settle) instead of spinning.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "column_names.h"
#include "score_order.h"

namespace afis {

constexpr uint32_t kLinkEntryFloor = 0x007fffffu;                           // rank_key(-inf): score_hist.h's kEntryFloor
constexpr int kLinkAny = 0, kLinkMutual = 1;                                // AFIS_LINK_ANY, AFIS_LINK_MUTUAL

AFIS_ORDER_FN bool link_reaches(uint32_t w, uint32_t thr_key) { return rank_key(__builtin_bit_cast(float, w)) >= thr_key; }
AFIS_ORDER_FN int64_t link_budget(int32_t n_nodes) { return 4 * (int64_t)n_nodes + 4; }

// the root above x, the path halved on the way; -1 where the budget ran out
template <class A>
AFIS_ORDER_FN int32_t link_find(A& a, int32_t x, int64_t* budget)
{
    for (;;) {
        const int32_t p = a.load(x);
        if (p == x) return x;
        const int32_t g = a.load(p);
        if (g != p) a.lower(x, g);
        x = g;                                                              // (g <= p < x: every trip lowers x)
        if (--*budget < 0) return -1;
    }
}

// u and v into one tree; false where the budget ran out
template <class A>
AFIS_ORDER_FN bool link_unite(A& a, int32_t u, int32_t v, int64_t budget)
{
    for (;;) {
        u = link_find(a, u, &budget);
        if (u < 0) return false;
        v = link_find(a, v, &budget);
        if (v < 0) return false;
        if (u == v) return true;
        const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
        if (a.hook(hi, lo)) return true;                                    // (lo may have stopped being a root meanwhile: it is smaller and in its tree, which is all a parent must be)
        if (--budget < 0) return false;
    }
}

// after every union, no writer left: the root above v by plain reads; -1 where the walk is longer than the node count (it cannot be)
AFIS_ORDER_FN int32_t link_root(const int32_t* parent, int32_t v, int32_t n_nodes)
{
    for (int32_t steps = 0; steps <= n_nodes; ++steps) {
        const int32_t p = parent[v];
        if (p == v) return v;
        v = p;
    }
    return -1;
}

// ---- the host half: node tables, and the arrangement of what the device returns ---------------------------------------------------------------------------

// the accessor of the sequential rendering
struct LinkSeq {
    int32_t* parent;
    int32_t load(int32_t i) const { return parent[i]; }
    void lower(int32_t i, int32_t v) { if (v < parent[i]) parent[i] = v; }
    bool hook(int32_t hi, int32_t lo) { if (parent[hi] != hi) return false; parent[hi] = lo; return true; }
};

using LinkColumns = ColumnNames;                                            // the names of the column nodes, ascending and distinct (column_names.h)

struct LinkNodes {
    int32_t n_col = 0, n_nodes = 0;
    std::vector<int64_t> extra;                                             // the names of the nodes n_col .. : named rows that are no column node, ascending
    std::vector<int32_t> anon;                                              // the rows of the nodes n_col + extra.size() .. : ascending
    std::vector<int32_t> row_node;                                          // [n_q] the node of row q
    std::vector<int32_t> first_row;                                         // [n_nodes] the first row whose node this is, -1: none (mutual mode's reverse row)
    int64_t name(const LinkColumns& cols, int32_t v) const
    {
        if (v < n_col) return cols.name(v);
        const size_t e = (size_t)(v - n_col);
        return e < extra.size() ? extra[e] : -1 - (int64_t)anon[e - extra.size()];
    }
    // where a node stands in the output order: named nodes by name (names are >= 0), then the anonymous rows
    uint64_t order_key(const LinkColumns& cols, int32_t v) const { const int64_t nm = name(cols, v); return nm >= 0 ? (uint64_t)nm : ((uint64_t)1 << 63) | (uint64_t)(-1 - nm); }
};

// row_node [n_q] (NULL: every row anonymous; entries >= -1) over the columns cols -> the node numbering above; false: more than 2^31 - 1 nodes
inline bool link_build_nodes(const LinkColumns& cols, const int64_t* row_node, int n_q, LinkNodes& out)
{
    out = LinkNodes();
    out.row_node.assign((size_t)n_q, -1);
    for (int q = 0; q < n_q; ++q) {
        const int64_t nm = row_node ? row_node[q] : -1;
        if (nm < 0) out.anon.push_back(q);
        else if (cols.find(nm) < 0) out.extra.push_back(nm);
    }
    std::sort(out.extra.begin(), out.extra.end());
    out.extra.erase(std::unique(out.extra.begin(), out.extra.end()), out.extra.end());
    const int64_t total = cols.n + (int64_t)out.extra.size() + (int64_t)out.anon.size();
    if (total > (int64_t)INT32_MAX) return false;
    out.n_col = (int32_t)cols.n; out.n_nodes = (int32_t)total;
    size_t a = 0;
    for (int q = 0; q < n_q; ++q) {
        const int64_t nm = row_node ? row_node[q] : -1;
        int64_t v;
        if (nm < 0) v = cols.n + (int64_t)out.extra.size() + (int64_t)a++;
        else if ((v = cols.find(nm)) < 0) v = cols.n + (int64_t)(std::lower_bound(out.extra.begin(), out.extra.end(), nm) - out.extra.begin());
        out.row_node[(size_t)q] = (int32_t)v;
    }
    out.first_row.assign((size_t)out.n_nodes, -1);
    for (int q = n_q - 1; q >= 0; --q) out.first_row[(size_t)out.row_node[(size_t)q]] = q;
    return true;
}

struct LinkCounts { int64_t n_groups, n_members, n_listed; };

// The (node, label) pairs of the nodes in groups of two or more, in any order — label: the same for the members of one group — arranged into the CSR: every group's
// members in the output order, the groups ordered by their first member.  The lists hold the longest prefix of the groups that fits both caps: group_off [cap_groups
// + 1] (group_off[0 .. n_listed] is written), member [cap_members].
inline LinkCounts link_arrange(const LinkColumns& cols, const LinkNodes& nodes, const int32_t* pairs, int64_t n_pairs, int64_t cap_groups, int64_t cap_members,
                               int64_t* group_off, int64_t* member)
{
    struct M { int32_t label; uint64_t key; int64_t name; };
    std::vector<M> m((size_t)n_pairs);
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int32_t v = pairs[2 * i];
        m[(size_t)i] = M{pairs[2 * i + 1], nodes.order_key(cols, v), nodes.name(cols, v)};
    }
    std::sort(m.begin(), m.end(), [](const M& x, const M& y) { return x.label != y.label ? x.label < y.label : x.key < y.key; });
    struct Grp { uint64_t first_key; size_t at, n; };
    std::vector<Grp> g;
    for (size_t i = 0; i < m.size(); ++i) {
        if (i == 0 || m[i].label != m[i - 1].label) g.push_back(Grp{m[i].key, i, 0});
        ++g.back().n;
    }
    std::sort(g.begin(), g.end(), [](const Grp& x, const Grp& y) { return x.first_key < y.first_key; });
    LinkCounts c{(int64_t)g.size(), n_pairs, 0};
    int64_t at = 0;
    group_off[0] = 0;
    for (const Grp& x : g) {
        if (c.n_listed >= cap_groups || at + (int64_t)x.n > cap_members) break;
        for (size_t i = 0; i < x.n; ++i) member[at++] = m[x.at + i].name;
        group_off[++c.n_listed] = at;
    }
    return c;
}
}  // namespace afis
