// afis_link.cpp — link groups of the C ABI (include/afis_matcher.h): afis_link_groups and afis_link_subject_groups return the connected components — of two or more
// nodes — of the graph the last search's matrix makes of its rows and columns above a decision score: which enrolled prints, or persons, are one finger or person
// (a print search), which latents hit the same print or person (a latent search).  The definitions (a cell that reaches, the nodes, an edge under either mode, the
// groups and their order, the union and its bound) are link_groups.h's.  A matrix call (MatrixCall, afis_ctx.h) whose kernels are link_groups.hip's.  In the subject form
// the exclusions name persons: where a filtered subject list drops them from a row's maxima, the scan drops them from the row's cells (sorted (row, slot) keys, looked
// up only where a cell reaches).  The counts return first, then — a second copy and a second bounded wait, here — only the (node, label) pairs of the linked nodes: what
// crosses PCIe is 32 bytes + 8 per linked node, whatever G is; the matrix may be normalised.  link_arrange puts the pairs into the caller's CSR.
// The call's device words, ctx->link_tab, every area on a 256-byte boundary:
//   counters (n_edges u64 | n_pairs u32 | err u32 | 16 spare bytes) | parent [n_nodes] | label [n_nodes] | size [n_nodes] | the subject form in mutual mode: first_col
//   [S] | the tables, ONE upload: row_node [n_q] | mutual mode: first_row [n_nodes] | col_of_row [n_q] (the template form's; the subject form's is made on the device) |
//   on an 8-byte boundary the subject form's exclusion keys
// ctx->link_out: the pairs, [n_nodes][2] int32 at most.
#include "afis_ctx.h"
#include "link_groups.h"

using namespace afis;

static_assert(kLinkAny == AFIS_LINK_ANY && kLinkMutual == AFIS_LINK_MUTUAL, "link_groups.h holds the modes of include/afis_matcher.h");

namespace afis {

constexpr size_t kLinkCounterBytes = 32;

// both entry points behind their checks (subj == NULL: the templates); pairs: the exclusions as check_filtered resolved them — (row, column), or (row, slot)
static int link_groups(afis_ctx* ctx, const char* who, const afis_subjects* subj, const afis_labels* labels, const uint64_t* masks, const std::vector<int32_t>& pairs, int n_q,
                       const int64_t* row_node, float min_score, int mode, int64_t cap_groups, int64_t cap_members, int64_t* n_edges, int64_t* n_groups, int64_t* n_members,
                       int64_t* n_listed, int64_t* group_off, int64_t* member)
{
    const LastSearch ls = ctx->last_search;
    const int64_t G = ls.G;
    *n_edges = *n_groups = *n_members = *n_listed = 0;
    group_off[0] = 0;
    if (n_q == 0 || G == 0) return AFIS_OK;                                 // no cell: no edge, no device work

    // ---- the node tables
    const LinkColumns cols = column_names(ctx, subj);
    LinkNodes nodes;
    if (!link_build_nodes(cols, row_node, n_q, nodes)) return fail(ctx, AFIS_EINVAL, std::string(who) + ": more than 2^31 - 1 nodes");
    const bool mutual = mode == kLinkMutual;
    const size_t nn = (size_t)nodes.n_nodes, n_first = subj && mutual ? (size_t)subj->S : 0;
    std::vector<uint64_t> keys;                                             // the subject form's exclusions, sorted
    if (subj) {
        keys.resize(pairs.size() / 2);
        for (size_t i = 0; i < keys.size(); ++i) keys[i] = ((uint64_t)(uint32_t)pairs[2 * i] << 32) | (uint32_t)pairs[2 * i + 1];
        std::sort(keys.begin(), keys.end());
    }
    const size_t tab_ints = (size_t)n_q + (mutual ? nn + (size_t)n_q : 0), keys_at_rel = (tab_ints * 4 + 7) / 8 * 8, tab_bytes = keys_at_rel + keys.size() * 8;
    std::vector<uint8_t> tab(tab_bytes, 0);
    {
        int32_t* const t = (int32_t*)tab.data();
        std::copy(nodes.row_node.begin(), nodes.row_node.end(), t);
        if (mutual) {
            std::copy(nodes.first_row.begin(), nodes.first_row.end(), t + n_q);
            for (int q = 0; q < n_q; ++q) t[(size_t)n_q + nn + (size_t)q] = nodes.row_node[(size_t)q] < nodes.n_col ? nodes.row_node[(size_t)q] : -1;   // the template form: a column node is its position
        }
        if (!keys.empty()) memcpy(tab.data() + keys_at_rel, keys.data(), keys.size() * 8);
    }

    // ---- the device: the counters' memset, the scan and the labels
    const size_t parent_at = up256(kLinkCounterBytes), label_at = parent_at + up256(nn * 4), size_at = label_at + up256(nn * 4), first_at = size_at + up256(nn * 4),
                 tab_at = first_at + up256(n_first * 4), total = tab_at + tab_bytes, pin_bytes = kLinkCounterBytes + nn * 8;
    const std::vector<int32_t> no_cells;                                    // the subject form's exclusions are not cells of the copy
    MatrixCall mc{ctx, who, subj, kTemplateCells, {ctx, labels, masks, subj ? no_cells : pairs, subj != nullptr}};   // (the template cells in either form: FilterPass drops no cell for a person)
    AFISCHK(mc.room({{&ctx->link_tab, total}, {&ctx->link_out, std::max<size_t>(nn * 8, 16)}}, pin_bytes));
    hipStream_t s = ctx->stream;
    uint8_t* const d = ctx->link_tab.as<uint8_t>();
    AFISCHK(mc.begin({{d + tab_at, tab.data(), tab_bytes}}));
    HIPCHK(ctx, hipMemsetAsync(d, 0, kLinkCounterBytes, s));
    const int32_t* const d_tab = (const int32_t*)(d + tab_at);
    int32_t* const d_col_of_row = mutual ? (int32_t*)(d + tab_at) + (size_t)n_q + nn : nullptr;
    LinkScan scan{};
    scan.thr = rank_key(min_score); scan.n_nodes = nodes.n_nodes;
    scan.row_node = d_tab; scan.first_row = mutual ? d_tab + n_q : nullptr; scan.col_of_row = d_col_of_row;
    scan.slot_of = subj ? subj->d_slot_of.as<int32_t>() : nullptr; scan.d_global = subj ? global_map(ls) : nullptr; scan.index_base = (long long)ctx->index_base;
    scan.excl = keys.empty() ? nullptr : (const u64*)(d + tab_at + keys_at_rel); scan.n_excl = keys.size();
    scan.parent = (int32_t*)(d + parent_at); scan.n_edges = (u64*)d; scan.err = (uint32_t*)(d + 12);
    HIPCHK(ctx, launch_link_groups(mc.fp.matrix(), n_q, (int)G, scan, (int32_t*)(d + label_at), (int32_t*)(d + size_at), n_first ? (int32_t*)(d + first_at) : nullptr, (int32_t)n_first,
                                   n_first ? d_col_of_row : nullptr, (uint32_t*)(d + 8), ctx->link_out.as<int32_t>(), s));
    AFISCHK(mc.finish(d, kLinkCounterBytes, &ctx->link_groups_us));         // the counts first
    ctx->link_d2h_bytes = (int64_t)kLinkCounterBytes;
    uint8_t* const pin = (uint8_t*)ctx->h_pin; uint64_t edges; uint32_t n_pairs, err;
    memcpy(&edges, pin, 8); memcpy(&n_pairs, pin + 8, 4); memcpy(&err, pin + 12, 4);
    if (err || (size_t)n_pairs > nn) return fail(ctx, AFIS_EDEVICE, std::string(who) + ": the union did not settle (a step bound of link_groups.h was reached); the matrix is as it was");
    if (n_pairs) {                                                          // ... then only the linked nodes
        HIPCHK(ctx, hipMemcpyAsync(pin + kLinkCounterBytes, ctx->link_out.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, s));
        { const int rcw = wait_streams(ctx, {s}, who); if (rcw != AFIS_OK) { ctx->last_search.valid = false; return rcw; } }
        ctx->link_d2h_bytes += (int64_t)n_pairs * 8;
    }
    const LinkCounts c = link_arrange(cols, nodes, (const int32_t*)(pin + kLinkCounterBytes), (int64_t)n_pairs, cap_groups, cap_members, group_off, member);
    *n_edges = (int64_t)edges; *n_groups = c.n_groups; *n_members = c.n_members; *n_listed = c.n_listed;
    return AFIS_OK;
}

// the checks of both entry points: the plain arguments, then the filtered ranking calls', then the rows' names
static int link_entry(afis_ctx* ctx, const char* who, afis_subjects* s, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl, int n_q,
                      const int64_t* row_node, float min_score, int mode, int64_t cap_groups, int64_t cap_members, int64_t* n_edges, int64_t* n_groups, int64_t* n_members,
                      int64_t* n_listed, int64_t* group_off, int64_t* member)
{
    const std::string w(who);
    if (s) AFISCHK(check_subject_handle(ctx, who, s));
    if (mode != AFIS_LINK_ANY && mode != AFIS_LINK_MUTUAL) return fail(ctx, AFIS_EINVAL, w + ": mode must be AFIS_LINK_ANY (0) or AFIS_LINK_MUTUAL (1)");
    if (std::isnan(min_score)) return fail(ctx, AFIS_EINVAL, w + ": min_score must be a number");
    if (cap_groups < 0 || cap_members < 0) return fail(ctx, AFIS_EINVAL, w + ": a cap is negative");
    if (!n_edges || !n_groups || !n_members || !n_listed || !group_off || (cap_members > 0 && !member)) return fail(ctx, AFIS_EINVAL, w + ": an output is null");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, s, labels, masks, excl_off, excl, n_q, min_score, 1, true, pairs));
    if (row_node) for (int q = 0; q < n_q; ++q) if (row_node[q] < -1) return fail(ctx, AFIS_EINVAL, w + ": a row_node is below -1");
    return link_groups(ctx, who, s, labels, masks, pairs, n_q, row_node, min_score, mode, cap_groups, cap_members, n_edges, n_groups, n_members, n_listed, group_off, member);
}

}  // namespace afis

extern "C" {

int afis_link_groups(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl, int n_q, const int64_t* row_node, float min_score,
                     int mode, int64_t cap_groups, int64_t cap_members, int64_t* n_edges, int64_t* n_groups, int64_t* n_members, int64_t* n_listed, int64_t* group_off, int64_t* member)
{
    if (!ctx) return fail(ctx, AFIS_EINVAL, "afis_link_groups: null argument");
    ctx->link_groups_us = 0; ctx->link_d2h_bytes = 0;
    return link_entry(ctx, "afis_link_groups", nullptr, labels, masks, excl_off, excl, n_q, row_node, min_score, mode, cap_groups, cap_members, n_edges, n_groups, n_members, n_listed,
                      group_off, member);
}

int afis_link_subject_groups(afis_ctx* ctx, afis_subjects* s, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl_subject, int n_q,
                             const int64_t* row_node, float min_score, int mode, int64_t cap_groups, int64_t cap_members, int64_t* n_edges, int64_t* n_groups, int64_t* n_members,
                             int64_t* n_listed, int64_t* group_off, int64_t* member)
{
    if (ctx) { ctx->link_groups_us = 0; ctx->link_d2h_bytes = 0; }
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, "afis_link_subject_groups: null argument");
    return link_entry(ctx, "afis_link_subject_groups", s, labels, masks, excl_off, excl_subject, n_q, row_node, min_score, mode, cap_groups, cap_members, n_edges, n_groups, n_members,
                      n_listed, group_off, member);
}

}  // extern "C"
