// afis_distribution.cpp — score distributions of the C ABI (include/afis_matcher.h), of templates and of persons: afis_score_histogram counts, per query of the last search (axis 0) or per column
// (axis 1), the entries of the matrix into the bins a list of edges makes — afis_rank_hits_filtered's n_hits for many thresholds in one pass — and afis_entries_at
// returns the entry at a given rank of a query's list, for every rank, not only the first AFIS_HITS_MAX: the inverse of afis_rank_positions.  The definitions (an entry,
// its bin, one digit of the select) are score_hist.h's.  Both are matrix calls (MatrixCall, afis_ctx.h) whose kernels are score_hist.hip's; axis 1 reads the transposed copy
// afis_rank_latent_hits_filtered makes (launch_transpose_scores into ctx->scores_t).  Integer counts only: histograms of disjoint shards add up bit for bit; the matrix may be normalised.
// A subset listed out of order: the sub-shard stands in ascending global index order, so a row's tie rule (ascending position) is the rule on global indices; axis 1's
// histograms are put in the caller's column order here (column_order, afis_normalize.cpp).
// The person forms, afis_subject_score_histogram and afis_subject_entries_at, run through the same two functions with a subject handle, as afis_filter.cpp's hit lists
// do: the cells are the person cells [n_q][S] k_subject_keys makes of ctx->subj_best (queue_subject_keys below; score_cell.h), a column is a slot — the distinct ids
// ascending, so no column order is to be restored — and an edge's key is its raw ordered word.
#include "afis_ctx.h"
#include "score_hist.h"
#include "target_tables.h"

using namespace afis;

static_assert(kHistEdgesMax == AFIS_HIST_EDGES_MAX && kHistCountsMax == AFIS_HIST_COUNTS_MAX, "score_hist.h holds the limits of include/afis_matcher.h");

namespace afis {

hipError_t ensure_subject_keys(afis_ctx* ctx, const afis_subjects* subj)
{
    const size_t cells = (size_t)ctx->last_search.n_q * (size_t)subj->S;
    const hipError_t e = ctx->subj_best.ensure(cells * 8);
    return e != hipSuccess ? e : ctx->subj_keys.ensure(cells * 4);
}

int queue_subject_keys(afis_ctx* ctx, const afis_subjects* subj, FilterPass& fp)
{
    AFISCHK(fp.queue_cells());                                              // neither masks nor exclusions: nothing, and the search's matrix itself is folded
    AFISCHK(queue_subject_best(ctx, subj, fp.matrix()));                    // the maxima of the filtered rows, then the excluded persons: rank_hits_filtered's sequence
    AFISCHK(fp.queue_drop_subjects(subj->S));
    HIPCHK(ctx, launch_subject_keys(ctx->subj_best.as<unsigned long long>(), ctx->last_search.n_q, (int)subj->S, ctx->subj_keys.as<uint32_t>(), ctx->stream));
    return AFIS_OK;
}

// afis_score_histogram (subj == NULL: the matrix's columns) and afis_subject_score_histogram (the handle's slots) behind their checks; keys: the edges as the cells'
// keys; pairs: the exclusions as check_filtered resolved them
static int score_histogram(afis_ctx* ctx, afis_subjects* subj, int axis, const afis_labels* labels, const uint64_t* masks, const std::vector<int32_t>& pairs, const std::vector<uint32_t>& keys,
                           int64_t* counts)
{
    const char* const who = subj ? "afis_subject_score_histogram" : "afis_score_histogram";
    const LastSearch ls = ctx->last_search;
    const int n_q = ls.n_q, n_edges = (int)keys.size();
    const int64_t G = ls.G, cols = subj ? subj->S : G, n_out = axis == 0 ? n_q : cols, n_bins = n_edges + 1;
    const size_t out_bytes = (size_t)n_out * (size_t)n_bins * 8, row_bytes = (size_t)n_bins * 8;
    if (n_q == 0 || G == 0 || cols == 0) {                                  // no cell: no device work
        if (out_bytes) memset(counts, 0, out_bytes);
        return AFIS_OK;
    }
    const std::vector<int32_t> order = axis == 1 && !subj ? column_order(ls) : std::vector<int32_t>();
    MatrixCall mc{ctx, who, subj, subj ? kPersonKeys : kTemplateCells, {ctx, labels, masks, pairs, subj != nullptr}};
    AFISCHK(mc.room({{&ctx->scores_t, axis == 1 ? (size_t)cols * (size_t)n_q * 4 : 0}, {&ctx->hist_tab, out_bytes + keys.size() * 4}}, out_bytes));
    hipStream_t s = ctx->stream;
    uint32_t* const d_keys = (uint32_t*)(ctx->hist_tab.as<uint8_t>() + out_bytes);
    AFISCHK(mc.begin({{d_keys, keys.data(), keys.size() * 4}}));
    const float* cells = subj ? ctx->subj_keys.as<float>() : mc.fp.matrix();   // (4-byte cells either way: the transposition moves words)
    if (axis == 1) { HIPCHK(ctx, launch_transpose_scores(cells, ctx->scores_t.as<float>(), n_q, (int)cols, s)); cells = ctx->scores_t.as<float>(); }
    const int h_rows = axis == 0 ? n_q : (int)cols, h_cols = axis == 0 ? (int)cols : n_q;
    if (subj) HIPCHK(ctx, launch_subject_hist((const uint32_t*)cells, h_rows, h_cols, d_keys, n_edges, ctx->hist_tab.as<unsigned long long>(), s));
    else HIPCHK(ctx, launch_score_hist(cells, h_rows, h_cols, d_keys, n_edges, ctx->hist_tab.as<unsigned long long>(), s));
    AFISCHK(mc.finish(ctx->hist_tab.p, out_bytes, subj ? &ctx->subject_score_histogram_us : &ctx->score_histogram_us));
    const uint8_t* const pin = (const uint8_t*)ctx->h_pin;
    if (order.empty()) memcpy(counts, pin, out_bytes);
    else for (size_t t = 0; t < order.size(); ++t) memcpy((uint8_t*)counts + (size_t)order[t] * row_bytes, pin + t * row_bytes, row_bytes);
    return AFIS_OK;
}

// afis_entries_at (subj == NULL: idx names a template, best_idx unused) and afis_subject_entries_at (idx names a person, best_idx the person's best template) behind
// their checks; pairs: the exclusions as check_filtered resolved them
static int entries_at(afis_ctx* ctx, afis_subjects* subj, const afis_labels* labels, const uint64_t* masks, const std::vector<int32_t>& pairs, int64_t nt, const int32_t* query,
                      const int64_t* rank, int32_t* status, int64_t* idx, float* score, int64_t* best_idx)
{
    const char* const who = subj ? "afis_subject_entries_at" : "afis_entries_at";
    const LastSearch ls = ctx->last_search;
    const int n_q = ls.n_q;
    const int64_t G = ls.G, cols = subj ? subj->S : G;                      // the entries of a row: the matrix's columns, or the handle's slots
    const std::string w(who);
    if (nt > (int64_t)INT32_MAX) return fail(ctx, AFIS_EINVAL, w + ": more than 2^31 - 1 targets");
    for (int64_t i = 0; i < nt; ++i) {
        if (query[i] < 0 || query[i] >= n_q) return fail(ctx, AFIS_EINVAL, w + ": a target's query is outside 0 .. n_q - 1");
        if (rank[i] < 0) return fail(ctx, AFIS_EINVAL, w + ": a target's rank is negative");
    }
    for (int64_t i = 0; i < nt; ++i) { status[i] = AFIS_POS_NO_ENTRY; idx[i] = -1; score[i] = -INFINITY; if (best_idx) best_idx[i] = -1; }   // what holds for every target of an empty shard
    if (nt == 0 || G == 0 || cols == 0) return AFIS_OK;

    // ---- a CSR by row, a row's targets in ascending rank: targets whose entries share their leading digits become neighbours, and the select counts once for them
    const TargetTables tt = build_target_tables(query, nullptr, (size_t)nt, rank);   // tt.order[t]: the caller's target at place t of the CSR
    const size_t m = (size_t)nt, n_rows = tt.rows.size();
    // the tables as two uploads: state = prefix [m] | its spare [m] | remain [m]; tab = rows [n_rows] | off [n_rows + 1] | row [m] | first [m]
    std::vector<int32_t> tab(2 * n_rows + 1 + 2 * m);
    int32_t* const t_first = tt.write(tab.data());
    const uint64_t prefix0 = (uint64_t)0xffffffffu & ~(((uint64_t)1 << (8 * select_position_digits(cols))) - 1);   // the position bytes no entry of a row differs in
    std::vector<uint64_t> state(3 * m, prefix0);
    for (size_t r = 0; r < n_rows; ++r)
        for (int32_t t = tt.off[r]; t < tt.off[r + 1]; ++t) { t_first[t] = tt.off[r]; state[2 * m + (size_t)t] = (uint64_t)rank[tt.order[(size_t)t]]; }

    // ---- the device: the select
    const size_t state_bytes = 3 * m * 8, bins_at = up256(state_bytes), bins_bytes = m * kSelectBins * 8, csr_at = bins_at + bins_bytes, tab_bytes = csr_at + tab.size() * 4;
    const size_t idx_at = 0, best_at = m * 8, score_at = best_at + (subj ? m * 8 : 0), status_at = score_at + m * 4, out_bytes = status_at + m * 4;
    MatrixCall mc{ctx, who, subj, subj ? kPersonKeys : kTemplateCells, {ctx, labels, masks, pairs, subj != nullptr}};
    AFISCHK(mc.room({{&ctx->sel_tab, tab_bytes}, {&ctx->sel_out, out_bytes}}, out_bytes));
    hipStream_t s = ctx->stream;
    uint8_t* const d_tab = ctx->sel_tab.as<uint8_t>(), * const d_out = ctx->sel_out.as<uint8_t>();
    AFISCHK(mc.begin({{d_tab, state.data(), state_bytes}, {d_tab + csr_at, tab.data(), tab.size() * 4}}));
    unsigned long long* const d_prefix = (unsigned long long*)d_tab, * const d_remain = d_prefix + 2 * m;
    const int32_t* const d_rows = (const int32_t*)(d_tab + csr_at), * const d_off = d_rows + n_rows, * const d_row = d_off + n_rows + 1, * const d_first = d_row + m;
    if (subj)
        HIPCHK(ctx, launch_subject_entries_at(ctx->subj_keys.as<uint32_t>(), ctx->subj_best.as<unsigned long long>(), (int)cols, (int)G, d_rows, d_off, (int)n_rows, tt.max_row_targets, d_row,
                                              d_first, m, d_prefix, d_prefix + m, d_remain, (unsigned long long*)(d_tab + bins_at), subj->d_ids.as<long long>(), global_map(ls),
                                              (long long)ctx->index_base, (long long*)(d_out + idx_at), (float*)(d_out + score_at), (long long*)(d_out + best_at),
                                              (int32_t*)(d_out + status_at), s));
    else
        HIPCHK(ctx, launch_entries_at(mc.fp.matrix(), (int)G, d_rows, d_off, (int)n_rows, tt.max_row_targets, d_row, d_first, m, d_prefix, d_prefix + m, d_remain,
                                      (unsigned long long*)(d_tab + bins_at), global_map(ls), (long long)ctx->index_base, (long long*)(d_out + idx_at), (float*)(d_out + score_at),
                                      (int32_t*)(d_out + status_at), s));
    AFISCHK(mc.finish(d_out, out_bytes, subj ? &ctx->subject_entries_at_us : &ctx->entries_at_us));

    // ---- back into the caller's order
    const uint8_t* const pin = (const uint8_t*)ctx->h_pin;
    for (size_t t = 0; t < m; ++t) {
        const size_t i = (size_t)tt.order[t];
        memcpy(idx + i, pin + idx_at + t * 8, 8);
        if (subj) memcpy(best_idx + i, pin + best_at + t * 8, 8);
        memcpy(score + i, pin + score_at + t * 4, 4);
        memcpy(status + i, pin + status_at + t * 4, 4);
    }
    return AFIS_OK;
}

}  // namespace afis

extern "C" {

int afis_score_histogram(afis_ctx* ctx, int axis, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl, int n_q,
                         int n_edges, const float* edges, int64_t* counts)
{
    const char* const who = "afis_score_histogram";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    ctx->score_histogram_us = 0;
    if (axis != 0 && axis != 1) return fail(ctx, AFIS_EINVAL, std::string(who) + ": axis must be 0 (rows) or 1 (columns)");
    if (n_edges < 1 || n_edges > AFIS_HIST_EDGES_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_edges must be in 1 .. AFIS_HIST_EDGES_MAX (1023)");
    std::vector<uint32_t> keys((size_t)n_edges);
    if (edges && hist_edge_keys(edges, n_edges, keys.data()) != 0)
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": no edge may be a NaN, and the edges must ascend strictly (by rank key: the two zeros are one value)");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, nullptr, labels, masks, excl_off, excl, n_q, -INFINITY, 1, true, pairs));
    const int64_t G = ctx->last_search.G, n_out = axis == 0 ? (int64_t)n_q : G;
    if (n_out * (n_edges + 1) > AFIS_HIST_COUNTS_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": more than AFIS_HIST_COUNTS_MAX counts (outputs x (n_edges + 1))");
    if (n_out > 0 && !counts) return fail(ctx, AFIS_EINVAL, std::string(who) + ": counts is null");
    if (n_q > 0 && G > 0 && !edges) return fail(ctx, AFIS_EINVAL, std::string(who) + ": edges is null");
    return score_histogram(ctx, nullptr, axis, labels, masks, pairs, keys, counts);
}

int afis_subject_score_histogram(afis_ctx* ctx, afis_subjects* s, int axis, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl_subject, int n_q,
                                 int n_edges, const float* edges, int64_t* counts)
{
    const char* const who = "afis_subject_score_histogram";
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    ctx->subject_score_histogram_us = 0;
    AFISCHK(check_subject_handle(ctx, who, s));
    if (axis != 0 && axis != 1) return fail(ctx, AFIS_EINVAL, std::string(who) + ": axis must be 0 (queries) or 1 (subjects)");
    if (n_edges < 1 || n_edges > AFIS_HIST_EDGES_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_edges must be in 1 .. AFIS_HIST_EDGES_MAX (1023)");
    std::vector<uint32_t> keys((size_t)n_edges);
    if (edges && hist_edge_keys<PersonCell>(edges, n_edges, keys.data()) != 0)
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": no edge may be a NaN, and the edges must ascend strictly (by ordered word: -0.0 stands below +0.0)");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, s, labels, masks, excl_off, excl_subject, n_q, -INFINITY, 1, true, pairs));
    const int64_t n_out = axis == 0 ? (int64_t)n_q : s->S;
    if (n_out * (n_edges + 1) > AFIS_HIST_COUNTS_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": more than AFIS_HIST_COUNTS_MAX counts (outputs x (n_edges + 1))");
    if (n_out > 0 && !counts) return fail(ctx, AFIS_EINVAL, std::string(who) + ": counts is null");
    if (n_q > 0 && ctx->last_search.G > 0 && s->S > 0 && !edges) return fail(ctx, AFIS_EINVAL, std::string(who) + ": edges is null");
    return score_histogram(ctx, s, axis, labels, masks, pairs, keys, counts);
}

int afis_entries_at(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl,
                    int n_q, int64_t n_targets, const int32_t* query, const int64_t* rank, int32_t* status, int64_t* idx, float* score)
{
    const char* const who = "afis_entries_at";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    ctx->entries_at_us = 0;
    if (n_targets < 0 || (n_targets > 0 && !(query && rank && status && idx && score))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_targets must be >= 0 and every target array given");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, nullptr, labels, masks, excl_off, excl, n_q, -INFINITY, 1, true, pairs));
    return entries_at(ctx, nullptr, labels, masks, pairs, n_targets, query, rank, status, idx, score, nullptr);
}

int afis_subject_entries_at(afis_ctx* ctx, afis_subjects* s, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl_subject,
                            int n_q, int64_t n_targets, const int32_t* query, const int64_t* rank, int32_t* status, int64_t* subject_id, float* subject_score, int64_t* best_idx)
{
    const char* const who = "afis_subject_entries_at";
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    ctx->subject_entries_at_us = 0;
    AFISCHK(check_subject_handle(ctx, who, s));
    if (n_targets < 0 || (n_targets > 0 && !(query && rank && status && subject_id && subject_score && best_idx)))
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_targets must be >= 0 and every target array given");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, s, labels, masks, excl_off, excl_subject, n_q, -INFINITY, 1, true, pairs));
    return entries_at(ctx, s, labels, masks, pairs, n_targets, query, rank, status, subject_id, subject_score, best_idx);
}

}  // extern "C"
