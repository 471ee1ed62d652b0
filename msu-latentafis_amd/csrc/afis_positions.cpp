// afis_positions.cpp — rank positions of the C ABI (include/afis_matcher.h): afis_rank_positions and afis_rank_subject_positions say where a NAMED template, or person,
// stands in the list afis_rank_hits_filtered / afis_rank_subject_hits_filtered would give a query of the last search at min_score = -inf — for every position, not only
// the first AFIS_HITS_MAX — and afis_count_before counts the entries of a row that stand before a hypothetical entry (score, global index): the per-shard term of a
// global position.  A matrix call (MatrixCall, afis_ctx.h) whose kernels are the two passes of rank_position.hip.  Here: the targets resolved to (row, position) the way
// check_filtered resolves exclusions (column_names), sorted into a CSR by row (target_tables.h), scattered back into the caller's order; about 24 bytes a covered target return.
#include "afis_ctx.h"
#include "target_tables.h"

using namespace afis;

static_assert(kPosListed == AFIS_POS_LISTED && kPosNoEntry == AFIS_POS_NO_ENTRY, "rank_position.hip writes the status values of include/afis_matcher.h");

namespace afis {

enum { kPosTemplates = 0, kPosSubjects = 1, kPosCount = 2 };                // launch_position_targets' modes

// what a call asks and where the answers go (templates: best_idx NULL; afis_count_before: in_score given, n_before the only output)
struct PositionCall {
    const char* who; int mode; afis_subjects* subj; const afis_labels* labels; const uint64_t* masks;
    int64_t n_targets; const int32_t* query; const int64_t* name; const float* in_score;
    int32_t* status; int64_t* n_before; float* score; int64_t* best_idx;
};

// the three entry points behind their checks; pairs: the exclusions as check_filtered resolved them
static int rank_positions(afis_ctx* ctx, const PositionCall& pc, const std::vector<int32_t>& pairs)
{
    const LastSearch ls = ctx->last_search;
    const int n_q = ls.n_q;
    const int64_t G = ls.G, S = pc.subj ? pc.subj->S : 0, nt = pc.n_targets;
    const std::string w(pc.who);
    ctx->rank_positions_us = 0;
    if (nt > (int64_t)INT32_MAX) return fail(ctx, AFIS_EINVAL, w + ": more than 2^31 - 1 targets");
    for (int64_t i = 0; i < nt; ++i) {
        if (pc.query[i] < 0 || pc.query[i] >= n_q) return fail(ctx, AFIS_EINVAL, w + ": a target's query is outside 0 .. n_q - 1");
        if (pc.name[i] < 0) return fail(ctx, AFIS_EINVAL, w + (pc.subj ? ": a target's subject id is negative" : ": a target's index is negative"));
        if (pc.in_score && std::isnan(pc.in_score[i])) return fail(ctx, AFIS_EINVAL, w + ": a target's score is a NaN");
    }
    // what holds for a target nothing of the search covers — and for every target of an empty shard
    for (int64_t i = 0; i < nt; ++i) {
        if (pc.mode == kPosCount) { pc.n_before[i] = 0; continue; }
        pc.status[i] = AFIS_POS_NOT_COVERED; pc.n_before[i] = -1; pc.score[i] = -INFINITY;
        if (pc.best_idx) pc.best_idx[i] = -1;
    }
    if (nt == 0 || G == 0 || (pc.subj && S == 0)) return AFIS_OK;

    // ---- the targets as (row, position): a column of the matrix, or a slot of the handle; afis_count_before: the tie position, and the column the index names (or -1)
    const ColumnNames names = column_names(ctx, pc.subj);
    std::vector<int32_t> src, pos, tie;                                     // per device target: the caller's target, its position, (afis_count_before) its tie position
    for (int64_t i = 0; i < nt; ++i) {
        const int64_t lb = names.lower(pc.name[i]), c = lb < names.n && names.name(lb) == pc.name[i] ? lb : -1;   // (names.find, on the one search)
        if (c < 0 && pc.mode != kPosCount) continue;                        // not covered: the answer stands already
        src.push_back((int32_t)i); pos.push_back((int32_t)c); tie.push_back((int32_t)lb);
    }
    const size_t m = src.size();
    if (m == 0) return AFIS_OK;

    // ---- a CSR by row, a row's targets in the caller's order; the tables as one upload: the composites [m] | rows [n_rows] | off [n_rows + 1] | row [m] | pos [m]
    const TargetTables tt = build_target_tables(pc.query, src.data(), m, nullptr);   // tt.order[t]: the device target at place t of the CSR
    const size_t n_rows = tt.rows.size();
    std::vector<int32_t> tab(2 * n_rows + 1 + 2 * m);
    int32_t* const t_pos = tt.write(tab.data());
    std::vector<uint64_t> comp(pc.mode == kPosCount ? m : 0);
    for (size_t t = 0; t < m; ++t) {
        const size_t k = (size_t)tt.order[t]; t_pos[t] = pos[k];
        if (pc.mode == kPosCount) comp[t] = rank_composite(rank_key(pc.in_score[src[k]]), (uint32_t)tie[k]);
    }

    // ---- the device: the target pass, the counting pass
    const size_t comp_bytes = m * 8, tab_bytes = comp_bytes + tab.size() * 4;
    const size_t count_at = 0, best_at = m * 8, status_at = 2 * m * 8, score_at = status_at + m * 4, out_bytes = score_at + m * 4, back_bytes = pc.mode == kPosCount ? m * 8 : out_bytes;
    MatrixCall mc{ctx, pc.who, pc.subj, pc.subj ? kPersonBest : kTemplateCells, {ctx, pc.labels, pc.masks, pairs, pc.subj != nullptr}};
    AFISCHK(mc.room({{&ctx->pos_tab, tab_bytes}, {&ctx->pos_out, out_bytes}}, back_bytes));
    uint8_t* const d_tab = ctx->pos_tab.as<uint8_t>(), * const d_out = ctx->pos_out.as<uint8_t>();
    AFISCHK(mc.begin({{d_tab + comp_bytes, tab.data(), tab.size() * 4}, {d_tab, comp.data(), comp.size() * 8}}));
    const float* const matrix = mc.fp.matrix();
    unsigned long long* const d_comp = (unsigned long long*)d_tab, * const d_count = (unsigned long long*)(d_out + count_at);
    const int32_t* const d_rows = (const int32_t*)(d_tab + comp_bytes), * const d_off = d_rows + n_rows, * const d_row = d_off + n_rows + 1, * const d_pos = d_row + m;
    const unsigned long long* const best = pc.subj ? ctx->subj_best.as<unsigned long long>() : nullptr;
    HIPCHK(ctx, launch_position_targets(pc.mode, matrix, (int)G, best, (int)S, d_row, d_pos, m, global_map(ls), (long long)ctx->index_base, d_comp, d_count,
                                        (int32_t*)(d_out + status_at), (float*)(d_out + score_at), (long long*)(d_out + best_at), ctx->stream));
    HIPCHK(ctx, launch_count_before(matrix, best, (int)(pc.subj ? S : G), d_rows, d_off, (int)n_rows, tt.max_row_targets, d_comp, d_count, ctx->stream));
    AFISCHK(mc.finish(d_out, back_bytes, &ctx->rank_positions_us));

    // ---- back into the caller's order
    const uint8_t* const pin = (const uint8_t*)ctx->h_pin;
    for (size_t t = 0; t < m; ++t) {
        const int64_t i = src[(size_t)tt.order[t]];
        int64_t count; memcpy(&count, pin + count_at + t * 8, 8);
        if (pc.mode == kPosCount) { pc.n_before[i] = count; continue; }
        memcpy(pc.status + i, pin + status_at + t * 4, 4);
        memcpy(pc.score + i, pin + score_at + t * 4, 4);
        if (pc.best_idx) memcpy(pc.best_idx + i, pin + best_at + t * 8, 8);
        pc.n_before[i] = pc.status[i] == AFIS_POS_LISTED ? count : -1;
    }
    return AFIS_OK;
}

}  // namespace afis

extern "C" {

int afis_rank_positions(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl,
                        int n_q, int64_t n_targets, const int32_t* query, const int64_t* idx, int32_t* status, int64_t* n_before, float* score)
{
    const char* const who = "afis_rank_positions";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    if (n_targets < 0 || (n_targets > 0 && !(query && idx && status && n_before && score))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_targets must be >= 0 and every target array given");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, nullptr, labels, masks, excl_off, excl, n_q, -INFINITY, 1, true, pairs));
    return rank_positions(ctx, PositionCall{who, kPosTemplates, nullptr, labels, masks, n_targets, query, idx, nullptr, status, n_before, score, nullptr}, pairs);
}

int afis_rank_subject_positions(afis_ctx* ctx, afis_subjects* s, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl_subject,
                                int n_q, int64_t n_targets, const int32_t* query, const int64_t* subject_id, int32_t* status, int64_t* n_before, float* score, int64_t* best_idx)
{
    const char* const who = "afis_rank_subject_positions";
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    AFISCHK(check_subject_handle(ctx, who, s));
    if (n_targets < 0 || (n_targets > 0 && !(query && subject_id && status && n_before && score && best_idx)))
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_targets must be >= 0 and every target array given");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, s, labels, masks, excl_off, excl_subject, n_q, -INFINITY, 1, true, pairs));
    return rank_positions(ctx, PositionCall{who, kPosSubjects, s, labels, masks, n_targets, query, subject_id, nullptr, status, n_before, score, best_idx}, pairs);
}

int afis_count_before(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl,
                      int n_q, int64_t n_targets, const int32_t* query, const float* score, const int64_t* idx, int64_t* n_before)
{
    const char* const who = "afis_count_before";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    if (n_targets < 0 || (n_targets > 0 && !(query && score && idx && n_before))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_targets must be >= 0 and every target array given");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, nullptr, labels, masks, excl_off, excl, n_q, -INFINITY, 1, true, pairs));
    return rank_positions(ctx, PositionCall{who, kPosCount, nullptr, labels, masks, n_targets, query, idx, score, nullptr, n_before, nullptr, nullptr}, pairs);
}

}  // extern "C"
