// afis_positions.cpp — rank positions of the C ABI (include/afis_matcher.h): afis_rank_positions and afis_rank_subject_positions say where a NAMED template, or person,
// stands in the list afis_rank_hits_filtered / afis_rank_subject_hits_filtered would give a query of the last search at min_score = -inf — for every position, not only
// the first AFIS_HITS_MAX — and afis_count_before counts the entries of a row that stand before a hypothetical entry (score, global index): the per-shard term of a
// global position.  The checks are the filtered hit lists' (check_filtered), the filters run as they run there (FilterPass, queue_subject_best, the drops: no second
// definition of eligibility), and the two passes of rank_position.hip read the matrix, or its filtered copy.  Here: the targets resolved to (row, position) the way
// check_filtered resolves exclusions, sorted into a CSR by row as afis_cases.cpp sorts the members of its cases, and scattered back into the caller's order.  About 24
// bytes per covered target return, through the context's pinned buffer; the [n_q][G] matrix stays where it is, and as it is.
#include "afis_ctx.h"

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
    std::vector<int64_t> held;                                              // a subset's device order: its listed indices ascending
    if (!pc.subj && ls.sub) { held = ls.sub->idx; std::sort(held.begin(), held.end()); }
    const std::vector<int64_t>& names = pc.subj ? pc.subj->ids : held;
    const bool by_offset = !pc.subj && !ls.sub;
    std::vector<int32_t> src, pos, tie;                                     // per device target: the caller's target, its position, (afis_count_before) its tie position
    for (int64_t i = 0; i < nt; ++i) {
        int64_t c, lb;
        if (by_offset) { c = pc.name[i] - ctx->index_base; lb = std::min<int64_t>(std::max<int64_t>(c, 0), G); if (c >= G) c = -1; }
        else {
            const auto it = std::lower_bound(names.begin(), names.end(), pc.name[i]);
            lb = (int64_t)(it - names.begin());
            c = (it != names.end() && *it == pc.name[i]) ? lb : -1;
        }
        if (c < 0 && pc.mode != kPosCount) continue;                        // not covered: the answer stands already
        src.push_back((int32_t)i); pos.push_back((int32_t)std::max<int64_t>(c, -1)); tie.push_back((int32_t)lb);
    }
    const size_t m = src.size();
    if (m == 0) return AFIS_OK;

    // ---- a CSR by row: a counting sort keeps a row's targets in the caller's order
    std::vector<int32_t> per_row((size_t)n_q + 1, 0);
    for (size_t k = 0; k < m; ++k) ++per_row[(size_t)pc.query[src[k]] + 1];
    std::vector<int32_t> rows, off(1, 0), first((size_t)n_q, 0);
    for (int q = 0; q < n_q; ++q)
        if (per_row[(size_t)q + 1]) { first[(size_t)q] = off.back(); rows.push_back(q); off.push_back(off.back() + per_row[(size_t)q + 1]); }
    const size_t n_rows = rows.size();
    // the tables as one upload: rows [n_rows] | off [n_rows + 1] | row [m] | pos [m]; order[t]: the device target at place t of the CSR
    std::vector<int32_t> tab(2 * n_rows + 1 + 2 * m), order(m);
    std::copy(rows.begin(), rows.end(), tab.begin());
    std::copy(off.begin(), off.end(), tab.begin() + (ptrdiff_t)n_rows);
    int32_t* const t_row = tab.data() + 2 * n_rows + 1, * const t_pos = t_row + m;
    std::vector<uint64_t> comp(pc.mode == kPosCount ? m : 0);
    for (size_t k = 0; k < m; ++k) {
        const int32_t q = pc.query[src[k]], t = first[(size_t)q]++;
        order[(size_t)t] = (int32_t)k; t_row[t] = q; t_pos[t] = pos[k];
        if (pc.mode == kPosCount) comp[(size_t)t] = rank_composite(rank_key(pc.in_score[src[k]]), (uint32_t)tie[k]);
    }

    // ---- the device: room first, then the filter pass exactly as the filtered hit lists run it, the target pass, the counting pass
    const size_t comp_bytes = m * 8, tab_bytes = comp_bytes + tab.size() * 4;
    const size_t count_at = 0, best_at = m * 8, status_at = 2 * m * 8, score_at = status_at + m * 4, out_bytes = score_at + m * 4;
    const size_t back_bytes = pc.mode == kPosCount ? m * 8 : out_bytes;
    FilterPass fp{ctx, pc.labels, pc.masks, pairs, pc.subj != nullptr};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, fp.ensure());
    if (pc.subj) HIPCHK(ctx, ctx->subj_best.ensure((size_t)n_q * (size_t)S * 8));
    HIPCHK(ctx, ctx->pos_tab.ensure(tab_bytes));
    HIPCHK(ctx, ctx->pos_out.ensure(out_bytes));
    HIPCHK(ctx, ensure_pin(ctx, back_bytes));
    Events ev{2};
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    hipStream_t s = ctx->stream;
    uint8_t* const d_tab = ctx->pos_tab.as<uint8_t>(), * const d_out = ctx->pos_out.as<uint8_t>();
    const HitCall::H2D ups[] = {{d_tab + comp_bytes, tab.data(), tab.size() * 4}, {d_tab, comp.data(), comp.size() * 8}, fp.masks_up(), fp.pairs_up()};
    for (const HitCall::H2D& u : ups) if (u.bytes) HIPCHK(ctx, hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipEventRecord(ev[0], s));
    AFISCHK(fp.queue_cells());                                              // neither masks nor exclusions: nothing, and the search's matrix itself is read
    if (pc.subj) {                                                          // the maxima of the filtered rows, then the excluded persons: rank_hits_filtered's sequence
        AFISCHK(queue_subject_best(ctx, pc.subj, fp.matrix()));
        AFISCHK(fp.queue_drop_subjects(S));
    }
    unsigned long long* const d_comp = (unsigned long long*)d_tab, * const d_count = (unsigned long long*)(d_out + count_at);
    const int32_t* const d_rows = (const int32_t*)(d_tab + comp_bytes), * const d_off = d_rows + n_rows, * const d_row = d_off + n_rows + 1, * const d_pos = d_row + m;
    const unsigned long long* const best = pc.subj ? ctx->subj_best.as<unsigned long long>() : nullptr;
    HIPCHK(ctx, launch_position_targets(pc.mode, fp.matrix(), (int)G, best, (int)S, d_row, d_pos, m, global_map(ls), (long long)ctx->index_base, d_comp, d_count,
                                        (int32_t*)(d_out + status_at), (float*)(d_out + score_at), (long long*)(d_out + best_at), s));
    HIPCHK(ctx, launch_count_before(fp.matrix(), best, (int)(pc.subj ? S : G), d_rows, d_off, (int)n_rows, *std::max_element(per_row.begin(), per_row.end()), d_comp, d_count, s));
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_out, back_bytes, hipMemcpyDeviceToHost, s));
    int64_t total_us = 0;
    AFISCHK(wait_elapsed(ctx, pc.who, ev, &total_us));
    ctx->rank_positions_us = total_us;

    // ---- back into the caller's order
    const uint8_t* const pin = (const uint8_t*)ctx->h_pin;
    for (size_t t = 0; t < m; ++t) {
        const int64_t i = src[(size_t)order[t]];
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
