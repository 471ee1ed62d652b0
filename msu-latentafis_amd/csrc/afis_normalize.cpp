// afis_normalize.cpp — cohort statistics and z-normalised scores of the C ABI (include/afis_matcher.h); afis_subject_score_stats is afis_score_stats over persons
// (score_cell.h: a person's cell is the best of their eligible covered templates).  afis_score_stats reads the last search's matrix along its rows
// (axis 0: one statistic per query, "T-norm") or its columns (axis 1: one per print, "Z-norm") and returns exact integer statistics (score_stats.h) of the cells the
// call's filter leaves: a matrix call (MatrixCall, afis_ctx.h).  afis_normalize_scores puts every cell of the UNFILTERED matrix on the scale of its row's or column's
// (offset, scale) pair; the result is built in ctx->elig_scores and swapped with ctx->scores, the way afis_search_eligible ends, so that every ranking call then reads
// z-scores — no filter pass, no pinned copy, two matrices swapped: not that driver's.  The three host helpers (add, remove, moments) are plain integer arithmetic, no context.
// A subset listed out of order: the sub-shard stands in ascending global index order; statistics per column, pairs per column and scores_out are put in the caller's
// column order here — the rank of idx[j] among the listed indices is its position in the sub-shard (afis_subset_create), as afis_rank_latent_hits orders its rows.
#include "afis_ctx.h"
#include "score_stats.h"

using namespace afis;

static_assert(sizeof(afis_score_stat) == sizeof(ScoreStat) && offsetof(afis_score_stat, n_outside) == offsetof(ScoreStat, n_outside) && offsetof(afis_score_stat, s1) == offsetof(ScoreStat, s1) &&
              offsetof(afis_score_stat, s2_lo) == offsetof(ScoreStat, s2_lo) && offsetof(afis_score_stat, s2_hi) == offsetof(ScoreStat, s2_hi) &&
              offsetof(afis_score_stat, min) == offsetof(ScoreStat, min) && offsetof(afis_score_stat, max) == offsetof(ScoreStat, max) && sizeof(ScoreStat) == 48,
              "score_stats.h::ScoreStat is the layout of afis_score_stat");

namespace afis {

// order[t]: the caller's column of sub-shard position t; empty: the identity (afis_distribution.cpp orders its columns by it too)
std::vector<int32_t> column_order(const LastSearch& ls)
{
    std::vector<int32_t> order(ls.sub && !ls.sub->identity ? (size_t)ls.G : 0);
    if (!order.empty()) {
        const std::vector<int64_t>& idx = ls.sub->idx;
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin(), order.end(), [&idx](int32_t a, int32_t b) { return idx[(size_t)a] < idx[(size_t)b]; });
    }
    return order;
}

// afis_score_stats (subj == NULL: the cells of the matrix) and afis_subject_score_stats (the person cells [n_q][S] of the handle: queue_subject_keys,
// afis_distribution.cpp; a column is a slot, the distinct ids ascending) behind their checks; pairs: the exclusions as check_filtered resolved them
static int score_stats(afis_ctx* ctx, afis_subjects* subj, int axis, const afis_labels* labels, const uint64_t* masks, const std::vector<int32_t>& pairs, afis_score_stat* out)
{
    const char* const who = subj ? "afis_subject_score_stats" : "afis_score_stats";
    const LastSearch ls = ctx->last_search;
    const int n_q = ls.n_q;
    const int64_t G = ls.G, cols = subj ? subj->S : G, n_out = axis == 0 ? n_q : cols, len = axis == 0 ? cols : n_q;
    if (len > kStatMaxCells) return fail(ctx, AFIS_EINVAL, std::string(who) + ": a statistic takes 2^27 cells at most");
    ScoreStat none{}; none.min = INFINITY; none.max = -INFINITY;
    if (n_q == 0 || G == 0 || cols == 0) {                                  // no cell: no device work
        for (int64_t i = 0; i < n_out; ++i) memcpy(out + i, &none, sizeof none);
        return AFIS_OK;
    }
    const std::vector<int32_t> order = axis == 1 && !subj ? column_order(ls) : std::vector<int32_t>();
    const size_t out_bytes = (size_t)n_out * sizeof(ScoreStat);
    MatrixCall mc{ctx, who, subj, subj ? kPersonKeys : kTemplateCells, {ctx, labels, masks, pairs, subj != nullptr}};
    AFISCHK(mc.room({{&ctx->stat_tab, axis == 0 ? (size_t)n_q * kStatWords * 8 : 0}, {&ctx->stat_out, out_bytes}}, out_bytes));
    AFISCHK(mc.begin());
    if (subj) HIPCHK(ctx, launch_subject_stats(axis, ctx->subj_keys.as<uint32_t>(), n_q, (int)cols, ctx->stat_tab.as<unsigned long long>(), ctx->stat_out.p, ctx->stream));
    else HIPCHK(ctx, launch_score_stats(axis, mc.fp.matrix(), n_q, (int)G, ctx->stat_tab.as<unsigned long long>(), ctx->stat_out.p, ctx->stream));
    AFISCHK(mc.finish(ctx->stat_out.p, out_bytes, subj ? &ctx->subject_score_stats_us : &ctx->score_stats_us));
    const uint8_t* const pin = (const uint8_t*)ctx->h_pin;
    if (order.empty()) memcpy(out, pin, out_bytes);
    else for (size_t t = 0; t < order.size(); ++t) memcpy(out + order[t], pin + t * sizeof(ScoreStat), sizeof(ScoreStat));
    return AFIS_OK;
}

// afis_normalize_scores behind its checks
static int normalize_scores(afis_ctx* ctx, int axis, const double* offset, const double* scale, float* scores_out)
{
    const char* const who = "afis_normalize_scores";
    const LastSearch ls = ctx->last_search;
    const int n_q = ls.n_q;
    const int64_t G = ls.G, n_pairs = axis == 0 ? n_q : G;
    if (n_q == 0 || G == 0) { ctx->last_search.normalized = true; return AFIS_OK; }   // no cell: no device work
    const std::vector<int32_t> order = column_order(ls);
    std::vector<double> pair((size_t)n_pairs * 2);                          // in the order of the matrix on the device
    for (int64_t t = 0; t < n_pairs; ++t) {
        const size_t j = axis == 1 && !order.empty() ? (size_t)order[(size_t)t] : (size_t)t;
        pair[(size_t)t * 2] = offset[j]; pair[(size_t)t * 2 + 1] = scale[j];
    }
    const size_t bytes = (size_t)n_q * (size_t)G * 4;
    const bool perm = scores_out && !order.empty();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, ctx->elig_scores.ensure(bytes));
    HIPCHK(ctx, ctx->stat_tab.ensure(pair.size() * 8));
    if (perm) HIPCHK(ctx, ctx->out_perm.ensure(bytes));
    Events ev{2};
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->stat_tab.p, pair.data(), pair.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipEventRecord(ev[0], s));
    HIPCHK(ctx, launch_normalize_scores(axis, ctx->scores.as<float>(), n_q, (int)G, ctx->stat_tab.as<double>(), ctx->elig_scores.as<float>(), s));
    if (perm)
        for (int r0 = 0; r0 < n_q; r0 += 65535)                             // (launch_permute_columns takes a grid's second dimension of rows)
            HIPCHK(ctx, launch_permute_columns(ctx->elig_scores.as<float>() + (size_t)r0 * (size_t)G, ctx->out_perm.as<float>() + (size_t)r0 * (size_t)G, 4, std::min(65535, n_q - r0), (int)G,
                                               ls.sub->d_pos.as<int32_t>(), s));
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    int64_t total_us = 0;
    AFISCHK(wait_elapsed(ctx, who, ev, &total_us));
    if (scores_out) HIPCHK(ctx, hipMemcpy(scores_out, perm ? ctx->out_perm.p : ctx->elig_scores.p, bytes, hipMemcpyDeviceToHost));
    std::swap(ctx->scores, ctx->elig_scores);                               // the normalised matrix is the last search's from here on
    ctx->last_search.normalized = true;
    ctx->normalize_us = total_us;
    return AFIS_OK;
}

static int refuse_normalized(afis_ctx* ctx, const char* who)
{
    return fail(ctx, AFIS_ESTATE, std::string(who) + ": the last search's matrix holds normalised scores already (afis_normalize_scores); search again");
}

}  // namespace afis

extern "C" {

int afis_score_stats(afis_ctx* ctx, int axis, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl, int n_q, afis_score_stat* out)
{
    const char* const who = "afis_score_stats";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    ctx->score_stats_us = 0;
    if (axis != 0 && axis != 1) return fail(ctx, AFIS_EINVAL, std::string(who) + ": axis must be 0 (rows) or 1 (columns)");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, nullptr, labels, masks, excl_off, excl, n_q, -INFINITY, 1, true, pairs));
    if (ctx->last_search.normalized) return refuse_normalized(ctx, who);
    if (!out && (axis == 0 ? (int64_t)n_q : ctx->last_search.G) > 0) return fail(ctx, AFIS_EINVAL, std::string(who) + ": out is null");
    return score_stats(ctx, nullptr, axis, labels, masks, pairs, out);
}

int afis_subject_score_stats(afis_ctx* ctx, afis_subjects* s, int axis, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl_subject, int n_q,
                             afis_score_stat* out)
{
    const char* const who = "afis_subject_score_stats";
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    ctx->subject_score_stats_us = 0;
    AFISCHK(check_subject_handle(ctx, who, s));
    if (axis != 0 && axis != 1) return fail(ctx, AFIS_EINVAL, std::string(who) + ": axis must be 0 (queries) or 1 (subjects)");
    std::vector<int32_t> pairs;
    AFISCHK(check_filtered(ctx, who, s, labels, masks, excl_off, excl_subject, n_q, -INFINITY, 1, true, pairs));
    if (ctx->last_search.normalized) return refuse_normalized(ctx, who);
    if (!out && (axis == 0 ? (int64_t)n_q : s->S) > 0) return fail(ctx, AFIS_EINVAL, std::string(who) + ": out is null");
    return score_stats(ctx, s, axis, labels, masks, pairs, out);
}

int afis_normalize_scores(afis_ctx* ctx, int axis, int n_q, const double* offset, const double* scale, float* scores_out)
{
    const char* const who = "afis_normalize_scores";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    ctx->normalize_us = 0;
    if (axis != 0 && axis != 1) return fail(ctx, AFIS_EINVAL, std::string(who) + ": axis must be 0 (rows) or 1 (columns)");
    AFISCHK(check_last_search(ctx, who, n_q, nullptr));
    if (ctx->last_search.normalized) return refuse_normalized(ctx, who);
    const int64_t n = axis == 0 ? (int64_t)n_q : ctx->last_search.G;
    if (n > 0 && !(offset && scale)) return fail(ctx, AFIS_EINVAL, std::string(who) + ": offset and scale must be given");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(offset[i]) || !std::isfinite(scale[i]) || !(scale[i] > 0.0))
            return fail(ctx, AFIS_EINVAL, std::string(who) + ": every offset must be finite and every scale finite and > 0 (entry " + std::to_string((long long)i) + ")");
    return normalize_scores(ctx, axis, offset, scale, scores_out);
}

int afis_score_stat_add(afis_score_stat* acc, const afis_score_stat* other)
{
    if (!acc || !other) return AFIS_EINVAL;
    ScoreStat a, o;
    memcpy(&a, acc, sizeof a); memcpy(&o, other, sizeof o);
    if (stat_add(a, o) != 0) return AFIS_EINVAL;
    memcpy(acc, &a, sizeof a);
    return AFIS_OK;
}

int afis_score_stat_remove(afis_score_stat* acc, float score)
{
    if (!acc) return AFIS_EINVAL;
    ScoreStat a;
    memcpy(&a, acc, sizeof a);
    if (stat_remove(a, score) != 0) return AFIS_EINVAL;
    memcpy(acc, &a, sizeof a);
    return AFIS_OK;
}

int afis_score_stat_moments(const afis_score_stat* st, double* mean, double* sd)
{
    if (!st || !mean || !sd) return AFIS_EINVAL;
    ScoreStat a;
    memcpy(&a, st, sizeof a);
    return stat_moments(a, mean, sd) == 0 ? AFIS_OK : AFIS_EINVAL;
}

}  // extern "C"
