// afis_weighted.cpp — the weighted search of the C ABI (include/afis_matcher.h): afis_search_weighted scores ANY set of a latent's templates — every minutiae and
// texture template with a non-zero weight — against the resident shard and leaves the weighted sum as a full [n_q][G] matrix, so that the whole ranking family reads
// it unchanged.  No scoring kernel knows about it: the active minutiae templates of a query are packed three to a PSEUDO-QUERY in ascending order and its active texture
// templates one to a pseudo-query (afis_match_all_templates' packing, over the active list), the pseudo-queries of a BATCH of queries are searched through
// upload_queries / search_shard with a selection per pseudo-query (build_group's spec) and their per-part scores kept on the device, and template_fold.hip folds a
// batch's parts into the batch's rows of the combined matrix.  A scorer's value depends on nothing but its (latent template, print), so the packing changes no bit.
#include "afis_ctx.h"

#include <climits>

using namespace afis;

namespace {

// one query of the call: its active templates (ascending) and where its pseudo-queries stand in the call's numbering
struct WQuery { std::vector<int> am, at; int64_t first = 0; int n_pq = 0; };
typedef PseudoBatch WBatch;                                                 // queries [q0, q1), pseudo-queries [p0, p1) — cut at query boundaries

// template i of a query with n templates of that kind is ACTIVE when i < n, i < n_w and the weight is not a zero (of either sign)
void active_list(int n, const float* w, int n_w, std::vector<int>& out)
{
    out.clear();
    for (int i = 0; i < n && i < n_w; ++i) if (w[i] != 0.0f) out.push_back(i);
}

std::vector<WBatch> plan_batches(const std::vector<WQuery>& wq, int64_t cap)
{
    std::vector<int> n_pq;
    for (const WQuery& q : wq) n_pq.push_back(q.n_pq);
    return plan_pseudo_batches(n_pq, cap);
}

// Everything of the call that touches the device.  What it leaves in ctx->elig_scores / ctx->wt_tab after a failure is the caller's to release.
int search_batches(afis_ctx* ctx, const std::vector<WQuery>& wq, const std::vector<WBatch>& batches, const afis_template_view* queries, int n_q,
                   const float* w_minu, int n_wm, const float* w_tex, int n_wt)
{
    const int64_t G = ctx->gal.G;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx));
    // room before anything is queued: the combined matrix, the largest batch's per-part scores and tables (descriptors [queries][4] int32 | weights [pseudo][4] float)
    size_t parts_max = 16, tab_max = 16;
    for (const WBatch& b : batches) {
        parts_max = std::max(parts_max, (size_t)(b.p1 - b.p0) * (size_t)G * 16);
        tab_max = std::max(tab_max, (size_t)(b.q1 - b.q0) * 16 + (size_t)(b.p1 - b.p0) * 16);
    }
    if (G > 0) { HIPCHK(ctx, ctx->elig_scores.ensure((size_t)n_q * (size_t)G * 4)); HIPCHK(ctx, ctx->parts.ensure(parts_max)); }
    HIPCHK(ctx, ctx->wt_tab.ensure(tab_max));
    Events ev(2);
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    afis_timing acc = {};
    int64_t most_pairs = -1, fold_us = 0;
    std::vector<afis_template_view> views;
    std::vector<int> spec;
    std::vector<int32_t> qd;
    std::vector<float> wt;
    for (const WBatch& b : batches) {
        const int nq_b = b.q1 - b.q0;
        const int np_b = (int)(b.p1 - b.p0);
        views.clear(); spec.clear(); qd.clear(); wt.clear();
        for (int i = b.q0; i < b.q1; ++i) {
            const WQuery& q = wq[(size_t)i];
            const float* wm = n_wm > 0 ? w_minu + (size_t)i * n_wm : nullptr;
            const float* wx = n_wt > 0 ? w_tex + (size_t)i * n_wt : nullptr;
            qd.insert(qd.end(), {(int32_t)(q.first - b.p0), q.n_pq, (int32_t)q.at.size(), q.n_pq == 0 ? AFIS_QUERY_LATENT_EMPTY : AFIS_QUERY_OK});
            for (int j = 0; j < q.n_pq; ++j) {
                views.push_back(queries[i]);
                for (int k = 0; k < 3; ++k) {
                    const size_t a = (size_t)3 * j + k;
                    spec.push_back(a < q.am.size() ? q.am[a] : -1);
                    wt.push_back(a < q.am.size() ? wm[q.am[a]] : 0.0f);
                }
                spec.push_back((size_t)j < q.at.size() ? q.at[(size_t)j] : -1);
                wt.push_back((size_t)j < q.at.size() ? wx[q.at[(size_t)j]] : 0.0f);
            }
        }
        afis_queries* q = nullptr;
        struct FreeQ { afis_ctx* c; afis_queries** q; ~FreeQ() { afis_queries_free(c, *q); } } free_q{ctx, &q};
        if (np_b > 0) {
            AFISCHK(upload_queries(ctx, views.data(), np_b, 0, &q, spec.data()));       // the active views are validated here, under afis_search's rules
            AFISCHK(search_shard(ctx, *ctx, nullptr, q, nullptr, nullptr, nullptr, 0, nullptr, nullptr, true));
            ctx->last_search.valid = false;                                 // (a batch's pseudo-query matrix is nobody's to rank)
            add_timing(acc, ctx->timing, most_pairs);
        }
        if (G == 0) continue;
        // the batch's rows of the combined matrix: the device is idle (the search has waited), the tables are this batch's until the wait below
        int32_t* const d_qd = ctx->wt_tab.as<int32_t>();
        float* const d_wt = reinterpret_cast<float*>(ctx->wt_tab.as<uint8_t>() + (size_t)nq_b * 16);
        HIPCHK(ctx, hipMemcpyAsync(d_qd, qd.data(), (size_t)nq_b * 16, hipMemcpyHostToDevice, s));
        if (np_b > 0) HIPCHK(ctx, hipMemcpyAsync(d_wt, wt.data(), (size_t)np_b * 16, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipEventRecord(ev[0], s));
        HIPCHK(ctx, launch_fold_templates(ctx->parts.as<float>(), d_qd, d_wt, ctx->gal.empty, nq_b, (int)G, ctx->elig_scores.as<float>() + (size_t)b.q0 * (size_t)G, s));
        HIPCHK(ctx, hipEventRecord(ev[1], s));
        int64_t us = 0;
        AFISCHK(wait_elapsed(ctx, "afis_search_weighted", ev, &us));
        fold_us += us;
    }
    std::swap(ctx->scores, ctx->elig_scores);                               // the combined matrix is the last search's from here on
    ctx->timing = acc;
    ctx->weighted_pseudo_queries = batches.empty() ? 0 : batches.back().p1; ctx->weighted_fold_us = fold_us;
    return AFIS_OK;
}

}  // namespace

extern "C" {

int afis_search_weighted(afis_ctx* ctx, const afis_template_view* queries, int n_q, const float* w_minu, int n_wm, const float* w_tex, int n_wt, float* scores, int32_t* status)
{
    if (!ctx) return fail(ctx, AFIS_EINVAL, "afis_search_weighted: null context");
    ctx->weighted_pseudo_queries = 0; ctx->weighted_fold_us = 0;
    ctx->last_search = LastSearch{};                                        // whatever this call returns, the matrix of an earlier search is no longer there to rank
    if (n_q < 0 || (n_q > 0 && !queries) || n_wm < 0 || n_wt < 0 || (n_q > 0 && ((n_wm > 0 && !w_minu) || (n_wt > 0 && !w_tex))))
        return fail(ctx, AFIS_EINVAL, "afis_search_weighted: bad argument");
    for (int k = 0; k < 2; ++k) {
        const float* w = k ? w_tex : w_minu;
        const size_t n = (size_t)n_q * (size_t)(k ? n_wt : n_wm);
        for (size_t i = 0; i < n; ++i)
            if (!(w[i] >= 0.0f) || std::isinf(w[i])) return fail(ctx, AFIS_EINVAL, "afis_search_weighted: a weight must be finite and >= 0 (-1 means \"empty\", every other cell is >= +0)");
    }
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_search_weighted: commit the gallery first");
    if (n_q == 0) return afis_search(ctx, nullptr, 0, scores, nullptr, status, 0, nullptr, nullptr);
    const int64_t G = ctx->gal.G;
    // the plan: active lists, pseudo-queries, batches
    std::vector<WQuery> wq((size_t)n_q);
    int64_t n_pseudo = 0;
    for (int i = 0; i < n_q; ++i) {
        WQuery& q = wq[(size_t)i];
        active_list(queries[i].n_minu, n_wm > 0 ? w_minu + (size_t)i * n_wm : nullptr, n_wm, q.am);
        active_list(queries[i].n_tex, n_wt > 0 ? w_tex + (size_t)i * n_wt : nullptr, n_wt, q.at);
        q.first = n_pseudo;
        q.n_pq = (int)std::max((q.am.size() + 2) / 3, q.at.size());
        n_pseudo += q.n_pq;
        if (status) status[i] = q.n_pq == 0 ? AFIS_QUERY_LATENT_EMPTY : AFIS_QUERY_OK;
    }
    // pseudo-queries per batch at most: the option, or as many as an eighth of the group budget holds the per-part scores of (16 bytes per pair)
    (void)hipSetDevice(ctx->device);
    const int64_t cap_auto = std::max<int64_t>(1, group_budget_bytes(ctx) / 8 / (16 * std::max<int64_t>(1, G)));
    const int64_t cap = std::min<int64_t>(ctx->weighted_batch_pseudo > 0 ? ctx->weighted_batch_pseudo : cap_auto, INT_MAX / 4);
    const std::vector<WBatch> batches = plan_batches(wq, cap);
    for (const WBatch& b : batches)
        if (b.p1 - b.p0 > INT_MAX / 4) return fail(ctx, AFIS_EINVAL, "afis_search_weighted: one query has too many active templates");
    int rc = search_batches(ctx, wq, batches, queries, n_q, w_minu, n_wm, w_tex, n_wt);
    if (rc == AFIS_OK && scores && G > 0) {                                 // the device is idle: a plain copy, as at the end of a search
        const hipError_t e = hipMemcpy(scores, ctx->scores.p, (size_t)n_q * (size_t)G * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, AFIS_EDEVICE, std::string("afis_search_weighted: the scores: ") + hipGetErrorString(e));
    }
    if (rc != AFIS_OK) {                                                    // after a timeout a launch may still read the tables: the bounded wait first, then nothing of the call stays
        const std::string keep = ctx->err;
        (void)quiesce(ctx, "afis_search_weighted");
        ctx->err = keep;
        ctx->elig_scores.release(); ctx->wt_tab.release();
        ctx->weighted_pseudo_queries = 0; ctx->weighted_fold_us = 0;
    }
    ctx->last_search = rc == AFIS_OK ? LastSearch{true, n_q, G, nullptr, ctx->gallery_epoch} : LastSearch{};
    return rc;
}

}  // extern "C"
