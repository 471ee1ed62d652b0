// afis_print_pairs.cpp — the pair forms for RESIDENT PRINT pairs of the C ABI (include/afis_matcher.h): afis_score_print_pairs gives the weighted score — and the two
// parts — of a list of (query print, column print) pairs, bit for bit the cells afis_search_prints would write for them, and afis_correspondences_print_pairs the
// surviving minutiae correspondences of such a list: verification of two enrolled prints, card against card, the candidates an operator opens after a print search,
// labelled print pairs.  Nothing here scores on its own.  The plan (print_pairs_plan.h, host only) names the distinct query prints of the pairs that need the device, cuts
// them into batches and gives every pair the position of its query print in its batch; per batch the driver builds a temporary query handle of the prints' views on the
// device, exactly as afis_search_prints builds its batches' (afis_prints.cpp::build_print_queries — without invalidating the last search), and runs the existing pair
// drivers over the batch's pairs: afis_pairs.cpp::score_pairs with the weighted fold of a print pair in place of fuse_cell (template_fold.hip::k_fold_print_pairs),
// afis_corr.cpp::correspondences_pairs with slot 0 alone in its output.  Those drivers settle an empty or removed column print and the chunks; what is not covered, a
// pair with nothing active and a query print without minutiae is settled here from the host's tables.  The caller's arrays are written once, after the last batch.
#include "afis_ctx.h"
#include "print_pairs_plan.h"

#include <limits>

using namespace afis;

namespace {

struct Call {                                                               // what both entry points share
    afis_ctx* ctx; const char* who; int64_t n_pairs; const int64_t* a_idx; const int64_t* b_idx;
    int64_t G = 0, base = 0;
    PrintPairsPlan plan;
    std::vector<PrintGroupPlan> plans;                                      // the host's copies of a batch's group tables: they live until the device is known idle
    int64_t us = 0;
    bool covered(int64_t i) const { return a_idx[i] >= base && a_idx[i] - base < G && b_idx[i] >= base && b_idx[i] - base < G; }
    bool has_minu(int64_t g) const { const size_t t = (size_t)(g - base); return ctx->res_mo[t + 1] > ctx->res_mo[t]; }
    bool has_tex(int64_t g) const { const size_t t = (size_t)(g - base); return ctx->res_to[t + 1] > ctx->res_to[t]; }

    void make_plan(const uint8_t* want_minu, const uint8_t* want_tex)
    {
        const int64_t budget = ctx->print_pairs_batch_prints > 0 ? 0 : group_budget_bytes(ctx) / 8;
        plan_print_pairs(n_pairs, a_idx, b_idx, base, G, ctx->res_mo.data(), ctx->res_to.data(), want_minu, want_tex, ctx->print_pairs_batch_prints, budget, plan);
    }

    // run(q, first entry of plan.pair / plan.pos, entries) for every batch, over that batch's temporary handle
    int batches(const std::function<int(afis_queries*, size_t, size_t)>& run)
    {
        const std::vector<int32_t> res_tile = resident_tile_offsets(ctx);
        for (size_t k = 0; k + 1 < plan.batch_first.size(); ++k) {
            const size_t p0 = plan.batch_first[k], n = plan.batch_first[k + 1] - p0;
            afis_queries* q = nullptr;
            struct FreeQ { afis_ctx* c; afis_queries** q; ~FreeQ() { afis_queries_free(c, *q); } } free_q{ctx, &q};     // (parked while a timed-out launch may still read it)
            int64_t h2d = 0;
            AFISCHK(build_print_queries(ctx, who, res_tile, plan.prints.data() + p0, plan.use_minu.data() + p0, plan.use_tex.data() + p0, (int)n, true, plans, &q, &h2d, &us));
            AFISCHK(run(q, plan.pair_first[k], plan.pair_first[k + 1] - plan.pair_first[k]));
        }
        return AFIS_OK;
    }

    // after a failure a launch or a copy may still read the tables: the bounded wait first (the last search's matrix stays), the error the caller sees is the first one
    // us_option: where the call's device time goes (NULL: "print_pairs_us", with "print_pairs_query_prints" beside it)
    int end(int rc, int64_t* us_option = nullptr)
    {
        if (rc != AFIS_OK) {
            const std::string keep = ctx->err;
            (void)quiesce(ctx, who, true);
            ctx->err = keep;
            return rc;
        }
        if (us_option) { *us_option = us; return AFIS_OK; }
        ctx->print_pairs_us = us; ctx->print_pairs_query_prints = (int64_t)plan.prints.size();
        return AFIS_OK;
    }
};

int check_common(afis_ctx* ctx, const char* who, int64_t n_pairs, bool arrays)
{
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null context");
    ctx->print_pairs_us = 0; ctx->print_pairs_query_prints = 0;
    if (n_pairs < 0 || (n_pairs > 0 && !arrays)) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_pairs must be >= 0 and every required pair array given");
    return AFIS_OK;
}

}  // namespace

extern "C" {

int afis_score_print_pairs(afis_ctx* ctx, int64_t n_pairs, const int64_t* a_idx, const int64_t* b_idx, const float* w_minu, const float* w_tex, int32_t* status, float* score, float* parts)
{
    const char* const who = "afis_score_print_pairs";
    AFISCHK(check_common(ctx, who, n_pairs, a_idx && b_idx && w_minu && w_tex && status && score));
    for (int k = 0; k < 2; ++k) {
        const float* w = k ? w_tex : w_minu;
        for (int64_t i = 0; i < n_pairs; ++i)
            if (!(w[i] >= 0.0f) || std::isinf(w[i])) return fail(ctx, AFIS_EINVAL, std::string(who) + ": a weight must be finite and >= 0");
    }
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    if (n_pairs == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));                                   // the last search's matrix stays rankable
    Call c{ctx, who, n_pairs, a_idx, b_idx};
    c.G = (int64_t)ctx->res_empty.size(); c.base = ctx->index_base;
    // ---- what holds without the device, into arrays of the call's own; a pair's weights with a zero where the query print does not hold the template
    const size_t N = (size_t)n_pairs;
    std::vector<int32_t> st(N);
    std::vector<float> sc(N), pt(N * 2, 0.0f), wm(N, 0.0f), wt(N, 0.0f);
    std::vector<uint8_t> want_m(N, 0), want_t(N, 0);
    for (size_t i = 0; i < N; ++i) {
        const bool cov = c.covered((int64_t)i);
        st[i] = cov ? AFIS_PAIR_OK : AFIS_PAIR_NOT_COVERED;
        sc[i] = cov ? -1.0f : -std::numeric_limits<float>::infinity();      // -1: nothing of a is active, or b is empty or removed
        if (!cov) continue;
        wm[i] = c.has_minu(a_idx[i]) ? w_minu[i] : 0.0f; wt[i] = c.has_tex(a_idx[i]) ? w_tex[i] : 0.0f;
        want_m[i] = wm[i] != 0.0f; want_t[i] = wt[i] != 0.0f;
    }
    c.make_plan(want_m.data(), want_t.data());
    // ---- batch after batch: the pairs of the batch as a list of (position in the handle, column print) for the pair driver
    std::vector<int32_t> query, b_st;
    std::vector<int64_t> idx;
    std::vector<float> b_wm, b_wt, b_sc, b_pt;
    const int64_t keep_us = ctx->score_pairs_us;                            // (option score_pairs_us describes the last afis_score_pairs: the driver counts there)
    const int rc = c.batches([&](afis_queries* q, size_t first, size_t m) {
        query.assign(c.plan.pos.begin() + first, c.plan.pos.begin() + first + m);
        idx.resize(m); b_wm.resize(m); b_wt.resize(m); b_st.assign(m, 0); b_sc.assign(m, 0.0f); b_pt.assign(2 * m, 0.0f);
        for (size_t k = 0; k < m; ++k) { const size_t i = (size_t)c.plan.pair[first + k]; idx[k] = b_idx[i]; b_wm[k] = wm[i]; b_wt[k] = wt[i]; }
        const PrintPairWeights fold{b_wm.data(), b_wt.data()};
        const int r = score_pairs(ctx, who, q, (int64_t)m, query.data(), idx.data(), b_st.data(), b_sc.data(), b_pt.data(), &fold);
        c.us += ctx->score_pairs_us;
        if (r != AFIS_OK) return r;
        for (size_t k = 0; k < m; ++k) { const size_t i = (size_t)c.plan.pair[first + k]; sc[i] = b_sc[k]; pt[2 * i] = b_pt[2 * k]; pt[2 * i + 1] = b_pt[2 * k + 1]; }
        return (int)AFIS_OK;
    });
    ctx->score_pairs_us = keep_us;
    if (rc == AFIS_OK) {
        memcpy(status, st.data(), N * 4); memcpy(score, sc.data(), N * 4);
        if (parts) memcpy(parts, pt.data(), N * 8);
    }
    return c.end(rc);
}

int afis_correspondences_print_pairs(afis_ctx* ctx, int64_t n_pairs, const int64_t* a_idx, const int64_t* b_idx, int32_t* counts, int16_t* xy, float* part)
{
    const char* const who = "afis_correspondences_print_pairs";
    AFISCHK(check_common(ctx, who, n_pairs, a_idx && b_idx && counts && xy));
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    if (n_pairs == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));                                   // the last search's matrix stays rankable
    Call c{ctx, who, n_pairs, a_idx, b_idx};
    c.G = (int64_t)ctx->res_empty.size(); c.base = ctx->index_base;
    const size_t N = (size_t)n_pairs, row = (size_t)kTopMinu * 4;          // int16 per pair of xy
    std::vector<int32_t> cn(N);
    std::vector<int16_t> out_xy(N * row, 0);
    std::vector<float> pt(N, 0.0f);
    for (size_t i = 0; i < N; ++i) cn[i] = c.covered((int64_t)i) ? AFIS_CORR_NOT_RUN : AFIS_CORR_NOT_COVERED;
    const std::vector<uint8_t> want_m(N, 1);                                // minutiae only: a query print without minutiae is in no batch and keeps its NOT_RUN
    c.make_plan(want_m.data(), nullptr);
    std::vector<int32_t> query, b_cn;
    std::vector<int64_t> idx;
    std::vector<int16_t> b_xy;
    std::vector<float> b_pt;
    const int64_t keep_us = ctx->correspondences_us;                        // (option correspondences_us describes the last afis_correspondences_pairs: the driver counts there)
    const int rc = c.batches([&](afis_queries* q, size_t first, size_t m) {
        query.assign(c.plan.pos.begin() + first, c.plan.pos.begin() + first + m);
        idx.resize(m); b_cn.assign(m, 0); b_xy.assign(m * row, 0); b_pt.assign(m, 0.0f);
        for (size_t k = 0; k < m; ++k) idx[k] = b_idx[(size_t)c.plan.pair[first + k]];
        const int r = correspondences_pairs(ctx, who, q->groups, q->status, q->n_q, (int64_t)m, query.data(), idx.data(), b_cn.data(), b_xy.data(), b_pt.data(), 1);
        c.us += ctx->correspondences_us;
        if (r != AFIS_OK) return r;
        for (size_t k = 0; k < m; ++k) {
            const size_t i = (size_t)c.plan.pair[first + k];
            cn[i] = b_cn[k]; pt[i] = b_pt[k];
            memcpy(&out_xy[i * row], &b_xy[k * row], row * sizeof(int16_t));
        }
        return (int)AFIS_OK;
    });
    ctx->correspondences_us = keep_us;
    if (rc == AFIS_OK) {
        memcpy(counts, cn.data(), N * 4); memcpy(xy, out_xy.data(), N * row * sizeof(int16_t));
        if (part) memcpy(part, pt.data(), N * 4);
    }
    return c.end(rc);
}

// The evidence calls for print pairs (afis_evidence.cpp has the latent forms): the batches' temporary handles carry what the call reads — the texture export a's texture
// template alone, the alignments both templates — and the latent forms' functions run over every batch's pairs.  Their device time, gathers included, goes to the latent
// forms' options; "print_pairs_us" and "print_pairs_query_prints" keep describing the last score or minutiae correspondence call.
int afis_texture_correspondences_print_pairs(afis_ctx* ctx, int64_t n_pairs, const int64_t* a_idx, const int64_t* b_idx, int32_t* counts, int16_t* xy, int16_t* pt, float* sim, float* part)
{
    const char* const who = "afis_texture_correspondences_print_pairs";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null context");
    if (n_pairs < 0 || (n_pairs > 0 && !(a_idx && b_idx && counts && xy))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_pairs must be >= 0 and every pair array but pt, sim and part given");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    ctx->texture_correspondences_us = 0;
    if (n_pairs == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));                                   // the last search's matrix stays rankable
    Call c{ctx, who, n_pairs, a_idx, b_idx};
    c.G = (int64_t)ctx->res_empty.size(); c.base = ctx->index_base;
    const size_t N = (size_t)n_pairs, row = (size_t)kTopTex;               // entries per pair
    std::vector<int32_t> cn(N);
    std::vector<int16_t> out_xy(N * row * 4, 0), out_pt(N * row * 2, 0);
    std::vector<float> out_sim(N * row, 0.0f), out_part(N, 0.0f);
    for (size_t i = 0; i < N; ++i) cn[i] = c.covered((int64_t)i) ? AFIS_CORR_NOT_RUN : AFIS_CORR_NOT_COVERED;
    const std::vector<uint8_t> want_t(N, 1);                                // texture only: a query print without a texture template is in no batch and keeps its NOT_RUN
    c.make_plan(nullptr, want_t.data());
    std::vector<int32_t> query, b_cn;
    std::vector<int64_t> idx;
    std::vector<int16_t> b_xy, b_pt;
    std::vector<float> b_sim, b_part;
    const int rc = c.batches([&](afis_queries* q, size_t first, size_t m) {
        query.assign(c.plan.pos.begin() + first, c.plan.pos.begin() + first + m);
        idx.resize(m); b_cn.assign(m, 0); b_xy.assign(m * row * 4, 0); b_pt.assign(m * row * 2, 0); b_sim.assign(m * row, 0.0f); b_part.assign(m, 0.0f);
        for (size_t k = 0; k < m; ++k) idx[k] = b_idx[(size_t)c.plan.pair[first + k]];
        const int r = texture_correspondences_pairs(ctx, who, q->groups, q->status, q->n_q, (int64_t)m, query.data(), idx.data(), b_cn.data(), b_xy.data(), b_pt.data(), b_sim.data(), b_part.data());
        c.us += ctx->texture_correspondences_us;
        if (r != AFIS_OK) return r;
        for (size_t k = 0; k < m; ++k) {
            const size_t i = (size_t)c.plan.pair[first + k];
            cn[i] = b_cn[k]; out_part[i] = b_part[k];
            memcpy(&out_xy[i * row * 4], &b_xy[k * row * 4], row * 4 * sizeof(int16_t)); memcpy(&out_pt[i * row * 2], &b_pt[k * row * 2], row * 2 * sizeof(int16_t));
            memcpy(&out_sim[i * row], &b_sim[k * row], row * sizeof(float));
        }
        return (int)AFIS_OK;
    });
    ctx->texture_correspondences_us = 0;
    if (rc == AFIS_OK) {
        memcpy(counts, cn.data(), N * 4); memcpy(xy, out_xy.data(), N * row * 4 * sizeof(int16_t));
        if (pt) memcpy(pt, out_pt.data(), N * row * 2 * sizeof(int16_t));
        if (sim) memcpy(sim, out_sim.data(), N * row * sizeof(float));
        if (part) memcpy(part, out_part.data(), N * 4);
    }
    return c.end(rc, &ctx->texture_correspondences_us);
}

int afis_print_pair_alignments(afis_ctx* ctx, int64_t n_pairs, const int64_t* a_idx, const int64_t* b_idx, int32_t* status, afis_corr_moments* out)
{
    const char* const who = "afis_print_pair_alignments";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null context");
    if (n_pairs < 0 || (n_pairs > 0 && !(a_idx && b_idx && status && out))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_pairs must be >= 0 and every pair array given");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    ctx->pair_alignments_us = 0;
    if (n_pairs == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));                                   // the last search's matrix stays rankable
    Call c{ctx, who, n_pairs, a_idx, b_idx};
    c.G = (int64_t)ctx->res_empty.size(); c.base = ctx->index_base;
    const size_t N = (size_t)n_pairs;
    std::vector<int32_t> st(N);
    std::vector<afis_corr_moments> mo(N * 2, afis_corr_moments{0, 0, 0, 0, 0, 0, 0, 0, 0});
    for (size_t i = 0; i < N; ++i) st[i] = c.covered((int64_t)i) ? AFIS_PAIR_OK : AFIS_PAIR_NOT_COVERED;
    const std::vector<uint8_t> want(N, 1);                                  // both templates of a; a print with neither is in no batch and keeps its zeros
    c.make_plan(want.data(), want.data());
    std::vector<int32_t> query, b_st;
    std::vector<int64_t> idx;
    std::vector<afis_corr_moments> b_mo;
    const int rc = c.batches([&](afis_queries* q, size_t first, size_t m) {
        query.assign(c.plan.pos.begin() + first, c.plan.pos.begin() + first + m);
        idx.resize(m); b_st.assign(m, 0); b_mo.resize(m * 2);
        for (size_t k = 0; k < m; ++k) idx[k] = b_idx[(size_t)c.plan.pair[first + k]];
        const int r = pair_alignments(ctx, who, q->groups, q->status, q->n_q, (int64_t)m, query.data(), idx.data(), b_st.data(), b_mo.data(), 2);
        c.us += ctx->pair_alignments_us;
        if (r != AFIS_OK) return r;
        for (size_t k = 0; k < m; ++k) { const size_t i = (size_t)c.plan.pair[first + k]; mo[2 * i] = b_mo[2 * k]; mo[2 * i + 1] = b_mo[2 * k + 1]; }
        return (int)AFIS_OK;
    });
    ctx->pair_alignments_us = 0;
    if (rc == AFIS_OK) { memcpy(status, st.data(), N * 4); memcpy(out, mo.data(), N * 2 * sizeof(afis_corr_moments)); }
    return c.end(rc, &ctx->pair_alignments_us);
}

}  // extern "C"
