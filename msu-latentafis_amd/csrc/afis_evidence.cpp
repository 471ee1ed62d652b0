// afis_evidence.cpp — the evidence calls of the C ABI (include/afis_matcher.h) for a LIST of (latent, rolled print) pairs: afis_texture_correspondences_pairs gives the
// surviving correspondences of the TEXTURE scorer (matcher.cpp:767-781: corr3 in the reference's list order) as coordinates, template indices and similarities, and
// afis_pair_alignments the exact moments (pair_moments.h) of all four scorers' survivors, 288 bytes a pair, from which afis_alignment_fit places the latent on the print.
// Both are the pair-list calls' one driver (PairCall, afis_ctx.h; afis_pairs.cpp) in its evidence form: the score form's launch sequence — candidates, minutiae lists,
// exact texture row maxima, texture lists — with the texture list kernel's tap after S9 switched on, and pair_evidence.hip's kernel behind every launch group's launches;
// what that kernel wrote is the one run that returns.  What is stated here is what differs: which pairs go to the device, what the arrays hold without it, and where a
// slot's results go.  The forms for resident print pairs (afis_print_pairs.cpp) run these functions over temporary handles of prints' views.
// The host-only helpers afis_corr_moments_add and afis_alignment_fit are pair_moments.h's arithmetic behind argument checks.
// The last search's matrix is neither written nor invalidated, as by every pair call.
#include "afis_ctx.h"

using namespace afis;

static_assert(sizeof(afis_corr_moments) == sizeof(CorrMoments) && sizeof(CorrMoments) == 72 && offsetof(afis_corr_moments, rr) == offsetof(CorrMoments, rr), "afis_corr_moments is pair_moments.h's record");
static_assert(AFIS_TEX_CORR_MAX == kTopTex, "the texture scorer's list");

namespace afis {

int texture_correspondences_pairs(afis_ctx* ctx, const char* who, const std::vector<QueryGroup>& groups, const std::vector<int32_t>& status, int n_q, int64_t n_pairs,
                                  const int32_t* query, const int64_t* idx, int32_t* counts, int16_t* xy, int16_t* pt, float* sim, float* part)
{
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    std::vector<uint8_t> has((size_t)n_q, 0);                              // whether the reference runs the texture scorer for a query: scored at all, and with a texture template
    {
        int q0 = 0;
        for (const QueryGroup& grp : groups) {
            for (int j = 0; j < grp.nq && q0 + j < n_q; ++j) has[(size_t)(q0 + j)] = status[(size_t)(q0 + j)] == AFIS_QUERY_OK && grp.h_lt_n[(size_t)j] > 0;
            q0 += grp.nq;
        }
    }
    PairCall c{ctx, who, groups, n_q, n_pairs, query, idx, ctx->corr_pairs_per_launch, &ctx->texture_correspondences_us, true, nullptr, kPairTexExport};
    // a covered print with a texture template and a latent with one (matcher.cpp:411)
    c.needs_device = [&](int64_t i) {
        const int64_t t = idx[i] - base;
        return t >= 0 && t < G && !ctx->res_empty[(size_t)t] && ctx->res_to[(size_t)t + 1] - ctx->res_to[(size_t)t] > 0 && has[(size_t)query[i]] != 0;
    };
    // -2 outside the shard, -1 where the reference does not call the scorer
    c.defaults = [&] {
        memset(xy, 0, (size_t)n_pairs * kTopTex * 4 * sizeof(int16_t));
        if (pt) memset(pt, 0, (size_t)n_pairs * kTopTex * 2 * sizeof(int16_t));
        if (sim) memset(sim, 0, (size_t)n_pairs * kTopTex * sizeof(float));
        for (int64_t i = 0; i < n_pairs; ++i) {
            const int64_t t = idx[i] - base;
            counts[i] = (t < 0 || t >= G) ? AFIS_CORR_NOT_COVERED : AFIS_CORR_NOT_RUN;
            if (part) part[i] = 0.0f;
        }
    };
    c.stage = [&](const PairGroup& g) -> int {
        AFISCHK(queue_texture_pairs(ctx, ctx->gal, g.qd, g.tab, g.n, g.seg, g.n_seg, g.rm_val, g.rm_arg, g.parts, ctx->pair_tex_slab, nullptr, ctx->stream, g.ev.tap, g.ev.tap_n));
        HIPCHK(ctx, launch_pair_evidence(g.qd, ctx->gal, g.tab, g.n, g.ev, ctx->stream));
        return AFIS_OK;
    };
    c.take = [&](int64_t i, size_t slot, const PairBack& b) {
        const int32_t n = std::min(b.ex_n[slot], (int32_t)kTopTex);
        if (n < 0) return;                                                  // (the device's own -1: the host's tables said the same)
        counts[i] = n;
        memcpy(xy + (size_t)i * kTopTex * 4, b.ex_xy + slot * kTopTex, (size_t)n * sizeof(short4));
        if (pt) memcpy(pt + (size_t)i * kTopTex * 2, b.ex_pt + slot * kTopTex, (size_t)n * sizeof(short2));
        if (sim) memcpy(sim + (size_t)i * kTopTex, b.ex_sim + slot * kTopTex, (size_t)n * sizeof(float));
        if (part) part[i] = b.ex_part[slot];
    };
    return c.run();
}

int pair_alignments(afis_ctx* ctx, const char* who, const std::vector<QueryGroup>& groups, const std::vector<int32_t>& status, int n_q, int64_t n_pairs,
                    const int32_t* query, const int64_t* idx, int32_t* pair_status, afis_corr_moments* out, int records)
{
    const size_t R = records == 2 ? 2 : 4;                                 // records per pair in the caller's array: all four scorers, or scorer 0 and the texture scorer (a print's view has no other)
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    PairCall c{ctx, who, groups, n_q, n_pairs, query, idx, ctx->corr_pairs_per_launch, &ctx->pair_alignments_us, true, nullptr, kPairMoments};
    // a covered print that is not empty and a latent the reference scores: the list kernels leave an empty list for every scorer it does not run
    c.needs_device = [&](int64_t i) { const int64_t t = idx[i] - base; return t >= 0 && t < G && status[(size_t)query[i]] == AFIS_QUERY_OK && !ctx->res_empty[(size_t)t]; };
    c.defaults = [&] {
        memset(out, 0, (size_t)n_pairs * R * sizeof(afis_corr_moments));
        for (int64_t i = 0; i < n_pairs; ++i) { const int64_t t = idx[i] - base; pair_status[i] = t >= 0 && t < G ? AFIS_PAIR_OK : AFIS_PAIR_NOT_COVERED; }
    };
    c.stage = [&](const PairGroup& g) -> int {
        AFISCHK(queue_texture_pairs(ctx, ctx->gal, g.qd, g.tab, g.n, g.seg, g.n_seg, g.rm_val, g.rm_arg, g.parts, ctx->pair_tex_slab, nullptr, ctx->stream, g.ev.tap, g.ev.tap_n));
        HIPCHK(ctx, launch_pair_evidence(g.qd, ctx->gal, g.tab, g.n, g.ev, ctx->stream));
        return AFIS_OK;
    };
    c.take = [&](int64_t i, size_t slot, const PairBack& b) {
        if (R == 4) { memcpy(out + (size_t)i * 4, b.mom + slot * 4, 4 * sizeof(CorrMoments)); return; }
        memcpy(out + (size_t)i * 2, b.mom + slot * 4, sizeof(CorrMoments)); memcpy(out + (size_t)i * 2 + 1, b.mom + slot * 4 + 3, sizeof(CorrMoments));
    };
    return c.run();
}

}  // namespace afis

extern "C" {

int afis_texture_correspondences_pairs(afis_ctx* ctx, afis_queries* q, int64_t n_pairs, const int32_t* query, const int64_t* idx, int32_t* counts, int16_t* xy, int16_t* pt,
                                       float* sim, float* part)
{
    const char* const who = "afis_texture_correspondences_pairs";
    if (!ctx || !q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    if (n_pairs < 0 || (n_pairs > 0 && !(query && idx && counts && xy))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_pairs must be >= 0 and every pair array but pt, sim and part given");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    ctx->texture_correspondences_us = 0;
    if (n_pairs == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));                                   // the last search's matrix stays rankable
    return texture_correspondences_pairs(ctx, who, q->groups, q->status, q->n_q, n_pairs, query, idx, counts, xy, pt, sim, part);
}

int afis_pair_alignments(afis_ctx* ctx, afis_queries* q, int64_t n_pairs, const int32_t* query, const int64_t* idx, int32_t* status, afis_corr_moments* out)
{
    const char* const who = "afis_pair_alignments";
    if (!ctx || !q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    if (n_pairs < 0 || (n_pairs > 0 && !(query && idx && status && out))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_pairs must be >= 0 and every pair array given");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    ctx->pair_alignments_us = 0;
    if (n_pairs == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));                                   // the last search's matrix stays rankable
    return pair_alignments(ctx, who, q->groups, q->status, q->n_q, n_pairs, query, idx, status, out, 4);
}

int afis_corr_moments_add(afis_corr_moments* acc, const afis_corr_moments* other)
{
    if (!acc || !other) return AFIS_EINVAL;
    CorrMoments a, o;
    memcpy(&a, acc, sizeof a); memcpy(&o, other, sizeof o);
    if (mom_add(a, o) != 0) return AFIS_EINVAL;
    memcpy(acc, &a, sizeof a);
    return AFIS_OK;
}

int afis_alignment_fit(const afis_corr_moments* m, double* c, double* s, double* tx, double* ty, double* rms)
{
    if (!m) return AFIS_EINVAL;
    CorrMoments r;
    memcpy(&r, m, sizeof r);
    return mom_fit(r, c, s, tx, ty, rms) == 0 ? AFIS_OK : AFIS_EINVAL;
}

}  // extern "C"
