// afis_reverse.cpp — the reverse search of the C ABI (include/afis_matcher.h): a file of unsolved latents kept on the device is searched against every newly enrolled card.
// Two things make that a transaction of its own.  afis_queries_upload_reserved cuts a handle's launch groups for a shard of a stated size instead of the resident one, so
// that the handle outlives the enrolments and serves every subset up to that size (afis_search.cpp::upload_queries does the cutting).  afis_rank_latent_hits ranks the
// score matrix of the last search along its columns — per print, which latents reach the decision score — on the device: the matrix is transposed (latent_rank.hip) and
// k_rank_hits (rank_hits.hip) runs on the transposed rows as it runs on a search's.  Only n_templates x (8 + cap x 12) bytes return.  afis_rank_latent_hits_filtered
// transposes the filtered copy (FilterPass, afis_filter.cpp) instead: per print, only the latents that are eligible for it.
#include "afis_ctx.h"

using namespace afis;

namespace afis {

// afis_rank_latent_hits and afis_rank_latent_hits_filtered behind their argument checks: the matrix is ctx->scores, [ls.n_q][ls.G] in the order of the shard searched;
// pairs: the exclusions as check_filtered resolved them.  Neither masks nor pairs: the search's matrix itself is transposed
static int rank_latent_hits(afis_ctx* ctx, const char* who, const afis_labels* labels, const uint64_t* masks, const std::vector<int32_t>& pairs, float min_score, int cap,
                            int64_t latent_base, int64_t* n_hits, int64_t* latent_idx, float* score)
{
    const LastSearch ls = ctx->last_search;
    const int64_t n = ls.G;
    const int n_q = ls.n_q;
    HitCall hc{ctx, who, n, cap, n_hits, latent_idx, score, nullptr};
    ctx->rank_latents_us = 0; ctx->transpose_us = 0; ctx->transpose_bytes = 0;
    if (hc.empty(n_q == 0)) return AFIS_OK;                                 // (no query was scored: no hit)
    // A subset listed out of order: the sub-shard, and so the transposed rows, stand in ascending global index order.  Row j of the outputs is the caller's idx[j]: the
    // small lists are put in that order on the way out (the rank of idx[j] among the listed indices is its position in the sub-shard, afis_subset_create).
    std::vector<int32_t> order(ls.sub && !ls.sub->identity ? (size_t)n : 0);
    if (!order.empty()) {
        const std::vector<int64_t>& idx = ls.sub->idx;
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin(), order.end(), [&idx](int32_t a, int32_t b) { return idx[(size_t)a] < idx[(size_t)b]; });
    }
    FilterPass fp{ctx, labels, masks, pairs, false};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, fp.ensure());
    HIPCHK(ctx, ctx->scores_t.ensure((size_t)n * (size_t)n_q * 4));
    AFISCHK(hc.begin({fp.masks_up(), fp.pairs_up()}));
    AFISCHK(fp.queue_cells());                                              // (no filter: nothing, and fp.matrix() is the search's)
    HIPCHK(ctx, launch_transpose_scores(fp.matrix(), ctx->scores_t.as<float>(), n_q, (int)n, ctx->stream));
    // rows = the prints, in the order of the shard searched; entries = the queries: position + latent_base, equal keys by ascending position (launch_rank_hits' template form)
    AFISCHK(hc.finish({ctx->scores_t.as<float>(), n_q, nullptr, nullptr, (long long)latent_base}, min_score, order.empty() ? nullptr : order.data()));
    ctx->rank_latents_us = hc.total_us;
    ctx->transpose_us = hc.pre_us; ctx->transpose_bytes = (int64_t)n * n_q * 8;   // (a filtered call: pre_us holds the filter pass too)
    return AFIS_OK;
}

}  // namespace afis

extern "C" {

int afis_queries_upload_reserved(afis_ctx* ctx, const afis_template_view* queries, int n_q, int64_t max_templates, afis_queries** out)
{
    if (!ctx || !out || n_q < 0 || (n_q > 0 && !queries)) return fail(ctx, AFIS_EINVAL, "afis_queries_upload_reserved: bad argument");
    if (max_templates < 1) return fail(ctx, AFIS_EINVAL, "afis_queries_upload_reserved: max_templates must be at least 1");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_queries_upload_reserved: commit the gallery first");
    return upload_queries(ctx, queries, n_q, max_templates, out);
}

int afis_rank_latent_hits(afis_ctx* ctx, int64_t n_templates, float min_score, int cap, int64_t latent_base, int64_t* n_hits, int64_t* latent_idx, float* score)
{
    if (!ctx) return fail(ctx, AFIS_EINVAL, "afis_rank_latent_hits: null argument");
    if (latent_base < 0) return fail(ctx, AFIS_EINVAL, "afis_rank_latent_hits: latent_base must not be negative");
    const int rc = check_hits(ctx, "afis_rank_latent_hits", ctx->last_search.n_q, min_score, cap, n_hits && latent_idx && score, nullptr);
    if (rc != AFIS_OK) return rc;
    if (n_templates != ctx->last_search.G)
        return fail(ctx, AFIS_EINVAL, "afis_rank_latent_hits: n_templates is " + std::to_string((long long)n_templates) + ", the last search covered " + std::to_string((long long)ctx->last_search.G) + " templates");
    return rank_latent_hits(ctx, "afis_rank_latent_hits", nullptr, nullptr, {}, min_score, cap, latent_base, n_hits, latent_idx, score);
}

int afis_rank_latent_hits_filtered(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl,
                                   int64_t n_templates, float min_score, int cap, int64_t latent_base, int64_t* n_hits, int64_t* latent_idx, float* score)
{
    const char* const who = "afis_rank_latent_hits_filtered";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    if (latent_base < 0) return fail(ctx, AFIS_EINVAL, std::string(who) + ": latent_base must not be negative");
    std::vector<int32_t> pairs;
    const int rc = check_filtered(ctx, who, nullptr, labels, masks, excl_off, excl, ctx->last_search.n_q, min_score, cap, n_hits && latent_idx && score, pairs);
    if (rc != AFIS_OK) return rc;
    if (n_templates != ctx->last_search.G)
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_templates is " + std::to_string((long long)n_templates) + ", the last search covered " + std::to_string((long long)ctx->last_search.G) + " templates");
    return rank_latent_hits(ctx, who, labels, masks, pairs, min_score, cap, latent_base, n_hits, latent_idx, score);
}

}  // extern "C"
