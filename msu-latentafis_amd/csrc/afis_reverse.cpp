// afis_reverse.cpp — the reverse search of the C ABI (include/afis_matcher.h): a file of unsolved latents kept on the device is searched against every newly enrolled card.
// Two things make that a transaction of its own.  afis_queries_upload_reserved cuts a handle's launch groups for a shard of a stated size instead of the resident one, so
// that the handle outlives the enrolments and serves every subset up to that size (afis_search.cpp::upload_queries does the cutting).  afis_rank_latent_hits ranks the
// score matrix of the last search along its columns — per print, which latents reach the decision score — on the device: the matrix is transposed (latent_rank.hip) and
// k_rank_hits (rank_hits.hip) runs on the transposed rows as it runs on a search's.  Only n_templates x (8 + cap x 12) bytes return.
#include "afis_ctx.h"

using namespace afis;

namespace afis {

// afis_rank_latent_hits behind its argument checks: the matrix is ctx->scores, [ls.n_q][ls.G] in the order of the shard searched
static int rank_latent_hits(afis_ctx* ctx, float min_score, int cap, int64_t latent_base, int64_t* n_hits, int64_t* latent_idx, float* score)
{
    const LastSearch ls = ctx->last_search;
    const int64_t n = ls.G;
    const int n_q = ls.n_q;
    const size_t n_out = (size_t)n * (size_t)cap;
    ctx->rank_latents_us = 0; ctx->transpose_us = 0; ctx->transpose_bytes = 0;
    if (n == 0) return AFIS_OK;
    if (n_q == 0) {                                                         // no query was scored: no hit, every entry is padding
        for (int64_t j = 0; j < n; ++j) n_hits[j] = 0;
        for (size_t o = 0; o < n_out; ++o) { latent_idx[o] = -1; score[o] = -INFINITY; }
        return AFIS_OK;
    }
    const uint32_t thr = ordered_word(min_score + 0.0f);                    // k_topk's key: -0.0 -> +0.0
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // room first: a failed allocation leaves everything as it was
    HIPCHK(ctx, ctx->scores_t.ensure((size_t)n * (size_t)n_q * 4));
    const size_t idx_at = (size_t)n * 8, score_at = idx_at + n_out * 8, out_bytes = score_at + n_out * 4;
    HIPCHK(ctx, ctx->hits_out.ensure(out_bytes));
    HIPCHK(ctx, ensure_pin(ctx, out_bytes));
    hipStream_t s = ctx->stream;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 3; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } drop_ev{ev};
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    uint8_t* const d_out = ctx->hits_out.as<uint8_t>();
    uint8_t* const pin = (uint8_t*)ctx->h_pin;
    HIPCHK(ctx, hipEventRecord(ev[0], s));
    HIPCHK(ctx, launch_transpose_scores(ctx->scores.as<float>(), ctx->scores_t.as<float>(), n_q, (int)n, s));
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    // rows = the prints, in the order of the shard searched; entries = the queries: position + latent_base, equal keys by ascending position
    HIPCHK(ctx, launch_rank_hits(ctx->scores_t.as<float>(), (int)n, n_q, nullptr, 0, nullptr, nullptr, (long long)latent_base, thr, cap, (long long*)d_out, (long long*)(d_out + idx_at),
                                 (float*)(d_out + score_at), nullptr, s));
    HIPCHK(ctx, hipEventRecord(ev[2], s));
    HIPCHK(ctx, hipMemcpyAsync(pin, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    { const int rcw = wait_streams(ctx, {s}, "afis_rank_latent_hits"); if (rcw != AFIS_OK) { ctx->last_search.valid = false; return rcw; } }
    float ms = 0, ms_t = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[2]));
    HIPCHK(ctx, hipEventElapsedTime(&ms_t, ev[0], ev[1]));
    ctx->rank_latents_us = (int64_t)((double)ms * 1e3);
    ctx->transpose_us = (int64_t)((double)ms_t * 1e3); ctx->transpose_bytes = (int64_t)n * n_q * 8;
    if (!ls.sub || ls.sub->identity) {
        memcpy(n_hits, pin, (size_t)n * 8); memcpy(latent_idx, pin + idx_at, n_out * 8); memcpy(score, pin + score_at, n_out * 4);
        return AFIS_OK;
    }
    // A subset listed out of order: the sub-shard, and so the transposed rows, stand in ascending global index order.  Row j of the outputs is the caller's idx[j]: the
    // small lists are put in that order here (the rank of idx[j] among the listed indices is its position in the sub-shard, afis_subset_create).
    const std::vector<int64_t>& idx = ls.sub->idx;
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&idx](int32_t a, int32_t b) { return idx[(size_t)a] < idx[(size_t)b]; });
    for (int64_t t = 0; t < n; ++t) {
        const size_t j = (size_t)order[(size_t)t];
        memcpy(n_hits + j, pin + (size_t)t * 8, 8);
        memcpy(latent_idx + j * (size_t)cap, pin + idx_at + (size_t)t * (size_t)cap * 8, (size_t)cap * 8);
        memcpy(score + j * (size_t)cap, pin + score_at + (size_t)t * (size_t)cap * 4, (size_t)cap * 4);
    }
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
    return rank_latent_hits(ctx, min_score, cap, latent_base, n_hits, latent_idx, score);
}

}  // extern "C"
