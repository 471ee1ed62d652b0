// afis_hits.cpp — hit lists of the C ABI (include/afis_matcher.h): afis_rank_hits lists, per query of the last search, every template whose score reaches a decision
// score, afis_rank_subject_hits every enrolled person — how many there are, and the `cap` best in rank-list order (rank_hits.hip).  Only n_q x (8 + cap x 12 or 20)
// bytes return; the [n_q][G] matrix stays where it is.
#include "afis_ctx.h"

using namespace afis;

static_assert(kRankHitsMax == AFIS_HITS_MAX, "rank_hits.hip sorts a list of AFIS_HITS_MAX composites in LDS");

namespace afis {

int rank_hits(afis_ctx* ctx, afis_subjects* subj, int n_q, float min_score, int cap, int64_t* n_hits, int64_t* out_a, float* out_score, int64_t* out_b)
{
    const LastSearch ls = ctx->last_search;
    const int64_t G = ls.G, S = subj ? subj->S : 0;
    const size_t n_out = (size_t)n_q * (size_t)cap;
    ctx->rank_hits_us = 0;
    if (n_q == 0) return AFIS_OK;
    if (G == 0 || (subj && S == 0)) {                                       // nothing was scored: no hit, every entry is padding
        for (int i = 0; i < n_q; ++i) n_hits[i] = 0;
        for (size_t o = 0; o < n_out; ++o) { out_a[o] = -1; out_score[o] = -INFINITY; if (subj) out_b[o] = -1; }
        return AFIS_OK;
    }
    // template hits compare k_topk's key, which adds + 0.0f to the score (-0.0 -> +0.0); subject hits compare the raw word, as k_topk_subjects' key
    const uint32_t thr = ordered_word(subj ? min_score : min_score + 0.0f);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // room first: a failed allocation leaves everything as it was
    if (subj) HIPCHK(ctx, ctx->subj_best.ensure((size_t)n_q * (size_t)S * 8));
    const size_t a_at = (size_t)n_q * 8, b_at = a_at + n_out * 8, score_at = b_at + (subj ? n_out * 8 : 0), out_bytes = score_at + n_out * 4;
    HIPCHK(ctx, ctx->hits_out.ensure(out_bytes));
    HIPCHK(ctx, ensure_pin(ctx, out_bytes));
    hipStream_t s = ctx->stream;
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } drop_ev{ev};
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    const long long* const d_global = ls.sub ? ls.sub->d_global.as<long long>() : nullptr;
    uint8_t* const d_out = ctx->hits_out.as<uint8_t>();
    uint8_t* const pin = (uint8_t*)ctx->h_pin;
    HIPCHK(ctx, hipEventRecord(ev[0], s));
    if (subj)                                                               // the maxima first, exactly as rank_subjects makes them
        HIPCHK(ctx, launch_subject_best(ctx->scores.as<float>(), n_q, (int)G, subj->d_slot_of.as<int32_t>(), d_global, (long long)ctx->index_base, (int)S,
                                        ctx->subj_best.as<unsigned long long>(), s));
    HIPCHK(ctx, launch_rank_hits(ctx->scores.as<float>(), n_q, (int)G, subj ? ctx->subj_best.as<unsigned long long>() : nullptr, (int)S, subj ? subj->d_ids.as<long long>() : nullptr,
                                 d_global, (long long)ctx->index_base, thr, cap, (long long*)d_out, (long long*)(d_out + a_at), (float*)(d_out + score_at),
                                 subj ? (long long*)(d_out + b_at) : nullptr, s));
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    HIPCHK(ctx, hipMemcpyAsync(pin, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    { const int rcw = wait_streams(ctx, {s}, subj ? "afis_rank_subject_hits" : "afis_rank_hits"); if (rcw != AFIS_OK) { ctx->last_search.valid = false; return rcw; } }
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    ctx->rank_hits_us = (int64_t)((double)ms * 1e3);
    memcpy(n_hits, pin, (size_t)n_q * 8); memcpy(out_a, pin + a_at, n_out * 8); memcpy(out_score, pin + score_at, n_out * 4);
    if (subj) memcpy(out_b, pin + b_at, n_out * 8);
    return AFIS_OK;
}

// what the hit-list entry points ask of the context and of their plain arguments (the order of afis_rank_subjects' checks)
int check_hits(afis_ctx* ctx, const char* who, int n_q, float min_score, int cap, bool outputs, const afis_subjects* s)
{
    const std::string w(who);
    if (cap < 1 || cap > AFIS_HITS_MAX || !outputs || std::isnan(min_score)) return fail(ctx, AFIS_EINVAL, w + ": cap must be 1 .. AFIS_HITS_MAX, min_score a number and every output array given");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, w + ": commit the gallery first");
    if (s && s->gallery_epoch != ctx->gallery_epoch)
        return fail(ctx, AFIS_ESTATE, w + ": the gallery was edited (afis_gallery_commit after afis_gallery_reopen, afis_gallery_remove) after these subjects were given; free the handle and create it again");
    if (!ctx->last_search.valid || ctx->last_search.gallery_epoch != ctx->gallery_epoch)
        return fail(ctx, AFIS_ESTATE, w + ": no score matrix to rank: call it after a search that succeeded, before any other call that queues device work or edits the gallery");
    if (n_q != ctx->last_search.n_q) return fail(ctx, AFIS_EINVAL, w + ": n_q is not the last search's");
    return AFIS_OK;
}

}  // namespace afis

extern "C" {

int afis_rank_hits(afis_ctx* ctx, int n_q, float min_score, int cap, int64_t* n_hits, int64_t* idx, float* score)
{
    if (!ctx) return fail(ctx, AFIS_EINVAL, "afis_rank_hits: null argument");
    const int rc = check_hits(ctx, "afis_rank_hits", n_q, min_score, cap, n_hits && idx && score, nullptr);
    return rc != AFIS_OK ? rc : rank_hits(ctx, nullptr, n_q, min_score, cap, n_hits, idx, score, nullptr);
}

int afis_rank_subject_hits(afis_ctx* ctx, afis_subjects* s, int n_q, float min_score, int cap, int64_t* n_hits, int64_t* subject_id, float* subject_score, int64_t* best_idx)
{
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, "afis_rank_subject_hits: null argument");
    if (std::find(ctx->subject_sets.begin(), ctx->subject_sets.end(), s) == ctx->subject_sets.end()) return fail(ctx, AFIS_EINVAL, "afis_rank_subject_hits: not a live subject handle of this context");
    const int rc = check_hits(ctx, "afis_rank_subject_hits", n_q, min_score, cap, n_hits && subject_id && subject_score && best_idx, s);
    return rc != AFIS_OK ? rc : rank_hits(ctx, s, n_q, min_score, cap, n_hits, subject_id, subject_score, best_idx);
}

}  // extern "C"
