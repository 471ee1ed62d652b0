// afis_hits.cpp — hit lists of the C ABI (include/afis_matcher.h): afis_rank_hits lists, per query of the last search, every template whose score reaches a decision
// score, afis_rank_subject_hits every enrolled person — how many there are, and the `cap` best in rank-list order (rank_hits.hip).  Only n_q x (8 + cap x 12 or 20)
// bytes return; the [n_q][G] matrix stays where it is.  The host sequences of a hit-list call and of a call that reads the matrix in place (HitCall, MatrixCall: afis_ctx.h) and the ranking calls' checks live here, for every entry point.
#include "afis_ctx.h"

using namespace afis;

static_assert(kRankHitsMax == AFIS_HITS_MAX, "rank_hits.hip sorts a list of AFIS_HITS_MAX composites in LDS");

namespace afis {

bool HitCall::empty(bool nothing_scored)
{
    if (rows == 0) return true;
    if (!nothing_scored) return false;
    for (int64_t i = 0; i < rows; ++i) n_hits[i] = 0;
    for (size_t o = 0; o < n_out; ++o) { out_a[o] = -1; out_score[o] = -INFINITY; if (out_b) out_b[o] = -1; }
    return true;
}

// the start of both drivers' device work: the call's events, its tables to the device — not timed —, event 0
static int start_call(afis_ctx* ctx, Events& ev, std::initializer_list<HitCall::H2D> uploads, std::initializer_list<HitCall::H2D> filter = {})
{
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    for (const auto& list : {uploads, filter}) for (const HitCall::H2D& u : list) if (u.bytes) HIPCHK(ctx, hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ev[0], ctx->stream));
    return AFIS_OK;
}

int HitCall::begin(std::initializer_list<H2D> uploads)
{
    HIPCHK(ctx, ctx->hits_out.ensure(out_bytes));
    HIPCHK(ctx, ensure_pin(ctx, out_bytes));
    return start_call(ctx, ev, uploads);
}

int MatrixCall::room(std::initializer_list<std::pair<DevBuf*, size_t>> own, size_t pin_bytes)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, fp.ensure());
    if (cells == kPersonBest) HIPCHK(ctx, ctx->subj_best.ensure((size_t)fp.n_q * (size_t)subj->S * 8));
    if (cells == kPersonKeys) HIPCHK(ctx, ensure_subject_keys(ctx, subj));
    for (const auto& r : own) HIPCHK(ctx, r.first->ensure(r.second));
    HIPCHK(ctx, ensure_pin(ctx, pin_bytes));
    return AFIS_OK;
}

int MatrixCall::begin(std::initializer_list<HitCall::H2D> uploads)
{
    AFISCHK(start_call(ctx, ev, uploads, {fp.masks_up(), fp.pairs_up()}));
    if (cells == kPersonKeys) return queue_subject_keys(ctx, subj, fp);
    AFISCHK(fp.queue_cells());                                              // neither masks nor exclusions: nothing, and the search's matrix itself is read
    if (cells == kPersonBest) { AFISCHK(queue_subject_best(ctx, subj, fp.matrix())); AFISCHK(fp.queue_drop_subjects(subj->S)); }   // rank_hits_filtered's sequence: the maxima of the filtered rows, then the excluded persons
    return AFIS_OK;
}

int MatrixCall::finish(const void* src, size_t bytes, int64_t* us)
{
    HIPCHK(ctx, hipEventRecord(ev[1], ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return wait_elapsed(ctx, who, ev, us);                                  // (*us is written on success only)
}

int HitCall::finish(const HitMatrix& m, float min_score, const int32_t* out_row)
{
    hipStream_t s = ctx->stream;
    uint8_t* const d_out = ctx->hits_out.as<uint8_t>();
    uint8_t* const pin = (uint8_t*)ctx->h_pin;
    // template lists compare k_topk's key, which merges the two zeros; subject lists the raw word, as k_topk_subjects' key
    const uint32_t thr = m.subj ? ordered_word(min_score) : rank_key(min_score);
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    HIPCHK(ctx, launch_rank_hits(m.scores, (int)rows, (int)m.cols, m.subj ? ctx->subj_best.as<unsigned long long>() : nullptr, m.subj ? (int)m.subj->S : 0,
                                 m.subj ? m.subj->d_ids.as<long long>() : nullptr, m.map, m.base, thr, cap, (long long*)d_out, (long long*)(d_out + a_at), (float*)(d_out + score_at),
                                 out_b ? (long long*)(d_out + b_at) : nullptr, s));
    HIPCHK(ctx, hipEventRecord(ev[2], s));
    HIPCHK(ctx, hipMemcpyAsync(pin, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    AFISCHK(wait_elapsed(ctx, who, ev, &total_us, &pre_us, &rank_us));
    if (!out_row) {
        memcpy(n_hits, pin, (size_t)rows * 8); memcpy(out_a, pin + a_at, n_out * 8); memcpy(out_score, pin + score_at, n_out * 4);
        if (out_b) memcpy(out_b, pin + b_at, n_out * 8);
        return AFIS_OK;
    }
    const size_t c = (size_t)cap;
    for (int64_t t = 0; t < rows; ++t) {
        const size_t j = (size_t)out_row[t];
        memcpy(n_hits + j, pin + (size_t)t * 8, 8);
        memcpy(out_a + j * c, pin + a_at + (size_t)t * c * 8, c * 8);
        memcpy(out_score + j * c, pin + score_at + (size_t)t * c * 4, c * 4);
        if (out_b) memcpy(out_b + j * c, pin + b_at + (size_t)t * c * 8, c * 8);
    }
    return AFIS_OK;
}

int wait_elapsed(afis_ctx* ctx, const char* who, const Events& ev, int64_t* total_us, int64_t* first_us, int64_t* second_us)
{
    { const int rcw = wait_streams(ctx, {ctx->stream}, who); if (rcw != AFIS_OK) { ctx->last_search.valid = false; return rcw; } }
    float ms = 0, ms_1 = 0, ms_2 = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[ev.n - 1]));
    if (first_us) HIPCHK(ctx, hipEventElapsedTime(&ms_1, ev[0], ev[1]));
    if (second_us) HIPCHK(ctx, hipEventElapsedTime(&ms_2, ev[1], ev[2]));
    *total_us = (int64_t)((double)ms * 1e3);
    if (first_us) *first_us = (int64_t)((double)ms_1 * 1e3);
    if (second_us) *second_us = (int64_t)((double)ms_2 * 1e3);
    return AFIS_OK;
}

int queue_subject_best(afis_ctx* ctx, const afis_subjects* subj, const float* matrix)
{
    const LastSearch& ls = ctx->last_search;
    HIPCHK(ctx, launch_subject_best(matrix, ls.n_q, (int)ls.G, subj->d_slot_of.as<int32_t>(), global_map(ls), (long long)ctx->index_base, (int)subj->S, ctx->subj_best.as<unsigned long long>(), ctx->stream));
    return AFIS_OK;
}

int rank_hits(afis_ctx* ctx, afis_subjects* subj, int n_q, float min_score, int cap, int64_t* n_hits, int64_t* out_a, float* out_score, int64_t* out_b)
{
    const LastSearch ls = ctx->last_search;
    const int64_t G = ls.G, S = subj ? subj->S : 0;
    HitCall hc{ctx, subj ? "afis_rank_subject_hits" : "afis_rank_hits", n_q, cap, n_hits, out_a, out_score, subj ? out_b : nullptr};
    ctx->rank_hits_us = 0;
    if (hc.empty(G == 0 || (subj && S == 0))) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (subj) HIPCHK(ctx, ctx->subj_best.ensure((size_t)n_q * (size_t)S * 8));
    AFISCHK(hc.begin());
    if (subj) AFISCHK(queue_subject_best(ctx, subj, ctx->scores.as<float>()));   // the maxima first, exactly as rank_subjects makes them
    AFISCHK(hc.finish({ctx->scores.as<float>(), G, subj, global_map(ls), (long long)ctx->index_base}, min_score));
    ctx->rank_hits_us = hc.total_us;
    return AFIS_OK;
}

int check_subject_handle(afis_ctx* ctx, const char* who, const afis_subjects* s)
{
    if (std::find(ctx->subject_sets.begin(), ctx->subject_sets.end(), s) != ctx->subject_sets.end()) return AFIS_OK;
    return fail(ctx, AFIS_EINVAL, std::string(who) + ": not a live subject handle of this context");
}

int check_last_search(afis_ctx* ctx, const char* who, int n_q, const afis_subjects* s)
{
    const std::string w(who);
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, w + ": commit the gallery first");
    // the labels are positions of the shard as it was: after an edit they may name other templates
    if (s && s->gallery_epoch != ctx->gallery_epoch) return fail_edited(ctx, who, "these subjects were given; free the handle and create it again");
    if (!ctx->last_search.valid || ctx->last_search.gallery_epoch != ctx->gallery_epoch)
        return fail(ctx, AFIS_ESTATE, w + ": no score matrix to rank: call it after a search that succeeded, before any other call that queues device work or edits the gallery");
    if (n_q != ctx->last_search.n_q) return fail(ctx, AFIS_EINVAL, w + ": n_q is not the last search's");
    return AFIS_OK;
}

int check_hits(afis_ctx* ctx, const char* who, int n_q, float min_score, int cap, bool outputs, const afis_subjects* s)
{
    if (cap < 1 || cap > AFIS_HITS_MAX || !outputs || std::isnan(min_score)) return fail(ctx, AFIS_EINVAL, std::string(who) + ": cap must be 1 .. AFIS_HITS_MAX, min_score a number and every output array given");
    return check_last_search(ctx, who, n_q, s);
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
    AFISCHK(check_subject_handle(ctx, "afis_rank_subject_hits", s));
    const int rc = check_hits(ctx, "afis_rank_subject_hits", n_q, min_score, cap, n_hits && subject_id && subject_score && best_idx, s);
    return rc != AFIS_OK ? rc : rank_hits(ctx, s, n_q, min_score, cap, n_hits, subject_id, subject_score, best_idx);
}

}  // extern "C"
