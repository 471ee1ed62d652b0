// afis_subjects.cpp — subject rank lists of the C ABI (include/afis_matcher.h): afis_subjects_create labels every template of the resident shard with the enrolled person
// it belongs to, afis_rank_subjects groups the score matrix the last search left on the device by those labels — per (query, subject) the best score and the template
// that reached it — and lists the k best subjects of every query (subject_rank.hip).  Only n_q x k x 20 bytes return; the [n_q][G] matrix stays where it is.
#include "afis_ctx.h"

using namespace afis;

namespace afis {

void release_subjects(afis_subjects* s)
{
    if (!s) return;
    s->d_slot_of.release(); s->d_ids.release();
    delete s;
}

static void pad_entry(int64_t* id, float* score, int64_t* best) { *id = -1; *score = -INFINITY; *best = -1; }

int rank_subjects(afis_ctx* ctx, afis_subjects* subj, int n_q, int k, int64_t* subject_id, float* subject_score, int64_t* best_idx)
{
    const LastSearch ls = ctx->last_search;
    const int64_t G = ls.G, S = subj->S;
    const size_t n_out = (size_t)n_q * (size_t)k;
    ctx->subject_rank_us = 0;
    if (n_q == 0) return AFIS_OK;
    if (G == 0 || S == 0) {                                                // nothing was scored: every entry is padding
        for (size_t o = 0; o < n_out; ++o) pad_entry(subject_id + o, subject_score + o, best_idx + o);
        return AFIS_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool dev_topk = k <= kDeviceTopK;
    // room first: a failed allocation leaves everything as it was
    HIPCHK(ctx, ctx->subj_best.ensure((size_t)n_q * (size_t)S * 8));
    const size_t score_at = n_out * 8, best_at = (score_at + n_out * 4 + 7) / 8 * 8, out_bytes = best_at + n_out * 8;
    if (dev_topk) {
        HIPCHK(ctx, ctx->subj_out.ensure(out_bytes));
        HIPCHK(ctx, ensure_pin(ctx, out_bytes));
    }
    hipStream_t s = ctx->stream;
    Events ev(2);
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    uint8_t* const d_out = ctx->subj_out.as<uint8_t>();
    uint8_t* const pin = (uint8_t*)ctx->h_pin;
    HIPCHK(ctx, hipEventRecord(ev[0], s));
    AFISCHK(queue_subject_best(ctx, subj, ctx->scores.as<float>()));
    if (dev_topk)
        HIPCHK(ctx, launch_topk_subjects(ctx->subj_best.as<unsigned long long>(), n_q, (int)S, subj->d_ids.as<long long>(), ctx->scores.as<float>(), (int)G, global_map(ls),
                                         (long long)ctx->index_base, k, (long long*)d_out, (float*)(d_out + score_at), (long long*)(d_out + best_at), s));
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    if (dev_topk) HIPCHK(ctx, hipMemcpyAsync(pin, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    AFISCHK(wait_elapsed(ctx, "afis_rank_subjects", ev, &ctx->subject_rank_us));
    if (dev_topk) {
        memcpy(subject_id, pin, n_out * 8); memcpy(subject_score, pin + score_at, n_out * 4); memcpy(best_idx, pin + best_at, n_out * 8);
        return AFIS_OK;
    }
    // k > kDeviceTopK: the [n_q][S] maxima come to the host and are sorted there on the same keys.  A composite carries the score's own bits (the ordered form is a
    // bijection of the word) and the position; a subset's positions are its listed indices in ascending order.
    std::vector<unsigned long long> best((size_t)n_q * (size_t)S);
    HIPCHK(ctx, hipMemcpy(best.data(), ctx->subj_best.p, best.size() * 8, hipMemcpyDeviceToHost));
    const ColumnNames columns = column_names(ctx, nullptr);
    std::vector<unsigned long long> keys;
    for (int i = 0; i < n_q; ++i) {
        const unsigned long long* row = best.data() + (size_t)i * (size_t)S;
        keys.clear();
        for (int64_t e = 0; e < S; ++e) if (row[e]) keys.push_back(composite_at(row[e], (uint32_t)e));
        const size_t kk = std::min<size_t>((size_t)k, keys.size());
        std::partial_sort(keys.begin(), keys.begin() + kk, keys.end(), std::greater<unsigned long long>());
        for (int r = 0; r < k; ++r) {
            const size_t o = (size_t)i * k + r;
            if ((size_t)r >= kk) { pad_entry(subject_id + o, subject_score + o, best_idx + o); continue; }
            const uint32_t slot = composite_position(keys[(size_t)r]), pos = composite_position(row[slot]), bits = score_bits_of(composite_word(keys[(size_t)r]));
            subject_id[o] = subj->ids[slot];
            memcpy(subject_score + o, &bits, 4);
            best_idx[o] = columns.name(pos);
        }
    }
    return AFIS_OK;
}

}  // namespace afis

extern "C" {

int afis_subjects_create(afis_ctx* ctx, const int64_t* subject, int64_t n, afis_subjects** out)
{
    if (!ctx || !out || n < 0 || (n > 0 && !subject)) return fail(ctx, AFIS_EINVAL, "afis_subjects_create: bad argument");
    *out = nullptr;
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_subjects_create: commit the gallery first");
    if (n != (int64_t)ctx->res_empty.size()) return fail(ctx, AFIS_EINVAL, "afis_subjects_create: one subject id per template of the resident shard (option gallery_resident)");
    for (int64_t i = 0; i < n; ++i) if (subject[i] < 0) return fail(ctx, AFIS_EINVAL, "afis_subjects_create: a subject id is negative");
    std::unique_ptr<afis_subjects> sj(new afis_subjects());
    sj->n = n; sj->gallery_epoch = ctx->gallery_epoch;
    sj->ids.assign(subject, subject + n);
    std::sort(sj->ids.begin(), sj->ids.end());
    sj->ids.erase(std::unique(sj->ids.begin(), sj->ids.end()), sj->ids.end());
    sj->S = (int64_t)sj->ids.size();
    std::vector<int32_t> slot_of((size_t)n);
    for (int64_t i = 0; i < n; ++i) slot_of[(size_t)i] = (int32_t)(std::lower_bound(sj->ids.begin(), sj->ids.end(), subject[i]) - sj->ids.begin());
    { const int rcq = quiesce(ctx, "afis_subjects_create", true); if (rcq != AFIS_OK) return rcq; }
    if (n > 0) {
        const int64_t h2d_before = ctx->gallery_h2d_bytes;
        auto tables = [&]() -> int {
            HIPCHK(ctx, sj->d_slot_of.ensure(slot_of.size() * 4)); HIPCHK(ctx, sj->d_ids.ensure(sj->ids.size() * 8));
            HIPCHK(ctx, hipMemcpyAsync(sj->d_slot_of.p, slot_of.data(), slot_of.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(sj->d_ids.p, sj->ids.data(), sj->ids.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            ctx->gallery_h2d_bytes += (int64_t)(slot_of.size() * 4 + sj->ids.size() * 8);
            return wait_streams(ctx, {ctx->stream}, "afis_subjects_create");
        };
        const int rc = tables();
        if (rc != AFIS_OK) {                                                // nothing allocated, nothing changed
            (void)hipStreamSynchronize(ctx->stream);
            ctx->gallery_h2d_bytes = h2d_before;
            release_subjects(sj.release());
            return rc;
        }
    }
    ctx->subject_sets.push_back(sj.get());
    *out = sj.release();
    return AFIS_OK;
}

void afis_subjects_free(afis_ctx* ctx, afis_subjects* s)
{
    if (!s) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)quiesce(ctx, "afis_subjects_free", true);
        ctx->subject_sets.erase(std::remove(ctx->subject_sets.begin(), ctx->subject_sets.end(), s), ctx->subject_sets.end());
    }
    release_subjects(s);
}

int afis_rank_subjects(afis_ctx* ctx, afis_subjects* s, int n_q, int k, int64_t* subject_id, float* subject_score, int64_t* best_idx)
{
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, "afis_rank_subjects: null argument");
    AFISCHK(check_subject_handle(ctx, "afis_rank_subjects", s));
    if (k <= 0 || !subject_id || !subject_score || !best_idx) return fail(ctx, AFIS_EINVAL, "afis_rank_subjects: k must be positive and the three output arrays given");
    AFISCHK(check_last_search(ctx, "afis_rank_subjects", n_q, s));
    return rank_subjects(ctx, s, n_q, k, subject_id, subject_score, best_idx);
}

}  // extern "C"
