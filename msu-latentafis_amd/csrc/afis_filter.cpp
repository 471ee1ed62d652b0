// afis_filter.cpp — filtered hit lists of the C ABI (include/afis_matcher.h): afis_labels_create gives every template of the resident shard one 64-bit attribute word,
// afis_rank_hits_filtered and afis_rank_subject_hits_filtered list, per query of the last search, the templates or the enrolled persons that reach a decision score
// among the cells the query is ELIGIBLE for — the label passes the query's three masks, and the template or the person is not on the query's exclusion list.  The
// ineligible cells are taken out of a copy of the matrix (hit_filter.hip) and the copy is ranked by k_subject_best and k_rank_hits, unchanged, the way afis_cases.cpp
// ranks its fused rows.  Only n_q x (8 + cap x 12 or 20) bytes return; the [n_q][G] matrix stays where it is, and as it is.
#include "afis_ctx.h"

using namespace afis;

namespace afis {

void release_labels(afis_labels* l)
{
    if (!l) return;
    l->d_label.release();
    delete l;
}

hipError_t FilterPass::ensure()
{
    if (copy) { const hipError_t e = ctx->filt_scores.ensure((size_t)n_q * (size_t)G * 4); if (e != hipSuccess) return e; }
    return tab_bytes ? ctx->filt_tab.ensure(tab_bytes) : hipSuccess;
}

int FilterPass::queue_cells()
{
    hipStream_t s = ctx->stream;
    const LastSearch& ls = ctx->last_search;
    if (masks) HIPCHK(ctx, launch_filter_rows(ctx->scores.as<float>(), n_q, (int)G, labels->d_label.as<unsigned long long>(), ctx->filt_tab.as<unsigned long long>(), global_map(ls),
                                              (long long)ctx->index_base, ctx->filt_scores.as<float>(), s));
    else if (copy) HIPCHK(ctx, hipMemcpyAsync(ctx->filt_scores.p, ctx->scores.p, (size_t)n_q * (size_t)G * 4, hipMemcpyDeviceToDevice, s));
    if (!subjects) HIPCHK(ctx, launch_filter_drop_cells((const int32_t*)(ctx->filt_tab.as<uint8_t>() + mask_bytes), n_pairs, ctx->filt_scores.as<float>(), n_q, (int)G, s));
    return AFIS_OK;
}

int FilterPass::queue_drop_subjects(int64_t S)
{
    HIPCHK(ctx, launch_filter_drop_subjects((const int32_t*)(ctx->filt_tab.as<uint8_t>() + mask_bytes), n_pairs, ctx->subj_best.as<unsigned long long>(), n_q, (int)S, ctx->stream));
    return AFIS_OK;
}

// both entry points behind their checks (subj == NULL: the templates; out_a = idx, out_b unused).  masks NULL or [n_q][3]; pairs: the exclusions as (row, column) —
// columns of the matrix for the templates, slots of the handle for the subjects — already inside the matrix
static int rank_hits_filtered(afis_ctx* ctx, afis_subjects* subj, const afis_labels* labels, const uint64_t* masks, const std::vector<int32_t>& pairs, int n_q, float min_score, int cap,
                              int64_t* n_hits, int64_t* out_a, float* out_score, int64_t* out_b)
{
    const LastSearch ls = ctx->last_search;
    const int64_t G = ls.G, S = subj ? subj->S : 0;
    HitCall hc{ctx, subj ? "afis_rank_subject_hits_filtered" : "afis_rank_hits_filtered", n_q, cap, n_hits, out_a, out_score, subj ? out_b : nullptr};
    ctx->rank_filtered_us = 0; ctx->filter_us = 0;
    if (hc.empty(G == 0 || (subj && S == 0))) return AFIS_OK;
    FilterPass fp{ctx, labels, masks, pairs, subj != nullptr};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, fp.ensure());
    if (subj) HIPCHK(ctx, ctx->subj_best.ensure((size_t)n_q * (size_t)S * 8));
    AFISCHK(hc.begin({fp.masks_up(), fp.pairs_up()}));
    AFISCHK(fp.queue_cells());                                              // neither masks nor exclusions: nothing, and the search's matrix itself is ranked
    if (subj) {                                                             // the maxima of the filtered rows, exactly as rank_hits makes them; then the excluded persons
        AFISCHK(queue_subject_best(ctx, subj, fp.matrix()));
        AFISCHK(fp.queue_drop_subjects(S));
    }
    AFISCHK(hc.finish({fp.matrix(), G, subj, global_map(ls), (long long)ctx->index_base}, min_score));   // afis_rank_hits' thresholds, unchanged
    ctx->rank_filtered_us = hc.total_us; ctx->filter_us = hc.pre_us;
    return AFIS_OK;
}

// the checks every filtered ranking call shares, in the order of afis_rank_hits'; on AFIS_OK pairs holds the exclusions that name something the search covered, as (row, column or slot)
int check_filtered(afis_ctx* ctx, const char* who, const afis_subjects* s, const afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl,
                   int n_q, float min_score, int cap, bool outputs, std::vector<int32_t>& pairs)
{
    const std::string w(who);
    if (labels && std::find(ctx->label_sets.begin(), ctx->label_sets.end(), labels) == ctx->label_sets.end()) return fail(ctx, AFIS_EINVAL, w + ": not a live labels handle of this context");
    if (masks && !labels) return fail(ctx, AFIS_EINVAL, w + ": masks need a labels handle");
    AFISCHK(check_hits(ctx, who, n_q, min_score, cap, outputs, s));
    // the labels are positions of the shard as it was: after an edit they may belong to other templates
    if (labels && labels->gallery_epoch != ctx->gallery_epoch)
        return fail_edited(ctx, who, "these labels were given; free the handle and create it again");
    pairs.clear();
    if (!excl_off) return AFIS_OK;
    if (excl_off[0] != 0) return fail(ctx, AFIS_EINVAL, w + ": excl_off[0] must be 0");
    for (int i = 0; i < n_q; ++i) if (excl_off[i + 1] < excl_off[i]) return fail(ctx, AFIS_EINVAL, w + ": excl_off decreases");
    const int64_t total = excl_off[n_q];
    if (total > 0 && !excl) return fail(ctx, AFIS_EINVAL, w + ": excl_off lists entries, the entries are null");
    for (int64_t e = 0; e < total; ++e) if (excl[e] < 0) return fail(ctx, AFIS_EINVAL, w + ": an exclusion is negative");
    // an entry that names nothing the search covered is ignored: another shard's template, one the subset does not list, an id the handle does not hold
    const ColumnNames names = column_names(ctx, s);
    for (int i = 0; i < n_q; ++i)
        for (int64_t e = excl_off[i]; e < excl_off[i + 1]; ++e) {
            const int64_t c = names.find(excl[e]);
            if (c >= 0) { pairs.push_back((int32_t)i); pairs.push_back((int32_t)c); }
        }
    return AFIS_OK;
}

ColumnNames column_names(const afis_ctx* ctx, const afis_subjects* s)
{
    const LastSearch& ls = ctx->last_search;
    return s ? ColumnNames{s->ids.data(), s->S, 0} : ls.sub ? ColumnNames{ls.sub->held.data(), (int64_t)ls.sub->held.size(), 0} : ColumnNames{nullptr, ls.G, ctx->index_base};
}

}  // namespace afis

extern "C" {

int afis_labels_create(afis_ctx* ctx, const uint64_t* label, int64_t n, afis_labels** out)
{
    if (!ctx || !out || n < 0 || (n > 0 && !label)) return fail(ctx, AFIS_EINVAL, "afis_labels_create: bad argument");
    *out = nullptr;
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_labels_create: commit the gallery first");
    if (n != (int64_t)ctx->res_empty.size()) return fail(ctx, AFIS_EINVAL, "afis_labels_create: one label per template of the resident shard (option gallery_resident)");
    std::unique_ptr<afis_labels> lb(new afis_labels());
    lb->n = n; lb->gallery_epoch = ctx->gallery_epoch;
    if (n > 0) lb->h_label.assign(label, label + n);
    { const int rcq = quiesce(ctx, "afis_labels_create", true); if (rcq != AFIS_OK) return rcq; }
    if (n > 0) {
        const int64_t h2d_before = ctx->gallery_h2d_bytes;
        auto table = [&]() -> int {
            HIPCHK(ctx, hipSetDevice(ctx->device));
            HIPCHK(ctx, lb->d_label.ensure((size_t)n * 8));
            HIPCHK(ctx, hipMemcpyAsync(lb->d_label.p, label, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
            ctx->gallery_h2d_bytes += n * 8;
            return wait_streams(ctx, {ctx->stream}, "afis_labels_create");
        };
        const int rc = table();
        if (rc != AFIS_OK) {                                                // nothing allocated, nothing changed
            (void)hipStreamSynchronize(ctx->stream);
            ctx->gallery_h2d_bytes = h2d_before;
            release_labels(lb.release());
            return rc;
        }
    }
    ctx->label_sets.push_back(lb.get());
    *out = lb.release();
    return AFIS_OK;
}

void afis_labels_free(afis_ctx* ctx, afis_labels* labels)
{
    if (!labels) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)quiesce(ctx, "afis_labels_free", true);
        ctx->label_sets.erase(std::remove(ctx->label_sets.begin(), ctx->label_sets.end(), labels), ctx->label_sets.end());
    }
    release_labels(labels);
}

int afis_rank_hits_filtered(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl,
                            int n_q, float min_score, int cap, int64_t* n_hits, int64_t* idx, float* score)
{
    if (!ctx) return fail(ctx, AFIS_EINVAL, "afis_rank_hits_filtered: null argument");
    std::vector<int32_t> pairs;
    const int rc = check_filtered(ctx, "afis_rank_hits_filtered", nullptr, labels, masks, excl_off, excl, n_q, min_score, cap, n_hits && idx && score, pairs);
    return rc != AFIS_OK ? rc : rank_hits_filtered(ctx, nullptr, labels, masks, pairs, n_q, min_score, cap, n_hits, idx, score, nullptr);
}

int afis_rank_subject_hits_filtered(afis_ctx* ctx, afis_subjects* s, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl_subject,
                                    int n_q, float min_score, int cap, int64_t* n_hits, int64_t* subject_id, float* subject_score, int64_t* best_idx)
{
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, "afis_rank_subject_hits_filtered: null argument");
    AFISCHK(check_subject_handle(ctx, "afis_rank_subject_hits_filtered", s));
    std::vector<int32_t> pairs;
    const int rc = check_filtered(ctx, "afis_rank_subject_hits_filtered", s, labels, masks, excl_off, excl_subject, n_q, min_score, cap, n_hits && subject_id && subject_score && best_idx, pairs);
    return rc != AFIS_OK ? rc : rank_hits_filtered(ctx, s, labels, masks, pairs, n_q, min_score, cap, n_hits, subject_id, subject_score, best_idx);
}

}  // extern "C"
