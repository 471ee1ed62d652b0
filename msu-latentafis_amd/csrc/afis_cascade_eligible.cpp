// afis_cascade_eligible.cpp — the cascade search over a part of the resident shard (include/afis_matcher.h): afis_search_cascade_subset runs the cascade over the
// columns of a live subset, afis_search_cascade_eligible over the templates each latent is eligible for.  Both are afis_search_cascade's driver (CascadeCall: afis_ctx.h,
// afis_cascade.cpp) and its latent side (latent_cascade) over a SUB-SHARD: stage 1, the selection and the pair kernels work on the sub-shard's own positions, the
// selection names the kept prints by global index through the sub-shard's d_global, and the mapped kernels of cascade_mapped.hip go from a kept global index back to the
// sub-shard position (inv) and write the kept cell at the row and column of the matrix the call leaves (row_of, out_col).
//   subset    the sub-shard is the subset's (ascending global index: the selection's tie rule is the rule on global indices); the matrix [n_q][n] stays in the
//             sub-shard's order on the device, as every subset search leaves it — the ranking family names its columns through the subset —, and `scores` leaves in the
//             caller's column order through out_perm
//   eligible  afis_search_eligible's plan (plan_classes): per class of identical mask triples one temporary sub-shard (plan_sub_shard, build_subset: class after class
//             into the same buffers, never in ctx->subsets), the class's latents uploaded for a shard of m templates, ONE cascade over it whose closing kernel writes the
//             kept cells into the combined matrix [n_q][G] at (the query's row, the resident column); the combined matrix is filled with the no-entry word once, before
//             the first class.  A class every template passes runs on the resident shard itself; a class nothing passes scores nothing
#include "afis_ctx.h"

using namespace afis;

namespace {

// resident position -> position in a sub-shard whose templates are the resident positions sel (ascending)
std::vector<int32_t> inverse_of(const std::vector<int32_t>& sel, int64_t G)
{
    std::vector<int32_t> inv((size_t)G, -1);
    for (size_t t = 0; t < sel.size(); ++t) inv[(size_t)sel[t]] = (int32_t)t;
    return inv;
}

// what a failed cascade call leaves: the bounded wait (after a timeout the device may still use the buffers), nothing the call allocated, no matrix
void give_up(afis_ctx* ctx, const char* who)
{
    const std::string keep_err = ctx->err;
    (void)quiesce(ctx, who);
    ctx->err = keep_err;
    ctx->casc_buf.release(); ctx->casc_slab.release(); ctx->elig_scores.release();
    ctx->cascade_stage1_us = ctx->cascade_select_us = ctx->cascade_stage2_us = ctx->cascade_kept_pairs = 0;
    ctx->timing = afis_timing{};
    ctx->last_search = LastSearch{};
}

// Everything of afis_search_cascade_eligible that touches the device.  tmp and d_sel are the caller's to release, whatever this returns.
int cascade_classes(afis_ctx* ctx, const char* who, const std::vector<EligClass>& classes, const afis_template_view* queries, int n_q, int keep, int32_t* status,
                    int64_t* n_kept, int64_t* kept_idx, float* kept_parts, afis_subset* tmp, DevBuf& d_sel)
{
    const int64_t G = ctx->gal.G;
    hipStream_t s = ctx->stream;
    if ((int64_t)n_q * G > 0x7ffffff0LL) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_q x keep or n_q x G exceeds what one call takes");
    // the combined matrix: room, and the no-entry word in every cell, once per call
    if (G > 0) {
        HIPCHK(ctx, ctx->elig_scores.ensure((size_t)n_q * (size_t)G * 4));
        HIPCHK(ctx, hipMemsetAsync(ctx->elig_scores.p, 0xff, (size_t)n_q * (size_t)G * 4, s));
    }
    afis_timing acc = {};
    int64_t most_pairs = -1, sum[4] = {0, 0, 0, 0};
    std::vector<afis_template_view> qv;
    std::vector<int64_t> global, c_n, c_idx;
    std::vector<float> c_parts;
    const std::vector<int32_t> none, no_pos;
    for (const EligClass& cl : classes) {
        const int n_c = (int)cl.rows.size();
        const int64_t m = (int64_t)cl.sel.size();
        const bool direct = m == G;                                         // every template passes: the resident shard itself, no copy
        qv.clear();
        for (int32_t r : cl.rows) qv.push_back(queries[r]);
        afis_queries* q = nullptr;
        AFISCHK(upload_queries(ctx, qv.data(), n_c, direct || m == 0 ? 0 : m, &q));      // the launch groups are cut for the shard that is searched
        struct FreeQ { afis_ctx* c; afis_queries* q; ~FreeQ() { afis_queries_free(c, q); } } free_q{ctx, q};
        if (status) for (int r = 0; r < n_c; ++r) status[cl.rows[(size_t)r]] = q->status[(size_t)r];      // what a search would say
        c_n.assign((size_t)n_c, 0); c_idx.assign((size_t)n_c * (size_t)keep, -1); c_parts.assign((size_t)n_c * (size_t)keep * 4, 0.0f);
        if (m > 0) {                                                        // (a class nothing passes scores nothing: no list holds anything)
            int64_t o[4] = {0, 0, 0, 0};
            CascadeCall c{ctx, who, n_c, keep, {&o[0], &o[1], &o[2], &o[3]}, 4, false};
            c.own_matrix = false;
            std::vector<int32_t> inv;
            if (!direct) {
                plan_sub_shard(ctx, tmp, cl.sel, global);
                AFISCHK(build_subset(ctx, tmp, cl.sel, global, no_pos, &d_sel));
                inv = inverse_of(cl.sel, G);
                c.sub = tmp;
            }
            const CascadeMap map{&inv, direct ? &none : &cl.sel, &cl.rows, n_q, G};
            AFISCHK(latent_cascade(c, q, &map, c_n.data(), c_idx.data(), c_parts.data()));
            c.t = nullptr;
            add_timing(acc, ctx->timing, most_pairs);
            for (int k = 0; k < 4; ++k) sum[k] += o[k];
        }
        for (int r = 0; r < n_c; ++r) {
            const size_t row = (size_t)cl.rows[(size_t)r], w = (size_t)keep;
            if (n_kept) n_kept[row] = c_n[(size_t)r];
            if (kept_idx) memcpy(kept_idx + row * w, c_idx.data() + (size_t)r * w, w * 8);
            if (kept_parts) memcpy(kept_parts + row * w * 4, c_parts.data() + (size_t)r * w * 4, w * 16);
        }
    }
    AFISCHK(wait_streams(ctx, {s}, who));                                   // (the fill, where no class queued anything behind it)
    if (G > 0) std::swap(ctx->scores, ctx->elig_scores);                    // the combined matrix is the last search's from here on
    ctx->timing = acc;
    ctx->cascade_stage1_us = sum[0]; ctx->cascade_select_us = sum[1]; ctx->cascade_stage2_us = sum[2]; ctx->cascade_kept_pairs = sum[3];
    ctx->eligible_classes = (int64_t)classes.size();
    return AFIS_OK;
}

}  // namespace

extern "C" {

int afis_search_cascade_subset(afis_ctx* ctx, afis_subset* sub, afis_queries* q, int keep, float* scores, int32_t* status, int64_t* n_kept, int64_t* kept_idx, float* kept_parts)
{
    const char* const who = "afis_search_cascade_subset";
    if (!ctx || !sub || !q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    CascadeCall c{ctx, who, q->n_q, keep, {&ctx->cascade_stage1_us, &ctx->cascade_select_us, &ctx->cascade_stage2_us, &ctx->cascade_kept_pairs}, 4, false};
    c.clear();
    ctx->last_search.valid = false;
    if (keep < 1 || keep > AFIS_HITS_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": keep must be 1 .. AFIS_HITS_MAX, the longest list the selection makes");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    if (std::find(ctx->subsets.begin(), ctx->subsets.end(), sub) == ctx->subsets.end()) return fail(ctx, AFIS_EINVAL, std::string(who) + ": not a live subset of this context");
    if (sub->gallery_epoch != ctx->gallery_epoch) return fail_edited(ctx, who, "this subset was created; free it and create it again");
    AFISCHK(check_query_handle(ctx, who, q, sub->n, true));                 // afis_search_subset_resident's rules for the handle
    c.sub = sub;
    if (q->n_q == 0 || sub->n == 0)                                         // nothing to score: as a subset search answers it; no list holds anything
        return c.empty(search_shard(ctx, sub->sh, sub, q, scores, nullptr, status, 0, nullptr, nullptr), n_kept, kept_idx, kept_parts);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx));
    // the sub-shard holds the listed templates in ascending global index: its position t is the t-th smallest index of the list
    std::vector<int32_t> sel((size_t)sub->n);
    for (int64_t j = 0; j < sub->n; ++j) sel[(size_t)j] = (int32_t)(sub->idx[(size_t)j] - ctx->index_base);
    std::sort(sel.begin(), sel.end());
    const std::vector<int32_t> inv = inverse_of(sel, ctx->gal.G), none;
    const CascadeMap map{&inv, &none, &none, q->n_q, sub->n};
    const bool perm = scores && !sub->identity;                             // a subset listed out of order: the columns into the caller's order on the device, as a subset search's leave (run() sized out_perm)
    int rc = c.end(latent_cascade(c, q, &map, n_kept, kept_idx, kept_parts), perm ? nullptr : scores);
    if (rc == AFIS_OK && perm) {
        rc = [&]() -> int {
            HIPCHK(ctx, launch_permute_columns(ctx->scores.p, ctx->out_perm.p, 4, q->n_q, (int)sub->n, sub->d_pos.as<int32_t>(), ctx->stream));
            AFISCHK(wait_streams(ctx, {ctx->stream}, who));
            HIPCHK(ctx, hipMemcpy(scores, ctx->out_perm.p, (size_t)q->n_q * (size_t)sub->n * 4, hipMemcpyDeviceToHost));
            return AFIS_OK;
        }();
        if (rc != AFIS_OK) give_up(ctx, who);
    }
    if (rc == AFIS_OK && status) for (int i = 0; i < q->n_q; ++i) status[i] = q->status[(size_t)i];
    return rc;
}

int afis_search_cascade_eligible(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const afis_template_view* queries, int n_q, int keep, float* scores, int32_t* status,
                                 int64_t* n_kept, int64_t* kept_idx, float* kept_parts)
{
    const char* const who = "afis_search_cascade_eligible";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": bad argument");
    ctx->cascade_stage1_us = ctx->cascade_select_us = ctx->cascade_stage2_us = ctx->cascade_kept_pairs = 0;
    ctx->eligible_classes = 0;
    ctx->last_search.valid = false;
    if (!labels || !masks || n_q < 0 || (n_q > 0 && !queries)) return fail(ctx, AFIS_EINVAL, std::string(who) + ": bad argument");
    if (keep < 1 || keep > AFIS_HITS_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": keep must be 1 .. AFIS_HITS_MAX, the longest list the selection makes");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    if (std::find(ctx->label_sets.begin(), ctx->label_sets.end(), labels) == ctx->label_sets.end()) return fail(ctx, AFIS_EINVAL, std::string(who) + ": not a live labels handle of this context");
    // the labels are positions of the shard as it was: after an edit they may belong to other templates
    if (labels->gallery_epoch != ctx->gallery_epoch) return fail_edited(ctx, who, "these labels were given; free the handle and create it again");
    const int64_t G = ctx->gal.G;
    if (n_q == 0) return afis_search(ctx, nullptr, 0, scores, nullptr, status, 0, nullptr, nullptr);
    const std::vector<EligClass> classes = plan_classes(labels->h_label, G, masks, n_q);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the sub-shards come and go in buffers searches read: all device work of the context first, as for afis_subset_create
    AFISCHK(quiesce(ctx, who));
    std::unique_ptr<afis_subset> tmp(new afis_subset());                     // the one temporary sub-shard: never in ctx->subsets (option subset_device_bytes reads as before)
    DevBuf d_sel;
    const int64_t h2d_before = ctx->gallery_h2d_bytes, gather_us = ctx->subset_gather_us;
    int rc = cascade_classes(ctx, who, classes, queries, n_q, keep, status, n_kept, kept_idx, kept_parts, tmp.get(), d_sel);
    ctx->gallery_h2d_bytes = h2d_before; ctx->subset_gather_us = gather_us;     // (the two options speak of commits, removals and afis_subset_create: they read as before)
    if (rc == AFIS_OK && scores && G > 0) {                                 // the device is idle: a plain copy, as at the end of a search
        const hipError_t e = hipMemcpy(scores, ctx->scores.p, (size_t)n_q * (size_t)G * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, AFIS_EDEVICE, std::string(who) + ": the scores: " + hipGetErrorString(e));
    }
    // the temporary sub-shard goes whatever happened; after a timeout a launch may still read it: the bounded wait first
    if (rc != AFIS_OK) { give_up(ctx, who); ctx->eligible_classes = 0; }
    d_sel.release();
    release_subset(tmp.release());
    ctx->last_search = rc == AFIS_OK ? LastSearch{true, n_q, G, nullptr, ctx->gallery_epoch} : LastSearch{};
    return rc;
}

}  // extern "C"
