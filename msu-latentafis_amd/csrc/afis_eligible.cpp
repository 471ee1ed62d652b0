// afis_eligible.cpp — the eligible search of the C ABI (include/afis_matcher.h): afis_search_eligible scores a (latent, template) pair only where the latent is
// ELIGIBLE for the template — the label test of the filtered hit lists (hit_filter.hip), word for word — and leaves a full [n_q][G] matrix whose other cells hold the
// "no entry" word, so that the whole ranking family reads it unchanged.  No scoring kernel knows about it: the queries are grouped into CLASSES of identical mask
// triples, every class is searched over a temporary sub-shard of its eligible templates through the code of a subset search (afis_subset.cpp::build_subset,
// afis_search.cpp::search_shard), and eligible_expand.hip writes the class's rows of the combined matrix.  A score depends on nothing but its pair, so every eligible
// cell is bit for bit afis_search's.
#include "afis_ctx.h"

using namespace afis;

namespace {

inline bool label_passes(uint64_t L, uint64_t any_of, uint64_t all_of, uint64_t none_of)
{
    return (any_of == 0 || (L & any_of) != 0) && (L & all_of) == all_of && (L & none_of) == 0;
}

}  // namespace

std::vector<EligClass> afis::plan_classes(const std::vector<uint64_t>& label, int64_t G, const uint64_t* masks, int n_q)
{
    std::vector<EligClass> cls;
    for (int i = 0; i < n_q; ++i) {
        const uint64_t* k = masks + (size_t)i * 3;
        auto it = std::find_if(cls.begin(), cls.end(), [k](const EligClass& c) { return c.any_of == k[0] && c.all_of == k[1] && c.none_of == k[2]; });
        if (it == cls.end()) { cls.push_back(EligClass{k[0], k[1], k[2], {}, {}}); it = cls.end() - 1; }
        it->rows.push_back((int32_t)i);
    }
    for (EligClass& c : cls)
        for (int64_t t = 0; t < G; ++t)
            if (label_passes(label[(size_t)t], c.any_of, c.all_of, c.none_of)) c.sel.push_back((int32_t)t);
    return cls;
}

// every additive field is the sum over the searches of the call; the two clock fields come from the search with the most pairs (afis_search_weighted's batches too)
void afis::add_timing(afis_timing& acc, const afis_timing& t, int64_t& most_pairs)
{
    acc.lut_ms += t.lut_ms; acc.adc_ms += t.adc_ms; acc.tex_tail_ms += t.tex_tail_ms; acc.minu_ms += t.minu_ms; acc.fuse_ms += t.fuse_ms; acc.topk_ms += t.topk_ms;
    acc.total_ms += t.total_ms; acc.adc_launches += t.adc_launches; acc.adc_lookups += t.adc_lookups; acc.pairs += t.pairs; acc.adc_bound_ms += t.adc_bound_ms;
    acc.adc_refine_ms += t.adc_refine_ms; acc.cands_ms += t.cands_ms; acc.minu_graph_ms += t.minu_graph_ms; acc.launch_groups += t.launch_groups;
    acc.overlapped_groups += t.overlapped_groups; acc.minu_tasks += t.minu_tasks; acc.minu_fallback_tasks += t.minu_fallback_tasks; acc.minu_tasks_small += t.minu_tasks_small;
    acc.minu_tasks_medium += t.minu_tasks_medium; acc.minu_tasks_large += t.minu_tasks_large;
    if (t.pairs > most_pairs) { most_pairs = t.pairs; acc.bound_clock_ghz = t.bound_clock_ghz; acc.cands_clock_ghz = t.cands_clock_ghz; }
}

void afis::plan_sub_shard(afis_ctx* ctx, afis_subset* sub, const std::vector<int32_t>& sel, std::vector<int64_t>& global)
{
    const size_t n = sel.size();
    Shard& sh = sub->sh;
    sub->n = (int64_t)n; sub->gallery_epoch = ctx->gallery_epoch; sub->identity = true;
    global.resize(n);
    sh.res_mo.assign(n + 1, 0); sh.res_to.assign(n + 1, 0); sh.res_empty.resize(n);
    int64_t nm = 0, nt = 0;
    for (size_t t = 0; t < n; ++t) {
        const size_t g = (size_t)sel[t];
        global[t] = ctx->index_base + (int64_t)g;
        nm += ctx->res_mo[g + 1] - ctx->res_mo[g]; nt += ctx->res_to[g + 1] - ctx->res_to[g];
        sh.res_mo[t + 1] = (int32_t)nm; sh.res_to[t + 1] = (int32_t)nt;      // (sums of a part of a shard that passed the commit's 2^31 check)
        sh.res_empty[t] = ctx->res_empty[g];
    }
    sub->idx = global; sub->held = global;                                  // (sel ascends: the caller's order is the sub-shard's)
    sh.mf_gal_built = false; sh.codes_q_built = false; sh.codes_cf_built = false;      // the derived streams are this class's to lay out (their buffers stay)
}

namespace {

// Everything of the call that touches the device.  tmp, d_sel and d_tab are the caller's to release, whatever this returns.
int search_classes(afis_ctx* ctx, const std::vector<EligClass>& classes, const afis_template_view* queries, int n_q, int32_t* status, afis_subset* tmp, DevBuf& d_sel, DevBuf& d_tab)
{
    const int64_t G = ctx->gal.G;
    hipStream_t s = ctx->stream;
    // room before anything is queued: the combined matrix, and one class's tables (inv [G] | row_of [n_q], int32)
    const size_t inv_bytes = ((size_t)G * 4 + 15) / 16 * 16;
    if (G > 0) HIPCHK(ctx, ctx->elig_scores.ensure((size_t)n_q * (size_t)G * 4));
    HIPCHK(ctx, d_tab.ensure(inv_bytes + (size_t)n_q * 4));
    Events ev(2);
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    afis_timing acc = {};
    int64_t most_pairs = -1, expand_us = 0;
    std::vector<afis_template_view> qv;
    std::vector<int32_t> st, inv;
    std::vector<int64_t> global;
    const std::vector<int32_t> no_pos;
    for (const EligClass& c : classes) {
        const int n_c = (int)c.rows.size();
        const int64_t m = (int64_t)c.sel.size();
        const bool direct = m == G;                                         // every template passes: the resident shard itself, no copy
        qv.clear();
        for (int32_t r : c.rows) qv.push_back(queries[r]);
        afis_queries* q = nullptr;
        AFISCHK(upload_queries(ctx, qv.data(), n_c, direct || m == 0 ? 0 : m, &q));      // the launch groups are cut for the shard that is searched
        struct FreeQ { afis_ctx* c; afis_queries* q; ~FreeQ() { afis_queries_free(c, q); } } free_q{ctx, q};
        st.assign((size_t)n_c, 0);
        if (m == 0) st = q->status;                                         // nothing is scored; status is what a search would say
        else if (direct) AFISCHK(search_shard(ctx, *ctx, nullptr, q, nullptr, nullptr, st.data(), 0, nullptr, nullptr));
        else {
            plan_sub_shard(ctx, tmp, c.sel, global);
            AFISCHK(build_subset(ctx, tmp, c.sel, global, no_pos, &d_sel));
            AFISCHK(search_shard(ctx, tmp->sh, tmp, q, nullptr, nullptr, st.data(), 0, nullptr, nullptr));
        }
        ctx->last_search.valid = false;                                     // (a class's matrix is nobody's to rank)
        if (m > 0) add_timing(acc, ctx->timing, most_pairs);
        if (status) for (int r = 0; r < n_c; ++r) status[c.rows[(size_t)r]] = st[(size_t)r];
        if (G == 0) continue;
        // the class's rows of the combined matrix: the device is idle (the search has waited), the tables are this class's until the wait below
        if (!direct && m > 0) {
            inv.assign((size_t)G, -1);
            for (int64_t t = 0; t < m; ++t) inv[(size_t)c.sel[(size_t)t]] = (int32_t)t;
            HIPCHK(ctx, hipMemcpyAsync(d_tab.p, inv.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
        }
        int32_t* const d_rows = reinterpret_cast<int32_t*>(d_tab.as<uint8_t>() + inv_bytes);
        HIPCHK(ctx, hipMemcpyAsync(d_rows, c.rows.data(), (size_t)n_c * 4, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipEventRecord(ev[0], s));
        HIPCHK(ctx, launch_expand_rows(m > 0 ? ctx->scores.as<float>() : nullptr, n_c, (int)m, direct || m == 0 ? nullptr : d_tab.as<int32_t>(), d_rows, n_q, (int)G,
                                       ctx->elig_scores.as<float>(), s));
        HIPCHK(ctx, hipEventRecord(ev[1], s));
        int64_t us = 0;
        AFISCHK(wait_elapsed(ctx, "afis_search_eligible", ev, &us));
        expand_us += us;
    }
    std::swap(ctx->scores, ctx->elig_scores);                               // the combined matrix is the last search's from here on
    ctx->timing = acc;
    ctx->eligible_classes = (int64_t)classes.size(); ctx->eligible_expand_us = expand_us;
    return AFIS_OK;
}

}  // namespace

extern "C" {

int afis_search_eligible(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const afis_template_view* queries, int n_q, float* scores, int32_t* status)
{
    if (!ctx || !labels || !masks || n_q < 0 || (n_q > 0 && !queries)) return fail(ctx, AFIS_EINVAL, "afis_search_eligible: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_search_eligible: commit the gallery first");
    if (std::find(ctx->label_sets.begin(), ctx->label_sets.end(), labels) == ctx->label_sets.end()) return fail(ctx, AFIS_EINVAL, "afis_search_eligible: not a live labels handle of this context");
    // the labels are positions of the shard as it was: after an edit they may belong to other templates
    if (labels->gallery_epoch != ctx->gallery_epoch) return fail_edited(ctx, "afis_search_eligible", "these labels were given; free the handle and create it again");
    const int64_t G = ctx->gal.G;
    ctx->eligible_classes = 0; ctx->eligible_expand_us = 0;
    if (n_q == 0) return afis_search(ctx, nullptr, 0, scores, nullptr, status, 0, nullptr, nullptr);
    const std::vector<EligClass> classes = plan_classes(labels->h_label, G, masks, n_q);
    // the sub-shards come and go in buffers searches read: all device work of the context first, as for afis_subset_create
    AFISCHK(quiesce(ctx, "afis_search_eligible"));
    std::unique_ptr<afis_subset> tmp(new afis_subset());                     // the one temporary sub-shard: never in ctx->subsets (option subset_device_bytes reads as before)
    DevBuf d_sel, d_tab;
    const int64_t h2d_before = ctx->gallery_h2d_bytes, gather_us = ctx->subset_gather_us;
    int rc = search_classes(ctx, classes, queries, n_q, status, tmp.get(), d_sel, d_tab);
    ctx->gallery_h2d_bytes = h2d_before; ctx->subset_gather_us = gather_us;     // (the two options speak of commits, removals and afis_subset_create: they read as before)
    if (rc == AFIS_OK && scores && G > 0) {                                 // the device is idle: a plain copy, as at the end of a search
        const hipError_t e = hipMemcpy(scores, ctx->scores.p, (size_t)n_q * (size_t)G * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, AFIS_EDEVICE, std::string("afis_search_eligible: the scores: ") + hipGetErrorString(e));
    }
    // the temporary sub-shard goes whatever happened; after a timeout a search may still read it: the bounded wait of afis_subset_free first
    if (rc != AFIS_OK) {
        const std::string keep = ctx->err;
        (void)quiesce(ctx, "afis_search_eligible");
        ctx->err = keep;
        ctx->elig_scores.release();
        ctx->eligible_classes = 0; ctx->eligible_expand_us = 0;
    }
    d_sel.release(); d_tab.release();
    release_subset(tmp.release());
    ctx->last_search = rc == AFIS_OK ? LastSearch{true, n_q, G, nullptr, ctx->gallery_epoch} : LastSearch{};
    return rc;
}

}  // extern "C"
