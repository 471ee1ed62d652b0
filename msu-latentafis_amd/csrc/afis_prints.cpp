// afis_prints.cpp — the print search of the C ABI (include/afis_matcher.h): afis_search_prints takes RESIDENT prints as queries — the duplicate check of an enrolment, the
// linking of an unsolved-latent file enrolled as a gallery — and leaves the matrix afis_search_weighted would leave for the prints' own templates as query views.  No
// template crosses PCIe for it: a print is one pseudo-query with the spec (0 or -1, -1, -1, 0 or -1), the query groups of a batch are cut as upload_queries cuts them and
// FILLED ON THE DEVICE from the resident shard (print_queries.hip: segment copies, the fragment tiles as they stand, the PQ codes decoded through the fp32 codebook),
// then searched and folded exactly as the weighted search's are (search_shard with the per-part scores kept, template_fold.hip).  Only the index list's consequences —
// a group's seven tables and three source offset tables, the fold's two — are uploaded.
#include "afis_ctx.h"

#include <climits>

using namespace afis;

namespace afis {

// first fragment tile of every resident template: the prefix sums of ceil(minutiae / 16), what g_minu_tile_off holds
std::vector<int32_t> resident_tile_offsets(const afis_ctx* ctx)
{
    const size_t G = ctx->res_empty.size();
    std::vector<int32_t> t(G + 1, 0);
    for (size_t i = 0; i < G; ++i) t[i + 1] = t[i] + (ctx->res_mo[i + 1] - ctx->res_mo[i] + 15) / 16;
    return t;
}

int prepare_print_group(afis_ctx* ctx, const std::vector<int32_t>& res_tile, const int32_t* local, const uint8_t* use_minu, const uint8_t* use_tex, int n, QueryGroup& grp,
                        PrintGroupPlan& plan, std::vector<int32_t>& status_out)
{
    const size_t nq = (size_t)n;
    auto pad4 = [](size_t k) { return (k + 3) / 4 * 4; };                   // every table starts on a 16-byte boundary
    // tab: lm_off [3 n + 1] | lm_tile_off [3 n + 1] | lt_off [n + 1] | tile_off [n + 1] | tile16_off [n + 1] | tex_slot [n] | status [n] | first_minu [n] | first_tile [n] | first_tex [n]
    const size_t at_lm = 0, at_lmt = at_lm + pad4(3 * nq + 1), at_lt = at_lmt + pad4(3 * nq + 1), at_tile = at_lt + pad4(nq + 1), at_t16 = at_tile + pad4(nq + 1),
                 at_slot = at_t16 + pad4(nq + 1), at_status = at_slot + pad4(nq), at_first = at_status + pad4(nq), n_tab = at_first + 3 * pad4(nq);
    std::vector<int32_t>& tab = plan.tab;
    tab.assign(n_tab, 0);
    int32_t* const lm_off = &tab[at_lm]; int32_t* const lm_tile_off = &tab[at_lmt]; int32_t* const lt_off = &tab[at_lt]; int32_t* const tile_off = &tab[at_tile];
    int32_t* const tile16_off = &tab[at_t16]; int32_t* const tex_slot = &tab[at_slot]; int32_t* const status = &tab[at_status];
    int32_t* const first_minu = &tab[at_first]; int32_t* const first_tile = first_minu + pad4(nq); int32_t* const first_tex = first_tile + pad4(nq);
    int max_nL = 0, lt_max = 0;
    grp.h_has_lm.clear(); grp.h_lt_n.clear();
    for (size_t p = 0; p < nq; ++p) {
        const size_t t = (size_t)local[p];
        const int nm_all = ctx->res_mo[t + 1] - ctx->res_mo[t], nt_all = ctx->res_to[t + 1] - ctx->res_to[t];    // (texture counts are clamped to 1000 at enrolment)
        const int nm = use_minu[p] ? nm_all : 0, nt = use_tex[p] ? nt_all : 0;
        first_minu[p] = ctx->res_mo[t]; first_tile[p] = res_tile[t]; first_tex[p] = ctx->res_to[t];
        lm_off[3 * p + 1] = lm_off[3 * p + 2] = lm_off[3 * p + 3] = lm_off[3 * p] + nm;          // slot 0 holds the template, slots 1 and 2 are empty ranges
        lm_tile_off[3 * p + 1] = lm_tile_off[3 * p + 2] = lm_tile_off[3 * p + 3] = lm_tile_off[3 * p] + (nm + 15) / 16;
        lt_off[p + 1] = lt_off[p] + nt;
        tile_off[p + 1] = tile_off[p] + (nt + kTileRows - 1) / kTileRows;
        tile16_off[p + 1] = tile16_off[p] + (nt + 15) / 16;
        tex_slot[p] = nt > 0 ? (nm_all > 0 ? 1 : 0) : -1;                   // build_group's: the view's minutiae template count where the texture template is selected
        status[p] = AFIS_QUERY_OK;                                          // (a pseudo-query with a spec is never "latent empty")
        for (int s = 0; s < 3; ++s) grp.h_has_lm.push_back(s == 0 && nm > 0);
        grp.h_lt_n.push_back(nt);
        max_nL = std::max(max_nL, nm); lt_max = std::max(lt_max, nt);
    }
    plan.first_at = at_first; plan.n_lm = lm_off[3 * nq]; plan.n_lm_tiles = lm_tile_off[3 * nq]; plan.n_lt = lt_off[nq];
    // room: the tables in one buffer (grp.lm_off owns it), the 4-byte arrays in whole 16-byte words (the gather stores nothing narrower)
    auto words16 = [](size_t bytes) { return std::max<size_t>((bytes + 15) / 16 * 16, 16); };
    HIPCHK(ctx, grp.lm_off.ensure(words16(n_tab * 4)));
    HIPCHK(ctx, grp.lm_xy.ensure(words16((size_t)plan.n_lm * 4))); HIPCHK(ctx, grp.lm_ori.ensure(words16((size_t)plan.n_lm * 4)));
    HIPCHK(ctx, grp.lm_des.ensure(words16((size_t)plan.n_lm * kDes * 4))); HIPCHK(ctx, grp.lm_frag.ensure(words16((size_t)plan.n_lm_tiles * 6 * 64 * 16)));
    HIPCHK(ctx, grp.lt_xy.ensure(words16((size_t)plan.n_lt * 4))); HIPCHK(ctx, grp.lt_ori.ensure(words16((size_t)plan.n_lt * 4)));
    HIPCHK(ctx, grp.lt_des.ensure(words16((size_t)plan.n_lt * kDes * 4)));
    const int32_t* const d_tab = grp.lm_off.as<int32_t>();
    QueryDev& d = grp.dev;
    d.nq = n;
    d.lm_off = d_tab + at_lm; d.lm_tile_off = d_tab + at_lmt; d.lt_off = d_tab + at_lt; d.tile_off = d_tab + at_tile; d.tile16_off = d_tab + at_t16;
    d.tex_slot = d_tab + at_slot; d.status = d_tab + at_status;
    d.lm_xy = grp.lm_xy.as<short2>(); d.lm_ori = grp.lm_ori.as<float>(); d.lm_des = grp.lm_des.as<float>(); d.lm_frag = grp.lm_frag.as<float4>();
    d.lt_xy = grp.lt_xy.as<short2>(); d.lt_ori = grp.lt_ori.as<float>(); d.lt_des = grp.lt_des.as<float>();
    d.n_tiles = tile_off[nq]; d.n_tiles16 = tile16_off[nq];
    d.lt_pad = std::max(kTileRows, (lt_max + kTileRows - 1) / kTileRows * kTileRows);
    grp.nq = n; grp.max_nL = max_nL; grp.n_lm_points = plan.n_lm; grp.n_lt_rows = plan.n_lt;
    status_out.insert(status_out.end(), status, status + nq);
    return AFIS_OK;
}

int queue_print_group(afis_ctx* ctx, const QueryGroup& grp, const PrintGroupPlan& plan, int64_t* h2d_bytes, hipEvent_t before_gather, hipEvent_t after_gather)
{
    hipStream_t s = ctx->stream;
    const size_t nq4 = ((size_t)grp.nq + 3) / 4 * 4;
    HIPCHK(ctx, hipMemcpyAsync(grp.lm_off.p, plan.tab.data(), plan.tab.size() * 4, hipMemcpyHostToDevice, s));
    *h2d_bytes += (int64_t)(plan.tab.size() * 4);
    const int32_t* const first = grp.lm_off.as<int32_t>() + plan.first_at;
    if (before_gather) HIPCHK(ctx, hipEventRecord(before_gather, s));
    HIPCHK(ctx, launch_print_queries(ctx->gal, ctx->codewords.as<float>(), first, first + nq4, first + 2 * nq4, grp.dev, plan.n_lm, plan.n_lm_tiles, plan.n_lt, s));
    if (after_gather) HIPCHK(ctx, hipEventRecord(after_gather, s));
    return AFIS_OK;
}

namespace {
struct EventList {                                                          // two events per launch group of a batch, destroyed with the batch
    std::vector<hipEvent_t> e;
    ~EventList() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
}  // namespace

int build_print_queries(afis_ctx* ctx, const char* who, const std::vector<int32_t>& res_tile, const int32_t* local, const uint8_t* use_minu, const uint8_t* use_tex, int n,
                        bool keep_last_search, std::vector<PrintGroupPlan>& plans, afis_queries** q, int64_t* h2d_bytes, int64_t* gather_us)
{
    std::vector<long long> rows(1, 0);
    for (int p = 0; p < n; ++p) rows.push_back(rows.back() + (use_tex[p] ? ctx->res_to[(size_t)local[p] + 1] - ctx->res_to[(size_t)local[p]] : 0));
    // the launch groups: cut as upload_queries cuts them, every DevBuf sized — then the tables and the gathers queued group after group
    plans.clear();
    AFISCHK(upload_query_groups(ctx, rows, n, 0, q, [&](int g0, int m, QueryGroup& grp, std::vector<int32_t>& status) {
        plans.emplace_back();
        return prepare_print_group(ctx, res_tile, local + g0, use_minu + g0, use_tex + g0, m, grp, plans.back(), status);
    }, keep_last_search));
    EventList gev;
    gev.e.assign((*q)->groups.size() * 2, nullptr);
    for (hipEvent_t& e : gev.e) HIPCHK(ctx, hipEventCreate(&e));
    for (size_t gi = 0; gi < (*q)->groups.size(); ++gi) AFISCHK(queue_print_group(ctx, (*q)->groups[gi], plans[gi], h2d_bytes, gev.e[2 * gi], gev.e[2 * gi + 1]));
    // the bounded wait: the groups are what upload_queries would have left — complete — before anything sizes its buffers on an idle device
    AFISCHK(wait_streams(ctx, {ctx->stream}, who));
    for (size_t gi = 0; gi < (*q)->groups.size(); ++gi) {
        float ms = 0.0f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, gev.e[2 * gi], gev.e[2 * gi + 1]));
        *gather_us += (int64_t)((double)ms * 1000.0 + 0.5);
    }
    return AFIS_OK;
}

}  // namespace afis

namespace {

// one query of the call: its print (shard-local), what of it is active, and its pseudo-query (n_pq is 0 or 1)
struct PQuery { int32_t local; bool am, at; int n_pq; };

// Everything of the call that touches the device.  What it leaves in ctx->elig_scores / ctx->wt_tab after a failure is the caller's to release; `plans` (the host's
// copies of tables a copy may still read) lives in the caller, beyond its bounded wait.
int search_batches(afis_ctx* ctx, afis_subset* sub, const std::vector<PQuery>& pq, const std::vector<PseudoBatch>& batches, int n_q, const float* w_minu, const float* w_tex,
                   bool want_perm, std::vector<PrintGroupPlan>& plans, std::vector<int32_t>& fold_tab)
{
    Shard& sh = sub ? sub->sh : static_cast<Shard&>(*ctx);
    const int64_t G = sh.gal.G;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx));
    // room before anything is queued: the combined matrix, the largest batch's per-part scores and fold tables (descriptors [queries][4] int32 | weights [pseudo][4] float),
    // the caller's column order for a subset listed out of order
    size_t parts_max = 16, tab_max = 16;
    for (const PseudoBatch& b : batches) {
        parts_max = std::max(parts_max, (size_t)(b.p1 - b.p0) * (size_t)G * 16);
        tab_max = std::max(tab_max, (size_t)(b.q1 - b.q0) * 16 + (size_t)(b.p1 - b.p0) * 16);
    }
    if (G > 0) { HIPCHK(ctx, ctx->elig_scores.ensure((size_t)n_q * (size_t)G * 4)); HIPCHK(ctx, ctx->parts.ensure(parts_max)); }
    if (G > 0 && want_perm) HIPCHK(ctx, ctx->out_perm.ensure((size_t)n_q * (size_t)G * 4));
    HIPCHK(ctx, ctx->wt_tab.ensure(tab_max));
    const std::vector<int32_t> res_tile = resident_tile_offsets(ctx);
    Events ev(2);
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    afis_timing acc = {};
    int64_t most_pairs = -1, fold_us = 0, gather_us = 0, h2d = 0, n_pseudo = 0;
    std::vector<int32_t> local;
    std::vector<uint8_t> use_m, use_t;
    for (const PseudoBatch& b : batches) {
        const int nq_b = b.q1 - b.q0;
        const int np_b = (int)(b.p1 - b.p0);
        local.clear(); use_m.clear(); use_t.clear();
        fold_tab.assign((size_t)nq_b * 4 + (size_t)np_b * 4, 0);           // qd [nq_b][4] int32 | wt [np_b][4] float, as the weighted search's
        float* const wt = reinterpret_cast<float*>(fold_tab.data() + (size_t)nq_b * 4);
        for (int i = b.q0; i < b.q1; ++i) {
            const PQuery& q = pq[(size_t)i];
            int32_t* const qd = &fold_tab[(size_t)(i - b.q0) * 4];
            qd[0] = (int32_t)local.size(); qd[1] = q.n_pq; qd[2] = q.at ? 1 : 0; qd[3] = q.n_pq == 0 ? AFIS_QUERY_LATENT_EMPTY : AFIS_QUERY_OK;
            if (q.n_pq == 0) continue;
            wt[local.size() * 4 + 0] = q.am ? w_minu[i] : 0.0f; wt[local.size() * 4 + 3] = q.at ? w_tex[i] : 0.0f;
            local.push_back(q.local); use_m.push_back(q.am); use_t.push_back(q.at);
        }
        afis_queries* q = nullptr;
        struct FreeQ { afis_ctx* c; afis_queries** q; ~FreeQ() { afis_queries_free(c, *q); } } free_q{ctx, &q};
        if (np_b > 0) {
            // the batch's temporary handle: launch groups cut, tables and gathers queued, one bounded wait (the pair calls for prints build theirs the same way)
            AFISCHK(build_print_queries(ctx, "afis_search_prints", res_tile, local.data(), use_m.data(), use_t.data(), np_b, false, plans, &q, &h2d, &gather_us));
            AFISCHK(search_shard(ctx, sh, sub, q, nullptr, nullptr, nullptr, 0, nullptr, nullptr, true));
            ctx->last_search.valid = false;                                 // (a batch's pseudo-query matrix is nobody's to rank)
            add_timing(acc, ctx->timing, most_pairs);
            n_pseudo += np_b;
        }
        if (G == 0) continue;
        // the batch's rows of the combined matrix: the device is idle (the search has waited), the tables are this batch's until the wait below
        int32_t* const d_qd = ctx->wt_tab.as<int32_t>();
        float* const d_wt = reinterpret_cast<float*>(ctx->wt_tab.as<uint8_t>() + (size_t)nq_b * 16);
        HIPCHK(ctx, hipMemcpyAsync(d_qd, fold_tab.data(), (size_t)nq_b * 16, hipMemcpyHostToDevice, s));
        h2d += (int64_t)nq_b * 16;
        if (np_b > 0) { HIPCHK(ctx, hipMemcpyAsync(d_wt, wt, (size_t)np_b * 16, hipMemcpyHostToDevice, s)); h2d += (int64_t)np_b * 16; }
        HIPCHK(ctx, hipEventRecord(ev[0], s));
        HIPCHK(ctx, launch_fold_templates(ctx->parts.as<float>(), d_qd, d_wt, sh.gal.empty, nq_b, (int)G, ctx->elig_scores.as<float>() + (size_t)b.q0 * (size_t)G, s));
        HIPCHK(ctx, hipEventRecord(ev[1], s));
        int64_t us = 0;
        AFISCHK(wait_elapsed(ctx, "afis_search_prints", ev, &us));
        fold_us += us;
    }
    std::swap(ctx->scores, ctx->elig_scores);                               // the combined matrix is the last search's from here on
    ctx->timing = acc;
    ctx->weighted_pseudo_queries = n_pseudo; ctx->weighted_fold_us = fold_us;
    ctx->print_gather_us = gather_us; ctx->print_h2d_bytes = h2d;
    return AFIS_OK;
}

}  // namespace

extern "C" {

int afis_search_prints(afis_ctx* ctx, afis_subset* sub, const int64_t* idx, int n_q, const float* w_minu, const float* w_tex, float* scores, int32_t* status)
{
    if (!ctx) return fail(ctx, AFIS_EINVAL, "afis_search_prints: null context");
    ctx->print_gather_us = 0; ctx->print_h2d_bytes = 0; ctx->weighted_pseudo_queries = 0; ctx->weighted_fold_us = 0;
    ctx->last_search = LastSearch{};                                        // whatever this call returns, the matrix of an earlier search is no longer there to rank
    if (n_q < 0 || (n_q > 0 && (!idx || !w_minu || !w_tex))) return fail(ctx, AFIS_EINVAL, "afis_search_prints: bad argument");
    for (int k = 0; k < 2; ++k) {
        const float* w = k ? w_tex : w_minu;
        for (int i = 0; i < n_q; ++i)
            if (!(w[i] >= 0.0f) || std::isinf(w[i])) return fail(ctx, AFIS_EINVAL, "afis_search_prints: a weight must be finite and >= 0 (-1 means \"empty\", every other cell is >= +0)");
    }
    if (sub && std::find(ctx->subsets.begin(), ctx->subsets.end(), sub) == ctx->subsets.end()) return fail(ctx, AFIS_EINVAL, "afis_search_prints: not a live subset of this context");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_search_prints: commit the gallery first");
    if (sub && sub->gallery_epoch != ctx->gallery_epoch) return fail_edited(ctx, "afis_search_prints", "this subset was created; free it and create it again");
    const int64_t G_res = (int64_t)ctx->res_empty.size(), G_all = afis_gallery_size(ctx);
    for (int i = 0; i < n_q; ++i) {
        const int64_t t = idx[i] - ctx->index_base;
        if (idx[i] < ctx->index_base || t >= G_all) return fail(ctx, AFIS_EINVAL, "afis_search_prints: index " + std::to_string((long long)idx[i]) + " is outside the resident shard");
        if (t >= G_res) return fail(ctx, AFIS_ESTATE, "afis_search_prints: index " + std::to_string((long long)idx[i]) + " is staged but not committed (afis_gallery_commit first)");
    }
    if (n_q == 0) return sub ? afis_search_subset(ctx, sub, nullptr, 0, scores, nullptr, status, 0, nullptr, nullptr) : afis_search(ctx, nullptr, 0, scores, nullptr, status, 0, nullptr, nullptr);
    const int64_t G = sub ? (int64_t)sub->sh.gal.G : (int64_t)ctx->gal.G;
    // the plan: what of every print is active, one pseudo-query per print that has something active, batches
    std::vector<PQuery> pq((size_t)n_q);
    std::vector<int> n_pq((size_t)n_q);
    for (int i = 0; i < n_q; ++i) {
        PQuery& q = pq[(size_t)i];
        q.local = (int32_t)(idx[i] - ctx->index_base);
        q.am = ctx->res_mo[(size_t)q.local + 1] > ctx->res_mo[(size_t)q.local] && w_minu[i] != 0.0f;
        q.at = ctx->res_to[(size_t)q.local + 1] > ctx->res_to[(size_t)q.local] && w_tex[i] != 0.0f;
        q.n_pq = n_pq[(size_t)i] = q.am || q.at ? 1 : 0;
        if (status) status[i] = q.n_pq == 0 ? AFIS_QUERY_LATENT_EMPTY : AFIS_QUERY_OK;
    }
    // pseudo-queries per batch at most: afis_search_weighted's rule
    (void)hipSetDevice(ctx->device);
    const int64_t cap_auto = std::max<int64_t>(1, group_budget_bytes(ctx) / 8 / (16 * std::max<int64_t>(1, G)));
    const int64_t cap = std::min<int64_t>(ctx->weighted_batch_pseudo > 0 ? ctx->weighted_batch_pseudo : cap_auto, INT_MAX / 4);
    const std::vector<PseudoBatch> batches = plan_pseudo_batches(n_pq, cap);
    const bool want_perm = scores && sub && !sub->identity;
    std::vector<PrintGroupPlan> plans;
    std::vector<int32_t> fold_tab;
    int rc = search_batches(ctx, sub, pq, batches, n_q, w_minu, w_tex, want_perm, plans, fold_tab);
    if (rc == AFIS_OK && scores && G > 0) {                                 // the device is idle: a subset's columns into the caller's order, then a plain copy
        const float* out = ctx->scores.as<float>();
        hipError_t e = hipSuccess;
        if (want_perm) {
            for (int r0 = 0; r0 < n_q && e == hipSuccess; r0 += 65535)     // (launch_permute_columns takes a grid's second dimension of rows)
                e = launch_permute_columns(ctx->scores.as<float>() + (size_t)r0 * (size_t)G, ctx->out_perm.as<float>() + (size_t)r0 * (size_t)G, 4, std::min(65535, n_q - r0), (int)G,
                                           sub->d_pos.as<int32_t>(), ctx->stream);
            if (e == hipSuccess) rc = wait_streams(ctx, {ctx->stream}, "afis_search_prints");
            out = ctx->out_perm.as<float>();
        }
        if (e == hipSuccess && rc == AFIS_OK) e = hipMemcpy(scores, out, (size_t)n_q * (size_t)G * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, AFIS_EDEVICE, std::string("afis_search_prints: the scores: ") + hipGetErrorString(e));
    }
    if (rc != AFIS_OK) {                                                    // after a timeout a launch may still read the tables: the bounded wait first, then nothing of the call stays
        const std::string keep = ctx->err;
        (void)quiesce(ctx, "afis_search_prints");
        ctx->err = keep;
        ctx->elig_scores.release(); ctx->wt_tab.release();
        ctx->weighted_pseudo_queries = 0; ctx->weighted_fold_us = 0; ctx->print_gather_us = 0; ctx->print_h2d_bytes = 0;
    }
    ctx->last_search = rc == AFIS_OK ? LastSearch{true, n_q, G, sub, ctx->gallery_epoch} : LastSearch{};
    return rc;
}

}  // extern "C"
