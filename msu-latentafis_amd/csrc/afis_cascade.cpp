// afis_cascade.cpp — the cascade search of the C ABI (include/afis_matcher.h), and the driver of every cascade call (CascadeCall, afis_ctx.h: afis_search_prints_cascade
// in afis_print_cascade.cpp runs through it too).  afis_search_cascade runs the three minutiae scorers for every (latent, print) cell of the resident shard, selects per
// latent the `keep` best prints by that partial score on the device, and runs the texture scorer for the kept cells only.  A kept cell is, bit for bit, afis_search's;
// every other cell holds the "no entry" word (score_order.h), so the ranking family reads the matrix as it reads afis_search_eligible's.
// One launch sequence on the context's stream, no host round trip between the stages, one wait at the end (CascadeCall::run):
//   stage 1   per launch group of the handle the minutiae stage of a search (afis_search.cpp::queue_minutiae_stage: the group's own candidate grid), unconfined: the whole
//             chip, no CU-masked side streams — with the per-part scores of ALL the handle's queries kept in ctx->parts [.][G][4] —, then the caller's fusion -> ctx->scores:
//             m, the cell with the texture score left out (here k_fuse_stage1 per group, cascade.hip).  None of the texture stage's G-sized buffers (rm_*, the bound
//             pass's records, tex_slab) is touched
//   select    launch_rank_hits, unchanged, on that matrix at the ordered word of -inf with cap = keep: its device outputs are the kept lists
//   stage 2   the STRUCTURE of the pair tables is known beforehand (cascade_tables.h: every query that has pairs keeps n_kept = min(keep, G) prints) and goes up once,
//             before stage 1, with the caller's extra tables; the caller's gather kernel fills the tables from the kept lists (here k_cascade_gather, which also fills the
//             pairs' parts blocks); per chunk of option cascade_pairs_per_launch pairs and launch group the pair kernels afis_score_pairs proved bit-exact, as
//             that call queues them (queue_texture_pairs: the ADC kernel, the texture list kernel and, here, the fusion); the caller's closing kernel writes the kept cells into the combined matrix
//             (ctx->elig_scores, filled with the no-entry word by a memset of 0xff bytes; here k_cascade_scatter), which is swapped in at the end
// A kept pair whose print is empty or carries no texture template goes through the pair kernels as it is: k_adc_pairs skips a print without texture points before it
// reads one (n_rt <= 0), k_graph_texture's pair form writes +0.0f for such a pair before it reads a row maximum (n_lt <= 0 || n_rt <= 0), fuse_cell gives an empty print its -1.
// The driver runs over the resident shard or over a SUB-SHARD (CascadeCall::sub; afis_cascade_eligible.cpp): stage 1, the selection — which then names the kept prints
// through the sub-shard's d_global — and the pair kernels take CascadeCall::shard(); with own_matrix false the combined matrix is the caller's to size, fill and swap.
// casc_buf:  n_hits [n_q] int64 | kept [n_q][keep] int64 | kept score [n_q][keep] | own_kept_parts' [n_q][keep][kept_w] | pair parts [total][4] | pair score [total] | tab |
//            the tables that went up (cascade_tables.h's, then the caller's) | rm_val [P][lt_pad] | rm_arg [P][lt_pad], P = pairs of a chunk at most, lt_pad the handle's
//            longest texture template
#include "afis_ctx.h"
#include "cascade_tables.h"
#include "pair_tables.h"

using namespace afis;

static_assert(kCascadePairsPerLaunch == AFIS_CASCADE_PAIRS_PER_LAUNCH, "option cascade_pairs_per_launch's default is the header's");

namespace afis {

int CascadeCall::empty(int rc, int64_t* n_kept, int64_t* kept_idx, float* kept_parts)
{
    if (rc != AFIS_OK) { ctx->last_search = LastSearch{}; return rc; }
    for (int i = 0; i < n_q; ++i) {
        if (n_kept) n_kept[i] = 0;
        for (int r = 0; r < keep; ++r) {
            if (kept_idx) kept_idx[(size_t)i * keep + r] = -1;
            if (kept_parts) for (int c = 0; c < kept_w; ++c) kept_parts[((size_t)i * keep + r) * kept_w + c] = 0.0f;
        }
    }
    return AFIS_OK;
}

int CascadeCall::check_limits()
{
    const int64_t G = shard().gal.G;
    if ((int64_t)n_q * std::min<int64_t>(keep, G) > 0x7fffffffLL || (int64_t)n_q * G > 0x7ffffff0LL)
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_q x keep or n_q x G exceeds what one call takes");
    return AFIS_OK;
}

// Everything of the call that touches the device, for n_q > 0 and G > 0.  end() releases what the call allocated when this fails.
int CascadeCall::run(int64_t* n_kept, int64_t* kept_idx, float* kept_parts)
{
    Shard& sh = shard();                                                    // the resident shard, or the sub-shard of the call
    const int64_t G = sh.gal.G;
    base = ctx->index_base; nk = (int)std::min<int64_t>(keep, G);
    std::vector<QueryGroup> no_groups;
    std::vector<QueryGroup>& grps = groups ? *groups : no_groups;
    const size_t n_grp = grps.size();
    hipStream_t s = ctx->stream;
    // ---- the structure of stage 2, on the host
    CascadeTables tabs;
    if (!build_cascade_tables((size_t)n_q, has.data(), (size_t)nk, n_grp, q_first.data(), kAdcPairsSegment, (size_t)ctx->cascade_pairs_per_launch, tabs))
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_q x keep or n_q x G exceeds what one call takes");
    t = &tabs;
    std::vector<int32_t> up = tabs.dev;
    if (extra_tables) extra_tables(up);
    size_t n_pseudo = 0, Lp = 0;
    for (const QueryGroup& grp : grps) { n_pseudo += (size_t)grp.nq; Lp = std::max(Lp, (size_t)grp.dev.lt_pad); }
    const size_t total = tabs.total, n_pieces = tabs.pieces.size();
    const size_t P = std::min(total, (size_t)ctx->cascade_pairs_per_launch);
    const size_t n_out = (size_t)n_q * (size_t)keep, kparts_bytes = own_kept_parts ? n_out * (size_t)kept_w * 4 : 0;
    const size_t kept_at = up256((size_t)n_q * 8), kscore_at = up256(kept_at + n_out * 8), kparts_at = up256(kscore_at + n_out * 4), parts_at = up256(kparts_at + kparts_bytes),
                 score_at = up256(parts_at + std::max<size_t>(total, 1) * 16), tab_at = up256(score_at + std::max<size_t>(total, 1) * 4),
                 dev_at = up256(tab_at + std::max<size_t>(tabs.tab_ints(), 1) * 4), rmv_at = up256(dev_at + up.size() * 4), rma_at = up256(rmv_at + P * Lp * 4),
                 buf_bytes = rma_at + P * Lp * 4 + 16;
    // what returns through the pinned buffer: n_hits | kept | the kept parts (own_kept_parts' array, or the pair parts) | the diagnostics rows; behind them the tables on
    // their way up (pinned memory of the context, so that an early return leaves nothing queued that reads memory of this call)
    const size_t back_bytes = own_kept_parts ? kparts_bytes : total * 16, diag_bytes = std::max<size_t>(n_grp, 1) * kDiagWords * 8;
    const size_t pin_parts_at = up256(kept_at + n_out * 8), pin_diag_at = up256(pin_parts_at + back_bytes), pin_dev_at = up256(pin_diag_at + diag_bytes),
                 pin_bytes = pin_dev_at + up.size() * 4;
    // ---- room first: every allocation precedes everything the call queues and the first write into the caller's arrays
    const size_t n_cells = (size_t)n_q * (size_t)G;
    HIPCHK(ctx, ctx->scores.ensure(n_cells * 4));
    if (own_matrix) HIPCHK(ctx, ctx->elig_scores.ensure(n_cells * 4));
    if (own_matrix && sub && !sub->identity) HIPCHK(ctx, ctx->out_perm.ensure(n_cells * 4));     // (the scores leave in the caller's column order: afis_search_cascade_subset)
    HIPCHK(ctx, ctx->parts.ensure(std::max<size_t>(n_pseudo * (size_t)G * 16, 16)));
    AFISCHK(ensure_minutiae_stage(ctx, sh, grps, 1));
    HIPCHK(ctx, ctx->diag.ensure(diag_bytes));
    HIPCHK(ctx, ctx->casc_buf.ensure(buf_bytes));
    if (P > 0) HIPCHK(ctx, ctx->casc_slab.ensure(graph_texture_slab_bytes((long long)P)));
    HIPCHK(ctx, ensure_pin(ctx, pin_bytes));
    while (ctx->evpool.size() < n_grp * 10 + 2) { hipEvent_t e; HIPCHK(ctx, hipEventCreate(&e)); ctx->evpool.push_back(e); }
    Events ev(8);                                                           // four pairs: stage 1, selection, stage 2, and fuse_all alone (afis_timing's fuse_ms)
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));

    uint8_t* const d = ctx->casc_buf.as<uint8_t>();
    uint8_t* const pin = (uint8_t*)ctx->h_pin;
    d_kept = (long long*)(d + kept_at); d_kparts = (float*)(d + kparts_at); d_pparts = (float*)(d + parts_at); d_pscore = (float*)(d + score_at);
    d_tab = (int32_t*)(d + tab_at); d_dev = (const int32_t*)(d + dev_at); d_q_slot = d_dev + tabs.q_slot_at;
    // ---- the tables, then stage 1: the minutiae scorers for every cell, group after group on the whole chip
    memcpy(pin + pin_dev_at, up.data(), up.size() * 4);
    HIPCHK(ctx, hipMemcpyAsync(d + dev_at, pin + pin_dev_at, up.size() * 4, hipMemcpyHostToDevice, s));
    h2d_bytes = (int64_t)(up.size() * 4);
    HIPCHK(ctx, hipMemsetAsync(ctx->diag.p, 0, diag_bytes, s));
    HIPCHK(ctx, hipEventRecord(ev[0], s));
    int p0 = 0;
    for (size_t gi = 0; gi < n_grp; ++gi) {
        QueryGroup& grp = grps[gi];
        hipEvent_t* gev = &ctx->evpool[gi * 10];
        grp.overlapped = false;
        HIPCHK(ctx, hipEventRecord(gev[0], s));
        AFISCHK(queue_minutiae_stage(ctx, sh, grp, ctx->parts.as<float>() + (size_t)p0 * (size_t)G * 4, ctx->diag.as<unsigned long long>() + gi * kDiagWords, s, gev[1]));
        HIPCHK(ctx, hipEventRecord(gev[2], s));
        if (fuse_group) { AFISCHK(fuse_group(grp, p0)); HIPCHK(ctx, hipEventRecord(gev[3], s)); }
        p0 += grp.nq;
    }
    if (fuse_all) { HIPCHK(ctx, hipEventRecord(ev[6], s)); AFISCHK(fuse_all()); HIPCHK(ctx, hipEventRecord(ev[7], s)); }
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    // ---- selection: per query the nk best by m — rank_key descending, equal keys by ascending global index; every column is an entry
    HIPCHK(ctx, hipEventRecord(ev[2], s));
    HIPCHK(ctx, launch_rank_hits(ctx->scores.as<float>(), n_q, (int)G, nullptr, 0, nullptr, sub ? sub->d_global.as<long long>() : nullptr, base, kPosFloor, keep, (long long*)d, d_kept, (float*)(d + kscore_at), nullptr, s));
    HIPCHK(ctx, hipEventRecord(ev[3], s));
    // ---- stage 2: the texture scorer for the kept cells that are pairs, the caller's closing kernel for every kept cell
    HIPCHK(ctx, hipEventRecord(ev[4], s));
    if (own_matrix) HIPCHK(ctx, hipMemsetAsync(ctx->elig_scores.p, 0xff, n_cells * 4, s));
    if (own_kept_parts) HIPCHK(ctx, hipMemsetAsync(d_kparts, 0, kparts_bytes, s));
    AFISCHK(gather());
    for (size_t i = 0; i < n_pieces; ++i) {
        const CascadePiece& pc = tabs.pieces[i];
        const QueryDev& qd = grps[pc.group].dev;
        const size_t in_chunk = pc.first - pc.chunk * (size_t)ctx->cascade_pairs_per_launch;      // the piece's place in its chunk's row maxima: in_chunk + n <= P, and the group's stride qd.lt_pad <= Lp
        AFISCHK(queue_texture_pairs(ctx, sh.gal, qd, d_tab + 2 * pc.first + i, (int)pc.n, d_dev + tabs.seg_at + 2 * pc.seg_first, (int)pc.n_seg, (float*)(d + rmv_at) + in_chunk * Lp,
                                    (int32_t*)(d + rma_at) + in_chunk * Lp, d_pparts + pc.first * 4, ctx->casc_slab, fuse_pairs ? d_pscore + pc.first : nullptr, s));
    }
    AFISCHK(finish());
    HIPCHK(ctx, hipEventRecord(ev[5], s));
    // ---- what returns, through the pinned buffer; the one wait
    HIPCHK(ctx, hipMemcpyAsync(pin, d, kept_at + n_out * 8, hipMemcpyDeviceToHost, s));
    if (back_bytes > 0) HIPCHK(ctx, hipMemcpyAsync(pin + pin_parts_at, own_kept_parts ? d_kparts : d_pparts, back_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(pin + pin_diag_at, ctx->diag.p, diag_bytes, hipMemcpyDeviceToHost, s));
    AFISCHK(wait_streams(ctx, {s}, who));
    // ---- times: the options, each from its own pair of events; afis_timing reports stage 1
    afis_timing tm = {};
    float ms[4] = {0, 0, 0, 0};
    for (int k = 0; k < (fuse_all ? 4 : 3); ++k) HIPCHK(ctx, hipEventElapsedTime(&ms[k], ev[2 * k], ev[2 * k + 1]));
    for (int k = 0; k < 3; ++k) *opts[k] = (int64_t)((double)ms[k] * 1e3);
    *opts[3] = (int64_t)total;
    ctx->h_diag.assign(std::max<size_t>(n_grp, 1) * kDiagWords, 0ull);
    memcpy(ctx->h_diag.data(), pin + pin_diag_at, diag_bytes);
    minutiae_diagnostics(ctx, n_grp, tm);
    for (size_t i = 0; i < n_grp; ++i) {
        hipEvent_t* gev = &ctx->evpool[i * 10];
        float t_c = 0, t_g = 0, t_f = 0;
        HIPCHK(ctx, hipEventElapsedTime(&t_c, gev[0], gev[1])); HIPCHK(ctx, hipEventElapsedTime(&t_g, gev[1], gev[2]));
        if (fuse_group) HIPCHK(ctx, hipEventElapsedTime(&t_f, gev[2], gev[3]));
        tm.cands_ms += t_c; tm.minu_graph_ms += t_g; tm.minu_ms += t_c + t_g; tm.fuse_ms += t_f; tm.total_ms += t_c + t_g + t_f;
    }
    if (fuse_all) { tm.fuse_ms = ms[3]; tm.total_ms += ms[3]; }
    tm.pairs = (int64_t)n_pseudo * G; tm.launch_groups = (int32_t)n_grp;
    // ---- into the caller's arrays
    const long long* const h_hits = (const long long*)pin;
    const size_t w = (size_t)kept_w;
    for (int i = 0; i < n_q; ++i) {
        const size_t o = (size_t)i * (size_t)keep;
        if (n_kept) n_kept[i] = std::min<int64_t>(h_hits[i], keep);
        if (kept_idx) memcpy(kept_idx + o, pin + kept_at + o * 8, (size_t)keep * 8);
        if (kept_parts && own_kept_parts) memcpy(kept_parts + o * w, pin + pin_parts_at + o * w * 4, (size_t)keep * w * 4);
        else if (kept_parts) {
            memset(kept_parts + o * w, 0, (size_t)keep * w * 4);               // +0.0f: the padding, and the cells of a query without pairs (no scorer ran)
            if (has[(size_t)i]) memcpy(kept_parts + o * w, pin + pin_parts_at + tabs.q_slot[(size_t)i] * 16, (size_t)nk * 16);
        }
    }
    if (own_matrix) std::swap(ctx->scores, ctx->elig_scores);               // the combined matrix is the last search's from here on
    ctx->timing = tm;
    return AFIS_OK;
}

int CascadeCall::end(int rc, float* scores)
{
    const int64_t G = shard().gal.G;
    if (rc == AFIS_OK && scores) {                                          // the device is idle: a plain copy, as at the end of a search
        const hipError_t e = hipMemcpy(scores, ctx->scores.p, (size_t)n_q * (size_t)G * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, AFIS_EDEVICE, std::string(who) + ": the scores: " + hipGetErrorString(e));
    }
    if (rc != AFIS_OK) {                                                    // the call holds nothing it allocated; after a timeout the device may still use it: the bounded wait first
        const std::string keep_err = ctx->err;
        (void)quiesce(ctx, who);
        ctx->err = keep_err;
        ctx->casc_buf.release(); ctx->casc_slab.release(); ctx->elig_scores.release();
        clear();
        ctx->timing = afis_timing{};
    }
    ctx->last_search = rc == AFIS_OK ? LastSearch{true, n_q, G, sub, ctx->gallery_epoch} : LastSearch{};
    t = nullptr;
    return rc;
}

}  // namespace afis

// afis_search_cascade's queries are the handle's queries, its groups the handle's groups; a pair's four parts are the kept cell's
int afis::latent_cascade(CascadeCall& c, afis_queries* q, const CascadeMap* map, int64_t* n_kept, int64_t* kept_idx, float* kept_parts)
{
    afis_ctx* const ctx = c.ctx;
    const GalleryDev& gal = c.shard().gal;
    const int n_q = c.n_q, keep = c.keep, G = (int)gal.G, G_res = (int)ctx->gal.G;
    hipStream_t s = ctx->stream;
    AFISCHK(c.check_limits());
    c.q_first.assign(1, 0);
    for (const QueryGroup& grp : q->groups) c.q_first.push_back(c.q_first.back() + grp.nq);
    if (c.q_first.back() != n_q) return fail(ctx, AFIS_EINVAL, std::string(c.who) + ": the query handle's launch groups do not add up to its queries");
    c.has.resize((size_t)n_q);
    for (int i = 0; i < n_q; ++i) c.has[(size_t)i] = q->status[(size_t)i] == AFIS_QUERY_OK;
    c.groups = &q->groups;
    c.fuse_pairs = true;
    c.fuse_group = [&](const QueryGroup& grp, int q0) -> int {
        HIPCHK(ctx, launch_fuse_stage1(grp.dev, gal, ctx->parts.as<float>() + (size_t)q0 * (size_t)G * 4, ctx->scores.as<float>() + (size_t)q0 * (size_t)G, s));
        return AFIS_OK;
    };
    size_t inv_at = 0, col_at = 0, row_at = 0;                              // int positions of the map's tables behind cascade_tables.h's
    if (map) c.extra_tables = [&](std::vector<int32_t>& up) {
        inv_at = up.size(); up.insert(up.end(), map->inv->begin(), map->inv->end());
        col_at = up.size(); up.insert(up.end(), map->out_col->begin(), map->out_col->end());
        row_at = up.size(); up.insert(up.end(), map->row_of->begin(), map->row_of->end());
    };
    const auto table = [&](const std::vector<int32_t>* v, size_t at) { return v->empty() ? nullptr : c.d_dev + at; };
    c.gather = [&]() -> int {
        if (map) {
            HIPCHK(ctx, launch_cascade_gather_mapped(n_q, G_res, G, keep, c.nk, c.base, c.d_kept, c.d_q_slot, c.d_dev + c.t->piece_first_at, (int)c.t->pieces.size(),
                                                     c.d_dev + c.t->piece_q0_at, table(map->inv, inv_at), ctx->parts.as<float>(), c.d_tab, c.d_pparts, s));
            return AFIS_OK;
        }
        HIPCHK(ctx, launch_cascade_gather(n_q, G, keep, c.nk, c.base, c.d_kept, c.d_q_slot, c.d_dev + c.t->piece_first_at, (int)c.t->pieces.size(), c.d_dev + c.t->piece_q0_at,
                                          ctx->parts.as<float>(), c.d_tab, c.d_pparts, s));
        return AFIS_OK;
    };
    c.finish = [&]() -> int {
        if (map) {
            HIPCHK(ctx, launch_cascade_scatter_mapped(n_q, G_res, G, keep, c.nk, c.base, c.d_kept, c.d_q_slot, c.d_pscore, table(map->inv, inv_at), table(map->row_of, row_at),
                                                      table(map->out_col, col_at), (long long)map->out_rows, (long long)map->out_stride, ctx->elig_scores.as<float>(), s));
            return AFIS_OK;
        }
        HIPCHK(ctx, launch_cascade_scatter(n_q, G, keep, c.nk, c.base, c.d_kept, c.d_q_slot, c.d_pscore, ctx->elig_scores.as<float>(), s));
        return AFIS_OK;
    };
    return c.run(n_kept, kept_idx, kept_parts);
}

extern "C" {

int afis_search_cascade(afis_ctx* ctx, afis_queries* q, int keep, float* scores, int32_t* status, int64_t* n_kept, int64_t* kept_idx, float* kept_parts)
{
    const char* const who = "afis_search_cascade";
    if (!ctx || !q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    CascadeCall c{ctx, who, q->n_q, keep, {&ctx->cascade_stage1_us, &ctx->cascade_select_us, &ctx->cascade_stage2_us, &ctx->cascade_kept_pairs}, 4, false};
    c.clear();
    ctx->last_search.valid = false;
    if (keep < 1 || keep > AFIS_HITS_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": keep must be 1 .. AFIS_HITS_MAX, the longest list the selection makes");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    AFISCHK(check_query_handle(ctx, who, q, (int64_t)ctx->gal.G));          // afis_search_resident's rules for the handle
    if (q->n_q == 0 || ctx->gal.G == 0)                                      // nothing to score: as afis_search_resident answers it; no list holds anything
        return c.empty(search_shard(ctx, *ctx, nullptr, q, scores, nullptr, status, 0, nullptr, nullptr), n_kept, kept_idx, kept_parts);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx));
    const int rc = c.end(latent_cascade(c, q, nullptr, n_kept, kept_idx, kept_parts), scores);
    if (rc == AFIS_OK && status) for (int i = 0; i < q->n_q; ++i) status[i] = q->status[(size_t)i];
    return rc;
}

}  // extern "C"
