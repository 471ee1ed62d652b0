// afis_print_cascade.cpp — the print cascade of the C ABI (include/afis_matcher.h): afis_search_prints_cascade takes RESIDENT prints as queries, runs the minutiae scorer
// for every (query print, column print) cell of the resident shard, selects per query the `keep` best columns by that partial score on the device, and runs the texture
// scorer for the kept cells only.  A kept cell is, bit for bit, afis_search_prints'; every other cell holds the "no entry" word (score_order.h), so the ranking family
// reads the matrix as it reads afis_search_cascade's.  A query with something active is one PSEUDO-QUERY of a temporary handle that is filled on the device
// (afis_prints.cpp::build_print_queries: its own bounded wait; the texture view is gathered only where the texture term is active); after it one launch sequence on the
// context's stream, no host round trip between the stages, one wait at the end:
//   stage 1   per launch group of the handle the candidate kernel and the minutiae list kernel — the body of search_shard's minutiae stage, unconfined: the whole chip,
//             no CU-masked side streams — with the per-part scores of ALL pseudo-queries kept in ctx->parts [n_pseudo][G][4], then k_print_cascade_stage1
//             (print_cascade.hip) -> ctx->scores [n_q][G]: m, the print cell with the texture term left out.  None of the texture stage's G-sized buffers is touched
//   select    launch_rank_hits, unchanged, on that matrix at the ordered word of -inf with cap = keep: its device outputs are the kept lists
//   stage 2   the STRUCTURE of the pair tables is known beforehand (cascade_tables.h with has[q] = "the texture term of query q is active": such a query keeps
//             n_kept = min(keep, G) columns) and goes up once, with the queries' rows and weights; k_print_cascade_gather fills the tables from the kept lists; per
//             chunk of option cascade_pairs_per_launch pairs and launch group launch_adc_pairs and launch_graph_texture_pairs; k_print_cascade_finish folds every
//             kept cell into the combined matrix (ctx->elig_scores, filled with the no-entry word by a memset of 0xff bytes), which is swapped in at the end, and
//             writes the kept cells' two parts
// The queries of the call and the pseudo-queries of the handle differ, so the tables' launch groups are stated in QUERIES: group g begins at the query of its first
// pseudo-query (group 0 at query 0); the queries between two pseudo-queries have no pairs, whatever group they are counted in.
// casc_buf:  n_hits [n_q] int64 | kept [n_q][keep] int64 | kept score [n_q][keep] | kept parts [n_q][keep][2] | pair parts [total][4] | tab | the tables of
//            cascade_tables.h | q_row [n_q] | piece_p0 [n_pieces] | q_w [n_q][2] | rm_val [P][lt_pad] | rm_arg [P][lt_pad], P = pairs of a chunk at most, lt_pad the
//            handle's longest texture view
#include "afis_ctx.h"
#include "cascade_tables.h"
#include "pair_tables.h"

using namespace afis;

namespace {

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

struct EventSet {                                   // four pairs of events: stage 1, selection, stage 2, and k_print_cascade_stage1 alone (afis_timing's fuse_ms)
    hipEvent_t e[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    EventSet() = default;  EventSet(const EventSet&) = delete;
    ~EventSet() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

void clear_options(afis_ctx* ctx)
{
    ctx->print_cascade_stage1_us = ctx->print_cascade_select_us = ctx->print_cascade_stage2_us = ctx->print_cascade_kept_pairs = 0;
    ctx->print_gather_us = 0; ctx->print_h2d_bytes = 0;
}

// one query of the call: its print (shard-local) and what of it is active
struct PQuery { int32_t local; bool am, at; };

// Everything of the call that touches the device, for n_q > 0 and G > 0.  The caller releases what the call allocated when this fails; `plans` and `up` (the host's
// copies of tables a copy may still read) live in the caller, beyond its bounded wait.
int cascade(afis_ctx* ctx, const char* who, const std::vector<PQuery>& pq, const float* w_minu, const float* w_tex, int keep, int64_t* n_kept, int64_t* kept_idx,
            float* kept_parts, std::vector<PrintGroupPlan>& plans, std::vector<int32_t>& up)
{
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    const int n_q = (int)pq.size();
    const int nk = (int)std::min<int64_t>(keep, G);
    hipStream_t s = ctx->stream;
    if ((int64_t)n_q * nk > 0x7fffffffLL || (int64_t)n_q * G > 0x7ffffff0LL) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_q x keep or n_q x G exceeds what one call takes");
    // ---- the pseudo-queries and the temporary handle: the views gathered on the device, one bounded wait
    std::vector<int32_t> local, q_row((size_t)n_q, -1), pseudo_q;
    std::vector<uint8_t> use_m, use_t, has((size_t)n_q, 0);
    std::vector<float> q_w((size_t)n_q * 2, 0.0f);
    for (int i = 0; i < n_q; ++i) {
        const PQuery& p = pq[(size_t)i];
        has[(size_t)i] = p.at;
        if (!p.am && !p.at) continue;
        q_row[(size_t)i] = (int32_t)local.size();
        q_w[(size_t)i * 2] = p.am ? w_minu[i] : 0.0f; q_w[(size_t)i * 2 + 1] = p.at ? w_tex[i] : 0.0f;
        local.push_back(p.local); use_m.push_back(p.am); use_t.push_back(p.at); pseudo_q.push_back(i);
    }
    const int n_pseudo = (int)local.size();
    afis_queries* q = nullptr;
    struct FreeQ { afis_ctx* c; afis_queries** q; ~FreeQ() { afis_queries_free(c, *q); } } free_q{ctx, &q};     // (parked while a timed-out launch may still read it)
    int64_t h2d = 0, gather_us = 0;
    if (n_pseudo > 0) {
        const std::vector<int32_t> res_tile = resident_tile_offsets(ctx);
        AFISCHK(build_print_queries(ctx, who, res_tile, local.data(), use_m.data(), use_t.data(), n_pseudo, false, plans, &q, &h2d, &gather_us));
    }
    std::vector<QueryGroup> no_groups;                                      // (no query has anything active: no handle, every kept cell is the -1)
    std::vector<QueryGroup>& groups = q ? q->groups : no_groups;
    const size_t n_grp = groups.size();
    // ---- the structure of stage 2, on the host
    std::vector<int32_t> q_first(n_grp + 1, 0), p_first(n_grp + 1, 0);
    int nq_max = 0, nL_max = 1, lt_pad = 0;
    for (size_t gi = 0; gi < n_grp; ++gi) {
        const QueryGroup& grp = groups[gi];
        p_first[gi + 1] = p_first[gi] + grp.nq;
        nq_max = std::max(nq_max, grp.nq); nL_max = std::max(nL_max, grp.max_nL); lt_pad = std::max(lt_pad, (int)grp.dev.lt_pad);
    }
    if (p_first[n_grp] != n_pseudo) return fail(ctx, AFIS_EINVAL, std::string(who) + ": the query handle's launch groups do not add up to its pseudo-queries");
    for (size_t gi = 1; gi < n_grp; ++gi) q_first[gi] = pseudo_q[(size_t)p_first[gi]];
    q_first[n_grp] = n_q;
    CascadeTables t;
    if (!build_cascade_tables((size_t)n_q, has.data(), (size_t)nk, n_grp, q_first.data(), kAdcPairsSegment, (size_t)ctx->cascade_pairs_per_launch, t))
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_q x keep or n_q x G exceeds what one call takes");
    const size_t total = t.total, n_pieces = t.pieces.size();
    const size_t P = std::min(total, (size_t)ctx->cascade_pairs_per_launch), Lp = (size_t)lt_pad;
    const size_t n_out = (size_t)n_q * (size_t)keep;
    // what goes up once: the tables of cascade_tables.h | q_row [n_q] | piece_p0 [n_pieces] | q_w [n_q][2] (on an 8-byte boundary)
    const size_t up_row_at = t.dev.size(), up_p0_at = up_row_at + (size_t)n_q, up_w_at = (up_p0_at + n_pieces + 1) / 2 * 2, up_ints = up_w_at + (size_t)n_q * 2;
    up.assign(up_ints, 0);
    memcpy(up.data(), t.dev.data(), t.dev.size() * 4);
    memcpy(up.data() + up_row_at, q_row.data(), (size_t)n_q * 4);
    for (size_t i = 0; i < n_pieces; ++i) up[up_p0_at + i] = p_first[t.pieces[i].group];
    memcpy(up.data() + up_w_at, q_w.data(), (size_t)n_q * 8);
    const size_t kept_at = up256((size_t)n_q * 8), kscore_at = up256(kept_at + n_out * 8), kparts_at = up256(kscore_at + n_out * 4), parts_at = up256(kparts_at + n_out * 8),
                 tab_at = up256(parts_at + std::max<size_t>(total, 1) * 16), dev_at = up256(tab_at + std::max<size_t>(t.tab_ints(), 1) * 4), rmv_at = up256(dev_at + up_ints * 4),
                 rma_at = up256(rmv_at + P * Lp * 4), buf_bytes = rma_at + P * Lp * 4 + 16;
    // what returns through the pinned buffer: n_hits | kept | kept parts | the diagnostics rows
    const size_t pin_kparts_at = up256(kept_at + n_out * 8), pin_diag_at = up256(pin_kparts_at + n_out * 8), diag_bytes = std::max<size_t>(n_grp, 1) * kDiagWords * 8,
                 pin_bytes = pin_diag_at + diag_bytes;
    // ---- room first: every allocation precedes everything the cascade queues and the first write into the caller's arrays
    const size_t n_cells = (size_t)n_q * (size_t)G, grp_pairs = (size_t)nq_max * (size_t)G;
    const size_t per_wg = minu_scratch_floats(nL_max, ctx->max_nR, ctx->s3_tie_order);
    int n_wg = 1024;
    while (n_wg > 64 && per_wg * 4 * n_wg > (8ull << 30)) n_wg /= 2;
    const size_t minu_slab_1 = graph_minutiae_slab_bytes(3 * (long long)grp_pairs);
    HIPCHK(ctx, ctx->scores.ensure(n_cells * 4));
    HIPCHK(ctx, ctx->elig_scores.ensure(n_cells * 4));
    HIPCHK(ctx, ctx->parts.ensure(std::max<size_t>((size_t)n_pseudo * (size_t)G * 16, 16)));
    if (n_grp > 0) {
        HIPCHK(ctx, ctx->cands.ensure(grp_pairs * 3 * kTopMinu * sizeof(MinuCand)));
        HIPCHK(ctx, ctx->cand_n.ensure(grp_pairs * 3 * 4));
        HIPCHK(ctx, ctx->minu_fb.ensure(minu_fb_ints(grp_pairs * 3, (size_t)G) * 4));
        HIPCHK(ctx, ctx->minu_slab.ensure(minu_slab_1));
        HIPCHK(ctx, ctx->scratch.ensure(per_wg * 4 * (size_t)n_wg));
    }
    HIPCHK(ctx, ctx->diag.ensure(diag_bytes));
    HIPCHK(ctx, ctx->casc_buf.ensure(buf_bytes));
    if (P > 0) HIPCHK(ctx, ctx->casc_slab.ensure(graph_texture_slab_bytes((long long)P)));
    HIPCHK(ctx, ensure_pin(ctx, pin_bytes));
    while (ctx->evpool.size() < n_grp * 10 + 2) { hipEvent_t e; HIPCHK(ctx, hipEventCreate(&e)); ctx->evpool.push_back(e); }
    EventSet ev;
    for (hipEvent_t& e : ev.e) HIPCHK(ctx, hipEventCreate(&e));

    uint8_t* const d = ctx->casc_buf.as<uint8_t>();
    uint8_t* const pin = (uint8_t*)ctx->h_pin;
    long long* const d_kept = (long long*)(d + kept_at);
    float* const d_kparts = (float*)(d + kparts_at);
    const int32_t* const d_dev = (const int32_t*)(d + dev_at);
    const int32_t* const d_q_slot = d_dev + t.q_slot_at;
    const int32_t* const d_q_row = d_dev + up_row_at;
    const float* const d_q_w = (const float*)(d_dev + up_w_at);
    int32_t* const d_tab = (int32_t*)(d + tab_at);
    float* const d_pparts = (float*)(d + parts_at);
    // ---- the tables, then stage 1: the minutiae scorer for every cell, group after group on the whole chip
    HIPCHK(ctx, hipMemcpyAsync(d + dev_at, up.data(), up_ints * 4, hipMemcpyHostToDevice, s));
    h2d += (int64_t)(up_ints * 4);
    HIPCHK(ctx, hipMemsetAsync(ctx->diag.p, 0, diag_bytes, s));
    HIPCHK(ctx, hipEventRecord(ev.e[0], s));
    int p0 = 0;
    for (size_t gi = 0; gi < n_grp; ++gi) {
        QueryGroup& grp = groups[gi];
        const QueryDev& qd = grp.dev;
        hipEvent_t* gev = &ctx->evpool[gi * 10];
        unsigned long long* const diag_row = ctx->diag.as<unsigned long long>() + gi * kDiagWords;
        float* const grp_parts = ctx->parts.as<float>() + (size_t)p0 * (size_t)G * 4;
        const size_t wg_floats = minu_scratch_floats(grp.max_nL, ctx->max_nR, ctx->s3_tie_order);
        grp.overlapped = false;
        HIPCHK(ctx, hipEventRecord(gev[0], s));
        HIPCHK(ctx, launch_minu_cands(qd, ctx->gal, ctx->scratch.as<float>(), wg_floats, n_wg, ctx->minu_generic | (ctx->s3_tie_order << 1), ctx->cands.as<MinuCand>(), ctx->cand_n.as<int32_t>(),
                                      ctx->minu_fb.as<int32_t>(), grp.max_nL, ctx->max_nR, diag_row, s));
        HIPCHK(ctx, hipEventRecord(gev[1], s));
        HIPCHK(ctx, launch_graph_minutiae(qd, ctx->gal, ctx->cands.as<MinuCand>(), ctx->cand_n.as<int32_t>(), grp_parts, nullptr, nullptr, ctx->minu_slab.p, minu_slab_1, nullptr, nullptr,
                                          2 | (ctx->s89_tie_order << 8), s));
        HIPCHK(ctx, hipEventRecord(gev[2], s));
        p0 += grp.nq;
    }
    HIPCHK(ctx, hipEventRecord(ev.e[6], s));
    HIPCHK(ctx, launch_print_cascade_stage1(ctx->parts.as<float>(), d_q_row, d_q_w, ctx->gal.empty, n_q, (int)G, ctx->scores.as<float>(), s));
    HIPCHK(ctx, hipEventRecord(ev.e[7], s));
    HIPCHK(ctx, hipEventRecord(ev.e[1], s));
    // ---- selection: per query the nk best by m — rank_key descending, equal keys by ascending global index; every column is an entry
    HIPCHK(ctx, hipEventRecord(ev.e[2], s));
    HIPCHK(ctx, launch_rank_hits(ctx->scores.as<float>(), n_q, (int)G, nullptr, 0, nullptr, nullptr, (long long)base, kPosFloor, keep, (long long*)d, d_kept, (float*)(d + kscore_at), nullptr, s));
    HIPCHK(ctx, hipEventRecord(ev.e[3], s));
    // ---- stage 2: the texture scorer for the kept cells of the queries whose texture term is active, the fold for every kept cell
    HIPCHK(ctx, hipEventRecord(ev.e[4], s));
    HIPCHK(ctx, hipMemsetAsync(ctx->elig_scores.p, 0xff, n_cells * 4, s));
    HIPCHK(ctx, hipMemsetAsync(d_kparts, 0, n_out * 8, s));
    HIPCHK(ctx, launch_print_cascade_gather(n_q, (int)G, keep, nk, (long long)base, d_kept, d_q_slot, d_dev + t.piece_first_at, (int)n_pieces, d_dev + up_p0_at, d_q_row, d_tab, s));
    for (size_t i = 0; i < n_pieces; ++i) {
        const CascadePiece& pc = t.pieces[i];
        const QueryDev& qd = groups[pc.group].dev;
        const size_t in_chunk = pc.first - pc.chunk * (size_t)ctx->cascade_pairs_per_launch;      // the piece's place in its chunk's row maxima: in_chunk + n <= P, and the group's stride qd.lt_pad <= Lp
        const int32_t* const p_tab = d_tab + 2 * pc.first + i;
        float* const rm_val = (float*)(d + rmv_at) + in_chunk * Lp;
        int32_t* const rm_arg = (int32_t*)(d + rma_at) + in_chunk * Lp;
        HIPCHK(ctx, launch_adc_pairs(qd, ctx->gal, ctx->codewords.as<float>(), p_tab, d_dev + t.seg_at + 2 * pc.seg_first, (int)pc.n_seg, rm_val, rm_arg, s));
        HIPCHK(ctx, launch_graph_texture_pairs(qd, ctx->gal, p_tab, (int)pc.n, ctx->table.as<float>(), rm_val, rm_arg, d_pparts + pc.first * 4, ctx->casc_slab.p, ctx->casc_slab.bytes,
                                               ctx->s89_tie_order, s));
    }
    HIPCHK(ctx, launch_print_cascade_finish(n_q, (int)G, keep, nk, (long long)base, d_kept, d_q_slot, d_q_row, d_q_w, ctx->gal.empty, ctx->parts.as<float>(), d_pparts,
                                            ctx->elig_scores.as<float>(), d_kparts, s));
    HIPCHK(ctx, hipEventRecord(ev.e[5], s));
    // ---- what returns, through the pinned buffer; the one wait
    HIPCHK(ctx, hipMemcpyAsync(pin, d, kept_at + n_out * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(pin + pin_kparts_at, d_kparts, n_out * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(pin + pin_diag_at, ctx->diag.p, diag_bytes, hipMemcpyDeviceToHost, s));
    AFISCHK(wait_streams(ctx, {s}, who));
    // ---- times: the options, each from its own pair of events; afis_timing reports stage 1
    afis_timing tm = {};
    {
        float ms[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) HIPCHK(ctx, hipEventElapsedTime(&ms[k], ev.e[2 * k], ev.e[2 * k + 1]));
        ctx->print_cascade_stage1_us = (int64_t)((double)ms[0] * 1e3); ctx->print_cascade_select_us = (int64_t)((double)ms[1] * 1e3);
        ctx->print_cascade_stage2_us = (int64_t)((double)ms[2] * 1e3);
        ctx->print_cascade_kept_pairs = (int64_t)total;
        ctx->print_gather_us = gather_us; ctx->print_h2d_bytes = h2d;
        ctx->h_diag.assign(std::max<size_t>(n_grp, 1) * kDiagWords, 0ull);
        memcpy(ctx->h_diag.data(), pin + pin_diag_at, diag_bytes);
        unsigned long long acc[kDiagWords] = {};
        for (size_t i = 0; i < n_grp; ++i) for (int w = 0; w < kDiagWords; ++w) acc[w] += ctx->h_diag[i * kDiagWords + w];
        tm.minu_fallback_tasks = (int64_t)acc[kDiagFallback];
        tm.minu_tasks_small = (int64_t)acc[kDiagSmall]; tm.minu_tasks_medium = (int64_t)acc[kDiagSmall + 1]; tm.minu_tasks_large = (int64_t)acc[kDiagSmall + 2];
        tm.minu_tasks = tm.minu_tasks_small + tm.minu_tasks_medium + tm.minu_tasks_large + tm.minu_fallback_tasks;
        tm.cands_clock_ghz = acc[kDiagCandsWall] ? (float)((double)acc[kDiagCandsClk] / (double)acc[kDiagCandsWall] * 0.1) : 0.0f;
        for (size_t i = 0; i < n_grp; ++i) {
            hipEvent_t* gev = &ctx->evpool[i * 10];
            float t_c = 0, t_g = 0;
            HIPCHK(ctx, hipEventElapsedTime(&t_c, gev[0], gev[1])); HIPCHK(ctx, hipEventElapsedTime(&t_g, gev[1], gev[2]));
            tm.cands_ms += t_c; tm.minu_graph_ms += t_g; tm.minu_ms += t_c + t_g; tm.total_ms += t_c + t_g;
        }
        tm.fuse_ms = ms[3]; tm.total_ms += ms[3];
        tm.pairs = (int64_t)n_pseudo * G; tm.launch_groups = (int32_t)n_grp;
    }
    // ---- into the caller's arrays
    const long long* const h_hits = (const long long*)pin;
    for (int i = 0; i < n_q; ++i) {
        const size_t o = (size_t)i * (size_t)keep;
        if (n_kept) n_kept[i] = std::min<int64_t>(h_hits[i], keep);
        if (kept_idx) memcpy(kept_idx + o, pin + kept_at + o * 8, (size_t)keep * 8);
        if (kept_parts) memcpy(kept_parts + o * 2, pin + pin_kparts_at + o * 8, (size_t)keep * 8);
    }
    std::swap(ctx->scores, ctx->elig_scores);                               // the combined matrix is the last search's from here on
    ctx->timing = tm;
    return AFIS_OK;
}

}  // namespace

extern "C" {

int afis_search_prints_cascade(afis_ctx* ctx, const int64_t* idx, int n_q, const float* w_minu, const float* w_tex, int keep, float* scores, int32_t* status, int64_t* n_kept,
                               int64_t* kept_idx, float* kept_parts)
{
    const char* const who = "afis_search_prints_cascade";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null context");
    clear_options(ctx);
    ctx->last_search = LastSearch{};                                        // whatever this call returns, the matrix of an earlier search is no longer there to rank
    if (n_q < 0 || (n_q > 0 && (!idx || !w_minu || !w_tex))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": bad argument");
    for (int k = 0; k < 2; ++k) {
        const float* w = k ? w_tex : w_minu;
        for (int i = 0; i < n_q; ++i)
            if (!(w[i] >= 0.0f) || std::isinf(w[i])) return fail(ctx, AFIS_EINVAL, std::string(who) + ": a weight must be finite and >= 0 (-1 means \"empty\", every other cell is >= +0)");
    }
    if (keep < 1 || keep > AFIS_HITS_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": keep must be 1 .. AFIS_HITS_MAX, the longest list the selection makes");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    const int64_t G_res = (int64_t)ctx->res_empty.size(), G_all = afis_gallery_size(ctx);
    for (int i = 0; i < n_q; ++i) {
        const int64_t t = idx[i] - ctx->index_base;
        if (idx[i] < ctx->index_base || t >= G_all) return fail(ctx, AFIS_EINVAL, std::string(who) + ": index " + std::to_string((long long)idx[i]) + " is outside the resident shard");
        if (t >= G_res) return fail(ctx, AFIS_ESTATE, std::string(who) + ": index " + std::to_string((long long)idx[i]) + " is staged but not committed (afis_gallery_commit first)");
    }
    const int64_t G = (int64_t)ctx->gal.G;
    if (n_q == 0 || G == 0) {                                               // nothing to score: as afis_search answers it; no list holds anything
        const int rc = afis_search(ctx, nullptr, 0, scores, nullptr, nullptr, 0, nullptr, nullptr);
        if (rc != AFIS_OK) { ctx->last_search = LastSearch{}; return rc; }
        for (int i = 0; i < n_q; ++i) {
            if (status) status[i] = AFIS_QUERY_LATENT_EMPTY;
            if (n_kept) n_kept[i] = 0;
            for (int r = 0; r < keep; ++r) {
                if (kept_idx) kept_idx[(size_t)i * keep + r] = -1;
                if (kept_parts) kept_parts[((size_t)i * keep + r) * 2] = kept_parts[((size_t)i * keep + r) * 2 + 1] = 0.0f;
            }
        }
        return AFIS_OK;
    }
    // what of every print is active: afis_search_prints' rule
    std::vector<PQuery> pq((size_t)n_q);
    for (int i = 0; i < n_q; ++i) {
        PQuery& p = pq[(size_t)i];
        p.local = (int32_t)(idx[i] - ctx->index_base);
        p.am = ctx->res_mo[(size_t)p.local + 1] > ctx->res_mo[(size_t)p.local] && w_minu[i] != 0.0f;
        p.at = ctx->res_to[(size_t)p.local + 1] > ctx->res_to[(size_t)p.local] && w_tex[i] != 0.0f;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx));
    std::vector<PrintGroupPlan> plans;
    std::vector<int32_t> up;
    int rc = cascade(ctx, who, pq, w_minu, w_tex, keep, n_kept, kept_idx, kept_parts, plans, up);
    if (rc == AFIS_OK && scores) {                                          // the device is idle: a plain copy, as at the end of a search
        const hipError_t e = hipMemcpy(scores, ctx->scores.p, (size_t)n_q * (size_t)G * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, AFIS_EDEVICE, std::string(who) + ": the scores: " + hipGetErrorString(e));
    }
    if (rc == AFIS_OK && status) for (int i = 0; i < n_q; ++i) status[i] = pq[(size_t)i].am || pq[(size_t)i].at ? AFIS_QUERY_OK : AFIS_QUERY_LATENT_EMPTY;
    if (rc != AFIS_OK) {                                                    // the call holds nothing it allocated; after a timeout the device may still use it: the bounded wait first
        const std::string keep_err = ctx->err;
        (void)quiesce(ctx, who);
        ctx->err = keep_err;
        ctx->casc_buf.release(); ctx->casc_slab.release(); ctx->elig_scores.release();
        clear_options(ctx);
        ctx->timing = afis_timing{};
    }
    ctx->last_search = rc == AFIS_OK ? LastSearch{true, n_q, G, nullptr, ctx->gallery_epoch} : LastSearch{};
    return rc;
}

}  // extern "C"
