// afis_cascade.cpp — the cascade search of the C ABI (include/afis_matcher.h): afis_search_cascade runs the three minutiae scorers for every (latent, print) cell of the
// resident shard, selects per latent the `keep` best prints by that partial score on the device, and runs the texture scorer for the kept cells only.  A kept cell is,
// bit for bit, afis_search's; every other cell holds the "no entry" word (score_order.h), so the ranking family reads the matrix as it reads afis_search_eligible's.
// One launch sequence on the context's stream, no host round trip between the stages, one wait at the end:
//   stage 1   per launch group of the handle the candidate kernel and the minutiae list kernel — the body of search_shard's minutiae stage, unconfined: the whole chip,
//             no CU-masked side streams — with the per-part scores of ALL queries kept in ctx->parts [n_q][G][4], then k_fuse_stage1 (cascade.hip) -> ctx->scores: m, the
//             fusion with the texture score taken as +0.0f.  None of the texture stage's G-sized buffers (rm_*, the bound pass's records, tex_slab) is touched
//   select    launch_rank_hits, unchanged, on that matrix at the ordered word of -inf with cap = keep: its device outputs are the kept lists
//   stage 2   the STRUCTURE of the pair tables is known beforehand (cascade_tables.h: every query that is scored keeps n_kept = min(keep, G) prints) and goes up once;
//             k_cascade_gather fills the tables and the pairs' parts blocks from the kept lists; per chunk of option cascade_pairs_per_launch pairs and launch group
//             the pair kernels afis_score_pairs proved bit-exact — launch_adc_pairs, launch_graph_texture_pairs, launch_fuse_pairs —; k_cascade_scatter writes the
//             pair scores into the combined matrix (ctx->elig_scores, filled with the no-entry word by a memset of 0xff bytes), which is swapped in at the end
// A kept pair whose print is empty or carries no texture template goes through the pair kernels as it is: k_adc_pairs skips a print without texture points before it
// reads one (n_rt <= 0), k_graph_texture's pair form writes +0.0f for such a pair before it reads a row maximum (n_lt <= 0 || n_rt <= 0), fuse_cell gives an empty print its -1.
// casc_buf:  n_hits [n_q] int64 | kept [n_q][keep] int64 | kept score [n_q][keep] | pair parts [total][4] | pair score [total] | tab | the tables of cascade_tables.h |
//            rm_val [P][lt_pad] | rm_arg [P][lt_pad], P = pairs of a chunk at most, lt_pad the handle's longest latent texture template
#include "afis_ctx.h"
#include "cascade_tables.h"
#include "pair_tables.h"

using namespace afis;

static_assert(kCascadePairsPerLaunch == AFIS_CASCADE_PAIRS_PER_LAUNCH, "option cascade_pairs_per_launch's default is the header's");

namespace {

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

struct EventSet {                                   // three pairs of events: stage 1, selection, stage 2
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    EventSet() = default;  EventSet(const EventSet&) = delete;
    ~EventSet() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

void clear_cascade_options(afis_ctx* ctx) { ctx->cascade_stage1_us = ctx->cascade_select_us = ctx->cascade_stage2_us = ctx->cascade_kept_pairs = 0; }

// Everything of the call that touches the device, for n_q > 0 and G > 0.  The caller releases what the call allocated when this fails.
int cascade(afis_ctx* ctx, const char* who, afis_queries* q, int keep, int32_t* status, int64_t* n_kept, int64_t* kept_idx, float* kept_parts)
{
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    const int n_q = q->n_q;
    const int nk = (int)std::min<int64_t>(keep, G);
    const size_t n_grp = q->groups.size();
    hipStream_t s = ctx->stream;
    // ---- the structure of stage 2, on the host
    std::vector<int32_t> q_first(n_grp + 1, 0);
    int nq_max = 0, nL_max = 1, lt_pad = 0;
    for (size_t gi = 0; gi < n_grp; ++gi) {
        const QueryGroup& grp = q->groups[gi];
        q_first[gi + 1] = q_first[gi] + grp.nq;
        nq_max = std::max(nq_max, grp.nq); nL_max = std::max(nL_max, grp.max_nL); lt_pad = std::max(lt_pad, (int)grp.dev.lt_pad);
    }
    if (q_first[n_grp] != n_q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": the query handle's launch groups do not add up to its queries");
    std::vector<uint8_t> has((size_t)n_q);
    for (int i = 0; i < n_q; ++i) has[(size_t)i] = q->status[(size_t)i] == AFIS_QUERY_OK;
    CascadeTables t;
    if (!build_cascade_tables((size_t)n_q, has.data(), (size_t)nk, n_grp, q_first.data(), kAdcPairsSegment, (size_t)ctx->cascade_pairs_per_launch, t) ||
        (int64_t)n_q * nk > 0x7fffffffLL || (int64_t)n_q * G > 0x7ffffff0LL)
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_q x keep or n_q x G exceeds what one call takes");
    const size_t total = t.total, n_pieces = t.pieces.size();
    const size_t P = std::min(total, (size_t)ctx->cascade_pairs_per_launch), Lp = (size_t)lt_pad;
    const size_t n_out = (size_t)n_q * (size_t)keep;
    const size_t kept_at = up256((size_t)n_q * 8), kscore_at = up256(kept_at + n_out * 8), parts_at = up256(kscore_at + n_out * 4), score_at = up256(parts_at + total * 16),
                 tab_at = up256(score_at + std::max<size_t>(total, 1) * 4), dev_at = up256(tab_at + t.tab_ints() * 4), rmv_at = up256(dev_at + t.dev.size() * 4),
                 rma_at = up256(rmv_at + P * Lp * 4), buf_bytes = rma_at + P * Lp * 4 + 16;
    // what returns through the pinned buffer: n_hits | kept | pair parts | the diagnostics rows; behind them the tables on their way up (pinned memory of the context,
    // so that an early return leaves nothing queued that reads memory of this call)
    const size_t pin_parts_at = up256(kept_at + n_out * 8), pin_diag_at = up256(pin_parts_at + total * 16), diag_bytes = std::max<size_t>(n_grp, 1) * kDiagWords * 8,
                 pin_dev_at = up256(pin_diag_at + diag_bytes), pin_bytes = pin_dev_at + t.dev.size() * 4;
    // ---- room first: every allocation precedes all device work and the first write into the caller's arrays
    const size_t n_cells = (size_t)n_q * (size_t)G, grp_pairs = (size_t)nq_max * (size_t)G;
    const size_t per_wg = minu_scratch_floats(nL_max, ctx->max_nR, ctx->s3_tie_order);
    int n_wg = 1024;
    while (n_wg > 64 && per_wg * 4 * n_wg > (8ull << 30)) n_wg /= 2;
    const size_t minu_slab_1 = graph_minutiae_slab_bytes(3 * (long long)grp_pairs);
    HIPCHK(ctx, ctx->scores.ensure(n_cells * 4));
    HIPCHK(ctx, ctx->elig_scores.ensure(n_cells * 4));
    HIPCHK(ctx, ctx->parts.ensure(n_cells * 16));
    HIPCHK(ctx, ctx->cands.ensure(grp_pairs * 3 * kTopMinu * sizeof(MinuCand)));
    HIPCHK(ctx, ctx->cand_n.ensure(grp_pairs * 3 * 4));
    HIPCHK(ctx, ctx->minu_fb.ensure(minu_fb_ints(grp_pairs * 3, (size_t)G) * 4));
    HIPCHK(ctx, ctx->minu_slab.ensure(minu_slab_1));
    HIPCHK(ctx, ctx->scratch.ensure(per_wg * 4 * (size_t)n_wg));
    HIPCHK(ctx, ctx->diag.ensure(diag_bytes));
    HIPCHK(ctx, ctx->casc_buf.ensure(buf_bytes));
    if (P > 0) HIPCHK(ctx, ctx->casc_slab.ensure(graph_texture_slab_bytes((long long)P)));
    HIPCHK(ctx, ensure_pin(ctx, pin_bytes));
    while (ctx->evpool.size() < n_grp * 10 + 2) { hipEvent_t e; HIPCHK(ctx, hipEventCreate(&e)); ctx->evpool.push_back(e); }
    EventSet ev;
    for (hipEvent_t& e : ev.e) HIPCHK(ctx, hipEventCreate(&e));
    if (status) for (int i = 0; i < n_q; ++i) status[i] = q->status[(size_t)i];

    uint8_t* const d = ctx->casc_buf.as<uint8_t>();
    uint8_t* const pin = (uint8_t*)ctx->h_pin;
    long long* const d_kept = (long long*)(d + kept_at);
    const int32_t* const d_dev = (const int32_t*)(d + dev_at);
    const int32_t* const d_q_slot = d_dev + t.q_slot_at;
    int32_t* const d_tab = (int32_t*)(d + tab_at);
    float* const d_pparts = (float*)(d + parts_at);
    float* const d_pscore = (float*)(d + score_at);
    // ---- stage 1: the minutiae scorers for every cell, group after group on the whole chip
    HIPCHK(ctx, hipMemsetAsync(ctx->diag.p, 0, diag_bytes, s));
    HIPCHK(ctx, hipEventRecord(ev.e[0], s));
    int q0 = 0;
    for (size_t gi = 0; gi < n_grp; ++gi) {
        QueryGroup& grp = q->groups[gi];
        const QueryDev& qd = grp.dev;
        hipEvent_t* gev = &ctx->evpool[gi * 10];
        unsigned long long* const diag_row = ctx->diag.as<unsigned long long>() + gi * kDiagWords;
        float* const grp_parts = ctx->parts.as<float>() + (size_t)q0 * (size_t)G * 4;
        const size_t wg_floats = minu_scratch_floats(grp.max_nL, ctx->max_nR, ctx->s3_tie_order);
        grp.overlapped = false;
        HIPCHK(ctx, hipEventRecord(gev[0], s));
        HIPCHK(ctx, launch_minu_cands(qd, ctx->gal, ctx->scratch.as<float>(), wg_floats, n_wg, ctx->minu_generic | (ctx->s3_tie_order << 1), ctx->cands.as<MinuCand>(), ctx->cand_n.as<int32_t>(),
                                      ctx->minu_fb.as<int32_t>(), grp.max_nL, ctx->max_nR, diag_row, s));
        HIPCHK(ctx, hipEventRecord(gev[1], s));
        HIPCHK(ctx, launch_graph_minutiae(qd, ctx->gal, ctx->cands.as<MinuCand>(), ctx->cand_n.as<int32_t>(), grp_parts, nullptr, nullptr, ctx->minu_slab.p, minu_slab_1, nullptr, nullptr,
                                          2 | (ctx->s89_tie_order << 8), s));
        HIPCHK(ctx, hipEventRecord(gev[2], s));
        HIPCHK(ctx, launch_fuse_stage1(qd, ctx->gal, grp_parts, ctx->scores.as<float>() + (size_t)q0 * (size_t)G, s));
        HIPCHK(ctx, hipEventRecord(gev[3], s));
        q0 += grp.nq;
    }
    HIPCHK(ctx, hipEventRecord(ev.e[1], s));
    // ---- selection: per query the nk best by m — rank_key descending, equal keys by ascending global index; every column is an entry
    HIPCHK(ctx, hipEventRecord(ev.e[2], s));
    HIPCHK(ctx, launch_rank_hits(ctx->scores.as<float>(), n_q, (int)G, nullptr, 0, nullptr, nullptr, (long long)base, kPosFloor, keep, (long long*)d, d_kept, (float*)(d + kscore_at), nullptr, s));
    HIPCHK(ctx, hipEventRecord(ev.e[3], s));
    // ---- stage 2: the texture scorer for the kept cells
    memcpy(pin + pin_dev_at, t.dev.data(), t.dev.size() * 4);
    HIPCHK(ctx, hipMemcpyAsync(d + dev_at, pin + pin_dev_at, t.dev.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipEventRecord(ev.e[4], s));
    HIPCHK(ctx, hipMemsetAsync(ctx->elig_scores.p, 0xff, n_cells * 4, s));
    HIPCHK(ctx, launch_cascade_gather(n_q, (int)G, keep, nk, (long long)base, d_kept, d_q_slot, d_dev + t.piece_first_at, (int)n_pieces, d_dev + t.piece_q0_at, ctx->parts.as<float>(),
                                      d_tab, d_pparts, s));
    for (size_t i = 0; i < n_pieces; ++i) {
        const CascadePiece& pc = t.pieces[i];
        const QueryDev& qd = q->groups[pc.group].dev;
        const size_t in_chunk = pc.first - pc.chunk * (size_t)ctx->cascade_pairs_per_launch;      // the piece's place in its chunk's row maxima: in_chunk + n <= P, and the group's stride qd.lt_pad <= Lp
        const int32_t* const p_tab = d_tab + 2 * pc.first + i;
        float* const rm_val = (float*)(d + rmv_at) + in_chunk * Lp;
        int32_t* const rm_arg = (int32_t*)(d + rma_at) + in_chunk * Lp;
        float* const p_parts = d_pparts + pc.first * 4;
        HIPCHK(ctx, launch_adc_pairs(qd, ctx->gal, ctx->codewords.as<float>(), p_tab, d_dev + t.seg_at + 2 * pc.seg_first, (int)pc.n_seg, rm_val, rm_arg, s));
        HIPCHK(ctx, launch_graph_texture_pairs(qd, ctx->gal, p_tab, (int)pc.n, ctx->table.as<float>(), rm_val, rm_arg, p_parts, ctx->casc_slab.p, ctx->casc_slab.bytes, ctx->s89_tie_order, s));
        HIPCHK(ctx, launch_fuse_pairs(qd, ctx->gal, p_tab, (int)pc.n, p_parts, d_pscore + pc.first, s));
    }
    HIPCHK(ctx, launch_cascade_scatter(n_q, (int)G, keep, nk, (long long)base, d_kept, d_q_slot, d_pscore, ctx->elig_scores.as<float>(), s));
    HIPCHK(ctx, hipEventRecord(ev.e[5], s));
    // ---- what returns, through the pinned buffer; the one wait
    HIPCHK(ctx, hipMemcpyAsync(pin, d, kept_at + n_out * 8, hipMemcpyDeviceToHost, s));
    if (total > 0) HIPCHK(ctx, hipMemcpyAsync(pin + pin_parts_at, d + parts_at, total * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(pin + pin_diag_at, ctx->diag.p, diag_bytes, hipMemcpyDeviceToHost, s));
    AFISCHK(wait_streams(ctx, {s}, who));
    // ---- times: the three options, each from its own pair of events; afis_timing reports stage 1
    afis_timing tm = {};
    {
        float ms[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) HIPCHK(ctx, hipEventElapsedTime(&ms[k], ev.e[2 * k], ev.e[2 * k + 1]));
        ctx->cascade_stage1_us = (int64_t)((double)ms[0] * 1e3); ctx->cascade_select_us = (int64_t)((double)ms[1] * 1e3); ctx->cascade_stage2_us = (int64_t)((double)ms[2] * 1e3);
        ctx->cascade_kept_pairs = (int64_t)total;
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
            float t_c = 0, t_g = 0, t_f = 0;
            HIPCHK(ctx, hipEventElapsedTime(&t_c, gev[0], gev[1])); HIPCHK(ctx, hipEventElapsedTime(&t_g, gev[1], gev[2])); HIPCHK(ctx, hipEventElapsedTime(&t_f, gev[2], gev[3]));
            tm.cands_ms += t_c; tm.minu_graph_ms += t_g; tm.minu_ms += t_c + t_g; tm.fuse_ms += t_f; tm.total_ms += t_c + t_g + t_f;
        }
        tm.pairs = (int64_t)n_cells; tm.launch_groups = (int32_t)n_grp;
    }
    // ---- into the caller's arrays
    const long long* const h_hits = (const long long*)pin;
    for (int i = 0; i < n_q; ++i) {
        const size_t o = (size_t)i * (size_t)keep;
        if (n_kept) n_kept[i] = std::min<int64_t>(h_hits[i], keep);
        if (kept_idx) memcpy(kept_idx + o, pin + kept_at + o * 8, (size_t)keep * 8);
        if (kept_parts) {
            memset(kept_parts + o * 4, 0, (size_t)keep * 16);                  // +0.0f: the padding, and the cells of a latent-empty query (no scorer ran)
            if (has[(size_t)i]) memcpy(kept_parts + o * 4, pin + pin_parts_at + t.q_slot[(size_t)i] * 16, (size_t)nk * 16);
        }
    }
    std::swap(ctx->scores, ctx->elig_scores);                               // the combined matrix is the last search's from here on
    ctx->timing = tm;
    return AFIS_OK;
}

}  // namespace

extern "C" {

int afis_search_cascade(afis_ctx* ctx, afis_queries* q, int keep, float* scores, int32_t* status, int64_t* n_kept, int64_t* kept_idx, float* kept_parts)
{
    const char* const who = "afis_search_cascade";
    if (!ctx || !q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    clear_cascade_options(ctx);
    ctx->last_search.valid = false;
    if (keep < 1 || keep > AFIS_HITS_MAX) return fail(ctx, AFIS_EINVAL, std::string(who) + ": keep must be 1 .. AFIS_HITS_MAX, the longest list the selection makes");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    // afis_search_resident's rules for the handle: a reserved one while the shard fits, any other only for the shard it was uploaded against
    if (q->max_templates > 0) {
        if ((int64_t)ctx->gal.G > q->max_templates)
            return fail(ctx, AFIS_EINVAL, std::string(who) + ": the resident shard holds " + std::to_string((long long)ctx->gal.G) + " templates, these queries were uploaded for at most " +
                                              std::to_string((long long)q->max_templates) + " (afis_queries_upload_reserved)");
    } else if (q->gallery_epoch != ctx->gallery_epoch)
        return fail_edited(ctx, who, "these queries were uploaded; free the handle and upload them again");
    const int64_t G = ctx->gal.G;
    const int n_q = q->n_q;
    if (n_q == 0 || G == 0) {                                               // nothing to score: as afis_search_resident answers it; no list holds anything
        const int rc = search_shard(ctx, *ctx, nullptr, q, scores, nullptr, status, 0, nullptr, nullptr);
        if (rc != AFIS_OK) { ctx->last_search.valid = false; return rc; }
        for (int i = 0; i < n_q; ++i) {
            if (n_kept) n_kept[i] = 0;
            for (int r = 0; r < keep; ++r) {
                if (kept_idx) kept_idx[(size_t)i * keep + r] = -1;
                if (kept_parts) for (int c = 0; c < 4; ++c) kept_parts[((size_t)i * keep + r) * 4 + c] = 0.0f;
            }
        }
        return AFIS_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx));
    int rc = cascade(ctx, who, q, keep, status, n_kept, kept_idx, kept_parts);
    if (rc == AFIS_OK && scores) {                                          // the device is idle: a plain copy, as at the end of a search
        const hipError_t e = hipMemcpy(scores, ctx->scores.p, (size_t)n_q * (size_t)G * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, AFIS_EDEVICE, std::string(who) + ": the scores: " + hipGetErrorString(e));
    }
    if (rc != AFIS_OK) {                                                    // the call holds nothing it allocated; after a timeout the device may still use it: the bounded wait first
        const std::string keep_err = ctx->err;
        (void)quiesce(ctx, who);
        ctx->err = keep_err;
        ctx->casc_buf.release(); ctx->casc_slab.release(); ctx->elig_scores.release();
        clear_cascade_options(ctx);
        ctx->timing = afis_timing{};
    }
    ctx->last_search = rc == AFIS_OK ? LastSearch{true, n_q, G, nullptr, ctx->gallery_epoch} : LastSearch{};
    return rc;
}

}  // extern "C"
