// afis_pairs.cpp — the pair-list calls' one host driver (PairCall, afis_ctx.h: afis_correspondences_pairs and afis_correspondences in afis_corr.cpp run through it, and
// through those two the pair calls for resident prints, afis_print_pairs.cpp), the texture stage of a pair table (queue_texture_pairs: the driver's score form and stage 2 of
// every cascade queue it) and pair scoring of the C ABI (include/afis_matcher.h): afis_score_pairs gives the fused score and the four parts of a LIST of (latent, rolled
// print) pairs — one verification, N labelled mates, the candidates of per-latent lists — bit for bit the cells afis_search would have written for them, without scoring a
// matrix.  The latents are those of a query handle, already resident; the prints are those of the resident shard itself.  The pairs that need the device are cut into
// chunks of the call's option (corr_pairs_per_launch, score_pairs_per_launch); per chunk ONE upload of the tables (pair_tables.h: the chunk's pairs sorted by launch group,
// then by latent, and for the score form the work list of the ADC kernel), then for every launch group of the handle that has pairs in the chunk the any-shape candidate
// kernel and the minutiae list kernel in their pair-table forms (minu.hip, graph.hip: task 3 p + s = selected template s of pair p, compact slots) and the caller's stage —
// for a score the exact texture row maxima over the pair table (adc_pairs.hip), the texture list kernel in its pair-table form (graph_pairs.hip) and the fusion
// (minu.hip::fuse_cell, the search's own expression) —, and ONE copy back through the pinned buffer.  Nothing is read back per pair.
// The score call: what this shard does not hold (NOT_COVERED) and what the reference does not score (-1: a latent-empty query, an empty or removed print — the search
// leaves their four parts at +0.0f: no scorer finds anything to run on) is settled from the host's copies of the shard's tables.  Every other pair goes to the device, a
// print without minutiae or a latent without any of the three selected templates too: the pair forms of the minutiae kernels write an empty list and a +0.0f part for a
// scorer the reference does not run (k_minu_cands: nL <= 0 || nR <= 0; k_graph_minutiae: num <= 0), and such a pair still has a texture score; its survivors go to an area
// nobody reads.
// The last search's matrix is neither written nor invalidated: a pair call uses a buffer of its own, the scratch and the slab of the minutiae stage, which nothing outlives,
// and the list counters, which every launcher resets.
// afis_score_print_pairs (afis_print_pairs.cpp) drives score_pairs over temporary handles of prints' views, with the fold of a print pair as the fuse step.
// The evidence form (afis_evidence.cpp: afis_texture_correspondences_pairs, afis_pair_alignments) is the score form without the fusion: the same areas and slab, the texture
// list kernel's tap [P][200] | [P] behind the weights and, behind that, what pair_evidence.hip's kernel makes of a launch group's lists — the one run that returns.
#include "afis_ctx.h"
#include "pair_tables.h"

#include <limits>

using namespace afis;

static_assert(kScorePairsPerLaunch == AFIS_SCORE_PAIRS_PER_LAUNCH, "option score_pairs_per_launch's default is the header's");

namespace afis {

int queue_texture_pairs(afis_ctx* ctx, const GalleryDev& gal, const QueryDev& qd, const int32_t* pair_tab, int n, const int32_t* seg, int n_seg, float* rm_val, int32_t* rm_arg,
                        float* parts, const DevBuf& slab, float* score_or_null, hipStream_t stream, MinuCand* tap_out, int32_t* tap_n)
{
    HIPCHK(ctx, launch_adc_pairs(qd, gal, ctx->codewords.as<float>(), pair_tab, seg, n_seg, rm_val, rm_arg, stream));
    HIPCHK(ctx, launch_graph_texture_pairs(qd, gal, pair_tab, n, ctx->table.as<float>(), rm_val, rm_arg, parts, slab.p, slab.bytes, ctx->s89_tie_order, tap_out, tap_n, stream));
    if (score_or_null) HIPCHK(ctx, launch_fuse_pairs(qd, gal, pair_tab, n, parts, score_or_null, stream));
    return AFIS_OK;
}

int PairCall::run()
{
    const std::string w(who);
    *us = 0;
    for (int64_t i = 0; i < n_pairs; ++i)
        if (query[i] < 0 || query[i] >= n_q) return fail(ctx, AFIS_EINVAL, w + ": a pair's query is outside 0 .. n_q - 1");
    const size_t n_grp = groups.size();
    std::vector<int32_t> q_first(n_grp + 1, 0);
    int max_nL = 1, lt_pad = 0;
    for (size_t gi = 0; gi < n_grp; ++gi) {
        q_first[gi + 1] = q_first[gi] + groups[gi].nq;
        max_nL = std::max(max_nL, groups[gi].max_nL); lt_pad = std::max(lt_pad, (int)groups[gi].dev.lt_pad);
    }
    if (q_first[n_grp] != n_q) return fail(ctx, AFIS_EINVAL, w + ": the query handle's launch groups do not add up to its queries");
    std::vector<int64_t> dev;                                              // the caller's pair numbers of the pairs that need the device, in the caller's order
    for (int64_t i = 0; i < n_pairs; ++i) if (needs_device(i)) dev.push_back(i);
    // ---- room first: every allocation precedes all device work and the first write into the caller's arrays
    const size_t P = (size_t)std::min<int64_t>((int64_t)dev.size(), per_launch);
    const size_t Lp = texture ? (size_t)lt_pad : 0, tab_ints = 2 * P + n_grp + (texture ? 2 * P : 0), w_bytes = weights ? P * 8 : 0;
    static_assert(sizeof(MinuCand) == 8 && sizeof(short4) == 8, "5.8 KB per pair");
    const size_t cands_at = 0, cand_n_at = up256(cands_at + P * 3 * kTopMinu * sizeof(MinuCand)), rmv_at = up256(cand_n_at + P * 3 * 4), rma_at = up256(rmv_at + P * Lp * 4),
                 corr_at = up256(rma_at + P * Lp * 4), corr_n_at = up256(corr_at + P * 3 * kTopMinu * sizeof(short4)), parts_at = up256(corr_n_at + P * 3 * 4),
                 score_at = up256(parts_at + P * 16), tab_at = up256(score_at + (texture ? P * 4 : 0)), w_at = up256(tab_at + tab_ints * 4);
    // the evidence form: the tap, then the call's outputs in one run (afis_ctx.h has the areas)
    static_assert(sizeof(CorrMoments) == 72 && sizeof(short2) == 4, "288 bytes of moments, 3 208 of texture export per pair");
    const bool ex = evidence == kPairTexExport, mo = evidence == kPairMoments;
    const size_t tap_at = up256(w_at + w_bytes), tap_n_at = up256(tap_at + (evidence ? P * kTopTex * sizeof(MinuCand) : 0)), ev_at = up256(tap_n_at + (evidence ? P * 4 : 0)),
                 ex_part_at = up256(ev_at + (ex ? P * 4 : 0)), ex_xy_at = up256(ex_part_at + (ex ? P * 4 : 0)), ex_pt_at = up256(ex_xy_at + (ex ? P * kTopTex * sizeof(short4) : 0)),
                 ex_sim_at = up256(ex_pt_at + (ex ? P * kTopTex * sizeof(short2) : 0)), ev_end = ex_sim_at + (ex ? P * kTopTex * 4 : 0) + (mo ? P * 4 * sizeof(CorrMoments) : 0),
                 buf_bytes = evidence ? ev_end : w_at + w_bytes;
    const size_t back_at = evidence ? ev_at : texture ? parts_at : corr_at, back_bytes = (evidence ? ev_end : texture ? score_at + P * 4 : parts_at + P * 16) - back_at;      // what returns, through the pinned buffer
    const size_t pin_tab_at = up256(back_bytes), pin_w_at = up256(pin_tab_at + tab_ints * 4), pin_bytes = pin_w_at + w_bytes;           // ... behind it the chunk's tables and weights on their way up
    MinuGrid grid{0, 1};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (P > 0) {
        grid = minu_cands_pairs_grid(max_nL, ctx->max_nR, ctx->s3_tie_order, ctx->n_cus, minu_cands_lds_bytes(ctx->s3_tie_order), ctx->scratch.bytes, P);
        HIPCHK(ctx, ctx->scratch.ensure(grid.bytes()));
        HIPCHK(ctx, ctx->minu_slab.ensure(graph_minutiae_slab_bytes(3 * (long long)P)));
        if (texture) HIPCHK(ctx, ctx->pair_tex_slab.ensure(graph_texture_slab_bytes((long long)P)));
        HIPCHK(ctx, ctx->pair_buf.ensure(buf_bytes));
        HIPCHK(ctx, ensure_pin(ctx, pin_bytes));
    }
    defaults();
    if (P == 0) return AFIS_OK;

    hipStream_t s = ctx->stream;
    const int64_t base = ctx->index_base;
    uint8_t* const d = ctx->pair_buf.as<uint8_t>();
    uint8_t* const pin = (uint8_t*)ctx->h_pin;
    int32_t* const tab = (int32_t*)(pin + pin_tab_at);                     // one chunk's tables: the groups' pair tables, then the work list (rewritten only after the chunk's wait)
    const int32_t* const d_tabs = (const int32_t*)(d + tab_at);
    PairBack back{texture ? nullptr : (const short4*)pin, texture ? nullptr : (const int32_t*)(pin + corr_n_at - back_at), evidence ? nullptr : (const float*)(pin + parts_at - back_at),
                  texture && !evidence ? (const float*)(pin + score_at - back_at) : nullptr};
    if (ex) { back.ex_n = (const int32_t*)pin; back.ex_part = (const float*)(pin + ex_part_at - back_at); back.ex_xy = (const short4*)(pin + ex_xy_at - back_at);
              back.ex_pt = (const short2*)(pin + ex_pt_at - back_at); back.ex_sim = (const float*)(pin + ex_sim_at - back_at); }
    if (mo) back.mom = (const CorrMoments*)pin;
    PairChunkTables t;
    std::vector<int32_t> c_query(P), c_tmpl(P);
    for (size_t c0 = 0; c0 < dev.size(); c0 += P) {
        const size_t m = std::min(P, dev.size() - c0);
        for (size_t k = 0; k < m; ++k) { c_query[k] = query[dev[c0 + k]]; c_tmpl[k] = (int32_t)(idx[dev[c0 + k]] - base); }
        const size_t n_seg = build_pair_tables(m, c_query.data(), c_tmpl.data(), n_grp, q_first.data(), kAdcPairsSegment, tab, texture ? tab + 2 * m + n_grp : nullptr, t);
        Events ev{2};
        for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
        HIPCHK(ctx, hipMemcpyAsync(d + tab_at, tab, (2 * m + n_grp + 2 * n_seg) * 4, hipMemcpyHostToDevice, s));
        if (weights) {                                                      // the slots' weights, in slot order
            float* const wt = (float*)(pin + pin_w_at);
            for (size_t slot = 0; slot < m; ++slot) {
                const int64_t i = dev[c0 + (size_t)t.slot_of[slot]];
                wt[2 * slot] = weights->w_minu[i]; wt[2 * slot + 1] = weights->w_tex[i];
            }
            HIPCHK(ctx, hipMemcpyAsync(d + w_at, wt, m * 8, hipMemcpyHostToDevice, s));
        }
        HIPCHK(ctx, hipEventRecord(ev[0], s));
        for (size_t gi = 0; gi < n_grp; ++gi) {
            const size_t b = t.first[gi]; const int n = (int)(t.first[gi + 1] - b);
            if (n == 0) continue;
            // (the row maxima at the group's own stride qd.lt_pad <= Lp: its n pairs stay inside n * Lp)
            PairGroup g{groups[gi].dev, d_tabs + 2 * b + gi, n, texture ? d_tabs + 2 * m + n_grp + 2 * t.seg_first[gi] : nullptr, (int)(t.seg_first[gi + 1] - t.seg_first[gi]),
                              (float*)(d + parts_at) + b * 4, texture ? (float*)(d + rmv_at) + b * Lp : nullptr, texture ? (int32_t*)(d + rma_at) + b * Lp : nullptr,
                              texture ? (float*)(d + score_at) + b : nullptr, weights ? (const float*)(d + w_at) + 2 * b : nullptr, PairEvidence{}};
            MinuCand* cands = (MinuCand*)(d + cands_at) + b * 3 * kTopMinu;
            int32_t* cand_n = (int32_t*)(d + cand_n_at) + b * 3;
            short4* const corr = (short4*)(d + corr_at) + b * 3 * kTopMinu;
            int32_t* const corr_n = (int32_t*)(d + corr_n_at) + b * 3;
            if (evidence) g.ev = PairEvidence{corr, corr_n, (MinuCand*)(d + tap_at) + b * kTopTex, (int32_t*)(d + tap_n_at) + b, g.parts, mo ? (CorrMoments*)(d + ev_at) + b * 4 : nullptr,
                                              ex ? (int32_t*)(d + ev_at) + b : nullptr, ex ? (float*)(d + ex_part_at) + b : nullptr, ex ? (short4*)(d + ex_xy_at) + b * kTopTex : nullptr,
                                              ex ? (short2*)(d + ex_pt_at) + b * kTopTex : nullptr, ex ? (float*)(d + ex_sim_at) + b * kTopTex : nullptr};
            HIPCHK(ctx, launch_minu_cands_pairs(g.qd, ctx->gal, ctx->scratch.as<float>(), grid.wg_floats, grid.n_wg, ctx->s3_tie_order, g.tab, n, cands, cand_n, s));
            HIPCHK(ctx, launch_graph_minutiae_pairs(g.qd, ctx->gal, g.tab, n, cands, cand_n, g.parts, corr, corr_n, ctx->minu_slab.p, ctx->minu_slab.bytes, ctx->s89_tie_order, s));
            if (stage) AFISCHK(stage(g));
        }
        HIPCHK(ctx, hipEventRecord(ev[1], s));
        HIPCHK(ctx, hipMemcpyAsync(pin, d + back_at, back_bytes, hipMemcpyDeviceToHost, s));
        int64_t chunk_us = 0;
        AFISCHK(wait_elapsed(ctx, who, ev, &chunk_us));
        *us += chunk_us;
        for (size_t slot = 0; slot < m; ++slot) take(dev[c0 + (size_t)t.slot_of[slot]], slot, back);      // into the caller's order
    }
    return AFIS_OK;
}

// fold == NULL: afis_score_pairs — the fusion is fuse_cell, parts is [n_pairs][4].  fold != NULL: afis_score_print_pairs (afis_print_pairs.cpp) — the handle's queries are
// prints' views, the fusion is the weighted fold of a print pair (template_fold.hip::k_fold_print_pairs) with the pair's two weights, uploaded in slot order beside the
// chunk's tables, and parts is [n_pairs][2]: the minutiae template's part and the texture template's, +0.0f where the pair's weight is zero.
int score_pairs(afis_ctx* ctx, const char* who, afis_queries* q, int64_t n_pairs, const int32_t* query, const int64_t* idx, int32_t* status, float* score, float* parts,
                const PrintPairWeights* fold)
{
    const size_t part_w = fold ? 2 : 4;                                    // floats of parts per pair in the caller's array
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    PairCall c{ctx, who, q->groups, q->n_q, n_pairs, query, idx, ctx->score_pairs_per_launch, &ctx->score_pairs_us, true, fold};
    // a covered print that is not empty and a latent the reference scores
    c.needs_device = [&](int64_t i) { const int64_t t = idx[i] - base; return t >= 0 && t < G && q->status[(size_t)query[i]] == AFIS_QUERY_OK && !ctx->res_empty[(size_t)t]; };
    // NOT_COVERED outside the shard, -1 where the reference runs no scorer (the search's parts of such a cell are +0.0f)
    c.defaults = [&] {
        for (int64_t i = 0; i < n_pairs; ++i) {
            const int64_t t = idx[i] - base;
            const bool covered = t >= 0 && t < G;
            status[i] = covered ? AFIS_PAIR_OK : AFIS_PAIR_NOT_COVERED;
            score[i] = covered ? -1.0f : -std::numeric_limits<float>::infinity();
            if (parts) for (size_t s = 0; s < part_w; ++s) parts[(size_t)i * part_w + s] = 0.0f;
        }
    };
    c.stage = [&](const PairGroup& g) -> int {
        AFISCHK(queue_texture_pairs(ctx, ctx->gal, g.qd, g.tab, g.n, g.seg, g.n_seg, g.rm_val, g.rm_arg, g.parts, ctx->pair_tex_slab, fold ? nullptr : g.score, ctx->stream));
        if (fold) HIPCHK(ctx, launch_fold_print_pairs(g.parts, g.weights, (size_t)g.n, g.score, ctx->stream));
        return AFIS_OK;
    };
    c.take = [&](int64_t i, size_t slot, const PairBack& b) {
        score[i] = b.score[slot];
        if (parts && !fold) memcpy(parts + i * 4, b.parts + slot * 4, 16);
        if (parts && fold) { parts[i * 2] = b.parts[slot * 4]; parts[i * 2 + 1] = b.parts[slot * 4 + 3]; }
    };
    return c.run();
}

}  // namespace afis

extern "C" {

int afis_score_pairs(afis_ctx* ctx, afis_queries* q, int64_t n_pairs, const int32_t* query, const int64_t* idx, int32_t* status, float* score, float* parts)
{
    const char* const who = "afis_score_pairs";
    if (!ctx || !q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    if (n_pairs < 0 || (n_pairs > 0 && !(query && idx && status && score))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_pairs must be >= 0 and every pair array but parts given");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    ctx->score_pairs_us = 0;
    if (n_pairs == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));                                   // the last search's matrix stays rankable
    return score_pairs(ctx, who, q, n_pairs, query, idx, status, score, parts, nullptr);
}

}  // extern "C"
