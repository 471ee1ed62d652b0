// afis_pairs.cpp — pair scoring of the C ABI (include/afis_matcher.h): afis_score_pairs gives the fused score and the four parts of a LIST of (latent, rolled print) pairs —
// one verification, N labelled mates, the candidates of per-latent lists — bit for bit the cells afis_search would have written for them, without scoring a matrix.  The
// latents are those of a query handle, already resident; the prints are those of the resident shard itself.  The driver has afis_corr.cpp's shape: the pairs that need the
// device are cut into chunks of option score_pairs_per_launch pairs; per chunk ONE upload of the tables (pair_tables.h: the chunk's pairs sorted by launch group, then by
// latent, and the work list of the ADC kernel), then for every launch group of the handle that has pairs in the chunk the any-shape candidate kernel and the minutiae list
// kernel in their pair-table forms (minu.hip, graph.hip; the survivors go to a scratch area nobody reads), the exact texture row maxima over the pair table (adc_pairs.hip),
// the texture list kernel in its pair-table form (graph_pairs.hip) and the fusion (minu.hip::fuse_cell, the search's own expression), and ONE copy back of parts | scores
// through the pinned buffer.  What this shard does not hold (NOT_COVERED) and what the reference does not score (-1: a latent-empty query, an empty or removed print — the
// search leaves their four parts at +0.0f: no scorer finds anything to run on) is settled here from the host's copies of the shard's tables.  Every other pair goes to the
// device, a print without minutiae or a latent without any of the three selected templates too: the pair forms of the minutiae kernels write an empty list and a +0.0f part
// for a scorer the reference does not run (k_minu_cands: nL <= 0 || nR <= 0; k_graph_minutiae: num <= 0), and such a pair still has a texture score.
// The last search's matrix is neither written nor invalidated: the call uses buffers of its own, the scratch and the slab of the minutiae stage, which nothing outlives, and
// the list counters, which every launcher resets.
// afis_score_print_pairs (afis_print_pairs.cpp) drives the same function over temporary handles of prints' views, with the fold of a print pair as the fuse step.
#include "afis_ctx.h"
#include "pair_tables.h"

#include <limits>

using namespace afis;

static_assert(kScorePairsPerLaunch == AFIS_SCORE_PAIRS_PER_LAUNCH, "option score_pairs_per_launch's default is the header's");

namespace afis {

// fold == NULL: afis_score_pairs — the fusion is fuse_cell, parts is [n_pairs][4].  fold != NULL: afis_score_print_pairs (afis_print_pairs.cpp) — the handle's queries are
// prints' views, the fusion is the weighted fold of a print pair (template_fold.hip::k_fold_print_pairs) with the pair's two weights, uploaded in slot order beside the
// chunk's tables, and parts is [n_pairs][2]: the minutiae template's part and the texture template's, +0.0f where the pair's weight is zero.
int score_pairs(afis_ctx* ctx, const char* who, afis_queries* q, int64_t n_pairs, const int32_t* query, const int64_t* idx, int32_t* status, float* score, float* parts,
                const PrintPairWeights* fold)
{
    const size_t part_w = fold ? 2 : 4;                                    // floats of parts per pair in the caller's array
    const std::string w(who);
    const std::vector<QueryGroup>& groups = q->groups;
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    const int n_q = q->n_q;
    ctx->score_pairs_us = 0;
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
    // ---- the pairs that need the device: a covered print that is not empty and a latent the reference scores
    std::vector<int64_t> dev;                                              // the caller's pair numbers, in the caller's order
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int64_t t = idx[i] - base;
        if (t < 0 || t >= G || q->status[(size_t)query[i]] != AFIS_QUERY_OK || ctx->res_empty[(size_t)t]) continue;
        dev.push_back(i);
    }
    // ---- room first: every allocation precedes all device work and the first write into the caller's arrays
    const size_t P = (size_t)std::min<int64_t>((int64_t)dev.size(), ctx->score_pairs_per_launch);
    const size_t Lp = (size_t)lt_pad;
    const size_t cands_at = 0, corr_at = up256(cands_at + P * 3 * kTopMinu * sizeof(MinuCand)), corr_n_at = up256(corr_at + P * 3 * kTopMinu * sizeof(short4)), cand_n_at = up256(corr_n_at + P * 3 * 4),
                 rmv_at = up256(cand_n_at + P * 3 * 4), rma_at = up256(rmv_at + P * Lp * 4), parts_at = up256(rma_at + P * Lp * 4), score_at = parts_at + P * 16, tab_at = up256(score_at + P * 4),
                 tab_ints = 4 * P + n_grp, w_at = (tab_ints + 1) / 2 * 2,           // (the weights of a print pair: [P][2] floats behind the tables, 8-byte aligned)
                 all_ints = fold ? w_at + 2 * P : tab_ints, buf_bytes = tab_at + all_ints * 4;
    const size_t back_bytes = P * 20;                                     // parts | scores: what returns, through the pinned buffer
    const size_t pin_tab_at = up256(back_bytes), pin_bytes = pin_tab_at + all_ints * 4;   // ... behind them a chunk's tables on their way up: pinned memory of the context, so that
                                                                          // an early return leaves nothing queued that reads memory of this call
    static_assert(sizeof(MinuCand) == 8 && sizeof(short4) == 8, "5.8 KB per pair");
    size_t per_wg = 0; int n_wg = 1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (P > 0) {
        // the candidate kernel's grid, as afis_correspondences_pairs sizes it: what fits the chip at once, within the scratch the context can afford
        per_wg = minu_scratch_floats(max_nL, ctx->max_nR, ctx->s3_tie_order);
        const size_t afford = std::max<size_t>(ctx->scratch.bytes, (size_t)1 << 30);
        const int per_cu = (int)std::max<size_t>(1, (size_t)(160 << 10) / minu_cands_lds_bytes(ctx->s3_tie_order));
        n_wg = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(ctx->n_cus, 1) * per_cu, afford / (per_wg * 4)));
        n_wg = (int)std::min<size_t>((size_t)n_wg, 3 * P);
        HIPCHK(ctx, ctx->scratch.ensure(per_wg * 4 * (size_t)n_wg));
        HIPCHK(ctx, ctx->minu_slab.ensure(graph_minutiae_slab_bytes(3 * (long long)P)));
        HIPCHK(ctx, ctx->pair_tex_slab.ensure(graph_texture_slab_bytes((long long)P)));
        HIPCHK(ctx, ctx->pair_buf.ensure(buf_bytes));
        HIPCHK(ctx, ensure_pin(ctx, pin_bytes));
    }
    // ---- what holds without the device: NOT_COVERED outside the shard, -1 where the reference runs no scorer (the search's parts of such a cell are +0.0f)
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int64_t t = idx[i] - base;
        const bool covered = t >= 0 && t < G;
        status[i] = covered ? AFIS_PAIR_OK : AFIS_PAIR_NOT_COVERED;
        score[i] = covered ? -1.0f : -std::numeric_limits<float>::infinity();
        if (parts) for (size_t s = 0; s < part_w; ++s) parts[(size_t)i * part_w + s] = 0.0f;
    }
    if (P == 0) return AFIS_OK;

    hipStream_t s = ctx->stream;
    uint8_t* const d = ctx->pair_buf.as<uint8_t>();
    const uint8_t* const pin = (const uint8_t*)ctx->h_pin;
    int32_t* const tab = (int32_t*)((uint8_t*)ctx->h_pin + pin_tab_at);   // one chunk's tables: the groups' pair tables, then the work list (rewritten only after the chunk's wait)
    PairChunkTables t;
    std::vector<int32_t> c_query(P), c_tmpl(P);
    for (size_t c0 = 0; c0 < dev.size(); c0 += P) {
        const size_t m = std::min(P, dev.size() - c0);
        for (size_t k = 0; k < m; ++k) { c_query[k] = query[dev[c0 + k]]; c_tmpl[k] = (int32_t)(idx[dev[c0 + k]] - base); }
        int32_t* const seg = tab + 2 * m + n_grp;
        const size_t n_seg = build_pair_tables(m, c_query.data(), c_tmpl.data(), n_grp, q_first.data(), kAdcPairsSegment, tab, seg, t);
        Events ev{2};
        for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
        HIPCHK(ctx, hipMemcpyAsync(d + tab_at, tab, (2 * m + n_grp + 2 * n_seg) * 4, hipMemcpyHostToDevice, s));
        if (fold) {                                                         // the slots' weights, in slot order
            float* const w = reinterpret_cast<float*>(tab + w_at);
            for (size_t slot = 0; slot < m; ++slot) {
                const int64_t i = dev[c0 + (size_t)t.slot_of[slot]];
                w[2 * slot] = fold->w_minu[i]; w[2 * slot + 1] = fold->w_tex[i];
            }
            HIPCHK(ctx, hipMemcpyAsync(d + tab_at + w_at * 4, w, m * 8, hipMemcpyHostToDevice, s));
        }
        HIPCHK(ctx, hipEventRecord(ev[0], s));
        for (size_t gi = 0; gi < n_grp; ++gi) {
            const size_t b = t.first[gi]; const int n = (int)(t.first[gi + 1] - b);
            if (n == 0) continue;
            const QueryDev& qd = groups[gi].dev;
            const int32_t* d_tab = (const int32_t*)(d + tab_at) + 2 * b + gi;
            const int32_t* d_seg = (const int32_t*)(d + tab_at) + 2 * m + n_grp + 2 * t.seg_first[gi];
            MinuCand* cands = (MinuCand*)(d + cands_at) + b * 3 * kTopMinu;
            int32_t* cand_n = (int32_t*)(d + cand_n_at) + b * 3;
            float* g_parts = (float*)(d + parts_at) + b * 4;
            float* rm_val = (float*)(d + rmv_at) + b * Lp;                // (the group's own stride q.lt_pad <= Lp: its n pairs stay inside n * Lp)
            int32_t* rm_arg = (int32_t*)(d + rma_at) + b * Lp;
            HIPCHK(ctx, launch_minu_cands_pairs(qd, ctx->gal, ctx->scratch.as<float>(), per_wg, n_wg, ctx->s3_tie_order, d_tab, n, cands, cand_n, s));
            HIPCHK(ctx, launch_graph_minutiae_pairs(qd, ctx->gal, d_tab, n, cands, cand_n, g_parts, (short4*)(d + corr_at) + b * 3 * kTopMinu, (int32_t*)(d + corr_n_at) + b * 3,
                                                    ctx->minu_slab.p, ctx->minu_slab.bytes, ctx->s89_tie_order, s));
            HIPCHK(ctx, launch_adc_pairs(qd, ctx->gal, ctx->codewords.as<float>(), d_tab, d_seg, (int)(t.seg_first[gi + 1] - t.seg_first[gi]), rm_val, rm_arg, s));
            HIPCHK(ctx, launch_graph_texture_pairs(qd, ctx->gal, d_tab, n, ctx->table.as<float>(), rm_val, rm_arg, g_parts, ctx->pair_tex_slab.p, ctx->pair_tex_slab.bytes, ctx->s89_tie_order, s));
            if (fold) HIPCHK(ctx, launch_fold_print_pairs(g_parts, (const float*)(d + tab_at + w_at * 4) + 2 * b, (size_t)n, (float*)(d + score_at) + b, s));
            else HIPCHK(ctx, launch_fuse_pairs(qd, ctx->gal, d_tab, n, g_parts, (float*)(d + score_at) + b, s));
        }
        HIPCHK(ctx, hipEventRecord(ev[1], s));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d + parts_at, back_bytes, hipMemcpyDeviceToHost, s));
        int64_t us = 0;
        AFISCHK(wait_elapsed(ctx, who, ev, &us));
        ctx->score_pairs_us += us;
        // ---- into the caller's order
        for (size_t slot = 0; slot < m; ++slot) {
            const int64_t i = dev[c0 + (size_t)t.slot_of[slot]];
            memcpy(score + i, pin + P * 16 + slot * 4, 4);
            if (parts && !fold) memcpy(parts + i * 4, pin + slot * 16, 16);
            if (parts && fold) { memcpy(parts + i * 2, pin + slot * 16, 4); memcpy(parts + i * 2 + 1, pin + slot * 16 + 12, 4); }
        }
    }
    return AFIS_OK;
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
