// afis_corr.cpp — correspondence export of the C ABI (include/afis_matcher.h): afis_correspondences_pairs gives the surviving minutiae correspondences (matcher.cpp:497-505)
// of a LIST of (latent, rolled print) pairs — an examiner's candidate list as afis_rank_hits flattens it — and afis_correspondences, the call of rounds 1-3 for one latent
// as a host view, is a wrapper around the same driver.  The latents are those of a query handle, already resident; the prints are those of the resident shard itself: the
// list is cut into chunks of option corr_pairs_per_launch pairs, and per chunk every launch group of the handle that has pairs in it gets ONE launch of the any-shape
// candidate kernel and ONE of the list kernel, both in their pair-table form (minu.hip, graph.hip: task 3 p + s = selected template s of pair p, compact slots).  What the
// reference does not score (the -1 rules) and what this shard does not hold (-2) is settled here from the host's copies of the shard's tables; nothing is read back per pair.
// The last search's matrix is neither written nor invalidated by the pair call: it uses buffers of its own and the scratch of the minutiae stage, which nothing outlives.
#include "afis_ctx.h"

using namespace afis;

static_assert(kCorrPairsPerLaunch == AFIS_CORR_PAIRS_PER_LAUNCH, "option corr_pairs_per_launch's default is the header's");

namespace afis {

int correspondences_pairs(afis_ctx* ctx, const char* who, const std::vector<QueryGroup>& groups, const std::vector<int32_t>& status, int n_q, int64_t n_pairs,
                          const int32_t* query, const int64_t* idx, int32_t* counts, int16_t* xy, float* part, int out_slots)
{
    const std::string w(who);
    const size_t S = out_slots == 1 ? 1 : 3;                               // selected templates per pair in the caller's arrays: all three, or slot 0 alone (a print's view has no other)
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    ctx->correspondences_us = 0;
    for (int64_t i = 0; i < n_pairs; ++i)
        if (query[i] < 0 || query[i] >= n_q) return fail(ctx, AFIS_EINVAL, w + ": a pair's query is outside 0 .. n_q - 1");
    // a query -> (launch group, position in it), whether it carries selected template s
    std::vector<int32_t> grp_of((size_t)n_q), local((size_t)n_q);
    std::vector<uint8_t> has((size_t)n_q * 3, 0);
    int max_nL = 1;
    {
        int q0 = 0;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            const QueryGroup& grp = groups[gi];
            for (int j = 0; j < grp.nq && q0 + j < n_q; ++j) {
                grp_of[(size_t)(q0 + j)] = (int32_t)gi; local[(size_t)(q0 + j)] = j;
                for (int s = 0; s < 3; ++s) has[(size_t)(q0 + j) * 3 + s] = status[(size_t)(q0 + j)] == AFIS_QUERY_OK && grp.h_has_lm[(size_t)j * 3 + s];
            }
            q0 += grp.nq; max_nL = std::max(max_nL, grp.max_nL);
        }
        if (q0 != n_q) return fail(ctx, AFIS_EINVAL, w + ": the query handle's launch groups do not add up to its queries");
    }
    // ---- the pairs that need the device: a covered print with minutiae and a latent with at least one of the three templates (matcher.cpp:383-404 scores nothing else)
    std::vector<int64_t> dev;                                              // the caller's pair numbers, in the caller's order
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int64_t t = idx[i] - base;
        if (t < 0 || t >= G) continue;
        const uint8_t* h = &has[(size_t)query[i] * 3];
        if (ctx->res_empty[(size_t)t] || ctx->res_mo[(size_t)t + 1] - ctx->res_mo[(size_t)t] <= 0 || !(S == 1 ? h[0] : h[0] | h[1] | h[2])) continue;
        dev.push_back(i);
    }
    // ---- room first: every allocation precedes all device work and the first write into the caller's arrays
    const size_t P = (size_t)std::min<int64_t>((int64_t)dev.size(), ctx->corr_pairs_per_launch);
    const size_t n_grp = groups.size();
    const size_t cands_at = 0, corr_at = cands_at + P * 3 * kTopMinu * sizeof(MinuCand), corr_n_at = corr_at + P * 3 * kTopMinu * sizeof(short4), parts_at = corr_n_at + P * 3 * 4,
                 cand_n_at = parts_at + P * 16, tab_at = cand_n_at + P * 3 * 4, buf_bytes = tab_at + (2 * P + n_grp) * 4;
    const size_t back_bytes = cand_n_at - corr_at;                        // survivors | their counts | parts: what returns, through the pinned buffer
    const size_t pin_tab_at = back_bytes, pin_bytes = pin_tab_at + (2 * P + n_grp) * 4;   // ... behind them a chunk's tables on their way up: pinned memory of the context, so that
                                                                          // an early return leaves nothing queued that reads memory of this call
    static_assert(sizeof(MinuCand) == 8 && sizeof(short4) == 8, "5.8 KB per pair");
    size_t per_wg = 0; int n_wg = 1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (P > 0) {
        // the candidate kernel's grid: what fits the chip at once (its workgroups stride over the tasks), within the scratch the context can afford — what the
        // searches have made it hold already, or 1 GB: a pair of 2000 x 2000 minutiae takes 32 MB of it per workgroup
        per_wg = minu_scratch_floats(max_nL, ctx->max_nR, ctx->s3_tie_order);
        const size_t afford = std::max<size_t>(ctx->scratch.bytes, (size_t)1 << 30);
        const int per_cu = (int)std::max<size_t>(1, (size_t)(160 << 10) / minu_cands_lds_bytes(ctx->s3_tie_order));
        n_wg = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(ctx->n_cus, 1) * per_cu, afford / (per_wg * 4)));
        n_wg = (int)std::min<size_t>((size_t)n_wg, 3 * P);
        HIPCHK(ctx, ctx->scratch.ensure(per_wg * 4 * (size_t)n_wg));
        HIPCHK(ctx, ctx->minu_slab.ensure(graph_minutiae_slab_bytes(3 * (long long)P)));
        HIPCHK(ctx, ctx->corr_buf.ensure(buf_bytes));
        HIPCHK(ctx, ensure_pin(ctx, pin_bytes));
    }
    // ---- what holds without the device: -2 outside the shard, -1 where the reference runs no scorer
    memset(xy, 0, (size_t)n_pairs * S * kTopMinu * 4 * sizeof(int16_t));
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int64_t t = idx[i] - base;
        for (size_t s = 0; s < S; ++s) { counts[(size_t)i * S + s] = (t < 0 || t >= G) ? AFIS_CORR_NOT_COVERED : AFIS_CORR_NOT_RUN; if (part) part[(size_t)i * S + s] = 0.0f; }
    }
    if (P == 0) return AFIS_OK;

    hipStream_t s = ctx->stream;
    uint8_t* const d = ctx->corr_buf.as<uint8_t>();
    const uint8_t* const pin = (const uint8_t*)ctx->h_pin;
    int32_t* const tab = (int32_t*)((uint8_t*)ctx->h_pin + pin_tab_at);   // one chunk's tables, group after group (rewritten only after the chunk's wait)
    std::vector<int32_t> slot_of;                                          // the chunk's pair at every slot
    std::vector<size_t> first(n_grp + 1);
    for (size_t c0 = 0; c0 < dev.size(); c0 += P) {
        const size_t m = std::min(P, dev.size() - c0);
        // the chunk's pairs by launch group (a counting sort: a group's pairs keep the caller's order); slot = place in that order
        std::fill(first.begin(), first.end(), 0);
        for (size_t k = 0; k < m; ++k) ++first[(size_t)grp_of[(size_t)query[dev[c0 + k]]] + 1];
        for (size_t gi = 0; gi < n_grp; ++gi) first[gi + 1] += first[gi];
        std::fill(tab, tab + 2 * m + n_grp, 0); slot_of.assign(m, 0);
        std::vector<size_t> next(first.begin(), first.end() - 1);
        for (size_t gi = 0; gi < n_grp; ++gi) tab[2 * first[gi] + gi] = (int32_t)(first[gi + 1] - first[gi]);      // group gi's table: [count | pairs] at 2 first[gi] + gi
        for (size_t k = 0; k < m; ++k) {
            const int64_t i = dev[c0 + k];
            const size_t gi = (size_t)grp_of[(size_t)query[i]], slot = next[gi]++;
            slot_of[slot] = (int32_t)k;
            tab[2 * slot + gi + 1] = local[(size_t)query[i]]; tab[2 * slot + gi + 2] = (int32_t)(idx[i] - base);
        }
        Events ev{2};
        for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
        HIPCHK(ctx, hipMemcpyAsync(d + tab_at, tab, (2 * m + n_grp) * 4, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipEventRecord(ev[0], s));
        for (size_t gi = 0; gi < n_grp; ++gi) {
            const size_t b = first[gi]; const int n = (int)(first[gi + 1] - b);
            if (n == 0) continue;
            const int32_t* d_tab = (const int32_t*)(d + tab_at) + 2 * b + gi;
            MinuCand* cands = (MinuCand*)(d + cands_at) + b * 3 * kTopMinu;
            int32_t* cand_n = (int32_t*)(d + cand_n_at) + b * 3;
            HIPCHK(ctx, launch_minu_cands_pairs(groups[gi].dev, ctx->gal, ctx->scratch.as<float>(), per_wg, n_wg, ctx->s3_tie_order, d_tab, n, cands, cand_n, s));
            HIPCHK(ctx, launch_graph_minutiae_pairs(groups[gi].dev, ctx->gal, d_tab, n, cands, cand_n, (float*)(d + parts_at) + b * 4, (short4*)(d + corr_at) + b * 3 * kTopMinu,
                                                    (int32_t*)(d + corr_n_at) + b * 3, ctx->minu_slab.p, ctx->minu_slab.bytes, ctx->s89_tie_order, s));
        }
        HIPCHK(ctx, hipEventRecord(ev[1], s));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d + corr_at, back_bytes, hipMemcpyDeviceToHost, s));
        int64_t us = 0;
        AFISCHK(wait_elapsed(ctx, who, ev, &us));
        ctx->correspondences_us += us;
        // ---- into the caller's order; a scorer the reference does not run keeps its -1 (its slot holds an empty list)
        for (size_t slot = 0; slot < m; ++slot) {
            const int64_t i = dev[c0 + (size_t)slot_of[slot]];
            for (size_t sl = 0; sl < S; ++sl) {
                if (!has[(size_t)query[i] * 3 + sl]) continue;
                int32_t n; memcpy(&n, pin + (corr_n_at - corr_at) + (slot * 3 + sl) * 4, 4);
                n = std::min(std::max(n, 0), kTopMinu);
                counts[(size_t)i * S + sl] = n;
                memcpy(xy + ((size_t)i * S + sl) * kTopMinu * 4, pin + (slot * 3 + sl) * kTopMinu * sizeof(short4), (size_t)n * sizeof(short4));
                if (part) memcpy(part + (size_t)i * S + sl, pin + (parts_at - corr_at) + (slot * 4 + sl) * 4, 4);
            }
        }
    }
    return AFIS_OK;
}

}  // namespace afis

extern "C" {

int afis_correspondences_pairs(afis_ctx* ctx, afis_queries* q, int64_t n_pairs, const int32_t* query, const int64_t* idx, int32_t* counts, int16_t* xy, float* part)
{
    const char* const who = "afis_correspondences_pairs";
    if (!ctx || !q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    if (n_pairs < 0 || (n_pairs > 0 && !(query && idx && counts && xy))) return fail(ctx, AFIS_EINVAL, std::string(who) + ": n_pairs must be >= 0 and every pair array given");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    if (n_pairs == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));                                   // the last search's matrix stays rankable
    return correspondences_pairs(ctx, who, q->groups, q->status, q->n_q, n_pairs, query, idx, counts, xy, part);
}

// Correspondence export (matcher.cpp:321-327 calling :376-417 with save_corr = true, :497-505) for one latent given as a host view: the latent becomes a query group of its
// own, the listed templates the pairs (0, gallery_idx[i]).
int afis_correspondences(afis_ctx* ctx, const afis_template_view* query, const int64_t* gallery_idx, int n, int32_t* counts, int16_t* xy)
{
    if (!ctx || !query || n < 0 || (n > 0 && (!gallery_idx || !counts || !xy))) return fail(ctx, AFIS_EINVAL, "afis_correspondences: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_correspondences: commit the gallery first");
    if (n == 0) return AFIS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx));
    for (int i = 0; i < n; ++i)
        if (gallery_idx[i] < ctx->index_base || gallery_idx[i] >= ctx->index_base + ctx->gal.G) return fail(ctx, AFIS_EINVAL, "afis_correspondences: gallery index outside this shard");
    std::vector<QueryGroup> groups(1);
    std::vector<int32_t> status;
    int rc = build_group(ctx, query, 1, groups[0], status);
    if (rc == AFIS_OK) {
        const std::vector<int32_t> zero((size_t)n, 0);
        rc = correspondences_pairs(ctx, "afis_correspondences", groups, status, 1, n, zero.data(), gallery_idx, counts, xy, nullptr);
    }
    if (ctx->search_abandoned) {                                           // timed out: the kernels may still read the group — park it (see afis_queries_free)
        afis_queries* keep = new afis_queries; keep->groups.swap(groups); ctx->parked_queries.push_back(keep);
    }
    for (QueryGroup& g : groups) g.release();
    return rc;
}

}  // extern "C"
