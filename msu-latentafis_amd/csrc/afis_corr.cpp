// afis_corr.cpp — correspondence export of the C ABI (include/afis_matcher.h): afis_correspondences_pairs gives the surviving minutiae correspondences (matcher.cpp:497-505)
// of a LIST of (latent, rolled print) pairs — an examiner's candidate list as afis_rank_hits flattens it — and afis_correspondences, the call of rounds 1-3 for one latent
// as a host view, is a wrapper around the same function.  The latents are those of a query handle, already resident; the prints are those of the resident shard itself.
// The launch sequence is the pair-list calls' one driver (PairCall, afis_ctx.h; afis_pairs.cpp): chunks of option corr_pairs_per_launch pairs, per chunk and launch group
// of the handle ONE launch of the any-shape candidate kernel and ONE of the list kernel in their pair-table forms, and nothing behind them; the survivors, their counts and
// the parts return.  What is stated here is what differs: what the reference does not score (the -1 rules) and what this shard does not hold (-2), settled from the host's
// copies of the shard's tables, and where a slot's survivors go in the caller's arrays.
// The last search's matrix is neither written nor invalidated by the pair call: it uses a buffer of its own and the scratch of the minutiae stage, which nothing outlives.
#include "afis_ctx.h"

using namespace afis;

static_assert(kCorrPairsPerLaunch == AFIS_CORR_PAIRS_PER_LAUNCH, "option corr_pairs_per_launch's default is the header's");

namespace afis {

int correspondences_pairs(afis_ctx* ctx, const char* who, const std::vector<QueryGroup>& groups, const std::vector<int32_t>& status, int n_q, int64_t n_pairs,
                          const int32_t* query, const int64_t* idx, int32_t* counts, int16_t* xy, float* part, int out_slots)
{
    const size_t S = out_slots == 1 ? 1 : 3;                               // selected templates per pair in the caller's arrays: all three, or slot 0 alone (a print's view has no other)
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    std::vector<uint8_t> has((size_t)n_q * 3, 0);                          // whether a query carries selected template s (for a handle the driver refuses, only what exists of it)
    {
        int q0 = 0;
        for (const QueryGroup& grp : groups) {
            for (int j = 0; j < grp.nq && q0 + j < n_q; ++j)
                for (int s = 0; s < 3; ++s) has[(size_t)(q0 + j) * 3 + s] = status[(size_t)(q0 + j)] == AFIS_QUERY_OK && grp.h_has_lm[(size_t)j * 3 + s];
            q0 += grp.nq;
        }
    }
    PairCall c{ctx, who, groups, n_q, n_pairs, query, idx, ctx->corr_pairs_per_launch, &ctx->correspondences_us, false, nullptr};
    // a covered print with minutiae and a latent with at least one of the three templates (matcher.cpp:383-404 scores nothing else)
    c.needs_device = [&](int64_t i) {
        const int64_t t = idx[i] - base;
        if (t < 0 || t >= G) return false;
        const uint8_t* h = &has[(size_t)query[i] * 3];
        return !ctx->res_empty[(size_t)t] && ctx->res_mo[(size_t)t + 1] - ctx->res_mo[(size_t)t] > 0 && (S == 1 ? h[0] : h[0] | h[1] | h[2]) != 0;
    };
    // -2 outside the shard, -1 where the reference runs no scorer
    c.defaults = [&] {
        memset(xy, 0, (size_t)n_pairs * S * kTopMinu * 4 * sizeof(int16_t));
        for (int64_t i = 0; i < n_pairs; ++i) {
            const int64_t t = idx[i] - base;
            for (size_t s = 0; s < S; ++s) { counts[(size_t)i * S + s] = (t < 0 || t >= G) ? AFIS_CORR_NOT_COVERED : AFIS_CORR_NOT_RUN; if (part) part[(size_t)i * S + s] = 0.0f; }
        }
    };
    // a scorer the reference does not run keeps its -1 (its slot holds an empty list)
    c.take = [&](int64_t i, size_t slot, const PairBack& b) {
        for (size_t sl = 0; sl < S; ++sl) {
            if (!has[(size_t)query[i] * 3 + sl]) continue;
            const int32_t n = std::min(std::max(b.corr_n[slot * 3 + sl], 0), kTopMinu);
            counts[(size_t)i * S + sl] = n;
            memcpy(xy + ((size_t)i * S + sl) * kTopMinu * 4, b.corr + (slot * 3 + sl) * kTopMinu, (size_t)n * sizeof(short4));
            if (part) part[(size_t)i * S + sl] = b.parts[slot * 4 + sl];
        }
    };
    return c.run();
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
