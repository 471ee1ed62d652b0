// afis_print_cascade.cpp — the print cascade of the C ABI (include/afis_matcher.h): afis_search_prints_cascade takes RESIDENT prints as queries, runs the minutiae scorer
// for every (query print, column print) cell of the resident shard, selects per query the `keep` best columns by that partial score on the device, and runs the texture
// scorer for the kept cells only.  A kept cell is, bit for bit, afis_search_prints'; every other cell holds the "no entry" word (score_order.h), so the ranking family
// reads the matrix as it reads afis_search_cascade's.  The launch sequence, the buffers' layout, the times and the ends of the call are the cascade driver's
// (CascadeCall: afis_ctx.h, afis_cascade.cpp); this file states what a print cascade's queries are and the kernels that differ (print_cascade.hip):
//   queries   a query with something active is one PSEUDO-QUERY of a temporary handle that is filled on the device (afis_prints.cpp::build_print_queries: its own
//             bounded wait; the texture view is gathered only where the texture term is active), before the driver queues anything.  The queries of the call and the
//             pseudo-queries of the handle differ, so the tables' launch groups are stated in QUERIES: group g begins at the query of its first pseudo-query (group 0 at
//             query 0); the queries between two pseudo-queries have no pairs, whatever group they are counted in.  has[q] = "the texture term of query q is active"
//   tables    behind cascade_tables.h's: q_row [n_q] (the query's pseudo-query, or -1) | piece_p0 [n_pieces] (the first pseudo-query of the piece's group) | q_w [n_q][2]
//   stage 1   k_print_cascade_stage1, once behind the groups, from the per-part scores of ALL pseudo-queries (ctx->parts [n_pseudo][G][4]) -> ctx->scores [n_q][G]: m,
//             the print cell with the texture term left out
//   stage 2   k_print_cascade_gather fills the pair tables from the kept lists; no piece ends in a fusion; k_print_cascade_finish folds every kept cell into the combined
//             matrix and writes the kept cells' two parts into an array of the call's own
#include "afis_ctx.h"
#include "cascade_tables.h"

using namespace afis;

namespace {

// one query of the call: its print (shard-local) and what of it is active
struct PQuery { int32_t local; bool am, at; };

// The temporary handle, the caller's side of the driver, the driver's run.  `plans` (the host's copies of tables a copy may still read) and *q live in the caller,
// beyond its bounded wait.
int print_cascade(CascadeCall& c, const std::vector<PQuery>& pq, const float* w_minu, const float* w_tex, int64_t* n_kept, int64_t* kept_idx, float* kept_parts,
                  std::vector<PrintGroupPlan>& plans, afis_queries** q)
{
    afis_ctx* const ctx = c.ctx;
    const int n_q = c.n_q, keep = c.keep, G = (int)ctx->gal.G;
    hipStream_t s = ctx->stream;
    AFISCHK(c.check_limits());
    // ---- the pseudo-queries and the temporary handle: the views gathered on the device, one bounded wait
    std::vector<int32_t> local, q_row((size_t)n_q, -1), pseudo_q;
    std::vector<uint8_t> use_m, use_t;
    std::vector<float> q_w((size_t)n_q * 2, 0.0f);
    c.has.assign((size_t)n_q, 0);
    for (int i = 0; i < n_q; ++i) {
        const PQuery& p = pq[(size_t)i];
        c.has[(size_t)i] = p.at;
        if (!p.am && !p.at) continue;
        q_row[(size_t)i] = (int32_t)local.size();
        q_w[(size_t)i * 2] = p.am ? w_minu[i] : 0.0f; q_w[(size_t)i * 2 + 1] = p.at ? w_tex[i] : 0.0f;
        local.push_back(p.local); use_m.push_back(p.am); use_t.push_back(p.at); pseudo_q.push_back(i);
    }
    const int n_pseudo = (int)local.size();
    int64_t h2d = 0, gather_us = 0;
    if (n_pseudo > 0) {
        const std::vector<int32_t> res_tile = resident_tile_offsets(ctx);
        AFISCHK(build_print_queries(ctx, c.who, res_tile, local.data(), use_m.data(), use_t.data(), n_pseudo, false, plans, q, &h2d, &gather_us));
        c.groups = &(*q)->groups;                                           // (else no query has anything active: no handle, every kept cell is the -1)
    }
    const size_t n_grp = c.groups ? c.groups->size() : 0;
    std::vector<int32_t> p_first(n_grp + 1, 0);
    for (size_t gi = 0; gi < n_grp; ++gi) p_first[gi + 1] = p_first[gi] + (*c.groups)[gi].nq;
    if (p_first[n_grp] != n_pseudo) return fail(ctx, AFIS_EINVAL, std::string(c.who) + ": the query handle's launch groups do not add up to its pseudo-queries");
    c.q_first.assign(n_grp + 1, 0);
    for (size_t gi = 1; gi < n_grp; ++gi) c.q_first[gi] = pseudo_q[(size_t)p_first[gi]];
    c.q_first[n_grp] = n_q;
    size_t row_at = 0, p0_at = 0, w_at = 0;                                 // int positions of the call's own tables behind cascade_tables.h's (q_w on an 8-byte boundary)
    c.extra_tables = [&](std::vector<int32_t>& up) {
        const size_t n_pieces = c.t->pieces.size();
        row_at = up.size(); p0_at = row_at + (size_t)n_q; w_at = (p0_at + n_pieces + 1) / 2 * 2;
        up.resize(w_at + (size_t)n_q * 2, 0);
        memcpy(up.data() + row_at, q_row.data(), (size_t)n_q * 4);
        for (size_t i = 0; i < n_pieces; ++i) up[p0_at + i] = p_first[c.t->pieces[i].group];
        memcpy(up.data() + w_at, q_w.data(), (size_t)n_q * 8);
    };
    c.fuse_all = [&]() -> int {
        HIPCHK(ctx, launch_print_cascade_stage1(ctx->parts.as<float>(), c.d_dev + row_at, (const float*)(c.d_dev + w_at), ctx->gal.empty, n_q, G, ctx->scores.as<float>(), s));
        return AFIS_OK;
    };
    c.gather = [&]() -> int {
        HIPCHK(ctx, launch_print_cascade_gather(n_q, G, keep, c.nk, c.base, c.d_kept, c.d_q_slot, c.d_dev + c.t->piece_first_at, (int)c.t->pieces.size(), c.d_dev + p0_at, c.d_dev + row_at,
                                                c.d_tab, s));
        return AFIS_OK;
    };
    c.finish = [&]() -> int {
        HIPCHK(ctx, launch_print_cascade_finish(n_q, G, keep, c.nk, c.base, c.d_kept, c.d_q_slot, c.d_dev + row_at, (const float*)(c.d_dev + w_at), ctx->gal.empty, ctx->parts.as<float>(),
                                                c.d_pparts, ctx->elig_scores.as<float>(), c.d_kparts, s));
        return AFIS_OK;
    };
    AFISCHK(c.run(n_kept, kept_idx, kept_parts));
    ctx->print_gather_us = gather_us; ctx->print_h2d_bytes = h2d + c.h2d_bytes;
    return AFIS_OK;
}

}  // namespace

extern "C" {

int afis_search_prints_cascade(afis_ctx* ctx, const int64_t* idx, int n_q, const float* w_minu, const float* w_tex, int keep, float* scores, int32_t* status, int64_t* n_kept,
                               int64_t* kept_idx, float* kept_parts)
{
    const char* const who = "afis_search_prints_cascade";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null context");
    CascadeCall c{ctx, who, n_q, keep, {&ctx->print_cascade_stage1_us, &ctx->print_cascade_select_us, &ctx->print_cascade_stage2_us, &ctx->print_cascade_kept_pairs}, 2, true};
    c.clear();
    ctx->print_gather_us = 0; ctx->print_h2d_bytes = 0;
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
    if (n_q == 0 || ctx->gal.G == 0) {                                      // nothing to score: as afis_search answers it; no list holds anything
        AFISCHK(c.empty(afis_search(ctx, nullptr, 0, scores, nullptr, nullptr, 0, nullptr, nullptr), n_kept, kept_idx, kept_parts));
        if (status) for (int i = 0; i < n_q; ++i) status[i] = AFIS_QUERY_LATENT_EMPTY;
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
    afis_queries* q = nullptr;
    const int rc = c.end(print_cascade(c, pq, w_minu, w_tex, n_kept, kept_idx, kept_parts, plans, &q), scores);
    afis_queries_free(ctx, q);                                              // (parked while a timed-out launch may still read it)
    if (rc != AFIS_OK) { ctx->print_gather_us = 0; ctx->print_h2d_bytes = 0; }
    else if (status) for (int i = 0; i < n_q; ++i) status[i] = pq[(size_t)i].am || pq[(size_t)i].at ? AFIS_QUERY_OK : AFIS_QUERY_LATENT_EMPTY;
    return rc;
}

}  // extern "C"
