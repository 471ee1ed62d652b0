// afis_taps.cpp — the parity taps (include/afis_matcher_taps.h: afis_debug_*): stage intermediates for tests/, and the host side of the direct exact ADC kernels
// (adc_direct.hip, adc_variant 0-3, 6, 7).  Built ONLY into libafis_hip_test.so, with adc_direct.o; the product library exports none of the taps and has none of the kernels.
#include "afis_ctx.h"
#include "../../include/afis_matcher_taps.h"
#include "cascade_tables.h"
#include "pair_tables.h"

using namespace afis;

// The conflict-free kernel's lane-ordered code stream (variants 6 / 7) — a full copy of the PQ codes that nothing else reads — and its block offsets
// ((blocks + 1) x 64 entries per template), laid out at the first use of those variants.
static int ensure_codes_cf(afis_ctx* ctx, Shard& sh, int variant)
{
    if ((variant != 6 && variant != 7) || sh.codes_cf_built) return AFIS_OK;
    const int64_t G = sh.gal.G;
    std::vector<int32_t> to((size_t)G + 1), cfb((size_t)G + 1);
    HIPCHK(ctx, hipMemcpyAsync(to.data(), sh.gal.tex_off, to.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int64_t nblk = 0;
    for (int64_t t = 0; t < G; ++t) { cfb[(size_t)t] = (int32_t)nblk; const int64_t n = to[(size_t)t + 1] - to[(size_t)t]; nblk += n > 0 ? (n + 63) / 64 + 1 : 0; }
    cfb[(size_t)G] = (int32_t)nblk;
    if (nblk > 0x7fffffff / 64) return fail(ctx, AFIS_EINVAL, "adc_variant 6 / 7: shard too large for the direct kernel's code stream; split the gallery into more shards");
    HIPCHK(ctx, upload(sh.g_tex_cf_blk, cfb, ctx->stream));
    HIPCHK(ctx, sh.g_tex_codes_cf.ensure(std::max<size_t>((size_t)nblk * 64 * 16, 16)));
    sh.gal.tex_cf_blk = sh.g_tex_cf_blk.as<int32_t>();
    sh.gal.tex_codes_cf = sh.g_tex_codes_cf.as<uint4>();
    HIPCHK(ctx, launch_codes_cf(sh.gal, sh.g_tex_codes_cf.p, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    sh.codes_cf_built = true;
    return AFIS_OK;
}

// S4-S6 of a direct kernel for the query group d against the gallery view g (rm_val / rm_arg sized by the caller)
static int direct_rowmax(afis_ctx* ctx, const QueryDev& d, const GalleryDev& g, int variant, int chunk, hipEvent_t after_lut)
{
    HIPCHK(ctx, ctx->lut.ensure(std::max<size_t>((size_t)d.n_tiles * kTileFloats * 4, 16)));
    HIPCHK(ctx, launch_lut_build(d, ctx->codewords.as<float>(), ctx->lut.as<float>(), variant, ctx->stream));
    if (after_lut) HIPCHK(ctx, hipEventRecord(after_lut, ctx->stream));
    HIPCHK(ctx, launch_adc_rowmax(d, g, ctx->lut.as<float>(), chunk, variant, ctx->rm_val.as<float>(), ctx->rm_arg.as<int32_t>(), ctx->stream));
    return AFIS_OK;
}

// g_direct_adc_stage (afis_ctx.h): the selected direct kernel against a shard (the resident one, or a subset's)
static int direct_adc_stage(afis_ctx* ctx, Shard& sh, const QueryDev& d, int chunk, hipEvent_t after_lut)
{
    const int rcf = ensure_codes_cf(ctx, sh, ctx->adc_variant);
    if (rcf != AFIS_OK) return rcf;
    return direct_rowmax(ctx, d, sh.gal, ctx->adc_variant, chunk, after_lut);
}
__attribute__((constructor)) static void set_direct_adc_stage() { g_direct_adc_stage = direct_adc_stage; }

extern "C" {

int afis_debug_phase_cycles(afis_ctx* ctx, unsigned long long* out32, int reset)
{
    if (!ctx || !out32) return AFIS_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, read_phase_cycles(out32, reset != 0));
    unsigned long long gph[16];                          // graph.hip phases (only in PHASE_TIMING builds) reported in slots 0..15 + 32.. is not
    HIPCHK(ctx, read_graph_phase_cycles(gph, reset != 0)); // possible with a 32-slot array: they overlay the unused slots 5..15 and 21..25
    for (int i = 0; i < 8; ++i) { out32[5 + i] = gph[i]; out32[21 + i] = gph[8 + i]; }
    return AFIS_OK;
}

// adc_variant 9, after afis_set_option("mf_stats", 1): counters of the selection / recomputation kernel accumulated since the last reset:
// out[0] pairs, [1] latent rows, [2] rows evaluated (may reach the top 200), [3] candidate cells evaluated, [4] rows evaluated over every point,
// [5] rows whose exact maximum lay outside its bounds (self-check, must be 0)
int afis_debug_refine_stats(afis_ctx* ctx, unsigned long long* out8, int reset)
{
    if (!ctx || !out8) return fail(ctx, AFIS_EINVAL, "afis_debug_refine_stats: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    if (!ctx->mf_stats.p) return AFIS_OK;
    HIPCHK(ctx, hipMemcpy(out8, ctx->mf_stats.p, 64, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(ctx, hipMemset(ctx->mf_stats.p, 0, 64));
    return AFIS_OK;
}

int afis_debug_compact_stats(afis_ctx* ctx, long long* out2)
{
    if (!ctx || !out2) return fail(ctx, AFIS_EINVAL, "afis_debug_compact_stats: bad argument");
    out2[0] = ctx->compact_us; out2[1] = ctx->compact_bytes;
    return AFIS_OK;
}

// A caller-made score matrix [n_q][G] for the resident shard in place of a search's: uploaded into ctx->scores, marked as a full search of n_q queries leaves it,
// then ranked by the code afis_rank_subjects runs.
int afis_debug_rank_subjects(afis_ctx* ctx, afis_subjects* subjects, const float* scores, int n_q, int k, int64_t* subject_id, float* subject_score, int64_t* best_idx)
{
    if (!ctx || !subjects || !scores || n_q <= 0) return fail(ctx, AFIS_EINVAL, "afis_debug_rank_subjects: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_debug_rank_subjects: commit the gallery first");
    { const int rcq = quiesce(ctx, "afis_debug_rank_subjects"); if (rcq != AFIS_OK) return rcq; }
    const int64_t G = ctx->gal.G;
    if (G > 0) {
        HIPCHK(ctx, ctx->scores.ensure((size_t)n_q * (size_t)G * 4));
        HIPCHK(ctx, hipMemcpy(ctx->scores.p, scores, (size_t)n_q * (size_t)G * 4, hipMemcpyHostToDevice));
    }
    ctx->last_search = LastSearch{true, n_q, G, nullptr, ctx->gallery_epoch};
    return afis_rank_subjects(ctx, subjects, n_q, k, subject_id, subject_score, best_idx);
}

// The same for the hit lists: the matrix is uploaded and marked valid, then afis_rank_hits (subjects == NULL; out_b is not touched) or afis_rank_subject_hits runs.
int afis_debug_rank_hits(afis_ctx* ctx, afis_subjects* subjects, const float* scores, int n_q, float min_score, int cap, int64_t* n_hits, int64_t* out_a, float* out_score, int64_t* out_b)
{
    if (!ctx || !scores || n_q <= 0) return fail(ctx, AFIS_EINVAL, "afis_debug_rank_hits: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_debug_rank_hits: commit the gallery first");
    { const int rcq = quiesce(ctx, "afis_debug_rank_hits"); if (rcq != AFIS_OK) return rcq; }
    const int64_t G = ctx->gal.G;
    if (G > 0) {
        HIPCHK(ctx, ctx->scores.ensure((size_t)n_q * (size_t)G * 4));
        HIPCHK(ctx, hipMemcpy(ctx->scores.p, scores, (size_t)n_q * (size_t)G * 4, hipMemcpyHostToDevice));
    }
    ctx->last_search = LastSearch{true, n_q, G, nullptr, ctx->gallery_epoch};
    return subjects ? afis_rank_subject_hits(ctx, subjects, n_q, min_score, cap, n_hits, out_a, out_score, out_b) : afis_rank_hits(ctx, n_q, min_score, cap, n_hits, out_a, out_score);
}

// ... and for the column hit lists: afis_rank_latent_hits runs on the uploaded matrix, n_templates = the resident shard's size.
int afis_debug_rank_latent_hits(afis_ctx* ctx, const float* scores, int n_q, float min_score, int cap, int64_t latent_base, int64_t* n_hits, int64_t* latent_idx, float* score)
{
    if (!ctx || !scores || n_q <= 0) return fail(ctx, AFIS_EINVAL, "afis_debug_rank_latent_hits: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_debug_rank_latent_hits: commit the gallery first");
    { const int rcq = quiesce(ctx, "afis_debug_rank_latent_hits"); if (rcq != AFIS_OK) return rcq; }
    const int64_t G = ctx->gal.G;
    if (G > 0) {
        HIPCHK(ctx, ctx->scores.ensure((size_t)n_q * (size_t)G * 4));
        HIPCHK(ctx, hipMemcpy(ctx->scores.p, scores, (size_t)n_q * (size_t)G * 4, hipMemcpyHostToDevice));
    }
    ctx->last_search = LastSearch{true, n_q, G, nullptr, ctx->gallery_epoch};
    return afis_rank_latent_hits(ctx, G, min_score, cap, latent_base, n_hits, latent_idx, score);
}

// ... and for the rank list of afis_search* itself: the matrix [n_q][n] over the resident shard (sub == NULL) or over a subset's sub-shard — its columns in the order the
// sub-shard holds them, ascending global index — is uploaded and marked valid as that search marks it, then listed by the code at the end of search_shard: k_topk with the
// base the search passes (and the subset's index map) for k <= kDeviceTopK, host_rank_rows on the caller's column order (launch_permute_columns for a subset listed out
// of order) beyond.
int afis_debug_rank_rows(afis_ctx* ctx, afis_subset* sub, const float* scores, int n_q, int k, int64_t* topk_idx, float* topk_score)
{
    if (!ctx || !scores || n_q <= 0 || k <= 0 || !topk_idx || !topk_score) return fail(ctx, AFIS_EINVAL, "afis_debug_rank_rows: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_debug_rank_rows: commit the gallery first");
    if (sub && std::find(ctx->subsets.begin(), ctx->subsets.end(), sub) == ctx->subsets.end()) return fail(ctx, AFIS_EINVAL, "afis_debug_rank_rows: not a live subset of this context");
    if (sub && sub->gallery_epoch != ctx->gallery_epoch) return fail_edited(ctx, "afis_debug_rank_rows", "this subset was created", false);
    { const int rcq = quiesce(ctx, "afis_debug_rank_rows"); if (rcq != AFIS_OK) return rcq; }
    const Shard& sh = sub ? sub->sh : *ctx;
    const int64_t G = sh.gal.G;
    const size_t n_out = (size_t)n_q * (size_t)k, bytes = (size_t)n_q * (size_t)G * 4;
    hipStream_t s = ctx->stream;
    if (G > 0) {
        HIPCHK(ctx, ctx->scores.ensure(bytes));
        HIPCHK(ctx, hipMemcpy(ctx->scores.p, scores, bytes, hipMemcpyHostToDevice));
    }
    ctx->last_search = LastSearch{true, n_q, G, sub, ctx->gallery_epoch};
    if (k <= kDeviceTopK && G > 0) {
        HIPCHK(ctx, ctx->topk_idx.ensure(n_out * 8)); HIPCHK(ctx, ctx->topk_score.ensure(n_out * 4));
        HIPCHK(ctx, launch_topk(ctx->scores.as<float>(), n_q, (int)G, k, sub ? 0ll : (long long)sh.index_base, ctx->topk_idx.as<long long>(), ctx->topk_score.as<float>(), s));
        if (sub) HIPCHK(ctx, launch_subset_topk_map(ctx->topk_idx.as<long long>(), (long long)n_out, sub->d_global.as<long long>(), (int)G, s));
        HIPCHK(ctx, hipMemcpyAsync(topk_idx, ctx->topk_idx.p, n_out * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(topk_score, ctx->topk_score.p, n_out * 4, hipMemcpyDeviceToHost, s));
        const int rcw = wait_streams(ctx, {s}, "afis_debug_rank_rows");
        if (rcw != AFIS_OK) ctx->last_search.valid = false;
        return rcw;
    }
    std::vector<float> h((size_t)n_q * (size_t)G);
    if (G > 0) {
        const void* src = ctx->scores.p;
        if (sub && !sub->identity) {
            HIPCHK(ctx, ctx->out_perm.ensure(bytes));
            HIPCHK(ctx, launch_permute_columns(ctx->scores.p, ctx->out_perm.p, 4, n_q, (int)G, sub->d_pos.as<int32_t>(), s));
            src = ctx->out_perm.p;
        }
        HIPCHK(ctx, hipMemcpyAsync(h.data(), src, bytes, hipMemcpyDeviceToHost, s));
        const int rcw = wait_streams(ctx, {s}, "afis_debug_rank_rows");
        if (rcw != AFIS_OK) { ctx->last_search.valid = false; return rcw; }
    }
    host_rank_rows(h.data(), n_q, G, k, sub ? sub->idx.data() : nullptr, sh.index_base, topk_idx, topk_score);
    return AFIS_OK;
}

int afis_debug_transpose_stats(afis_ctx* ctx, long long* out2)
{
    if (!ctx || !out2) return fail(ctx, AFIS_EINVAL, "afis_debug_transpose_stats: bad argument");
    out2[0] = ctx->transpose_us; out2[1] = ctx->transpose_bytes;
    return AFIS_OK;
}

// k_expand_rows on planted data: the tables are made as afis_search_eligible makes them (inv from the ascending column list), in buffers of the call's own
int afis_debug_expand_rows(afis_ctx* ctx, const float* cls, int n_c, int64_t m, const int32_t* row_of, const int32_t* sel, int n_q, int64_t G, float* out)
{
    if (!ctx || n_c <= 0 || n_q <= 0 || G <= 0 || G > 0x7fffffff || m < 0 || m > G || !row_of || !out || (m > 0 && !cls) || (!sel && m > 0 && m != G))
        return fail(ctx, AFIS_EINVAL, "afis_debug_expand_rows: bad argument");
    std::vector<uint8_t> seen((size_t)n_q, 0);
    for (int r = 0; r < n_c; ++r) {
        if (row_of[r] < 0 || row_of[r] >= n_q || seen[(size_t)row_of[r]]) return fail(ctx, AFIS_EINVAL, "afis_debug_expand_rows: row_of must hold distinct rows of out");
        seen[(size_t)row_of[r]] = 1;
    }
    std::vector<int32_t> inv;
    if (sel && m > 0) {
        inv.assign((size_t)G, -1);
        for (int64_t i = 0; i < m; ++i) {
            if (sel[i] < 0 || sel[i] >= G || (i > 0 && sel[i] <= sel[i - 1])) return fail(ctx, AFIS_EINVAL, "afis_debug_expand_rows: sel must be strictly ascending columns of out");
            inv[(size_t)sel[i]] = (int32_t)i;
        }
    }
    { const int rcq = quiesce(ctx, "afis_debug_expand_rows"); if (rcq != AFIS_OK) return rcq; }
    DevBuf d_cls, d_inv, d_rows, d_out;
    struct Drop { DevBuf *a, *b, *c, *d; ~Drop() { a->release(); b->release(); c->release(); d->release(); } } drop{&d_cls, &d_inv, &d_rows, &d_out};
    const size_t out_bytes = (size_t)n_q * (size_t)G * 4, cls_bytes = (size_t)n_c * (size_t)m * 4;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, d_out.ensure(out_bytes)); HIPCHK(ctx, d_rows.ensure((size_t)n_c * 4));
    if (cls_bytes) HIPCHK(ctx, d_cls.ensure(cls_bytes));
    if (!inv.empty()) HIPCHK(ctx, d_inv.ensure((size_t)G * 4));
    HIPCHK(ctx, hipMemcpy(d_out.p, out, out_bytes, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(d_rows.p, row_of, (size_t)n_c * 4, hipMemcpyHostToDevice));
    if (cls_bytes) HIPCHK(ctx, hipMemcpy(d_cls.p, cls, cls_bytes, hipMemcpyHostToDevice));
    if (!inv.empty()) HIPCHK(ctx, hipMemcpy(d_inv.p, inv.data(), (size_t)G * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, launch_expand_rows(d_cls.as<float>(), n_c, (int)m, inv.empty() ? nullptr : d_inv.as<int32_t>(), d_rows.as<int32_t>(), n_q, (int)G, d_out.as<float>(), s));
    { const int rcw = wait_streams(ctx, {s}, "afis_debug_expand_rows"); if (rcw != AFIS_OK) return rcw; }
    HIPCHK(ctx, hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
    return AFIS_OK;
}

// k_cascade_gather_mapped and k_cascade_scatter_mapped on planted tables: the structure is made as the cascade driver makes it (cascade_tables.h), in buffers of the call's own
int afis_debug_kept_cells_mapped(afis_ctx* ctx, int n_q, int64_t G_res, int64_t m, int keep, int n_kept, int64_t index_base, const int64_t* kept, const uint8_t* has,
                              const int32_t* q_first, int n_grp, int per_launch, const int32_t* sel, const float* parts, const float* pair_score, const int32_t* row_of,
                              const int32_t* out_col, int64_t out_rows, int64_t out_stride, int32_t* tab, int64_t tab_ints, int32_t* n_pieces, float* pair_parts, float* out)
{
    const char* const who = "afis_debug_kept_cells_mapped";
    if (!ctx || n_q <= 0 || G_res <= 0 || G_res > 0x7fffffff || m <= 0 || m > G_res || (!sel && m != G_res) || keep < 1 || keep > AFIS_HITS_MAX || n_kept < 1 || n_kept > keep ||
        n_kept > m || !kept || !has || !q_first || n_grp < 1 || per_launch < 1 || !parts || !pair_score || out_rows <= 0 || out_stride <= 0 ||
        out_rows * out_stride > 0x7ffffff0LL || (int64_t)n_q * m > 0x7ffffff0LL / 4 || !tab || !n_pieces || !pair_parts || !out)
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": bad argument");
    if (q_first[0] != 0 || q_first[n_grp] != n_q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": q_first must run from 0 to n_q");
    for (int g = 0; g < n_grp; ++g) if (q_first[g + 1] < q_first[g]) return fail(ctx, AFIS_EINVAL, std::string(who) + ": q_first must ascend");
    std::vector<int32_t> inv;
    if (sel) {
        inv.assign((size_t)G_res, -1);
        for (int64_t i = 0; i < m; ++i) {
            if (sel[i] < 0 || sel[i] >= G_res || (i > 0 && sel[i] <= sel[i - 1])) return fail(ctx, AFIS_EINVAL, std::string(who) + ": sel must be strictly ascending positions of the resident shard");
            inv[(size_t)sel[i]] = (int32_t)i;
        }
    }
    for (int q = 0; q < n_q && row_of; ++q) if (row_of[q] < 0 || row_of[q] >= out_rows) return fail(ctx, AFIS_EINVAL, std::string(who) + ": row_of must hold rows of out");
    for (int64_t t = 0; t < m && out_col; ++t) if (out_col[t] < 0 || out_col[t] >= out_stride) return fail(ctx, AFIS_EINVAL, std::string(who) + ": out_col must hold columns of out");
    CascadeTables t;
    if (!build_cascade_tables((size_t)n_q, has, (size_t)n_kept, (size_t)n_grp, q_first, kAdcPairsSegment, (size_t)per_launch, t) || (int64_t)t.tab_ints() > tab_ints)
        return fail(ctx, AFIS_EINVAL, std::string(who) + ": tab does not hold the pair tables");
    *n_pieces = (int32_t)t.pieces.size();
    { const int rcq = quiesce(ctx, who); if (rcq != AFIS_OK) return rcq; }
    DevBuf b[10];
    struct Drop { DevBuf* b; ~Drop() { for (int i = 0; i < 10; ++i) b[i].release(); } } drop{b};
    const size_t total = t.total, out_bytes = (size_t)out_rows * (size_t)out_stride * 4;
    const struct Up { const void* src; size_t bytes; } ups[10] = {{kept, (size_t)n_q * (size_t)keep * 8}, {t.dev.data(), t.dev.size() * 4}, {inv.data(), inv.size() * 4},
        {parts, (size_t)n_q * (size_t)m * 16}, {pair_score, total * 4}, {row_of, row_of ? (size_t)n_q * 4 : 0}, {out_col, out_col ? (size_t)m * 4 : 0}, {tab, (size_t)tab_ints * 4},
        {pair_parts, total * 16}, {out, out_bytes}};
    for (int i = 0; i < 10; ++i) {
        HIPCHK(ctx, b[i].ensure(std::max<size_t>(ups[i].bytes, 16)));
        if (ups[i].bytes) HIPCHK(ctx, hipMemcpy(b[i].p, ups[i].src, ups[i].bytes, hipMemcpyHostToDevice));
    }
    hipStream_t s = ctx->stream;
    const int32_t* const d_dev = b[1].as<int32_t>();
    const int32_t* const d_inv = sel ? b[2].as<int32_t>() : nullptr;
    HIPCHK(ctx, launch_cascade_gather_mapped(n_q, (int)G_res, (int)m, keep, n_kept, index_base, b[0].as<long long>(), d_dev + t.q_slot_at, d_dev + t.piece_first_at, (int)t.pieces.size(),
                                             d_dev + t.piece_q0_at, d_inv, b[3].as<float>(), b[7].as<int32_t>(), b[8].as<float>(), s));
    HIPCHK(ctx, launch_cascade_scatter_mapped(n_q, (int)G_res, (int)m, keep, n_kept, index_base, b[0].as<long long>(), d_dev + t.q_slot_at, b[4].as<float>(), d_inv,
                                              row_of ? b[5].as<int32_t>() : nullptr, out_col ? b[6].as<int32_t>() : nullptr, (long long)out_rows, (long long)out_stride, b[9].as<float>(), s));
    { const int rcw = wait_streams(ctx, {s}, who); if (rcw != AFIS_OK) return rcw; }
    HIPCHK(ctx, hipMemcpy(tab, b[7].p, (size_t)tab_ints * 4, hipMemcpyDeviceToHost));
    if (total) HIPCHK(ctx, hipMemcpy(pair_parts, b[8].p, total * 16, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(out, b[9].p, out_bytes, hipMemcpyDeviceToHost));
    return AFIS_OK;
}

int afis_debug_fold_templates(afis_ctx* ctx, const float* parts, int64_t n_pseudo, int64_t G, const int32_t* qd, int n_q, const float* w, const uint8_t* empty, float* out)
{
    if (!ctx || n_q <= 0 || G <= 0 || G > 0x7fffffff || n_pseudo < 0 || n_pseudo > 0x7fffffff / 4 || !qd || !empty || !out || (n_pseudo > 0 && (!parts || !w)))
        return fail(ctx, AFIS_EINVAL, "afis_debug_fold_templates: bad argument");
    for (int q = 0; q < n_q; ++q) {
        const int32_t* d = qd + (size_t)q * 4;
        if (d[0] < 0 || d[1] < 0 || (int64_t)d[0] + d[1] > n_pseudo || d[2] < 0 || d[2] > d[1])
            return fail(ctx, AFIS_EINVAL, "afis_debug_fold_templates: a query's pseudo-queries must lie inside parts, its texture count inside them");
    }
    { const int rcq = quiesce(ctx, "afis_debug_fold_templates"); if (rcq != AFIS_OK) return rcq; }
    DevBuf d_parts, d_tab, d_empty, d_out;
    struct Drop { DevBuf *a, *b, *c, *d; ~Drop() { a->release(); b->release(); c->release(); d->release(); } } drop{&d_parts, &d_tab, &d_empty, &d_out};
    const size_t out_bytes = (size_t)n_q * (size_t)G * 4, parts_bytes = (size_t)n_pseudo * (size_t)G * 16, w_bytes = (size_t)n_pseudo * 16;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, d_out.ensure(out_bytes)); HIPCHK(ctx, d_empty.ensure((size_t)G));
    HIPCHK(ctx, d_parts.ensure(std::max<size_t>(parts_bytes, 16))); HIPCHK(ctx, d_tab.ensure((size_t)n_q * 16 + std::max<size_t>(w_bytes, 16)));
    HIPCHK(ctx, hipMemcpy(d_out.p, out, out_bytes, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(d_empty.p, empty, (size_t)G, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(d_tab.p, qd, (size_t)n_q * 16, hipMemcpyHostToDevice));
    float* const d_w = reinterpret_cast<float*>(d_tab.as<uint8_t>() + (size_t)n_q * 16);
    if (parts_bytes) { HIPCHK(ctx, hipMemcpy(d_parts.p, parts, parts_bytes, hipMemcpyHostToDevice)); HIPCHK(ctx, hipMemcpy(d_w, w, w_bytes, hipMemcpyHostToDevice)); }
    HIPCHK(ctx, launch_fold_templates(d_parts.as<float>(), d_tab.as<int32_t>(), d_w, d_empty.as<uint8_t>(), n_q, (int)G, d_out.as<float>(), s));
    { const int rcw = wait_streams(ctx, {s}, "afis_debug_fold_templates"); if (rcw != AFIS_OK) return rcw; }
    HIPCHK(ctx, hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
    return AFIS_OK;
}

int afis_debug_print_queries(afis_ctx* ctx, const int64_t* idx, int n, const uint8_t* use_minu, const uint8_t* use_tex, int32_t* counts, int32_t* lm_off, int32_t* lm_tile_off,
                             int32_t* lt_off, int32_t* tile_off, int32_t* tile16_off, int32_t* tex_slot, int32_t* status, int16_t* lm_xy, float* lm_ori, float* lm_des, float* lm_frag,
                             int16_t* lt_xy, float* lt_ori, float* lt_des)
{
    if (!ctx || n <= 0 || !idx || !use_minu || !use_tex || !counts) return fail(ctx, AFIS_EINVAL, "afis_debug_print_queries: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_debug_print_queries: commit the gallery first");
    std::vector<int32_t> local((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (idx[i] < ctx->index_base || idx[i] - ctx->index_base >= (int64_t)ctx->res_empty.size()) return fail(ctx, AFIS_EINVAL, "afis_debug_print_queries: an index outside the resident shard");
        local[(size_t)i] = (int32_t)(idx[i] - ctx->index_base);
    }
    { const int rcq = quiesce(ctx, "afis_debug_print_queries"); if (rcq != AFIS_OK) return rcq; }
    QueryGroup grp;
    struct Drop { QueryGroup* g; ~Drop() { g->release(); } } drop{&grp};
    PrintGroupPlan plan;
    std::vector<int32_t> st;
    AFISCHK(prepare_print_group(ctx, resident_tile_offsets(ctx), local.data(), use_minu, use_tex, n, grp, plan, st));
    counts[0] = plan.n_lm; counts[1] = plan.n_lm_tiles; counts[2] = plan.n_lt; counts[3] = grp.dev.lt_pad;
    if (!lm_off) return AFIS_OK;                                            // the sizes only: the caller allocates and calls again
    if (!lm_tile_off || !lt_off || !tile_off || !tile16_off || !tex_slot || !status || !lm_xy || !lm_ori || !lm_des || !lm_frag || !lt_xy || !lt_ori || !lt_des)
        return fail(ctx, AFIS_EINVAL, "afis_debug_print_queries: a null output");
    // every byte of the arrays is planted, so that a word the gather leaves out shows
    for (DevBuf* b : {&grp.lm_off, &grp.lm_xy, &grp.lm_ori, &grp.lm_des, &grp.lm_frag, &grp.lt_xy, &grp.lt_ori, &grp.lt_des}) HIPCHK(ctx, hipMemsetAsync(b->p, 0xA5, b->bytes, ctx->stream));
    int64_t h2d = 0;
    AFISCHK(queue_print_group(ctx, grp, plan, &h2d));
    { const int rcw = wait_streams(ctx, {ctx->stream}, "afis_debug_print_queries"); if (rcw != AFIS_OK) return rcw; }
    const QueryDev& d = grp.dev;
    const size_t nq = (size_t)n, n_lm = (size_t)plan.n_lm, n_tiles = (size_t)plan.n_lm_tiles, n_lt = (size_t)plan.n_lt;
    struct Back { void* dst; const void* src; size_t bytes; };
    for (const Back& b : {Back{lm_off, d.lm_off, (3 * nq + 1) * 4}, Back{lm_tile_off, d.lm_tile_off, (3 * nq + 1) * 4}, Back{lt_off, d.lt_off, (nq + 1) * 4}, Back{tile_off, d.tile_off, (nq + 1) * 4},
                          Back{tile16_off, d.tile16_off, (nq + 1) * 4}, Back{tex_slot, d.tex_slot, nq * 4}, Back{status, d.status, nq * 4}, Back{lm_xy, d.lm_xy, n_lm * 4},
                          Back{lm_ori, d.lm_ori, n_lm * 4}, Back{lm_des, d.lm_des, n_lm * kDes * 4}, Back{lm_frag, d.lm_frag, n_tiles * 6 * 64 * 16}, Back{lt_xy, d.lt_xy, n_lt * 4},
                          Back{lt_ori, d.lt_ori, n_lt * 4}, Back{lt_des, d.lt_des, n_lt * kDes * 4}})
        if (b.bytes) HIPCHK(ctx, hipMemcpy(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost));
    return AFIS_OK;
}

int afis_debug_atan2_grid(afis_ctx* ctx, int R, float* out)
{
    if (!ctx || !out || R < 0 || R > 4096) return fail(ctx, AFIS_EINVAL, "afis_debug_atan2_grid: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)(2 * R + 1) * (2 * R + 1);
    DevBuf d;
    HIPCHK(ctx, d.ensure(n * 4));
    hipError_t e = launch_debug_atan2_grid(R, d.as<float>(), ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d.p, n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    d.release();
    if (e != hipSuccess) return fail(ctx, AFIS_EDEVICE, std::string("afis_debug_atan2_grid: ") + hipGetErrorString(e));
    return AFIS_OK;
}

int afis_debug_graph_arith(afis_ctx* ctx, unsigned long long* out8)
{
    if (!ctx || !out8) return fail(ctx, AFIS_EINVAL, "afis_debug_graph_arith: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf d;
    HIPCHK(ctx, d.ensure(64));
    hipError_t e = launch_debug_graph_arith(d.as<unsigned long long>(), ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out8, d.p, 64, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    d.release();
    if (e != hipSuccess) return fail(ctx, AFIS_EDEVICE, std::string("afis_debug_graph_arith: ") + hipGetErrorString(e));
    return AFIS_OK;
}

int afis_debug_lut(afis_ctx* ctx, const afis_template_view* query, float* out, int32_t* n_rows)
{
    if (!ctx || !query || !out) return fail(ctx, AFIS_EINVAL, "afis_debug_lut: null argument");
    if (query->n_tex <= 0) { if (n_rows) *n_rows = 0; return AFIS_OK; }
    const afis_texture_view& x = query->tex[0];
    if (x.des_len != kDes || !x.des) return fail(ctx, AFIS_EINVAL, "afis_debug_lut: latent texture template needs fp32 descriptors of length 96");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf des, lut;
    std::vector<float> h(x.des, x.des + (size_t)x.n * kDes);
    HIPCHK(ctx, upload(des, h, ctx->stream));
    HIPCHK(ctx, lut.ensure((size_t)x.n * kM * kK * 4));
    HIPCHK(ctx, launch_lut_reference_layout(des.as<float>(), x.n, ctx->codewords.as<float>(), lut.as<float>(), ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out, lut.p, (size_t)x.n * kM * kK * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    des.release(); lut.release();
    if (n_rows) *n_rows = x.n;
    return AFIS_OK;
}

int afis_debug_texture_rowmax(afis_ctx* ctx, const afis_template_view* query, int64_t gidx, float* val, int32_t* arg, int32_t* n_rows)
{
    if (!ctx || !query || !val || !arg) return fail(ctx, AFIS_EINVAL, "afis_debug_texture_rowmax: null argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_debug_texture_rowmax: commit the gallery first");
    if (gidx < 0 || gidx >= ctx->gal.G) return fail(ctx, AFIS_EINVAL, "afis_debug_texture_rowmax: gallery index out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    QueryGroup grp; std::vector<int32_t> st;
    int rc = build_group(ctx, query, 1, grp, st);
    if (rc != AFIS_OK) { grp.release(); return rc; }
    const QueryDev& d = grp.dev;
    const int n_lt = grp.h_lt_n[0];
    if (n_rows) *n_rows = n_lt;
    if (n_lt > 0) {
        const size_t n_pairs = (size_t)ctx->gal.G;
        HIPCHK(ctx, ctx->rm_val.ensure(n_pairs * d.lt_pad * 4));
        HIPCHK(ctx, ctx->rm_arg.ensure(n_pairs * d.lt_pad * 4));
        HIPCHK(ctx, hipMemsetAsync(ctx->rm_val.p, 0, n_pairs * d.lt_pad * 4, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(ctx->rm_arg.p, 0, n_pairs * d.lt_pad * 4, ctx->stream));
        if (ctx->adc_variant == 9) { int rc9 = adc_stage_mfma(ctx, *ctx, grp, true); if (rc9 != AFIS_OK) { grp.release(); return rc9; } }
        else if (ctx->adc_variant == 8) { int rc16 = adc_stage_q(ctx, *ctx, grp, ctx->chunk > 0 ? ctx->chunk : 32, true); if (rc16 != AFIS_OK) { grp.release(); return rc16; } }
        else { int rcd = direct_adc_stage(ctx, *ctx, d, ctx->chunk > 0 ? ctx->chunk : 32, nullptr); if (rcd != AFIS_OK) { grp.release(); return rcd; } }
        HIPCHK(ctx, hipMemcpyAsync(val, ctx->rm_val.as<float>() + (size_t)gidx * d.lt_pad, (size_t)n_lt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(arg, ctx->rm_arg.as<int32_t>() + (size_t)gidx * d.lt_pad, (size_t)n_lt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    grp.release();
    return AFIS_OK;
}

// Parity tap: the correspondence list of one (latent, gallery template) pair after a stage of a scorer.
//   which 0 = texture scorer, 1..3 = minutiae scorer of selected template 27 / 3 / 12;  stage 0 = candidates (S3 / S7),
//   1 = after the distance filter (S8), 2 = after the angle filter (S9).  *n = -1 when the scorer is not run for the pair.
int afis_debug_stage_list(afis_ctx* ctx, const afis_template_view* query, int64_t gidx, int which, int stage,
                          float* sim, int32_t* li, int32_t* ri, int32_t* n)
{
    if (!ctx || !query || !sim || !li || !ri || !n || which < 0 || which > 3 || stage < 0 || stage > 2) return fail(ctx, AFIS_EINVAL, "afis_debug_stage_list: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_debug_stage_list: commit the gallery first");
    if (gidx < 0 || gidx >= ctx->gal.G) return fail(ctx, AFIS_EINVAL, "afis_debug_stage_list: gallery index out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    QueryGroup grp; std::vector<int32_t> st;
    int rc = build_group(ctx, query, 1, grp, st);
    if (rc != AFIS_OK) { grp.release(); return rc; }
    *n = -1;
    DevBuf d_out, d_n;
    auto body = [&]() -> int {
        if (st[0] != AFIS_QUERY_OK) return AFIS_OK;
        const QueryDev& d = grp.dev;
        GalleryDev one = ctx->gal;
        one.G = 1; one.minu_off += gidx; one.minu_tile_off += gidx; one.tex_off += gidx; one.empty += gidx;
        hipStream_t s = ctx->stream;
        HIPCHK(ctx, d_out.ensure(3 * (size_t)kTopTex * sizeof(MinuCand)));
        HIPCHK(ctx, d_n.ensure(3 * 4));
        HIPCHK(ctx, hipMemsetAsync(d_n.p, 0xff, 12, s));
        HIPCHK(ctx, ctx->parts.ensure(16));
        int slot = 0, cap = kTopTex;
        if (which == 0) {
            if (d.n_tiles <= 0) return AFIS_OK;
            HIPCHK(ctx, ctx->rm_val.ensure((size_t)d.lt_pad * 4)); HIPCHK(ctx, ctx->rm_arg.ensure((size_t)d.lt_pad * 4));
            const int av = ctx->adc_variant >= 8 ? 0 : ctx->adc_variant;     // the tap always uses a direct exact kernel (same bits); for the
            { int rcf = ensure_codes_cf(ctx, *ctx, av); if (rcf != AFIS_OK) return rcf; }  // bound + refine variants the plain one, which needs no extra code stream
            if (av == 6 || av == 7) { one.tex_codes_cf = ctx->gal.tex_codes_cf; one.tex_cf_blk = ctx->gal.tex_cf_blk + gidx; }
            { int rcd = direct_rowmax(ctx, d, one, av, 32, nullptr); if (rcd != AFIS_OK) return rcd; }
            HIPCHK(ctx, ctx->tex_slab.ensure(graph_texture_slab_bytes(d.nq)));
            HIPCHK(ctx, launch_graph_texture(d, one, ctx->table.as<float>(), ctx->rm_val.as<float>(), ctx->rm_arg.as<int32_t>(), nullptr, nullptr, ctx->parts.as<float>(), ctx->tex_slab.p, ctx->tex_slab.bytes,
                                             d_out.as<MinuCand>(), d_n.as<int32_t>(), stage | (ctx->s89_tie_order << 8), s));
        } else {
            slot = which - 1; cap = kTopMinu;
            const size_t per_wg = minu_scratch_floats(grp.max_nL, ctx->max_nR, ctx->s3_tie_order);
            HIPCHK(ctx, ctx->scratch.ensure(per_wg * 4 * 64));
            HIPCHK(ctx, ctx->cands.ensure(3 * (size_t)kTopMinu * sizeof(MinuCand))); HIPCHK(ctx, ctx->cand_n.ensure(12)); HIPCHK(ctx, ctx->minu_fb.ensure(minu_fb_ints(3, 1) * 4));
            HIPCHK(ctx, launch_minu_cands(d, one, ctx->scratch.as<float>(), per_wg, 64, ctx->minu_generic | (ctx->s3_tie_order << 1), ctx->cands.as<MinuCand>(), ctx->cand_n.as<int32_t>(), ctx->minu_fb.as<int32_t>(), grp.max_nL, ctx->max_nR, nullptr, s));
            HIPCHK(ctx, ctx->minu_slab.ensure(graph_minutiae_slab_bytes(3ll * d.nq)));
            HIPCHK(ctx, launch_graph_minutiae(d, one, ctx->cands.as<MinuCand>(), ctx->cand_n.as<int32_t>(), ctx->parts.as<float>(), nullptr, nullptr, ctx->minu_slab.p, ctx->minu_slab.bytes,
                                              d_out.as<MinuCand>(), d_n.as<int32_t>(), stage | (ctx->s89_tie_order << 8), s));
        }
        std::vector<MinuCand> h((size_t)3 * kTopTex); int32_t hn[3] = {-1, -1, -1};
        HIPCHK(ctx, hipMemcpyAsync(h.data(), d_out.p, h.size() * sizeof(MinuCand), hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(hn, d_n.p, 12, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (ctx->res_empty[(size_t)gidx]) return AFIS_OK;                   // rolled empty: no scorer runs
        *n = hn[slot];
        for (int t = 0; t < hn[slot]; ++t) { const MinuCand& c = h[(size_t)slot * cap + t]; sim[t] = c.sim; li[t] = c.li; ri[t] = c.ri; }
        return AFIS_OK;
    };
    rc = body();
    d_out.release(); d_n.release(); grp.release();
    return rc;
}


}  // extern "C"
