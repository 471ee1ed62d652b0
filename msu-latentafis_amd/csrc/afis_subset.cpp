// afis_subset.cpp — subset search of the C ABI (include/afis_matcher.h): afis_subset_create gathers a candidate list of the resident shard into a device-resident sub-shard
// of its own (gallery_subset.hip: device to device, only the index list and the offset tables cross PCIe), afis_search_subset / afis_search_subset_resident run the launch
// sequence of a search (afis_search.cpp::search_shard — the same code a full search runs) over it.  A score depends only on its (latent, rolled) pair, so every value is
// bit for bit the full search's value for that pair.
#include "afis_ctx.h"
#include "afis_offsets.h"

using namespace afis;

namespace afis {

void release_subset(afis_subset* s)
{
    if (!s) return;
    free_gallery_dev(&s->sh);
    s->d_global.release(); s->d_pos.release();
    delete s;
}

// the tables of a subset: counted in option gallery_h2d_bytes like every host-to-device copy of the gallery side
template <class T>
static hipError_t upload_counted(afis_ctx* ctx, DevBuf& b, const std::vector<T>& v, hipStream_t s)
{
    const hipError_t e = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
    if (e != hipSuccess || v.empty()) return e;
    ctx->gallery_h2d_bytes += (int64_t)(v.size() * sizeof(T));
    return hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
}

// Everything of afis_subset_create that touches the device; on failure the caller releases the half-made subset.  (afis_search_eligible builds its temporary sub-shards
// through it too, one after the other into the same afis_subset and the same sel_buf: every DevBuf::ensure below then finds room from the second class on.)
int build_subset(afis_ctx* ctx, afis_subset* sub, const std::vector<int32_t>& sel, const std::vector<int64_t>& global, const std::vector<int32_t>& pos, DevBuf* sel_buf)
{
    Shard& sh = sub->sh;
    const int64_t n = sub->n;
    hipStream_t s = ctx->stream;
    std::vector<int32_t> toff, qb, tb;
    int64_t q_blocks = 0, t32 = 0; int max_nR = 0;
    derived_offsets(sh.res_mo, sh.res_to, toff, qb, tb, q_blocks, t32, max_nR);     // the tables a fresh commit of exactly these templates has
    const size_t NM = (size_t)sh.res_mo[(size_t)n], NT = (size_t)sh.res_to[(size_t)n];
    // room first (a failure here has copied nothing), then the tables, then the gather
    struct Arr { DevBuf* dst; const DevBuf* src; int elem; bool minu; };
    const Arr arrs[] = {{&sh.g_minu_des, &ctx->g_minu_des, kDes * 4, true}, {&sh.g_tex_codes, &ctx->g_tex_codes, kM, false}, {&sh.g_minu_xy, &ctx->g_minu_xy, 4, true},
                        {&sh.g_minu_ori, &ctx->g_minu_ori, 4, true}, {&sh.g_tex_xy, &ctx->g_tex_xy, 4, false}, {&sh.g_tex_ori, &ctx->g_tex_ori, 4, false}};
    for (const Arr& a : arrs) HIPCHK(ctx, a.dst->ensure(std::max<size_t>((a.minu ? NM : NT) * (size_t)a.elem, 16)));
    HIPCHK(ctx, sh.g_minu_frag.ensure(std::max<size_t>((size_t)toff[(size_t)n] * 6 * 64 * 16, 16)));
    HIPCHK(ctx, sh.g_task_ctr.ensure(64));
    DevBuf own_sel;
    struct Drop { DevBuf& b; ~Drop() { b.release(); } } drop_sel{own_sel};      // (nothing to release where the caller's buffer is used)
    DevBuf& d_sel = sel_buf ? *sel_buf : own_sel;
    HIPCHK(ctx, upload_counted(ctx, d_sel, sel, s));
    HIPCHK(ctx, upload_counted(ctx, sh.g_minu_off, sh.res_mo, s)); HIPCHK(ctx, upload_counted(ctx, sh.g_tex_off, sh.res_to, s));
    HIPCHK(ctx, upload_counted(ctx, sh.g_minu_tile_off, toff, s)); HIPCHK(ctx, upload_counted(ctx, sh.g_tex_q_blk, qb, s)); HIPCHK(ctx, upload_counted(ctx, sh.g_tex_t32_blk, tb, s));
    HIPCHK(ctx, upload_counted(ctx, sh.g_empty, sh.res_empty, s));
    HIPCHK(ctx, upload_counted(ctx, sub->d_global, global, s));
    if (!sub->identity) HIPCHK(ctx, upload_counted(ctx, sub->d_pos, pos, s));
    // the gather: six launches, HIP events around them (option subset_gather_us)
    Events ev(2);
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    HIPCHK(ctx, hipEventRecord(ev[0], s));
    for (const Arr& a : arrs)
        HIPCHK(ctx, launch_gather_ranges(a.src->p, a.dst->p, a.elem, a.minu ? ctx->g_minu_off.as<int32_t>() : ctx->g_tex_off.as<int32_t>(), d_sel.as<int32_t>(),
                                         a.minu ? sh.g_minu_off.as<int32_t>() : sh.g_tex_off.as<int32_t>(), (int)n, (long long)(a.minu ? NM : NT), s));
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    // the view, and the derived layouts of the default path with the commit's own kernels over the gathered arrays
    GalleryDev& g = sh.gal;
    g.G = (int32_t)n;
    g.minu_off = sh.g_minu_off.as<int32_t>(); g.minu_xy = sh.g_minu_xy.as<short2>(); g.minu_ori = sh.g_minu_ori.as<float>(); g.minu_des = sh.g_minu_des.as<float>();
    g.minu_frag = sh.g_minu_frag.as<float4>(); g.minu_tile_off = sh.g_minu_tile_off.as<int32_t>(); g.tex_off = sh.g_tex_off.as<int32_t>(); g.tex_xy = sh.g_tex_xy.as<short2>();
    g.tex_ori = sh.g_tex_ori.as<float>(); g.tex_codes = sh.g_tex_codes.as<uint4>(); g.tex_codes_cf = nullptr; g.tex_cf_blk = nullptr; g.empty = sh.g_empty.as<uint8_t>();
    g.task_ctr = sh.g_task_ctr.as<int32_t>();
    sh.max_nR = max_nR; sh.q_blocks = q_blocks; sh.t32_tiles = t32; sh.minu_tiles = toff[(size_t)n];
    sh.total_minutiae = (int64_t)NM; sh.total_tex_points = (int64_t)NT;
    sh.index_base = ctx->index_base;
    HIPCHK(ctx, launch_fragment_tiles(sh.g_minu_des.as<float>(), sh.g_minu_off.as<int32_t>(), sh.g_minu_tile_off.as<int32_t>(), (int)n, sh.g_minu_frag.p, s));
    if (ctx->adc_variant == 9) { const int rcg = ensure_mf_gallery(ctx, sh, s); if (rcg != AFIS_OK) return rcg; }     // (another variant: on the subset's first use, as for the shard)
    return wait_elapsed(ctx, "afis_subset_create", ev, &ctx->subset_gather_us);   // (afis_subset_create's quiesce() gave the last search's matrix up already)
}

}  // namespace afis

extern "C" {

int afis_subset_create(afis_ctx* ctx, const int64_t* idx, int64_t n, afis_subset** out)
{
    if (!ctx || !out || n < 0 || (n > 0 && !idx)) return fail(ctx, AFIS_EINVAL, "afis_subset_create: bad argument");
    *out = nullptr;
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_subset_create: commit the gallery first");
    const int64_t G = ctx->gal.G, base = ctx->index_base;
    const int64_t staged = ctx->reopened ? (ctx->pend ? ctx->pend_count : ctx->hg.size()) : 0;
    bool in_staging = false;
    for (int64_t i = 0; i < n; ++i) {
        if (idx[i] >= base && idx[i] < base + G) continue;
        if (idx[i] >= base + G && idx[i] < base + G + staged) { in_staging = true; continue; }
        return fail(ctx, AFIS_EINVAL, "afis_subset_create: gallery index outside this shard");
    }
    if (in_staging) return fail(ctx, AFIS_ESTATE, "afis_subset_create: a listed template is staged but not committed; commit it first");
    // ascending global index order inside the sub-shard; the caller's order is restored on the way out
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [idx](int32_t a, int32_t b) { return idx[a] < idx[b]; });
    for (int64_t t = 1; t < n; ++t)
        if (idx[order[(size_t)t]] == idx[order[(size_t)t - 1]]) return fail(ctx, AFIS_EINVAL, "afis_subset_create: an index is listed twice");
    std::vector<int32_t> sel((size_t)n), pos((size_t)n);
    std::vector<int64_t> global((size_t)n);
    std::unique_ptr<afis_subset> sub(new afis_subset());
    sub->n = n; sub->gallery_epoch = ctx->gallery_epoch; sub->idx.assign(idx, idx + n);
    Shard& sh = sub->sh;
    sh.res_mo.assign((size_t)n + 1, 0); sh.res_to.assign((size_t)n + 1, 0); sh.res_empty.resize((size_t)n);
    int64_t nm = 0, nt = 0;
    for (int64_t t = 0; t < n; ++t) {
        const int32_t j = order[(size_t)t];
        const size_t g = (size_t)(idx[j] - base);
        sel[(size_t)t] = (int32_t)g; global[(size_t)t] = idx[j]; pos[(size_t)j] = (int32_t)t;
        if (j != (int32_t)t) sub->identity = false;
        nm += ctx->res_mo[g + 1] - ctx->res_mo[g]; nt += ctx->res_to[g + 1] - ctx->res_to[g];
        sh.res_mo[(size_t)t + 1] = (int32_t)nm; sh.res_to[(size_t)t + 1] = (int32_t)nt;      // (sums of a part of a shard that passed the commit's 2^31 check)
        sh.res_empty[(size_t)t] = ctx->res_empty[g];
    }
    sub->held = global;
    { const int rcq = quiesce(ctx, "afis_subset_create"); if (rcq != AFIS_OK) return rcq; }
    if (n > 0) {
        const int64_t h2d_before = ctx->gallery_h2d_bytes;
        const int rc = build_subset(ctx, sub.get(), sel, global, pos);
        if (rc != AFIS_OK) {                                                // nothing allocated, nothing changed
            (void)hipStreamSynchronize(ctx->stream);
            ctx->gallery_h2d_bytes = h2d_before;
            release_subset(sub.release());
            return rc;
        }
    } else {
        sh.index_base = base;
        ctx->subset_gather_us = 0;
    }
    ctx->subsets.push_back(sub.get());
    *out = sub.release();
    return AFIS_OK;
}

void afis_subset_free(afis_ctx* ctx, afis_subset* s)
{
    if (!s) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)quiesce(ctx, "afis_subset_free");                             // a search that timed out may still read the sub-shard: bounded wait, as every gallery edit (past its deadline hipFree itself waits for the device)
        ctx->subsets.erase(std::remove(ctx->subsets.begin(), ctx->subsets.end(), s), ctx->subsets.end());
        matrices_lose_subset(ctx, s);                                       // kept matrices of this subset (afis_matrix_keep) are stale from here on
    }
    release_subset(s);
}

int afis_search_subset_resident(afis_ctx* ctx, afis_subset* s, afis_queries* q, float* scores, float* parts, int32_t* status, int k, int64_t* topk_idx, float* topk_score)
{
    if (!ctx || !s || !q) return fail(ctx, AFIS_EINVAL, "afis_search_subset_resident: null argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_search_subset: commit the gallery first");
    if (k < 0 || (k > 0 && (!topk_idx || !topk_score))) return fail(ctx, AFIS_EINVAL, "afis_search_subset: k > 0 needs topk_idx and topk_score");
    if (std::find(ctx->subsets.begin(), ctx->subsets.end(), s) == ctx->subsets.end()) return fail(ctx, AFIS_EINVAL, "afis_search_subset: not a live subset of this context");
    // A subset is a copy of templates of the shard as it was: after an edit the copy may hold a template that has left, and the indices may mean other templates.
    if (s->gallery_epoch != ctx->gallery_epoch)
        return fail_edited(ctx, "afis_search_subset", "this subset was created; free it and create it again");
    // (the launch groups of a handle were cut for the whole shard, G >= n: they fit any subset of the same epoch)
    // (... and those of afis_queries_upload_reserved for a shard of max_templates templates: any subset up to that size, of any epoch)
    AFISCHK(check_query_handle(ctx, "afis_search_subset_resident", q, s->n, true));
    return search_shard(ctx, s->sh, s, q, scores, parts, status, k, topk_idx, topk_score);
}

int afis_search_subset(afis_ctx* ctx, afis_subset* s, const afis_template_view* queries, int n_q, float* scores, float* parts, int32_t* status, int k, int64_t* topk_idx, float* topk_score)
{
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, "afis_search_subset: null argument");
    if (k < 0 || (k > 0 && (!topk_idx || !topk_score))) return fail(ctx, AFIS_EINVAL, "afis_search_subset: k > 0 needs topk_idx and topk_score");
    afis_queries* q = nullptr;
    int rc = afis_queries_upload(ctx, queries, n_q, &q);
    if (rc != AFIS_OK) return rc;
    rc = afis_search_subset_resident(ctx, s, q, scores, parts, status, k, topk_idx, topk_score);
    afis_queries_free(ctx, q);
    return rc;
}

}  // extern "C"
