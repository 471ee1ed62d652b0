// afis_gallery.cpp — the gallery side of the C ABI (include/afis_matcher.h): staging of rolled templates (views, .dat bytes, packed arrays, the AFISGAL1 container),
// the PQ encoder entry points, and afis_gallery_commit: SoA packing, upload through pinned buffers, the device-side derived streams.
// Replaces the per-pair load_FP_template(rolled) of matching/matcher.cpp:173 / :278: parse once, keep the shard resident in HBM.
#include "afis_ctx.h"
#include "afis_offsets.h"
#include "gallery_splice_plan.h"
#include <sys/stat.h>

using namespace afis;

namespace afis {

// the staged gallery as host arrays: a container that afis_gallery_load only mapped is copied into ctx->hg now
int materialise(afis_ctx* ctx)
{
    if (!ctx->pend) return AFIS_OK;
    std::string err;
    HostGallery add;
    if (!copy_from_mapping(*ctx->pend, ctx->pend_first, ctx->pend_count, add, err)) return fail(ctx, AFIS_EFORMAT, "gallery container: " + err);   // from the mapping afis_gallery_load validated: no second open of the path
    ctx->hg = std::move(add);
    ctx->pend.reset(); ctx->pend_first = ctx->pend_count = 0;
    return AFIS_OK;
}

// t->codes == NULL: `encoded` holds the PQ codes the device made from t->des (afis_gallery_add)
void append_entry(HostGallery& hg, const afis_minutiae_view* m, const afis_texture_view* t, const uint8_t* encoded = nullptr)
{
    if (m && m->n > 0) {
        hg.mx.insert(hg.mx.end(), m->x, m->x + m->n); hg.my.insert(hg.my.end(), m->y, m->y + m->n);
        hg.mori.insert(hg.mori.end(), m->ori, m->ori + m->n);
        hg.mdes.insert(hg.mdes.end(), m->des, m->des + (size_t)m->n * kDes);
    }
    hg.minu_off.push_back((int64_t)hg.mx.size());
    if (t && t->n > 0) {
        const int n = std::min(t->n, kTexMax);                              // matcher.cpp:546-547
        hg.tx.insert(hg.tx.end(), t->x, t->x + n); hg.ty.insert(hg.ty.end(), t->y, t->y + n);
        hg.tori.insert(hg.tori.end(), t->ori, t->ori + n);
        const uint8_t* codes = t->codes ? t->codes : encoded;
        hg.tcodes.insert(hg.tcodes.end(), codes, codes + (size_t)n * kM);
    }
    hg.tex_off.push_back((int64_t)hg.tx.size());
    hg.empty.push_back((!(m && m->n > 0) && !(t && t->n > 0)) ? 1 : 0);
}

int check_rolled(afis_ctx* ctx, const afis_template_view& t)
{
    if (t.n_minu < 0 || t.n_tex < 0 || (t.n_minu > 0 && !t.minu) || (t.n_tex > 0 && !t.tex)) return fail(ctx, AFIS_EINVAL, "rolled template: bad view");
    if (t.n_minu > 0) {
        const afis_minutiae_view& m = t.minu[0];
        if (m.n <= 0 || m.n > 2000 || !m.x || !m.y || !m.ori || !m.des) return fail(ctx, AFIS_EINVAL, "rolled minutiae template: bad view (n must be 1..2000)");
        if (m.des_len != kDes) return fail(ctx, AFIS_EINVAL, "rolled minutiae template: des_len must be 96");
    }
    if (t.n_tex > 0) {
        const afis_texture_view& x = t.tex[0];
        if (x.n <= 0 || x.n > 2000 || !x.x || !x.y || !x.ori || (!x.codes && !x.des)) return fail(ctx, AFIS_EINVAL, "rolled texture template: bad view (n must be 1..2000, codes or des required)");
        if (x.codes ? x.des_len != kM : x.des_len != kDes)
            return fail(ctx, AFIS_EINVAL, "rolled texture template: des_len must be 16 with PQ codes, 96 with fp32 descriptors (encoded on the device)");
    }
    return AFIS_OK;
}

void views_of(const HostTemplate& t, std::vector<afis_minutiae_view>& mv, std::vector<afis_texture_view>& tv, afis_template_view& out)
{
    mv.clear(); tv.clear();
    for (const HostMinutiae& m : t.minu) mv.push_back({m.n(), m.x.data(), m.y.data(), m.ori.data(), m.des_len, m.des.data()});
    for (const HostTexture& x : t.tex) tv.push_back({x.n(), x.x.data(), x.y.data(), x.ori.data(), x.des_len, x.des.empty() ? nullptr : x.des.data(), x.codes.empty() ? nullptr : x.codes.data()});
    out.n_minu = (int)mv.size(); out.minu = mv.data(); out.n_tex = (int)tv.size(); out.tex = tv.data();
}

void free_gallery_dev(Shard* c)
{
    c->g_minu_off.release(); c->g_minu_xy.release(); c->g_minu_ori.release(); c->g_minu_des.release(); c->g_minu_frag.release(); c->g_minu_tile_off.release();
    c->g_tex_off.release(); c->g_tex_xy.release(); c->g_tex_ori.release(); c->g_tex_codes.release(); c->g_tex_codes_cf.release(); c->g_tex_cf_blk.release(); c->g_tex_codes_q.release(); c->g_tex_q_blk.release(); c->g_tex_t32_blk.release(); c->g_empty.release(); c->g_task_ctr.release();
    c->g_codes_p.release(); c->g_nrm_p.release(); c->g_tile_meta.release(); c->mf_gal_built = false; c->codes_cf_built = false; c->codes_q_built = false;
}

}  // namespace afis

extern "C" {

int afis_gallery_add(afis_ctx* ctx, const afis_template_view* t, int n)
{
    if (!ctx || (n > 0 && !t)) return fail(ctx, AFIS_EINVAL, "afis_gallery_add: null argument");
    if (ctx->committed && !ctx->reopened) return fail(ctx, AFIS_ESTATE, "afis_gallery_add: gallery already committed (afis_gallery_reopen opens it for more)");
    if (int rc_ = materialise(ctx)) return rc_;
    for (int i = 0; i < n; ++i) { int rc = check_rolled(ctx, t[i]); if (rc) return rc; }
    std::vector<uint8_t> enc;
    for (int i = 0; i < n; ++i) {
        const afis_texture_view* x = t[i].n_tex > 0 ? &t[i].tex[0] : nullptr;
        if (x && !x->codes) {                                               // fp32 descriptors: PQ-encode on the device
            enc.resize((size_t)x->n * kM);
            int rc = afis_pq_encode(ctx, x->des, x->n, enc.data());
            if (rc != AFIS_OK) return rc;
        }
        append_entry(ctx->hg, t[i].n_minu > 0 ? &t[i].minu[0] : nullptr, x, enc.data());
    }
    return AFIS_OK;
}

// PQ encoder: TrainedPQEncoder.encode_multi (extraction/descriptor_PQ.py:19-27) on the device, in slices that fit a fixed
// staging buffer.
int afis_pq_encode(afis_ctx* ctx, const float* des, int64_t n, uint8_t* codes)
{
    if (!ctx || n < 0 || (n > 0 && (!des || !codes))) return fail(ctx, AFIS_EINVAL, "afis_pq_encode: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t slice = 1 << 20;                                          // 1 Mi points = 384 MiB of descriptors per launch
    DevBuf d_des, d_codes;
    int rc = AFIS_OK;
    for (int64_t i0 = 0; i0 < n && rc == AFIS_OK; i0 += slice) {
        const int64_t m = std::min(slice, n - i0);
        if (d_des.ensure((size_t)m * kDes * 4) != hipSuccess || d_codes.ensure((size_t)m * kM) != hipSuccess ||
            hipMemcpyAsync(d_des.p, des + i0 * kDes, (size_t)m * kDes * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            launch_pq_encode(d_des.as<float>(), m, ctx->codewords.as<float>(), d_codes.as<uint8_t>(), ctx->stream) != hipSuccess ||
            hipMemcpyAsync(codes + i0 * kM, d_codes.p, (size_t)m * kM, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = fail(ctx, AFIS_EDEVICE, std::string("afis_pq_encode: ") + hipGetErrorString(hipGetLastError()));
    }
    d_des.release(); d_codes.release();
    return rc;
}

// The rolled branch of descriptor_PQ.py::encode_PQ (:332-349): a template whose texture descriptors are fp32 (the latent
// on-disk layout, descriptor_PQ.py:80-175) is rewritten in the rolled layout (:178-272) with every texture template's
// descriptors replaced by their PQ codes.
int afis_encode_rolled_dat(afis_ctx* ctx, const void* bytes, size_t len, void* out, size_t out_cap, size_t* out_len, int* load_rc)
{
    if (!ctx || !out_len || (len > 0 && !bytes)) return fail(ctx, AFIS_EINVAL, "afis_encode_rolled_dat: bad argument");
    HostTemplate t;
    const int rc = parse_latent_dat(bytes, len, t);
    if (load_rc) *load_rc = rc;
    if (rc < 0) { t.minu.clear(); t.tex.clear(); }
    for (HostTexture& x : t.tex) {
        if (x.des_len != kDes) return fail(ctx, AFIS_EINVAL, "afis_encode_rolled_dat: texture descriptors must be 96-d fp32");
        x.codes.resize((size_t)x.n() * kM);
        const int e = afis_pq_encode(ctx, x.des.data(), x.n(), x.codes.data());
        if (e != AFIS_OK) return e;
        x.des.clear(); x.des_len = kM;
    }
    const std::vector<uint8_t> w = write_rolled_dat(t);
    *out_len = w.size();
    if (!out || out_cap < w.size()) return out ? fail(ctx, AFIS_EINVAL, "afis_encode_rolled_dat: output buffer too small") : AFIS_OK;
    memcpy(out, w.data(), w.size());
    return AFIS_OK;
}

int afis_gallery_add_dat(afis_ctx* ctx, const void* bytes, size_t len, int* load_rc)
{
    if (!ctx) return AFIS_EINVAL;
    if (ctx->committed && !ctx->reopened) return fail(ctx, AFIS_ESTATE, "afis_gallery_add_dat: gallery already committed (afis_gallery_reopen opens it for more)");
    if (int rc_ = materialise(ctx)) return rc_;
    HostTemplate t;
    int rc = parse_rolled_dat(bytes, len, t);
    // matcher.cpp:173-177: a negative code discards the template.  Code 8 (a descriptor length outside 1..192, where the reference overruns a
    // stack buffer) is this parser's own: the cursor is misaligned from there on, so the partial template is discarded too (score -1).
    if (rc < 0 || rc == 8) { t.minu.clear(); t.tex.clear(); }
    if (load_rc) *load_rc = rc;
    std::vector<afis_minutiae_view> mv; std::vector<afis_texture_view> tv; afis_template_view v;
    views_of(t, mv, tv, v);
    int ok = check_rolled(ctx, v);
    if (ok != AFIS_OK) return ok;
    append_entry(ctx->hg, v.n_minu > 0 ? &v.minu[0] : nullptr, v.n_tex > 0 ? &v.tex[0] : nullptr);
    return AFIS_OK;
}

// n rolled .dat files at once: parsed on the host's threads (a 100k-file gallery is 5 GB of parsing: 3.7 s on one thread), appended in order.
int afis_gallery_add_dat_batch(afis_ctx* ctx, const void* const* bytes, const size_t* lens, int64_t n, int* load_rc)
{
    if (!ctx || n < 0 || (n > 0 && (!bytes || !lens))) return fail(ctx, AFIS_EINVAL, "afis_gallery_add_dat_batch: bad argument");
    if (ctx->committed && !ctx->reopened) return fail(ctx, AFIS_ESTATE, "afis_gallery_add_dat_batch: gallery already committed (afis_gallery_reopen opens it for more)");
    if (int rc_ = materialise(ctx)) return rc_;
    std::vector<HostTemplate> ts((size_t)n);
    std::vector<int> rcs((size_t)n, 0);
    parallel_for(n, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            int rc = parse_rolled_dat(bytes[i], lens[i], ts[(size_t)i]);
            if (rc < 0 || rc == 8) { ts[(size_t)i].minu.clear(); ts[(size_t)i].tex.clear(); }     // as afis_gallery_add_dat
            rcs[(size_t)i] = rc;
        }
    });
    std::vector<afis_minutiae_view> mv; std::vector<afis_texture_view> tv; afis_template_view v;
    for (int64_t i = 0; i < n; ++i) {                                      // validate everything before anything is appended
        views_of(ts[(size_t)i], mv, tv, v);
        int ok = check_rolled(ctx, v);
        if (ok != AFIS_OK) return ok;
        if (v.n_tex > 0 && !v.tex[0].codes) return fail(ctx, AFIS_EFORMAT, "afis_gallery_add_dat_batch: rolled texture template without PQ codes");
    }
    // append_entry for all of them at once: the slots follow from the counts, the staged arrays grow once (without a zero-fill) and the templates
    // are copied to their slots by the host's threads (appending one by one was a serial pass over 50 KB per template)
    HostGallery& hg = ctx->hg;
    std::vector<int64_t> mo((size_t)n + 1), to((size_t)n + 1);
    mo[0] = (int64_t)hg.mx.size(); to[0] = (int64_t)hg.tx.size();
    for (int64_t i = 0; i < n; ++i) {
        const HostTemplate& t = ts[(size_t)i];
        mo[(size_t)i + 1] = mo[(size_t)i] + (t.minu.empty() ? 0 : t.minu[0].n());
        to[(size_t)i + 1] = to[(size_t)i] + (t.tex.empty() ? 0 : std::min(t.tex[0].n(), kTexMax));          // matcher.cpp:546-547
    }
    const size_t M = (size_t)mo[(size_t)n], X = (size_t)to[(size_t)n];
    hg.mx.resize(M); hg.my.resize(M); hg.mori.resize(M); hg.mdes.resize(M * kDes);
    hg.tx.resize(X); hg.ty.resize(X); hg.tori.resize(X); hg.tcodes.resize(X * kM);
    parallel_for(n, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const HostTemplate& t = ts[(size_t)i];
            const size_t a = (size_t)mo[(size_t)i], nm = (size_t)(mo[(size_t)i + 1] - mo[(size_t)i]);
            if (nm) {
                const HostMinutiae& m = t.minu[0];
                memcpy(&hg.mx[a], m.x.data(), nm * 2); memcpy(&hg.my[a], m.y.data(), nm * 2); memcpy(&hg.mori[a], m.ori.data(), nm * 4);
                memcpy(&hg.mdes[a * kDes], m.des.data(), nm * kDes * 4);
            }
            const size_t b = (size_t)to[(size_t)i], nt = (size_t)(to[(size_t)i + 1] - to[(size_t)i]);
            if (nt) {
                const HostTexture& x = t.tex[0];
                memcpy(&hg.tx[b], x.x.data(), nt * 2); memcpy(&hg.ty[b], x.y.data(), nt * 2); memcpy(&hg.tori[b], x.ori.data(), nt * 4);
                memcpy(&hg.tcodes[b * kM], x.codes.data(), nt * kM);
            }
        }
    });
    for (int64_t i = 0; i < n; ++i) {
        hg.minu_off.push_back(mo[(size_t)i + 1]); hg.tex_off.push_back(to[(size_t)i + 1]);
        hg.empty.push_back(mo[(size_t)i + 1] == mo[(size_t)i] && to[(size_t)i + 1] == to[(size_t)i] ? 1 : 0);
        if (load_rc) load_rc[i] = rcs[(size_t)i];
    }
    return AFIS_OK;
}

int afis_gallery_reserve(afis_ctx* ctx, int64_t n_templates)
{
    if (!ctx || n_templates < 0) return fail(ctx, AFIS_EINVAL, "afis_gallery_reserve: bad argument");
    if (ctx->committed && !ctx->reopened) return fail(ctx, AFIS_ESTATE, "afis_gallery_reserve: gallery already committed (afis_gallery_reopen opens it for more)");
    if (ctx->pend) return AFIS_OK;                                          // a mapped container is not staged in host arrays at all
    HostGallery& hg = ctx->hg;
    const double have = (double)hg.size();
    if ((double)n_templates <= have) return AFIS_OK;
    const double scale = have > 0 ? (double)n_templates / have * 1.02 : 0;  // 2 % headroom over the running average
    const size_t nm = have > 0 ? (size_t)((double)hg.mx.size() * scale) : (size_t)n_templates * 80;
    const size_t nt = have > 0 ? (size_t)((double)hg.tx.size() * scale) : (size_t)n_templates * 800;
    try {
        hg.mx.reserve(nm); hg.my.reserve(nm); hg.mori.reserve(nm); hg.mdes.reserve(nm * kDes);
        hg.tx.reserve(nt); hg.ty.reserve(nt); hg.tori.reserve(nt); hg.tcodes.reserve(nt * kM);
        hg.minu_off.reserve((size_t)n_templates + 1); hg.tex_off.reserve((size_t)n_templates + 1); hg.empty.reserve((size_t)n_templates);
    } catch (const std::bad_alloc&) { return fail(ctx, AFIS_EINVAL, "afis_gallery_reserve: out of host memory"); }
    return AFIS_OK;
}

int afis_gallery_add_packed(afis_ctx* ctx, int64_t n, const int64_t* minu_off, const int16_t* minu_x, const int16_t* minu_y,
                            const float* minu_ori, const float* minu_des, const int64_t* tex_off, const int16_t* tex_x,
                            const int16_t* tex_y, const float* tex_ori, const uint8_t* tex_codes)
{
    if (!ctx || n < 0 || !minu_off || !tex_off) return fail(ctx, AFIS_EINVAL, "afis_gallery_add_packed: null argument");
    if (ctx->committed && !ctx->reopened) return fail(ctx, AFIS_ESTATE, "afis_gallery_add_packed: gallery already committed (afis_gallery_reopen opens it for more)");
    if (int rc_ = materialise(ctx)) return rc_;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t nm = minu_off[i + 1] - minu_off[i], nt = tex_off[i + 1] - tex_off[i];
        if (nm < 0 || nm > 2000 || nt < 0 || nt > 2000) return fail(ctx, AFIS_EINVAL, "afis_gallery_add_packed: template point count must be 0..2000");
    }
    HostGallery& hg = ctx->hg;
    const int64_t m0 = minu_off[0], m1 = minu_off[n], t0 = tex_off[0];
    hg.mx.insert(hg.mx.end(), minu_x + m0, minu_x + m1); hg.my.insert(hg.my.end(), minu_y + m0, minu_y + m1);
    hg.mori.insert(hg.mori.end(), minu_ori + m0, minu_ori + m1);
    hg.mdes.insert(hg.mdes.end(), minu_des + m0 * kDes, minu_des + m1 * kDes);
    const int64_t mbase = hg.minu_off.back() - m0;
    for (int64_t i = 0; i < n; ++i) {
        hg.minu_off.push_back(minu_off[i + 1] + mbase);
        const int64_t a = tex_off[i], nt = std::min<int64_t>(tex_off[i + 1] - a, kTexMax);
        hg.tx.insert(hg.tx.end(), tex_x + a, tex_x + a + nt); hg.ty.insert(hg.ty.end(), tex_y + a, tex_y + a + nt);
        hg.tori.insert(hg.tori.end(), tex_ori + a, tex_ori + a + nt);
        hg.tcodes.insert(hg.tcodes.end(), tex_codes + a * kM, tex_codes + (a + nt) * kM);
        hg.tex_off.push_back((int64_t)hg.tx.size());
        hg.empty.push_back((minu_off[i + 1] == minu_off[i] && nt == 0) ? 1 : 0);
    }
    (void)t0;
    return AFIS_OK;
}

// ---- packed gallery container (layout in template_io.h) ---------------------------------------------------
int afis_gallery_save(afis_ctx* ctx, const char* path, const char* const* names)
{
    if (!ctx || !path) return fail(ctx, AFIS_EINVAL, "afis_gallery_save: null argument");
    if (ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_gallery_save: the host staging copy is released at commit; save before afis_gallery_commit");
    if (int rc_ = materialise(ctx)) return rc_;
    std::vector<std::string> nm;
    if (names) for (int64_t i = 0; i < ctx->hg.size(); ++i) nm.emplace_back(names[i] ? names[i] : "");
    std::string err;
    if (!write_gallery_container(path, ctx->hg, nm, err)) return fail(ctx, AFIS_EFORMAT, "afis_gallery_save: " + err);
    return AFIS_OK;
}

int afis_gallery_load(afis_ctx* ctx, const char* path, int64_t first, int64_t count)
{
    if (!ctx || !path) return fail(ctx, AFIS_EINVAL, "afis_gallery_load: null argument");
    if (ctx->committed && !ctx->reopened) return fail(ctx, AFIS_ESTATE, "afis_gallery_load: gallery already committed (afis_gallery_reopen opens it for more)");
    std::string err;
    if (ctx->hg.size() == 0 && !ctx->pend) {                               // the usual case (one container, or one shard of it): map it, validate it, read it at the commit
        std::unique_ptr<GalleryMapping> gm = map_gallery_container(path, err);
        if (!gm) return fail(ctx, AFIS_EFORMAT, "afis_gallery_load: " + err);
        if (count < 0) count = gm->G - first;
        if (first < 0 || count < 0 || first + count > gm->G) return fail(ctx, AFIS_EFORMAT, std::string("afis_gallery_load: ") + path + ": template range outside the container");
        for (int64_t i = first; i < first + count; ++i) {
            const int64_t nm = gm->minu_off[i + 1] - gm->minu_off[i], nt = gm->tex_off[i + 1] - gm->tex_off[i];
            if (nm > 2000 || nt > kTexMax || (gm->empty[i] != 0) != (nm == 0 && nt == 0)) return fail(ctx, AFIS_EFORMAT, "afis_gallery_load: template counts out of range");
        }
        ctx->pend = std::move(gm); ctx->pend_first = first; ctx->pend_count = count;
        return AFIS_OK;
    }
    if (int rc_ = materialise(ctx)) return rc_;
    HostGallery add;                                                       // parsed aside so a bad file leaves the staged gallery untouched
    if (!read_gallery_container(path, first, count, add, nullptr, nullptr, err)) return fail(ctx, AFIS_EFORMAT, "afis_gallery_load: " + err);
    const int64_t n = add.size();
    for (int64_t i = 0; i < n; ++i) {
        const int64_t nm = add.minu_off[i + 1] - add.minu_off[i], nt = add.tex_off[i + 1] - add.tex_off[i];
        if (nm > 2000 || nt > kTexMax || (add.empty[i] != 0) != (nm == 0 && nt == 0)) return fail(ctx, AFIS_EFORMAT, "afis_gallery_load: template counts out of range");
    }
    HostGallery& hg = ctx->hg;
    if (hg.size() == 0) { hg = std::move(add); return AFIS_OK; }
    const int64_t mb = hg.minu_off.back(), tb = hg.tex_off.back();
    hg.mx.insert(hg.mx.end(), add.mx.begin(), add.mx.end()); hg.my.insert(hg.my.end(), add.my.begin(), add.my.end());
    hg.mori.insert(hg.mori.end(), add.mori.begin(), add.mori.end()); hg.mdes.insert(hg.mdes.end(), add.mdes.begin(), add.mdes.end());
    hg.tx.insert(hg.tx.end(), add.tx.begin(), add.tx.end()); hg.ty.insert(hg.ty.end(), add.ty.begin(), add.ty.end());
    hg.tori.insert(hg.tori.end(), add.tori.begin(), add.tori.end()); hg.tcodes.insert(hg.tcodes.end(), add.tcodes.begin(), add.tcodes.end());
    for (int64_t i = 0; i < n; ++i) { hg.minu_off.push_back(mb + add.minu_off[i + 1]); hg.tex_off.push_back(tb + add.tex_off[i + 1]); hg.empty.push_back(add.empty[i]); }
    return AFIS_OK;
}

int afis_gallery_file_info(const char* path, int64_t* G, int64_t* n_minutiae, int64_t* n_tex_points, int32_t* tex_counts)
{
    if (!path) return fail(nullptr, AFIS_EINVAL, "afis_gallery_file_info: null argument");
    std::string err;
    GalleryFileInfo info;
    if (!gallery_container_info(path, info, err)) return fail(nullptr, AFIS_EFORMAT, "afis_gallery_file_info: " + err);
    if (G) *G = info.G;
    if (n_minutiae) *n_minutiae = info.n_minu;
    if (n_tex_points) *n_tex_points = info.n_tex;
    if (tex_counts) {
        HostGallery none; std::vector<int32_t> tc;
        if (!read_gallery_container(path, 0, 0, none, nullptr, &tc, err, false)) return fail(nullptr, AFIS_EFORMAT, "afis_gallery_file_info: " + err);
        memcpy(tex_counts, tc.data(), tc.size() * sizeof(int32_t));
    }
    return AFIS_OK;
}

int afis_gallery_file_names(const char* path, int64_t first, int64_t count, char* buf, size_t cap, size_t* need)
{
    if (!path || !need) return fail(nullptr, AFIS_EINVAL, "afis_gallery_file_names: null argument");
    std::string err;
    HostGallery none; std::vector<std::string> names;
    if (!read_gallery_container(path, first, count, none, &names, nullptr, err, false)) return fail(nullptr, AFIS_EFORMAT, "afis_gallery_file_names: " + err);
    size_t total = 0;
    for (const std::string& n : names) total += n.size() + 1;
    *need = total;
    if (!buf) return AFIS_OK;
    if (cap < total) return fail(nullptr, AFIS_EINVAL, "afis_gallery_file_names: buffer too small");
    char* w = buf;
    for (const std::string& n : names) { memcpy(w, n.c_str(), n.size() + 1); w += n.size() + 1; }
    return AFIS_OK;
}

// The arrays of a shard are 50 KB per template (5 GB per 100 000): a pageable hipMemcpy moves them at 8-11 GB/s through the runtime's one staging thread.
// Here they go through two pinned 64 MB buffers: the host's threads fill one (from the staged arrays or straight from a mapped container: that is where
// the page cache is read) while the DMA engine empties the other.
struct PinnedPipe {
    static constexpr size_t kCap = (size_t)64 << 20;
    void* buf[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; bool used[2] = {false, false}; int k = 0;
    size_t direct_below = (size_t)4 << 20;                                 // smaller copies go straight from the caller's memory
    int64_t* h2d = nullptr;                                                // option gallery_h2d_bytes: every host-to-device copy issued through the pipe adds its bytes here
    hipError_t init()
    {
        for (int i = 0; i < 2; ++i) {
            hipError_t e = hipHostMalloc(&buf[i], kCap, hipHostMallocDefault); if (e != hipSuccess) return e;
            e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming); if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    ~PinnedPipe() { for (int i = 0; i < 2; ++i) { if (ev[i]) (void)hipEventDestroy(ev[i]); if (buf[i]) (void)hipHostFree(buf[i]); } }
};

// ... to device memory that is already there (dst): the whole array of a first commit, or the tail an appending commit adds behind the resident part
static hipError_t upload_bulk_at(PinnedPipe& pp, void* dst, const void* src, size_t bytes, hipStream_t s)
{
    hipError_t e = hipSuccess;
    if (bytes == 0) return e;
    if (bytes < pp.direct_below) { if (pp.h2d) *pp.h2d += (int64_t)bytes; return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); }
    if (!pp.buf[1]) { e = pp.init(); if (e != hipSuccess) return e; }       // (an appending commit pins the buffers only when an array is large enough to need them)
    for (size_t off = 0; off < bytes; off += PinnedPipe::kCap) {
        const size_t n = std::min(PinnedPipe::kCap, bytes - off);
        const int slot = pp.k & 1;
        if (pp.used[slot]) { e = hipEventSynchronize(pp.ev[slot]); if (e != hipSuccess) return e; }
        const uint8_t* from = (const uint8_t*)src + off; uint8_t* to = (uint8_t*)pp.buf[slot];
        parallel_for((int64_t)((n + 4095) / 4096), [&](int64_t lo, int64_t hi) { const size_t a = (size_t)lo * 4096, z = std::min(n, (size_t)hi * 4096); memcpy(to + a, from + a, z - a); });
        if (pp.h2d) *pp.h2d += (int64_t)n;
        e = hipMemcpyAsync((uint8_t*)dst + off, pp.buf[slot], n, hipMemcpyHostToDevice, s); if (e != hipSuccess) return e;
        e = hipEventRecord(pp.ev[slot], s); if (e != hipSuccess) return e;
        pp.used[slot] = true; ++pp.k;
    }
    return hipSuccess;
}

static hipError_t upload_bulk(PinnedPipe& pp, DevBuf& b, const void* src, size_t bytes, hipStream_t s)
{
    const hipError_t e = b.ensure(std::max<size_t>(bytes, 16));
    return e != hipSuccess ? e : upload_bulk_at(pp, b.p, src, bytes, s);
}

// The gallery's own host-to-device copies outside the pipe — offset tables, empty flags — counted the same way: by the bytes handed to the copy.
static hipError_t h2d_copy(afis_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return hipSuccess;
    ctx->gallery_h2d_bytes += (int64_t)bytes;
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
}
static hipError_t upload_table(afis_ctx* ctx, DevBuf& b, const std::vector<int32_t>& v, hipStream_t s)
{
    const hipError_t e = b.ensure(std::max<size_t>(v.size() * sizeof(int32_t), 16));
    return e != hipSuccess ? e : h2d_copy(ctx, b.p, v.data(), v.size() * sizeof(int32_t), s);
}
static int commit_shard(afis_ctx* ctx, int64_t index_base);
static int append_shard(afis_ctx* ctx);
static void release_staging(afis_ctx* ctx);

// A failed commit leaves the context as it was before the call: not committed, no half-uploaded shard on the device, the staged templates (host arrays or the mapped
// container) still in place, so that the caller may retry or destroy.
int afis_gallery_commit(afis_ctx* ctx, int64_t index_base)
{
    if (!ctx) return AFIS_EINVAL;
    if (ctx->committed && !ctx->reopened) return fail(ctx, AFIS_ESTATE, "afis_gallery_commit: already committed (afis_gallery_reopen opens the gallery for more)");
    if (ctx->committed) {                                                   // reopened: the staged templates go behind the resident shard, which is not uploaded again
        if (index_base != ctx->index_base) return fail(ctx, AFIS_EINVAL, "afis_gallery_commit: index_base differs from the resident shard's");
        return append_shard(ctx);                                           // a failure leaves the resident shard searchable and the staged templates in place
    }
    const int rc = commit_shard(ctx, index_base);
    if (rc != AFIS_OK) {
        ctx->committed = false;
        (void)hipStreamSynchronize(ctx->stream);
        free_gallery_dev(ctx);
        ctx->gal = GalleryDev();
    }
    return rc;
}

static int commit_shard(afis_ctx* ctx, int64_t index_base)
{
    // The staged shard as plain arrays: ctx->hg, or the mapped container's range (offsets rebased to the shard's first point).
    HostGallery& hg = ctx->hg;
    const GalleryMapping* gm = ctx->pend.get();
    const int64_t G = gm ? ctx->pend_count : hg.size();
    const int64_t* src_mo = gm ? gm->minu_off + ctx->pend_first : hg.minu_off.data();
    const int64_t* src_to = gm ? gm->tex_off + ctx->pend_first : hg.tex_off.data();
    const int64_t m0 = src_mo[0], t0 = src_to[0];
    const size_t NM = (size_t)(src_mo[G] - m0), NT = (size_t)(src_to[G] - t0);
    const int16_t* s_mx = gm ? gm->mx + m0 : hg.mx.data(); const int16_t* s_my = gm ? gm->my + m0 : hg.my.data();
    const float* s_mori = gm ? gm->mori + m0 : hg.mori.data(); const float* s_mdes = gm ? gm->mdes + (size_t)m0 * kDes : hg.mdes.data();
    const int16_t* s_tx = gm ? gm->tx + t0 : hg.tx.data(); const int16_t* s_ty = gm ? gm->ty + t0 : hg.ty.data();
    const float* s_tori = gm ? gm->tori + t0 : hg.tori.data(); const uint8_t* s_tcodes = gm ? gm->tcodes + (size_t)t0 * kM : hg.tcodes.data();
    const uint8_t* s_empty = gm ? gm->empty + ctx->pend_first : hg.empty.data();
    if (G > 0x7fffffff / 8 || NM > 0x7fffffffull || NT > 0x7fffffffull)
        return fail(ctx, AFIS_EINVAL, "afis_gallery_commit: shard too large for 32-bit point offsets; split the gallery into more shards");
    if (gm && gm->fd_ >= 0) {                                               // the arrays are read straight from the mapping, by several threads: a file truncated since afis_gallery_load would fault.  This check catches a truncation that
                                                                            // happened BEFORE the commit; one that happens while the copy below runs still faults (SIGBUS): a container must not be modified while a context has it loaded (include/afis_matcher.h says so)
        struct stat st;
        if (fstat(gm->fd_, &st) != 0 || (size_t)st.st_size < gm->len_) return fail(ctx, AFIS_EFORMAT, "gallery container: " + gm->path + " was truncated after it was loaded");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool clock_it = getenv("AFIS_COMMIT_TIMING") != nullptr;           // development aid: where the commit's time goes, on stderr
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_prev = now();
    auto lap = [&](const char* what) { if (clock_it) { (void)hipStreamSynchronize(ctx->stream); const double t = now(); fprintf(stderr, "commit: %-28s %8.1f ms\n", what, t - t_prev); t_prev = t; } };
    PinnedPipe pp;
    pp.h2d = &ctx->gallery_h2d_bytes;
    HIPCHK(ctx, pp.init());
    lap("pinned buffers");
    std::vector<int32_t> mo(G + 1), to(G + 1), toff, qb, tb;
    int max_nR = 0;
    for (int64_t i = 0; i <= G; ++i) { mo[i] = (int32_t)(src_mo[i] - m0); to[i] = (int32_t)(src_to[i] - t0); }
    // tile offsets of the descriptor fragments (16 descriptors), block offsets of the quantised path's code stream (64 points; made on first use), tile offsets of the
    // matrix-core bound pass's stream (32 points): one routine for the commit and the edits, so that an edited shard's tables are a fresh commit's
    int64_t n_q_blocks = 0, n_t32 = 0;
    derived_offsets(mo, to, toff, qb, tb, n_q_blocks, n_t32, max_nR);
    if (n_t32 > 0x7fffffff / 32) return fail(ctx, AFIS_EINVAL, "afis_gallery_commit: shard too large for the bound pass's code stream; split the gallery into more shards");
    HIPCHK(ctx, upload_bulk(pp, ctx->g_minu_des, s_mdes, NM * kDes * sizeof(float), ctx->stream));     // the big one first: the fragment kernel below runs while the rest is uploaded
    lap("minutiae descriptors");
    HIPCHK(ctx, upload_table(ctx, ctx->g_minu_off, mo, ctx->stream));
    {   // the descriptors as MFMA operand fragments: laid out on the device from the descriptors just uploaded (round 3 transposed them on the host and uploaded another 34 KB per template)
        HIPCHK(ctx, upload_table(ctx, ctx->g_minu_tile_off, toff, ctx->stream));
        HIPCHK(ctx, ctx->g_minu_frag.ensure(std::max<size_t>((size_t)toff[(size_t)G] * 6 * 64 * 16, 16)));
        HIPCHK(ctx, launch_fragment_tiles(ctx->g_minu_des.as<float>(), ctx->g_minu_off.as<int32_t>(), ctx->g_minu_tile_off.as<int32_t>(), (int)G, ctx->g_minu_frag.p, ctx->stream));
    }
    lap("fragment tiles");
    std::vector<short2> mxy(NM), txy(NT);
    parallel_for((int64_t)NM, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) mxy[(size_t)i] = make_short2(s_mx[i], s_my[i]); });
    parallel_for((int64_t)NT, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) txy[(size_t)i] = make_short2(s_tx[i], s_ty[i]); });
    lap("xy packing");
    HIPCHK(ctx, upload_bulk(pp, ctx->g_minu_xy, mxy.data(), NM * sizeof(short2), ctx->stream));
    HIPCHK(ctx, upload_bulk(pp, ctx->g_minu_ori, s_mori, NM * sizeof(float), ctx->stream));
    HIPCHK(ctx, upload_table(ctx, ctx->g_tex_off, to, ctx->stream));
    HIPCHK(ctx, upload_bulk(pp, ctx->g_tex_xy, txy.data(), NT * sizeof(short2), ctx->stream));
    HIPCHK(ctx, upload_bulk(pp, ctx->g_tex_ori, s_tori, NT * sizeof(float), ctx->stream));
    lap("small arrays");
    HIPCHK(ctx, upload_bulk(pp, ctx->g_tex_codes, s_tcodes, NT * kM, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    lap("texture codes");
    ctx->q_blocks = n_q_blocks; ctx->t32_tiles = n_t32;
    HIPCHK(ctx, upload_table(ctx, ctx->g_tex_q_blk, qb, ctx->stream)); HIPCHK(ctx, upload_table(ctx, ctx->g_tex_t32_blk, tb, ctx->stream));
    { DevBuf& eb = ctx->g_empty; HIPCHK(ctx, eb.ensure(std::max<size_t>((size_t)G, 16))); HIPCHK(ctx, h2d_copy(ctx, eb.p, s_empty, (size_t)G, ctx->stream)); }
    HIPCHK(ctx, ctx->g_task_ctr.ensure(64));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    GalleryDev& g = ctx->gal;
    g.G = (int32_t)G;
    g.minu_off = ctx->g_minu_off.as<int32_t>(); g.minu_xy = ctx->g_minu_xy.as<short2>(); g.minu_ori = ctx->g_minu_ori.as<float>();
    g.minu_des = ctx->g_minu_des.as<float>(); g.minu_frag = ctx->g_minu_frag.as<float4>(); g.minu_tile_off = ctx->g_minu_tile_off.as<int32_t>(); g.tex_off = ctx->g_tex_off.as<int32_t>(); g.tex_xy = ctx->g_tex_xy.as<short2>();
    g.tex_ori = ctx->g_tex_ori.as<float>(); g.tex_codes = ctx->g_tex_codes.as<uint4>(); g.tex_codes_cf = nullptr; g.tex_cf_blk = nullptr; g.empty = ctx->g_empty.as<uint8_t>();
    g.task_ctr = ctx->g_task_ctr.as<int32_t>();
    ctx->max_nR = max_nR;
    ctx->total_tex_points = (int64_t)NT; ctx->total_minutiae = (int64_t)NM;
    ctx->index_base = index_base;
    ctx->committed = true;
    ++ctx->gallery_epoch;                                                   // (no handle can exist before a first commit; one may after a removal that failed and dropped the shard)
    if (ctx->adc_variant == 9 && G > 0) {                                    // the default path's derived streams belong to the resident gallery: built here, not by the first search
        int rcg = ensure_mf_gallery(ctx, *ctx, ctx->stream);
        if (rcg != AFIS_OK) return rcg;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        lap("bound pass's code stream");
    }
    // what the host keeps of the resident shard: the empty flags and the offsets (a later edit rewrites the offset tables from them)
    ctx->res_empty.assign(s_empty, s_empty + G);
    ctx->minu_tiles = toff[(size_t)G];
    ctx->res_mo = std::move(mo); ctx->res_to = std::move(to);
    lap("offset tables");
    release_staging(ctx);
    lap("staging released");
    return AFIS_OK;
}

// the host staging copy (arrays or mapping) is no longer needed
static void release_staging(afis_ctx* ctx)
{
    HostGallery& hg = ctx->hg;
    if (hg.mdes.capacity() > ((size_t)16 << 20)) {                           // a large staging copy is released by a thread of its own
        // The pages go back in 32 MB pieces (madvise takes the address-space lock shared and briefly); one munmap of 3 GB holds it exclusively for
        // a third of a second, and every allocation the caller makes next — the commit's own clean-up, the first search — would wait for it.
        HostGallery* old = new HostGallery(std::move(ctx->hg));
        // (an earlier commit's thread may still be at work — an append right behind a 5 GB commit — and is waited for by the new one, not by the caller)
        std::thread earlier = std::move(ctx->staging_reaper);
        ctx->staging_reaper = std::thread([old, prev = std::move(earlier)]() mutable {
            if (prev.joinable()) prev.join();
            std::vector<std::pair<uintptr_t, size_t>> pieces;
            auto drop = [&](void* p, size_t bytes) {
                const uintptr_t a = ((uintptr_t)p + 4095) & ~(uintptr_t)4095, z = ((uintptr_t)p + bytes) & ~(uintptr_t)4095;
                for (uintptr_t q = a; q < z; q += (uintptr_t)32 << 20) pieces.emplace_back(q, (size_t)std::min<uintptr_t>((uintptr_t)32 << 20, z - q));
            };
            drop(old->mdes.data(), old->mdes.capacity() * sizeof(float)); drop(old->tcodes.data(), old->tcodes.capacity());
            drop(old->mori.data(), old->mori.capacity() * 4); drop(old->tori.data(), old->tori.capacity() * 4);
            std::atomic<size_t> next{0};
            auto work = [&]() { for (size_t i = next.fetch_add(1); i < pieces.size(); i = next.fetch_add(1)) (void)madvise((void*)pieces[i].first, pieces[i].second, MADV_DONTNEED); };
            std::thread helpers[3];                                          // four threads return 5 GB in a quarter of the time one takes
            for (std::thread& h : helpers) h = std::thread(work);
            work();
            for (std::thread& h : helpers) h.join();
            delete old;
        });
    }
    ctx->hg = HostGallery();
    ctx->pend.reset(); ctx->pend_first = ctx->pend_count = 0;
}

// ---- the live gallery: afis_gallery_reopen, the appending commit, afis_gallery_remove, afis_gallery_commit_at, afis_gallery_export ---------------------------------
// An edit replaces device buffers that searches read: nothing of the context may be running.  The search that timed out (if any) first, then all three streams.
// (afis_subset_create / afis_subset_free wait the same way: afis_subset.cpp)
}  // extern "C"
namespace afis {
int quiesce(afis_ctx* ctx, const char* what, bool keep_last_search)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    { const int rcd = drain_abandoned(ctx, keep_last_search); if (rcd != AFIS_OK) return rcd; }
    return wait_streams(ctx, {ctx->stream_lo, ctx->stream_hi, ctx->stream}, what);
}
}  // namespace afis
extern "C" {

// the SoA pointers of ctx->gal from the buffers that hold them now (a buffer that grew or was compacted has moved)
static void refresh_gallery_view(afis_ctx* ctx)
{
    GalleryDev& g = ctx->gal;
    g.minu_off = ctx->g_minu_off.as<int32_t>(); g.minu_xy = ctx->g_minu_xy.as<short2>(); g.minu_ori = ctx->g_minu_ori.as<float>();
    g.minu_des = ctx->g_minu_des.as<float>(); g.minu_frag = ctx->g_minu_frag.as<float4>(); g.minu_tile_off = ctx->g_minu_tile_off.as<int32_t>(); g.tex_off = ctx->g_tex_off.as<int32_t>(); g.tex_xy = ctx->g_tex_xy.as<short2>();
    g.tex_ori = ctx->g_tex_ori.as<float>(); g.tex_codes = ctx->g_tex_codes.as<uint4>(); g.empty = ctx->g_empty.as<uint8_t>();
}

// the streams laid out on first use belong to the shard they were made from
static void invalidate_lazy_streams(afis_ctx* ctx)
{
    ctx->codes_q_built = false; ctx->codes_cf_built = false;
    ctx->gal.tex_codes_cf = nullptr; ctx->gal.tex_cf_blk = nullptr;
}

// DevBuf::ensure frees before it allocates; the resident part must survive: the new buffer first (with headroom: one capacity copy per eighth of growth), a device-to-device
// copy of the `used` bytes, then the old buffer goes.  On failure the old buffer is untouched.
static hipError_t grow_keep(DevBuf& b, size_t used, size_t need, hipStream_t s)
{
    if (need <= b.bytes) return hipSuccess;
    const size_t cap = (need + need / 8 + 255) & ~(size_t)255;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, cap);
    if (e != hipSuccess) return e;
    if (used > 0) e = hipMemcpyAsync(p, b.p, used, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(p); return e; }
    if (b.p) (void)hipFree(b.p);
    b.p = p; b.bytes = cap;
    return hipSuccess;
}

struct TableSet {                                                           // offset tables written aside, swapped in when everything else has succeeded
    DevBuf minu_off, tile_off, tex_off, q_blk, t32_blk;
    ~TableSet() { minu_off.release(); tile_off.release(); tex_off.release(); q_blk.release(); t32_blk.release(); }
};

int afis_gallery_reopen(afis_ctx* ctx)
{
    if (!ctx) return AFIS_EINVAL;
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_gallery_reopen: commit the gallery first");
    ctx->reopened = true;                                                   // (again on a reopened gallery: nothing changes, what is staged stays)
    return AFIS_OK;
}

// afis_gallery_commit on a reopened gallery.  Order: (1) every array grows to hold the sum — the resident bytes are copied on the device, never uploaded; (2) the staged
// points go behind them; (3) the offset tables of the whole shard are written into buffers of their own; (4) fragment tiles and the bound pass's tiles are laid out
// for the new templates only; (5) the tables and the counters are switched.  Up to (5) the resident shard is what it was: a failure returns with it searchable.
static int append_shard(afis_ctx* ctx)
{
    HostGallery& hg = ctx->hg;
    const GalleryMapping* gm = ctx->pend.get();
    const int64_t Gn = gm ? ctx->pend_count : hg.size();
    const int64_t G0 = ctx->gal.G, G1 = G0 + Gn;
    const int64_t* src_mo = gm ? gm->minu_off + ctx->pend_first : hg.minu_off.data();
    const int64_t* src_to = gm ? gm->tex_off + ctx->pend_first : hg.tex_off.data();
    const int64_t m0 = src_mo[0], t0 = src_to[0];
    const size_t NMn = (size_t)(src_mo[Gn] - m0), NTn = (size_t)(src_to[Gn] - t0);
    const size_t NM0 = (size_t)ctx->total_minutiae, NT0 = (size_t)ctx->total_tex_points, NM1 = NM0 + NMn, NT1 = NT0 + NTn;
    const int16_t* s_mx = gm ? gm->mx + m0 : hg.mx.data(); const int16_t* s_my = gm ? gm->my + m0 : hg.my.data();
    const float* s_mori = gm ? gm->mori + m0 : hg.mori.data(); const float* s_mdes = gm ? gm->mdes + (size_t)m0 * kDes : hg.mdes.data();
    const int16_t* s_tx = gm ? gm->tx + t0 : hg.tx.data(); const int16_t* s_ty = gm ? gm->ty + t0 : hg.ty.data();
    const float* s_tori = gm ? gm->tori + t0 : hg.tori.data(); const uint8_t* s_tcodes = gm ? gm->tcodes + (size_t)t0 * kM : hg.tcodes.data();
    const uint8_t* s_empty = gm ? gm->empty + ctx->pend_first : hg.empty.data();
    if (G1 > 0x7fffffff / 8 || NM1 > 0x7fffffffull || NT1 > 0x7fffffffull)
        return fail(ctx, AFIS_EINVAL, "afis_gallery_commit: shard too large for 32-bit point offsets; split the gallery into more shards");
    if (gm && gm->fd_ >= 0) {
        struct stat st;
        if (fstat(gm->fd_, &st) != 0 || (size_t)st.st_size < gm->len_) return fail(ctx, AFIS_EFORMAT, "gallery container: " + gm->path + " was truncated after it was loaded");
    }
    if (Gn == 0) { release_staging(ctx); ctx->reopened = false; return AFIS_OK; }      // nothing staged: the shard is what it was
    std::vector<int32_t> mo((size_t)G1 + 1), to((size_t)G1 + 1), toff, qb, tb;
    std::copy(ctx->res_mo.begin(), ctx->res_mo.end(), mo.begin()); std::copy(ctx->res_to.begin(), ctx->res_to.end(), to.begin());
    for (int64_t i = 1; i <= Gn; ++i) { mo[(size_t)(G0 + i)] = (int32_t)((int64_t)NM0 + src_mo[i] - m0); to[(size_t)(G0 + i)] = (int32_t)((int64_t)NT0 + src_to[i] - t0); }
    int64_t q_blocks = 0, t32 = 0; int max_nR = 0;
    derived_offsets(mo, to, toff, qb, tb, q_blocks, t32, max_nR);
    if (t32 > 0x7fffffff / 32) return fail(ctx, AFIS_EINVAL, "afis_gallery_commit: shard too large for the bound pass's code stream; split the gallery into more shards");
    { const int rcq = quiesce(ctx, "afis_gallery_commit"); if (rcq != AFIS_OK) return rcq; }
    hipStream_t s = ctx->stream;
    const bool clock_it = getenv("AFIS_COMMIT_TIMING") != nullptr;           // development aid, as in commit_shard
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_prev = now();
    auto lap = [&](const char* what) { if (clock_it) { (void)hipStreamSynchronize(s); const double t = now(); fprintf(stderr, "append: %-28s %8.1f ms\n", what, t - t_prev); t_prev = t; } };
    const size_t tiles0 = (size_t)ctx->minu_tiles, tiles1 = (size_t)toff[(size_t)G1], t32_0 = (size_t)ctx->t32_tiles;
    const size_t kFragTile = 6 * 64 * 16;
    // (1) room for the sum
    struct Grow { DevBuf* b; size_t used, need; bool bound_pass; };          // bound_pass: the matrix-core pass's stream, which may not exist yet (its first use then lays out the whole shard)
    const Grow grows[] = {
        {&ctx->g_minu_des, NM0 * kDes * 4, NM1 * kDes * 4, false}, {&ctx->g_minu_frag, tiles0 * kFragTile, tiles1 * kFragTile, false}, {&ctx->g_tex_codes, NT0 * kM, NT1 * kM, false},
        {&ctx->g_minu_xy, NM0 * 4, NM1 * 4, false}, {&ctx->g_minu_ori, NM0 * 4, NM1 * 4, false}, {&ctx->g_tex_xy, NT0 * 4, NT1 * 4, false}, {&ctx->g_tex_ori, NT0 * 4, NT1 * 4, false},
        {&ctx->g_empty, (size_t)G0, (size_t)G1, false},
        {&ctx->g_codes_p, t32_0 * 32 * 16, (size_t)t32 * 32 * 16, true}, {&ctx->g_nrm_p, t32_0 * 32 * 4, (size_t)t32 * 32 * 4, true}, {&ctx->g_tile_meta, t32_0 * 8, (size_t)t32 * 8, true},
    };
    for (const Grow& gr : grows) {
        if (gr.bound_pass && !ctx->mf_gal_built) continue;
        const hipError_t e = grow_keep(*gr.b, gr.used, std::max<size_t>(gr.need, 16), s);
        refresh_gallery_view(ctx);                                          // (the resident part has moved with its buffer)
        HIPCHK(ctx, e);
    }
    lap("capacity");
    // (2) the staged points behind the resident ones.  Pinning the pipe's 128 MB costs more than a pageable copy of a few thousand templates takes: arrays below 256 MB go directly.
    PinnedPipe pp;
    pp.h2d = &ctx->gallery_h2d_bytes;
    pp.direct_below = (size_t)256 << 20;
    HIPCHK(ctx, upload_bulk_at(pp, ctx->g_minu_des.as<uint8_t>() + NM0 * kDes * 4, s_mdes, NMn * kDes * 4, s));
    std::vector<short2> mxy(NMn), txy(NTn);
    parallel_for((int64_t)NMn, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) mxy[(size_t)i] = make_short2(s_mx[i], s_my[i]); });
    parallel_for((int64_t)NTn, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) txy[(size_t)i] = make_short2(s_tx[i], s_ty[i]); });
    HIPCHK(ctx, upload_bulk_at(pp, ctx->g_minu_xy.as<uint8_t>() + NM0 * 4, mxy.data(), NMn * 4, s));
    HIPCHK(ctx, upload_bulk_at(pp, ctx->g_minu_ori.as<uint8_t>() + NM0 * 4, s_mori, NMn * 4, s));
    HIPCHK(ctx, upload_bulk_at(pp, ctx->g_tex_xy.as<uint8_t>() + NT0 * 4, txy.data(), NTn * 4, s));
    HIPCHK(ctx, upload_bulk_at(pp, ctx->g_tex_ori.as<uint8_t>() + NT0 * 4, s_tori, NTn * 4, s));
    HIPCHK(ctx, upload_bulk_at(pp, ctx->g_tex_codes.as<uint8_t>() + NT0 * kM, s_tcodes, NTn * kM, s));
    HIPCHK(ctx, h2d_copy(ctx, ctx->g_empty.as<uint8_t>() + G0, s_empty, (size_t)Gn, s));
    lap("new points");
    // (3) the offset tables of the whole shard, aside
    TableSet nt;
    HIPCHK(ctx, upload_table(ctx, nt.minu_off, mo, s)); HIPCHK(ctx, upload_table(ctx, nt.tile_off, toff, s)); HIPCHK(ctx, upload_table(ctx, nt.tex_off, to, s));
    HIPCHK(ctx, upload_table(ctx, nt.q_blk, qb, s)); HIPCHK(ctx, upload_table(ctx, nt.t32_blk, tb, s));
    // (4) the derived layouts of the new templates: views whose CSR bases are shifted to the first of them (offsets are absolute)
    HIPCHK(ctx, launch_fragment_tiles(ctx->g_minu_des.as<float>(), nt.minu_off.as<int32_t>() + G0, nt.tile_off.as<int32_t>() + G0, (int)Gn, ctx->g_minu_frag.p, s));
    if (ctx->mf_gal_built) {
        GalleryDev v = ctx->gal;
        v.G = (int32_t)G1; v.tex_off = nt.tex_off.as<int32_t>();
        HIPCHK(ctx, launch_mf_tiles(v, nt.t32_blk.as<int32_t>(), ctx->mf_cwn.as<float>(), ctx->g_codes_p.p, ctx->g_nrm_p.as<float>(), ctx->g_tile_meta.p, s, (int)G0, (int)Gn));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    lap("tables and derived layouts");
    // (5) the switch
    std::swap(ctx->g_minu_off, nt.minu_off); std::swap(ctx->g_minu_tile_off, nt.tile_off); std::swap(ctx->g_tex_off, nt.tex_off);
    std::swap(ctx->g_tex_q_blk, nt.q_blk); std::swap(ctx->g_tex_t32_blk, nt.t32_blk);
    refresh_gallery_view(ctx);
    ctx->gal.G = (int32_t)G1;
    ctx->max_nR = max_nR; ctx->q_blocks = q_blocks; ctx->t32_tiles = t32; ctx->minu_tiles = (int64_t)tiles1;
    ctx->total_minutiae = (int64_t)NM1; ctx->total_tex_points = (int64_t)NT1;
    ctx->res_empty.insert(ctx->res_empty.end(), s_empty, s_empty + Gn);
    ctx->res_mo = std::move(mo); ctx->res_to = std::move(to);
    invalidate_lazy_streams(ctx);
    ++ctx->gallery_epoch;
    release_staging(ctx);
    ctx->reopened = false;
    lap("switch, staging released");
    return AFIS_OK;
}

int afis_gallery_remove(afis_ctx* ctx, const int64_t* idx, int64_t n)
{
    if (!ctx || n < 0 || (n > 0 && !idx)) return fail(ctx, AFIS_EINVAL, "afis_gallery_remove: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_gallery_remove: commit the gallery first");
    if (ctx->reopened && (ctx->pend ? ctx->pend_count : ctx->hg.size()) > 0)
        return fail(ctx, AFIS_ESTATE, "afis_gallery_remove: templates are staged; commit them first");
    const int64_t G = ctx->gal.G;
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < ctx->index_base || idx[i] >= ctx->index_base + G) return fail(ctx, AFIS_EINVAL, "afis_gallery_remove: gallery index outside this shard");
    std::vector<uint8_t> gone((size_t)G, 0);
    bool any = false;
    for (int64_t i = 0; i < n; ++i) { const size_t g = (size_t)(idx[i] - ctx->index_base); if (!ctx->res_empty[g]) { gone[g] = 1; any = true; } }
    if (!any) return AFIS_OK;                                               // only empty entries listed: nothing to do
    std::vector<int32_t> mo((size_t)G + 1, 0), to((size_t)G + 1, 0), toff, qb, tb;
    for (size_t t = 0; t < (size_t)G; ++t) {
        mo[t + 1] = mo[t] + (gone[t] ? 0 : ctx->res_mo[t + 1] - ctx->res_mo[t]);
        to[t + 1] = to[t] + (gone[t] ? 0 : ctx->res_to[t + 1] - ctx->res_to[t]);
    }
    int64_t q_blocks = 0, t32 = 0; int max_nR = 0;
    derived_offsets(mo, to, toff, qb, tb, q_blocks, t32, max_nR);
    std::vector<uint8_t> empty = ctx->res_empty;
    for (size_t t = 0; t < (size_t)G; ++t) if (gone[t]) empty[t] = 1;
    { const int rcq = quiesce(ctx, "afis_gallery_remove"); if (rcq != AFIS_OK) return rcq; }
    hipStream_t s = ctx->stream;
    const int64_t NM1 = mo[(size_t)G], NT1 = to[(size_t)G];
    // the parity tap afis_debug_compact_stats: device time of the compaction kernels of this call (HIP events around each launch) and the bytes they copied
    double compact_us = 0; int64_t compact_bytes = 0;
    hipEvent_t ev_c[2] = {nullptr, nullptr};
    for (hipEvent_t& e : ev_c) HIPCHK(ctx, hipEventCreate(&e));
    bool touched = false;                                                   // an array has been replaced: from here on a failure cannot leave the old shard behind
    auto body = [&]() -> int {
        TableSet nt;                                                        // the new CSR offsets beside the old ones: the compaction reads both
        HIPCHK(ctx, upload_table(ctx, nt.minu_off, mo, s)); HIPCHK(ctx, upload_table(ctx, nt.tex_off, to, s));
        // One array at a time into a buffer of its new size, the old one released before the next: the transient memory is the largest array's, and that one goes first —
        // when its buffer can be had, the smaller ones that follow fit into what it has just given back.
        struct Arr { DevBuf* b; int elem; bool minu; };
        const Arr arrs[] = {{&ctx->g_minu_des, kDes * 4, true}, {&ctx->g_tex_codes, kM, false}, {&ctx->g_minu_xy, 4, true}, {&ctx->g_minu_ori, 4, true}, {&ctx->g_tex_xy, 4, false}, {&ctx->g_tex_ori, 4, false}};
        for (const Arr& a : arrs) {
            const int64_t n_new = a.minu ? NM1 : NT1;
            DevBuf fresh;
            HIPCHK(ctx, fresh.ensure(std::max<size_t>((size_t)n_new * (size_t)a.elem, 16)));
            hipError_t e = hipEventRecord(ev_c[0], s);
            if (e == hipSuccess) e = launch_compact_ranges(a.b->p, fresh.p, a.elem, a.minu ? ctx->g_minu_off.as<int32_t>() : ctx->g_tex_off.as<int32_t>(),
                                                 a.minu ? nt.minu_off.as<int32_t>() : nt.tex_off.as<int32_t>(), (int)G, n_new, s);
            if (e == hipSuccess) e = hipEventRecord(ev_c[1], s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            float ms = 0;
            if (e == hipSuccess && n_new > 0) e = hipEventElapsedTime(&ms, ev_c[0], ev_c[1]);
            if (e != hipSuccess) { fresh.release(); HIPCHK(ctx, e); }
            compact_us += (double)ms * 1e3; compact_bytes += n_new * a.elem;
            std::swap(*a.b, fresh); fresh.release();
            touched = true;
            refresh_gallery_view(ctx);
        }
        std::swap(ctx->g_minu_off, nt.minu_off); std::swap(ctx->g_tex_off, nt.tex_off);
        HIPCHK(ctx, upload_table(ctx, ctx->g_minu_tile_off, toff, s)); HIPCHK(ctx, upload_table(ctx, ctx->g_tex_q_blk, qb, s)); HIPCHK(ctx, upload_table(ctx, ctx->g_tex_t32_blk, tb, s));      // ([G + 1] as before: written in place)
        HIPCHK(ctx, h2d_copy(ctx, ctx->g_empty.p, empty.data(), (size_t)G, s));
        refresh_gallery_view(ctx);
        // the derived layouts, from the compacted arrays into the buffers they already have (they only shrink)
        HIPCHK(ctx, launch_fragment_tiles(ctx->g_minu_des.as<float>(), ctx->g_minu_off.as<int32_t>(), ctx->g_minu_tile_off.as<int32_t>(), (int)G, ctx->g_minu_frag.p, s));
        if (ctx->mf_gal_built)
            HIPCHK(ctx, launch_mf_tiles(ctx->gal, ctx->g_tex_t32_blk.as<int32_t>(), ctx->mf_cwn.as<float>(), ctx->g_codes_p.p, ctx->g_nrm_p.as<float>(), ctx->g_tile_meta.p, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return AFIS_OK;
    };
    const int rc = body();
    for (hipEvent_t e : ev_c) (void)hipEventDestroy(e);
    if (rc != AFIS_OK) {
        if (touched) {                                                      // half-compacted arrays are no gallery: the context is back to "not committed", nothing staged
            (void)hipStreamSynchronize(s);
            free_gallery_dev(ctx);
            ctx->gal = GalleryDev(); ctx->committed = false; ctx->reopened = false;
            ++ctx->gallery_epoch;                                           // handles uploaded against the dropped shard stay refused whatever is committed next
            ctx->res_empty.clear(); ctx->res_mo.clear(); ctx->res_to.clear();
            ctx->err += " [afis_gallery_remove failed half-way: the resident shard was dropped; stage and commit the gallery again]";
        }
        return rc;
    }
    ctx->max_nR = max_nR; ctx->q_blocks = q_blocks; ctx->t32_tiles = t32; ctx->minu_tiles = toff[(size_t)G];
    ctx->total_minutiae = NM1; ctx->total_tex_points = NT1;
    ctx->res_empty = std::move(empty); ctx->res_mo = std::move(mo); ctx->res_to = std::move(to);
    ctx->compact_us = (int64_t)compact_us; ctx->compact_bytes = compact_bytes;
    invalidate_lazy_streams(ctx);
    ++ctx->gallery_epoch;
    return AFIS_OK;
}

// The third edit: staged template i takes the place of resident entry idx[i].  Order: (1) the plan on the host (gallery_splice_plan.h: validation, the shard's offsets and
// flags after the edit, one source table per point kind); (2) the staged points and every table go to buffers of their own; (3) each SoA array is spliced into a fresh buffer
// of its new size — resident ranges from the old array, replaced ones from the staged points — which is swapped in and the old one released, descriptors first as in the
// removal; (4) the tables are switched; (5) the derived layouts get buffers of their new sizes (they may have GROWN) and are laid out whole.  Up to the first swap of (3) the
// resident shard is what it was and the staged templates stay staged; a failure after it drops the shard, as a removal's does.
int afis_gallery_commit_at(afis_ctx* ctx, const int64_t* idx, int64_t n)
{
    if (!ctx) return AFIS_EINVAL;
    if (n < 0 || (n > 0 && !idx)) return fail(ctx, AFIS_EINVAL, "afis_gallery_commit_at: bad argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_gallery_commit_at: commit the gallery first");
    if (!ctx->reopened) return fail(ctx, AFIS_ESTATE, "afis_gallery_commit_at: the gallery is not reopened (afis_gallery_reopen, then stage the replacements)");
    HostGallery& hg = ctx->hg;
    const GalleryMapping* gm = ctx->pend.get();
    const int64_t Gn = gm ? ctx->pend_count : hg.size();
    if (Gn == 0) return fail(ctx, AFIS_ESTATE, "afis_gallery_commit_at: nothing is staged");
    const int64_t G = ctx->gal.G;
    const int64_t* src_mo = gm ? gm->minu_off + ctx->pend_first : hg.minu_off.data();
    const int64_t* src_to = gm ? gm->tex_off + ctx->pend_first : hg.tex_off.data();
    const uint8_t* s_empty = gm ? gm->empty + ctx->pend_first : hg.empty.data();
    SplicePlan plan;
    { const int e = plan_gallery_splice(ctx->res_mo.data(), ctx->res_to.data(), ctx->res_empty.data(), G, ctx->index_base, idx, n, Gn, src_mo, src_to, s_empty, plan);
      if (e != kSpliceOk) return fail(ctx, AFIS_EINVAL, std::string("afis_gallery_commit_at: ") + splice_plan_message(e)); }
    const int64_t m0 = src_mo[0], t0 = src_to[0];
    const size_t NMs = (size_t)(src_mo[Gn] - m0), NTs = (size_t)(src_to[Gn] - t0);
    const int16_t* s_mx = gm ? gm->mx + m0 : hg.mx.data(); const int16_t* s_my = gm ? gm->my + m0 : hg.my.data();
    const float* s_mori = gm ? gm->mori + m0 : hg.mori.data(); const float* s_mdes = gm ? gm->mdes + (size_t)m0 * kDes : hg.mdes.data();
    const int16_t* s_tx = gm ? gm->tx + t0 : hg.tx.data(); const int16_t* s_ty = gm ? gm->ty + t0 : hg.ty.data();
    const float* s_tori = gm ? gm->tori + t0 : hg.tori.data(); const uint8_t* s_tcodes = gm ? gm->tcodes + (size_t)t0 * kM : hg.tcodes.data();
    if (gm && gm->fd_ >= 0) {
        struct stat st;
        if (fstat(gm->fd_, &st) != 0 || (size_t)st.st_size < gm->len_) return fail(ctx, AFIS_EFORMAT, "gallery container: " + gm->path + " was truncated after it was loaded");
    }
    std::vector<int32_t> toff, qb, tb;
    int64_t q_blocks = 0, t32 = 0; int max_nR = 0;
    derived_offsets(plan.mo, plan.to, toff, qb, tb, q_blocks, t32, max_nR);
    { const int rcq = quiesce(ctx, "afis_gallery_commit_at"); if (rcq != AFIS_OK) return rcq; }
    hipStream_t s = ctx->stream;
    const bool clock_it = getenv("AFIS_COMMIT_TIMING") != nullptr;           // development aid, as in commit_shard
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_prev = now();
    auto lap = [&](const char* what) { if (clock_it) { (void)hipStreamSynchronize(s); const double t = now(); fprintf(stderr, "replace: %-28s %8.1f ms\n", what, t - t_prev); t_prev = t; } };
    const int64_t NM1 = plan.mo[(size_t)G], NT1 = plan.to[(size_t)G];
    // the parity tap afis_debug_compact_stats, as in the removal: device time of the splice kernels of this call and the bytes they wrote
    double compact_us = 0; int64_t compact_bytes = 0;
    hipEvent_t ev_c[2] = {nullptr, nullptr};
    for (hipEvent_t& e : ev_c) HIPCHK(ctx, hipEventCreate(&e));
    bool touched = false;                                                   // an array has been replaced: from here on a failure cannot leave the old shard behind
    auto body = [&]() -> int {
        // (2) the staged points and the two source tables in ONE device buffer, its parts on 256-byte boundaries (an allocation and a release instead of eight of each); the
        // offset tables beside the resident ones.  As in the append, arrays below 256 MB go without the pinned pipe.
        struct Staged { DevBuf buf; ~Staged() { buf.release(); } } sd;
        enum { kMdes, kTcodes, kMxy, kMori, kTxy, kTori, kSrcM, kSrcT, kParts };
        const size_t part_bytes[kParts] = {NMs * kDes * 4, NTs * kM, NMs * 4, NMs * 4, NTs * 4, NTs * 4, (size_t)G * 4, (size_t)G * 4};
        size_t part_at[kParts], total = 0;
        for (int k = 0; k < kParts; ++k) { part_at[k] = total; total += up256(part_bytes[k]); }
        HIPCHK(ctx, sd.buf.ensure(std::max<size_t>(total, 16)));
        auto part = [&](int k) { return sd.buf.as<uint8_t>() + part_at[k]; };
        PinnedPipe pp;
        pp.h2d = &ctx->gallery_h2d_bytes;
        pp.direct_below = (size_t)256 << 20;
        HIPCHK(ctx, upload_bulk_at(pp, part(kMdes), s_mdes, part_bytes[kMdes], s));
        std::vector<short2> mxy(NMs), txy(NTs);
        parallel_for((int64_t)NMs, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) mxy[(size_t)i] = make_short2(s_mx[i], s_my[i]); });
        parallel_for((int64_t)NTs, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) txy[(size_t)i] = make_short2(s_tx[i], s_ty[i]); });
        HIPCHK(ctx, upload_bulk_at(pp, part(kTcodes), s_tcodes, part_bytes[kTcodes], s));
        HIPCHK(ctx, upload_bulk_at(pp, part(kMxy), mxy.data(), part_bytes[kMxy], s)); HIPCHK(ctx, upload_bulk_at(pp, part(kMori), s_mori, part_bytes[kMori], s));
        HIPCHK(ctx, upload_bulk_at(pp, part(kTxy), txy.data(), part_bytes[kTxy], s)); HIPCHK(ctx, upload_bulk_at(pp, part(kTori), s_tori, part_bytes[kTori], s));
        HIPCHK(ctx, h2d_copy(ctx, part(kSrcM), plan.src_m.data(), part_bytes[kSrcM], s)); HIPCHK(ctx, h2d_copy(ctx, part(kSrcT), plan.src_t.data(), part_bytes[kSrcT], s));
        TableSet nt;
        HIPCHK(ctx, upload_table(ctx, nt.minu_off, plan.mo, s)); HIPCHK(ctx, upload_table(ctx, nt.tile_off, toff, s)); HIPCHK(ctx, upload_table(ctx, nt.tex_off, plan.to, s));
        HIPCHK(ctx, upload_table(ctx, nt.q_blk, qb, s)); HIPCHK(ctx, upload_table(ctx, nt.t32_blk, tb, s));
        HIPCHK(ctx, hipStreamSynchronize(s));                               // (mxy / txy are pageable host memory of this scope)
        lap("staged points and tables");
        // (3) one array at a time, the largest first: the transient memory is one array plus the staged buffer
        struct Arr { DevBuf* b; int stg; int elem; bool minu; };
        const Arr arrs[] = {{&ctx->g_minu_des, kMdes, kDes * 4, true}, {&ctx->g_tex_codes, kTcodes, kM, false}, {&ctx->g_minu_xy, kMxy, 4, true}, {&ctx->g_minu_ori, kMori, 4, true},
                            {&ctx->g_tex_xy, kTxy, 4, false}, {&ctx->g_tex_ori, kTori, 4, false}};
        for (const Arr& a : arrs) {
            const int64_t n_new = a.minu ? NM1 : NT1;
            DevBuf fresh;
            HIPCHK(ctx, fresh.ensure(std::max<size_t>((size_t)n_new * (size_t)a.elem, 16)));
            hipError_t e = hipEventRecord(ev_c[0], s);
            if (e == hipSuccess) e = launch_splice_ranges(a.b->p, part(a.stg), fresh.p, a.elem, (const int32_t*)part(a.minu ? kSrcM : kSrcT),
                                                          a.minu ? nt.minu_off.as<int32_t>() : nt.tex_off.as<int32_t>(), (int)G, n_new, s);
            if (e == hipSuccess) e = hipEventRecord(ev_c[1], s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            float ms = 0;
            if (e == hipSuccess && n_new > 0) e = hipEventElapsedTime(&ms, ev_c[0], ev_c[1]);
            if (e != hipSuccess) { fresh.release(); HIPCHK(ctx, e); }
            compact_us += (double)ms * 1e3; compact_bytes += n_new * a.elem;
            std::swap(*a.b, fresh); fresh.release();
            touched = true;
            refresh_gallery_view(ctx);
        }
        lap("splice");
        // (4) the switch of the tables; the flags in place ([G] as before)
        std::swap(ctx->g_minu_off, nt.minu_off); std::swap(ctx->g_minu_tile_off, nt.tile_off); std::swap(ctx->g_tex_off, nt.tex_off);
        std::swap(ctx->g_tex_q_blk, nt.q_blk); std::swap(ctx->g_tex_t32_blk, nt.t32_blk);
        HIPCHK(ctx, h2d_copy(ctx, ctx->g_empty.p, plan.empty.data(), (size_t)G, s));
        // (5) the derived layouts, whole, into buffers of the new sizes (DevBuf::ensure keeps a buffer that is large enough: nothing of the old contents is needed)
        HIPCHK(ctx, ctx->g_minu_frag.ensure(std::max<size_t>((size_t)toff[(size_t)G] * 6 * 64 * 16, 16)));
        if (ctx->mf_gal_built) {
            const size_t n_ent = std::max<size_t>((size_t)t32 * 32, 1);
            HIPCHK(ctx, ctx->g_codes_p.ensure(n_ent * 16)); HIPCHK(ctx, ctx->g_nrm_p.ensure(n_ent * 4)); HIPCHK(ctx, ctx->g_tile_meta.ensure(std::max<size_t>((size_t)t32 * 8, 16)));
        }
        refresh_gallery_view(ctx);
        HIPCHK(ctx, launch_fragment_tiles(ctx->g_minu_des.as<float>(), ctx->g_minu_off.as<int32_t>(), ctx->g_minu_tile_off.as<int32_t>(), (int)G, ctx->g_minu_frag.p, s));
        if (ctx->mf_gal_built)
            HIPCHK(ctx, launch_mf_tiles(ctx->gal, ctx->g_tex_t32_blk.as<int32_t>(), ctx->mf_cwn.as<float>(), ctx->g_codes_p.p, ctx->g_nrm_p.as<float>(), ctx->g_tile_meta.p, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        lap("tables and derived layouts");
        return AFIS_OK;
    };
    const int rc = body();
    for (hipEvent_t e : ev_c) (void)hipEventDestroy(e);
    if (rc != AFIS_OK) {
        if (touched) {                                                      // half-spliced arrays are no gallery: the context is back to "not committed", nothing staged
            (void)hipStreamSynchronize(s);
            free_gallery_dev(ctx);
            ctx->gal = GalleryDev(); ctx->committed = false; ctx->reopened = false;
            ++ctx->gallery_epoch;
            ctx->res_empty.clear(); ctx->res_mo.clear(); ctx->res_to.clear();
            release_staging(ctx);
            ctx->err += " [afis_gallery_commit_at failed half-way: the resident shard was dropped; stage and commit the gallery again]";
        }
        return rc;
    }
    ctx->max_nR = max_nR; ctx->q_blocks = q_blocks; ctx->t32_tiles = t32; ctx->minu_tiles = toff[(size_t)G];
    ctx->total_minutiae = NM1; ctx->total_tex_points = NT1;
    ctx->res_empty = std::move(plan.empty); ctx->res_mo = std::move(plan.mo); ctx->res_to = std::move(plan.to);
    ctx->compact_us = (int64_t)compact_us; ctx->compact_bytes = compact_bytes;
    invalidate_lazy_streams(ctx);
    ++ctx->gallery_epoch;
    release_staging(ctx);
    ctx->reopened = false;
    lap("staging released");
    return AFIS_OK;
}

int afis_gallery_export(afis_ctx* ctx, const char* path, const char* const* names)
{
    if (!ctx || !path) return fail(ctx, AFIS_EINVAL, "afis_gallery_export: null argument");
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, "afis_gallery_export: commit the gallery first (afis_gallery_save writes a staged one)");
    { const int rcq = quiesce(ctx, "afis_gallery_export"); if (rcq != AFIS_OK) return rcq; }
    const int64_t G = ctx->gal.G;
    const size_t NM = (size_t)ctx->total_minutiae, NT = (size_t)ctx->total_tex_points;
    HostGallery out;
    out.minu_off.assign(ctx->res_mo.begin(), ctx->res_mo.end()); out.tex_off.assign(ctx->res_to.begin(), ctx->res_to.end());
    out.empty = ctx->res_empty;
    std::vector<short2> mxy(NM), txy(NT);
    out.mx.resize(NM); out.my.resize(NM); out.mori.resize(NM); out.mdes.resize(NM * kDes);
    out.tx.resize(NT); out.ty.resize(NT); out.tori.resize(NT); out.tcodes.resize(NT * kM);
    if (NM) {
        HIPCHK(ctx, hipMemcpy(mxy.data(), ctx->g_minu_xy.p, NM * 4, hipMemcpyDeviceToHost)); HIPCHK(ctx, hipMemcpy(out.mori.data(), ctx->g_minu_ori.p, NM * 4, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(out.mdes.data(), ctx->g_minu_des.p, NM * kDes * 4, hipMemcpyDeviceToHost));
    }
    if (NT) {
        HIPCHK(ctx, hipMemcpy(txy.data(), ctx->g_tex_xy.p, NT * 4, hipMemcpyDeviceToHost)); HIPCHK(ctx, hipMemcpy(out.tori.data(), ctx->g_tex_ori.p, NT * 4, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(out.tcodes.data(), ctx->g_tex_codes.p, NT * kM, hipMemcpyDeviceToHost));
    }
    parallel_for((int64_t)NM, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) { out.mx[(size_t)i] = mxy[(size_t)i].x; out.my[(size_t)i] = mxy[(size_t)i].y; } });
    parallel_for((int64_t)NT, [&](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) { out.tx[(size_t)i] = txy[(size_t)i].x; out.ty[(size_t)i] = txy[(size_t)i].y; } });
    std::vector<std::string> nm;
    if (names) for (int64_t i = 0; i < G; ++i) nm.emplace_back(names[i] ? names[i] : "");
    std::string err;
    if (!write_gallery_container(path, out, nm, err)) return fail(ctx, AFIS_EFORMAT, "afis_gallery_export: " + err);
    return AFIS_OK;
}

int64_t afis_gallery_size(const afis_ctx* ctx) { return !ctx ? 0 : (int64_t)ctx->res_empty.size() + (ctx->pend ? ctx->pend_count : ctx->hg.size()); }

}  // extern "C"
