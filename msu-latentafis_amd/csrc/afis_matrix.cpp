// afis_matrix.cpp — kept matrices of the C ABI (include/afis_matcher.h): the last search's matrix as an object.  afis_matrix_keep copies it, with its record, into a
// plain allocation of its own (the matrix is read, not written: afis_score_stats' contract); afis_matrix_read downloads rows of a copy; afis_matrix_recall copies
// one back as the last search's matrix, record and normalised flag included; afis_matrix_fuse folds up to 16 copies of one shape cell by cell (matrix_fuse.h has the
// rule, matrix_fuse.hip the kernel) into ctx->elig_scores and swaps that with ctx->scores, the way afis_search_eligible and afis_normalize_scores end.
// A handle is STALE once the gallery epoch has moved on or the subset it was scored over has been freed (afis_subset_free calls matrices_lose_subset): it still
// answers afis_matrix_info and afis_matrix_free, nothing else.
// Transposed operands: k_transpose_scores (latent_rank.hip) into ctx->fuse_t first, once per distinct handle read transposed; the fuse kernel then sees an ordinary
// operand (DESIGN section 7 states why).
// A subset listed out of order: a kept matrix stands in the sub-shard's order (ascending global index); afis_matrix_read and scores_out put the columns in the
// caller's order, as afis_normalize_scores does.
#include "afis_ctx.h"
#include "matrix_fuse.h"

using namespace afis;

static_assert(AFIS_FUSE_SUM == kFuseSum && AFIS_FUSE_MAX == kFuseMax && AFIS_FUSE_MIN == kFuseMin && AFIS_FUSE_REQUIRE_ALL == kFuseRequireAll && AFIS_FUSE_OPERANDS_MAX == kFuseOperandsMax,
              "matrix_fuse.h's modes are the header's");

namespace afis {

void release_matrix(afis_matrix* m)
{
    if (!m) return;
    m->d.release();
    delete m;
}

size_t matrix_device_bytes(const afis_ctx* ctx)
{
    size_t n = 0;
    for (const afis_matrix* m : ctx->matrices) n += m->d.bytes;
    return n;
}

void matrices_lose_subset(afis_ctx* ctx, const afis_subset* s)
{
    for (afis_matrix* m : ctx->matrices)
        if (m->rec.sub == s) { m->rec.sub = nullptr; m->sub_freed = true; }
}

static bool is_stale(const afis_ctx* ctx, const afis_matrix* m) { return m->sub_freed || m->rec.gallery_epoch != ctx->gallery_epoch; }

static int check_matrix_handle(afis_ctx* ctx, const char* who, const afis_matrix* m)
{
    if (m && std::find(ctx->matrices.begin(), ctx->matrices.end(), m) != ctx->matrices.end()) return AFIS_OK;
    return fail(ctx, AFIS_EINVAL, std::string(who) + ": not a live kept matrix of this context");
}

// a live handle that may still be read: the shard and the subset it was scored over are the ones that stand
static int check_fresh(afis_ctx* ctx, const char* who, const afis_matrix* m)
{
    if (!ctx->committed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": commit the gallery first");
    if (m->rec.gallery_epoch != ctx->gallery_epoch) return fail_edited(ctx, who, "this matrix was kept; free the handle and search again");
    if (m->sub_freed) return fail(ctx, AFIS_ESTATE, std::string(who) + ": the subset this matrix was scored over has been freed (afis_subset_free) after the matrix was kept; free the handle and search again");
    return AFIS_OK;
}

// n_rows rows of host [..][G] (the sub-shard's order) into out, the columns in the caller's order; order: column_order's, not empty
static void take_rows(const float* host, const std::vector<int32_t>& order, int64_t n_rows, int64_t G, float* out)
{
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t t = 0; t < G; ++t) out[(size_t)r * (size_t)G + (size_t)order[(size_t)t]] = host[(size_t)r * (size_t)G + (size_t)t];
}

// afis_matrix_fuse behind its checks: every operand is live, fresh and of the record `rec`, which the result takes
static int matrix_fuse(afis_ctx* ctx, const afis_matrix* const* ms, const double* weights, const uint8_t* transposed, int n, int mode, const LastSearch& rec, float* scores_out)
{
    const char* const who = "afis_matrix_fuse";
    const int n_q = rec.n_q;
    const int64_t G = rec.G;
    if (n_q == 0 || G == 0) { ctx->last_search = rec; return AFIS_OK; }     // no cell: no device work
    const size_t bytes = (size_t)n_q * (size_t)G * 4, t_stride = up256(bytes);
    std::vector<const afis_matrix*> turned;                                 // the distinct handles read transposed, in order of first use
    const float* src[kFuseOperandsMax];
    std::vector<size_t> t_slot((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        if (!(transposed && transposed[k])) continue;
        auto at = std::find(turned.begin(), turned.end(), ms[k]);
        if (at == turned.end()) { turned.push_back(ms[k]); at = turned.end() - 1; }
        t_slot[(size_t)k] = (size_t)(at - turned.begin());
    }
    const std::vector<int32_t> order = scores_out ? column_order(rec) : std::vector<int32_t>();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AFISCHK(drain_abandoned(ctx, true));
    HIPCHK(ctx, ctx->elig_scores.ensure(bytes));                            // every allocation precedes everything queued: a failed one leaves the last matrix as it was
    if (!turned.empty()) HIPCHK(ctx, ctx->fuse_t.ensure(t_stride * turned.size()));
    for (int k = 0; k < n; ++k) src[k] = transposed && transposed[k] ? (const float*)(ctx->fuse_t.as<uint8_t>() + t_stride * t_slot[(size_t)k]) : ms[k]->d.as<float>();
    Events ev{2};
    for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipEventRecord(ev[0], s));
    for (size_t t = 0; t < turned.size(); ++t)
        HIPCHK(ctx, launch_transpose_scores(turned[t]->d.as<float>(), (float*)(ctx->fuse_t.as<uint8_t>() + t_stride * t), n_q, (int)G, s));
    HIPCHK(ctx, launch_matrix_fuse(src, weights, n, mode, rec.normalized ? 1 : 0, n_q, (int)G, ctx->elig_scores.as<float>(), s));
    HIPCHK(ctx, hipEventRecord(ev[1], s));
    int64_t total_us = 0;
    AFISCHK(wait_elapsed(ctx, who, ev, &total_us));
    if (scores_out) {
        if (order.empty()) HIPCHK(ctx, hipMemcpy(scores_out, ctx->elig_scores.p, bytes, hipMemcpyDeviceToHost));
        else {
            std::vector<float> host((size_t)n_q * (size_t)G);
            HIPCHK(ctx, hipMemcpy(host.data(), ctx->elig_scores.p, bytes, hipMemcpyDeviceToHost));
            take_rows(host.data(), order, n_q, G, scores_out);
        }
    }
    std::swap(ctx->scores, ctx->elig_scores);                               // the fused matrix is the last search's from here on
    ctx->last_search = rec;
    ctx->matrix_fuse_us = total_us;
    return AFIS_OK;
}

}  // namespace afis

extern "C" {

int afis_matrix_keep(afis_ctx* ctx, afis_matrix** out)
{
    const char* const who = "afis_matrix_keep";
    if (!ctx || !out) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    ctx->matrix_keep_us = 0;
    AFISCHK(check_last_search(ctx, who, ctx->last_search.n_q, nullptr));
    std::unique_ptr<afis_matrix, void (*)(afis_matrix*)> m(new afis_matrix(), release_matrix);
    m->rec = ctx->last_search;
    m->over_subset = m->rec.sub != nullptr;
    const size_t bytes = (size_t)m->rec.n_q * (size_t)m->rec.G * 4;
    if (bytes > 0) {                                                        // (an empty shard or n_q == 0: a handle of zero cells, no device work)
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, m->d.ensure(bytes));
        Events ev{2};
        for (hipEvent_t& e : ev) HIPCHK(ctx, hipEventCreate(&e));
        HIPCHK(ctx, hipEventRecord(ev[0], ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(m->d.p, ctx->scores.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipEventRecord(ev[1], ctx->stream));
        int64_t us = 0;
        AFISCHK(wait_elapsed(ctx, who, ev, &us));
        ctx->matrix_keep_us = us;
    }
    ctx->matrices.push_back(m.get());
    *out = m.release();
    return AFIS_OK;
}

void afis_matrix_free(afis_ctx* ctx, afis_matrix* m)
{
    if (!m) return;
    if (ctx) {
        if (std::find(ctx->matrices.begin(), ctx->matrices.end(), m) == ctx->matrices.end()) return;   // not a live handle of this context: nothing of ours to release
        (void)hipSetDevice(ctx->device);
        (void)quiesce(ctx, "afis_matrix_free", true);                       // a call that timed out may still read the copy: bounded wait, as afis_subset_free; the last search's matrix stays
        ctx->matrices.erase(std::remove(ctx->matrices.begin(), ctx->matrices.end(), m), ctx->matrices.end());
    }
    release_matrix(m);
}

int afis_matrix_info(afis_ctx* ctx, const afis_matrix* m, afis_matrix_desc* out)
{
    const char* const who = "afis_matrix_info";
    if (!ctx || !out) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    AFISCHK(check_matrix_handle(ctx, who, m));
    out->n_q = m->rec.n_q; out->normalized = m->rec.normalized ? 1 : 0; out->columns = m->rec.G;
    out->over_subset = m->over_subset ? 1 : 0; out->stale = is_stale(ctx, m) ? 1 : 0;
    return AFIS_OK;
}

int afis_matrix_read(afis_ctx* ctx, const afis_matrix* m, int row0, int n_rows, float* out)
{
    const char* const who = "afis_matrix_read";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    AFISCHK(check_matrix_handle(ctx, who, m));
    AFISCHK(check_fresh(ctx, who, m));
    const int64_t G = m->rec.G;
    if (row0 < 0 || n_rows < 0 || (int64_t)row0 + n_rows > m->rec.n_q) return fail(ctx, AFIS_EINVAL, std::string(who) + ": rows outside the matrix");
    if (n_rows == 0 || G == 0) return AFIS_OK;
    if (!out) return fail(ctx, AFIS_EINVAL, std::string(who) + ": out is null");
    const std::vector<int32_t> order = column_order(m->rec);
    const size_t bytes = (size_t)n_rows * (size_t)G * 4;
    const float* const src = m->d.as<float>() + (size_t)row0 * (size_t)G;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (order.empty()) { HIPCHK(ctx, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost)); return AFIS_OK; }
    std::vector<float> host((size_t)n_rows * (size_t)G);
    HIPCHK(ctx, hipMemcpy(host.data(), src, bytes, hipMemcpyDeviceToHost));
    take_rows(host.data(), order, n_rows, G, out);
    return AFIS_OK;
}

int afis_matrix_recall(afis_ctx* ctx, const afis_matrix* m)
{
    const char* const who = "afis_matrix_recall";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    AFISCHK(check_matrix_handle(ctx, who, m));
    AFISCHK(check_fresh(ctx, who, m));
    const size_t bytes = (size_t)m->rec.n_q * (size_t)m->rec.G * 4;
    if (bytes > 0) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        AFISCHK(drain_abandoned(ctx, true));
        ctx->last_search.valid = false;                                     // from here on the buffer holds the kept matrix, or nothing that can be ranked
        HIPCHK(ctx, ctx->scores.ensure(bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->scores.p, m->d.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        AFISCHK(wait_streams(ctx, {ctx->stream}, who));
    }
    ctx->last_search = m->rec;
    ctx->last_search.valid = true;
    return AFIS_OK;
}

int afis_matrix_fuse(afis_ctx* ctx, const afis_matrix* const* ms, const double* weights, const uint8_t* transposed, int n, int mode, float* scores_out)
{
    const char* const who = "afis_matrix_fuse";
    const std::string w(who);
    if (!ctx) return fail(ctx, AFIS_EINVAL, w + ": null argument");
    ctx->matrix_fuse_us = 0;
    if (n < 1 || n > AFIS_FUSE_OPERANDS_MAX) return fail(ctx, AFIS_EINVAL, w + ": 1 .. AFIS_FUSE_OPERANDS_MAX operands");
    if (!ms) return fail(ctx, AFIS_EINVAL, w + ": null argument");
    if (!fuse_mode_valid(mode)) return fail(ctx, AFIS_EINVAL, w + ": mode must be AFIS_FUSE_SUM, AFIS_FUSE_MAX or AFIS_FUSE_MIN, with AFIS_FUSE_REQUIRE_ALL or-ed in or not");
    for (int k = 0; k < n; ++k) AFISCHK(check_matrix_handle(ctx, who, ms[k]));
    for (int k = 0; k < n; ++k) AFISCHK(check_fresh(ctx, who, ms[k]));
    const LastSearch& a = ms[0]->rec;
    for (int k = 1; k < n; ++k) {
        const LastSearch& b = ms[k]->rec;
        if (b.n_q != a.n_q || b.G != a.G) return fail(ctx, AFIS_EINVAL, w + ": operand " + std::to_string(k) + " has another shape than operand 0");
        if (b.sub != a.sub) return fail(ctx, AFIS_EINVAL, w + ": operand " + std::to_string(k) + " was scored over other columns than operand 0 (all over one subset, or all over the whole shard)");
        if (b.normalized != a.normalized) return fail(ctx, AFIS_EINVAL, w + ": raw and normalised operands do not mix");
    }
    if (weights && (mode & 3) != AFIS_FUSE_SUM) return fail(ctx, AFIS_EINVAL, w + ": weights belong to AFIS_FUSE_SUM alone");
    if (weights)
        for (int k = 0; k < n; ++k)
            if (!std::isfinite(weights[k])) return fail(ctx, AFIS_EINVAL, w + ": every weight must be finite (operand " + std::to_string(k) + ")");
    if (transposed)
        for (int k = 0; k < n; ++k) {
            if (!transposed[k]) continue;
            if ((int64_t)a.n_q != a.G) return fail(ctx, AFIS_EINVAL, w + ": a transposed operand needs a square matrix (n_q == columns)");
            if (a.sub && !a.sub->identity) return fail(ctx, AFIS_EINVAL, w + ": a transposed operand over a subset listed out of order is not offered (list the subset in ascending order)");
        }
    LastSearch rec = a;
    rec.valid = true;
    return matrix_fuse(ctx, ms, weights, transposed, n, mode, rec, scores_out);
}

}  // extern "C"
