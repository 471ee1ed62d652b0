// afis_cases.cpp — case lists of the C ABI (include/afis_matcher.h): afis_rank_case_hits and afis_rank_case_subject_hits fuse the queries of the last search that
// belong to one case — by sum or by maximum (case_fuse.hip) — into one row per case, and list per case the templates, or the enrolled persons, whose fused score
// reaches a decision score.  Their _filtered forms fold, per column, only the members that are ELIGIBLE for it: the filter pass of the filtered hit lists (FilterPass,
// afis_filter.cpp) runs first, and the folds take its "no entry" cells for members that are not there.  The fused rows are ranked by k_rank_hits (rank_hits.hip) in its template form, unchanged, the way afis_reverse.cpp runs it on the
// transposed matrix: rows = the cases, entries = the columns of the search or the slots of the subject handle (the ids in ascending order, so that "ascending
// position" is "ascending subject id").  Only n_cases x (8 + cap x 12) bytes return; the [n_q][G] matrix stays where it is.
#include "afis_ctx.h"
#include "target_tables.h"

using namespace afis;

static_assert(kCaseSum == AFIS_CASE_SUM && kCaseMax == AFIS_CASE_MAX, "case_fuse.hip folds by the modes of include/afis_matcher.h");

namespace afis {

// what a filtered entry point adds to its plain sibling's arguments (all null: the sibling itself)
struct CaseFilter { const afis_labels* labels = nullptr; const uint64_t* masks = nullptr; const int64_t* excl_off = nullptr; const int64_t* excl = nullptr; };

// the four entry points behind their checks (subj == NULL: the templates); ids: the distinct case ids in ascending order, n_cases of them; pairs: the exclusions as
// check_filtered resolved them.  Neither masks nor pairs: the plain folds on the search's matrix itself
static int rank_case_hits(afis_ctx* ctx, const char* who, afis_subjects* subj, const CaseFilter& f, const std::vector<int32_t>& pairs, const int64_t* case_of, int mode,
                          const std::vector<int64_t>& ids, float min_score, int cap, int64_t* case_id, int64_t* n_hits, int64_t* out_a, float* out_score)
{
    const LastSearch ls = ctx->last_search;
    const int n_q = ls.n_q;
    const int64_t n_cases = (int64_t)ids.size(), cols = subj ? subj->S : ls.G;
    HitCall hc{ctx, who, n_cases, cap, n_hits, out_a, out_score, nullptr};
    ctx->rank_cases_us = 0; ctx->case_fuse_us = 0; ctx->case_rank_us = 0;
    if (hc.empty(ls.G == 0 || cols == 0)) { std::copy(ids.begin(), ids.end(), case_id); return AFIS_OK; }
    // the cases as a CSR (target_tables.h: every case has a member, so its rows are the cases): the positions of a case stay in ascending order; off [n_cases + 1] | member [n_q]
    std::vector<int32_t> row_of((size_t)n_q);
    for (int i = 0; i < n_q; ++i) row_of[(size_t)i] = (int32_t)(std::lower_bound(ids.begin(), ids.end(), case_of[i]) - ids.begin());
    const TargetTables tt = build_target_tables(row_of.data(), nullptr, (size_t)n_q, nullptr);
    std::vector<int32_t> tab(tt.off);
    tab.insert(tab.end(), tt.order.begin(), tt.order.end());
    FilterPass fp{ctx, f.labels, f.masks, pairs, subj != nullptr};
    const bool eligible = fp.filters();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, fp.ensure());
    HIPCHK(ctx, ctx->case_fused.ensure((size_t)n_cases * (size_t)cols * 4));
    HIPCHK(ctx, ctx->case_tab.ensure(tab.size() * 4));
    if (subj) HIPCHK(ctx, ctx->subj_best.ensure((size_t)n_q * (size_t)cols * 8));
    AFISCHK(hc.begin({{ctx->case_tab.p, tab.data(), tab.size() * 4}, fp.masks_up(), fp.pairs_up()}));
    hipStream_t s = ctx->stream;
    const int32_t* const d_off = ctx->case_tab.as<int32_t>(), * const d_member = d_off + n_cases + 1;
    float* const fused = ctx->case_fused.as<float>();
    AFISCHK(fp.queue_cells());                                              // (no filter: nothing, and fp.matrix() is the search's)
    if (subj) {                                                             // the maxima first, exactly as rank_hits and rank_hits_filtered make them
        unsigned long long* const best = ctx->subj_best.as<unsigned long long>();
        AFISCHK(queue_subject_best(ctx, subj, fp.matrix()));
        AFISCHK(fp.queue_drop_subjects(cols));
        if (eligible) HIPCHK(ctx, launch_case_fuse_subjects_eligible(best, (int)cols, d_off, d_member, (int)n_cases, mode, fused, s));
        else HIPCHK(ctx, launch_case_fuse_subjects(best, (int)cols, d_off, d_member, (int)n_cases, mode, fused, s));
    } else if (eligible) HIPCHK(ctx, launch_case_fuse_eligible(fp.matrix(), (int)cols, d_off, d_member, (int)n_cases, mode, fused, s));
    else HIPCHK(ctx, launch_case_fuse(fp.matrix(), (int)cols, d_off, d_member, (int)n_cases, mode, fused, s));
    // rows = the cases; entries = the columns: a template's global index (index_base + position, or the subset's table), or the id of a subject slot.  The template
    // form either way: a fused subject row holds scores, and the folds compared rank_key
    AFISCHK(hc.finish({fused, cols, nullptr, subj ? subj->d_ids.as<long long>() : global_map(ls), (long long)ctx->index_base}, min_score));
    ctx->rank_cases_us = hc.total_us; ctx->case_fuse_us = hc.pre_us; ctx->case_rank_us = hc.rank_us;
    std::copy(ids.begin(), ids.end(), case_id);
    return AFIS_OK;
}

// the checks the entry points share, in the order of afis_rank_hits'; on AFIS_OK ids holds the distinct case ids in ascending order.  f: a filtered entry point —
// check_filtered stands where check_hits does (it makes that check, between its own) and leaves the resolved exclusions in pairs
static int check_cases(afis_ctx* ctx, const char* who, const afis_subjects* s, const int64_t* case_of, int n_q, int mode, int64_t n_cases, float min_score, int cap, bool outputs,
                       std::vector<int64_t>& ids, const CaseFilter* f = nullptr, std::vector<int32_t>* pairs = nullptr)
{
    const std::string w(who);
    if (mode != AFIS_CASE_SUM && mode != AFIS_CASE_MAX) return fail(ctx, AFIS_EINVAL, w + ": mode must be AFIS_CASE_SUM (0) or AFIS_CASE_MAX (1)");
    if (f) AFISCHK(check_filtered(ctx, who, s, f->labels, f->masks, f->excl_off, f->excl, n_q, min_score, cap, outputs && case_of, *pairs));
    else AFISCHK(check_hits(ctx, who, n_q, min_score, cap, outputs && case_of, s));
    ids.assign(case_of, case_of + n_q);
    std::sort(ids.begin(), ids.end());
    if (!ids.empty() && ids.front() < 0) return fail(ctx, AFIS_EINVAL, w + ": a case id is negative");
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    if (n_cases != (int64_t)ids.size())
        return fail(ctx, AFIS_EINVAL, w + ": n_cases is " + std::to_string((long long)n_cases) + ", case_of holds " + std::to_string((long long)ids.size()) + " distinct case ids");
    return AFIS_OK;
}

}  // namespace afis

extern "C" {

int afis_rank_case_hits(afis_ctx* ctx, const int64_t* case_of, int n_q, int mode, int64_t n_cases, float min_score, int cap,
                        int64_t* case_id, int64_t* n_hits, int64_t* idx, float* score)
{
    if (!ctx) return fail(ctx, AFIS_EINVAL, "afis_rank_case_hits: null argument");
    std::vector<int64_t> ids;
    const int rc = check_cases(ctx, "afis_rank_case_hits", nullptr, case_of, n_q, mode, n_cases, min_score, cap, case_id && n_hits && idx && score, ids);
    return rc != AFIS_OK ? rc : rank_case_hits(ctx, "afis_rank_case_hits", nullptr, CaseFilter{}, {}, case_of, mode, ids, min_score, cap, case_id, n_hits, idx, score);
}

int afis_rank_case_subject_hits(afis_ctx* ctx, afis_subjects* s, const int64_t* case_of, int n_q, int mode, int64_t n_cases, float min_score, int cap,
                                int64_t* case_id, int64_t* n_hits, int64_t* subject_id, float* score)
{
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, "afis_rank_case_subject_hits: null argument");
    AFISCHK(check_subject_handle(ctx, "afis_rank_case_subject_hits", s));
    std::vector<int64_t> ids;
    const int rc = check_cases(ctx, "afis_rank_case_subject_hits", s, case_of, n_q, mode, n_cases, min_score, cap, case_id && n_hits && subject_id && score, ids);
    return rc != AFIS_OK ? rc : rank_case_hits(ctx, "afis_rank_case_subject_hits", s, CaseFilter{}, {}, case_of, mode, ids, min_score, cap, case_id, n_hits, subject_id, score);
}

int afis_rank_case_hits_filtered(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl,
                                 const int64_t* case_of, int n_q, int mode, int64_t n_cases, float min_score, int cap,
                                 int64_t* case_id, int64_t* n_hits, int64_t* idx, float* score)
{
    const char* const who = "afis_rank_case_hits_filtered";
    if (!ctx) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    const CaseFilter f{labels, masks, excl_off, excl};
    std::vector<int64_t> ids;
    std::vector<int32_t> pairs;
    const int rc = check_cases(ctx, who, nullptr, case_of, n_q, mode, n_cases, min_score, cap, case_id && n_hits && idx && score, ids, &f, &pairs);
    return rc != AFIS_OK ? rc : rank_case_hits(ctx, who, nullptr, f, pairs, case_of, mode, ids, min_score, cap, case_id, n_hits, idx, score);
}

int afis_rank_case_subject_hits_filtered(afis_ctx* ctx, afis_subjects* s, afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl_subject,
                                         const int64_t* case_of, int n_q, int mode, int64_t n_cases, float min_score, int cap,
                                         int64_t* case_id, int64_t* n_hits, int64_t* subject_id, float* score)
{
    const char* const who = "afis_rank_case_subject_hits_filtered";
    if (!ctx || !s) return fail(ctx, AFIS_EINVAL, std::string(who) + ": null argument");
    AFISCHK(check_subject_handle(ctx, who, s));
    const CaseFilter f{labels, masks, excl_off, excl_subject};
    std::vector<int64_t> ids;
    std::vector<int32_t> pairs;
    const int rc = check_cases(ctx, who, s, case_of, n_q, mode, n_cases, min_score, cap, case_id && n_hits && subject_id && score, ids, &f, &pairs);
    return rc != AFIS_OK ? rc : rank_case_hits(ctx, who, s, f, pairs, case_of, mode, ids, min_score, cap, case_id, n_hits, subject_id, score);
}

}  // extern "C"
