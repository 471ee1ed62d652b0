// ref_matcher_harness.cpp — C-ABI driver around the REFERENCE's own matching/matcher.cpp, which oracle/Makefile compiles unmodified
// from where it lies against the stand-in headers of oracle/standin/ (nothing from the reference is copied into this repository).
//
// TEST INFRASTRUCTURE ONLY (see oracle/afis_oracle.cpp header).  Output: oracle/_ref/libafis_refmatcher.so.  Only
// tests/golden/make_golden_matcher_ref.py uses it, to record tests/golden/golden_matcher_ref.npz; the tests read that record.
//
// What runs here is the reference's control flow, comparisons, float/double promotions, loaders and sort calls.  What does NOT is
// Eigen's summation order: the sums matcher.cpp leaves to Eigen are taken by oracle/standin/Eigen/Dense in the order set with
// refm_set_order().
//
// Every entry point takes FILE PATHS, so that the reference's own loaders (load_FP_template, both overloads, and the
// codebook-reading constructor) are part of what is pinned.
//
// Built with -fno-access-control: the stage functions (LSS_R_Fast2_Dist_eigen / _lookup, LSS_R_Fast2) are private members.
//
// Where the reference has no defined answer, this file does not ask it for one:
//   * One2One_matching_selected_templates / _all_templates end without a return statement (matcher.cpp:417, :374).  Their return
//     value is never read here; the status is decided from the loaded template counts with the conditions of :383-391 / :345-353.
//   * One2List_matching indexes with an uninitialised variable (:244).  It is never called.
//   * List2List_matching reads that undefined return value (:180-186) and score[28] whatever the vector's length (:188); the recorder
//     only runs it on latents with 28 minutiae templates and a texture template and accepts its rows only where they agree with the
//     per-pair scores.
#include <tuple>      // matcher.h names std::tuple without including it
#include <cstdint>
#include <cstring>
#include <iostream>
#include <streambuf>
#include <string>
#include <vector>
#include "matcher.h"
#include <Eigen/Dense>

namespace {

struct NullBuf : std::streambuf { int overflow(int c) override { return c; } };

// the reference reports progress on std::cout; keep it off the recorder's output
struct Quiet {
    NullBuf nb; std::streambuf* old;
    Quiet() : old(std::cout.rdbuf(&nb)) {}
    ~Quiet() { std::cout.rdbuf(old); }
};

struct Pair {
    LatentFPTemplate latent;
    RolledFPTemplate rolled;
    int latent_rc = 0, rolled_rc = 0;
};

typedef std::vector<std::tuple<float, int, int> > List;

List list_in(int n, const uint32_t* sim_bits, const int* li, const int* ri)
{
    List c((size_t)n);
    for (int k = 0; k < n; ++k) { float s; memcpy(&s, &sim_bits[k], 4); c[(size_t)k] = std::make_tuple(s, li[k], ri[k]); }
    return c;
}

int list_out(const List& c, uint32_t* sim_bits, int* li, int* ri, int cap)
{
    const int n = (int)c.size();
    for (int k = 0; k < n && k < cap; ++k) {
        float s = std::get<0>(c[(size_t)k]); memcpy(&sim_bits[k], &s, 4);
        li[k] = std::get<1>(c[(size_t)k]); ri[k] = std::get<2>(c[(size_t)k]);
    }
    return n;
}

int vector_out(const std::vector<float>& v, uint32_t* bits, int cap)
{
    const int n = (int)v.size();
    for (int k = 0; k < n && k < cap; ++k) memcpy(&bits[k], &v[(size_t)k], 4);
    return n;
}

}  // namespace

extern "C" {

void* refm_new(const char* codebook_path) { Quiet q; return new PQ::Matcher(std::string(codebook_path)); }

void refm_free(void* m) { delete (PQ::Matcher*)m; }

void refm_set_order(int order) { Eigen::standin::order = order; }
int refm_get_order(void) { return Eigen::standin::order; }

// codebook dimensions as the constructor read them (matcher.cpp:74-76)
void refm_dims(void* m, int* out) { PQ::Matcher* M = (PQ::Matcher*)m; out[0] = M->nrof_subs; out[1] = M->nrof_clusters; out[2] = M->sub_dim; }

// Loads both files with the reference's loaders.  info: latent return code, rolled return code, then the template counts the
// loaders left: latent minutiae, latent texture, rolled minutiae, rolled texture.  With zero_failed_rolled, a rolled file whose
// loader returned a negative code then has its counts zeroed, as the reference's caller does (matcher.cpp:173-177).
void* refm_pair_load(void* m, const char* latent_path, const char* rolled_path, int zero_failed_rolled, int* info)
{
    Quiet q;
    PQ::Matcher* M = (PQ::Matcher*)m;
    Pair* p = new Pair;
    p->latent_rc = M->load_FP_template(std::string(latent_path), p->latent);
    p->rolled_rc = M->load_FP_template(std::string(rolled_path), p->rolled);
    info[0] = p->latent_rc; info[1] = p->rolled_rc;
    info[2] = p->latent.m_nrof_minu_templates; info[3] = p->latent.m_nrof_texture_templates;
    info[4] = p->rolled.m_nrof_minu_templates; info[5] = p->rolled.m_nrof_texture_templates;
    if (zero_failed_rolled && p->rolled_rc < 0) { p->rolled.m_nrof_minu_templates = 0; p->rolled.m_nrof_texture_templates = 0; }
    return p;
}

void refm_pair_free(void* pair) { delete (Pair*)pair; }

// number of points of a loaded template: kind 0 latent minutiae, 1 latent texture, 2 rolled minutiae, 3 rolled texture; -1 if absent
int refm_points(void* pair, int kind, int t)
{
    Pair* p = (Pair*)pair;
    if (t < 0) return -1;
    if (kind == 0) return t < (int)p->latent.m_minu_templates.size() ? p->latent.m_minu_templates[t].m_nrof_minu : -1;
    if (kind == 1) return t < (int)p->latent.m_texture_templates.size() ? p->latent.m_texture_templates[t].m_nrof_minu : -1;
    if (kind == 2) return t < (int)p->rolled.m_minu_templates.size() ? p->rolled.m_minu_templates[t].m_nrof_minu : -1;
    return t < (int)p->rolled.m_texture_templates.size() ? p->rolled.m_texture_templates[t].m_nrof_minu : -1;
}

// One2One_matching_selected_templates (matcher.cpp:376-417).  Returns the status (0, 1 latent empty, 2 rolled empty) decided here
// from the counts; *n = length of the score vector, bits = its elements.  save_corr: the three correspondence files
// <prefix>_<i>.csv of :405 / :497-505.
int refm_selected(void* m, void* pair, int save_corr, const char* prefix, uint32_t* bits, int cap, int* n)
{
    Quiet q;
    PQ::Matcher* M = (PQ::Matcher*)m; Pair* p = (Pair*)pair;
    std::vector<float> score;
    M->One2One_matching_selected_templates(p->latent, p->rolled, score, save_corr != 0, std::string(prefix ? prefix : ""));
    *n = vector_out(score, bits, cap);
    if (p->latent.m_nrof_minu_templates <= 27 - 1 && p->latent.m_nrof_texture_templates <= 0) return 1;   // :383
    if (p->rolled.m_nrof_minu_templates <= 0 && p->rolled.m_nrof_texture_templates <= 0) return 2;        // :388
    return 0;
}

// One2One_matching_all_templates (matcher.cpp:339-374); status from the conditions of :345 / :350
int refm_all(void* m, void* pair, uint32_t* bits, int cap, int* n)
{
    Quiet q;
    PQ::Matcher* M = (PQ::Matcher*)m; Pair* p = (Pair*)pair;
    std::vector<float> score;
    M->One2One_matching_all_templates(p->latent, p->rolled, score);
    *n = vector_out(score, bits, cap);
    if (p->latent.m_nrof_minu_templates <= 0 && p->latent.m_nrof_texture_templates <= 0) return 1;
    if (p->rolled.m_nrof_minu_templates <= 0 && p->rolled.m_nrof_texture_templates <= 0) return 2;
    return 0;
}

// One stage function on a caller-given correspondence list, with the arguments of the reference's own call sites (`int d_thr = 30`
// passed on, matcher.cpp:491-495 and :758-767).  fn: 0 LSS_R_Fast2_Dist_eigen, 1 LSS_R_Fast2_Dist_lookup, 2 LSS_R_Fast2.
// texture != 0: latent texture template 0 against rolled texture template 0, both clamped to 1000 points first as the texture
// scorer does before it calls them (:544-547); else latent minutiae template `latent_t` against rolled minutiae template 0.
// Returns the length of the list that came back, -1 when a template is absent.
int refm_stage(void* m, void* pair, int fn, int texture, int latent_t, int n_in, const uint32_t* sim_in, const int* li_in, const int* ri_in,
               uint32_t* sim_out, int* li_out, int* ri_out, int cap)
{
    Quiet q;
    PQ::Matcher* M = (PQ::Matcher*)m; Pair* p = (Pair*)pair;
    SingleTemplate* L; SingleTemplate* R;
    if (texture) {
        if (p->latent.m_texture_templates.empty() || p->rolled.m_texture_templates.empty()) return -1;
        L = &p->latent.m_texture_templates[0]; R = &p->rolled.m_texture_templates[0];
        if (L->m_nrof_minu > PQ::MaxNLatentMinu) L->m_nrof_minu = PQ::MaxNLatentMinu;
        if (R->m_nrof_minu > PQ::MaxNRolledMinu) R->m_nrof_minu = PQ::MaxNRolledMinu;
    } else {
        if (latent_t < 0 || latent_t >= (int)p->latent.m_minu_templates.size() || p->rolled.m_minu_templates.empty()) return -1;
        L = &p->latent.m_minu_templates[latent_t]; R = &p->rolled.m_minu_templates[0];
    }
    List in = list_in(n_in, sim_in, li_in, ri_in), out;
    int d_thr = 30;
    if (fn == 0) out = M->LSS_R_Fast2_Dist_eigen(in, *L, *R, d_thr);
    else if (fn == 1) out = M->LSS_R_Fast2_Dist_lookup(in, *L, *R, d_thr);
    else out = M->LSS_R_Fast2(in, *L, *R, d_thr);
    return list_out(out, sim_out, li_out, ri_out, cap);
}

// List2List_matching (matcher.cpp:96-214): one <score_prefix><latent stem>.csv per latent .dat of latent_dir
int refm_list2list(void* m, const char* latent_dir, const char* rolled_dir, const char* score_prefix)
{
    Quiet q;
    return ((PQ::Matcher*)m)->List2List_matching(std::string(latent_dir), std::string(rolled_dir), std::string(score_prefix));
}

}  // extern "C"
