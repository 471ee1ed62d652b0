// afis_ctx.h — the host side's internal state and helpers, shared by its translation units: afis_api.cpp (context, options, timing), afis_gallery.cpp (staging,
// container, commit), afis_search.cpp (query groups, the launch sequence of a search, the minutiae stage every driver of the search family sizes and queues, the query handle's rule, all-templates mode), afis_corr.cpp (correspondence export of a pair list: what it asks of the pair driver), afis_pairs.cpp (the driver every pair-list call goes through, the texture stage of a pair table, and pair scoring: the fused scores and parts of a pair list), afis_subset.cpp (subset search), afis_subjects.cpp (subject rank lists), afis_hits.cpp (hit lists, the driver and checks every hit-list call goes through, and the driver of every other call that reads the last search's matrix in place), afis_cases.cpp (case lists), afis_filter.cpp (labels, filtered hit lists), afis_positions.cpp (rank positions: where a named template or person stands), afis_normalize.cpp (cohort statistics of the last search's matrix, its z-normalisation, and the host arithmetic on statistics), afis_distribution.cpp (score distributions of that matrix: per-row histograms and the entry at any rank, of templates and of enrolled persons — whose statistics are afis_normalize.cpp's too), afis_link.cpp (link groups: the connected components rows and columns of that matrix make above a decision score), afis_eligible.cpp (eligible search: the classes of a batch over temporary sub-shards), afis_weighted.cpp (weighted search: any set of a latent's templates, folded on the device), afis_prints.cpp (print search: resident prints as queries, built on the device), afis_evidence.cpp (the evidence calls of a pair list: the texture scorer's correspondences, the exact moments of every scorer's survivors and the fit they give; what they ask of the pair driver), afis_print_pairs.cpp (pair scoring, correspondence export and the evidence calls for resident print pairs: temporary print handles in batches, the pair drivers over them), afis_reverse.cpp (reverse search: reserved query handles, column hit lists), afis_cascade.cpp (cascade search: the minutiae scorers for every cell, the texture scorer for the kept ones; and the driver every cascade call goes through), afis_cascade_eligible.cpp (the cascade over a live subset's columns, and per latent over the templates it is eligible for: that driver over sub-shards), afis_print_cascade.cpp (print cascade: resident prints as that driver's queries, and the kernels that differ), afis_matrix.cpp (kept matrices: the last search's matrix kept, read, recalled and fused on the device) and afis_taps.cpp (parity taps and the direct ADC kernels' host side, test library only).
// The order of scores — the ordered word, the two keys made of it, the composites — is score_order.h's (through afis_device.h), shared with the kernels.
// Not part of the ABI: include/afis_matcher.h is.
#pragma once
#include "../../include/afis_matcher.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <thread>
#include <chrono>
#include <vector>
#include <sys/mman.h>

#include "afis_device.h"
#include "column_names.h"
#include "pair_moments.h"
#include "template_io.h"
#include <memory>
#include <functional>

namespace afis {

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    hipError_t ensure(size_t n)
    {
        if (n <= bytes) return hipSuccess;
        static const bool trace = getenv("AFIS_ALLOC_TRACE") != nullptr;   // development aid: every (re)allocation of 64 MB or more, with the time it took, on stderr
        const auto t0 = std::chrono::steady_clock::now();
        const size_t was = bytes;
        if (p) { hipError_t e = hipFree(p); p = nullptr; bytes = 0; if (e != hipSuccess) return e; }
        const auto t1 = std::chrono::steady_clock::now();
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        if (trace && n >= ((size_t)64 << 20))
            fprintf(stderr, "alloc: %.3f GB (was %.3f): hipFree %.1f ms, hipMalloc %.1f ms\n", n / 1e9, was / 1e9, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return (T*)p; }
};

}  // namespace afis

using namespace afis;       // (an internal header: every host unit that includes it works inside this namespace)

// One group of latents resident on the device.
struct QueryGroup {
    QueryDev dev;
    DevBuf lm_off, lm_xy, lm_ori, lm_des, lm_frag, lm_tile_off, lt_off, lt_xy, lt_ori, lt_des, tile_off, tile16_off, tex_slot, status;
    int nq = 0; int max_nL = 0; int n_lt_rows = 0; int64_t lut_rows_x_tiles = 0;
    int64_t n_lm_points = 0;             // latent minutiae of the group's three selected templates per query, summed
    bool overlapped = false;             // how the last search scheduled this group (afis_search_resident)
    std::vector<int32_t> h_lt_n;
    std::vector<uint8_t> h_has_lm;       // [nq][3] 1 = the latent carries selected minutiae template s (the host's copy of "lm_off's range is not empty": afis_correspondences_pairs' -1 rule)
    void release() { lm_off.release(); lm_xy.release(); lm_ori.release(); lm_des.release(); lm_frag.release(); lm_tile_off.release(); lt_off.release(); lt_xy.release(); lt_ori.release();
                     lt_des.release(); tile_off.release(); tile16_off.release(); tex_slot.release(); status.release(); }
};

struct afis_queries {
    std::vector<QueryGroup> groups;
    std::vector<int32_t> status;     // per query
    int n_q = 0;
    uint64_t gallery_epoch = 0;      // afis_ctx::gallery_epoch when the handle was uploaded: its launch groups were cut for that shard's size (afis_search_resident refuses it after an edit)
    int64_t max_templates = 0;       // > 0 (afis_queries_upload_reserved): the launch groups were cut for a shard of this many templates; the handle is taken by any shard or subset up to that size, whatever edits happened since
};

// What describes "the shard being searched": the SoA arrays of a set of rolled templates in HBM with their offset tables, the derived layouts, the streams laid out on first
// use and the counts the launch sequence of a search sizes its work by.  The context's resident shard is one instance (afis_ctx derives from it, so that ctx->gal and the
// g_* buffers read as they always did); every live afis_subset holds another, gathered from the resident one on the device (afis_subset.cpp).  The launch sequence
// (afis_search.cpp::search_shard) takes the instance.
struct Shard {
    GalleryDev gal;
    DevBuf g_minu_off, g_minu_xy, g_minu_ori, g_minu_des, g_minu_frag, g_minu_tile_off, g_tex_off, g_tex_xy, g_tex_ori, g_tex_codes, g_tex_codes_cf, g_tex_cf_blk, g_tex_codes_q, g_tex_q_blk, g_tex_t32_blk, g_empty, g_task_ctr;
    DevBuf g_codes_p, g_nrm_p, g_tile_meta;   // adc_variant 9: pair-aligned gallery codes / point terms / pair directory (commit, or first use)
    bool codes_cf_built = false;         // variants 6 / 7 (test library): their lane-ordered code stream and its block offsets, laid out on first use
    bool codes_q_built = false;          // adc_variant 8's lane-ordered code stream is laid out on first use
    bool mf_gal_built = false;           // adc_variant 9's streams above exist
    int64_t q_blocks = 0;
    int64_t t32_tiles = 0;               // tiles of 32 rolled texture points (ceil(n/32) per template): the matrix-core bound pass's stream
    int64_t minu_tiles = 0;              // 16-descriptor tiles in g_minu_frag
    int max_nR = 0;
    int64_t total_tex_points = 0;
    int64_t total_minutiae = 0;          // rolled minutiae of the shard
    int64_t index_base = 0;
    std::vector<uint8_t> res_empty;      // [G] 1 = entry is empty (score -1, rolled_status 2)
    std::vector<int32_t> res_mo, res_to; // [G + 1] the shard's CSR offsets (what g_minu_off / g_tex_off hold): the offset tables are rewritten whole from these
    size_t device_bytes() const
    {
        size_t n = 0;
        for (const DevBuf* b : {&g_minu_off, &g_minu_xy, &g_minu_ori, &g_minu_des, &g_minu_frag, &g_minu_tile_off, &g_tex_off, &g_tex_xy, &g_tex_ori, &g_tex_codes, &g_tex_codes_cf, &g_tex_cf_blk,
                                &g_tex_codes_q, &g_tex_q_blk, &g_tex_t32_blk, &g_empty, &g_task_ctr, &g_codes_p, &g_nrm_p, &g_tile_meta}) n += b->bytes;
        return n;
    }
};

// A candidate list of the resident shard as a sub-shard of its own (afis_subset_create): the listed templates in ASCENDING global index order, so that the rank-list kernel's
// tie rule (ascending position) is the rule on global indices; d_global maps a position back, d_pos is where the caller's column j sits.
struct afis_subset {
    Shard sh;
    int64_t n = 0;
    uint64_t gallery_epoch = 0;          // afis_ctx::gallery_epoch at creation: both search calls refuse the handle after an edit
    bool identity = true;                // the caller listed the indices in ascending order: no column permutation on the way out
    std::vector<int64_t> idx;            // [n] the caller's list (global indices, the caller's order): column j of the outputs
    std::vector<int64_t> held;           // [n] the same indices ascending: the name of every position of the sub-shard (column_names), filled where idx is
    DevBuf d_global, d_pos;              // [n] int64 global index of position t; [n] int32 position of the caller's column j
    size_t device_bytes() const { return sh.device_bytes() + d_global.bytes + d_pos.bytes; }
};

// The enrolled person of every template of the resident shard (afis_subjects_create): the distinct ids in ascending order are the slots 0 .. S-1 of the subject rank
// lists, slot_of maps a template (shard-local index) to its slot.
struct afis_subjects {
    int64_t n = 0, S = 0;                // templates labelled (the resident shard's size at creation), distinct subjects
    uint64_t gallery_epoch = 0;          // afis_ctx::gallery_epoch at creation: afis_rank_subjects refuses the handle after an edit
    std::vector<int64_t> ids;            // [S] ascending (the host's copy: rank lists of k > 64)
    DevBuf d_slot_of, d_ids;             // [n] int32, [S] int64
};

// One attribute word per template of the resident shard (afis_labels_create): what the masks of the filtered hit lists are tested against (hit_filter.hip).
struct afis_labels {
    int64_t n = 0;                       // templates labelled (the resident shard's size at creation)
    uint64_t gallery_epoch = 0;          // afis_ctx::gallery_epoch at creation: the filtered ranking calls refuse the handle after an edit
    DevBuf d_label;                      // [n] uint64
    std::vector<uint64_t> h_label;       // [n] the host's copy: afis_search_eligible lists a class's eligible templates from it
};

// The score matrix the last search left in afis_ctx::scores ([n_q][G] in the order of the shard searched: the resident one, or sub's sub-shard), while nothing has
// touched it or what it refers to: afis_rank_subjects ranks it.  Set by a search that succeeded, cleared by drain_abandoned at the top of every entry point that queues work.
struct LastSearch { bool valid = false; int n_q = 0; int64_t G = 0; const afis_subset* sub = nullptr; uint64_t gallery_epoch = 0; bool normalized = false; };   // (gallery_epoch: the shard the matrix was scored against; normalized: afis_normalize_scores has replaced the scores by z-scores — that call and afis_score_stats refuse the matrix, every search starts a record without the flag)

// A kept matrix (afis_matrix_keep): a device copy of the last search's matrix as it stood, with its record.  rec.valid is unused; rec.sub is cleared — and sub_freed
// set — when the subset it names is freed (afis_subset_free).
struct afis_matrix {
    DevBuf d;                            // [rec.n_q][rec.G] floats in the order of the shard searched; nothing where there is no cell
    LastSearch rec;
    bool over_subset = false, sub_freed = false;
};

struct afis_ctx : Shard {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream_hi = nullptr;     // option bound_cus: the complement of stream_lo's CUs, for the minutiae stage while the bound pass runs
    hipStream_t stream_lo = nullptr;     // option bound_cus: a stream confined to the low N CUs (N / 8 of every XCD) for the power-limited bound pass; the rest of a launch group runs beside it
    int bound_cus = 0;                   // 0 = off: one stream, the kernels of a group back to back
    int n_cus = 0;                       // compute units of the device (hipDeviceProp_t::multiProcessorCount): the CU masks are built for this many
    std::vector<hipEvent_t> evpool;      // 10 per query group + 2: the groups of a search run back to back, timings are read at the end
    std::string err;
    DevBuf codewords, table;
    HostGallery hg;
    // afis_gallery_load into an empty staging area keeps the container MAPPED instead of copying its 50 KB per template into hg: the commit uploads the shard
    // [pend_first, pend_first + pend_count) straight from the mapping.  Anything else that touches the staged gallery first copies it into hg (materialise()).
    std::unique_ptr<GalleryMapping> pend;
    int64_t pend_first = 0, pend_count = 0;
    std::thread staging_reaper;          // returns the staged arrays to the system after the commit (0.5 s per 5 GB), off the caller's path; joined in afis_destroy
    bool committed = false;
    // The live gallery (afis_gallery_reopen / afis_gallery_remove / afis_gallery_export).  `hg` / `pend` hold STAGED templates only; what the host keeps of the resident shard is below.
    bool reopened = false;               // afis_gallery_reopen: the staging calls append to hg / pend again, beside the resident shard, until the next commit
    uint64_t gallery_epoch = 0;          // counts the edits of the resident shard (appending commits, removals)
    std::vector<afis_subset*> subsets;   // live subsets (afis_subset_create .. afis_subset_free; afis_destroy releases what is left)
    int64_t subset_gather_us = 0;        // option subset_gather_us (read-only): device time of the last afis_subset_create's gather launches (HIP events around them)
    std::vector<afis_subjects*> subject_sets;   // live subject handles (afis_subjects_create .. afis_subjects_free; afis_destroy releases what is left)
    LastSearch last_search;
    DevBuf subj_best, subj_out;          // afis_rank_subjects: best[n_q][S] composites (grown on demand), and the three [n_q][k] output arrays behind one another
    int64_t subject_rank_us = 0;         // option subject_rank_us (read-only): device time of the last afis_rank_subjects' launches (HIP events around them)
    DevBuf hits_out;                     // afis_rank_hits / afis_rank_subject_hits: n_hits [n_q] and the two or three [n_q][cap] output arrays behind one another
    int64_t rank_hits_us = 0;            // option rank_hits_us (read-only): device time of the last hit-list call's launches (HIP events around them)
    DevBuf scores_t;                     // afis_rank_latent_hits: the last search's matrix transposed, [n_templates][n_q] (its lists leave through hits_out)
    int64_t rank_latents_us = 0;         // option rank_latents_us (read-only): device time of the last afis_rank_latent_hits' or afis_rank_latent_hits_filtered's launches (the filtered call's filter pass; k_transpose_scores, k_rank_hits)
    int64_t transpose_us = 0, transpose_bytes = 0;   // k_transpose_scores alone in that call — behind the filter pass in a filtered call — (its own pair of events) and the bytes it read and wrote (parity tap afis_debug_transpose_stats)
    DevBuf case_fused, case_tab;         // afis_rank_case_hits / afis_rank_case_subject_hits and their _filtered forms: the fused matrix [n_cases][columns] floats, and the cases' CSR (case_off [n_cases + 1] | member [n_q], int32); the lists leave through hits_out
    int64_t rank_cases_us = 0;           // option rank_cases_us (read-only): device time of the last case-list call's launches, plain or filtered (a filtered call's filter pass; the fold, for subjects behind the maxima's memset, k_subject_best and the drops; then k_rank_hits)
    int64_t case_fuse_us = 0, case_rank_us = 0;   // options case_fuse_us / case_rank_us (read-only): that time's two parts, each from its own pair of events: everything before k_rank_hits, and k_rank_hits
    std::vector<afis_labels*> label_sets;   // live label handles (afis_labels_create .. afis_labels_free; afis_destroy releases what is left)
    DevBuf filt_scores, filt_tab;        // every filtered ranking call (FilterPass): the filtered copy of the matrix [n_q][G] floats, and the call's tables (masks [n_q][3] uint64 | the exclusions' (row, column) pairs, int32 x 2); the lists leave through hits_out
    int64_t rank_filtered_us = 0;        // option rank_filtered_us (read-only): device time of the last filtered call's launches (the filter pass, for subjects the maxima's memset and k_subject_best, the drops; then k_rank_hits)
    int64_t filter_us = 0;               // option filter_us (read-only): of which everything before k_rank_hits, from its own pair of events
    DevBuf pos_tab, pos_out;             // afis_rank_positions / afis_rank_subject_positions / afis_count_before: the call's tables (the targets' composites [m] uint64 | rows | off | row [m] | position [m], int32) and its answers (count [m] uint64 | best_idx [m] int64 | status [m] int32 | score [m])
    int64_t rank_positions_us = 0;       // option rank_positions_us (read-only): device time of the last such call's launches (a filtered call's filter pass, for persons the maxima and the drops; k_position_targets, k_count_before)
    DevBuf stat_tab, stat_out;           // afis_score_stats: the limb table [rows][9] uint64 and the statistics [rows or columns] x 48 bytes; afis_normalize_scores: the (offset, scale) pairs [rows or columns][2] double in stat_tab (its matrix is built in elig_scores and swapped in as afis_search_eligible's is)
    int64_t score_stats_us = 0;          // option score_stats_us (read-only): device time of the last afis_score_stats' launches (the filter pass, the table's memset, the statistics kernels)
    int64_t normalize_us = 0;            // option normalize_us (read-only): device time of the last afis_normalize_scores' launches (k_normalize_scores; for a subset listed out of order the columns' permutation of scores_out)
    DevBuf hist_tab;                     // afis_score_histogram: the counts [rows or columns][n_edges + 1] uint64, then the edges' keys [n_edges] uint32 (axis 1 transposes into scores_t, as afis_rank_latent_hits)
    int64_t score_histogram_us = 0;      // option score_histogram_us (read-only): device time of the last afis_score_histogram's launches (the filter pass, axis 1: the transposition, the table's memset, k_score_hist_rows)
    DevBuf sel_tab, sel_out;             // afis_entries_at: the call's tables (prefix [m] | its spare [m] | remain [m] uint64, the bins [m][256] uint64, rows | off | row [m] | first [m] int32) and its answers (idx [m] int64 | score [m] | status [m] int32)
    int64_t entries_at_us = 0;           // option entries_at_us (read-only): device time of the last afis_entries_at's launches (the filter pass, then per digit the bins' memset, k_select_count and k_select_step; k_select_finish)
    DevBuf subj_keys;                    // afis_subject_score_stats / afis_subject_score_histogram / afis_subject_entries_at: the person cells [n_q][S] uint32, the high halves of subj_best (k_subject_keys); their tables and answers go through the template forms' buffers (stat_tab, stat_out, hist_tab, scores_t, sel_tab, sel_out)
    int64_t subject_score_stats_us = 0, subject_score_histogram_us = 0, subject_entries_at_us = 0;   // options of those names (read-only): device time of the last such call's launches (the filter pass, the maxima's memset, k_subject_best, the drops, k_subject_keys, then the template form's kernels over the person cells)
    DevBuf link_tab, link_out;           // afis_link_groups / afis_link_subject_groups: the call's words (afis_link.cpp has the layout: counters, parent | label | size [n_nodes] int32, the subject form's first_col, the uploaded tables) and the (node, label) pairs of the linked nodes
    int64_t link_groups_us = 0;          // option link_groups_us (read-only): device time of the last such call's launches (the filter pass, the counters' memset, k_link_init, the subject form's two column kernels in mutual mode, k_link_scan, k_link_flatten, k_link_compact)
    int64_t link_d2h_bytes = 0;          // option link_d2h_bytes (read-only): bytes that call returned from the device: 32 of counters, then 8 per linked node
    std::vector<afis_matrix*> matrices;  // live kept matrices (afis_matrix_keep .. afis_matrix_free; afis_destroy releases what is left); option matrix_device_bytes (read-only) is what they hold
    DevBuf fuse_t;                       // afis_matrix_fuse: its transposed operands, one [n][n] matrix per distinct handle read transposed, each on a 256-byte boundary (the result is built in elig_scores and swapped in as afis_search_eligible's is)
    int64_t matrix_keep_us = 0, matrix_fuse_us = 0;   // options of those names (read-only): device time of the last afis_matrix_keep's copy / the last afis_matrix_fuse's launches (k_transpose_scores per distinct transposed operand, k_matrix_fuse), HIP events around them
    int corr_pairs_per_launch = kCorrPairsPerLaunch;   // option corr_pairs_per_launch: pairs per chunk of that call at most
    int64_t correspondences_us = 0;      // option correspondences_us (read-only): device time of the last afis_correspondences_pairs' / afis_correspondences' launches (HIP events around every chunk's, summed)
    DevBuf pair_buf, pair_tex_slab;      // every pair-list call (PairCall below has the layout), grown on demand: one chunk's candidate lists, survivors, counts, parts and tables — about 5.8 KB per pair of option corr_pairs_per_launch for afis_correspondences_pairs; with afis_score_pairs' dense row maxima and scores kScorePairBytes + 8 lt_pad per pair of option score_pairs_per_launch —, and the texture list kernel's slab for a chunk's launches of afis_score_pairs
    int64_t texture_correspondences_us = 0, pair_alignments_us = 0;   // options of those names (read-only): device time of the last afis_texture_correspondences_pairs' / afis_pair_alignments' launches (HIP events around every chunk's, summed), or of their forms' for print pairs, gathers included; both calls chunk by corr_pairs_per_launch
    int score_pairs_per_launch = kScorePairsPerLaunch;   // option score_pairs_per_launch: pairs per chunk of that call at most
    int64_t score_pairs_us = 0;          // option score_pairs_us (read-only): device time of the last afis_score_pairs' launches (HIP events around every chunk's, summed)
    DevBuf elig_scores;                  // afis_search_eligible: the combined matrix [n_q][G] while the classes are searched (every class search overwrites `scores`); swapped with `scores` at the end, so between calls it holds the spare of the two
    int64_t eligible_classes = 0;        // option eligible_classes (read-only): classes (distinct mask triples) of the last afis_search_eligible
    int64_t eligible_expand_us = 0;      // option eligible_expand_us (read-only): device time of that call's k_expand_rows launches, HIP events around each, summed over the classes
    DevBuf wt_tab;                       // afis_search_weighted: one batch's tables (query descriptors [queries][4] int32 | weights [pseudo-queries][4] float); the combined matrix is built in elig_scores and swapped in as afis_search_eligible's is
    int weighted_batch_pseudo = 0;       // option weighted_batch_pseudo: pseudo-queries per batch of that call at most; 0 = as many as an eighth of the group budget holds the per-part scores of
    int64_t weighted_pseudo_queries = 0; // option weighted_pseudo_queries (read-only): pseudo-queries the last afis_search_weighted scored
    int64_t weighted_fold_us = 0;        // option weighted_fold_us (read-only): device time of that call's k_fold_templates launches, HIP events around each, summed over the batches
    int64_t print_gather_us = 0;         // option print_gather_us (read-only): device time of the last afis_search_prints' gather launches (print_queries.hip), HIP events around each group's, summed
    int64_t print_h2d_bytes = 0;         // option print_h2d_bytes (read-only): bytes that call handed to host-to-device copies (the groups' tables and the fold's), counted where the copies are issued
    int print_pairs_batch_prints = 0;    // option print_pairs_batch_prints: query prints per batch (one temporary handle) of afis_score_print_pairs / afis_correspondences_print_pairs at most; 0 = as many as an eighth of the group budget holds the views of
    int64_t print_pairs_us = 0;          // option print_pairs_us (read-only): device time of the last such call's launches, gathers included, summed over batches and chunks
    int64_t print_pairs_query_prints = 0;   // option print_pairs_query_prints (read-only): distinct query prints that call gathered
    DevBuf casc_buf, casc_slab;          // afis_search_cascade: the kept lists, the second stage's pair tables, parts and scores, one chunk's dense row maxima (afis_cascade.cpp has the layout), and the texture list kernel's slab for a chunk's launches; the combined matrix is built in elig_scores and swapped in as afis_search_eligible's is
    int cascade_pairs_per_launch = kCascadePairsPerLaunch;   // option cascade_pairs_per_launch: pairs per chunk of that call's second stage at most
    int64_t cascade_stage1_us = 0, cascade_select_us = 0, cascade_stage2_us = 0;   // options of those names (read-only): device time of the last afis_search_cascade's three parts, each from its own pair of HIP events
    int64_t cascade_kept_pairs = 0;      // option cascade_kept_pairs (read-only): pairs that call's second stage scored
    int64_t print_cascade_stage1_us = 0, print_cascade_select_us = 0, print_cascade_stage2_us = 0;   // options of those names (read-only): device time of the last afis_search_prints_cascade's three parts, each from its own pair of HIP events; the call builds its lists and tables in casc_buf / casc_slab and its matrix in elig_scores, as afis_search_cascade does
    int64_t print_cascade_kept_pairs = 0;   // option print_cascade_kept_pairs (read-only): pairs that call's second stage scored
    DevBuf out_perm;                     // a subset search's scores / parts in the caller's column order (sized before the search queues)
    int64_t gallery_h2d_bytes = 0;       // option gallery_h2d_bytes (read-only): host-to-device bytes of every commit and removal so far
    int64_t compact_us = 0, compact_bytes = 0;   // the last removal's compaction kernels, or the last afis_gallery_commit_at's splice kernels: device time (events around each launch) and the bytes they copied (parity tap afis_debug_compact_stats)
    // adc_variant 9: fp16 codebook + |cw|^2 (once), per group B fragments, row constants and the bound pass's records (the gallery's own streams: Shard)
    DevBuf mf_cw16, mf_cwn, mf_bfrag, mf_rowk, mf_rec, mf_stats;
    bool mf_cb_built = false;
    int mf_collect_stats = 0;
    DevBuf lutq, lutq_min, lutq_rng, lutq_rowc, lut32;      // adc_variant 8: 16-row fixed-point tiles, per-(row, m) min / range, per-row (offset, step, margin), fp32 table
    DevBuf lut, rm_val, rm_arg, rm_cv, rm_n, parts, scores, scratch, cands, cand_n, minu_fb, topk_idx, topk_score;
    // The list kernels' slabs (afis_device.h: kTexSlabWgBytes / kMinuSlabWgBytes per one-wave workgroup of the launch): the neighbour values of S8's power iterations, written in
    // iteration 0 and read back by the later ones.  minu_slab holds TWO instances' worth: the overlapped schedule runs the minutiae list kernel twice at once (side stream + context's stream).
    // Sized with the launch groups' buffers (prepare_search_buffers) and counted in their budget (graph_slab_bytes); nothing in them outlives a kernel.
    DevBuf tex_slab, minu_slab;
    DevBuf diag;                         // kDiagWords unsigned 64-bit counters per launch group of a search (afis_device.h): zeroed when the search starts, read back with its results
    std::vector<unsigned long long> h_diag;
    void* h_pin = nullptr; size_t h_pin_bytes = 0;   // pinned host buffer for what a search reads back inside its wait (rank lists, diagnostics)
    std::vector<float> h_scores, h_parts;
    int adc_variant = 9;                 // 9: fp16 matrix-core bound pass + exact recomputation (default); 8: 16-bit LDS-table bound pass + exact refine; 7: direct exact kernel; 0-3, 6: earlier direct kernels (0-3, 6, 7: test library only)
    int tile_share = 0;                  // adc_variant 8: consecutive chunks per tile on an XCD; 0 = 4 (the refine's fp32 table stays in L2)
    int query_batch = 0;                 // latents per launch group at most; 0 = by shard size (afis_queries_upload); adc_variant 9 places the cuts by latent texture rows
    int chunk = 0;                       // gallery templates per ADC workgroup; 0 = by gallery size
    int minu_generic = 0;
    int s3_tie_order = 0;                // 1: equal candidate norms in the order libstdc++'s std::sort leaves them (matcher.cpp:476); 0: ascending element index
    int s89_tie_order = 0;               // 1 (option ref_tie_order 2): the greedy selections of S8 and S9 walk equal scores in std::sort's order too (graph.hip::sort_scores)
    double search_timeout_s = 600.0;     // bound on every host wait of a search (AFIS_SEARCH_TIMEOUT_S; <= 0: plain hipStreamSynchronize, unbounded)
    int64_t planned_group_bytes = 0;     // per-group buffers the largest launch group uploaded so far will take (group_budget_bytes of OTHER contexts on the device leaves room for it)
    std::vector<afis_queries*> parked_queries;   // query groups a timed-out search may still be reading: freed by drain_abandoned() once the device is back (afis_queries_free parks them here)
    bool search_abandoned = false;       // the last search returned at its deadline: the device may still be working on it (the next search waits for it first)
    bool overlap_failed = false;         // a wait of the overlapped schedule timed out: later searches keep to one stream
    double overlap_cell_ratio = 0.037;   // a launch group runs the overlapped schedule while (latent x rolled minutiae cells) <= this x (latent texture rows x rolled texture points); AFIS_OVERLAP_CELL_RATIO
    int64_t rowmax_budget_bytes = 0;     // device memory a launch group's per-pair buffers may take (option rowmax_budget_mb); 0 = 60 % of what hipMemGetInfo reports free
    afis_timing timing = {};
};

namespace afis {

extern thread_local std::string g_create_error;   // last afis_create failure of THIS thread (there is no context to hang it on)

inline int fail(afis_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}
#define HIPCHK(ctx, call)                                                                                       \
    do { hipError_t e_ = (call); if (e_ != hipSuccess)                                                          \
        return fail(ctx, AFIS_EDEVICE, std::string(#call) + ": " + hipGetErrorString(e_) + (e_ == hipErrorOutOfMemory ?                                      \
            " (device memory: a launch group's buffers are sized from the memory that was free when the queries were uploaded - with several contexts or processes on one "  \
            "device lower option rowmax_budget_mb or query_batch)" : "")); } while (0)
#define AFISCHK(call) do { const int rc_ = (call); if (rc_ != AFIS_OK) return rc_; } while (0)
// a handle outlived an edit of the resident shard; `then`: what the handle was given for, and what to do now
__attribute__((visibility("hidden"))) inline int fail_edited(afis_ctx* ctx, const char* who, const char* then, bool name_calls = true)
{
    return fail(ctx, AFIS_ESTATE, std::string(who) + ": the gallery was edited " + (name_calls ? "(afis_gallery_commit after afis_gallery_reopen, afis_gallery_remove) " : "") + "after " + then);
}

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }   // the parts of a call's device and pinned buffers begin on 256-byte boundaries

struct Events {                                     // the HIP events of one call, 8 at most (for (hipEvent_t& e : ev) creates them), destroyed when it returns
    hipEvent_t e[8] = {};
    const int n;
    explicit Events(int count) : n(count) {}  Events(const Events&) = delete;
    __attribute__((visibility("hidden"))) ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipEvent_t* begin() { return e; }  hipEvent_t* end() { return e + n; }
    hipEvent_t operator[](int i) const { return e[i]; }
};

// the context's pinned read-back buffer, grown to at least `bytes` (nothing may be in flight into it)
inline hipError_t ensure_pin(afis_ctx* ctx, size_t bytes)
{
    if (ctx->h_pin_bytes >= bytes) return hipSuccess;
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    ctx->h_pin = nullptr; ctx->h_pin_bytes = 0;
    const hipError_t e = hipHostMalloc(&ctx->h_pin, bytes, hipHostMallocDefault);
    if (e == hipSuccess) ctx->h_pin_bytes = bytes;
    return e;
}

template <class T, class A>
inline hipError_t upload(DevBuf& b, const std::vector<T, A>& v, hipStream_t s)
{
    hipError_t e = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
    if (e != hipSuccess) return e;
    if (!v.empty()) e = hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    return e;
}

// host-side re-layouts at commit touch every byte of the shard once: split [0, n) over a few threads
template <class F>
void parallel_for(int64_t n, F body)
{
    const int64_t nt = std::min<int64_t>(std::max<int64_t>(1, (int64_t)std::thread::hardware_concurrency()), std::min<int64_t>(16, std::max<int64_t>(1, n / 256)));
    if (nt <= 1) { body((int64_t)0, n); return; }
    std::vector<std::thread> th;
    for (int64_t i = 0; i < nt; ++i) th.emplace_back(body, n * i / nt, n * (i + 1) / nt);
    for (std::thread& t : th) t.join();
}

// Descriptors re-laid as operand fragments of v_mfma_f32_16x16x4_f32 (minu.hip): template t (rows off[t] .. off[t+1]) becomes
// ceil(n/16) tiles of 6 x 64 float4; lane l of load v holds des[16*tile + (l&15)][4*(4v + c) + (l>>4)], c = 0..3.  Rows past the
// template's end are zero.  tile_off[t] = first tile of template t.
template <class Off>
std::vector<float> fragment_tiles(const std::vector<float>& des, const std::vector<Off>& off, std::vector<int32_t>& tile_off)
{
    const int64_t T = (int64_t)off.size() - 1;
    tile_off.assign((size_t)T + 1, 0);
    for (int64_t t = 0; t < T; ++t) tile_off[(size_t)t + 1] = tile_off[(size_t)t] + (int32_t)((off[(size_t)t + 1] - off[(size_t)t] + 15) / 16);
    std::vector<float> out((size_t)tile_off[(size_t)T] * 6 * 64 * 4, 0.0f);
    parallel_for(T, [&](int64_t lo, int64_t hi) {
        for (int64_t t = lo; t < hi; ++t) {
            const int64_t r0 = (int64_t)off[(size_t)t], n = (int64_t)off[(size_t)t + 1] - r0;
            for (int64_t row = 0; row < n; ++row) {
                const float* src = &des[(size_t)(r0 + row) * kDes];
                float* tile = &out[(size_t)(tile_off[(size_t)t] + row / 16) * 6 * 64 * 4];
                const int li = (int)(row & 15);
                for (int v = 0; v < 6; ++v)
                    for (int lg = 0; lg < 4; ++lg)
                        for (int c = 0; c < 4; ++c) tile[((size_t)v * 64 + lg * 16 + li) * 4 + c] = src[4 * (4 * v + c) + lg];
            }
        }
    });
    return out;
}

// Rank lists (of templates: afis_search*; of subjects: afis_rank_subjects) are made on the device for k <= kDeviceTopK (k passes of a workgroup-wide maximum per query); larger k sorts on the host.
constexpr int kDeviceTopK = 64;
constexpr int64_t kMfRecBytesPerRow = 8;               // adc_variant 9: one 8-byte record per (rolled template, latent texture row)
// afis_gallery.cpp
int materialise(afis_ctx* ctx);                        // the staged gallery as host arrays: a container that afis_gallery_load only mapped is copied into ctx->hg now
void free_gallery_dev(Shard* c);                       // every device buffer of a shard (the context's resident one, or a subset's)
int quiesce(afis_ctx* ctx, const char* what, bool keep_last_search = false);   // an edit replaces or releases device buffers that searches read: waits (bounded) for all device work of the context
int ensure_mf_gallery(afis_ctx* ctx, Shard& sh, hipStream_t s);   // adc_variant 9's tile-aligned copy of the gallery codes (built at commit, or by the first search after the variant was selected)
void views_of(const HostTemplate& t, std::vector<afis_minutiae_view>& mv, std::vector<afis_texture_view>& tv, afis_template_view& out);
// afis_search.cpp
// spec == NULL: the reference's selection for every query (templates 27, 3, 12 and texture template 0, matcher.cpp:380-415).
// spec != NULL (afis_match_all_templates): query i uses latent minutiae templates spec[i*4 + 0..2] (-1 = none) and latent texture
// template spec[i*4 + 3] (-1 = none), and is never "latent empty".
int build_group(afis_ctx* ctx, const afis_template_view* qs, int nq, QueryGroup& grp, std::vector<int32_t>& status_out, const int* spec = nullptr);
// (the ADC stages work on the shard `sh`: the context's own — *ctx — or a subset's)
int adc_stage_q(afis_ctx* ctx, Shard& sh, QueryGroup& grp, int chunk, bool exact, hipEvent_t after_lut = nullptr);
int adc_refine_mfma(afis_ctx* ctx, Shard& sh, QueryGroup& grp, bool all_rows, bool compact);
int adc_stage_mfma(afis_ctx* ctx, Shard& sh, QueryGroup& grp, bool all_rows, hipEvent_t after_lut = nullptr, hipEvent_t after_bound = nullptr, bool compact = false, hipStream_t sb = nullptr,
                   bool refine_now = true, unsigned long long* diag = nullptr);
// S4-S6 of the direct exact ADC kernels (adc_direct.hip, adc_variant 0-3, 6, 7) for one query group against a shard, on the context's stream, into
// rm_val / rm_arg (sized by the caller); after_lut is recorded between the table and the row maxima.  Set by afis_taps.cpp, so only libafis_hip_test.so has it:
// null in libafis_hip.so, which rejects those variants.  Hidden: with both libraries in one process, neither may bind to the other's copy.
typedef int (*DirectAdcStage)(afis_ctx* ctx, Shard& sh, const QueryDev& d, int chunk, hipEvent_t after_lut);
extern DirectAdcStage g_direct_adc_stage __attribute__((visibility("hidden")));
int64_t group_budget_bytes(const afis_ctx* ctx);       // device bytes a launch group's buffers may take: option rowmax_budget_mb, or 60 % of what is free
// afis_timing of a call that runs several searches (afis_eligible.cpp; afis_search_eligible, afis_search_weighted): additive fields summed, the clock fields from the search with the most pairs
void add_timing(afis_timing& acc, const afis_timing& t, int64_t& most_pairs) __attribute__((visibility("hidden")));
int64_t graph_slab_bytes(int64_t n_pairs);             // both slabs for a launch of n_pairs (latent, rolled) pairs (1.0 GB + 2 x 0.67 GB from 16 384 pairs on)
int wait_streams(afis_ctx* ctx, std::initializer_list<hipStream_t> streams, const char* what);
void register_context(afis_ctx* ctx); void unregister_context(afis_ctx* ctx);   // the process-wide list group_budget_bytes consults
int drain_abandoned(afis_ctx* ctx, bool keep_last_search = false);   // waits (bounded) for a search that returned at its deadline; the caller is about to queue work: the last search's score matrix is no longer afis_rank_subjects' to rank (unless kept)
// The launch sequence of a search over one shard: the context's resident one (sub == NULL, sh == *ctx) or a subset's (sh == sub->sh).  afis_search_resident and
// afis_search_subset_resident check their handles and call it.
// keep_parts: the per-part scores of all queries stay on the device in ctx->parts [n_q][G][4] and are not copied back (afis_search_weighted folds them there).
int search_shard(afis_ctx* ctx, Shard& sh, const afis_subset* sub, afis_queries* q, float* scores, float* parts, int32_t* status, int k, int64_t* topk_idx, float* topk_score, bool keep_parts = false);
// The rule every call that takes a query handle applies to it: a reserved handle (afis_queries_upload_reserved) while `templates` — the size of what is searched — fits
// what it was cut for, any other handle only in the epoch it was uploaded in.  subset: afis_search_subset_resident's wording (`templates` is the subset's size).
int check_query_handle(afis_ctx* ctx, const char* who, const afis_queries* q, int64_t templates, bool subset = false);
// The minutiae stage of a launch group — the candidate kernel, then the minutiae list kernel — in the one form every driver of the search family queues it in.
//   ensure_minutiae_stage  cands, cand_n, minu_fb, minu_slab (slab_instances instances of the list kernel at once: 2 where the overlapped schedule may run) and the
//                          candidate kernel's scratch, for the LARGEST group of `groups`; the scratch for the largest need of any group (afis_device.h: minu_scratch_bytes).
//                          The only sizing of these buffers in a search: called before anything is queued, nothing below allocates
//   queue_minutiae_stage   launch_minu_cands with the group's own grid (minu_cands_grid), `between` recorded, launch_graph_minutiae, on stream s; the three per-part scores
//                          go to grp_parts [grp.nq][G][4].  shared_counter (the overlapped schedule): the list counter is reset between the two kernels and the list kernel
//                          runs in its `join` form, so that a second instance on another stream may draw from the same counter
//   minutiae_diagnostics   ctx->h_diag's rows of n_groups launch groups summed into acc [kDiagWords] (or a row of its own), and afis_timing's minu_tasks*,
//                          minu_fallback_tasks and cands_clock_ghz from the sum
int ensure_minutiae_stage(afis_ctx* ctx, const Shard& sh, const std::vector<QueryGroup>& groups, int slab_instances);
int queue_minutiae_stage(afis_ctx* ctx, const Shard& sh, const QueryGroup& grp, float* grp_parts, unsigned long long* diag_row, hipStream_t s, hipEvent_t between, bool shared_counter = false);
void minutiae_diagnostics(const afis_ctx* ctx, size_t n_groups, afis_timing& tm, unsigned long long* acc = nullptr);
// The host's rank lists (k > kDeviceTopK) of a score matrix [n_q][G] whose column j is template col[j] (a subset in the caller's order) or index_base + j (col == NULL);
// the parity tap afis_debug_rank_rows runs it too.  Hidden, as rank_subjects below.
void host_rank_rows(const float* sc, int n_q, int64_t G, int k, const int64_t* col, int64_t index_base, int64_t* topk_idx, float* topk_score) __attribute__((visibility("hidden")));
size_t subset_device_bytes(const afis_ctx* ctx);       // option subset_device_bytes: what the live subsets hold on the device
void release_subset(afis_subset* s);                   // its device buffers and the handle itself (afis_subset.cpp)
// Everything of afis_subset_create that touches the device (afis_subset.cpp): sub->n, the host tables of sub->sh (res_mo, res_to, res_empty) and the three lists are the
// caller's — sel [n] shard-local indices ascending, global [n] their global indices, pos [n] the caller's column order (unused while sub->identity).  afis_search_eligible
// builds its temporary sub-shard through it, class after class into the same afis_subset: its buffers only grow.  sel_buf: where the index list goes on the device
// (NULL: a buffer of the call's own, released on return).  Ends in a bounded wait.  Hidden, as rank_subjects below.
int build_subset(afis_ctx* ctx, afis_subset* sub, const std::vector<int32_t>& sel, const std::vector<int64_t>& global, const std::vector<int32_t>& pos, DevBuf* sel_buf = nullptr) __attribute__((visibility("hidden")));
// afis_queries_upload (max_templates == 0: the launch groups are cut for the resident shard's size) and afis_queries_upload_reserved (afis_reverse.cpp: for a shard of
// max_templates templates) behind their argument checks.  Hidden, as rank_subjects below.
// spec != NULL: build_group's selection per query [n_q][4] (afis_search_weighted's pseudo-queries).
int upload_queries(afis_ctx* ctx, const afis_template_view* queries, int n_q, int64_t max_templates, afis_queries** out, const int* spec = nullptr) __attribute__((visibility("hidden")));
// ... and its sibling for query groups that are not made of views: the same cuts from the queries' texture rows (rows [n_q + 1], prefix sums), every group made by
// `build` (first query, queries, the group to fill, the handle's status list to append to).  afis_search_prints fills its groups on the device through it (afis_prints.cpp).
typedef std::function<int(int, int, QueryGroup&, std::vector<int32_t>&)> QueryGroupBuilder;
// keep_last_search: drain_abandoned's (the pair calls for prints build their handles without invalidating the last search's matrix).
int upload_query_groups(afis_ctx* ctx, const std::vector<long long>& rows, int n_q, int64_t max_templates, afis_queries** out, const QueryGroupBuilder& build,
                        bool keep_last_search = false) __attribute__((visibility("hidden")));
// The batches of afis_search_weighted and afis_search_prints: queries [q0, q1) with pseudo-queries [p0, p1) of the call's numbering, cut at query boundaries — at most
// `cap` pseudo-queries; a query with more than that is a batch of its own, a query without pseudo-queries joins the batch that is open.
struct PseudoBatch { int q0, q1; int64_t p0, p1; };
inline std::vector<PseudoBatch> plan_pseudo_batches(const std::vector<int>& n_pq, int64_t cap)
{
    std::vector<PseudoBatch> b;
    int64_t first = 0;
    for (int i = 0; i < (int)n_pq.size(); ++i) {
        if (b.empty() || (b.back().p1 > b.back().p0 && b.back().p1 - b.back().p0 + n_pq[(size_t)i] > cap)) b.push_back(PseudoBatch{i, i, first, first});
        b.back().q1 = i + 1; b.back().p1 += n_pq[(size_t)i];
        first += n_pq[(size_t)i];
    }
    return b;
}
// afis_prints.cpp
// One launch group of afis_search_prints in two steps (the parity tap afis_debug_print_queries runs them too).  prepare_print_group: queries p < n are the prints
// local[p] (shard-local indices of the resident shard) with their minutiae template where use_minu[p] and their texture template where use_tex[p], where the print has
// one — build_group's group for the spec (0 or -1, -1, -1, 0 or -1): the host's copy of the group's tables (the seven query-side tables and the three source offset
// tables, each padded to 16 bytes) in plan.tab, every DevBuf of the group at its size, grp.dev pointing into them; nothing is queued.  res_tile [G + 1]: the first
// fragment tile of every resident template (resident_tile_offsets).  queue_print_group: the tables in one host-to-device copy and the gather (print_queries.hip) on the
// context's stream; plan must live until the stream has passed the copy; *h2d_bytes grows by the bytes handed to the copy; the two events, where given, are recorded around the gather's launches.  Hidden, as rank_subjects below.
struct PrintGroupPlan { std::vector<int32_t> tab; size_t first_at = 0; int n_lm = 0, n_lm_tiles = 0, n_lt = 0; };   // first_at: int32 position of first_minu | first_tile | first_tex in tab
std::vector<int32_t> resident_tile_offsets(const afis_ctx* ctx) __attribute__((visibility("hidden")));
int prepare_print_group(afis_ctx* ctx, const std::vector<int32_t>& res_tile, const int32_t* local, const uint8_t* use_minu, const uint8_t* use_tex, int n, QueryGroup& grp,
                        PrintGroupPlan& plan, std::vector<int32_t>& status_out) __attribute__((visibility("hidden")));
int queue_print_group(afis_ctx* ctx, const QueryGroup& grp, const PrintGroupPlan& plan, int64_t* h2d_bytes, hipEvent_t before_gather = nullptr, hipEvent_t after_gather = nullptr) __attribute__((visibility("hidden")));
// A temporary query handle of n prints' views (afis_search_prints' batches, the batches of the pair calls for prints): the launch groups cut by upload_query_groups from
// the texture rows gathered, every group prepared, its tables and gather queued, then ONE bounded wait on the context's stream.  local / use_minu / use_tex [n] as
// prepare_print_group's; plans: the host's copies of the groups' tables, the caller's to keep until the device is known idle (a timed-out copy may still read them);
// *h2d_bytes and *gather_us grow by the bytes handed to copies and the device time of the gathers.  *q is the caller's to free (afis_queries_free), after a failure too.
int build_print_queries(afis_ctx* ctx, const char* who, const std::vector<int32_t>& res_tile, const int32_t* local, const uint8_t* use_minu, const uint8_t* use_tex, int n,
                        bool keep_last_search, std::vector<PrintGroupPlan>& plans, afis_queries** q, int64_t* h2d_bytes, int64_t* gather_us) __attribute__((visibility("hidden")));
// afis_corr.cpp
// afis_correspondences_pairs behind its argument checks, and what afis_correspondences runs for its one latent: the pairs (query[i], idx[i]) of the query groups `groups`
// (n_q queries in all, status per query) against the resident shard.  part may be NULL.  out_slots 1 (afis_correspondences_print_pairs): counts [n_pairs], xy [n_pairs][120][4]
// and part [n_pairs] hold selected template 0 alone.  The caller has drained the context (drain_abandoned).  Hidden, as rank_subjects below.
int correspondences_pairs(afis_ctx* ctx, const char* who, const std::vector<QueryGroup>& groups, const std::vector<int32_t>& status, int n_q, int64_t n_pairs,
                          const int32_t* query, const int64_t* idx, int32_t* counts, int16_t* xy, float* part, int out_slots = 3) __attribute__((visibility("hidden")));
// afis_evidence.cpp
// afis_texture_correspondences_pairs and afis_pair_alignments behind their argument checks, over the query groups `groups` as correspondences_pairs above; pt, sim and part
// may be NULL.  records 2 (afis_print_pair_alignments): out [n_pairs][2] holds scorer 0's record and the texture scorer's.  They count their device time in
// ctx->texture_correspondences_us / ctx->pair_alignments_us.  The caller has drained the context.  Hidden, as rank_subjects below.
int texture_correspondences_pairs(afis_ctx* ctx, const char* who, const std::vector<QueryGroup>& groups, const std::vector<int32_t>& status, int n_q, int64_t n_pairs,
                                  const int32_t* query, const int64_t* idx, int32_t* counts, int16_t* xy, int16_t* pt, float* sim, float* part) __attribute__((visibility("hidden")));
int pair_alignments(afis_ctx* ctx, const char* who, const std::vector<QueryGroup>& groups, const std::vector<int32_t>& status, int n_q, int64_t n_pairs,
                    const int32_t* query, const int64_t* idx, int32_t* pair_status, afis_corr_moments* out, int records = 4) __attribute__((visibility("hidden")));
// afis_pairs.cpp
// afis_score_pairs behind its argument checks: the pairs (query[i], idx[i]) of the handle q against the resident shard.  The caller has drained the context.
// fold != NULL (afis_score_print_pairs): q's queries are prints' views; w_minu / w_tex [n_pairs] are the pairs' weights — zero where the query print does not hold the
// template — the fusion is launch_fold_print_pairs and parts is [n_pairs][2].  Counts its device time in ctx->score_pairs_us.  Hidden, as rank_subjects below.
struct PrintPairWeights { const float* w_minu; const float* w_tex; };
int score_pairs(afis_ctx* ctx, const char* who, afis_queries* q, int64_t n_pairs, const int32_t* query, const int64_t* idx, int32_t* status, float* score, float* parts,
                const PrintPairWeights* fold = nullptr) __attribute__((visibility("hidden")));
// The texture stage of one pair table — [count | (query of the group qd, template of gal) x n] on the device, with its work list seg (pair_tables.h) — as the pair calls
// and stage 2 of every cascade (CascadeCall::run) queue it: launch_adc_pairs -> the dense row maxima rm_val / rm_arg [n][qd.lt_pad], launch_graph_texture_pairs ->
// parts[4 p + 3] (slab: the list kernel's, sized by the caller for its largest table) and, where score is given, launch_fuse_pairs -> score[p]
int queue_texture_pairs(afis_ctx* ctx, const GalleryDev& gal, const QueryDev& qd, const int32_t* pair_tab, int n, const int32_t* seg, int n_seg, float* rm_val, int32_t* rm_arg,
                        float* parts, const DevBuf& slab, float* score_or_null, hipStream_t stream, MinuCand* tap_out = nullptr, int32_t* tap_n = nullptr) __attribute__((visibility("hidden")));   // (tap: launch_graph_texture_pairs', the evidence calls')
// One pair-list call, whatever it returns: the pairs (query[i], idx[i]) of a handle's launch groups against the resident shard, in chunks of `per_launch` pairs, every
// chunk one launch sequence with one upload and one copy back.  correspondences_pairs and score_pairs state what differs — the constants below and four callbacks —
// run() is everything else, in this order:
//   checks          *us = 0; query[] inside 0 .. n_q - 1; the groups add up to n_q
//   needs_device(i) after the checks: the list of pairs that go to the device, in the caller's order; P = the pairs of a chunk at most
//   room            the candidate grid (minu_cands_pairs_grid), scratch, minu_slab, with texture the call's texture slab, the call's device buffer ctx->pair_buf and the
//                   pinned buffer: every allocation precedes the first write into the caller's arrays and everything queued — a failed one leaves the arrays untouched
//   defaults()      what the caller's arrays hold without the device; no pair for the device: done
//   per chunk       the tables in pinned memory (pair_tables.h::build_pair_tables: slots by launch group, then latent), event 0, ONE upload (the weights in slot order
//                   behind it), per launch group with pairs launch_minu_cands_pairs, launch_graph_minutiae_pairs and stage(group), event 1, ONE copy back,
//                   wait_elapsed, *us += the chunk's device time, then take(i, slot, back) for every slot: the caller's pair i from slot `slot` of the pinned copy
// ctx->pair_buf, every area on a 256-byte boundary (P pairs, n_grp launch groups, lt_pad the handle's longest texture template):
//   cands [3 P][120] | cand_n [3 P] | texture: rm_val [P][lt_pad] | rm_arg [P][lt_pad] | survivors [3 P][120] | their counts [3 P] | parts [P][4] | texture: score [P] |
//   tab 2 P + n_grp ints, with texture the work list behind it, 2 P more | weights [P][2]
// An area the call does not use takes no room.  What returns is one run of it — parts | score with texture, else survivors | counts | parts —, to the start of the pinned
// buffer; behind it, in pinned memory too, a chunk's tables and weights on their way up (so that an early return leaves nothing queued that reads memory of this call).
struct PairGroup {                                  // one launch group's share of a chunk, for stage(): its pair table and, of every per-pair area, the group's first slot
    const QueryDev& qd; const int32_t* tab; int n; const int32_t* seg; int n_seg;
    float* parts; float* rm_val; int32_t* rm_arg; float* score; const float* weights;
    PairEvidence ev;                                // the evidence form: the group's first slot of the survivors, the texture tap and the call's outputs (all NULL otherwise)
};
struct PairBack {                                   // the pinned copy's areas (slot 0 of each; NULL: not returned)
    const short4* corr; const int32_t* corr_n; const float* parts; const float* score;
    const int32_t* ex_n = nullptr; const float* ex_part = nullptr; const short4* ex_xy = nullptr; const short2* ex_pt = nullptr; const float* ex_sim = nullptr;   // evidence kPairTexExport
    const CorrMoments* mom = nullptr;               // evidence kPairMoments: [4] per slot
};
enum { kPairNoEvidence = 0, kPairTexExport = 1, kPairMoments = 2 };
struct __attribute__((visibility("hidden"))) PairCall {
    afis_ctx* const ctx; const char* const who;
    const std::vector<QueryGroup>& groups; const int n_q; const int64_t n_pairs; const int32_t* const query; const int64_t* const idx;
    const int per_launch; int64_t* const us;        // the options the caller names: pairs per chunk at most, the device time summed over the chunks
    const bool texture;                             // the score form: row maxima, scores and the work list have room, pair_tex_slab is sized, parts | score return
    const PrintPairWeights* const weights;          // a print pair's two weights [n_pairs] each (NULL: no such area)
    const int evidence = kPairNoEvidence;           // the evidence form (with texture): the texture list kernel's tap [P][200] | [P] has room, and what pair_evidence.hip makes of a
                                                    // chunk's lists returns INSTEAD of parts | score — kPairTexExport: ex_n [P] | ex_part [P] | ex_xy [P][200] | ex_pt [P][200] |
                                                    // ex_sim [P][200], 3 208 bytes a pair; kPairMoments: mom [P][4], 288 bytes a pair.  These areas lie behind the weights
    std::function<bool(int64_t)> needs_device;
    std::function<void()> defaults;
    std::function<int(const PairGroup&)> stage;     // (empty: nothing follows the minutiae launches)
    std::function<void(int64_t, size_t, const PairBack&)> take;
    int run();
};
// afis_subjects.cpp
void release_subjects(afis_subjects* s);               // its device buffers and the handle itself
// afis_rank_subjects behind its argument checks; the parity tap afis_debug_rank_subjects runs it too.  Hidden, as g_direct_adc_stage: each library calls its own copy.
int rank_subjects(afis_ctx* ctx, afis_subjects* subj, int n_q, int k, int64_t* subject_id, float* subject_score, int64_t* best_idx) __attribute__((visibility("hidden")));
// afis_hits.cpp
// afis_rank_hits (subj == NULL: out_a = idx, out_b unused) and afis_rank_subject_hits (out_a = subject_id, out_b = best_idx) behind their argument checks.  Hidden, as rank_subjects.
int rank_hits(afis_ctx* ctx, afis_subjects* subj, int n_q, float min_score, int cap, int64_t* n_hits, int64_t* out_a, float* out_score, int64_t* out_b) __attribute__((visibility("hidden")));
// The checks of the ranking calls, in the order every entry point makes them: a live subject handle of this context — the call's plain arguments (check_hits: the hit
// lists'; afis_rank_subjects has its own) — then a committed gallery, a handle that labels the shard as it stands, the last search's matrix still there, and its n_q
int check_subject_handle(afis_ctx* ctx, const char* who, const afis_subjects* s) __attribute__((visibility("hidden")));
int check_last_search(afis_ctx* ctx, const char* who, int n_q, const afis_subjects* s) __attribute__((visibility("hidden")));
int check_hits(afis_ctx* ctx, const char* who, int n_q, float min_score, int cap, bool outputs, const afis_subjects* s) __attribute__((visibility("hidden")));
inline const long long* global_map(const LastSearch& ls) { return ls.sub ? ls.sub->d_global.as<long long>() : nullptr; }   // a position of the last search's matrix -> global index: NULL (index_base + position) or the subset's table
// k_subject_best over `matrix`, laid out as the last search's, into ctx->subj_best [n_q][S] (sized by the caller): the maxima every subject list is made of
int queue_subject_best(afis_ctx* ctx, const afis_subjects* subj, const float* matrix) __attribute__((visibility("hidden")));
// the end of a ranking call's device work: the bounded wait on the context's stream (a failed one clears last_search.valid), then the device time from the call's first event to its last and, where asked for, either side of ev[1]
int wait_elapsed(afis_ctx* ctx, const char* who, const Events& ev, int64_t* total_us, int64_t* first_us = nullptr, int64_t* second_us = nullptr) __attribute__((visibility("hidden")));
// What k_rank_hits ranks: scores [rows][cols], entry e of a row named map[e] or base + e — or, with a subject handle, the slots of ctx->subj_best [rows][S] as
// queue_subject_best(subj, scores) left them (map / base then name a slot's best template).  The template form compares rank_key, the subject form the raw ordered word
struct HitMatrix { const float* scores; int64_t cols; const afis_subjects* subj; const long long* map; long long base; };
// One hit-list call, whatever it ranks: the entry points (afis_hits.cpp, afis_cases.cpp, afis_filter.cpp, afis_reverse.cpp) supply what differs, between its steps:
//   empty(nothing was scored)   no list, or n_hits = 0 and padding: no device work
//   begin(uploads)              after hipSetDevice and the caller's DevBuf::ensure()s: the rest of the room (every allocation precedes all device work: a failed one leaves
//                               everything as it was), the caller's tables to the device — not timed; the host arrays live until finish() returns — then event 0
//   finish(matrix, min_score)   after the caller's pre-passes: event 1, k_rank_hits, event 2, the lists to the pinned buffer, wait_elapsed, the lists into the caller's
//                               arrays — list t as row out_row[t] (NULL: t).  total_us spans events 0 - 2, pre_us 0 - 1, rank_us 1 - 2; all 0 until finish() succeeds
// rows: lists (queries, cases, prints); out_b NULL: the two-array form; hits_out and its pinned copy hold n_hits [rows] | a [rows][cap] | b [rows][cap] | score [rows][cap]
struct __attribute__((visibility("hidden"))) HitCall {
    afis_ctx* const ctx; const char* const who; const int64_t rows; const int cap;
    int64_t* const n_hits; int64_t* const out_a; float* const out_score; int64_t* const out_b;
    const size_t n_out = (size_t)rows * (size_t)cap, a_at = (size_t)rows * 8, b_at = a_at + n_out * 8, score_at = b_at + (out_b ? n_out * 8 : 0), out_bytes = score_at + n_out * 4;
    Events ev{3}; int64_t total_us = 0, pre_us = 0, rank_us = 0;
    struct H2D { void* dst; const void* src; size_t bytes; };                // (bytes 0: nothing to upload)
    bool empty(bool nothing_scored);
    int begin(std::initializer_list<H2D> uploads = {});
    int finish(const HitMatrix& m, float min_score, const int32_t* out_row = nullptr);
};
// afis_filter.cpp
void release_labels(afis_labels* l);                   // its device buffer and the handle itself
// The checks every filtered ranking call shares (afis_filter.cpp, afis_cases.cpp, afis_reverse.cpp), in the order of afis_rank_hits_filtered's: a live labels handle of this
// context, masks with labels, check_hits, labels of the shard as it stands, a valid CSR.  On AFIS_OK pairs holds the exclusions that name something the last search
// covered, as (row, column of the matrix — or slot of s)
int check_filtered(afis_ctx* ctx, const char* who, const afis_subjects* s, const afis_labels* labels, const uint64_t* masks, const int64_t* excl_off, const int64_t* excl,
                   int n_q, float min_score, int cap, bool outputs, std::vector<int32_t>& pairs) __attribute__((visibility("hidden")));
// The filter pass of a filtered ranking call, whatever it ranks afterwards — the one definition of eligibility on the device (hit_filter.hip).  Between HitCall's steps:
//   ensure()           with the caller's DevBuf::ensure()s: the filtered copy and the call's tables (masks | pairs)
//   masks_up/pairs_up  the two uploads, for HitCall::begin
//   queue_cells()      after begin(): the copy — launch_filter_rows, or a device-to-device copy where only cells are dropped — and the excluded templates' cells;
//                      matrix() is then what the call ranks, folds or transposes: the copy, or the search's matrix itself where no cell changed
//   queue_drop_subjects(S)  after queue_subject_best(matrix()): the excluded persons out of ctx->subj_best
// subjects: pairs name (row, slot) and are dropped from the maxima, not from the cells.  filters() false: nothing is allocated, uploaded or queued
struct __attribute__((visibility("hidden"))) FilterPass {
    afis_ctx* const ctx; const afis_labels* const labels; const uint64_t* const masks; const std::vector<int32_t>& pairs; const bool subjects;
    const int n_q = ctx->last_search.n_q; const int64_t G = ctx->last_search.G;
    const size_t n_pairs = pairs.size() / 2, mask_bytes = masks ? (size_t)n_q * 24 : 0, tab_bytes = mask_bytes + n_pairs * 8;
    const bool copy = masks || (!subjects && n_pairs > 0);              // the copy is needed where cells change: by the masks, or by a template's exclusions
    bool filters() const { return masks || n_pairs > 0; }
    hipError_t ensure();
    HitCall::H2D masks_up() const { return {ctx->filt_tab.p, masks, mask_bytes}; }
    HitCall::H2D pairs_up() const { return {ctx->filt_tab.as<uint8_t>() + mask_bytes, pairs.data(), n_pairs * 8}; }
    const float* matrix() const { return copy ? ctx->filt_scores.as<float>() : ctx->scores.as<float>(); }
    int queue_cells();
    int queue_drop_subjects(int64_t S);
};
// afis_distribution.cpp
// The person cells of a person distribution call (afis_distribution.cpp, afis_normalize.cpp): ensure_subject_keys with the caller's other DevBuf::ensure()s — subj_best
// and subj_keys [n_q][S] —; queue_subject_keys after the uploads: afis_rank_subject_hits_filtered's pre-passes, unchanged and in its order (fp.queue_cells(),
// queue_subject_best(fp.matrix()), fp.queue_drop_subjects(S)), then k_subject_keys -> ctx->subj_keys
hipError_t ensure_subject_keys(afis_ctx* ctx, const afis_subjects* subj) __attribute__((visibility("hidden")));
int queue_subject_keys(afis_ctx* ctx, const afis_subjects* subj, FilterPass& fp) __attribute__((visibility("hidden")));
// One call that reads the last search's matrix in place, whatever it computes (afis_hits.cpp; the entry points: afis_positions.cpp, afis_normalize.cpp, afis_distribution.cpp,
// afis_link.cpp): behind their checks — the filtered ranking calls' (check_filtered) — and defaults — no cell or no covered target: no device work — the entry points state their
// buffers, uploads and kernels and read the pinned copy; the filter runs as it runs for the hit lists (fp: no second definition of eligibility); the matrix stays as it is.
//   room(own, pin_bytes)   hipSetDevice, fp.ensure(), the person cells' buffers, the call's own DevBufs in the order given (0 bytes: not needed), the pinned buffer:
//                          every allocation precedes the first write into a caller's array and everything queued — a failed one leaves everything as it was
//   begin(uploads)         the two events, the call's tables, then the masks and the exclusions, to the device — not timed; the host arrays live until finish() returns —, event 0,
//                          the pre-passes of `cells`: the kernels then read fp.matrix() — the filtered copy, or the search's matrix itself —, ctx->subj_best or ctx->subj_keys
//   finish(src, bytes, us) after the call's kernels: event 1, `bytes` of src to the pinned buffer, wait_elapsed; *us = the device time between the events, on success only (more to return: afis_link.cpp)
enum { kTemplateCells = 0, kPersonBest = 1, kPersonKeys = 2 };              // the cells of the matrix; afis_rank_subject_hits_filtered's maxima; ensure_ / queue_subject_keys above
struct __attribute__((visibility("hidden"))) MatrixCall {
    afis_ctx* const ctx; const char* const who; const afis_subjects* const subj; const int cells;   // subj: the handle of a person form (unused with kTemplateCells)
    FilterPass fp; Events ev{2};                    // fp holds a REFERENCE to the caller's pairs: a named vector that outlives the call, never a temporary
    int room(std::initializer_list<std::pair<DevBuf*, size_t>> own, size_t pin_bytes);   // (a buffer of the call's own, the bytes it needs)
    int begin(std::initializer_list<HitCall::H2D> uploads = {});
    int finish(const void* src, size_t bytes, int64_t* us);
};
// The names of what the last search covered — a handle's ids, else index_base + position or a subset's afis_subset::held: what resolves exclusions, targets and row_node
ColumnNames column_names(const afis_ctx* ctx, const afis_subjects* s) __attribute__((visibility("hidden")));
// afis_normalize.cpp
// order[t]: the caller's column of position t of the last search's matrix — a subset listed out of order stands in ascending global index order on the device; empty: the identity
std::vector<int32_t> column_order(const LastSearch& ls) __attribute__((visibility("hidden")));
// afis_matrix.cpp
void release_matrix(afis_matrix* m);                   // its device buffer and the handle itself
size_t matrix_device_bytes(const afis_ctx* ctx);       // option matrix_device_bytes: what the live kept matrices hold on the device
void matrices_lose_subset(afis_ctx* ctx, const afis_subset* s);   // afis_subset_free: the context's kept matrices that were scored over s are stale from here on
// afis_cascade.cpp
// One cascade call, whatever its queries are: the minutiae stage for every cell, the selection of the `keep` best columns per query, the texture scorer for the kept
// cells.  The driver owns the launch sequence, the layout of casc_buf and of the pinned buffer, the times and the ends of the entry points; afis_search_cascade and
// afis_search_prints_cascade (afis_print_cascade.cpp) state their queries and the kernels that differ.  In the order of a call:
//   clear()         the four options (opts: stage 1, selection, stage 2 in us, kept pairs) to 0
//   empty(rc, ..)   n_q == 0 or G == 0, rc the answer of the empty search: no list holds anything
//   check_limits()  n_q x keep and n_q x G within what one call takes
//   run(..)         after the caller has filled in groups .. finish: the pair tables' structure (cascade_tables.h), room for everything before anything is queued, the
//                   tables with the caller's extra ones to the device through the pinned buffer (h2d_bytes), stage 1 group after group (queue_minutiae_stage,
//                   fuse_group), fuse_all, launch_rank_hits, the combined matrix in ctx->elig_scores filled with the no-entry word, gather, per piece
//                   queue_texture_pairs (with the fusion where fuse_pairs), finish, the read-back, ONE bounded wait, the options, afis_timing (stage 1), the
//                   kept lists into the caller's arrays, the two matrices swapped
//   end(rc, scores) the scores copy; after a failure the bounded wait, the call's buffers released, options and timing cleared; last_search either way
struct CascadeTables;
struct __attribute__((visibility("hidden"))) CascadeCall {
    afis_ctx* const ctx; const char* const who; const int n_q, keep;
    int64_t* const opts[4];
    const int kept_w;                               // floats of kept_parts per kept cell
    const bool own_kept_parts;                      // kept_parts is a device array of the call's own [n_q][keep][kept_w], zeroed before gather(), that finish() fills; false: the kept cells' pair parts, through q_slot
    // the caller's, before run()
    afis_subset* sub = nullptr;                     // the sub-shard the call runs over — stage 1, the selection (its d_global names the kept prints) and the pair kernels —; NULL: the resident shard, positions named index_base + position
    bool own_matrix = true;                         // run() sizes ctx->elig_scores [n_q][G of the shard], fills it with the no-entry word and swaps it in; false (afis_search_cascade_eligible: one combined matrix for all classes): the caller's to size, fill and swap
    std::vector<QueryGroup>* groups = nullptr;      // the launch groups of the handle whose (pseudo-)queries stage 1 scores (NULL: none); their per-part scores lie in ctx->parts in the handle's order
    std::vector<int32_t> q_first;                   // [groups + 1] the query of the CALL every group begins at (cascade_tables.h), n_q last
    std::vector<uint8_t> has;                       // [n_q] 1 = the query's kept cells are pairs of stage 2
    bool fuse_pairs = false;                        // a piece ends in launch_fuse_pairs -> d_pscore
    std::function<void(std::vector<int32_t>&)> extra_tables;          // appends to the tables that go up (t->dev first): they then stand at d_dev + their position
    std::function<int(const QueryGroup&, int)> fuse_group;            // (group, its first query of the handle) after a group's list kernel: stage 1's matrix from the parts, timed per group as fuse_ms
    std::function<int()> fuse_all, gather, finish;                    // stage 1's matrix in one launch behind the groups (fuse_ms), the pair tables from the kept lists, the kept cells into ctx->elig_scores
    // run()'s, for the caller's kernels
    const CascadeTables* t = nullptr;
    int nk = 0; long long base = 0;                 // min(keep, G), ctx->index_base
    long long* d_kept = nullptr; const int32_t* d_dev = nullptr; const int32_t* d_q_slot = nullptr; int32_t* d_tab = nullptr;
    float* d_pparts = nullptr; float* d_pscore = nullptr; float* d_kparts = nullptr;    // pair parts [total][4], pair scores [total], own_kept_parts' array
    int64_t h2d_bytes = 0;
    Shard& shard() const { return sub ? sub->sh : static_cast<Shard&>(*ctx); }
    void clear() { for (int64_t* o : opts) *o = 0; }
    int empty(int rc, int64_t* n_kept, int64_t* kept_idx, float* kept_parts);
    int check_limits();
    int run(int64_t* n_kept, int64_t* kept_idx, float* kept_parts);
    int end(int rc, float* scores);
};
// Where a latent cascade over a sub-shard reads and writes (afis_cascade_eligible.cpp; the kernels of cascade_mapped.hip): inv [templates of the resident shard] the
// sub-shard position of a resident position or -1, out_col [m] the column of the combined matrix a sub-shard position is written to, row_of [n_q] its row — each may be
// empty: the identity —, and the matrix ctx->elig_scores as [out_rows][out_stride].  The three tables go up with the call's other tables
struct CascadeMap { const std::vector<int32_t>* inv; const std::vector<int32_t>* out_col; const std::vector<int32_t>* row_of; int64_t out_rows, out_stride; };
// afis_search_cascade's side of the driver behind its argument checks: the handle's queries and groups, the kernels of cascade.hip — with map == NULL its gather and
// scatter for the resident shard, else cascade_mapped.hip's pair — and the driver's run.  Hidden, as rank_subjects above.
int latent_cascade(CascadeCall& c, afis_queries* q, const CascadeMap* map, int64_t* n_kept, int64_t* kept_idx, float* kept_parts) __attribute__((visibility("hidden")));
// afis_eligible.cpp: the class plan of a batch (afis_search_eligible, afis_search_cascade_eligible) and the host side of a class's temporary sub-shard
// one class: the queries (ascending position) that share a mask triple, and the templates of the shard (ascending shard-local index) the triple passes
struct EligClass {
    uint64_t any_of, all_of, none_of;
    std::vector<int32_t> rows, sel;
};
// classes in order of first query position; a triple of zeros lists every template without looking at the labels
std::vector<EligClass> plan_classes(const std::vector<uint64_t>& label, int64_t G, const uint64_t* masks, int n_q) __attribute__((visibility("hidden")));
// the host side of a temporary sub-shard, as afis_subset_create lays it out for a list that is already ascending; what an earlier class built in the same buffers goes
void plan_sub_shard(afis_ctx* ctx, afis_subset* sub, const std::vector<int32_t>& sel, std::vector<int64_t>& global) __attribute__((visibility("hidden")));

}  // namespace afis
