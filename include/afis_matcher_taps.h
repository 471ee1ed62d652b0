/* afis_matcher_taps.h — parity-test taps of the MI355X matcher: stage intermediates the tests compare with oracle/ bit for bit.
 * TEST INFRASTRUCTURE: exported by libafis_hip_test.so only (csrc/Makefile: the product objects plus afis_taps.cpp and adc_direct.hip); the product
 * library libafis_hip.so (include/afis_matcher.h) does not contain them. */
#ifndef AFIS_MATCHER_TAPS_H
#define AFIS_MATCHER_TAPS_H

#include "afis_matcher.h"

#ifdef __cplusplus
extern "C" {
#endif

/* S4: the per-query LUT of queries[0].tex[0], out = [n][16][256] in the reference's m_dist_codewords layout. */
int afis_debug_lut(afis_ctx* ctx, const afis_template_view* query, float* out, int32_t* n_rows);
/* S5+S6: row maxima / first arg-max of latent texture 0 vs gallery template g (g is shard-local). */
int afis_debug_texture_rowmax(afis_ctx* ctx, const afis_template_view* query, int64_t g,
                              float* val, int32_t* arg, int32_t* n_rows);

/* S3 / S7 / S8 / S9: the correspondence list of (query, gallery template g) inside one scorer, as (sim, latent index, rolled
 * index) triples in list order.  which: 0 = texture scorer, 1..3 = minutiae scorer of selected latent template 27 / 3 / 12;
 * stage: 0 = the candidates (top 120 / top 200), 1 = after the distance filter, 2 = after the angle filter.  Capacity 200.
 * *n = -1 when the reference does not run that scorer for the pair. */
int afis_debug_stage_list(afis_ctx* ctx, const afis_template_view* query, int64_t g, int which, int stage,
                          float* sim, int32_t* li, int32_t* ri, int32_t* n);

/* S9: the angle stage's atan2 (matching/matcher.cpp:1516, :1524) on every integer coordinate difference of the grid
 * [-R, R]^2: out[(dy + R) * (2R + 1) + (dx + R)] = line angle atan2(dy, dx) as the device evaluates it.  R <= 4096. */
int afis_debug_atan2_grid(afis_ctx* ctx, int R, float* out);

/* S8: the distance stage's packed arithmetic (csrc/graph_arith.h: a one-transcendental correctly rounded square root of integers and
 * a square-root-free "H != 0" test with a guard band) against the plain evaluation of matching/matcher.cpp:1246-1272, :1372-1393 that
 * it replaces, on the device.  out8[0] = integers n in [0, 2*2047^2] whose root differs; out8[1..3] = texture pairs checked (all of
 * [0, 4802]^2), pairs inside the guard band, wrong decisions; out8[4..6] = the same for minutiae pairs near the 30 px threshold
 * (4e8 of them).  out8[0], [3], [6] must be 0. */
int afis_debug_graph_arith(afis_ctx* ctx, unsigned long long* out8);
/* adc_variant 9 with afis_set_option("mf_stats", 1): counters of the selection / recomputation kernel since the last reset:
 * out8[0] pairs, [1] latent rows, [2] rows evaluated exactly, [3] candidate cells evaluated, [4] rows evaluated over every point,
 * [5] rows whose exact maximum lay outside the bounds the selection used (a self-check: must be 0). */
int afis_debug_refine_stats(afis_ctx* ctx, unsigned long long* out8, int reset);

/* The compaction kernels of the last afis_gallery_remove, or the splice kernels of the last afis_gallery_commit_at, whichever edit came last (gallery_edit.hip):
 * out2[0] = their device time in microseconds (HIP events around each of the six launches, summed), out2[1] = the bytes they copied.  tools/bench_live_gallery.py sets
 * the removal's beside a device-to-device copy of the same bytes; tools/bench_gallery_replace.py reports the replace's. */
int afis_debug_compact_stats(afis_ctx* ctx, long long* out2);

/* Subject rank lists (afis_rank_subjects) over a caller-made score matrix: scores [n_q][G] for the resident shard is uploaded in place of the matrix a search leaves,
 * marked valid as a full search of n_q queries marks it, and ranked by the code afis_rank_subjects runs — score patterns (ties, zeros of both signs, infinities, NaN) that
 * no search produces on demand.  Outputs as afis_rank_subjects'. */
int afis_debug_rank_subjects(afis_ctx* ctx, afis_subjects* subjects, const float* scores /*[n_q][G]*/, int n_q, int k,
                             int64_t* subject_id, float* subject_score, int64_t* best_idx);

/* Hit lists (afis_rank_hits, afis_rank_subject_hits) over a caller-made score matrix, uploaded and marked valid as afis_debug_rank_subjects does, then ranked by the code
 * of the two entry points: subjects == NULL gives template hits (out_a = idx; out_b is ignored), a handle gives subject hits (out_a = subject_id, out_b = best_idx).
 * The matrix stays rankable afterwards, so that the entry points themselves can be called on it. */
int afis_debug_rank_hits(afis_ctx* ctx, afis_subjects* subjects, const float* scores /*[n_q][G]*/, int n_q, float min_score, int cap,
                         int64_t* n_hits /*[n_q]*/, int64_t* out_a /*[n_q][cap]*/, float* out_score /*[n_q][cap]*/, int64_t* out_b /*[n_q][cap] or NULL*/);

/* Column hit lists (afis_rank_latent_hits) over a caller-made score matrix, uploaded and marked valid as afis_debug_rank_hits does (a full search of n_q queries over the
 * resident shard), then ranked by the entry point itself with n_templates = the resident shard's size.  The matrix stays rankable afterwards. */
int afis_debug_rank_latent_hits(afis_ctx* ctx, const float* scores /*[n_q][G]*/, int n_q, float min_score, int cap, int64_t latent_base,
                                int64_t* n_hits /*[G]*/, int64_t* latent_idx /*[G][cap]*/, float* score /*[G][cap]*/);
/* The rank list of afis_search* (topk_idx / topk_score) over a caller-made score matrix: scores [n_q][n] is uploaded in place of the matrix a search leaves, marked valid as
 * a full search (subset == NULL: n = the resident shard's size, column j = template index_base + j) or a subset search of n_q queries marks it, and listed by the code
 * the search itself runs: for k <= 64 the rank-list kernel with the base the search passes, then the subset's index map; for k > 64 the host's list over the columns in the
 * order the search hands it (the caller's order of the subset's list, restored on the device when the subset was listed out of order).
 * For a subset the caller supplies the columns in the order the device holds them: column t belongs to the t-th SMALLEST listed index (n = the subset's size).
 * k >= 1.  Outputs as afis_search's, padding (-1, -inf) included.  The matrix stays rankable afterwards (afis_rank_hits, afis_rank_subjects, afis_rank_latent_hits). */
int afis_debug_rank_rows(afis_ctx* ctx, afis_subset* subset, const float* scores /*[n_q][n]*/, int n_q, int k,
                         int64_t* topk_idx /*[n_q][k]*/, float* topk_score /*[n_q][k]*/);
/* The transpose of the last afis_rank_latent_hits (latent_rank.hip: k_transpose_scores): out2[0] = its device time in microseconds (a pair of HIP events of its own),
 * out2[1] = the bytes it read and wrote; both 0 when that call queued nothing.  tools/reverse_search_timing.py turns them into bytes per second. */
int afis_debug_transpose_stats(afis_ctx* ctx, long long* out2);
/* The expand pass of afis_search_eligible (eligible_expand.hip: k_expand_rows) on planted data, so that its shapes are swept without a search: cls [n_c][m] stands for
 * the rows of one class scored against m of G templates, sel [m] the columns those templates have in the combined matrix, strictly ascending in [0, G) — NULL with
 * m == G is the identity (the class that passes every template), m == 0 the class no template is eligible for (cls and sel may be NULL) — and row_of [n_c] the
 * distinct rows the class's queries have there, each in [0, n_q).  out [n_q][G] is uploaded as the caller filled it, the kernel runs once, out is copied back:
 *   out[row_of[r]][t] = cls[r][i] where t == sel[i], 0xffffffff in every other column; rows row_of does not name come back as they went in.
 * Words, not numbers: every bit pattern passes through unchanged.  AFIS_EINVAL for a list that breaks the rules above; no gallery is needed. */
int afis_debug_expand_rows(afis_ctx* ctx, const float* cls /*[n_c][m]*/, int n_c, int64_t m, const int32_t* row_of /*[n_c]*/, const int32_t* sel /*[m] or NULL*/,
                           int n_q, int64_t G, float* out /*[n_q][G]*/);
/* The fold of afis_search_weighted (template_fold.hip: k_fold_templates) on planted data, so that its shapes and bit patterns are swept without a search:
 * parts [n_pseudo][G][4] stands for one batch's per-part scores, qd [n_q][4] holds per query of the batch (first pseudo-query, pseudo-queries n_pq, of which carry a
 * texture template n_at <= n_pq, status: != 0 = the query has no active template), w [n_pseudo][4] the weights aligned to the part slots (0 = the slot is not summed),
 * empty [G] 1 = the rolled entry is empty.  The kernel runs once over out [n_q][G] and out is copied back:
 *   out[q][g] = -1 where status != 0 or empty[g]; otherwise (float) of the double sum, from +0.0, of (double)w * (double)part over slots 0..2 of pseudo-queries
 *   first .. first + n_pq - 1 in order, then over slot 3 of first .. first + n_at - 1; a slot of weight +-0 is skipped whatever its part holds.
 * AFIS_EINVAL for a query whose pseudo-queries leave [0, n_pseudo); no gallery is needed. */
int afis_debug_fold_templates(afis_ctx* ctx, const float* parts /*[n_pseudo][G][4]*/, int64_t n_pseudo, int64_t G, const int32_t* qd /*[n_q][4]*/, int n_q,
                              const float* w /*[n_pseudo][4]*/, const uint8_t* empty /*[G]*/, float* out /*[n_q][G]*/);
/* The query groups of afis_search_prints (print_queries.hip) without a search: ONE launch group is built from the resident prints idx [n] (global indices, any order,
 * repeats allowed) — print i with its minutiae template where use_minu[i] != 0 and its texture template where use_tex[i] != 0, where it has one — exactly as that call
 * builds a batch's groups: the tables on the host, the arrays by the gather on the device, over buffers planted with 0xA5 bytes.  counts [4] = (minutiae, fragment
 * tiles, texture rows of the group, lt_pad).  With lm_off == NULL only counts is filled (the caller sizes its arrays and calls again); otherwise the tables —
 * lm_off, lm_tile_off [3 n + 1], lt_off, tile_off, tile16_off [n + 1], tex_slot, status [n] — and the arrays — lm_xy [counts[0]][2], lm_ori [counts[0]], lm_des
 * [counts[0]][96], lm_frag [counts[1]][6][64][4], lt_xy [counts[2]][2], lt_ori [counts[2]], lt_des [counts[2]][96] — are copied back as the device holds them.
 * AFIS_EINVAL for an index outside the resident shard, AFIS_ESTATE before the first commit. */
int afis_debug_print_queries(afis_ctx* ctx, const int64_t* idx /*[n]*/, int n, const uint8_t* use_minu /*[n]*/, const uint8_t* use_tex /*[n]*/, int32_t* counts /*[4]*/,
                             int32_t* lm_off, int32_t* lm_tile_off, int32_t* lt_off, int32_t* tile_off, int32_t* tile16_off, int32_t* tex_slot, int32_t* status,
                             int16_t* lm_xy, float* lm_ori, float* lm_des, float* lm_frag, int16_t* lt_xy, float* lt_ori, float* lt_des);

/* The two mapped kernels of a two-stage search over a sub-shard (the mapped gather and scatter of the kept cells: csrc, the .hip unit whose name ends in _mapped) on
 * planted tables, without a search.  The call stands for n_q queries over a sub-shard of m templates of a resident shard of G_res:
 * kept [n_q][keep] are the kept lists as the selection leaves them (global indices, -1 padding), has [n_q] 1 = the query's kept cells are pairs, q_first [n_grp + 1]
 * the launch groups' first queries (ascending, 0 .. n_q) and per_launch the chunk size — from these the pair tables' structure is built as the driver builds it
 * (the driver's tables header) —, sel [m] the resident positions of the sub-shard's templates, strictly ascending (NULL with m == G_res: the identity), parts [n_q][m][4] the
 * per-part scores of stage 1, pair_score [pairs] what the pair kernels would have left (pairs = n_kept x the queries with has), row_of [n_q] / out_col [m] the rows and
 * columns of out [out_rows][out_stride] (NULL: q and the sub-shard position).  tab (tab_ints >= 2 pairs + pieces ints), pair_parts [pairs][4] and out are uploaded as the
 * caller filled them, each kernel runs once, and the three come back; *n_pieces = the pieces of the structure:
 *   piece i's table at tab + 2 piece_first[i] + i = [count | (q - first query of the piece's group, sub-shard position) x count]; pair_parts[slot] = (parts[q][t][0..2], +0.0f);
 *   out[row_of[q]][out_col[t]] = pair_score[slot], or -1.0f for a query without pairs, for every kept (q, t) that names a template of the sub-shard.
 * A kept entry that names none (padding, outside the shard, not in sel) is routed to template 0 with parts of +0.0f and written nowhere.  Words, not numbers.
 * 1 <= n_kept <= min(keep, m).  AFIS_EINVAL for tables that break the rules above; no gallery is needed. */
int afis_debug_kept_cells_mapped(afis_ctx* ctx, int n_q, int64_t G_res, int64_t m, int keep, int n_kept, int64_t index_base, const int64_t* kept /*[n_q][keep]*/,
                              const uint8_t* has /*[n_q]*/, const int32_t* q_first /*[n_grp + 1]*/, int n_grp, int per_launch, const int32_t* sel /*[m] or NULL*/,
                              const float* parts /*[n_q][m][4]*/, const float* pair_score /*[pairs]*/, const int32_t* row_of /*[n_q] or NULL*/,
                              const int32_t* out_col /*[m] or NULL*/, int64_t out_rows, int64_t out_stride, int32_t* tab, int64_t tab_ints, int32_t* n_pieces,
                              float* pair_parts /*[pairs][4]*/, float* out /*[out_rows][out_stride]*/);

/* In-kernel phase timers (only when the library is built with PHASE_TIMING=1; all zeros otherwise): 32 cycle counters
 * accumulated since the last reset.  Development aid. */
int afis_debug_phase_cycles(afis_ctx* ctx, unsigned long long* out32, int reset);

#ifdef __cplusplus
}
#endif
#endif /* AFIS_MATCHER_TAPS_H */
