/* afis_matcher.h — C ABI of the MI355X-native latent-vs-gallery matcher (libafis_hip.so).
 *
 * This is the drop-in boundary for the hot path of prip-lab/MSU-LatentAFIS `matching/`: the body of the
 * reference's OpenMP gallery loop (matching/matcher.cpp:168-190 == :273-295), i.e. everything reached from
 * PQ::Matcher::One2One_matching_selected_templates (matcher.h:43) for every (latent, rolled) pair, plus the
 * score fusion at matcher.cpp:188/:293.  The reference has no plugin/FFI interface of its own; a maintainer
 * replaces the loop body with one afis_search() call (see INTEGRATION.md for the exact patch).
 *
 * Conventions: plain C types only, no exceptions cross the boundary, every function returns 0 on success or a
 * negative AFIS_E* code (afis_last_error() gives the text).  A context is bound to ONE HIP device and is used
 * by one host thread at a time (PQ::Matcher is not re-entrant either).  All pointers are HOST pointers; the
 * library copies what it needs, the caller keeps ownership.  There is no CPU fallback: without a usable
 * gfx950 device afis_create() fails.
 */
#ifndef AFIS_MATCHER_H
#define AFIS_MATCHER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFIS_OK            0
#define AFIS_EINVAL       -1   /* bad argument / unsupported shape                     */
#define AFIS_EDEVICE      -2   /* HIP error, no device, out of device memory            */
#define AFIS_ESTATE       -3   /* call order (search before commit, add after commit)   */
#define AFIS_EFORMAT      -4   /* malformed template / codebook bytes                   */

/* Per-query status, mirrors One2One_matching_selected_templates' return (matcher.cpp:383-391). */
#define AFIS_QUERY_OK            0
#define AFIS_QUERY_LATENT_EMPTY  1   /* whole query skipped, its scores are left at -1 (matcher.cpp:191-194) */

typedef struct afis_ctx afis_ctx;   /* opaque; owns all device memory */

/* One minutiae template (reference: MinutiaeTemplate, matching/include.h:203-252).  x,y in pixels. */
typedef struct afis_minutiae_view {
    int32_t        n;        /* number of minutiae (> 0; n <= 0 templates are dropped, matcher.cpp:835-836) */
    const int16_t* x;        /* [n] */
    const int16_t* y;        /* [n] */
    const float*   ori;      /* [n] radians */
    int32_t        des_len;  /* descriptor length, must be 96 on this path */
    const float*   des;      /* [n][des_len] row-major fp32 */
} afis_minutiae_view;

/* One texture (virtual-minutiae) template.  x,y in BLOCK units ((px-24)/16).
 * Latent (LatentTextureTemplate, include.h:298-364): des = fp32 [n][96], codes = NULL.
 * Rolled (RolledTextureTemplatePQ, include.h:366-485): codes = u8 [n][16] PQ codes, des = NULL. */
typedef struct afis_texture_view {
    int32_t        n;
    const int16_t* x;
    const int16_t* y;
    const float*   ori;
    int32_t        des_len;  /* 96 (latent) or 16 (rolled) */
    const float*   des;
    const uint8_t* codes;
} afis_texture_view;

/* A whole fingerprint template (LatentFPTemplate / RolledFPTemplate, include.h:519-558), already stripped of
 * zero-minutiae templates exactly as Matcher::load_FP_template does (indices are post-strip indices). */
typedef struct afis_template_view {
    int32_t                   n_minu;
    const afis_minutiae_view* minu;
    int32_t                   n_tex;
    const afis_texture_view*  tex;
} afis_template_view;

/* Per-stage device time of the last afis_search call, milliseconds, from HIP events on the context's stream. */
typedef struct afis_timing {
    float   lut_ms;        /* S4  per-query LUT build                                  */
    float   adc_ms;        /* S5+S6 texture ADC similarity + row arg-max (dominant)     */
    float   tex_tail_ms;   /* S7+S8b+S9 on the texture correspondences                  */
    float   minu_ms;       /* S1-S3+S8a+S9 for the three selected minutiae templates    */
    float   fuse_ms;       /* S10 fusion                                                */
    float   topk_ms;       /* S11 per-query rank lists on the device (k <= 64)           */
    float   total_ms;      /* sum of the stages above                                   */
    int32_t adc_launches;  /* number of ADC kernel launches in the call                 */
    int64_t adc_lookups;   /* LUT look-ups performed by those launches                  */
    int64_t pairs;         /* (query, gallery template) pairs scored                    */
    float   adc_bound_ms;  /* part of adc_ms: the bound pass over every cell (adc_variant 8: the whole kernel; 9: k_adc_mfma) */
    float   adc_refine_ms; /* part of adc_ms: adc_variant 9's selection + exact recomputation kernel; 0 otherwise             */
    float   cands_ms;      /* part of minu_ms: S1-S3 (descriptor GEMM, normalisation, top-120 candidates)                      */
    float   minu_graph_ms; /* part of minu_ms: S8a + S9 on the minutiae correspondence lists                                   */
    int32_t launch_groups; /* launch groups the queries were cut into                                                          */
    int32_t overlapped_groups; /* of those: groups that ran the overlapped schedule (option bound_cus); the others ran their kernels back to back */
    /* round 5 (afis_get_timing2 with the caller's struct size): where the minutiae candidate tasks went, and the clocks the device held */
    int64_t minu_tasks;          /* (latent minutiae list, rolled template) candidate tasks of the call with minutiae on both sides   */
    int64_t minu_fallback_tasks; /* of those: tasks the shape-class kernels handed to the any-shape kernel (k_minu_cands)             */
    int64_t minu_tasks_small;    /* tasks done by the small  shape class of the fast kernel (k_minu_cands_rt<1>: 256 threads, <= 64 x 128) */
    int64_t minu_tasks_medium;   /* ... by the medium class (k_minu_cands_rt<2>: 512 threads, <= 16 384 similarities)                     */
    int64_t minu_tasks_large;    /* ... by the large  class (k_minu_cands_rt<4>: 1024 threads, <= 38 912 similarities incl. the stride padding, <= 256 latent x 512 rolled) */
    float   bound_clock_ghz;     /* shader clock under the bound pass: s_memtime ticks / s_memrealtime (100 MHz) over workgroup lifetimes, mean of the sampled workgroups; 0 = not sampled */
    float   cands_clock_ghz;     /* the same under the candidate kernel (a kernel that is not power-limited, for comparison)          */
} afis_timing;

/* Replaces PQ::Matcher::Matcher(code_file) (matcher.cpp:31-94).  codewords = [M][K][dsub] fp32 exactly as stored
 * in the codebook .dat after its 3 x int16 header.  Only M=16, K=256, dsub=6 is supported. */
int afis_create(afis_ctx** out, const float* codewords, int M, int K, int dsub, int device_id);
/* Same, from the bytes of a codebook .dat file (3 x int16 header + floats). */
int afis_create_from_codebook(afis_ctx** out, const void* codebook_bytes, size_t len, int device_id);
void afis_destroy(afis_ctx* ctx);
const char* afis_last_error(const afis_ctx* ctx);   /* ctx may be NULL: last afis_create failure */

/* Identity of HIP device `device_id` as the runtime reports it: marketing name + architecture, PCI bus id ("0000:c1:00.0", hipDeviceGetPCIBusId), UUID as 32 hex digits
 * (hipDeviceGetUuid), compute units.  Any output may be NULL.  One process per GPU: a multi-GPU job reports these per rank so that it can be told
 * from ranks sharing one device. */
int afis_device_info(int device_id, char* name, size_t name_cap, char* pci_bus_id, size_t pci_cap, char* uuid_hex /* >= 33 bytes */, size_t uuid_cap, int* n_cus);

/* Gallery build: replaces the per-pair load_FP_template(rolled) at matcher.cpp:173/:278 — parse once, keep the
 * gallery resident in HBM.  Only minutiae template 0 and texture template 0 of a rolled template are ever used
 * by the reference (matcher.cpp:406,:413).  Templates keep insertion order; index = position. */
int afis_gallery_add(afis_ctx* ctx, const afis_template_view* templates, int n);
/* Parse one rolled .dat (layout of Matcher::load_FP_template(string, RolledFPTemplate&), matcher.cpp:886-983).
 * *load_rc receives the reference's return code (0 ok, 1 empty file, 2, 4, -1); an entry is ALWAYS appended so
 * indices stay aligned with the caller's file list (empty entry => score -1, matcher.cpp:184-187). */
int afis_gallery_add_dat(afis_ctx* ctx, const void* bytes, size_t len, int* load_rc);
/* n rolled .dat files in one call: parsed on the host's threads, appended in order; load_rc (optional) receives n reader codes.
 * Nothing is appended when any file is rejected (AFIS_EINVAL, as afis_gallery_add_dat). */
int afis_gallery_add_dat_batch(afis_ctx* ctx, const void* const* bytes, const size_t* lens, int64_t n, int* load_rc);
/* Hint: the staged gallery will grow to about n_templates templates.  The host arrays reserve address space for them pro rata (from what is
 * staged so far; 80 minutiae and 800 texture points per template if nothing is), so that a gallery added in many slices is not re-copied every
 * time an array outgrows its allocation (a 100 000-file directory: 5 GB staged, 6 GB of re-copying without the hint).  Never required. */
int afis_gallery_reserve(afis_ctx* ctx, int64_t n_templates);
/* Bulk add of n templates with exactly one minutiae and one texture template each, as concatenated arrays with
 * CSR offsets (off[n+1], in points).  A zero-length range means "template absent". */
int afis_gallery_add_packed(afis_ctx* ctx, int64_t n,
                            const int64_t* minu_off, const int16_t* minu_x, const int16_t* minu_y,
                            const float* minu_ori, const float* minu_des /* [sum][96] */,
                            const int64_t* tex_off, const int16_t* tex_x, const int16_t* tex_y,
                            const float* tex_ori, const uint8_t* tex_codes /* [sum][16] */);
/* SoA-pack and upload.  index_base is added to every index afis_search reports (gallery sharding: each rank
 * commits its contiguous shard with the shard's global offset). */
int afis_gallery_commit(afis_ctx* ctx, int64_t index_base);
int64_t afis_gallery_size(const afis_ctx* ctx);

/* Live gallery (no reference counterpart: the reference's gallery is whatever the directory holds at the moment of a search): enrol and remove rolled prints
 * after the commit, without staging and uploading the resident shard again.  Every edit first waits for all device work of the context.
 * afis_gallery_reopen  valid on a committed gallery only (AFIS_ESTATE otherwise): opens a new staging area beside the resident shard.  Until the next commit every
 *                     staging call above and afis_gallery_load append to it exactly as before the first commit; searches, afis_correspondences and
 *                     afis_match_all_templates stay allowed and see the resident shard only; afis_gallery_size reports resident + staged; afis_gallery_save
 *                     stays AFIS_ESTATE (afis_gallery_export writes a resident shard).
 * afis_gallery_commit  on a reopened gallery appends the staged templates: they take the indices index_base + G_old ... in staging order.  index_base must be the
 *                     shard's (AFIS_EINVAL otherwise, nothing changes).  Only the new points and the offset tables cross PCIe: the device arrays grow by
 *                     capacity with a device-to-device copy, and the derived layouts are made for the new templates only.  The shard size limits apply to the
 *                     sum.  A failed append leaves the resident shard searchable and the staged templates in place.
 * afis_gallery_remove  idx[0 .. n): global indices as afis_search reports them.  The listed entries become EMPTY entries — their points leave every device array
 *                     (one compaction pass per call, whatever n is), every other template keeps its index — exactly as if the gallery had been committed with
 *                     empty templates at those positions: score -1, rolled_status 2.  An entry that is empty already, or listed twice, is a no-op; an index
 *                     outside the shard is AFIS_EINVAL with nothing changed; templates staged but not yet committed are AFIS_ESTATE.  Should the device run
 *                     out of memory half-way (AFIS_EDEVICE), the resident shard is dropped and the context is back to "not committed".
 * afis_gallery_export  writes the resident shard as a packed container (below): byte for byte the file afis_gallery_save writes from a context staged with the
 *                     same entries.  names as for afis_gallery_save, one per resident template.
 * Query handles (afis_queries_upload) are cut into launch groups for the shard size of the moment: after an appending commit or a removal that changed the shard,
 * afis_search_resident refuses an older handle with AFIS_ESTATE; free it and upload the latents again.  afis_search uploads per call and is not affected; a handle of
 * afis_queries_upload_reserved (below) is cut for a stated shard size instead and survives the edits.
 * After every edit the results are, bit for bit, those of a context freshly committed with the final gallery. */
int afis_gallery_reopen(afis_ctx* ctx);
int afis_gallery_remove(afis_ctx* ctx, const int64_t* idx, int64_t n);
/* Replace enrolled prints in place.  Valid on a reopened gallery with templates staged through any route above (afis_gallery_add with codes or fp32 descriptors,
 * afis_gallery_add_dat, _add_dat_batch, _add_packed, afis_gallery_load with or without a first / count slice): staged template i takes the place of resident entry
 * idx[i] (global indices, in staging order, in any order).  Nothing is appended: the shard keeps its size and every other template its index.  The final gallery is the old
 * one with entry idx[i] = staged template i, and the sentence above holds for it: results bit for bit those of a fresh commit of that gallery, afis_gallery_export byte for
 * byte the file afis_gallery_save writes of it.
 *   - a staged EMPTY template (no minutiae, no texture) makes the entry an empty entry, as afis_gallery_remove does; a live template onto an entry that is empty or was
 *     removed is re-enrolment at that index; minutiae-only and texture-only templates go in both directions; the staging routes clip and check as always.
 *   - AFIS_EINVAL, nothing changed (shard searchable, staged templates still staged, afis_gallery_size as before): idx NULL with n > 0; n not the number of staged
 *     templates; an index outside [index_base, index_base + G); an index listed twice; point sums beyond a shard's limits (2^31 - 1 minutiae or texture points, the bound
 *     pass's code stream).  AFIS_ESTATE, nothing changed: gallery not committed; not reopened; nothing staged.  After either a correct call succeeds, and a plain
 *     afis_gallery_commit(index_base) still appends what is staged.
 *   - on success it is an edit like the other two: it waits for the context's device work (the last search's matrix is gone), plain query handles, subsets, labels and
 *     subjects made before it are refused afterwards (handles of afis_queries_upload_reserved are taken), the code layouts built on first use are built again, the staging
 *     area is released and the gallery is no longer reopened.
 *   - only the staged points, the offset tables (five of G + 1 words, two source tables of G words) and the empty flags cross PCIe (option gallery_h2d_bytes counts
 *     them).  On the device every SoA array is written once into a buffer of its new size by one splice kernel (csrc/gallery_edit.hip: resident ranges from the old array,
 *     replaced ones from the staged points), swapped in and the old one released, the descriptors first: the transient memory is one array plus the staged points.  The
 *     derived layouts are then laid out whole in buffers of their new sizes.
 *   - device memory failure (AFIS_EDEVICE): before the first array has been switched the old shard is intact and the staged templates stay staged; after that the
 *     resident shard is dropped and the context is back to "not committed" with nothing staged, as after a removal that failed half-way.
 * Measured (profiles/gallery_replace_timing.json; MI355X, 10 000 resident templates, 500 replaced, medians of five): the transaction reopen + stage + afis_gallery_commit_at 20.9 ms
 * (20.7 - 21.7) against 31.6 ms (22.8 - 39.3) for afis_gallery_remove of the same 500 entries + reopen + stage + appending commit of the same 500 templates, interleaved in
 * one process, host wall-clock with the device idle at return; the six splice launches write 505.5 MB in 347 us of device time (HIP events around each), the removal's
 * compaction 480.5 MB in 327 us. */
int afis_gallery_commit_at(afis_ctx* ctx, const int64_t* idx /* [n], global */, int64_t n);
int afis_gallery_export(afis_ctx* ctx, const char* path, const char* const* names);

/* The hot path.  Replaces the body of the OpenMP loop of One2List_matching / List2List_matching
 * (matcher.cpp:168-190, :273-295) for n_q latents at once.
 *   scores      [n_q][G] or NULL : final fused score per gallery template, -1 where the rolled template is empty
 *                                  (or for every entry of a latent-empty query)
 *   parts       [n_q][G][4] or NULL : s0, s1, s2 (latent minutiae templates 26, 2, 11) and the texture score
 *   status      [n_q] or NULL    : AFIS_QUERY_*
 *   k, topk_idx [n_q][k], topk_score [n_q][k] : rank list, sorted on the key rank_key(score) = the bits of score + 0.0f in their total order (csrc/rank_order.h; the
 *                                  device's list for k <= 64 and the host's beyond sort on it alike), descending, equal keys by ascending global index: on the scores
 *                                  a search produces plainly score descending, ties by ascending index; a NaN stands where its bits put it, above +inf with the
 *                                  sign clear and below -inf with it set, and moves no other entry
 *                                  (the reference's tie order is unspecified, matcher.cpp:306-309 — a caller that wants the
 *                                  binary's order of EQUAL scores passes the score column to afis_rank_list(..., ref_order 1), as match -l -tie does); padded with
 *                                  idx -1 when k > G.  k = 0 skips it. */
int afis_search(afis_ctx* ctx, const afis_template_view* queries, int n_q,
                float* scores, float* parts, int32_t* status,
                int k, int64_t* topk_idx, float* topk_score);
/* Same with the queries given as latent .dat bytes (Matcher::load_FP_template(string, LatentFPTemplate&),
 * matcher.cpp:785-884). */
int afis_search_dat(afis_ctx* ctx, const void* const* latent_bytes, const size_t* lens, int n_q,
                    float* scores, float* parts, int32_t* status,
                    int k, int64_t* topk_idx, float* topk_score);

/* Queries resident in HBM before the timed region (bench): upload once, search many times.
 * afis_search_resident (and afis_search on top of it) runs the query groups back to back on the context's stream and syncs once.
 * For k <= 64 the rank lists are made on the device (per-query top-k kernel over the shard's scores, score descending / index
 * ascending) and only n_q x k x 12 bytes return to the host; the [n_q][G] score matrix crosses PCIe only when `scores` is given
 * (-ldir mode) and the per-part scores only when `parts` is.  k > 64 sorts on the host. */
typedef struct afis_queries afis_queries;
int afis_queries_upload(afis_ctx* ctx, const afis_template_view* queries, int n_q, afis_queries** out);
/* A query handle that survives gallery edits (reverse search, below): as afis_queries_upload, except that the launch groups are cut as that function would cut them at a
 * shard of max_templates templates — the memory budget, the latents per launch (option "query_batch", or the automatic figure for that size) and the row-group cuts —
 * whatever the resident shard holds at the time, which may be more.  The handle records max_templates and is accepted whatever edits have happened since it was
 * uploaded: by afis_search_resident while the resident shard holds at most max_templates templates, by afis_search_subset_resident for a live, current subset of at most
 * max_templates templates; a larger shard or subset is AFIS_EINVAL with both numbers in the message.  max_templates < 1 is AFIS_EINVAL, a call before the first commit
 * AFIS_ESTATE.  Device memory behaves as with subsets: later enrolments take memory the cuts did not know of, and a search that cannot get its buffers returns
 * AFIS_EDEVICE before it has queued anything.  A handle is not edited in place: a latent file that grows is kept as several handles (afis_rank_latent_hits' latent_base). */
int afis_queries_upload_reserved(afis_ctx* ctx, const afis_template_view* queries, int n_q, int64_t max_templates, afis_queries** out);
int afis_search_resident(afis_ctx* ctx, afis_queries* q,
                         float* scores, float* parts, int32_t* status,
                         int k, int64_t* topk_idx, float* topk_score);
void afis_queries_free(afis_ctx* ctx, afis_queries* q);

/* Subset search (no reference counterpart: the reference scores whatever the directory holds): score a candidate list of the resident shard — a filter of the caller's
 * database, the survivors of a cheaper first stage, re-enrolled templates — without searching the whole shard and without staging the candidates from the host again.
 * afis_subset_create   idx[0 .. n): global indices as afis_search reports them (index_base included), in any order; n == 0 is a valid, empty subset.  The listed
 *                     templates' points are gathered on the device into a sub-shard of the subset's own: every SoA array, the derived layouts of the default path
 *                     and an empty flag per entry (the streams of adc_variant 8 are laid out on the subset's first use of it, as they are for the shard).  Nothing of
 *                     the gallery crosses PCIe: only the index list and the offset tables do.  An index outside the resident shard or listed twice is AFIS_EINVAL, an
 *                     index of a template that is staged but not committed AFIS_ESTATE (as afis_gallery_remove), a call before the first commit AFIS_ESTATE; a refused
 *                     call leaves nothing allocated and nothing changed.  Create and free first wait for all device work of the context, as every gallery edit does.
 *                     Several subsets may be live at once; afis_destroy releases those that are left.  Their device memory is what option "subset_device_bytes"
 *                     reports: launch groups cut afterwards (afis_queries_upload) are cut to the memory the subsets leave free.
 * afis_search_subset / afis_search_subset_resident   as afis_search / afis_search_resident over the listed templates only: scores [n_q][n] and parts [n_q][n][4] with
 *                     column j belonging to idx[j] in the caller's order (a listed entry that is empty scores -1), status as afis_search gives it, topk_idx GLOBAL
 *                     indices, score descending, equal scores by ascending global index whatever order the list had; k > n pads as afis_search pads k > G; k <= 64 on
 *                     the device, larger k on the host.  afis_timing counts the subset's work (pairs == n_q * n).  Every value is bit for bit the value afis_search
 *                     gives for that (query, template) pair, under every option.
 * A subset belongs to the gallery as it was when the subset was made: after an appending commit or a removal that changed the shard both search calls refuse it with
 * AFIS_ESTATE (afis_subset_free still works).  A query handle stays valid for any subset of the shard it was uploaded for.  Full searches, afis_correspondences and
 * afis_match_all_templates neither see a subset nor change when one exists. */
typedef struct afis_subset afis_subset;
int afis_subset_create(afis_ctx* ctx, const int64_t* idx, int64_t n, afis_subset** out);
void afis_subset_free(afis_ctx* ctx, afis_subset* s);
int afis_search_subset(afis_ctx* ctx, afis_subset* s, const afis_template_view* queries, int n_q,
                       float* scores, float* parts, int32_t* status,
                       int k, int64_t* topk_idx, float* topk_score);
int afis_search_subset_resident(afis_ctx* ctx, afis_subset* s, afis_queries* q,
                                float* scores, float* parts, int32_t* status,
                                int k, int64_t* topk_idx, float* topk_score);

/* Subject rank lists (no reference counterpart: the reference ranks the files of a directory): a resident gallery holds prints, an examiner is handed persons — a ten-print
 * card is ten templates, a re-enrolment adds more.  The score matrix a search leaves on the device is grouped by enrolled person there, and only n_q x k x 20 bytes return.
 * afis_subjects_create  subject[0 .. n): the caller's id of the person resident template index_base + i belongs to — any int64 >= 0, in any order, not necessarily dense.  n must
 *                     be the resident shard's size (option "gallery_resident"; AFIS_EINVAL otherwise, as for a negative id); a call before the first commit is AFIS_ESTATE; a
 *                     refused call leaves nothing allocated.  The distinct ids in ascending order become the slots of the rank lists; the slot of every template (int32) and
 *                     the id table are uploaded, and counted in option "gallery_h2d_bytes" as a subset's tables are.  Create and free first wait for all device work of the
 *                     context.  Several handles may be live at once; afis_destroy releases those that are left.  A handle belongs to the gallery as it was: after an
 *                     appending commit or a removal that changed the shard afis_rank_subjects refuses it with AFIS_ESTATE (afis_subjects_free still works).
 * afis_rank_subjects   ranks the score matrix of the context's LAST search — any of afis_search, afis_search_dat, afis_search_resident, afis_search_subset,
 *                     afis_search_subset_resident, afis_search_eligible, afis_search_weighted, afis_search_prints, afis_search_cascade, afis_search_cascade_subset, afis_search_cascade_eligible, afis_search_prints_cascade, whatever outputs that call was asked for — as afis_get_timing reports the last search's times.  n_q must be that
 *                     search's (AFIS_EINVAL otherwise, as for k <= 0 or a null output).  Per query the k best subjects:
 *                       subject_score  the greatest fused score among the subject's templates that the search covered: all of them for a full search, the listed ones for a
 *                                      subset search (a subject without a listed template does not appear).  An empty or removed entry contributes its -1: a subject all of
 *                                      whose templates are empty scores -1, and a latent-empty query lists the subjects by ascending id, all at -1.
 *                       subject_id     score descending, equal scores by ascending subject id whatever order the templates or a subset's list had
 *                       best_idx       the global index (index_base included) of the subject's best template, the lowest such index among equal scores
 *                     padded with id -1, score -inf, best_idx -1 where k exceeds the subjects present.  "Greatest" and "descending" are taken on the score's bits in their
 *                     total order (sign-magnitude: -0.0 below +0.0, a NaN where its bits put it); on the scores a search produces that is the order of the template rank
 *                     lists, so that with subject[i] = c + i the result is entry for entry the rank list of afis_search: ids c + position, the same scores, the same
 *                     indices.  k <= 64 is made on the device; larger k copies the [n_q][subjects] maxima to the host and sorts there, on the same keys.  The device
 *                     keeps n_q x subjects x 8 bytes for the maxima (80 MB at 100 x 100 000), allocated on first use: AFIS_EDEVICE, with nothing changed, when that fails.
 *                     The matrix stays rankable from the successful return of the search until the next call on the context that queues device work or edits the gallery —
 *                     a search (a failed or timed-out one included), afis_queries_upload, afis_correspondences, afis_match_all_templates, every gallery
 *                     edit and export, afis_subset_create, afis_subset_free, a change of option "bound_cus" — after which afis_rank_subjects is AFIS_ESTATE.  It may itself
 *                     be repeated, with another k or another handle; afis_correspondences_pairs, afis_score_pairs, afis_score_print_pairs, afis_correspondences_print_pairs, afis_subjects_create, afis_subjects_free, afis_queries_free, afis_get_timing*, afis_get_option,
 *                     afis_last_error and afis_gallery_size leave the matrix alone.  No result of a search changes because subjects exist.
 * Shards: every rank labels its own shard and ranks its own subjects; the per-rank lists merge exactly although a person's prints may lie in several shards
 * (host/sharding.py::merge_subject_topk). */
typedef struct afis_subjects afis_subjects;
int afis_subjects_create(afis_ctx* ctx, const int64_t* subject /*[n]*/, int64_t n, afis_subjects** out);
void afis_subjects_free(afis_ctx* ctx, afis_subjects* s);
int afis_rank_subjects(afis_ctx* ctx, afis_subjects* s, int n_q, int k,
                       int64_t* subject_id /*[n_q][k]*/, float* subject_score /*[n_q][k]*/, int64_t* best_idx /*[n_q][k]*/);

/* Hit lists (no reference counterpart): "who is above the decision score?" — lights-out identification, watch-list alarms and deduplication want every template, or every
 * person, whose score reaches a threshold, and how many there are; an ELFT-style candidate list wants 100 entries, more than the rank lists make on the device.  Both are
 * answered on the device from the score matrix of the context's LAST search, in one workgroup per query that passes over its row five times at most (rank_hits.hip): only
 * n_q x (8 + cap x 12) bytes (templates) or n_q x (8 + cap x 20) bytes (subjects) return, through the context's pinned buffer.
 * afis_rank_hits          the templates: idx / score as afis_search's topk_idx / topk_score (global indices; for a subset search the listed templates only).
 * afis_rank_subject_hits  the enrolled persons of a subject handle: subject_id / subject_score / best_idx as afis_rank_subjects'.
 * A hit list is the longest prefix of the corresponding rank list — afis_search's for templates, afis_rank_subjects' for subjects — whose entries reach min_score:
 *   n_hits[q]     how many entries qualify; it may exceed cap, which is how a caller sees that the list was cut
 *   the lists     the first min(n_hits[q], cap) entries of the rank list; the rest is padded as the rank lists are: idx / subject_id / best_idx -1, score -inf
 * "Reach" is decided on the ordered key the rank list itself is sorted by, so that the qualifying entries are a prefix of it whatever bit patterns the matrix holds:
 * for templates the bits of score + 0.0f in their total order (min_score gets the same + 0.0f, so the two zeros are one value; equal scores by ascending global index,
 * also for a subset listed out of order), for subjects the raw bits of the subject's best score in their total order (-0.0 below +0.0; equal scores by ascending subject
 * id; a subject none of whose templates the search covered is no entry and is not counted).  A NaN orders where its bits put it: above +inf with the sign clear, below
 * -inf — and so below every min_score — with it set; afis_search's lists of every k, afis_rank_list and the merges of the per-rank lists sort on the same key.  On the scores a search produces, -1 or a finite value >= +0.0, both rules are plainly score >= min_score.
 * min_score = -INFINITY turns the call into a rank list of length cap: entry for entry afis_search's top-k, or afis_rank_subjects' list (short of NaNs with the sign
 * set, which stand at the tail of those lists and, lying below -inf, are padding here).
 * Which searches count, what invalidates the matrix and what leaves it alone are exactly as for afis_rank_subjects: AFIS_ESTATE when there is no matrix to rank or the
 * subject handle belongs to an older gallery; AFIS_EINVAL when n_q is not the last search's, the handle is not live, an output is null, cap is outside
 * 1 .. AFIS_HITS_MAX (the list is sorted in the workgroup's local memory) or min_score is a NaN.  Both calls leave the matrix rankable: they may be repeated with other
 * arguments, and afis_rank_subjects may follow; a wait that times out invalidates it.  With an empty shard, or a handle without subjects, every n_hits is 0 and every
 * entry padding; n_q == 0 returns AFIS_OK.  Device and pinned room (n_q x subjects x 8 bytes for the subjects' maxima, as afis_rank_subjects) is ensured before anything
 * is queued: AFIS_EDEVICE, with nothing changed, when that fails.  No result of a search changes because these functions exist.
 * Shards: host/sharding.py::merge_hits and merge_subject_hits merge the per-rank lists and counts. */
#define AFIS_HITS_MAX 4096
int afis_rank_hits(afis_ctx* ctx, int n_q, float min_score, int cap,
                   int64_t* n_hits /*[n_q]*/, int64_t* idx /*[n_q][cap]*/, float* score /*[n_q][cap]*/);
int afis_rank_subject_hits(afis_ctx* ctx, afis_subjects* s, int n_q, float min_score, int cap,
                           int64_t* n_hits /*[n_q]*/, int64_t* subject_id /*[n_q][cap]*/, float* subject_score /*[n_q][cap]*/, int64_t* best_idx /*[n_q][cap]*/);

/* Rank positions (no reference counterpart): the lists above answer "who is at the top?"; these calls answer "where does THIS print, or this person, stand in that
 * query's list?" — the rank of the true mate of every latent (a CMC curve), a named suspect's prints among 100 000 under the latent's filters, the per-shard term of a
 * mate's global rank — for EVERY position, not only the first AFIS_HITS_MAX, without the [n_q][G] matrix leaving the device.  All three read the score matrix of the
 * context's LAST search: one small pass reads the targets' cells, one counting pass reads each row that has
 * targets once (rank_position.hip); about 24 bytes per target return, through the context's pinned buffer.  The matrix is neither written nor invalidated.
 * Targets: n_targets pairs (query[i], idx[i] or subject_id[i]) — query[i] a query position of the last search, idx GLOBAL template indices — in any order, repeated or
 * not; a query may have no target.  The outputs are per target, in the caller's order.
 * afis_rank_positions          For target (q, t), n_before is the position of t in the list afis_rank_hits_filtered(labels, masks, excl, ..., min_score = -INFINITY, cap)
 *                              gives query q — with no filters, the list afis_rank_hits gives: idx[q][n_before] == t for any cap > n_before, so that n_before is defined
 *                              for every position.  score is the cell's own bits.  The order is csrc/rank_order.h::rank_before: rank_key descending, equal keys by
 *                              ascending GLOBAL index, also for a subset listed out of order.  An ENTRY is a cell whose rank_key >= rank_key(-inf): a cell that holds
 *                              0xffffffff (a filter or an exclusion took it out, or afis_search_eligible left it unscored) or any other NaN with the sign set is no
 *                              entry, exactly as the hit lists treat it.
 *                                AFIS_POS_LISTED       the target is an entry: n_before and score as above
 *                                AFIS_POS_NO_ENTRY     the target is a column of the search but no entry: n_before -1, score -inf
 *                                AFIS_POS_NOT_COVERED  idx lies outside this shard, or is not in the subset's list: the same outputs.  Silent, not an error, so that the
 *                                                      same target list can go to every rank of a sharded gallery, as exclusion lists may
 * afis_rank_subject_positions  the same sentence against afis_rank_subject_hits(_filtered) at -INFINITY: the key is the raw ordered word of the person's best eligible
 *                              covered score, ties by ascending subject id, best_idx that call's best_idx.  A person on the query's excl_subject list, or with no
 *                              eligible covered template, is AFIS_POS_NO_ENTRY (best_idx -1); an id the handle does not hold is AFIS_POS_NOT_COVERED.
 * afis_count_before            the sharding primitive: n_before[i] is the number of ENTRIES of row query[i], under the same optional filters, that stand before a
 *                              hypothetical entry (score[i], idx[i]) by rank_before.  A column whose global index equals idx is never counted — it is the target itself —
 *                              and idx need not be covered.  On the owning rank afis_count_before(the cell's score, idx) equals afis_rank_positions' n_before; across
 *                              ranks with disjoint columns the global n_before is the sum of the per-rank counts (host/sharding.py::merge_positions).  A NaN score is
 *                              AFIS_EINVAL.
 * Everything else is afis_rank_hits_filtered's: which searches count and what invalidates the matrix, the AFIS_ESTATE and AFIS_EINVAL cases, the handles' life cycles,
 * the rules of masks and of the exclusions' CSR.  With neither masks nor exclusions the matrix itself is read; after afis_search_eligible the plain call gives what the
 * filtered call gives after a full search.  In addition AFIS_EINVAL: a query[i] outside 0 .. n_q - 1, a negative idx or subject_id, n_targets < 0, a null array with
 * n_targets > 0.  n_targets == 0 returns AFIS_OK; with an empty shard, or a handle without subjects, every target is AFIS_POS_NOT_COVERED and every count 0.  Device and
 * pinned room — the filtered copy, the tables, n_q x subjects x 8 bytes for the subjects' maxima, 24 bytes per target — is ensured before anything is queued:
 * AFIS_EDEVICE, with nothing changed, when that fails.  No result of a search changes because these functions exist.
 * These calls do not give: positions in case lists and in column (reverse) lists; person positions summed across shards — a person's prints may lie in two shards, and the
 * per-shard counts of persons do not add up (the caveat of host/sharding.py::merge_case_subject_hits). */
#define AFIS_POS_LISTED      0   /* the target is an entry of the list                                             */
#define AFIS_POS_NO_ENTRY    1   /* covered by the search, but no entry: ineligible, excluded, or a key below -inf's */
#define AFIS_POS_NOT_COVERED 2   /* not a column of the last search / not a person the handle and the search hold   */
typedef struct afis_labels afis_labels;
int afis_rank_positions(afis_ctx* ctx, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                        const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/,
                        int n_q, int64_t n_targets, const int32_t* query /*[n_targets]*/, const int64_t* idx /*[n_targets], GLOBAL*/,
                        int32_t* status /*[n_targets]*/, int64_t* n_before /*[n_targets]*/, float* score /*[n_targets]*/);
int afis_rank_subject_positions(afis_ctx* ctx, afis_subjects* s, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                                const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl_subject /*[excl_off[n_q]]*/,
                                int n_q, int64_t n_targets, const int32_t* query /*[n_targets]*/, const int64_t* subject_id /*[n_targets]*/,
                                int32_t* status /*[n_targets]*/, int64_t* n_before /*[n_targets]*/, float* score /*[n_targets]*/, int64_t* best_idx /*[n_targets]*/);
int afis_count_before(afis_ctx* ctx, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                      const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/,
                      int n_q, int64_t n_targets, const int32_t* query /*[n_targets]*/, const float* score /*[n_targets]*/, const int64_t* idx /*[n_targets], GLOBAL*/,
                      int64_t* n_before /*[n_targets]*/);

/* Cohort statistics and z-normalised scores (no reference counterpart): every list above is cut by one decision score, and a raw fused score grows with the minutiae a
 * latent carries and with a print that scores high against everything.  Cohort normalisation puts the matrix on a common scale: a latent's scores in units of that
 * latent's own non-mate distribution (per row, "T-norm", axis 0), or a print's scores in units of that print's distribution over many latents (per column, "Z-norm",
 * axis 1: what the reverse search needs) — on the device, without the [n_q][G] matrix leaving it.
 * Definitions (csrc/score_stats.h holds them once, for the kernels and the host; the tests hold the device to them bit for bit):
 *   cell classes   a cell (word w, float v) is NO ENTRY (w == 0xffffffff: a filter took it out, or afis_search_eligible left it unscored), VALUED (v finite, the sign
 *                  bit of v + 0.0f clear, v < 65536.0f) or OUTSIDE (everything else: -1 of an empty template or latent, negative values, +-inf, NaN, values >= 2^16)
 *   quantisation   q(v) = llrint((double)v * 1048576.0) under round-to-nearest-even, for a valued v: the product is exact in fp64 and 0 <= q < 2^36
 *   statistic      of a set of cells — a row's (axis 0) or a column's (axis 1) after the call's eligibility filter —: n the valued cells, n_outside the outside
 *                  cells, s1 = sum q, s2 = sum q^2 as a 128-bit unsigned integer (s2_lo, s2_hi), min / max the valued cells' least and greatest value by rank_key
 *                  (the two zeros are one value, +0.0); +inf / -inf while n == 0.  Exact integers: statistics of disjoint cell sets — the shards of a gallery —
 *                  add up to the statistic of their union bit for bit, whatever the order of the sums and wherever the shards were cut
 *   THE BOUND      n <= 2^27, for a shard and for a sum of shards.  Then s1 < 2^63, s2 < 2^99, and n x s2 and s1^2 stay below 2^126.  The add helper checks it
 *   moments        mean = double(s1) / (double(n) * 1048576.0); N = n x s2 - s1^2, exact in 128 bits; sd = sqrt(double(N)) / (double(n) * 1048576.0) — the
 *                  population deviation; double(.) is the correctly rounded conversion of the integer; n == 0 gives (0, 0)
 *   normalised     z = (float)(((double)v - offset) * scale): an fp64 subtraction, an fp64 multiplication (no fused multiply-add) and one conversion.  Every valued
 *                  cell becomes its z, every outside cell becomes no entry (a template without a print has no z-score), every no-entry cell stays
 * afis_score_stats        reads the LAST search's matrix, whatever left it (a full, subset, eligible, weighted, print or cascade search), through the filtered ranking
 *                         calls' own checks and filter pass (afis_rank_hits_filtered's rules for labels, masks and the exclusions' CSR at min_score = -inf): the
 *                         filter decides which cells are in the cohort — elimination prints and a known mate go into excl.  axis 0: out [n_q], one statistic per
 *                         query; axis 1: out [columns], one per column in the order of the search's scores output (for a subset the caller's column order).  The
 *                         matrix is neither written nor invalidated.  AFIS_EINVAL in addition: an axis other than 0 or 1, a null out, a row or column of more than
 *                         2^27 cells.  An empty shard or n_q == 0: every statistic is (0, 0, 0, 0, 0, +inf, -inf), no device work.  Device and pinned room — the
 *                         filtered copy, 72 bytes per row, 48 bytes per statistic — is ensured before anything is queued (AFIS_EDEVICE otherwise)
 * afis_normalize_scores   applies "normalised" to every cell of the UNFILTERED matrix with its row's (axis 0: offset, scale [n_q]) or column's (axis 1: [columns], in
 *                         the order above) pair: a mate is normalised against the cohort it was left out of.  offset must be finite and scale finite and > 0, else
 *                         AFIS_EINVAL before anything is queued, with the matrix unchanged and rankable.  After AFIS_OK the last-search matrix holds the z-scores:
 *                         every ranking call reads them and takes min_score in z units; scores_out, where given, receives the normalised matrix in the search's
 *                         column order.  The matrix is then marked normalised: both calls refuse it with AFIS_ESTATE, and the next search clears the mark.  n_q must
 *                         be the last search's.  Normalising along both axes of one matrix is not offered
 *                         (by this call alone: the kept matrices below keep the raw matrix, recall it for the other axis and fuse the two halves)
 * The three helpers are host arithmetic on statistics — no context, no device:
 * afis_score_stat_add     acc += other, field by field with carry, min of mins and max of maxes; AFIS_EINVAL, acc unchanged, where n would pass 2^27
 * afis_score_stat_remove  takes one valued cell's contribution out of acc exactly, so that trimming a cohort by its best k cells is integer arithmetic over the top-k a
 *                         search already returns, and works across shards.  AFIS_EINVAL, acc unchanged, for a score that is not valued or where a field would go
 *                         below zero.  min and max are LEFT AS THEY ARE: they stay the extremes of the cohort before the removal
 * afis_score_stat_moments "moments" above; AFIS_EINVAL for a statistic outside the bound or one that no set of cells has (n x s2 < s1^2)
 * Options "score_stats_us" and "normalize_us" (read-only): the device time of the last call's launches.  The sharded recipe — statistics per rank, merged on the
 * host, every rank normalised with the merged pair, then the usual rank exchange — is INTEGRATION.md's (host/sharding.py::merge_score_stats, trim_score_stats).
 * These calls do not give: an exchange of statistics between ranks inside the library (histograms and the entry at a rank: the score distributions below). */
typedef struct { int64_t n, n_outside; uint64_t s1, s2_lo, s2_hi; float min, max; } afis_score_stat;   /* 48 bytes */
int afis_score_stats(afis_ctx* ctx, int axis, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                     const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/, int n_q,
                     afis_score_stat* out /*axis 0: [n_q]; axis 1: [columns]*/);
int afis_normalize_scores(afis_ctx* ctx, int axis, int n_q, const double* offset, const double* scale /*[n_q] or [columns]*/,
                          float* scores_out /*[n_q][columns] or NULL*/);
int afis_score_stat_add(afis_score_stat* acc, const afis_score_stat* other);
int afis_score_stat_remove(afis_score_stat* acc, float score);
int afis_score_stat_moments(const afis_score_stat* st, double* mean, double* sd);

/* Score distributions (no reference counterpart): the lists say who is at the top, the positions where a named print stands, the statistics what mean and deviation
 * are; these two calls answer the opposite questions — how many entries lie between two scores, for many scores at once (the non-mate distribution behind a DET curve,
 * the threshold that gives a chosen false-positive rate or a candidate list of a chosen length), and WHICH entry stands at a given rank (the score at rank 5 000 of
 * 100 000: a median, a cohort trimmed by its best 1 %) — on the device, without the [n_q][G] matrix leaving it.  Both read the score matrix of the context's LAST
 * search through the filtered ranking calls' own checks and filter pass (afis_rank_hits_filtered's rules for labels, masks and the exclusions' CSR at min_score =
 * -inf), and both ACCEPT a normalised matrix: edges are then in z units, as min_score is for the hit lists, and negative z-scores are ordinary entries.  Integer
 * arithmetic only.  The matrix is neither written nor invalidated.
 * Definitions (csrc/score_hist.h holds them once, for the kernels and the host; the tests hold the device to them exactly):
 *   entry          a cell whose rank_key >= rank_key(-inf), exactly as the hit lists and the positions define it: a cell that holds 0xffffffff, or any other NaN with
 *                  the sign set, is counted nowhere and stands at no rank
 *   bin            an entry goes to bin b = the number of edges e with rank_key(e) <= rank_key(cell) (csrc/score_order.h).  Bin 0 holds the entries below edges[0] — the
 *                  -1 of empty templates and -inf among them —, bin n_edges those that reach the last edge — NaNs with the sign clear among them.  An edge is inclusive
 *                  from below, and the two zeros are one value, for cells and for edges
 *   THE PROPERTY   for every j, counts[r][j + 1] + ... + counts[r][n_edges] is the n_hits afis_rank_hits_filtered returns row r for min_score = edges[j] under the
 *                  same filters, and the sum of all bins its n_hits at -INFINITY.  Counts of disjoint cell sets — the shards of a gallery — add up bit for bit
 * afis_score_histogram  axis 0: counts [n_q][n_edges + 1], one histogram per query; axis 1: counts [columns][n_edges + 1], one per column in the order of the search's
 *                       scores output (for a subset the caller's column order).  AFIS_EINVAL, before anything is queued and with the matrix still rankable: an axis
 *                       other than 0 or 1, n_edges outside 1 .. AFIS_HIST_EDGES_MAX, an edge that is a NaN, edges that do not ascend strictly by rank_key, outputs x
 *                       (n_edges + 1) above AFIS_HIST_COUNTS_MAX, a null edges or counts where there is something to count.  An empty shard or n_q == 0: every count
 *                       0, no device work.  Device and pinned room — the filtered copy, axis 1's transposed copy, 8 bytes per count — is ensured before anything is
 *                       queued (AFIS_EDEVICE otherwise)
 * afis_entries_at       for target (q, r) — query[i] a query position of the last search, rank[i] >= 0, in any order, repeated or not; a query may have no target —
 *                       idx and score are entry r of the list afis_rank_hits_filtered(labels, masks, excl, ..., min_score = -INFINITY, cap) gives query q, for any cap >
 *                       r: defined for every r, not only the first AFIS_HITS_MAX.  The order is csrc/rank_order.h::rank_before: rank_key descending, equal keys by
 *                       ascending GLOBAL index, also for a subset listed out of order.  status AFIS_POS_LISTED: idx the GLOBAL index, score the cell's own bits (a cell
 *                       that holds -0.0 returns -0.0).  r at or beyond the row's number of entries: AFIS_POS_NO_ENTRY, idx -1, score -inf.  The round trip:
 *                       afis_rank_positions(q, idx) returns n_before == r.  AFIS_EINVAL in addition to afis_rank_positions' cases: a negative rank.  n_targets == 0
 *                       returns AFIS_OK; with an empty shard every target is AFIS_POS_NO_ENTRY.  Device room: 2 KB per target besides the filtered copy; 16 bytes per
 *                       target return.  On the device a radix select over the row's 64-bit composites (key, ~position), which are unique inside a row: no tie handling
 * Everything else is afis_score_stats' and afis_rank_positions': which searches count and what invalidates the matrix, the AFIS_ESTATE and AFIS_EINVAL cases, the
 * handles' life cycles, the rules of masks and of the exclusions' CSR.  No result of a search changes because these functions exist.
 * Options "score_histogram_us" and "entries_at_us" (read-only): the device time of the last call's launches.  Measured on one MI355X on a planted matrix of 100 latents
 * x 100 000 templates (tools/score_distribution_timing.py, profiles/score_distribution_timing.json; medians of five): afis_score_histogram along the rows 44 / 60 / 156
 * us at 16 / 256 / 1024 bins on cells uniform in [0, 300) with 5 % of -1, 37 / 54 / 95 us where every cell is 0.0 — one bin, the shape of real non-mate rows: the wave
 * aggregation works, the one-bin matrix is the faster of the two —, 207 us along the columns at 16 bins; afis_entries_at 203 us with one rank per row and 1224 us with
 * 64 (207 and 687 us on the one-bin matrix); afis_score_stats along the rows of the same matrix in the same process, which also reads every word once, 52 us.
 * Shards: histograms add (host/sharding.py::merge_score_histograms); ranks do not, so there is no global afis_entries_at — the sharded quantile recipe of INTEGRATION.md
 * brackets the rank with the merged histogram (histogram_rank_bin) and settles it with afis_count_before.
 * These calls do not give: ranks in case lists and in column (reverse) lists; bins of unequal weight (persons: the person distributions below). */
#define AFIS_HIST_EDGES_MAX 1023          /* 1024 bins */
#define AFIS_HIST_COUNTS_MAX (1 << 24)    /* counts one call returns: outputs x (n_edges + 1) */
int afis_score_histogram(afis_ctx* ctx, int axis, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                         const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/, int n_q,
                         int n_edges, const float* edges /*[n_edges]*/, int64_t* counts /*axis 0: [n_q][n_edges + 1]; axis 1: [columns][n_edges + 1]*/);
int afis_entries_at(afis_ctx* ctx, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                    const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/,
                    int n_q, int64_t n_targets, const int32_t* query /*[n_targets]*/, const int64_t* rank /*[n_targets], >= 0*/,
                    int32_t* status /*[n_targets]*/, int64_t* idx /*[n_targets], GLOBAL*/, float* score /*[n_targets]*/);

/* Person distributions (no reference counterpart): afis_score_stats, afis_score_histogram and afis_entries_at over enrolled PERSONS — the three calls that turn a
 * matrix into a decision score, for the lists an examiner is handed.  A person's score is the maximum over their templates: someone enrolled with two ten-print cards
 * puts 20 cells into a latent's cohort under afis_score_stats and a single flat print one, so the z-score that cuts afis_rank_subject_hits must come from the persons'
 * statistics; and "the score at which 1 latent in 100 raises a false person alarm" is a question about the distribution of persons' best scores.  All three read the
 * score matrix of the context's LAST search through afis_rank_subject_hits_filtered's own checks and pre-passes — the handle's, labels and masks on the TEMPLATES, excl
 * as SUBJECT ids, the filter pass, k_subject_best over the filtered rows, the excluded persons dropped: no second definition of eligibility, none of a person's best.
 * Definitions (csrc/score_cell.h, csrc/score_hist.h and csrc/score_stats.h hold them once, for the kernels and the host; the tests hold the device to them exactly):
 *   person cell    of (query q, person s): the best eligible covered cell of the person's templates by the RAW ordered word (csrc/score_order.h::ordered_word), ties to
 *                  the lowest position — not rank_key: -0.0 stands below +0.0, and a NaN with the sign clear stands above +inf and wins.  There is NO cell where the
 *                  search covered none of the person's templates (a subset search), the person is on q's excl list, or every template of theirs is ineligible or
 *                  itself holds 0xffffffff
 *   entry          a person cell whose ordered word >= ordered_word(-inf): what afis_rank_subject_hits counts at min_score = -INFINITY
 *   bin            an entry goes to bin b = the number of edges e with ordered_word(e) <= the cell's ordered word.  Edges must not be NaN and must ascend strictly BY
 *                  THAT KEY: (-0.0, +0.0) is a valid pair of edges here — three bins — although afis_score_histogram refuses it, and a person whose best is -0.0
 *                  falls below an edge at +0.0.  THE PROPERTY: for every j, counts[q][j + 1] + ... + counts[q][n_edges] is the n_hits
 *                  afis_rank_subject_hits_filtered returns query q at min_score = edges[j] under the same arguments; the sum of all bins its n_hits at -INFINITY
 *   statistic      afis_score_stats' definitions, unchanged, over the persons' score words: a person whose best is -1 (all their prints empty) is outside, a best of
 *                  -0.0 is valued with q = 0, a NaN with the sign clear is outside; min and max by rank_key.  THE BOUND n <= 2^27 holds per statistic
 *   entry at r     entry r of the list afis_rank_subject_hits_filtered(..., -INFINITY, cap) gives query q, for any cap > r and every r, not only the first
 *                  AFIS_HITS_MAX: ordered word descending, equal words by ascending subject id
 * "[subjects]" below is one output per distinct id of the handle in ascending id order (the handle's slots), whatever the search covered.
 * afis_subject_score_stats      axis 0: out [n_q], per query the statistic over the persons (the person cohort: T-norm at the person level); axis 1: out [subjects],
 *                               per person the statistic over the queries (the per-person Z-norm).  Refuses a normalised matrix with AFIS_ESTATE, as afis_score_stats
 * afis_subject_score_histogram  axis 0: counts [n_q][n_edges + 1]; axis 1: counts [subjects][n_edges + 1] (the reverse-direction threshold).  Accepts a normalised
 *                               matrix: edges are then in z units
 * afis_subject_entries_at       for target (q, r): status AFIS_POS_LISTED, subject_id, subject_score (the bits of the person's best cell) and best_idx (the GLOBAL index
 *                               of the template that holds it, as afis_rank_subject_hits names it); r at or beyond the row's number of entries: AFIS_POS_NO_ENTRY, id
 *                               -1, score -inf, best_idx -1.  The round trip: afis_rank_subject_positions(q, subject_id) returns n_before == r.  Accepts a normalised
 *                               matrix.  On the device the select runs over the composites (ordered word, ~slot), unique inside a row
 * A person the search did not cover (a subset search) has no cell in any row: along axis 1 their statistic is (0, 0, 0, 0, 0, +inf, -inf) and their counts are 0; the
 * names stay global.  The matrix is neither written nor invalidated; a refused call leaves it rankable.  AFIS_EINVAL, before anything is queued: a handle that is not a
 * live subject handle of this context, an axis other than 0 or 1, n_edges outside 1 .. AFIS_HIST_EDGES_MAX, a NaN edge, edges that do not ascend strictly, outputs x
 * (n_edges + 1) above AFIS_HIST_COUNTS_MAX, a statistic over more than 2^27 cells, a negative rank, a query outside 0 .. n_q - 1, a null output where there is
 * something to return, and afis_rank_subject_hits_filtered's cases.  n_q == 0, an empty shard or a handle without subjects: AFIS_OK, no device work — statistics empty,
 * counts 0, every target AFIS_POS_NO_ENTRY.  Device and pinned room — the filtered copy, 12 bytes per (query, person) for the maxima and their keys, axis 1's transposed
 * keys, the template forms' tables and outputs — is ensured before anything is queued (AFIS_EDEVICE otherwise).  Everything else is afis_rank_subject_hits_filtered's.
 * NO NEW NORMALISING CALL: z = (v - offset) x scale with scale > 0 is increasing, so a person's best z is the z of their best score; afis_normalize_scores(axis 1),
 * fed with every column's PERSON pair (host/matcher.py::expand_subject_pairs), or axis 0 with the person cohort's pair, leaves exactly the person z-scores in every
 * subject list.
 * On the device: k_subject_keys takes the high halves of the maxima [n_q][S] into a matrix of 4-byte person cells in one coalesced pass, and the kernels of the
 * template forms run over it — the same counting bodies, instantiated for a cell that is its own key (csrc/score_cell.h); only the select's last kernel differs.
 * Options "subject_score_stats_us", "subject_score_histogram_us" and "subject_entries_at_us" (read-only): the device time of the last call's launches, the pre-passes
 * included.  Measured on one MI355X on a planted matrix of 100 latents x 100 000 templates (tools/subject_distribution_timing.py,
 * profiles/subject_distribution_timing.json; medians of five rounds after a discarded first, the cases interleaved), 10 000 persons of ten templates / every template a
 * person: afis_subject_score_stats per latent 93 / 145 us, afis_subject_score_histogram at 256 bins 85 / 140 us, afis_subject_entries_at with one rank per row 152 / 283
 * us — beside afis_rank_subject_hits at cap 1 with the same handle (the fold and one rank pass) 77 / 360 us and the template forms over the 100 000 columns 64, 68 and
 * 207 us: every person call stays below the sum of its two yardsticks (0.23 to 0.83 of it).
 * Shards: person distributions merge only for galleries SHARDED BY PERSON — the maxima of two ranks over one person's prints neither add nor concatenate, the caveat
 * of merge_case_subject_hits' sums — (host/sharding.py::merge_subject_score_stats, merge_subject_score_histograms: ValueError where an id appears on two ranks).
 * These calls do not give: distributions of case lists or of column (reverse) lists; an exchange between ranks inside the library; persons whose prints straddle
 * shards. */
int afis_subject_score_stats(afis_ctx* ctx, afis_subjects* s, int axis, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                             const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl_subject /*[excl_off[n_q]]*/, int n_q,
                             afis_score_stat* out /*axis 0: [n_q]; axis 1: [subjects]*/);
int afis_subject_score_histogram(afis_ctx* ctx, afis_subjects* s, int axis, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                                 const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl_subject /*[excl_off[n_q]]*/, int n_q,
                                 int n_edges, const float* edges /*[n_edges]*/, int64_t* counts /*axis 0: [n_q][n_edges + 1]; axis 1: [subjects][n_edges + 1]*/);
int afis_subject_entries_at(afis_ctx* ctx, afis_subjects* s, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                            const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl_subject /*[excl_off[n_q]]*/,
                            int n_q, int64_t n_targets, const int32_t* query /*[n_targets]*/, const int64_t* rank /*[n_targets], >= 0*/,
                            int32_t* status /*[n_targets]*/, int64_t* subject_id /*[n_targets]*/, float* subject_score /*[n_targets]*/, int64_t* best_idx /*[n_targets], GLOBAL*/);

/* Link groups (no reference counterpart): every call above answers a question about one row or one column; these two look at rows and columns together and return the
 * GROUPS the last search's matrix makes above a decision score — consolidation: which enrolled prints, or persons, are one finger or person (if A hits B and B hits C
 * that is one group {A, B, C}, not three lists to reconcile); cross-case linking: which latents hit the same print, or the same person — as the connected components of
 * a graph, on the device, without the [n_q][G] matrix leaving it.  Both read the score matrix of the context's LAST search through the filtered ranking calls' own checks
 * and filter pass (afis_rank_hits_filtered's rules for labels, masks and the exclusions' CSR; afis_link_subject_groups' excl holds SUBJECT ids as
 * afis_rank_subject_hits_filtered's, and a person excluded for a row takes every cell of that row at a print of theirs out), and both ACCEPT a normalised matrix:
 * min_score is then in z units.  Integers and names only: no float is added anywhere.  The matrix is neither written nor invalidated.
 * Definitions (csrc/link_groups.h holds them once, for the kernels and the host; the tests hold the device to them exactly):
 *   reaches        a cell reaches when rank_key(cell) >= rank_key(min_score): afis_rank_hits' decision and its + 0.0f, so the two zeros are one value.  A cell that holds
 *                  0xffffffff, or any other NaN with the sign set, is no entry and never an edge
 *   nodes          every column is a node: its name is its GLOBAL template index (afis_link_groups) or the subject id of its template (afis_link_subject_groups: all
 *                  columns of one person are ONE node).  Row q is the node row_node[q] names — a global template index (the resident print the row is, as passed to
 *                  afis_search_prints), or a subject id — or, at -1, a node of its own (a latent), reported as -1 - q; row_node NULL: every row is -1.  A named row whose
 *                  name is a column's name IS that column's node; a named row that matches no column — a print outside the subset's columns, a person the handle does
 *                  not hold, a print of another rank that arrived as a host view — is a node with that name; several rows with one name are one node
 *   edges          AFIS_LINK_ANY: cell (q, c) is an edge when it reaches and row q and column c are different nodes.  AFIS_LINK_MUTUAL: and the REVERSE cell reaches too
 *                  — the matcher is not symmetric: cell (A, B) is A as a query view against B as a gallery template —: the cell in the first row whose node is c's
 *                  node, at the column of row q's print.  afis_link_subject_groups' row_node names only a person: the column is the FIRST column, by ascending global
 *                  template index, whose node is q's node; a reverse cell at another print of the same person is not seen.  Where no such row or no such column
 *                  exists in this matrix the cell is not an edge: it cannot be confirmed here.  The reverse cell is read from the same matrix, filtered or not, as the
 *                  forward cell.  A cell between a node and itself is never an edge and never counted: a print against itself, two prints of one person, a repeated
 *                  query print.  n_edges is the number of cells that are edges: a mutual pair counts as two.  In AFIS_LINK_ANY mode with row_node NULL it is the sum
 *                  of afis_rank_hits_filtered's n_hits at min_score
 *   groups         the connected components of that graph that hold at least two nodes (single linkage).  The order of nodes: named nodes by ascending name, then
 *                  anonymous rows by ascending q; a group's members stand in that order and the groups are ordered by their first member.  A group always holds a
 *                  named node.  A subset listed out of order behaves as everywhere else: names are global and the order is by name
 * Outputs: n_groups and n_members are the true totals; group_off[0 .. n_listed] is a CSR into member over the longest prefix of the groups that fits both caps, n_listed
 * the groups in it.  The caps may be 0: counts only (group_off still takes group_off[0]).  The result is a function of the matrix and the arguments only, never of the
 * order in which the device meets the edges.
 * AFIS_EINVAL, before anything is queued and with the matrix still rankable, in addition to afis_rank_hits_filtered's cases: a NaN min_score, a mode other than 0 or 1, a
 * row_node below -1, a negative cap, a null output (member may be null at cap_members 0).  An empty shard or n_q == 0: AFIS_OK, every count 0, no device work.  Device
 * and pinned room — the filtered copy, 12 bytes per node (columns or persons, named rows, anonymous rows) and the tables, 8 bytes per node to return — is ensured before
 * anything is queued (AFIS_EDEVICE otherwise).  AFIS_EDEVICE "the union did not settle": a step bound of the device's union-find (csrc/link_groups.h derives it) was
 * reached, which a correct run never does; the matrix stays rankable.  Everything else is afis_rank_hits_filtered's: which searches count and what invalidates the
 * matrix, the AFIS_ESTATE cases, the handles' life cycles.  No result of a search changes because these functions exist.
 * On the device (csrc/link_groups.hip): one pass over the matrix in k_score_hist_rows' access pattern, with work only where a cell reaches — mutual mode adds one
 * dependent read there — and a lock-free union-find whose hooks always hang the greater root under the smaller; labels, group sizes and the compaction of the linked
 * nodes follow behind a kernel boundary.  The counts return first, then 8 bytes per linked node: what crosses PCIe is proportional to the linked nodes, not to G.
 * Options "link_groups_us" (read-only): the device time of the last call's launches; "link_d2h_bytes" (read-only): the bytes it returned from the device, 32 where
 * nothing links.
 * Measured on one MI355X on planted matrices of cells uniform in [0, 1) (tools/link_groups_timing.py, profiles/link_groups_timing.json; medians of three rounds after
 * a discarded first, the cases interleaved, spread in brackets), AFIS_LINK_ANY: 100 latents x 100 000 — 32 us [2] where no cell reaches (afis_score_histogram with
 * one edge over the same matrix, which reads it once: 32 us [13]; ratio 1.0), 282 us [4] where 1e-3 of the cells reach (9 983 edges, one group of 9 568 nodes, 76 576
 * bytes returned), 2 997 us [44] where every cell reaches (1e7 edges); 1 000 prints x 100 000 — 121 us [6] (the histogram: 155 us [1]; ratio 0.78; 32 bytes
 * returned), 1 247 us [48] at 1e-3 (100 024 edges, 63 757 nodes linked, 510 088 bytes), 188 us [4] at 1e-3 in AFIS_LINK_MUTUAL (2 edges), 3 359 us [221] where every
 * cell reaches (1e8 edges).  The host route — the matrix's bytes copied to the host (0.7 / 7.2 ms) plus numpy keys and a Python union-find — took 66 and 74 ms for
 * the latents' matrix and 492 and 573 ms for the prints' at the first two thresholds.
 * Shards (host/sharding.py::merge_link_groups): a host union over the per-rank CSRs by member name.  Named nodes share one name space across ranks; the anonymous rows
 * -1 - q are shared when every rank ran the same queries.  AFIS_LINK_MUTUAL groups merge correctly only where a pair's two cells lie on one rank.
 * These calls do not give: linkage rules other than single linkage — average or complete linkage, a per-group weakest link: a later call on top of the same labels —;
 * mutual confirmation across ranks; the `match` CLI. */
#define AFIS_LINK_ANY    0
#define AFIS_LINK_MUTUAL 1
int afis_link_groups(afis_ctx* ctx, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                     const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/, int n_q,
                     const int64_t* row_node /*[n_q] or NULL*/, float min_score, int mode, int64_t cap_groups, int64_t cap_members,
                     int64_t* n_edges, int64_t* n_groups, int64_t* n_members, int64_t* n_listed,
                     int64_t* group_off /*[cap_groups + 1]*/, int64_t* member /*[cap_members]*/);
int afis_link_subject_groups(afis_ctx* ctx, afis_subjects* s, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                             const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl_subject /*[excl_off[n_q]]*/, int n_q,
                             const int64_t* row_node /*[n_q] subject ids, or NULL*/, float min_score, int mode, int64_t cap_groups, int64_t cap_members,
                             int64_t* n_edges, int64_t* n_groups, int64_t* n_members, int64_t* n_listed,
                             int64_t* group_off /*[cap_groups + 1]*/, int64_t* member /*[cap_members]*/);

/* Case lists (no reference counterpart): an examiner's unit of work is a CASE — the same impression encoded twice, several lifts of one finger, several fingers of one
 * hand — and fusing the queries of a case is one list per case instead of one per query.  Both calls rank the matrix of the context's LAST search; a case cannot span
 * searches: all its latents must be queries of the one search that is ranked.  On the device the member rows of every case are folded into one fused row
 * (case_fuse.hip) and the fused rows are ranked by the kernel of afis_rank_hits, unchanged; only n_cases x (8 + cap x 12) bytes return, through the pinned buffer.
 * afis_rank_case_hits          the templates: idx / score as afis_rank_hits' (global indices; for a subset search the listed templates only, whatever order the list had).
 * afis_rank_case_subject_hits  the enrolled persons of a subject handle: subject_id / score.  No best_idx: per-latent detail is afis_rank_subject_hits' job, and that call
 *                              stays available on the same matrix.
 * Rows: case_of[i] is the caller's id (any int64 >= 0, any order, not dense) of the case query position i belongs to.  The distinct ids in ascending order are the rows
 * of the outputs, case_id[c] returns the id of row c, and n_cases must be the number of distinct ids (AFIS_EINVAL otherwise; the message carries both numbers).
 * The fused value of (case, column j) — a column is a template, or a subject slot — over the case's MEMBERS, its queries in ascending query position, v_m a member's value
 * in that column: the score the matrix holds, or the subject's best score for that query exactly as afis_rank_subject_hits makes it (a subject none of whose templates the
 * search covered is no entry, for every case alike, and is neither counted nor listed).  A member TAKES PART when rank_key(v_m) >= rank_key(+0.0f) (csrc/rank_order.h):
 * the -1 of an empty entry or of a latent-empty query, every negative value and a NaN with the sign set stay out.
 *   AFIS_CASE_SUM  acc = +0.0f; for the members in ascending position, if the member takes part, acc = acc + v_m — one fp32 add each, never reassociated, never
 *                  contracted; -1.0f when no member takes part
 *   AFIS_CASE_MAX  the v_m of greatest rank_key, with the bits of the first such member (-1 loses by itself)
 * The lists are afis_rank_hits' lists over the fused rows in every respect: the key is the bits of fused + 0.0f in their total order, min_score treated the same way,
 * descending; equal keys by ascending global template index, or ascending subject id; n_hits[c] may exceed cap; the rest is padded with -1 / -inf; min_score = -INFINITY
 * gives a rank list of length cap.  (On the device an uncovered subject's fused word is 0xffffffff: a NaN with the sign set, whose key lies below -inf's and so below
 * every min_score — the property of the key stated for afis_rank_hits above.)
 * Which searches count, what invalidates the matrix and what leaves it alone are exactly as for afis_rank_hits.  Both calls leave the matrix rankable: they may be
 * repeated and mixed with afis_rank_hits, afis_rank_subject_hits, afis_rank_subjects and afis_rank_latent_hits; a wait that times out invalidates it.  AFIS_ESTATE: no
 * matrix to rank, or a subject handle of an older gallery.  AFIS_EINVAL: a mode other than AFIS_CASE_SUM / AFIS_CASE_MAX, a negative case id, a null array, an n_q that
 * is not the last search's, a wrong n_cases, cap outside 1 .. AFIS_HITS_MAX, a NaN min_score, a subject handle that is not live.  n_q == 0 returns AFIS_OK when
 * n_cases == 0.  With an empty shard, or a handle without subjects, every n_hits is 0 and every entry padding.  Device and pinned room — the fused matrix,
 * n_cases x columns x 4 bytes in a buffer of its own, the cases' member tables, n_q x subjects x 8 bytes for the subjects' maxima, the outputs — is ensured before
 * anything is queued: AFIS_EDEVICE, with nothing changed, when that fails.  No result of a search changes because these functions exist.
 * Shards: the columns of different shards are disjoint and a case's row is common, so the per-rank template lists merge with host/sharding.py::merge_hits as they are;
 * the subject lists merge with merge_case_subject_hits — exactly for AFIS_CASE_MAX, for AFIS_CASE_SUM only while no subject's prints lie in two shards. */
#define AFIS_CASE_SUM 0
#define AFIS_CASE_MAX 1
int afis_rank_case_hits(afis_ctx* ctx, const int64_t* case_of /*[n_q]*/, int n_q, int mode, int64_t n_cases, float min_score, int cap,
                        int64_t* case_id /*[n_cases]*/, int64_t* n_hits /*[n_cases]*/, int64_t* idx /*[n_cases][cap]*/, float* score /*[n_cases][cap]*/);
int afis_rank_case_subject_hits(afis_ctx* ctx, afis_subjects* s, const int64_t* case_of /*[n_q]*/, int n_q, int mode, int64_t n_cases, float min_score, int cap,
                                int64_t* case_id /*[n_cases]*/, int64_t* n_hits /*[n_cases]*/, int64_t* subject_id /*[n_cases][cap]*/, float* score /*[n_cases][cap]*/);

/* Filtered hit lists (no reference counterpart): an operational latent search is never unrestricted — a latent record carries the finger positions it may come from,
 * often a hand, a sex or a region code, and the elimination prints (the victim's, the officers', persons already examined) leave the list before anyone looks at it.  A
 * filter shared by a whole batch is best served by afis_subset_create, which saves the scoring; a filter that differs PER QUERY is applied here, at ranking time, on the
 * device: the cells a query is not eligible for are taken out of a copy of the matrix (hit_filter.hip) and the copy is ranked by the kernels of afis_rank_hits and
 * afis_rank_subject_hits, unchanged.  The matrix itself is never written.
 * afis_labels_create   label[0 .. n): one 64-bit attribute word for resident template index_base + i; the bits are the caller's (say ten one-hot finger positions, two for
 *                     sex, the rest a region code).  The life cycle is afis_subjects_create's, rule for rule: n must be the resident shard's size (option
 *                     "gallery_resident"; AFIS_EINVAL otherwise); a call before the first commit is AFIS_ESTATE; a refused call leaves nothing allocated; create and free
 *                     first wait for all device work of the context and leave the last search's matrix rankable; several handles may be live at once and afis_destroy
 *                     releases those that are left; the n x 8 bytes uploaded count in option "gallery_h2d_bytes".  A handle belongs to the gallery as it was: after an
 *                     appending commit or a removal that changed the shard both ranking calls refuse it with AFIS_ESTATE (afis_labels_free still works).
 * afis_rank_hits_filtered          afis_rank_hits over the eligible cells; excl holds GLOBAL template indices.
 * afis_rank_subject_hits_filtered  afis_rank_subject_hits over the eligible cells; excl_subject holds subject ids, and an excluded person is no entry for that query.
 * Eligibility of cell (q, t), L the label of the template at that column (for a subset search: of the listed template the column belongs to):
 *   the label test  masks[q] = (any_of, all_of, none_of); the cell passes when (any_of == 0 || (L & any_of) != 0) && (L & all_of) == all_of && (L & none_of) == 0.
 *                   With one-hot fields "finger in {2, 7} and sex = F" is a single none_of: the complement of the allowed bits inside those fields.  masks == NULL
 *                   means no label test, and labels may then be NULL; masks given with labels == NULL is AFIS_EINVAL.
 *   the exclusions  a CSR per query: excl_off[n_q + 1] with excl_off[0] == 0, never decreasing, into excl[excl_off[n_q]], every entry >= 0 (any violation is AFIS_EINVAL
 *                   with nothing queued).  An entry that names nothing the search covered — an index outside this shard, an index a subset does not list, an id the
 *                   subject handle does not hold — is ignored silently, so that the same list can be handed to every rank of a sharded gallery; duplicates are
 *                   no-ops.  excl_off == NULL means no exclusions.
 * The result is exactly the lists afis_rank_hits or afis_rank_subject_hits would give if the ineligible cells did not exist: the keys, the tie rules, the treatment of
 * min_score, n_hits exceeding cap and the padding (-1 / -inf / -1) are theirs; min_score = -INFINITY gives a rank list of length cap.  For subjects a person's score is
 * the best among their ELIGIBLE covered templates and best_idx the lowest such index among equal scores; a person with no eligible covered template is neither counted
 * nor listed.  With no masks and no exclusions the outputs are entry for entry those of the unfiltered call.  (On the device an ineligible cell is the word 0xffffffff,
 * the "no entry" word of the case lists: a NaN with the sign set, whose key lies below -inf's and so below every min_score.  A matrix cell that already held that word
 * could not be told from an ineligible one; a search never produces it.)
 * Which searches count, what invalidates the matrix and what leaves it alone, the AFIS_ESTATE and AFIS_EINVAL cases and the answers for an empty shard and n_q == 0 are
 * exactly afis_rank_hits' and afis_rank_subject_hits'; in addition a labels handle that is not live in this context is AFIS_EINVAL.  Both calls leave the matrix
 * rankable and unchanged: they may be repeated with other filters and mixed with every other ranking call, which keep returning their unfiltered results.  Device and
 * pinned room — the filtered copy, n_q x templates x 4 bytes in a buffer of its own, the masks and the resolved exclusions, n_q x subjects x 8 bytes for the subjects'
 * maxima, the outputs — is ensured before anything is queued: AFIS_EDEVICE, with nothing changed, when that fails.  No result of a search changes because these
 * functions exist.
 * The same eligibility filters the case lists and the reverse (column) lists:
 * afis_rank_case_hits_filtered          afis_rank_case_hits, every column folded over the members that are eligible for it; excl holds GLOBAL template indices.
 * afis_rank_case_subject_hits_filtered  afis_rank_case_subject_hits likewise; excl_subject holds subject ids.
 * afis_rank_latent_hits_filtered        afis_rank_latent_hits over the eligible cells: per covered template, the queries that are eligible for it; excl holds GLOBAL
 *                                       template indices.
 * masks, excl_off and excl are per QUERY (n_q of the last search), as above, whatever the call lists: a case's members carry their own masks — "several fingers of one
 * hand" is latent A an index or a middle finger, latent B a ring or a little finger — and a case-wide elimination list is that list repeated for each member.
 * Filtered case lists: for case c and column j let E be the members of c that are eligible for j, in ascending query position.
 *   templates  v_m is the matrix cell.
 *   subjects   v_m is the person's best score among their covered templates that are eligible for member m, compared on the raw ordered word exactly as
 *              afis_rank_subject_hits_filtered makes it; m is in E only if such a template exists and the person is not on m's exclusion list.
 *   E empty    NO ENTRY: the column is neither counted nor listed for that case, whatever min_score is.  (An uncovered subject is uncovered for every member: the
 *              unfiltered calls' "no entry, for every case alike" is this state.)
 *   AFIS_CASE_SUM  acc = +0.0f; for m in E in ascending position, if m takes part, acc = acc + v_m — one fp32 add each, never reassociated, never contracted; -1.0f when
 *                  E is not empty and no member of E takes part: that is an entry, listed when min_score <= -1
 *   AFIS_CASE_MAX  the v_m of greatest rank_key over E, with the bits of the first such member
 * Everything else — the rows and case_id, the key and the treatment of min_score, the tie rules, n_hits exceeding cap, the padding, min_score = -INFINITY — is
 * afis_rank_case_hits' / afis_rank_case_subject_hits'.  With filters that pass every cell the outputs are entry for entry those of the unfiltered call.
 * Filtered reverse lists: the key, the tie rule (ascending query position), latent_base, the padding and the row order for a subset listed out of order are
 * afis_rank_latent_hits'; a template no query is eligible for has n_hits 0 and all padding.
 * The caveat above carries over: a matrix cell that already held 0xffffffff could not be told from an ineligible one; a search never produces it.
 * Every argument rule, AFIS_EINVAL / AFIS_ESTATE case, empty-shard and n_q == 0 answer of the two siblings a call combines applies unchanged, nothing is queued on a
 * refusal, and which searches count, what invalidates the matrix and what leaves it alone are afis_rank_hits'.  All three calls leave the matrix rankable and unwritten
 * and may be mixed with every other ranking call.  With neither masks nor exclusions they are their plain siblings, on the matrix itself.  Device and pinned room — the
 * filtered copy, the fused or transposed matrix, the tables, the subjects' maxima, the outputs — is ensured before anything is queued: AFIS_EDEVICE, with nothing
 * changed, when that fails.  On the device the filter pass above runs first, unchanged; the folds of case_fuse.hip then skip a member whose cell is no entry, and the
 * transpose reads the copy.
 * Not in this interface: a case spanning searches (a case cannot span searches, filtered or not), and filters on afis_search's own top-k and on afis_rank_subjects.
 * Shards: every rank labels its own shard and takes the same masks and exclusion lists; the columns of different shards are disjoint and a filtered maximum is still a
 * maximum, so the per-rank lists merge with host/sharding.py::merge_hits and merge_subject_hits as they are.  The filtered case template lists and the filtered column
 * lists are merge_hits input as they are; the filtered case subject lists merge with merge_case_subject_hits under its conditions — exactly for AFIS_CASE_MAX, for
 * AFIS_CASE_SUM only while no subject's prints lie in two shards. */
/* (typedef afis_labels: with the rank positions above, which take the handle too) */
int afis_labels_create(afis_ctx* ctx, const uint64_t* label /*[n]*/, int64_t n, afis_labels** out);
void afis_labels_free(afis_ctx* ctx, afis_labels* labels);
int afis_rank_hits_filtered(afis_ctx* ctx, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                            const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/,
                            int n_q, float min_score, int cap, int64_t* n_hits /*[n_q]*/, int64_t* idx /*[n_q][cap]*/, float* score /*[n_q][cap]*/);
int afis_rank_subject_hits_filtered(afis_ctx* ctx, afis_subjects* s, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                                    const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl_subject /*[excl_off[n_q]]*/,
                                    int n_q, float min_score, int cap, int64_t* n_hits /*[n_q]*/, int64_t* subject_id /*[n_q][cap]*/, float* subject_score /*[n_q][cap]*/,
                                    int64_t* best_idx /*[n_q][cap]*/);
int afis_rank_case_hits_filtered(afis_ctx* ctx, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                                 const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/,
                                 const int64_t* case_of /*[n_q]*/, int n_q, int mode, int64_t n_cases, float min_score, int cap,
                                 int64_t* case_id /*[n_cases]*/, int64_t* n_hits /*[n_cases]*/, int64_t* idx /*[n_cases][cap]*/, float* score /*[n_cases][cap]*/);
int afis_rank_case_subject_hits_filtered(afis_ctx* ctx, afis_subjects* s, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                                         const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl_subject /*[excl_off[n_q]]*/,
                                         const int64_t* case_of /*[n_q]*/, int n_q, int mode, int64_t n_cases, float min_score, int cap,
                                         int64_t* case_id /*[n_cases]*/, int64_t* n_hits /*[n_cases]*/, int64_t* subject_id /*[n_cases][cap]*/, float* score /*[n_cases][cap]*/);

/* Reverse search (no reference counterpart): every newly enrolled ten-print card is searched against the file of unsolved latents — the transaction that solves old cases.
 * The pair score is the forward search's; what differs is who stays on the device and which way the matrix is read.  The latents (about 260 KB each, against 50 KB per
 * print) are uploaded once with afis_queries_upload_reserved; per card the caller appends the prints (afis_gallery_reopen, afis_gallery_add*, afis_gallery_commit), lists
 * their indices in afis_subset_create, runs afis_search_subset_resident with k = 0 and no outputs, and reads the answer with
 * afis_rank_latent_hits  the hit lists of the context's LAST search taken along the COLUMNS of its matrix: per template the search covered, the search's queries whose
 *                     score reaches min_score.  n_templates must be the number of columns that search covered — the resident shard's size for a full search, the
 *                     subset's n for a subset search (AFIS_EINVAL otherwise).  Row j of the outputs belongs to idx[j] of the subset's list in the caller's order, or to
 *                     template index_base + j of a full search:
 *                       n_hits[j]      how many queries qualify; it may exceed cap
 *                       latent_idx     latent_base + the query's position in the search, for the first min(n_hits[j], cap) entries of the order below; then -1
 *                       score          the scores of those entries, their own bits; then -inf
 *                     The key is afis_rank_hits': the bits of score + 0.0f in their total order, min_score treated the same way, descending; equal keys by ascending
 *                     query position.  On the scores a search produces that is plainly score >= min_score.  min_score = -INFINITY gives the cap best latents of
 *                     every print.  Latent-empty queries and empty or removed templates take part with the -1 the matrix holds.  With n_templates == 0, or a last
 *                     search of no queries, the call returns AFIS_OK with zero counts and padding.  latent_base (>= 0) is where this handle's first latent stands
 *                     in the caller's file: a file kept as several handles, or spread over ranks, is searched handle by handle and the per-column lists merge
 *                     exactly (host/sharding.py::merge_hits — the columns are common, the latents disjoint).
 *                     Which searches count, what invalidates the matrix and what leaves it alone are exactly as for afis_rank_hits; the call may be repeated and mixed
 *                     with afis_rank_hits, afis_rank_subject_hits and afis_rank_subjects.  AFIS_EINVAL: cap outside 1 .. AFIS_HITS_MAX, a NaN min_score, a negative
 *                     latent_base, a null output, a wrong n_templates; AFIS_ESTATE: no matrix to rank.  On the device the matrix is transposed through local memory
 *                     in 64 x 64 tiles (latent_rank.hip) and the transposed rows are ranked by the kernel of afis_rank_hits, unchanged.  The device keeps
 *                     n_templates x n_q x 4 bytes for the transposed matrix beside the outputs; that room and the pinned return buffer are ensured before anything is
 *                     queued: AFIS_EDEVICE, with nothing changed, when that fails.  Only n_templates x (8 + cap x 12) bytes return.
 * The P prints of one card fuse into one list per card with host/sharding.py::merge_prints_to_card.  No result of a search changes because these functions exist. */
int afis_rank_latent_hits(afis_ctx* ctx, int64_t n_templates, float min_score, int cap, int64_t latent_base,
                          int64_t* n_hits /*[n_templates]*/, int64_t* latent_idx /*[n_templates][cap]*/, float* score /*[n_templates][cap]*/);
/* afis_rank_latent_hits over the cells each query is eligible for (the contract stands with the filtered hit lists, above): n_q of masks and excl_off is the last search's */
int afis_rank_latent_hits_filtered(afis_ctx* ctx, afis_labels* labels /*or NULL*/, const uint64_t* masks /*[n_q][3] or NULL*/,
                                   const int64_t* excl_off /*[n_q + 1] or NULL*/, const int64_t* excl /*[excl_off[n_q]]*/,
                                   int64_t n_templates, float min_score, int cap, int64_t latent_base,
                                   int64_t* n_hits /*[n_templates]*/, int64_t* latent_idx /*[n_templates][cap]*/, float* score /*[n_templates][cap]*/);

/* Eligible search (no reference counterpart): the filters above run at ranking time, after every pair has been scored; with masks that pass a tenth of the cells nine
 * tenths of the search's work goes into cells the next call removes.  afis_search_eligible scores a (query, template) pair only where the query is ELIGIBLE for the
 * template and leaves a matrix the whole ranking family reads unchanged.  labels and masks [n_q][3] are both required (AFIS_EINVAL when either is NULL).
 * Eligibility of cell (q, t) is the label test of the filtered hit lists, word for word, L the label of resident template index_base + t:
 *   (any_of == 0 || (L & any_of) != 0) && (L & all_of) == all_of && (L & none_of) == 0
 * Values   an eligible cell holds, bit for bit, the value afis_search gives that pair under every option (an empty or removed entry and a latent-empty query give their
 *          -1); an ineligible cell holds the word 0xffffffff, the "no entry" word of the filtered lists (csrc/score_order.h: kNoEntryWord) — in the matrix left on
 *          the device and in scores [n_q][G] (NULL: not copied).  status [n_q] (or NULL) is afis_search's.
 * The matrix afterwards   after AFIS_OK the context's last-search matrix is this [n_q][G] matrix: a full search's in every respect — no subset, the resident shard as
 *          it stands — under afis_search's invalidation rules; the call is one of the searches that count.  Consequences:
 *            - afis_rank_hits, afis_rank_subject_hits and afis_rank_latent_hits on it return exactly what their _filtered forms return after a full search with the
 *              same labels and masks and no exclusions;
 *            - the _filtered calls with the same labels and masks, with or without exclusion lists, return exactly what they return after a full search: the filter
 *              pass re-marks cells that are marked already.  The CASE lists must be read this way: the plain case folds turn a no-entry member into "takes no part"
 *              and so list -1 where the filtered folds list no entry;
 *            - exclusion lists stay a ranking-time matter: they are a few cells and save no scoring;
 *            - afis_rank_subjects, rank lists of afis_search's own kind (k, topk_idx) and parts are not in this interface: afis_rank_subjects on this matrix would
 *              take the no-entry word for a score.
 * How     the queries are grouped into CLASSES of identical mask triples, in order of first query position.  A class's eligible templates, in ascending index, are
 *          gathered into a temporary sub-shard through afis_subset_create's path and searched with afis_search_subset's launch sequence — no scoring kernel knows
 *          of it, and a score depends on nothing but its pair — then one pass (csrc/eligible_expand.hip) writes every word of the class's rows of the combined
 *          matrix once.  One temporary sub-shard is live at a time, in buffers that only grow from class to class; it is never a subset of the caller's: option
 *          "subset_device_bytes", "subset_gather_us" and "gallery_h2d_bytes" read as before, and it is released before the call returns.  A class that passes every
 *          template — the triple (0, 0, 0), or any triple the whole shard passes — runs on the resident shard itself, with no copy; a class no template passes
 *          scores nothing: its rows are all no entry, its status is still afis_search's.  The combined matrix lives in a buffer of its own ([n_q][G] floats beside
 *          the search's) whose room, with the call's tables, is ensured before anything is queued.
 *          It PAYS WHEN LATENTS SHARE MASKS: every class costs a sub-shard (tables, derived layouts, waits) and a launch sequence of its own, whatever its size
 *          (DESIGN section 7, row 13 has the measurements; merging small classes into one search over the union of their templates is a follow-up).
 * Arguments   AFIS_EINVAL: labels or masks NULL, n_q < 0, n_q > 0 with queries NULL, a labels handle not live in this context, a bad latent view (as afis_search);
 *          AFIS_ESTATE: a call before the first commit, a labels handle from before a gallery edit (afis_rank_hits_filtered's rules).  n_q == 0 returns AFIS_OK as
 *          afis_search with no queries does.  On any failure in the middle the call returns that code and holds nothing it allocated; the last-search matrix is
 *          invalid; the caller's own live subsets and query handles are untouched.  A timeout follows afis_search_subset's rules (option "search_timeout_s").
 * Timing   afis_get_timing*: every additive field is the sum over the searches the call ran — pairs is the number of pairs actually SCORED, the sum over the classes
 *          of queries x eligible templates — and the two clock fields come from the search with the most pairs.  Options "eligible_classes" and
 *          "eligible_expand_us" (read-only) describe the last call.
 * Shards: every rank labels its own shard and takes the same masks; the columns of different shards are disjoint, so the per-rank lists read from this matrix are
 * host/sharding.py::merge_hits / merge_subject_hits input as they are.  No result of afis_search changes because this function exists. */
int afis_search_eligible(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks /*[n_q][3]*/,
                         const afis_template_view* queries, int n_q,
                         float* scores /*[n_q][G] or NULL*/, int32_t* status /*[n_q] or NULL*/);

/* Packed gallery container (no reference counterpart: the reference re-parses every rolled .dat for every pair,
 * matching/matcher.cpp:173,:278).  One mmap-able file holding the staged gallery's SoA arrays (layout: csrc/template_io.h), so a
 * 100k-1M template gallery is loaded — whole, or one contiguous shard per GPU — without touching 100k-1M small files.
 * afis_gallery_save   writes the templates staged so far (before afis_gallery_commit); names[i] (optional) = the path template
 *                     i was read from, kept for the score files.
 * afis_gallery_load   appends templates [first, first+count) of the file (count < 0: to the end) to the staged gallery.  Into an EMPTY staging
 *                     area (the usual case: one container, or one shard of it per rank) the file is validated and kept mapped, and
 *                     afis_gallery_commit uploads the range straight from the mapping (no host copy of its 50 KB per template): the
 *                     file must not be truncated or rewritten between the two calls (a truncation found at commit time is AFIS_EFORMAT; one that happens WHILE the commit copies from the mapping
 *                     faults in the host process, as for any mapped file).  Any other staging call in between first copies
 *                     the range into host memory, as every load into a non-empty staging area does.
 * afis_gallery_file_info  template / point totals, and (optional) the texture point count of every template, the quantity shards
 *                     are balanced by.
 * afis_gallery_file_names  the names of a range as consecutive NUL-terminated strings; buf == NULL only reports *need. */
int afis_gallery_save(afis_ctx* ctx, const char* path, const char* const* names);
int afis_gallery_load(afis_ctx* ctx, const char* path, int64_t first, int64_t count);
int afis_gallery_file_info(const char* path, int64_t* G, int64_t* n_minutiae, int64_t* n_tex_points, int32_t* tex_counts /*[G] or NULL*/);
int afis_gallery_file_names(const char* path, int64_t first, int64_t count, char* buf, size_t cap, size_t* need);

/* Matcher::One2One_matching_all_templates (matching/matcher.cpp:339-374) for one latent against the whole resident gallery:
 * scores[g][i] for i < n_minu = latent minutiae template i vs rolled minutiae template 0, scores[g][n_minu + t] = latent texture
 * template t vs rolled texture template 0; zero where the reference leaves the zero-filled vector untouched.
 *   scores        [G][query->n_minu + query->n_tex]
 *   rolled_status [G] or NULL : 0, or 2 = rolled template empty (the reference returns 2 before scoring, :350-353)
 *   query_status  NULL or out : AFIS_QUERY_LATENT_EMPTY when the latent has no template at all (:345-348) */
int afis_match_all_templates(afis_ctx* ctx, const afis_template_view* query, float* scores, int32_t* rolled_status, int32_t* query_status);

/* Weighted search (no reference counterpart): afis_search fuses one fixed set of a latent's templates — minutiae templates 27, 3 and 12 and 0.3 x texture template 0,
 * the layout of one extractor.  afis_search_weighted fuses ANY set, per query, as a weighted sum on the device, for a batch of latents, and leaves a matrix the whole
 * ranking family reads: the accuracy of afis_match_all_templates (all 28 + 1 scores) for lists, hits, subjects, cases, filters and positions, and a sensible score for a
 * latent of another extractor (a manual markup plus one automatic template, a re-encoding with 12 templates).
 *   w_minu [n_q][n_wm], w_tex [n_q][n_wt]   one weight row per query; indices are post-strip, as everywhere in this header
 * Active templates   minutiae template i of query q is ACTIVE when i < queries[q].n_minu, i < n_wm and w_minu[q * n_wm + i] != 0.0f; texture template t by the same
 *          rule against n_wt / w_tex.  Only active templates are validated (afis_search's view rules) and uploaded; a template past the end of a weight row or with
 *          weight +-0 costs nothing.
 * Value of cell (q, g)   -1.0f when the rolled entry is empty or removed; -1.0f for the whole row when query q has no active template at all (status[q] is then
 *          AFIS_QUERY_LATENT_EMPTY, otherwise AFIS_QUERY_OK); otherwise (float)acc with
 *            double acc = +0.0;
 *            for the active minutiae templates in ascending i:  acc = acc + (double)w * (double)v_i;
 *            then for the active texture templates in ascending t:  the same
 *          where v is, bit for bit, the entry afis_match_all_templates gives that (latent template, print) — the zeros it leaves included, e.g. for a print without a
 *          minutiae template — under every value of "s3_tie_order", "ref_tie_order" and "adc_variant" 8 / 9.  The product of two fp32 values is exact in fp64, so the
 *          definition does not depend on whether a compiler contracts the multiply-add.  Weights must be finite and >= 0 (-0.0f is a zero) so that -1 keeps meaning
 *          "empty" and every other cell is finite or +inf and >= +0.0, the property all ranking calls state.
 *          With weights 1 at minutiae templates 26, 2, 11 and 0.3f at texture 0 the call runs exactly the scorers afis_search runs.  It does NOT give afis_search's
 *          bits: that fusion adds in fp32 and multiplies by the double 0.3 (the two differ by less than 2^-21 x max(1, score)); and it knows nothing of afis_search's
 *          quirk for latents with fewer than 27 minutiae templates.
 * The matrix afterwards   after AFIS_OK the context's last-search matrix is this [n_q][G] matrix: a full search's in every respect — no subset, the resident shard as it
 *          stands — under afis_search's invalidation rules.  Every ranking call reads it unchanged: afis_rank_hits, afis_rank_subject_hits, afis_rank_latent_hits, the
 *          case and filtered families, afis_rank_positions / afis_rank_subject_positions / afis_count_before and afis_rank_subjects.  afis_correspondences_pairs and
 *          afis_score_pairs leave it alone, as they do after afis_search (they score afis_search's selection, not the weighted one).
 * How     per query the active minutiae templates are packed three to a PSEUDO-QUERY in ascending order and the active texture templates one to a pseudo-query:
 *          n_pq(q) = max(ceil(|A_m| / 3), |A_t|), afis_match_all_templates' packing over the active list.  A scorer's value depends on nothing but its (latent
 *          template, print), so the packing changes no bit.  The pseudo-queries run through afis_search's launch sequence in BATCHES cut at query boundaries — at most
 *          option "weighted_batch_pseudo" pseudo-queries (0 [default]: as many as an eighth of the launch-group budget holds the per-part scores of, 16 bytes per
 *          pair; a query with more pseudo-queries than that is a batch of its own) — their per-part scores stay on the device, and one pass (csrc/template_fold.hip)
 *          folds a batch's parts into its rows of the combined matrix: one thread per cell, in registers, in the order above.  The combined matrix lives in the spare
 *          [n_q][G] buffer beside the search's (afis_search_eligible's) and is swapped in at the end; its room, the largest batch's per-part scores and the call's
 *          tables are ensured before anything is queued (AFIS_EDEVICE when that fails).
 * Arguments   AFIS_EINVAL: a null ctx, n_q < 0, n_q > 0 with queries NULL, n_wm < 0 or n_wt < 0, a null weight array whose width is > 0 (with n_q > 0), a weight
 *          that is NaN, infinite or negative, a bad ACTIVE view; AFIS_ESTATE before the first commit.  n_q == 0 returns AFIS_OK as afis_search with no queries does.
 *          After ANY return other than AFIS_OK — a refused argument included — the last-search matrix is invalid and the call holds nothing it allocated; the
 *          caller's live subsets and query handles are untouched (afis_search_eligible's rules).  Host waits are bounded as a search's are ("search_timeout_s").
 * Timing   afis_get_timing*: every additive field is the sum over the batches — pairs = pseudo-queries x G — and the two clock fields come from the batch with the
 *          most pairs.  Options "weighted_pseudo_queries" and "weighted_fold_us" (read-only) describe the last call.
 * Not in this interface: a subset form; a resident query-handle form; rank lists of afis_search's own kind (k, topk_idx) — afis_rank_hits(-INFINITY, cap) serves;
 *          parts; fusion rules other than the weighted sum; the match CLI.
 * Shards: the columns of different shards are disjoint and the weights common, so the per-rank lists read from this matrix are host/sharding.py::merge_hits /
 *          merge_subject_hits input as they are.  No result of afis_search changes because this function exists.
 * Cost    one MI355X, 100 latents of 28 + 1 templates x 100 000 prints, interleaved runs, medians of three after a discarded first, host clock
 *          (tools/weighted_search_timing.py, profiles/weighted_search_timing.json): (a) all 28 + 1 templates — 1 000 pseudo-queries, 10^8 pairs — 10 384 ms (spread 10)
 *          against 11 311 ms (spread 17) for the only route there was before, one afis_match_all_templates call per latent with the parent commit's library and the
 *          fold on the host: 0.92 x, the same bits; nearly all of either is the scoring (device clock 10 339 ms), what the call adds is the matrix the ranking family
 *          reads.  (b) The reference's selection as weights 1 853.2 ms (spread 19) against afis_search's 1 851.9 ms (spread 12) on the same context, device clock
 *          1 824.9 against 1 823.8 ms: the plan and the fold cost about a millisecond.  (c) The fold of (a) — 1.64 GB read and written — 293 us (spread 14) where a
 *          memory-bound pass at 16 bytes per pseudo-pair predicts 260 us at the 6.3 TB/s a float4 copy reaches here (205 us at the specified 8 TB/s): 5.6 TB/s.
 *          The launch groups of (a) are afis_search's, cut for latents that all carry texture; nine in ten pseudo-queries carry none.  Nothing here is tuned. */
int afis_search_weighted(afis_ctx* ctx, const afis_template_view* queries, int n_q,
                         const float* w_minu /*[n_q][n_wm]*/, int n_wm,
                         const float* w_tex  /*[n_q][n_wt]*/, int n_wt,
                         float* scores /*[n_q][G] or NULL*/, int32_t* status /*[n_q] or NULL*/);

/* Print search (no reference counterpart): every search above starts from a latent.  "Is this person already enrolled?" — the duplicate check of every enrolment — and
 * the linking of the entries of an unsolved-latent file that was enrolled as a gallery start from a RESIDENT PRINT.  afis_search_prints takes resident prints as the
 * queries, builds their query views on the device from the resident shard — only an index list's offset tables cross PCIe, no template does — and leaves a matrix
 * the whole ranking family reads, so that hit lists, subject lists, case lists, filtered lists, rank positions and column lists work for print-to-print search unchanged,
 * with eligibility filters and exclusion lists.
 *   idx [n_q]   GLOBAL indices of the resident shard (index_base included); entries may repeat and come in any order
 *   s           NULL: the columns are the whole resident shard; or a live subset: the columns are the subset's, in the caller's order, exactly as afis_search_subset
 *               lays them out (the query prints need not be in the subset) — a finger-position-restricted duplicate check holds one subset per finger
 *   w_minu [n_q], w_tex [n_q]   one weight per query for the print's minutiae template and for its texture template
 * The query view P of a print   n_minu = 1 when the print has a minutiae template, else 0; minu[0] is that template as the shard holds it — x, y, ori and des, bit for
 *          bit.  n_tex = 1 when it has a texture template, else 0; tex[0] holds the resident points (already clamped to 1000 at enrolment), x, y and ori as held, and
 *          des[r][6 m + k] = codewords[m][code[r][m]][k]: the PQ codes decoded, the codewords' bits copied, no arithmetic.
 * Value of cell (q, column)   bit for bit the value afis_search_weighted gives for the query P, n_wm = 1, n_wt = 1 and the weight rows {w_minu[q]} and {w_tex[q]}:
 *          its activity rule, (float) of the fp64 sum with minutiae before texture, -1 for an empty or removed column, AFIS_QUERY_LATENT_EMPTY and a row of -1 when
 *          nothing is active — an empty or removed print, or both weights zero —, finite weights >= 0 only, and its behaviour under "s3_tie_order", "ref_tie_order"
 *          and "adc_variant" 8 / 9.  A print against itself is an ordinary cell: the caller takes it out with an exclusion list (afis_rank_hits_filtered's excl).
 * The matrix afterwards   after AFIS_OK the context's last-search matrix is this matrix — a full search's record with s == NULL, a subset search's with a subset — under
 *          afis_search's invalidation rules; the call is one of the searches that count, for every ranking call.
 * How     one PSEUDO-QUERY per print with something active, with the selection (0 or -1, -1, -1, 0 or -1); batches are cut as afis_search_weighted cuts them, under
 *          "weighted_batch_pseudo", and a batch's launch groups by the prints' texture rows, from the host's copy of the shard's offsets.  Per launch group seven
 *          query-side tables and three source offset tables are uploaded (one copy, under 128 bytes per query) and csrc/print_queries.hip fills the group's arrays from
 *          the shard: segment copies of the minutiae arrays and the texture points, the print's descriptor fragment tiles as they stand, the texture descriptors
 *          decoded from the PQ codes through the fp32 codebook (read through L2; every output word written once, 16-byte stores).  Then the launch sequence of a
 *          search with the per-part scores kept, and the weighted search's fold (csrc/template_fold.hip), with the subset's empty flags when s is given.  The
 *          combined matrix, the largest batch's per-part scores, the tables and a subset's column permutation are ensured before anything is queued.
 * Arguments   AFIS_EINVAL: a null ctx, n_q < 0, a null idx or weight array with n_q > 0, an index outside the resident shard, a weight that is NaN, infinite or
 *          negative, a subset that is not live in this context.  AFIS_ESTATE: a call before the first commit, an index that is staged but not committed, a subset
 *          made before the last gallery edit.  n_q == 0 returns AFIS_OK as afis_search with no queries does.  After ANY other return the last-search matrix is
 *          invalid and the call holds nothing it allocated.  Host waits are bounded as a search's are ("search_timeout_s").
 * Timing   as afis_search_weighted: the additive fields summed over the batches, pairs = pseudo-queries x columns; "weighted_pseudo_queries" and "weighted_fold_us"
 *          describe this call too.  "print_gather_us" and "print_h2d_bytes" (read-only): the device time of the call's gather launches, and the bytes it handed to
 *          host-to-device copies (the groups' tables and the fold's); both 0 after a failed or empty call.
 * Not in this interface: the pair and verification forms for prints (afis_score_print_pairs and afis_correspondences_print_pairs below give them, without a matrix);
 *          rolled templates beyond index 0 (the
 *          shard holds one minutiae and one texture template per print); the match CLI.  Shards: a print is a query only on the rank that holds it; against the
 *          other shards its template must be present there, and the existing afis_search_weighted route over host views serves that.  The per-rank lists read from
 *          the matrix are host/sharding.py::merge_hits / merge_subject_hits input as they are.  No result of any other search changes because this function exists.
 * Cost    one MI355X, 100 resident prints (78 minutiae and 811 texture points on average) x 100 000 prints, weights 1 and 0.3f, interleaved runs, medians of three
 *          after a discarded first, spread = max - min (tools/print_search_timing.py, profiles/print_search_timing.json): (a) the call 2 156.2 ms on the host clock
 *          (spread 25.4), device clock 2 152.3 ms (spread 2.4), against 2 163.0 ms (spread 5.8) and 2 154.3 ms (spread 6.3) for afis_search_weighted over host views of
 *          the same prints on the same context — the only route before, the same bits: the device times lie inside each other's spread, the host clock gains 6.9 ms,
 *          about the upload of the views' 34.8 MB that is no longer made (the call hands 9 040 bytes to host-to-device copies).  (b) The gather: 130 us (spread 25)
 *          for 38.1 MB written, three launch groups of seven launches, where a device-to-device copy of 38.1 MB takes 13.1 us (spread 0.7): 9.9 x the copy's time.
 *          It is the launches, not the bytes: the gather of ONE print — seven launches over 0.4 MB — takes 22 us, so 66 of the 130 us are three groups' launch
 *          sequences, and what remains is seven short kernels per group (at most 10 MB each) that end before they reach a byte rate: every thread first walks a
 *          binary search of up to nine dependent loads, and each kernel waits for the previous one's tail.  Store width (16 bytes), occupancy (8 waves per SIMD) and
 *          the codebook reads (cache-resident) are not what limits it; one fused launch per group would be.  Not built: the gather is 0.006 % of the call.
 *          (c) The full search is untouched: tools/lib_ab.py against the parent commit's library, twice, scores bit-identical both times; this tree's median total_ms
 *          1 860.0 against the parent's 1 862.1 (its steps 1 860.6 .. 1 864.4: 0.5 ms BELOW the parent's fastest step) and 1 877.1 against 1 878.2 (inside its
 *          1 876.3 .. 1 880.0) — profiles/print_full_search_ab.txt. */
int afis_search_prints(afis_ctx* ctx, afis_subset* s /* or NULL: the whole resident shard */, const int64_t* idx /*[n_q], GLOBAL*/, int n_q,
                       const float* w_minu /*[n_q]*/, const float* w_tex /*[n_q]*/,
                       float* scores /*[n_q][columns] or NULL*/, int32_t* status /*[n_q] or NULL*/);

/* The rank list of One2List_matching, matcher.cpp:306-309, from a score column (host memory, no device work): idx[0 .. k) / sc[0 .. k) = the k best of scores[0 .. n), descending
 * in afis_search's key rank_key(score) (csrc/rank_order.h: the bits of score + 0.0f in their total order; on a NaN-free column that is score descending).
 * ref_order 0: equal keys by ascending index (what afis_search's own top-k delivers); 1: the reference's statement itself — std::sort of the indices 0 .. n-1 on a non-strict
 * "greater" comparator, with this library's libstdc++ — so that equal scores (the zero scores at the tail of a small gallery's list) come out in the order the reference
 * binary leaves them.  The comparison is rank_key(scores[a]) > rank_key(scores[b]): for every pair of a NaN-free column the outcome of the reference's scores[a] > scores[b],
 * hence the same permutation, and a strict weak order on every column — a NaN score (the reference's own sort is undefined behaviour there) takes the place its key gives
 * it and leaves the other entries in order.  k > n: the rest is padded with idx -1, sc 0.  sc may be NULL. */
int afis_rank_list(const float* scores, int64_t n, int ref_order, int k, int64_t* idx, float* sc);

/* PQ encoder — replaces TrainedPQEncoder.encode_multi (extraction/descriptor_PQ.py:19-27, scipy.cluster.vq.vq per
 * sub-space): codes[i][m] = index of the codeword of sub-quantizer m nearest (squared L2 in fp32 as vq evaluates it,
 * |x|^2 + |c|^2 - 2 x.c; first minimum) to
 * des[i][6m .. 6m+5].  des: [n][96] fp32, codes: [n][16] u8, host pointers.  afis_gallery_add calls it for rolled texture
 * views that carry fp32 descriptors (codes == NULL, des_len == 96). */
int afis_pq_encode(afis_ctx* ctx, const float* des, int64_t n, uint8_t* codes);

/* The rolled branch of descriptor_PQ.py::encode_PQ (:332-349) for one file: `bytes` is a template with fp32 texture
 * descriptors in the latent on-disk layout (descriptor_PQ.py:80-175); the result is the same template in the rolled layout
 * (:178-272), texture descriptors replaced by PQ codes.  out == NULL only reports *out_len.  load_rc: the reader's code. */
int afis_encode_rolled_dat(afis_ctx* ctx, const void* bytes, size_t len, void* out, size_t out_cap, size_t* out_len, int* load_rc);

/* Codebook training — replaces training (extraction/descriptor_PQ.py:41-77: scipy.cluster.vq.kmeans2 per sub-space, minit='points') for the one geometry
 * afis_create accepts, codebook [16][256][6] fp32 over points des [n][96] fp32.  No context: a context needs a codebook; device_id as afis_device_info's, the error text
 * where afis_create's goes (afis_last_error with a NULL context).
 *
 * One Lloyd step is defined bit for bit and independent of the order of its additions, so that the device, a numpy model (tests/pq_train_model.py) and, later, the
 * ranks of a sharded training set agree to the bit.  With C the current codebook, for every point i and sub-quantizer m:
 *   assignment    label[i][m] = the code afis_pq_encode returns for point i under C (the fp32 |x|^2 + |c|^2 - 2 x.c expansion, fma chain over d ascending, first
 *                 strict minimum from +inf: csrc/pq_nearest.h, the one definition the encoder's kernel and the trainer's share)
 *   accumulation  q(x) = (int64) rint((double) x * 2^30), round to nearest even (the widening and the scaling are exact: one rounding); per (m, k) count[m][k] = the
 *                 points with label[i][m] == k and S[m][k][d] = the int64 sum of q(des[i][6m + d]) over them.  Integer addition is associative: atomics,
 *                 per-workgroup partial sums and any tiling give the same words
 *   update        count > 0: C'[m][k][d] = (float)((double) S / ((double) count * 1073741824.0)) — one int64 -> fp64 conversion (nearest even), one IEEE fp64
 *                 division (the divisor is exact), one fp64 -> fp32 rounding, done on the host between steps; count == 0: the codeword keeps its old BITS
 *                 (kmeans2's missing='warn' without the warning)
 *   range         every component of des finite with |x| <= 64 and n <= 2^26 (then |q| <= 2^36 and |S| <= 2^62); init finite.  A violation is AFIS_EINVAL before
 *                 any output is written: des is checked on the device in the first pass over the points.
 * afis_pq_train runs `iters` such steps from init.
 *   codewords  [16][256][6]   the codebook after the last step
 *   counts     [16][256] or NULL : count[m][k] of the last executed assignment (the assignment that produced codewords)
 *   changed    [iters] or NULL   : changed[t] = the (i, m) labels of step t that differ from step t - 1's; changed[0] = 16 n
 *   iters_run  or NULL           : the steps executed.  When changed[t] == 0 for a t >= 1 the codebook is a fixed point — step t + 1 would reproduce step t's labels,
 *                                  sums and codewords — and the call stops after step t: iters_run = t + 1, the remaining changed entries are 0, and every output
 *                                  is what the full run of `iters` steps would have given
 * iters == 0 or n == 0: AFIS_OK without device work, codewords = init's bits, counts 0, changed 0, iters_run 0.  iters outside 0 .. 1000, n < 0 or n > 2^26, a NULL
 * des / init / codewords, a device_id out of range: AFIS_EINVAL; no usable gfx950 device or a failed allocation: AFIS_EDEVICE.  The points stay resident on the device
 * across the steps — 384 n bytes transposed to [16][n][6], 16 n bytes of labels, one upload slice of at most 96 MiB — all allocated before anything is queued; per step
 * only the codebook (96 KB down) and the sums and counts (224 KB up) move.  Every host wait is bounded by AFIS_SEARCH_TIMEOUT_S as a search's is.
 *
 * afis_pq_train_init_points (host only, as afis_rank_list): kmeans2's minit='points' made reproducible.  Per sub-quantizer m it draws 256 DISTINCT point indices and
 * copies those points' sub-vectors: init[m][k] = des[idx(m, k)][6m .. 6m + 5].  The generator is counter-based, splitmix64's output function
 *   mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31   (uint64 arithmetic)
 *   draw(m, j) = mix(mix(seed) + 256 m + j)
 * and the indices are the first 256 steps of a Fisher-Yates shuffle of a = (0, .., n - 1): step j = 0 .. 255 swaps a[j] with a[j + draw(m, j) mod (n - j)], and
 * idx(m, j) is the new a[j] (csrc/pq_train_plan.h).  n < 256 is AFIS_EINVAL (the reference's assert Ks < N).  Distinct points may hold equal values: the later of two
 * equal codewords never wins the first-minimum rule, so its cluster stays empty (and keeps its bits) until its twin has moved — kmeans2 behaves the same way.
 *
 * afis_codebook_write: the bytes afis_create_from_codebook reads — the 3 x int16 header 16, 256, 6 and the 24 576 floats (98 310 bytes); out == NULL only reports
 * *out_len; another geometry or a buffer too small is AFIS_EINVAL.
 *
 * Not in this interface: geometries other than 16 x 256 x 6; k-means++ or any other initialisation (the caller may pass any finite init); a per-rank partial-sum
 * call for sharded training sets (the integer sums make it exact when someone builds it); training from a resident gallery (the shard holds codes, not descriptors).
 *
 * Cost (profiles/pq_train_timing.json, one MI355X; 10^6 clustered points x 20 steps, medians of three interleaved rounds after a discarded first, spread in brackets):
 * the call 40.1 ms on the host's clock (0.8) — the first pass, 384 MB of upload and the transpose, 7.1 ms (0.3), a step 1.283 ms of device time (0.011) — where
 * scipy's kmeans2 per sub-space on the same machine's CPUs, 16 threads, takes 10.9 s for two iterations (108.6 s scaled to twenty).  The step kernel takes 0.98 of
 * the encoder kernel's time at the same n (1.427 ms against 1.450 ms under the profiler): the accumulation costs nothing measurable beside the 256-codeword search.
 * DESIGN section 7, "Codebook training (row 23)", has the kernels and the breakdown. */
int afis_pq_train(int device_id, const float* des /*[n][96]*/, int64_t n, const float* init /*[16][256][6]*/, int iters,
                  float* codewords /*[16][256][6]*/, int64_t* counts /*[16][256] or NULL*/, int64_t* changed /*[iters] or NULL*/, int* iters_run /*or NULL*/);
int afis_pq_train_init_points(const float* des /*[n][96]*/, int64_t n, uint64_t seed, float* init /*[16][256][6]*/);
int afis_codebook_write(const float* codewords, int M, int K, int dsub, void* out, size_t out_cap, size_t* out_len);

/* Correspondence export — replaces One2One_matching_selected_templates(..., save_corr = true, corr_file) as called for the
 * top-24 of One2List_matching (matching/matcher.cpp:321-327, :376-417, :497-505).  For one latent and each of the n listed
 * gallery templates (indices as reported by afis_search, i.e. including index_base) it re-runs the three minutiae scorers and
 * returns the correspondences that survive both graph filters, in the reference's order (corr3):
 *   counts[i*3 + s]                 number of survivors for selected latent template s (0 -> 27th, 1 -> 3rd, 2 -> 12th)
 *   xy[((i*3 + s)*120 + t)*4 + 0..3] latent x, latent y, rolled x, rolled y of survivor t  (one line of <corr_file>_<s>.csv)
 * counts is -1 where the reference does not run that scorer and writes no file (latent empty, rolled empty or without a
 * minutiae template, latent without the selected template), and 0 where it writes an empty file. */
int afis_correspondences(afis_ctx* ctx, const afis_template_view* query, const int64_t* gallery_idx, int n,
                         int32_t* counts /*[n][3]*/, int16_t* xy /*[n][3][120][4]*/);

/* Correspondence export for a whole candidate list: the surviving correspondences of n_pairs (latent, rolled print) pairs in one launch sequence — what an examiner opens
 * after afis_rank_hits, whose flattened idx can be passed as it is.  q is a handle of afis_queries_upload or afis_queries_upload_reserved, typically the one the last
 * search ran on; a handle of ANY gallery epoch is taken (the pairs read the latents' minutiae only; the launch-group cuts play no part).  query[i] is a query position of
 * the handle, idx[i] a global index of the RESIDENT shard as it stands — never a subset's position, and whatever search ran last.  Pairs may come in any order and repeat.
 *   counts[i*3 + s], xy[((i*3 + s)*120 + t)*4 + 0..3]   byte for byte what afis_correspondences(latent query[i], {idx[i]}) returns — AFIS_CORR_NOT_RUN (-1) included, under
 *                                                      every value of "s3_tie_order" / "ref_tie_order"; the xy rows beyond counts are zero
 *   part[i*3 + s]  (part may be NULL)                   the scorer's return value, bit for bit afis_search's parts[q][t][s], where counts >= 0; +0.0f elsewhere
 * An idx outside [index_base, index_base + G) — the -1 that pads the list calls included — gives AFIS_CORR_NOT_COVERED (-2) three times and zeros, silently: the same pair
 * list can go to every rank of a sharded gallery (host/sharding.py::merge_correspondences), as the targets of afis_rank_positions and the exclusion lists can.
 * The call neither writes nor invalidates the last search's matrix: every ranking call may precede and follow it (afis_correspondences, by contrast, stays on the list of
 * calls after which they answer AFIS_ESTATE).  AFIS_EINVAL: a null ctx or q, n_pairs < 0, a null array with n_pairs > 0, a query[i] outside 0 .. n_q - 1; AFIS_ESTATE
 * before the first commit; n_pairs == 0 is AFIS_OK.  Device and pinned room is ensured before anything is queued: AFIS_EDEVICE when that fails, with nothing changed that a caller can see — the caller's arrays and the
 * last search's matrix are untouched; the context's own scratch buffers may have been reallocated, and "correspondences_us" reads 0.
 * Any n_pairs: the list is cut into chunks of at most option "corr_pairs_per_launch" pairs (1 .. 1 048 576; default AFIS_CORR_PAIRS_PER_LAUNCH; about 5.8 KB of device
 * memory per pair — candidates 2880 B, survivors 2880 B, counts, parts — and 2.9 KB pinned); per chunk and launch group of the handle one launch of the any-shape candidate
 * kernel and one of the list kernel, over a device table of the group's pairs, against the resident shard itself.  Option "correspondences_us" (read-only): the device time
 * of the last call's launches (afis_correspondences' too), from HIP events around every chunk's.  Host waits are bounded as a search's are ("search_timeout_s"). */
#define AFIS_CORR_NOT_RUN      -1   /* the reference runs no scorer and writes no file (afis_correspondences' -1) */
#define AFIS_CORR_NOT_COVERED  -2   /* idx is not a template of this shard */
#define AFIS_CORR_PAIRS_PER_LAUNCH 8192
int afis_correspondences_pairs(afis_ctx* ctx, afis_queries* q, int64_t n_pairs,
                               const int32_t* query /*[n_pairs]*/, const int64_t* idx /*[n_pairs], GLOBAL*/,
                               int32_t* counts /*[n_pairs][3]*/, int16_t* xy /*[n_pairs][3][120][4]*/,
                               float* part /*[n_pairs][3] or NULL*/);

/* Pair scoring: the fused score — and on request the four parts — of n_pairs (latent, rolled print) pairs, without scoring a matrix: one verification (1:1), the N labelled
 * mates of a ROC study, the candidates of per-latent lists that came from another rank, an index or a first stage, the parts of a hit list after a search that was run
 * without them.  The arguments follow afis_correspondences_pairs rule for rule: q is a handle of afis_queries_upload or afis_queries_upload_reserved of ANY gallery epoch,
 * query[i] a query position of the handle, idx[i] a global index of the RESIDENT shard as it stands — never a subset's position, whatever search ran last.  Pairs may come
 * in any order and repeat.
 *   a covered pair (index_base <= idx[i] < index_base + G):  status[i] = AFIS_PAIR_OK; score[i] is bit for bit afis_search's scores[query[i]][idx[i] - index_base] — the -1
 *                                                      of an empty or removed print and of a latent-empty query included —, parts[i*4 + 0..3] (parts may be NULL) bit for bit
 *                                                      its parts of that cell (+0.0f four times where the score is that -1: no scorer ran), under every value of
 *                                                      "s3_tie_order" / "ref_tie_order" and "adc_variant" 8 and 9 alike
 *   an uncovered pair (the -1 that pads the list calls included):  status[i] = AFIS_PAIR_NOT_COVERED, score[i] = -inf, parts +0.0f, silently: the same pair list can go to
 *                                                      every rank of a sharded gallery (host/sharding.py::merge_pair_scores)
 * The call neither writes nor invalidates the last search's matrix: every ranking call may precede and follow it.  AFIS_EINVAL: a null ctx or q, n_pairs < 0, a null
 * query, idx, status or score with n_pairs > 0, a query[i] outside 0 .. n_q - 1; AFIS_ESTATE before the first commit; n_pairs == 0 is AFIS_OK.  Device and pinned room is
 * ensured before anything is queued: AFIS_EDEVICE when that fails, with nothing changed that a caller can see — the caller's arrays and the last search's matrix are
 * untouched; the context's own scratch buffers may have been reallocated, and "score_pairs_us" reads 0.
 * Any n_pairs: the pairs that are scored are cut into chunks of at most option "score_pairs_per_launch" pairs (1 .. 1 048 576; default AFIS_SCORE_PAIRS_PER_LAUNCH).  A pair
 * costs about 5.8 KB of device memory for the minutiae stage (candidates 2880 B, a survivor scratch 2880 B, counts, parts, score, the tables' entries) plus lt_pad x 8 bytes
 * for the dense texture row maxima (lt_pad: the longest latent texture template of the handle, at most 1000 rows: 8 KB) — the default keeps a chunk below 113 MB — and 36
 * bytes pinned; beside them the list kernels' slabs for a chunk's launches (60 KB per pair up to 16 384 pairs for the texture lists, 3 x 20 KB up to 10 922 for the
 * minutiae lists).  Per chunk one upload of the tables, then per launch group of the handle the any-shape candidate kernel and the minutiae list kernel over the group's
 * pair table, the exact texture row maxima (k_adc_pairs: a workgroup per 8 latent rows and segment of at most 64 pairs of one latent, the look-up table tile built in LDS),
 * the texture list kernel and the fusion in their pair forms, and one copy back.  Option "score_pairs_us" (read-only): the device time of the last call's launches, from
 * HIP events around every chunk's, summed; 0 when nothing was queued.  Host waits are bounded as a search's are ("search_timeout_s").
 * Cost against the route through a subset (afis_subset_create over the union of the list's prints, afis_search_subset_resident, afis_subset_free), device time on one
 * MI355X, 100 latents x 100 000 prints, interleaved runs (profiles/score_pairs_timing.json): the flattened lists of
 * afis_rank_hits(-inf, 100) — 10 000 pairs, 100 per latent, against a union of 9 511 prints x 100 latents — 26.3 ms against 191.4 ms (7.3 x); one pair per latent — 100
 * pairs against 100 x 100 — 6.2 ms against 12.6 ms (2.0 x); ONE latent against its 4 096 best candidates — where the subset route scores exactly the same 4 096 pairs with
 * the search's tuned kernels — 6.4 ms against 2.8 ms: there the subset is the better call, 2.3 x.  So: latents with candidate lists of their own — the pair call, at 100 pairs
 * per latent and at 1; ONE latent (or latents that share their candidates) with thousands of pairs per latent — afis_subset_create + afis_search_subset_resident.  Per pair
 * the call cost 1.6 - 2.6 us on the two long lists where a subset search cost 0.2 - 0.7 us per cell of its cross product: for lists of thousands of pairs the crossover lies
 * where (latents x union of their prints) is some three to ten times the pair list (an estimate from these figures, not a measurement).  Nothing here is tuned. */
#define AFIS_PAIR_OK           0
#define AFIS_PAIR_NOT_COVERED  1
#define AFIS_SCORE_PAIRS_PER_LAUNCH 8192
int afis_score_pairs(afis_ctx* ctx, afis_queries* q, int64_t n_pairs,
                     const int32_t* query /*[n_pairs]*/, const int64_t* idx /*[n_pairs], GLOBAL*/,
                     int32_t* status /*[n_pairs]*/, float* score /*[n_pairs]*/, float* parts /*[n_pairs][4] or NULL*/);

/* Print pairs (no reference counterpart): the pair forms for RESIDENT PRINT pairs — what afis_score_pairs and afis_correspondences_pairs are for latents, for the
 * queries of afis_search_prints.  Verification (1:1) of two enrolled prints; card against card (ten pairs, finger i against finger i, no 10 x 10 cross product); the
 * second half of the operator's transaction after afis_rank_hits on a print search — the parts behind each score and the surviving correspondences of every (query
 * print, candidate) pair —; labelled print pairs (a ROC over mated and non-mated impressions, a de-duplication audit) without scoring a matrix.
 *   a_idx [n_pairs], b_idx [n_pairs]   the query print and the column print of pair i: GLOBAL indices of the resident shard as it stands (index_base included) — never
 *               a subset's position, whatever search ran last.  Pairs may come in any order and may repeat; a pair (a, a) is an ordinary pair.  No handle is involved:
 *               the calls see the shard as it stands after any edit.
 *   w_minu [n_pairs], w_tex [n_pairs]   afis_score_print_pairs: one weight per PAIR for a's minutiae template and for a's texture template; finite and >= 0 (-0.0f is a
 *               zero), as afis_search_prints': a violation is AFIS_EINVAL before anything is written or queued.
 * Covered     a pair is covered when BOTH indices lie in [index_base, index_base + G) of the resident shard.  Anything else — the -1 that pads the list calls, an
 *               index of another shard, a template staged but not committed — is uncovered, silently: status[i] = AFIS_PAIR_NOT_COVERED, score[i] = -inf, parts +0.0f;
 *               counts[i] = AFIS_CORR_NOT_COVERED, zeros.  This differs on purpose from afis_search_prints, where a query outside the shard is AFIS_EINVAL: the same
 *               pair list can go to every rank of a sharded gallery, and the rank that holds both prints answers it (host/sharding.py::merge_print_pair_scores,
 *               merge_print_correspondences).  A pair whose prints lie in two shards is answered by NO rank: the existing afis_search_weighted route over host views
 *               serves those pairs.
 * Values of afis_score_print_pairs, a covered pair   status[i] = AFIS_PAIR_OK; score[i] is bit for bit the cell afis_search_prints writes for query a, column b and the
 *               weights (w_minu[i], w_tex[i]).  The minutiae term is active when a holds a minutiae template and w_minu[i] != 0.0f, the texture term likewise.  The
 *               score is -1.0f when b is empty or removed, or when nothing of a is active.  Otherwise double acc = +0.0; minutiae active: acc = acc + (double)w_minu *
 *               (double)v_m; then texture active: acc = acc + (double)w_tex * (double)v_t; score = (float)acc — v_m and v_t being the entries afis_match_all_templates
 *               gives the print's view (P of the print-search paragraph) against b; a print b without a minutiae template leaves a zero, and that zero is included.
 *               parts[i*2 + 0..1] (parts may be NULL) = (v_m if active else +0.0f, v_t if active else +0.0f), +0.0f twice where the score is that -1.  All of it under
 *               every value of "s3_tie_order" / "ref_tie_order" and "adc_variant" 8 and 9 alike.
 * Values of afis_correspondences_print_pairs, a covered pair   a or b holds no minutiae template (empty and removed entries included): counts[i] = AFIS_CORR_NOT_RUN,
 *               zeros.  Otherwise counts[i] is the number of survivors of both graph filters, xy[(i*120 + t)*4 + 0..3] a's x, a's y, b's x, b's y of survivor t in the
 *               scorer's order (rows beyond the count zero), and part[i] (part may be NULL) the scorer's return value: bit for bit parts[i*2 + 0] of the score call with
 *               a non-zero w_minu; +0.0f where counts < 0.  Byte for byte these are counts[.][0], xy[.][0] and the part afis_correspondences(_pairs) gives for a latent
 *               view of 27 minutiae templates whose 27th is a's minutiae template as the shard holds it, against b: a scorer's value depends on nothing but its
 *               (latent template, print) pair.
 * State       as afis_score_pairs: the last search's matrix is neither written nor invalidated — every ranking call may precede and follow, and a following
 *               afis_search_resident returns the bytes it returned before.  AFIS_EINVAL: a null ctx, n_pairs < 0, a null required array with n_pairs > 0 (parts and part
 *               may be NULL), a bad weight.  AFIS_ESTATE: a call before the first commit.  n_pairs == 0 is AFIS_OK.  Every batch ensures its room before it queues
 *               anything, and the caller's arrays are written once, after the last batch: a call that fails — AFIS_EDEVICE — has changed nothing a caller can see
 *               (the context's own scratch buffers may have been reallocated).  Host waits are bounded as a search's are ("search_timeout_s").
 * How         the distinct covered query prints that have something a pair wants, in order of first appearance, are cut into batches (csrc/print_pairs_plan.h) of at
 *               most option "print_pairs_batch_prints" prints — 0, the default: as many consecutive prints as an eighth of the launch-group budget holds the views of (392
 *               bytes per minutia and per texture point, 6 144 per fragment tile), and at least one.  Every pair belongs to the batch of its a; results do not depend
 *               on the option.  Per batch a temporary query handle is filled on the device exactly as a batch of afis_search_prints is (a template no pair of a print
 *               weights is not gathered; the correspondence call gathers minutiae only), then the pair drivers of afis_score_pairs / afis_correspondences_pairs run over
 *               the batch's pairs, in chunks of "score_pairs_per_launch" / "corr_pairs_per_launch" pairs, and the handle is freed under afis_queries_free's rules.  The
 *               one device piece of its own is the fold of a print pair (csrc/template_fold.hip::k_fold_print_pairs) in the place of the latent call's fusion.
 *               "print_pairs_us" (read-only): the device time of the last call's launches, gathers included, summed over batches and chunks; "print_pairs_query_prints"
 *               (read-only): the distinct query prints it gathered; both 0 after a call that failed or queued nothing.
 * Cost        one MI355X, 100 000 resident prints, weights 1 and 0.3f, against the only route there was — afis_subset_create over the union of the b's,
 *               afis_search_prints of the distinct a's over it, afis_subset_free —, interleaved runs, medians of three after a discarded first, spread = max - min
 *               (tools/print_pairs_timing.py, profiles/print_pairs_timing.json), the same bits on both routes and in the full print search's cells.  (a) Card against
 *               card, 10 pairs: 0.94 ms on the host clock (spread 0.02), device clock 615 us (spread 7), against 2.16 ms (0.04) and 856 us (9): 2.3 x on the host,
 *               1.4 x on the device.  (b) 100 query prints x their 100 best from afis_rank_hits, 10 000 pairs against a union of 9 507 prints x 100: 31.1 ms (0.1)
 *               and 29.99 ms (0.03) against 217.8 ms (0.5) and 211.4 ms (0.5): 7.0 x.  (c) ONE print against its 4 096 best, where the subset route scores exactly the
 *               same 4 096 cells with the search's tuned kernels: 9.98 ms (0.11) and 9.60 ms (0.06) against 6.77 ms (0.07) and 3.40 ms (0.05) — there the subset is
 *               the better call, 2.8 x on the device clock and 1.5 x on the host's.  afis_correspondences_print_pairs on list (b): 9.65 ms (0.26) and 7.52 ms (0.03);
 *               9 338 of the 10 000 pairs have survivors.  Where the time goes (a kernel trace of all three lists together, a run of its own): of the score calls'
 *               device time k_adc_pairs 50 %, the texture list kernel 21 %, the two minutiae launches 28 %, the gathers about 1 % (5 % of the call on list (a): 31 us
 *               for ten prints; 0.4 % on (b), 0.25 % on (c)) and k_fold_print_pairs 0.07 % (4.6 us a launch).  So: prints with candidate lists of their own — the pair
 *               call; ONE print (or prints that share their candidates) against thousands — afis_subset_create + afis_search_prints.  Nothing here is tuned.  The full
 *               search is untouched: tools/lib_ab.py against the parent commit's library, scores bit-identical, this tree's median total_ms 1 882.6 inside the
 *               parent's steps 1 881.9 .. 1 884.8 (median 1 884.4) — profiles/print_pairs_full_search_ab.txt. */
int afis_score_print_pairs(afis_ctx* ctx, int64_t n_pairs,
                           const int64_t* a_idx /*[n_pairs], GLOBAL: the query print*/, const int64_t* b_idx /*[n_pairs], GLOBAL: the column print*/,
                           const float* w_minu /*[n_pairs]*/, const float* w_tex /*[n_pairs]*/,
                           int32_t* status /*[n_pairs]*/, float* score /*[n_pairs]*/, float* parts /*[n_pairs][2] or NULL*/);
int afis_correspondences_print_pairs(afis_ctx* ctx, int64_t n_pairs,
                                     const int64_t* a_idx, const int64_t* b_idx,
                                     int32_t* counts /*[n_pairs]*/, int16_t* xy /*[n_pairs][120][4]*/, float* part /*[n_pairs] or NULL*/);

/* Texture correspondences (no reference file: matcher.cpp writes none for the texture scorer): the evidence behind the FOURTH part of a fused score, for a list of pairs —
 * which virtual minutiae of the latent the texture scorer matched to which points of the print (S7's 200 best rows after the filters S8b and S9: corr3 of
 * matcher.cpp:767-781).  A latent of a few minutiae often gets most of its score here, and without this call the examiner has nothing to overlay on such a hit.
 * The arguments, AFIS_EINVAL / AFIS_ESTATE / AFIS_EDEVICE, the chunks (option "corr_pairs_per_launch") and the rule that the last search's matrix is neither written
 * nor invalidated follow afis_correspondences_pairs rule for rule; pairs may come in any order and may repeat; pt, sim and part may be NULL.  For pair i:
 *   counts[i]                        the survivors of S9, 0 .. AFIS_TEX_CORR_MAX.  AFIS_CORR_NOT_RUN (-1): the reference does not call the texture scorer — a latent-empty
 *                                    query, an empty or removed print, a latent without a texture template, a print without one (matcher.cpp:411).  AFIS_CORR_NOT_COVERED
 *                                    (-2): idx outside the shard, the -1 that pads the list calls included, silently (host/sharding.py::merge_texture_correspondences)
 *   xy[(i*200 + t)*4 + 0..3]         latent x, latent y, rolled x, rolled y of survivor t in the templates' own BLOCK units, exactly as stored (a pixel is 16 b + 24)
 *   pt[(i*200 + t)*2 + 0..1]         the latent's texture row and the print's texture point, as indices into the templates
 *   sim[i*200 + t]                   the survivor's similarity: the row maximum the list carries, bit for bit
 *   part[i]                          the scorer's return value: bit for bit afis_search's parts[q][t][3] where counts >= 0 — the fp32 sum of sim[i*200 + 0 .. counts) in
 *                                    that order —, +0.0f elsewhere
 * all in the reference's list order under every value of "ref_tie_order"; rows at or beyond counts are zero.
 * The print form takes two RESIDENT prints under afis_correspondences_print_pairs' rules (covered: both in the shard; a pair (a, a) is an ordinary pair); a's texture
 * view is the one afis_search_prints builds, so pt's first component indexes a's texture points; AFIS_CORR_NOT_RUN where a or b holds no texture template.
 * How: the pair driver's score sequence with the texture list kernel's tap after S9 switched on — 1 600 bytes a pair on the device — and one wave per pair behind it
 * (csrc/pair_evidence.hip) that gathers the coordinates; 3 208 bytes a pair return through the pinned buffer, one copy per chunk.  Option "texture_correspondences_us"
 * (read-only): the device time of the last call's launches — the print form's gathers included —, from HIP events around every chunk's, summed; 0 when nothing was queued. */
#define AFIS_TEX_CORR_MAX 200
int afis_texture_correspondences_pairs(afis_ctx* ctx, afis_queries* q, int64_t n_pairs,
                                       const int32_t* query /*[n_pairs]*/, const int64_t* idx /*[n_pairs], GLOBAL*/,
                                       int32_t* counts /*[n_pairs]*/, int16_t* xy /*[n_pairs][200][4]*/,
                                       int16_t* pt /*[n_pairs][200][2] or NULL*/, float* sim /*[n_pairs][200] or NULL*/, float* part /*[n_pairs] or NULL*/);
int afis_texture_correspondences_print_pairs(afis_ctx* ctx, int64_t n_pairs,
                                             const int64_t* a_idx, const int64_t* b_idx,
                                             int32_t* counts /*[n_pairs]*/, int16_t* xy /*[n_pairs][200][4]*/,
                                             int16_t* pt /*[n_pairs][200][2] or NULL*/, float* sim /*[n_pairs][200] or NULL*/, float* part /*[n_pairs] or NULL*/);

/* Pair alignments (no reference counterpart): where the latent lies on the print — the rotation and translation every workstation draws — without pulling the
 * correspondences over the bus.  The device sums, per pair and scorer, the MOMENTS of the surviving correspondences (l, r) in PIXELS — a minutia's coordinates as they are,
 * a texture point's block coordinate b as 16 b + 24 —
 *   n  the survivors;  slx, sly, srx, sry  the coordinate sums;  dot = sum (lx rx + ly ry);  cross = sum (lx ry - ly rx);  ll = sum (lx^2 + ly^2);  rr = sum (rx^2 + ry^2)
 * in exact integer arithmetic (csrc/pair_moments.h, shared by the kernel and the host: with int16 coordinates and at most 560 points in a record the sums stay below
 * 2^29 and the sums of products below 2^50): the order of the additions cannot matter, every field EQUALS the value computed from the exported correspondences, and
 * records add.  A scorer that did not run, or left no survivor, is all zeros.
 *   afis_pair_alignments        arguments and rules as afis_score_pairs; status[i] = AFIS_PAIR_OK or AFIS_PAIR_NOT_COVERED (zeros; host/sharding.py::merge_pair_alignments);
 *                               out[i*4 + 0..2] the minutiae scorers' records (selected templates 27, 3, 12), out[i*4 + 3] the texture scorer's.  288 bytes a pair
 *                               return instead of the 2.9 KB + 3.2 KB of the two correspondence calls
 *   afis_print_pair_alignments  arguments and rules as afis_correspondences_print_pairs; out[i*2 + 0] a's minutiae template against b, out[i*2 + 1] a's texture template
 *   afis_corr_moments_add       host only: acc += other, field by field — pools scorers (all four into one placement), exactly.  AFIS_EINVAL, acc unchanged: a null
 *                               pointer, an operand or a sum outside the bound above (n beyond 560 included)
 *   afis_alignment_fit          host only: the rigid least-squares placement r ~ R l + t, R = [[c, -s], [s, c]], of one record.  P = n dot - (slx srx + sly sry) and
 *                               Q = n cross - (slx sry - sly srx) exactly (128-bit integers); p, q their correctly rounded doubles; h = sqrt(p p + q q); c = p / h;
 *                               s = q / h; tx = (srx - (c slx - s sly)) / n; ty = (sry - (s slx + c sly)) / n; with the exact integers U = n ll - slx^2 - sly^2 and
 *                               V = n rr - srx^2 - sry^2, rms = sqrt(max(0, double(U + V) - 2 h)) / n, the root mean square residual in pixels.  Every operation is one
 *                               correctly rounded fp64 operation, no fused multiply-add.  AFIS_EINVAL with the outputs untouched: a null record, one outside the bound,
 *                               n < 2, or P = Q = 0 (no rotation is determined).  Every output may be NULL
 * The device calls chunk by "corr_pairs_per_launch" and neither write nor invalidate the last search's matrix.  Option "pair_alignments_us" (read-only): the device time
 * of the last call's launches (the print form's gathers included), summed over the chunks; 0 when nothing was queued.
 * Cost        one MI355X, 100 latents x their 100 best candidates — the flattened lists of afis_rank_hits(-inf, 100), 10 000 pairs — of a 100 000-print planted gallery,
 *               the routes interleaved on one context, medians of five after a discarded first, spread = max - min (tools/pair_evidence_timing.py,
 *               profiles/pair_evidence_timing.json).  afis_pair_alignments: 26.4 ms on the device clock (spread 0.4) and 27.1 ms on the host's (0.5), 2.9 MB returned.
 *               afis_texture_correspondences_pairs with pt, sim and part: 26.4 ms (0.2) and 29.2 ms (0.3), 32 MB.  The route there was for the same moments —
 *               afis_correspondences_pairs (6.8 ms on the device, 9.2 ms on the host), plus the texture export, plus the moments of the four lists in numpy (106 ms,
 *               spread 1.6) —: 33.1 ms (0.1) of device time and 144.4 ms (1.5) on the host, 61 MB.  So the alignment call takes 0.80 x the device time of the two
 *               exports — both routes run the same four scorers, whose exact texture row maxima and list kernels are nearly all of either; the copy back is not on
 *               the device clock — and 0.19 x the host time of that route as measured, most of which is the numpy pass: against the two C calls alone (38.2 ms) it
 *               is 0.71 x.  The records equalled the numpy moments of the exports; 8 594 .. 8 796 of the 10 000 records of a scorer held survivors; afis_rank_hits
 *               returned afterwards what it had returned before.  Nothing here is tuned. */
typedef struct { int64_t n, slx, sly, srx, sry, dot, cross, ll, rr; } afis_corr_moments;  /* 72 bytes */
int afis_pair_alignments(afis_ctx* ctx, afis_queries* q, int64_t n_pairs,
                         const int32_t* query /*[n_pairs]*/, const int64_t* idx /*[n_pairs], GLOBAL*/,
                         int32_t* status /*[n_pairs]*/, afis_corr_moments* out /*[n_pairs][4]*/);
int afis_print_pair_alignments(afis_ctx* ctx, int64_t n_pairs,
                               const int64_t* a_idx, const int64_t* b_idx,
                               int32_t* status /*[n_pairs]*/, afis_corr_moments* out /*[n_pairs][2]*/);
int afis_corr_moments_add(afis_corr_moments* acc, const afis_corr_moments* other);
int afis_alignment_fit(const afis_corr_moments* m, double* c, double* s, double* tx, double* ty, double* rms);

/* Cascade search (no reference counterpart): a cheap first stage in front of the expensive one.  afis_search scores every (latent, print) cell with all four scorers, and
 * about 60 % of its device time is the texture path, spent on cells of which a handful per latent ever reach an examiner.  afis_search_cascade runs the
 * three MINUTIAE scorers for every cell of the resident shard, keeps per latent the `keep` best prints by that partial score — selected on the device — and runs the
 * TEXTURE scorer for the kept cells only.  No host round trip lies between the stages; there is one wait at the end.
 * Handle   q is a handle as afis_search_resident takes it, under that call's epoch rules: a handle from before a gallery edit is AFIS_ESTATE, a reserved handle
 *          (afis_queries_upload_reserved) is accepted while the shard fits.  The columns are the whole resident shard.
 * keep     1 <= keep <= AFIS_HITS_MAX, anything else is AFIS_EINVAL; n_kept[q] = min(keep, G).
 * Stage-1 value m(q, t)   the fusion of afis_search (csrc/fuse_cell.h: the one definition of the expression) with the texture score taken as +0.0f: -1.0f for an empty
 *          or removed print or a latent-empty query, otherwise (a0 + a1) + a2 in fp32, where a_s = +0.0f if the latent's texture slot is s, else parts[s].  The
 *          texture's slot rule for latents with fewer than three minutiae templates stays in force: the slot the texture would occupy contributes zero.
 * Selection   per query the kept columns are the first n_kept entries of the list afis_rank_hits(min_score = -INFINITY, cap = keep) would give on the matrix of m: rank_key
 *          descending, equal keys by ascending GLOBAL index (csrc/rank_order.h).  Every column is an entry; the -1 cells stand last and are kept only when keep exceeds
 *          the non-empty prints.  kept_idx[q] is that list (global indices, index_base included), padded with -1.
 * Values   a kept cell holds, bit for bit, afis_search's scores[q][t], and kept_parts holds that cell's four parts (+0.0f four times where the score is the -1; +0.0f
 *          in the padding), in kept_idx order — under every value of "s3_tie_order" / "ref_tie_order" and "adc_variant" 8 and 9 alike.  Every other cell holds the word
 *          0xffffffff, the "no entry" word (csrc/score_order.h: kNoEntryWord), in the matrix left on the device and in scores [n_q][G] (NULL: not copied).  status
 *          [n_q] (or NULL) is afis_search's.  n_kept, kept_idx and kept_parts may each be NULL.
 * The matrix afterwards   after AFIS_OK the context's last-search matrix is this [n_q][G] matrix: a full search's record under afis_search's invalidation rules; the
 *          call is one of the searches that count.  It reads as afis_search_eligible's matrix reads: afis_rank_hits, afis_rank_subject_hits, afis_rank_latent_hits,
 *          their _filtered forms, and afis_rank_positions / afis_rank_subject_positions / afis_count_before see the kept cells as the only entries; the CASE lists
 *          must be read through their _filtered forms; afis_rank_subjects is not in this interface.  A mate that stage 1 dropped is AFIS_POS_NO_ENTRY in
 *          afis_rank_positions: that is how a caller measures what a given keep costs in accuracy.  After any return other than AFIS_OK the matrix is invalid and the
 *          call holds nothing it allocated.  A following afis_search_resident on the same context returns the bytes it returned before the cascade call.
 * Arguments   AFIS_EINVAL: a null ctx or q, keep out of range; AFIS_ESTATE: a call before the first commit, a stale handle.  n_q == 0 or G == 0 returns AFIS_OK as
 *          afis_search does (n_kept 0, kept_idx -1).  Room — the two matrices, the per-part scores of all queries [n_q][G][4], the minutiae stage's buffers for the
 *          largest launch group, the kept lists and pair tables, one chunk's dense row maxima and the texture list kernel's slab — is ensured before anything is
 *          queued: AFIS_EDEVICE otherwise.  Host waits are bounded by "search_timeout_s".
 * Options  "cascade_pairs_per_launch" (settable, 1 .. 1 048 576; default AFIS_CASCADE_PAIRS_PER_LAUNCH): the pairs of one chunk of the second stage at most; results do
 *          not depend on it.  "cascade_stage1_us", "cascade_select_us", "cascade_stage2_us" (read-only): the device time of the last call's three parts, each from its
 *          own pair of HIP events; "cascade_kept_pairs" (read-only): the pairs its second stage scored.  All four read 0 after a call that failed or was empty.
 * Timing   afis_get_timing* reports stage 1: cands_ms, minu_graph_ms, minu_ms, fuse_ms (k_fuse_stage1), total_ms their sum, pairs = n_q x G, launch_groups and the
 *          minutiae task counters; the texture fields are 0.
 * How      csrc/afis_cascade.cpp.  Stage 1 is the minutiae stage of a search, per launch group of the handle on the context's stream, unconfined (no CU-masked side
 *          streams); k_fuse_stage1 writes m.  The selection is k_rank_hits, unchanged.  The structure of the second stage's pair tables is known before anything runs
 *          (csrc/cascade_tables.h) and uploaded once; k_cascade_gather (csrc/cascade.hip) fills them from the kept lists; per chunk and launch group the pair kernels
 *          of afis_score_pairs (k_adc_pairs, k_graph_texture in its pair form, k_fuse_pairs); k_cascade_scatter writes the combined matrix, which was filled with the
 *          no-entry word first, so every matrix word is written at most twice.
 * Cost     against the full search — afis_search_resident(k = 0) on the same context — on one MI355X, 100 latents x 100 000 prints, interleaved runs, medians of three
 *          after a discarded first, device clock (profiles/cascade_search_timing.json, tools/cascade_search_timing.py; the host clock agrees within 0.5 ms).  Headline
 *          workload: keep 100 — 819.3 ms (stage 1 801.0, selection 0.29, stage 2 18.1) against 1 875.8 ms: 0.44 x; keep 1000 — 923.9 ms (803.6 / 0.30 / 120.6)
 *          against 1 881.8 ms: 0.49 x; keep 4096 — 1 237.9 ms (801.1 / 0.33 / 436.5) against 1 879.3 ms: 0.66 x.  Structured workload: keep 100 — 853.8 ms (839.3 / 0.29 / 14.3) against
 *          2 220.5 ms: 0.38 x; keep 1000 — 937.1 ms (840.5 / 0.31 / 96.4) against 2 226.2 ms: 0.42 x; keep 4096 — 1 200.6 ms (840.5 / 0.34 / 359.8) against
 *          2 223.8 ms: 0.54 x.  Spreads (max - min) at most 3.3 ms for the cascade, 5.3 ms for the full search.
 *          Stage 1 alone is 0.43 of the full step on the headline workload (cands_ms 380, minu_graph_ms 421) and 0.38 on the structured one (389, 451): the two
 *          minutiae kernels back to back on the whole chip.  Stage 2 costs 0.9 - 1.8 us per pair and at keep 4096 is a third of the call: k_adc_pairs is untuned
 *          (its comment says where to look first) — the follow-up.
 *          What keep costs in accuracy, on these SYNTHETIC galleries (facts about the generator, not about fingerprints; read through afis_rank_positions on both
 *          matrices): of the 400 planted mates of either workload every one is kept at keep 100, 1000 and 4096, and the 100 that stand at rank 1 under afis_search
 *          still stand at rank 1.  The generator's non-mates score next to nothing with the minutiae scorers, so these shares say little about real prints.
 * Shards: every rank keeps `keep` of its OWN shard.  The per-rank lists are host/sharding.py::merge_hits / merge_subject_hits input as they are; their union contains
 *          the global stage-1 top `keep`, so the merged result is a superset of the single-context cascade, not the same list.
 * Not in this interface: a keep above AFIS_HITS_MAX; a first stage other than the minutiae scorers; the match CLI.  What this list used to name as missing is below:
 *          a subset form is afis_search_cascade_subset; a host-view form is afis_search_cascade_eligible (a zero mask triple passes every template).  No result of
 *          afis_search changes because this function exists. */
#define AFIS_CASCADE_PAIRS_PER_LAUNCH 16384
int afis_search_cascade(afis_ctx* ctx, afis_queries* q, int keep,
                        float* scores /*[n_q][G] or NULL*/, int32_t* status /*[n_q] or NULL*/,
                        int64_t* n_kept /*[n_q] or NULL*/,
                        int64_t* kept_idx /*[n_q][keep] or NULL*/, float* kept_parts /*[n_q][keep][4] or NULL*/);

/* Cascade search over a part of the shard (no reference counterpart).  A latent that may only come from some fingers pays, under afis_search_cascade, for stage 1 on
 * every cell, and its `keep` slots go to the best of ALL columns: the ranking call's masks then drop most of them.  The two calls below run the cascade over the columns
 * that matter only — stage 1, the selection and the texture scorer.
 *
 * afis_search_cascade_subset is afis_search_cascade with the columns of a live subset (afis_subset_create).
 * Handles  afis_search_subset_resident's rules: s a live subset of this context (else AFIS_EINVAL) created in the current gallery epoch (else AFIS_ESTATE); q under that
 *          call's handle rules — a handle of the current epoch, or a reserved one (afis_queries_upload_reserved) while the subset's size n fits it.
 * keep     1 <= keep <= AFIS_HITS_MAX, anything else is AFIS_EINVAL; n_kept[q] = min(keep, n).
 * Stage-1 value and selection   afis_search_cascade's, sentence for sentence, over the listed templates: rank_key of m descending, equal keys by ascending GLOBAL index
 *          whatever order the subset's list had.  kept_idx holds global indices, padded with -1.
 * Values   a kept cell holds, bit for bit, the word afis_search_subset_resident writes at (q, column j), kept_parts its four parts (+0.0f four times where the score is
 *          the -1, and in the padding); every other cell the no-entry word 0xffffffff.  Column j of scores [n_q][n] belongs to idx[j], the caller's order.  status is
 *          afis_search's.  Under every value of "s3_tie_order" / "ref_tie_order" and "adc_variant" 8 and 9.
 * The matrix afterwards   a subset search's record of n_q queries over s, held on the device as every subset search holds it; the call is one of the searches that
 *          count.  The ranking family reads it exactly as it reads afis_search_cascade's matrix, naming templates by global index: the kept cells are the only entries,
 *          the case lists go through their _filtered forms, afis_rank_subjects is not in this interface.  After any return other than AFIS_OK the matrix is invalid and
 *          the call holds nothing it allocated.
 * Arguments   n == 0 or n_q == 0 returns AFIS_OK as afis_search_cascade answers G == 0 (n_kept 0, kept_idx -1, kept_parts +0.0f).  Room is ensured before anything is
 *          queued; host waits are bounded by "search_timeout_s".  Options and timing are afis_search_cascade's ("cascade_*"; pairs = n_q x n).
 *
 * afis_search_cascade_eligible takes afis_search_eligible's arguments, and refuses what it refuses, plus keep: labels and masks are both required, a labels handle that
 * is not live is AFIS_EINVAL, one from an older gallery epoch AFIS_ESTATE, keep outside 1 .. AFIS_HITS_MAX AFIS_EINVAL.
 * Eligibility   E(q) = the resident templates whose label passes masks[q] — the label test of the filtered hit lists, word for word.  The result is what
 *          afis_search_cascade would give latent q on a shard that held only E(q), at their own global indices.
 * Values   n_kept[q] = min(keep, |E(q)|).  The kept columns are the first n_kept[q] entries of the list afis_rank_hits_filtered(labels, masks, min_score = -INFINITY,
 *          cap = keep) would give on the stage-1 matrix m.  A kept cell is bit for bit afis_search's scores[q][t], kept_parts its parts (+0.0f four times where the
 *          score is the -1, and in the padding).  Every other cell of the [n_q][G] matrix — eligible but dropped, or not eligible — is the no-entry word.  A latent-empty
 *          query keeps its first min(keep, |E(q)|) eligible columns by index at -1.  |E(q)| == 0: n_kept 0, a row of no-entry words, the status a search would report.
 *          status is afis_search's.  Under every value of "s3_tie_order" / "ref_tie_order" and "adc_variant" 8 and 9.
 * The matrix afterwards   a full search's record [n_q][G], as after afis_search_eligible; the call is one of the searches that count.  After any return other than
 *          AFIS_OK the matrix is invalid and the call holds nothing it allocated; a following afis_search_resident or afis_search_eligible returns the bytes it
 *          returned before.  Exclusion lists stay a matter of the ranking call, as they are for afis_search_eligible: an excluded print may take a kept slot.
 * How      csrc/afis_cascade_eligible.cpp.  The latents are grouped into classes of identical mask triples; per class one temporary sub-shard of the class's eligible
 *          templates (gathered on the device, class after class into the same buffers; "subset_device_bytes", "gallery_h2d_bytes" and "subset_gather_us" read as
 *          before), the class's latents uploaded, one cascade over the sub-shard.  k_cascade_gather_mapped / k_cascade_scatter_mapped (csrc/cascade_mapped.hip) go from a kept
 *          global index to the sub-shard's position and write the kept cell straight into the combined matrix, which is filled with the no-entry word once per call.
 *          A class whose masks pass every template runs on the resident shard itself; a class nothing passes scores nothing.  Room for a class is ensured before that
 *          class queues anything; host waits are bounded by "search_timeout_s".
 * Options  "cascade_stage1_us", "cascade_select_us", "cascade_stage2_us", "cascade_kept_pairs": the sums over the classes; "eligible_classes": the classes.
 *          afis_get_timing* adds the classes' stage-1 figures up (pairs = the cells stage 1 scored).
 * Cost     about (eligible share) x afis_search_cascade's time, plus a fixed cost per class.  Measured on one MI355X, 100 latents x 100 000 prints, labels = ten one-hot
 *          finger classes, interleaved with the two routes that existed before on the same context, medians of three after a discarded first, HOST clock around the C
 *          calls (profiles/cascade_eligible_timing.json, tools/cascade_eligible_timing.py; device clock in brackets: the "cascade_*" options, afis_timing.total_ms).
 *          Every latent one finger (ten classes of ten latents, 10 000 columns each), headline workload: keep 100 — 171.5 ms (117.1: stage 1 91.6, selection 0.35,
 *          stage 2 25.2) against 285.4 ms (230.5) for afis_search_eligible and 823.2 ms for afis_search_cascade + afis_rank_hits_filtered: 0.60 x / 0.21 x; keep 1000 —
 *          261.0 ms (206.2) against 285.9 and 924.6 ms: 0.91 x / 0.28 x.  Structured workload: keep 100 — 171.8 ms (118.9) against 320.5 and 852.4 ms: 0.54 x / 0.20 x;
 *          keep 1000 — 255.7 ms (202.5) against 319.9 and 933.8 ms: 0.80 x / 0.27 x.
 *          Every latent the same two fingers (one class of 20 000 columns), headline: keep 100 — 191.8 ms (177.6: 163.2 / 0.05 / 14.4) against 392.0 and 823.9 ms:
 *          0.49 x / 0.23 x; keep 1000 — 292.0 ms (277.6) against 392.1 and 925.3 ms: 0.74 x / 0.32 x.  Structured: keep 100 — 204.2 ms (183.8) against 467.1 and
 *          852.9 ms: 0.44 x / 0.24 x; keep 1000 — 286.9 ms (266.4) against 466.7 and 935.4 ms: 0.61 x / 0.31 x.  Spreads (max - min) at most 8.2 ms.
 *          The fixed cost per class — the sub-shard's gather, the class's query upload, its wait: what the host clock holds beyond the device clock, per class —
 *            5.3 - 5.5 ms for a class of 10 latents x 10 000 columns, 14 - 21 ms for the class of 100 latents x 20 000 columns.
 *            afis_search_eligible pays the same per class (its host clock exceeds its device clock by 5.5 and 14 ms per class on the same headline runs).
 *          It decides where the call stops paying.  Against afis_search_cascade + filter a class saves stage 1 on the cells it does not score, 0.09 us per cell
 *          (91.6 ms for 10^6 cells), and pays the fixed cost: a class of n_c latents over m of G columns pays from about n_c x (G - m) > 60 000 cells on — ten latents
 *          that exclude 6 000 prints; one latent alone only in a shard where it excludes 60 000.  Against afis_search_eligible the fixed cost is the same and the
 *          question is stage 2: a kept pair costs 1.2 - 2.5 us where the texture path of a search costs 0.14 us per cell, so the call pays while keep stays below about
 *          a tenth of the class's columns (0.91 x at keep 1000 of 10 000, where stage 2's 115.1 ms already outweigh stage 1's 90.8 ms).
 *          What the routes list, on these SYNTHETIC galleries (facts about the generator, not about fingerprints; through afis_rank_positions on each route's
 *          matrix): of the 29 (one finger) and 76 (two fingers) eligible planted mates every route lists all, 27 and 54 of them at rank 1, at both keeps and on both
 *          workloads.  The generator's non-mates score next to nothing with the minutiae scorers, so afis_search_cascade's global keep loses no planted mate here; on
 *          real prints its `keep` slots go to all fingers, which is what this call is for.  The full search is untouched: bit-identical scores and a median total_ms
 *          within 0.2 % of the parent commit's library, of either sign over two runs (profiles/cascade_eligible_full_search_ab.txt).
 * Shards: no new merge.  Every rank keeps `keep` of its own shard's eligible prints; the per-rank lists are host/sharding.py::merge_hits input as they are, a superset
 *          of the single-context result.
 * Not in this interface: a subset or eligible form of afis_search_prints_cascade; exclusion lists applied before the selection; a keep above AFIS_HITS_MAX. */
int afis_search_cascade_subset(afis_ctx* ctx, afis_subset* s, afis_queries* q, int keep,
                               float* scores /*[n_q][n] or NULL*/, int32_t* status /*[n_q] or NULL*/,
                               int64_t* n_kept /*[n_q] or NULL*/,
                               int64_t* kept_idx /*[n_q][keep] or NULL, global indices*/, float* kept_parts /*[n_q][keep][4] or NULL*/);
int afis_search_cascade_eligible(afis_ctx* ctx, afis_labels* labels, const uint64_t* masks /*[n_q][3]*/,
                                 const afis_template_view* queries, int n_q, int keep,
                                 float* scores /*[n_q][G] or NULL*/, int32_t* status /*[n_q] or NULL*/,
                                 int64_t* n_kept /*[n_q] or NULL*/,
                                 int64_t* kept_idx /*[n_q][keep] or NULL, global indices*/, float* kept_parts /*[n_q][keep][4] or NULL*/);

/* Print cascade (no reference counterpart): the duplicate check of an enrolment with the texture scorer for the best `keep` columns only.  afis_search_prints pays the
 * full price of a search for every query print, and nearly all of it is the texture path: a print's view carries about 811 decoded texture rows, more than a latent's.
 * Rolled against rolled the minutiae scorer is the strong one, and a print's view has ONE minutiae template: afis_search_prints_cascade runs that one scorer for every
 * (query print, column print) cell of the resident shard, keeps per query the `keep` best columns by that partial score — selected on the device — and runs the texture
 * scorer for the kept cells only.  The columns are the whole resident shard as it stands; no handle is involved, the call is valid after any gallery edit.
 *   idx [n_q], w_minu [n_q], w_tex [n_q]   as afis_search_prints', rule for rule: GLOBAL indices (index_base included) in any order, entries may repeat; one weight per
 *          query for the print's minutiae template and for its texture template, finite and >= 0.  The minutiae term of query q is ACTIVE when the print holds a
 *          minutiae template and w_minu[q] != 0.0f, the texture term likewise.
 * keep     1 <= keep <= AFIS_HITS_MAX, anything else is AFIS_EINVAL; n_kept[q] = min(keep, G).
 * Stage-1 value m(q, t)   the word afis_search_prints writes at (q, t) for the weights (w_minu[q], +0.0f): -1.0f for an empty or removed column; -1.0f for the WHOLE
 *          ROW when the minutiae term of query q is not active — a print without a minutiae template, an empty or removed print, w_minu[q] == 0 —; otherwise
 *          (float)(+0.0 + (double)w_minu[q] * (double)v_m).  There is no special case: a row that stage 1 cannot rank is a row of equal keys and keeps its first
 *          min(keep, G) columns by index.  Such a query belongs to afis_search_prints, not here.
 * Selection   the rule of afis_search_cascade: per query the kept columns are the first n_kept entries of the list afis_rank_hits(min_score = -INFINITY, cap = keep)
 *          would give on the matrix of m: rank_key descending, equal keys by ascending GLOBAL index (csrc/rank_order.h).  Every column is an entry; the -1 cells stand
 *          last.  kept_idx[q] is that list (global indices, index_base included), padded with -1.
 * Values   a kept cell holds, bit for bit, the word afis_search_prints writes at (q, t) for the weights (w_minu[q], w_tex[q]); every other cell holds the word
 *          0xffffffff, the "no entry" word (csrc/score_order.h: kNoEntryWord), in the matrix left on the device and in scores [n_q][G] (NULL: not copied).
 *          kept_parts[q][r][0..1] are the parts afis_score_print_pairs defines for the pair (idx[q], kept_idx[q][r]) with those weights: (v_m if the minutiae term is
 *          active else +0.0f, v_t if the texture term is active else +0.0f); +0.0f twice where the cell is the -1, and in the padding.  status [n_q] (or NULL) is
 *          afis_search_prints' for the real weights: AFIS_QUERY_LATENT_EMPTY where nothing is active.  n_kept, kept_idx and kept_parts may each be NULL.  All of it
 *          under every value of "s3_tie_order" / "ref_tie_order" and "adc_variant" 8 and 9 alike.
 * The matrix afterwards   after AFIS_OK the context's last-search matrix is this [n_q][G] matrix: a full search's record under afis_search's invalidation rules; the
 *          call is one of the searches that count, for every ranking call.  It reads as afis_search_cascade's matrix reads: the hit lists, subject hit lists, column
 *          lists, their _filtered forms and the position calls see the kept cells as the only entries (a mate that stage 1 dropped is AFIS_POS_NO_ENTRY); the CASE
 *          lists must be read through their _filtered forms; afis_rank_subjects is not in this interface.  A print against itself is an ordinary kept cell: the
 *          caller takes it out with an exclusion list.  After any return other than AFIS_OK the matrix is invalid and the call holds nothing it allocated.  A
 *          following afis_search_prints on the same context returns the bytes it returned before.
 * Arguments   AFIS_EINVAL: a null ctx, n_q < 0, a null idx or weight array with n_q > 0, an index outside the resident shard, a weight that is NaN, infinite or
 *          negative, keep out of range, n_q x keep or n_q x G beyond what afis_search_cascade takes.  AFIS_ESTATE: a call before the first commit, an index that is
 *          staged but not committed.  n_q == 0 or G == 0 returns AFIS_OK as afis_search_cascade does (n_kept 0, kept_idx -1, kept_parts +0.0f).  Room — the two
 *          matrices, the per-part scores of all pseudo-queries [n_pseudo][G][4], the minutiae stage's buffers for the largest launch group, the kept lists and pair
 *          tables, one chunk's dense row maxima and the texture list kernel's slab — is ensured before anything of the cascade is queued: AFIS_EDEVICE otherwise.
 *          Host waits are bounded by "search_timeout_s".
 * Options  "cascade_pairs_per_launch" applies to this call too; results do not depend on it.  "print_cascade_stage1_us", "print_cascade_select_us",
 *          "print_cascade_stage2_us" (read-only): the device time of the last call's three parts, each from its own pair of HIP events; "print_cascade_kept_pairs"
 *          (read-only): the pairs its second stage scored.  All four read 0 after a call that failed or was empty.  "print_gather_us" and "print_h2d_bytes" describe
 *          this call as they describe afis_search_prints (the bytes: the launch groups' tables and the cascade's).
 * Timing   afis_get_timing* reports stage 1 as the latent cascade does: cands_ms, minu_graph_ms, minu_ms, fuse_ms (k_print_cascade_stage1), total_ms their sum, pairs
 *          = pseudo-queries x G, launch_groups and the minutiae task counters; the texture fields are 0.
 * How      csrc/afis_print_cascade.cpp.  One pseudo-query per print with something active, in ONE temporary query handle built as a batch of afis_search_prints is
 *          (the texture view is gathered only where the texture term is active), which has its own bounded wait; after it the cascade is one launch sequence with one
 *          wait.  Stage 1 is the minutiae stage of a search, per launch group on the context's stream, unconfined; k_print_cascade_stage1 (csrc/print_cascade.hip)
 *          writes m from slot 0 of the pseudo-queries' parts.  The selection is k_rank_hits, unchanged.  The second stage's pair tables (csrc/cascade_tables.h, a
 *          query having pairs when its texture term is active) are uploaded once; k_print_cascade_gather fills them from the kept lists; per chunk and launch group
 *          k_adc_pairs and k_graph_texture in its pair form; k_print_cascade_finish folds v_m and v_t of every kept cell in fp64 — csrc/print_fold.h, the expression
 *          of k_fold_templates and k_fold_print_pairs — into the combined matrix, which was filled with the no-entry word first.
 * Cost     against the full print search — afis_search_prints on the same context, the only route before — on one MI355X, 100 resident prints (of each of 100 synthetic
 *          latents the first planted mate) x 100 000 prints, weights 1 and 0.3f, interleaved runs, medians of three after a discarded first, device clock
 *          (profiles/print_cascade_timing.json, tools/print_cascade_timing.py; the host clock, which includes both calls' temporary handles, agrees within 1.5 ms).
 *          Headline workload: keep 100 — 669.8 ms (stage 1 650.5, selection 0.28, stage 2 19.0) against 2 183.7 ms: 0.31 x; keep 1000 — 783.9 ms (651.1 / 0.30 /
 *          132.3) against 2 181.1 ms: 0.36 x; keep 4096 — 1 159.9 ms (650.6 / 0.33 / 508.8) against 2 182.6 ms: 0.53 x.  Structured workload: keep 100 — 676.5 ms
 *          (659.8 / 0.29 / 16.4) against 2 403.6 ms: 0.28 x; keep 1000 — 774.1 ms (659.0 / 0.30 / 114.8) against 2 409.5 ms: 0.32 x; keep 4096 — 1 098.0 ms (659.5 /
 *          0.33 / 438.0) against 2 401.6 ms: 0.46 x.  Spreads (max - min) at most 1.9 ms for the cascade, 5.7 ms for the full print search; the gather of the handle
 *          0.10 ms.  Every kept cell bit-equal to the full print search's.
 *          The estimate this call was proposed with — stage 1 a third of the latent cascade's 801 ms, the whole call 0.15 x at keep 100 — did NOT hold: stage 1 alone
 *          is 0.30 of the full print search on the headline workload (cands_ms 272, minu_graph_ms 378) and 0.27 on the structured one (274, 385), 0.81 of the latent
 *          cascade's first stage.  A print's view has one minutiae template where a latent has three, but that template holds about 80 minutiae where each of the
 *          latent's holds 20 - 60: by the generator's sizes the candidate kernel's similarity cells drop by a third, not by two thirds (cands_ms 272 against the
 *          latent cascade's 380), and the list kernel's time hardly moves (378 ms against 421).  Stage 2 costs 1.1 - 1.9 us per pair and at keep 4096 is 0.40 -
 *          0.44 of the call: k_adc_pairs is untuned, as the latent cascade's paragraph says.  Nothing here is tuned.
 *          What keep costs in accuracy, on these SYNTHETIC galleries (facts about the generator, not about fingerprints; read through afis_rank_positions on both
 *          matrices with the query's own print excluded): the print mates are the other three planted mates of the query's latent, 300 per workload.  Headline: all
 *          300 are kept at keep 100, 1000 and 4096.  Structured: 297 are kept at keep 100, 298 at keep 1000 and at 4096 (why the last two are dropped was not
 *          examined).  On both workloads the 100 mates that stand at rank 1 under afis_search_prints still stand at rank 1 at every keep.  The generator's non-mates
 *          score next to nothing with the minutiae scorer, so these counts say little about real prints.
 *          The full search is untouched: tools/lib_ab.py against the parent commit's library, scores bit-identical, this tree's median total_ms 1 880.9 inside the
 *          parent's steps 1 879.4 .. 1 886.0 (median 1 879.7) — profiles/print_cascade_full_search_ab.txt.
 * Shards: a print is a query only on the rank that holds it, and every rank keeps `keep` of its OWN shard: the merged lists are a superset of the single-context
 *          result, as for afis_search_cascade.
 * Not in this interface: a subset form (the kept lists are global: put a finger restriction on the ranking call, with masks); a keep above AFIS_HITS_MAX; batching over
 *          queries (everything for all n_q queries is resident at once); the match CLI.  No result of any other search changes because this function exists. */
int afis_search_prints_cascade(afis_ctx* ctx, const int64_t* idx /*[n_q], GLOBAL*/, int n_q,
                               const float* w_minu /*[n_q]*/, const float* w_tex /*[n_q]*/, int keep,
                               float* scores /*[n_q][G] or NULL*/, int32_t* status /*[n_q] or NULL*/,
                               int64_t* n_kept /*[n_q] or NULL*/, int64_t* kept_idx /*[n_q][keep] or NULL*/,
                               float* kept_parts /*[n_q][keep][2] or NULL*/);

/* Kept matrices: the last search's matrix as an object — kept, read, recalled and fused on the device.
 * Why      every ranking and analysis call reads THE LAST search's matrix, the next search overwrites it and the normalisation rewrites it.  The raw lists after a
 *          z-normalisation, a normalisation along the other axis, the mean of two normalisations (S-norm), a symmetric print score (a -> b fused with b -> a) and
 *          the fusion of two searches of the same latents over the same columns each cost a second full search, or [n_q][columns] floats over the bus and back.
 * What     a handle holds a device copy of a matrix with its RECORD: n_q, columns, the subset it was scored over (or the whole shard), the gallery epoch and the
 *          normalised mark.  Kept matrices are plain allocations, as subsets are: option "matrix_device_bytes" (read-only) is what the live ones hold.
 *   STALE        a handle whose gallery epoch has passed (afis_gallery_commit after afis_gallery_reopen, afis_gallery_remove, afis_gallery_commit_at) or whose
 *                subset has been freed (afis_subset_free marks the context's kept matrices of that subset).  Reading, recalling and fusing a stale handle is
 *                AFIS_ESTATE, with a message that names the edit; the info call still answers, with stale = 1; freeing always works
 *   THE CELL RULE  (csrc/matrix_fuse.h, one definition for host and device) for the operands k = 0 .. n - 1 in argument order, c_k the cell word — the one across
 *                the diagonal where the operand is read transposed —, v_k its float, w_k its weight (1.0 where weights is NULL):
 *                  there_k   c_k is not the no-entry word 0xffffffff
 *                  part_k    raw matrices: there_k and the sign bit of v_k + 0.0f clear — the case lists' rule: the -1 of an empty template, every negative value
 *                            and a NaN with the sign set stay out.  Normalised matrices: there_k — a negative z-score is a value, and every outside cell became
 *                            no entry when the matrix was normalised
 *                  no operand is there                                        -> no entry
 *                  AFIS_FUSE_REQUIRE_ALL and some operand is not there        -> no entry
 *                  otherwise no operand takes part (raw matrices only), or with AFIS_FUSE_REQUIRE_ALL some operand that is there does not take part -> -1.0f
 *                  AFIS_FUSE_SUM   double acc = +0.0; for every k that takes part, in order: acc = acc + w_k * (double)v_k — the product and the sum each rounded
 *                            in fp64, no fused multiply-add; the result is (float)acc.  A sum that is no number is the one word 0x7fc00000: which NaN an
 *                            operation produces (the sign of inf - inf and of 0 x inf, what survives of a payload) differs between processors, so the rule names
 *                            the word
 *                  AFIS_FUSE_MAX / AFIS_FUSE_MIN   the v_k of greatest / least rank key (the ordered word of v_k + 0.0f) among those that take part; the first
 *                            operand that holds it keeps its bits
 * afis_matrix_keep    copies the last search's matrix, whatever left it, and its record into a new handle, on the context's stream.  The checks are the ranking
 *                     calls' (a committed gallery, a matrix still there and of the shard as it stands: AFIS_ESTATE otherwise); the matrix is neither written nor
 *                     invalidated, as by afis_score_stats.  An empty shard or n_q == 0 gives a valid handle of zero cells and queues nothing.  Option
 *                     "matrix_keep_us" (read-only): the device time of the copy
 * afis_matrix_free    releases a handle; NULL and a handle that is not live are ignored.  afis_destroy releases the handles that are left
 * afis_matrix_info    fills *out for any live handle, stale or not
 * afis_matrix_read    rows row0 .. row0 + n_rows - 1 of a kept matrix into out [n_rows][columns], the columns in the order of the search's scores output (for a
 *                     subset the caller's column order).  AFIS_EINVAL for rows outside the matrix or a null out
 * afis_matrix_recall  copies the kept matrix back as the last search's matrix and restores its record, the normalised mark included: after afis_normalize_scores and
 *                     a recall of the raw matrix afis_score_stats works again, and the matrix may be normalised along the other axis.  It needs no last search.
 *                     The handle stays usable
 * afis_matrix_fuse    applies the cell rule to 1 <= n <= AFIS_FUSE_OPERANDS_MAX operands.  All of one n_q and one columns, all over the same subset or all over the
 *                     whole shard, all raw or all normalised — AFIS_EINVAL otherwise.  transposed[k] != 0 reads operand k transposed: only where n_q == columns, and
 *                     the CALLER vouches that row i and column i name the same print (a print search of a set over the same set, in one order; a subset must
 *                     have been listed in ascending order).  weights belong to AFIS_FUSE_SUM — NULL for the other modes — and each must be finite.  Every argument
 *                     error is reported before anything is queued, with the last matrix unchanged and rankable.  The same handle may appear more than once:
 *                     (A, A) with transposed = (0, 1) under AFIS_FUSE_MIN is the symmetric score min(a -> b, b -> a).  After AFIS_OK the result IS the last
 *                     search's matrix, with the operands' record: every ranking call reads it (a fused normalised matrix takes min_score in z units), and
 *                     scores_out, where given, receives it in the search's column order.  Option "matrix_fuse_us" (read-only): the device time of the launches
 * How      csrc/afis_matrix.cpp, csrc/matrix_fuse.hip.  k_matrix_fuse: a thread owns one column of a row — four adjacent ones as one 16-byte word where columns
 *          % 4 == 0 —, the operands' pointers and weights travel in the kernel's argument segment (scalar loads), the loads of four operands are in flight
 *          together; no atomic, no LDS, every output word written once.  The result is built in the spare of the two score buffers and swapped in, as
 *          afis_search_eligible's and afis_normalize_scores' are.  A transposed operand goes through k_transpose_scores into scratch first, once per distinct handle.
 * Shards: every untransposed call is per rank, without an exchange: a rank's columns are its shard's, keep / recall / fuse the same operands on every rank and merge
 *          the ranking calls' lists as before.  S-norm needs the merged statistics first.
 * These calls do not give: fusing matrices of different column sets (a subset's columns into a whole-shard matrix); a transposed operand across shards (row i's mate
 *          column lies on another rank) or over a subset listed out of order; the match CLI. */
typedef struct afis_matrix afis_matrix;
#define AFIS_FUSE_SUM 0
#define AFIS_FUSE_MAX 1
#define AFIS_FUSE_MIN 2
#define AFIS_FUSE_REQUIRE_ALL 4        /* or-ed into mode */
#define AFIS_FUSE_OPERANDS_MAX 16
typedef struct { int32_t n_q; int32_t normalized; int64_t columns; int32_t over_subset; int32_t stale; } afis_matrix_desc;
int  afis_matrix_keep  (afis_ctx* ctx, afis_matrix** out);
void afis_matrix_free  (afis_ctx* ctx, afis_matrix* m);
int  afis_matrix_info  (afis_ctx* ctx, const afis_matrix* m, afis_matrix_desc* out);
int  afis_matrix_read  (afis_ctx* ctx, const afis_matrix* m, int row0, int n_rows, float* out /*[n_rows][columns]*/);
int  afis_matrix_recall(afis_ctx* ctx, const afis_matrix* m);
int  afis_matrix_fuse  (afis_ctx* ctx, const afis_matrix* const* ms /*[n]*/, const double* weights /*[n] or NULL*/,
                        const uint8_t* transposed /*[n] or NULL*/, int n, int mode, float* scores_out /*[n_q][columns] or NULL*/);

/* afis_get_timing2 copies min(struct_size, sizeof(afis_timing)) bytes: pass sizeof(afis_timing) of the header the caller was compiled
 * against, so that a library with a longer struct never writes past the caller's.  afis_get_timing (kept for callers of the round-2
 * header) fills only the fields up to `pairs` (48 bytes, the struct of that header); the fields after it need afis_get_timing2. */
int afis_get_timing(const afis_ctx* ctx, afis_timing* out);
int afis_get_timing2(const afis_ctx* ctx, afis_timing* out, size_t struct_size);
/* Tunables (INTEGRATION.md section E has the table; timings in profiles/r04_tables.md).  "adc_variant" — every variant gives bit-identical results:
 * 9 [default] = an fp16 matrix-core pass over all (latent row, rolled point) cells bounds every row maximum and pins its candidate points; the rows that can
 * reach a pair's top 200 then get the exact fp32 value of their candidates, the table entries recomputed in the reference's arithmetic and order
 * (adc_mfma.hip, adc_refine.hip); 8 = a 16-bit fixed-point LDS-table pass bounds the candidates, which are then evaluated exactly from an fp32 table in HBM/L2
 * (the north_star's LDS-LUT design; 1.6 x the time of 9).  libafis_hip.so (the product) accepts 9 and 8 only; the direct exact kernels of rounds 1-2 — 7 = conflict-free lane classes, 1024-thread
 * workgroups (2.9 x); 6 = the same with 512; 0 = plain LDS gather, 1 = chain/row-quad rotated lanes, 2/3 = 0/1 with 1024-thread workgroups — are reference kernels built into libafis_hip_test.so only.
 * "mf_blocks" (form of variant 9's bound pass: 2 = two row blocks per wave, the only value; the three-row-block form was removed), "bound_cus" (below), "query_batch" (latents per launch group),
 * "chunk" (gallery templates per workgroup), "minu_generic" (force the generic minutiae candidate kernel), "s3_tie_order" (0 [default]: candidate norms that tie — in practice the zero norms that fill a list with fewer
 * than 120 positive similarities — are taken in ascending element order; 1: in the order libstdc++'s std::sort leaves them, i.e. what the reference binary's matcher.cpp:473-476 delivers:
 * such lists — and the rare list in which two positive norms tie — then go through the any-shape candidate kernel, one wave of which runs the sort; about +2 % of a search on structured templates), "ref_tie_order" (0 [default], 1 = "s3_tie_order" 1, 2 = in addition the greedy selections of S8 and S9 — matcher.cpp:1301 / :1423 / :1590 — walk
 * equal SCORES in std::sort's order: that is where mated pairs differ, whose dozens of surviving correspondences tie exactly at S9; with 2 the scores are the reference binary's on all but three of
 * 710 000 synthetic pairs [the texture top-200 sort of S7 stays in index order]; no measurable cost beyond level 1; the match CLI: -tie <n>), "search_timeout_s" (every host wait of a search is bounded: after this many seconds
 * without the device finishing, afis_search returns AFIS_EDEVICE instead of blocking; default 600, AFIS_SEARCH_TIMEOUT_S; <= 0 = unbounded; "search_timeout_ms" sets the same bound in
 * milliseconds; afis_get_option reads "search_timeout_s" rounded UP to whole seconds and "search_timeout_ms" exactly.  After such a timeout the device may still be working on the call: the caller's output
 * buffers must stay valid until afis_destroy, or until a later call on the context succeeds; afis_queries_free then only parks the handle (its device buffers are released by the next call that finds the device idle),
 * and afis_destroy — which has to wait for the device — may block where the search did), "rowmax_budget_mb" (device memory of a launch group's per-pair
 * buffers; default 60 % of the free memory), "mf_stats" (adc_variant 9: collect the counters the parity tap afis_debug_refine_stats reads).  ("lut_dtype" accepts only 32: the
 * opt-in 16-bit tolerance path of rounds 1-2 did not meet its stated tolerance and was removed; every remaining path is bit-exact.)
 * Returns AFIS_EINVAL for unknown names. */
int afis_set_option(afis_ctx* ctx, const char* name, int64_t value);
/* The value an option has now (0 = automatic where the table says so).  Read-only: "minu_fast_max_latent" (256), "minu_fast_max_rolled" (512), "minu_fast_max_cells"
 * (38 912, counted with the odd row stride's padding column): the largest minutiae counts / latent x rolled similarities a candidate task may have to run in the matrix-core kernel's shape classes; larger tasks (the
 * reference's reader allows 2000 minutiae per template, matcher.cpp:788-790) go to the any-shape kernel — same results, slower (afis_timing.minu_fallback_tasks counts them).  "bound_cus": 128 by default — the bound pass runs on a stream confined to half of the chip's CUs
 * (hipExtStreamCreateWithCUMask) with the minutiae stage beside it on the other half: the pass is power-limited, half the CUs deliver 0.64 of its throughput;
 * 0 = one stream, kernels back to back; 32 ... 224 in steps of 32; the environment variable AFIS_BOUND_CUS sets the initial value.  "gallery_h2d_bytes" (read-only): the bytes handed to every host-to-device copy
 * of the context's gallery commits and removals so far, counted where the copies are issued: an appending commit adds its own points and the offset tables, not the resident shard.
 * "gallery_resident" (read-only): the templates of the committed shard, the G of afis_search's outputs (afis_gallery_size also counts what is staged beside it after afis_gallery_reopen).
 * "subset_device_bytes" (read-only): the device bytes held by the context's live subsets (0 when there is none); "subset_gather_us" (read-only): the device time of the last
 * afis_subset_create's gather launches, from HIP events around them.  "subject_rank_us" (read-only): the device time of the last afis_rank_subjects' launches (the maxima's
 * memset, k_subject_best and, for k <= 64, k_topk_subjects), from HIP events around them.  "rank_hits_us" (read-only): the device time of the last afis_rank_hits' or
 * afis_rank_subject_hits' launches (k_rank_hits; for subjects the maxima's memset and k_subject_best before it), from HIP events around them; 0 when that call queued nothing.
 * "rank_latents_us" (read-only): the device time of the last afis_rank_latent_hits' or afis_rank_latent_hits_filtered's launches (for the filtered call the filter pass
 * of hit_filter.hip first; k_transpose_scores, then k_rank_hits on the transposed matrix), from HIP events around them; 0 when that call queued nothing.
 * "rank_cases_us" (read-only): the device time of the last call of the case family, plain or filtered — afis_rank_case_hits, afis_rank_case_subject_hits and their
 * _filtered forms — (for a filtered call the filter pass first; the fold of case_fuse.hip — for subjects behind the maxima's memset, k_subject_best and the exclusions'
 * drops — then k_rank_hits on the fused rows), from HIP events around them; 0 when that call queued nothing.  "case_fuse_us" / "case_rank_us" (read-only): that call's
 * two parts, each from its own pair of events — everything before k_rank_hits (so a filtered call's filter pass too), and k_rank_hits.  "rank_filtered_us" (read-only): the device time of the last afis_rank_hits_filtered's or afis_rank_subject_hits_filtered's launches (the filter pass
 * of hit_filter.hip, for subjects the maxima's memset and k_subject_best, the exclusions' drops; then k_rank_hits), from HIP events around them; 0 when that call queued
 * nothing.  "filter_us" (read-only): of that call everything before k_rank_hits, from its own pair of events; 0 when the call queued nothing.
 * "rank_positions_us" (read-only): the device time of the last afis_rank_positions', afis_rank_subject_positions' or afis_count_before's launches (for a filtered call the
 * filter pass of hit_filter.hip first, for persons the maxima's memset, k_subject_best and the exclusions' drops; then k_position_targets and k_count_before), from HIP
 * events around them; 0 when that call queued nothing.
 * "score_stats_us" (read-only): the device time of the last afis_score_stats' launches (for a filtered call the filter pass of hit_filter.hip first; then, axis 0, the
 * limb table's memset, k_score_stats_rows and k_score_stats_finish, or, axis 1, k_score_stats_cols), from HIP events around them; 0 when that call queued nothing.
 * "normalize_us" (read-only): the device time of the last afis_normalize_scores' launches (k_normalize_scores; for a subset listed out of order with scores_out given
 * the columns' permutation too), from HIP events around them; 0 when that call queued nothing.
 * "score_histogram_us" (read-only): the device time of the last afis_score_histogram's launches (for a filtered call the filter pass of hit_filter.hip first; axis 1:
 * k_transpose_scores; then the counts' memset and k_score_hist_rows), from HIP events around them; 0 when that call queued nothing.
 * "entries_at_us" (read-only): the device time of the last afis_entries_at's launches (for a filtered call the filter pass of hit_filter.hip first; then per digit of the
 * select the bins' memset, k_select_count and k_select_step, and k_select_finish), from HIP events around them; 0 when that call queued nothing.
 * "subject_score_stats_us" (read-only): the device time of the last afis_subject_score_stats' launches (for a filtered call the filter pass of hit_filter.hip first; then
 * the maxima's memset, k_subject_best, the excluded persons' drops and k_subject_keys; then afis_score_stats' kernels over the person cells), from HIP events around
 * them; 0 when that call queued nothing.
 * "subject_score_histogram_us" (read-only): the same for the last afis_subject_score_histogram (behind k_subject_keys: axis 1's transposition, the table's memset,
 * k_score_hist_rows over the person cells); 0 when that call queued nothing.
 * "subject_entries_at_us" (read-only): the same for the last afis_subject_entries_at (behind k_subject_keys: per digit of the select the bins' memset, k_select_count and
 * k_select_step, and k_subject_select_finish); 0 when that call queued nothing.
 * "link_groups_us" (read-only): the device time of the last afis_link_groups' or afis_link_subject_groups' launches (for a filtered call the filter pass of hit_filter.hip
 * first; then the counters' memset, k_link_init, for persons in mutual mode k_link_first_cols and k_link_row_cols, k_link_scan, k_link_flatten and k_link_compact), from
 * HIP events around them; 0 when that call queued nothing.
 * "link_d2h_bytes" (read-only): the bytes that call returned from the device: 32 of counters, then 8 per node in a group of two or more; 0 when that call queued nothing.
 * "matrix_device_bytes" (read-only): the device bytes held by the context's live kept matrices (0 when there is none).  "matrix_keep_us" (read-only): the device time
 * of the last afis_matrix_keep's copy, from HIP events around it; 0 when that call queued nothing.  "matrix_fuse_us" (read-only): the device time of the last
 * afis_matrix_fuse's launches (k_transpose_scores once per distinct transposed operand, then k_matrix_fuse), from HIP events around them; 0 when that call queued nothing.
 * "corr_pairs_per_launch" (settable, 1 .. 1 048 576; default AFIS_CORR_PAIRS_PER_LAUNCH): the pairs of one chunk of afis_correspondences_pairs at most — about 5.8 KB of
 * device memory and 2.9 KB of pinned host memory each.  "correspondences_us" (read-only): the device time of the last afis_correspondences_pairs' or afis_correspondences'
 * launches (per chunk and launch group k_minu_cands<true> and k_graph_minutiae in its pair form), from HIP events around every chunk's, summed; 0 when that call queued nothing.
 * "score_pairs_per_launch" (settable, 1 .. 1 048 576; default AFIS_SCORE_PAIRS_PER_LAUNCH): the pairs of one chunk of afis_score_pairs at most — about 5.8 KB of device
 * memory each plus 8 bytes per row of the handle's longest latent texture template (at most 8 KB), and 36 bytes of pinned host memory.  "score_pairs_us" (read-only): the
 * device time of the last afis_score_pairs' launches (per chunk and launch group k_minu_cands<true>, k_graph_minutiae in its pair form, k_adc_pairs, k_graph_texture in its
 * pair form, k_fuse_pairs), from HIP events around every chunk's, summed; 0 when that call queued nothing.
 * "texture_correspondences_us" (read-only): the device time of the last afis_texture_correspondences_pairs' or afis_texture_correspondences_print_pairs' launches (per
 * chunk and launch group the score call's kernels without the fusion, the texture list kernel with its tap, and k_pair_evidence; the print form's gathers), from HIP
 * events around every chunk's, summed; 0 when that call queued nothing.  "pair_alignments_us" (read-only): the same for the last afis_pair_alignments or
 * afis_print_pair_alignments.  Both calls chunk by "corr_pairs_per_launch": a pair takes the score call's device memory plus 1.6 KB for the tap and 3.2 KB (the export)
 * or 288 bytes (the moments) of device and of pinned host memory.
 * "eligible_classes" (read-only): the classes — distinct mask triples — of the last afis_search_eligible; "eligible_expand_us" (read-only): the device time of that
 * call's expand launches (k_expand_rows), from HIP events around each, summed over the classes; both 0 after a call that failed or had no queries.
 * "weighted_batch_pseudo" (settable, >= 0; default 0): the pseudo-queries of one batch of afis_search_weighted at most; 0 = as many as an eighth of the launch-group
 * budget holds the per-part scores of.  Results do not depend on it.  "weighted_pseudo_queries" (read-only): the pseudo-queries the last afis_search_weighted scored;
 * "weighted_fold_us" (read-only): the device time of that call's fold launches (k_fold_templates), from HIP events around each, summed over the batches; both 0 after a
 * call that failed or had no queries (afis_search_prints sets the last two as well, and obeys the first).
 * "print_gather_us" (read-only): the device time of the last afis_search_prints' gather launches (print_queries.hip), from HIP events around each launch group's,
 * summed; "print_h2d_bytes" (read-only): the bytes that call handed to host-to-device copies — the launch groups' tables and the fold's —, counted where the copies
 * are issued; both 0 after a call that failed or had no queries.
 * "print_pairs_batch_prints" (settable, >= 0; default 0): the query prints of one batch — one temporary query handle — of afis_score_print_pairs and
 * afis_correspondences_print_pairs at most; 0 = as many consecutive prints as an eighth of the launch-group budget holds the views of, and at least one.  Results do not
 * depend on it.  "print_pairs_us" (read-only): the device time of the last such call's launches — the gathers of print_queries.hip and every chunk's pair kernels, the
 * score call's ending in k_fold_print_pairs —, from HIP events, summed over batches and chunks; "print_pairs_query_prints" (read-only): the distinct query prints that
 * call gathered; both 0 after a call that failed or queued nothing.
 * "cascade_pairs_per_launch" (settable, 1 .. 1 048 576; default AFIS_CASCADE_PAIRS_PER_LAUNCH): the pairs of one chunk of afis_search_cascade's second stage at most —
 * 8 bytes per row of the handle's longest latent texture template each (at most 8 KB) for the dense row maxima; results do not depend on it.
 * "cascade_stage1_us" (read-only): the device time of the last afis_search_cascade's first stage (per launch group the candidate kernel, the minutiae list kernel,
 * k_fuse_stage1); "cascade_select_us" (read-only): of its selection (k_rank_hits); "cascade_stage2_us" (read-only): of its second stage (the no-entry fill,
 * k_cascade_gather, per chunk and launch group k_adc_pairs, k_graph_texture in its pair form, k_fuse_pairs, then k_cascade_scatter) — each from its own pair of HIP
 * events; "cascade_kept_pairs" (read-only): the pairs that second stage scored; all four 0 after a call that failed or was empty.
 * "print_cascade_stage1_us" (read-only): the device time of the last afis_search_prints_cascade's first stage (per launch group the candidate kernel and the minutiae
 * list kernel, then k_print_cascade_stage1); "print_cascade_select_us" (read-only): of its selection (k_rank_hits); "print_cascade_stage2_us" (read-only): of its
 * second stage (the no-entry fill, k_print_cascade_gather, per chunk and launch group k_adc_pairs and k_graph_texture in its pair form, then k_print_cascade_finish) —
 * each from its own pair of HIP events; "print_cascade_kept_pairs" (read-only): the pairs that second stage scored; all four 0 after a call that failed or was empty.
 * That call obeys "cascade_pairs_per_launch" and sets "print_gather_us" and "print_h2d_bytes" as afis_search_prints does. */
int afis_get_option(const afis_ctx* ctx, const char* name, int64_t* value);

/* The parity-test taps (stage intermediates: afis_debug_*) are NOT part of this library: they are declared in
 * include/afis_matcher_taps.h and exported only by libafis_hip_test.so (the product objects plus afis_taps.cpp and adc_direct.hip),
 * which tests/ load.  libafis_hip.so exports exactly the functions declared above. */

#ifdef __cplusplus
}
#endif
#endif /* AFIS_MATCHER_H */
