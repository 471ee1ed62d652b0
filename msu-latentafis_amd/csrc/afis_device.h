// afis_device.h — device-side data layout and kernel launchers shared by the HIP translation units.
// gfx950 (MI355X / CDNA4) only; wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "score_order.h"

namespace afis {

typedef unsigned long long u64;
constexpr int kM = 16;            // PQ sub-quantizers         (codebook header, matcher.cpp:74)
constexpr int kK = 256;           // codewords per sub-quantizer
constexpr int kDsub = 6;          // dims per sub-quantizer
constexpr int kDes = 96;          // descriptor length
constexpr int kTexMax = 1000;     // MaxNRolledMinu / MaxNLatentMinu, matcher.h:31-32
constexpr int kTopTex = 200;      // Matcher::N, matcher.cpp:33
constexpr int kTopMinu = 120;     // topN, matcher.cpp:479
constexpr int kDistN = 50;        // dist_N, matcher.cpp:45
constexpr int kTileRows = 8;      // latent texture rows whose LUT one workgroup keeps in LDS (8*16 KB = 128 KB)
constexpr int kTileFloats = kTileRows * kM * kK;   // 32768 floats per LUT tile

// Rolled gallery shard, SoA in HBM.  Points of all templates are concatenated; *_off are CSR offsets.
struct GalleryDev {
    int32_t G = 0;
    const int32_t* minu_off = nullptr;   // [G+1]
    const short2*  minu_xy = nullptr;    // [NM]   pixel coords
    const float*   minu_ori = nullptr;   // [NM]
    const float*   minu_des = nullptr;   // [NM][96]
    const float4*  minu_frag = nullptr;  // the same descriptors as MFMA operand fragments: per template ceil(n/16) tiles of 16 descriptors,
                                         // tile = [v < 6][lane < 64] float4 with lane l, component c = des[16*tile + (l&15)][4*(4v + c) + (l>>4)]
                                         // (zero rows pad the last tile): a wave fetches a fragment with six fully coalesced 1 KB loads
    const int32_t* minu_tile_off = nullptr;  // [G+1] first tile of each template in minu_frag
    const int32_t* tex_off = nullptr;    // [G+1]  (counts already clamped to 1000)
    const short2*  tex_xy = nullptr;     // [NT]   block coords
    const float*   tex_ori = nullptr;    // [NT]
    const uint4*   tex_codes = nullptr;  // [NT]   16 PQ code bytes per point, byte m = sub-quantizer m
    const uint4*   tex_codes_cf = nullptr;  // the same bytes as a per-template stream of (blocks + 1) x 64 lane entries, permuted per
                                            // lane class and half-period shifted for the conflict-free direct ADC kernel (adc_direct.hip)
    const int32_t* tex_cf_blk = nullptr;    // [G+1] offset of each template's stream in tex_codes_cf, in 64-entry blocks (both laid out at the first use of that kernel)
    const uint8_t* empty = nullptr;      // [G] 1 = rolled template has neither minutiae nor texture (score -1)
    int32_t* task_ctr = nullptr;         // [4] next-task counters of the graph kernels (texture, minutiae), the refine kernel and the candidate kernel: zeroed by their launchers
};

// A group of latents resident on the device (selected minutiae templates 26, 2, 11 + texture template 0).
struct QueryDev {
    int32_t nq = 0;
    const int32_t* lm_off = nullptr;     // [nq*3+1] minutiae points of (query, selected template s); empty range = absent
    const short2*  lm_xy = nullptr;
    const float*   lm_ori = nullptr;
    const float*   lm_des = nullptr;     // [NLM][96]
    const float4*  lm_frag = nullptr;    // latent descriptors as MFMA operand fragments (layout as GalleryDev::minu_frag)
    const int32_t* lm_tile_off = nullptr;   // [nq*3+1]
    const int32_t* lt_off = nullptr;     // [nq+1] texture rows (clamped to 1000)
    const short2*  lt_xy = nullptr;
    const float*   lt_ori = nullptr;
    const float*   lt_des = nullptr;     // [NLT][96]
    const int32_t* tile_off = nullptr;   // [nq+1] LUT tiles (8 rows each) per query
    const int32_t* tile16_off = nullptr; // [nq+1] 16-row tiles of adc_variant 8's quantised table
    int32_t n_tiles16 = 0;
    const int32_t* tex_slot = nullptr;   // [nq] index of the texture score in the reference's score vector (= #latent minutiae templates), -1 = no texture
    const int32_t* status = nullptr;     // [nq] AFIS_QUERY_*
    int32_t n_tiles = 0;
    int32_t lt_pad = 0;                  // row stride of the rowmax buffers (max rows over the group, multiple of 8)
};

// ---- launchers (each enqueues on `stream`, returns hipGetLastError()) ------------------------------------------
// S4: LUT tiles.  variant selects the in-tile layout the ADC kernel of the same variant reads.
#ifdef __HIPCC__
// Correctly rounded fp32 square root for x == 0 or 1 <= x < 2^64 (squared distances): the hardware v_sqrt_f32 is only accurate to
// 1 ulp (and HIP's __fsqrt_rn IS that instruction, not a correctly rounded sqrt), so the result is settled between its two
// neighbours with two exact residuals — the core of LLVM's own correctly rounded sqrtf expansion, without the denormal scaling
// and the inf/nan handling this argument range does not need.  Checked against the definition of round-to-nearest for every
// float in the range by tools/ubench/sqrt_exact.hip.
__device__ __forceinline__ float sqrt_rn_pos(float x)
{
    float r = __builtin_amdgcn_sqrtf(x);
    const float dn = __int_as_float(__float_as_int(r) - 1), up = __int_as_float(__float_as_int(r) + 1);
    const float e_dn = __builtin_fmaf(-dn, r, x), e_up = __builtin_fmaf(-up, r, x);
    r = e_dn <= 0.0f ? dn : r;
    r = e_up > 0.0f ? up : r;
    return r;
}
#endif

#ifdef __HIPCC__
// S4, one table entry: lut[i][m][k] = sum_{d<6} (des[i][6m+d] - cw[m][k][d])^2, d ascending, difference, product and sum rounded separately
// (include.h:327-359; every translation unit is built with -ffp-contract=off).  Shared by the table builders (adc.hip), the PQ encoder and the
// exact recomputation of adc_mfma.hip: one definition, one set of bits.
__device__ __forceinline__ float lut_entry(const float* __restrict__ des6, const float* __restrict__ cw6)
{
    float dist = 0.0f;
#pragma unroll
    for (int d = 0; d < kDsub; ++d) {
        float t = des6[d] - cw6[d];
        float t2 = t * t;
        dist += t2;
    }
    return dist;
}
#endif

// The direct exact ADC kernels (adc_direct.hip, adc_variant 0-3, 6, 7; linked into libafis_hip_test.so only).  S4: the tile LUT of kTileRows rows.
hipError_t launch_lut_build(const QueryDev& q, const float* codewords, float* lut_tiles, int variant, hipStream_t stream);
// S5+S6: ADC similarity + per-row (max, first argmax) for queries [q0, q0+nq) against gallery templates.
hipError_t launch_adc_rowmax(const QueryDev& q, const GalleryDev& g, const float* lut_tiles, int chunk, int variant,
                             float* rm_val, int32_t* rm_arg, hipStream_t stream);
// the conflict-free kernel's lane-ordered code stream (variants 6 / 7): g.tex_cf_blk = its block offsets
hipError_t launch_codes_cf(const GalleryDev& g, void* out, hipStream_t stream);
// adc_variant 8 (adc.hip): 16-bit fixed-point LUT tiles of 16 rows + per-row (offset, step, margin); the lane-ordered code stream it reads
// (ceil(n/64) blocks per template, first block q_blk[t]); S5+S6 with integer sums as a bound pass.
hipError_t launch_lutq_build(const QueryDev& q, int n_rows_total, const float* codewords, float* row_min, float* row_rng, void* tiles, void* rowc, hipStream_t stream);
hipError_t launch_codes_q(const GalleryDev& g, const int32_t* q_blk, void* out, hipStream_t stream);
// lut32 != NULL (adc_variant 8): the quantised pass only bounds the candidates, which are then evaluated exactly from the fp32 table in the
// reference layout [row][16][256] (launch_lut_reference_layout over all latent texture rows of the group): exact results, bit for bit.
hipError_t launch_adc_rowmax_q(const QueryDev& q, const GalleryDev& g, const void* codes_q, const int32_t* q_blk, const void* lutq_tiles, const void* rowc,
                               const float* lut32, int chunk, int share, float* rm_val, int32_t* rm_arg, hipStream_t stream);
// adc_variant 9 (adc_mfma.hip): fp16 matrix-core bound pass + exact recomputation.  launch_mf_codebook: fp16 codebook (16-byte entries) and
// |cw|^2 table, once per context.  launch_mf_tiles: tile-aligned (32 points) codes / point terms / tile directory of the gallery (first use).
// launch_mf_rows: per latent row of a query group the fp16 B fragments and (c, Es, Tg, force).  launch_adc_mfma: the bound pass ->
// rec[template * R_pad + row].  launch_tex_refine: bounds -> the rows that can reach the top 200 -> exact (max, first arg-max).  Two output forms: compact (rm_n != NULL: what a
// search uses) — per pair the evaluated rows side by side in row order, value in rm_cv[pair * lt_pad + slot], (row | point << 16) in rm_arg[pair * lt_pad + slot], their count in rm_n[pair];
// rm_val is not touched — or dense (rm_n == NULL): value and point at rm_val / rm_arg[pair * lt_pad + row], -inf for the other rows (all_rows != 0: every row exactly; the parity taps use it).
hipError_t launch_mf_codebook(const float* codewords, void* cw16, float* cwn, hipStream_t stream);
// t_first / n_templates (afis_gallery_commit on a reopened gallery): only templates [t_first, t_first + n_templates) are laid out (n_templates < 0: to the end)
hipError_t launch_mf_tiles(const GalleryDev& g, const int32_t* t32_blk, const float* cwn, void* codes_p, float* nrm_p, void* tile_meta, hipStream_t stream, int t_first = 0, int n_templates = -1);
hipError_t launch_mf_rows(const float* lt_des, int n_rows, int n_rb, const float* codewords, const float* cwn, void* bfrag, void* rowk, hipStream_t stream);
hipError_t launch_adc_mfma(const GalleryDev& g, const void* codes_p, const float* nrm_p, const void* tile_meta, const int32_t* tile0, const void* cw16,
                           const void* bfrag, const void* rowk, int n_rows, int n_rb, int R_pad, int chunk, void* rec,
                           unsigned long long* diag /* NULL or a diagnostics row: clock samples */, hipStream_t stream);
hipError_t launch_tex_refine(const QueryDev& q, const GalleryDev& g, const float* codewords, const void* rec, const void* rowk, int R_pad, int all_rows,
                             float* rm_val, int32_t* rm_arg, unsigned long long* stats, float* rm_cv, int32_t* rm_n, hipStream_t stream);
// one correspondence of a minutiae-template list (S3 output), 8 bytes
struct MinuCand { float sim; short li, ri; };

// ---- shape classes of the fast candidate kernel k_minu_cands_rt<S> (minu.hip), S = 1, 2, 4: workgroups of 256 S threads.  A task (nL latent x nR rolled
// minutiae) fits class S when its similarity matrix fits the class's LDS array with row stride rt_row_stride() and the selection's 32 keys per thread
// cover it: nL <= rt_max_rows(S, nR).  It is done by the smallest class that takes it; tasks no class takes go to the any-shape kernel.
// (matcher.cpp:788-790 lets a template carry 2000 minutiae; extraction_rolled.py:105-108 caps nothing for rolled prints.)
#ifdef __HIPCC__
#define AFIS_HOST_DEVICE __host__ __device__
#else
#define AFIS_HOST_DEVICE
#endif
AFIS_HOST_DEVICE constexpr int rt_class_max_rolled(int S) { return S == 1 ? 128 : S == 2 ? 256 : 512; }
AFIS_HOST_DEVICE constexpr int rt_class_max_latent(int S) { return S == 1 ? 64 : 256; }
// floats of the similarity matrix in LDS: 32 similarities per thread (+ the odd stride's padding column) for S = 1, 2; the large class takes what a CU's 160 KB leave
// beside the other arrays (38 912 floats = 152 KB) and walks the rows beyond its threads' 32 register keys a second time (k_minu_cands_rt: "key blocks")
AFIS_HOST_DEVICE constexpr int rt_class_simi_floats(int S) { return S == 1 ? 8192 : S == 2 ? 8192 * 2 + 256 : 38912; }
AFIS_HOST_DEVICE constexpr int rt_class_keys_per_thread(int S) { return S == 4 ? 64 : 32; }
AFIS_HOST_DEVICE inline int rt_row_stride(int S, int nR) { return S == 1 ? (((nR & 1) || nR == 128) ? nR : nR + 1) : (nR | 1); }
AFIS_HOST_DEVICE inline int rt_max_rows(int S, int nR)            // the largest latent minutiae count class S takes against nR rolled minutiae (0: none); non-decreasing in S
{
    if (nR <= 0 || nR > rt_class_max_rolled(S)) return 0;
    int m = rt_class_keys_per_thread(S) * ((256 * S) / nR);                  // thread = (column, row phase): 32 keys in registers (the large class: and as many again recomputed)
    const int cap = rt_class_simi_floats(S) / rt_row_stride(S, nR);
    m = m < cap ? m : cap;
    return m < rt_class_max_latent(S) ? m : rt_class_max_latent(S);
}
// ---- launch groups (host): the latents of a search are cut into contiguous runs that are launched together (afis_search.cpp::afis_queries_upload).
// launch_group_latents: latents per launch at most when the option is 0 — about five million (latent, rolled) pairs, between 10 and 128 latents.
// launch_group_cuts: the group ends (exclusive) for n = rows_prefix.size() - 1 latents, at most `per` latents each.  by_row_groups (adc_variant 9): the bound pass works in row
// groups of 768 latent texture rows and a launch pays for its last one in full, so the cuts are placed where the total number of row groups is smallest (dynamic programme
// over the cut positions; ties: fewer launches, then the earliest last cut); otherwise runs of `per`.  rows_prefix[i] = latent texture rows of latents 0 .. i-1.  Results never depend on the cuts.
inline long long launch_group_latents(long long G) { if (G < 1) G = 1; const long long w = (5000000 + G / 2) / G; return w < 10 ? 10 : w > 128 ? 128 : w; }
inline void launch_group_cuts(const long long* rows_prefix, int n, int per, bool by_row_groups, int* cuts /* [n] at most */, int* n_cuts)
{
    *n_cuts = 0;
    if (n <= 0) return;
    if (per < 1) per = 1;
    if (!by_row_groups || n == 1) { for (int i = per; i < n; i += per) cuts[(*n_cuts)++] = i; cuts[(*n_cuts)++] = n; return; }
    const long long kInf = 1ll << 60, rg_rows = 768;
    long long* best = new long long[(size_t)n + 1]; int* from = new int[(size_t)n + 1]; int* cnt = new int[(size_t)n + 1];
    best[0] = 0; from[0] = 0; cnt[0] = 0;
    for (int i = 1; i <= n; ++i) {
        best[i] = kInf; from[i] = 0; cnt[i] = 0;
        for (int j = (i - per > 0 ? i - per : 0); j < i; ++j) {
            const long long c = best[j] + (rows_prefix[i] - rows_prefix[j] + rg_rows - 1) / rg_rows;
            if (c < best[i] || (c == best[i] && cnt[j] + 1 < cnt[i])) { best[i] = c; from[i] = j; cnt[i] = cnt[j] + 1; }
        }
    }
    int m = 0;
    for (int i = n; i > 0; i = from[i]) cuts[m++] = i;
    for (int a = 0, b = m - 1; a < b; ++a, --b) { const int t = cuts[a]; cuts[a] = cuts[b]; cuts[b] = t; }
    *n_cuts = m;
    delete[] best; delete[] from; delete[] cnt;
}
// ints of the candidate stage's control buffer: [fallback count | n_tasks fallback task ids | 8 control words | 3 G work-list entries]
inline size_t minu_fb_ints(size_t n_tasks, size_t G) { return 1 + n_tasks + 8 + 3 * G; }
// floats of global scratch one workgroup of k_minu_cands needs: simi[n] | keys[n] | rowsum[2048] | colsum[2048], n = the largest latent x rolled minutiae count of the launch
// (rounded to 64); with option s3_tie_order three more arrays of n words (the index array std::sort permutes and the two pointers' stops: minu.hip)
inline size_t minu_scratch_floats(int max_nL, int max_nR, int s3_tie_order)
{
    const size_t n = ((size_t)(max_nL > 1 ? max_nL : 1) * (size_t)(max_nR > 1 ? max_nR : 1) + 63) / 64 * 64;
    return (s3_tie_order ? 5 : 2) * n + 4096;
}
// The grid of k_minu_cands for a launch group of a search (launch_minu_cands' scratch_floats_per_wg and n_wg): 1024 workgroups, halved while their scratch exceeds 8 GiB,
// never below 64.  A group of shorter latent lists may keep MORE workgroups under the cap than a longer one, and then needs more scratch: what is prepared for several
// groups is minu_scratch_bytes, the largest of their needs, not the longest group's.
struct MinuGrid { size_t wg_floats; int n_wg; size_t bytes() const { return wg_floats * 4 * (size_t)n_wg; } };
inline MinuGrid minu_cands_grid(int max_nL, int max_nR, int s3_tie_order)
{
    MinuGrid g{minu_scratch_floats(max_nL, max_nR, s3_tie_order), 1024};
    while (g.n_wg > 64 && g.bytes() > ((size_t)8 << 30)) g.n_wg /= 2;
    return g;
}
// ... and for a chunk of n_pairs pairs of a pair-list call (launch_minu_cands_pairs; afis_ctx.h: PairCall): what fits the chip at once — n_cus CUs of 160 KB of LDS, a
// workgroup taking lds_bytes_per_wg (minu_cands_lds_bytes) — since its workgroups stride over the 3 n_pairs tasks, within the scratch the context can afford: what the
// searches have made it hold already (scratch_bytes_held), or 1 GB — a pair of 2000 x 2000 minutiae takes 32 MB of it per workgroup.  At least one workgroup.
inline MinuGrid minu_cands_pairs_grid(int max_nL, int max_nR, int s3_tie_order, int n_cus, size_t lds_bytes_per_wg, size_t scratch_bytes_held, size_t n_pairs)
{
    MinuGrid g{minu_scratch_floats(max_nL, max_nR, s3_tie_order), 1};
    const size_t afford = scratch_bytes_held > ((size_t)1 << 30) ? scratch_bytes_held : (size_t)1 << 30;
    const size_t per_cu = (size_t)(160 << 10) / lds_bytes_per_wg;
    size_t n = (size_t)(n_cus > 1 ? n_cus : 1) * (per_cu > 1 ? per_cu : 1);
    if (afford / (g.wg_floats * 4) < n) n = afford / (g.wg_floats * 4);
    if (n < 1) n = 1;
    if (3 * n_pairs < n) n = 3 * n_pairs;
    g.n_wg = (int)n;
    return g;
}
inline size_t minu_scratch_bytes(const int* max_nL, size_t n_groups, int max_nR, int s3_tie_order)   // max_nL [n_groups]: the longest latent list of every launch group
{
    size_t bytes = 0;
    for (size_t i = 0; i < n_groups; ++i) { const size_t b = minu_cands_grid(max_nL[i], max_nR, s3_tie_order).bytes(); if (b > bytes) bytes = b; }
    return bytes;
}
// One row of 16 unsigned 64-bit diagnostics per launch group, zeroed at the start of a search and read back with its results (afis_timing):
enum { kDiagFallback = 0,       // candidate tasks handed to the any-shape kernel
       kDiagSmall = 1,          // tasks done by k_minu_cands_rt<1>, <2>, <4> (kDiagSmall + class)
       kDiagCandsClk = 4, kDiagCandsWall = 5,      // sampled workgroups of the candidate kernel: shader cycles and 100 MHz ticks they lived
       kDiagBoundClk = 6, kDiagBoundWall = 7,      // the same for the bound pass
       kDiagWords = 16 };
// The list kernels' slabs (graph.hip::dist_filter): the power iterations of S8 compute a row's neighbour values H(t, k) once, in iteration 0, and keep the first kTexSlabSteps /
// kMinuSlabSteps of every row in a region of global memory that belongs to the WORKGROUP (blockIdx.x; one wave each): per pass of 64 rows and block of four steps the lanes'
// four values (16 B per lane), then, behind all values, the four neighbour indices as the bytes of a dword — passes x steps x 64 lanes x 5 bytes.  Longer rows recompute what
// lies beyond.  The capacities cover the longest row of nearly every pass of the headline lists (mean row 24.8 / 10.6 neighbours, mean longest row of a pass 36 / 15.6) and most
// of the structured workload's (39 / 21 per row); afis_get_option reports them (graph_slab_steps_texture / _minutiae).  The launchers refuse a slab smaller than grid x bytes per
// workgroup, and the kernels reach it through a buffer descriptor of exactly its size.
constexpr int kTexSlabSteps = 48, kMinuSlabSteps = 32;
constexpr size_t kTexSlabWgBytes = (size_t)((kTopTex + 63) / 64) * kTexSlabSteps * 64 * 5;       // 61 440
constexpr size_t kMinuSlabWgBytes = (size_t)((kTopMinu + 63) / 64) * kMinuSlabSteps * 64 * 5;    // 20 480
// one-wave workgroups the list kernels are launched with: lists are drawn from a counter, the grids only have to fill the chip and keep the tail short
inline int graph_texture_grid(long long n_tasks) { return (int)(n_tasks < 16384 ? n_tasks : 16384); }
inline int graph_minutiae_grid(long long n_tasks) { return (int)(n_tasks < 32768 ? n_tasks : 32768); }
inline size_t graph_texture_slab_bytes(long long n_tasks) { return n_tasks > 0 ? (size_t)graph_texture_grid(n_tasks) * kTexSlabWgBytes : 0; }
inline size_t graph_minutiae_slab_bytes(long long n_tasks) { return n_tasks > 0 ? (size_t)graph_minutiae_grid(n_tasks) * kMinuSlabWgBytes : 0; }   // per instance of the kernel
// S7+S8b+S9: texture lists, one wave per (query, gallery template) -> parts[(q*G+g)*4+3]; rm_n != NULL: the compact form above (rm_val unused), otherwise the dense one (rm_cv unused).
// tap_stage (this launcher and launch_graph_minutiae): bits 0-7 = the stage a parity tap stops after (2 = the whole scorer); bit 8 = option ref_tie_order 2 (the <1> instantiation of the
// kernel: equal selectable scores of S8 / S9 in std::sort's order, graph.hip::sort_scores)
hipError_t launch_graph_texture(const QueryDev& q, const GalleryDev& g, const float* table_dist,
                                const float* rm_val, const int32_t* rm_arg, const float* rm_cv, const int32_t* rm_n, float* parts, void* slab, size_t slab_bytes, MinuCand* tap_out, int32_t* tap_n, int tap_stage, hipStream_t stream);
// texture lists (one-wave workgroups of k_graph_texture) that the current device keeps resident on one CU: 16, the wave slots its 128 registers leave, as long as a list's LDS
// stays within a sixteenth of the CU's (graph.hip: static_assert below TexSmem); afis_get_option reports it (graph_texture_lists_per_cu)
hipError_t graph_texture_lists_per_cu(int* lists);
// S1-S3 for the three selected latent minutiae templates: correspondence lists in rank order, cands[task][120], cand_n[task]
// (task = (q*3+s)*G + g).  Pairs of up to 256 latent x 512 rolled minutiae and 38 912 similarities go through the rolled-template-stationary MFMA kernel in one of its
// three shape classes (above); what it cannot take (other shapes, degenerate key distributions) it appends to `fallback` (count, task ids), which the
// generic kernel then works off.  force_generic: a flags word — bit 0: the generic kernel does every task; bit 1: option s3_tie_order (equal norms in std::sort's order where the generic kernel holds the matrix in LDS).  max_nL / max_nR: the longest latent list of the launch and the
// longest rolled minutiae template of the gallery (which classes can have work at all).
hipError_t launch_minu_cands(const QueryDev& q, const GalleryDev& g, float* scratch, size_t scratch_floats_per_wg, int n_wg,
                             int force_generic, MinuCand* cands, int32_t* cand_n, int32_t* fallback /* minu_fb_ints() ints */, int max_nL, int max_nR,
                             unsigned long long* diag /* NULL or a diagnostics row */, hipStream_t stream);
// S8a+S9 on those lists, one wave per list -> parts[(q*G+g)*4+{0,1,2}].  join: a second instance beside one that is already running (same list counter, no reset): it needs a slab of its own
hipError_t launch_graph_minutiae(const QueryDev& q, const GalleryDev& g, const MinuCand* cands, const int32_t* cand_n,
                                 float* parts, short4* corr_out, int32_t* corr_n, void* slab, size_t slab_bytes, MinuCand* tap_out, int32_t* tap_n, int tap_stage, hipStream_t stream, bool join = false);
// afis_correspondences_pairs (afis_corr.cpp): S1-S3 and S8a+S9 over a TABLE of (latent, template) pairs instead of a latents x gallery cross product, against the resident
// GalleryDev itself.  pair_tab (device): [n_pairs | (query of the group q, shard-local template) x n_pairs] int32.  Task 3 p + s — selected template s of pair p — owns the
// compact slot of that number: cands[task][120], cand_n[task], corr_out[task][120], corr_n[task], parts[4 p + s].  One launch of the any-shape candidate kernel, its
// workgroups striding over the tasks (n_wg workgroups, each with scratch_floats_per_wg of scratch: minu_scratch_floats over the group's longest latent list and the
// shard's longest rolled template), and one of the list kernel in its survivor-exporting form (grid and slab: graph_minutiae_grid / _slab_bytes of 3 n_pairs tasks).
// minu_cands_lds_bytes: the dynamic LDS of a candidate workgroup (how many fit a CU).
constexpr int kCorrPairsPerLaunch = 8192;               // AFIS_CORR_PAIRS_PER_LAUNCH: option corr_pairs_per_launch's default (48 MB of device memory, 24 MB pinned)
constexpr int kCorrPairsMax = 1 << 20;                  // ... and its ceiling: 3 tasks per pair stay far inside the launchers' 2^31 and a chunk's buffers below 6.1 GB
constexpr size_t kCorrBytesPerPair = 2 * 3 * kTopMinu * 8 + 2 * 3 * 4 + 16 + 8;   // candidates, survivors, their two counts, parts, the table's entry: 5 808
size_t minu_cands_lds_bytes(int s3_tie_order);
hipError_t launch_minu_cands_pairs(const QueryDev& q, const GalleryDev& g, float* scratch, size_t scratch_floats_per_wg, int n_wg, int s3_tie_order,
                                   const int32_t* pair_tab, int n_pairs, MinuCand* cands, int32_t* cand_n, hipStream_t stream);
hipError_t launch_graph_minutiae_pairs(const QueryDev& q, const GalleryDev& g, const int32_t* pair_tab, int n_pairs, const MinuCand* cands, const int32_t* cand_n,
                                       float* parts, short4* corr_out, int32_t* corr_n, void* slab, size_t slab_bytes, int s89_tie_order, hipStream_t stream);
// S10: fusion -> scores[q*G+g]
hipError_t launch_fuse(const QueryDev& q, const GalleryDev& g, const float* parts, float* scores, hipStream_t stream);
// afis_score_pairs (afis_pairs.cpp): the fused score and the four parts of a TABLE of pairs, group after group of the handle: after the two minutiae launches above (survivors
// into a scratch area), launch_adc_pairs (adc_pairs.hip) — S4-S6 exactly, over the group's pair table and the work list `seg` of pair_tables.h ((first pair, pairs <=
// kAdcPairsSegment) per segment of one latent's pairs; grid = segments x the group's 8-row tiles) -> the dense row maxima rm_val / rm_arg[p * q.lt_pad + row] —,
// launch_graph_texture_pairs (graph_pairs.hip: S7+S8b+S9 of pair p from those -> parts[4 p + 3]; grid and slab: graph_texture_grid / _slab_bytes of n_pairs tasks) and
// launch_fuse_pairs (S10 of pair p -> scores[p]: minu.hip::fuse_cell, the search's own expression).
// A pair costs kScorePairBytes + 8 q.lt_pad bytes of device memory (lt_pad <= 1000: at most 13.8 KB) and 36 bytes of pinned host memory.
constexpr int kScorePairsPerLaunch = 8192;              // AFIS_SCORE_PAIRS_PER_LAUNCH: option score_pairs_per_launch's default (at most 113 MB of device memory per chunk)
constexpr int kScorePairsMax = 1 << 20;                 // ... and its ceiling
constexpr size_t kScorePairBytes = 2 * 3 * kTopMinu * 8 + 2 * 3 * 4 + 16 + 4 + 16;   // candidates, survivors (scratch), their two counts, parts, score, the tables' entries: 5 820
hipError_t launch_adc_pairs(const QueryDev& q, const GalleryDev& g, const float* codewords, const int32_t* pair_tab, const int32_t* seg, int n_seg,
                            float* rm_val, int32_t* rm_arg, hipStream_t stream);
// tap_out [n_pairs][200] / tap_n [n_pairs] (both or neither; NULL for a score): pair p's list after S9 as (similarity, latent row, print point) in the reference's order
// and its length, -1 where the scorer does not run — the evidence calls read them (launch_pair_evidence below)
hipError_t launch_graph_texture_pairs(const QueryDev& q, const GalleryDev& g, const int32_t* pair_tab, int n_pairs, const float* table_dist, const float* rm_val, const int32_t* rm_arg,
                                      float* parts, void* slab, size_t slab_bytes, int s89_tie_order, MinuCand* tap_out, int32_t* tap_n, hipStream_t stream);
hipError_t launch_fuse_pairs(const QueryDev& q, const GalleryDev& g, const int32_t* pair_tab, int n_pairs, const float* parts, float* scores, hipStream_t stream);
// The evidence calls (afis_evidence.cpp; pair_evidence.hip): behind a group's list launches, one wave per pair of its table.  In: the minutiae survivors corr [3 n][120] /
// corr_n [3 n] (read for the moments only), the texture tap [n][200] / tap_n [n] and parts [n][4].  Out, each where given: mom [n][4] (pair_moments.h: scorers 0, 1, 2
// and the texture scorer), and the texture export ex_n [n] | ex_part [n] | ex_xy [n][200] with, optionally, ex_pt [n][200] and ex_sim [n][200] — every row written, zeros
// at and beyond the count.  At least one of mom and ex_xy.
struct CorrMoments;
struct PairEvidence {
    const short4* corr; const int32_t* corr_n; MinuCand* tap; int32_t* tap_n; const float* parts;       // (tap / tap_n: the texture list kernel of the same group writes them first)
    CorrMoments* mom; int32_t* ex_n; float* ex_part; short4* ex_xy; short2* ex_pt; float* ex_sim;
};
hipError_t launch_pair_evidence(const QueryDev& q, const GalleryDev& g, const int32_t* pair_tab, int n_pairs, const PairEvidence& e, hipStream_t stream);
// afis_search_cascade (afis_cascade.cpp, cascade.hip): the minutiae scorers for every cell, the texture scorer for the `keep` best prints of every latent.
// launch_fuse_stage1: S10 of a launch group with the texture score taken as +0.0f (fuse_cell.h) from parts[(q*G+g)*4 + 0..2] -> scores[q*G+g], the matrix the kept lists
// are selected from (launch_rank_hits at the ordered word of -inf, cap = keep).  launch_cascade_gather: one thread per (query, rank < n_kept) of those lists kept
// [n_q][keep] — the pair's entry of the second stage's pair tables (cascade_tables.h: q_slot [n_q + 1], piece_first [n_pieces + 1], piece_q0 [n_pieces]; tab 2 total +
// n_pieces ints, the count words of the pieces included) and parts[q][t][0..2] | +0.0f -> pair_parts[slot]; a query whose slot range is empty has no pairs.
// launch_cascade_scatter: out[q][t] = pair_score[slot], or -1.0f for a query without pairs, for every kept (q, t); nothing else of out [n_q][G] is written.
constexpr int kCascadePairsPerLaunch = 16384;           // AFIS_CASCADE_PAIRS_PER_LAUNCH: option cascade_pairs_per_launch's default (131 MB of dense row maxima at lt_pad 1000, the texture slab at its full 1.0 GB)
constexpr int kCascadePairsMax = 1 << 20;               // ... and its ceiling
hipError_t launch_fuse_stage1(const QueryDev& q, const GalleryDev& g, const float* parts, float* scores, hipStream_t stream);
hipError_t launch_cascade_gather(int n_q, int G, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot, const int32_t* piece_first,
                                 int n_pieces, const int32_t* piece_q0, const float* parts, int32_t* tab, float* pair_parts, hipStream_t stream);
hipError_t launch_cascade_scatter(int n_q, int G, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot, const float* pair_score,
                                  float* out, hipStream_t stream);
// The mapped forms (cascade_mapped.hip), for a cascade over a sub-shard of m templates of the resident shard (G_res templates): inv [G_res] int32 = the sub-shard position of a resident
// position or -1 (NULL: the identity, m == G_res), parts [n_q][m][4].  A kept entry that names no template of the sub-shard is routed to template 0 and scattered
// nowhere.  launch_cascade_scatter_mapped writes the kept cell (q, template gi) at out[row_of[q] * out_stride + out_col[gi]] (NULL tables: q, gi), out being
// [out_rows][out_stride]; a target outside it is not written.
hipError_t launch_cascade_gather_mapped(int n_q, int G_res, int m, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot,
                                        const int32_t* piece_first, int n_pieces, const int32_t* piece_q0, const int32_t* inv, const float* parts, int32_t* tab,
                                        float* pair_parts, hipStream_t stream);
hipError_t launch_cascade_scatter_mapped(int n_q, int G_res, int m, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot,
                                         const float* pair_score, const int32_t* inv, const int32_t* row_of, const int32_t* out_col, long long out_rows, long long out_stride,
                                         float* out, hipStream_t stream);

// S11: per-query rank list over the shard's scores [n_q][G] on the device (score descending, index ascending); out_idx[n_q][k] carries
// index_base + local index (-1 / -inf beyond G)
hipError_t launch_topk(const float* scores, int n_q, int G, int k, long long index_base, long long* out_idx, float* out_score, hipStream_t stream);

// optional in-kernel phase timers (build with PHASE_TIMING=1); zeros otherwise
hipError_t launch_pq_encode(const float* des, long long n, const float* codewords, uint8_t* codes, hipStream_t stream);
// descriptors -> MFMA operand fragment tiles on the device (pq_encode.hip); off / tile_off: [n_templates + 1] device arrays
hipError_t launch_fragment_tiles(const float* des, const int32_t* off, const int32_t* tile_off, int n_templates, void* frag, hipStream_t stream);
// afis_gallery_remove (gallery_edit.hip): one SoA array of the shard copied into a new buffer with every surviving template's range moved from old_off[t] to new_off[t]
// (device offset tables [G + 1]); elem_bytes 384 (descriptors), 16 (PQ codes) or 4 ((x, y), orientations); n_new = new_off[G]
hipError_t launch_compact_ranges(const void* src, void* dst, int elem_bytes, const int32_t* old_off, const int32_t* new_off, int G, long long n_new, hipStream_t stream);
// afis_gallery_commit_at (gallery_edit.hip): one SoA array of the shard written into a new buffer in which template t's range starts at new_off[t] and comes from the resident
// array at src_tab[t] (>= 0: the template stays) or from the staged array at ~src_tab[t] (< 0: it is replaced).  Device tables: src_tab [G], new_off [G + 1]; elem_bytes as above
hipError_t launch_splice_ranges(const void* res, const void* stg, void* dst, int elem_bytes, const int32_t* src_tab, const int32_t* new_off, int G, long long n_new, hipStream_t stream);
// afis_subset_create (gallery_subset.hip): one SoA array of the resident shard gathered by a template list — template t of the output takes the src_off[sel[t]] .. range of
// src and lands at dst_off[t] (device tables: src_off [G + 1], sel [n], dst_off [n + 1]; ranges in any order, possibly empty); elem_bytes 384, 16 or 4; n_out = dst_off[n]
hipError_t launch_gather_ranges(const void* src, void* dst, int elem_bytes, const int32_t* src_off, const int32_t* sel, const int32_t* dst_off, int n, long long n_out, hipStream_t stream);
// a subset search's epilogues: positions of the rank lists -> global indices (idx[i] = map[idx[i]] where 0 <= idx[i] < n_map; the -1 padding stays), and the score (4-byte)
// or part (16-byte) columns into the caller's order: dst[q][j] = src[q][pos[j]], j < n
hipError_t launch_subset_topk_map(long long* idx, long long n_idx, const long long* map, int n_map, hipStream_t stream);
hipError_t launch_permute_columns(const void* src, void* dst, int elem_bytes, int n_q, int n, const int32_t* pos, hipStream_t stream);
// afis_rank_subjects (subject_rank.hip): per (query, subject slot) the greatest composite (ordered score bits << 32 | ~position) over the positions whose template belongs
// to the slot -> best[n_q][S] (zeroed first; 0 stays where no position of the row belongs to the slot).  slot_of: [templates of the resident shard] int32 in [0, S);
// d_global NULL: position p of scores[n_q][G] is template p (a full search) — or a subset's [G] global indices: template d_global[p] - index_base
hipError_t launch_subject_best(const float* scores, int n_q, int G, const int32_t* slot_of, const long long* d_global, long long index_base, int S,
                               unsigned long long* best, hipStream_t stream);
// ... and the k best slots of every query, score descending / slot ascending: out_id = ids[slot], out_score = the score at the slot's best position (read from scores),
// out_best = index_base + position, or d_global[position]; (-1, -inf, -1) where k exceeds the slots that hold a composite
hipError_t launch_topk_subjects(const unsigned long long* best, int n_q, int S, const long long* ids, const float* scores, int G, const long long* d_global, long long index_base,
                                int k, long long* out_id, float* out_score, long long* out_best, hipStream_t stream);
// afis_rank_hits / afis_rank_subject_hits (rank_hits.hip): per query the entries whose ordered score word is >= thr — out_n[q] how many, and the min(out_n[q], cap) best in
// rank-list order, padded with (-1, -inf, -1) to cap.  best == NULL: the entries are the G scores of the row, ordered as k_topk orders them, out_a = the global index
// (index_base + position, or d_global[position]), out_b unused.  best != NULL: the entries are the S slots of best[n_q][S] as launch_subject_best left it, ordered as
// launch_topk_subjects orders them, out_a = ids[slot], out_b = the global index of the slot's best template.  thr >= 1 (the ordered word of -inf is 0x007fffff).
constexpr int kRankHitsMax = 4096;                      // AFIS_HITS_MAX: the composites of a list are sorted in LDS (32 KB)
hipError_t launch_rank_hits(const float* scores, int n_q, int G, const unsigned long long* best, int S, const long long* ids, const long long* d_global, long long index_base,
                            uint32_t thr, int cap, long long* out_n, long long* out_a, float* out_score, long long* out_b, hipStream_t stream);
// afis_rank_latent_hits (latent_rank.hip): the score matrix in [n_q][n] -> out [n][n_q], 64 x 64 tiles through LDS, both sides coalesced; launch_rank_hits then ranks
// out's rows — per print the queries — as it ranks a search's
hipError_t launch_transpose_scores(const float* in, float* out, int n_q, int n, hipStream_t stream);
// afis_rank_case_hits / afis_rank_case_subject_hits (case_fuse.hip): the member rows of every case — the CSR case_off [n_cases + 1] into member [n_q], query positions in
// ascending order inside a case — folded into one row: fused [n_cases][G] from scores [n_q][G], or fused [n_cases][S] from best [n_q][S] as launch_subject_best left it
// (a slot no template of the search covered gets the word 0xffffffff, whose key lies below every thr).  mode: kCaseSum — +0.0f plus the members whose key reaches +0.0's,
// in member order, one fp32 add each, -1.0f when there is none — or kCaseMax — the member value of greatest key, first member's bits.  launch_rank_hits then ranks
// fused's rows in its template form
constexpr int kCaseSum = 0, kCaseMax = 1;                // AFIS_CASE_SUM, AFIS_CASE_MAX
hipError_t launch_case_fuse(const float* scores, int G, const int32_t* case_off, const int32_t* member, int n_cases, int mode, float* fused, hipStream_t stream);
hipError_t launch_case_fuse_subjects(const unsigned long long* best, int S, const int32_t* case_off, const int32_t* member, int n_cases, int mode, float* fused, hipStream_t stream);
// afis_rank_case_hits_filtered / afis_rank_case_subject_hits_filtered: the same folds over what the filter pass below left — filtered [n_q][G], or best [n_q][S] made of
// it with the excluded persons dropped.  A member whose cell is the word 0xffffffff, or whose composite has a zero score word, is not folded; a column without a folded
// member gets 0xffffffff (no entry), one whose folded members all hold -1 is kCaseSum's -1.0f
hipError_t launch_case_fuse_eligible(const float* filtered, int G, const int32_t* case_off, const int32_t* member, int n_cases, int mode, float* fused, hipStream_t stream);
hipError_t launch_case_fuse_subjects_eligible(const unsigned long long* best, int S, const int32_t* case_off, const int32_t* member, int n_cases, int mode, float* fused, hipStream_t stream);
// afis_matrix_fuse (matrix_fuse.hip; the cell rule: matrix_fuse.h): out [n_q][columns] = the fold of the n <= 16 matrices src[k] of that shape, in argument order, with
// weights [n] (NULL: 1.0 each; kFuseSum only) under mode (kFuseSum / kFuseMax / kFuseMin, kFuseRequireAll or-ed in); normalized: the operands hold z-scores.  src and
// weights are HOST arrays: they travel in the kernel's argument segment.  Every word of out is written once; out is none of the operands
hipError_t launch_matrix_fuse(const float* const* src, const double* weights, int n, int mode, int normalized, int n_q, int columns, float* out, hipStream_t stream);
// afis_rank_hits_filtered / afis_rank_subject_hits_filtered (hit_filter.hip): filtered [n_q][G] = scores [n_q][G] with every cell whose column's label fails the row's
// masks [n_q][3] (any_of, all_of, none_of) replaced by the word 0xffffffff, which launch_rank_hits never counts and launch_subject_best turns into a composite that is
// never counted; labels [templates of the resident shard], the label of position p is labels[p], or labels[d_global[p] - index_base] for a subset's matrix.  A thread
// loads its columns' labels once and walks a strip of kFilterRows rows.  The drops write the same word at (row, column) pairs of filtered, or 0 ("no entry") at
// (row, slot) pairs of best [n_q][S] after launch_subject_best; pairs [n_pairs][2] int32, resolved by the host
constexpr int kFilterRows = 8;
hipError_t launch_filter_rows(const float* scores, int n_q, int G, const unsigned long long* labels, const unsigned long long* masks, const long long* d_global, long long index_base,
                              float* filtered, hipStream_t stream);
hipError_t launch_filter_drop_cells(const int32_t* pairs, size_t n_pairs, float* filtered, int n_q, int G, hipStream_t stream);
hipError_t launch_filter_drop_subjects(const int32_t* pairs, size_t n_pairs, unsigned long long* best, int n_q, int S, hipStream_t stream);
// what the row-walking launchers of case_fuse.hip, hit_filter.hip and eligible_expand.hip share: a thread takes four adjacent columns as one 16-byte word where every row of both matrices
// starts on a 16-byte boundary, and a grid's second dimension holds 65 535 blocks (what lies beyond is walked in a loop; their one-dimensional grids stop there too)
inline bool rows_take_16_bytes(int G, const void* a, const void* b) { return G % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }
inline unsigned grid_clamp(size_t n) { return n < 65535 ? (unsigned)n : 65535u; }
// afis_search_eligible (eligible_expand.hip): the rows cls [n_c][m] of one class of queries — scored against the m eligible templates of the shard only, in ascending
// index — expanded into the class's rows of the combined matrix: out[row_of[r]][t] = inv[t] >= 0 ? cls[r][inv[t]] : 0xffffffff for every t < G, every word of those rows
// written once; inv [G] int32 (position in the sub-shard or -1), NULL = identity (m == G); m == 0: cls and inv are not read.  Rows row_of does not name stay untouched
hipError_t launch_expand_rows(const float* cls, int n_c, int m, const int32_t* inv, const int32_t* row_of, int n_q, int G, float* out, hipStream_t stream);
// afis_search_weighted (template_fold.hip): the per-part scores parts [n_pseudo][G][4] of one batch of queries, scored as pseudo-queries, folded into the batch's rows
// out [nq][G]: qd [nq][4] int32 = (first pseudo-query, pseudo-queries n_pq, of which carry a texture template n_at <= n_pq, status: != 0 = no active template),
// w [n_pseudo][4] the weights aligned to the part slots (0 = the slot is not summed); out[q][g] = -1 where status != 0 or empty[g], else the fp64 sum of weight x part
// over slots 0..2 of the query's pseudo-queries in order, then over slot 3 of its first n_at, converted once.  Every word of out is written once
hipError_t launch_fold_templates(const float* parts, const int32_t* qd, const float* w, const uint8_t* empty, int nq, int G, float* out, hipStream_t stream);
// afis_score_print_pairs (template_fold.hip): the fold of n_pairs pair slots whose latent side is a print's view — parts [n_pairs][4] (16-byte aligned; slot 0 the
// minutiae template's part, slot 3 the texture template's), w [n_pairs][2] (8-byte aligned) the slot's weights (w_minu, w_tex), zero = not active: score[p] = -1 where
// neither is active, else (float) of the fp64 sum w_minu x parts[p][0] then w_tex x parts[p][3] over the active ones; +0.0f is stored over an inactive part
hipError_t launch_fold_print_pairs(float* parts, const float* w, size_t n_pairs, float* score, hipStream_t stream);
// afis_search_prints (print_queries.hip): the arrays of a query group — q's lm_xy, lm_ori, lm_des, lm_frag, lt_xy, lt_ori, lt_des, allocated, the 4-byte ones in whole
// 16-byte words — filled from the resident shard g on the device.  q's tables are on the device already: pseudo-query p is a print whose minutiae template fills slot 0
// (entry 3 p of lm_off / lm_tile_off; entries 3 p + 1, 3 p + 2 are empty ranges) and whose texture template fills lt_off's entry p.  first_minu / first_tile / first_tex
// [q.nq] (device): where p's print starts in g.minu_*, in g.minu_frag (tiles) and in g.tex_*; n_lm / n_lm_tiles / n_lt: the last entries of the three CSRs.  Segment
// copies, the fragment tiles as they stand, and lt_des decoded from g.tex_codes through the fp32 codebook [16][256][6]; every output word written once
hipError_t launch_print_queries(const GalleryDev& g, const float* codewords, const int32_t* first_minu, const int32_t* first_tile, const int32_t* first_tex,
                                const QueryDev& q, int n_lm, int n_lm_tiles, int n_lt, hipStream_t stream);
// afis_rank_positions / afis_rank_subject_positions / afis_count_before (rank_position.hip): where named targets stand in the list launch_rank_hits would make of a
// row at thr = kPosFloor, the ordered word of -inf.  The host resolves a target to (row, position) and sorts the targets into a CSR by row: rows [n_rows] the rows that
// have targets, off [n_rows + 1] their ranges in the target arrays [m].
// launch_position_targets  mode 0: position = a column of scores [n_q][G] -> comp (the target's composite; ~0 for a target that is no entry), count = 0, status
//                          (kPosListed / kPosNoEntry), score (the cell's own bits, -inf for no entry).  mode 1: position = a slot of best [n_q][S] as launch_subject_best
//                          (and the drops) left it, scores the matrix it was made of -> the same and best_idx (global index of the slot's best template, -1).  mode 2
//                          (afis_count_before): comp is the host's, position the column the hypothetical entry's index names or -1 -> count = -1 where that column's
//                          own composite exceeds comp (the hot pass counts it, and it must not count), else 0.
// launch_count_before      count[t] += the entries of the target's row whose composite exceeds comp[t]: the columns of scores [n_q][n] (best == NULL; composites of
//                          rank_key and position, k_topk's order) or the slots of best [n_q][n] (composite_at(b, slot), 0 skipped).  Integer adds only.
//                          max_row_targets: the longest range of off — how many workgroups share a row's targets.
constexpr int kPosListed = 0, kPosNoEntry = 1;          // AFIS_POS_LISTED, AFIS_POS_NO_ENTRY
constexpr uint32_t kPosFloor = 0x007fffffu;             // rank_key(-inf) == ordered_word(-inf): an entry's word reaches it
constexpr int kPosLoads = 4, kPosTargetChunk = 64;      // k_count_before: loads in flight per thread; targets staged in LDS at a time
constexpr int kPosChunkScalar = 256 * kPosLoads, kPosChunkVec = 4 * kPosChunkScalar;   // columns per workgroup: 1024, or 4096 where a thread takes 16 bytes per load
hipError_t launch_position_targets(int mode, const float* scores, int G, const unsigned long long* best, int S, const int32_t* row, const int32_t* pos, size_t m,
                                   const long long* d_global, long long index_base, unsigned long long* comp, unsigned long long* count, int32_t* status, float* score,
                                   long long* best_idx, hipStream_t stream);
hipError_t launch_count_before(const float* scores, const unsigned long long* best, int n, const int32_t* rows, const int32_t* off, int n_rows, int max_row_targets,
                               const unsigned long long* comp, unsigned long long* count, hipStream_t stream);
// Cohort statistics and z-normalised scores (score_stats.hip; the definitions: score_stats.h).
// launch_score_stats       axis 0: per row of matrix [n_q][G] one statistic -> out [n_q] (48 bytes each, afis_score_stat's layout) through the limb table tab
//                          [n_q][9] uint64, which the launcher zeroes: a workgroup takes kSsChunkScalar adjacent columns of a row, kSsChunkVec where rows take 16-byte
//                          loads, and adds its sums to the row's words with integer atomics.  axis 1: per column -> out [G]; tab is not used
// launch_normalize_scores  out[q][t] = the normalised cell of scores[q][t] with pair[q] (axis 0) or pair[t] (axis 1), pair = (offset, scale) as two doubles on a
//                          16-byte boundary; out != scores
constexpr int kSsChunkScalar = 1024, kSsChunkVec = 4096;
hipError_t launch_score_stats(int axis, const float* matrix, int n_q, int G, unsigned long long* tab, void* out, hipStream_t stream);
hipError_t launch_normalize_scores(int axis, const float* scores, int n_q, int G, const double* pair, float* out, hipStream_t stream);
// Score distributions (score_hist.hip; the definitions: score_hist.h).
// launch_score_hist        per row of matrix [rows][cols] the histogram of its entries under edge_keys [n_edges] (device; ascending rank keys) -> tab [rows][n_edges + 1]
//                          uint64, which the launcher zeroes: a workgroup takes kShChunkScalar adjacent columns of a row, kShChunkVec where rows take 16-byte loads, and
//                          adds its non-zero bins to the row's with integer atomics.  Columns: the same launcher over launch_transpose_scores' output
// launch_entries_at        the entry at rank remain[t] of row row[t], for m targets sorted into a CSR by row (rows [n_rows], off [n_rows + 1], as launch_count_before's;
//                          max_row_targets: the longest range of off): a radix select over the row's composites, 4 + select_position_digits(n) passes of a counting
//                          kernel (tab [m][256] uint64, zeroed per pass; a row's targets pass through LDS kSelTargetChunk at a time) and a step kernel that fixes
//                          one byte of prefix [m] and reduces remain [m] (~0: the rank is not below the row's entries) -> idx (index_base + position, or
//                          d_global[position]; -1), score (the cell's own bits; -inf), status (kPosListed / kPosNoEntry).  A row's targets stand in ascending
//                          rank, first [m] is off of the target's row: targets of one chunk with the same fixed digits share one count.  prefix comes in with the
//                          skipped position bytes set, remain with the ranks; both are left changed, and prefix_spare [m] is the step kernel's other copy
constexpr int kShChunkScalar = 256, kShChunkVec = 1024;      // k_score_hist_rows: columns per workgroup, one column per thread or four where a thread takes 16 bytes
constexpr int kSelChunkScalar = 1024, kSelChunkVec = 4096;   // k_select_count: four loads per thread
constexpr int kSelTargetChunk = 16;                     // k_select_count: targets staged in LDS at a time (256 bins x 4 bytes each: 16 KB)
hipError_t launch_score_hist(const float* matrix, int rows, int cols, const uint32_t* edge_keys, int n_edges, unsigned long long* tab, hipStream_t stream);
hipError_t launch_entries_at(const float* scores, int n, const int32_t* rows, const int32_t* off, int n_rows, int max_row_targets, const int32_t* row, const int32_t* first, size_t m,
                             unsigned long long* prefix, unsigned long long* prefix_spare, unsigned long long* remain, unsigned long long* tab, const long long* d_global, long long index_base,
                             long long* idx, float* score, int32_t* status, hipStream_t stream);
// Person distributions (score_hist.hip, score_stats.hip; the person cell: score_cell.h): the launchers above over persons instead of templates.
// launch_subject_keys      best [n_q][S] as launch_subject_best (and the drops behind it) left it -> keys [n_q][S], the composites' high halves: the person cells
// launch_subject_stats     launch_score_stats over keys [n_q][S]: a cell stands for the score word whose ordered word it is
// launch_subject_hist      launch_score_hist over keys [rows][cols] (or their transposition); edge_keys are ordered words, and a cell is its own key
// launch_subject_entries_at  launch_entries_at over keys [n_q][S], a position being a slot -> id (ids[slot]; -1), score (the bits of the person's best cell; -inf),
//                          best_idx (the position in the low half of best [n_q][S], named index_base + position or d_global[position]; -1), status
hipError_t launch_subject_keys(const unsigned long long* best, int n_q, int S, uint32_t* keys, hipStream_t stream);
hipError_t launch_subject_stats(int axis, const uint32_t* keys, int n_q, int S, unsigned long long* tab, void* out, hipStream_t stream);
hipError_t launch_subject_hist(const uint32_t* keys, int rows, int cols, const uint32_t* edge_keys, int n_edges, unsigned long long* tab, hipStream_t stream);
hipError_t launch_subject_entries_at(const uint32_t* keys, const unsigned long long* best, int S, int G, const int32_t* rows, const int32_t* off, int n_rows, int max_row_targets,
                                     const int32_t* row, const int32_t* first, size_t m, unsigned long long* prefix, unsigned long long* prefix_spare, unsigned long long* remain,
                                     unsigned long long* tab, const long long* ids, const long long* d_global, long long index_base, long long* id, float* score, long long* best_idx,
                                     int32_t* status, hipStream_t stream);
// Link groups (link_groups.hip; the definitions: link_groups.h).
// launch_link_groups       the connected components of the graph the cells of matrix [n_q][G] that reach scan.thr make of rows and columns: k_link_init, in the subject
//                          form's mutual mode (n_first = the handle's slots > 0) the first column of every person (first_col [n_first]) and from it col_of_row_out
//                          [n_q] — the array scan.col_of_row names —, k_link_scan (the one pass over the matrix: a workgroup takes kLinkChunkScalar adjacent columns of a
//                          strip of kFilterRows rows, kLinkChunkVec where rows take 16-byte loads; it counts the edges into *scan.n_edges and unites their nodes in
//                          scan.parent), then, behind the kernel boundary, k_link_flatten (label [n_nodes], size [n_nodes]) and k_link_compact: the (node, label) pairs
//                          of the nodes in groups of two or more -> out_pairs [n_nodes][2] at most, *n_pairs how many.  The caller zeroes *scan.n_edges, *scan.err and *n_pairs.
struct LinkScan {
    uint32_t thr;                         // rank_key(min_score)
    int32_t n_nodes;
    const int32_t* row_node;              // [n_q] the node of a row
    const int32_t* first_row;             // [n_nodes] mutual mode: the first row whose node this is, -1: none; NULL: any mode
    const int32_t* col_of_row;            // [n_q] mutual mode: the column of the row's print, -1: none
    const int32_t* slot_of;               // the subject form: the slot of a template of the resident shard (afis_subjects::d_slot_of); NULL: a column's node is its position
    const long long* d_global;            // ... of column p: template d_global[p] - index_base (a subset's matrix), NULL: template p
    long long index_base;
    const u64* excl; size_t n_excl;       // the subject form: the excluded (row << 32 | slot) keys, ascending
    int32_t* parent;                      // [n_nodes]
    u64* n_edges; uint32_t* err;          // the cells that are edges; != 0: a step bound was reached (the union did not settle)
};
constexpr int kLinkChunkScalar = 256, kLinkChunkVec = 1024;   // k_link_scan: columns per workgroup, one column per thread or four where a thread takes 16 bytes
hipError_t launch_link_groups(const float* matrix, int n_q, int G, const LinkScan& scan, int32_t* label, int32_t* size, int32_t* first_col, int32_t n_first, int32_t* col_of_row_out,
                              uint32_t* n_pairs, int32_t* out_pairs, hipStream_t stream);
hipError_t read_phase_cycles(unsigned long long* out32, bool reset);
hipError_t read_graph_phase_cycles(unsigned long long* out16, bool reset);

// debug tap: the angle stage's atan2 on the integer grid [-R, R]^2, out[(dy + R) * (2R + 1) + (dx + R)] (device pointer)
hipError_t launch_debug_atan2_grid(int R, float* out, hipStream_t stream);
hipError_t launch_debug_graph_arith(unsigned long long* cnt8, hipStream_t stream);
// debug tap: LUT in the reference layout [n][16][256]
hipError_t launch_lut_reference_layout(const float* des, int n, const float* codewords, float* out, hipStream_t stream);

// afis_search_prints_cascade (afis_print_cascade.cpp, print_cascade.hip): resident prints as queries, the minutiae scorer for every cell, the texture scorer for the
// `keep` best columns of every query.  A query with something active is one pseudo-query of the temporary handle: q_row [n_q] is its row of parts [n_pseudo][G][4] (-1:
// none), q_w [n_q][2] (8-byte aligned) its weights (w_minu, w_tex) with a zero where the term is not active.
// launch_print_cascade_stage1: m [n_q][G] = -1.0f where column g is empty, q_row[q] < 0 or q_w[q][0] == 0, else (float)(+0.0 + (double)w_minu x (double)parts[row][g][0])
// (print_fold.h); every word written once.  launch_print_cascade_gather: launch_cascade_gather's tables for the queries whose slot range (q_slot) is not empty, the
// pair's query being q_row[q] - piece_p0[piece] (piece_p0 [n_pieces]: the first pseudo-query of the piece's launch group); no parts are copied.
// launch_print_cascade_finish: for every kept (q, t) the cell's word -> out[q][t] and (v_m, v_t) -> kept_parts[q][rank] ([n_q][keep][2], 8-byte aligned, zeroed by the
// caller): v_m = parts[row][t][0] where the minutiae term is active, v_t = pair_parts[slot][3] where the texture term is; -1.0f and +0.0f twice for an empty column or a
// query with nothing active; nothing else of out is written.
hipError_t launch_print_cascade_stage1(const float* parts, const int32_t* q_row, const float* q_w, const uint8_t* empty, int n_q, int G, float* m, hipStream_t stream);
hipError_t launch_print_cascade_gather(int n_q, int G, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot, const int32_t* piece_first,
                                       int n_pieces, const int32_t* piece_p0, const int32_t* q_row, int32_t* tab, hipStream_t stream);
hipError_t launch_print_cascade_finish(int n_q, int G, int keep, int n_kept, long long index_base, const long long* kept, const int32_t* q_slot, const int32_t* q_row,
                                       const float* q_w, const uint8_t* empty, const float* parts, const float* pair_parts, float* out, float* kept_parts, hipStream_t stream);

}  // namespace afis
