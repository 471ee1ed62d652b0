// adc_pairs.hip — S4-S6 of afis_score_pairs: the EXACT texture row maxima of a TABLE of (latent, rolled print) pairs, evaluated entry by entry with no bound pass.
// A product kernel (libafis_hip.so), modelled on the direct kernel of adc_direct.hip (variant 0: the plain LDS gather), which stays a test-library kernel.
//
// Reference: LatentTextureTemplate::compute_dist_to_codewords (matching/include.h:327-359), Matcher::One2One_texture_matching method 1 and the row arg-max
// (matching/matcher.cpp:563-595, :723-735).  S5 is fp32 add / sub only: with the reference's four chains kept — chain c starts from 6 / 0 / 0 / 0 and subtracts the
// entries of sub-quantizers c, c + 4, c + 8, c + 12 in that order, the chains meet as (d0 + d1) + (d2 + d3) — and contraction off (-ffp-contract=off, the Makefile's
// flags) the values are the CPU's bits, and so the search's (adc_variant 8 and 9 recompute the same entries in the same order).
//
// Work: the host sorts a launch group's pairs by latent and cuts every latent's run into segments of at most kAdcPairsSegment pairs (pair_tables.h).  One workgroup =
// (segment, tile of kTileRows = 8 latent texture rows): blockIdx.x names the segment, blockIdx.y the tile; tiles beyond the latent's rows leave at once.  The workgroup
// builds the LUT tile of its 8 rows in LDS from q.lt_des and the fp32 codewords with lut_entry() (8 x 16 x 256 fp32 = 128 KB of the CU's 160 KB: one workgroup per CU; the
// tile never goes to HBM), then every wave takes whole pairs of the segment in turn, lane <-> rolled texture point (one uint4 of 16 code bytes per point) in blocks of 64
// points, keeps a running (max, first arg-max) per row across the blocks and reduces it over the wave.  A latent with 4096 candidates is 64 segments x its tiles and fills
// the chip; a verification pair pays one LUT build per tile.
// Output, the dense form k_graph_texture reads: rm_val / rm_arg[p * q.lt_pad + row] for pair p of the table, every row < n_lt.  A pair whose latent or print has no
// texture points gets nothing written (k_graph_texture returns before reading), nor do the rows beyond n_lt of the last tile.
//
// Not tuned.  The gather of random codes from the tile is bank-conflicted by nature (64 lanes x ds_read_b128 at random 16-byte slots), and the table build is 64 entries
// per thread of plain VALU.  Whoever tunes it should look first, with rocprofv3 --pmc in a run of its own, at SQ_LDS_BANK_CONFLICT against SQ_LDS_ACTIVE (the
// gather; adc_direct.hip's variants 6 / 7 show what a conflict-free layout costs and gains), at SQ_INSTS_LDS against SQ_INSTS_VALU (the build's share: it dominates for
// segments of a few pairs), and at SQ_WAVES / GRBM_GUI_ACTIVE for how well short pair lists fill the chip.
#include "afis_device.h"
#include "adc_common.h"
#include "pair_tables.h"

namespace afis {

constexpr int kAdcPairsThreads = 512;   // 8 waves: two per SIMD

__global__ __launch_bounds__(kAdcPairsThreads) void k_adc_pairs(QueryDev q, GalleryDev g, const float* __restrict__ codewords, const int32_t* __restrict__ pair_tab,
                                                                const int32_t* __restrict__ seg, float* __restrict__ rm_val, int32_t* __restrict__ rm_arg)
{
    __shared__ float4 s_lut[kTileFloats / 4];                 // 128 KB: [row quad rq < 2][m < 16][k < 256] float4 of the quad's four rows

    const int p_first = seg[2 * blockIdx.x], n_seg_pairs = seg[2 * blockIdx.x + 1];
    const int qi = pair_tab[1 + 2 * p_first];                  // the segment's latent: every pair of it names the same one
    const int l0 = q.lt_off[qi], n_lt = q.lt_off[qi + 1] - l0;
    const int row0 = blockIdx.y * kTileRows;
    if (row0 >= n_lt) return;                                  // (uniform: before any barrier)

    // ---- S4: the tile, entry by entry.  Thread -> (m, k); rows beyond n_lt repeat the last row and are never written out
    for (int mk = threadIdx.x; mk < kM * kK; mk += kAdcPairsThreads) {
        const int m = mk >> 8;
        float cw6[kDsub];
#pragma unroll
        for (int d = 0; d < kDsub; ++d) cw6[d] = codewords[(size_t)mk * kDsub + d];
        float v[kTileRows];
#pragma unroll
        for (int r = 0; r < kTileRows; ++r) {
            const int row = min(row0 + r, n_lt - 1);
            const float* d6 = q.lt_des + (size_t)(l0 + row) * kDes + m * kDsub;
            float des6[kDsub];
#pragma unroll
            for (int d = 0; d < kDsub; ++d) des6[d] = d6[d];
            v[r] = lut_entry(des6, cw6);
        }
        s_lut[mk] = make_float4(v[0], v[1], v[2], v[3]);
        s_lut[kM * kK + mk] = make_float4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();

    constexpr int kWaves = kAdcPairsThreads / 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int j = wave; j < n_seg_pairs; j += kWaves) {
        const int p = p_first + j;
        const int gi = pair_tab[2 + 2 * p];
        const int r0 = g.tex_off[gi], n_rt = g.tex_off[gi + 1] - r0;
        if (n_rt <= 0) continue;
        float best[kTileRows], first[kTileRows];
        int bidx[kTileRows];
#pragma unroll
        for (int r = 0; r < kTileRows; ++r) { best[r] = -INFINITY; bidx[r] = 0x7fffffff; first[r] = 0.0f; }
        for (int pb = 0; pb < n_rt; pb += 64) {
            const int pt = pb + lane;
            const bool in = pt < n_rt;
            const uint4 cw = in ? g.tex_codes[r0 + pt] : make_uint4(0u, 0u, 0u, 0u);
            const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
            float acc[4][kTileRows];
#pragma unroll
            for (int r = 0; r < kTileRows; ++r) { acc[0][r] = 6.0f; acc[1][r] = 0.0f; acc[2][r] = 0.0f; acc[3][r] = 0.0f; }   // matcher.cpp:571-574
#pragma unroll
            for (int mg = 0; mg < 4; ++mg) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {                  // chain c sees m = c, c + 4, c + 8, c + 12 in this order (matcher.cpp:577-591)
                    const int m = mg * 4 + c;
                    const uint32_t code = (w[mg] >> (8 * c)) & 255u;
                    const float4 a = s_lut[m * kK + code];
                    const float4 b = s_lut[kM * kK + m * kK + code];
                    acc[c][0] -= a.x; acc[c][1] -= a.y; acc[c][2] -= a.z; acc[c][3] -= a.w;
                    acc[c][4] -= b.x; acc[c][5] -= b.y; acc[c][6] -= b.z; acc[c][7] -= b.w;
                }
            }
#pragma unroll
            for (int r = 0; r < kTileRows; ++r) {
                float s = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);                      // matcher.cpp:592
                if (pb == 0) first[r] = s;                     // (lane 0's is point 0's)
                s = in ? s : -INFINITY;                        // a point beyond n_rt never wins: -inf is not greater than the start, and its index is never taken
                if (s > best[r]) { best[r] = s; bidx[r] = pt; }
            }
        }
        // std::max_element (matcher.cpp:730): the first point's value stands until a STRICTLY greater one comes.  A NaN never compares greater, a NaN at point 0 is never
        // beaten, and a row of -inf keeps point 0 (adc_refine.hip's rule for the rows it evaluates in full)
        float outv = 0.0f; int outi = 0;
#pragma unroll
        for (int r = 0; r < kTileRows; ++r) {
            wave_argmax(best[r], bidx[r]);
            const float s0 = __shfl(first[r], 0);
            if (s0 != s0 || bidx[r] == 0x7fffffff) { best[r] = s0; bidx[r] = 0; }
            if (lane == r) { outv = best[r]; outi = bidx[r]; }
        }
        if (lane < kTileRows && row0 + lane < n_lt) {
            const size_t o = (size_t)p * q.lt_pad + row0 + lane;
            rm_val[o] = outv;
            rm_arg[o] = outi;
        }
    }
}

hipError_t launch_adc_pairs(const QueryDev& q, const GalleryDev& g, const float* codewords, const int32_t* pair_tab, const int32_t* seg, int n_seg,
                            float* rm_val, int32_t* rm_arg, hipStream_t stream)
{
    if (n_seg <= 0 || q.lt_pad <= 0) return hipSuccess;
    if (!codewords || !pair_tab || !seg || !rm_val || !rm_arg || q.lt_pad % kTileRows != 0 || q.lt_pad / kTileRows > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_adc_pairs, dim3((unsigned)n_seg, (unsigned)(q.lt_pad / kTileRows)), dim3(kAdcPairsThreads), 0, stream, q, g, codewords, pair_tab, seg, rm_val, rm_arg);
    return hipGetLastError();
}

}  // namespace afis
