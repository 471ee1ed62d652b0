// pair_evidence.hip — device code of the evidence calls of a pair list (afis_evidence.cpp: afis_texture_correspondences_pairs, afis_pair_alignments and their forms for
// resident print pairs): what the chunk's list launches left on the device — the three minutiae scorers' survivors as (lx, ly, rx, ry) (k_graph_minutiae's corr_out /
// corr_n, slot 3 p + s) and the texture scorer's as (similarity, latent row, print point) in the reference's list order (k_graph_texture's tap after S9, slot p) — becomes
// what the caller asked for, before anything crosses the bus:
//   the texture export   of pair p: count = the tap's count (-1: the scorer did not run), part = parts[4 p + 3], and per survivor t the block coordinates gathered from the
//                        templates (QueryDev::lt_xy, GalleryDev::tex_xy at the tap's indices), the indices themselves and the similarity's bits; rows at or beyond the
//                        count are zeros, so that the copy back is final
//   the moments          of pair p: four records (pair_moments.h: scorers 0, 1, 2 in pixels as stored, the texture scorer at 16 b + 24), exact integers
// One wave64 per pair, four pairs to a workgroup; a pair's lists are at most 120 and 200 entries, so a lane holds at most 2 + 4 of them.  The lanes stride the lists with
// coalesced 8-byte loads, gather the texture points' 4-byte coordinates, and add into int64 registers; a record's nine words are then summed across the wave with a
// butterfly of __shfl_xor — six steps of two 32-bit exchanges per word, no LDS, every lane ends with the total — and lane 0 writes the 72 bytes with ordinary stores.  The
// sums are integers: the order of the additions cannot matter.  The pair table's words and the counts are uniform over the wave (scalar loads).  No word is written by two
// waves, nothing is read that another wave of the launch writes, no atomics.  Every index is a size_t.  The time is a few microseconds a chunk beside the list launches'
// milliseconds: nothing here is tuned.
#include "afis_device.h"
#include "pair_moments.h"

namespace afis {

constexpr int kEvidenceWaves = 4;

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += (int64_t)__shfl_xor((long long)v, m, 64);
    return v;
}

__device__ __forceinline__ CorrMoments wave_sum(const CorrMoments& m)
{
    return CorrMoments{wave_sum(m.n), wave_sum(m.slx), wave_sum(m.sly), wave_sum(m.srx), wave_sum(m.sry), wave_sum(m.dot), wave_sum(m.cross), wave_sum(m.ll), wave_sum(m.rr)};
}

__global__ __launch_bounds__(kEvidenceWaves * 64) void k_pair_evidence(QueryDev q, GalleryDev g, const int32_t* __restrict__ tab, PairEvidence e)
{
    const int lane = threadIdx.x & 63;
    const int n_pairs = tab[0];
    const size_t stride = (size_t)gridDim.x * kEvidenceWaves;
    for (size_t p = (size_t)blockIdx.x * kEvidenceWaves + (threadIdx.x >> 6); p < (size_t)n_pairs; p += stride) {
        const int qi = tab[1 + 2 * p], gi = tab[2 + 2 * p];
        const int l0 = q.lt_off[qi], n_lt = q.lt_off[qi + 1] - l0;
        const int r0 = g.tex_off[gi], n_rt = g.tex_off[gi + 1] - r0;
        const int n_raw = e.tap_n[p];
        const int n_tex = min(max(n_raw, 0), kTopTex);
        if (e.mom) {
#pragma unroll 1
            for (int s = 0; s < 3; ++s) {                                   // the minutiae scorers: pixels as stored
                const int n = min(max(e.corr_n[3 * p + s], 0), kTopMinu);
                const short4* __restrict__ c = e.corr + (3 * p + s) * kTopMinu;
                CorrMoments m{0, 0, 0, 0, 0, 0, 0, 0, 0};
                for (int t = lane; t < n; t += 64) { const short4 v = c[t]; mom_point(m, v.x, v.y, v.z, v.w); }
                m = wave_sum(m);
                if (lane == 0) e.mom[4 * p + s] = m;
            }
        }
        CorrMoments m{0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int t = lane; t < kTopTex; t += 64) {                          // the texture scorer: the tap's indices -> the templates' block coordinates
            short4 xy = make_short4(0, 0, 0, 0); short2 pt = make_short2(0, 0); float sim = 0.0f;
            if (t < n_tex) {
                const MinuCand c = e.tap[p * kTopTex + t];
                if ((unsigned)c.li < (unsigned)n_lt && (unsigned)c.ri < (unsigned)n_rt) {     // (the list kernel's indices always are)
                    const short2 l = q.lt_xy[l0 + c.li], r = g.tex_xy[r0 + c.ri];
                    xy = make_short4(l.x, l.y, r.x, r.y); pt = make_short2(c.li, c.ri); sim = c.sim;
                    mom_point(m, mom_texture_px(l.x), mom_texture_px(l.y), mom_texture_px(r.x), mom_texture_px(r.y));
                }
            }
            if (e.ex_xy) {
                e.ex_xy[p * kTopTex + t] = xy;
                if (e.ex_pt) e.ex_pt[p * kTopTex + t] = pt;
                if (e.ex_sim) e.ex_sim[p * kTopTex + t] = sim;
            }
        }
        if (e.mom) { m = wave_sum(m); if (lane == 0) e.mom[4 * p + 3] = m; }
        if (e.ex_n && lane == 0) { e.ex_n[p] = n_raw < 0 ? -1 : n_tex; e.ex_part[p] = n_raw < 0 ? 0.0f : e.parts[4 * p + 3]; }
    }
}

hipError_t launch_pair_evidence(const QueryDev& q, const GalleryDev& g, const int32_t* pair_tab, int n_pairs, const PairEvidence& e, hipStream_t stream)
{
    if (n_pairs <= 0) return hipSuccess;
    if (!pair_tab || !e.tap || !e.tap_n || !e.parts || (e.mom && (!e.corr || !e.corr_n)) || (!e.mom && !e.ex_xy) || (e.ex_xy && (!e.ex_n || !e.ex_part))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pair_evidence, dim3(grid_clamp(((size_t)n_pairs + kEvidenceWaves - 1) / kEvidenceWaves)), dim3(kEvidenceWaves * 64), 0, stream, q, g, pair_tab, e);
    return hipGetLastError();
}

}  // namespace afis
