// fuse_cell.h — S10, the fusion of one (latent, rolled print) cell: the ONE definition of the expression, shared by k_fuse (a search's matrix), k_fuse_pairs
// (afis_score_pairs, and the second stage of afis_search_cascade) in minu.hip and k_fuse_stage1 (the first stage of afis_search_cascade) in cascade.hip.
// final = score[0] + score[1] + score[2] + score[28] * 0.3 (matcher.cpp:188), where the reference's score vector holds the three minutiae scores at [0..2] and the
// texture score at index (#latent minutiae templates): with fewer than three minutiae templates the texture score takes the slot of a minutiae score.
// Device code only (every unit that includes it is built with -ffp-contract=off).
#pragma once
#include "afis_device.h"

namespace afis {

// the fused score of cell (latent qi, template gi) from its three minutiae parts p[0..2] and the texture score tex (a search: p[3]; a first stage that has not run
// the texture scorer: +0.0f, so that the slot the texture would occupy contributes zero)
__device__ __forceinline__ float fuse_cell(const QueryDev& q, const GalleryDev& g, int qi, int gi, const float* __restrict__ p, float tex)
{
    if (q.status[qi] != 0 || g.empty[gi]) return -1.0f;                         // :145, :181-187
    const int slot = q.tex_slot[qi];
    const float a0 = slot == 0 ? tex : p[0];
    const float a1 = slot == 1 ? tex : p[1];
    const float a2 = slot == 2 ? tex : p[2];
    const float a28 = slot == 28 ? tex : 0.0f;
    float f = a0 + a1;
    f = f + a2;
    return (float)((double)f + (double)a28 * 0.3);
}

}  // namespace afis
