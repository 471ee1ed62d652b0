// print_queries.hip — device code of the print search (afis_prints.cpp: afis_search_prints): resident prints become the queries of a launch group without leaving the
// device.  Everything a QueryGroup's arrays hold is made here from the resident shard's own arrays (GalleryDev), driven by small host-made tables: per pseudo-query the
// first minutia, first fragment tile and first texture point of its print in the shard, and the destination CSRs the scorers read (lm_off, lm_tile_off, lt_off).
//
//   lm_xy, lm_ori, lt_xy, lt_ori   segment copies of minu_xy / minu_ori / tex_xy / tex_ori (4 bytes per point)
//   lm_des                         segment copies of minu_des (384 bytes per minutia)
//   lm_frag                        the print's minu_frag tiles as they stand (6 144 bytes per tile of 16 descriptors): the two layouts are one (afis_device.h), so the
//                                  zero rows that pad a template's last tile come along
//   lt_des                         tex_codes decoded through the fp32 codebook: des[r][6 m + k] = codewords[m][code[r][m]][k], the bits copied
//
// A pseudo-query has three minutiae slots; a print fills slot 0, slots 1 and 2 are empty ranges of the CSRs (entry 3 p + s), and a search finds the entry that owns an
// output element as the largest e with off[e] <= element — the empty entries before it share its offset and lose (gallery_subset.hip's rule).
//
// Work is spread over OUTPUT words: a thread owns one 16-byte word of an output array — four points of a 4-byte array, one of the 24 float4 of a descriptor row, one of
// the 384 of a tile — finds its owner by binary search over the CSR (at most 3 x 128 + 1 entries, L1-resident) and stores once, so a wave's stores are 1 KB contiguous,
// every output word is written exactly once (no memset, no atomics), and the 4-byte arrays, whose segments start at any multiple of 4 bytes on either side, pay with
// 4-byte loads only.  Their last word may reach past the last point: the arrays are allocated in whole 16-byte words and the padding gets zeros.
//
// The decode.  A texture row is 96 floats = 24 float4; float4 j holds floats 4 j .. 4 j + 3 and sub-quantizer m owns floats 6 m .. 6 m + 5, so a float4 spans at most
// two codewords and always consists of two aligned 8-byte halves of codewords: (j % 3 == 0) floats 0-1 and 2-3 of codeword m0 = 4 j / 6, (1) floats 4-5 of m0 and 0-1 of
// m0 + 1, (2) floats 2-3 and 4-5 of m0.  A thread reads its two code bytes, then the two halves — a select on j % 3, no loop over the floats — and stores 16 bytes.
// The codebook (96 KB) is read through L2, not staged in LDS: in LDS it would hold a CU to one workgroup, while every one of the 4 096 codewords is re-read
// thousands of times by a launch and stays cache-resident; with no LDS and a few registers the kernels keep full occupancy, which is what a copy wants.
//
// Every index into the arrays is a size_t.  The grids are one-dimensional and stop at 65 535 workgroups; what lies beyond is walked in a loop.
#include "afis_device.h"

namespace afis {

constexpr int kPqThreads = 256;

// the entry that owns element p: the largest e in [0, n_ent) with off[e] <= p (off[0] == 0 <= p is given)
__device__ __forceinline__ int pq_owner_of(const int32_t* __restrict__ off, int n_ent, int p)
{
    int lo = 0, hi = n_ent - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// 4-byte arrays: dst[off[e] + i] = src[first[e / per] + i].  n = off[n_ent] points; the store of the last 16-byte word zero-fills up to three points of padding
__global__ __launch_bounds__(kPqThreads) void k_pq_copy_points(const uint32_t* __restrict__ src, uint4* __restrict__ dst, const int32_t* __restrict__ first,
                                                               const int32_t* __restrict__ off, int n_ent, int per, int n)
{
    const size_t n_words = ((size_t)n + 3) / 4;
    for (size_t w = (size_t)blockIdx.x * kPqThreads + threadIdx.x; w < n_words; w += (size_t)gridDim.x * kPqThreads) {
        uint32_t v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const size_t p = w * 4 + c;
            v[c] = 0u;
            if (p < (size_t)n) {
                const int e = pq_owner_of(off, n_ent, (int)p);
                v[c] = src[(size_t)first[e / per] + (p - (size_t)off[e])];
            }
        }
        dst[w] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// elements of UPP 16-byte words (a descriptor row: 24; a fragment tile: 384): dst[off[e] + i] = src[first[e / per] + i], n = off[n_ent] elements
template <int UPP>
__global__ __launch_bounds__(kPqThreads) void k_pq_copy_units(const uint4* __restrict__ src, uint4* __restrict__ dst, const int32_t* __restrict__ first,
                                                              const int32_t* __restrict__ off, int n_ent, int per, int n)
{
    const size_t n_units = (size_t)n * UPP;
    for (size_t u = (size_t)blockIdx.x * kPqThreads + threadIdx.x; u < n_units; u += (size_t)gridDim.x * kPqThreads) {
        const size_t i = u / UPP, w = u - i * UPP;
        const int e = pq_owner_of(off, n_ent, (int)i);
        dst[u] = src[((size_t)first[e / per] + (i - (size_t)off[e])) * UPP + w];
    }
}

// lt_des[off[p] + i][4 j .. 4 j + 3] from the codes of texture point first[p] + i: codes [points][16] bytes, cw2 = the codebook [16][256][3] as 8-byte halves
__global__ __launch_bounds__(kPqThreads) void k_pq_decode_texture(const uint8_t* __restrict__ codes, const uint2* __restrict__ cw2, uint4* __restrict__ dst,
                                                                  const int32_t* __restrict__ first, const int32_t* __restrict__ off, int n_ent, int n)
{
    constexpr int kRowUnits = kDes / 4;                                     // 24
    static_assert(kDsub == 6 && kDes == kM * kDsub && kM == 16, "a float4 of a row is two 8-byte halves of at most two codewords");
    const size_t n_units = (size_t)n * kRowUnits;
    for (size_t u = (size_t)blockIdx.x * kPqThreads + threadIdx.x; u < n_units; u += (size_t)gridDim.x * kPqThreads) {
        const size_t i = u / kRowUnits;
        const int j = (int)(u - i * kRowUnits);
        const int p = pq_owner_of(off, n_ent, (int)i);
        const size_t pt = (size_t)first[p] + (i - (size_t)off[p]);
        const int r = j % 3, m0 = (4 * j) / kDsub;
        const int m_a = m0, m_b = r == 1 ? m0 + 1 : m0;                     // m_b <= 15: j = 22 is the last with r == 1, m0 = 14
        const int h_a = r == 0 ? 0 : r == 1 ? 2 : 1, h_b = r == 0 ? 1 : r == 1 ? 0 : 2;
        const uint32_t c_a = codes[pt * kM + m_a], c_b = codes[pt * kM + m_b];
        const uint2 a = cw2[((size_t)m_a * kK + c_a) * 3 + h_a], b = cw2[((size_t)m_b * kK + c_b) * 3 + h_b];
        dst[u] = make_uint4(a.x, a.y, b.x, b.y);
    }
}

static unsigned pq_grid(size_t n_units) { return grid_clamp((n_units + kPqThreads - 1) / kPqThreads); }

// q: a group's QueryDev whose seven tables (lm_off, lm_tile_off, lt_off, tile_off, tile16_off, tex_slot, status) are on the device already and whose seven arrays are
// allocated — the 4-byte ones in whole 16-byte words — and are filled here.  first_minu / first_tile / first_tex [q.nq]: where pseudo-query p's print starts in
// g.minu_* / g.minu_frag (tiles) / g.tex_* (read only where p's range of the CSR is not empty).  n_lm / n_lm_tiles / n_lt: the last entries of the three CSRs, which
// the host has made from the shard's own counts: every source element lies inside its print.
hipError_t launch_print_queries(const GalleryDev& g, const float* codewords, const int32_t* first_minu, const int32_t* first_tile, const int32_t* first_tex,
                                const QueryDev& q, int n_lm, int n_lm_tiles, int n_lt, hipStream_t stream)
{
    if (q.nq <= 0) return hipSuccess;
    if (q.nq > 0x7fffffff / 3 - 1 || n_lm < 0 || n_lm_tiles < 0 || n_lt < 0 || !first_minu || !first_tile || !first_tex || !q.lm_off || !q.lm_tile_off || !q.lt_off) return hipErrorInvalidValue;
    const int n_ent3 = 3 * q.nq;
    if (n_lm > 0) {
        if (!g.minu_xy || !g.minu_ori || !g.minu_des || !q.lm_xy || !q.lm_ori || !q.lm_des) return hipErrorInvalidValue;
        const dim3 gp(pq_grid(((size_t)n_lm + 3) / 4));
        hipLaunchKernelGGL(k_pq_copy_points, gp, dim3(kPqThreads), 0, stream, (const uint32_t*)g.minu_xy, (uint4*)q.lm_xy, first_minu, q.lm_off, n_ent3, 3, n_lm);
        hipLaunchKernelGGL(k_pq_copy_points, gp, dim3(kPqThreads), 0, stream, (const uint32_t*)g.minu_ori, (uint4*)q.lm_ori, first_minu, q.lm_off, n_ent3, 3, n_lm);
        hipLaunchKernelGGL((k_pq_copy_units<kDes / 4>), dim3(pq_grid((size_t)n_lm * (kDes / 4))), dim3(kPqThreads), 0, stream, (const uint4*)g.minu_des, (uint4*)q.lm_des,
                           first_minu, q.lm_off, n_ent3, 3, n_lm);
    }
    if (n_lm_tiles > 0) {
        if (!g.minu_frag || !q.lm_frag) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_pq_copy_units<6 * 64>), dim3(pq_grid((size_t)n_lm_tiles * (6 * 64))), dim3(kPqThreads), 0, stream, (const uint4*)g.minu_frag, (uint4*)q.lm_frag,
                           first_tile, q.lm_tile_off, n_ent3, 3, n_lm_tiles);
    }
    if (n_lt > 0) {
        if (!g.tex_xy || !g.tex_ori || !g.tex_codes || !codewords || !q.lt_xy || !q.lt_ori || !q.lt_des) return hipErrorInvalidValue;
        const dim3 gp(pq_grid(((size_t)n_lt + 3) / 4));
        hipLaunchKernelGGL(k_pq_copy_points, gp, dim3(kPqThreads), 0, stream, (const uint32_t*)g.tex_xy, (uint4*)q.lt_xy, first_tex, q.lt_off, q.nq, 1, n_lt);
        hipLaunchKernelGGL(k_pq_copy_points, gp, dim3(kPqThreads), 0, stream, (const uint32_t*)g.tex_ori, (uint4*)q.lt_ori, first_tex, q.lt_off, q.nq, 1, n_lt);
        hipLaunchKernelGGL(k_pq_decode_texture, dim3(pq_grid((size_t)n_lt * (kDes / 4))), dim3(kPqThreads), 0, stream, (const uint8_t*)g.tex_codes, (const uint2*)codewords,
                           (uint4*)q.lt_des, first_tex, q.lt_off, q.nq, n_lt);
    }
    return hipGetLastError();
}

}  // namespace afis
