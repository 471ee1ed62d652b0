// gallery_subset.hip — device code of the subset search (afis_subset.cpp): a candidate list of the resident shard is gathered into a sub-shard of its own, device to
// device, and a search over it hands its results back under the caller's indices.
//
// k_gather_ranges: the SoA arrays of the resident shard are CSR ranges per template; template t of the OUTPUT takes the range src_off[sel[t]] .. of the source array and
// lands at dst_off[t].  The source ranges come in no particular order and may be empty.  The kernel keeps what k_compact_ranges (gallery_edit.hip) documents: work is
// spread over OUTPUT POINTS, not templates — a workgroup owns kPts consecutive points of the new array, whatever templates they belong to (a 2 000-minutiae template is
// 32 workgroups of the descriptor copy, a run of 1-point templates is one); two threads find the templates of the span's first and last point by binary search over
// dst_off, every point's own template is then searched between those two and its source point goes to LDS; the copy loop stores fully coalesced and loads coalesced per
// template, 16 bytes wide for the descriptors (24 units per point) and the PQ codes, 4 bytes for (x, y) and the orientations (whose ranges start at any multiple of
// 4 bytes on both sides).  Vector loads and stores only.  The launcher refuses an output of 2^31 points or more.
//
// k_subset_topk_map / k_permute_columns: the two epilogues of a subset search.  The sub-shard holds its templates in ascending global index order, so k_topk's tie rule
// (ascending position) is the rule on global indices; its positions are mapped to global indices afterwards, and the score / part columns are brought to the order the
// caller listed the indices in before they are copied to the host.
#include "afis_device.h"

namespace afis {

// the template that owns point p of the output: the largest t in [lo, hi] with off[t] <= p (empty templates before it share its offset and lose; off[lo] <= p is given)
__device__ __forceinline__ int gather_owner_of(const int32_t* __restrict__ off, int lo, int hi, int p)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <class U, int UPP, int kPts>
__global__ __launch_bounds__(256) void k_gather_ranges(const U* __restrict__ src, U* __restrict__ dst, const int32_t* __restrict__ src_off, const int32_t* __restrict__ sel,
                                                       const int32_t* __restrict__ dst_off, int n, int n_out)
{
    __shared__ int s_src[kPts];
    __shared__ int s_t[2];
    const int p0 = blockIdx.x * kPts;                                       // (n_out < 2^31: the launcher's range check)
    const int np = min(kPts, n_out - p0);
    if (np <= 0) return;
    if (threadIdx.x < 2) s_t[threadIdx.x] = gather_owner_of(dst_off, 0, n - 1, threadIdx.x ? p0 + np - 1 : p0);
    __syncthreads();
    const int t_lo = s_t[0], t_hi = s_t[1];
    for (int i = threadIdx.x; i < np; i += 256) {
        const int p = p0 + i;
        const int t = gather_owner_of(dst_off, t_lo, t_hi, p);
        s_src[i] = src_off[sel[t]] + (p - dst_off[t]);                      // < src_off[sel[t] + 1]: the output's counts are the listed templates' own
    }
    __syncthreads();
    U* const out = dst + (size_t)p0 * UPP;
    for (int e = threadIdx.x; e < np * UPP; e += 256) {
        const int i = e / UPP, w = e - i * UPP;
        out[e] = src[(size_t)s_src[i] * UPP + w];
    }
}

// elem_bytes: 384 (descriptors), 16 (PQ codes), 4 ((x, y) pairs, orientations).  src_off [G + 1], sel [n] (each in [0, G)), dst_off [n + 1] with dst_off[n] == n_out and
// dst_off[t + 1] - dst_off[t] == src_off[sel[t] + 1] - src_off[sel[t]]: device arrays the host has checked.
hipError_t launch_gather_ranges(const void* src, void* dst, int elem_bytes, const int32_t* src_off, const int32_t* sel, const int32_t* dst_off, int n, long long n_out, hipStream_t stream)
{
    if (n <= 0 || n_out <= 0) return hipSuccess;
    if (n_out > 0x7fffffffll) return hipErrorInvalidValue;
    const int m = (int)n_out;
    if (elem_bytes == kDes * 4) {
        constexpr int kPts = 64;                                            // 24 KB copied per workgroup, six 16-byte units per thread
        hipLaunchKernelGGL((k_gather_ranges<uint4, kDes * 4 / 16, kPts>), dim3((m + kPts - 1) / kPts), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, src_off, sel, dst_off, n, m);
    } else if (elem_bytes == 16) {
        constexpr int kPts = 1024;                                          // 16 KB copied per workgroup
        hipLaunchKernelGGL((k_gather_ranges<uint4, 1, kPts>), dim3((m + kPts - 1) / kPts), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, src_off, sel, dst_off, n, m);
    } else if (elem_bytes == 4) {
        constexpr int kPts = 2048;                                          // 8 KB copied per workgroup
        hipLaunchKernelGGL((k_gather_ranges<uint32_t, 1, kPts>), dim3((m + kPts - 1) / kPts), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, src_off, sel, dst_off, n, m);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

// rank-list entries of k_topk launched with index_base 0: a position of the sub-shard -> its global index; the padding (-1 where k exceeds the subset) stays
__global__ __launch_bounds__(256) void k_subset_topk_map(long long* __restrict__ idx, long long n_idx, const long long* __restrict__ map, int n_map)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_idx) return;
    const long long v = idx[i];
    if (v >= 0 && v < n_map) idx[i] = map[v];
}

hipError_t launch_subset_topk_map(long long* idx, long long n_idx, const long long* map, int n_map, hipStream_t stream)
{
    if (n_idx <= 0 || n_map <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_subset_topk_map, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, stream, idx, n_idx, map, n_map);
    return hipGetLastError();
}

// dst[q][j] = src[q][pos[j]]: stores coalesced, loads gathered inside one row of n elements (the row of a query: 0.4 MB of scores at 100k templates, L2-resident)
template <class U>
__global__ __launch_bounds__(256) void k_permute_columns(const U* __restrict__ src, U* __restrict__ dst, int n, const int32_t* __restrict__ pos)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t row = (size_t)blockIdx.y * (size_t)n;
    dst[row + j] = src[row + pos[j]];
}

hipError_t launch_permute_columns(const void* src, void* dst, int elem_bytes, int n_q, int n, const int32_t* pos, hipStream_t stream)
{
    if (n_q <= 0 || n <= 0) return hipSuccess;
    if (n_q > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)n_q);
    if (elem_bytes == 4) hipLaunchKernelGGL((k_permute_columns<uint32_t>), grid, dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, n, pos);
    else if (elem_bytes == 16) hipLaunchKernelGGL((k_permute_columns<uint4>), grid, dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, n, pos);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace afis
