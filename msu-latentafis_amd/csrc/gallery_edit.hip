// gallery_edit.hip — range compaction for afis_gallery_remove and the range splice of afis_gallery_commit_at (afis_gallery.cpp; k_splice_ranges below has its own note): the SoA arrays of the resident shard are CSR ranges per template; when templates
// leave, every surviving template's range moves from old_off[t] to new_off[t].  One kernel, instantiated per element width, copies one array into a NEW buffer
// (the host then releases the old one and goes on to the next array: the transient memory is one array).
//
// Work is spread over OUTPUT POINTS, not templates: a workgroup owns kPts consecutive points of the new array, whatever templates they belong to (a 2 000-minutiae
// template is 32 workgroups of the descriptor copy, not one).  Two threads find the templates of the span's first and last point by binary search over new_off
// (17 steps at 100 000 templates); every point's own template is then searched between those two — one or two steps, a span rarely touches more than two templates —
// and its source point goes to LDS.  The copy loop that follows is fully coalesced on the store side and coalesced per template on the load side: lane i stores
// unit p0 * UPP + i, 16 bytes wide for the descriptors (24 units per point) and the PQ codes (1 unit), 4 bytes for (x, y) and the orientations (whose ranges
// start at any multiple of 4 bytes on both sides, so nothing wider is aligned).  Vector loads and stores only.
#include "afis_device.h"

namespace afis {

// the template that owns point p of the new array: the largest t in [lo, hi] with off[t] <= p (empty templates before it share its offset and lose; off[lo] <= p is given)
__device__ __forceinline__ int owner_of(const int32_t* __restrict__ off, int lo, int hi, int p)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <class U, int UPP, int kPts>
__global__ __launch_bounds__(256) void k_compact_ranges(const U* __restrict__ src, U* __restrict__ dst, const int32_t* __restrict__ old_off, const int32_t* __restrict__ new_off,
                                                        int G, int n_new)
{
    __shared__ int s_src[kPts];
    __shared__ int s_t[2];
    const int p0 = blockIdx.x * kPts;                                       // (n_new < 2^31: the commit's range check)
    const int np = min(kPts, n_new - p0);
    if (np <= 0) return;
    if (threadIdx.x < 2) s_t[threadIdx.x] = owner_of(new_off, 0, G - 1, threadIdx.x ? p0 + np - 1 : p0);
    __syncthreads();
    const int t_lo = s_t[0], t_hi = s_t[1];
    for (int i = threadIdx.x; i < np; i += 256) {
        const int p = p0 + i;
        const int t = owner_of(new_off, t_lo, t_hi, p);
        s_src[i] = old_off[t] + (p - new_off[t]);                           // < old_off[t + 1]: a surviving template keeps its count
    }
    __syncthreads();
    U* const out = dst + (size_t)p0 * UPP;
    for (int e = threadIdx.x; e < np * UPP; e += 256) {
        const int i = e / UPP, w = e - i * UPP;
        out[e] = src[(size_t)s_src[i] * UPP + w];
    }
}

// elem_bytes: 384 (descriptors), 16 (PQ codes), 4 ((x, y) pairs, orientations).  old_off / new_off: device arrays [G + 1], new_off[G] == n_new; src holds old_off[G] elements, dst n_new.
hipError_t launch_compact_ranges(const void* src, void* dst, int elem_bytes, const int32_t* old_off, const int32_t* new_off, int G, long long n_new, hipStream_t stream)
{
    if (G <= 0 || n_new <= 0) return hipSuccess;
    if (n_new > 0x7fffffffll) return hipErrorInvalidValue;
    const int n = (int)n_new;
    if (elem_bytes == kDes * 4) {
        constexpr int kPts = 64;                                            // 24 KB copied per workgroup, six 16-byte units per thread (LDS: 64 source indices = 256 B)
        hipLaunchKernelGGL((k_compact_ranges<uint4, kDes * 4 / 16, kPts>), dim3((n + kPts - 1) / kPts), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, old_off, new_off, G, n);
    } else if (elem_bytes == 16) {
        constexpr int kPts = 1024;                                          // 16 KB copied per workgroup (LDS: 4 KB of source indices)
        hipLaunchKernelGGL((k_compact_ranges<uint4, 1, kPts>), dim3((n + kPts - 1) / kPts), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, old_off, new_off, G, n);
    } else if (elem_bytes == 4) {
        constexpr int kPts = 2048;                                          // 8 KB copied per workgroup (LDS: 8 KB of source indices)
        hipLaunchKernelGGL((k_compact_ranges<uint32_t, 1, kPts>), dim3((n + kPts - 1) / kPts), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, old_off, new_off, G, n);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

// afis_gallery_commit_at: the sibling of k_compact_ranges for an edit that REPLACES templates.  The same spans of output points, the same two searches; what differs is where a
// point comes from.  Template t of the new array takes its points from the resident array (it stays, perhaps moved: src_tab[t] >= 0 is where its range starts there, its old
// offset) or from the staged array the host has just uploaded (it is replaced: src_tab[t] < 0, and ~src_tab[t] is where its range starts there).  The table is the host's
// (gallery_splice_plan.h), which also wrote new_off from the same counts: point k of template t exists on the source side whenever it exists on the output side.
// LDS carries the source point with the table's sign: i >= 0 resident point i, i < 0 staged point ~i.
template <class U, int UPP, int kPts>
__global__ __launch_bounds__(256) void k_splice_ranges(const U* __restrict__ res, const U* __restrict__ stg, U* __restrict__ dst, const int32_t* __restrict__ src_tab,
                                                       const int32_t* __restrict__ new_off, int G, int n_new)
{
    __shared__ int s_src[kPts];
    __shared__ int s_t[2];
    const int p0 = blockIdx.x * kPts;                                       // (n_new < 2^31: the plan's range check)
    const int np = min(kPts, n_new - p0);
    if (np <= 0) return;
    if (threadIdx.x < 2) s_t[threadIdx.x] = owner_of(new_off, 0, G - 1, threadIdx.x ? p0 + np - 1 : p0);
    __syncthreads();
    const int t_lo = s_t[0], t_hi = s_t[1];
    for (int i = threadIdx.x; i < np; i += 256) {
        const int p = p0 + i;
        const int t = owner_of(new_off, t_lo, t_hi, p);
        const int s = src_tab[t], k = p - new_off[t];                       // k < the template's count, on both sides
        s_src[i] = s >= 0 ? s + k : ~(~s + k);
    }
    __syncthreads();
    U* const out = dst + (size_t)p0 * UPP;
    for (int e = threadIdx.x; e < np * UPP; e += 256) {
        const int i = e / UPP, w = e - i * UPP;
        const int sp = s_src[i];
        const U* const from = sp >= 0 ? res + (size_t)sp * UPP : stg + (size_t)~sp * UPP;
        out[e] = from[w];
    }
}

// elem_bytes and the points per workgroup as for launch_compact_ranges.  src_tab: device array [G] (above); new_off: [G + 1], new_off[G] == n_new; res holds the resident
// array, stg the staged one (never read when no entry of src_tab is negative), dst n_new elements.
hipError_t launch_splice_ranges(const void* res, const void* stg, void* dst, int elem_bytes, const int32_t* src_tab, const int32_t* new_off, int G, long long n_new, hipStream_t stream)
{
    if (G <= 0 || n_new <= 0) return hipSuccess;
    if (n_new > 0x7fffffffll) return hipErrorInvalidValue;
    const int n = (int)n_new;
    if (elem_bytes == kDes * 4) {
        constexpr int kPts = 64;
        hipLaunchKernelGGL((k_splice_ranges<uint4, kDes * 4 / 16, kPts>), dim3((n + kPts - 1) / kPts), dim3(256), 0, stream, (const uint4*)res, (const uint4*)stg, (uint4*)dst, src_tab, new_off, G, n);
    } else if (elem_bytes == 16) {
        constexpr int kPts = 1024;
        hipLaunchKernelGGL((k_splice_ranges<uint4, 1, kPts>), dim3((n + kPts - 1) / kPts), dim3(256), 0, stream, (const uint4*)res, (const uint4*)stg, (uint4*)dst, src_tab, new_off, G, n);
    } else if (elem_bytes == 4) {
        constexpr int kPts = 2048;
        hipLaunchKernelGGL((k_splice_ranges<uint32_t, 1, kPts>), dim3((n + kPts - 1) / kPts), dim3(256), 0, stream, (const uint32_t*)res, (const uint32_t*)stg, (uint32_t*)dst, src_tab, new_off, G, n);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace afis
