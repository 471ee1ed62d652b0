// link_groups.hip — device code of the link groups (afis_link.cpp: afis_link_groups, afis_link_subject_groups).  The definitions — a cell that reaches, the nodes, an
// edge under either mode, the union and its step bound — are link_groups.h's, shared with the host.
//
//   k_link_init        parent[v] = v, size[v] = 0 for every node; first_col[s] = INT32_MAX where the subject form runs in mutual mode.
//   k_link_first_cols  (subject form, mutual mode) first_col[node of column p] = min p, by integer atomicMin: "row q's print" is the first column of q's person;
//   k_link_row_cols    col_of_row[q] = first_col[row_node[q]], -1 where the row is no column node or no column is its person's.  In the template form the host knows
//                      the column of a row's print and uploads col_of_row with the other tables.
//   k_link_scan        the one pass over the matrix [n_q][G], and the hooking kernel.  Grid = (column chunks, strips of kFilterRows rows), the shape of
//                      k_score_hist_rows: a workgroup owns kLinkChunkScalar adjacent columns — kLinkChunkVec where every row starts on a 16-byte boundary (four
//                      columns as one 16-byte word) — and a thread issues the whole strip's loads, one per row, before it looks at the first cell (a lane past the
//                      row's end holds the no-entry word, which never reaches).  A cell that does not reach costs one add and one compare.  A cell that reaches
//                      (link_cell) resolves its two nodes, in the subject form looks the (row, person) pair up in the sorted exclusion keys — the persons a filtered
//                      subject list drops from its maxima are dropped here from the cells —, in mutual mode reads the reverse cell (one dependent load), and where it
//                      is an edge unites the two nodes and counts 1 in a register.  The counts are summed inside the wave (shuffles), then over the workgroup's four
//                      waves in LDS: one 64-bit integer atomicAdd per workgroup that saw an edge.
//                      VISIBILITY: parent[] is shared by every workgroup of the grid, on every XCD, while the kernel runs.  Every read of it here is a relaxed atomic
//                      load of agent scope and every write an atomic of agent scope (LinkDev: the hook a compare-and-swap, the halving an atomicMin, so a late
//                      writer cannot raise a pointer); nothing else is published through it — a pointer is a node number, complete in itself — so no fence is needed.
//                      BOUNDED: link_unite's budget (link_groups.h derives it: 4 n_nodes + 4 steps cover every correct run); a thread that exhausts it raises the
//                      error word and unites nothing more.  The barrier of the count sits behind the strips' loop, whose bounds are block indices and launch arguments.
//   -- kernel boundary: plain loads of parent[] from here on --
//   k_link_flatten     label[v] = the root above v (link_root, bounded by the node count; the error word otherwise), size[root] += 1 by integer atomicAdd.
//   k_link_compact     the (node, label) pairs of the nodes whose group holds two or more, compacted into out: a wave ballots, its first lane draws the wave's slots
//                      from the counter with one atomicAdd.  The order of arrival is free: the host arranges the pairs (link_arrange).
// Matrix indices are size_t.  Integer atomics only; no cooperative launch, no grid barrier: the kernel boundaries order the phases.
#include "afis_device.h"
#include "link_groups.h"
#include <type_traits>

namespace afis {

constexpr int kLinkThreads = 256;
static_assert(kLinkChunkScalar == kLinkThreads && kLinkChunkVec == 4 * kLinkThreads, "afis_device.h names the column chunks");

// parent[] while the hooking kernel runs
struct LinkDev {
    int32_t* parent;
    __device__ __forceinline__ int32_t load(int32_t i) const { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void lower(int32_t i, int32_t v) { (void)__hip_atomic_fetch_min(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ bool hook(int32_t hi, int32_t lo)
    {
        int32_t expected = hi;
        return __hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__device__ __forceinline__ int32_t link_col_node(const LinkScan& a, size_t c)
{
    return a.slot_of ? a.slot_of[a.d_global ? (size_t)(a.d_global[c] - a.index_base) : c] : (int32_t)c;
}

// is (row, person) on the sorted exclusion keys?  (the subject form only: n_excl is 0 otherwise)
__device__ __forceinline__ bool link_excluded(const LinkScan& a, int q, int32_t node)
{
    const u64 key = ((u64)(uint32_t)q << 32) | (uint32_t)node;
    size_t lo = 0, hi = a.n_excl;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (a.excl[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < a.n_excl && a.excl[lo] == key;
}

// a cell (q, c) that reaches: 1 where it is an edge, its nodes then united.  dead: this thread has exhausted a budget before
__device__ __noinline__ uint32_t link_cell(const LinkScan& a, const uint32_t* __restrict__ matrix, int G, int q, size_t c, bool& dead)
{
    const int32_t rn = a.row_node[q], cn = link_col_node(a, c);
    if (rn == cn) return 0;
    if (a.n_excl && link_excluded(a, q, cn)) return 0;
    if (a.first_row) {                                                      // mutual mode: the reverse cell
        const int32_t r2 = a.first_row[cn], c2 = a.col_of_row[q];
        if (r2 < 0 || c2 < 0) return 0;
        if (!link_reaches(matrix[(size_t)r2 * (size_t)G + (size_t)c2], a.thr)) return 0;
        if (a.n_excl && link_excluded(a, r2, rn)) return 0;                 // (c2 is a column of q's person)
    }
    if (!dead) {
        LinkDev acc{a.parent};
        if (!link_unite(acc, rn, cn, link_budget(a.n_nodes))) { dead = true; atomicOr(a.err, 1u); }
    }
    return 1;
}

template <bool kVec>
__global__ __launch_bounds__(kLinkThreads) void k_link_scan(const uint32_t* __restrict__ matrix, int n_q, int G, LinkScan a)
{
    constexpr int kCols = kVec ? 4 : 1;
    using W = typename std::conditional<kVec, uint4, uint32_t>::type;
    __shared__ uint32_t s_cnt[kLinkThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t col = (size_t)blockIdx.x * (size_t)(kLinkThreads * kCols) + (size_t)tid * kCols;
    const int strips = (n_q + kFilterRows - 1) / kFilterRows;
    uint32_t cnt = 0;                                                       // (a thread sees at most 65 535 strips x 8 rows x 4 cells)
    bool dead = false;
    for (int st = (int)blockIdx.y; st < strips; st += (int)gridDim.y) {
        const int q0 = st * kFilterRows, rows = n_q - q0 < kFilterRows ? n_q - q0 : kFilterRows;
        W v[kFilterRows];
#pragma unroll
        for (int r = 0; r < kFilterRows; ++r) {                             // the whole strip's loads before the first cell is looked at (kVec: G % 4 == 0, so col < G means col + 3 < G)
            const bool in = r < rows && col < (size_t)G;
            const size_t at = (size_t)(q0 + r) * (size_t)G + col;
            if constexpr (kVec) v[r] = in ? *reinterpret_cast<const uint4*>(matrix + at) : make_uint4(kNoEntryWord, kNoEntryWord, kNoEntryWord, kNoEntryWord);
            else v[r] = in ? matrix[at] : kNoEntryWord;
        }
#pragma unroll
        for (int r = 0; r < kFilterRows; ++r) {
            if constexpr (kVec) {
                const uint32_t w[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) if (link_reaches(w[k], a.thr)) cnt += link_cell(a, matrix, G, q0 + r, col + (size_t)k, dead);
            } else if (link_reaches(v[r], a.thr)) cnt += link_cell(a, matrix, G, q0 + r, col, dead);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);        // the wave's edges
    if (lane == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();                                                        // (every thread arrives: no thread returns early, a dead one only stops uniting)
    if (tid == 0) {
        u64 total = 0;
        for (int w = 0; w < kLinkThreads / 64; ++w) total += s_cnt[w];
        if (total) atomicAdd(a.n_edges, total);
    }
}

__global__ __launch_bounds__(kLinkThreads) void k_link_init(int32_t* __restrict__ parent, int32_t* __restrict__ size, int32_t n_nodes, int32_t* __restrict__ first_col, int32_t n_first)
{
    const size_t i = (size_t)blockIdx.x * kLinkThreads + threadIdx.x;
    if (i < (size_t)n_nodes) { parent[i] = (int32_t)i; size[i] = 0; }
    if (i < (size_t)n_first) first_col[i] = INT32_MAX;
}

__global__ __launch_bounds__(kLinkThreads) void k_link_first_cols(LinkScan a, int G, int32_t* __restrict__ first_col)
{
    const size_t p = (size_t)blockIdx.x * kLinkThreads + threadIdx.x;
    if (p < (size_t)G) atomicMin(first_col + link_col_node(a, p), (int32_t)p);
}

__global__ __launch_bounds__(kLinkThreads) void k_link_row_cols(const int32_t* __restrict__ row_node, int n_q, const int32_t* __restrict__ first_col, int32_t n_first, int32_t* __restrict__ col_of_row)
{
    const size_t q = (size_t)blockIdx.x * kLinkThreads + threadIdx.x;
    if (q >= (size_t)n_q) return;
    const int32_t rn = row_node[q];
    const int32_t c = rn < n_first ? first_col[rn] : INT32_MAX;
    col_of_row[q] = c == INT32_MAX ? -1 : c;
}

__global__ __launch_bounds__(kLinkThreads) void k_link_flatten(const int32_t* __restrict__ parent, int32_t n_nodes, int32_t* __restrict__ label, int32_t* __restrict__ size, uint32_t* __restrict__ err)
{
    const size_t v = (size_t)blockIdx.x * kLinkThreads + threadIdx.x;
    if (v >= (size_t)n_nodes) return;
    int32_t r = link_root(parent, (int32_t)v, n_nodes);
    if (r < 0) { atomicOr(err, 2u); r = (int32_t)v; }
    label[v] = r;
    atomicAdd(size + r, 1);
}

__global__ __launch_bounds__(kLinkThreads) void k_link_compact(const int32_t* __restrict__ label, const int32_t* __restrict__ size, int32_t n_nodes, uint32_t* __restrict__ n_pairs, int2* __restrict__ out)
{
    const size_t v = (size_t)blockIdx.x * kLinkThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t lb = -1;
    bool in = false;
    if (v < (size_t)n_nodes) { lb = label[v]; in = size[lb] >= 2; }
    const u64 m = __ballot(in);
    if (m == 0) return;                                                     // (a ballot: the same in every lane)
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(n_pairs, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
    if (in) out[base + (uint32_t)__popcll(m & (((u64)1 << lane) - 1))] = make_int2((int32_t)v, lb);   // (at most n_nodes pairs: out holds as many)
}

hipError_t launch_link_groups(const float* matrix, int n_q, int G, const LinkScan& scan, int32_t* label, int32_t* size, int32_t* first_col, int32_t n_first, int32_t* col_of_row_out,
                              uint32_t* n_pairs, int32_t* out_pairs, hipStream_t stream)
{
    if (n_q <= 0 || G <= 0 || scan.n_nodes <= 0) return hipSuccess;
    if (!matrix || !scan.row_node || !scan.parent || !scan.n_edges || !scan.err || !label || !size || !n_pairs || !out_pairs || (scan.n_excl && !scan.excl) ||
        (scan.first_row && !scan.col_of_row) || (n_first > 0 && !(first_col && col_of_row_out && scan.slot_of))) return hipErrorInvalidValue;
    const int32_t n = scan.n_nodes;
    const dim3 per_node((unsigned)(((size_t)(n > n_first ? n : n_first) + kLinkThreads - 1) / kLinkThreads)), per_node_only((unsigned)(((size_t)n + kLinkThreads - 1) / kLinkThreads));
    hipLaunchKernelGGL(k_link_init, per_node, dim3(kLinkThreads), 0, stream, scan.parent, size, n, first_col, n_first);
    if (n_first > 0) {                                                      // the subject form in mutual mode: the column of a row's print
        hipLaunchKernelGGL(k_link_first_cols, dim3((unsigned)(((size_t)G + kLinkThreads - 1) / kLinkThreads)), dim3(kLinkThreads), 0, stream, scan, G, first_col);
        hipLaunchKernelGGL(k_link_row_cols, dim3((unsigned)(((size_t)n_q + kLinkThreads - 1) / kLinkThreads)), dim3(kLinkThreads), 0, stream, scan.row_node, n_q, first_col, n_first, col_of_row_out);
    }
    const bool vec = rows_take_16_bytes(G, matrix, matrix);
    const size_t chunk = vec ? kLinkChunkVec : kLinkChunkScalar;
    const dim3 grid((unsigned)(((size_t)G + chunk - 1) / chunk), grid_clamp((size_t)((n_q + kFilterRows - 1) / kFilterRows)));
    const uint32_t* const m = (const uint32_t*)matrix;
    if (vec) hipLaunchKernelGGL(k_link_scan<true>, grid, dim3(kLinkThreads), 0, stream, m, n_q, G, scan);
    else hipLaunchKernelGGL(k_link_scan<false>, grid, dim3(kLinkThreads), 0, stream, m, n_q, G, scan);
    hipLaunchKernelGGL(k_link_flatten, per_node_only, dim3(kLinkThreads), 0, stream, scan.parent, n, label, size, scan.err);
    hipLaunchKernelGGL(k_link_compact, per_node_only, dim3(kLinkThreads), 0, stream, label, size, n, n_pairs, (int2*)out_pairs);
    return hipGetLastError();
}

}  // namespace afis
