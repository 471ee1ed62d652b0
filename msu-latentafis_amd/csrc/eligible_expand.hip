// eligible_expand.hip — device code of the eligible search (afis_eligible.cpp: afis_search_eligible): the queries of one CLASS (identical mask triples) were scored
// against the class's eligible templates only — a temporary sub-shard of m of the shard's G templates, in ascending index — and their rows cls [n_c][m] are expanded
// into the rows the class's queries have in the combined matrix out [n_q][G]:
//   out[row_of[r]][t] = inv[t] >= 0 ? cls[r][inv[t]] : kNoEntryWord          inv [G]: the sub-shard position of shard column t, or -1; inv == NULL: identity (m == G)
// The GATHER form: one pass writes every word of the class's rows exactly once, so nothing has to be set beforehand (the scatter form — a memset of 0xff over the
// rows, then 4-byte stores at the eligible columns — writes the eligible cells twice and stores 4 bytes at a time).  The stores are coalesced: a thread owns one column
// — or, where every row of out starts on a 16-byte boundary (G % 4 == 0), four adjacent ones that leave as one 16-byte word, as in hit_filter.hip.  inv is ascending
// over the eligible columns, so the reads of a class row are monotone 4-byte loads: neighbouring lanes read neighbouring or equal cache lines.
//
// Grid = (column chunks, strips of kExRows class rows).  A thread loads inv for its columns ONCE and walks the rows of its strips; the class row r and its target
// row_of[r] depend on the block index and the loop counter only, so they are uniform over the workgroup.  m == 0 (a class no template is eligible for): every word
// of its rows is kNoEntryWord and neither cls nor inv is read.  A position outside [0, m) is treated as -1, which keeps every load inside cls.  No atomics, no
// cross-lane traffic, no LDS.  Rows of out that row_of does not name are not touched.
// Every index into the matrices is a size_t: n_q x G may pass 2^31.  A grid's second dimension holds 65 535 blocks; more strips than that are walked in a loop.
#include "afis_device.h"
#include <type_traits>

namespace afis {

constexpr int kExThreads = 256;
constexpr int kExRows = 8;                                                  // class rows per strip: inv is loaded once per thread, whatever the class's size

// cls [n_c][m] (NULL where m == 0); inv NULL or [G] with -1 <= inv[t] < m; row_of [n_c] with 0 <= row_of[r] < n_q (the host checks); out [n_q][G].  kVec: G % 4 == 0 and
// out 16-byte aligned
template <bool kVec>
__global__ __launch_bounds__(kExThreads) void k_expand_rows(const uint32_t* __restrict__ cls, int n_c, int m, const int32_t* __restrict__ inv, const int32_t* __restrict__ row_of,
                                                            int n_q, int G, uint32_t* __restrict__ out)
{
    constexpr int kCols = kVec ? 4 : 1;
    const size_t col = ((size_t)blockIdx.x * kExThreads + threadIdx.x) * kCols;
    if (col >= (size_t)G) return;                                           // (kVec: G % 4 == 0, so col + 3 < G too)
    int p[kCols];
#pragma unroll
    for (int j = 0; j < kCols; ++j) {
        const int v = m <= 0 ? -1 : inv ? inv[col + j] : (int)(col + j);
        p[j] = v >= 0 && v < m ? v : -1;
    }
    using W = typename std::conditional<kVec, uint4, uint32_t>::type;
    const int strips = (n_c + kExRows - 1) / kExRows;
    for (int st = (int)blockIdx.y; st < strips; st += (int)gridDim.y) {
        const int r0 = st * kExRows, rows = n_c - r0 < kExRows ? n_c - r0 : kExRows;
        for (int r = 0; r < rows; ++r) {
            const int to = row_of[r0 + r];                                  // uniform over the workgroup: a scalar load
            if (to < 0 || to >= n_q) continue;
            const uint32_t* __restrict__ src = cls + (size_t)(r0 + r) * (size_t)m;
            uint32_t w[kCols];
#pragma unroll
            for (int j = 0; j < kCols; ++j) w[j] = p[j] >= 0 ? src[p[j]] : kNoEntryWord;
            W* dst = reinterpret_cast<W*>(out + (size_t)to * (size_t)G + col);
            if constexpr (kVec) *dst = make_uint4(w[0], w[1], w[2], w[3]);
            else *dst = w[0];
        }
    }
}

hipError_t launch_expand_rows(const float* cls, int n_c, int m, const int32_t* inv, const int32_t* row_of, int n_q, int G, float* out, hipStream_t stream)
{
    if (n_c <= 0 || G <= 0) return hipSuccess;
    if (!row_of || !out || n_q <= 0 || m < 0 || m > G || (m > 0 && !cls) || (!inv && m > 0 && m != G) || (const void*)cls == (const void*)out) return hipErrorInvalidValue;
    const bool vec = rows_take_16_bytes(G, out, out);
    const size_t threads = vec ? (size_t)G / 4 : (size_t)G;
    const dim3 grid((unsigned)((threads + kExThreads - 1) / kExThreads), grid_clamp((size_t)((n_c + kExRows - 1) / kExRows)));
    if (vec) hipLaunchKernelGGL(k_expand_rows<true>, grid, dim3(kExThreads), 0, stream, (const uint32_t*)cls, n_c, m, inv, row_of, n_q, G, (uint32_t*)out);
    else hipLaunchKernelGGL(k_expand_rows<false>, grid, dim3(kExThreads), 0, stream, (const uint32_t*)cls, n_c, m, inv, row_of, n_q, G, (uint32_t*)out);
    return hipGetLastError();
}

}  // namespace afis
