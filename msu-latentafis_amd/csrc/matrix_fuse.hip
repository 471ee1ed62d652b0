// matrix_fuse.hip — device code of afis_matrix_fuse (afis_matrix.cpp): n <= 16 kept score matrices of one shape [n_q][columns] are folded cell by cell into one
// matrix, under the rule of matrix_fuse.h (sum in fp64 with weights, maximum, minimum; the no-entry word and the raw matrices' -1 as the case lists treat them).
//
// k_matrix_fuse<kOp, kVec>: grid = (column chunks, rows); a thread owns one column of a row — or, where every row of every matrix starts on a 16-byte boundary
// (columns % 4 == 0: the case-fuse kernel's rule), four adjacent ones that travel as one 16-byte word.  The operands arrive as a table passed BY VALUE: the pointers
// and weights sit in the kernel's argument segment, the walk over them is uniform, so every table read is a scalar load.  The operands are walked four at a time:
// the four loads of a group are issued before the first of them is folded (fuse_fold is selects, no branch), and the unrolled groups of a short table overlap.
// No atomic, no LDS, no sum across lanes: the order of a cell's additions is the order of the loop.  Every word of out is written exactly once — there is no memset
// before the launch — and out is none of the operands.
// A transposed operand does not come here as such: the host runs k_transpose_scores (latent_rank.hip) into scratch first and hands the scratch over as the operand.
// Every index into the matrices is a size_t: n_q x columns may pass 2^31.  A grid's second dimension holds 65 535 blocks; more rows than that are walked in a loop.
#include "afis_device.h"
#include "matrix_fuse.h"

namespace afis {

constexpr int kMfuThreads = 256;
constexpr int kMfuGroup = 4;                                                // operands whose loads are issued together

struct FuseTable { const float* src[kFuseOperandsMax]; double w[kFuseOperandsMax]; };

template <int kOp, bool kVec>
__global__ __launch_bounds__(kMfuThreads) void k_matrix_fuse(const FuseTable tab, int n, int n_q, int columns, int normalized, int require_all, float* __restrict__ out)
{
    constexpr int kCols = kVec ? 4 : 1;
    const size_t col = ((size_t)blockIdx.x * kMfuThreads + threadIdx.x) * kCols;
    if (col >= (size_t)columns) return;                                     // (kVec: columns % 4 == 0, so col + 3 < columns too)
    for (int r = (int)blockIdx.y; r < n_q; r += (int)gridDim.y) {
        const size_t at = (size_t)r * (size_t)columns + col;
        FuseAcc acc[kCols];
#pragma unroll
        for (int j = 0; j < kCols; ++j) fuse_start(acc[j]);
        for (int k0 = 0; k0 < n; k0 += kMfuGroup) {
            uint32_t c[kMfuGroup][kCols];
#pragma unroll
            for (int g = 0; g < kMfuGroup; ++g) {
                if (k0 + g < n) {                                           // (uniform)
                    if constexpr (kVec) {
                        const uint4 v = *reinterpret_cast<const uint4*>(tab.src[k0 + g] + at);
                        c[g][0] = v.x; c[g][1] = v.y; c[g][2] = v.z; c[g][3] = v.w;
                    } else c[g][0] = *reinterpret_cast<const uint32_t*>(tab.src[k0 + g] + at);
                }
            }
#pragma unroll
            for (int g = 0; g < kMfuGroup; ++g) {
                if (k0 + g < n) {
                    const double w = tab.w[k0 + g];
#pragma unroll
                    for (int j = 0; j < kCols; ++j) fuse_fold<kOp>(acc[j], c[g][j], w, normalized != 0);
                }
            }
        }
        uint32_t* const dst = reinterpret_cast<uint32_t*>(out + at);
        if constexpr (kVec) *reinterpret_cast<uint4*>(dst) = make_uint4(fuse_result<kOp>(acc[0], n, require_all != 0), fuse_result<kOp>(acc[1], n, require_all != 0),
                                                                         fuse_result<kOp>(acc[2], n, require_all != 0), fuse_result<kOp>(acc[3], n, require_all != 0));
        else dst[0] = fuse_result<kOp>(acc[0], n, require_all != 0);
    }
}

template <int kOp>
static void launch_op(bool vec, dim3 grid, hipStream_t stream, const FuseTable& tab, int n, int n_q, int columns, int normalized, int require_all, float* out)
{
    if (vec) hipLaunchKernelGGL((k_matrix_fuse<kOp, true>), grid, dim3(kMfuThreads), 0, stream, tab, n, n_q, columns, normalized, require_all, out);
    else hipLaunchKernelGGL((k_matrix_fuse<kOp, false>), grid, dim3(kMfuThreads), 0, stream, tab, n, n_q, columns, normalized, require_all, out);
}

hipError_t launch_matrix_fuse(const float* const* src, const double* weights, int n, int mode, int normalized, int n_q, int columns, float* out, hipStream_t stream)
{
    if (n_q <= 0 || columns <= 0) return hipSuccess;
    if (!src || !out || n < 1 || n > kFuseOperandsMax || !fuse_mode_valid(mode)) return hipErrorInvalidValue;
    FuseTable tab = {};
    bool vec = rows_take_16_bytes(columns, out, out);
    for (int k = 0; k < n; ++k) {
        if (!src[k] || src[k] == out) return hipErrorInvalidValue;
        tab.src[k] = src[k]; tab.w[k] = weights ? weights[k] : 1.0;
        vec = vec && rows_take_16_bytes(columns, src[k], out);
    }
    const size_t threads = vec ? (size_t)columns / 4 : (size_t)columns;
    const dim3 grid((unsigned)((threads + kMfuThreads - 1) / kMfuThreads), grid_clamp((size_t)n_q));
    const int op = mode & 3, all = (mode & kFuseRequireAll) ? 1 : 0;
    if (op == kFuseSum) launch_op<kFuseSum>(vec, grid, stream, tab, n, n_q, columns, normalized, all, out);
    else if (op == kFuseMax) launch_op<kFuseMax>(vec, grid, stream, tab, n, n_q, columns, normalized, all, out);
    else launch_op<kFuseMin>(vec, grid, stream, tab, n, n_q, columns, normalized, all, out);
    return hipGetLastError();
}

}  // namespace afis
