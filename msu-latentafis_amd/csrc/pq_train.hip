// pq_train.hip — one Lloyd step of the PQ codebook on the device (afis_pq_train, include/afis_matcher.h has the definition).
// Reference: extraction/descriptor_PQ.py:41-77 (training: scipy.cluster.vq.kmeans2 per sub-space, minit='points').  kmeans2's step is vq + a floating-point mean;
// here the assignment is the encoder's search (pq_nearest.h, the code afis_pq_encode returns) and the mean is made order-independent: every component enters an
// int64 sum as q(x) = rint(x 2^30), and the host divides sum by count once (afis_train.cpp).  Integer adds are associative, so LDS atomics, the per-workgroup
// partial sums and the global atomics below give the same words for every grid, schedule and arrival order.
//
// Work decomposition: the points are transposed once to sub-space-major xt [16][n][6] (k_train_transpose, which also validates the range), so that a step reads 24
// contiguous bytes per (point, sub-quantizer).  A step workgroup (4 waves) serves ONE sub-quantizer: its codebook slice (6 KB), the squared norms (1 KB) and int64
// accumulators [256][7] (14 KB) sit in LDS — 21 KB, where the encoder's all-sixteen-slices layout (137 KB) would leave no room for 229 KB of accumulators.  Lane =
// point; 256-codeword search as the encoder; seven 64-bit LDS atomic adds per point; at the end the non-zero accumulators go to the global [16][256][7] array
// with 64-bit atomic adds (consecutive lanes, consecutive words).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afis_device.h"
#include "pq_nearest.h"
#include "pq_train.h"

namespace afis {

static_assert(kTrainAcc == kDsub + 1, "S[0..5] and the count");

constexpr int kTrPts = 64;                    // points per tile of the transpose
constexpr int kTrStride = kDes + 1;           // padded row, as the encoder's

__global__ __launch_bounds__(256) void k_train_transpose(const float* __restrict__ des, long long p0, long long np, long long n, float* __restrict__ xt,
                                                         uint32_t* __restrict__ bad)
{
    __shared__ float s_des[kTrPts * kTrStride];                // 24.8 KB
    const int tid = threadIdx.x;
    const long long n_tiles = (np + kTrPts - 1) / kTrPts;
    bool any_bad = false;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long t0 = tile * kTrPts;
        const int nt = (int)((np - t0) < kTrPts ? (np - t0) : kTrPts);
        __syncthreads();                                       // the previous tile has been written out
        for (int i = tid; i < nt * kDes; i += 256) {
            const float v = des[t0 * kDes + i];
            any_bad |= !(__builtin_fabsf(v) <= 64.0f);         // NaN, +-inf and |v| > 64 alike
            s_des[(i / kDes) * kTrStride + (i % kDes)] = v;
        }
        __syncthreads();
        const int run = nt * kDsub;                            // floats of the tile in one sub-space: contiguous in xt
        for (int i = tid; i < kM * run; i += 256) {
            const int m = i / run, r = i - m * run, pt = r / kDsub, d = r - pt * kDsub;
            xt[((size_t)m * (size_t)n + (size_t)(p0 + t0 + pt)) * kDsub + d] = s_des[pt * kTrStride + m * kDsub + d];
        }
    }
    if (any_bad) atomicOr(bad, 1u);
}

hipError_t launch_train_transpose(const float* des, long long p0, long long np, long long n, float* xt, uint32_t* bad, hipStream_t stream)
{
    if (np <= 0) return hipSuccess;
    const long long n_tiles = (np + kTrPts - 1) / kTrPts;
    const int grid = (int)(n_tiles < 2048 ? n_tiles : 2048);
    hipLaunchKernelGGL(k_train_transpose, dim3(grid), dim3(256), 0, stream, des, p0, np, n, xt, bad);
    return hipGetLastError();
}

// q(x) = (int64) rint((double)x 2^30): the widening and the scaling are exact, rint rounds to nearest even — one rounding.  |x| <= 64 gives |q| <= 2^36.
__device__ __forceinline__ long long train_q(float x) { return (long long)__builtin_rint((double)x * 1073741824.0); }

__global__ __launch_bounds__(kTrainThreads) void k_train_step(const float* __restrict__ xt, long long n, const float* __restrict__ codewords,
                                                              uint8_t* __restrict__ labels, int first, unsigned long long* __restrict__ acc)
{
    __shared__ float s_cw[kK * kDsub];                         // 6 KB: this sub-quantizer's slice
    __shared__ float s_csq[kK];                                // 1 KB
    __shared__ unsigned long long s_acc[kK * kTrainAcc];       // 14 KB: two's-complement sums and counts of this workgroup's points
    __shared__ unsigned long long s_chg;
    const int tid = threadIdx.x, m = blockIdx.y;
    const float* cwm = codewords + m * kK * kDsub;
    for (int i = tid; i < kK * kDsub; i += kTrainThreads) s_cw[i] = cwm[i];
    for (int e = tid; e < kK; e += kTrainThreads) s_csq[e] = pq_sqnorm6(cwm + e * kDsub);
    for (int i = tid; i < kK * kTrainAcc; i += kTrainThreads) s_acc[i] = 0ull;
    if (tid == 0) s_chg = 0ull;
    __syncthreads();
    const float* xm = xt + (size_t)m * (size_t)n * kDsub;      // 24 m n bytes into a 256-byte aligned array: 8-byte aligned, as is every point's 24 p
    uint8_t* lm = labels + (size_t)m * (size_t)n;
    unsigned n_chg = 0;
    for (long long p = (long long)blockIdx.x * kTrainThreads + tid; p < n; p += (long long)gridDim.x * kTrainThreads) {
        const float2* src = reinterpret_cast<const float2*>(xm + p * kDsub);
        const float2 a = src[0], b = src[1], c = src[2];
        const float x[kDsub] = {a.x, a.y, b.x, b.y, c.x, c.y};
        const int k = pq_nearest(s_cw, s_csq, x);
#pragma unroll
        for (int d = 0; d < kDsub; ++d) atomicAdd(&s_acc[k * kTrainAcc + d], (unsigned long long)train_q(x[d]));
        atomicAdd(&s_acc[k * kTrainAcc + kDsub], 1ull);
        n_chg += (first || lm[p] != (uint8_t)k) ? 1u : 0u;
        lm[p] = (uint8_t)k;
    }
    if (n_chg) atomicAdd(&s_chg, (unsigned long long)n_chg);
    __syncthreads();
    unsigned long long* out = acc + (size_t)m * kK * kTrainAcc;
    for (int i = tid; i < kK * kTrainAcc; i += kTrainThreads) { const unsigned long long v = s_acc[i]; if (v) atomicAdd(&out[i], v); }
    if (tid == 0 && s_chg) atomicAdd(&acc[kTrainSumWords], s_chg);
}

hipError_t launch_train_step(const float* xt, long long n, const float* codewords, uint8_t* labels, int first, unsigned long long* acc, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const long long nb = (n + kTrainThreads - 1) / kTrainThreads;
    const int gx = (int)(nb < kTrainBlocksPerSub ? nb : kTrainBlocksPerSub);
    hipLaunchKernelGGL(k_train_step, dim3(gx, kM), dim3(kTrainThreads), 0, stream, xt, n, codewords, labels, first, acc);
    return hipGetLastError();
}

}  // namespace afis
