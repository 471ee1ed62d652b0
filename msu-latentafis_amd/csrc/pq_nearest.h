// pq_nearest.h — the nearest-codeword search of one sub-quantizer, the ONE definition the encoder (pq_encode.hip::k_pq_encode) and the trainer's assignment
// (pq_train.hip::k_train_step) share: a label of afis_pq_train is the code afis_pq_encode returns because both kernels inline these two functions.
// Arithmetic (scipy.cluster.vq.vq's float32 path for 5 or more features, pq_encode.hip's head comment): dist = fl(fl(-2 fma_chain(c, x) + |x|^2) + |c|^2), the dot
// product an fma chain over d ascending from 0, the squared norms plain sums of rounded squares, d ascending; the first strict minimum from +inf wins (a row
// whose distances are all +inf or NaN gets code 0).  Every unit that includes this is built with -ffp-contract=off: the only fused operations are the explicit ones.
#pragma once
#include <hip/hip_runtime.h>

#include "afis_device.h"

namespace afis {

__device__ __forceinline__ float pq_sqnorm6(const float* __restrict__ v)
{
    float s = 0.0f;
#pragma unroll
    for (int d = 0; d < kDsub; ++d) { const float w = v[d]; const float t = w * w; s += t; }
    return s;
}

// cw [256][6] and csq [256] = pq_sqnorm6 of every codeword, both in LDS (every lane reads the same codeword: a broadcast); x: the lane's sub-vector
__device__ __forceinline__ int pq_nearest(const float* __restrict__ cw, const float* __restrict__ csq, const float (&x)[kDsub])
{
    const float xsq = pq_sqnorm6(x);
    float best = INFINITY; int arg = 0;
#pragma unroll 4
    for (int k = 0; k < kK; ++k) {
        float dot = 0.0f;
#pragma unroll
        for (int d = 0; d < kDsub; ++d) dot = __builtin_fmaf(cw[k * kDsub + d], x[d], dot);
        const float t = -2.0f * dot + xsq;             // (-ffp-contract=off: the product -2 dot is exact, the sum rounds once)
        const float dist = t + csq[k];
        if (dist < best) { best = dist; arg = k; }     // strict: the first minimum wins
    }
    return arg;
}

}  // namespace afis
