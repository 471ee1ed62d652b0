// pq_train.h — the launchers of pq_train.hip, for afis_train.cpp (afis_pq_train): one Lloyd step of the 16 x 256 x 6 codebook on the device, in the
// order-independent definition of include/afis_matcher.h (assignment = the encoder's search, accumulation in int64 fixed point at 2^-30).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afis {

constexpr int kTrainThreads = 256;           // a step workgroup: 4 waves, lane = point
constexpr int kTrainBlocksPerSub = 64;       // step workgroups per sub-quantizer at most (grid 64 x 16 = 4 per CU of a 256-CU chip, 16 waves per CU as the encoder)
constexpr int kTrainAcc = 7;                 // accumulator words per codeword: S[0..5] and the count
constexpr long long kTrainMaxPoints = 1ll << 26;
constexpr size_t kTrainSumWords = (size_t)16 * 256 * kTrainAcc;      // sums [16][256][7] int64; the step's changed-label count is the word behind them

// The first pass: slice [np][96] of the caller's points, resident at `des`, into the sub-space-major copy xt [16][n][6] at points p0 .. p0 + np; *bad |= 1 when a
// component is not finite or exceeds 64 in magnitude.
hipError_t launch_train_transpose(const float* des, long long p0, long long np, long long n, float* xt, uint32_t* bad, hipStream_t stream);
// One step: labels [16][n] u8 rewritten with the step's assignment under `codewords` [16][256][6]; acc [kTrainSumWords + 1] (zeroed by the caller) += the fixed-point
// sums, the counts and, in its last word, the labels that differ from the stored ones (first != 0: every label counts, the stored ones are not read).
hipError_t launch_train_step(const float* xt, long long n, const float* codewords, uint8_t* labels, int first, unsigned long long* acc, hipStream_t stream);

}  // namespace afis
