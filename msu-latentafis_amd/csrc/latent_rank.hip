// latent_rank.hip — device code of the column hit lists (afis_reverse.cpp: afis_rank_latent_hits): the score matrix a search left on the device, [n_q][n], is ranked
// along its COLUMNS — per rolled print, which latents reach the decision score.  k_rank_hits (rank_hits.hip) ranks rows, each by one workgroup that passes over it with
// coalesced loads; a column of the matrix is n_q words n apart.  So the matrix is transposed once, k_transpose_scores, and k_rank_hits runs unchanged on [n][n_q]:
// rows = prints, entries = the search's queries, ties by ascending position = ascending query position.
//
// k_transpose_scores: one 256-thread workgroup per 64 x 64 tile, through LDS.
//   in    the tile's h x w words (h = rows of the matrix = queries, w = its columns = prints; both 64 except in the last tile of a dimension) are taken in the order they
//         lie in memory, element e = r * w + c by thread e % 256 in trip e / 256: a wave reads 64 consecutive words of a row of a full tile, and in a tile narrower than
//         64 — the ten prints of one card — runs of w words from consecutive rows, which for a matrix of n <= 64 columns are consecutive in memory too
//   LDS   tile[r][c] at word r * 65 + c.  Banks (cdna_hip_programming.md section 2: ds_write_b32 and ds_read_b32 bank on 32 dwords, and only the lanes of one 32-lane
//         half conflict): a full tile's write puts lanes l = c of one row on banks (r + c) % 32 — 32 consecutive lanes, 32 banks; the read below puts lanes l = r of one
//         column on banks (65 r + c) % 32 = (r + c) % 32 — again 32 banks.  An even pitch of 64 would put the whole column on one bank.  In a tile narrower than 64 a
//         write's half-wave spans several rows and two lanes with the same r + c meet on a bank (2-way as a rule): those tiles move w / 64 of the words.
//   out   wave v writes the columns c = v, v + 4, ... of the tile: lane l holds tile[l][c], 64 consecutive words of row c0 + c of the transposed matrix
// Every index into the matrices is a size_t: n_q x n words may pass 2^32.  The tiles are numbered along a one-dimensional grid (a shard of a million prints has more
// column tiles than a grid's second dimension takes).
#include "afis_device.h"

namespace afis {

constexpr int kTrTile = 64;
constexpr int kTrPitch = kTrTile + 1;                                       // odd: a column of the tile lies on 32 different banks
constexpr int kTrThreads = 256;
static_assert(kTrPitch % 2 == 1 && kTrThreads % 64 == 0 && kTrTile == 64, "one lane per row of the tile on the way out");

// in [n_q][n] -> out [n][n_q]; tiles_q = ceil(n_q / 64); grid: tiles_q * ceil(n / 64)
__global__ __launch_bounds__(kTrThreads) void k_transpose_scores(const float* __restrict__ in, float* __restrict__ out, int n_q, int n, unsigned tiles_q)
{
    __shared__ float tile[kTrTile * kTrPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = (int)(blockIdx.x % tiles_q) * kTrTile, c0 = (int)(blockIdx.x / tiles_q) * kTrTile;   // (both below n_q / n by the grid's size)
    const int h = min(kTrTile, n_q - q0), w = min(kTrTile, n - c0);
    const float* const src = in + (size_t)q0 * (size_t)n + (size_t)c0;
    for (int e = tid; e < h * w; e += kTrThreads) {
        const int r = e / w, c = e - r * w;
        tile[r * kTrPitch + c] = src[(size_t)r * (size_t)n + (size_t)c];
    }
    __syncthreads();
    if (lane < h) {
        float* const dst = out + (size_t)c0 * (size_t)n_q + (size_t)(q0 + lane);
        for (int c = wave; c < w; c += kTrThreads / 64) dst[(size_t)c * (size_t)n_q] = tile[lane * kTrPitch + c];
    }
}

hipError_t launch_transpose_scores(const float* in, float* out, int n_q, int n, hipStream_t stream)
{
    if (n_q <= 0 || n <= 0) return hipSuccess;
    const unsigned long long tiles_q = ((unsigned long long)n_q + kTrTile - 1) / kTrTile, tiles_n = ((unsigned long long)n + kTrTile - 1) / kTrTile;
    if (!in || !out || tiles_q * tiles_n > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_transpose_scores, dim3((unsigned)(tiles_q * tiles_n)), dim3(kTrThreads), 0, stream, in, out, n_q, n, (unsigned)tiles_q);
    return hipGetLastError();
}

}  // namespace afis
