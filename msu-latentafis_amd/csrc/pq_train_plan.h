// pq_train_plan.h — the host's plans of codebook training, device-free (checked by the stand-alone program pq_train_plan_check under the host sanitizers):
// the point sampler of afis_pq_train_init_points and the pq_train CLI's selection of a template's points.
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace afis {

constexpr int kTrainInitK = 256;              // codewords drawn per sub-quantizer

// The generator of include/afis_matcher.h: splitmix64's output function as a counter-based generator.
inline uint64_t train_mix(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t train_draw(uint64_t seed, int m, int j) { return train_mix(train_mix(seed) + (uint64_t)(kTrainInitK * m + j)); }

// 256 distinct indices of [0, n) for sub-quantizer m: the first 256 steps of a Fisher-Yates shuffle of a = (0, 1, .., n - 1) — step j swaps a[j] with
// a[j + draw(seed, m, j) mod (n - j)] and delivers the new a[j].  Only the entries a swap has moved are stored.  n < 256: false, nothing written.
inline bool train_init_indices(int64_t n, uint64_t seed, int m, int64_t* out /*[256]*/)
{
    if (n < kTrainInitK) return false;
    std::unordered_map<int64_t, int64_t> moved;
    auto at = [&](int64_t i) { const auto it = moved.find(i); return it == moved.end() ? i : it->second; };
    for (int j = 0; j < kTrainInitK; ++j) {
        const int64_t r = j + (int64_t)(train_draw(seed, m, j) % (uint64_t)(n - j));
        const int64_t aj = at(j), ar = at(r);
        moved[r] = aj; moved[j] = ar;
        out[j] = ar;
    }
    return true;
}

// extraction/descriptor_PQ.py:54-63: a template with fewer than min_points texture points is skipped; of the others every stride-th point is taken, from the first.
// The indices taken of a template of n_points, appended to out; returns how many.
inline int64_t train_take_points(int64_t n_points, int64_t min_points, int64_t stride, std::vector<int64_t>& out)
{
    if (stride < 1) stride = 1;
    if (n_points <= 0 || n_points < min_points) return 0;
    int64_t taken = 0;
    for (int64_t i = 0; i < n_points; i += stride, ++taken) out.push_back(i);
    return taken;
}

}  // namespace afis
