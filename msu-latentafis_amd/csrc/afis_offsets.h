// afis_offsets.h — the derived offset tables of a gallery shard, computed on the host (afis_gallery.cpp: the commit and the edits;
// match_selftest -selftest-offsets, which tests/test_host.py holds against a numpy restatement).  Host only: no kernel includes this.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace afis {

// block offsets of variant 8's code stream (64 points) and tile offsets of the bound pass's (32 points) and of the descriptor fragments (16), from the CSR offsets
// (host; one routine for the commit and the edits — afis_gallery.cpp — and for match_selftest -selftest-offsets, which tests/test_host.py holds against a numpy restatement)
inline void derived_offsets(const std::vector<int32_t>& mo, const std::vector<int32_t>& to, std::vector<int32_t>& toff, std::vector<int32_t>& qb, std::vector<int32_t>& tb,
                            int64_t& n_q_blocks, int64_t& n_t32, int& max_nR)
{
    const size_t G = mo.size() - 1;
    toff.assign(G + 1, 0); qb.assign(G + 1, 0); tb.assign(G + 1, 0);
    int64_t nq = 0, nt = 0; max_nR = 0;
    for (size_t t = 0; t < G; ++t) {
        toff[t + 1] = toff[t] + (mo[t + 1] - mo[t] + 15) / 16;
        qb[t] = (int32_t)nq; nq += ((int64_t)(to[t + 1] - to[t]) + 63) / 64;
        tb[t] = (int32_t)std::min<int64_t>(nt, 0x7fffffff); nt += ((int64_t)(to[t + 1] - to[t]) + 31) / 32;
        max_nR = std::max(max_nR, mo[t + 1] - mo[t]);
    }
    qb[G] = (int32_t)nq; tb[G] = (int32_t)std::min<int64_t>(nt, 0x7fffffff);
    n_q_blocks = nq; n_t32 = nt;
}

}  // namespace afis
