// count_before_check — rank_order.h::count_before as a program of its own, for tests/test_positions_host.py: g++ alone, no device.
//   count_before_check <file>    the file: n index_base has_col, then n lines "score word (hex)[ global index]", then any number of target lines
//                                "score word (hex) global index"; prints one count per target.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "rank_order.h"

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: count_before_check <file>\n"); return 2; }
    std::ifstream f(argv[1]);
    long long n = 0, base = 0; int has_col = 0;
    if (!(f >> n >> base >> has_col) || n < 0) { fprintf(stderr, "count_before_check: bad header\n"); return 2; }
    std::vector<float> sc((size_t)n);
    std::vector<int64_t> col(has_col ? (size_t)n : 0);
    for (long long i = 0; i < n; ++i) {
        std::string w; long long c = 0;
        if (!(f >> w) || (has_col && !(f >> c))) { fprintf(stderr, "count_before_check: short row\n"); return 2; }
        const uint32_t bits = (uint32_t)std::stoul(w, nullptr, 16);
        memcpy(&sc[(size_t)i], &bits, 4);
        if (has_col) col[(size_t)i] = c;
    }
    std::string w; long long idx = 0;
    while (f >> w >> idx) {
        const uint32_t bits = (uint32_t)std::stoul(w, nullptr, 16);
        float s; memcpy(&s, &bits, 4);
        printf("%lld\n", (long long)afis::count_before(sc.data(), n, has_col ? col.data() : nullptr, base, s, idx));
    }
    return 0;
}
