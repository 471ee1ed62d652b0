// score_stats_check.cpp — score_stats.h's host arithmetic on cohort statistics as a program of its own, built with the host sanitizers (Makefile: score_stats_check)
// and run directly by tests/test_score_stats_host.py, which holds its answers against Python integers.
// Reads commands from stdin, one per line, every number in hex (a statistic: n n_outside s1 s2_lo s2_hi min max, the last two as float words):
//   add <statistic> <statistic>   stat_add(acc, other)      -> rc and acc afterwards
//   rem <statistic> <float word>  stat_remove(acc, score)   -> rc and acc afterwards
//   mom <statistic>               stat_moments(st)          -> rc and the words of mean and sd
//   q <float word>                                           -> the cell's class and, for a valued cell, q
//   z <float word> <offset word> <scale word>                -> the normalised cell's word (offset and scale as double words)
// One line of answers per command; returns 1 on a line it cannot read.
#include "score_stats.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>

using namespace afis;

static bool read_stat(ScoreStat& s)
{
    uint64_t n, no; uint32_t mn, mx;
    if (scanf("%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx32 " %" SCNx32, &n, &no, &s.s1, &s.s2_lo, &s.s2_hi, &mn, &mx) != 7) return false;
    s.n = (int64_t)n; s.n_outside = (int64_t)no;
    s.min = __builtin_bit_cast(float, mn); s.max = __builtin_bit_cast(float, mx);
    return true;
}

static void print_stat(int rc, const ScoreStat& s)
{
    printf("%d %" PRIx64 " %" PRIx64 " %" PRIx64 " %" PRIx64 " %" PRIx64 " %08" PRIx32 " %08" PRIx32 "\n", rc, (uint64_t)s.n, (uint64_t)s.n_outside, s.s1, s.s2_lo, s.s2_hi,
           __builtin_bit_cast(uint32_t, s.min), __builtin_bit_cast(uint32_t, s.max));
}

int main()
{
    char op[8];
    while (scanf("%7s", op) == 1) {
        ScoreStat a{}, b{};
        if (!strcmp(op, "add")) {
            if (!read_stat(a) || !read_stat(b)) return 1;
            print_stat(stat_add(a, b), a);
        } else if (!strcmp(op, "rem")) {
            uint32_t w;
            if (!read_stat(a) || scanf("%" SCNx32, &w) != 1) return 1;
            print_stat(stat_remove(a, __builtin_bit_cast(float, w)), a);
        } else if (!strcmp(op, "mom")) {
            if (!read_stat(a)) return 1;
            double mean = -1.0, sd = -1.0;
            const int rc = stat_moments(a, &mean, &sd);
            printf("%d %016" PRIx64 " %016" PRIx64 "\n", rc, __builtin_bit_cast(uint64_t, mean), __builtin_bit_cast(uint64_t, sd));
        } else if (!strcmp(op, "q")) {
            uint32_t w;
            if (scanf("%" SCNx32, &w) != 1) return 1;
            const int c = stat_cell_class(w);
            printf("%d %" PRIx64 "\n", c, c == kCellValued ? stat_q(__builtin_bit_cast(float, w)) : (uint64_t)0);
        } else if (!strcmp(op, "z")) {
            uint32_t w; uint64_t o, s;
            if (scanf("%" SCNx32 " %" SCNx64 " %" SCNx64, &w, &o, &s) != 3) return 1;
            printf("%08" PRIx32 "\n", stat_normalized_word(w, __builtin_bit_cast(double, o), __builtin_bit_cast(double, s)));
        } else return 1;
    }
    return 0;
}
