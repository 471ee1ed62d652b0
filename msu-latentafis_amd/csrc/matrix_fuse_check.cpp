// matrix_fuse_check.cpp — matrix_fuse.h's cell rule as a program of its own, built with the host sanitizers (Makefile: matrix_fuse_check) and run directly by
// tests/test_matrix_host.py, which holds its answers against tests/matrix_model.py.
// Reads commands from stdin, every number in hex:
//   fuse <mode> <normalized> <n> <weights given: 0 | 1> [<weight, the 64 bits of a double> x n] <n_cells> <cell word> x n x n_cells
//        the cells operand by operand (operand 0's n_cells words first) -> rc, and (rc 0) one fused word per cell; rc 1: a mode or an operand count the rule
//        does not take
// One line of answers per command; returns 1 on a line it cannot read.
#include "matrix_fuse.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace afis;

template <int kOp>
static uint32_t cell(const std::vector<uint32_t>& cells, const std::vector<double>& w, uint32_t n, uint32_t n_cells, uint32_t i, bool normalized, bool require_all)
{
    FuseAcc a;
    fuse_start(a);
    for (uint32_t k = 0; k < n; ++k) fuse_fold<kOp>(a, cells[(size_t)k * n_cells + i], w[k], normalized);
    return fuse_result<kOp>(a, (int)n, require_all);
}

static int fuse()
{
    uint32_t mode, normalized, n, given, n_cells;
    if (scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &mode, &normalized, &n, &given) != 4) return 1;
    if (n > 0x10000) return 1;
    std::vector<double> w(n, 1.0);                                          // (exactly n weights: a read past them is the sanitizer's to find)
    if (given)
        for (double& x : w) { uint64_t bits; if (scanf("%" SCNx64, &bits) != 1) return 1; x = __builtin_bit_cast(double, bits); }
    if (scanf("%" SCNx32, &n_cells) != 1 || n_cells > 0x1000000) return 1;
    std::vector<uint32_t> cells((size_t)n * n_cells);
    for (uint32_t& c : cells) if (scanf("%" SCNx32, &c) != 1) return 1;
    if (!fuse_mode_valid((int)mode) || n < 1 || n > (uint32_t)kFuseOperandsMax) { printf("1\n"); return 0; }
    const bool all = (mode & (uint32_t)kFuseRequireAll) != 0;
    printf("0");
    for (uint32_t i = 0; i < n_cells; ++i) {
        const int op = (int)(mode & 3);
        const uint32_t r = op == kFuseSum ? cell<kFuseSum>(cells, w, n, n_cells, i, normalized != 0, all)
                         : op == kFuseMax ? cell<kFuseMax>(cells, w, n, n_cells, i, normalized != 0, all) : cell<kFuseMin>(cells, w, n, n_cells, i, normalized != 0, all);
        printf(" %" PRIx32, r);
    }
    printf("\n");
    return 0;
}

int main()
{
    char op[8];
    while (scanf("%7s", op) == 1) {
        if (!strcmp(op, "fuse")) {
            if (fuse() != 0) return 1;
        } else return 1;
    }
    return 0;
}
