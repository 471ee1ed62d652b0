// score_hist_check.cpp — score_hist.h's bin rule and select step as a program of its own, built with the host sanitizers (Makefile: score_hist_check) and run directly
// by tests/test_score_hist_host.py, which holds its answers against numpy (searchsorted on the keys, a sorted model of the counts).
// Reads commands from stdin, every number in hex:
//   bins <n_edges> <edge word> ... <n_cells> <cell word> ...   hist_edge_keys, then hist_bin per cell -> rc, and (rc 0) one bin per cell, ffffffff for no entry
//   pbins <n_edges> <edge word> ... <n_cells> <score word> ...  the person form (score_cell.h: PersonCell), held against numpy by tests/test_subject_distributions_host.py:
//                                                               hist_edge_keys by the raw ordered word, then per person whose best cell holds the score word — whose
//                                                               person cell is that word's ordered word, as k_subject_best makes it — hist_bin -> as bins
//   step <remain> <256 counts>                                  select_step -> the digit (ffffffff: none) and the residual
//   digits <n>                                                  select_position_digits -> the digits
// One line of answers per command; returns 1 on a line it cannot read.
#include "score_hist.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace afis;

// the rest of a bins / pbins line; person: the words read are score words, and a cell is the ordered word of one
template <class Cell>
static int bins(bool person)
{
    uint32_t n_edges, n_cells;
    if (scanf("%" SCNx32, &n_edges) != 1 || n_edges < 1 || n_edges > (uint32_t)kHistEdgesMax) return 1;
    std::vector<float> edges(n_edges);
    for (float& e : edges) { uint32_t w; if (scanf("%" SCNx32, &w) != 1) return 1; e = __builtin_bit_cast(float, w); }
    if (scanf("%" SCNx32, &n_cells) != 1) return 1;
    std::vector<uint32_t> cells(n_cells), keys(n_edges);                        // (exactly n_edges keys: a read past them is the sanitizer's to find)
    for (uint32_t& c : cells) { if (scanf("%" SCNx32, &c) != 1) return 1; if (person) c = person_cell(rank_composite(ordered_word(c), 0)); }
    const int rc = hist_edge_keys<Cell>(edges.data(), (int)n_edges, keys.data());
    printf("%d", rc);
    if (rc == 0) {
        const int top = hist_top_step((int)n_edges);
        for (uint32_t c : cells) printf(" %" PRIx32, (uint32_t)hist_bin<Cell>(keys.data(), (int)n_edges, top, c));
    }
    printf("\n");
    return 0;
}

int main()
{
    char op[8];
    while (scanf("%7s", op) == 1) {
        if (!strcmp(op, "bins")) {
            if (bins<ScoreCell>(false) != 0) return 1;
        } else if (!strcmp(op, "pbins")) {
            if (bins<PersonCell>(true) != 0) return 1;
        } else if (!strcmp(op, "step")) {
            uint64_t remain, counts[kSelectBins];
            if (scanf("%" SCNx64, &remain) != 1) return 1;
            for (uint64_t& c : counts) if (scanf("%" SCNx64, &c) != 1) return 1;
            const int d = select_step(counts, &remain);
            printf("%" PRIx32 " %" PRIx64 "\n", (uint32_t)d, remain);
        } else if (!strcmp(op, "digits")) {
            uint64_t n;
            if (scanf("%" SCNx64, &n) != 1) return 1;
            printf("%d\n", select_position_digits((int64_t)n));
        } else return 1;
    }
    return 0;
}
