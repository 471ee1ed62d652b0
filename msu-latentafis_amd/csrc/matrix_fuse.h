// matrix_fuse.h — the cell rule of afis_matrix_fuse, defined once for the host and the device.  Standard library only: usable from g++ alone (matrix_fuse_check.cpp
// runs it as a program, tests/test_matrix_host.py holds its answers against tests/matrix_model.py).
//
// One output cell is made of the cells c_k of the operands k = 0 .. n - 1 at the same place (a transposed operand's cell is the one across the diagonal), in argument
// order; v_k is the float of c_k, w_k the operand's weight (1.0 where the call gives none):
//   there_k        c_k != kNoEntryWord
//   part_k         raw matrices: there_k && reaches_zero(v_k) — the case lists' rule (case_fuse.hip): the -1 of an empty template, every negative value and a NaN with
//                  the sign set stay out.  Normalised matrices: there_k — a negative z-score is a value, and the outside cells became no entry when the matrix
//                  was normalised
//   no k is there                                  -> kNoEntryWord
//   kFuseRequireAll and some k is not there        -> kNoEntryWord
//   otherwise no k takes part (raw only), or with kFuseRequireAll some k that is there does not take part
//                                                  -> -1.0f
//   kFuseSum       double acc = +0.0; for the k that take part, in order: acc = acc + w_k * (double)v_k — the product and the sum each rounded in fp64, no fused
//                  multiply-add (every unit that includes this header is built with -ffp-contract=off); the result is (float)acc.  A sum that is no number is the
//                  one word kFuseNaNWord: which NaN an addition or a multiplication produces (the sign of inf - inf and of 0 x inf, what is kept of an operand's
//                  payload) is the processor's choice under IEEE 754 — the word of the result is not left to it, so host and device agree
//   kFuseMax/Min   the v_k of greatest / least rank_key among those that take part; the first operand that holds it keeps its bits
// FuseAcc carries one cell through the operands; fuse_fold is written with selects, not branches, so that a kernel's loads of all operands stay in flight together.
#pragma once
#include <cstdint>

#include "score_order.h"

namespace afis {

constexpr int kFuseSum = 0, kFuseMax = 1, kFuseMin = 2;                     // AFIS_FUSE_SUM, AFIS_FUSE_MAX, AFIS_FUSE_MIN
constexpr int kFuseRequireAll = 4;                                         // AFIS_FUSE_REQUIRE_ALL, or-ed into the mode
constexpr int kFuseOperandsMax = 16;                                       // AFIS_FUSE_OPERANDS_MAX
constexpr uint32_t kFuseNaNWord = 0x7fc00000u;                             // the quiet NaN with the sign clear and no payload

AFIS_ORDER_FN bool fuse_mode_valid(int mode) { return mode >= 0 && (mode & ~(3 | kFuseRequireAll)) == 0 && (mode & 3) != 3; }

struct FuseAcc { double sum; uint32_t word, key; int n_there, n_part; };

AFIS_ORDER_FN void fuse_start(FuseAcc& a) { a.sum = 0.0; a.word = 0; a.key = 0; a.n_there = 0; a.n_part = 0; }

// operand k's cell into the accumulator; kOp: kFuseSum, kFuseMax or kFuseMin (the mode without its flag)
template <int kOp>
AFIS_ORDER_FN void fuse_fold(FuseAcc& a, uint32_t cell, double w, bool normalized)
{
    const float v = __builtin_bit_cast(float, cell);
    const bool there = cell != kNoEntryWord;
    const bool part = there && (normalized || reaches_zero(v));
    if (kOp == kFuseSum) {
        const double p = w * (double)v;                                     // rounded here ...
        const double s = a.sum + p;                                         // ... and here: two fp64 operations
        a.sum = part ? s : a.sum;
    } else {
        const uint32_t key = rank_key(v);
        const bool take = part && (a.n_part == 0 || (kOp == kFuseMax ? key > a.key : key < a.key));   // strictly: the first operand of the extreme key keeps its bits
        a.word = take ? cell : a.word; a.key = take ? key : a.key;
    }
    a.n_there += there ? 1 : 0; a.n_part += part ? 1 : 0;
}

// the cell's word after n operands
template <int kOp>
AFIS_ORDER_FN uint32_t fuse_result(const FuseAcc& a, int n, bool require_all)
{
    if (a.n_there == 0 || (require_all && a.n_there != n)) return kNoEntryWord;
    if (a.n_part == 0 || (require_all && a.n_part != n)) return 0xbf800000u;   // -1.0f
    if (kOp != kFuseSum) return a.word;
    const float f = (float)a.sum;
    return f != f ? kFuseNaNWord : __builtin_bit_cast(uint32_t, f);
}

}  // namespace afis
