// score_cell.h — what a 4-byte cell of a matrix IS to the distribution and statistics kernels, defined once for the host and the device.  Standard library only
// (score_order.h is): usable from g++ alone.  score_hist.h and score_stats.hip take one of the two as a compile-time policy; the counting bodies are the same.
//
//   ScoreCell    a score word of a search's matrix (or of its filtered or transposed copy).  Its key is rank_key: the two zeros are one value, as in every template
//                list.  No entry: kNoEntryWord.
//   PersonCell   the high half K of a composite of ctx->subj_best [n_q][S] as k_subject_best, and the drops behind it, left it: the raw ordered word of the best
//                eligible covered cell of a person (subject_rank.hip).  The cell is its own key — -0.0 stands below +0.0, exactly as the subject hit lists compare —
//                and the person's score word is score_bits_of(K).  No entry: 0 — a person the search did not cover, one the query excludes, one whose every
//                template is ineligible or holds 0xffffffff (whose ordered word is 0); score_bits_of(0) is kNoEntryWord, so the statistics see no entry there too.
// An edge of a histogram is keyed the way the cells it cuts are: edge_key.
#pragma once
#include <cstdint>

#include "score_order.h"

namespace afis {

struct ScoreCell {
    static constexpr uint32_t kNone = kNoEntryWord;
    static AFIS_ORDER_FN uint32_t key(uint32_t cell) { return rank_key(__builtin_bit_cast(float, cell)); }
    static AFIS_ORDER_FN uint32_t word(uint32_t cell) { return cell; }       // the score word the statistics classify
    static AFIS_ORDER_FN uint32_t edge_key(float edge) { return rank_key(edge); }
};

struct PersonCell {
    static constexpr uint32_t kNone = 0;
    static AFIS_ORDER_FN uint32_t key(uint32_t cell) { return cell; }
    static AFIS_ORDER_FN uint32_t word(uint32_t cell) { return score_bits_of(cell); }
    static AFIS_ORDER_FN uint32_t edge_key(float edge) { return ordered_word(edge); }
};

// the person cell of a composite of subj_best
AFIS_ORDER_FN uint32_t person_cell(uint64_t best) { return composite_word(best); }

}  // namespace afis
