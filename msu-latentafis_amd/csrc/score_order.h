// score_order.h — the order of scores, defined once for the host and the device.  Standard library only: usable from g++ alone (rank_order.h includes it).
//
// The ORDERED WORD of a score word is a bijection of its 32 bits whose unsigned order is the total order of the floats' bits: -NaN < -inf < ... < -0.0 < +0.0 < ... <
// +inf < +NaN.  Two keys are made of it, and which one a path compares is stated by the function it calls:
//   rank_key(s)      the ordered word of s + 0.0f: the two zeros are one value.  Every TEMPLATE rank list and hit list compares it — k_topk (minu.hip), k_rank_hits'
//                    template form (rank_hits.hip), the case folds (case_fuse.hip), the list kernels' selections (graph.hip), the host's rank lists (rank_order.h)
//   ordered_word(s)  the raw word: -0.0 ranks below +0.0.  The composites of k_subject_best (subject_rank.hip), and so the thresholds of the subject hit lists, carry
//                    it, and adc_refine.hip's selection by bounds compares it.  (Every unit honours signed zeros, -ffp-contract=off: the compiler keeps the + 0.0f.)
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define AFIS_ORDER_FN __host__ __device__ __forceinline__
#else
#define AFIS_ORDER_FN inline
#endif

namespace afis {

AFIS_ORDER_FN uint32_t ordered_word(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
// the score word whose ordered word is `word`
AFIS_ORDER_FN uint32_t score_bits_of(uint32_t word) { return (word & 0x80000000u) ? (word ^ 0x80000000u) : ~word; }
AFIS_ORDER_FN uint32_t ordered_word(float s) { return ordered_word(__builtin_bit_cast(uint32_t, s)); }
AFIS_ORDER_FN uint32_t rank_key(float s) { return ordered_word(s + 0.0f); }   // -0.0 -> +0.0, so that equal floats get equal keys
// rank_key(s) >= rank_key(+0.0f), which is: the sign bit of s + 0.0f is clear
AFIS_ORDER_FN bool reaches_zero(float s) { return !(__builtin_bit_cast(uint32_t, s + 0.0f) & 0x80000000u); }

// a list entry as one 64-bit word: the greatest composite is the best word at the LOWEST position; 0 is no entry (a float's ordered word is >= 1 where a kernel makes one)
AFIS_ORDER_FN uint64_t rank_composite(uint32_t word, uint32_t position) { return ((uint64_t)word << 32) | (uint32_t)~position; }
AFIS_ORDER_FN uint32_t composite_word(uint64_t c) { return (uint32_t)(c >> 32); }
AFIS_ORDER_FN uint32_t composite_position(uint64_t c) { return ~(uint32_t)c; }
// c's word at another position: a composite over positions re-keyed by the slot it sits in
AFIS_ORDER_FN uint64_t composite_at(uint64_t c, uint32_t position) { return (c & 0xffffffff00000000ull) | (uint32_t)~position; }

// The score word that stands for "no entry" in a matrix k_rank_hits ranks (a cell a filter took out, a subject the search did not cover): a NaN with the sign
// set whose ordered word is 0.  k_rank_hits takes thr >= 1 — the ordered word of -inf is 0x007fffff, and a decision score is a number — so the cell is neither
// counted nor listed whatever min_score is.
constexpr uint32_t kNoEntryWord = 0xffffffffu;

}  // namespace afis
