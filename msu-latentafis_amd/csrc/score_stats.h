// score_stats.h — cohort statistics of score cells, defined once for the host and the device.  Standard library only (score_order.h is): usable from g++ alone.
// The kernels (score_stats.hip), the host unit (afis_normalize.cpp) and the check program (score_stats_check.cpp) share this text.
//
// A cell of a score matrix (word w, float v) is
//   no entry   w == kNoEntryWord (a filter took it out, afis_search_eligible left it unscored)
//   valued     v finite, the sign bit of v + 0.0f clear, v < 65536.0f
//   outside    everything else: -1 (empty template, empty latent), negative values, +-inf, NaN, values >= 2^16
// A valued cell is quantised to q(v) = rint(v x 2^20) under round-to-nearest-even: the product is exact in fp64 and 0 <= q < 2^36.  The statistic of a set of cells:
//   n, n_outside   the valued and the outside cells
//   s1 = sum q,  s2 = sum q^2 (128 bits: s2_lo, s2_hi)
//   min, max       the valued cells' extremes by rank_key (the two zeros are one value, +0.0); +inf / -inf while n == 0
// Integers, so that a statistic does not depend on the order of the sums or on where a gallery was cut into shards: statistics of disjoint sets ADD, bit for bit.
//
// THE BOUND: n <= kStatMaxCells = 2^27, for one statistic and for a sum of statistics.  Then s1 < 2^63, s2 < 2^99, and n x s2 and s1^2 stay below 2^126 (stat_moments);
// and the five limb sums of a kernel (stat_limbs below) stay below 2^63.  stat_add checks it where statistics are added.
//
// Moments: mean = double(s1) / (double(n) x 2^20), sd = sqrt(double(n x s2 - s1^2)) / (double(n) x 2^20) — the population deviation; double(.) the correctly rounded
// conversion of the integer; n == 0 gives (0, 0).
// A normalised cell: z = (float)(((double)v - offset) x scale), an fp64 subtraction, an fp64 multiplication (no fused multiply-add: -ffp-contract=off) and one
// conversion, for a valued cell; an outside cell becomes no entry (a template without a print has no z-score); a no-entry cell stays.
#pragma once
#include <cmath>
#include <cstdint>

#include "score_order.h"

namespace afis {

constexpr int64_t kStatMaxCells = (int64_t)1 << 27;
constexpr int kStatLimbBits = 18;                                           // q = a x 2^18 + b, a and b < 2^18
constexpr int kStatWords = 9;                                               // a row of a kernel's table: n | n_outside | sum a | sum b | sum a^2 | sum ab | sum b^2 | max ~min key | max key
enum { kCellNoEntry = 0, kCellValued = 1, kCellOutside = 2 };

// the layout of afis_score_stat (include/afis_matcher.h), 48 bytes
struct ScoreStat { int64_t n, n_outside; uint64_t s1, s2_lo, s2_hi; float min, max; };

AFIS_ORDER_FN int stat_cell_class(uint32_t w)
{
    if (w == kNoEntryWord) return kCellNoEntry;
    const float v = __builtin_bit_cast(float, w);
    const bool finite = (w & 0x7f800000u) != 0x7f800000u;
    return finite && reaches_zero(v) && v < 65536.0f ? kCellValued : kCellOutside;
}

// of a valued v
AFIS_ORDER_FN uint64_t stat_q(float v) { return (uint64_t)(int64_t)__builtin_rint((double)v * 1048576.0); }

AFIS_ORDER_FN uint32_t stat_normalized_word(uint32_t w, double offset, double scale)
{
    if (stat_cell_class(w) != kCellValued) return kNoEntryWord;
    const double d = (double)__builtin_bit_cast(float, w) - offset;
    return __builtin_bit_cast(uint32_t, (float)(d * scale));
}

// One cell into a row of limb sums t [kStatWords] (a thread's, a workgroup's or a table's: every word is a sum or a maximum, so rows combine word by word)
AFIS_ORDER_FN void stat_limbs_cell(uint64_t* t, uint32_t w)
{
    const int c = stat_cell_class(w);
    if (c == kCellOutside) ++t[1];
    if (c != kCellValued) return;
    const float v = __builtin_bit_cast(float, w);
    const uint64_t q = stat_q(v), a = q >> kStatLimbBits, b = q & (((uint64_t)1 << kStatLimbBits) - 1);
    const uint32_t key = rank_key(v);
    ++t[0]; t[2] += a; t[3] += b; t[4] += a * a; t[5] += a * b; t[6] += b * b;
    if ((uint32_t)~key > t[7]) t[7] = (uint32_t)~key;
    if (key > t[8]) t[8] = key;
}

// s1 = sum a x 2^18 + sum b;  s2 = sum a^2 x 2^36 + 2 x sum ab x 2^18 + sum b^2 in 128 bits
AFIS_ORDER_FN ScoreStat stat_from_limbs(const uint64_t* t)
{
    ScoreStat s;
    s.n = (int64_t)t[0]; s.n_outside = (int64_t)t[1];
    s.s1 = (t[2] << kStatLimbBits) + t[3];
    uint64_t lo = t[6], hi = 0, add = t[5] << (kStatLimbBits + 1);
    lo += add; hi += (lo < add) + (t[5] >> (64 - kStatLimbBits - 1));
    add = t[4] << (2 * kStatLimbBits);
    lo += add; hi += (lo < add) + (t[4] >> (64 - 2 * kStatLimbBits));
    s.s2_lo = lo; s.s2_hi = hi;
    s.min = s.n ? __builtin_bit_cast(float, score_bits_of(~(uint32_t)t[7])) : __builtin_bit_cast(float, 0x7f800000u);
    s.max = s.n ? __builtin_bit_cast(float, score_bits_of((uint32_t)t[8])) : __builtin_bit_cast(float, 0xff800000u);
    return s;
}

// ---- the host helpers' arithmetic (afis_score_stat_add / _remove / _moments): 0, or -1 where the ABI answers AFIS_EINVAL with the statistic unchanged ----
typedef unsigned __int128 stat_u128;
inline stat_u128 stat_s2(const ScoreStat& s) { return ((stat_u128)s.s2_hi << 64) | s.s2_lo; }
inline bool stat_in_bound(const ScoreStat& s)
{
    return s.n >= 0 && s.n <= kStatMaxCells && s.n_outside >= 0 && s.s1 < ((uint64_t)1 << 63) && s.s2_hi < ((uint64_t)1 << (99 - 64));
}
inline bool stat_float_before(float a, float b) { return rank_key(a) < rank_key(b); }

// field by field with carry, min of mins and max of maxes; -1 where n would pass kStatMaxCells (or an operand is outside the bound)
inline int stat_add(ScoreStat& acc, const ScoreStat& o)
{
    if (!stat_in_bound(acc) || !stat_in_bound(o) || acc.n + o.n > kStatMaxCells) return -1;
    const stat_u128 s2 = stat_s2(acc) + stat_s2(o);
    acc.n += o.n; acc.n_outside += o.n_outside; acc.s1 += o.s1;
    acc.s2_lo = (uint64_t)s2; acc.s2_hi = (uint64_t)(s2 >> 64);
    if (o.n > 0 && (acc.n == o.n || stat_float_before(o.min, acc.min))) acc.min = o.min;
    if (o.n > 0 && (acc.n == o.n || stat_float_before(acc.max, o.max))) acc.max = o.max;
    return 0;
}

// one valued cell's contribution out, exactly; min and max are left as they are (the extremes of the cells that remain are not known here).
// -1 for a score that is not valued, or where a field would go below zero
inline int stat_remove(ScoreStat& acc, float score)
{
    if (stat_cell_class(__builtin_bit_cast(uint32_t, score)) != kCellValued || !stat_in_bound(acc)) return -1;
    const uint64_t q = stat_q(score);
    const stat_u128 q2 = (stat_u128)q * q, s2 = stat_s2(acc);
    if (acc.n < 1 || acc.s1 < q || s2 < q2) return -1;
    --acc.n; acc.s1 -= q;
    acc.s2_lo = (uint64_t)(s2 - q2); acc.s2_hi = (uint64_t)((s2 - q2) >> 64);
    return 0;
}

// -1 for a statistic outside the bound, or one no set of cells has (n x s2 < s1^2)
inline int stat_moments(const ScoreStat& s, double* mean, double* sd)
{
    if (!stat_in_bound(s)) return -1;
    if (s.n == 0) { *mean = 0.0; *sd = 0.0; return 0; }
    const stat_u128 ns2 = (stat_u128)(uint64_t)s.n * stat_s2(s), s1s1 = (stat_u128)s.s1 * s.s1;
    if (ns2 < s1s1) return -1;
    const double den = (double)s.n * 1048576.0;
    *mean = (double)s.s1 / den;
    *sd = std::sqrt((double)(ns2 - s1s1)) / den;
    return 0;
}

}  // namespace afis
