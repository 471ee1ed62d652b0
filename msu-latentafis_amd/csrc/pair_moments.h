// pair_moments.h — the moments of a pair's surviving correspondences and the rigid placement they give, defined once for the host and the device.  Standard library
// only: usable from g++ alone.  The kernel (pair_evidence.hip) and the host units (through afis_ctx.h: afis_evidence.cpp has the two host helpers) share this text.
//
// Over the survivors (l, r) of one scorer — l = (lx, ly) the latent's point, r = (rx, ry) the print's —, in PIXELS: a minutia's coordinates as the template stores them,
// a texture point's block coordinates b as 16 b + 24 (mom_texture_px):
//   n                    the survivors
//   slx, sly, srx, sry   the sums of the coordinates
//   dot   = sum (lx rx + ly ry)        cross = sum (lx ry - ly rx)
//   ll    = sum (lx^2 + ly^2)          rr    = sum (rx^2 + ry^2)
// A scorer that did not run, or left no survivor, is all zeros.  Integers, so that a record does not depend on the order of the sums: records of disjoint survivor sets
// ADD, bit for bit (mom_add pools scorers — all four of a pair into one placement).
//
// THE BOUND: coordinates are int16 in the templates, so |c| <= kMomMaxCoord = 16 x 32767 + 24 = 524 296 < 2^19 + 2^4 in pixels, and a record — one scorer's, or a sum of
// records — has 0 <= n <= kMomMaxPoints = 560 (3 x 120 minutiae survivors + 200 texture survivors).  Then
//   |slx|, |sly|, |srx|, |sry|  <= 560 x 524 296      < 2^29
//   |dot|, |cross|, ll, rr      <= 560 x 2 x 524 296^2 < 2^50     (ll, rr >= 0)
// and, in mom_fit, n x dot, n x cross, n x ll, n x rr < 2^60 and every product of two sums < 2^58: all of it inside 64 bits; the fit carries them in 128 anyway.
// mom_in_bound checks it; mom_add refuses a sum beyond it.
//
// The rigid least-squares placement r ~ R l + t, R = [[c, -s], [s, c]] (mom_fit):
//   P = n dot - (slx srx + sly sry),  Q = n cross - (slx sry - sly srx)        exact integers
//   p, q = the correctly rounded doubles of P, Q;  h = sqrt(p p + q q);  c = p / h;  s = q / h
//   tx = (srx - (c slx - s sly)) / n;  ty = (sry - (s slx + c sly)) / n
//   U = n ll - slx^2 - sly^2,  V = n rr - srx^2 - sry^2                          exact integers (n^2 x the two point sets' scatter about their centroids)
//   rms = sqrt(max(0, double(U + V) - 2 h)) / n                                  the root mean square residual of the placed points
// Every fp64 operation is one correctly rounded operation — no fused multiply-add: -ffp-contract=off, as score_stats.h's moments are built.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define AFIS_MOM_FN __host__ __device__ inline
#else
#define AFIS_MOM_FN inline
#endif

namespace afis {

constexpr int64_t kMomMaxPoints = 560;
constexpr int64_t kMomMaxCoord = 16 * 32767 + 24;
constexpr int kMomWords = 9;

// the layout of afis_corr_moments (include/afis_matcher.h), 72 bytes
struct CorrMoments { int64_t n, slx, sly, srx, sry, dot, cross, ll, rr; };

AFIS_MOM_FN int64_t mom_texture_px(int b) { return 16 * (int64_t)b + 24; }

// one survivor into a record (a lane's, a wave's or a pair's: every word is a sum, so records combine word by word)
AFIS_MOM_FN void mom_point(CorrMoments& m, int64_t lx, int64_t ly, int64_t rx, int64_t ry)
{
    ++m.n; m.slx += lx; m.sly += ly; m.srx += rx; m.sry += ry;
    m.dot += lx * rx + ly * ry; m.cross += lx * ry - ly * rx;
    m.ll += lx * lx + ly * ly; m.rr += rx * rx + ry * ry;
}

// ---- the host helpers' arithmetic (afis_corr_moments_add, afis_alignment_fit): 0, or -1 where the ABI answers AFIS_EINVAL with the outputs unchanged ----
inline bool mom_in_bound(const CorrMoments& m)
{
    auto mag = [](int64_t v) { return v < 0 ? -(v + 1) : v; };              // (no overflow at INT64_MIN)
    const int64_t s_max = kMomMaxPoints * kMomMaxCoord, p_max = 2 * s_max * kMomMaxCoord;
    return m.n >= 0 && m.n <= kMomMaxPoints && mag(m.slx) <= s_max && mag(m.sly) <= s_max && mag(m.srx) <= s_max && mag(m.sry) <= s_max &&
           mag(m.dot) <= p_max && mag(m.cross) <= p_max && m.ll >= 0 && m.ll <= p_max && m.rr >= 0 && m.rr <= p_max;
}

// field by field; -1 where an operand or the sum is outside the bound
inline int mom_add(CorrMoments& acc, const CorrMoments& o)
{
    if (!mom_in_bound(acc) || !mom_in_bound(o)) return -1;
    const CorrMoments sum{acc.n + o.n, acc.slx + o.slx, acc.sly + o.sly, acc.srx + o.srx, acc.sry + o.sry, acc.dot + o.dot, acc.cross + o.cross, acc.ll + o.ll, acc.rr + o.rr};
    if (!mom_in_bound(sum)) return -1;
    acc = sum;
    return 0;
}

// -1 for a record outside the bound, fewer than two points, or points that fix no rotation (P = Q = 0: all latent points, or all print points, coincide); every output may be NULL
inline int mom_fit(const CorrMoments& m, double* c_out, double* s_out, double* tx_out, double* ty_out, double* rms_out)
{
    typedef __int128 i128;
    if (!mom_in_bound(m) || m.n < 2) return -1;
    const i128 n = m.n, slx = m.slx, sly = m.sly, srx = m.srx, sry = m.sry;
    const i128 P = n * m.dot - (slx * srx + sly * sry), Q = n * m.cross - (slx * sry - sly * srx);
    if (P == 0 && Q == 0) return -1;
    const i128 U = n * m.ll - slx * slx - sly * sly, V = n * m.rr - srx * srx - sry * sry;
    const double p = (double)P, q = (double)Q, nd = (double)m.n;
    const double pp = p * p, qq = q * q, h = std::sqrt(pp + qq);
    const double c = p / h, s = q / h;
    const double cx = c * (double)m.slx, sy = s * (double)m.sly, sx = s * (double)m.slx, cy = c * (double)m.sly;
    const double tx = ((double)m.srx - (cx - sy)) / nd, ty = ((double)m.sry - (sx + cy)) / nd;
    const double res = (double)(U + V) - 2.0 * h;
    const double rms = std::sqrt(res > 0.0 ? res : 0.0) / nd;
    if (c_out) *c_out = c;
    if (s_out) *s_out = s;
    if (tx_out) *tx_out = tx;
    if (ty_out) *ty_out = ty;
    if (rms_out) *rms_out = rms;
    return 0;
}

}  // namespace afis
