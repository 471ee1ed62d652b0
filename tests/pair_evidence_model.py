"""The model of the evidence calls (afis_texture_correspondences_pairs, afis_pair_alignments, afis_alignment_fit): the moments of a correspondence list in Python
integers, the rigid placement evaluated EXACTLY (integers, fractions, and decimal at 80 digits for the one square root), and the error bounds the fp64 fit of
csrc/pair_moments.h is held to.  Nothing here reads the code under test: the bounds are counted from the operations the header of include/afis_matcher.h lists.

The fp64 fit, operation by operation (u = 2^-53: one correctly rounded operation has relative error at most u; first order, the second-order terms are covered by SLACK):
  p = fl(P), q = fl(Q)                      u each
  h = sqrt(fl(fl(p p) + fl(q q)))           p p: 2u + u, q q likewise, the sum u more: 4u under the root, so 2u, and the root's own u: 3u
  c = fl(p / h), s = fl(q / h)              u + 3u + u = 5u                                                          -> K_CS = 5, relative to the exact value
  tx = fl(fl(srx - fl(fl(c slx) - fl(s sly))) / n)        (the sums are below 2^53: their conversions are exact)
       c slx: (5 + 1) u |slx| as |c| <= 1, s sly: 6u |sly|; their difference: + u (|slx| + |sly|): 7u (|slx| + |sly|);
       srx - that: + u (|srx| + |slx| + |sly|); the division: + u (|srx| + |slx| + |sly|)
       in all (9 (|slx| + |sly|) + 2 |srx|) u / n <= 9u (|sl| + |sr|) / n                                            -> K_T = 9, relative to (|slx| + |sly| + |srx| + |sry|) / n
  rms = fl(sqrt(max(0, fl(fl(U + V) - 2 h))) / n)
       fl(U + V): u (U + V); 2 h: 3u x 2H <= 3u (U + V), because H^2 = P^2 + Q^2 <= U V (Cauchy-Schwarz on the centred points) and 2 sqrt(U V) <= U + V;
       the subtraction: u more of a value <= U + V: the radicand r = U + V - 2H >= 0 is known to E = 5u (U + V), absolutely                -> K_R = 5
       (the subtraction cancels: nothing better can be said relative to r itself).  |sqrt(r~) - sqrt(r)| <= min(sqrt(E), E / sqrt(r)); the root and the division add 2u
       of the result."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

FIELDS = ("n", "slx", "sly", "srx", "sry", "dot", "cross", "ll", "rr")
MAX_POINTS = 560
MAX_COORD = 16 * 32767 + 24
U = Fraction(1, 2 ** 53)
SLACK = 1 + Fraction(1, 2 ** 20)                                            # the second-order terms of the counts above (a few u^2)
K_CS, K_T, K_R = 5, 9, 5
DIGITS = 80
getcontext().prec = DIGITS


def texture_px(b):
    return 16 * np.asarray(b, np.int64) + 24


def moments(lx, ly, rx, ry):
    """The nine fields of one correspondence list (coordinates in pixels) as Python integers."""
    lx, ly, rx, ry = ([int(v) for v in np.asarray(a).reshape(-1)] for a in (lx, ly, rx, ry))
    n = len(lx)
    return (n, sum(lx), sum(ly), sum(rx), sum(ry), sum(lx[i] * rx[i] + ly[i] * ry[i] for i in range(n)), sum(lx[i] * ry[i] - ly[i] * rx[i] for i in range(n)),
            sum(lx[i] ** 2 + ly[i] ** 2 for i in range(n)), sum(rx[i] ** 2 + ry[i] ** 2 for i in range(n)))


def moments_np(lx, ly, rx, ry):
    """The same nine fields in numpy int64 — exact inside the header's bound (every sum below 2^50) — for the thousands of lists of the GPU tests."""
    lx, ly, rx, ry = (np.asarray(a, np.int64).reshape(-1) for a in (lx, ly, rx, ry))
    return (len(lx), int(lx.sum()), int(ly.sum()), int(rx.sum()), int(ry.sum()), int((lx * rx + ly * ry).sum()), int((lx * ry - ly * rx).sum()),
            int((lx * lx + ly * ly).sum()), int((rx * rx + ry * ry).sum()))


def moments_of_xy(xy, texture=False):
    """... of an [n][4] array of (lx, ly, rx, ry) as the correspondence calls export it: minutiae in pixels, texture in blocks."""
    xy = np.asarray(xy, np.int64).reshape(-1, 4)
    if texture:
        xy = texture_px(xy)
    return moments_np(xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3])


def add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def in_bound(m):
    s_max = MAX_POINTS * MAX_COORD
    p_max = 2 * s_max * MAX_COORD
    return (0 <= m[0] <= MAX_POINTS and all(abs(v) <= s_max for v in m[1:5]) and abs(m[5]) <= p_max and abs(m[6]) <= p_max and 0 <= m[7] <= p_max and 0 <= m[8] <= p_max)


def exact_terms(m):
    n, slx, sly, srx, sry, dot, cross, ll, rr = m
    P = n * dot - (slx * srx + sly * sry)
    Q = n * cross - (slx * sry - sly * srx)
    Uu = n * ll - slx * slx - sly * sly
    V = n * rr - srx * srx - sry * sry
    return P, Q, Uu, V


def exact_fit(m):
    """(c, s, tx, ty, rms) as Decimals at DIGITS digits (the square roots are the only inexact steps, at 1e-80 relative), or None where the header refuses the record."""
    n, slx, sly, srx, sry = m[:5]
    if n < 2 or not in_bound(m):
        return None
    P, Q, Uu, V = exact_terms(m)
    if P == 0 and Q == 0:
        return None
    H = Decimal(P * P + Q * Q).sqrt()
    c, s = Decimal(P) / H, Decimal(Q) / H
    tx = (Decimal(srx) - (c * slx - s * sly)) / n
    ty = (Decimal(sry) - (s * slx + c * sly)) / n
    r = Decimal(Uu + V) - 2 * H
    rms = (r if r > 0 else Decimal(0)).sqrt() / n
    return c, s, tx, ty, rms


def bounds(m):
    """The absolute error bounds of (c, s, tx, ty, rms) for the record m, as Decimals (see the module's docstring)."""
    n, slx, sly, srx, sry = m[:5]
    P, Q, Uu, V = exact_terms(m)
    c, s, tx, ty, rms = exact_fit(m)
    u = Decimal(U.numerator) / Decimal(U.denominator) * (Decimal(SLACK.numerator) / Decimal(SLACK.denominator))
    bt = K_T * u * (abs(slx) + abs(sly) + abs(srx) + abs(sry)) / n
    E = K_R * u * (Uu + V)
    r = Decimal(Uu + V) - 2 * Decimal(P * P + Q * Q).sqrt()
    root = E.sqrt() if r <= 0 else min(E.sqrt(), E / r.sqrt())
    return K_CS * u * abs(c), K_CS * u * abs(s), bt, bt, root / n + 2 * u * (rms + root / n)


def as_record(dtype, m):
    out = np.zeros(1, dtype)
    out[0] = tuple(m)
    return out


def of_record(e):
    return tuple(int(e[f]) for f in FIELDS)


def sum_in_order(v):
    """The fp32 sum the reference forms over a survivor list (matcher.cpp:775-781)."""
    s = np.float32(0)
    for x in np.asarray(v, np.float32):
        s = np.float32(s + x)
    return s


def rotated(lx, ly, quarter_turns, tx, ty):
    """The points turned by quarter_turns x 90 degrees and moved by the integer (tx, ty): r = R l + t, R = [[c, -s], [s, c]]."""
    c, s = ((1, 0), (0, 1), (-1, 0), (0, -1))[quarter_turns % 4]
    lx, ly = np.asarray(lx, np.int64), np.asarray(ly, np.int64)
    return c * lx - s * ly + tx, s * lx + c * ly + ty, c, s


assert math.isclose(float(U), 2.0 ** -53)
