"""The cell rule of afis_matrix_fuse in numpy — the yardstick of tests/test_matrix_host.py and tests/test_gpu_matrix.py; it never calls the code under test.

For operands k = 0 .. n - 1 in argument order, c_k the cell word (the caller hands a transposed operand over already transposed), v_k its float, w_k its weight:
  there_k   c_k != 0xffffffff
  part_k    raw: there_k and the sign bit of v_k + 0 clear; normalised: there_k
  no operand there                                  -> no entry
  REQUIRE_ALL and some operand not there            -> no entry
  otherwise no operand takes part, or with REQUIRE_ALL some operand that is there does not -> -1.0
  SUM       acc = +0.0 (float64); for every k that takes part, in order: acc = acc + w_k * float64(v_k), two rounded float64 operations; float32(acc); a sum that
            is no number is the word 0x7fc00000
  MAX/MIN   the v_k of greatest / least key among those that take part, the first operand that holds it keeps its bits; a key is ordered((x + 0).view(u32))
Every array operation below is elementwise: each cell goes through the operands in order, on its own."""
import numpy as np

SUM, MAX, MIN, REQUIRE_ALL = 0, 1, 2, 4
NO_ENTRY = np.uint32(0xffffffff)
MINUS_ONE = np.uint32(0xbf800000)
NAN_WORD = np.uint32(0x7fc00000)
SIGN = np.uint32(0x80000000)
# tests/test_gpu_link_groups.py's SPECIAL: +-0, +-inf, +-NaN, -1, 65536, the float below it, two small values, no entry
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0xbf800000, 0x47800000, 0x477fffff, 0x35000000, 0x35c00000, 0xffffffff],
                   np.uint32).view(np.float32)


def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & SIGN, ~w, w | SIGN).astype(np.uint32)


def plus_zero(x):
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32)


def key_of(x):
    return ordered(plus_zero(x))


def fuse(ops, mode, normalized, weights=None):
    """ops: n float32 arrays of one shape -> the fused float32 array of that shape."""
    n = len(ops)
    op, require_all = mode & 3, bool(mode & REQUIRE_ALL)
    assert 1 <= n <= 16 and op in (SUM, MAX, MIN) and (weights is None or op == SUM)
    w = np.ones(n, np.float64) if weights is None else np.asarray(weights, np.float64)
    shape = np.asarray(ops[0]).shape
    n_there = np.zeros(shape, np.int64); n_part = np.zeros(shape, np.int64)
    acc = np.zeros(shape, np.float64)
    best = np.zeros(shape, np.uint32); best_key = np.zeros(shape, np.int64)
    with np.errstate(all="ignore"):
        for k in range(n):
            v = np.ascontiguousarray(ops[k], np.float32)
            assert v.shape == shape
            c = v.view(np.uint32)
            there = c != NO_ENTRY
            part = there if normalized else there & ((plus_zero(v) & SIGN) == 0)
            if op == SUM:
                product = np.float64(w[k]) * v.astype(np.float64)
                acc = np.where(part, acc + product, acc)
            else:
                key = key_of(v).astype(np.int64)
                take = part & ((n_part == 0) | ((key > best_key) if op == MAX else (key < best_key)))
                best = np.where(take, c, best); best_key = np.where(take, key, best_key)
            n_there += there; n_part += part
        if op == SUM:
            f = acc.astype(np.float32)
            res = np.where(np.isnan(f), NAN_WORD, f.view(np.uint32))
        else:
            res = best
    res = np.where((n_part == 0) | (require_all & (n_part != n)), MINUS_ONE, res)
    res = np.where((n_there == 0) | (require_all & (n_there != n)), NO_ENTRY, res)
    return res.astype(np.uint32).view(np.float32)


def cells(rng, shape, special=0.3, no_entry=0.12, minus_one=0.12, lo=-2.0, hi=40.0):
    """Random values in [lo, hi) with SPECIAL sprinkled over them; at least a tenth of the cells no entry and a tenth -1 (for shapes of ten cells or more)."""
    x = rng.uniform(lo, hi, shape).astype(np.float32)
    at = rng.random(shape) < special
    x[at] = SPECIAL[rng.integers(0, len(SPECIAL), shape)][at]
    flat = x.reshape(-1)
    n = flat.size
    pick = rng.permutation(n)
    n_ne, n_m1 = int(np.ceil(no_entry * n)), int(np.ceil(minus_one * n))
    flat[pick[:n_ne]] = NO_ENTRY.view(np.float32)
    flat[pick[n_ne:n_ne + n_m1]] = np.float32(-1.0)
    return x
