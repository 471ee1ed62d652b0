"""Cohort statistics and z-normalised scores without a GPU: the five entry points are declared, exported by both libraries and bound by the Python host; the kernels and
the host unit are product objects; the two options are documented; csrc/score_stats.h's host arithmetic — built with g++ under the host sanitizers as score_stats_check —
is held against Python integers (sums), float(int) and math.sqrt (moments) and numpy fp64 arithmetic (q, z); the C helpers refuse what the header says they refuse;
host/sharding.py::merge_score_stats over 1, 2 and 8 cuts of one matrix equals the uncut statistic.  Everything is exact: there is no tolerance anywhere.
(What the device answers is tests/test_gpu_score_stats.py's.)"""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NEW = {"afis_score_stats": 8, "afis_normalize_scores": 6, "afis_score_stat_add": 2, "afis_score_stat_remove": 2, "afis_score_stat_moments": 3}
OPTIONS = ("score_stats_us", "normalize_us")
SEED = 7741
EINVAL = -1
MAX_CELLS = 1 << 27
TOP = np.uint32(0x477fffff).view(np.float32)                                # the greatest valued float, 65536 - 2^-8
NO_ENTRY = 0xffffffff
M64 = (1 << 64) - 1
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0xbf800000, 0x47800000, 0x477fffff, 0x35000000, 0x35c00000, NO_ENTRY],
                   np.uint32)                                               # +-0, +-inf, +-NaN, -1, 65536, the float below it, 2^-21 and 1.5 x 2^-20 (the two rounding ties), no entry


# ---- the model: numpy and Python integers --------------------------------------------------------------------------------------------------------------
def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def classes(x):
    """(no entry, valued, outside) masks of float32 cells."""
    x = np.asarray(x, np.float32)
    none = x.view(np.uint32) == np.uint32(NO_ENTRY)
    with np.errstate(invalid="ignore"):
        valued = ~none & np.isfinite(x) & ~np.signbit(x + np.float32(0.0)) & (x < np.float32(65536.0))
    return none, valued, ~none & ~valued


def quant(v):
    return np.rint(np.asarray(v, np.float32).astype(np.float64) * 2 ** 20).astype(np.int64)


def model_stat(cells):
    """(n, n_outside, s1, s2, min word, max word) of a set of float32 cells; sums in Python int."""
    cells = np.asarray(cells, np.float32).reshape(-1)
    _, valued, outside = classes(cells)
    q = [int(t) for t in quant(cells[valued])]
    v = cells[valued] + np.float32(0.0)
    if len(v):
        key = ordered(v.view(np.uint32))
        lo, hi = int(v[key.argmin()].view(np.uint32)), int(v[key.argmax()].view(np.uint32))
    else:
        lo, hi = 0x7f800000, 0xff800000
    return (len(q), int(outside.sum()), sum(q), sum(t * t for t in q), lo, hi)


def model_moments(n, s1, s2):
    if n == 0:
        return 0.0, 0.0
    return float(s1) / (float(n) * 1048576.0), math.sqrt(float(n * s2 - s1 * s1)) / (float(n) * 1048576.0)


def dbits(x):
    return int(np.float64(x).view(np.uint64))


def as_struct(t):
    out = np.zeros(1, M.SCORE_STAT)
    out[0] = (t[0], t[1], t[2], t[3] & M64, t[3] >> 64, np.uint32(t[4]).view(np.float32), np.uint32(t[5]).view(np.float32))
    return out


def of_struct(e):
    return (int(e["n"]), int(e["n_outside"]), int(e["s1"]), (int(e["s2_hi"]) << 64) | int(e["s2_lo"]), int(e["min"].view(np.uint32)), int(e["max"].view(np.uint32)))


# ---- declared, exported, bound, built, documented ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*int64_t\s+n,\s*n_outside;\s*uint64_t\s+s1,\s*s2_lo,\s*s2_hi;\s*float\s+min,\s*max;\s*\}\s*afis_score_stat;", code)
    assert M.SCORE_STAT.itemsize == 48 and SH.SCORE_STAT == M.SCORE_STAT
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        for name, n_args in NEW.items():
            assert re.search(r"\bint\s+%s\s*\(" % name, code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert len(getattr(lib, name).argtypes) == n_args, name
    for method in ("score_stats", "normalize_scores", "score_moments"):
        assert hasattr(M.Matcher, method), method
    assert hasattr(SH, "merge_score_stats") and hasattr(SH, "trim_score_stats")
    assert hdr.index("int afis_count_before(") < hdr.index("int afis_score_stats(") < hdr.index("int afis_rank_case_hits(")   # a block of its own after the rank positions
    block = hdr[hdr.index("/* Cohort statistics"):hdr.index("int afis_score_stats(")]
    assert "2^27" in block and "LEFT AS THEY ARE" in block                  # the bound is stated beside the struct; what _remove does not do is said


def test_the_kernels_and_the_host_unit_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "score_stats.o" in objs and "afis_normalize.o" in objs
    assert re.search(r"^all:.*\bscore_stats_check\b", mk, flags=re.M) and re.search(r"^\trm -f .*\bscore_stats_check\b", mk, flags=re.M)
    src = open(os.path.join(CSRC, "score_stats.hip")).read()
    assert "__global__" in src and "k_score_stats" in src and "k_normalize_scores" in src and '#include "score_stats.h"' in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)", src) and "unsafeAtomicAdd" not in src   # integer adds and maxima only
    for unit in ("afis_normalize.cpp", "score_stats_check.cpp"):
        assert '#include "score_stats.h"' in open(os.path.join(CSRC, unit)).read(), unit               # one text for the kernels, the host unit and the check program


def test_the_options_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only\)' % opt, hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]), opt
        assert "`%s`" % opt in integ, opt


# ---- score_stats_check against the model ----------------------------------------------------------------------------------------------------------------
def tool():
    exe = os.path.join(CSRC, "score_stats_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, "score_stats_check"], check=True)
    return exe


def run_tool(lines):
    out = subprocess.run([tool()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def fmt(t):
    return "%x %x %x %x %x %08x %08x" % (t[0], t[1], t[2], t[3] & M64, t[3] >> 64, t[4], t[5])


def parse(row):
    """(rc, statistic) of an add / rem answer."""
    v = [int(x, 16) for x in row[1:]]
    return int(row[0]), (v[0], v[1], v[2], v[3] | (v[4] << 64), v[5], v[6])


def random_cells(rng, n):
    kind = rng.integers(0, 4)
    if kind == 0:
        x = rng.uniform(0, 300, n).astype(np.float32)
    elif kind == 1:
        x = np.where(rng.random(n) < 0.9, 0.0, rng.uniform(0, 65535, n)).astype(np.float32)
    elif kind == 2:
        x = SPECIAL[rng.integers(0, len(SPECIAL), n)].view(np.float32).copy()
    else:
        x = np.full(n, TOP, np.float32)
    return x


def model_add(a, b):
    """What stat_add leaves in acc: fields added; the extremes of the operands that hold a valued cell, acc's own where neither does."""
    lo, hi = a[4], a[5]
    if b[0] > 0:
        fa = np.array([a[4], a[5], b[4], b[5]], np.uint32).view(np.float32)
        ka = ordered((fa + np.float32(0.0)).view(np.uint32))
        lo = b[4] if a[0] == 0 or ka[2] < ka[0] else a[4]
        hi = b[5] if a[0] == 0 or ka[3] > ka[1] else a[5]
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3], lo, hi)


def test_the_check_program_on_random_statistics():
    rng = np.random.default_rng(SEED)
    lines, want = [], []
    for _ in range(200):
        a = model_stat(random_cells(rng, int(rng.integers(0, 400)))); b = model_stat(random_cells(rng, int(rng.integers(0, 400))))
        lines.append("add %s %s" % (fmt(a), fmt(b))); want.append(("stat", 0, model_add(a, b)))
        u = model_stat(np.concatenate([random_cells(rng, int(rng.integers(1, 400))), rng.uniform(0, 300, 3).astype(np.float32)]))
        lines.append("mom " + fmt(u)); want.append(("mom", 0, model_moments(u[0], u[2], u[3])))
        # a scaled-up statistic: the sums of 2^k copies of the same cells, so that n x s2 and s1^2 reach far into 128 bits
        k = int(rng.integers(1, 18))
        big = (u[0] << k, u[1], u[2] << k, u[3] << k, u[4], u[5])
        lines.append("mom " + fmt(big)); want.append(("mom", 0, model_moments(big[0], big[2], big[3])))
    cells = SPECIAL.view(np.float32)
    none, valued, outside = classes(cells)
    for w, cls, q in zip(SPECIAL.tolist(), np.where(none, 0, np.where(valued, 1, 2)).tolist(), np.where(valued, quant(np.where(valued, cells, 0)), 0).tolist()):
        lines.append("q %08x" % w); want.append(("q", cls, q))
    assert quant(np.uint32(0x35000000).view(np.float32)) == 0 and quant(np.uint32(0x35c00000).view(np.float32)) == 2      # the two ties round to even
    offs, scs = rng.uniform(-50, 300, 40), np.exp(rng.uniform(-8, 8, 40))
    zin = np.concatenate([SPECIAL, rng.uniform(0, 300, 40 - len(SPECIAL)).astype(np.float32).view(np.uint32)])
    zf = zin.view(np.float32)
    _, zval, _ = classes(zf)
    with np.errstate(invalid="ignore", over="ignore"):
        zw = np.where(zval, ((zf.astype(np.float64) - offs) * scs).astype(np.float32).view(np.uint32), np.uint32(NO_ENTRY))
    for w, o, s, z in zip(zin.tolist(), offs, scs, zw.tolist()):
        lines.append("z %08x %016x %016x" % (w, dbits(o), dbits(s))); want.append(("z", z, None))
    got = run_tool(lines)
    for ln, row, (kind, a, b) in zip(lines, got, want):
        if kind == "stat":
            assert parse(row) == (a, b), ln
        elif kind == "mom":
            assert (int(row[0]), int(row[1], 16), int(row[2], 16)) == (a, dbits(b[0]), dbits(b[1])), (ln, row)
        elif kind == "q":
            assert (int(row[0]), int(row[1], 16)) == (a, b), ln
        else:
            assert int(row[0], 16) == a, (ln, row)


def test_the_check_program_on_the_extremes():
    qt = int(quant(TOP)); top_w = int(TOP.view(np.uint32))
    assert qt == (1 << 36) - (1 << 12)
    full = (MAX_CELLS, 5, MAX_CELLS * qt, MAX_CELLS * qt * qt, top_w, top_w)                 # n = 2^27 cells of the greatest valued float
    half = (MAX_CELLS // 2, 2, (MAX_CELLS // 2) * qt, (MAX_CELLS // 2) * qt * qt, top_w, top_w)
    assert full[2] < 1 << 63 and full[3] < 1 << 99 and full[0] * full[3] < 1 << 126 and full[2] ** 2 < 1 << 126
    one = model_stat(np.array([3.25], np.float32)); none = model_stat(np.array([], np.float32))
    equal = model_stat(np.full(1000, 7.125, np.float32))                                       # all cells equal: N = 0
    mixed = (MAX_CELLS, 0, (MAX_CELLS // 2) * qt, (MAX_CELLS // 2) * qt * qt, 0, top_w)        # half at the top, half zero: the largest N
    assert none == (0, 0, 0, 0, 0x7f800000, 0xff800000)
    lines = ["mom " + fmt(s) for s in (full, one, none, equal, mixed)]
    lines += ["add %s %s" % (fmt(half), fmt(half)), "add %s %s" % (fmt(full), fmt(one)), "add %s %s" % (fmt(none), fmt(one)), "add %s %s" % (fmt(one), fmt(none)),
              "add %s %s" % (fmt(none), fmt(none))]
    got = run_tool(lines)
    for row, s in zip(got[:5], (full, one, none, equal, mixed)):
        mean, sd = model_moments(s[0], s[2], s[3])
        assert (int(row[0]), int(row[1], 16), int(row[2], 16)) == (0, dbits(mean), dbits(sd)), (s, row)
    assert int(got[0][2], 16) == 0 and int(got[3][2], 16) == 0 and int(got[2][1], 16) == 0 and dbits(float(TOP)) == int(got[0][1], 16)
    assert parse(got[5]) == (0, (full[0], 4, full[2], full[3], top_w, top_w))                   # up to 2^27 adds up ...
    assert parse(got[6]) == (-1, full)                                                           # ... and one cell more is refused, acc unchanged
    assert parse(got[7]) == (0, one) and parse(got[8]) == (0, one) and parse(got[9]) == (0, none)


def test_the_check_program_on_remove_after_add():
    rng = np.random.default_rng(SEED + 1)
    lines, want = [], []
    for _ in range(100):
        base = np.concatenate([random_cells(rng, int(rng.integers(0, 300))), rng.uniform(0, 300, 2).astype(np.float32)])
        extra = [np.float32(rng.uniform(0, 65535)), TOP, np.float32(0.0), np.uint32(0x80000000).view(np.float32), np.uint32(0x35c00000).view(np.float32)][int(rng.integers(0, 5))]
        a = model_stat(base); both = model_stat(np.concatenate([base, [extra]]))
        lines.append("rem %s %08x" % (fmt(both), int(np.float32(extra).view(np.uint32))))
        want.append((0, (a[0], a[1], a[2], a[3], both[4], both[5])))          # the sums return exactly; min and max are left as they were
    st = model_stat(np.array([1.0, 2.0], np.float32))
    for w in (0xbf800000, 0x7f800000, 0x7fc00000, 0x47800000, NO_ENTRY, 0xff800000):             # -1, +inf, NaN, 65536, no entry, -inf: not valued
        lines.append("rem %s %08x" % (fmt(st), w)); want.append((-1, st))
    lines.append("rem %s %08x" % (fmt(st), int(np.float32(3.0).view(np.uint32)))); want.append((-1, st))   # s1 would go below zero
    lines.append("rem %s %08x" % (fmt(model_stat([])), 0)); want.append((-1, model_stat([])))                # n would
    got = run_tool(lines)
    for ln, row, w in zip(lines, got, want):
        assert parse(row) == w, ln


# ---- the C helpers themselves (host only: no context, no device) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [M.LIB_PATH, M.TEST_LIB_PATH])
def test_the_abi_helpers_refuse_what_the_header_says(path):
    lib = M.load_library(path)
    p = lambda a: C.c_void_p(a.ctypes.data)
    qt = int(quant(TOP)); top_w = int(TOP.view(np.uint32))
    full = as_struct((MAX_CELLS, 0, MAX_CELLS * qt, MAX_CELLS * qt * qt, top_w, top_w)); one = as_struct(model_stat(np.array([2.5], np.float32)))
    before = full.tobytes()
    assert lib.afis_score_stat_add(p(full), p(one)) == EINVAL and full.tobytes() == before      # past 2^27
    acc = as_struct(model_stat(np.array([], np.float32)))
    cells = np.array([0.0, 1.5, 299.0, 7.0], np.float32)
    for lo in range(0, 4, 2):
        part = as_struct(model_stat(cells[lo:lo + 2]))
        assert lib.afis_score_stat_add(p(acc), p(part)) == 0
    assert of_struct(acc[0]) == model_stat(cells)
    before = acc.tobytes()
    for bad in (-1.0, float("inf"), float("nan"), 65536.0, float("-inf")):                         # an outside score
        assert lib.afis_score_stat_remove(p(acc), bad) == EINVAL and acc.tobytes() == before
    assert lib.afis_score_stat_remove(p(acc), 299.0) == 0
    left = model_stat(cells[[0, 1, 3]]); all4 = model_stat(cells)
    assert of_struct(acc[0]) == (left[0], left[1], left[2], left[3], all4[4], all4[5])
    mean, sd = C.c_double(), C.c_double()
    assert lib.afis_score_stat_moments(p(acc), C.byref(mean), C.byref(sd)) == 0
    assert (dbits(mean.value), dbits(sd.value)) == tuple(dbits(x) for x in model_moments(left[0], left[2], left[3]))
    assert lib.afis_score_stat_add(None, p(one)) == EINVAL and lib.afis_score_stat_moments(p(acc), None, C.byref(sd)) == EINVAL


# ---- merge_score_stats and trim_score_stats against the uncut statistic -------------------------------------------------------------------------------------
def stats_of(matrix):
    out = np.zeros(matrix.shape[0], M.SCORE_STAT)
    for i in range(matrix.shape[0]):
        out[i] = as_struct(model_stat(matrix[i]))[0]
    return out


@pytest.mark.parametrize("cuts", [1, 2, 8])
def test_merge_score_stats_over_cuts_equals_the_uncut_statistic(cuts):
    rng = np.random.default_rng([SEED, cuts])
    G, n_q = 403, 5
    m = rng.uniform(0, 300, (n_q, G)).astype(np.float32)
    m[1] = SPECIAL[rng.integers(0, len(SPECIAL), G)].view(np.float32)
    m[2] = 0.0
    m[3] = TOP
    m[4] = -1.0                                                              # no valued cell anywhere
    edge = np.r_[0, np.sort(rng.permutation(np.arange(1, G))[:cuts - 1]), G] if cuts > 1 else np.array([0, G])
    if cuts == 8:
        edge[3] = edge[2]                                                    # an empty shard
    per = np.stack([stats_of(m[:, int(edge[r]):int(edge[r + 1])]) for r in range(cuts)])
    got = SH.merge_score_stats(per)
    assert got.dtype == M.SCORE_STAT and got.tobytes() == stats_of(m).tobytes()
    assert np.isposinf(got["min"][4]) and np.isneginf(got["max"][4]) and got["n"][4] == 0 and got["n_outside"][4] == G
    with pytest.raises(ValueError):
        SH.merge_score_stats(np.stack([as_struct((MAX_CELLS, 0, 0, 0, 0, 0)), as_struct((1, 0, 0, 0, 0, 0))]))
    # a cohort trimmed by its best k cells: integer arithmetic over a top-k
    k = 7
    top = [np.sort(row[classes(row)[1]])[::-1][:k] for row in m]
    trimmed = SH.trim_score_stats(got, [np.r_[t, np.float32(-np.inf), np.float32(-1.0)] for t in top])    # (a list's padding is skipped)
    for i in range(n_q):
        row = m[i]; _, valued, _ = classes(row)
        rest = np.sort(row[valued])[::-1][k:]
        w = model_stat(np.r_[rest, row[~valued]]); full = model_stat(row)
        assert of_struct(trimmed[i]) == (w[0], w[1], w[2], w[3], full[4], full[5]), i
    with pytest.raises(ValueError):
        SH.trim_score_stats(got[4:5], [[np.float32(1.0)]])
