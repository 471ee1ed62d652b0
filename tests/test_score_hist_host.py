"""Score distributions without a GPU: the two entry points are declared, exported by both libraries, bound by the Python host and absent from the taps header; the
kernels and the host unit are product objects; the two options are documented; csrc/score_hist.h's bin rule and select step — built with g++ under the host sanitizers
as score_hist_check — are held against numpy (searchsorted on the keys, a sorted model of the counts); host/sharding.py::merge_score_histograms over 1, 2 and 8 cuts of
one matrix equals the uncut histogram, and histogram_rank_bin a sorted model.  Everything is exact: there is no tolerance anywhere.
(What the device answers is tests/test_gpu_score_hist.py's.)"""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NEW = {"afis_score_histogram": 10, "afis_entries_at": 12}
OPTIONS = ("score_histogram_us", "entries_at_us")
SEED = 9173
FLOOR = 0x007fffff                                                          # the key of -inf
NONE = 0xffffffff                                                           # the tool's word for "no bin" / "no digit"
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0xbf800000, 0x47800000, 0x477fffff, 0x35000000, 0x35c00000, 0xffffffff],
                   np.uint32)                                               # tests/test_score_stats_host.py's: +-0, +-inf, +-NaN, -1, 65536, the float below it, two small values, no entry


# ---- the model: numpy ----------------------------------------------------------------------------------------------------------------------------------
def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def key_of(words):
    with np.errstate(invalid="ignore"):
        return ordered((np.asarray(words, np.uint32).view(np.float32) + np.float32(0.0)).view(np.uint32))


def model_bins(edge_words, cell_words):
    """Per cell the bin, NONE for a cell that is no entry."""
    ek = key_of(edge_words); ck = key_of(cell_words)
    return np.where(ck >= FLOOR, np.searchsorted(ek, ck, side="right"), NONE).astype(np.int64)


def model_hist(x, edges):
    out = np.zeros((x.shape[0], len(edges) + 1), np.int64)
    for r in range(x.shape[0]):
        b = model_bins(edges.view(np.uint32), x[r].view(np.uint32))
        out[r] = np.bincount(b[b != NONE], minlength=len(edges) + 1)
    return out


# ---- declared, exported, bound, built, documented ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+AFIS_HIST_EDGES_MAX\s+1023\b", code) and re.search(r"#define\s+AFIS_HIST_COUNTS_MAX\s+\(1 << 24\)", code)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        for name, n_args in NEW.items():
            assert re.search(r"\bint\s+%s\s*\(" % name, code), name
            assert name in M.EXPORTS and name not in M.TAP_EXPORTS and hasattr(lib, name)
            assert len(getattr(lib, name).argtypes) == n_args, name
            assert name not in taps, name
    for method in ("score_histogram", "entries_at"):
        assert hasattr(M.Matcher, method), method
    assert hasattr(SH, "merge_score_histograms") and hasattr(SH, "histogram_rank_bin")
    assert hdr.index("int afis_score_stat_moments(") < hdr.index("int afis_score_histogram(") < hdr.index("int afis_entries_at(") < hdr.index("int afis_rank_case_hits(")
    block = hdr[hdr.index("/* Score distributions"):hdr.index("#define AFIS_HIST_EDGES_MAX")]
    assert "inclusive" in block and "These calls do not give" in block and "quantiles and histograms" not in hdr   # the statistics' paragraph no longer says histograms are missing


def test_the_kernels_and_the_host_unit_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "score_hist.o" in objs and "afis_distribution.o" in objs
    assert re.search(r"^all:.*\bscore_hist_check\b", mk, flags=re.M) and re.search(r"^\trm -f .*\bscore_hist_check\b", mk, flags=re.M)
    assert re.search(r"^score_hist_check:.*\n\tg\+\+ .*-fsanitize=address,undefined", mk, flags=re.M)
    src = open(os.path.join(CSRC, "score_hist.hip")).read()
    assert "__global__" in src and "k_score_hist_rows" in src and "k_select_count" in src and '#include "score_hist.h"' in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)", src) and "unsafeAtomicAdd" not in src   # integer adds only
    for unit in ("afis_distribution.cpp", "score_hist_check.cpp"):
        assert '#include "score_hist.h"' in open(os.path.join(CSRC, unit)).read(), unit                # one text for the kernels, the host unit and the check program
    dev = open(os.path.join(CSRC, "afis_device.h")).read()
    assert re.search(r"kShChunkScalar\s*=\s*256,\s*kShChunkVec\s*=\s*1024", dev) and re.search(r"kSelChunkScalar\s*=\s*1024,\s*kSelChunkVec\s*=\s*4096", dev)
    assert re.search(r"kSelTargetChunk\s*=\s*16", dev)                      # ... what tests/test_gpu_score_hist.py sizes its cases by
    norm = open(os.path.join(CSRC, "afis_normalize.cpp")).read(); dist = open(os.path.join(CSRC, "afis_distribution.cpp")).read()
    assert "column_order(" in dist and "std::sort" not in dist and "static std::vector<int32_t> column_order" not in norm   # shared, not copied


def test_the_options_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only\)' % opt, hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]), opt
        assert "`%s`" % opt in integ, opt
    assert "merge_score_histograms" in integ and "histogram_rank_bin" in integ and "afis_count_before" in integ   # the sharded quantile recipe


# ---- score_hist_check against the model -----------------------------------------------------------------------------------------------------------------
def tool():
    exe = os.path.join(CSRC, "score_hist_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, "score_hist_check"], check=True)
    return exe


def run_tool(lines):
    out = subprocess.run([tool()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def bins_line(edge_words, cell_words):
    return "bins %x %s %x %s" % (len(edge_words), " ".join("%x" % int(w) for w in edge_words), len(cell_words), " ".join("%x" % int(w) for w in cell_words))


def sorted_edges(words):
    """Distinct by key, ascending by key."""
    w = np.asarray(words, np.uint32)
    _, first = np.unique(key_of(w), return_index=True)
    return w[first]


def words_of(*floats):
    return np.array(floats, np.float32).view(np.uint32)


def test_bins_against_searchsorted():
    rng = np.random.default_rng(SEED)
    cases = []
    # every special word as a cell and, NaNs aside, as an edge: cells equal to an edge, edge +0.0 against cell -0.0 (and the other way round), edges -inf and +inf
    special_edges = sorted_edges(SPECIAL[~np.isnan(SPECIAL.view(np.float32))])
    cases.append((special_edges, SPECIAL))
    cases.append((words_of(0.0), words_of(-0.0, 0.0, -1.0, 1e-30, -1e-30)))
    cases.append((words_of(-0.0), words_of(-0.0, 0.0, -1.0)))
    cases.append((words_of(-np.inf), words_of(-np.inf, np.inf, -1.0, 0.0)))
    cases.append((np.concatenate([words_of(-np.inf), np.array([0xff7fffff], np.uint32)]), np.concatenate([words_of(-np.inf), np.array([0xff7fffff, 0xff800001, 0xffc00000], np.uint32)])))
    cases.append((words_of(np.inf), np.concatenate([words_of(np.inf, 3.0e38), np.array([0x7f800001, 0x7fffffff, 0xffffffff], np.uint32)])))
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 511, 512, 1022, 1023):        # every number of steps of the search, both sides of each power of two
        pool = np.concatenate([rng.uniform(-100, 300, 2 * n + 4).astype(np.float32).view(np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)])
        pool = pool[~np.isnan(pool.view(np.float32))]
        edges = sorted_edges(pool)
        edges = edges[np.sort(rng.choice(len(edges), n, replace=False))]
        cells = np.concatenate([edges, SPECIAL, rng.uniform(-120, 320, 300).astype(np.float32).view(np.uint32), rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32),
                                (edges.view(np.float32) * np.float32(1.0000001)).view(np.uint32)[:200]])
        cases.append((edges, cells))
    rows = run_tool([bins_line(e, c) for e, c in cases])
    for (e, c), row in zip(cases, rows):
        assert row[0] == "0", (len(e), row[:2])
        got = np.array([int(x, 16) for x in row[1:]], np.int64)
        want = model_bins(e, c)
        assert np.array_equal(got, want), (len(e), np.flatnonzero(got != want)[:4].tolist())
    both = model_bins(special_edges, SPECIAL)
    assert both[SPECIAL == 0x80000000] == both[SPECIAL == 0x00000000] and both[SPECIAL == 0xffffffff] == NONE and both[SPECIAL == 0xffc00000] == NONE
    assert both[SPECIAL == 0x7fc00000] == len(special_edges) and both[SPECIAL == 0xff800000] == 1      # +NaN reaches the last edge; -inf reaches an edge that is -inf


def test_bad_edges_are_refused():
    cell = words_of(1.0)
    bad = [words_of(0.0, np.nan), words_of(np.nan), words_of(1.0, 1.0), words_of(2.0, 1.0), words_of(-0.0, 0.0), words_of(0.0, -0.0), words_of(1.0, 2.0, 1.5), words_of(np.inf, -np.inf)]
    for e, row in zip(bad, run_tool([bins_line(e, cell) for e in bad])):
        assert row == ["-1"], e


def test_select_steps():
    """One digit of the select against a sorted model: the digits of the entries, greatest first; the entry at `remain` names the digit, and the residual is its rank among
    the entries of that digit."""
    rng = np.random.default_rng(SEED + 1)
    cases = []
    for kind in range(40):
        c = np.zeros(256, np.int64)
        if kind % 4 == 0: c[:] = rng.integers(0, 50, 256)
        elif kind % 4 == 1: c[rng.integers(0, 256)] = int(rng.integers(1, 100000))                       # all in one bin
        elif kind % 4 == 2: c[rng.integers(0, 256, 5)] = rng.integers(1, 1 << 40, 5)
        else: c[[0, 255]] = (3, 2)
        total = int(c.sum())
        for remain in sorted({0, total - 1, total, total + 7, 1 << 40} | {int(t) for t in rng.integers(0, max(total, 1), 6)}):
            if remain >= 0:
                cases.append((c, remain))
    cases.append((np.zeros(256, np.int64), 0))
    rows = run_tool(["step %x %s" % (r, " ".join("%x" % int(t) for t in c)) for c, r in cases])
    for (c, remain), row in zip(cases, rows):
        d, res = int(row[0], 16), int(row[1], 16)
        above = np.cumsum(c[::-1])[::-1]                                    # above[d]: the entries of digits d ..
        if remain >= int(c.sum()):
            assert (d, res) == (NONE, remain)
            continue
        want = int((above > remain).sum()) - 1
        assert d == want and res == remain - (int(above[want]) - int(c[want])), (remain, d, want)
        if int(c.sum()) <= 20000:
            digits = np.repeat(np.arange(256), c)[::-1]
            assert digits[remain] == d and res == remain - int((digits > d).sum())
    for n, want in ((1, 0), (2, 1), (256, 1), (257, 2), (65536, 2), (65537, 3), (1 << 24, 3), ((1 << 24) + 1, 4), (1 << 31, 4)):
        assert run_tool(["digits %x" % n]) == [[str(want)]], n


# ---- the sharding helpers -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", (1, 2, 8))
def test_cuts_add_up_to_the_uncut_histogram(cuts):
    rng = np.random.default_rng(SEED + 2 + cuts)
    n_q, G = 5, 3001
    x = rng.uniform(-20, 300, (n_q, G)).astype(np.float32)
    at = rng.random((n_q, G)) < 0.2
    x[at] = SPECIAL.view(np.float32)[rng.integers(0, len(SPECIAL), (n_q, G))][at]
    edges = np.sort(rng.uniform(-30, 310, 64).astype(np.float32))
    whole = model_hist(x, edges)
    bounds = [0] + sorted(int(t) for t in rng.choice(np.arange(1, G), cuts - 1, replace=False)) + [G]
    per = [model_hist(x[:, lo:hi], edges) for lo, hi in zip(bounds[:-1], bounds[1:])]
    merged = SH.merge_score_histograms(per)
    assert merged.dtype == np.int64 and np.array_equal(merged, whole)
    with pytest.raises(ValueError):
        SH.merge_score_histograms(per + [whole[:, :-1]])
    with pytest.raises(ValueError):
        SH.merge_score_histograms([])


def test_histogram_rank_bin_against_a_sorted_model():
    rng = np.random.default_rng(SEED + 3)
    for bins in (1, 2, 7, 64):
        c = rng.integers(0, 6, (9, bins)).astype(np.int64)
        c[1] = 0; c[2] = 0; c[2, rng.integers(0, bins)] = 11
        for rank in range(0, int(c.sum(axis=1).max()) + 2):
            b, res = SH.histogram_rank_bin(c, np.full(9, rank))
            for i in range(9):
                walk = np.repeat(np.arange(bins), c[i])[::-1]               # the bins of the row's entries, best first
                if rank < len(walk):
                    assert b[i] == walk[rank] and res[i] == rank - int((walk > walk[rank]).sum()), (bins, i, rank)
                else:
                    assert b[i] == -1 and res[i] == rank
    assert SH.histogram_rank_bin([0, 3, 0, 2], 2) == (1, 0) and SH.histogram_rank_bin([0, 3, 0, 2], 5) == (-1, 5)
    with pytest.raises(ValueError):
        SH.histogram_rank_bin([1, -1], 0)
    with pytest.raises(ValueError):
        SH.histogram_rank_bin([1, 2], -1)
