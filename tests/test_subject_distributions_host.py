"""Person distributions without a GPU: the three entry points are declared, exported by both libraries, bound by the Python host and absent from the taps header; the
kernels and the host units are product objects and share one text of the cell policy; the options and the two recipes are documented; the person form of
csrc/score_hist.h's bin rule and edge keys — the `pbins` command of score_hist_check, built with g++ under the host sanitizers — is held against numpy (searchsorted on
the raw ordered words); host/sharding.py's two person merges over 1, 2 and 8 person-aligned cuts equal the uncut model and refuse a straddling id;
Matcher.expand_subject_pairs against a plain loop.  Everything is exact: there is no tolerance anywhere.
(What the device answers is tests/test_gpu_subject_distributions.py's.)"""
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
NEW = {"afis_subject_score_stats": 9, "afis_subject_score_histogram": 11, "afis_subject_entries_at": 14}
OPTIONS = ("subject_score_stats_us", "subject_score_histogram_us", "subject_entries_at_us")
SEED = 6113
FLOOR = 0x007fffff                                                          # the ordered word of -inf
NONE = 0xffffffff                                                           # the tool's word for "no bin"; the no-entry score word
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0xbf800000, 0x47800000, 0x477fffff, 0x35000000, 0x35c00000, 0xffffffff],
                   np.uint32)                                               # tests/test_score_stats_host.py's: +-0, +-inf, +-NaN, -1, 65536, the float below it, two small values, no entry


# ---- the model: numpy ----------------------------------------------------------------------------------------------------------------------------------
def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def model_bins(edge_words, best_words):
    """Per person — best_words: the score word of the person's best cell — the bin, NONE for a person that is no entry."""
    ek = ordered(edge_words); ck = ordered(best_words)
    return np.where(ck >= FLOOR, np.searchsorted(ek, ck, side="right"), NONE).astype(np.int64)


def words_of(*floats):
    return np.array(floats, np.float32).view(np.uint32)


# ---- declared, exported, bound, built, documented ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        for name, n_args in NEW.items():
            decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
            assert decl and len(decl.group(1).split(",")) == n_args, name
            assert name in M.EXPORTS and name not in M.TAP_EXPORTS and hasattr(lib, name)
            assert len(getattr(lib, name).argtypes) == n_args, name
            assert name not in taps, name
    for method in ("subject_score_stats", "subject_score_histogram", "subject_entries_at", "expand_subject_pairs"):
        assert hasattr(M.Matcher, method), method
    assert hasattr(SH, "merge_subject_score_stats") and hasattr(SH, "merge_subject_score_histograms")
    assert hdr.index("int afis_entries_at(") < hdr.index("int afis_subject_score_stats(") < hdr.index("int afis_subject_score_histogram(") < hdr.index("int afis_subject_entries_at(")
    block = hdr[hdr.index("/* Person distributions"):hdr.index("int afis_subject_score_stats(")]
    for word in ("ordered_word", "(-0.0, +0.0)", "SHARDED BY PERSON", "expand_subject_pairs", "These calls do not give", "AFIS_POS_NO_ENTRY", "subject_distribution_timing"):
        assert word in block, word
    dist = hdr[hdr.index("/* Score distributions"):hdr.index("#define AFIS_HIST_EDGES_MAX")]
    assert "These calls do not give" in dist and "persons at a rank or histograms of persons' scores" not in hdr   # the template block no longer says persons are missing


def test_the_kernels_and_the_host_units_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    for o in ("score_hist.o", "score_stats.o", "afis_distribution.o", "afis_normalize.o", "subject_rank.o"):
        assert o in objs, o
    assert re.search(r"^all:.*\bscore_hist_check\b", mk, flags=re.M) and re.search(r"^\trm -f .*\bscore_hist_check\b", mk, flags=re.M)
    assert re.search(r"^score_hist_check:.*\bscore_cell\.h\b.*\n\tg\+\+ .*-fsanitize=address,undefined", mk, flags=re.M)
    hist = open(os.path.join(CSRC, "score_hist.hip")).read(); stats = open(os.path.join(CSRC, "score_stats.hip")).read()
    assert "k_subject_keys" in hist and "k_subject_select_finish" in hist
    # one counting body, two instantiations: each kernel is defined once, and launched for both cells
    for src, kernels in ((hist, ("k_score_hist_rows", "k_select_count")), (stats, ("k_score_stats_rows", "k_score_stats_cols"))):
        for k in kernels:
            assert len(re.findall(r"__global__[^;{]*\bvoid %s\(" % k, src)) == 1, k
            assert re.search(r"%s<\w+, Cell>" % k, src), k
        assert "ScoreCell>" in src and "PersonCell>" in src
        assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)", src) and "unsafeAtomicAdd" not in src   # integer atomics only
    for unit in ("score_hist.h", "score_stats.hip"):
        assert '#include "score_cell.h"' in open(os.path.join(CSRC, unit)).read(), unit               # one text for the kernels, the host units and the check program
    for unit in ("afis_distribution.cpp", "score_hist_check.cpp", "score_hist.hip"):
        assert '#include "score_hist.h"' in open(os.path.join(CSRC, unit)).read(), unit
    dist = open(os.path.join(CSRC, "afis_distribution.cpp")).read(); norm = open(os.path.join(CSRC, "afis_normalize.cpp")).read()
    # no second definition of eligibility or of a person's best: the pre-passes are the filtered subject hit lists', queued in one place
    # ... by the matrix calls' driver (MatrixCall, afis_hits.cpp), which every person distribution call asks for the person cells and hands the filter as the hit lists do
    assert dist.count("queue_subject_best(") == 1 and dist.count("queue_drop_subjects(") == 1 and "queue_subject_best(" not in norm and "queue_subject_keys(" not in norm
    hits = open(os.path.join(CSRC, "afis_hits.cpp")).read()
    drv = hits[hits.index("int MatrixCall::begin("):]
    assert "if (cells == kPersonKeys) return queue_subject_keys(ctx, subj, fp);" in drv[:drv.index("\n}\n")] and hits.count("queue_subject_keys(") == 1
    call = "MatrixCall mc{ctx, who, subj, subj ? kPersonKeys : kTemplateCells, {ctx, labels, masks, pairs, subj != nullptr}}"
    assert dist.count(call) == 2 and norm.count(call) == 1 and "FilterPass fp{" not in dist + norm


def test_the_options_and_the_recipes_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only\)' % opt, hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]), opt
        assert "`%s`" % opt in integ, opt
    for name in NEW:
        assert "`%s`" % name in integ, name
    for word in ("merge_subject_score_stats", "merge_subject_score_histograms", "expand_subject_pairs", "sharded by person", "false person alarm"):
        assert word in integ, word
    assert "afis_subject_score_histogram" in open(os.path.join(ROOT, "README.md")).read()
    assert "k_subject_keys" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- score_hist_check's person form against the model ---------------------------------------------------------------------------------------------------
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


def pbins_line(edge_words, best_words):
    return "pbins %x %s %x %s" % (len(edge_words), " ".join("%x" % int(w) for w in edge_words), len(best_words), " ".join("%x" % int(w) for w in best_words))


def sorted_edges(words):
    """Distinct, ascending by ordered word."""
    w = np.unique(np.asarray(words, np.uint32))
    return w[np.argsort(ordered(w))]


def test_person_bins_against_searchsorted():
    rng = np.random.default_rng(SEED)
    cases = []
    # every special word as a person's best and, NaNs aside, as an edge: -0.0 and +0.0 are two edges and two values
    special_edges = sorted_edges(SPECIAL[~np.isnan(SPECIAL.view(np.float32))])
    assert 0x80000000 in special_edges and 0x00000000 in special_edges
    cases.append((special_edges, SPECIAL))
    cases.append((words_of(0.0), words_of(-0.0, 0.0, -1.0, 1e-30, -1e-30)))
    cases.append((words_of(-0.0), words_of(-0.0, 0.0, -1.0, -1e-30)))
    cases.append((words_of(-0.0, 0.0), words_of(-0.0, 0.0, -1.0, 1e-30, -1e-30)))   # accepted as a pair: three bins
    cases.append((words_of(-np.inf), words_of(-np.inf, np.inf, -1.0, 0.0)))
    cases.append((words_of(np.inf), np.concatenate([words_of(np.inf, 3.0e38), np.array([0x7f800001, 0x7fffffff, 0xffffffff, 0xff800001], np.uint32)])))
    for n in (1, 2, 63, 64, 65, 255, 256, 1023):                            # every number of steps of the search
        pool = np.concatenate([rng.uniform(-100, 300, 2 * n + 4).astype(np.float32).view(np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)])
        pool = pool[~np.isnan(pool.view(np.float32))]
        edges = sorted_edges(pool)
        edges = edges[np.sort(rng.choice(len(edges), n, replace=False))]
        cells = np.concatenate([edges, SPECIAL, rng.uniform(-120, 320, 300).astype(np.float32).view(np.uint32), rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32),
                                (edges.view(np.float32) * np.float32(1.0000001)).view(np.uint32)[:200]])
        cases.append((edges, cells))
    rows = run_tool([pbins_line(e, c) for e, c in cases])
    for (e, c), row in zip(cases, rows):
        assert row[0] == "0", (len(e), row[:2])
        got = np.array([int(x, 16) for x in row[1:]], np.int64)
        want = model_bins(e, c)
        assert np.array_equal(got, want), (len(e), np.flatnonzero(got != want)[:4].tolist())
    both = model_bins(special_edges, SPECIAL)
    assert both[SPECIAL == 0x80000000] + 1 == both[SPECIAL == 0x00000000] and both[SPECIAL == 0xffffffff] == NONE and both[SPECIAL == 0xffc00000] == NONE
    assert both[SPECIAL == 0x7fc00000] == len(special_edges) and both[SPECIAL == 0xff800000] == 1      # +NaN reaches the last edge; -inf reaches an edge that is -inf
    three = [int(x, 16) for x in rows[3][1:]]
    assert three == [1, 2, 0, 2, 0]                                         # -0.0 in its own bin between the negatives and +0.0


def test_bad_person_edges_are_refused():
    cell = words_of(1.0)
    bad = [words_of(0.0, -0.0), words_of(0.0, np.nan), words_of(np.nan), words_of(1.0, 1.0), words_of(-0.0, -0.0), words_of(2.0, 1.0), words_of(1.0, 2.0, 1.5), words_of(np.inf, -np.inf)]
    for e, row in zip(bad, run_tool([pbins_line(e, cell) for e in bad])):
        assert row == ["-1"], e
    assert run_tool([pbins_line(words_of(-0.0, 0.0), cell)])[0] == ["0", "2"]
    assert run_tool(["bins 2 80000000 0 1 3f800000"])[0] == ["-1"]          # ... which the template form refuses: there the two zeros are one value


# ---- the sharding helpers -----------------------------------------------------------------------------------------------------------------------------------
def person_words(rng, n_q, S):
    """The persons' score words of a whole gallery, about a fifth special; 0xffffffff: no cell."""
    x = rng.uniform(-20, 300, (n_q, S)).astype(np.float32).view(np.uint32)
    at = rng.random((n_q, S)) < 0.2
    x[at] = SPECIAL[rng.integers(0, len(SPECIAL), (n_q, S))][at]
    return x


def model_hist(words, edges):
    out = np.zeros((words.shape[0], len(edges) + 1), np.int64)
    for r in range(words.shape[0]):
        b = model_bins(edges.view(np.uint32), words[r])
        out[r] = np.bincount(b[b != NONE], minlength=len(edges) + 1)
    return out


def model_stats(words):
    """SCORE_STAT per row of score words (tests/test_gpu_score_stats.py's model); the sums in Python int."""
    x = words.view(np.float32)
    none = words == NONE
    with np.errstate(invalid="ignore"):
        valued = ~none & np.isfinite(x) & ~np.signbit(x + np.float32(0.0)) & (x < np.float32(65536.0))
        z = x + np.float32(0.0)
    q = np.where(valued, np.rint(np.where(valued, x, 0).astype(np.float64) * 2 ** 20).astype(np.int64), 0).astype(object)
    out = np.zeros(x.shape[0], M.SCORE_STAT)
    out["n"] = valued.sum(axis=1); out["n_outside"] = (~none & ~valued).sum(axis=1)
    out["s1"] = np.array([int(t) for t in q.sum(axis=1)], np.uint64)
    s2 = (q * q).sum(axis=1)
    out["s2_lo"] = np.array([int(t) & ((1 << 64) - 1) for t in s2], np.uint64); out["s2_hi"] = np.array([int(t) >> 64 for t in s2], np.uint64)
    out["min"] = np.where(valued, z, np.float32(np.inf)).min(axis=1, initial=np.float32(np.inf))
    out["max"] = np.where(valued, z, np.float32(-np.inf)).max(axis=1, initial=np.float32(-np.inf))
    return out


@pytest.mark.parametrize("cuts", (1, 2, 8))
def test_person_aligned_cuts_merge_to_the_uncut_model(cuts):
    rng = np.random.default_rng(SEED + 2 + cuts)
    n_q, S = 5, 301
    ids = np.sort(rng.choice(1 << 40, S, replace=False).astype(np.int64))
    words = person_words(rng, n_q, S)
    edges = np.sort(rng.uniform(-30, 310, 64).astype(np.float32))
    owner = rng.integers(0, cuts, S)                                        # the rank every person's prints lie on: a rank's ids are ascending, the ranks' lists interleave
    owner[:cuts] = np.arange(cuts)
    mine = [np.flatnonzero(owner == r) for r in range(cuts)]
    ids_per_rank = [ids[c] for c in mine]
    for axis in (0, 1):
        rows = (lambda w: w) if axis == 0 else (lambda w: np.ascontiguousarray(w.T))
        st = SH.merge_subject_score_stats([model_stats(rows(words[:, c])) for c in mine], ids_per_rank, axis)
        hs = SH.merge_subject_score_histograms([model_hist(rows(words[:, c]), edges) for c in mine], ids_per_rank, axis)
        if axis == 1:
            assert np.array_equal(st[0], ids) and np.array_equal(hs[0], ids)
            st, hs = st[1], hs[1]
        assert st.dtype == M.SCORE_STAT and st.tobytes() == model_stats(rows(words)).tobytes(), axis
        assert hs.dtype == np.int64 and np.array_equal(hs, model_hist(rows(words), edges)), axis


def test_a_straddling_id_is_refused():
    rng = np.random.default_rng(SEED + 20)
    words = person_words(rng, 3, 7)
    edges = np.array([0.0, 100.0], np.float32)
    ids = [np.array([1, 5, 9, 11], np.int64), np.array([2, 9, 30], np.int64)]   # 9: prints on both ranks
    cols = [np.arange(4), np.arange(4, 7)]
    for axis in (0, 1):
        rows = (lambda w: w) if axis == 0 else (lambda w: np.ascontiguousarray(w.T))
        with pytest.raises(ValueError, match="sharded by person"):
            SH.merge_subject_score_stats([model_stats(rows(words[:, c])) for c in cols], ids, axis)
        with pytest.raises(ValueError, match="sharded by person"):
            SH.merge_subject_score_histograms([model_hist(rows(words[:, c]), edges) for c in cols], ids, axis)
    with pytest.raises(ValueError):
        SH.merge_subject_score_histograms([], [], 0)
    with pytest.raises(ValueError):
        SH.merge_subject_score_stats([model_stats(words)], [np.arange(7)], 2)
    with pytest.raises(ValueError):
        SH.merge_subject_score_stats([model_stats(np.ascontiguousarray(words.T))], [np.arange(6)], 1)   # a row per id


def test_expand_subject_pairs():
    """Against a plain loop, on a stand-in for a matcher (the method reads its index_base) and a handle as subjects_create returns it."""
    class Host:
        index_base = 1000
    rng = np.random.default_rng(SEED + 30)
    subjects = np.sort(rng.choice(1 << 40, 50, replace=False).astype(np.int64))
    per_template = subjects[rng.integers(0, 50, 400)]                       # the person of every template, any order, cards of any size
    handle = (None, 400, np.unique(per_template), per_template)
    n = len(handle[2])
    offset = rng.uniform(0, 10, n); scale = rng.uniform(0.1, 2, n)
    where = {int(v): i for i, v in enumerate(handle[2])}
    o, s = M.Matcher.expand_subject_pairs(Host, handle, offset, scale)      # a search of the whole shard
    assert o.dtype == np.float64 and o.tolist() == [offset[where[int(c)]] for c in per_template] and s.tolist() == [scale[where[int(c)]] for c in per_template]
    listed = 1000 + rng.permutation(400)[:77]                               # a subset's list, in the caller's order
    o, s = M.Matcher.expand_subject_pairs(Host, handle, offset, scale, columns=listed)
    assert o.tolist() == [offset[where[int(per_template[g - 1000])]] for g in listed] and s.tolist() == [scale[where[int(per_template[g - 1000])]] for g in listed]
    for bad in (lambda: M.Matcher.expand_subject_pairs(Host, handle, offset[:-1], scale), lambda: M.Matcher.expand_subject_pairs(Host, handle, offset, scale, columns=[999]),
                lambda: M.Matcher.expand_subject_pairs(Host, handle, offset, scale, columns=[1400])):
        with pytest.raises(ValueError):
            bad()
