"""Pair scoring without a GPU: afis_score_pairs, the two AFIS_PAIR_* values and the chunk default are declared, the entry point is exported by both libraries and bound
by the Python host; its host unit and the pair ADC kernel are product objects; the options are documented; host/sharding.py::merge_pair_scores on hand-made per-rank
answers; and pair_tables.h — the host's tables of a chunk: the counting sort by launch group and latent, the ADC kernel's work list — through the stand-alone program
csrc/pair_tables_check, built with the host sanitizers and run as a program (nothing is loaded into this process).  What the device answers is
tests/test_gpu_score_pairs.py's."""
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
NAME = "afis_score_pairs"
VALUES = {"AFIS_PAIR_OK": 0, "AFIS_PAIR_NOT_COVERED": 1}


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, value in VALUES.items():
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), code, flags=re.M), name
    assert (M.PAIR_OK, M.PAIR_NOT_COVERED) == (0, 1) == (SH.PAIR_OK, SH.PAIR_NOT_COVERED)
    assert re.search(r"\bint\s+%s\s*\(afis_ctx\*\s*ctx,\s*afis_queries\*\s*q,\s*int64_t\s+n_pairs,\s*const int32_t\*\s*query\s*,\s*const int64_t\*\s*idx\s*,"
                     r"\s*int32_t\*\s*status\s*,\s*float\*\s*score\s*,\s*float\*\s*parts\s*\)\s*;" % NAME, code)
    default = int(re.search(r"^#define\s+AFIS_SCORE_PAIRS_PER_LAUNCH\s+(\d+)\s*$", code, flags=re.M).group(1))
    assert 1 <= default <= 1 << 20                                          # the builder's choice, written into the header ...
    dev = open(os.path.join(CSRC, "afis_device.h")).read()
    assert int(re.search(r"constexpr int kScorePairsPerLaunch = (\d+);", dev).group(1)) == default      # ... and the context's initial value (afis_pairs.cpp asserts the same)
    assert default * (5820 + 8 * 1000) <= 128 << 20                         # a chunk near 128 MB at the longest latent texture template
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        assert NAME in M.EXPORTS and hasattr(lib, NAME)
        assert len(getattr(lib, NAME).argtypes) == 8
    assert hasattr(M.Matcher, "score_pairs") and hasattr(SH, "merge_pair_scores")
    assert hdr.index("int afis_correspondences_pairs(") < hdr.index("int %s(" % NAME) < hdr.index("int afis_get_timing(")
    alone = hdr[hdr.index("leave the matrix alone") - 400:hdr.index("leave the matrix alone")]
    assert NAME in alone                                                    # on the list of calls after which the ranking calls still answer


def test_the_host_unit_and_the_pair_adc_kernel_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "afis_pairs.o" in objs and "adc_pairs.o" in objs and "graph_pairs.o" in objs
    assert "adc_direct.o" not in objs                                       # the direct kernels stay test-library kernels
    assert re.search(r"^adc_pairs\.o:.*pair_tables\.h", mk, flags=re.M) and re.search(r"^afis_pairs\.o:.*pair_tables\.h", mk, flags=re.M)
    assert "-ffp-contract=off" in re.search(r"^CXXFLAGS\s*=(.*)$", mk, flags=re.M).group(1)          # no contraction: the four chains round as the reference's


def test_the_options_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    block = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    assert '"score_pairs_per_launch"' in block and re.search(r'"score_pairs_us" \(read-only\)', block)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`score_pairs_per_launch`" in doc and "`score_pairs_us`" in doc and "`%s`" % NAME in doc


# ---- merge_pair_scores --------------------------------------------------------------------------------------------------------------------------------
def _rank_answer(rng, covered, n_pairs, parts=True):
    """One rank's answer: the pairs of `covered` with made-up scores, every other pair AFIS_PAIR_NOT_COVERED / -inf / zeros."""
    st = np.full(n_pairs, SH.PAIR_NOT_COVERED, np.int32); sc = np.full(n_pairs, -np.inf, np.float32); pt = np.zeros((n_pairs, 4), np.float32)
    for p in covered:
        st[p] = SH.PAIR_OK
        sc[p] = -1.0 if rng.random() < 0.3 else rng.random() * 100             # (-1: a pair the reference does not score is still covered)
        pt[p] = rng.random(4)
    return {"status": st, "score": sc, "parts": pt if parts else None}


def test_merge_takes_every_pair_from_the_rank_that_covers_it():
    rng = np.random.default_rng(41)
    P = 9
    owners = [0, 2, 1, 1, 0, 2, 2, 0, 1]                                    # disjoint: every pair covered by exactly one of three ranks
    ranks = [_rank_answer(rng, [p for p in range(P) if owners[p] == r], P) for r in range(3)]
    out = SH.merge_pair_scores(ranks)
    assert out["owner"].tolist() == owners and (out["status"] == SH.PAIR_OK).all()
    for p in range(P):
        src = ranks[owners[p]]
        assert out["score"][p].tobytes() == src["score"][p].tobytes() and out["parts"][p].tobytes() == src["parts"][p].tobytes()
    for r in ranks:
        r["parts"] = None                                                   # without parts
    out2 = SH.merge_pair_scores(ranks)
    assert out2["parts"] is None and out2["score"].tobytes() == out["score"].tobytes() and out2["owner"].tolist() == owners


def test_merge_marks_a_pair_no_rank_covers():
    rng = np.random.default_rng(42)
    ranks = [_rank_answer(rng, [0, 3], 5), _rank_answer(rng, [1], 5)]       # pairs 2 and 4: the -1 padding of a list call, or a print of a shard not asked
    out = SH.merge_pair_scores(ranks)
    assert out["owner"].tolist() == [0, 1, -1, 0, -1]
    for p in (2, 4):
        assert out["status"][p] == SH.PAIR_NOT_COVERED and np.isneginf(out["score"][p]) and (out["parts"][p].view(np.uint32) == 0).all()
    empty = SH.merge_pair_scores([{"status": np.full(3, SH.PAIR_NOT_COVERED, np.int32), "score": np.full(3, -np.inf, np.float32), "parts": None}])
    assert (empty["status"] == SH.PAIR_NOT_COVERED).all() and empty["owner"].tolist() == [-1, -1, -1] and np.isneginf(empty["score"]).all()


def test_merge_refuses_a_pair_two_ranks_cover():
    rng = np.random.default_rng(43)
    ranks = [_rank_answer(rng, [0, 1], 3), _rank_answer(rng, [1, 2], 3)]
    with pytest.raises(ValueError, match=r"covered by two ranks"):
        SH.merge_pair_scores(ranks)
    with pytest.raises(ValueError):                                         # answers that do not belong together
        SH.merge_pair_scores([_rank_answer(rng, [0], 3), _rank_answer(rng, [1], 4)])


# ---- pair_tables.h ---------------------------------------------------------------------------------------------------------------------------------------
def test_pair_tables_check_runs_clean_under_the_host_sanitizers():
    exe = os.path.join(CSRC, "pair_tables_check")
    src = [os.path.join(CSRC, f) for f in ("pair_tables_check.cpp", "pair_tables.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in src):
        subprocess.run(["make", "-s", "-C", CSRC, "pair_tables_check"], check=True)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("\npair_tables_check:"):]
    assert "-fsanitize=address,undefined" in rule[:rule.index("\n\n")] and "-fno-sanitize-recover=undefined" in rule[:rule.index("\n\n")]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"pair_tables_check: \d+ cases ok", out.stdout), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert int(re.search(r"(\d+) cases ok", out.stdout).group(1)) >= 200
    hdr = open(os.path.join(CSRC, "pair_tables.h")).read()
    assert not re.search(r'#include\s*[<"](hip|afis_)', hdr)                  # device-free: no runtime header, none of the project's device headers
