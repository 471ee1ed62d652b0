"""Correspondence export for a pair list without a GPU: afis_correspondences_pairs and the two AFIS_CORR_* values are declared, the entry point is exported by both
libraries and bound by the Python host; its host unit and the pair form's translation unit are product objects; the options are documented;
host/sharding.py::merge_correspondences on hand-made per-rank arrays.  (The -1 / -2 rule is applied inside the entry point from the context's tables, behind a
committed gallery: it is not reachable without a device — tests/test_gpu_correspondence_pairs.py holds it, and what the device answers, against the oracle.)"""
import importlib
import os
import re

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NAME = "afis_correspondences_pairs"
VALUES = {"AFIS_CORR_NOT_RUN": -1, "AFIS_CORR_NOT_COVERED": -2}


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, value in VALUES.items():
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), code, flags=re.M), name
    assert (M.CORR_NOT_RUN, M.CORR_NOT_COVERED) == (-1, -2) == (SH.CORR_NOT_RUN, SH.CORR_NOT_COVERED)
    assert re.search(r"\bint\s+%s\s*\(afis_ctx\*\s*ctx,\s*afis_queries\*\s*q,\s*int64_t\s+n_pairs," % NAME, code)
    default = int(re.search(r"^#define\s+AFIS_CORR_PAIRS_PER_LAUNCH\s+(\d+)\s*$", code, flags=re.M).group(1))
    assert 1 <= default <= 1 << 20                                          # the builder's choice, written into the header
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        assert NAME in M.EXPORTS and hasattr(lib, NAME) and hasattr(lib, "afis_correspondences")
        assert len(getattr(lib, NAME).argtypes) == 8
    assert hasattr(M.Matcher, "correspondences_pairs") and hasattr(SH, "merge_correspondences")
    assert M.NOT_COVERED is not None and not M.NOT_COVERED and repr(M.NOT_COVERED) == "NOT_COVERED"   # a marker of its own: not the None of "no file"
    assert hdr.index("int afis_correspondences(") < hdr.index("int %s(" % NAME)


def test_the_host_unit_and_the_pair_kernels_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "afis_corr.o" in objs and "graph_pairs.o" in objs
    assert re.search(r"^graph_pairs\.o:.*\n\t.*-fno-slp-vectorize", mk, flags=re.M)              # graph.hip's own flags


def test_the_options_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    block = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    assert '"corr_pairs_per_launch"' in block and re.search(r'"correspondences_us" \(read-only\)', block)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`corr_pairs_per_launch`" in doc and "`correspondences_us`" in doc and "`%s`" % NAME in doc


# ---- merge_correspondences ----------------------------------------------------------------------------------------------------------------------------
def _rank_arrays(rng, covered, n_pairs):
    """One rank's answer: the pairs of `covered` with made-up survivors, every other pair AFIS_CORR_NOT_COVERED and zeros."""
    cn = np.full((n_pairs, 3), SH.CORR_NOT_COVERED, np.int32); xy = np.zeros((n_pairs, 3, 120, 4), np.int16); pt = np.zeros((n_pairs, 3), np.float32)
    for p in covered:
        for s in range(3):
            n = int(rng.integers(-1, 6))                                    # -1: the reference runs no scorer
            cn[p, s] = n
            if n > 0:
                xy[p, s, :n] = rng.integers(-300, 3000, (n, 4)); pt[p, s] = rng.random()
    return cn, xy, pt


def test_merge_takes_every_pair_from_the_rank_that_covers_it():
    rng = np.random.default_rng(31)
    P = 9
    owners = [0, 2, 1, 1, 0, 2, 2, 0, 1]                                    # disjoint: every pair covered by exactly one of three ranks
    ranks = [_rank_arrays(rng, [p for p in range(P) if owners[p] == r], P) for r in range(3)]
    cn, xy, pt, owner = SH.merge_correspondences([a[0] for a in ranks], [a[1] for a in ranks], [a[2] for a in ranks])
    assert owner.tolist() == owners
    for p in range(P):
        src = ranks[owners[p]]
        assert cn[p].tobytes() == src[0][p].tobytes() and xy[p].tobytes() == src[1][p].tobytes() and pt[p].tobytes() == src[2][p].tobytes()
    out = SH.merge_correspondences([a[0] for a in ranks], [a[1] for a in ranks])      # without parts: three results
    assert len(out) == 3 and out[0].tobytes() == cn.tobytes() and out[1].tobytes() == xy.tobytes() and out[2].tolist() == owners
    # a pair whose scorers the reference does not run at all (-1 three times) is still covered by its rank
    ranks[1][0][2] = SH.CORR_NOT_RUN; ranks[1][1][2] = 0
    assert SH.merge_correspondences([a[0] for a in ranks], [a[1] for a in ranks])[2][2] == 1


def test_merge_marks_a_pair_no_rank_covers():
    rng = np.random.default_rng(32)
    ranks = [_rank_arrays(rng, [0, 3], 5), _rank_arrays(rng, [1], 5)]       # pairs 2 and 4: the -1 padding of a list call, or a print of a shard not asked
    cn, xy, pt, owner = SH.merge_correspondences([a[0] for a in ranks], [a[1] for a in ranks], [a[2] for a in ranks])
    assert owner.tolist() == [0, 1, -1, 0, -1]
    for p in (2, 4):
        assert (cn[p] == SH.CORR_NOT_COVERED).all() and not xy[p].any() and (pt[p].view(np.uint32) == 0).all()
    empty = SH.merge_correspondences(np.zeros((0, 3, 3), np.int32), np.zeros((0, 3, 3, 120, 4), np.int16))      # no rank at all
    assert (empty[0] == SH.CORR_NOT_COVERED).all() and empty[2].tolist() == [-1, -1, -1]


def test_merge_refuses_a_pair_two_ranks_cover():
    rng = np.random.default_rng(33)
    ranks = [_rank_arrays(rng, [0, 1], 3), _rank_arrays(rng, [1, 2], 3)]
    with pytest.raises(ValueError, match=r"covered by two ranks"):
        SH.merge_correspondences([a[0] for a in ranks], [a[1] for a in ranks])
    with pytest.raises(ValueError):                                         # shapes that do not belong together
        SH.merge_correspondences(ranks[0][0][None], ranks[0][1][None, :2])
