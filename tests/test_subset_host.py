"""Subset search without a GPU: the four entry points are declared, exported by both libraries and bound by the Python host; the gather kernels are part of the
product objects; the option is documented; the sharding helper splits a global candidate list over a shard plan.  (What a subset search computes is
tests/test_gpu_subset_search.py's.)"""
import importlib
import os
import re

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"afis_subset_create": "int", "afis_subset_free": "void", "afis_search_subset": "int", "afis_search_subset_resident": "int"}


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s+afis_subset\s+afis_subset\s*;", code)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):        # dlopen only: no device call
        for name, ret in NEW.items():
            assert re.search(r"\b%s\s+%s\s*\(afis_ctx\*" % (ret, name), code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert getattr(lib, name).argtypes is not None, name
    for method in ("subset_create", "subset_free", "search_subset", "search_subset_resident"):
        assert hasattr(M.Matcher, method), method
    assert '"subset_device_bytes"' in hdr


def test_gather_kernels_are_product_objects():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "gallery_subset.o" in objs
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "gallery_subset.hip")).read()
    assert "__global__" in src and "launch_gather_ranges" in src


def test_split_candidates_over_a_three_shard_plan():
    """Indices on both sides of every shard boundary, one rank without any, unsorted input: the union of the parts is the input, each part lies inside its shard and
    keeps the caller's order."""
    bounds = [(0, 100), (100, 250), (250, 400)]
    idx = [399, 0, 250, 99, 251, 7, 300, 98]                                # nothing in [100, 250): rank 1 gets an empty list
    parts = SH.split_candidates(idx, bounds)
    assert [p.tolist() for p in parts] == [[0, 99, 7, 98], [], [399, 250, 251, 300]]
    assert all(p.dtype == np.int64 for p in parts)
    assert sorted(np.concatenate(parts).tolist()) == sorted(idx)
    for p, (lo, hi) in zip(parts, bounds):
        assert ((p >= lo) & (p < hi)).all()
    # the boundaries themselves: hi - 1 belongs to the rank, hi to the next one
    parts = SH.split_candidates([100, 99, 249, 250], bounds)
    assert [p.tolist() for p in parts] == [[99], [100, 249], [250]]
    # a plan with an empty rank (shard_bounds may produce one) and the empty list
    assert [p.tolist() for p in SH.split_candidates([5, 1], [(0, 3), (3, 3), (3, 9)])] == [[1], [], [5]]
    assert [p.tolist() for p in SH.split_candidates([], bounds)] == [[], [], []]
    for bad in ([400], [-1], [3, 1 << 40]):
        with pytest.raises(ValueError):
            SH.split_candidates(bad, bounds)


def test_split_parts_merge_like_full_rank_lists():
    """The per-rank rank lists of subset searches carry global indices, so the existing merge takes them unchanged: a host model of three ranks scoring their parts."""
    rng = np.random.default_rng(7)
    G, k = 400, 6
    bounds = SH.shard_bounds(rng.integers(1, 9, G), 3)
    score = np.round(rng.random(G) * 8).astype(np.float32)                  # many equal scores: the tie rule decides
    cand = rng.permutation(G)[:57]
    lists_i = np.full((3, 1, k), -1, np.int64); lists_s = np.full((3, 1, k), -np.inf, np.float32)
    for r, part in enumerate(SH.split_candidates(cand, bounds)):
        order = np.lexsort((part, -score[part].astype(np.float64)))[:k]
        lists_i[r, 0, :len(order)] = part[order]; lists_s[r, 0, :len(order)] = score[part[order]]
    got_i, got_s = SH.merge_topk(lists_i, lists_s, k)
    want = np.lexsort((cand, -score[cand].astype(np.float64)))[:k]
    assert got_i[0].tolist() == cand[want].tolist() and np.array_equal(got_s[0], score[cand[want]])
