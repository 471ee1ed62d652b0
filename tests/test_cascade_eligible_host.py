"""Cascade over a part of the shard without a GPU: afis_search_cascade_subset and afis_search_cascade_eligible are declared, exported by both libraries and bound by the
Python host; the mapped kernels are a product object; the header carries the contracts; and the numpy model (tests/cascade_eligible_model.py) is held against hand-made
matrices.  What the device computes is tests/test_gpu_cascade_eligible.py's."""
import importlib
import os
import re

import numpy as np

import cascade_model as CM
import cascade_eligible_model as EM
from test_cascade_host import hand_search

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
F = np.float32
BASE = 1000


def test_both_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    tail = r"int keep,\s*float\*\s*scores\s*,\s*int32_t\*\s*status\s*,\s*int64_t\*\s*n_kept\s*,\s*int64_t\*\s*kept_idx\s*,\s*float\*\s*kept_parts\s*\)\s*;"
    assert re.search(r"\bint\s+afis_search_cascade_subset\s*\(afis_ctx\*\s*ctx,\s*afis_subset\*\s*s,\s*afis_queries\*\s*q,\s*" + tail, code)
    assert re.search(r"\bint\s+afis_search_cascade_eligible\s*\(afis_ctx\*\s*ctx,\s*afis_labels\*\s*labels,\s*const uint64_t\*\s*masks\s*,\s*const afis_template_view\*\s*queries,"
                     r"\s*int n_q,\s*" + tail, code)
    for name, n_args in (("afis_search_cascade_subset", 9), ("afis_search_cascade_eligible", 11)):
        assert name in M.EXPORTS
        for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):     # dlopen only: no device call
            assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args, name
        assert name in hdr[hdr.index("afis_rank_subjects   ranks the score matrix"):hdr.index("n_q must be that")]      # the list of searches that count
    assert hasattr(M.Matcher, "search_cascade_subset") and hasattr(M.Matcher, "search_cascade_eligible")
    assert "afis_debug_kept_cells_mapped" in M.TAP_EXPORTS and hasattr(M.load_library(M.TEST_LIB_PATH), "afis_debug_kept_cells_mapped")
    assert not hasattr(M.load_library(), "afis_debug_kept_cells_mapped")    # a tap: the product library does not export it


def test_the_mapped_kernels_are_a_product_object_and_the_contract_is_in_the_header():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "cascade_mapped.o" in objs and "afis_cascade_eligible.o" in objs
    body = open(os.path.join(CSRC, "cascade_mapped.hip")).read().split("namespace afis {", 1)[1]
    assert body.count("__global__ __launch_bounds__(256)") == 2 == body.count("__global__")
    assert "atomic" not in body and "__shared__" not in body and "__syncthreads" not in body and "asm" not in body
    drv = open(os.path.join(CSRC, "afis_cascade_eligible.cpp")).read()
    for call in ("plan_classes(", "plan_sub_shard(", "build_subset(", "upload_queries(", "latent_cascade(", "add_timing(", "check_query_handle("):
        assert call in drv, call
    assert "launch_expand_rows(" not in drv and "search_shard(ctx, tmp" not in drv       # the kept cells go straight into the combined matrix
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    contract = re.sub(r"\s*\n \*\s+", " ", hdr[hdr.index("Cascade search over a part of the shard"):hdr.index("int afis_search_cascade_subset(")])
    for phrase in ("n_kept[q] = min(keep, n)", "ascending GLOBAL index whatever order the subset's list had", "afis_search_subset_resident writes at (q, column j)",
                   "n_kept[q] = min(keep, |E(q)|)", "afis_rank_hits_filtered(labels, masks, min_score = -INFINITY, cap = keep)", "eligible but dropped, or not eligible",
                   "holds nothing it allocated", "Exclusion lists stay a matter of the ranking call", "eligible_classes", "merge_hits input as they are", "superset"):
        assert phrase in contract, phrase
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "afis_search_cascade_eligible" in text and "afis_search_cascade_subset" in text, doc


# ---- the model against hand-made matrices ---------------------------------------------------------------------------------------------------------------------
def hand():
    """3 latents x 8 prints.  Row 0: columns 1, 3, 4, 6 tie at m = 0, columns 2 and 5 are positive, 0 and 7 are empty prints.  Row 1 is latent-empty.  Row 2 as row 0."""
    parts = np.zeros((3, 8, 4), F)
    for q in (0, 2):
        parts[q, 2] = (3, 0, 1, 50); parts[q, 5] = (9, 0, 0, 0); parts[q, 1, 3] = 70; parts[q, 6, 3] = 90
    return hand_search(parts, [28, 28, 28], [1, 1, 1], empty_cols=(0, 7), empty_rows=(1,))


def test_the_eligible_model_on_ties_across_the_border_an_empty_class_and_a_long_keep():
    scores, parts = hand()
    labels = np.array([1, 2, 1, 1, 2, 2, 1, 2], np.uint64)                  # bit 0: columns 0, 2, 3, 6; bit 1: columns 1, 4, 5, 7 — the tie 1, 3, 4, 6 straddles the border
    masks = np.array([[1, 0, 0], [0, 0, 1], [4, 0, 0]], np.uint64)          # row 0: any_of bit 0; row 1: none_of bit 0 (= bit 1's columns); row 2: a bit no label has
    E = EM.eligible(labels, masks)
    assert E.sum(axis=1).tolist() == [4, 4, 0] and np.flatnonzero(E[0]).tolist() == [0, 2, 3, 6] and np.flatnonzero(E[1]).tolist() == [1, 4, 5, 7]
    for keep, kept0 in ((1, [2]), (2, [2, 3]), (3, [2, 3, 6]), (4, [2, 3, 6, 0]), (9, [2, 3, 6, 0])):
        e = EM.expected_eligible(scores, parts, [28] * 3, [1] * 3, labels, masks, keep, BASE)
        n = min(keep, 4)
        assert e["n_kept"].tolist() == [n, n, 0], keep                      # keep above |E(q)|; a class with no eligible column
        assert e["kept_idx"][0].tolist() == [BASE + t for t in kept0] + [-1] * (keep - n), keep        # the tie among ELIGIBLE columns 3, 6 by index; 1 and 4 never listed
        assert e["kept_idx"][1].tolist() == [BASE + t for t in (1, 4, 5, 7)[:n]] + [-1] * (keep - n)   # latent-empty: the first eligible columns by index, at -1
        assert (e["kept_idx"][2] == -1).all() and (e["matrix"][2] == CM.NO_ENTRY).all() and not e["kept_parts"][2].any()
        mat = e["matrix"]
        assert (mat != CM.NO_ENTRY).sum(axis=1).tolist() == [n, n, 0]
        assert np.array_equal(mat[0, kept0], scores.view(np.uint32)[0, kept0]) and (mat[1, [1, 4, 5, 7][:n]] == CM.MINUS_ONE).all()
        assert (mat[~E] == CM.NO_ENTRY).all()                               # an ineligible cell is never an entry
        assert np.array_equal(e["kept_parts"].view(F)[0, :n], np.where((scores[0, kept0] == -1)[:, None], F(0), parts[0, kept0]))
    # a zero triple is afis_search_cascade's model
    z = EM.expected_eligible(scores, parts, [28] * 3, [1] * 3, labels, np.zeros((3, 3), np.uint64), 5, BASE)
    c = CM.expected(scores, parts, [28] * 3, [1] * 3, 5, BASE)
    for key in ("n_kept", "kept_idx", "matrix", "kept_parts"):
        assert np.array_equal(z[key], c[key]), key
    # the full cascade at keep 3 keeps 5, 2, 1 for row 0: only one of them is eligible — the eligible form keeps three eligible ones
    assert c["kept_idx"][0, :3].tolist() == [BASE + 5, BASE + 2, BASE + 1]


def test_the_subset_model_breaks_ties_by_global_index_not_by_column():
    scores, parts = hand()
    idx = np.array([1006, 1004, 1003, 1002, 1001], np.int64)                # descending: columns 0 .. 4 are prints 6, 4, 3, 2, 1; the keys of 6, 4, 3, 1 tie at 0
    cols = (idx - BASE).astype(int)
    s, p = np.ascontiguousarray(scores[:, cols]), np.ascontiguousarray(parts[:, cols])
    for keep, kept0 in ((1, [1002]), (2, [1002, 1001]), (3, [1002, 1001, 1003]), (5, [1002, 1001, 1003, 1004, 1006]), (7, [1002, 1001, 1003, 1004, 1006])):
        e = EM.expected_subset(s, p, [28] * 3, [1] * 3, idx, keep)
        n = min(keep, 5)
        assert e["n_kept"].tolist() == [n] * 3
        assert e["kept_idx"][0].tolist() == kept0 + [-1] * (keep - n), keep
        assert e["kept_idx"][1].tolist() == sorted(idx.tolist())[:n] + [-1] * (keep - n)                # latent-empty: ascending global index
        col_of = {int(g): j for j, g in enumerate(idx)}
        want_cols = [col_of[g] for g in kept0]
        assert e["kept_pos"][0, :n].tolist() == want_cols
        assert np.array_equal(e["matrix"][0, want_cols], s.view(np.uint32)[0, want_cols]) and (e["matrix"] != CM.NO_ENTRY).sum(axis=1).tolist() == [n] * 3
        assert np.array_equal(e["kept_parts"].view(F)[0, :n], p[0, want_cols])
    # ascending order is cascade_model.expected on the sub-matrix, with the subset's names
    asc = np.sort(idx); cols = (asc - BASE).astype(int)
    s, p = np.ascontiguousarray(scores[:, cols]), np.ascontiguousarray(parts[:, cols])
    e = EM.expected_subset(s, p, [28] * 3, [1] * 3, asc, 3)
    c = CM.expected(s, p, [28] * 3, [1] * 3, 3, 0)
    assert np.array_equal(e["matrix"], c["matrix"]) and np.array_equal(e["kept_parts"], c["kept_parts"])
    assert np.array_equal(e["kept_idx"], np.where(c["kept_pos"] >= 0, asc[np.maximum(c["kept_pos"], 0)], -1))
    # an empty subset
    e0 = EM.expected_subset(np.zeros((3, 0), F), np.zeros((3, 0, 4), F), [28] * 3, [1] * 3, [], 4)
    assert e0["n_kept"].tolist() == [0, 0, 0] and (e0["kept_idx"] == -1).all() and e0["matrix"].shape == (3, 0)
