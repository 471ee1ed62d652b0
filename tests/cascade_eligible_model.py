"""The numpy model of afis_search_cascade_eligible and afis_search_cascade_subset (include/afis_matcher.h), built on tests/cascade_model.py: from a reference search's
scores and parts it computes what either call must return — the matrix with its no-entry cells, kept_idx, kept_parts and n_kept.  Everything is compared on uint32
views, exactly.  (tests/test_cascade_eligible_host.py holds it against hand-made matrices, tests/test_gpu_cascade_eligible.py the device against it.)"""
import numpy as np

import cascade_model as CM


def eligible(labels, masks):
    """E [n_q][G] bool: the label test of the filtered hit lists (csrc/hit_filter.hip) — masks [n_q][3] = (any_of, all_of, none_of)."""
    L = np.asarray(labels, np.uint64)[None, :]
    mk = np.asarray(masks, np.uint64).reshape(-1, 3)
    any_of, all_of, none_of = mk[:, 0:1], mk[:, 1:2], mk[:, 2:3]
    return ((any_of == 0) | ((L & any_of) != 0)) & ((L & all_of) == all_of) & ((L & none_of) == 0)


def _kept(scores, parts, m, keep, names):
    """The kept lists of a stage-1 matrix m whose no-entry cells are no entries, and what is returned for them: names [G] the global index of column t."""
    n_q, G = scores.shape
    n_hits, _, kept_pos = CM.rank_rows(m, keep, 0)
    n_kept = np.minimum(n_hits, keep)
    kept_idx = np.full((n_q, keep), -1, np.int64)
    matrix = np.full((n_q, G), CM.NO_ENTRY, np.uint32)
    kept_parts = np.zeros((n_q, keep, 4), np.uint32)
    sw = scores.view(np.uint32); pw = parts.view(np.uint32)
    for q in range(n_q):
        p = kept_pos[q, :n_kept[q]]
        kept_idx[q, :n_kept[q]] = names[p]
        matrix[q, p] = sw[q, p]
        kept_parts[q, :n_kept[q]] = np.where((sw[q, p] == CM.MINUS_ONE)[:, None], np.uint32(0), pw[q, p])
    return {"m": m, "n_kept": n_kept, "kept_idx": kept_idx, "kept_pos": kept_pos, "matrix": matrix, "kept_parts": kept_parts}


def expected_eligible(scores, parts, n_minu, n_tex, labels, masks, keep, index_base):
    """afis_search_cascade_eligible(keep) after the FULL search that gave scores [n_q][G] / parts [n_q][G][4]: stage 1's m with the ineligible cells set to the no-entry
    word, its rank lists, the kept cells.  "E" is the eligibility matrix; the other keys are cascade_model.expected's."""
    scores = np.ascontiguousarray(scores, np.float32); parts = np.ascontiguousarray(parts, np.float32)
    E = eligible(labels, masks)
    m = CM.stage1(scores, parts, n_minu, n_tex).view(np.uint32).copy()
    m[~E] = CM.NO_ENTRY
    out = _kept(scores, parts, m.view(np.float32), keep, np.arange(scores.shape[1], dtype=np.int64) + index_base)
    assert np.array_equal(out["n_kept"], np.minimum(keep, E.sum(axis=1)))   # every eligible column is an entry
    out["E"] = E
    return out


def expected_subset(scores, parts, n_minu, n_tex, idx, keep):
    """afis_search_cascade_subset(keep) after the subset search that gave scores [n_q][n] / parts [n_q][n][4] in the CALLER'S column order, idx [n] the subset's global
    indices in that order.  Equal keys go by ascending global index, not by column: the columns are ranked in ascending index order and mapped back.  "matrix" and
    "kept_pos" are in the caller's column order."""
    scores = np.ascontiguousarray(scores, np.float32); parts = np.ascontiguousarray(parts, np.float32)
    idx = np.asarray(idx, np.int64).reshape(-1)
    order = np.argsort(idx, kind="stable")                                  # ascending position t -> the caller's column
    s2 = np.ascontiguousarray(scores[:, order]); p2 = np.ascontiguousarray(parts[:, order])
    out = _kept(s2, p2, CM.stage1(s2, p2, n_minu, n_tex), keep, idx[order])
    assert (out["n_kept"] == min(keep, len(idx))).all()
    matrix = np.full(scores.shape, CM.NO_ENTRY, np.uint32)
    matrix[:, order] = out["matrix"]
    out["matrix"] = matrix
    out["kept_pos"] = np.where(out["kept_pos"] >= 0, order[np.maximum(out["kept_pos"], 0)] if len(order) else -1, -1)
    return out
