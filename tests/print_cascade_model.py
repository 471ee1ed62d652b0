"""The numpy model of afis_search_prints_cascade (include/afis_matcher.h).  Every value of the call is defined by afis_search_prints on the same context, so the model's
inputs are four of its matrices [n_q][G] for the same query prints —
    final   weights (w_minu, w_tex)      the kept cells
    m       weights (w_minu, 0)          the stage-1 value
    v_m     weights (1, 0)               the minutiae part (1 x v_m is exact)
    v_t     weights (0, 1)               the texture part
— the query prints' has-minutiae / has-texture flags and the weights (for the activity rule of kept_parts).  It computes the kept lists, the expected matrix with its
no-entry cells, n_kept and kept_parts.  The selection is cascade_model.rank_rows, the rule of afis_rank_hits.  Everything is compared on uint32 views, exactly.
(tests/test_print_cascade_host.py holds it against hand-made matrices, tests/test_gpu_print_cascade.py the device against it.)"""
import numpy as np

from cascade_model import MINUS_ONE, NO_ENTRY, rank_rows

F = np.float32


def active(has_minu, has_tex, w_minu, w_tex):
    """-> (am [n_q], at [n_q]): a term is active when the query print holds the template and its weight is not zero (-0.0f is a zero)."""
    return (np.asarray(has_minu, bool) & (np.asarray(w_minu, F) != 0)), (np.asarray(has_tex, bool) & (np.asarray(w_tex, F) != 0))


def expected(final, m, v_m, v_t, has_minu, has_tex, w_minu, w_tex, keep, index_base):
    """What afis_search_prints_cascade(keep) returns: "n_kept" [n_q], "kept_idx" [n_q][keep] (global, -1 padded), "kept_pos" (shard-local, -1 padded), "matrix"
    [n_q][G] uint32 (a kept cell: final's word; every other: NO_ENTRY), "kept_parts" [n_q][keep][2] uint32 ((v_m if the minutiae term is active else +0.0f, v_t if the
    texture term is active else +0.0f) of the kept cells in kept_idx order; +0.0f twice where the cell is the -1 and in the padding) and "status" [n_q]."""
    final, m, v_m, v_t = (np.ascontiguousarray(x, F) for x in (final, m, v_m, v_t))
    n_q, G = final.shape
    am, at = active(has_minu, has_tex, w_minu, w_tex)
    n_hits, kept_idx, kept_pos = rank_rows(m, keep, index_base)
    n_kept = np.minimum(n_hits, keep)
    assert (n_kept == min(keep, G)).all()                                    # every column is an entry
    matrix = np.full((n_q, G), NO_ENTRY, np.uint32)
    kept_parts = np.zeros((n_q, keep, 2), np.uint32)
    fw, mw, tw = final.view(np.uint32), v_m.view(np.uint32), v_t.view(np.uint32)
    for q in range(n_q):
        p = kept_pos[q, :n_kept[q]]
        matrix[q, p] = fw[q, p]
        scored = fw[q, p] != MINUS_ONE
        kept_parts[q, :n_kept[q], 0] = np.where(scored & am[q], mw[q, p], np.uint32(0))
        kept_parts[q, :n_kept[q], 1] = np.where(scored & at[q], tw[q, p], np.uint32(0))
    status = np.where(am | at, 0, 1).astype(np.int32)
    return {"n_kept": n_kept, "kept_idx": kept_idx, "kept_pos": kept_pos, "matrix": matrix, "kept_parts": kept_parts, "status": status}


def fold(v_m, v_t, w_minu, w_tex, am, at, empty_cols):
    """afis_search_prints' cell for hand-made parts [n_q][G]: -1 for an empty column or a row with nothing active, else (float) of the fp64 sum, minutiae before
    texture, over the active terms (what the hand-made tests build their four matrices with)."""
    v_m = np.asarray(v_m, F); v_t = np.asarray(v_t, F)
    n_q, G = v_m.shape
    out = np.full((n_q, G), -1.0, F)
    for q in range(n_q):
        if not (am[q] or at[q]):
            continue
        acc = np.zeros(G, np.float64)
        if am[q]:
            acc = acc + np.float64(F(w_minu[q])) * v_m[q].astype(np.float64)
        if at[q]:
            acc = acc + np.float64(F(w_tex[q])) * v_t[q].astype(np.float64)
        out[q] = acc.astype(F)
    out[:, list(empty_cols)] = -1.0
    return out


def four_matrices(v_m, v_t, has_minu, has_tex, w_minu, w_tex, empty_cols=()):
    """(final, m, v_m, v_t) as afis_search_prints would give them for the weights (w_minu, w_tex), (w_minu, 0), (1, 0) and (0, 1)."""
    n_q = len(has_minu)
    one, zero = np.ones(n_q, F), np.zeros(n_q, F)
    out = []
    for wm, wt in ((w_minu, w_tex), (w_minu, zero), (one, zero), (zero, one)):
        am, at = active(has_minu, has_tex, wm, wt)
        out.append(fold(v_m, v_t, wm, wt, am, at, empty_cols))
    return tuple(out)
