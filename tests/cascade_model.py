"""The numpy model of afis_search_cascade (include/afis_matcher.h): from a full search's scores [n_q][G] and parts [n_q][G][4], the latents' template counts and
index_base it computes the stage-1 matrix m, the kept lists and what the call must return — the matrix with its no-entry cells, kept_idx, kept_parts and n_kept.
Everything is compared on uint32 views, exactly.  (tests/test_cascade_host.py holds it against hand-made matrices, tests/test_gpu_cascade_search.py the device against it.)"""
import numpy as np

NO_ENTRY = np.uint32(0xFFFFFFFF)           # csrc/score_order.h: kNoEntryWord
MINUS_ONE = np.uint32(0xBF800000)          # -1.0f: an empty or removed print, a latent-empty query


def ordered_word(bits):
    """csrc/score_order.h: the bijection of a score word whose unsigned order is the total order of the floats' bits."""
    b = np.asarray(bits, np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def rank_key(s):
    """The key of every template rank list: the ordered word of s + 0.0f (the two zeros are one value)."""
    with np.errstate(invalid="ignore"):
        return ordered_word((np.asarray(s, np.float32) + np.float32(0.0)).view(np.uint32))


def tex_slots(n_minu, n_tex):
    """Where the texture score sits in the reference's score vector: the number of latent minutiae templates, -1 without a texture template."""
    n_minu = np.asarray(n_minu, np.int64); n_tex = np.asarray(n_tex, np.int64)
    return np.where(n_tex > 0, n_minu, -1)


def stage1(scores, parts, n_minu, n_tex):
    """m(q, t): fuse_cell's expression with the texture score taken as +0.0f — -1 where the search's cell is the -1, else (a0 + a1) + a2 in fp32 with a_s = +0.0f where
    the texture's slot is s (the double-precision tail adds slot 28's +0.0 x 0.3)."""
    scores = np.asarray(scores, np.float32); parts = np.asarray(parts, np.float32)
    slot = tex_slots(n_minu, n_tex)
    a = [np.where((slot == s)[:, None], np.float32(0.0), parts[:, :, s]).astype(np.float32) for s in range(3)]
    f = ((a[0] + a[1]).astype(np.float32) + a[2]).astype(np.float32)
    m = (f.astype(np.float64) + 0.0 * 0.3).astype(np.float32)
    return np.where(scores.view(np.uint32) == MINUS_ONE, np.float32(-1.0), m).astype(np.float32)


def rank_rows(matrix, cap, index_base):
    """afis_rank_hits(min_score = -inf, cap) on a matrix [n_q][G]: per row the entries — the cells whose key reaches -inf's; the no-entry word's does not — by rank_key
    descending, equal keys by ascending index.  -> n_hits [n_q], idx [n_q][cap] global indices padded with -1, positions [n_q][cap] (-1 padded)."""
    matrix = np.asarray(matrix, np.float32)
    n_q, G = matrix.shape
    n_hits = np.zeros(n_q, np.int64); idx = np.full((n_q, cap), -1, np.int64); pos = np.full((n_q, cap), -1, np.int64)
    floor = rank_key(np.float32(-np.inf))
    for q in range(n_q):
        key = rank_key(matrix[q])
        entries = np.flatnonzero(key >= floor)
        order = entries[np.lexsort((entries, -key[entries].astype(np.int64)))]
        n_hits[q] = len(order)
        n = min(cap, len(order))
        pos[q, :n] = order[:n]; idx[q, :n] = order[:n] + index_base
    return n_hits, idx, pos


def expected(scores, parts, n_minu, n_tex, keep, index_base):
    """What afis_search_cascade(keep) returns after the search that gave scores / parts: "m", "n_kept" [n_q], "kept_idx" [n_q][keep], "kept_pos" (shard-local, -1
    padded), "matrix" [n_q][G] uint32 (a kept cell: the search's word; every other: NO_ENTRY) and "kept_parts" [n_q][keep][4] uint32 (the search's parts of the kept
    cells in kept_idx order, +0.0f four times where the score is the -1 and in the padding)."""
    scores = np.asarray(scores, np.float32); parts = np.asarray(parts, np.float32)
    n_q, G = scores.shape
    m = stage1(scores, parts, n_minu, n_tex)
    n_hits, kept_idx, kept_pos = rank_rows(m, keep, index_base)
    n_kept = np.minimum(n_hits, keep)
    assert (n_kept == min(keep, G)).all()                                    # every column is an entry
    matrix = np.full((n_q, G), NO_ENTRY, np.uint32)
    kept_parts = np.zeros((n_q, keep, 4), np.uint32)
    sw = scores.view(np.uint32); pw = parts.view(np.uint32)
    for q in range(n_q):
        p = kept_pos[q, :n_kept[q]]
        matrix[q, p] = sw[q, p]
        kept_parts[q, :n_kept[q]] = np.where((sw[q, p] == MINUS_ONE)[:, None], np.uint32(0), pw[q, p])
    return {"m": m, "n_kept": n_kept, "kept_idx": kept_idx, "kept_pos": kept_pos, "matrix": matrix, "kept_parts": kept_parts}
