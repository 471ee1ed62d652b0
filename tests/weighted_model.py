"""Numpy models of the weighted search (afis_search_weighted), shared by tests/test_weighted_host.py and tests/test_gpu_weighted_search.py: the plan (active
templates, packing into pseudo-queries, weight tables aligned to the part slots, batches) and the fold (fp64 sum in the stated order, one conversion)."""
import numpy as np

LATENT_EMPTY = 1                                                            # AFIS_QUERY_LATENT_EMPTY


def active(n, w_row):
    """Template i is active when i < n, i < len(w_row) and the weight is not a zero of either sign."""
    k = max(0, min(int(n), len(w_row)))
    return np.flatnonzero(np.asarray(w_row[:k], np.float32) != 0).astype(np.int32)


def plan(counts, w_minu, w_tex):
    """counts [n_q] of (n_minu, n_tex); w_minu / w_tex [n_q][n_w].  -> (qd [n_q][4] int32 = (first pseudo-query, n_pq, n_at, status), spec [P][4] int32 — the
    templates in the three minutiae slots and the texture slot, -1 = none —, wtab [P][4] float32 aligned to spec, 0 where unused)"""
    qd, spec, wtab = [], [], []
    for q, (n_minu, n_tex) in enumerate(counts):
        am, at = active(n_minu, w_minu[q]), active(n_tex, w_tex[q])
        n_pq = max((len(am) + 2) // 3, len(at))
        qd.append((len(spec), n_pq, len(at), 0 if n_pq else LATENT_EMPTY))
        for j in range(n_pq):
            m3 = am[3 * j:3 * j + 3]
            spec.append([int(x) for x in m3] + [-1] * (3 - len(m3)) + [int(at[j]) if j < len(at) else -1])
            wtab.append([float(w_minu[q][x]) for x in m3] + [0.0] * (3 - len(m3)) + [float(w_tex[q][at[j]]) if j < len(at) else 0.0])
    return np.array(qd, np.int32).reshape(-1, 4), np.array(spec, np.int32).reshape(-1, 4), np.array(wtab, np.float32).reshape(-1, 4)


def batches(qd, cap):
    """Batches of at most cap pseudo-queries cut at query boundaries; a query with more is a batch of its own, one with none joins the open batch.  -> [(q0, q1)]"""
    out, cur = [], 0
    for q, d in enumerate(qd):
        if not out or (cur > 0 and cur + int(d[1]) > cap):
            out.append([q, q]); cur = 0
        out[-1][1] = q + 1; cur += int(d[1])
    return [tuple(b) for b in out]


def fold(parts, qd, wtab, empty):
    """parts [P][G][4] float32 -> out [n_q][G] float32: the fold as k_fold_templates states it, vectorised over the columns.  fp64 multiply and add are two
    operations here; the product of two fp32 values is exact in fp64, so that is the fused result too."""
    parts = np.asarray(parts, np.float32); G = parts.shape[1] if parts.ndim == 3 else len(empty)
    out = np.full((len(qd), G), -1.0, np.float32)
    live = np.asarray(empty, np.uint8) == 0
    for q, (first, n_pq, n_at, status) in enumerate(np.asarray(qd, np.int64)):
        if status:
            continue
        acc = np.zeros(G, np.float64)
        with np.errstate(all="ignore"):                                     # (an empty column may hold anything: its sum is not used)
            for j in range(n_pq):
                for s in range(3):
                    w = np.float32(wtab[first + j][s])
                    if w != 0:
                        acc = acc + np.float64(w) * parts[first + j, :, s].astype(np.float64)
            for j in range(n_at):
                w = np.float32(wtab[first + j][3])
                if w != 0:
                    acc = acc + np.float64(w) * parts[first + j, :, 3].astype(np.float64)
            out[q, live] = acc.astype(np.float32)[live]
    return out


def fold_vectors(vec, n_minu, w_minu_row, w_tex_row, empty):
    """One query from its all-templates vectors vec [G][n_minu + n_tex] (what afis_match_all_templates / the oracle give): the definition of
    include/afis_matcher.h, without any packing.  -> (row [G] float32, status)"""
    vec = np.asarray(vec, np.float32); G = len(empty)
    n_tex = vec.shape[1] - n_minu
    am, at = active(n_minu, w_minu_row), active(n_tex, w_tex_row)
    if len(am) + len(at) == 0:
        return np.full(G, -1.0, np.float32), LATENT_EMPTY
    acc = np.zeros(G, np.float64)
    for i in am:
        acc = acc + np.float64(np.float32(w_minu_row[i])) * vec[:, i].astype(np.float64)
    for t in at:
        acc = acc + np.float64(np.float32(w_tex_row[t])) * vec[:, n_minu + t].astype(np.float64)
    with np.errstate(over="ignore"):
        row = acc.astype(np.float32)
    row[np.asarray(empty, np.uint8) != 0] = -1.0
    return row, 0
