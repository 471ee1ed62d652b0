"""Numpy model of the plan of afis_score_print_pairs / afis_correspondences_print_pairs (csrc/print_pairs_plan.h), shared by tests/test_print_pairs_host.py and
tests/test_gpu_print_pairs.py: which pairs are covered, which of them need the device (planned), the distinct query prints in order of first appearance with what of
each is gathered, the batches, and every planned pair's batch and position in its batch's handle."""
import numpy as np

POINT_BYTES, TILE_BYTES = 392, 6 * 64 * 16                                  # a minutia or texture point of a view; a fragment tile of 16 descriptors


def view_bytes(nm, nt):
    return (nm + nt) * POINT_BYTES + (nm + 15) // 16 * TILE_BYTES


def covered(a_idx, b_idx, base, G):
    a = np.asarray(a_idx, np.int64); b = np.asarray(b_idx, np.int64)
    return (a >= base) & (a < base + G) & (b >= base) & (b < base + G)


def plan(a_idx, b_idx, base, counts, want_minu, want_tex, cap=0, budget=1 << 62):
    """counts [G] of (minutiae, texture points) as resident; want_minu / want_tex [n] bool (a scalar is every pair's).
    -> {"prints": [(shard-local print, gathers minutiae, gathers texture)], "batches": [[positions of `prints`]], "pairs": [[(pair number, position in the batch's
    handle)] per batch, in the caller's order], "planned": [pair numbers]}"""
    a = np.asarray(a_idx, np.int64).reshape(-1); n = len(a)
    G = len(counts)
    cov = covered(a, b_idx, base, G)
    wm = np.broadcast_to(np.asarray(want_minu, bool), (n,)); wt = np.broadcast_to(np.asarray(want_tex, bool), (n,))
    slot, prints, planned = {}, [], []
    for i in range(n):
        if not cov[i]:
            continue
        t = int(a[i] - base)
        m, x = bool(wm[i]) and counts[t][0] > 0, bool(wt[i]) and counts[t][1] > 0
        if not (m or x):
            continue
        if t not in slot:
            slot[t] = len(prints); prints.append([t, False, False])
        prints[slot[t]][1] |= m; prints[slot[t]][2] |= x
        planned.append(i)
    batches, held = [], 0
    for k, (t, m, x) in enumerate(prints):
        nbytes = view_bytes(counts[t][0] if m else 0, counts[t][1] if x else 0)
        if not batches or (len(batches[-1]) >= cap if cap > 0 else held + nbytes > budget):
            batches.append([]); held = 0
        batches[-1].append(k); held += nbytes
    batch_of = {k: (bi, pos) for bi, b in enumerate(batches) for pos, k in enumerate(b)}
    pairs = [[] for _ in batches]
    for i in planned:
        bi, pos = batch_of[slot[int(a[i] - base)]]
        pairs[bi].append((i, pos))
    return {"prints": [tuple(p) for p in prints], "batches": batches, "pairs": pairs, "planned": planned}
