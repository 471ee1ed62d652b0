#!/usr/bin/env python
"""What the pair calls for resident prints cost (afis_score_print_pairs, afis_correspondences_print_pairs) beside the only route there was before them, on one MI355X
with the headline's synthetic gallery (committed as bench.py commits it): 100 000 resident prints by default.  One print search of 100 query prints for the
candidate lists; then three pair lists:

  card        card against card: 10 pairs, print i against its best candidate other than itself
  hit_lists   100 query prints x their 100 best from afis_rank_hits: 10 000 pairs
  one_print   ONE print against its 4096 best

and for each, INTERLEAVED repetition by repetition (`--reps` kept after a discarded first; median and spread = max - min):

  pairs   afis_score_print_pairs with parts, weights (1, 0.3f): HOST clock (perf_counter around the C call alone, arrays made before it) and option print_pairs_us,
          the DEVICE clock (HIP events around the gathers and every chunk's launches, summed)
  union   afis_subset_create over the union of the b's + afis_search_prints of the distinct a's against it + afis_subset_free — host clock around the three calls;
          device clock = option subset_gather_us + afis_timing.total_ms of the print search

and, on hit_lists, afis_correspondences_print_pairs (host and device clock).  The gather's share of a pair call is taken from option print_gather_us of a print
search of the SAME query prints against a one-print subset (the gather launches are the same; the pair call has no option for them alone); the kernels' shares are a
profiler's to give (`rocprofv3 --kernel-trace --stats -- python tools/print_pairs_timing.py --reps 1 --out ''`, a run of its own).  Beside them whether the pair
call's scores are bit for bit the print search's cells (and the subset route's), and whether afis_rank_hits returns after the pair calls what it returned before them.
Recorded, not asserted; no figure here is tuned for.  One JSON document on stdout and in --out."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100, help="query prints of the hit lists")
    ap.add_argument("--cap", type=int, default=100, help="candidates per query print of the hit lists")
    ap.add_argument("--one", type=int, default=4096, help="candidates of the one-print list (at most AFIS_HITS_MAX and the gallery)")
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "print_pairs_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G = a.queries, a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    gal = S.make_packed_gallery(a.seed, G, cb)
    m = M.Matcher(cbb)
    out = {"queries": Q, "gallery": G, "reps": a.reps, "interleaved": True, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "score_pairs_per_launch": m.get_option("score_pairs_per_launch"), "corr_pairs_per_launch": m.get_option("corr_pairs_per_launch"), "weights": [1.0, 0.3],
           "clocks": {"pairs_us / corr_us": "device: option print_pairs_us, HIP events inside the library", "union_us": "device: option subset_gather_us + afis_timing.total_ms of the print search over the subset",
                      "*_ms": "host: perf_counter around the C calls, which return after their wait", "search_total_ms": "device: afis_timing.total_ms of the full print search"}}
    m.gallery_add_packed(gal); m.gallery_commit(0)
    wm, wt = np.float32(1.0), np.float32(0.3)
    rng = np.random.default_rng(a.seed)
    qp = np.sort(rng.choice(G, Q, replace=False)).astype(np.int64)         # the query prints
    m.search_prints(qp[:2], wm, wt, want_scores=False)                      # warm-up: first-use allocations
    full = m.search_prints(qp, wm, wt)["scores"]
    out["search_total_ms"] = m.timing()["total_ms"]
    ninf = float("-inf")
    cap, one = min(a.cap, G), min(a.one, G, 4096)
    lists = m.rank_hits(ninf, max(cap, one, 2))["idx"]
    best_other = np.array([row[0] if row[0] != q else row[1] for q, row in zip(qp, lists)], np.int64)
    shapes = {
        "card": (qp[:10].copy(), best_other[:10].copy()),
        "hit_lists": (np.repeat(qp, cap), np.ascontiguousarray(lists[:, :cap]).reshape(-1)),
        "one_print": (np.full(one, qp[0], np.int64), np.ascontiguousarray(lists[0, :one])),
    }
    row_of = {int(q): i for i, q in enumerate(qp)}
    rows = {}
    for name, (pa, pb) in shapes.items():
        n = len(pa)
        union = np.unique(pb); qa = np.unique(pa)
        w_m = np.full(n, wm, np.float32); w_t = np.full(n, wt, np.float32)
        status = np.zeros(n, np.int32); score = np.zeros(n, np.float32); parts = np.zeros((n, 2), np.float32)
        pair_ms, pair_us, union_ms, union_us = [], [], [], []
        sub_scores = None
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            m._chk(m.lib.afis_score_print_pairs(m.ctx, n, M._ptr(pa, C.c_int64), M._ptr(pb, C.c_int64), M._ptr(w_m, C.c_float), M._ptr(w_t, C.c_float),
                                                M._ptr(status, C.c_int32), M._ptr(score, C.c_float), M._ptr(parts, C.c_float)))
            ms = (time.perf_counter() - t0) * 1e3
            us = m.get_option("print_pairs_us")
            t0 = time.perf_counter()
            sub = m.subset_create(union)
            gather_us = m.get_option("subset_gather_us")
            sub_scores = m.search_prints(qa, wm, wt, subset=sub)["scores"]
            search_ms = m.timing()["total_ms"]
            m.subset_free(sub)
            ums = (time.perf_counter() - t0) * 1e3
            if rep:
                pair_ms.append(ms); pair_us.append(us); union_ms.append(ums); union_us.append(gather_us + search_ms * 1e3)
        # the gather alone: what a print search of the same query prints reports for its gather launches (against one column: the search itself is short)
        m.search_prints(qa, wm, wt, subset=(sub := m.subset_create(union[:1])), want_scores=False)
        gather_alone_us = m.get_option("print_gather_us")
        m.subset_free(sub)
        cells = full[[row_of[int(x)] for x in pa], pb]
        col = np.searchsorted(union, pb); arow = np.searchsorted(qa, pa)
        rows[name] = {"pairs": n, "query_prints": int(len(qa)), "union_prints": int(len(union)), "union_cells_scored": int(len(union) * len(qa)),
                      "pairs_ms": med(pair_ms), "pairs_us": med(pair_us), "union_ms": med(union_ms), "union_us": med(union_us),
                      "union_over_pairs_device": statistics.median(union_us) / max(statistics.median(pair_us), 1),
                      "union_over_pairs_host": statistics.median(union_ms) / statistics.median(pair_ms),
                      "gather_us_of_the_same_prints_in_a_print_search": gather_alone_us,
                      "gather_share_of_the_call": gather_alone_us / max(statistics.median(pair_us), 1),
                      "all_covered": bool((status == M.PAIR_OK).all()),
                      "equal_to_the_print_search_cells": bool(np.array_equal(score.view(np.uint32), np.ascontiguousarray(cells).view(np.uint32))),
                      "equal_to_the_subset_route": bool(np.array_equal(score.view(np.uint32), np.ascontiguousarray(sub_scores[arow, col]).view(np.uint32)))}
    # the correspondence call on the hit lists
    pa, pb = shapes["hit_lists"]
    n = len(pa)
    counts = np.zeros(n, np.int32); xy = np.zeros((n, 120, 4), np.int16); part = np.zeros(n, np.float32)
    c_ms, c_us = [], []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        m._chk(m.lib.afis_correspondences_print_pairs(m.ctx, n, M._ptr(pa, C.c_int64), M._ptr(pb, C.c_int64), M._ptr(counts, C.c_int32), M._ptr(xy, C.c_int16), M._ptr(part, C.c_float)))
        ms = (time.perf_counter() - t0) * 1e3
        if rep:
            c_ms.append(ms); c_us.append(m.get_option("print_pairs_us"))
    rows["hit_lists"]["corr_ms"] = med(c_ms); rows["hit_lists"]["corr_us"] = med(c_us)
    rows["hit_lists"]["corr_pairs_with_survivors"] = int((counts > 0).sum())
    # the subset routes replaced the matrix; after a full print search the pair calls leave it as it was
    m.search_prints(qp, wm, wt, want_scores=False)
    before = m.rank_hits(ninf, cap)
    m.score_print_pairs(pa, pb, wm, wt); m.correspondences_print_pairs(pa, pb)
    after = m.rank_hits(ninf, cap)
    out["matrix_survived"] = bool(all(before[k].tobytes() == after[k].tobytes() for k in ("n_hits", "idx", "score")))
    out["lists"] = rows
    m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
