#!/usr/bin/env python
"""What pair scoring costs (afis_score_pairs) beside the route a caller had before it, on one MI355X with the headline's synthetic gallery and latents (committed as
bench.py commits them): 100 latents x 100 000 templates by default.  One search with scores; then three pair lists:

  hit_lists     the flattened lists of afis_rank_hits(-inf, 100): 100 pairs per latent, every latent other candidates
  verification  one pair per latent: each latent against its best candidate
  one_latent    latent 0 against its 4096 best candidates, on a handle that holds that latent alone (both routes)

and for each, INTERLEAVED repetition by repetition (`--reps` kept after a discarded first; median and spread = max - min):

  pairs   afis_score_pairs with parts: HOST clock (perf_counter around the C call alone, arrays made before it) and option score_pairs_us, the DEVICE clock (HIP events
          around every chunk's launches, summed)
  union   the same library's route through a subset: afis_subset_create over the union of the list's prints + afis_search_subset_resident(k = 0, scores) +
          afis_subset_free — host clock around the three calls; device clock = option subset_gather_us + afis_timing.total_ms of the subset search

Beside them the pairs each route scores, whether the pair call's scores are bit for bit the matrix cells of the full search (and the subset search's), and whether
afis_rank_hits returns after the pair calls what it returned before them.  Recorded, not asserted; no figure here is tuned for.  One JSON document on stdout and in --out."""
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
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--cap", type=int, default=100, help="candidates per latent of the hit lists")
    ap.add_argument("--one", type=int, default=4096, help="candidates of the one-latent list (at most AFIS_HITS_MAX and the gallery)")
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_pairs_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G = a.queries, a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats)
    m = M.Matcher(cbb)
    out = {"queries": Q, "gallery": G, "reps": a.reps, "interleaved": True, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "score_pairs_per_launch": m.get_option("score_pairs_per_launch"),
           "clocks": {"pairs_us": "device: option score_pairs_us, HIP events inside the library", "union_us": "device: option subset_gather_us + afis_timing.total_ms of the subset search",
                      "*_ms": "host: perf_counter around the C calls, which return after their wait", "search_total_ms": "device: afis_timing.total_ms of the full search"}}
    m.gallery_add_packed(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    q1 = m.upload_queries(lats[:1])
    m.search_resident(qh, k=0)                                              # warm-up: first-use allocations
    full = m.search_resident(qh, k=0, want_scores=True)["scores"]
    out["search_total_ms"] = m.timing()["total_ms"]
    ninf = float("-inf")
    cap, one = min(a.cap, G), min(a.one, G, 4096)
    hits = m.rank_hits(ninf, max(cap, one))
    lists = hits["idx"]
    shapes = {
        "hit_lists": (qh, np.repeat(np.arange(Q, dtype=np.int32), cap), np.ascontiguousarray(lists[:, :cap]).reshape(-1), np.arange(Q)),
        "verification": (qh, np.arange(Q, dtype=np.int32), np.ascontiguousarray(lists[:, 0]), np.arange(Q)),
        "one_latent": (q1, np.zeros(one, np.int32), np.ascontiguousarray(lists[0, :one]), np.zeros(1, np.int64)),
    }
    rows = {}
    for name, (handle, query, idx, rows_of) in shapes.items():
        n = len(query)
        union = np.unique(idx)
        status = np.zeros(n, np.int32); score = np.zeros(n, np.float32); parts = np.zeros((n, 4), np.float32)
        pair_ms, pair_us, union_ms, union_us = [], [], [], []
        sub_scores = None
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            m._chk(m.lib.afis_score_pairs(m.ctx, handle[0], n, M._ptr(query, C.c_int32), M._ptr(idx, C.c_int64), M._ptr(status, C.c_int32), M._ptr(score, C.c_float), M._ptr(parts, C.c_float)))
            ms = (time.perf_counter() - t0) * 1e3
            us = m.get_option("score_pairs_us")
            t0 = time.perf_counter()
            sub = m.subset_create(union)
            gather_us = m.get_option("subset_gather_us")
            sub_scores = m.search_subset_resident(sub, handle, k=0, want_scores=True)["scores"]
            search_ms = m.timing()["total_ms"]
            m.subset_free(sub)
            ums = (time.perf_counter() - t0) * 1e3
            if rep:
                pair_ms.append(ms); pair_us.append(us); union_ms.append(ums); union_us.append(gather_us + search_ms * 1e3)
        col = np.searchsorted(union, idx)
        cells = full[rows_of[query], idx]
        rows[name] = {"pairs": n, "pairs_per_latent": n / len(rows_of), "union_prints": int(len(union)), "union_pairs_scored": int(len(union) * handle[1]),
                      "pairs_ms": med(pair_ms), "pairs_us": med(pair_us), "union_ms": med(union_ms), "union_us": med(union_us),
                      "union_over_pairs_device": statistics.median(union_us) / max(statistics.median(pair_us), 1),
                      "union_over_pairs_host": statistics.median(union_ms) / statistics.median(pair_ms),
                      "pairs_over_search": statistics.median(pair_us) / 1e3 / out["search_total_ms"],
                      "all_covered": bool((status == M.PAIR_OK).all()),
                      "equal_to_the_matrix_cells": bool(np.array_equal(score.view(np.uint32), np.ascontiguousarray(cells).view(np.uint32))),
                      "equal_to_the_subset_search": bool(np.array_equal(score.view(np.uint32), np.ascontiguousarray(sub_scores[query, col]).view(np.uint32)))}
    # the subset searches replaced the matrix; after a full search the pair calls leave it as it was
    m.search_resident(qh, k=0)
    before = m.rank_hits(ninf, cap)
    handle, query, idx, _ = shapes["hit_lists"]
    m.score_pairs(handle, query, idx)
    after = m.rank_hits(ninf, cap)
    out["matrix_survived"] = bool(all(before[k].tobytes() == after[k].tobytes() for k in ("n_hits", "idx", "score")))
    out["lists"] = rows
    m.free_queries(qh); m.free_queries(q1); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
