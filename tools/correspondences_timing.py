#!/usr/bin/env python
"""What the correspondence export of a whole candidate list costs (afis_correspondences_pairs), on one MI355X with the headline's synthetic gallery and latents
(committed as bench.py commits them): 100 latents x 100 000 templates by default.  One search; then, for the lists of afis_rank_hits(-inf, 24) and (-inf, 100):

  pairs         afis_correspondences_pairs with the flattened lists on the handle the search ran on: HOST clock (perf_counter around the C call alone, arrays made
                before it), `--reps` kept repetitions after a discarded first, median and spread (max - min); and option correspondences_us, the DEVICE clock (HIP
                events around every chunk's launches, summed)
  one_latent    this tree's afis_correspondences, one call per latent with that latent's list (the wrapper around the same driver), host clock, the same repetitions
  parent        with --parent <libafis_hip.so of the parent commit>, loaded beside this tree's as tools/lib_ab.py loads it: the same one call per latent against the
                parent's library — its per-template loop — host clock, the same repetitions; its counts, and the coordinates below them, are compared with the pair call's

Beside them the search step of the same run (afis_timing.total_ms: the yardstick), and whether afis_rank_hits after the pair calls returns the lists it returned before
them (the matrix survived).  Recorded, not asserted; no figure here is tuned for.  One JSON document on stdout and in --out."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def one_latent_route(m, views, lists, counts, xy):
    """One afis_correspondences call per latent; -> host milliseconds of the C calls."""
    cap = lists.shape[1]
    t0 = time.perf_counter()
    for q, v in enumerate(views):
        n = int((lists[q] >= 0).sum())
        m._chk(m.lib.afis_correspondences(m.ctx, v.arr, M._ptr(lists[q], C.c_int64), n, M._ptr(counts[q * cap:], C.c_int32), M._ptr(xy[q * cap:], C.c_int16)))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--caps", default="24,100")
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--parent", default="", help="libafis_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correspondences_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G = a.queries, a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats)
    m = M.Matcher(cbb)
    out = {"queries": Q, "gallery": G, "reps": a.reps, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "corr_pairs_per_launch": m.get_option("corr_pairs_per_launch"),
           "clocks": {"correspondences_us": "device: HIP events inside the library", "*_ms": "host: perf_counter around the C calls, which return after their wait",
                      "search_total_ms": "device: afis_timing.total_ms of the search whose lists are exported"}}
    m.gallery_add_packed(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    m.search_resident(qh, k=0)                                              # warm-up: first-use allocations
    m.search_resident(qh, k=0)
    out["search_total_ms"] = m.timing()["total_ms"]
    mp = None
    if a.parent:
        mp = M.Matcher(cbb, lib_path=a.parent)
        mp.gallery_add_packed(gal); mp.gallery_commit(0)
        out["parent_has_the_pair_call"] = hasattr(mp.lib, "afis_correspondences_pairs")
    views = [M._Views([L]) for L in lats]
    ninf = float("-inf")
    rows = {}
    for cap in [int(c) for c in a.caps.split(",")]:
        before = m.rank_hits(ninf, cap)
        lists = np.ascontiguousarray(before["idx"])
        n = Q * cap
        query = np.repeat(np.arange(Q, dtype=np.int32), cap); idx = lists.reshape(-1)
        counts = np.zeros((n, 3), np.int32); xy = np.zeros((n, 3, 120, 4), np.int16); part = np.zeros((n, 3), np.float32)
        c1 = np.zeros_like(counts); x1 = np.zeros_like(xy); cp = np.zeros_like(counts); xp = np.zeros_like(xy)
        pair_ms, pair_us, one_ms, parent_ms = [], [], [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            m._chk(m.lib.afis_correspondences_pairs(m.ctx, qh[0], n, M._ptr(query, C.c_int32), M._ptr(idx, C.c_int64), M._ptr(counts, C.c_int32), M._ptr(xy, C.c_int16), M._ptr(part, C.c_float)))
            ms = (time.perf_counter() - t0) * 1e3
            us = m.get_option("correspondences_us")
            if rep:
                pair_ms.append(ms); pair_us.append(us)
        after = m.rank_hits(ninf, cap)
        survived = all(before[k].tobytes() == after[k].tobytes() for k in ("n_hits", "idx", "score"))
        for rep in range(a.reps + 1):
            ms = one_latent_route(m, views, lists, c1, x1)
            if rep:
                one_ms.append(ms)
        m.search_resident(qh, k=0)                                          # (the one-latent call invalidated the matrix: the next cap ranks a fresh one)
        if mp is not None:
            for rep in range(a.reps + 1):
                ms = one_latent_route(mp, views, lists, cp, xp)
                if rep:
                    parent_ms.append(ms)
        row = {"pairs": n, "lists_with_survivors": int((counts > 0).sum()), "not_run": int((counts == -1).sum()), "not_covered": int((counts == -2).sum()),
               "pairs_ms": med(pair_ms), "correspondences_us": med(pair_us), "one_latent_ms": med(one_ms),
               "pairs_over_search": statistics.median(pair_ms) / out["search_total_ms"],
               "matrix_survived": bool(survived), "one_latent_equal_to_pairs": bool(np.array_equal(counts, c1) and np.array_equal(xy, x1))}
        if parent_ms:
            row["parent_ms"] = med(parent_ms)
            live = np.arange(120)[None, None, :] < np.maximum(cp, 0)[:, :, None]           # the rows below counts: what the parent's call defines (it copies its
            row["parent_equal_to_pairs"] = bool(np.array_equal(counts, cp) and np.array_equal(xy[live], xp[live]))   # whole device buffer back, rows beyond counts as they lay)
            row["parent_rows_beyond_counts_zero"] = bool(not xp[~live].any())
            row["parent_over_pairs"] = statistics.median(parent_ms) / statistics.median(pair_ms)
        rows["cap %d" % cap] = row
    out["lists"] = rows
    m.free_queries(qh); m.close()
    if mp is not None:
        mp.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
