#!/usr/bin/env python
"""What a hit list costs (afis_rank_hits / afis_rank_subject_hits), on one MI355X with the headline's synthetic gallery and latents (committed as bench.py commits them):
one search with k = 64, then on the matrix it left on the device the device time of each call's launches (option rank_hits_us: HIP events around them), the median of
`--reps` calls after a discarded first one:

  rank_hits          (-inf, 100)          a candidate list of 100: the radix select cuts inside the positive scores
  rank_hits          (-inf, 4096)         the longest list
  rank_hits          (just above 0, 4096) every positive score, no selection when they fit
  rank_subject_hits  (-inf, 100)          ten templates per subject: k_subject_best, then the same kernel over 10 000 maxima

The yardstick is topk_ms of that search (afis_timing, HIP events too): k_topk's 64 passes over the same rows.  Recorded, not asserted.  Every list is checked against
numpy on the score matrix.  One JSON document on stdout and in --out (default: profiles/r07_rank_hits.json)."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def template_hits(scores, thr, cap):
    n = np.empty(len(scores), np.int64); idx = np.full((len(scores), cap), -1, np.int64)
    for q, row in enumerate(scores):
        at = np.flatnonzero(row >= thr)
        at = at[np.lexsort((at, -row[at].astype(np.float64)))][:cap]
        n[q] = int((row >= thr).sum()); idx[q, :len(at)] = at
    return n, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_rank_hits.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    G, Q = a.gallery, a.queries
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats, G=G)
    out = {"gallery": G, "queries": Q, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "clocks": {"rank_hits_us": "device: HIP events around the call's launches", "topk_ms": "device: HIP events (afis_timing), k_topk at k = 64"}}
    m = M.Matcher(cbb)
    out["device"] = m.device_info(0)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    m.search_resident(qh, k=64)                                             # (the first search of a context allocates)
    r = m.search_resident(qh, k=64, want_scores=True)
    scores = r["scores"]
    out["afis_timing"] = {"topk_ms": round(m.timing()["topk_ms"], 3), "total_ms": round(m.timing()["total_ms"], 2)}
    out["scores"] = {"zero_fraction": round(float((scores == 0).mean()), 4), "positive_per_query_median": int(np.median((scores > 0).sum(axis=1)))}
    hair = float(np.nextafter(np.float32(0), np.float32(1)))
    h = m.subjects_create(np.arange(G, dtype=np.int64) // 10)
    calls = [("rank_hits(-inf, 100)", None, float("-inf"), 100), ("rank_hits(-inf, 4096)", None, float("-inf"), 4096),
             ("rank_hits(>0, 4096)", None, hair, 4096), ("rank_subject_hits(-inf, 100), ten templates per subject", h, float("-inf"), 100)]
    out["calls"] = {}
    for name, handle, thr, cap in calls:
        us, wall = [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            got = m.rank_hits(thr, cap) if handle is None else m.rank_subject_hits(handle, thr, cap)
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                us.append(m.get_option("rank_hits_us")); wall.append(round(ms, 3))
        if handle is None:
            n, idx = template_hits(scores, np.float32(thr), cap)
            same = bool(np.array_equal(n, got["n_hits"]) and np.array_equal(idx, got["idx"]))
        else:
            best = scores.reshape(Q, G // 10, 10).max(axis=2) if G % 10 == 0 else None
            same = None if best is None else bool(np.array_equal(np.ascontiguousarray(np.sort(best, axis=1)[:, ::-1][:, :cap]).view(np.uint32), got["score"].view(np.uint32)))
        out["calls"][name] = {"rank_hits_us": us, "median_rank_hits_us": statistics.median(us), "call_wall_ms": wall, "n_hits_median": int(np.median(got["n_hits"])),
                              "checked_against_numpy": same, "below_topk_ms": bool(statistics.median(us) < out["afis_timing"]["topk_ms"] * 1e3)}
    m.subjects_free(h); m.free_queries(qh); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
