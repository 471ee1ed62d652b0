#!/usr/bin/env python
"""A/B of the pair-list calls and stage 2 of the cascade between this tree's libafis_hip.so and another build's (--parent: the parent commit's), in ONE process on ONE
MI355X with the headline's synthetic gallery and latents (100 latents x 100 000 templates by default), the two libraries ALTERNATING repetition by repetition, `--reps`
kept after a discarded first (median, spread = max - min, every value).  The lists are those of the timing tools of the single calls:

  correspondences   afis_correspondences_pairs on the lists of afis_rank_hits(-inf, 24) and (-inf, 100)  (tools/correspondences_timing.py): option correspondences_us, host clock
  score_pairs       afis_score_pairs with parts on hit_lists / verification / one_latent                 (tools/score_pairs_timing.py):     option score_pairs_us
  print_pairs       afis_score_print_pairs (weights 1, 0.3f) and afis_correspondences_print_pairs of 100 query prints x the 100 columns of those hit lists
                    (tools/print_pairs_timing.py's hit_lists shape, the columns taken from the latent search): option print_pairs_us
  cascade           afis_search_cascade, keep 100 and 1000                                              (tools/cascade_search_timing.py): option cascade_stage2_us

Per figure: both libraries' values, whether this tree's median lies inside the other library's [min, max], and if not how far outside in units of that spread; per call
whether every returned byte equals the other library's.  Recorded, not asserted.  One JSON document on stdout and in --out."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--parent", required=True, help="libafis_hip.so built from the parent commit")
    ap.add_argument("--parent-first", action="store_true", help="create the parent's context first and run it first in every repetition (the order's own effect)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_call_ab.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G = a.queries, a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats)
    libs = {}
    for name, path in (("tree", M.LIB_PATH), ("parent", a.parent))[::-1 if a.parent_first else 1]:
        m = M.Matcher(cbb, lib_path=path)
        m.gallery_add_packed(gal); m.gallery_commit(0)
        qh, q1 = m.upload_queries(lats), m.upload_queries(lats[:1])
        m.search_resident(qh, k=0)                                          # warm-up: first-use allocations
        m.search_resident(qh, k=0)
        libs[name] = (m, qh, q1)
    m0 = libs["tree"][0]
    out = {"queries": Q, "gallery": G, "reps": a.reps, "alternating": True, "order": list(libs), "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m0.device_info(0),
           "clocks": {"*_us": "device: the option named, HIP events inside the library", "host_ms": "host: perf_counter around the C call alone"}}
    ninf = float("-inf")
    one = min(4096, G)
    lists = m0.rank_hits(ninf, one)["idx"]
    qp = np.sort(np.random.default_rng(a.seed).choice(G, Q, replace=False)).astype(np.int64)      # the query prints of the print pairs
    flat = lambda cap: (np.repeat(np.arange(Q, dtype=np.int32), cap), np.ascontiguousarray(lists[:, :cap]).reshape(-1))
    p = lambda arr, t: M._ptr(arr, t)

    def corr(m, qh, q1, cap):
        query, idx = flat(cap)
        n = len(query); cn = np.zeros((n, 3), np.int32); xy = np.zeros((n, 3, 120, 4), np.int16); pt = np.zeros((n, 3), np.float32)
        return lambda: m.lib.afis_correspondences_pairs(m.ctx, qh[0], n, p(query, C.c_int32), p(idx, C.c_int64), p(cn, C.c_int32), p(xy, C.c_int16), p(pt, C.c_float)), (cn, xy, pt), "correspondences_us"

    def score(m, qh, q1, shape):
        handle, (query, idx) = {"hit_lists": (qh, flat(100)), "verification": (qh, flat(1)), "one_latent": (q1, (np.zeros(one, np.int32), np.ascontiguousarray(lists[0, :one])))}[shape]
        n = len(query); st = np.zeros(n, np.int32); sc = np.zeros(n, np.float32); pt = np.zeros((n, 4), np.float32)
        return lambda: m.lib.afis_score_pairs(m.ctx, handle[0], n, p(query, C.c_int32), p(idx, C.c_int64), p(st, C.c_int32), p(sc, C.c_float), p(pt, C.c_float)), (st, sc, pt), "score_pairs_us"

    def print_score(m, qh, q1, _):
        pa, pb = np.repeat(qp, 100), flat(100)[1]
        n = len(pa); wm = np.full(n, 1.0, np.float32); wt = np.full(n, 0.3, np.float32); st = np.zeros(n, np.int32); sc = np.zeros(n, np.float32); pt = np.zeros((n, 2), np.float32)
        return lambda: m.lib.afis_score_print_pairs(m.ctx, n, p(pa, C.c_int64), p(pb, C.c_int64), p(wm, C.c_float), p(wt, C.c_float), p(st, C.c_int32), p(sc, C.c_float), p(pt, C.c_float)), (st, sc, pt), "print_pairs_us"

    def print_corr(m, qh, q1, _):
        pa, pb = np.repeat(qp, 100), flat(100)[1]
        n = len(pa); cn = np.zeros(n, np.int32); xy = np.zeros((n, 120, 4), np.int16); pt = np.zeros(n, np.float32)
        return lambda: m.lib.afis_correspondences_print_pairs(m.ctx, n, p(pa, C.c_int64), p(pb, C.c_int64), p(cn, C.c_int32), p(xy, C.c_int16), p(pt, C.c_float)), (cn, xy, pt), "print_pairs_us"

    def cascade(m, qh, q1, keep):
        sc = np.empty((Q, G), np.float32); st = np.zeros(Q, np.int32); nk = np.zeros(Q, np.int64); ki = np.full((Q, keep), -1, np.int64); kp = np.zeros((Q, keep, 4), np.float32)
        return lambda: m.lib.afis_search_cascade(m.ctx, qh[0], keep, p(sc, C.c_float), p(st, C.c_int32), p(nk, C.c_int64), p(ki, C.c_int64), p(kp, C.c_float)), (sc, st, nk, ki, kp), "cascade_stage2_us"

    rows = {}
    for label, make, arg in (("correspondences_cap24", corr, 24), ("correspondences_cap100", corr, 100), ("score_pairs_hit_lists", score, "hit_lists"),
                             ("score_pairs_verification", score, "verification"), ("score_pairs_one_latent", score, "one_latent"), ("print_pairs_score", print_score, None),
                             ("print_pairs_correspondences", print_corr, None), ("cascade_keep100", cascade, 100), ("cascade_keep1000", cascade, 1000)):
        calls = {name: make(m, qh, q1, arg) for name, (m, qh, q1) in libs.items()}
        us = {name: [] for name in libs}; ms = {name: [] for name in libs}
        for rep in range(a.reps + 1):
            for name, (m, _, _) in libs.items():
                call, _, option = calls[name]
                t0 = time.perf_counter()
                m._chk(call())
                t = (time.perf_counter() - t0) * 1e3
                if rep:
                    us[name].append(m.get_option(option)); ms[name].append(round(t, 3))
        row = {"option": calls["tree"][2], "equal_bytes": bool(all(x.tobytes() == y.tobytes() for x, y in zip(calls["tree"][1], calls["parent"][1])))}
        for key, v in (("us", us), ("host_ms", ms)):
            t, q = v["tree"], v["parent"]
            lo, hi, md = min(q), max(q), statistics.median(t)
            row[key] = {"tree": {"median": md, "spread": max(t) - min(t), "all": t}, "parent": {"median": statistics.median(q), "spread": hi - lo, "all": q},
                        "tree_median_inside_parent_spread": bool(lo <= md <= hi),
                        "outside_by_parent_spreads": 0.0 if lo <= md <= hi else round((md - hi if md > hi else lo - md) / max(hi - lo, 1e-9), 2)}
        rows[label] = row
    out["calls"] = rows
    for m, qh, q1 in libs.values():
        m.free_queries(qh); m.free_queries(q1); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
