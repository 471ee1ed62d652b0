#!/usr/bin/env python
"""What it costs to ask where named templates stand (afis_rank_positions), on one MI355X with the headline's synthetic gallery and latents (committed as bench.py
commits them): 100 latents x 100 000 templates by default.  One search; then, on the matrix it left on the device, every call below is made `--reps` + 1 times, the
first discarded; medians with the spread (max - min) beside them:

  (a) one target per latent      the planted full mate of every latent: the CMC case
  (b) ten per latent             its four planted mates and six templates drawn at random
  (c) 1 000 targets, one latent  a suspect list against latent 0
  (d) (a) under filters          per query a finger / sex mask (one none_of over cards of ten one-hot fingers) and `--excluded` elimination prints:
                                 tools/filtered_hits_timing.py's masks + exclusions

Beside each case, in the same run on the same matrix: rank_hits_us of afis_rank_hits(-inf, cap) — the list the positions refer to, which reaches no further than 4096
entries — for (d) rank_filtered_us of afis_rank_hits_filtered with the same filters, and the HOST route: the [n_q][G] matrix copied out by a search that asks for
`scores` (the wall-clock difference to the same search without them, medians), then numpy — per row that has targets one lexsort on (key, index) and its inverse
(perf_counter).  Clocks otherwise: DEVICE only (HIP events inside the library): option rank_positions_us around the call's launches.  The counting pass is also
given as bytes per second over what it must read, rows with targets x G x 4.  Every answer is checked against the numpy route.  Recorded, not asserted.  One JSON
document on stdout and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
U64 = np.uint64
FLOOR = 0x007fffff                                                          # the ordered word of -inf


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def template_key(x):
    w = (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def host_positions(scores, glob, ok, query, idx):
    """The numpy route: per row that has targets one lexsort of its eligible entries and the inverse permutation."""
    nb = np.full(len(query), -1, np.int64)
    for q in np.unique(query):
        key = template_key(scores[q]).astype(np.int64)
        entry = (key >= FLOOR) if ok is None else (key >= FLOOR) & ok[q]
        o = np.lexsort((glob, -key))
        o = o[entry[o]]
        pos = np.full(len(glob), -1, np.int64); pos[o] = np.arange(len(o))
        mine = query == q
        nb[mine] = pos[idx[mine]]                                           # (index_base 0: a global index is a column)
    return nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--excluded", type=int, default=20, help="elimination prints per query in case (d)")
    ap.add_argument("--reps", type=int, default=5, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--search-reps", type=int, default=2, help="kept repetitions of the two searches of the host route")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_positions_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G, cap = a.queries, a.gallery, a.cap
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    planted = S.plant_mates(a.seed, gal, cb, lats)
    rng = np.random.default_rng(a.seed)
    m = M.Matcher(cbb)
    out = {"queries": Q, "gallery": G, "cap": cap, "excluded_per_query": a.excluded, "reps": a.reps, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "device": m.device_info(0), "clocks": {"rank_positions_us, rank_hits_us, rank_filtered_us": "device: HIP events inside the library",
                                                  "search_*_ms, numpy_ms": "host: perf_counter around calls that return after their wait"}}
    m.gallery_add_packed(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    # the host route's first half: what asking the search for the matrix costs
    walls = {True: [], False: []}
    for rep in range(a.search_reps + 1):
        for want in (False, True):
            t0 = time.perf_counter()
            r = m.search_resident(qh, k=0, want_scores=want)
            if rep:
                walls[want].append((time.perf_counter() - t0) * 1e3)
    scores = r["scores"]                                                    # (the last search asked for them, and its matrix is the one ranked below)
    m.free_queries(qh)
    out["search_with_scores_ms"] = med(walls[True]); out["search_without_scores_ms"] = med(walls[False])
    out["scores_copy_ms"] = statistics.median(walls[True]) - statistics.median(walls[False])
    out["scores"] = {"zero_fraction": round(float((scores == 0).mean()), 4), "bytes": int(scores.nbytes)}
    glob = np.arange(G, dtype=np.int64)
    card = glob // 10
    sex = rng.integers(0, 2, card.max() + 1)[card]
    labels = (U64(1) << (glob % 10).astype(U64)) | (U64(1) << (10 + sex).astype(U64))
    masks = np.zeros((Q, 3), U64)
    for q in range(Q):                                                      # one to three finger positions and one sex allowed: the complement inside the two fields
        allowed = sum(1 << int(f) for f in rng.choice(10, int(rng.integers(1, 4)), replace=False)) | (1 << (10 + int(rng.integers(0, 2))))
        masks[q, 2] = U64(0xfff & ~allowed)
    excl = [rng.choice(G, a.excluded, replace=False).tolist() for _ in range(Q)]
    ok = ((labels[None, :] & masks[:, 2:3]) == 0)
    for q in range(Q):
        ok[q, excl[q]] = False
    hl = m.labels_create(labels)
    mates = {q: [g for g, _ in planted[q]] for q in range(Q)}
    qa = np.arange(Q, dtype=np.int32); ia = np.array([mates[q][0] for q in range(Q)], np.int64)
    qb = np.repeat(qa, 10); ib = np.concatenate([np.r_[mates[q][:4], rng.choice(G, 10 - len(mates[q][:4]), replace=False)] for q in range(Q)]).astype(np.int64)
    qc = np.zeros(1000, np.int32); ic = rng.choice(G, 1000, replace=False).astype(np.int64)
    flt = dict(labels=hl, masks=masks, excl=excl)
    ninf = float("-inf")
    cases = [("a: one target per latent", qa, ia, {}, None), ("b: ten per latent", qb, ib, {}, None), ("c: 1000 targets for one latent", qc, ic, {}, None),
             ("d: (a) with masks and exclusions", qa, ia, flt, ok)]
    rows = {}
    for name, query, idx, kw, okk in cases:
        us, hits_us, filt_us, host_ms = [], [], [], []
        for rep in range(a.reps + 1):
            got = m.rank_positions(query, idx, **kw)
            u = m.get_option("rank_positions_us")
            m.rank_hits(ninf, cap)
            h = m.get_option("rank_hits_us")
            f = None
            if kw:
                m.rank_hits_filtered(ninf, cap, **kw)
                f = m.get_option("rank_filtered_us")
            t0 = time.perf_counter()
            want = host_positions(scores, glob, okk, query, idx)
            hm = (time.perf_counter() - t0) * 1e3
            if rep:
                us.append(u); hits_us.append(h); host_ms.append(hm)
                if f is not None:
                    filt_us.append(f)
        read = len(np.unique(query)) * G * 4
        row = {"targets": int(len(query)), "rows_with_targets": int(len(np.unique(query))), "rank_positions_us": med(us), "rank_hits_us": med(hits_us), "numpy_ms": med(host_ms),
               "host_route_ms": out["scores_copy_ms"] + statistics.median(host_ms), "bytes_back": int(24 * len(query)),
               "row_read": {"bytes": read, "tb_per_s": round(read / (statistics.median(us) * 1e-6) / 1e12, 3) if statistics.median(us) > 0 and not kw else None},
               "listed": int((got["status"] == 0).sum()), "median_position": int(np.median(got["n_before"][got["status"] == 0])) if (got["status"] == 0).any() else None,
               "beyond_4096": int((got["n_before"] >= 4096).sum()), "equal_to_numpy": bool(np.array_equal(got["n_before"], want)),
               "below_the_hit_list": bool(statistics.median(us) < statistics.median(hits_us))}
        if filt_us:
            row["rank_filtered_us"] = med(filt_us)
            row["below_the_filtered_hit_list"] = bool(statistics.median(us) < statistics.median(filt_us))
        rows[name] = row
    out["cases"] = rows
    m.labels_free(hl); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
