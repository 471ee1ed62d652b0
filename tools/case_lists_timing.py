#!/usr/bin/env python
"""What a case list costs (afis_rank_case_hits / afis_rank_case_subject_hits), on one MI355X with the headline's synthetic gallery and latents (committed as bench.py
commits them): one search, then on the matrix it left on the device the latents are dealt into cases of `--case-size` (query i belongs to case i mod n_cases, so the
members of a case are interleaved) and every call below is made `--reps` + 1 times, the first discarded; medians with the spread (max - min) beside them:

  rank_case_hits          SUM and MAX, (-inf, cap): one candidate list per case
  rank_case_hits          SUM, (just above 0, cap): every positive fused score
  rank_case_subject_hits  SUM and MAX, (-inf, cap), ten templates per subject: k_subject_best, the fold over the maxima, k_rank_hits over 10 000 fused maxima

Clocks.  DEVICE (HIP events inside the library): option rank_cases_us around the call's launches, and its two parts, each from its own pair of events — case_fuse_us
(the fold; for subjects the maxima's memset and k_subject_best before it) and case_rank_us (k_rank_hits).  The fold's traffic is what it must move — n_q x G x 4 bytes
read, n_cases x G x 4 written — over case_fuse_us, set against the 6.3 TB/s a float4 copy reaches on this chip: where it stands, not a target.  HOST (perf_counter
around calls that return with the device idle): the only route open before — the search with `scores` requested (against the same search without), then the fold and
the sort in numpy.  Every list is checked against that numpy answer.  Recorded, not asserted.  One JSON document on stdout and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
COPY_TBS = 6.3                                                              # a float4 copy on this chip


def fuse(rows, case_of, mode):
    """The header's fold on whole rows: members in ascending query position; a member takes part when its score is >= 0 (a search's scores are -1 or >= +0.0)."""
    out = []
    for cid in np.unique(case_of):
        members = np.flatnonzero(case_of == cid)
        if mode == M.CASE_SUM:
            acc = np.zeros(rows.shape[1], np.float32); took = np.zeros(rows.shape[1], bool)
            for i in members:
                part = rows[i] >= 0
                acc = np.where(part, (acc + rows[i]).astype(np.float32), acc); took |= part
            out.append(np.where(took, acc, np.float32(-1)))
        else:
            out.append(rows[members].max(axis=0))
    return np.array(out, np.float32)


def lists(fused, names, thr, cap):
    n = np.empty(len(fused), np.int64); a = np.full((len(fused), cap), -1, np.int64); sc = np.full((len(fused), cap), -np.inf, np.float32)
    for c, row in enumerate(fused):
        at = np.flatnonzero(row >= thr)
        at = at[np.lexsort((names[at], -row[at].astype(np.float64)))][:cap]
        n[c] = int((row >= thr).sum()); a[c, :len(at)] = names[at]; sc[c, :len(at)] = row[at]
    return n, a, sc


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--case-size", type=int, default=4)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_case_lists.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    G, Q, cap = a.gallery, a.queries, a.cap
    n_cases = max(1, Q // a.case_size)
    case_of = (np.arange(Q) % n_cases).astype(np.int64)
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats, G=G)
    out = {"gallery": G, "queries": Q, "cases": n_cases, "case_size": a.case_size, "cap": cap, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "clocks": {"rank_cases_us, case_fuse_us, case_rank_us": "device: HIP events inside the library", "wall_ms": "host: perf_counter around calls that return with the device idle"}}
    m = M.Matcher(cbb)
    out["device"] = m.device_info(0)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    m.search_resident(qh, k=0)                                              # (the first search of a context allocates)
    walls = {"search_without_scores": [], "search_with_scores": []}
    for rep in range(a.reps + 1):
        for name, want in (("search_without_scores", False), ("search_with_scores", True)):
            t0 = time.perf_counter()
            r = m.search_resident(qh, k=0, want_scores=want)
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                walls[name].append(round(ms, 2))
    scores = r["scores"]                                                    # the last search asked for them: its matrix is the one ranked below
    out["search_wall_ms"] = {k: med(v) for k, v in walls.items()}
    out["scores"] = {"zero_fraction": round(float((scores == 0).mean()), 4), "positive_per_query_median": int(np.median((scores > 0).sum(axis=1)))}
    hair = float(np.nextafter(np.float32(0), np.float32(1)))
    subject = np.arange(G, dtype=np.int64) // 10
    h = m.subjects_create(subject)
    best = scores[:, :G // 10 * 10].reshape(Q, G // 10, 10).max(axis=2) if G % 10 == 0 else None
    calls = [("rank_case_hits(SUM, -inf)", None, M.CASE_SUM, float("-inf")), ("rank_case_hits(MAX, -inf)", None, M.CASE_MAX, float("-inf")),
             ("rank_case_hits(SUM, >0)", None, M.CASE_SUM, hair),
             ("rank_case_subject_hits(SUM, -inf), ten templates per subject", h, M.CASE_SUM, float("-inf")),
             ("rank_case_subject_hits(MAX, -inf), ten templates per subject", h, M.CASE_MAX, float("-inf"))]
    out["calls"] = {}
    for name, handle, mode, thr in calls:
        us = {"rank_cases_us": [], "case_fuse_us": [], "case_rank_us": []}; wall = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            got = m.rank_case_hits(case_of, mode, thr, cap) if handle is None else m.rank_case_subject_hits(handle, case_of, mode, thr, cap)
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                for k in us:
                    us[k].append(m.get_option(k))
                wall.append(round(ms, 3))
        t0 = time.perf_counter()
        if handle is None:
            want = lists(fuse(scores, case_of, mode), np.arange(G, dtype=np.int64), np.float32(thr), cap)
            names = got["idx"]
        else:
            want = lists(fuse(best, case_of, mode), np.arange(G // 10, dtype=np.int64), np.float32(thr), cap) if best is not None else None
            names = got["subject"]
        numpy_ms = (time.perf_counter() - t0) * 1e3
        same = None if want is None else bool(np.array_equal(want[0], got["n_hits"]) and np.array_equal(want[1], names) and np.array_equal(want[2].view(np.uint32), got["score"].view(np.uint32)))
        row = {k: med(v) for k, v in us.items()}
        row.update({"call_wall_ms": med(wall), "n_hits_median": int(np.median(got["n_hits"])), "equal_to_the_numpy_route": same, "numpy_fold_and_sort_ms": round(numpy_ms, 1)})
        if handle is None:
            moved = (Q + n_cases) * G * 4
            tbs = moved / (row["case_fuse_us"]["median"] * 1e-6) / 1e12 if row["case_fuse_us"]["median"] > 0 else None
            row["fold"] = {"bytes_read_and_written": moved, "tb_per_s": None if tbs is None else round(tbs, 3), "of_a_float4_copy": None if tbs is None else round(tbs / COPY_TBS, 3)}
            row["host_route_ms"] = round(out["search_wall_ms"]["search_with_scores"]["median"] - out["search_wall_ms"]["search_without_scores"]["median"] + numpy_ms, 1)
        out["calls"][name] = row
    m.subjects_free(h); m.free_queries(qh); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
