#!/usr/bin/env python
"""What the evidence calls of a candidate list cost (afis_pair_alignments, afis_texture_correspondences_pairs), on one MI355X with the headline's synthetic gallery and
latents (committed as bench.py commits them): 100 latents x their 100 best candidates of a 100 000-print planted gallery by default.  One search, the lists of
afis_rank_hits(-inf, 100) flattened; then three routes INTERLEAVED on the one context — route after route within a repetition, `--reps` kept repetitions after a
discarded first, median and spread (max - min) of each figure:

  alignments      afis_pair_alignments: option pair_alignments_us, the DEVICE clock (HIP events around every chunk's launches, summed), and the HOST clock
                  (perf_counter around the C call alone, arrays made before it)
  texture_export  afis_texture_correspondences_pairs with pt, sim and part: option texture_correspondences_us, and the host clock
  lists_route     what a host had to do for the same moments with the exports: afis_correspondences_pairs (option correspondences_us), plus the texture export (as
                  above, run again inside this route), plus the moments of all four lists in numpy int64; device clock = the two calls' options added, host clock =
                  the two C calls plus the numpy pass, which is also given alone

Beside them: whether the records of the alignment call equal the numpy moments of the exports (they must), how many records hold survivors, the bytes each route
returns, the search step of the same run, and whether afis_rank_hits returns afterwards what it returned before (the matrix survived).  Measured, not asserted; nothing
here is tuned for.  One JSON document on stdout and in --out."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def numpy_moments(counts, xy, tcounts, txy):
    """[n][4][9] int64: the moments of the three minutiae lists (pixels) and of the texture list (blocks -> 16 b + 24), rows beyond the counts masked out."""
    n = len(tcounts)
    out = np.zeros((n, 4, 9), np.int64)
    for k in range(4):
        pts = (xy[:, k] if k < 3 else 16 * txy.astype(np.int64) + 24).astype(np.int64)
        cn = np.maximum(counts[:, k] if k < 3 else tcounts, 0)
        live = (np.arange(pts.shape[1])[None, :] < cn[:, None]).astype(np.int64)
        lx, ly, rx, ry = (pts[:, :, c] * live for c in range(4))
        out[:, k] = np.stack([cn, lx.sum(1), ly.sum(1), rx.sum(1), ry.sum(1), (lx * rx + ly * ry).sum(1), (lx * ry - ly * rx).sum(1), (lx * lx + ly * ly).sum(1),
                              (rx * rx + ry * ry).sum(1)], axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_evidence_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G, cap = a.queries, a.gallery, a.cap
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats)
    m = M.Matcher(cbb)
    out = {"queries": Q, "gallery": G, "cap": cap, "reps": a.reps, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "corr_pairs_per_launch": m.get_option("corr_pairs_per_launch"),
           "clocks": {"*_us": "device: HIP events inside the library, around every chunk's launches, summed", "*_ms": "host: perf_counter around the C calls, which return after their wait",
                      "search_total_ms": "device: afis_timing.total_ms of the search whose lists are opened"}}
    m.gallery_add_packed(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    m.search_resident(qh, k=0)                                              # warm-up: first-use allocations
    m.search_resident(qh, k=0)
    out["search_total_ms"] = m.timing()["total_ms"]
    before = m.rank_hits(float("-inf"), cap)
    n = Q * cap
    query = np.repeat(np.arange(Q, dtype=np.int32), cap); idx = np.ascontiguousarray(before["idx"]).reshape(-1)
    status = np.zeros(n, np.int32); mom = np.zeros((n, 4), M.CORR_MOMENTS)
    counts = np.zeros((n, 3), np.int32); xy = np.zeros((n, 3, 120, 4), np.int16); part = np.zeros((n, 3), np.float32)
    tcounts = np.zeros(n, np.int32); txy = np.zeros((n, 200, 4), np.int16); tpt = np.zeros((n, 200, 2), np.int16); tsim = np.zeros((n, 200), np.float32); tpart = np.zeros(n, np.float32)
    p = M._ptr

    def alignments():
        t0 = time.perf_counter()
        m._chk(m.lib.afis_pair_alignments(m.ctx, qh[0], n, p(query, C.c_int32), p(idx, C.c_int64), p(status, C.c_int32), C.c_void_p(mom.ctypes.data)))
        return (time.perf_counter() - t0) * 1e3, m.get_option("pair_alignments_us")

    def texture_export():
        t0 = time.perf_counter()
        m._chk(m.lib.afis_texture_correspondences_pairs(m.ctx, qh[0], n, p(query, C.c_int32), p(idx, C.c_int64), p(tcounts, C.c_int32), p(txy, C.c_int16), p(tpt, C.c_int16), p(tsim, C.c_float), p(tpart, C.c_float)))
        return (time.perf_counter() - t0) * 1e3, m.get_option("texture_correspondences_us")

    def minutiae_export():
        t0 = time.perf_counter()
        m._chk(m.lib.afis_correspondences_pairs(m.ctx, qh[0], n, p(query, C.c_int32), p(idx, C.c_int64), p(counts, C.c_int32), p(xy, C.c_int16), p(part, C.c_float)))
        return (time.perf_counter() - t0) * 1e3, m.get_option("correspondences_us")

    keys = ("alignments_ms", "alignments_us", "texture_export_ms", "texture_export_us", "lists_route_ms", "lists_route_us", "lists_route_minutiae_ms", "lists_route_minutiae_us",
            "lists_route_texture_ms", "lists_route_texture_us", "lists_route_numpy_ms")
    runs = {k: [] for k in keys}
    model = None
    for rep in range(a.reps + 1):                                           # interleaved: every route once per repetition
        r = {}
        r["alignments_ms"], r["alignments_us"] = alignments()
        r["texture_export_ms"], r["texture_export_us"] = texture_export()
        r["lists_route_minutiae_ms"], r["lists_route_minutiae_us"] = minutiae_export()
        r["lists_route_texture_ms"], r["lists_route_texture_us"] = texture_export()
        t0 = time.perf_counter()
        model = numpy_moments(counts, xy, tcounts, txy)
        r["lists_route_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        r["lists_route_ms"] = r["lists_route_minutiae_ms"] + r["lists_route_texture_ms"] + r["lists_route_numpy_ms"]
        r["lists_route_us"] = r["lists_route_minutiae_us"] + r["lists_route_texture_us"]
        if rep:
            for k in keys: runs[k].append(r[k])
    after = m.rank_hits(float("-inf"), cap)
    got = np.stack([mom[f] for f in M.CORR_MOMENTS.names], axis=2)
    out["figures"] = {k: med(v) for k, v in runs.items()}
    out["pairs"] = n
    out["records_equal_the_numpy_moments_of_the_exports"] = bool(np.array_equal(got, model))
    out["records_with_survivors"] = [int((got[:, k, 0] > 0).sum()) for k in range(4)]
    out["not_covered"] = int((status != 0).sum())
    out["bytes_returned"] = {"alignments": int(mom.nbytes + status.nbytes), "texture_export": int(tcounts.nbytes + txy.nbytes + tpt.nbytes + tsim.nbytes + tpart.nbytes),
                             "lists_route": int(counts.nbytes + xy.nbytes + part.nbytes + tcounts.nbytes + txy.nbytes + tpt.nbytes + tsim.nbytes + tpart.nbytes)}
    out["matrix_survived"] = bool(all(before[k].tobytes() == after[k].tobytes() for k in ("n_hits", "idx", "score")))
    f = out["figures"]
    out["alignments_over_lists_route"] = {"device": f["alignments_us"]["median"] / f["lists_route_us"]["median"], "host": f["alignments_ms"]["median"] / f["lists_route_ms"]["median"]}
    m.free_queries(qh); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
