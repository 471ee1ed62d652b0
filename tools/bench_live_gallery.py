#!/usr/bin/env python
"""What the live gallery costs (afis_gallery_reopen / _commit / _remove / _export), on one MI355X with the headline's synthetic gallery:

  edits      a full commit of G templates against reopen + stage + commit of N onto G - N, and against a removal of N from G; every repetition builds its contexts
             anew, the kinds interleaved (full, append, remove, full, ...), the first repetition reported but kept out of the medians (it pays the process's warm-up)
  compaction the removal's compaction kernels (parity tap afis_debug_compact_stats: HIP events around each launch) beside a device-to-device copy of the same bytes
             on the same box, timed with HIP events as well
  search     the step time against a gallery assembled by ten appends and against one committed at once, steps interleaved; the rank lists must agree and the
             two exported containers must be byte-identical

One JSON document on stdout (and to --out).  Edit and step times are host wall-clock around calls that return with the device idle; the compaction figures are device-event times."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def timed(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


def file_digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest(), os.path.getsize(path)


def dtod_copy_us(nbytes, reps):
    """hipMemcpyAsync device-to-device of nbytes between two fresh buffers, HIP-event time per copy in microseconds (the runtime the library itself runs on, bound with ctypes)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]; hip.hipFree.argtypes = [vp]
    hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]; hip.hipEventRecord.argtypes = [vp, vp]; hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]; hip.hipEventDestroy.argtypes = [vp]

    def chk(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    chk(hip.hipMalloc(C.byref(src), nbytes)); chk(hip.hipMalloc(C.byref(dst), nbytes))
    chk(hip.hipEventCreate(C.byref(e0))); chk(hip.hipEventCreate(C.byref(e1)))
    out = []
    for i in range(reps + 1):                                               # the first copy touches the fresh pages: not reported
        chk(hip.hipEventRecord(e0, None)); chk(hip.hipMemcpyAsync(dst, src, nbytes, 3, None)); chk(hip.hipEventRecord(e1, None)); chk(hip.hipEventSynchronize(e1))
        ms = C.c_float(0); chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        if i:
            out.append(ms.value * 1e3)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1); hip.hipFree(src); hip.hipFree(dst)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--edit", type=int, default=1000, help="templates appended / removed")
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--no-export", action="store_true", help="skip writing and comparing the two exported containers (2 x 50 KB per template on disk)")
    ap.add_argument("--other-lib", default="", metavar="SO", help="another build of libafis_hip.so (the parent commit's): its full commit is timed in the same rotation")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    G, N = a.gallery, a.edit
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    t0 = time.perf_counter()
    lats = S.make_latents(a.seed, a.queries)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats, G=G)
    gen_s = time.perf_counter() - t0
    head, tail = gal.slice(0, G - N), gal.slice(G - N, G)
    rng = np.random.default_rng(a.seed + 1)
    victims = np.sort(rng.permutation(G)[:N]).astype(np.int64)
    out = {"gallery": G, "edit": N, "queries": a.queries, "generation_s": round(gen_s, 1), "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12]}

    def committed(pg, **kw):
        m = M.Matcher(cbb, **kw); m.gallery_add_packed(pg)
        ms = timed(lambda: m.gallery_commit(0))
        return m, ms

    # ---- edits against a full commit ----
    rows = []
    for rep in range(a.reps):
        other_ms = None
        if a.other_lib:                                                     # the same full commit through another build of the library (the parent commit's), in the same rotation
            m, other_ms = committed(gal, lib_path=a.other_lib)
            m.close()
        m, full_ms = committed(gal)
        if rep == 0:
            out["device"] = m.device_info(0)
        m.close()
        m, head_ms = committed(head, taps=True)                             # the test library: the product objects + the tap that reports the compaction kernels' device time
        h0 = m.get_option("gallery_h2d_bytes")

        def do_append():
            m.gallery_reopen(); m.gallery_add_packed(tail); m.gallery_commit(0)
        append_ms = timed(do_append)
        append_h2d = m.get_option("gallery_h2d_bytes") - h0
        remove_ms = timed(lambda: m.gallery_remove(victims))
        rows.append({"rep": rep, "full_commit_ms": round(full_ms, 1), "commit_of_head_ms": round(head_ms, 1), "append_ms": round(append_ms, 1), "append_h2d_bytes": int(append_h2d),
                     "remove_ms": round(remove_ms, 1), "compact_us": m.compact_stats()[0], "compact_bytes": m.compact_stats()[1]})
        if other_ms is not None:
            rows[-1]["other_lib_full_commit_ms"] = round(other_ms, 1)
        m.close()
    kept = rows[1:] if len(rows) > 1 else rows
    med = lambda k: statistics.median(r[k] for r in kept)
    out["edits"] = {"reps": rows, "median_full_commit_ms": med("full_commit_ms"), "median_append_ms": med("append_ms"), "median_remove_ms": med("remove_ms"),
                    "full_over_append": round(med("full_commit_ms") / med("append_ms"), 1), "full_over_remove": round(med("full_commit_ms") / med("remove_ms"), 1),
                    "note": "commit / append / remove only; staging the templates on the host (afis_gallery_add_packed) is inside append_ms and outside full_commit_ms"}
    if a.other_lib:
        out["edits"]["median_other_lib_full_commit_ms"] = med("other_lib_full_commit_ms")

    # ---- the compaction kernels beside a plain device-to-device copy of the same bytes ----
    nbytes = int(kept[-1]["compact_bytes"])
    copies = dtod_copy_us(nbytes, 5)
    gbs = lambda us: round(nbytes / us / 1e3, 1)
    out["compaction"] = {"bytes_copied": nbytes, "kernels_us": [r["compact_us"] for r in rows], "kernels_gb_per_s": gbs(med("compact_us")),
                         "dtod_copy_us": [round(c, 1) for c in copies], "dtod_copy_gb_per_s": gbs(statistics.median(copies)),
                         "note": "GB/s = bytes copied / time (each byte is read once and written once); both times are device times between HIP events: around each of the six "
                                 "compaction launches, summed, and around the one copy"}

    # ---- search: ten appends against one commit ----
    first = G // 20
    per = (G - first + 9) // 10
    mx, _ = committed(gal.slice(0, first))
    lo = first
    while lo < G:
        hi = min(G, lo + per)
        mx.gallery_reopen(); mx.gallery_add_packed(gal.slice(lo, hi)); mx.gallery_commit(0)
        lo = hi
    my, _ = committed(gal)
    qx, qy = mx.upload_queries(lats), my.upload_queries(lats)
    tx, ty = [], []
    rx = ry = None
    for step in range(a.steps + 1):
        box = {}
        ms_x = timed(lambda: box.__setitem__("x", mx.search_resident(qx, k=24)))
        ms_y = timed(lambda: box.__setitem__("y", my.search_resident(qy, k=24)))
        rx, ry = box["x"], box["y"]
        if step > 0:
            tx.append(round(ms_x, 1)); ty.append(round(ms_y, 1))
    same = bool(np.array_equal(rx["topk_idx"], ry["topk_idx"]) and np.array_equal(rx["topk_score"].view(np.uint32), ry["topk_score"].view(np.uint32)))
    out["search"] = {"appended_step_ms": tx, "committed_step_ms": ty, "median_appended_ms": statistics.median(tx), "median_committed_ms": statistics.median(ty),
                     "rank_lists_identical": same, "assembled_as": f"{first} committed + ten appends of up to {per}"}
    if not a.no_export:
        try:
            with tempfile.TemporaryDirectory() as d:
                pa, pb = os.path.join(d, "a.gal"), os.path.join(d, "b.gal")
                ea = timed(lambda: mx.gallery_export(pa)); da = file_digest(pa); os.remove(pa)
                eb = timed(lambda: my.gallery_export(pb)); db = file_digest(pb); os.remove(pb)
            out["export"] = {"appended_ms": round(ea, 1), "committed_ms": round(eb, 1), "bytes": da[1], "byte_identical": da == db, "sha256": da[0]}
        except Exception as e:                                              # (a box without room for two 5 GB files)
            out["export"] = {"error": str(e)}
    mx.free_queries(qx); my.free_queries(qy); mx.close(); my.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
