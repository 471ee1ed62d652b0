#!/usr/bin/env python
"""What the print search costs (afis_search_prints), on one MI355X with the headline's synthetic gallery (committed as bench.py commits it): 100 resident prints
against 100 000 prints by default.  Every comparison is interleaved, `--reps` + 1 times each, the first round discarded; medians with the spread (max - min) beside
them.  Two clocks: the HOST's (perf_counter around the call, nothing copied back) and the library's total_ms (HIP events around the launch groups of the searches
a call ran).

  (a) afis_search_prints against the only route there was before it: afis_search_weighted on the same context over HOST views of the same prints (the minutiae
      template as held, the texture codes decoded in numpy), n_wm = n_wt = 1, weights 1 and 0.3f.  Both queue the same scoring launches; the route over host views
      also uploads the views.  Whether the two give the same bits is recorded (from the discarded round).
  (b) option print_gather_us of (a) and the bytes the gather wrote, beside a device-to-device copy of the same byte count timed with HIP events in the same run,
      and beside the gather of ONE print (seven launches over 0.4 MB: what the launches of a group cost before any byte rate shows).

Recorded, not asserted.  One JSON document on stdout and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def host_view(t, words):
    """The query view of a resident print, made on the host: what the route over host views has to hold and upload."""
    out = T.FPTemplate(minu=list(t.minu[:1]))
    if t.tex and t.tex[0].n:
        x = t.tex[0]; n = min(x.n, 1000)
        codes = np.asarray(x.codes[:n], np.int64)
        des = np.ascontiguousarray(words[np.arange(words.shape[0])[None, :], codes].reshape(n, -1))
        out.tex.append(T.TextureTemplate(x.x[:n], x.y[:n], x.ori[:n], des=des))
    return out


def d2d_copy_us(n_bytes, reps):
    """hipMemcpyAsync device-to-device of n_bytes between two fresh buffers, HIP events around each copy, in microseconds (the runtime the library itself runs on,
    bound with ctypes: tools/bench_live_gallery.py's yardstick).  The first copy touches the fresh pages and is not reported."""
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
    chk(hip.hipMalloc(C.byref(src), n_bytes)); chk(hip.hipMalloc(C.byref(dst), n_bytes))
    chk(hip.hipEventCreate(C.byref(e0))); chk(hip.hipEventCreate(C.byref(e1)))
    out = []
    for i in range(reps + 1):
        chk(hip.hipEventRecord(e0, None)); chk(hip.hipMemcpyAsync(dst, src, n_bytes, 3, None)); chk(hip.hipEventRecord(e1, None)); chk(hip.hipEventSynchronize(e1))
        ms = C.c_float(0); chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        if i:
            out.append(ms.value * 1e3)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1); hip.hipFree(src); hip.hipFree(dst)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "print_search_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G = a.queries, a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    gal = S.make_packed_gallery(a.seed, G, cb)
    m = M.Matcher(cbb)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    note(f"{G} prints committed")
    idx = (np.arange(Q, dtype=np.int64) * (G // Q) + 7) % G                 # Q resident prints spread over the shard
    views = [host_view(gal.template(int(g)), cb.words) for g in idx]
    n_minu = np.array([v.minu[0].n if v.minu else 0 for v in views]); n_tex = np.array([v.tex[0].n if v.tex else 0 for v in views])
    view_bytes = int((n_minu * 392 + n_tex * 392).sum())
    gather_bytes = int((n_minu * 392 + (n_minu + 15) // 16 * 6144 + n_tex * 392).sum())      # points, descriptors, fragment tiles, decoded texture rows
    wm, wt = np.ones(Q, np.float32), np.full(Q, 0.3, np.float32)
    out = {"queries": Q, "templates": G, "reps": a.reps, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "query_prints": {"minutiae_mean": float(n_minu.mean()), "texture_points_mean": float(n_tex.mean()), "host_view_bytes": view_bytes},
           "clocks": {"host_ms": "perf_counter around the call (queries built or uploaded, scored, folded; nothing copied back)",
                      "total_ms": "afis_timing.total_ms: HIP events around the launch groups, summed over the searches the call ran",
                      "print_gather_us": "HIP events around each launch group's gather launches (print_queries.hip), summed"}}
    t = {"prints": {"host_ms": [], "total_ms": [], "gather_us": [], "h2d_bytes": []}, "weighted": {"host_ms": [], "total_ms": []}}
    equal = groups = None
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        got = m.search_prints(idx, wm, wt, want_scores=rep == 0)["scores"]   # (the discarded round copies the matrix back, for the comparison below)
        dt = (time.perf_counter() - t0) * 1e3
        tm = m.timing(); groups = tm["launch_groups"]
        if rep:
            t["prints"]["host_ms"].append(dt); t["prints"]["total_ms"].append(tm["total_ms"])
            t["prints"]["gather_us"].append(m.get_option("print_gather_us")); t["prints"]["h2d_bytes"].append(m.get_option("print_h2d_bytes"))
        t0 = time.perf_counter()
        ref = m.search_weighted(views, wm[:, None], wt[:, None], want_scores=rep == 0)["scores"]
        dt2 = (time.perf_counter() - t0) * 1e3
        if rep:
            t["weighted"]["host_ms"].append(dt2); t["weighted"]["total_ms"].append(m.timing()["total_ms"])
        else:
            equal = bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
        note(f"round {rep}: prints {dt:.0f} ms, host views {dt2:.0f} ms on the host clock")
    ra = {"weights": "1 at the minutiae template, 0.3f at the texture template", "launch_groups": groups, "same_bits": equal,
          "afis_search_prints": {k: med(v) for k, v in t["prints"].items()}, "afis_search_weighted_over_host_views": {k: med(v) for k, v in t["weighted"].items()}}
    ra["host_ms_gain"] = round(ra["afis_search_weighted_over_host_views"]["host_ms"]["median"] - ra["afis_search_prints"]["host_ms"]["median"], 3)
    ra["total_ms_difference"] = round(ra["afis_search_prints"]["total_ms"]["median"] - ra["afis_search_weighted_over_host_views"]["total_ms"]["median"], 3)
    out["a_call_against_host_views"] = ra
    gather = ra["afis_search_prints"]["gather_us"]
    copy = med(d2d_copy_us(gather_bytes, a.reps))
    # the floor: one print alone is one launch group — the gather's seven launches over 0.4 MB — so its time is what the launches cost before any byte rate shows
    floor, floor_bytes = [], int(n_minu[0] * 392 + (n_minu[0] + 15) // 16 * 6144 + n_tex[0] * 392)
    for rep in range(a.reps + 1):
        m.search_prints(idx[:1], wm[:1], wt[:1], want_scores=False)
        if rep:
            floor.append(m.get_option("print_gather_us"))
    rb = {"bytes_written_by_the_gather": gather_bytes, "print_gather_us": gather, "launch_groups": groups, "launches": 7 * groups, "device_to_device_copy_us": copy,
          "one_print": {"bytes_written": floor_bytes, "launches": 7, "print_gather_us": med(floor)}}
    rb["gather_over_copy_time"] = round(gather["median"] / copy["median"], 3)
    rb["gather_GB_per_s_written"] = round(gather_bytes / (gather["median"] * 1e-6) / 1e9, 1)
    rb["copy_GB_per_s_written"] = round(gather_bytes / (copy["median"] * 1e-6) / 1e9, 1)
    beyond = gather["median"] - groups * statistics.median(floor)
    rb["gather_us_beyond_the_groups_floors"] = beyond
    rb["GB_per_s_written_beyond_the_floors"] = round(gather_bytes / (beyond * 1e-6) / 1e9, 1) if beyond > 0 else None
    out["b_gather"] = rb
    m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
