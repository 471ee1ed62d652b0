#!/usr/bin/env python
"""What the link groups cost (afis_link_groups), on one MI355X, on planted matrices of 100 latents x 100 000 templates and of 1 000 prints x 100 000 templates (row i is
resident print i), uploaded with the parity tap afis_debug_rank_hits over a packed gallery of one-point templates.  Cells are uniform in [0, 1), so the share of cells
that reach is set by the threshold: 2.0 (no cell), 0.999 (about 1e-3 of the cells) and 0.0 (every cell).  tools/print_search_timing.py's method: every case is run in
every round, the rounds interleave the cases, `--reps` + 1 rounds with the first discarded; medians with the spread (max - min) beside them.

  link_groups_us       the call's device time (HIP events inside the library) at the three thresholds, AFIS_LINK_ANY; for the prints' matrix AFIS_LINK_MUTUAL at 0.999 too
  link_d2h_bytes       what the call returned from the device
  score_histogram_us   the streaming yardstick: afis_score_histogram with a single edge over the same matrix, an existing kernel that reads the matrix once; and the ratio
                       of the no-edge call to it
  host route           the only route without the call: the matrix downloaded (hipMemcpy device-to-host of its bytes into pageable memory, host clock) plus numpy's
                       keys and a dictionary union-find over the reaching cells (tests/link_model.py's, host clock).  Not run where every cell reaches (1e7 / 1e8 edges
                       in a Python loop)

The groups of every device call are checked against that model once.  Recorded, not asserted.  One JSON document on stdout and in --out."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
import link_model as LM  # noqa: E402

THRESHOLDS = (("none", 2.0), ("1e-3", 0.999), ("all", 0.0))


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def download_ms(n_bytes, reps):
    """hipMemcpy device-to-host of n_bytes from a fresh device buffer into pageable host memory, on the host clock, in milliseconds; the first copy is not reported."""
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]; hip.hipFree.argtypes = [vp]; hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]; hip.hipMemset.argtypes = [vp, C.c_int, C.c_size_t]
    src = vp()
    if hip.hipMalloc(C.byref(src), n_bytes) != 0 or hip.hipMemset(src, 0, n_bytes) != 0:
        raise RuntimeError("hipMalloc")
    dst = np.empty(n_bytes, np.uint8)
    out = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        if hip.hipMemcpy(dst.ctypes.data, src, n_bytes, 2) != 0:
            raise RuntimeError("hipMemcpy")
        if i:
            out.append((time.perf_counter() - t0) * 1e3)
    hip.hipFree(src)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3, help="kept rounds (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_groups_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    G = a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    rng = np.random.default_rng(a.seed)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    gal = S.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
                          off.copy(), rng.integers(0, 30, G).astype(np.int16), rng.integers(0, 30, G).astype(np.int16), rng.uniform(-1.5, 1.5, G).astype(np.float32),
                          rng.integers(0, cb.K, (G, cb.M)).astype(np.uint8))
    m = M.Matcher(cbb, taps=True)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    glob = np.arange(G, dtype=np.int64)
    out = {"gallery": G, "reps": a.reps, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "clocks": {"link_groups_us / score_histogram_us": "device: HIP events inside the library", "download_ms / host_union_ms": "host: perf_counter"}}
    edge = np.array([0.5], np.float32)
    for name, Q, row_node in (("latents_100", 100, None), ("prints_1000", min(1000, G), glob[:min(1000, G)])):
        scores = rng.random((Q, G), dtype=np.float32)
        m.debug_rank_hits(None, scores, float("-inf"), 1)
        cases = [("histogram_1_edge", lambda: m.score_histogram(edge), "score_histogram_us", None)]
        for tname, thr in THRESHOLDS:
            modes = ((LM.ANY, "any"),) + (((LM.MUTUAL, "mutual"),) if row_node is not None and tname == "1e-3" else ())
            for mode, mname in modes:
                cases.append(("link_%s_%s" % (mname, tname), (lambda t, md: lambda: m.link_groups(t, md, row_node=row_node, cap_groups=0, cap_members=0))(thr, mode), "link_groups_us", (thr, mode)))
        seen = {c[0]: {"us": [], "d2h": []} for c in cases}
        res = {"queries": Q, "matrix_bytes": int(scores.nbytes)}
        for rep in range(a.reps + 1):                                       # every case in every round: the cases interleave
            for cname, call, opt, _ in cases:
                got = call()
                if rep:
                    seen[cname]["us"].append(m.get_option(opt))
                    if opt == "link_groups_us":
                        seen[cname]["d2h"].append(m.get_option("link_d2h_bytes"))
                elif opt == "link_groups_us":
                    seen[cname]["counts"] = {k: got[k] for k in ("n_edges", "n_groups", "n_members")}
            note(f"{name}: round {rep} done")
        for cname, _, opt, _ in cases:
            res[cname] = {opt: med(seen[cname]["us"])}
            if opt == "link_groups_us":
                res[cname]["link_d2h_bytes"] = seen[cname]["d2h"][0]; res[cname].update(seen[cname]["counts"])
                res[cname]["share_of_cells_that_are_edges"] = seen[cname]["counts"]["n_edges"] / float(Q * G)
        stream = res["histogram_1_edge"]["score_histogram_us"]["median"]
        res["histogram_GB_per_s"] = round(scores.nbytes / (stream * 1e-6) / 1e9, 1)
        res["no_edge_call_over_histogram"] = round(res["link_any_none"]["link_groups_us"]["median"] / stream, 2)
        # the host route, and the check of the device's groups against it
        res["download_ms"] = med(download_ms(scores.nbytes, a.reps))
        for cname, _, opt, arg in cases:
            if arg is None or arg[0] == 0.0:
                continue
            thr, mode = arg
            t = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                want = LM.link(scores, thr, glob, row_node, mode)
                if rep:
                    t.append((time.perf_counter() - t0) * 1e3)
            res[cname]["host_union_ms"] = med(t)
            got = m.link_groups(thr, mode, row_node=row_node)
            assert got["n_edges"] == want["n_edges"] and np.array_equal(got["group_off"], want["group_off"]) and np.array_equal(got["member"], want["member"]), "the device's groups differ from the model's"
            res[cname]["host_route_ms"] = round(res["download_ms"]["median"] + res[cname]["host_union_ms"]["median"], 3)
        out[name] = res
    m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
