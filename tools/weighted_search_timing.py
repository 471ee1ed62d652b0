#!/usr/bin/env python
"""What the weighted search costs (afis_search_weighted), on one MI355X with the headline's synthetic gallery and latents (committed as bench.py commits them): 100
latents x 100 000 templates by default.  Every comparison is interleaved, `--reps` + 1 times each, the first round discarded; medians with the spread (max - min)
beside them.  Two clocks: the HOST's (perf_counter around the call: latents uploaded, scored, nothing copied back unless the route needs it) and the library's
total_ms (HIP events around the launch groups of the searches a call ran).

  (a) all 28 + 1 templates (weights 1, texture 0.3f) against the only route there was before the call existed: one afis_match_all_templates call per latent — its
      [G][29] result crosses PCIe — and the fold on the host (numpy, fp64, the header's order).  That route is run with the PARENT commit's library, loaded into the
      same process as tools/lib_ab.py loads it (--parent-lib; default tools/libafis_prev.so, a build of the parent commit, not kept in git).  Whether the two routes
      give the same bits is recorded.
  (b) the reference's selection (weights 1 at 26, 2, 11 and 0.3f at texture 0) against afis_search on the same context: the scorers are the same, the difference is
      the price of the plan and the fold.
  (c) option weighted_fold_us of (a) against the estimate for a memory-bound pass: 16 bytes per pseudo-pair read and 4 bytes per cell written, at the 6.3 TB/s a
      float4 copy reaches on this device and at the 8 TB/s of its specification.

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
    print(*a, file=sys.stderr, flush=True)                                  # progress: a round of route (a) takes a minute


def host_fold(sc, n_minu, wm, wt):
    """One latent's row from afis_match_all_templates' [G][n_minu + n_tex] vectors: the header's definition (the empty entries are put back by the caller)."""
    acc = np.zeros(sc.shape[0], np.float64)
    for i in range(min(n_minu, len(wm))):
        if wm[i] != 0:
            acc = acc + np.float64(wm[i]) * sc[:, i].astype(np.float64)
    for t in range(min(sc.shape[1] - n_minu, len(wt))):
        if wt[t] != 0:
            acc = acc + np.float64(wt[t]) * sc[:, n_minu + t].astype(np.float64)
    return acc.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "libafis_prev.so"), help="libafis_hip.so of the parent commit, for route (a)'s yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_search_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G = a.queries, a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats, G=G)
    m = M.Matcher(cbb)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    note(f"{Q} latents x {G} templates committed")
    parent = None
    if os.path.exists(a.parent_lib):
        parent = M.Matcher(cbb, lib_path=a.parent_lib)
        assert not hasattr(parent.lib, "afis_search_weighted"), "--parent-lib must be a build of the parent commit"
        parent.gallery_add_packed(gal); parent.gallery_commit(0)
    n_minu = max(len(L.minu) for L in lats)
    ones, sel = np.ones(n_minu, np.float32), np.zeros(n_minu, np.float32)
    sel[[26, 2, 11]] = 1.0
    wt = np.array([0.3], np.float32)
    out = {"queries": Q, "templates": G, "reps": a.reps, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "latent_templates": sorted({(len(L.minu), len(L.tex)) for L in lats}),
           "clocks": {"host_ms": "perf_counter around the route (latents uploaded and scored; route (a)'s yardstick also copies its vectors back and folds them)",
                      "total_ms": "afis_timing.total_ms: HIP events around the launch groups, summed over the searches the route ran",
                      "weighted_fold_us": "HIP events around each k_fold_templates launch, summed over the batches"}}

    # (a) all templates
    t = {"weighted": {"host_ms": [], "total_ms": [], "fold_us": []}, "parent": {"host_ms": [], "total_ms": []}}
    pseudo = pairs = groups = None
    equal = None
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        got = m.search_weighted(lats, ones, wt, want_scores=rep == 0)["scores"]     # (the discarded round copies the matrix back, for the comparison below)
        dt = (time.perf_counter() - t0) * 1e3
        tm = m.timing()
        pseudo, pairs, groups = m.get_option("weighted_pseudo_queries"), tm["pairs"], tm["launch_groups"]
        if rep:
            t["weighted"]["host_ms"].append(dt); t["weighted"]["total_ms"].append(tm["total_ms"]); t["weighted"]["fold_us"].append(m.get_option("weighted_fold_us"))
        if parent is not None:
            t0 = time.perf_counter()
            rows, dev_ms = [], 0.0
            for L in lats:
                qs, rs, sc = parent.One2One_matching_all_templates(L)
                dev_ms += parent.timing()["total_ms"]
                row = host_fold(sc, len(L.minu), ones, wt)
                row[rs == 2] = -1.0
                rows.append(row)
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                t["parent"]["host_ms"].append(dt); t["parent"]["total_ms"].append(dev_ms)
            note(f"(a) round {rep}: weighted {tm['total_ms']:.0f} ms on the device, the parent's route {dt:.0f} ms on the host")
            if rep == 0:
                equal = bool(np.array_equal(got.view(np.uint32), np.stack(rows).view(np.uint32)))
    ra = {"weights": "1 at every minutiae template, 0.3f at texture 0", "pseudo_queries": pseudo, "pairs": pairs, "launch_groups": groups,
          "afis_search_weighted": {k: med(v) for k, v in t["weighted"].items()}}
    if parent is not None:
        ra["parent_route"] = dict({k: med(v) for k, v in t["parent"].items()}, what="per latent afis_match_all_templates of the parent commit's library (total_ms: the last batch of each "
                                  "call only, a lower bound), its [G][width] vectors copied back, the fp64 fold in numpy")
        ra["same_bits"] = equal
        ra["host_time_ratio"] = round(ra["afis_search_weighted"]["host_ms"]["median"] / ra["parent_route"]["host_ms"]["median"], 4)
    else:
        ra["parent_route"] = "not measured: no parent library at --parent-lib"
    out["a_all_templates"] = ra

    # (b) the reference's selection against afis_search
    t = {"weighted": {"host_ms": [], "total_ms": [], "fold_us": []}, "search": {"host_ms": [], "total_ms": []}}
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        m.search_weighted(lats, sel, wt, want_scores=False)
        dt = (time.perf_counter() - t0) * 1e3
        tm = m.timing()
        pseudo_b = m.get_option("weighted_pseudo_queries")
        if rep:
            t["weighted"]["host_ms"].append(dt); t["weighted"]["total_ms"].append(tm["total_ms"]); t["weighted"]["fold_us"].append(m.get_option("weighted_fold_us"))
        t0 = time.perf_counter()
        m.search(lats, k=0, want_scores=False)
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            t["search"]["host_ms"].append(dt); t["search"]["total_ms"].append(m.timing()["total_ms"])
    rb = {"weights": "1 at minutiae templates 26, 2, 11, 0.3f at texture 0", "pseudo_queries": pseudo_b,
          "afis_search_weighted": {k: med(v) for k, v in t["weighted"].items()}, "afis_search": {k: med(v) for k, v in t["search"].items()}}
    rb["host_time_ratio"] = round(rb["afis_search_weighted"]["host_ms"]["median"] / rb["afis_search"]["host_ms"]["median"], 4)
    rb["total_ms_ratio"] = round(rb["afis_search_weighted"]["total_ms"]["median"] / rb["afis_search"]["total_ms"]["median"], 4)
    out["b_reference_selection"] = rb

    # (c) the fold against a memory-bound pass
    n_bytes = pseudo * G * 16 + Q * G * 4
    fold = ra["afis_search_weighted"]["fold_us"]["median"]
    out["c_fold"] = {"pseudo_queries": pseudo, "bytes_read_and_written": n_bytes, "measured_us": fold,
                     "estimate_us_at_6.3_TB_per_s": round(n_bytes / 6.3e12 * 1e6, 1), "estimate_us_at_8_TB_per_s": round(n_bytes / 8e12 * 1e6, 1),
                     "achieved_TB_per_s": round(n_bytes / (fold * 1e-6) / 1e12, 3) if fold else None}
    m.close()
    if parent is not None:
        parent.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
