#!/usr/bin/env python
"""A/B of the calls that read the last search's matrix in place between this tree's libafis_hip.so and another build's (--parent: the parent commit's), in ONE process on
ONE MI355X with the headline's synthetic gallery and latents (100 latents x 100 000 templates by default), one search per library, the two libraries ALTERNATING
repetition by repetition, `--reps` kept after a discarded first (median, spread = max - min, every value).  The filter is tools/filtered_hits_timing.py's — labels of
ten one-hot fingers and a sex, per latent one none_of mask and 20 exclusions — and the persons are cards of ten prints (10 000 at the default size):

  score_stats       afis_score_stats on axis 0 and axis 1, plain and with masks; afis_subject_score_stats with masks on both axes
  score_histogram   afis_score_histogram, 256 bins on axis 0 and 16 bins on axis 1; the person form of both
  entries_at        afis_entries_at, 64 random ranks per row; afis_subject_entries_at
  rank_positions    afis_rank_positions, ten targets per latent, plain and filtered; afis_count_before on the same targets; afis_rank_subject_positions on their persons
  rank_hits         afis_rank_hits_filtered and afis_rank_subject_hits_filtered at cap 100 (check_filtered resolves their exclusions)
  link_groups       afis_link_groups and afis_link_subject_groups, AFIS_LINK_ANY at the histogram edge that about 1e-3 of the cells reach

Per figure — the call's device option (HIP events inside the library) and the host clock around the C call alone — both libraries' values, whether this tree's median lies
inside the other library's [min, max], and if not how far outside in units of that spread; per call whether every returned byte equals the other library's.  Recorded,
not asserted.  One JSON document on stdout and in --out."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
U64 = np.uint64


def join(a):
    runs = [json.load(open(f)) for f in a.join]
    slow = {"us": {}, "host_ms": {}}
    for i, r in enumerate(runs):
        for label, c in r["calls"].items():
            for key in slow:
                v = c[key]
                if not v["tree_median_inside_parent_spread"] and v["tree"]["median"] > v["parent"]["median"]:
                    slow[key].setdefault(label, []).append("run %d: %s against the parent's %s .. %s" % (i + 1, v["tree"]["median"], min(v["parent"]["all"]), max(v["parent"]["all"])))
    doc = {"what": "tools/matrix_call_ab.py --parent <the parent commit's libafis_hip.so>, two runs on one MI355X joined by --join: this tree's context created and run first, then (--parent-first) the parent's",
           "every_byte_equal_in_both_runs": bool(all(r["every_byte_equal"] for r in runs)),
           "device_figures_on_the_slow_side_of_the_parents_spread": slow["us"],
           "device_figures_on_the_slow_side_in_both_runs": sorted(k for k, v in slow["us"].items() if len(v) == len(runs)), "device_note": a.device_note,
           "host_medians_on_the_slow_side_of_the_parents_spread": slow["host_ms"],
           "host_medians_on_the_slow_side_in_both_runs": sorted(k for k, v in slow["host_ms"].items() if len(v) == len(runs)), "host_note": a.host_note, "runs": runs}
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "runs"}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--excluded", type=int, default=20, help="elimination prints (or persons) per query")
    ap.add_argument("--reps", type=int, default=5, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--parent", help="libafis_hip.so built from the parent commit (required unless --join)")
    ap.add_argument("--parent-first", action="store_true", help="create the parent's context first and run it first in every repetition (the order's own effect)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_call_ab.json"), help="where the JSON document goes ('' = stdout only)")
    ap.add_argument("--join", nargs=2, metavar="RUN", help="no device work: two runs' documents (this tree first, then --parent-first, each written with its own --out) joined into --out under a head "
                    "that names every figure on the slow side of the parent's [min, max], run by run")
    ap.add_argument("--device-note", default="", help="--join: what is known of the device figures named in the head")
    ap.add_argument("--host-note", default="", help="--join: what is known of the host medians named in the head")
    a = ap.parse_args()
    if a.join:
        return join(a)
    if not a.parent:
        ap.error("--parent is required")
    Q, G = a.queries, a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats)
    rng = np.random.default_rng(a.seed)
    glob = np.arange(G, dtype=np.int64)
    card = glob // 10
    sex = rng.integers(0, 2, card.max() + 1)[card]
    labels = (U64(1) << (glob % 10).astype(U64)) | (U64(1) << (10 + sex).astype(U64))
    masks = np.zeros((Q, 3), U64)
    for q in range(Q):                                                      # one to three finger positions and one sex allowed: the complement inside the two fields
        allowed = sum(1 << int(f) for f in rng.choice(10, int(rng.integers(1, 4)), replace=False)) | (1 << (10 + int(rng.integers(0, 2))))
        masks[q, 2] = U64(0xfff & ~allowed)
    excl = [rng.choice(G, a.excluded, replace=False).tolist() for _ in range(Q)]
    excl_s = [np.unique(card[e]).tolist() for e in excl]
    libs, scores = {}, None
    for name, path in (("tree", M.LIB_PATH), ("parent", a.parent))[::-1 if a.parent_first else 1]:
        m = M.Matcher(cbb, lib_path=path)
        m.gallery_add_packed(gal); m.gallery_commit(0)
        hl, hj = m.labels_create(labels), m.subjects_create(card)           # (before the search: creating a handle gives the matrix up)
        qh = m.upload_queries(lats)
        sc = m.search_resident(qh, k=0, want_scores=True)["scores"]         # ONE search: every call below reads the matrix it left
        m.free_queries(qh)
        scores = sc if scores is None else scores
        assert sc.tobytes() == scores.tobytes()
        libs[name] = (m, hl, hj)
    m0 = libs["tree"][0]
    out = {"queries": Q, "gallery": G, "subjects": int(card.max()) + 1, "excluded_per_query": a.excluded, "reps": a.reps, "alternating": True, "order": list(libs),
           "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m0.device_info(0),
           "clocks": {"*_us": "device: the option named, HIP events inside the library", "host_ms": "host: perf_counter around the C call alone"}}
    top = float(scores.max())
    edges = {256: np.linspace(0.0, top, 255).astype(np.float32), 16: np.linspace(0.0, top, 15).astype(np.float32)}
    reach = np.cumsum(m0.score_histogram(edges[256]).sum(axis=0)[::-1])[::-1][1:]      # reach[j]: the cells at or above edges[j]
    thr = float(edges[256][int(np.argmin(np.abs(reach - 1e-3 * Q * G)))])
    out["link_min_score"] = thr; out["link_cells_reaching"] = int((scores >= thr).sum())
    tq = np.repeat(np.arange(Q, dtype=np.int32), 10)
    ti = np.ascontiguousarray(rng.integers(0, G, 10 * Q).astype(np.int64))
    ts = np.ascontiguousarray(scores[tq, ti]); tp = np.ascontiguousarray(card[ti])
    rq = np.repeat(np.arange(Q, dtype=np.int32), 64)
    rr = np.ascontiguousarray(rng.integers(0, G, 64 * Q).astype(np.int64)); rs = np.ascontiguousarray(rr % (int(card.max()) + 1))
    p = M._ptr
    ninf = float("-inf")

    def filt(m, hl, persons, which):
        """which: "plain", "masks" or "masks + exclusions" -> the keep-alive and the four filter arguments"""
        _, keep, f = m._filter(None if which == "plain" else hl, None if which == "plain" else masks, (excl_s if persons else excl) if "exclusions" in which else None, Q)
        return keep, f

    def stats(m, hl, hj, axis, which, persons):
        keep, f = filt(m, hl, persons, which)
        o = np.zeros(Q if axis == 0 else (int(card.max()) + 1 if persons else G), M.SCORE_STAT)
        fn, h = (m.lib.afis_subject_score_stats, (hj[0],)) if persons else (m.lib.afis_score_stats, ())
        return lambda: fn(m.ctx, *h, axis, *f, Q, o.ctypes.data_as(C.c_void_p)), (o,), "subject_score_stats_us" if persons else "score_stats_us", keep

    def hist(m, hl, hj, axis, bins, persons):
        keep, f = filt(m, hl, persons, "plain")
        e = edges[bins]
        o = np.zeros((Q if axis == 0 else (int(card.max()) + 1 if persons else G), len(e) + 1), np.int64)
        fn, h = (m.lib.afis_subject_score_histogram, (hj[0],)) if persons else (m.lib.afis_score_histogram, ())
        return lambda: fn(m.ctx, *h, axis, *f, Q, len(e), p(e, C.c_float), p(o, C.c_int64)), (o,), "subject_score_histogram_us" if persons else "score_histogram_us", keep

    def at(m, hl, hj, persons):
        keep, f = filt(m, hl, persons, "plain")
        n = len(rq); st = np.zeros(n, np.int32); ix = np.zeros(n, np.int64); sc = np.zeros(n, np.float32); bi = np.zeros(n, np.int64)
        if persons:
            return (lambda: m.lib.afis_subject_entries_at(m.ctx, hj[0], *f, Q, n, p(rq, C.c_int32), p(rs, C.c_int64), p(st, C.c_int32), p(ix, C.c_int64), p(sc, C.c_float), p(bi, C.c_int64)),
                    (st, ix, sc, bi), "subject_entries_at_us", keep)
        return lambda: m.lib.afis_entries_at(m.ctx, *f, Q, n, p(rq, C.c_int32), p(rr, C.c_int64), p(st, C.c_int32), p(ix, C.c_int64), p(sc, C.c_float)), (st, ix, sc), "entries_at_us", keep

    def pos(m, hl, hj, form, which):
        keep, f = filt(m, hl, form == "persons", which)
        n = len(tq); st = np.zeros(n, np.int32); nb = np.zeros(n, np.int64); sc = np.zeros(n, np.float32); bi = np.zeros(n, np.int64)
        if form == "count":
            return lambda: m.lib.afis_count_before(m.ctx, *f, Q, n, p(tq, C.c_int32), p(ts, C.c_float), p(ti, C.c_int64), p(nb, C.c_int64)), (nb,), "rank_positions_us", keep
        if form == "persons":
            return (lambda: m.lib.afis_rank_subject_positions(m.ctx, hj[0], *f, Q, n, p(tq, C.c_int32), p(tp, C.c_int64), p(st, C.c_int32), p(nb, C.c_int64), p(sc, C.c_float), p(bi, C.c_int64)),
                    (st, nb, sc, bi), "rank_positions_us", keep)
        return lambda: m.lib.afis_rank_positions(m.ctx, *f, Q, n, p(tq, C.c_int32), p(ti, C.c_int64), p(st, C.c_int32), p(nb, C.c_int64), p(sc, C.c_float)), (st, nb, sc), "rank_positions_us", keep

    def hits(m, hl, hj, persons):
        keep, f = filt(m, hl, persons, "masks + exclusions")
        nh = np.zeros(Q, np.int64); ix = np.zeros((Q, 100), np.int64); sc = np.zeros((Q, 100), np.float32); bi = np.zeros((Q, 100), np.int64)
        if persons:
            return (lambda: m.lib.afis_rank_subject_hits_filtered(m.ctx, hj[0], *f, Q, ninf, 100, p(nh, C.c_int64), p(ix, C.c_int64), p(sc, C.c_float), p(bi, C.c_int64)),
                    (nh, ix, sc, bi), "rank_filtered_us", keep)
        return lambda: m.lib.afis_rank_hits_filtered(m.ctx, *f, Q, ninf, 100, p(nh, C.c_int64), p(ix, C.c_int64), p(sc, C.c_float)), (nh, ix, sc), "rank_filtered_us", keep

    def link(m, hl, hj, persons):
        keep, f = filt(m, hl, persons, "plain")
        cnt = np.zeros(4, np.int64); goff = np.zeros(Q + G + 1, np.int64); mem = np.zeros(Q + G, np.int64)
        c = [C.cast(cnt.ctypes.data + 8 * i, C.POINTER(C.c_int64)) for i in range(4)]
        fn, h = (m.lib.afis_link_subject_groups, (hj[0],)) if persons else (m.lib.afis_link_groups, ())
        return lambda: fn(m.ctx, *h, *f, Q, None, thr, 0, Q + G, Q + G, *c, p(goff, C.c_int64), p(mem, C.c_int64)), (cnt, goff, mem), "link_groups_us", keep

    plan = [("score_stats_axis0", stats, (0, "plain", False)), ("score_stats_axis0_masks", stats, (0, "masks", False)), ("score_stats_axis1", stats, (1, "plain", False)),
            ("score_stats_axis1_masks", stats, (1, "masks", False)), ("subject_score_stats_axis0_masks", stats, (0, "masks", True)), ("subject_score_stats_axis1_masks", stats, (1, "masks", True)),
            ("score_histogram_axis0_256", hist, (0, 256, False)), ("score_histogram_axis1_16", hist, (1, 16, False)), ("subject_score_histogram_axis0_256", hist, (0, 256, True)),
            ("subject_score_histogram_axis1_16", hist, (1, 16, True)), ("entries_at_64", at, (False,)), ("subject_entries_at_64", at, (True,)),
            ("rank_positions_10", pos, ("templates", "plain")), ("rank_positions_10_filtered", pos, ("templates", "masks + exclusions")), ("count_before_10", pos, ("count", "plain")),
            ("count_before_10_filtered", pos, ("count", "masks + exclusions")), ("rank_subject_positions_10_filtered", pos, ("persons", "masks + exclusions")),
            ("rank_hits_filtered_cap100", hits, (False,)), ("rank_subject_hits_filtered_cap100", hits, (True,)), ("link_groups_any", link, (False,)), ("link_subject_groups_any", link, (True,))]
    rows = {}
    for label, make, args in plan:
        calls = {name: make(m, hl, hj, *args) for name, (m, hl, hj) in libs.items()}
        us = {name: [] for name in libs}; ms = {name: [] for name in libs}
        for rep in range(a.reps + 1):
            for name, (m, _, _) in libs.items():
                call, _, option, _ = calls[name]
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
    out["every_byte_equal"] = bool(all(r["equal_bytes"] for r in rows.values()))
    for m, hl, hj in libs.values():
        m.labels_free(hl); m.subjects_free(hj); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
