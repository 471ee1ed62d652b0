#!/usr/bin/env python
"""What a subset search costs (afis_subset_create / afis_search_subset_resident), on one MI355X with the headline's synthetic gallery and latents.  For every subset size:

  create   afis_subset_create's wall time and the device time of its gather launches (option subset_gather_us: HIP events around them), beside the only way to the same
           search without subsets: a second context that stages those templates from the host (afis_gallery_add_packed) and commits them, timed in the same run.
           Picking the templates out of the host copy of the gallery (numpy) is the caller's database work and is timed apart.
  step     the search step on the subset beside the step on that freshly committed context, which holds exactly those templates in the same (ascending) order: the
           same kernels over the same bytes.  The steps are interleaved (subset, fresh, fresh with the subset handle's launch-group size, subset, ...), the first
           round is a warm-up and is reported but kept out of the medians; `spread` is max - min of one kind's kept steps, to set the difference against.  A query
           handle's launch groups are cut for the whole shard, so a subset search may run more, smaller groups than the fresh context does by default: the third
           kind gives the fresh context the whole shard's group size (option query_batch), hence the same cuts.
  full     the full-shard step for the same latents, for scale.

Wall times are host clocks around calls that return with the device idle; device_ms is afis_timing.total_ms (HIP events on the context's stream).  One process, one
device.  One JSON document on stdout (and to --out)."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def timed(fn):
    t0 = time.perf_counter(); r = fn(); return (time.perf_counter() - t0) * 1e3, r


def pick(pg, idx):
    """The listed templates of a packed gallery as a packed gallery (in the order listed)."""
    nm, nt = np.diff(pg.minu_off)[idx], np.diff(pg.tex_off)[idx]
    mrows = np.concatenate([np.arange(pg.minu_off[g], pg.minu_off[g + 1]) for g in idx]) if len(idx) else np.zeros(0, np.int64)
    trows = np.concatenate([np.arange(pg.tex_off[g], pg.tex_off[g + 1]) for g in idx]) if len(idx) else np.zeros(0, np.int64)
    return S.PackedGallery(np.concatenate([[0], np.cumsum(nm)]).astype(np.int64), pg.minu_x[mrows], pg.minu_y[mrows], pg.minu_ori[mrows], pg.minu_des[mrows],
                           np.concatenate([[0], np.cumsum(nt)]).astype(np.int64), pg.tex_x[trows], pg.tex_y[trows], pg.tex_ori[trows], pg.tex_codes[trows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--sizes", default="1000,10000,50000")
    ap.add_argument("--reps", type=int, default=3, help="repetitions of create / second context (the first is reported, not in the medians)")
    ap.add_argument("--steps", type=int, default=3, help="kept search steps per kind (one more is run first as warm-up)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    G = a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    t0 = time.perf_counter()
    lats = S.make_latents(a.seed, a.queries)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats, G=G)
    out = {"gallery": G, "queries": a.queries, "generation_s": round(time.perf_counter() - t0, 1), "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12]}
    m = M.Matcher(cbb)
    out["device"] = m.device_info(0)
    m.gallery_add_packed(gal)
    out["full_commit_ms"] = round(timed(lambda: m.gallery_commit(0))[0], 1)
    qh = m.upload_queries(lats)
    med = statistics.median
    spread = lambda v: round(max(v) - min(v), 2)

    # ---- (c) the full-shard step, for scale ----
    full_wall, full_dev = [], []
    full = None
    for step in range(a.steps + 1):
        ms, full = timed(lambda: m.search_resident(qh, k=24))
        tm = m.timing()
        if step:
            full_wall.append(round(ms, 2)); full_dev.append(round(tm["total_ms"], 2))
    out["full"] = {"step_wall_ms": full_wall, "step_device_ms": full_dev, "median_wall_ms": med(full_wall), "spread_wall_ms": spread(full_wall),
                   "launch_groups": tm["launch_groups"], "overlapped_groups": tm["overlapped_groups"], "pairs": tm["pairs"]}
    # latents per launch group at most, as the library sets it for the WHOLE shard when option query_batch is 0 (afis_device.h::launch_group_latents): given to the
    # third kind's context, whose own default would follow its smaller gallery, it makes afis_queries_upload place the same cuts there
    per_group = min(128, max(10, (5000000 + G // 2) // G))

    rng = np.random.default_rng(a.seed + 2)
    out["subsets"] = []
    for n in [int(x) for x in a.sizes.split(",") if x]:
        idx = np.sort(rng.permutation(G)[:n]).astype(np.int64)
        pick_ms, sub_pg = timed(lambda: pick(gal, idx))
        row = {"n": n, "host_pick_ms": round(pick_ms, 1)}
        # ---- (a) create against a second context staged from the host ----
        reps = []
        h = m2 = None
        for rep in range(a.reps):
            if h is not None:
                m.subset_free(h); m2.close()
            h2d0 = m.get_option("gallery_h2d_bytes")
            create_ms, h = timed(lambda: m.subset_create(idx))
            m2 = M.Matcher(cbb)
            stage_ms, _ = timed(lambda: m2.gallery_add_packed(sub_pg))
            commit_ms, _ = timed(lambda: m2.gallery_commit(0))
            reps.append({"rep": rep, "subset_create_ms": round(create_ms, 2), "gather_launches_us": m.get_option("subset_gather_us"), "subset_h2d_bytes": m.get_option("gallery_h2d_bytes") - h2d0,
                         "second_context_stage_ms": round(stage_ms, 1), "second_context_commit_ms": round(commit_ms, 1), "second_context_h2d_bytes": m2.get_option("gallery_h2d_bytes")})
        kept = reps[1:] if len(reps) > 1 else reps
        cm = med([r["subset_create_ms"] for r in kept]); sm = med([r["second_context_stage_ms"] + r["second_context_commit_ms"] for r in kept])
        row["create"] = {"reps": reps, "median_subset_create_ms": cm, "median_gather_launches_us": med([r["gather_launches_us"] for r in kept]),
                         "median_second_context_ms": round(sm, 1), "second_context_over_subset_create": round(sm / cm, 1), "subset_device_bytes": m.get_option("subset_device_bytes")}
        # ---- (b) the step on the subset against the step on the fresh context ----
        m3 = M.Matcher(cbb); m3.set_option("query_batch", per_group)       # the fresh context with the subset handle's launch-group size
        m3.gallery_add_packed(sub_pg); m3.gallery_commit(0)
        q2, q3 = m2.upload_queries(lats), m3.upload_queries(lats)
        kinds = {"subset": lambda: m.search_subset_resident(h, qh, k=24), "fresh": lambda: m2.search_resident(q2, k=24), "fresh_same_groups": lambda: m3.search_resident(q3, k=24)}
        owner = {"subset": m, "fresh": m2, "fresh_same_groups": m3}
        wall = {k: [] for k in kinds}; dev = {k: [] for k in kinds}; groups = {}; last = {}
        for step in range(a.steps + 1):
            for kind, fn in kinds.items():
                ms, last[kind] = timed(fn)
                tm = owner[kind].timing()
                groups[kind] = (tm["launch_groups"], tm["overlapped_groups"], tm["pairs"])
                if step:
                    wall[kind].append(round(ms, 2)); dev[kind].append(round(tm["total_ms"], 2))
        same = all(np.array_equal(last["subset"]["topk_score"].view(np.uint32), last[k]["topk_score"].view(np.uint32)) and
                   np.array_equal(last["subset"]["topk_idx"], idx[last[k]["topk_idx"]]) for k in ("fresh", "fresh_same_groups"))
        cols = full["topk_idx"][:, 0]                                       # (the full search's best entry, where it is listed, must lead the subset's list)
        row["step"] = {k: {"wall_ms": wall[k], "device_ms": dev[k], "median_wall_ms": med(wall[k]), "median_device_ms": med(dev[k]), "spread_wall_ms": spread(wall[k]),
                           "launch_groups": groups[k][0], "overlapped_groups": groups[k][1], "pairs": groups[k][2]} for k in kinds}
        row["step"]["subset_minus_fresh_wall_ms"] = round(med(wall["subset"]) - med(wall["fresh"]), 2)
        row["step"]["subset_minus_fresh_same_groups_wall_ms"] = round(med(wall["subset"]) - med(wall["fresh_same_groups"]), 2)
        row["step"]["rank_lists_identical_to_fresh"] = bool(same)
        row["step"]["full_best_leads_where_listed"] = bool(all(int(last["subset"]["topk_idx"][q, 0]) == int(cols[q]) for q in range(a.queries) if int(cols[q]) in set(idx.tolist())))
        row["step"]["full_over_subset"] = round(out["full"]["median_wall_ms"] / med(wall["subset"]), 1)
        m2.free_queries(q2); m3.free_queries(q3); m2.close(); m3.close(); m.subset_free(h)
        out["subsets"].append(row)
    m.free_queries(qh); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
