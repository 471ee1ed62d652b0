#!/usr/bin/env python
"""What scoring only the eligible pairs saves (afis_search_eligible), on one MI355X with the headline's synthetic gallery and latents (committed as bench.py commits
them): 100 latents x 100 000 templates by default.  The yardstick is afis_search on the same context in the same run — the only route to the same lists before this
call existed: a full search, then the _filtered ranking calls.  The two are interleaved, `--reps` + 1 times each, the first pair discarded; medians with the spread
(max - min) beside them.  Both clocks are recorded: the HOST's (perf_counter around the call: latents uploaded, searched, nothing copied back) and the library's
total_ms (HIP events: the launch groups of the searches the call ran — for the eligible call neither the sub-shards' gathers nor the expand passes).

Two mask sets over cards of ten one-hot fingers and two sex bits:
  few classes     four kinds of mask dealt over the latents in turn — all pass, one hand, one finger, two fingers of one sex: four classes
  one per latent  the masks of tools/filtered_hits_timing.py: one to three finger positions and one sex per latent, about a tenth of
                  the cells eligible and nearly every latent a class of its own — the worst case: one sub-shard and one launch sequence per latent

Per set: pairs scored against the full search's, option eligible_classes, option eligible_expand_us, and whether rank_hits(-inf, cap) on the eligible matrix equals
rank_hits_filtered(-inf, cap) with the same labels and masks after the full search.  Recorded, not asserted.  One JSON document on stdout and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
U64 = np.uint64


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def same(a, b):
    return bool(all(np.array_equal(np.asarray(a[k]).view(np.uint32) if a[k].dtype == np.float32 else a[k], np.asarray(b[k]).view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eligible_search_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G, cap = a.queries, a.gallery, a.cap
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats, G=G)
    rng = np.random.default_rng(a.seed)
    m = M.Matcher(cbb)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    glob = np.arange(G, dtype=np.int64)
    card = glob // 10
    sex = rng.integers(0, 2, card.max() + 1)[card]
    labels = (U64(1) << (glob % 10).astype(U64)) | (U64(1) << (10 + sex).astype(U64))
    per_latent = np.zeros((Q, 3), U64)
    for q in range(Q):                                                      # as tools/filtered_hits_timing.py: one to three finger positions and one sex allowed
        allowed = sum(1 << int(f) for f in rng.choice(10, int(rng.integers(1, 4)), replace=False)) | (1 << (10 + int(rng.integers(0, 2))))
        per_latent[q, 2] = U64(0xfff & ~allowed)
    kinds = [(0, 0, 0), (0x1F, 0, 0), (1 << 3, 0, 0), (0, 0, 0xfff & ~((1 << 2) | (1 << 7) | (1 << 10)))]     # all pass, one hand, one finger, two fingers of one sex
    few = np.array([kinds[q % 4] for q in range(Q)], U64)
    hl = m.labels_create(labels)
    out = {"queries": Q, "templates": G, "cap": cap, "reps": a.reps, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "clocks": {"host_ms": "perf_counter around the call (upload of the latents, search, no scores copied back)",
                      "total_ms": "afis_timing.total_ms: HIP events around the launch groups, summed over the searches the call ran",
                      "eligible_expand_us": "HIP events around each expand launch, summed over the classes"},
           "mask_sets": {}}
    ninf = float("-inf")
    for name, masks in (("few classes", few), ("one class per latent (row 11's masks)", per_latent)):
        L = labels[None, :]
        ok = ((masks[:, 0:1] == 0) | ((L & masks[:, 0:1]) != 0)) & ((L & masks[:, 1:2]) == masks[:, 1:2]) & ((L & masks[:, 2:3]) == 0)
        t = {"eligible": {"host_ms": [], "total_ms": [], "expand_us": []}, "full": {"host_ms": [], "total_ms": []}}
        pairs = classes = full_pairs = None
        lists_equal = True
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            m.search_eligible(lats, hl, masks, want_scores=False)
            dt = (time.perf_counter() - t0) * 1e3
            tm = m.timing()
            pairs, classes = tm["pairs"], m.get_option("eligible_classes")
            if rep:
                t["eligible"]["host_ms"].append(dt); t["eligible"]["total_ms"].append(tm["total_ms"]); t["eligible"]["expand_us"].append(m.get_option("eligible_expand_us"))
            got = m.rank_hits(ninf, cap)
            t0 = time.perf_counter()
            m.search(lats, k=0, want_scores=False)
            dt = (time.perf_counter() - t0) * 1e3
            tm = m.timing()
            full_pairs = tm["pairs"]
            if rep:
                t["full"]["host_ms"].append(dt); t["full"]["total_ms"].append(tm["total_ms"])
            lists_equal = lists_equal and same(got, m.rank_hits_filtered(ninf, cap, labels=hl, masks=masks))
        row = {"eligible_fraction": round(float(ok.mean()), 4), "classes": classes, "pairs_scored": pairs, "pairs_of_the_full_search": full_pairs,
               "pair_ratio": round(pairs / full_pairs, 4), "pairs_equal_the_eligible_cells": bool(pairs == int(ok.sum())),
               "afis_search_eligible": {k: med(v) for k, v in t["eligible"].items()}, "afis_search": {k: med(v) for k, v in t["full"].items()},
               "lists_equal_the_filtered_route": lists_equal}
        row["host_time_ratio"] = round(row["afis_search_eligible"]["host_ms"]["median"] / row["afis_search"]["host_ms"]["median"], 4)
        row["total_ms_ratio"] = round(row["afis_search_eligible"]["total_ms"]["median"] / row["afis_search"]["total_ms"]["median"], 4)
        out["mask_sets"][name] = row
    m.labels_free(hl); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
