#!/usr/bin/env python
"""What cohort statistics and the z-normalisation cost (afis_score_stats, afis_normalize_scores), on one MI355X, on a planted matrix of 100 latents x 100 000 templates
by default: cells uniform in [0, 300) with 5 % of -1, uploaded with the parity tap afis_debug_rank_hits over a packed gallery of one-point templates.  In one process,
on the same matrix, every call below is made `--reps` + 1 times, the first discarded; medians with the spread (max - min) beside them:

  score_stats_us     axis 0 and axis 1, without a filter and with masks (per query one none_of mask over a finger / sex label: tools/filtered_hits_timing.py's)
  normalize_us       axis 0 and axis 1 (the matrix is planted again before every call: a normalised matrix is refused)
  rank_filtered_us   afis_rank_hits_filtered(-inf, cap 1) with the same masks: it reads the matrix through the same filter pass and once more — the yardstick of a
                     filtered statistics call; filter_us beside it
  rank_hits_us       afis_rank_hits(-inf, cap 1): one read of the matrix — the yardstick of a normalisation (one read, one write)

Clocks: DEVICE only (HIP events inside the library).  Each call is also given as bytes per second over what it must move (the matrix once for statistics, twice for a
normalisation; a filtered call three times).  Every answer is checked against numpy on one row and one column.  Recorded, not asserted.  One JSON document on stdout
and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
U64 = np.uint64


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def check(stat, cells):
    valued = np.isfinite(cells) & ~np.signbit(cells + np.float32(0)) & (cells < 65536)
    q = [int(t) for t in np.rint(cells[valued].astype(np.float64) * 2 ** 20).astype(np.int64)]
    s2 = (int(stat["s2_hi"]) << 64) | int(stat["s2_lo"])
    assert (int(stat["n"]), int(stat["n_outside"]), int(stat["s1"]), s2) == (len(q), int((~valued).sum()), sum(q), sum(t * t for t in q)), "a statistic differs from numpy"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_stats_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, G = a.queries, a.gallery
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    rng = np.random.default_rng(a.seed)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    gal = S.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
                          off.copy(), rng.integers(0, 30, G).astype(np.int16), rng.integers(0, 30, G).astype(np.int16), rng.uniform(-1.5, 1.5, G).astype(np.float32),
                          rng.integers(0, cb.K, (G, cb.M)).astype(np.uint8))
    scores = np.where(rng.random((Q, G)) < 0.05, -1.0, rng.uniform(0, 300, (Q, G))).astype(np.float32)
    m = M.Matcher(cbb, taps=True)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    ninf = float("-inf")
    plant = lambda: m.debug_rank_hits(None, scores, ninf, 1)
    glob = np.arange(G, dtype=np.int64)
    card = glob // 10
    sex = rng.integers(0, 2, card.max() + 1)[card]
    labels = (U64(1) << (glob % 10).astype(U64)) | (U64(1) << (10 + sex).astype(U64))
    masks = np.zeros((Q, 3), U64)
    for q in range(Q):                                                      # one to three finger positions and one sex allowed: the complement inside the two fields
        allowed = sum(1 << int(f) for f in rng.choice(10, int(rng.integers(1, 4)), replace=False)) | (1 << (10 + int(rng.integers(0, 2))))
        masks[q, 2] = U64(0xfff & ~allowed)
    plant()
    hl = m.labels_create(labels)
    flt = dict(labels=hl, masks=masks)
    mb = scores.nbytes
    out = {"queries": Q, "gallery": G, "reps": a.reps, "matrix_bytes": int(mb), "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "eligible_fraction": round(float(((labels[None, :] & masks[:, 2:3]) == 0).mean()), 4), "clocks": "device: HIP events inside the library"}
    st0 = m.score_stats(axis=0); st1 = m.score_stats(axis=1)
    check(st0[Q // 2], scores[Q // 2]); check(st1[G // 3], scores[:, G // 3])
    mean, sd = m.score_moments(st0)
    mean1, sd1 = m.score_moments(st1)
    cases = [("score_stats_axis0", ["score_stats_us"], lambda: m.score_stats(axis=0), False, 1), ("score_stats_axis1", ["score_stats_us"], lambda: m.score_stats(axis=1), False, 1),
             ("score_stats_axis0_masks", ["score_stats_us"], lambda: m.score_stats(axis=0, **flt), False, 3), ("score_stats_axis1_masks", ["score_stats_us"], lambda: m.score_stats(axis=1, **flt), False, 3),
             ("rank_hits_filtered_masks", ["rank_filtered_us", "filter_us"], lambda: m.rank_hits_filtered(ninf, 1, **flt), False, 3),
             ("rank_hits", ["rank_hits_us"], lambda: m.rank_hits(ninf, 1), False, 1),
             ("normalize_axis0", ["normalize_us"], lambda: m.normalize_scores(mean, 1.0 / sd, axis=0), True, 2),
             ("normalize_axis1", ["normalize_us"], lambda: m.normalize_scores(mean1, 1.0 / sd1, axis=1), True, 2)]
    for name, opts, call, replant, moves in cases:
        seen = {o: [] for o in opts}
        for rep in range(a.reps + 1):
            if replant:
                plant()
            call()
            if rep:
                for o in opts:
                    seen[o].append(m.get_option(o))
        row = {o: med(v) for o, v in seen.items()}
        row["matrix_passes"] = moves
        row["gb_per_s"] = round(moves * mb / (statistics.median(seen[opts[0]]) * 1e-6) / 1e9, 1)
        out[name] = row
    m.labels_free(hl)
    m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
