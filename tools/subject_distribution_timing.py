#!/usr/bin/env python
"""What the person distributions cost (afis_subject_score_stats, afis_subject_score_histogram, afis_subject_entries_at), on one MI355X, on a planted matrix of 100
latents x 100 000 templates by default — cells uniform in [0, 300) with 5 % of -1 —, uploaded with the parity tap afis_debug_rank_hits over a packed gallery of
one-point templates.  Two subject handles: TEN — 10 000 persons of ten consecutive templates, the ten-print card — and IDENTITY — every template a person of its own, the
most slots a handle can have.  Every person call stands beside the yardsticks that already exist, in the same process on the same matrix:

  rank_hits_us          afis_rank_subject_hits at cap 1 with the same handle: the fold (the maxima's memset and k_subject_best) plus one rank pass
  score_stats_us, score_histogram_us, entries_at_us   the template forms over the [n_q][G] matrix

The expectation to judge a person call against: the fold + the key pass + the template form's pass over S columns instead of G.
The cases are interleaved: `--reps` + 1 rounds, each running every case once, the first round discarded; medians with the spread (max - min) beside them.
Clocks: DEVICE only (HIP events inside the library).  Every person answer is checked against numpy on one row.  Recorded, not asserted.  One JSON document on stdout
and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def even_edges(bins):
    """bins - 1 edges: bin 0 lies below 0.0 (the -1 cells), the others split [0, 300) evenly; what reaches 300 falls into the last."""
    return np.linspace(0.0, 300.0, bins - 1, endpoint=False).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--card", type=int, default=10, help="templates per person of the TEN handle")
    ap.add_argument("--reps", type=int, default=5, help="kept rounds (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subject_distribution_timing.json"), help="where the JSON document goes ('' = stdout only)")
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
    m.debug_rank_hits(None, scores, ninf, 1)
    handles = {"ten": m.subjects_create(np.arange(G, dtype=np.int64) // a.card), "identity": m.subjects_create(np.arange(G, dtype=np.int64))}
    out = {"queries": Q, "gallery": G, "card": a.card, "reps": a.reps, "matrix_bytes": int(scores.nbytes), "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "device": m.device_info(0), "clocks": "device: HIP events inside the library", "cases": "interleaved: every round runs every case once"}
    row = Q // 2
    e256, e16 = even_edges(256), even_edges(16)
    cases = [("templates", "score_stats_axis0", "score_stats_us", lambda: m.score_stats(axis=0)), ("templates", "histogram_256_bins", "score_histogram_us", lambda: m.score_histogram(e256)),
             ("templates", "histogram_16_bins_axis1", "score_histogram_us", lambda: m.score_histogram(e16, axis=1))]
    for n in (1, 64):
        q = np.repeat(np.arange(Q, dtype=np.int32), n); r = rng.integers(0, G, Q * n).astype(np.int64)
        cases.append(("templates", "entries_at_%d_per_row" % n, "entries_at_us", (lambda q, r: lambda: m.entries_at(q, r))(q, r)))
    for name, h in handles.items():
        n_s = len(h[2])
        # the model on one row: a person's best is the maximum of the row over the person's templates (no NaN, no -0.0: float order is the order of the words)
        best = np.maximum.reduceat(scores[row], np.flatnonzero(np.r_[True, h[3][1:] != h[3][:-1]]))
        assert np.array_equal(m.subject_score_histogram(h, e256)[row], np.bincount(np.searchsorted(e256, best, side="right"), minlength=256)), "a person histogram differs from numpy"
        order = np.lexsort((np.arange(n_s), -best.astype(np.float64)))
        st = m.subject_score_stats(h, axis=0)[row]
        qv = np.rint(best[best >= 0].astype(np.float64) * 2 ** 20).astype(np.int64)
        assert int(st["n"]) == len(qv) and int(st["s1"]) == int(qv.sum()) and int(st["n_outside"]) == int((best < 0).sum()), "a person statistic differs from numpy"
        cases += [(name, "rank_subject_hits_cap_1", "rank_hits_us", (lambda h: lambda: m.rank_subject_hits(h, ninf, 1))(h)),
                  (name, "subject_score_stats_axis0", "subject_score_stats_us", (lambda h: lambda: m.subject_score_stats(h, axis=0))(h)),
                  (name, "subject_score_stats_axis1", "subject_score_stats_us", (lambda h: lambda: m.subject_score_stats(h, axis=1))(h)),
                  (name, "subject_histogram_256_bins", "subject_score_histogram_us", (lambda h: lambda: m.subject_score_histogram(h, e256))(h)),
                  (name, "subject_histogram_16_bins_axis1", "subject_score_histogram_us", (lambda h: lambda: m.subject_score_histogram(h, e16, axis=1))(h))]
        for n in (1, 64):
            q = np.repeat(np.arange(Q, dtype=np.int32), n); r = rng.integers(0, n_s, Q * n).astype(np.int64)
            got = m.subject_entries_at(h, q, r)
            at = q == row
            assert np.array_equal(got["subject"][at], h[2][order[r[at]]]) and np.array_equal(got["score"][at], best[order[r[at]]]), "a person entry differs from numpy"
            cases.append((name, "subject_entries_at_%d_per_row" % n, "subject_entries_at_us", (lambda h, q, r: lambda: m.subject_entries_at(h, q, r))(h, q, r)))
    seen = {(grp, name): [] for grp, name, _, _ in cases}
    for rnd in range(a.reps + 1):
        for grp, name, opt, call in cases:
            call()
            if rnd:
                seen[(grp, name)].append(m.get_option(opt))
    for grp, name, opt, _ in cases:
        out.setdefault(grp, {})[name] = {opt: med(seen[(grp, name)])}
    # a person call beside the sum of its two yardsticks: the fold with one rank pass, and the template form over G columns
    pairs = {"subject_score_stats_axis0": "score_stats_axis0", "subject_histogram_256_bins": "histogram_256_bins", "subject_histogram_16_bins_axis1": "histogram_16_bins_axis1",
             "subject_entries_at_1_per_row": "entries_at_1_per_row", "subject_entries_at_64_per_row": "entries_at_64_per_row"}
    for name in handles:
        fold = out[name]["rank_subject_hits_cap_1"]["rank_hits_us"]["median"]
        beside = {}
        for person, template in pairs.items():
            p = next(iter(out[name][person].values()))["median"]; t = next(iter(out["templates"][template].values()))["median"]
            beside[person] = {"person_us": p, "fold_plus_rank_us": fold, "template_form_us": t, "person_over_sum": round(p / (fold + t), 2)}
        out[name]["beside_the_yardsticks"] = beside
    m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
