#!/usr/bin/env python
"""What the score distributions cost (afis_score_histogram, afis_entries_at), on one MI355X, on a planted matrix of 100 latents x 100 000 templates by default, uploaded
with the parity tap afis_debug_rank_hits over a packed gallery of one-point templates.  Two matrices: RANDOM — cells uniform in [0, 300) with 5 % of -1 — and ONE BIN —
every cell 0.0, the shape of a real non-mate row at its extreme: every cell of a wave goes to the same LDS word, which is what the kernels' wave aggregation is for.
In one process every call below is made `--reps` + 1 times, the first discarded; medians with the spread (max - min) beside them:

  score_histogram_us   axis 0 at 16, 256 and 1024 bins (edges evenly spaced over [0, 300)), on both matrices; axis 1 at 16 bins on the random one
  entries_at_us        1 and 64 random ranks per row, on both matrices
  score_stats_us       afis_score_stats axis 0 on the same matrix in the same process: the reference point — it also reads every word once

Clocks: DEVICE only (HIP events inside the library).  The histogram is also given as bytes per second over the matrix read once.  Every answer is checked against numpy
on one row.  Recorded, not asserted.  One JSON document on stdout and in --out."""
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
    ap.add_argument("--reps", type=int, default=5, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_distribution_timing.json"), help="where the JSON document goes ('' = stdout only)")
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
    matrices = {"random": np.where(rng.random((Q, G)) < 0.05, -1.0, rng.uniform(0, 300, (Q, G))).astype(np.float32), "one_bin": np.zeros((Q, G), np.float32)}
    m = M.Matcher(cbb, taps=True)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    ninf = float("-inf")
    mb = matrices["random"].nbytes
    out = {"queries": Q, "gallery": G, "reps": a.reps, "matrix_bytes": int(mb), "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "clocks": "device: HIP events inside the library"}
    row = Q // 2
    for kind, scores in matrices.items():
        m.debug_rank_hits(None, scores, ninf, 1)
        order = np.lexsort((np.arange(G), -scores[row].astype(np.float64)))   # (no NaN, and the two zeros do not meet: float order is key order here)
        cases = []
        for bins in (16, 256, 1024):
            edges = even_edges(bins)
            want = np.bincount(np.searchsorted(edges, scores[row], side="right"), minlength=bins)
            got = m.score_histogram(edges)
            assert np.array_equal(got[row], want), "a histogram differs from numpy"
            cases.append(("histogram_%d_bins" % bins, "score_histogram_us", (lambda e: lambda: m.score_histogram(e))(edges), 1))
        if kind == "random":
            e16 = even_edges(16)
            cases.append(("histogram_16_bins_axis1", "score_histogram_us", lambda: m.score_histogram(e16, axis=1), 1))
        for per_row in (1, 64):
            query = np.repeat(np.arange(Q, dtype=np.int32), per_row); rank = rng.integers(0, G, Q * per_row).astype(np.int64)
            got = m.entries_at(query, rank)
            at = query == row
            assert np.array_equal(got["idx"][at], order[rank[at]]) and np.array_equal(got["score"][at], scores[row][order[rank[at]]]), "an entry differs from numpy"
            cases.append(("entries_at_%d_per_row" % per_row, "entries_at_us", (lambda q, r: lambda: m.entries_at(q, r))(query, rank), None))
        cases.append(("score_stats_axis0", "score_stats_us", lambda: m.score_stats(axis=0), 1))
        res = {}
        for name, opt, call, moves in cases:
            seen = []
            for rep in range(a.reps + 1):
                call()
                if rep:
                    seen.append(m.get_option(opt))
            res[name] = {opt: med(seen)}
            if moves:
                res[name]["gb_per_s"] = round(moves * mb / (statistics.median(seen) * 1e-6) / 1e9, 1)
        out[kind] = res
    r16, o16 = out["random"]["histogram_16_bins"]["score_histogram_us"]["median"], out["one_bin"]["histogram_16_bins"]["score_histogram_us"]["median"]
    out["one_bin_over_random_16_bins"] = round(o16 / r16, 2)
    m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
