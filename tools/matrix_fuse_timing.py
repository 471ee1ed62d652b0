#!/usr/bin/env python
"""What the kept matrices cost (afis_matrix_keep, afis_matrix_fuse), on one MI355X, on planted matrices uploaded with the parity tap afis_debug_rank_hits over a
packed gallery of one-point templates.  Cells are uniform in [0, 1) with a tenth at -1 and a tenth no entry.  tools/print_search_timing.py's method: every case is
run in every round, the rounds interleave the cases, `--reps` + 1 rounds with the first discarded; medians with the spread (max - min) beside them.  All times are
device times from HIP events inside the library.

  matrix_keep_us          100 x 100 000: one device-to-device copy; bytes = 2 x the matrix
  matrix_fuse_us          100 x 100 000 with 2 and with 4 operands, AFIS_FUSE_SUM (weights given) and AFIS_FUSE_MAX; bytes = (n + 1) x the matrix
  case_fuse_us            the yardstick of the same traffic: afis_rank_case_hits folding the same number of rows of one planted matrix — 200 (400) rows in cases of
                          2 (4) members, AFIS_CASE_SUM and AFIS_CASE_MAX —, everything of that call before k_rank_hits; and the ratio of the times per byte
  matrix_fuse_us, square  4096 x 4096, (A, A) with the second operand transposed, AFIS_FUSE_MIN: k_transpose_scores (2 x the matrix) + k_matrix_fuse (3 x)

Every fused matrix is checked against tests/matrix_model.py once.  Recorded, not asserted.  One JSON document on stdout and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
import matrix_model as MM  # noqa: E402

NINF = float("-inf")


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def rate(n_bytes, us):
    return round(n_bytes / (us * 1e-6) / 1e9, 1) if us > 0 else None


def matcher(cbb, cb, G, seed):
    rng = np.random.default_rng(seed)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    gal = S.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
                          off.copy(), rng.integers(0, 30, G).astype(np.int16), rng.integers(0, 30, G).astype(np.int16), rng.uniform(-1.5, 1.5, G).astype(np.float32),
                          rng.integers(0, cb.K, (G, cb.M)).astype(np.uint8))
    m = M.Matcher(cbb, taps=True)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    return m


def cells(rng, shape):
    x = rng.random(shape, dtype=np.float32)
    r = rng.random(shape)
    x[r < 0.1] = np.float32(-1.0)
    x[r > 0.9] = MM.NO_ENTRY.view(np.float32)
    return x


def same(got, want):
    return bool(np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--square", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5, help="kept rounds (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_fuse_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    G, Q = a.gallery, a.queries
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    rng = np.random.default_rng(a.seed)
    m = matcher(cbb, cb, G, a.seed)
    out = {"gallery": G, "queries": Q, "reps": a.reps, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": m.device_info(0),
           "clocks": "device: HIP events inside the library"}
    one = Q * G * 4
    ops = [cells(rng, (Q, G)) for _ in range(4)]
    hs = []
    for x in ops:
        m.debug_rank_hits(None, x, NINF, 1)
        hs.append(m.matrix_keep())
    w4 = [0.4, 0.3, 0.2, 0.1]
    res = {"matrix_bytes": one}
    # the fused matrices against the model, once
    res["checked_against_the_model"] = all([
        same(m.matrix_fuse(hs[:2], MM.SUM, weights=w4[:2], want_scores=True), MM.fuse(ops[:2], MM.SUM, False, w4[:2])),
        same(m.matrix_fuse(hs, MM.SUM, weights=w4, want_scores=True), MM.fuse(ops, MM.SUM, False, w4)),
        same(m.matrix_fuse(hs[:2], MM.MAX, want_scores=True), MM.fuse(ops[:2], MM.MAX, False)),
        same(m.matrix_fuse(hs, MM.MAX, want_scores=True), MM.fuse(ops, MM.MAX, False))])
    seen = {}

    def take(name, opt):
        seen.setdefault(name, []).append(m.get_option(opt))

    stacked = {n: np.ascontiguousarray(np.stack(ops[:n], axis=1).reshape(n * Q, G)) for n in (2, 4)}   # rows q*n + k: case q's member k is operand k's row q
    for rep in range(a.reps + 1):
        m.debug_rank_hits(None, ops[0], NINF, 1)
        h = m.matrix_keep()
        if rep:
            take("keep", "matrix_keep_us")
        m.matrix_free(h)
        for n in (2, 4):
            m.matrix_fuse(hs[:n], MM.SUM, weights=w4[:n])
            if rep:
                take("fuse_sum_%d" % n, "matrix_fuse_us")
            m.matrix_fuse(hs[:n], MM.MAX)
            if rep:
                take("fuse_max_%d" % n, "matrix_fuse_us")
            m.debug_rank_hits(None, stacked[n], NINF, 1)
            for cmode, cname in ((0, "sum"), (1, "max")):
                m.rank_case_hits(np.arange(n * Q) // n, cmode, 2.0, 1)
                if rep:
                    take("case_%s_%d" % (cname, n), "case_fuse_us")
        note("round", rep, "done")
    res["keep"] = {"matrix_keep_us": med(seen["keep"]), "bytes": 2 * one, "GB_per_s": rate(2 * one, statistics.median(seen["keep"]))}
    for n in (2, 4):
        nbytes = (n + 1) * one
        for op in ("sum", "max"):
            f, c = statistics.median(seen["fuse_%s_%d" % (op, n)]), statistics.median(seen["case_%s_%d" % (op, n)])
            res["fuse_%s_%d" % (op, n)] = {"matrix_fuse_us": med(seen["fuse_%s_%d" % (op, n)]), "bytes": nbytes, "GB_per_s": rate(nbytes, f),
                                          "case_fuse_us": med(seen["case_%s_%d" % (op, n)]), "case_GB_per_s": rate(nbytes, c),
                                          "time_per_byte_over_case_fuse": round(f / c, 2) if c > 0 else None}
    out["rows_%d" % Q] = res
    for h in hs:
        m.matrix_free(h)
    m.close()
    # the square matrix with one transposed operand
    n = a.square
    m = matcher(cbb, cb, n, a.seed + 1)
    x = cells(rng, (n, n))
    m.debug_rank_hits(None, x, NINF, 1)
    h = m.matrix_keep()
    sq = {"matrix_bytes": n * n * 4, "checked_against_the_model": same(m.matrix_fuse([h, h], MM.MIN, transposed=[0, 1], want_scores=True), MM.fuse([x, np.ascontiguousarray(x.T)], MM.MIN, False))}
    t, u = [], []
    for rep in range(a.reps + 1):
        m.matrix_fuse([h, h], MM.MIN, transposed=[0, 1])
        if rep:
            t.append(m.get_option("matrix_fuse_us"))
        m.matrix_fuse([h, h], MM.MIN)
        if rep:
            u.append(m.get_option("matrix_fuse_us"))
    sq["fuse_min_A_At"] = {"matrix_fuse_us": med(t), "bytes": 5 * n * n * 4, "GB_per_s": rate(5 * n * n * 4, statistics.median(t))}
    sq["fuse_min_A_A"] = {"matrix_fuse_us": med(u), "bytes": 3 * n * n * 4, "GB_per_s": rate(3 * n * n * 4, statistics.median(u))}
    out["square_%d" % n] = sq
    m.matrix_free(h)
    m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
