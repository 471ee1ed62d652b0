#!/usr/bin/env python
"""What a per-query filter costs at ranking time (afis_rank_hits_filtered / afis_rank_subject_hits_filtered), on one MI355X with the headline's synthetic gallery and
latents (committed as bench.py commits them).  Per gallery size — 100 000 and 10 000 templates by default, 100 latents — one search, then on the matrix it left on the
device every call below is made `--reps` + 1 times, the first discarded; medians with the spread (max - min) beside them:

  rank_hits(-inf, cap)                              the unfiltered list: the baseline of the same run, option rank_hits_us
  rank_hits_filtered, masks                         per query a set of finger positions and a sex, as ONE none_of over cards of ten one-hot fingers
  rank_hits_filtered, masks + exclusions            the same, and `--excluded` elimination prints per query
  rank_hits_filtered, exclusions alone              a device-to-device copy instead of the filter pass
  rank_subject_hits(-inf, cap) / ..._filtered       ten templates per subject; masks + excluded persons

Clocks: DEVICE only (HIP events inside the library): option rank_filtered_us around the call's launches and filter_us, from its own pair of events, around everything
before k_rank_hits.  The filter pass is reported as bytes per second over what it must move, n_q x G x 8 (4 B in, 4 B out per cell) + G x 8 x ceil(n_q / R) (a
column's label once per strip of R rows), set against the 6.3 TB/s a float4 copy reaches on this chip: where it stands, not a target (and with the caveat of
DESIGN section 7, row 10: the matrix was just written and 40 MB fit the last-level cache, so this is not an HBM figure).  The whole filtered call is set against
rank_hits_us of afis_rank_hits on the same matrix: the difference should be the filter pass and no more — k_rank_hits itself sees fewer qualifying entries.  Every
list is checked against numpy.  Recorded, not asserted.  One JSON document on stdout and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
COPY_TBS = 6.3                                                              # a float4 copy on this chip
R = 8                                                                       # csrc/afis_device.h: kFilterRows
U64 = np.uint64


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def lists(scores, names, ok, cap):
    """min_score = -inf over a search's scores (-1 or >= +0.0): the eligible cells, score descending, name ascending."""
    n = np.empty(len(scores), np.int64); a = np.full((len(scores), cap), -1, np.int64); sc = np.full((len(scores), cap), -np.inf, np.float32)
    for q, row in enumerate(scores):
        at = np.flatnonzero(ok[q])
        at = at[np.lexsort((names[at], -row[at].astype(np.float64)))][:cap]
        n[q] = int(ok[q].sum()); a[q, :len(at)] = names[at]; sc[q, :len(at)] = row[at]
    return n, a, sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--excluded", type=int, default=20, help="elimination prints (or persons) per query")
    ap.add_argument("--reps", type=int, default=5, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_hits_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    Q, cap = a.queries, a.cap
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, max(a.gallery), cb)
    S.plant_mates(a.seed, gal, cb, lats, G=min(a.gallery))
    rng = np.random.default_rng(a.seed)
    out = {"queries": Q, "cap": cap, "excluded_per_query": a.excluded, "strip_rows": R, "float4_copy_tb_per_s": COPY_TBS, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "clocks": {"rank_hits_us, rank_filtered_us, filter_us": "device: HIP events inside the library"}, "galleries": {}}
    for G in a.gallery:
        m = M.Matcher(cbb)
        out["device"] = m.device_info(0)
        m.gallery_add_packed(gal.slice(0, G) if G < gal.G else gal); m.gallery_commit(0)
        qh = m.upload_queries(lats)
        scores = m.search_resident(qh, k=0, want_scores=True)["scores"]
        m.free_queries(qh)                                                  # (leaves the matrix alone)
        glob = np.arange(G, dtype=np.int64)
        card = glob // 10
        sex = rng.integers(0, 2, card.max() + 1)[card]
        labels = (U64(1) << (glob % 10).astype(U64)) | (U64(1) << (10 + sex).astype(U64))
        masks = np.zeros((Q, 3), U64)
        for q in range(Q):                                                  # one to three finger positions and one sex allowed: the complement inside the two fields
            allowed = sum(1 << int(f) for f in rng.choice(10, int(rng.integers(1, 4)), replace=False)) | (1 << (10 + int(rng.integers(0, 2))))
            masks[q, 2] = U64(0xfff & ~allowed)
        excl = [rng.choice(G, a.excluded, replace=False).tolist() for _ in range(Q)]
        excl_s = [np.unique(card[e]).tolist() for e in excl]
        lt = ((labels[None, :] & masks[:, 2:3]) == 0)
        nl = np.ones((Q, G), bool); nls = np.ones((Q, G), bool)
        for q in range(Q):
            nl[q, excl[q]] = False; nls[q] = ~np.isin(card, excl_s[q])
        hl = m.labels_create(labels)
        hj = m.subjects_create(card)
        every = np.ones((Q, G), bool)

        def subject_lists(ok):
            """ten templates a subject, ids = slots: the best eligible score per card (-2: none eligible), then the cards that have one."""
            Gs = G // 10 * 10
            best = np.where(ok[:, :Gs], scores[:, :Gs], np.float32(-2)).reshape(Q, Gs // 10, 10).max(axis=2)
            return lists(best, np.arange(Gs // 10, dtype=np.int64), best > -2, cap)

        ninf = float("-inf")
        calls = [("rank_hits(-inf)", "rank_hits_us", lambda: m.rank_hits(ninf, cap), lambda: lists(scores, glob, every, cap), "idx"),
                 ("rank_hits_filtered(-inf), masks", None, lambda: m.rank_hits_filtered(ninf, cap, labels=hl, masks=masks), lambda: lists(scores, glob, lt, cap), "idx"),
                 ("rank_hits_filtered(-inf), masks + exclusions", None, lambda: m.rank_hits_filtered(ninf, cap, labels=hl, masks=masks, excl=excl), lambda: lists(scores, glob, lt & nl, cap), "idx"),
                 ("rank_hits_filtered(-inf), exclusions alone", None, lambda: m.rank_hits_filtered(ninf, cap, excl=excl), lambda: lists(scores, glob, nl, cap), "idx"),
                 ("rank_subject_hits(-inf), ten templates per subject", "rank_hits_us", lambda: m.rank_subject_hits(hj, ninf, cap), lambda: subject_lists(every) if G % 10 == 0 else None, "subject"),
                 ("rank_subject_hits_filtered(-inf), masks + excluded persons", None, lambda: m.rank_subject_hits_filtered(hj, ninf, cap, labels=hl, masks=masks, excl=excl_s),
                  lambda: subject_lists(lt & nls) if G % 10 == 0 else None, "subject")]
        rows = {}
        for name, base_opt, call, model, key in calls:
            opts = [base_opt] if base_opt else ["rank_filtered_us", "filter_us"]
            us = {k: [] for k in opts}
            for rep in range(a.reps + 1):
                got = call()
                if rep:
                    for k in us:
                        us[k].append(m.get_option(k))
            want = model()
            same = None if want is None else bool(np.array_equal(want[0], got["n_hits"]) and np.array_equal(want[1], got[key]) and np.array_equal(want[2].view(np.uint32), got["score"].view(np.uint32)))
            row = {k: med(v) for k, v in us.items()}
            row.update({"n_hits_median": int(np.median(got["n_hits"])), "equal_to_numpy": same})
            rows[name] = row
        for name, row in rows.items():
            if "filter_us" not in row:
                continue
            base = rows["rank_hits(-inf)" if name.startswith("rank_hits") else "rank_subject_hits(-inf), ten templates per subject"]["rank_hits_us"]["median"]
            row["over_the_unfiltered_call_us"] = row["rank_filtered_us"]["median"] - base
            if name.startswith("rank_hits") and "masks" in name:
                moved = Q * G * 8 + G * 8 * ((Q + R - 1) // R)
                f = row["filter_us"]["median"]
                row["filter_pass"] = {"bytes": moved, "tb_per_s": round(moved / (f * 1e-6) / 1e12, 3) if f > 0 else None, "of_a_float4_copy": round(moved / (f * 1e-6) / 1e12 / COPY_TBS, 3) if f > 0 else None,
                                      "note": "filter_us also holds the exclusions' drop kernel where the call has exclusions"}
        out["galleries"][str(G)] = {"scores": {"zero_fraction": round(float((scores == 0).mean()), 4)}, "eligible_fraction_by_masks": round(float(lt.mean()), 4), "calls": rows}
        m.labels_free(hl); m.subjects_free(hj); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
