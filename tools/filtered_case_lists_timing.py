#!/usr/bin/env python
"""What per-latent eligibility costs on the case lists and the reverse lists (afis_rank_case_hits_filtered / afis_rank_case_subject_hits_filtered /
afis_rank_latent_hits_filtered), on one MI355X with the headline's synthetic gallery and latents (committed as bench.py commits them): one search of 100 latents x
100 000 templates, then on the matrix it left on the device the latents are dealt into 25 cases of four interleaved members (query i belongs to case i mod 25), with
the labels, masks and exclusion lists of tools/filtered_hits_timing.py (cards of ten one-hot fingers and a sex; per query one to three fingers and one sex allowed,
about a tenth of the gallery; `--excluded` elimination prints per query).  Every call below is made `--reps` + 1 times, the first discarded; medians with the spread
(max - min) beside them; every filtered call stands next to its unfiltered sibling ON THE SAME MATRIX IN THE SAME RUN:

  rank_case_hits / ..._filtered           SUM and MAX, (-inf, cap)
  rank_case_subject_hits / ..._filtered   SUM, (-inf, cap), ten templates per subject, the excluded prints' persons excluded
  rank_latent_hits / ..._filtered         (-inf, cap): per template the eligible latents
  rank_hits_filtered                      the same filter on the per-query lists: filter_us is the filter pass's own figure in this run

Clocks.  DEVICE (HIP events inside the library): rank_cases_us with its parts case_fuse_us (everything before k_rank_hits: for a filtered call the filter pass too)
and case_rank_us; rank_latents_us; rank_filtered_us / filter_us.  HOST (perf_counter): the numpy route — eligibility, fold and sort on the [n_q][G] matrix — which
is also what every list is checked against.  Expectation: a filtered call costs its sibling plus about the filter pass; the masks leave k_rank_hits less to select, so
it may cost less.  `explained` says whether (filtered - sibling) exceeds filter_us by more than the spreads of the two calls.  Recorded, not asserted.  One JSON
document on stdout and in --out."""
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


def fuse(rows, ok, case_of, mode):
    """The header's fold on whole rows over the ELIGIBLE members in ascending query position (a search's scores are -1 or >= +0.0) -> (fused, entry)."""
    out, ent = [], []
    for cid in np.unique(case_of):
        members = np.flatnonzero(case_of == cid)
        if mode == M.CASE_SUM:
            acc = np.zeros(rows.shape[1], np.float32); took = np.zeros(rows.shape[1], bool)
            for i in members:
                part = ok[i] & (rows[i] >= 0)
                acc = np.where(part, (acc + rows[i]).astype(np.float32), acc); took |= part
            out.append(np.where(took, acc, np.float32(-1)))
        else:
            out.append(np.where(ok[members], rows[members], np.float32(-2)).max(axis=0))
        ent.append(ok[members].any(axis=0))
    return np.array(out, np.float32), np.array(ent, bool)


def lists(fused, entry, names, cap):
    """min_score = -inf: every entry, score descending, name ascending."""
    n = np.empty(len(fused), np.int64); a = np.full((len(fused), cap), -1, np.int64); sc = np.full((len(fused), cap), -np.inf, np.float32)
    for c, row in enumerate(fused):
        at = np.flatnonzero(entry[c])
        at = at[np.lexsort((names[at], -row[at].astype(np.float64)))][:cap]
        n[c] = int(entry[c].sum()); a[c, :len(at)] = names[at]; sc[c, :len(at)] = row[at]
    return n, a, sc


def column_lists(scores, ok, cap):
    """Per column the eligible queries, score descending, position ascending: one stable sort of the transposed matrix."""
    st = np.where(ok, scores, np.float32(-np.inf)).T                        # (a search's scores are >= -1: -inf sorts the ineligible cells last)
    order = np.argsort(-st, axis=1, kind="stable")[:, :cap]
    n = ok.sum(axis=0).astype(np.int64)
    keep = np.arange(order.shape[1])[None, :] < n[:, None]
    a = np.where(keep, order, -1).astype(np.int64); sc = np.where(keep, np.take_along_axis(st, order, axis=1), np.float32(-np.inf)).astype(np.float32)
    pad = cap - order.shape[1]
    if pad > 0:
        a = np.pad(a, ((0, 0), (0, pad)), constant_values=-1); sc = np.pad(sc, ((0, 0), (0, pad)), constant_values=-np.inf)
    return n, a, sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--case-size", type=int, default=4)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--excluded", type=int, default=20, help="elimination prints per query")
    ap.add_argument("--reps", type=int, default=5, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_case_lists_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    G, Q, cap = a.gallery, a.queries, a.cap
    n_cases = max(1, Q // a.case_size)
    case_of = (np.arange(Q) % n_cases).astype(np.int64)
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats, G=G)
    rng = np.random.default_rng(a.seed)
    out = {"gallery": G, "queries": Q, "cases": n_cases, "case_size": a.case_size, "cap": cap, "excluded_per_query": a.excluded,
           "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "clocks": {"rank_cases_us, case_fuse_us, case_rank_us, rank_latents_us, rank_filtered_us, filter_us": "device: HIP events inside the library",
                      "numpy_route_ms": "host: perf_counter around eligibility, fold and sort in numpy"}}
    m = M.Matcher(cbb)
    out["device"] = m.device_info(0)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    scores = m.search_resident(qh, k=0, want_scores=True)["scores"]
    m.free_queries(qh)                                                      # (leaves the matrix alone)
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
    hl = m.labels_create(labels)
    hj = m.subjects_create(card)
    every = np.ones((Q, G), bool)

    def eligibility():
        ok = (labels[None, :] & masks[:, 2:3]) == 0
        for q in range(Q):
            ok[q, excl[q]] = False
        return ok

    def subject_model(ok, excluded, mode):
        """ten templates a subject, ids = slots: a member's value is the best eligible score of the card; the member is there when one exists and the card is not excluded."""
        Gs = G // 10 * 10
        best = np.where(ok[:, :Gs], scores[:, :Gs], np.float32(-2)).reshape(Q, Gs // 10, 10).max(axis=2)
        have = best > -2
        if excluded:
            for q in range(Q):
                have[q, excl_s[q]] = False
        f, e = fuse(best, have, case_of, mode)
        return lists(f, e, np.arange(Gs // 10, dtype=np.int64), cap)

    def label_only():
        return (labels[None, :] & masks[:, 2:3]) == 0

    def case_model(ok, mode):
        f, e = fuse(scores, ok, case_of, mode)
        return lists(f, e, glob, cap)

    ninf = float("-inf")
    case_opts, latent_opts = ["rank_cases_us", "case_fuse_us", "case_rank_us"], ["rank_latents_us"]
    SUM, MAX = M.CASE_SUM, M.CASE_MAX
    flt = dict(labels=hl, masks=masks, excl=excl)
    # name, options, call, numpy route (None: the sibling — checked against the route with every cell eligible), key of the names, the sibling's name
    calls = [("rank_case_hits(SUM)", case_opts, lambda: m.rank_case_hits(case_of, SUM, ninf, cap), lambda: case_model(every, SUM), "idx", None),
             ("rank_case_hits_filtered(SUM)", case_opts, lambda: m.rank_case_hits_filtered(case_of, SUM, ninf, cap, **flt), lambda: case_model(eligibility(), SUM), "idx", "rank_case_hits(SUM)"),
             ("rank_case_hits(MAX)", case_opts, lambda: m.rank_case_hits(case_of, MAX, ninf, cap), lambda: case_model(every, MAX), "idx", None),
             ("rank_case_hits_filtered(MAX)", case_opts, lambda: m.rank_case_hits_filtered(case_of, MAX, ninf, cap, **flt), lambda: case_model(eligibility(), MAX), "idx", "rank_case_hits(MAX)"),
             ("rank_case_subject_hits(SUM)", case_opts, lambda: m.rank_case_subject_hits(hj, case_of, SUM, ninf, cap), lambda: subject_model(every, False, SUM) if G % 10 == 0 else None, "subject", None),
             ("rank_case_subject_hits_filtered(SUM)", case_opts, lambda: m.rank_case_subject_hits_filtered(hj, case_of, SUM, ninf, cap, labels=hl, masks=masks, excl=excl_s),
              lambda: subject_model(label_only(), True, SUM) if G % 10 == 0 else None, "subject", "rank_case_subject_hits(SUM)"),
             ("rank_latent_hits", latent_opts, lambda: m.rank_latent_hits(ninf, cap), lambda: column_lists(scores, every, cap), "latent", None),
             ("rank_latent_hits_filtered", latent_opts, lambda: m.rank_latent_hits_filtered(ninf, cap, **flt), lambda: column_lists(scores, eligibility(), cap), "latent", "rank_latent_hits"),
             ("rank_hits_filtered", ["rank_filtered_us", "filter_us"], lambda: m.rank_hits_filtered(ninf, cap, **flt), None, "idx", None)]
    rows = {}
    for name, opts, call, model, key, sibling in calls:
        us = {k: [] for k in opts}
        for rep in range(a.reps + 1):
            got = call()
            if rep:
                for k in us:
                    us[k].append(m.get_option(k))
        row = {k: med(v) for k, v in us.items()}
        row["n_hits_median"] = int(np.median(got["n_hits"]))
        if model is not None:
            t0 = time.perf_counter()
            want = model()
            row["numpy_route_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["equal_to_the_numpy_route"] = None if want is None else bool(
                np.array_equal(want[0], got["n_hits"]) and np.array_equal(want[1], got[key]) and np.array_equal(want[2].view(np.uint32), got["score"].view(np.uint32)))
        rows[name] = row
    filter_us = rows["rank_hits_filtered"]["filter_us"]
    for name, opts, call, model, key, sibling in calls:
        if sibling is None:
            continue
        total = opts[0]
        over = rows[name][total]["median"] - rows[sibling][total]["median"]
        slack = rows[name][total]["spread"] + rows[sibling][total]["spread"] + filter_us["spread"]
        rows[name]["over_the_sibling_us"] = over
        rows[name]["filter_us_of_this_run"] = filter_us["median"]
        rows[name]["explained"] = bool(over - filter_us["median"] <= slack)   # no more than the filter pass, within the spreads
    ok = eligibility()
    out["scores"] = {"zero_fraction": round(float((scores == 0).mean()), 4)}
    out["eligible_fraction"] = round(float(ok.mean()), 4)
    out["columns_without_an_eligible_member_per_case_median"] = int(np.median([(~ok[case_of == c].any(axis=0)).sum() for c in range(n_cases)]))
    out["calls"] = rows
    m.labels_free(hl); m.subjects_free(hj); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
