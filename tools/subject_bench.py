#!/usr/bin/env python
"""What a subject rank list costs (afis_subjects_create / afis_rank_subjects), on one MI355X with the headline's synthetic gallery and latents: one full search, then for
three label sets of the same shard the device time of afis_rank_subjects' launches at k = 24 (option subject_rank_us: HIP events around the maxima's memset,
k_subject_best and k_topk_subjects) — the median of `--reps` calls after a discarded first one:

  contiguous_tens   cards enrolled one after the other: templates 10 c .. 10 c + 9 belong to subject c
  random_tens       the same subjects, their templates dealt over the shard by a permutation
  hot_subject       one subject holds the first half of the shard (the "unknown" bucket of a real database), every other template is a subject of its own

Beside them: topk_ms of the same search (afis_timing: the template rank list, the stage this one resembles, on the same clock: HIP events), and what a caller pays
today for the same answer — the [n_q][G] score matrix copied to the host and grouped there with numpy — on the HOST clock (time.perf_counter) in the same process: the
copy as the difference of the search's wall time with and without `scores` asked for (medians of `--reps`), the grouping (a stable sort order of the labels made
once, np.maximum.reduceat per call, argpartition for the 24 best) timed per call.  Every rank list is checked against that host grouping.  One JSON document on
stdout (and to --out)."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def timed(fn):
    t0 = time.perf_counter(); r = fn(); return (time.perf_counter() - t0) * 1e3, r


def host_group(scores, order, starts, ids, k):
    """The k best subjects of every row from the score matrix on the host: maxima per label segment, then the k greatest (score descending, id ascending)."""
    best = np.maximum.reduceat(scores[:, order], starts, axis=1)           # [n_q][S], the subjects in ascending id order
    kk = min(k, best.shape[1])
    part = np.argpartition(-best, kk - 1, axis=1)[:, :kk] if kk < best.shape[1] else np.tile(np.arange(best.shape[1]), (best.shape[0], 1))
    out_i = np.empty((best.shape[0], kk), np.int64); out_s = np.empty((best.shape[0], kk), np.float32)
    for q in range(best.shape[0]):
        cut = best[q, part[q]].min()
        cand = np.flatnonzero(best[q] >= cut)                               # everything that ties with the k-th goes into the final sort: the id rule decides
        sel = cand[np.lexsort((ids[cand], -best[q, cand].astype(np.float64)))][:kk]
        out_i[q] = ids[sel]; out_s[q] = best[q, sel]
    return out_i, out_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--k", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    G, Q, k = a.gallery, a.queries, a.k
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    t0 = time.perf_counter()
    lats = S.make_latents(a.seed, Q)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats, G=G)
    out = {"gallery": G, "queries": Q, "k": k, "generation_s": round(time.perf_counter() - t0, 1), "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "clocks": {"subject_rank_us": "device: HIP events around afis_rank_subjects' launches", "topk_ms": "device: HIP events (afis_timing)",
                      "scores_copy_ms, host_group_ms, rank_call_wall_ms": "host: time.perf_counter around calls that return with the device idle"}}
    m = M.Matcher(cbb)
    out["device"] = m.device_info(0)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    med = statistics.median
    rng = np.random.default_rng(a.seed + 3)
    tens = np.arange(G, dtype=np.int64) // 10
    hot = np.where(np.arange(G) < G // 2, 0, np.arange(G, dtype=np.int64))
    labels = {"contiguous_tens": tens, "random_tens": tens[rng.permutation(G)], "hot_subject": hot}

    # ---- the search itself, with and without the score matrix ----
    wall = {False: [], True: []}; topk_ms = []; scores = None
    for step in range(a.reps + 1):
        for want in (False, True):
            ms, r = timed(lambda: m.search_resident(qh, k=k, want_scores=want))
            if want: scores = r["scores"]
            if step:
                wall[want].append(round(ms, 2)); topk_ms.append(round(m.timing()["topk_ms"], 3))
    out["search"] = {"step_wall_ms": wall[False], "step_wall_ms_with_scores": wall[True], "topk_ms": topk_ms, "median_topk_ms": med(topk_ms),
                     "scores_copy_ms": round(med(wall[True]) - med(wall[False]), 2), "scores_bytes": int(scores.nbytes)}

    # ---- the subject rank lists of that search (the last call above left its matrix on the device) ----
    out["labels"] = {}
    for name, subject in labels.items():
        create_ms, h = timed(lambda: m.subjects_create(subject))
        us, call = [], []
        for rep in range(a.reps + 1):
            ms, r = timed(lambda: m.rank_subjects(h, Q, k))
            if rep:
                us.append(m.get_option("subject_rank_us")); call.append(round(ms, 3))
        ids, inv = np.unique(subject, return_inverse=True)
        order = np.argsort(inv, kind="stable"); starts = np.flatnonzero(np.r_[True, inv[order][1:] != inv[order][:-1]])
        group = []
        for rep in range(a.reps + 1):
            ms, (hi, hs) = timed(lambda: host_group(scores, order, starts, ids, k))
            if rep: group.append(round(ms, 2))
        same = bool(np.array_equal(hi, r["subject"][:, :hi.shape[1]]) and np.array_equal(hs.view(np.uint32), r["score"][:, :hs.shape[1]].view(np.uint32)))
        out["labels"][name] = {"subjects": int(len(ids)), "subjects_create_ms": round(create_ms, 2), "subject_rank_us": us, "median_subject_rank_us": med(us),
                               "rank_call_wall_ms": call, "host_group_ms": group, "median_host_group_ms": med(group),
                               "host_route_ms": round(out["search"]["scores_copy_ms"] + med(group), 2), "identical_to_host_grouping": same,
                               "returned_bytes": Q * k * 20}
        m.subjects_free(h)
    c, hs_ = out["labels"]["contiguous_tens"]["median_subject_rank_us"], out["labels"]["hot_subject"]["median_subject_rank_us"]
    out["hot_over_contiguous"] = round(hs_ / max(c, 1), 2)
    m.free_queries(qh); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
