#!/usr/bin/env python
"""What a reverse search costs (afis_queries_upload_reserved / afis_rank_latent_hits), on one MI355X with the headline's synthetic gallery (committed as bench.py commits
it) and a file of `--latents` synthetic latents kept on the device by ONE handle uploaded with reserve=16.  A card is ten rolled prints.  Medians of `--reps` repetitions
after a discarded first; the kinds that are compared are interleaved.

  lists        option rank_latents_us (DEVICE: HIP events around k_transpose_scores + k_rank_hits) of afis_rank_latent_hits(cap 100) on the matrix one card's search left,
               for min_score -inf and for the smallest positive float; beside it, on the HOST clock, the call itself and what the same answer costs without it on this
               build: the same search with want_scores (the matrix to the host) and numpy on the transposed matrix.  Every list is checked against that numpy answer.
  transpose    k_transpose_scores alone, from its own pair of HIP events (parity tap afis_debug_transpose_stats): time, bytes read + written, bytes per second — for the
               card's matrix [latents][10], and for a caller-made matrix of 1000 queries over the whole shard through afis_debug_rank_latent_hits.
  transaction  one card with the reserved handle — Matcher.reverse_search: reopen, add, commit, subset, search, lists, subset_free — against the only route open
               without it, on the same build: the handle freed, all latents uploaded again after the commit, the same subset searched with want_scores, the lists
               sorted on the host.  HOST clock around each; every repetition enrols a new card, the two routes alternate.
  per_pair     afis_timing of the card's search (launch_groups, pairs, total_ms: DEVICE) as time per (latent, print) pair, against the per-pair time of the headline
               step — 100 latents against the whole shard — in the same process.  The search kernels were tuned at launch groups of up to 128 latents against
               shards of 10^4 .. 10^5 templates; whether 128 latents per launch cost time at ten-template shards is what the ratio records.

One process, one device.  One JSON document on stdout and in --out."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def timed(fn):
    t0 = time.perf_counter(); r = fn(); return (time.perf_counter() - t0) * 1e3, r


def column_hits(scores, thr, cap, latent_base=0):
    """numpy on the transposed matrix: (n_hits [n], latent [n][cap], score [n][cap]) of scores [n_q][n]."""
    cols = np.ascontiguousarray(scores.T)
    n = np.empty(len(cols), np.int64); li = np.full((len(cols), cap), -1, np.int64); ls = np.full((len(cols), cap), -np.inf, np.float32)
    for j, col in enumerate(cols):
        at = np.flatnonzero(col >= thr)
        n[j] = len(at)
        at = at[np.lexsort((at, -col[at].astype(np.float64)))][:cap]
        li[j, :len(at)] = latent_base + at; ls[j, :len(at)] = col[at]
    return n, li, ls


def same_lists(got, want):
    return bool(np.array_equal(got["n_hits"], want[0]) and np.array_equal(got["latent"], want[1]) and np.array_equal(got["score"].view(np.uint32), want[2].view(np.uint32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--latents", type=int, default=2000, help="the latent file kept on the device")
    ap.add_argument("--headline-queries", type=int, default=100)
    ap.add_argument("--card", type=int, default=10)
    ap.add_argument("--reserve", type=int, default=16)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--tap-queries", type=int, default=1000, help="queries of the caller-made matrix whose transpose is timed over the whole shard (0 = skip)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_reverse_search.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    G, L, P, cap = a.gallery, a.latents, a.card, a.cap
    med = statistics.median
    spread = lambda v: round(max(v) - min(v), 3)
    hair = float(np.nextafter(np.float32(0), np.float32(1)))
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    t0 = time.perf_counter()
    lats = S.make_latents(a.seed, L)
    gal = S.make_packed_gallery(a.seed, G, cb)
    S.plant_mates(a.seed, gal, cb, lats[:a.headline_queries], G=G)
    n_cards = 2 * (a.reps + 1) + 1
    rng = np.random.default_rng([a.seed, 0xCA])
    cards = []                                                             # per card: ten rolled prints, two of them mates of latents of the file
    for c in range(n_cards):
        prints = [S.make_rolled(np.random.default_rng([a.seed, 0xCB, c, j]), cb) for j in range(P)]
        for j in rng.permutation(P)[:2]:
            prints[j] = S.make_mate(np.random.default_rng([a.seed, 0xCC, c, int(j)]), cb, lats[int(rng.integers(L))])
        cards.append(prints)
    out = {"gallery": G, "latents": L, "card": P, "reserve": a.reserve, "cap": cap, "reps_kept": a.reps, "generation_s": round(time.perf_counter() - t0, 1),
           "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "clocks": {"rank_latents_us, transpose_us, afis_timing": "device: HIP events", "wall_ms": "host: perf_counter around calls that return with the device idle"}}
    m = M.Matcher(cbb, taps=True)                                           # the test library: the product objects plus the taps (transpose_stats)
    out["device"] = m.device_info(0)
    m.gallery_add_packed(gal); m.gallery_commit(0)

    # ---- per_pair, first half: the headline step in this process ----
    qh = m.upload_queries(lats[:a.headline_queries])
    head = []
    for step in range(a.reps + 1):
        m.search_resident(qh, k=24)
        tm = m.timing()
        if step:
            head.append(round(tm["total_ms"], 2))
    m.free_queries(qh)
    head_pairs, head_groups = tm["pairs"], tm["launch_groups"]

    up_ms, qr = timed(lambda: m.upload_queries(lats, reserve=a.reserve))
    out["upload_reserved_ms"] = round(up_ms, 1)

    # ---- lists and per_pair on one card's matrix: the card is enrolled once, its subset searched repeatedly ----
    m.gallery_reopen(); m.gallery_add(cards[-1]); m.gallery_commit(0)
    new_idx = np.arange(G, G + P, dtype=np.int64)
    hs = m.subset_create(new_idx)
    kinds = {"search_k0": [], "search_want_scores": [], "device_call_-inf": [], "device_call_hair": [], "numpy_-inf": [], "numpy_hair": []}
    dev_us = {"-inf": [], "hair": []}; tr = []; search_dev = []; checked = True
    for rep in range(a.reps + 1):
        ms_s, r = timed(lambda: m.search_subset_resident(hs, qr, k=0, want_scores=True))
        scores = r["scores"]
        ms_np = {}
        want = {}
        for name, thr in (("-inf", float("-inf")), ("hair", hair)):
            ms_np[name], want[name] = timed(lambda: column_hits(scores, np.float32(thr), cap))
        ms_0, _ = timed(lambda: m.search_subset_resident(hs, qr, k=0))
        tm = m.timing()
        row = {"search_k0": ms_0, "search_want_scores": ms_s, "numpy_-inf": ms_np["-inf"], "numpy_hair": ms_np["hair"]}
        for name, thr in (("-inf", float("-inf")), ("hair", hair)):
            row["device_call_" + name], got = timed(lambda: m.rank_latent_hits(thr, cap))
            checked = checked and same_lists(got, want[name])
            if rep:
                dev_us[name].append(m.get_option("rank_latents_us")); tr.append(m.transpose_stats())
        if rep:
            for k, v in row.items():
                kinds[k].append(round(v, 3))
            search_dev.append(round(tm["total_ms"], 3))
    card_pairs, card_groups = tm["pairs"], tm["launch_groups"]
    out["lists"] = {"matrix": [L, P], "rank_latents_us": dev_us, "median_rank_latents_us": {k: med(v) for k, v in dev_us.items()}, "wall_ms": kinds,
                    "median_wall_ms": {k: round(med(v), 3) for k, v in kinds.items()},
                    "device_route_wall_ms": {n: round(med(kinds["search_k0"]) + med(kinds["device_call_" + n]), 3) for n in ("-inf", "hair")},
                    "host_route_wall_ms": {n: round(med(kinds["search_want_scores"]) + med(kinds["numpy_" + n]), 3) for n in ("-inf", "hair")},
                    "hits_per_print_median_hair": int(np.median(want["hair"][0])), "checked_against_numpy": bool(checked)}
    t_us = [t[0] for t in tr]
    out["transpose"] = {"card_matrix": {"shape": [L, P], "bytes": tr[0][1], "transpose_us": t_us, "median_us": med(t_us),
                                        "bytes_per_s": round(tr[0][1] / max(med(t_us), 1) * 1e6) if med(t_us) > 0 else None}}
    out["per_pair"] = {"card_search": {"launch_groups": card_groups, "pairs": card_pairs, "total_ms": search_dev, "median_total_ms": med(search_dev), "spread_ms": spread(search_dev),
                                       "ns_per_pair": round(med(search_dev) * 1e6 / max(card_pairs, 1), 1)},
                       "headline_step": {"queries": a.headline_queries, "launch_groups": head_groups, "pairs": head_pairs, "total_ms": head, "median_total_ms": med(head), "spread_ms": spread(head),
                                         "ns_per_pair": round(med(head) * 1e6 / max(head_pairs, 1), 1)}}
    out["per_pair"]["card_over_headline"] = round(out["per_pair"]["card_search"]["ns_per_pair"] / out["per_pair"]["headline_step"]["ns_per_pair"], 2)
    m.subset_free(hs)

    # ---- transpose over the whole shard: a caller-made matrix through the tap ----
    if a.tap_queries > 0:
        Gn = m.resident_size
        u = np.random.default_rng(a.seed + 5).random((a.tap_queries, Gn), dtype=np.float32)
        sc = np.where(u < 0.4, u * 12, 0).astype(np.float32)
        t_us = []
        for rep in range(a.reps + 1):
            got = m.debug_rank_latent_hits(sc, hair, 1)
            if rep:
                t_us.append(m.transpose_stats()[0]); nbytes = m.transpose_stats()[1]
        out["transpose"]["shard_matrix"] = {"shape": [a.tap_queries, Gn], "bytes": nbytes, "transpose_us": t_us, "median_us": med(t_us), "bytes_per_s": round(nbytes / med(t_us) * 1e6),
                                            "rank_latents_us": m.get_option("rank_latents_us"),
                                            "best_latent_checked": bool(np.array_equal(got["latent"][:, 0], np.where(sc.max(axis=0) > 0, np.argmax(sc, axis=0), -1)))}
        del sc, u

    # ---- transaction: the reserved handle against uploading everything again ----
    new_ms, old_ms, old_parts = [], [], {"upload_ms": [], "search_ms": [], "numpy_ms": []}
    same = True
    qp = None
    for rep in range(a.reps + 1):
        ms, (idx, lists) = timed(lambda: m.reverse_search(qr, cards[2 * rep], hair, cap))
        if rep:
            new_ms.append(round(ms, 2))

        def old_route(card):
            nonlocal qp
            first = m.resident_size
            m.gallery_reopen(); m.gallery_add(card); m.gallery_commit(0)
            if qp is not None:
                m.free_queries(qp)
            t1 = time.perf_counter()
            qp = m.upload_queries(lats)
            t2 = time.perf_counter()
            h = m.subset_create(np.arange(first, first + len(card), dtype=np.int64))
            t3 = time.perf_counter()
            r = m.search_subset_resident(h, qp, k=0, want_scores=True)
            t4 = time.perf_counter()
            res = column_hits(r["scores"], np.float32(hair), cap)
            t5 = time.perf_counter()
            m.subset_free(h)
            return res, ((t2 - t1) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3)
        ms, (res, parts) = timed(lambda: old_route(cards[2 * rep + 1]))
        if rep:
            old_ms.append(round(ms, 2))
            for k, v in zip(old_parts, parts):
                old_parts[k].append(round(v, 2))
        # the reserved handle on the card the old route just enrolled: the same lists
        hs = m.subset_create(np.arange(m.resident_size - P, m.resident_size, dtype=np.int64))
        m.search_subset_resident(hs, qr, k=0)
        same = same and same_lists(m.rank_latent_hits(hair, cap), res)
        m.subset_free(hs)
    out["transaction"] = {"reserved_handle_ms": new_ms, "median_reserved_handle_ms": med(new_ms), "spread_reserved_handle_ms": spread(new_ms),
                          "upload_again_ms": old_ms, "median_upload_again_ms": med(old_ms), "spread_upload_again_ms": spread(old_ms), "upload_again_parts": old_parts,
                          "upload_again_over_reserved": round(med(old_ms) / med(new_ms), 1), "lists_identical": bool(same), "resident_templates_at_end": m.resident_size}
    if qp is not None:
        m.free_queries(qp)
    m.free_queries(qr); m.close()
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
