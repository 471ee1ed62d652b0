#!/usr/bin/env python
"""What the eligible cascade costs (afis_search_cascade_eligible) beside the two routes that existed before it, on one MI355X with bench.py's synthetic gallery and
latents: 100 latents x 100 000 prints by default, labels = ten one-hot finger classes (t % 10), two mask layouts:

  one_finger    latent q may only come from finger q % 10: ten classes of ten latents, 10 000 columns each
  two_fingers   every latent may come from fingers {2, 7}: one class of 20 000 columns

  (a) time    per layout and keep (100, 1000), INTERLEAVED repetition by repetition, `--reps` kept after a discarded first, median and spread = max - min, of
                eligible_cascade   afis_search_cascade_eligible(labels, masks, keep)
                eligible_search    afis_search_eligible(labels, masks): all four scorers for the eligible cells
                cascade_filtered   afis_search_cascade(keep) followed by afis_rank_hits_filtered(labels, masks, -inf, cap = keep): stage 1 for every cell
              the HOST clock (perf_counter around the C calls alone; no matrix crosses to the host) and the DEVICE clock (the options cascade_stage1_us +
              cascade_select_us + cascade_stage2_us, afis_timing.total_ms, plus rank_filtered_us for the third route).  The eligible cascade's per-class fixed cost —
              the sub-shard's gather, the class's query upload and its wait — is what the host clock holds beyond the device clock, divided by the classes
  (b) lists   for the ELIGIBLE planted mates (synthetic data: facts about this generator, not about fingerprints): how many each route lists at all and how many it
              lists at rank 1, read through afis_rank_positions on each route's matrix (with the labels and masks where the matrix holds ineligible cells)
Recorded, not asserted; nothing here is tuned for.  One JSON document on stdout; --out merges the workloads measured into the file (one workload per run keeps every
GPU step under a time limit of its own)."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
from cascade_search_timing import med, workload                             # the same workloads, the same statistics

NINF = float("-inf")
STAGES = ("stage1", "select", "stage2")


def layouts(Q):
    one = np.zeros((Q, 3), np.uint64); one[:, 0] = np.uint64(1) << (np.arange(Q) % 10).astype(np.uint64)
    two = np.zeros((Q, 3), np.uint64); two[:, 0] = (1 << 2) | (1 << 7)
    return {"one_finger": one, "two_fingers": two}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(name, a, cb, cbb):
    Q, G = a.queries, a.gallery
    lats, gal, planted = workload(name, a.seed, Q, G, cb, cbb)
    m = M.Matcher(cbb)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    h = m.upload_queries(lats)
    v = M._Views(lats)
    lab = (np.uint64(1) << (np.arange(G) % 10).astype(np.uint64)).astype(np.uint64)
    lh = m.labels_create(lab)
    st = np.zeros(Q, np.int32); pst = M._ptr(st, C.c_int32)
    n_hits = np.zeros(Q, np.int64)
    mq = np.array([q for q, lst in planted.items() for _ in lst], np.int32)
    mi = np.array([g for q, lst in planted.items() for g, _ in lst], np.int64)
    out = {"mates": int(len(mq)), "layouts": {}}
    for lay, masks in layouts(Q).items():
        mk = np.ascontiguousarray(masks); pmk = M._ptr(mk, C.c_uint64)
        a_of, none_of = mk[mq, 0], mk[mq, 2]
        elig = ((lab[mi] & a_of) != 0) & ((lab[mi] & none_of) == 0)
        eq, ei = mq[elig], mi[elig]
        res = {"classes": len({tuple(r) for r in mk.tolist()}), "eligible_mates": int(elig.sum()), "keeps": {}}
        for keep in a.keep:
            idx = np.full((Q, keep), -1, np.int64); sc = np.zeros((Q, keep), np.float32)

            def eligible_cascade():
                m._chk(m.lib.afis_search_cascade_eligible(m.ctx, lh[0], pmk, v.arr, v.n, keep, None, pst, None, None, None))

            def eligible_search():
                m._chk(m.lib.afis_search_eligible(m.ctx, lh[0], pmk, v.arr, v.n, None, pst))

            def cascade_filtered():
                m._chk(m.lib.afis_search_cascade(m.ctx, h[0], keep, None, pst, None, None, None))
                m._chk(m.lib.afis_rank_hits_filtered(m.ctx, lh[0], pmk, None, None, Q, NINF, keep, M._ptr(n_hits, C.c_int64), M._ptr(idx, C.c_int64), M._ptr(sc, C.c_float)))

            def cascade_us():
                return sum(m.get_option("cascade_%s_us" % k) for k in STAGES)
            r = {k: [] for k in ("ec_host", "ec_dev", "ec_s1", "ec_sel", "ec_s2", "es_host", "es_dev", "cf_host", "cf_dev")}
            for rep in range(a.reps + 2):                                   # the first warms every route's buffers up, the second is discarded
                ms = timed(eligible_cascade)
                us = [m.get_option("cascade_%s_us" % k) for k in STAGES]
                pairs, classes, cells = m.get_option("cascade_kept_pairs"), m.get_option("eligible_classes"), m.timing()["pairs"]
                es = timed(eligible_search); es_dev = m.timing()["total_ms"]
                cf = timed(cascade_filtered); cf_dev = (cascade_us() + m.get_option("rank_filtered_us")) / 1e3
                if rep > 1:
                    r["ec_host"].append(ms); r["ec_dev"].append(sum(us) / 1e3); r["ec_s1"].append(us[0] / 1e3); r["ec_sel"].append(us[1] / 1e3); r["ec_s2"].append(us[2] / 1e3)
                    r["es_host"].append(es); r["es_dev"].append(es_dev); r["cf_host"].append(cf); r["cf_dev"].append(cf_dev)
            # what each route lists of the eligible planted mates
            lists = {}
            m.last_n_q = Q
            for route, call, filt in (("eligible_cascade", eligible_cascade, False), ("eligible_search", eligible_search, False), ("cascade_filtered", cascade_filtered, True)):
                call()
                p = m.rank_positions(eq, ei, labels=lh, masks=mk) if filt else m.rank_positions(eq, ei)
                lists[route] = {"listed": int((p["status"] == 0).sum()), "at_rank_1": int((p["n_before"] == 0).sum())}
            h_ec, d_ec = statistics.median(r["ec_host"]), statistics.median(r["ec_dev"])
            res["keeps"][str(keep)] = {
                "kept_pairs": pairs, "classes": classes, "stage1_cells": cells,
                "eligible_cascade": {"host_ms": med(r["ec_host"]), "device_ms": med(r["ec_dev"]), "stage1_ms": med(r["ec_s1"]), "select_ms": med(r["ec_sel"]), "stage2_ms": med(r["ec_s2"]),
                                     "per_class_fixed_ms": (h_ec - d_ec) / max(classes, 1)},
                "eligible_search": {"host_ms": med(r["es_host"]), "device_ms": med(r["es_dev"])},
                "cascade_filtered": {"host_ms": med(r["cf_host"]), "device_ms": med(r["cf_dev"])},
                "eligible_cascade_over_eligible_search_host": h_ec / statistics.median(r["es_host"]),
                "eligible_cascade_over_cascade_filtered_host": h_ec / statistics.median(r["cf_host"]),
                "synthetic_eligible_mates": lists,
            }
        out["layouts"][lay] = res
    m.labels_free(lh); m.free_queries(h); m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--keep", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--workloads", nargs="+", default=["headline", "structured"], choices=sorted(S.WORKLOADS))
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (a warm-up and one discarded repetition are run first)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_eligible_timing.json"), help="the JSON document the measured workloads are merged into ('' = stdout only)")
    a = ap.parse_args()
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    if "structured" in a.workloads:                                         # the structured generator draws on the GPU through torch: torch opens the device first, as in bench.py
        import torch
        torch.zeros(1, device=torch.device("cuda", 0))
    probe = M.Matcher(cbb)
    out = {"queries": a.queries, "gallery": a.gallery, "reps": a.reps, "interleaved": True, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "device": probe.device_info(0), "cascade_pairs_per_launch": probe.get_option("cascade_pairs_per_launch"), "labels": "ten one-hot finger classes, t % 10",
           "clocks": {"host_ms": "host: perf_counter around the C call(s), which return after their waits; no matrix crosses to the host",
                      "device_ms": "device: cascade_stage1_us + cascade_select_us + cascade_stage2_us (summed over the classes); afis_timing.total_ms for eligible_search; "
                                   "plus rank_filtered_us for cascade_filtered",
                      "per_class_fixed_ms": "(host - device) / classes of the eligible cascade: the sub-shard's gather, the class's query upload, its wait"},
           "mates": "planted by the synthetic generator: the counts are facts about this synthetic data, not about fingerprints", "workloads": {}}
    probe.close()
    if a.out and os.path.exists(a.out):
        try:
            out["workloads"] = json.load(open(a.out)).get("workloads", {})
        except ValueError:
            pass
    for name in a.workloads:
        out["workloads"][name] = measure(name, a, cb, cbb)
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
