#!/usr/bin/env python
"""What the print cascade costs and what it drops (afis_search_prints_cascade) beside the full print search, on one MI355X with bench.py's synthetic gallery: 100
resident prints x 100 000 prints by default, weights 1 and 0.3f, the headline and the structured workload.

The query prints are PLANTED: the generator plants several mates of every synthetic latent into the gallery (make_mate), and two mates of one latent are two
impressions of one finger.  Query q is the first planted mate of latent q; its print mates are the latent's other planted mates.

  (a) time    per keep (100, 1000, 4096), INTERLEAVED repetition by repetition with the yardstick — afis_search_prints on the same context, the only route before,
              never the code under test — `--reps` kept after a discarded first, median and spread = max - min: the HOST clock (perf_counter around the C call alone,
              which builds the temporary query handle too) and the DEVICE clock (the cascade: options print_cascade_stage1_us + print_cascade_select_us +
              print_cascade_stage2_us, each from its own pair of HIP events; the full print search: afis_timing.total_ms), the three stage options, cands_ms /
              minu_graph_ms of stage 1, print_gather_us, and the ratio cascade / full as measured
  (b) keep    for the planted print mates (synthetic data: facts about this generator, not about fingerprints): how many are kept at each keep, and of the mates
              that stand at rank 1 under afis_search_prints — the query's own print excluded — how many still stand at rank 1: both read through
              afis_rank_positions on the two matrices
Beside them whether every kept cell is bit for bit the full print search's cell.  Recorded, not asserted; nothing here is tuned for.  One JSON document on stdout and in
--out."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
from cascade_search_timing import med, workload                            # the same galleries, latents and planted mates as the latent cascade's figures

NO_ENTRY = np.uint32(0xFFFFFFFF)
STAGES = ("stage1", "select", "stage2")


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def cascade_call(m, idx, wm, wt, keep, G):
    """The C call alone under the host clock, without scores or lists crossing to the host: what a caller that goes on with the ranking family pays."""
    n = len(idx)
    st = np.zeros(n, np.int32)
    t0 = time.perf_counter()
    m._chk(m.lib.afis_search_prints_cascade(m.ctx, M._ptr(idx, C.c_int64), n, M._ptr(wm, C.c_float), M._ptr(wt, C.c_float), keep, None, M._ptr(st, C.c_int32), None, None, None))
    ms = (time.perf_counter() - t0) * 1e3
    m.last_n_q = n; m.last_n_templates = G
    return ms


def full_call(m, idx, wm, wt, G):
    n = len(idx)
    st = np.zeros(n, np.int32)
    t0 = time.perf_counter()
    m._chk(m.lib.afis_search_prints(m.ctx, None, M._ptr(idx, C.c_int64), n, M._ptr(wm, C.c_float), M._ptr(wt, C.c_float), None, M._ptr(st, C.c_int32)))
    ms = (time.perf_counter() - t0) * 1e3
    m.last_n_q = n; m.last_n_templates = G
    return ms


def measure(name, a, cb, cbb):
    Q, G = a.queries, a.gallery
    _, gal, planted = workload(name, a.seed, Q, G, cb, cbb)
    m = M.Matcher(cbb)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    fingers = [[int(g) for g, _ in lst] for _, lst in sorted(planted.items()) if len(lst) >= 2]
    idx = np.ascontiguousarray([f[0] for f in fingers], np.int64)
    n_q = len(idx)
    wm, wt = np.ones(n_q, np.float32), np.full(n_q, 0.3, np.float32)
    mq = np.array([q for q, f in enumerate(fingers) for _ in f[1:]], np.int32)
    mi = np.array([g for f in fingers for g in f[1:]], np.int64)
    own = [[int(g)] for g in idx]
    full = m.search_prints(idx, wm, wt)["scores"]                           # warm-up of the full print search: first-use allocations
    pos_full = m.rank_positions(mq, mi, excl=own)
    first = pos_full["n_before"] == 0
    note(f"{name}: {n_q} query prints x {G}, {len(mq)} print mates, {int(first.sum())} at rank 1 under the full print search")
    out = {"query_prints": n_q, "print_mates": int(len(mq)), "print_mates_at_rank_1_under_the_full_print_search": int(first.sum()), "keeps": {}}
    for keep in a.keep:
        keep = min(keep, 4096)
        cascade_call(m, idx, wm, wt, keep, G)                               # warm-up of this keep: the call's own buffers
        c_ms, c_us, f_ms, f_dev, st_us, cands, graph, gather, f_gather = [], [], [], [], {k: [] for k in STAGES}, [], [], [], []
        for rep in range(a.reps + 1):
            ms = cascade_call(m, idx, wm, wt, keep, G)
            st = [m.get_option("print_cascade_%s_us" % k) for k in STAGES]
            tm = m.timing(); g_us = m.get_option("print_gather_us")
            fms = full_call(m, idx, wm, wt, G)
            ftm = m.timing()
            if rep:
                c_ms.append(ms); c_us.append(sum(st)); cands.append(tm["cands_ms"]); graph.append(tm["minu_graph_ms"]); gather.append(g_us)
                for k, v in zip(STAGES, st):
                    st_us[k].append(v)
                f_ms.append(fms); f_dev.append(ftm["total_ms"]); f_gather.append(m.get_option("print_gather_us"))
            note(f"{name} keep {keep} round {rep}: cascade {ms:.0f} ms, full {fms:.0f} ms on the host clock")
        got = m.search_prints_cascade(idx, wm, wt, keep)
        g = got["scores"].view(np.uint32)
        kept = g != NO_ENTRY
        pos = m.rank_positions(mq, mi, excl=own)
        listed = pos["status"] == 0
        pairs = m.get_option("print_cascade_kept_pairs")
        out["keeps"][str(keep)] = {
            "kept_pairs": pairs, "launch_groups": tm["launch_groups"],
            "cascade_host_ms": med(c_ms), "cascade_device_us": med(c_us), "stage1_us": med(st_us["stage1"]), "select_us": med(st_us["select"]), "stage2_us": med(st_us["stage2"]),
            "stage2_us_per_pair": statistics.median(st_us["stage2"]) / max(pairs, 1),
            "stage1_cands_ms": med(cands), "stage1_minu_graph_ms": med(graph), "cascade_print_gather_us": med(gather),
            "full_host_ms": med(f_ms), "full_device_ms": med(f_dev), "full_print_gather_us": med(f_gather),
            "cascade_over_full_host": statistics.median(c_ms) / statistics.median(f_ms),
            "cascade_over_full_device": statistics.median(c_us) / 1e3 / statistics.median(f_dev),
            "stage1_over_full_device": statistics.median(st_us["stage1"]) / 1e3 / statistics.median(f_dev),
            "kept_cells_equal_the_full_print_search": bool(np.array_equal(g[kept], full.view(np.uint32)[kept])), "kept_cells": int(kept.sum()),
            "synthetic_print_mates_kept": int(listed.sum()),
            "synthetic_rank_1_print_mates_still_rank_1": int((pos["n_before"][first] == 0).sum()),
        }
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100, help="synthetic latents whose planted mates are the query prints and their print mates")
    ap.add_argument("--keep", type=int, nargs="+", default=[100, 1000, 4096])
    ap.add_argument("--workloads", nargs="+", default=["headline", "structured"], choices=sorted(S.WORKLOADS))
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "print_cascade_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    if "structured" in a.workloads:                                         # the structured generator draws on the GPU through torch: torch opens the device first, as in bench.py
        import torch
        torch.zeros(1, device=torch.device("cuda", 0))
    probe = M.Matcher(cbb)
    out = {"queries": a.queries, "gallery": a.gallery, "weights": "1 at the minutiae template, 0.3f at the texture template", "reps": a.reps, "interleaved": True,
           "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12], "device": probe.device_info(0),
           "cascade_pairs_per_launch": probe.get_option("cascade_pairs_per_launch"),
           "clocks": {"*_host_ms": "host: perf_counter around the C call, which returns after its wait; no matrix or list crosses to the host; both calls build their temporary query handles inside",
                      "cascade_device_us": "device: options print_cascade_stage1_us + print_cascade_select_us + print_cascade_stage2_us, each from its own pair of HIP events (the gather beside it: print_gather_us)",
                      "full_device_ms": "device: afis_timing.total_ms of afis_search_prints, the yardstick"},
           "mates": "planted by the synthetic generator (two make_mate prints of one latent): the counts are facts about this synthetic data, the query's own print excluded", "workloads": {}}
    probe.close()
    for name in a.workloads:
        out["workloads"][name] = measure(name, a, cb, cbb)
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
