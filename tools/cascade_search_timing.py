#!/usr/bin/env python
"""What the cascade search costs and what it drops (afis_search_cascade) beside the full search, on one MI355X with bench.py's synthetic gallery and latents: 100
latents x 100 000 prints by default, the headline and the structured workload.

  (a) time    per keep (100, 1000, 4096), INTERLEAVED repetition by repetition with the yardstick — afis_search_resident(k = 0) on the same context, never the code
              under test — `--reps` kept after a discarded first, median and spread = max - min: the HOST clock (perf_counter around the C call alone) and the DEVICE
              clock (the cascade: options cascade_stage1_us + cascade_select_us + cascade_stage2_us, each from its own pair of HIP events; the full search:
              afis_timing.total_ms), the three stage options, cands_ms / minu_graph_ms of stage 1, and the ratio cascade / full as measured
  (b) keep    for the PLANTED mates of the workload (synthetic data: facts about this generator, not about fingerprints): the share that is kept at each keep, and of
              the mates that stand at rank 1 under afis_search the share that still stands at rank 1 — both read through afis_rank_positions on the two matrices
Beside them whether every kept cell is bit for bit the full search's cell.  Recorded, not asserted; nothing here is tuned for.  One JSON document on stdout and in --out."""
import argparse, ctypes as C, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")
NO_ENTRY = np.uint32(0xFFFFFFFF)


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def workload(name, seed, Q, G, cb, cbb):
    wl = S.WORKLOADS[name]
    if name == "structured":
        import torch
        SS = importlib.import_module("msu-latentafis_amd.host.synth_structured")
        sigma = SS.DUP_SIGMA[10]
        lats = SS.make_structured_latents(seed, Q, sigma=sigma, **wl["latent"])
        enc = M.Matcher(cbb)
        gal = SS.make_packed_gallery_structured(seed, G, cb, 0, G, sigma=sigma, encode=enc.pq_encode, device=torch.device("cuda", 0), **wl["gallery"])
        enc.close()
        return lats, gal, SS.plant_structured_mates(seed, gal, cb, lats, G=G, lo=0, sigma=sigma)
    lats = S.make_latents(seed, Q, **wl["latent"])
    gal = S.make_packed_gallery(seed, G, cb, **wl["gallery"])
    return lats, gal, S.plant_mates(seed, gal, cb, lats)


def cascade_call(m, h, keep, n_q, G):
    """The C call alone under the host clock, without scores or lists crossing to the host: what a caller that goes on with the ranking family pays."""
    st = np.zeros(n_q, np.int32)
    t0 = time.perf_counter()
    m._chk(m.lib.afis_search_cascade(m.ctx, h[0], keep, None, M._ptr(st, C.c_int32), None, None, None))
    ms = (time.perf_counter() - t0) * 1e3
    m.last_n_q = n_q; m.last_n_templates = G
    return ms


def full_call(m, h, n_q):
    st = np.zeros(n_q, np.int32)
    t0 = time.perf_counter()
    m._chk(m.lib.afis_search_resident(m.ctx, h[0], None, None, M._ptr(st, C.c_int32), 0, None, None))
    return (time.perf_counter() - t0) * 1e3


def measure(name, a, cb, cbb):
    Q, G = a.queries, a.gallery
    lats, gal, planted = workload(name, a.seed, Q, G, cb, cbb)
    m = M.Matcher(cbb)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    h = m.upload_queries(lats)
    full = m.search_resident(h, k=0, want_scores=True)["scores"]           # warm-up of the full search: first-use allocations
    m.last_n_q = Q
    mq = np.array([q for q, lst in planted.items() for _ in lst], np.int32)
    mi = np.array([g for q, lst in planted.items() for g, _ in lst], np.int64)
    pos_full = m.rank_positions(mq, mi)
    first = pos_full["n_before"] == 0
    out = {"mates": int(len(mq)), "mates_at_rank_1_under_the_full_search": int(first.sum()), "keeps": {}}
    for keep in a.keep:
        keep = min(keep, 4096)
        cascade_call(m, h, keep, Q, G)                                      # warm-up of this keep: the call's own buffers
        c_ms, c_us, f_ms, f_dev, s1, sel, s2, cands, graph = [], [], [], [], [], [], [], [], []
        for rep in range(a.reps + 1):
            ms = cascade_call(m, h, keep, Q, G)
            st = [m.get_option("cascade_%s_us" % k) for k in ("stage1", "select", "stage2")]
            tm = m.timing()
            fms = full_call(m, h, Q)
            ftm = m.timing()
            if rep:
                c_ms.append(ms); c_us.append(sum(st)); s1.append(st[0]); sel.append(st[1]); s2.append(st[2]); cands.append(tm["cands_ms"]); graph.append(tm["minu_graph_ms"])
                f_ms.append(fms); f_dev.append(ftm["total_ms"])
        got = m.search_cascade(h, keep, want_scores=True, want_kept=True)
        g = got["scores"].view(np.uint32)
        kept = g != NO_ENTRY
        pos = m.rank_positions(mq, mi)
        listed = pos["status"] == 0
        out["keeps"][str(keep)] = {
            "kept_pairs": m.get_option("cascade_kept_pairs"),
            "cascade_host_ms": med(c_ms), "cascade_device_us": med(c_us), "stage1_us": med(s1), "select_us": med(sel), "stage2_us": med(s2),
            "stage1_cands_ms": med(cands), "stage1_minu_graph_ms": med(graph),
            "full_host_ms": med(f_ms), "full_device_ms": med(f_dev),
            "cascade_over_full_host": statistics.median(c_ms) / statistics.median(f_ms),
            "cascade_over_full_device": statistics.median(c_us) / 1e3 / statistics.median(f_dev),
            "stage1_over_full_device": statistics.median(s1) / 1e3 / statistics.median(f_dev),
            "kept_cells_equal_the_full_search": bool(np.array_equal(g[kept], full.view(np.uint32)[kept])), "kept_cells": int(kept.sum()),
            "synthetic_mates_kept_share": float(listed.mean()),
            "synthetic_rank_1_mates_still_rank_1_share": float((pos["n_before"][first] == 0).mean()) if first.any() else None,
        }
    m.free_queries(h); m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--keep", type=int, nargs="+", default=[100, 1000, 4096])
    ap.add_argument("--workloads", nargs="+", default=["headline", "structured"], choices=sorted(S.WORKLOADS))
    ap.add_argument("--reps", type=int, default=3, help="kept repetitions (one more is run first and discarded)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_search_timing.json"), help="where the JSON document goes ('' = stdout only)")
    a = ap.parse_args()
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    if "structured" in a.workloads:                                         # the structured generator draws on the GPU through torch: torch opens the device first, as in bench.py
        import torch
        torch.zeros(1, device=torch.device("cuda", 0))
    probe = M.Matcher(cbb)
    out = {"queries": a.queries, "gallery": a.gallery, "reps": a.reps, "interleaved": True, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "device": probe.device_info(0), "cascade_pairs_per_launch": probe.get_option("cascade_pairs_per_launch"),
           "clocks": {"*_host_ms": "host: perf_counter around the C call, which returns after its wait; no matrix or list crosses to the host",
                      "cascade_device_us": "device: options cascade_stage1_us + cascade_select_us + cascade_stage2_us, each from its own pair of HIP events",
                      "full_device_ms": "device: afis_timing.total_ms of afis_search_resident(k = 0), the yardstick"},
           "mates": "planted by the synthetic generator: the shares are facts about this synthetic data", "workloads": {}}
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
