#!/usr/bin/env python
"""What replacing enrolled prints in place costs (afis_gallery_commit_at), on one MI355X: N templates of a shard of G replaced in one call, against the only way there was
before — afis_gallery_remove of the same N entries followed by an appending commit of the same N templates (which gives other indices: a yardstick for time only).

Every repetition builds its two contexts anew (a commit of the G templates and --settle seconds of rest, outside the timing); the two kinds are interleaved in one process (replace, pair, replace,
...), one warm-up repetition of each is discarded, and the medians of the wall time per TRANSACTION — staging included: reopen + add_packed + commit_at against
remove + reopen + add_packed + commit — are reported with every repetition.  The replace runs on the test library, whose tap afis_debug_compact_stats reports the splice
kernels' device time (HIP events around each of the six launches) and the bytes they wrote; the pair's removal reports its compaction kernels the same way.

--laps: one more repetition of each kind with AFIS_COMMIT_TIMING set; the library writes where the time went to stderr (each lap synchronises: not a timed repetition).

One JSON document on stdout (and to --out)."""
import argparse, hashlib, importlib, json, os, socket, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")
T = importlib.import_module("msu-latentafis_amd.host.templates")


def timed(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=10000)
    ap.add_argument("--edit", type=int, default=500, help="templates replaced")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--settle", type=float, default=0.5, help="seconds between a context's commit and its timed transaction")
    ap.add_argument("--laps", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    G, N = a.gallery, a.edit
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    cb = T.Codebook.from_bytes(cbb)
    gal = S.make_packed_gallery(a.seed, G + N, cb)
    A, B = gal.slice(0, G), gal.slice(G, G + N)
    idx = np.random.default_rng(a.seed + 1).permutation(G)[:N].astype(np.int64)
    out = {"gallery": G, "replaced": N, "reps_kept": a.reps, "settle_s": a.settle, "host": hashlib.sha256(socket.gethostname().encode()).hexdigest()[:12],
           "resident_bytes": int(A.minu_off[-1]) * 392 + int(A.tex_off[-1]) * 24, "staged_bytes": int(B.minu_off[-1]) * 392 + int(B.tex_off[-1]) * 24}

    def committed():
        m = M.Matcher(cbb, taps=True); m.gallery_add_packed(A); m.gallery_commit(0)
        # the commit hands its staging copy (50 KB per template) to a thread that returns the pages to the system while the caller goes on — 50 ms for this shard, during
        # which every allocation of the process waits for the address-space lock now and then.  An edit arrives at a shard that has been resident for a while: let it finish.
        time.sleep(a.settle)
        return m

    def do_replace(m):
        m.gallery_reopen(); m.gallery_add_packed(B); m.gallery_commit_at(idx)

    def do_pair(m):
        m.gallery_remove(idx); m.gallery_reopen(); m.gallery_add_packed(B); m.gallery_commit(0)

    rows = []
    for rep in range(a.reps + 1):
        m = committed()
        if rep == 0:
            out["device"] = m.device_info(0)
        h0 = m.get_option("gallery_h2d_bytes")
        replace_ms = timed(lambda: do_replace(m))
        h2d = m.get_option("gallery_h2d_bytes") - h0
        splice_us, splice_bytes = m.compact_stats()
        m.close()
        m = committed()
        box = {}

        def pair():
            box["remove_ms"] = timed(lambda: m.gallery_remove(idx))
            box["compact"] = m.compact_stats()
            m.gallery_reopen(); m.gallery_add_packed(B); m.gallery_commit(0)
        pair_ms = timed(pair)
        m.close()
        rows.append({"rep": rep, "replace_ms": round(replace_ms, 2), "replace_h2d_bytes": int(h2d), "splice_us": int(splice_us), "splice_bytes": int(splice_bytes),
                     "pair_ms": round(pair_ms, 2), "pair_remove_ms": round(box["remove_ms"], 2), "pair_compact_us": int(box["compact"][0]), "pair_compact_bytes": int(box["compact"][1])})
    kept = rows[1:]
    med = lambda k: statistics.median(r[k] for r in kept)
    out["reps"] = rows
    out["median_replace_ms"] = med("replace_ms"); out["median_pair_ms"] = med("pair_ms")
    out["replace_over_pair"] = round(med("replace_ms") / med("pair_ms"), 3)
    out["median_splice_us"] = med("splice_us"); out["splice_bytes"] = kept[-1]["splice_bytes"]
    out["splice_gb_per_s"] = round(kept[-1]["splice_bytes"] / max(med("splice_us"), 1) / 1e3, 1)
    out["median_pair_compact_us"] = med("pair_compact_us")
    out["note"] = ("wall time per transaction, staging included, device idle at return; the first repetition of each kind is discarded; splice_us / pair_compact_us are device "
                   "times between HIP events around each of the six launches, summed; GB/s = bytes written / time (each byte is read once and written once)")
    if a.laps:
        os.environ["AFIS_COMMIT_TIMING"] = "1"
        m = committed(); do_replace(m); m.close()
        m = committed(); do_pair(m); m.close()
        del os.environ["AFIS_COMMIT_TIMING"]
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
