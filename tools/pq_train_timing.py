#!/usr/bin/env python
"""What codebook training costs (afis_pq_train), on one MI355X: 10^6 clustered points x 20 steps by default.  The comparisons are interleaved, `--reps` + 1 rounds
each, the first round discarded; medians with the spread (max - min) beside them.

  (a) afis_pq_train on the HOST's clock (perf_counter around the call: upload, first pass, steps, the host's divisions), with the device time of the first pass and
      of every step (HIP events inside the call, printed by the library under AFIS_TRAIN_TRACE and parsed here) — against the only route there was before it:
      scipy's kmeans2 per sub-space (extraction/descriptor_PQ.py:71-73) on this machine's CPUs, the 16 sub-spaces on at most 16 threads, `--kmeans2-runs` times
      (one by default: it takes minutes; `--kmeans2-steps k` runs k of the iterations and scales); without scipy the comparison is the numpy model of tests/pq_train_model.py, named as such.
  (b) one step against the encoder at the same n: afis_pq_encode host to host (tools/bench_encode.py's workload) beside the step's device time; with
      `--kernel-stats <csv>` (tools/rocprof_summary.py over a rocprofv3 --kernel-trace --stats run of `--kernels-only`: one encode and one 3-step training) the kernels' own times —
      k_pq_encode, k_train_step, k_train_transpose — and the ratio step / encoder.

Recorded, not asserted.  One JSON document on stdout and in --out."""
import argparse, csv, importlib, json, os, re, socket, statistics, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["AFIS_TRAIN_TRACE"] = "1"                                        # read once by the library: set before it is loaded
M = importlib.import_module("msu-latentafis_amd.host.matcher")
import pq_train_model as model                                              # noqa: E402  (the clustered set's generator, and the stand-in comparison)


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": list(v)}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def traced_train(des, init, iters):
    """(result, host seconds, first-pass device ms, [step device ms]): the library's trace lines are taken from stderr for the length of the call."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            r = M.pq_train(des, init, iters=iters)
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2); os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    first = [float(x) for x in re.findall(r"first pass ([0-9.]+) ms", text)]
    steps = [float(x) for x in re.findall(r"step \d+ device ([0-9.]+) ms", text)]
    return r, dt, first[0] if first else None, steps


def kmeans2_route(des, init, iters, threads):
    from scipy.cluster.vq import kmeans2
    import warnings

    def one(m):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return kmeans2(des[:, 6 * m:6 * m + 6].astype(np.float64), init[m].astype(np.float64), iter=iters, minit="matrix")[0]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, range(16)))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kmeans2-runs", type=int, default=1)
    ap.add_argument("--kmeans2-steps", type=int, default=0, help="run kmeans2 with this many iterations and scale the time to --steps (0: run all of them)")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pq_train_timing.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    des = model.clustered(rng, a.points)
    init = M.pq_train_init_points(des, 0)
    cbb = open(os.path.join(ROOT, "tests", "golden", "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"), "rb").read()
    m = M.Matcher(cbb)
    if a.kernels_only:
        m.pq_encode(des); M.pq_train(des, init, iters=3); m.close()
        return
    train_s, first_ms, step_ms, enc_s, iters_run = [], [], [], [], None
    for rep in range(a.reps + 1):
        r, dt, first, steps = traced_train(des, init, a.steps)
        t0 = time.perf_counter(); m.pq_encode(des); de = time.perf_counter() - t0
        note("round %d: afis_pq_train %.3f s (%d steps, first pass %.1f ms, step median %.3f ms), afis_pq_encode %.3f s" % (rep, dt, r["iters_run"], first, statistics.median(steps), de))
        if rep:
            train_s.append(dt); first_ms.append(first); step_ms.append(statistics.median(steps)); enc_s.append(de)
        iters_run = r["iters_run"]
    m.close()
    doc = {"host": socket.gethostname(), "points": a.points, "steps": a.steps, "iters_run": iters_run, "reps": a.reps,
           "set": "tests/pq_train_model.py::clustered (40 blobs of sigma 0.3 per sub-space), init afis_pq_train_init_points seed 0",
           "a": {"afis_pq_train_host_s": med(train_s), "first_pass_device_ms": med(first_ms), "step_device_ms": med(step_ms),
                 "empty_clusters": int((r["counts"] == 0).sum())},
           "b": {"afis_pq_encode_host_to_host_s": med(enc_s)}}
    try:
        import scipy
        ks = a.kmeans2_steps or a.steps
        measured = [kmeans2_route(des, init, ks, a.threads) for _ in range(a.kmeans2_runs)]
        runs = [t * a.steps / ks for t in measured]                          # kmeans2's iterations are alike: vq over every point, then the means
        doc["a"]["before"] = {"route": "scipy %s kmeans2(iter=%d, minit='matrix') per sub-space, %d threads" % (scipy.__version__, ks, a.threads), "host_s": med(runs),
                              "measured_s": measured, "scaled": "measured at iter=%d and scaled by %d/%d" % (ks, a.steps, ks) if ks != a.steps else "no"}
    except ImportError:
        from oracle_lib import Oracle
        orc = Oracle(); sub = des[:20000]
        t0 = time.perf_counter(); model.train(orc, sub, init, 2, early_stop=False); dt = (time.perf_counter() - t0) / 2 / len(sub) * a.points * a.steps
        doc["a"]["before"] = {"route": "the numpy model of tests/pq_train_model.py (scipy is not importable), extrapolated from 2 steps over 20 000 points", "host_s": med([dt])}
    doc["a"]["speedup_host_clock"] = doc["a"]["before"]["host_s"]["median"] / doc["a"]["afis_pq_train_host_s"]["median"]
    if a.kernel_stats:
        k = {}
        for row in csv.DictReader(open(a.kernel_stats)):
            for want in ("k_pq_encode", "k_train_step", "k_train_transpose"):       # tools/rocprof_summary.py's columns
                if want in row["kernel"]:
                    k[want] = {"calls": int(row["calls"]), "average_us": float(row["avg_ms"]) * 1e3, "total_us": float(row["total_ms"]) * 1e3}
        doc["b"]["kernels"] = k
        if "k_pq_encode" in k and "k_train_step" in k:
            doc["b"]["step_over_encoder"] = k["k_train_step"]["average_us"] / k["k_pq_encode"]["total_us"]
    s = json.dumps(doc, indent=1)
    print(s)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
