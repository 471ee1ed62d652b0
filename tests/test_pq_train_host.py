"""Codebook training without a GPU: the numpy model of afis_pq_train's step (tests/pq_train_model.py) against the reference's own routine, scipy's kmeans2, STEP BY
STEP; the point sampler (csrc/pq_train_plan.h) through the stand-alone program csrc/pq_train_plan_check, built with the host sanitizers and run as a program
(nothing is loaded into this process), and against the model's restatement of the generator; afis_pq_train_init_points and afis_codebook_write, which need no
device; the model's early-stop property; the entry points declared, exported, bound and built.  What the device computes is tests/test_gpu_pq_train.py's."""
import importlib
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import pq_train_model as model

M = importlib.import_module("msu-latentafis_amd.host.matcher")
T = importlib.import_module("msu-latentafis_amd.host.templates")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NAMES = {"afis_pq_train": 9, "afis_pq_train_init_points": 4, "afis_codebook_write": 7}


def test_the_entry_points_are_declared_exported_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+afis_pq_train\s*\(int device_id,\s*const float\*\s*des\s*,\s*int64_t n,\s*const float\*\s*init\s*,\s*int iters,\s*float\*\s*codewords\s*,"
                     r"\s*int64_t\*\s*counts\s*,\s*int64_t\*\s*changed\s*,\s*int\*\s*iters_run\s*\)\s*;", code)
    assert re.search(r"\bint\s+afis_pq_train_init_points\s*\(const float\*\s*des\s*,\s*int64_t n,\s*uint64_t seed,\s*float\*\s*init\s*\)\s*;", code)
    assert re.search(r"\bint\s+afis_codebook_write\s*\(const float\*\s*codewords,\s*int M,\s*int K,\s*int dsub,\s*void\*\s*out,\s*size_t out_cap,\s*size_t\*\s*out_len\)\s*;", code)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        for name, n_args in NAMES.items():
            assert name in M.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args
    assert all(callable(getattr(M, f)) for f in ("pq_train", "pq_train_init_points", "codebook_bytes"))
    for word in ("Not in this interface", "k-means++", "sharded", "resident gallery", "missing='warn'", "rint", "1073741824.0", "Fisher-Yates", "0x9E3779B97F4A7C15"):
        assert word in hdr, word
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "pq_train.o" in objs and "afis_train.o" in objs
    everything = re.search(r"^all:(.*)$", mk, flags=re.M).group(1).split()
    cleaned = mk[mk.index("\nclean:"):]
    for prog in ("pq_train", "pq_train_plan_check"):
        assert prog in everything and re.search(r"\b%s\b" % prog, cleaned)
    # ONE definition of the assignment: both kernels' units include it, and neither spells the expansion out again
    for unit in ("pq_encode.hip", "pq_train.hip"):
        src = open(os.path.join(CSRC, unit)).read()
        assert '#include "pq_nearest.h"' in src and "pq_nearest(" in src and "dist < best" not in src
    assert re.search(r"^pq_train\.o:.*pq_nearest\.h", mk, flags=re.M) and re.search(r"^pq_encode\.o:.*pq_nearest\.h", mk, flags=re.M)
    rule = mk[mk.index("\npq_train.o:"):]
    assert rule.split("\n")[2].strip() == "$(HIPCC) $(HIPFLAGS) -c $< -o $@"                       # compiled as pq_encode.o is: no flag of its own, no fast-math
    assert "fast-math" not in mk and "-ffp-contract=off" in re.search(r"^CXXFLAGS\s*=(.*)$", mk, flags=re.M).group(1)


# ---- (a) the model against scipy's kmeans2, one step at a time ----------------------------------------------------------------------------------------
def test_every_step_of_the_model_is_a_kmeans2_step(oracle):
    """n = 20 000 points of one 6-d sub-space, 40 Gaussian blobs of sigma 0.3 around centres of sigma 0.4, init = 256 of the points with one codeword duplicated, 20
    steps.  From the model's current codebook, kmeans2(x64, C64, iter=1, minit='matrix') — the reference's routine, descriptor_PQ.py:73 — must give the same label
    for all but at most 1 in 10 000 points per step (the fp32 expansion and fp64 differ at near-ties only), and for every cluster of identical membership each
    component of the model's codeword must lie within 2^-24 |mean| + 2^-31 of scipy's fp64 mean: the fp32 rounding of the result plus the fixed-point resolution of
    q (each point's q is off by at most 2^-31, hence so is their mean; the fp64 operations contribute below 2^-50).  A 20-step run is NOT compared end to end: one
    flipped label diverges chaotically.  Measured with scipy 1.15.3: 0 differing labels over the 20 steps, worst error 0.984 of the bound; the
    duplicate's cluster is empty in step 0 and alive from step 1 on."""
    vq = pytest.importorskip("scipy.cluster.vq")
    rng = np.random.default_rng(2024)
    n = 20000
    x = model.clustered(rng, n)[:, :6].copy()
    cw = x[rng.choice(n, 256, replace=False)].copy()
    cw[200] = cw[17]                                                        # one codeword twice: the later copy's cluster starts empty
    init = cw.copy()
    x64 = x.astype(np.float64)
    worst, differing, alive = 0.0, 0, []
    for t in range(20):
        new, labels, count = model.step6(oracle, cw, x)
        assert count.sum() == n
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                 # missing='warn': an empty cluster keeps its codeword, with a warning
            ref_cw, ref_lab = vq.kmeans2(x64, cw.astype(np.float64), iter=1, minit="matrix")
        diff = labels != ref_lab
        differing += int(diff.sum())
        assert diff.sum() * 10000 <= n, (t, int(diff.sum()))
        same = np.ones(256, bool)
        same[labels[diff]] = False; same[ref_lab[diff]] = False             # clusters whose membership differs are not compared
        full, empty = same & (count > 0), same & (count == 0)
        err = np.abs(new.astype(np.float64) - ref_cw)[full]
        bound = (2.0 ** -24 * np.abs(ref_cw) + 2.0 ** -31)[full]
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (t, float((err / bound).max()))
        assert np.array_equal(new[empty].view(np.uint32), cw[empty].view(np.uint32)) and np.array_equal(ref_cw[empty], cw[empty].astype(np.float64))
        alive.append(bool(count[200] > 0))
        cw = new
    print("PQ_TRAIN_MODEL_VS_KMEANS2 differing labels %d, worst error %.3f of the bound, the twin's cluster alive in steps %s" % (differing, worst, [t for t, a in enumerate(alive) if a]))
    assert not alive[0] and np.array_equal(model.step6(oracle, init, x)[0][200].view(np.uint32), init[200].view(np.uint32))       # empty in step 0: the twin keeps its bits


def test_the_96d_step_is_sixteen_independent_6d_steps(oracle):
    rng = np.random.default_rng(5)
    des = model.clustered(rng, 700)
    des[100:140] = des[3]                                                   # equal rows (assign encodes them once)
    init = model.init_points(des, 11)
    new, labels, count = model.step(oracle, init, des)
    for m in (0, 9, 15):
        n6, l6, c6 = model.step6(oracle, init[m], des[:, 6 * m:6 * m + 6])
        assert np.array_equal(n6.view(np.uint32), new[m].view(np.uint32)) and np.array_equal(l6, labels[:, m]) and np.array_equal(c6, count[m])


# ---- (b) the sampler ----------------------------------------------------------------------------------------------------------------------------------
def _check_program():
    exe = os.path.join(CSRC, "pq_train_plan_check")
    src = [os.path.join(CSRC, f) for f in ("pq_train_plan_check.cpp", "pq_train_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in src):
        subprocess.run(["make", "-s", "-C", CSRC, "pq_train_plan_check"], check=True)
    return exe


def test_pq_train_plan_check_runs_clean_under_the_host_sanitizers():
    exe = _check_program()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("\npq_train_plan_check:"):]
    assert "-fsanitize=address,undefined" in rule[:rule.index("\n\n")] and "-fno-sanitize-recover=undefined" in rule[:rule.index("\n\n")]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"pq_train_plan_check: \d+ cases ok", out.stdout), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert int(re.search(r"(\d+) cases ok", out.stdout).group(1)) >= 600
    hdr = open(os.path.join(CSRC, "pq_train_plan.h")).read()
    assert not re.search(r'#include\s*[<"](hip|afis_)', hdr)                  # device-free


@pytest.mark.parametrize("n, seed", [(256, 0), (257, 1), (5000, 7), (1 << 26, 2 ** 64 - 1)])
def test_the_sampler_is_the_generator_the_header_states(n, seed):
    """The program's indices, the model's restatement on Python integers, and (where the points fit) afis_pq_train_init_points agree; distinct, in range."""
    out = subprocess.run([_check_program(), str(n), str(seed)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(got) == 16 and got == [model.init_indices(n, seed, m) for m in range(16)]
    for row in got:
        assert len(set(row)) == 256 and 0 <= min(row) and max(row) < n
    assert len({tuple(r) for r in got}) == 16                              # every sub-quantizer draws its own
    if n <= 5000:
        des = np.random.default_rng(n).standard_normal((n, 96)).astype(np.float32)
        init = M.pq_train_init_points(des, seed)
        assert np.array_equal(init.view(np.uint32), model.init_points(des, seed).view(np.uint32))
        assert np.array_equal(M.pq_train_init_points(des, seed), init) and not np.array_equal(M.pq_train_init_points(des, seed + 1 & model.MASK), init)


def test_init_points_refuses_fewer_than_256_points():
    des = np.zeros((255, 96), np.float32)
    with pytest.raises(M.AfisError, match=r"\(-1\).*fewer than 256"):
        M.pq_train_init_points(des, 0)


# ---- (c) afis_codebook_write -----------------------------------------------------------------------------------------------------------------------------
def test_codebook_write_round_trips_through_the_parser(codebook_bytes):
    import ctypes as C
    cb = T.Codebook.from_bytes(codebook_bytes)
    words = np.ascontiguousarray(cb.words, np.float32).reshape(16, 256, 6)
    assert M.codebook_bytes(words) == codebook_bytes == model.codebook_file(words)       # the shipped file, byte for byte
    rng = np.random.default_rng(9)
    w = rng.standard_normal((16, 256, 6)).astype(np.float32)
    w.view(np.uint32)[0, 0, :3] = [0x7FC00001, 0x80000000, 0x00000001]      # bits travel as they are: a NaN payload, -0.0, a denormal
    back = T.Codebook.from_bytes(M.codebook_bytes(w))
    assert (back.M, back.K, back.dsub) == (16, 256, 6) and np.array_equal(np.asarray(back.words, np.float32).reshape(16, 256, 6).view(np.uint32), w.view(np.uint32))
    lib = M.load_library()
    need = C.c_size_t(0); fp = w.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.afis_codebook_write(fp, 16, 256, 6, None, 0, C.byref(need)) == 0 and need.value == 6 + 16 * 256 * 6 * 4
    buf = C.create_string_buffer(b"\x5a" * need.value, need.value)
    assert lib.afis_codebook_write(fp, 16, 256, 6, buf, need.value - 1, C.byref(need)) == -1 and buf.raw == b"\x5a" * need.value       # too small: AFIS_EINVAL, untouched
    assert lib.afis_codebook_write(fp, 16, 256, 8, buf, need.value, C.byref(need)) == -1 and b"geometry" in lib.afis_last_error(None)
    assert lib.afis_codebook_write(None, 16, 256, 6, buf, need.value, C.byref(need)) == -1
    with pytest.raises(M.AfisError):
        M.codebook_bytes(np.zeros((16, 256, 8), np.float32))


# ---- (d) the early stop ----------------------------------------------------------------------------------------------------------------------------------
def test_the_models_early_stop_changes_no_output(oracle):
    """A set that reaches changed == 0: stopping there gives what running on gives — codewords, counts, and zeros in the rest of `changed`."""
    rng = np.random.default_rng(77)
    des = model.clustered(rng, 1200, blobs=12, sigma=0.05)
    init = model.init_points(des, 3)
    a = model.train(oracle, des, init, 200)
    assert 2 <= a["iters_run"] < 200 and a["changed"][0] == 16 * len(des) and a["changed"][a["iters_run"] - 1] == 0 and (a["changed"][a["iters_run"]:] == 0).all()
    assert (a["changed"][:a["iters_run"] - 1] > 0).all()
    b = model.train(oracle, des, init, a["iters_run"] + 3, early_stop=False)
    assert b["iters_run"] == a["iters_run"] + 3 and np.array_equal(b["changed"][:a["iters_run"]], a["changed"][:a["iters_run"]]) and (b["changed"][a["iters_run"]:] == 0).all()
    assert np.array_equal(a["codewords"].view(np.uint32), b["codewords"].view(np.uint32)) and np.array_equal(a["counts"], b["counts"])
    c = model.train(oracle, des, init, a["iters_run"])
    assert c["iters_run"] == a["iters_run"] and np.array_equal(a["codewords"].view(np.uint32), c["codewords"].view(np.uint32)) and np.array_equal(a["counts"], c["counts"])
    assert a["counts"].sum(axis=1).tolist() == [len(des)] * 16
    z = model.train(oracle, des, init, 0)
    assert z["iters_run"] == 0 and np.array_equal(z["codewords"].view(np.uint32), init.view(np.uint32)) and not z["counts"].any()
