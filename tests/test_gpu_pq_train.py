"""Codebook training on the device: afis_pq_train (csrc/pq_train.hip, afis_train.cpp) through the C ABI and the Python host against the numpy model of its
definition (tests/pq_train_model.py: the oracle's encoder, int64 sums of rint(x 2^30), one fp64 division) BIT FOR BIT — codewords as uint32, counts, changed,
iters_run — at the step kernel's tile remainders, on a clustered set, at ties, at the halves of the fixed-point rounding, beyond what a double could sum, to a fixed
point, at every refusal, and through the pq_train CLI; a search on the shipped codebook returns the same bytes before and after a training call."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import pq_train_model as model

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")


def _same(got, want, what=""):
    assert got["iters_run"] == want["iters_run"], (what, got["iters_run"], want["iters_run"])
    assert np.array_equal(got["changed"], want["changed"]), (what, got["changed"], want["changed"])
    assert np.array_equal(got["counts"], want["counts"]), (what, np.argwhere(got["counts"] != want["counts"])[:6].tolist())
    g, w = got["codewords"].view(np.uint32), want["codewords"].view(np.uint32)
    assert np.array_equal(g, w), (what, np.argwhere(g != w)[:6].tolist())


def _far_init(rng):
    """An init not drawn from the points: most of its clusters stay empty and must keep these bits."""
    return (rng.standard_normal((16, 256, 6)) * 0.5).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256 * 64 + 1])
def test_tile_remainders(n, oracle):
    """One point, either side of a wave, and one point past a full pass of the step grid (64 workgroups of 256 points per sub-quantizer); 3 steps."""
    rng = np.random.default_rng(100 + n)
    des = (rng.standard_normal((n, 96)) * 0.45).astype(np.float32)
    init = _far_init(rng)
    got = M.pq_train(des, init, iters=3)
    want = model.train(oracle, des, init, 3)
    _same(got, want, n)
    if n <= 65:
        one = M.pq_train(des, init, iters=1)                                # after one step an empty cluster holds init's bits
        kept = one["counts"] == 0
        assert kept.sum() >= 16 * (256 - n) and np.array_equal(one["codewords"].view(np.uint32)[kept], init.view(np.uint32)[kept])


@pytest.fixture(scope="module")
def clustered_set(oracle):
    rng = np.random.default_rng(31)
    des = model.clustered(rng, 5000)
    init = model.init_points(des, 12345)
    return des, init, model.train(oracle, des, init, 20)


def test_clustered_set_twenty_steps(clustered_set):
    des, init, want = clustered_set
    assert np.array_equal(M.pq_train_init_points(des, 12345).view(np.uint32), init.view(np.uint32))
    got = M.pq_train(des, M.pq_train_init_points(des, 12345), iters=20)
    _same(got, want)
    assert got["changed"][0] == 16 * 5000 and (got["counts"].sum(axis=1) == 5000).all()


def _write_training_dir(rng, path, sizes):
    """Templates in the latent on-disk layout with fp32 texture descriptors; returns the points the CLI's defaults take (every 2nd of templates of 100 or more)."""
    taken = []
    for i, n in enumerate(sizes):
        filler = S.make_latent(rng, n_tex_lo=10, n_tex_hi=10)
        tex = []
        if n is not None:
            des = model.clustered(rng, n, blobs=9, sigma=0.1)
            x = (np.arange(n) % 45).astype(np.int16); y = (np.arange(n) // 45 % 47).astype(np.int16)
            tex = [T.TextureTemplate(x, y, np.linspace(-1.5, 1.5, n).astype(np.float32), des=des)]
            if n >= 100:
                taken.append(des[::2])
        (path / ("t%02d.dat" % (len(sizes) - i))).write_bytes(T.write_latent(T.FPTemplate(minu=filler.minu[:1], tex=tex)))       # names in descending order of creation
    return np.concatenate(taken[::-1])                                         # the CLI reads in name order


def test_the_cli_and_python_give_the_same_codebook(oracle, tmp_path):
    exe = os.path.join(os.path.dirname(M.LIB_PATH), "pq_train")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(M.LIB_PATH), "pq_train"], check=True)
    rng = np.random.default_rng(8)
    (tmp_path / "in").mkdir()
    des = _write_training_dir(rng, tmp_path / "in", [400, 99, 641, None, 100, 333])
    assert len(des) == 200 + 321 + 50 + 167
    out = subprocess.run([exe, "--input_dir", str(tmp_path / "in") + "/", "--output", str(tmp_path / "cb.dat"), "--iters", "6", "--seed", "77"], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    got = M.pq_train(des, M.pq_train_init_points(des, 77), iters=6)
    assert (tmp_path / "cb.dat").read_bytes() == M.codebook_bytes(got["codewords"])
    _same(got, model.train(oracle, des, model.init_points(des, 77), 6))
    lines = out.stdout.splitlines()
    assert lines[:got["iters_run"]] == ["step %d: changed %d" % (t, got["changed"][t]) for t in range(got["iters_run"])]
    assert lines[-1].startswith("pq_train: %d points of 4 templates, %d steps run, %d empty clusters" % (len(des), got["iters_run"], int((got["counts"] == 0).sum())))
    few = subprocess.run([exe, "--input_dir", str(tmp_path / "in") + "/", "--output", str(tmp_path / "none.dat"), "--min_points", "500", "--stride", "3"], capture_output=True, text=True)
    assert few.returncode == 2 and "fewer than 256" in few.stderr and not (tmp_path / "none.dat").exists()       # 214 points of one template


def test_ties(oracle):
    """Duplicated codewords (the first minimum wins, the twin stays empty and keeps its bits), duplicated points, and points exactly between two codewords."""
    rng = np.random.default_rng(55)
    des = (rng.integers(-8, 9, (900, 96)) * 0.125).astype(np.float32)       # a coarse grid: many equal points, many exact ties
    des[300:600] = des[:300]
    init = (rng.integers(-8, 9, (16, 256, 6)) * 0.125).astype(np.float32)
    init[:, 0] = 0.0; init[:, 1] = 0.0; init[:, 1, 0] = 0.25                # codewords 0 and 1 differ in one component ...
    init[:, 128:] = init[:, :128]                                           # every codeword twice
    des[:40] = 0.0; des[:40, 0::6] = 0.125                                  # ... and these points lie exactly between them in every sub-space: the first wins
    got = M.pq_train(des, init, iters=4)
    _same(got, model.train(oracle, des, init, 4))
    first = model.assign(oracle, init, des)
    assert (first < 128).all() and (first[:40] == 0).all()
    one = M.pq_train(des, init, iters=1)
    assert not one["counts"][:, 128:].any() and np.array_equal(one["codewords"][:, 128:].view(np.uint32), init[:, 128:].view(np.uint32))


def test_rounding_of_q(oracle):
    """Components at the halves of the fixed point — 2^-31 and 3 2^-31 round to 0 and 2 (nearest even) — their negatives, denormals, and +-64 exactly, in rows
    of one value (beside a codeword at that value) and mixed at random."""
    h = np.float32(2.0 ** -31)
    vals = np.array([h, 3 * h, -h, -3 * h, 5 * h, -5 * h, np.float32(1e-40), np.float32(-1e-40), 64.0, -64.0, 2.0 ** -30, 1.0 + 2.0 ** -23, 0.0, -0.0], np.float32)
    rng = np.random.default_rng(66)
    des = vals[rng.integers(0, len(vals), (700, 96))]
    des[:len(vals)] = vals[:, None]                                         # rows of one value each
    init = np.zeros((16, 256, 6), np.float32)
    init[:, :len(vals)] = vals[None, :, None]                               # a codeword at every value
    init[:, len(vals):] = 100.0
    got = M.pq_train(des, init, iters=2)
    want = model.train(oracle, des, init, 2)
    _same(got, want)
    S6, c6 = model.accumulate6(np.repeat(vals[:4, None], 6, axis=1), np.arange(4))
    assert S6[:4, 0].tolist() == [0, 2, 0, -2] and c6[:4].tolist() == [1, 1, 1, 1]
    two = M.pq_train(des[:4], init, iters=1)                                # the four halves alone: means 0, 2^-29, -0 -> +0 (an integer zero has no sign), -2^-29
    assert two["codewords"][0, :4, 0].view(np.uint32).tolist() == np.array([0.0, 2.0 ** -29, 0.0, -2.0 ** -29], np.float32).view(np.uint32).tolist()


def test_sums_are_int64_not_fp64(oracle):
    """200 000 points whose first sub-vector is about +-63.99 (sign by component) with odd low mantissa bits, and a handful of components of a few 2^-30, all in one
    cluster: |S| > 2^53 with low bits set — a sum kept in a double would lose what the model keeps."""
    rng = np.random.default_rng(77)
    pool = np.zeros((512, 96), np.float32)
    sign = np.array([1, -1, 1, -1, 1, -1], np.float32)
    big = (np.float32(63.99) + rng.integers(0, 64, (512, 6)).astype(np.float32) * np.float32(2.0 ** -18)).astype(np.float32)
    big.view(np.uint32)[...] |= 1                                           # odd mantissas (ulp 2^-18 in [32, 64))
    pool[:, :6] = big * sign
    pool[:, 6:] = (rng.standard_normal((512, 90)) * 0.4).astype(np.float32)
    des = pool[rng.integers(0, 512, 200000)]
    tiny = np.zeros((37, 96), np.float32)
    tiny[:, :6] = (rng.integers(1, 8, (37, 6)) * 2 + 1).astype(np.float32) * np.float32(2.0 ** -30) * sign
    des = np.concatenate([des, tiny])
    init = _far_init(rng)
    init[0, :, :] = -100.0 * sign; init[0, 0] = 50.0 * sign                 # sub-quantizer 0: codeword 0 takes every point, the tiny ones too
    S6, c6 = model.accumulate6(des[:, :6], np.zeros(len(des), np.int64))
    assert (np.abs(S6[0]) > 2 ** 53).all() and any(int(float(int(v))) != int(v) for v in S6[0])        # not representable in a double
    got = M.pq_train(des, init, iters=2)
    want = model.train(oracle, des, init, 2)
    _same(got, want)
    assert got["counts"][0, 0] == len(des)


def test_fixed_point_stops_early_and_ties_to_the_encoder(oracle):
    rng = np.random.default_rng(88)
    des = model.clustered(rng, 2000, blobs=12, sigma=0.05)
    init = M.pq_train_init_points(des, 4)
    got = M.pq_train(des, init, iters=200)
    r = got["iters_run"]
    assert 2 <= r < 200 and got["changed"][r - 1] == 0 and (got["changed"][:r - 1] > 0).all() and (got["changed"][r:] == 0).all() and len(got["changed"]) == 200
    again = M.pq_train(des, init, iters=r)
    assert again["iters_run"] == r and np.array_equal(again["changed"], got["changed"][:r]) and np.array_equal(again["counts"], got["counts"])
    assert np.array_equal(again["codewords"].view(np.uint32), got["codewords"].view(np.uint32))
    _same(got, model.train(oracle, des, init, 200))
    m = M.Matcher(M.codebook_bytes(got["codewords"]))                       # the product encoder under the trained codebook: at a fixed point its codes ARE the last labels
    codes = m.pq_encode(des)
    m.close()
    hist = np.stack([np.bincount(codes[:, j], minlength=256) for j in range(16)])
    assert np.array_equal(hist, got["counts"])


def _raw_train(lib, des, n, init, iters, poison=0x5A):
    cw = np.full((16, 256, 6), np.float32(7.25)); counts = np.full((16, 256), poison, np.int64); changed = np.full(max(iters, 1) if iters <= 1000 else 8, poison, np.int64)
    run = C.c_int32(poison)
    fp, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    rc = lib.afis_pq_train(0, des.ctypes.data_as(fp), n, init.ctypes.data_as(fp), iters, cw.ctypes.data_as(fp), counts.ctypes.data_as(i64p), changed.ctypes.data_as(i64p), C.byref(run))
    untouched = (cw == np.float32(7.25)).all() and (counts == poison).all() and (changed == poison).all() and run.value == poison
    return rc, untouched, cw, counts, changed, run.value


def test_refusals_leave_the_outputs_untouched():
    lib = M.load_library()
    rng = np.random.default_rng(99)
    des = (rng.standard_normal((300, 96)) * 0.4).astype(np.float32)
    init = _far_init(rng)
    for what, value in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf), ("64.001", 64.001), ("-64.001", -64.001)):
        bad = des.copy(); bad[299, 95] = value
        rc, untouched = _raw_train(lib, bad, 300, init, 3)[:2]
        assert rc == -1 and untouched, what
        assert b"64" in lib.afis_last_error(None)
    for iters in (-1, 1001):
        rc, untouched = _raw_train(lib, des, 300, init, iters)[:2]
        assert rc == -1 and untouched, iters
    rc, untouched = _raw_train(lib, des, -1, init, 3)[:2]
    assert rc == -1 and untouched
    bad_init = init.copy(); bad_init[15, 255, 5] = np.inf
    rc, untouched = _raw_train(lib, des, 300, bad_init, 3)[:2]
    assert rc == -1 and untouched
    ok = des.copy(); ok[0, 0] = 64.0; ok[1, 1] = -64.0                      # the limit itself is inside the range
    assert _raw_train(lib, ok, 300, init, 1)[0] == 0
    with pytest.raises(M.AfisError, match=r"\(-1\)"):
        M.pq_train_init_points(des[:255], 0)
    for n, iters in ((0, 5), (300, 0)):                                     # nothing to do: init's bits, zero counts, zero steps
        rc, _, cw, counts, changed, run = _raw_train(lib, des, n, init, iters)
        assert rc == 0 and run == 0 and np.array_equal(cw.view(np.uint32), init.view(np.uint32)) and not counts.any()
        assert not changed[:iters].any()
    assert lib.afis_pq_train(99, des.ctypes.data_as(C.POINTER(C.c_float)), 300, init.ctypes.data_as(C.POINTER(C.c_float)), 1, init.ctypes.data_as(C.POINTER(C.c_float)), None, None, None) == -1


def test_a_training_call_leaves_the_search_unchanged(codebook_bytes):
    cb = T.Codebook.from_bytes(codebook_bytes)
    lats, gal = cases.small_set(cb, seed=3, n_lat=2, n_gal=12)
    m = M.Matcher(codebook_bytes)
    m.gallery_add(gal); m.gallery_commit(0)
    before = m.search(lats, k=5, want_parts=True)
    des = model.clustered(np.random.default_rng(1), 3000)
    M.pq_train(des, M.pq_train_init_points(des, 0), iters=3)
    after = m.search(lats, k=5, want_parts=True)
    for key in ("scores", "parts", "topk_idx", "topk_score"):
        assert before[key].tobytes() == after[key].tobytes(), key
    m.close()
