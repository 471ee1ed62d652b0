"""One rank-list order on the host paths, without a GPU: afis_rank_list, the exchange's merge_topk (match_selftest -selftest-merge) and the five merges of
host/sharding.py, on score rows whose bits no clean search produces — infinities, both zeros, quiet NaNs of both signs.

The yardstick is numpy: np.lexsort((global_index, -key.astype(np.int64))) with key = the ordered bits of score + 0.0f (tests/test_gpu_rank_hits.py::template_key; the
subject lists use the raw word, subject_key).  Indices and raw score words are compared with np.array_equal, padding included.  On NaN-free rows every changed function
must return what it returned before it compared keys: afis_rank_list(ref_order 1) is held against a restatement of the old statement built with g++
(rank_order_check -old-rank-list), the Python merges against their old bodies kept below.

csrc/rank_order_check is a stand-alone program built with -fsanitize=address,undefined: it is run as a program, nothing is loaded into this process."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import test_gpu_rank_hits as RH

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
SEED = 4211
SIZES = (0, 1, 2, 15, 16, 17, 1000, 5000)                                   # either side of libstdc++'s insertion-sort threshold of 16, and well past it
NAN_FREE = range(RH.ROW_SPECIAL)                                            # rows 0 .. 7 of RH.matrix
ROW_TWO_NANS = 9
NEG_INF_WORD = 0xff800000
QNAN, QNAN_NEG = 0x7fc00000, 0xffc00000


def rows_of(n, rng):
    """The nine kinds of tests/test_gpu_rank_hits.py::matrix and a tenth: finite values (small integers: many ties) except one 0x7fc00000 and one 0xffc00000 at random places."""
    rows = np.empty((10, n), np.float32)
    rows[:9] = RH.matrix(n, rng)
    rows[ROW_TWO_NANS] = rng.integers(-8, 32, n).astype(np.float32)
    w = rows[ROW_TWO_NANS].view(np.uint32)
    at = rng.permutation(n)[:2]
    for p, word in zip(at, (QNAN, QNAN_NEG)):
        w[p] = word
    return rows


def model_order(row, glob=None):
    glob = np.arange(len(row), dtype=np.int64) if glob is None else np.asarray(glob, np.int64)
    return np.lexsort((glob, -RH.template_key(row).astype(np.int64)))


def model_topk(row, glob, k):
    """(idx [k], score words [k]) of a row whose column j is template glob[j]; (-1, -inf) pads."""
    o = model_order(row, glob)[:k]
    idx = np.full(k, -1, np.int64); sc = np.full(k, NEG_INF_WORD, np.uint32)
    idx[:len(o)] = np.asarray(glob, np.int64)[o]; sc[:len(o)] = row.view(np.uint32)[o]
    return idx, sc


def tool(name):
    exe = os.path.join(CSRC, name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, name], check=True)
    return exe


@pytest.fixture(scope="module")
def lib():
    return M.load_library()                                                 # dlopen only: afis_rank_list does no device work


def rank_list(lib, row, ref_order):
    n = len(row)
    row = np.ascontiguousarray(row, np.float32)
    idx = np.full(max(n, 1), -7, np.int64); sc = np.zeros(max(n, 1), np.float32)
    rc = lib.afis_rank_list(row.ctypes.data_as(C.POINTER(C.c_float)) if n else None, C.c_int64(n), ref_order, n, idx.ctypes.data_as(C.POINTER(C.c_int64)), sc.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    return idx[:n], sc[:n].view(np.uint32)


def old_rank_list(exe, row, tmp_path):
    """The statement afis_rank_list(ref_order 1) made before: std::sort of 0 .. n-1 on scores[a] > scores[b], with g++'s libstdc++ (NaN-free rows only)."""
    f = tmp_path / "column.txt"
    f.write_text("%d\n" % len(row) + "".join("%08x\n" % w for w in row.view(np.uint32).tolist()))
    out = subprocess.run([exe, "-old-rank-list", str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return np.array(out.stdout.split(), np.int64)


# ---- 1: afis_rank_list ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_rank_list_on_every_row_kind(n, lib, tmp_path):
    exe = tool("rank_order_check")
    rows = rows_of(n, np.random.default_rng(SEED + n))
    for kind, row in enumerate(rows):
        words, key = row.view(np.uint32), RH.template_key(row).astype(np.int64)
        want = model_order(row)
        idx, sc = rank_list(lib, row, 0)
        assert np.array_equal(idx, want) and np.array_equal(sc, words[want]), (n, kind, "ref_order 0 is the model")
        idx, sc = rank_list(lib, row, 1)
        assert np.array_equal(np.sort(idx), np.arange(n)), (n, kind, "ref_order 1 is a permutation")
        assert (np.diff(key[idx]) <= 0).all() and np.array_equal(sc, words[idx]), (n, kind, "ref_order 1 descends in key")
        again = rank_list(lib, row, 1)
        assert np.array_equal(again[0], idx) and np.array_equal(again[1], sc), (n, kind, "ref_order 1 twice")
        if kind in NAN_FREE:
            assert np.array_equal(idx, old_rank_list(exe, row, tmp_path)), (n, kind, "ref_order 1 is the old statement's permutation on a NaN-free row")
    if n >= 1000:                                                           # the kinds are what they claim: NaNs of both signs where they should be, ties for the unstable sort to move
        assert (rows[RH.ROW_SPECIAL].view(np.uint32) == QNAN).any() and (rows[RH.ROW_SPECIAL].view(np.uint32) == QNAN_NEG).any()
        assert np.isnan(rows[ROW_TWO_NANS]).sum() == 2 and not np.isnan(rows[:RH.ROW_SPECIAL]).any()
        assert not np.array_equal(rank_list(lib, rows[1], 1)[0], rank_list(lib, rows[1], 0)[0])


def test_rank_list_padding_and_arguments(lib):
    row = np.array([1.0, np.nan, 3.0], np.float32)
    idx = np.full(5, -7, np.int64); sc = np.full(5, 9, np.float32)
    p = (row.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(3))
    assert lib.afis_rank_list(*p, 0, 5, idx.ctypes.data_as(C.POINTER(C.c_int64)), sc.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert idx.tolist() == [1, 2, 0, -1, -1] and np.isnan(sc[0]) and sc[1:].tolist() == [3.0, 1.0, 0.0, 0.0]     # a NaN with the sign clear ranks above everything
    assert lib.afis_rank_list(*p, 1, 2, idx.ctypes.data_as(C.POINTER(C.c_int64)), None) == 0 and idx[:2].tolist() == [1, 2]
    assert lib.afis_rank_list(None, C.c_int64(3), 0, 1, idx.ctypes.data_as(C.POINTER(C.c_int64)), None) == -1


# ---- 2: the sanitizer-built program -------------------------------------------------------------------------------------------------------------------------
def test_rank_order_check_runs_clean():
    """rank_order.h's functions and afis_rank_list's body on NaN rows at every n above, under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
    out = subprocess.run([tool("rank_order_check")], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 failures" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk[mk.index("rank_order_check:"):]


# ---- 3: the exchange's merge ----------------------------------------------------------------------------------------------------------------------------------
def shard_lists(row, bounds, k):
    idx = np.empty((len(bounds), k), np.int64); sc = np.empty((len(bounds), k), np.uint32)
    for r, (lo, hi) in enumerate(bounds):
        idx[r], sc[r] = model_topk(row[lo:hi], np.arange(lo, hi), k)
    return idx, sc


@pytest.mark.parametrize("k_out", [24, 10])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_exchange_merge_of_special_rows(world, k_out, tmp_path):
    exe = tool("match_selftest")
    n, k = 3001, 24
    rng = np.random.default_rng(SEED + world)
    rows = rows_of(n, rng)
    bounds = SH.shard_bounds(rng.integers(1, 9, n), world)
    for kind in (RH.ROW_SPECIAL, ROW_TWO_NANS, 3):
        row = rows[kind]
        idx, sc = shard_lists(row, bounds, k)
        f = tmp_path / ("merge_%d.txt" % kind)
        f.write_text("%d %d %d\n" % (world, k, k_out) + "".join("%d %08x\n" % (i, w) for i, w in zip(idx.ravel().tolist(), sc.ravel().tolist())))
        out = subprocess.run([exe, "-selftest-merge", str(f)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        got = out.stdout.split()
        gi, gs = np.array(got[0::2], np.int64), np.array([int(w, 16) for w in got[1::2]], np.uint32)
        wi, ws = model_topk(row, np.arange(n), k_out)
        assert np.array_equal(gi, wi) and np.array_equal(gs, ws), (world, k_out, kind, gi.tolist(), wi.tolist())
    assert np.isnan(model_topk(rows[RH.ROW_SPECIAL], np.arange(n), k)[1].view(np.float32)).all()     # the head of the special row is NaNs: the merge was about them
    short = np.array([2.0, np.nan], np.float32)                               # fewer entries than k_out: padding
    f = tmp_path / "short.txt"
    f.write_text("2 1 4\n0 %08x\n1 %08x\n" % tuple(short.view(np.uint32).tolist()))
    out = subprocess.run([exe, "-selftest-merge", str(f)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["1", "7fc00000", "0", "40000000", "-1", "ff800000", "-1", "ff800000"]


# ---- 4: host/sharding.py ---------------------------------------------------------------------------------------------------------------------------------------
def _old_merge_topk(idx, score, k):
    R, Q, kk = idx.shape
    fi = np.transpose(idx, (1, 0, 2)).reshape(Q, R * kk)
    fs = np.transpose(score, (1, 0, 2)).reshape(Q, R * kk).astype(np.float32)
    out_i = np.full((Q, k), -1, np.int64); out_s = np.full((Q, k), -np.inf, np.float32)
    for q in range(Q):
        valid = fi[q] >= 0
        vi, vs = fi[q][valid], fs[q][valid]
        order = np.lexsort((vi, -vs.astype(np.float64)))[:k]
        out_i[q, :len(order)] = vi[order]; out_s[q, :len(order)] = vs[order]
    return out_i, out_s


def _old_merge_subject_topk(ids, score, best_idx, k):
    R, Q, kk = ids.shape
    fi = np.transpose(ids, (1, 0, 2)).reshape(Q, R * kk)
    fs = np.transpose(score, (1, 0, 2)).reshape(Q, R * kk).astype(np.float32)
    fb = np.transpose(best_idx, (1, 0, 2)).reshape(Q, R * kk)
    out_i = np.full((Q, k), -1, np.int64); out_s = np.full((Q, k), -np.inf, np.float32); out_b = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        valid = fi[q] >= 0
        vi, vs, vb = fi[q][valid], fs[q][valid], fb[q][valid]
        order = np.lexsort((vb, -vs.astype(np.float64), vi))
        first = np.ones(len(order), bool); first[1:] = vi[order][1:] != vi[order][:-1]
        keep = order[first]
        vi, vs, vb = vi[keep], vs[keep], vb[keep]
        order = np.lexsort((vi, -vs.astype(np.float64)))[:k]
        out_i[q, :len(order)] = vi[order]; out_s[q, :len(order)] = vs[order]; out_b[q, :len(order)] = vb[order]
    return out_i, out_s, out_b


def _old_merge_prints_to_card(n_hits, latent, score, cap):
    li = np.asarray(latent, np.int64)
    P, kk = li.shape
    fs = np.asarray(score, np.float32).reshape(P * kk)
    fp = np.repeat(np.arange(P, dtype=np.int64), kk)
    fl = li.reshape(P * kk)
    valid = fl >= 0
    vl, vs, vp = fl[valid], fs[valid], fp[valid]
    order = np.lexsort((vp, -vs.astype(np.float64), vl))
    first = np.ones(len(order), bool); first[1:] = vl[order][1:] != vl[order][:-1]
    keep = order[first]
    vl, vs, vp = vl[keep], vs[keep], vp[keep]
    order = np.lexsort((vl, -vs.astype(np.float64)))[:cap]
    out_l = np.full(cap, -1, np.int64); out_s = np.full(cap, -np.inf, np.float32); out_p = np.full(cap, -1, np.int64)
    out_l[:len(order)] = vl[order]; out_s[:len(order)] = vs[order]; out_p[:len(order)] = vp[order]
    return out_l, out_s, out_p, int(len(vl)), bool((np.asarray(n_hits, np.int64) > kk).any())


def same(got, want):
    """Every array of the two tuples equal, float arrays as words."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


def words_to_f32(a):
    return np.ascontiguousarray(a, np.uint32).view(np.float32)


def stack_hits(models, thr, kk, keys):
    """Per-rank hit lists of RH.TemplateModel / RH.SubjectModel objects as [R, Q] / [R, Q, kk] arrays, scores as float32."""
    hs = [m.hits(thr, kk) for m in models]
    return [np.stack([words_to_f32(h[key]) if key == "score" else h[key] for h in hs]) for key in keys]


N_SHARD, BASE = 3001, 700
SPECIAL_KINDS = [RH.ROW_SPECIAL, ROW_TWO_NANS]


@pytest.fixture(scope="module")
def sharded():
    """Rows of 3001 scores (every kind), global indices from 700, a subject plan whose persons straddle the shards, and shard plans for 2, 3 and 8 ranks."""
    rng = np.random.default_rng(SEED)
    rows = rows_of(N_SHARD, rng)
    glob = BASE + np.arange(N_SHARD, dtype=np.int64)
    subject = (rng.permutation(1000)[:260].astype(np.int64) * 7 + 3)[rng.integers(0, 260, N_SHARD)]
    plans = {w: SH.shard_bounds(rng.integers(1, 9, N_SHARD), w) for w in (2, 3, 8)}
    return rows, glob, subject, plans


@pytest.mark.parametrize("world", [2, 3, 8])
def test_template_merges(world, sharded):
    rows, glob, _, plans = sharded
    bounds = plans[world]
    F = np.float32
    for kk, cap in ((24, 24), (24, 10), (100, 65)):
        models = [RH.TemplateModel(rows[:, lo:hi], glob[lo:hi]) for lo, hi in bounds]
        whole = RH.TemplateModel(rows, glob)
        for thr in (F(-np.inf), F(0.0), F(1.5)):
            nh, li, ls = stack_hits(models, thr, kk, ("n_hits", "idx", "score"))
            want = whole.hits(thr, cap)
            n, i, s = SH.merge_hits(nh, li, ls, cap)
            assert n.dtype == np.int64 and i.dtype == np.int64 and s.dtype == np.float32
            assert np.array_equal(n, want["n_hits"]) and np.array_equal(i, want["idx"]) and np.array_equal(s.view(np.uint32), want["score"]), (world, kk, cap, float(thr))
            if np.isneginf(thr):                                            # the rank lists themselves; and on NaN-free rows the parent's function, bit for bit
                i2, s2 = SH.merge_topk(li, ls, cap)
                assert np.array_equal(i2, want["idx"]) and np.array_equal(s2.view(np.uint32), want["score"])
                keep = list(NAN_FREE)
                same(SH.merge_topk(li[:, keep], ls[:, keep], cap), _old_merge_topk(li[:, keep], ls[:, keep], cap))
    assert np.isnan(whole.hits(F(-np.inf), 10)["score"].view(np.float32)[SPECIAL_KINDS]).any()      # a NaN stands at the head of the special rows


def subject_rows(rows, rng):
    """The rows with their -0.0 kept and more planted: the subject key ranks -0.0 below +0.0."""
    out = rows.copy()
    w = out.view(np.uint32)
    zero = np.flatnonzero(w[3] == 0)
    w[3, rng.choice(zero, len(zero) // 2, replace=False)] = 0x80000000        # the search-like row: half of its zeros negative
    return out


@pytest.mark.parametrize("world", [2, 3, 8])
def test_subject_merges(world, sharded):
    rows, glob, subject, plans = sharded
    bounds = plans[world]
    F = np.float32
    rows = subject_rows(rows, np.random.default_rng(SEED + 1))
    whole = RH.SubjectModel(rows, glob, subject)
    models = [RH.SubjectModel(rows[:, lo:hi], glob[lo:hi], subject[lo:hi]) for lo, hi in bounds]
    n_subjects = len(np.unique(subject))
    for kk, cap in ((24, 24), (24, 10), (300, 65)):
        for thr in (F(-np.inf), F(0.0), F(-0.0)):
            nh, li, ls, lb = stack_hits(models, thr, kk, ("n_hits", "subject", "score", "best_idx"))
            want = whole.hits(thr, cap)
            n, trunc, i, s, b = SH.merge_subject_hits(nh, li, ls, lb, cap)
            assert np.array_equal(trunc, (nh > kk).any(axis=0))
            assert np.array_equal(i, want["subject"]) and np.array_equal(s.view(np.uint32), want["score"]) and np.array_equal(b, want["best_idx"]), (world, kk, cap, float(thr))
            assert ((n == want["n_hits"]) | trunc).all() and (n <= want["n_hits"]).all()
            if kk == 300:
                assert not trunc.any() and n_subjects <= kk
            if np.isneginf(thr):
                same(SH.merge_subject_topk(li, ls, lb, cap), (want["subject"], words_to_f32(want["score"]), want["best_idx"]))
    # -0.0 beside +0.0 in different shards: a person whose best is +0.0 in one shard and -0.0 in another keeps the +0.0 and its template, whichever rank comes first
    lo1 = bounds[1][0]
    for first, second in ((0x00000000, 0x80000000), (0x80000000, 0x00000000)):
        two = np.full((1, N_SHARD), -1.0, np.float32)
        two.view(np.uint32)[0, [5, lo1 + 5]] = (first, second)
        subj2 = np.arange(N_SHARD, dtype=np.int64) + 10
        subj2[[5, lo1 + 5]] = 4
        parts = [RH.SubjectModel(two[:, lo:hi], glob[lo:hi], subj2[lo:hi]) for lo, hi in bounds]
        nh, li, ls, lb = stack_hits(parts, F(-np.inf), 24, ("n_hits", "subject", "score", "best_idx"))
        i, s, b = SH.merge_subject_topk(li, ls, lb, 24)
        want = RH.SubjectModel(two, glob, subj2).hits(F(-np.inf), 24)
        assert np.array_equal(i, want["subject"]) and np.array_equal(s.view(np.uint32), want["score"]) and np.array_equal(b, want["best_idx"])
        assert i[0, 0] == 4 and s.view(np.uint32)[0, 0] == 0 and b[0, 0] == BASE + (5 if first == 0 else lo1 + 5)
    # rows without NaN and without -0.0: the parent's function, bit for bit
    clean = [k for k in NAN_FREE if not (rows[k].view(np.uint32) == 0x80000000).any()]
    assert len(clean) == 7
    nh, li, ls, lb = stack_hits(models, F(-np.inf), 24, ("n_hits", "subject", "score", "best_idx"))
    same(SH.merge_subject_topk(li[:, clean], ls[:, clean], lb[:, clean], 24), _old_merge_subject_topk(li[:, clean], ls[:, clean], lb[:, clean], 24))


def card_model(scores, thr, cap):
    """scores [P][L]: per latent the best key over the card's prints (the lowest print position among equals), among entries whose key reaches thr's; key descending, latent ascending."""
    key = RH.template_key(scores).astype(np.int64)
    key = np.where(key >= int(RH.template_key(np.array([thr], np.float32))[0]), key, -1)
    best_p = np.argmax(key, axis=0)                                         # the first maximum: the lowest print position
    lat = np.flatnonzero(key.max(axis=0) >= 0)
    o = lat[np.lexsort((lat, -key[best_p[lat], lat]))][:cap]
    out_l = np.full(cap, -1, np.int64); out_s = np.full(cap, NEG_INF_WORD, np.uint32); out_p = np.full(cap, -1, np.int64)
    out_l[:len(o)] = o; out_s[:len(o)] = scores.view(np.uint32)[best_p[o], o]; out_p[:len(o)] = best_p[o]
    return out_l, out_s, out_p, len(lat)


def test_prints_to_card(sharded):
    rows = sharded[0]
    F = np.float32
    L = 400
    card = np.ascontiguousarray(rows[[RH.ROW_SPECIAL, ROW_TWO_NANS, 1, 3, RH.ROW_SPECIAL], 1000:1000 + L])   # five prints x 400 latents, special values in three of them
    card[4] = card[4][::-1]
    per_print = [RH.TemplateModel(card[p:p + 1], np.arange(L)) for p in range(len(card))]
    for kk, cap in ((L, 24), (L, 65), (100, 65)):
        for thr in (F(-np.inf), F(0.0)):
            hs = [m.hits(thr, kk) for m in per_print]
            nh = np.array([h["n_hits"][0] for h in hs]); lat = np.stack([h["idx"][0] for h in hs]); sc = np.stack([words_to_f32(h["score"][0]) for h in hs])
            got = SH.merge_prints_to_card(nh, lat, sc, cap)
            wl, ws, wp, wn = card_model(card, thr, cap)
            assert np.array_equal(got[0], wl) and np.array_equal(got[1].view(np.uint32), ws) and np.array_equal(got[2], wp), (kk, cap, float(thr))
            assert got[4] == bool((nh > kk).any()) and (got[3] == wn if not got[4] else got[3] <= wn)
    clean = np.ascontiguousarray(rows[[0, 1, 3, 5], 1000:1000 + L])           # NaN-free: the parent's function, bit for bit
    hs = [RH.TemplateModel(clean[p:p + 1], np.arange(L)).hits(F(-np.inf), 100) for p in range(len(clean))]
    args = (np.array([h["n_hits"][0] for h in hs]), np.stack([h["idx"][0] for h in hs]), np.stack([words_to_f32(h["score"][0]) for h in hs]), 65)
    got, want = SH.merge_prints_to_card(*args), _old_merge_prints_to_card(*args)
    same(got[:3], want[:3])
    assert got[3:] == want[3:]


def test_python_keys_are_the_models():
    w = np.r_[RH.SPECIAL.view(np.uint32), np.random.default_rng(SEED).integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)]
    w = w[~((w & 0x7f800000 == 0x7f800000) & (w & 0x003fffff != 0) & (w & 0x00400000 == 0))]     # (no signalling NaN: an addition quietens it)
    f = w.view(np.float32)
    assert np.array_equal(SH.rank_key(f), RH.template_key(f)) and np.array_equal(SH.subject_key(f), RH.subject_key(f))
    assert SH.rank_key(np.float32(-0.0)) == SH.rank_key(np.float32(0.0)) and SH.subject_key(np.float32(-0.0)) < SH.subject_key(np.float32(0.0))
