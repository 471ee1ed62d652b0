"""Hit lists without a GPU: the two entry points and AFIS_HITS_MAX are declared, exported by both libraries and bound by the Python host; the parity tap is the test
library's alone; the kernel is part of the product objects; the option is documented; the two shard merges are held against a global model.  (What a hit list holds is
tests/test_gpu_rank_hits.py's.)"""
import importlib
import os
import re

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afis_rank_hits", "afis_rank_subject_hits")
TAP = "afis_debug_rank_hits"


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"^#define\s+AFIS_HITS_MAX\s+4096\s*$", code, flags=re.M)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):        # dlopen only: no device call
        for name in NEW:
            assert re.search(r"\bint\s+%s\s*\(afis_ctx\*" % name, code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert getattr(lib, name).argtypes is not None, name
    for method in ("rank_hits", "rank_subject_hits", "debug_rank_hits"):
        assert hasattr(M.Matcher, method), method
    assert "score >= min_score" in hdr                                      # the plain rule on a search's scores, next to the key rule
    assert re.search(r'"rank_hits_us" \(read-only\)', hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")])
    assert "`rank_hits_us`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_tap_is_the_test_librarys_alone():
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    assert re.search(r"\bint\s+%s\s*\(afis_ctx\*" % TAP, re.sub(r"/\*.*?\*/", "", taps, flags=re.S))
    assert TAP in M.TAP_EXPORTS and TAP not in M.EXPORTS
    assert TAP not in open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    assert not hasattr(M.load_library(), TAP)
    tlib = M.load_library(M.TEST_LIB_PATH)
    assert hasattr(tlib, TAP) and getattr(tlib, TAP).argtypes is not None


def test_the_kernel_is_a_product_object():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "rank_hits.o" in objs and "afis_hits.o" in objs
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "rank_hits.hip")).read()
    assert "__global__" in src and "k_rank_hits" in src


# ---- the merges against a global model -----------------------------------------------------------------------------------------------------------
def pad(k, *cols):
    """Columns of one list cut / padded to k with (-1, -inf, -1, ...): int columns with -1, the float column with -inf."""
    out = []
    for c in cols:
        a = np.full(k, -np.inf, np.float32) if c.dtype == np.float32 else np.full(k, -1, np.int64)
        a[:min(k, len(c))] = c[:k]
        out.append(a)
    return out


def template_hits(score, lo, hi, thr, k):
    """(n_hits, idx, score) of templates [lo, hi) of one query — what Matcher.rank_hits returns on a shard with index_base lo."""
    at = lo + np.flatnonzero(score[lo:hi] >= thr)
    at = at[np.lexsort((at, -score[at].astype(np.float64)))]
    return (len(at),) + tuple(pad(k, at.astype(np.int64), score[at]))


def subject_hits(score, subject, lo, hi, thr, k):
    """(n_hits, subject, score, best_idx) of templates [lo, hi) of one query — Matcher.rank_subject_hits on that shard."""
    rows = []
    for s in np.unique(subject[lo:hi]):
        at = lo + np.flatnonzero(subject[lo:hi] == s)
        best = score[at].max()
        if best >= thr:
            rows.append((int(s), best, int(at[score[at] == best].min())))
    rows.sort(key=lambda r: (-float(r[1]), r[0]))
    cols = [np.array([r[j] for r in rows], dt) for j, dt in ((0, np.int64), (1, np.float32), (2, np.int64))]
    return (len(rows),) + tuple(pad(k, *cols))


def plan(rng, G=400, n_subjects=70):
    """70 subjects of 1-12 templates each, dealt over the 400 positions by a permutation (tests/test_subjects_host.py's plan): most subjects straddle the three shards."""
    counts = rng.integers(1, 13, n_subjects)
    while counts.sum() != G:
        j = rng.integers(n_subjects)
        if counts.sum() > G and counts[j] > 1: counts[j] -= 1
        elif counts.sum() < G and counts[j] < 12: counts[j] += 1
    labels = np.repeat(rng.permutation(1000)[:n_subjects].astype(np.int64) * 7 + 3, counts)
    return labels[rng.permutation(G)], SH.shard_bounds(rng.integers(1, 9, G), 3)


EMPTY_RANK = [(0, 150), (150, 150), (150, 400)]


def check_templates(score, bounds, thr, cap):
    Q, R = score.shape[0], len(bounds)
    nh = np.empty((R, Q), np.int64); li = np.empty((R, Q, cap), np.int64); ls = np.empty((R, Q, cap), np.float32)
    for q in range(Q):
        for r, (lo, hi) in enumerate(bounds):
            nh[r, q], li[r, q], ls[r, q] = template_hits(score[q], lo, hi, thr, cap)
    n, i, s = SH.merge_hits(nh, li, ls, cap)
    assert n.dtype == np.int64 and i.dtype == np.int64 and s.dtype == np.float32 and i.shape == (Q, cap)
    for q in range(Q):
        wn, wi, ws = template_hits(score[q], 0, score.shape[1], thr, cap)
        assert n[q] == wn and np.array_equal(i[q], wi) and np.array_equal(s[q], ws), (q, thr, cap)
    return nh, n


def check_subjects(score, subject, bounds, thr, cap):
    Q, R = score.shape[0], len(bounds)
    nh = np.empty((R, Q), np.int64); li = np.empty((R, Q, cap), np.int64); ls = np.empty((R, Q, cap), np.float32); lb = np.empty((R, Q, cap), np.int64)
    for q in range(Q):
        for r, (lo, hi) in enumerate(bounds):
            nh[r, q], li[r, q], ls[r, q], lb[r, q] = subject_hits(score[q], subject, lo, hi, thr, cap)
    n, trunc, i, s, b = SH.merge_subject_hits(nh, li, ls, lb, cap)
    assert trunc.dtype == bool and np.array_equal(trunc, (nh > cap).any(axis=0))
    for q in range(Q):
        wn, wi, ws, wb = subject_hits(score[q], subject, 0, len(subject), thr, cap)
        assert np.array_equal(i[q], wi) and np.array_equal(s[q], ws) and np.array_equal(b[q], wb), (q, thr, cap)   # the list is exact, cut or not
        assert n[q] == wn if not trunc[q] else n[q] <= wn, (q, thr, cap, int(n[q]), wn)                             # the count only while no rank was cut
    return nh, n, trunc


@pytest.mark.parametrize("cap", [6, 64])
@pytest.mark.parametrize("bounds_kind", ["balanced", "an empty rank"])
def test_merges_against_a_global_model(cap, bounds_kind):
    """Three ranks, scores rounded to 9 distinct values (the tie rules decide nearly every place); thresholds -inf, a value present in the data and one above the maximum."""
    rng = np.random.default_rng(21)
    subject, bounds = plan(rng)
    if bounds_kind == "an empty rank":
        bounds = EMPTY_RANK
    score = np.round(rng.random((4, 400)) * 8).astype(np.float32)
    assert len(np.unique(score)) == 9
    for thr in (-np.inf, 6.0, 9.0):
        nh, n = check_templates(score, bounds, thr, cap)
        assert (n == 0).all() if thr == 9.0 else (n > cap).all()
        if bounds_kind == "an empty rank":
            assert (nh[1] == 0).all()
        nh, n, trunc = check_subjects(score, subject, bounds, thr, cap)
        if thr == 9.0:
            assert (n == 0).all() and not trunc.any()
        elif cap == 6:
            assert trunc.all() and (n < len(np.unique(subject))).all()      # a rank was cut: the count is a lower bound, and here a strict one
        elif thr == -np.inf:
            assert not trunc.any() and (n == len(np.unique(subject))).all()  # no rank holds 64 subjects: nothing cut, every subject counted once although most straddle shards


def test_merges_all_minus_one():
    """A latent-empty query: every score -1.  At -1 everything hits, in ascending index / id order; at 0 nothing does."""
    rng = np.random.default_rng(22)
    subject, bounds = plan(rng)
    score = np.full((2, 400), -1, np.float32)
    nh, n = check_templates(score, bounds, -1.0, 6)
    assert (n == 400).all()
    assert (check_templates(score, bounds, 0.0, 6)[1] == 0).all()
    nh, n, trunc = check_subjects(score, subject, bounds, -1.0, 64)
    assert not trunc.any() and (n == 70).all()
    assert (check_subjects(score, subject, bounds, 0.0, 64)[1] == 0).all()


def test_merge_subject_hits_with_lists_longer_than_cap():
    """Per-rank lists of 64 merged into a list of 6: `truncated` is about what the ranks handed over (n_hits > 64), not about the merged list's cut — no rank holds 64
    subjects here, so the count is exact although the merged list is cut at 6; with per-rank lists of 6 the same data is truncated."""
    rng = np.random.default_rng(23)
    subject, bounds = plan(rng)
    score = np.round(rng.random((3, 400)) * 8).astype(np.float32)
    Q, R, kk, cap = 3, len(bounds), 64, 6
    nh = np.empty((R, Q), np.int64); li = np.empty((R, Q, kk), np.int64); ls = np.empty((R, Q, kk), np.float32); lb = np.empty((R, Q, kk), np.int64)
    for q in range(Q):
        for r, (lo, hi) in enumerate(bounds):
            nh[r, q], li[r, q], ls[r, q], lb[r, q] = subject_hits(score[q], subject, lo, hi, 4.0, kk)
    assert (nh > cap).all() and (nh <= kk).all()
    n, trunc, i, s, b = SH.merge_subject_hits(nh, li, ls, lb, cap)
    assert i.shape == (Q, cap) and not trunc.any()
    for q in range(Q):
        wn, wi, ws, wb = subject_hits(score[q], subject, 0, 400, 4.0, cap)
        assert n[q] == wn > cap and np.array_equal(i[q], wi) and np.array_equal(s[q], ws) and np.array_equal(b[q], wb)
    n6, trunc6 = SH.merge_subject_hits(nh, li[:, :, :cap], ls[:, :, :cap], lb[:, :, :cap], cap)[:2]
    assert trunc6.all() and (n6 <= n).all()
    tn, ti, ts = SH.merge_hits(*[np.stack(x) for x in zip(*[[np.array(v) for v in zip(*[template_hits(score[q], lo, hi, 4.0, kk) for q in range(Q)])] for lo, hi in bounds])], cap)
    for q in range(Q):
        wn, wi, ws = template_hits(score[q], 0, 400, 4.0, cap)
        assert tn[q] == wn and np.array_equal(ti[q], wi) and np.array_equal(ts[q], ws)
