"""Case lists without a GPU: the two entry points and the two modes are declared, exported by both libraries and bound by the Python host; the fold kernel is part of
the product objects; the option is documented; the shard merges are held against a global numpy model.  (What a case list holds is tests/test_gpu_case_lists.py's.)"""
import importlib
import os
import re

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afis_rank_case_hits", "afis_rank_case_subject_hits")
SUM, MAX = 0, 1


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"^#define\s+AFIS_CASE_SUM\s+0\s*$", code, flags=re.M) and re.search(r"^#define\s+AFIS_CASE_MAX\s+1\s*$", code, flags=re.M)
    assert (M.CASE_SUM, M.CASE_MAX) == (SUM, MAX)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):        # dlopen only: no device call
        for name in NEW:
            assert re.search(r"\bint\s+%s\s*\(afis_ctx\*" % name, code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert getattr(lib, name).argtypes is not None, name
    for method in ("rank_case_hits", "rank_case_subject_hits"):
        assert hasattr(M.Matcher, method), method
    assert "cannot span" in hdr                                             # a case is the queries of ONE search
    assert re.search(r'"rank_cases_us" \(read-only\)', hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")])
    assert "`rank_cases_us`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_kernel_is_a_product_object():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "case_fuse.o" in objs and "afis_cases.o" in objs
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "case_fuse.hip")).read()
    assert "__global__" in src and "k_case_fuse" in src and "k_case_fuse_subjects" in src


# ---- the merges against a global model -----------------------------------------------------------------------------------------------------------
def fuse(rows, case_of, mode):
    """rows [n_q][n] -> fused [n_cases][n], the rows in ascending case id: member by member in query order; a member takes part when its value is >= 0."""
    out = []
    for cid in np.unique(case_of):
        members = np.flatnonzero(case_of == cid)
        if mode == SUM:
            acc = np.zeros(rows.shape[1], np.float32); took = np.zeros(rows.shape[1], bool)
            for i in members:
                part = rows[i] >= 0
                acc = np.where(part, (acc + rows[i]).astype(np.float32), acc); took |= part
            out.append(np.where(took, acc, np.float32(-1)))
        else:
            out.append(rows[members].max(axis=0))
    return np.array(out, np.float32).reshape(len(out), rows.shape[1])


def lists(fused, names, thr, k):
    """(n_hits [C], names [C][k], score [C][k]) of the fused rows: value descending, name ascending, cut at thr and k, padded with (-1, -inf)."""
    C = fused.shape[0]
    n = np.empty(C, np.int64); a = np.full((C, k), -1, np.int64); sc = np.full((C, k), -np.inf, np.float32)
    for c in range(C):
        at = np.flatnonzero(fused[c] >= thr)
        at = at[np.lexsort((names[at], -fused[c, at].astype(np.float64)))]
        n[c] = len(at); a[c, :min(k, len(at))] = names[at[:k]]; sc[c, :min(k, len(at))] = fused[c, at[:k]]
    return n, a, sc


def subject_rows(rows, subject):
    """rows [n_q][n] over columns labelled subject [n] -> (the labels present ascending, best [n_q][S])."""
    ids = np.unique(subject)
    return ids, np.stack([rows[:, subject == s].max(axis=1) for s in ids], axis=1).astype(np.float32)


def search_like(rng, n_q, G):
    """-1, 0 and positives rounded to a few values: the tie rules decide nearly every place; one latent-empty row."""
    u = rng.random((n_q, G))
    m = np.where(u < 0.1, -1.0, np.where(u < 0.5, np.round(rng.random((n_q, G)) * 6) / 2, 0.0)).astype(np.float32)
    m[n_q // 2] = -1
    return m


CASE_OF = np.array([40, 7, 40, 7, 7, 1 << 35, 40, 7, 12], np.int64)
THRS = (-np.inf, 0.0, 2.5, 100.0)


@pytest.mark.parametrize("mode", [SUM, MAX])
@pytest.mark.parametrize("cap", [6, 64])
def test_template_lists_merge_with_merge_hits(mode, cap):
    """The columns of different shards are disjoint and a case's row is common: the per-rank case lists are merge_hits' input as they are, over random shard cuts
    (an empty rank among them)."""
    rng = np.random.default_rng(31 + mode)
    G = 400
    rows = search_like(rng, len(CASE_OF), G)
    fused = fuse(rows, CASE_OF, mode)
    glob = np.arange(G, dtype=np.int64) + 5000
    for trial in range(4):
        cuts = np.sort(rng.integers(0, G + 1, 3)) if trial else np.array([150, 150, 300])
        bounds = list(zip(np.r_[0, cuts], np.r_[cuts, G]))
        for thr in THRS:
            per = [lists(fuse(rows[:, lo:hi], CASE_OF, mode), glob[lo:hi], thr, cap) for lo, hi in bounds]
            n, i, s = SH.merge_hits(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), cap)
            wn, wi, ws = lists(fused, glob, thr, cap)
            assert np.array_equal(n, wn) and np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (trial, thr)
            assert (n == 0).all() if thr == 100.0 else (n > 0).any()


def plan(rng, G=400, n_subjects=70):
    """70 subjects of 1-12 templates each, dealt over the 400 positions by a permutation: most subjects straddle the shards."""
    counts = rng.integers(1, 13, n_subjects)
    while counts.sum() != G:
        j = rng.integers(n_subjects)
        if counts.sum() > G and counts[j] > 1: counts[j] -= 1
        elif counts.sum() < G and counts[j] < 12: counts[j] += 1
    labels = np.repeat(rng.permutation(1000)[:n_subjects].astype(np.int64) * 7 + 3, counts)
    return labels, counts


def per_rank_subject_lists(rows, subject, bounds, mode, thr, kk):
    per = []
    for lo, hi in bounds:
        if hi > lo:
            ids, best = subject_rows(rows[:, lo:hi], subject[lo:hi])
            per.append(lists(fuse(best, CASE_OF, mode), ids, thr, kk))
        else:                                                               # an empty shard: zero counts and padding
            C = len(np.unique(CASE_OF))
            per.append((np.zeros(C, np.int64), np.full((C, kk), -1, np.int64), np.full((C, kk), -np.inf, np.float32)))
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per])


@pytest.mark.parametrize("cap", [6, 64])
def test_merge_case_subject_hits_max(cap):
    """Exact although most subjects straddle the shards: a maximum over members of a maximum over templates is the greatest per-rank value."""
    rng = np.random.default_rng(41)
    labels, _ = plan(rng)
    subject = labels[rng.permutation(len(labels))]
    rows = search_like(rng, len(CASE_OF), len(subject))
    ids, best = subject_rows(rows, subject)
    fused = fuse(best, CASE_OF, MAX)
    for bounds in (SH.shard_bounds(rng.integers(1, 9, len(subject)), 3), [(0, 150), (150, 150), (150, 400)]):
        straddle = sum(len({r for r, (lo, hi) in enumerate(bounds) if (subject[lo:hi] == s).any()}) > 1 for s in ids)
        assert straddle > 30
        for thr in THRS:
            nh, li, ls = per_rank_subject_lists(rows, subject, bounds, MAX, thr, cap)
            n, trunc, i, s = SH.merge_case_subject_hits(nh, li, ls, cap, MAX)
            wn, wi, ws = lists(fused, ids, thr, cap)
            assert np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), thr   # the list is exact, cut or not
            assert trunc.dtype == bool and np.array_equal(trunc, (nh > cap).any(axis=0))
            for c in range(len(wn)):
                assert n[c] == wn[c] if not trunc[c] else n[c] <= wn[c], (thr, c)                       # the count only while no rank was cut
            if cap == 64:
                assert not trunc.any()


@pytest.mark.parametrize("cap", [6, 64])
def test_merge_case_subject_hits_sum(cap):
    """Whole subjects per shard: every id arrives from one rank, the counts add and the lists merge exactly.  A subject in two shards is refused."""
    rng = np.random.default_rng(43)
    labels, counts = plan(rng)                                              # contiguous runs: a cut between two runs keeps every subject whole
    rows = search_like(rng, len(CASE_OF), len(labels))
    ids, best = subject_rows(rows, labels)
    fused = fuse(best, CASE_OF, SUM)
    ends = np.cumsum(counts)
    a, b = int(ends[20]), int(ends[45])
    for bounds in ([(0, a), (a, b), (b, len(labels))], [(0, a), (a, a), (a, len(labels))]):
        for thr in THRS:
            nh, li, ls = per_rank_subject_lists(rows, labels, bounds, SUM, thr, cap)
            n, trunc, i, s = SH.merge_case_subject_hits(nh, li, ls, cap, SUM)
            wn, wi, ws = lists(fused, ids, thr, cap)
            assert np.array_equal(n, wn) and np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), thr
            assert np.array_equal(trunc, (nh > cap).any(axis=0))
    # a cut through a subject's run: its id arrives from two ranks, and a sum of per-shard maxima is not the maximum's sum
    inside = next(int(e) - 1 for e, c in zip(ends, counts) if c > 1 and e > 100)
    nh, li, ls = per_rank_subject_lists(rows, labels, [(0, inside), (inside, len(labels))], SUM, -np.inf, 64)
    with pytest.raises(ValueError, match="AFIS_CASE_SUM.*two ranks"):
        SH.merge_case_subject_hits(nh, li, ls, 64, SUM)
    n, trunc, i, s = SH.merge_case_subject_hits(nh, li, ls, 64, MAX)        # (the same input merges in max mode)
    assert (n == len(ids)).all()
    with pytest.raises(ValueError, match="mode"):
        SH.merge_case_subject_hits(nh, li, ls, 64, 2)
