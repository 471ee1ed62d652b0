"""Filtered case lists and filtered reverse lists without a GPU: the three entry points are declared, exported by both libraries and bound by the Python host; the
folds are still case_fuse.hip's; the header keeps the phrases other tests read; the shard merges are held against a one-shard numpy model of the header's semantics.
(What the lists hold is tests/test_gpu_case_filters.py's.)"""
import importlib
import os
import re

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afis_rank_case_hits_filtered", "afis_rank_case_subject_hits_filtered", "afis_rank_latent_hits_filtered")
SUM, MAX = 0, 1
U64 = np.uint64


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):        # dlopen only: no device call
        for name in NEW:
            assert re.search(r"\bint\s+%s\s*\(afis_ctx\*" % name, code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert getattr(lib, name).argtypes is not None, name
    assert len(M.load_library().afis_rank_case_hits_filtered.argtypes) == 15 and len(M.load_library().afis_rank_case_subject_hits_filtered.argtypes) == 16
    assert len(M.load_library().afis_rank_latent_hits_filtered.argtypes) == 12
    for method in ("rank_case_hits_filtered", "rank_case_subject_hits_filtered", "rank_latent_hits_filtered"):
        assert hasattr(M.Matcher, method), method


def test_the_header_keeps_its_phrases():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    assert "Not in this interface" in hdr and "cannot span" in hdr and "0xffffffff" in hdr
    left_out = hdr[hdr.index("Not in this interface"):]
    left_out = left_out[:left_out.index("\n * Shards")]
    assert "spanning searches" in left_out and "afis_rank_subjects" in left_out and "top-k" in left_out
    assert "filters on the case lists" not in hdr                           # what was left out is in now
    option_text = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    for opt in ("rank_cases_us", "case_fuse_us", "case_rank_us", "rank_latents_us", "rank_filtered_us", "filter_us"):
        assert '"%s"' % opt in option_text, opt
    assert "afis_rank_latent_hits_filtered" in option_text and "_filtered forms" in option_text


def test_the_folds_are_case_fuse_hip():
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "case_fuse.hip")).read()
    assert "__global__" in src and "k_case_fuse" in src and "k_case_fuse_subjects" in src
    assert "kNoEntryWord" in src and "composite_word(b)" in src
    ctx = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "afis_ctx.h")).read()
    assert re.search(r"int check_filtered\([^;]*visibility\(\"hidden\"\)", ctx, flags=re.S)   # one definition of the checks, shared
    flt = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "afis_filter.cpp")).read()
    assert "static int check_filtered" not in flt


# ---- the header's semantics as a numpy model, and the merges against it -----------------------------------------------------------------------------------
def eligible(labels, masks, names, excl):
    """labels, names [n] of the columns, masks [n_q][3], excl: per query a list of names -> [n_q][n] bool."""
    L = labels[None, :]
    any_of, all_of, none_of = masks[:, 0:1], masks[:, 1:2], masks[:, 2:3]
    ok = ((any_of == 0) | ((L & any_of) != 0)) & ((L & all_of) == all_of) & ((L & none_of) == 0)
    for q, e in enumerate(excl):
        ok[q] &= ~np.isin(names, np.asarray(e, np.int64))
    return ok


def fuse(rows, ok, case_of, mode):
    """-> (fused [n_cases][n], entry [n_cases][n]): over the eligible members in query order; a member takes part when its value is >= 0; no eligible member: no entry."""
    out, ent = [], []
    for cid in np.unique(case_of):
        members = np.flatnonzero(case_of == cid)
        seen = ok[members].any(axis=0)
        if mode == SUM:
            acc = np.zeros(rows.shape[1], np.float32); took = np.zeros(rows.shape[1], bool)
            for i in members:
                part = ok[i] & (rows[i] >= 0)
                acc = np.where(part, (acc + rows[i]).astype(np.float32), acc); took |= part
            out.append(np.where(took, acc, np.float32(-1)))
        else:
            out.append(np.where(ok[members], rows[members], -np.inf).max(axis=0))   # (the model's scores are finite)
        ent.append(seen)
    return np.array(out, np.float32).reshape(len(out), rows.shape[1]), np.array(ent, bool).reshape(len(ent), rows.shape[1])


def lists(fused, entry, names, thr, k):
    """(n_hits [C], names [C][k], score [C][k]) of the rows' entries: value descending, name ascending, cut at thr and k, padded with (-1, -inf)."""
    C = fused.shape[0]
    n = np.empty(C, np.int64); a = np.full((C, k), -1, np.int64); sc = np.full((C, k), -np.inf, np.float32)
    for c in range(C):
        at = np.flatnonzero(entry[c] & (fused[c] >= thr))
        at = at[np.lexsort((names[at], -fused[c, at].astype(np.float64)))]
        n[c] = len(at); a[c, :min(k, len(at))] = names[at[:k]]; sc[c, :min(k, len(at))] = fused[c, at[:k]]
    return n, a, sc


def subject_rows(rows, ok, subject, excl):
    """-> (the persons present ascending, best [n_q][S], have [n_q][S]): a person's best eligible score per query; have: there is one and the person is not excluded."""
    ids = np.unique(subject)
    best = np.stack([np.where(ok[:, subject == s], rows[:, subject == s], -np.inf).max(axis=1) for s in ids], axis=1).astype(np.float32)
    have = np.stack([ok[:, subject == s].any(axis=1) for s in ids], axis=1)
    for q, e in enumerate(excl):
        have[q] &= ~np.isin(ids, np.asarray(e, np.int64))
    return ids, best, have


def search_like(rng, n_q, G):
    """-1, 0 and positives rounded to a few values: the tie rules decide nearly every place; one latent-empty row."""
    u = rng.random((n_q, G))
    m = np.where(u < 0.1, -1.0, np.where(u < 0.5, np.round(rng.random((n_q, G)) * 6) / 2, 0.0)).astype(np.float32)
    m[n_q // 2] = -1
    return m


CASE_OF = np.array([40, 7, 40, 7, 7, 1 << 35, 40, 7, 12], np.int64)
N_Q = len(CASE_OF)
THRS = (-np.inf, -1.0, 0.0, 2.5, 100.0)
G = 400
BASE = 5000


def world(rng, subject=None):
    """One gallery of 400 labelled templates, per query a finger mask (a fifth passes; query 3 passes nothing, query 8 everything) and an exclusion list — of
    templates, or of persons — that also names what no shard holds."""
    rows = search_like(rng, N_Q, G)
    labels = (U64(1) << rng.integers(0, 10, G).astype(U64)) | (U64(1) << U64(20))
    masks = np.zeros((N_Q, 3), U64)
    masks[:, 0] = (U64(1) << rng.integers(0, 10, N_Q).astype(U64)) | (U64(1) << rng.integers(0, 10, N_Q).astype(U64))
    masks[3] = (0, 0, U64(1) << U64(20)); masks[8] = 0
    names = BASE + np.arange(G, dtype=np.int64) if subject is None else np.unique(subject)
    excl = [[int(x) for x in names[rng.integers(0, len(names), 6)]] + [1 << 40, 3] for _ in range(N_Q)]
    excl[2] = []
    return rows, labels, masks, excl


@pytest.mark.parametrize("mode", [SUM, MAX])
@pytest.mark.parametrize("world_size", [2, 3])
def test_filtered_case_template_lists_merge_with_merge_hits(mode, world_size):
    """Each shard labels its own templates; every rank gets the same masks, exclusions and case_of.  The columns of different shards are disjoint and "no entry" is a
    property of a column: the per-rank lists are merge_hits' input as they are."""
    rng = np.random.default_rng(61 + mode)
    rows, labels, masks, excl = world(rng)
    glob = BASE + np.arange(G, dtype=np.int64)
    ok = eligible(labels, masks, glob, excl)
    fused, entry = fuse(rows, ok, CASE_OF, mode)
    assert (~entry).any() and entry.any(axis=1).all()
    for trial in range(3):
        cuts = np.sort(rng.integers(0, G + 1, world_size - 1)) if trial else np.array([150, 150][:world_size - 1])
        bounds = list(zip(np.r_[0, cuts], np.r_[cuts, G]))
        for cap in (6, 64):
            for thr in THRS:
                per = []
                for lo, hi in bounds:
                    f, e = fuse(rows[:, lo:hi], eligible(labels[lo:hi], masks, glob[lo:hi], excl), CASE_OF, mode)
                    per.append(lists(f, e, glob[lo:hi], thr, cap))
                n, i, s = SH.merge_hits(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), cap)
                wn, wi, ws = lists(fused, entry, glob, thr, cap)
                assert np.array_equal(n, wn) and np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (trial, cap, thr)
    wn, _, ws = lists(fused, entry, glob, -np.inf, G)
    assert (wn == entry.sum(axis=1)).all() and (wn < G).all()               # -inf lists the entries, not the columns
    if mode == SUM:
        assert (ws == -1).any()                                             # eligible members that all hold -1: an entry


@pytest.mark.parametrize("world_size", [2, 3])
def test_filtered_column_lists_merge_with_merge_hits(world_size):
    """The reverse lists with the LATENTS split over handles or ranks, each part with its latent_base, its rows of the masks and its exclusion lists: the columns are
    common, a latent lies in one part, and the per-column lists merge with merge_hits as the unfiltered ones do."""
    rng = np.random.default_rng(67)
    rows, labels, masks, excl = world(rng)
    glob = BASE + np.arange(G, dtype=np.int64)
    labels[17] = U64(1) << U64(20); excl[8] = excl[8] + [BASE + 17]         # no finger bit, the bit query 3 refuses, and on the list of the query that passes everything
    ok = eligible(labels, masks, glob, excl)
    latents = 900 + np.arange(N_Q, dtype=np.int64)
    assert (~ok.any(axis=0)).any()                                          # templates no query is eligible for
    cuts = (4,) if world_size == 2 else (3, 3)                              # (3, 3): an empty part
    bounds = list(zip((0,) + cuts, cuts + (N_Q,)))
    for cap in (2, 16):
        for thr in THRS:
            per = [lists(rows[lo:hi].T, ok[lo:hi].T, latents[lo:hi], thr, cap) for lo, hi in bounds]
            n, i, s = SH.merge_hits(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), cap)
            wn, wi, ws = lists(rows.T, ok.T, latents, thr, cap)
            assert np.array_equal(n, wn) and np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (cap, thr)
    assert (lists(rows.T, ok.T, latents, -np.inf, 4)[0][~ok.any(axis=0)] == 0).all()


def plan(rng, n_subjects=70):
    """70 persons of 1-12 templates each, in contiguous runs."""
    counts = rng.integers(1, 13, n_subjects)
    while counts.sum() != G:
        j = rng.integers(n_subjects)
        if counts.sum() > G and counts[j] > 1: counts[j] -= 1
        elif counts.sum() < G and counts[j] < 12: counts[j] += 1
    return np.repeat(rng.permutation(1000)[:n_subjects].astype(np.int64) * 7 + 3, counts), counts


def per_rank_subject_lists(rows, labels, masks, excl, subject, bounds, mode, thr, kk):
    glob = BASE + np.arange(G, dtype=np.int64)
    per = []
    for lo, hi in bounds:
        if hi > lo:
            ok = eligible(labels[lo:hi], masks, glob[lo:hi], [[]] * N_Q)
            ids, best, have = subject_rows(rows[:, lo:hi], ok, subject[lo:hi], excl)
            f, e = fuse(best, have, CASE_OF, mode)
            per.append(lists(f, e, ids, thr, kk))
        else:                                                               # an empty shard: zero counts and padding
            C = len(np.unique(CASE_OF))
            per.append((np.zeros(C, np.int64), np.full((C, kk), -1, np.int64), np.full((C, kk), -np.inf, np.float32)))
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per])


@pytest.mark.parametrize("world_size", [2, 3])
def test_filtered_case_subject_lists_max(world_size):
    """Exact although persons straddle the cuts: a maximum over the eligible members of a maximum over the eligible templates is the greatest per-rank value, and a
    person is an entry of the case where some rank holds an eligible template of theirs for a member that does not exclude them."""
    rng = np.random.default_rng(71)
    labels_of, _ = plan(rng)
    subject = labels_of[rng.permutation(G)]                                 # dealt over the positions: most persons straddle
    rows, labels, masks, excl = world(rng, subject)
    glob = BASE + np.arange(G, dtype=np.int64)
    ids, best, have = subject_rows(rows, eligible(labels, masks, glob, [[]] * N_Q), subject, excl)
    fused, entry = fuse(best, have, CASE_OF, MAX)
    assert (~entry).any()
    bounds = [(0, 150), (150, 400)] if world_size == 2 else [(0, 150), (150, 150), (150, 400)]
    for bs in (bounds, SH.shard_bounds(rng.integers(1, 9, G), world_size)):
        assert sum(len({r for r, (lo, hi) in enumerate(bs) if (subject[lo:hi] == s).any()}) > 1 for s in ids) > 30
        for cap in (6, 64):
            for thr in THRS:
                nh, li, ls = per_rank_subject_lists(rows, labels, masks, excl, subject, bs, MAX, thr, cap)
                n, trunc, i, s = SH.merge_case_subject_hits(nh, li, ls, cap, MAX)
                wn, wi, ws = lists(fused, entry, ids, thr, cap)
                assert np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (cap, thr)
                assert np.array_equal(trunc, (nh > cap).any(axis=0))
                for c in range(len(wn)):
                    assert n[c] == wn[c] if not trunc[c] else n[c] <= wn[c], (cap, thr, c)


@pytest.mark.parametrize("world_size", [2, 3])
def test_filtered_case_subject_lists_sum(world_size):
    """Whole persons per shard: every id arrives from one rank, the counts add and the lists merge exactly.  A person in two shards is refused."""
    rng = np.random.default_rng(73)
    subject, counts = plan(rng)                                             # contiguous runs: a cut between two runs keeps every person whole
    rows, labels, masks, excl = world(rng, subject)
    glob = BASE + np.arange(G, dtype=np.int64)
    ids, best, have = subject_rows(rows, eligible(labels, masks, glob, [[]] * N_Q), subject, excl)
    fused, entry = fuse(best, have, CASE_OF, SUM)
    ends = np.cumsum(counts)
    a, b = int(ends[20]), int(ends[45])
    bounds = [(0, a), (a, G)] if world_size == 2 else [(0, a), (a, b), (b, G)]
    for cap in (6, 64):
        for thr in THRS:
            nh, li, ls = per_rank_subject_lists(rows, labels, masks, excl, subject, bounds, SUM, thr, cap)
            n, trunc, i, s = SH.merge_case_subject_hits(nh, li, ls, cap, SUM)
            wn, wi, ws = lists(fused, entry, ids, thr, cap)
            assert np.array_equal(n, wn) and np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (cap, thr)
    # a cut through a run of a person who is an entry on both sides: the id arrives from two ranks
    whole = np.ones((N_Q, 3), U64) * U64(0)
    inside = next(int(e) - 1 for e, c in zip(ends, counts) if c > 1 and e > 100)
    nh, li, ls = per_rank_subject_lists(rows, labels, whole, [[]] * N_Q, subject, [(0, inside), (inside, G)], SUM, -np.inf, 64)
    with pytest.raises(ValueError, match="AFIS_CASE_SUM.*two ranks"):
        SH.merge_case_subject_hits(nh, li, ls, 64, SUM)
    n, trunc, i, s = SH.merge_case_subject_hits(nh, li, ls, 64, MAX)        # (the same input merges in max mode)
    assert (n == len(ids)).all()
