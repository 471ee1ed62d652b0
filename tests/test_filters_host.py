"""Filtered hit lists without a GPU: the four entry points are declared, exported by both libraries and bound by the Python host; the filter kernels are part of the
product objects; the two options are documented; a numpy model of the contract, split over 2 and 3 shards — each shard with its own labels, every rank with the same
exclusion lists, a person's prints in two shards — merges with merge_hits / merge_subject_hits into the one-shard model.  (What a filtered list holds on the device is
tests/test_gpu_filtered_hits.py's.)"""
import importlib
import os
import re

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afis_labels_create", "afis_labels_free", "afis_rank_hits_filtered", "afis_rank_subject_hits_filtered")
OPTIONS = ("rank_filtered_us", "filter_us")
U64 = np.uint64


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s+afis_labels\s+afis_labels\s*;", code)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):        # dlopen only: no device call
        for name in NEW:
            assert re.search(r"\b(int|void)\s+%s\s*\(afis_ctx\*" % name, code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert getattr(lib, name).argtypes is not None, name
    for method in ("labels_create", "labels_free", "rank_hits_filtered", "rank_subject_hits_filtered"):
        assert hasattr(M.Matcher, method), method
    option_text = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only\)' % opt, option_text), opt
        assert "`%s`" % opt in integration, opt
    assert "0xffffffff" in hdr and "Not in this interface" in hdr            # the no-entry word's caveat, and what is left out (case lists, column lists)


def test_the_kernels_are_product_objects():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "hit_filter.o" in objs and "afis_filter.o" in objs
    assert re.search(r"^hit_filter\.o:\s*hit_filter\.hip", mk, flags=re.M) and re.search(r"^afis_filter\.o:\s*afis_filter\.cpp", mk, flags=re.M)
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "hit_filter.hip")).read()
    assert "__global__" in src and "k_filter_rows" in src and "atomic" not in src.split("#include")[1] and "__shfl" not in src and "__ballot" not in src


def test_the_python_host_builds_the_csr():
    mk, off, ent = M.Matcher._filter_args(3, [[1, 2, 3], [0, 0, 0], [1 << 63, 0, (1 << 64) - 1]], [[5, 5], [], [9]])
    assert mk.dtype == U64 and mk.shape == (3, 3) and int(mk[2, 0]) == 1 << 63 and int(mk[2, 2]) == (1 << 64) - 1
    assert off.tolist() == [0, 2, 2, 3] and ent.tolist() == [5, 5, 9]
    assert M.Matcher._filter_args(2, None, None) == (None, None, None)
    mk, off, ent = M.Matcher._filter_args(2, None, [[], []])
    assert mk is None and off.tolist() == [0, 0, 0] and len(ent) >= 1       # (a pointer to hand over; no entry is read)
    with pytest.raises(ValueError):
        M.Matcher._filter_args(2, None, [[1]])


# ---- the contract as a numpy model ---------------------------------------------------------------------------------------------------------------
def passes(labels, mask):
    any_of, all_of, none_of = (U64(x) for x in mask)
    return ((any_of == 0) | ((labels & any_of) != 0)) & ((labels & all_of) == all_of) & ((labels & none_of) == 0)


def template_hits(rows, glob, labels, masks, excl, thr, cap):
    """rows [n_q][n] over the columns glob [n] with labels [n] -> (n_hits [n_q], idx [n_q][cap], score [n_q][cap]): afis_rank_hits over the eligible cells only."""
    n_q = rows.shape[0]
    n = np.zeros(n_q, np.int64); idx = np.full((n_q, cap), -1, np.int64); sc = np.full((n_q, cap), -np.inf, np.float32)
    for q in range(n_q):
        key = SH.rank_key(rows[q]).astype(np.int64)
        at = np.flatnonzero(passes(labels, masks[q]) & ~np.isin(glob, excl[q]) & (key >= int(SH.rank_key(np.array([thr], np.float32))[0])))
        at = at[np.lexsort((glob[at], -key[at]))]
        n[q] = len(at); idx[q, :min(cap, len(at))] = glob[at[:cap]]; sc[q, :min(cap, len(at))] = rows[q, at[:cap]]
    return n, idx, sc


def subject_hits(rows, glob, subject, labels, masks, excl, thr, cap):
    """... -> (n_hits, subject [n_q][cap], score, best_idx): per person the best ELIGIBLE template (raw-word key, lowest index among equals); excluded ids are no entries."""
    n_q = rows.shape[0]
    n = np.zeros(n_q, np.int64); ids = np.full((n_q, cap), -1, np.int64); sc = np.full((n_q, cap), -np.inf, np.float32); bi = np.full((n_q, cap), -1, np.int64)
    for q in range(n_q):
        key = SH.subject_key(rows[q]).astype(np.int64)
        at = np.flatnonzero(passes(labels, masks[q]) & ~np.isin(subject, excl[q]))
        at = at[np.lexsort((glob[at], -key[at], subject[at]))]              # by person; inside one the greatest key first, equal keys by ascending index
        first = np.ones(len(at), bool); first[1:] = subject[at][1:] != subject[at][:-1]
        best = at[first]
        best = best[key[best] >= int(SH.subject_key(np.array([thr], np.float32))[0])]
        best = best[np.lexsort((subject[best], -key[best]))]
        t = min(cap, len(best))
        n[q] = len(best); ids[q, :t] = subject[best[:t]]; sc[q, :t] = rows[q, best[:t]]; bi[q, :t] = glob[best[:t]]
    return n, ids, sc, bi


def test_the_model_on_a_hand_made_case():
    """Five templates, fingers as one-hot bits 0-2, sex as bits 8-9."""
    F = lambda finger, sex: U64((1 << finger) | (1 << (8 + sex)))
    labels = np.array([F(0, 0), F(1, 0), F(1, 1), F(2, 1), F(0, 1)], U64)
    rows = np.array([[5, 4, 3, 2, 1]] * 4, np.float32)
    glob = np.arange(5, dtype=np.int64) + 100
    allowed = U64((1 << 1) | (1 << 2) | (1 << 9))                           # finger in {1, 2} and sex = 1, as ONE none_of: the complement inside the two fields
    masks = np.array([[0, 0, 0], [0, 0, U64(0x307) & ~allowed], [1 << 0, 1 << 9, 0], [0, 1 << 40, 0]], U64)
    n, idx, sc = template_hits(rows, glob, labels, masks, [[], [], [], []], -np.inf, 3)
    assert n.tolist() == [5, 2, 1, 0] and idx.tolist() == [[100, 101, 102], [102, 103, -1], [104, -1, -1], [-1, -1, -1]]
    n, idx, sc = template_hits(rows, glob, labels, masks, [[100, 100, 7, 9999], [103], [], []], 1.5, 3)
    assert n.tolist() == [3, 1, 0, 0] and idx[0].tolist() == [101, 102, 103] and idx[1].tolist() == [102, -1, -1] and sc[1, 0] == 3
    subject = np.array([7, 7, 7, 9, 9], np.int64)
    n, ids, sc, bi = subject_hits(rows, glob, subject, labels, masks, [[], [], [9], []], -np.inf, 2)
    assert n.tolist() == [2, 2, 0, 0] and ids[:2].tolist() == [[7, 9], [7, 9]] and sc[:2].tolist() == [[5, 2], [3, 2]] and bi[:2].tolist() == [[100, 103], [102, 103]]


# ---- the shard merges -----------------------------------------------------------------------------------------------------------------------------
def search_like(rng, n_q, G):
    """-1, 0 and positives rounded to a few values: the tie rules decide nearly every place; one latent-empty row."""
    u = rng.random((n_q, G))
    m = np.where(u < 0.1, -1.0, np.where(u < 0.5, np.round(rng.random((n_q, G)) * 6) / 2, 0.0)).astype(np.float32)
    m[n_q // 2] = -1
    return m


def finger_cards(rng, G):
    """Ten one-hot finger bits, two for sex, a region code above: a card's ten prints share sex and region."""
    card = np.arange(G) // 10
    sex = rng.integers(0, 2, card.max() + 1)[card]; region = rng.integers(0, 5, card.max() + 1)[card]
    return (U64(1) << (np.arange(G) % 10).astype(U64)) | (U64(1) << (10 + sex).astype(U64)) | (region.astype(U64) << U64(12))


def plans(rng, n_q, G, base, subject):
    fingers = lambda allowed: U64(0x3ff) & ~U64(sum(1 << f for f in allowed))
    masks = np.zeros((n_q, 3), U64)
    masks[1] = (0, 0, fingers({2, 7}) | U64(1 << 10))                       # finger in {2, 7}, sex bit 11
    masks[2] = (U64(0x3 << 12), 0, 0)                                       # any of two region bits
    masks[3] = (0, U64(1 << 11), 0)
    masks[4] = (U64(0x1f), U64(1 << 10), U64(3 << 13))
    masks[5] = (0, U64(1 << 63), 0)                                         # nothing passes
    excl_t = [[] for _ in range(n_q)]; excl_s = [[] for _ in range(n_q)]
    excl_t[0] = [base - 5, base + G + 40, base + 3, base + 3]               # outside the gallery on both sides, a duplicate
    excl_t[2] = (base + rng.permutation(G)[:G // 2]).tolist()
    excl_t[6] = (base + np.arange(G)).tolist()                              # everything
    excl_s[0] = [int(subject[0]), 10 ** 12]                                 # an id nobody holds
    excl_s[3] = np.unique(subject)[::2].tolist()
    excl_s[6] = np.unique(subject).tolist()
    return masks, excl_t, excl_s


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cap", [6, 64])
def test_shards_merge_into_the_one_shard_model(world, cap):
    rng = np.random.default_rng(61 + world)
    G, n_q, base = 400, 8, 5000
    rows = search_like(rng, n_q, G)
    glob = np.arange(G, dtype=np.int64) + base
    labels = finger_cards(rng, G)
    subject = (rng.permutation(G) // 6).astype(np.int64) * 7 + 3            # persons of six prints dealt over the whole gallery: nearly all lie in several shards
    masks, excl_t, excl_s = plans(rng, n_q, G, base, subject)
    for trial in range(3):
        cuts = np.sort(rng.integers(0, G + 1, world - 1)) if trial else np.array([150, 150, 300][:world - 1])
        bounds = list(zip(np.r_[0, cuts], np.r_[cuts, G]))
        assert trial or sum(len({r for r, (lo, hi) in enumerate(bounds) if (subject[lo:hi] == s).any()}) > 1 for s in np.unique(subject)) > 30
        for thr in (-np.inf, 0.0, 2.5, 100.0):
            per = [template_hits(rows[:, lo:hi], glob[lo:hi], labels[lo:hi], masks, excl_t, thr, cap) for lo, hi in bounds]   # the SAME lists on every rank
            n, i, s = SH.merge_hits(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), cap)
            wn, wi, ws = template_hits(rows, glob, labels, masks, excl_t, thr, cap)
            assert np.array_equal(n, wn) and np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (trial, thr)
            assert wn[5] == 0 and wn[6] == 0 and ((wn == 0).all() if thr == 100.0 else wn[0] > 0)
            per = [subject_hits(rows[:, lo:hi], glob[lo:hi], subject[lo:hi], labels[lo:hi], masks, excl_s, thr, cap) for lo, hi in bounds]
            n, trunc, i, s, b = SH.merge_subject_hits(*(np.stack([p[j] for p in per]) for j in range(4)), cap)
            wn, wi, ws, wb = subject_hits(rows, glob, subject, labels, masks, excl_s, thr, cap)
            assert np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)) and np.array_equal(b, wb), (trial, thr)   # a filtered maximum is still a maximum
            for q in range(n_q):
                assert n[q] == wn[q] if not trunc[q] else n[q] <= wn[q], (trial, thr, q)
            assert wn[5] == 0 and wn[6] == 0 and not np.isin(wi[3], excl_s[3]).any()
