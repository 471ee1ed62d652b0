"""Eligible search without a GPU: afis_search_eligible is declared, exported by both libraries and bound by the Python host, its kernel and its driver are product
objects, its two options are documented; a numpy model of the class plan (grouping, eligible sets, pair count, the expand pass) is held against a brute-force loop
over the cells; per-shard eligible matrices, ranked by a model of the PLAIN lists and merged with merge_hits / merge_subject_hits, equal the one-shard model of the
FILTERED lists.  (What the device computes is tests/test_gpu_eligible_search.py's.)"""
import importlib
import os
import re

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
NO_ENTRY = np.uint32(0xFFFFFFFF)                                            # csrc/score_order.h: kNoEntryWord
OPTIONS = ("eligible_classes", "eligible_expand_us")


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+afis_search_eligible\s*\(afis_ctx\*\s*ctx,\s*afis_labels\*\s*labels,\s*const uint64_t\*\s*masks", code)
    taps = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+afis_debug_expand_rows\s*\(afis_ctx\*", taps)
    product, test = M.load_library(), M.load_library(M.TEST_LIB_PATH)       # dlopen only: no device call
    for lib in (product, test):
        assert hasattr(lib, "afis_search_eligible") and lib.afis_search_eligible.argtypes is not None
    assert "afis_search_eligible" in M.EXPORTS and "afis_debug_expand_rows" in M.TAP_EXPORTS
    assert hasattr(test, "afis_debug_expand_rows") and not hasattr(product, "afis_debug_expand_rows")
    for method in ("search_eligible", "debug_expand_rows"):
        assert hasattr(M.Matcher, method), method
    option_text = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only\)' % opt, option_text), opt
        assert "`%s`" % opt in integration, opt
    contract = hdr[hdr.index("Eligible search (no reference counterpart"):hdr.index("int afis_search_eligible")]
    for phrase in ("0xffffffff", "bit for bit", "pairs actually SCORED", "PAYS WHEN LATENTS SHARE MASKS", "afis_rank_subjects", "not in this interface", "CASE lists"):
        assert phrase in contract, phrase


def test_the_kernel_and_the_driver_are_product_objects():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "eligible_expand.o" in objs and "afis_eligible.o" in objs
    assert re.search(r"^TEST_OBJS\s*=\s*\$\(OBJS\)", mk, flags=re.M)          # the test library is the product objects plus the taps
    assert re.search(r"^eligible_expand\.o:\s*eligible_expand\.hip", mk, flags=re.M) and re.search(r"^afis_eligible\.o:\s*afis_eligible\.cpp", mk, flags=re.M)
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "eligible_expand.hip")).read()
    body = src.split("namespace afis {", 1)[1]                                # the code, without the header comment
    assert "__global__" in src and "k_expand_rows" in src and "rows_take_16_bytes" in src and "grid_clamp" in src and "size_t" in body
    assert "atomic" not in body and "__shfl" not in src and "__shared__" not in src and "hipMemset" not in src


# ---- the class plan as a numpy model --------------------------------------------------------------------------------------------------------------
def passes(labels, mask):
    any_of, all_of, none_of = (U64(x) for x in mask)
    return ((any_of == 0) | ((labels & any_of) != 0)) & ((labels & all_of) == all_of) & ((labels & none_of) == 0)


def class_plan(labels, masks):
    """The plan of afis_search_eligible: classes of identical mask triples in order of first query position, members ascending; per class the eligible templates,
    ascending.  -> [(rows, sel)]"""
    order, members = [], {}
    for q, mk in enumerate(np.asarray(masks, U64)):
        key = tuple(int(x) for x in mk)
        if key not in members:
            members[key] = []; order.append(key)
        members[key].append(q)
    return [(np.array(members[key], np.int32), np.flatnonzero(passes(labels, key)).astype(np.int32)) for key in order]


def eligible_matrix(rows, labels, masks):
    """What the call leaves, from a full matrix: per class the sub-matrix [n_c][m] a sub-shard search would give, expanded as k_expand_rows expands it.  -> (words
    [n_q][G] uint32, pairs scored, classes)"""
    full = np.ascontiguousarray(rows, np.float32).view(np.uint32)
    n_q, G = full.shape
    out = np.zeros((n_q, G), np.uint32)
    written = np.zeros((n_q, G), np.int32)
    plan = class_plan(labels, masks)
    pairs = 0
    for members, sel in plan:
        cls = full[np.ix_(members, sel)]                                    # a score depends on nothing but its pair
        inv = np.full(G, -1, np.int32); inv[sel] = np.arange(len(sel), dtype=np.int32)
        for r, q in enumerate(members):
            out[q] = np.where(inv >= 0, cls[r][np.maximum(inv, 0)] if len(sel) else NO_ENTRY, NO_ENTRY)
            written[q] += 1
        pairs += len(members) * len(sel)
    assert (written == 1).all()                                             # every word of the matrix exactly once
    return out, pairs, len(plan)


def random_labels_and_masks(rng, n_q, G):
    labels = (U64(1) << (rng.integers(0, 10, G)).astype(U64)) | (U64(1) << (10 + rng.integers(0, 2, G)).astype(U64)) | (rng.integers(0, 4, G).astype(U64) << U64(12))
    kinds = [(0, 0, 0), (0x3FF, 0, 0), (0, 0, 0x3FF & ~0x84), (1 << 3, 1 << 10, 0), (0, 1 << 50, 0), (3 << 12, 0, 1 << 11), (0x1F, 1 << 11, 1 << 13), (1 << 12, 0, 0)]
    return labels, np.array([kinds[i] for i in rng.integers(0, len(kinds), n_q)], U64)


@pytest.mark.parametrize("n_q, G", [(1, 1), (7, 97), (23, 400), (100, 1000)])
def test_the_class_plan_against_a_cell_loop(n_q, G):
    rng = np.random.default_rng(7 + n_q + G)
    for trial in range(3):
        labels, masks = random_labels_and_masks(rng, n_q, G)
        rows = rng.random((n_q, G)).astype(np.float32)
        got, pairs, classes = eligible_matrix(rows, labels, masks)
        want = np.empty((n_q, G), np.uint32); cells = 0
        for q in range(n_q):                                                # brute force: the label test, cell by cell
            a, b, c = (int(x) for x in masks[q])
            for t in range(G):
                L = int(labels[t])
                ok = (a == 0 or (L & a) != 0) and (L & b) == b and (L & c) == 0
                want[q, t] = rows[q, t].view(np.uint32) if ok else NO_ENTRY
                cells += ok
        assert np.array_equal(got, want) and pairs == cells
        assert classes == len({tuple(int(x) for x in mk) for mk in masks})
        plan = class_plan(labels, masks)
        assert [int(p[0][0]) for p in plan] == sorted(int(p[0][0]) for p in plan)                      # classes in order of first query position
        assert all((np.diff(p[0]) > 0).all() and (np.diff(p[1]) > 0).all() for p in plan)               # members and templates ascending
        assert sorted(int(q) for p in plan for q in p[0]) == list(range(n_q))


def test_the_plan_on_a_hand_made_case():
    F = lambda finger, sex: U64((1 << finger) | (1 << (10 + sex)))
    labels = np.array([F(0, 0), F(1, 0), F(1, 1), F(2, 1), F(0, 1)], U64)
    masks = np.array([[0, 0, 1 << 0], [0, 0, 0], [0, 1 << 50, 0], [0, 0, 1 << 0], [0x3FF, 0, 0]], U64)
    plan = class_plan(labels, masks)
    assert [(p[0].tolist(), p[1].tolist()) for p in plan] == [([0, 3], [1, 2, 3]), ([1], [0, 1, 2, 3, 4]), ([2], []), ([4], [0, 1, 2, 3, 4])]
    rows = np.arange(25, dtype=np.float32).reshape(5, 5)
    words, pairs, classes = eligible_matrix(rows, labels, masks)
    assert pairs == 2 * 3 + 5 + 0 + 5 and classes == 4                       # (0, 0, 0) and "any finger" are two classes, both over the whole shard
    assert (words[2] == NO_ENTRY).all() and words[0].tolist() == [int(NO_ENTRY)] + rows[0, 1:4].view(np.uint32).tolist() + [int(NO_ENTRY)]


# ---- the lists read from such a matrix, and the shard merges ----------------------------------------------------------------------------------------
def template_hits(rows, glob, entry, thr, cap):
    """rows [n_q][n] over the columns glob [n] -> (n_hits, idx, score): afis_rank_hits over the cells where `entry` holds."""
    n_q = rows.shape[0]
    n = np.zeros(n_q, np.int64); idx = np.full((n_q, cap), -1, np.int64); sc = np.full((n_q, cap), -np.inf, np.float32)
    for q in range(n_q):
        key = SH.rank_key(rows[q]).astype(np.int64)
        at = np.flatnonzero(entry[q] & (key >= int(SH.rank_key(np.array([thr], np.float32))[0])))
        at = at[np.lexsort((glob[at], -key[at]))]
        n[q] = len(at); idx[q, :min(cap, len(at))] = glob[at[:cap]]; sc[q, :min(cap, len(at))] = rows[q, at[:cap]]
    return n, idx, sc


def subject_hits(rows, glob, subject, entry, thr, cap):
    """... -> (n_hits, subject, score, best_idx): per person the best cell where `entry` holds (raw-word key, lowest index among equals)."""
    n_q = rows.shape[0]
    n = np.zeros(n_q, np.int64); ids = np.full((n_q, cap), -1, np.int64); sc = np.full((n_q, cap), -np.inf, np.float32); bi = np.full((n_q, cap), -1, np.int64)
    for q in range(n_q):
        key = SH.subject_key(rows[q]).astype(np.int64)
        at = np.flatnonzero(entry[q])
        at = at[np.lexsort((glob[at], -key[at], subject[at]))]
        first = np.ones(len(at), bool); first[1:] = subject[at][1:] != subject[at][:-1]
        best = at[first]
        best = best[key[best] >= int(SH.subject_key(np.array([thr], np.float32))[0])]
        best = best[np.lexsort((subject[best], -key[best]))]
        t = min(cap, len(best))
        n[q] = len(best); ids[q, :t] = subject[best[:t]]; sc[q, :t] = rows[q, best[:t]]; bi[q, :t] = glob[best[:t]]
    return n, ids, sc, bi


def search_like(rng, n_q, G):
    """-1, 0 and positives rounded to a few values: the tie rules decide nearly every place; one latent-empty row."""
    u = rng.random((n_q, G))
    m = np.where(u < 0.1, -1.0, np.where(u < 0.5, np.round(rng.random((n_q, G)) * 6) / 2, 0.0)).astype(np.float32)
    m[n_q // 2] = -1
    return m


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cap", [6, 64])
def test_per_shard_eligible_matrices_merge_into_the_one_shard_filtered_model(world, cap):
    """Every rank labels its own shard and takes the same masks; the plain lists read from each rank's eligible matrix are merge input as they are."""
    rng = np.random.default_rng(83 + world)
    G, n_q, base = 400, 9, 5000
    rows = search_like(rng, n_q, G)
    glob = np.arange(G, dtype=np.int64) + base
    labels, masks = random_labels_and_masks(rng, n_q, G)
    masks[5] = (0, 1 << 50, 0)                                              # nothing passes
    subject = (rng.permutation(G) // 6).astype(np.int64) * 7 + 3            # persons of six prints dealt over the whole gallery: nearly all lie in several shards
    ok = np.stack([passes(labels, masks[q]) for q in range(n_q)])
    for trial in range(3):
        cuts = np.sort(rng.integers(0, G + 1, world - 1)) if trial else np.array([150, 150, 300][:world - 1])
        bounds = list(zip(np.r_[0, cuts], np.r_[cuts, G]))
        shards = []
        for lo, hi in bounds:                                               # what each rank's afis_search_eligible leaves, and what the plain lists take for an entry
            words, pairs, _ = eligible_matrix(rows[:, lo:hi], labels[lo:hi], masks)
            assert pairs == int(ok[:, lo:hi].sum())
            shards.append((words.view(np.float32), words != NO_ENTRY))
        for thr in (-np.inf, float(np.nextafter(np.float32(0), np.float32(1))), 2.5, 100.0):
            per = [template_hits(w, glob[lo:hi], e, thr, cap) for (w, e), (lo, hi) in zip(shards, bounds)]
            n, i, s = SH.merge_hits(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), cap)
            wn, wi, ws = template_hits(rows, glob, ok, thr, cap)            # the one-shard model of afis_rank_hits_filtered
            assert np.array_equal(n, wn) and np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (trial, thr)
            assert wn[5] == 0 and ((wn == 0).all() if thr == 100.0 else wn.sum() > 0)
            per = [subject_hits(w, glob[lo:hi], subject[lo:hi], e, thr, cap) for (w, e), (lo, hi) in zip(shards, bounds)]
            n, trunc, i, s, b = SH.merge_subject_hits(*(np.stack([p[j] for p in per]) for j in range(4)), cap)
            wn, wi, ws, wb = subject_hits(rows, glob, subject, ok, thr, cap)
            assert np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)) and np.array_equal(b, wb), (trial, thr)
            for q in range(n_q):
                assert n[q] == wn[q] if not trunc[q] else n[q] <= wn[q], (trial, thr, q)
