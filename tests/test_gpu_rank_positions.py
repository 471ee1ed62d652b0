"""Rank positions on the GPU: afis_rank_positions, afis_rank_subject_positions, afis_count_before.

The yardstick throughout is numpy.  The position of a target is its place in the lexsort order of its row's ENTRIES:
  templates  key = ordered bits of (score + 0.0f), descending, ties by ascending global index; an entry is an eligible cell whose key reaches the key of -inf
  persons    key = ordered bits of the raw word of the person's best eligible covered score (the lowest index among equal words), ties by ascending subject id
and the same sentence is held against the sibling that makes the list: idx[q][n_before] == target in afis_rank_hits(-inf, 4096) wherever the position is inside it.

Matrices are planted with the tap afis_debug_rank_hits, which leaves its matrix rankable.  The counting kernel works on column chunks of 1024 (one column per load) or,
where the row length is a multiple of four, 4096 (16-byte loads), and stages 64 targets of a row at a time (csrc/afis_device.h: kPosChunkScalar, kPosChunkVec,
kPosTargetChunk), its chunks dealt to at most 32 workgroups per column chunk: the sizes sit before, on and after those edges.  index_base is never 0."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")

SEED = 6151
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
LISTED, NO_ENTRY, NOT_COVERED = 0, 1, 2
NINF = float("-inf")
NEG_INF = np.float32(-np.inf).view(np.uint32)
FLOOR = 0x007fffff                                                          # the ordered word of -inf
NO_ENTRY_WORD = np.uint32(0xffffffff)
U64 = np.uint64
CHUNK_SCALAR, CHUNK_VEC, TARGET_CHUNK = 1024, 4096, 64
TARGET_DEPTH = 32                                                           # rank_position.hip: kCbDepth, the workgroups that share one row's target chunks
G_IDENTITY = (1, 63, 64, 65, 1023, 1025, 4095, 4096)
G_LARGE = (4097, 9001, 70001, CHUNK_VEC - 4, CHUNK_VEC + 4, 2 * CHUNK_VEC, 2 * CHUNK_SCALAR + 1)   # past the list kernels' reach; before / after / two chunks of each form
G_SUBJECTS = (65, 1025, 4099)
SPECIAL = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x3fc00000, 0xbf800000, 0x40500000], np.uint32).view(np.float32)   # +-inf, +-0, +-NaN, 1.5, -1, 3.25


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """70 001 rolled templates of one minutia and one texture point each (the recipe of tests/test_gpu_rank_hits.py), made as one packed gallery."""
    G = max(G_LARGE)
    rng = np.random.default_rng(SEED)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    return S.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
                           off.copy(), rng.integers(0, 30, G).astype(np.int16), rng.integers(0, 30, G).astype(np.int16), rng.uniform(-1.5, 1.5, G).astype(np.float32),
                           rng.integers(0, cb.K, (G, cb.M)).astype(np.uint8))


def tap_matcher(cbb, tiny, G, lo=0, base=BASE):
    m = M.Matcher(cbb, taps=True)
    m.gallery_add_packed(tiny.slice(lo, lo + G)); m.gallery_commit(base)
    return m


def plant(m, rows):
    """The matrix of the "last search": uploaded by the tap, which leaves it rankable."""
    m.debug_rank_hits(None, rows, NINF, 1)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------
def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def template_key(x):
    return ordered((np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32))


def subject_key(x):
    return ordered(np.asarray(x, np.float32).view(np.uint32))


def label_test(labels, masks):
    """ok [n_q][n]: the label of column j passes query q's (any_of, all_of, none_of)."""
    L = np.asarray(labels, U64)[None, :]; mk = np.asarray(masks, U64)
    a, b, c = mk[:, 0:1], mk[:, 1:2], mk[:, 2:3]
    return ((a == 0) | ((L & a) != 0)) & ((L & b) == b) & ((L & c) == 0)


def not_excluded(names, excl, n_q):
    ok = np.ones((n_q, len(names)), bool)
    for q in range(n_q):
        ok[q] = ~np.isin(names, np.asarray(excl[q], np.int64))
    return ok


class TemplateModel:
    """status / n_before / score words per CELL of scores [n_q][n] whose column j is template glob[j]; ok: the eligible cells (None: all)."""

    def __init__(self, scores, glob, ok=None):
        self.words = scores.view(np.uint32); self.glob = np.asarray(glob, np.int64)
        n_q, n = scores.shape
        key = template_key(scores).astype(np.int64)
        self.entry = (key >= FLOOR) & (np.ones((n_q, n), bool) if ok is None else ok)
        self.pos = np.full((n_q, n), -1, np.int64)
        self.order = []
        for q in range(n_q):
            o = np.lexsort((self.glob, -key[q]))
            o = o[self.entry[q][o]]
            self.pos[q, o] = np.arange(len(o)); self.order.append(o)
        self.col_of = {int(g): j for j, g in enumerate(self.glob)}

    def answer(self, query, idx):
        st = np.empty(len(query), np.int32); nb = np.empty(len(query), np.int64); sc = np.empty(len(query), np.uint32)
        for i, (q, g) in enumerate(zip(query, idx)):
            j = self.col_of.get(int(g))
            if j is None: st[i], nb[i], sc[i] = NOT_COVERED, -1, NEG_INF
            elif self.entry[q, j]: st[i], nb[i], sc[i] = LISTED, self.pos[q, j], self.words[q, j]
            else: st[i], nb[i], sc[i] = NO_ENTRY, -1, NEG_INF
        return {"status": st, "n_before": nb, "score": sc}

    def count_before(self, q, score, idx):
        key = template_key(self.words[q].view(np.float32)).astype(np.int64); k = int(template_key(np.array([score], np.float32))[0])
        e = self.entry[q] & (self.glob != idx)
        return int((e & ((key > k) | ((key == k) & (self.glob < idx)))).sum())


class SubjectModel:
    """The persons of scores [n_q][n] (column j: template glob[j] of person subject[j]); ok: the eligible cells; excl: per query the excluded ids; held: the handle's ids."""

    def __init__(self, scores, glob, subject, held, ok=None, excl=None):
        words = scores.view(np.uint32); glob = np.asarray(glob, np.int64); subject = np.asarray(subject, np.int64)
        n_q, n = scores.shape
        ok = np.ones((n_q, n), bool) if ok is None else ok
        self.held = set(int(s) for s in held); self.rows = []
        for q in range(n_q):
            at = np.flatnonzero(ok[q])
            key = subject_key(scores[q]).astype(np.int64)
            o = at[np.lexsort((glob[at], -key[at], subject[at]))]           # by person; inside one the greatest word first, equal words by ascending index
            first = np.ones(len(o), bool); first[1:] = subject[o][1:] != subject[o][:-1]
            best = o[first]
            best = best[key[best] >= FLOOR]
            if excl is not None:
                best = best[~np.isin(subject[best], np.asarray(excl[q], np.int64))]
            rank = best[np.lexsort((subject[best], -key[best]))]            # word descending, id ascending
            self.rows.append({int(subject[j]): (r, int(words[q, j]), int(glob[j])) for r, j in enumerate(rank)})

    def answer(self, query, ids):
        n = len(query)
        st = np.empty(n, np.int32); nb = np.empty(n, np.int64); sc = np.empty(n, np.uint32); bi = np.empty(n, np.int64)
        for i, (q, s) in enumerate(zip(query, ids)):
            if int(s) not in self.held: st[i], nb[i], sc[i], bi[i] = NOT_COVERED, -1, NEG_INF, -1
            elif int(s) in self.rows[q]: st[i] = LISTED; nb[i], sc[i], bi[i] = self.rows[q][int(s)]
            else: st[i], nb[i], sc[i], bi[i] = NO_ENTRY, -1, NEG_INF, -1
        return {"status": st, "n_before": nb, "score": sc, "best_idx": bi}


def as_words(r):
    return {k: (v.view(np.uint32) if k == "score" else v) for k, v in r.items()}


def assert_same(got, want, what=""):
    got = as_words(got)
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key, np.flatnonzero(got[key] != want[key])[:6].tolist(),
                                                                                          got[key][got[key] != want[key]][:6].tolist(), want[key][got[key] != want[key]][:6].tolist())


def matrix(G, rng, no_entry=True):
    """Six rows: 0 all-distinct values, 1 nine distinct values (ties everywhere), 2 the special words, 3 all +0.0, 4 99 % zero, 5 search-like with no-entry words planted."""
    rows = np.empty((6, G), np.float32)
    rows[0] = rng.permutation(G).astype(np.float32) - np.float32(G // 3)
    rows[1] = np.round(rng.random(G) * 8)
    rows[2] = SPECIAL[rng.integers(0, len(SPECIAL), G)]
    rows[3] = 0.0
    rows[4] = np.where(rng.random(G) < 0.99, 0.0, rng.random(G) * 5 + 0.01)
    u = rng.random(G)
    rows[5] = np.where(u < 0.05, -1.0, np.where(u < 0.15, rng.random(G) * 5 + 0.01, 0.0))
    if no_entry:
        rows[5].view(np.uint32)[rng.random(G) < 0.2] = NO_ENTRY_WORD
    return rows


def every_cell(n_q, glob, rng):
    q, j = np.divmod(rng.permutation(n_q * len(glob)), len(glob))
    return q.astype(np.int32), np.asarray(glob, np.int64)[j]


def held_against_the_list(m, got, query, idx, n_q, hits=None):
    """idx[q][n_before] == target for every listed target inside the list, and per row the listed positions are exactly 0 .. n_hits - 1."""
    hits = m.rank_hits(NINF, 4096) if hits is None else hits
    listed = got["status"] == LISTED
    inside = listed & (got["n_before"] < 4096)
    assert np.array_equal(hits["idx"][query[inside], got["n_before"][inside]], idx[inside])
    assert np.array_equal(hits["score"].view(np.uint32)[query[inside], got["n_before"][inside]], got["score"].view(np.uint32)[inside])
    for q in range(n_q):
        mine = listed & (query == q)
        assert np.array_equal(np.sort(got["n_before"][mine]), np.arange(hits["n_hits"][q])), q
    return hits


# ---- 1: the identity ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", G_IDENTITY)
def test_every_cell_is_a_target(G, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    rows = matrix(G, rng)
    glob = BASE + np.arange(G)
    plant(m, rows)
    model = TemplateModel(rows, glob)
    query, idx = every_cell(6, glob, rng)
    got = m.rank_positions(query, idx)
    assert_same(got, model.answer(query, idx), G)
    held_against_the_list(m, got, query, idx, 6)
    words = rows.view(np.uint32)[query, idx - BASE]
    gone = (words == 0xffc00000) | (words == NO_ENTRY_WORD)
    assert (got["status"][gone] == NO_ENTRY).all() and (got["status"][~gone] == LISTED).all()
    if G >= 63:
        assert gone.any() and (words == 0x7fc00000).any()
    # a cell's own score and index, as a hypothetical entry: the same count
    num = ~gone & ~np.isnan(got["score"])                                  # (a NaN score is AFIS_EINVAL for afis_count_before)
    assert np.array_equal(m.count_before(query[num], rows[query[num], idx[num] - BASE], idx[num]), got["n_before"][num])
    assert m.get_option("rank_positions_us") > 0
    m.close()


# ---- 2: sizes past the list kernels' reach ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", G_LARGE)
def test_positions_beyond_the_lists(G, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 3 * G)
    rows = matrix(G, rng)
    glob = BASE + np.arange(G)
    plant(m, rows)
    model = TemplateModel(rows, glob)
    n = 400
    query = rng.integers(0, 6, n).astype(np.int32)
    idx = BASE + np.r_[rng.integers(0, G, n - 8), [0, G - 1, G - 2, G - 3, G - 4, G - 5, min(G - 1, CHUNK_SCALAR), min(G - 1, CHUNK_VEC)]].astype(np.int64)
    got = m.rank_positions(query, idx)
    want = model.answer(query, idx)
    assert_same(got, want, G)
    assert (got["n_before"][got["status"] == LISTED] < 4096).any() and ((got["n_before"] > 4096).any() or G < 2 * CHUNK_VEC)
    hits = m.rank_hits(NINF, 4096)
    inside = (got["status"] == LISTED) & (got["n_before"] < 4096)
    assert np.array_equal(hits["idx"][query[inside], got["n_before"][inside]], idx[inside])
    ok = (got["status"] == LISTED) & ~np.isnan(got["score"])
    hyp = rng.choice(np.array([-np.inf, -1.0, 0.0, 0.5, 3.25, np.inf], np.float32), n)
    anywhere = np.where(rng.random(n) < 0.5, idx, rng.integers(0, BASE + G + 50, n)).astype(np.int64)   # covered or not, before the shard and past it
    cb_got = m.count_before(query, hyp, anywhere)
    assert np.array_equal(cb_got, np.array([model.count_before(int(q), s, int(i)) for q, s, i in zip(query, hyp, anywhere)], np.int64))
    assert np.array_equal(m.count_before(query[ok], got["score"][ok], idx[ok]), got["n_before"][ok])
    m.close()


# ---- 3: target-table shapes ---------------------------------------------------------------------------------------------------------------------------------
def test_target_tables(codebook_bytes, tiny):
    G = 1025
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 5)
    rows = matrix(G, rng)
    glob = BASE + np.arange(G)
    plant(m, rows)
    model = TemplateModel(rows, glob)
    for n in (1, 63, TARGET_CHUNK - 1, TARGET_CHUNK, TARGET_CHUNK + 1, 2 * TARGET_CHUNK, 2 * TARGET_CHUNK + 1, 1000, TARGET_DEPTH * TARGET_CHUNK + TARGET_CHUNK + 1):
        for q in (1, 5):                                                    # every other query has no target
            query = np.full(n, q, np.int32); idx = BASE + rng.integers(0, G, n).astype(np.int64)
            assert_same(m.rank_positions(query, idx), model.answer(query, idx), (n, q))
    # duplicates, unsorted, rows 0 and 3 without targets, a target outside the shard between the others
    query = np.array([4, 1, 4, 2, 1, 4, 5, 2, 4, 4], np.int32)
    idx = BASE + np.array([7, 7, 7, 1024, 0, 7, 500, -3, 1025, 6], np.int64)
    got = m.rank_positions(query, idx)
    assert_same(got, model.answer(query, idx), "duplicates")
    assert got["status"][7] == NOT_COVERED and got["status"][8] == NOT_COVERED and got["n_before"][0] == got["n_before"][2] == got["n_before"][5]
    us = m.get_option("rank_positions_us")
    assert us > 0
    none = m.rank_positions(np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert none["status"].shape == (0,) and m.get_option("rank_positions_us") == 0
    assert m.count_before(np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int64)).shape == (0,)
    only_outside = m.rank_positions(np.array([0, 1], np.int32), np.array([5, BASE + G], np.int64))      # nothing the search covers: nothing is queued
    assert only_outside["status"].tolist() == [NOT_COVERED, NOT_COVERED] and (only_outside["n_before"] == -1).all() and np.isneginf(only_outside["score"]).all()
    assert m.get_option("rank_positions_us") == 0
    m.close()


# ---- 4: a real search -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_set(cb):
    lats = S.make_latents(91, 4)
    gal = S.make_packed_gallery(91, 500, cb)
    planted = S.plant_mates(91, gal, cb, lats)
    return lats, gal, planted


def test_a_real_search(codebook_bytes, planted_set):
    lats, gal, planted = planted_set
    G, Q = gal.G, len(lats)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal); m.gallery_commit(BASE)
    r = m.search(lats, k=24, want_scores=True)
    query = np.array([q for q in planted for _ in planted[q]], np.int32)
    idx = np.array([BASE + g for q in planted for g, _ in planted[q]], np.int64)
    model = TemplateModel(r["scores"], BASE + np.arange(G))
    got = m.rank_positions(query, idx)
    assert_same(got, model.answer(query, idx), "mates, full search")
    assert (got["status"] == LISTED).all()
    in_list = 0
    for i, (q, g) in enumerate(zip(query, idx)):
        at = np.flatnonzero(r["topk_idx"][q] == g)
        if len(at):
            assert got["n_before"][i] == at[0]; in_list += 1
    assert in_list >= 1
    out = m.rank_positions(np.array([0, 0, 0], np.int32), np.array([BASE - 1, BASE + G, 3], np.int64))
    assert out["status"].tolist() == [NOT_COVERED] * 3
    # a subset listed out of order
    rng = np.random.default_rng(SEED + 9)
    mates = sorted({int(g) for q in planted for g, _ in planted[q]})
    listed = [int(g) for g in rng.permutation(np.r_[mates[::2], rng.permutation(np.setdiff1d(np.arange(G), mates))[:150]])]
    assert listed != sorted(listed)
    hs = m.subset_create([BASE + g for g in listed])
    rs = m.search_subset(hs, lats, k=24, want_scores=True)                  # scores: column j belongs to listed[j]
    sub_glob = BASE + np.asarray(listed, np.int64)
    sm = TemplateModel(rs["scores"], sub_glob)
    got = m.rank_positions(query, idx)
    assert_same(got, sm.answer(query, idx), "mates, subset")
    assert (got["status"] == NOT_COVERED).any() and (got["status"] == LISTED).any()   # the mates the subset does not list
    allq, alli = every_cell(Q, sub_glob, rng)
    got = m.rank_positions(allq, alli)
    assert_same(got, sm.answer(allq, alli), "every cell of the subset")
    held_against_the_list(m, got, allq, alli, Q)
    hyp = rng.choice(np.array([0.0, 0.5, -1.0], np.float32), 60)
    anyi = BASE + rng.integers(0, G, 60).astype(np.int64)
    anyq = rng.integers(0, Q, 60).astype(np.int32)
    assert np.array_equal(m.count_before(anyq, hyp, anyi), np.array([sm.count_before(int(q), s, int(i)) for q, s, i in zip(anyq, hyp, anyi)], np.int64))
    m.subset_free(hs)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_positions(query, idx)
    m.close()


# ---- 5: filters ---------------------------------------------------------------------------------------------------------------------------------------------------
def filter_plan(G, n_q, rng):
    labels = (U64(1) << rng.integers(0, 10, G).astype(U64)) | (U64(1) << (U64(10) + rng.integers(0, 2, G).astype(U64)))    # a finger and a sex
    masks = np.zeros((n_q, 3), U64)
    for q in range(n_q):
        kind = q % 4
        if kind == 0: masks[q] = (U64(0b11 << (q % 9)), 0, 0)                # one of two fingers
        elif kind == 1: masks[q] = (0, U64(1 << 10), 0)                      # one sex
        elif kind == 2: masks[q] = (0, 0, U64(0b111 << (q % 8)))             # none of three fingers
        else: masks[q] = (0, 0, 0)                                           # everything passes
    excl = [BASE + rng.integers(-5, G + 5, int(rng.integers(0, 40))).astype(np.int64) for _ in range(n_q)]   # some outside the shard, some repeated
    excl[0] = np.zeros(0, np.int64)
    return labels, masks, excl


def test_filters_on_planted_rows(codebook_bytes, tiny):
    G, n_q = 1025, 12                                                       # a strip of the filter pass and a half
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 11)
    rows = np.concatenate([matrix(G, rng, no_entry=False), matrix(G, rng, no_entry=False)])
    glob = BASE + np.arange(G)
    plant(m, rows)
    labels, masks, excl = filter_plan(G, n_q, rng)
    hl = m.labels_create(labels)
    before = m.rank_hits(NINF, 4096)
    query, idx = every_cell(n_q, glob, rng)
    ok_m, ok_e = label_test(labels, masks), not_excluded(glob, excl, n_q)
    for what, kw, ok in (("masks", dict(labels=hl, masks=masks), ok_m), ("exclusions", dict(excl=excl), ok_e), ("both", dict(labels=hl, masks=masks, excl=excl), ok_m & ok_e)):
        model = TemplateModel(rows, glob, ok)
        got = m.rank_positions(query, idx, **kw)
        assert_same(got, model.answer(query, idx), what)
        out = ~ok[query, idx - BASE]
        assert out.any() and (got["status"][out] == NO_ENTRY).all()
        held_against_the_list(m, got, query, idx, n_q, m.rank_hits_filtered(NINF, 4096, **kw))
        lst = (got["status"] == LISTED) & ~np.isnan(got["score"])
        assert np.array_equal(m.count_before(query[lst], got["score"][lst], idx[lst], **kw), got["n_before"][lst]), what
        assert m.get_option("rank_positions_us") > 0
    after = m.rank_hits(NINF, 4096)
    for key in ("n_hits", "idx", "score"):
        assert np.array_equal(before[key].view(np.uint32) if key == "score" else before[key], after[key].view(np.uint32) if key == "score" else after[key]), key   # the matrix is unwritten
    assert_same(m.rank_positions(query, idx), TemplateModel(rows, glob).answer(query, idx), "plain, after the filtered calls")
    m.labels_free(hl)
    m.close()


def test_eligible_search_reads_as_the_filtered_call(codebook_bytes, planted_set):
    lats, gal, planted = planted_set
    G, Q = gal.G, len(lats)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal); m.gallery_commit(BASE)
    rng = np.random.default_rng(SEED + 13)
    labels, masks, excl = filter_plan(G, Q, rng)
    masks[1] = masks[0]                                                     # two latents share a class
    hl = m.labels_create(labels)
    query, idx = every_cell(Q, BASE + np.arange(G), rng)
    full = m.search(lats, k=24, want_scores=True)["scores"]
    want = m.rank_positions(query, idx, labels=hl, masks=masks)
    want_x = m.rank_positions(query, idx, labels=hl, masks=masks, excl=excl)
    assert_same(want, TemplateModel(full, BASE + np.arange(G), label_test(labels, masks)).answer(query, idx), "filtered, full search")
    m.search_eligible(lats, hl, masks)
    assert_same(m.rank_positions(query, idx), as_words(want), "plain after the eligible search")
    assert_same(m.rank_positions(query, idx, excl=excl), as_words(want_x), "exclusions after the eligible search")
    assert_same(m.rank_positions(query, idx, labels=hl, masks=masks, excl=excl), as_words(want_x), "the filtered call after the eligible search")
    m.labels_free(hl)
    m.close()


# ---- 6: persons ---------------------------------------------------------------------------------------------------------------------------------------------------
def subject_plan(G, kind, rng):
    if kind == "identity":
        return 7000 + np.arange(G, dtype=np.int64)
    if kind == "cards":                                                     # cards of ten, ids in shuffled order; one hot subject holds a quarter of the gallery
        ids = rng.permutation(np.unique(rng.integers(0, 1 << 40, 4 * G, dtype=np.int64)))[:G // 10 + 1]
        s = ids[np.arange(G) // 10]
        s[(np.arange(G) >= G // 4) & (np.arange(G) < G // 2)] = ids[0]
        return s
    return rng.permutation(np.unique(rng.integers(0, 1 << 40, 4 * G, dtype=np.int64)))[:max(1, G // 7)][rng.integers(0, max(1, G // 7), G)]   # random labels


@pytest.mark.parametrize("kind", ["cards", "random", "identity"])
@pytest.mark.parametrize("G", G_SUBJECTS)
def test_persons(G, kind, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 7 * G + len(kind))
    rows = matrix(G, rng, no_entry=False)
    subject = subject_plan(G, kind, rng)
    glob = BASE + np.arange(G)
    plant(m, rows)
    h = m.subjects_create(subject)
    held = np.unique(subject)
    unknown = np.setdiff1d(np.r_[held + 1, 0, 1 << 41], held)[:5]
    n_q = 6
    ids = np.r_[held, unknown]
    q, j = np.divmod(rng.permutation(n_q * len(ids)), len(ids))
    query, sid = q.astype(np.int32), ids[j]
    got = m.rank_subject_positions(h, query, sid)
    assert_same(got, SubjectModel(rows, glob, subject, held).answer(query, sid), (G, kind))
    assert (got["status"][np.isin(sid, unknown)] == NOT_COVERED).all() and (got["status"] == LISTED).any()
    lists = m.rank_subject_hits(h, NINF, 4096)
    inside = (got["status"] == LISTED) & (got["n_before"] < 4096)
    assert np.array_equal(lists["subject"][query[inside], got["n_before"][inside]], sid[inside])
    assert np.array_equal(lists["best_idx"][query[inside], got["n_before"][inside]], got["best_idx"][inside])
    assert np.array_equal(lists["score"].view(np.uint32)[query[inside], got["n_before"][inside]], got["score"].view(np.uint32)[inside])
    for qq in range(n_q):
        assert (got["status"][query == qq] == LISTED).sum() == lists["n_hits"][qq]
    if kind == "identity":                                                  # one person per template: the template call, entry for entry, on rows that hold no -0.0
        keep = (query != 2) & ~np.isin(sid, unknown)
        tpl = m.rank_positions(query[keep], sid[keep] - 7000 + BASE)
        for key in ("status", "n_before"):
            assert np.array_equal(tpl[key], got[key][keep]), key
        assert np.array_equal(tpl["score"].view(np.uint32), got["score"].view(np.uint32)[keep]) and np.array_equal(got["best_idx"][keep], sid[keep] - 7000 + BASE)
    # filters: a person all of whose templates are ineligible, and an excluded person
    labels = np.where(subject == held[0], U64(2), U64(1)); labels[rng.random(G) < 0.3] |= U64(4)
    masks = np.tile(np.array([[0, 0, 2]], U64), (n_q, 1)); masks[1] = (0, 0, 4); masks[2] = (0, 0, 0)
    excl = [held[rng.integers(0, len(held), 3)] for _ in range(n_q)]; excl[3] = np.r_[excl[3], unknown[:1]]
    hl = m.labels_create(labels)
    ok = label_test(labels, masks)
    for what, kw, okk, ex in (("masks", dict(labels=hl, masks=masks), ok, None), ("exclusions", dict(excl=excl), None, excl), ("both", dict(labels=hl, masks=masks, excl=excl), ok, excl)):
        got = m.rank_subject_positions(h, query, sid, **kw)
        assert_same(got, SubjectModel(rows, glob, subject, held, okk, ex).answer(query, sid), (G, kind, what))
        lists = m.rank_subject_hits_filtered(h, NINF, 4096, **kw)
        inside = (got["status"] == LISTED) & (got["n_before"] < 4096)
        assert np.array_equal(lists["subject"][query[inside], got["n_before"][inside]], sid[inside]), what
        if okk is not None:
            gone = (sid == held[0]) & (query != 1) & (query != 2)
            assert gone.any() and (got["status"][gone] == NO_ENTRY).all()   # every template of the person fails none_of
        if ex is not None:
            named = [set(e.tolist()) & set(held.tolist()) for e in excl]
            hit = np.array([int(s) in named[qq] for qq, s in zip(query, sid)])
            assert hit.any() and (got["status"][hit] == NO_ENTRY).all()
    m.labels_free(hl)
    m.subjects_free(h)
    m.close()


# ---- 7: shards ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [400, 1024])
def test_two_shards_add_up(cut, codebook_bytes, tiny):
    G, n_q = 1025, 6
    rng = np.random.default_rng(SEED + cut)
    rows = matrix(G, rng)
    w = rows.view(np.uint32); w[w == 0x7fc00000] = 0x40200000                # (afis_count_before takes numbers: the NaN with the sign clear becomes 2.5)
    whole = tap_matcher(codebook_bytes, tiny, G)
    a = tap_matcher(codebook_bytes, tiny, cut)
    b = tap_matcher(codebook_bytes, tiny, G - cut, lo=cut, base=BASE + cut)
    plant(whole, rows); plant(a, np.ascontiguousarray(rows[:, :cut])); plant(b, np.ascontiguousarray(rows[:, cut:]))
    glob = BASE + np.arange(G)
    query, idx = every_cell(n_q, np.r_[glob, BASE + G + 3], rng)            # and a target neither shard covers
    want = whole.rank_positions(query, idx)
    per = [s.rank_positions(query, idx) for s in (a, b)]
    status = np.stack([p["status"] for p in per]); score = np.stack([p["score"] for p in per])
    assert ((status != NOT_COVERED).sum(axis=0) <= 1).all()
    owner = (status != NOT_COVERED).argmax(axis=0)
    own_score = score[owner, np.arange(len(query))]
    live = (status == LISTED).any(axis=0)
    counts = np.zeros((2, len(query)), np.int64)
    for r, s in enumerate((a, b)):
        counts[r, live] = s.count_before(query[live], own_score[live], idx[live])
    assert np.array_equal(counts.sum(axis=0)[live], want["n_before"][live]) and np.array_equal(live, want["status"] == LISTED)
    for r in range(2):                                                      # on the owning rank the count is that rank's own position
        mine = live & (owner == r)
        assert np.array_equal(counts[r, mine], per[r]["n_before"][mine])
    st, sc, nb, own = SH.merge_positions(status, score, counts)
    assert np.array_equal(st, want["status"]) and np.array_equal(nb, want["n_before"]) and np.array_equal(sc.view(np.uint32), want["score"].view(np.uint32))
    assert (own[idx == BASE + G + 3] == -1).all() and (st[idx == BASE + G + 3] == NOT_COVERED).all()
    for s in (whole, a, b):
        s.close()


# ---- 8: arguments and state -------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_states(codebook_bytes, planted_set):
    lats, gal, _ = planted_set
    lats = lats[:3]
    G = 150
    i32p, i64p, fp, u64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal.slice(0, G)); m.gallery_commit(BASE)
    tens = np.arange(G, dtype=np.int64) // 10
    ha = m.subjects_create(tens)
    hl = m.labels_create(np.ones(G, U64))
    q1, i1 = np.array([0, 2], np.int32), np.array([BASE + 3, BASE + 4], np.int64)
    with pytest.raises(M.AfisError, match=ESTATE):                          # before any search
        m.rank_positions(q1, i1, n_q=3)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subject_positions(ha, q1, np.array([1, 2], np.int64), n_q=3)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.count_before(q1, np.zeros(2, np.float32), i1, n_q=3)
    scores = m.search(lats, k=24, want_scores=True)["scores"]
    glob = BASE + np.arange(G)
    n = 2
    st = np.zeros(n, np.int32); nb = np.zeros(n, np.int64); sc = np.zeros(n, np.float32); bi = np.zeros(n, np.int64)
    pq, pi, pst, pnb, psc, pbi = q1.ctypes.data_as(i32p), i1.ctypes.data_as(i64p), st.ctypes.data_as(i32p), nb.ctypes.data_as(i64p), sc.ctypes.data_as(fp), bi.ctypes.data_as(i64p)
    rp, rs, cbf = m.lib.afis_rank_positions, m.lib.afis_rank_subject_positions, m.lib.afis_count_before
    nofilt = (None, None, None, None)
    assert rp(m.ctx, *nofilt, 2, n, pq, pi, pst, pnb, psc) == -1            # n_q is not the search's
    assert rp(m.ctx, *nofilt, 3, -1, pq, pi, pst, pnb, psc) == -1           # n_targets < 0
    for args in ((None, pi, pst, pnb, psc), (pq, None, pst, pnb, psc), (pq, pi, None, pnb, psc), (pq, pi, pst, None, psc), (pq, pi, pst, pnb, None)):
        assert rp(m.ctx, *nofilt, 3, n, *args) == -1                        # a null array with n_targets > 0
    for args in ((None, pi, pst, pnb, psc, pbi), (pq, pi, pst, pnb, psc, None)):
        assert rs(m.ctx, ha[0], *nofilt, 3, n, *args) == -1
    assert rs(m.ctx, None, *nofilt, 3, n, pq, pi, pst, pnb, psc, pbi) == -1
    for args in ((None, psc, pi, pnb), (pq, None, pi, pnb), (pq, psc, None, pnb), (pq, psc, pi, None)):
        assert cbf(m.ctx, *nofilt, 3, n, *args) == -1
    assert cbf(m.ctx, *nofilt, 3, -1, pq, psc, pi, pnb) == -1
    assert rp(m.ctx, *nofilt, 3, 0, None, None, None, None, None) == 0 and m.get_option("rank_positions_us") == 0   # n_targets == 0
    assert rs(m.ctx, ha[0], *nofilt, 3, 0, None, None, None, None, None, None) == 0 and cbf(m.ctx, *nofilt, 3, 0, None, None, None, None) == 0
    for bad_q in (-1, 3):
        with pytest.raises(M.AfisError, match=EINVAL):
            m.rank_positions(np.array([0, bad_q], np.int32), i1)
        with pytest.raises(M.AfisError, match=EINVAL):
            m.rank_subject_positions(ha, np.array([bad_q, 0], np.int32), np.array([1, 2], np.int64))
        with pytest.raises(M.AfisError, match=EINVAL):
            m.count_before(np.array([0, bad_q], np.int32), np.zeros(2, np.float32), i1)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.rank_positions(q1, np.array([BASE, -1], np.int64))                # a negative index
    with pytest.raises(M.AfisError, match=EINVAL):
        m.rank_subject_positions(ha, q1, np.array([-1, 2], np.int64))
    with pytest.raises(M.AfisError, match=EINVAL):
        m.count_before(q1, np.zeros(2, np.float32), np.array([-7, BASE], np.int64))
    with pytest.raises(M.AfisError, match=EINVAL):
        m.count_before(q1, np.array([0.0, np.nan], np.float32), i1)         # a NaN score
    masks = np.zeros((3, 3), U64)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.rank_positions(q1, i1, masks=masks)                               # masks without labels
    off = np.array([0, 2, 1, 1], np.int64); ent = np.zeros(2, np.int64)
    assert rp(m.ctx, None, None, off.ctypes.data_as(i64p), ent.ctypes.data_as(i64p), 3, n, pq, pi, pst, pnb, psc) == -1     # a CSR that decreases
    hb = m.subjects_create(tens + 5); m.subjects_free(hb)
    assert rs(m.ctx, hb[0], *nofilt, 3, n, pq, pi, pst, pnb, psc, pbi) == -1   # a freed handle
    hm = m.labels_create(np.ones(G, U64)); m.labels_free(hm)
    assert rp(m.ctx, hm[0], masks.ctypes.data_as(u64p), None, None, 3, n, pq, pi, pst, pnb, psc) == -1
    # the refused calls left the matrix rankable, and the answers are right through the C ABI
    assert rp(m.ctx, *nofilt, 3, n, pq, pi, pst, pnb, psc) == 0
    assert_same({"status": st, "n_before": nb, "score": sc}, TemplateModel(scores, glob).answer(q1, i1), "through the C ABI")
    assert m.get_option("rank_positions_us") > 0
    sid = np.array([1, 14, 99], np.int64); qs = np.array([0, 1, 2], np.int32)
    assert_same(m.rank_subject_positions(ha, qs, sid), SubjectModel(scores, glob, tens, np.unique(tens)).answer(qs, sid), "persons")
    assert m.get_option("rank_positions_us") > 0
    assert (m.rank_hits(NINF, 24)["n_hits"] == G).all()
    # calls that queue device work take the matrix away; a gallery edit takes the handles too
    qh = m.upload_queries(lats)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_positions(q1, i1)
    m.search_resident(qh, k=24)
    assert (m.rank_positions(q1, i1)["status"] == LISTED).all()
    m.free_queries(qh)
    m.gallery_remove([BASE + 47])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_positions(q1, i1)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.count_before(q1, np.zeros(2, np.float32), i1)
    edited = m.search(lats, k=24, want_scores=True)["scores"]
    with pytest.raises(M.AfisError, match=ESTATE):                          # stale handles
        m.rank_subject_positions(ha, qs, sid)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_positions(q1, i1, labels=hl, masks=masks)
    allq, alli = every_cell(3, glob, np.random.default_rng(SEED))
    assert_same(m.rank_positions(allq, alli), TemplateModel(edited, glob).answer(allq, alli), "after the removal")
    m.subjects_free(ha); m.labels_free(hl)
    m.close()


def test_an_empty_shard(codebook_bytes, planted_set):
    """A search that covered no column — an empty subset: every target is not covered, every count 0, nothing is queued."""
    lats, gal, _ = planted_set
    e = M.Matcher(codebook_bytes)
    e.gallery_add_packed(gal.slice(0, 20)); e.gallery_commit(BASE)
    he = e.subset_create([])
    e.search_subset(he, lats[:2], k=0, want_scores=False)
    hs = e.subjects_create(np.arange(20, dtype=np.int64) // 10)
    got = e.rank_positions(np.array([0, 1], np.int32), np.array([BASE, 5], np.int64))
    assert got["status"].tolist() == [NOT_COVERED, NOT_COVERED] and (got["n_before"] == -1).all() and np.isneginf(got["score"]).all()
    sub = e.rank_subject_positions(hs, np.array([0, 1], np.int32), np.array([0, 7], np.int64))
    assert sub["status"].tolist() == [NOT_COVERED, NOT_COVERED] and (sub["best_idx"] == -1).all()
    assert e.count_before(np.array([0], np.int32), np.array([1.0], np.float32), np.array([BASE], np.int64)).tolist() == [0]
    assert e.get_option("rank_positions_us") == 0
    e.subjects_free(hs); e.subset_free(he)
    e.close()
