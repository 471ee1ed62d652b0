"""Person distributions on the GPU: afis_subject_score_stats, afis_subject_score_histogram, afis_subject_entries_at.

The yardstick is numpy built from the planted matrix, never the code under test: per (query, person) the maximum of ordered(raw word) over the person's eligible
covered columns, ties to the lowest column (0: no cell); an entry is a maximum >= the ordered word of -inf; the bins are np.searchsorted(ordered(edges), maximum,
side="right"); the lists a lexsort on (maximum descending, subject id ascending); the statistics tests/test_gpu_score_stats.py's model over the persons' words, sums
in Python integers.  Everything is compared exactly: counts as integers, scores as words, statistics as bytes; there is no tolerance anywhere.

Matrices are planted with the tap afis_debug_rank_hits, which leaves its matrix rankable, on a packed gallery of one-point templates (the recipe of
tests/test_gpu_score_hist.py); index_base is 1000.  The kernels read a matrix of 4-byte person cells [n_q][S]: the numbers of persons sit before, on and after the
column chunks of the histogram and select kernels (csrc/afis_device.h: kShChunkScalar 256, kShChunkVec 1024, kSelChunkScalar 1024, kSelChunkVec 4096; a row whose
length is a multiple of four takes the 16-byte form), n_q either side of a strip of kFilterRows = 8 rows, the targets per row around kSelTargetChunk = 16."""
import importlib
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
SY = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")

SEED = 5527
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NINF = float("-inf")
NO_ENTRY_WORD = np.uint32(0xffffffff)
FLOOR = 0x007fffff                                                          # the ordered word of -inf
LISTED, NO_ENTRY = 0, 1
U64 = np.uint64
EDGES_MAX, COUNTS_MAX = 1023, 1 << 24
N_PERSONS = (1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 1028, 4095, 4096, 4097, 4100)
N_Q = (1, 7, 8, 9, 17)
N_EDGES = (1, 2, 63, 64, 65, 255, 256, 1023)
PER_ROW = (1, 15, 16, 17, 40)
G_MAX = 3 * max(N_PERSONS)                                                  # 12 300 templates
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0xbf800000, 0x47800000, 0x477fffff, 0x35000000, 0x35c00000, 0xffffffff],
                   np.uint32).view(np.float32)                              # +-0, +-inf, +-NaN, -1, 65536, the float below it, two small values, no entry


@pytest.fixture(scope="module")
def tiny(codebook_bytes):
    """12 300 rolled templates of one minutia and one texture point each, made as one packed gallery."""
    cb = T.Codebook.from_bytes(codebook_bytes)
    G = G_MAX
    rng = np.random.default_rng(SEED)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    return SY.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
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


def edge_words(edges):
    return ordered(np.asarray(edges, np.float32).view(np.uint32))


class Persons:
    """The person cells of a planted matrix.  rows [n_q][C] float32 in the device's column order, col_subject [C] the subject id of every column, glob [C] its global
    index, ids [S] the handle's distinct ids ascending (persons the columns do not hold stay without a cell), ok [n_q][C] the eligible cells (None: all), excl: per
    query the excluded subject ids (None: none).  K [n_q][S] the maxima (0: no cell), word [n_q][S] the person's score word (0xffffffff: no cell), best [n_q][S] the
    global index of the best template."""

    def __init__(self, rows, col_subject, glob, ids, ok=None, excl=None):
        n_q, C = rows.shape
        self.ids = np.asarray(ids, np.int64); S = len(self.ids)
        w = ordered(rows.view(np.uint32))
        if ok is not None:
            w = np.where(ok, w, np.uint32(0))                              # an ineligible cell is the no-entry word: ordered word 0
        slot = np.searchsorted(self.ids, col_subject)
        assert np.array_equal(self.ids[slot], col_subject)
        self.K = np.zeros((n_q, S), np.uint32); self.word = np.full((n_q, S), NO_ENTRY_WORD, np.uint32); self.best = np.full((n_q, S), -1, np.int64)
        cols = np.arange(C)
        for q in range(n_q):
            o = np.lexsort((cols, -w[q].astype(np.int64)))                  # the greatest word first, equal words by ascending column
            u, first = np.unique(slot[o], return_index=True)                # (a stable sort: a slot's first place in o)
            c = o[first]
            self.K[q, u] = w[q, c]; self.best[q, u] = glob[c]; self.word[q, u] = rows.view(np.uint32)[q, c]
            if excl is not None:
                gone = np.flatnonzero(np.isin(self.ids, np.asarray(excl[q], np.int64)))
                self.K[q, gone] = 0
        none = self.K == 0
        self.word[none] = NO_ENTRY_WORD; self.best[none] = -1
        self.entry = self.K >= FLOOR

    def hist(self, edges, axis):
        K = self.K if axis == 0 else np.ascontiguousarray(self.K.T)
        ek = edge_words(edges)
        assert (np.diff(ek.astype(np.int64)) > 0).all()
        out = np.zeros((K.shape[0], len(ek) + 1), np.int64)
        for r in range(K.shape[0]):
            out[r] = np.bincount(np.searchsorted(ek, K[r][K[r] >= FLOOR], side="right"), minlength=len(ek) + 1)
        return out

    def lists(self, q):
        """The slots of row q in rank order: the maximum descending, equal maxima by ascending id; entries only."""
        o = np.lexsort((self.ids, -self.K[q].astype(np.int64)))
        return o[self.entry[q][o]]

    def entries(self, query, rank):
        lists = {q: self.lists(q) for q in set(int(t) for t in query)}
        n = len(query)
        st = np.full(n, NO_ENTRY, np.int32); sid = np.full(n, -1, np.int64); sc = np.full(n, 0xff800000, np.uint32); bi = np.full(n, -1, np.int64)
        for i, (q, r) in enumerate(zip(query, rank)):
            o = lists[int(q)]
            if r < len(o):
                st[i] = LISTED; sid[i] = self.ids[o[r]]; sc[i] = self.word[q, o[r]]; bi[i] = self.best[q, o[r]]
        return st, sid, sc, bi

    def stats(self, axis):
        return model_stats(self.word.view(np.float32) if axis == 0 else np.ascontiguousarray(self.word.T).view(np.float32))


def model_stats(x):
    """SCORE_STAT per row of float32 cells (tests/test_gpu_score_stats.py's model); the sums in Python int."""
    none = x.view(np.uint32) == NO_ENTRY_WORD
    with np.errstate(invalid="ignore"):
        valued = ~none & np.isfinite(x) & ~np.signbit(x + np.float32(0.0)) & (x < np.float32(65536.0))
        z = x + np.float32(0.0)
    outside = ~none & ~valued
    q = np.where(valued, np.rint(np.where(valued, x, 0).astype(np.float64) * 2 ** 20).astype(np.int64), 0).astype(object)
    s1 = q.sum(axis=1); s2 = (q * q).sum(axis=1)
    out = np.zeros(x.shape[0], M.SCORE_STAT)
    out["n"] = valued.sum(axis=1); out["n_outside"] = outside.sum(axis=1)
    out["s1"] = np.array([int(t) for t in s1], np.uint64)
    out["s2_lo"] = np.array([int(t) & ((1 << 64) - 1) for t in s2], np.uint64); out["s2_hi"] = np.array([int(t) >> 64 for t in s2], np.uint64)
    out["min"] = np.where(valued, z, np.float32(np.inf)).min(axis=1, initial=np.float32(np.inf))
    out["max"] = np.where(valued, z, np.float32(-np.inf)).max(axis=1, initial=np.float32(-np.inf))
    return out


def model_moments(st):
    mean = np.zeros(len(st)); sd = np.zeros(len(st))
    for i, e in enumerate(st):
        n, s1, s2 = int(e["n"]), int(e["s1"]), (int(e["s2_hi"]) << 64) | int(e["s2_lo"])
        if n:
            mean[i] = float(s1) / (float(n) * 1048576.0); sd[i] = math.sqrt(float(n * s2 - s1 * s1)) / (float(n) * 1048576.0)
    return mean, sd


def label_test(labels, masks):
    L = np.asarray(labels, U64)[None, :]; mk = np.asarray(masks, U64)
    a, b, c = mk[:, 0:1], mk[:, 1:2], mk[:, 2:3]
    return ((a == 0) | ((L & a) != 0)) & ((L & b) == b) & ((L & c) == 0)


# ---- matrices, person layouts, edges, targets ---------------------------------------------------------------------------------------------------------------
def matrix(n_q, G, rng, special=0.2):
    """Uniform values with about 20 % special words; row 1 holds one value only (one bin, every key digit equal), row 3 mostly zeros of both signs and -1."""
    rows = rng.uniform(-20, 300, (n_q, G)).astype(np.float32)
    if n_q > 1:
        rows[1] = np.float32(12.5)
    if n_q > 3:
        rows[3] = np.where(rng.random(G) < 0.5, np.float32(0.0), np.where(rng.random(G) < 0.5, np.float32(-0.0), np.float32(-1.0)))
    at = rng.random((n_q, G)) < special
    rows[at] = SPECIAL[rng.integers(0, len(SPECIAL), (n_q, G))][at]
    return rows


def card_sizes(S, G, rng, most=12):
    """S sizes in 1 .. most that add up to G (S <= G <= most x S)."""
    sizes = np.ones(S, np.int64)
    left = G - S
    while left > 0:
        room = np.flatnonzero(sizes < most)
        take = rng.choice(room, min(left, len(room)), replace=False)
        sizes[take] += 1; left -= len(take)
    return sizes


def layout(kind, S, G, rng):
    """subject [G]: the subject id of every template, S distinct ids."""
    if kind == "sparse":
        ids = np.sort(rng.choice(1 << 40, S, replace=False).astype(np.int64)); ids[-1] = (1 << 40) - 1
        ids = np.unique(ids)
        while len(ids) < S:
            ids = np.unique(np.concatenate([ids, rng.integers(0, 1 << 40, S - len(ids))]))
    else:
        ids = 7 + 3 * np.arange(S, dtype=np.int64)
    if kind == "half" and S > 1:                                            # one person on every other column, as many as the others leave: half the gallery where G >= 2 S
        a = min((G + 1) // 2, G - (S - 1))
        sub = np.empty(G, np.int64)
        mine = np.zeros(G, bool); mine[0:2 * a:2] = True
        sub[mine] = ids[S // 2]
        sub[~mine] = np.repeat(np.delete(ids, S // 2), card_sizes(S - 1, G - a, rng, most=G))
        return sub
    sub = np.repeat(ids, card_sizes(S, G, rng))                             # cards of 1 to 12 consecutive templates
    if kind == "interleaved":                                               # A B A: a person's templates scattered over the gallery
        sub = sub[rng.permutation(G)]
    return sub


LAYOUTS = ("cards", "interleaved", "half", "sparse")


def edges_for(n, P, rng):
    """n edges, strictly ascending by ordered word, no NaN: random values, values of the persons themselves (an edge is inclusive from below), -1, BOTH zeros and
    the two infinities."""
    cells = P.word[P.entry].view(np.float32)
    cells = cells[~np.isnan(cells)]
    pool = np.concatenate([rng.uniform(-30, 310, 3 * n + 8).astype(np.float32), rng.choice(cells, min(len(cells), n)) if len(cells) else np.zeros(0, np.float32),
                           np.array([-1.0, -0.0, 0.0, 12.5, -np.inf, np.inf], np.float32)]).astype(np.float32)
    _, first = np.unique(edge_words(pool), return_index=True)
    pool = pool[first]
    must = pool[np.isin(edge_words(pool), edge_words(np.array([-np.inf, np.inf, -0.0, 0.0, 12.5], np.float32)))] if n >= 8 else pool[:0]
    rest = pool[~np.isin(edge_words(pool), edge_words(must))]
    e = np.concatenate([must, rng.choice(rest, n - len(must), replace=False)])
    return e[np.argsort(edge_words(e))]


def rank_plan(P, rng, per_row):
    """Targets: row r gets per_row[r % len(per_row)] of them — ranks 0, entries - 1, entries, 2^40, repeated ranks and random ones — shuffled over the rows."""
    query, rank = [], []
    for r in range(P.K.shape[0]):
        n = per_row[r % len(per_row)]
        entries = int(P.entry[r].sum())
        fixed = [entries, max(entries - 1, 0), 0, 1 << 40, 0, entries // 2, entries // 2]
        rk = (fixed + [int(t) for t in rng.integers(0, entries + 3, max(n - len(fixed), 0))])[:n]
        query += [r] * len(rk); rank += rk
    o = rng.permutation(len(query))
    return np.asarray(query, np.int32)[o], np.asarray(rank, np.int64)[o]


# ---- the three calls against the model --------------------------------------------------------------------------------------------------------------------------
def same_stats(got, want, what):
    assert got.dtype == M.SCORE_STAT and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError((what, bad[:4], got[bad[:2]], want[bad[:2]]))


def check_all(m, hs, P, rng, what, n_edges=64, per_row=PER_ROW, stats=True, **kw):
    if stats:
        for axis in (0, 1):
            same_stats(m.subject_score_stats(hs, axis=axis, **kw), P.stats(axis), (what, "stats", axis))
            assert m.get_option("subject_score_stats_us") > 0
    edges = edges_for(n_edges, P, rng)
    for axis in (0, 1):
        want = P.hist(edges, axis)
        got = m.subject_score_histogram(hs, edges, axis=axis, **kw)
        assert got.dtype == np.int64 and got.shape == want.shape, (what, axis)
        assert np.array_equal(got, want), (what, "histogram", axis, len(edges), np.argwhere(got != want)[:4].tolist())
        assert m.get_option("subject_score_histogram_us") > 0
    query, rank = rank_plan(P, rng, per_row)
    check_entries(m, hs, P, query, rank, what, **kw)
    return edges


def check_entries(m, hs, P, query, rank, what, **kw):
    st, sid, sc, bi = P.entries(query, rank)
    got = m.subject_entries_at(hs, query, rank, **kw)
    bad = np.flatnonzero((got["status"] != st) | (got["subject"] != sid) | (got["score"].view(np.uint32) != sc) | (got["best_idx"] != bi))
    assert len(bad) == 0, (what, "entries", len(bad), [(int(query[i]), int(rank[i]), int(got["status"][i]), int(got["subject"][i]), int(sid[i]), int(got["best_idx"][i]), int(bi[i])) for i in bad[:4]])
    assert len(query) == 0 or m.get_option("subject_entries_at_us") > 0
    return got


def check_against_the_lists(m, hs, P, edges, **kw):
    """The existing calls on the same matrix: the tails of the bins are the hit lists' counts, the entries their lists, and the positions invert the entries."""
    counts = m.subject_score_histogram(hs, edges, axis=0, **kw)
    full = m.rank_subject_hits_filtered(hs, NINF, 4096, **kw)
    assert np.array_equal(counts.sum(axis=1), full["n_hits"]) and np.array_equal(full["n_hits"], P.entry.sum(axis=1))
    for j, e in enumerate(edges):
        assert np.array_equal(counts[:, j + 1:].sum(axis=1), m.rank_subject_hits_filtered(hs, float(e), 1, **kw)["n_hits"]), (j, float(e))
    n_q = P.K.shape[0]
    for q in range(n_q):
        n = min(int(full["n_hits"][q]), 4096)
        got = m.subject_entries_at(hs, np.full(n + 1, q, np.int32), np.arange(n + 1, dtype=np.int64), **kw)
        assert (got["status"][:n] == LISTED).all() and np.array_equal(got["subject"][:n], full["subject"][q, :n]) and np.array_equal(got["best_idx"][:n], full["best_idx"][q, :n])
        assert np.array_equal(got["score"].view(np.uint32)[:n], full["score"][q, :n].view(np.uint32))
        assert got["status"][n] == (NO_ENTRY if n == full["n_hits"][q] else LISTED)
        back = m.rank_subject_positions(hs, np.full(n, q, np.int32), got["subject"][:n], **kw)
        assert (back["status"] == LISTED).all() and np.array_equal(back["n_before"], np.arange(n)) and np.array_equal(back["best_idx"], got["best_idx"][:n])


def g_of(S, i):
    return 3 * S if i % 2 == 0 else 2 * S + 1


# ---- 1: numbers of persons, n_q, n_edges, targets per row, person layouts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", N_PERSONS)
def test_person_counts(S, codebook_bytes, tiny):
    i = N_PERSONS.index(S)
    G = g_of(S, i)
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + S)
    glob = BASE + np.arange(G, dtype=np.int64)
    for j, n_q in enumerate(N_Q):
        sub = layout(LAYOUTS[(i + j) % len(LAYOUTS)], S, G, rng)
        hs = m.subjects_create(sub)
        assert len(hs[2]) == S
        rows = matrix(n_q, G, rng)
        plant(m, rows)
        P = Persons(rows, sub, glob, hs[2])
        check_all(m, hs, P, rng, (S, n_q, LAYOUTS[(i + j) % len(LAYOUTS)]), n_edges=N_EDGES[(i + j) % len(N_EDGES)], per_row=PER_ROW[j:] + PER_ROW[:j])
        m.subjects_free(hs)
    m.close()


@pytest.mark.parametrize("n_edges", N_EDGES)
def test_edge_counts(n_edges, codebook_bytes, tiny):
    S, G, n_q = 1025, 2051, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 100 + n_edges)
    sub = layout("cards", S, G, rng)
    hs = m.subjects_create(sub)
    rows = matrix(n_q, G, rng)
    plant(m, rows)
    P = Persons(rows, sub, BASE + np.arange(G, dtype=np.int64), hs[2])
    check_all(m, hs, P, rng, n_edges, n_edges=n_edges, stats=False)
    m.close()


def test_every_rank_the_lists_and_the_round_trip(codebook_bytes, tiny):
    """Every rank 0 .. S of every row; the hit lists at cap 4096, their counts at every edge, and afis_rank_subject_positions of what comes back."""
    S, G, n_q = 261, 700, 7
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 5)
    sub = layout("interleaved", S, G, rng)
    hs = m.subjects_create(sub)
    rows = matrix(n_q, G, rng)
    plant(m, rows)
    P = Persons(rows, sub, BASE + np.arange(G, dtype=np.int64), hs[2])
    query = np.repeat(np.arange(n_q, dtype=np.int32), S + 1); rank = np.tile(np.arange(S + 1, dtype=np.int64), n_q)
    check_entries(m, hs, P, query, rank, "every rank")
    check_against_the_lists(m, hs, P, edges_for(65, P, rng))
    none = m.subject_entries_at(hs, np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert none["status"].shape == (0,) and m.get_option("subject_entries_at_us") == 0
    m.close()


# ---- 2: the key is the raw ordered word ---------------------------------------------------------------------------------------------------------------------------
def test_the_key_is_the_raw_ordered_word(codebook_bytes, tiny):
    G, n_q = 12, 2
    m = tap_matcher(codebook_bytes, tiny, G)
    sub = np.repeat(np.arange(6, dtype=np.int64) * 5 + 2, 2)                # six persons of two templates: ids 2, 7, 12, 17, 22, 27
    hs = m.subjects_create(sub)
    w = np.empty((n_q, G), np.uint32)
    w[:] = np.array([0x80000000, 0xbf800000,                                # person 2: -0.0 and -1: the best is -0.0
                     0x00000000, 0x80000000,                                # person 7: +0.0 and -0.0: the best is +0.0
                     0x7fc00000, 0x7f800000,                                # person 12: a NaN with the sign clear and +inf: the NaN wins
                     0xffffffff, 0xffffffff,                                # person 17: no template holds an entry
                     0xbf800000, 0xffffffff,                                # person 22: -1 (an empty print) and no entry
                     0x3f800000, 0xffc00000], np.uint32)                    # person 27: 1.0 and a NaN with the sign set
    rows = w.view(np.float32)
    plant(m, rows)
    P = Persons(rows, sub, BASE + np.arange(G, dtype=np.int64), hs[2])
    assert P.word[0].tolist() == [0x80000000, 0x00000000, 0x7fc00000, 0xffffffff, 0xbf800000, 0x3f800000]
    zero = np.array([0.0], np.float32)
    h = m.subject_score_histogram(hs, zero)
    assert h[0].tolist() == [2, 3] and np.array_equal(h, P.hist(zero, 0))   # below +0.0: -1 and the person whose best is -0.0 ...
    assert m.score_histogram(zero)[0].tolist() == [2, 6]                   # ... which the template-level call over the same cells counts above it, with the other zeros
    both = np.array([-0.0, 0.0], np.float32)
    h = m.subject_score_histogram(hs, both)
    assert h[0].tolist() == [1, 1, 3] and np.array_equal(h, P.hist(both, 0))   # three distinct bins: below -0.0, -0.0 itself, from +0.0 on (+0.0, 1.0, the NaN)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.score_histogram(both)                                             # the template form: the two zeros are one value
    with pytest.raises(M.AfisError, match=EINVAL):
        m.subject_score_histogram(hs, both[::-1].copy())
    top = np.array([1.0, np.inf], np.float32)
    assert m.subject_score_histogram(hs, top)[0].tolist() == [3, 1, 1]      # the NaN with the sign clear reaches the last edge
    assert m.subject_score_histogram(hs, top, axis=1).tolist() == [[2, 0, 0], [2, 0, 0], [0, 0, 2], [0, 0, 0], [2, 0, 0], [0, 2, 0]]   # person 17 is counted nowhere
    st = m.subject_score_stats(hs, axis=0)
    same_stats(st, P.stats(0), "the key")
    assert int(st["n"][0]) == 3 and int(st["n_outside"][0]) == 2 and int(st["s1"][0]) == 1 << 20   # valued: -0.0 (q = 0), +0.0, 1.0; outside: the NaN and -1
    st1 = m.subject_score_stats(hs, axis=1)
    same_stats(st1, P.stats(1), "the key, per person")
    assert [int(t) for t in st1["n"]] == [2, 2, 0, 0, 0, 2] and [int(t) for t in st1["n_outside"]] == [0, 0, 2, 0, 2, 0] and np.isposinf(st1["min"][3]) and np.isneginf(st1["max"][3])
    got = m.subject_entries_at(hs, np.zeros(6, np.int32), np.arange(6, dtype=np.int64))
    assert got["subject"].tolist() == [12, 27, 7, 2, 22, -1] and got["status"].tolist() == [LISTED] * 5 + [NO_ENTRY]
    assert got["score"].view(np.uint32).tolist() == [0x7fc00000, 0x3f800000, 0x00000000, 0x80000000, 0xbf800000, 0xff800000] and got["best_idx"].tolist() == [BASE + 4, BASE + 10, BASE + 2, BASE, BASE + 8, -1]
    m.close()


# ---- 3: against the template forms, where rank_key and the raw word agree ------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (255, 1028, 4097))
def test_identity_subjects_equal_the_template_forms(G, codebook_bytes, tiny):
    n_q = 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 200 + G)
    sub = BASE + np.arange(G, dtype=np.int64)                               # subject[i] = c + i: a person is a template, and an id its global index
    hs = m.subjects_create(sub)
    rows = np.where(rng.random((n_q, G)) < 0.2, np.float32(-1.0), np.where(rng.random((n_q, G)) < 0.1, np.float32(0.0), rng.uniform(0, 300, (n_q, G)))).astype(np.float32)
    plant(m, rows)
    edges = np.sort(np.concatenate([rng.uniform(0, 300, 62).astype(np.float32), np.array([-1.0, 0.0], np.float32)]))
    excl = [BASE + rng.integers(0, G, 5).astype(np.int64) for _ in range(n_q)]
    for kw in ({}, dict(excl=excl)):
        for axis in (0, 1):
            assert m.subject_score_stats(hs, axis=axis, **kw).tobytes() == m.score_stats(axis=axis, **kw).tobytes()
            assert np.array_equal(m.subject_score_histogram(hs, edges, axis=axis, **kw), m.score_histogram(edges, axis=axis, **kw))
        query = rng.integers(0, n_q, 200).astype(np.int32); rank = rng.integers(0, G + 2, 200).astype(np.int64)
        a = m.subject_entries_at(hs, query, rank, **kw); b = m.entries_at(query, rank, **kw)
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["subject"], b["idx"]) and np.array_equal(a["best_idx"], b["idx"])
        assert np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32))
    m.close()


# ---- 4: filters and subsets -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (257, 1028))
def test_filters(S, codebook_bytes, tiny):
    G, n_q = 3 * S, 12
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 300 + S)
    sub = layout("cards", S, G, rng)
    hs = m.subjects_create(sub)
    rows = matrix(n_q, G, rng)
    rows[:, sub == hs[2][5]] = NO_ENTRY_WORD.view(np.float32)               # cells as afis_search_eligible leaves them: a whole person unscored, and a third of row 2
    rows[2][rng.random(G) < 0.33] = NO_ENTRY_WORD.view(np.float32)
    plant(m, rows)
    glob = BASE + np.arange(G, dtype=np.int64)
    labels = (U64(1) << rng.integers(0, 10, G).astype(U64)) | (U64(1) << (U64(10) + rng.integers(0, 2, G).astype(U64)))    # a finger and a sex
    masks = np.zeros((n_q, 3), U64)
    for q in range(n_q):
        masks[q] = ((U64(0b11 << (q % 9)), 0, 0), (0, U64(1 << 10), 0), (0, 0, U64(0b111 << (q % 8))), (0, 0, 0))[q % 4]
    excl = [np.concatenate([hs[2][rng.integers(0, S, int(rng.integers(0, 30)))], np.array([1, 1 << 41], np.int64)]) for _ in range(n_q)]   # repeated ids, and ids nobody holds
    excl[0] = np.zeros(0, np.int64)
    hl = m.labels_create(labels)
    before = m.rank_hits(NINF, 64)
    ok = label_test(labels, masks)
    assert not ok.all()
    for what, kw, mk, ex in (("masks", dict(labels=hl, masks=masks), ok, None), ("exclusions", dict(excl=excl), None, excl),
                             ("both", dict(labels=hl, masks=masks, excl=excl), ok, excl), ("plain, after the filtered calls", {}, None, None)):
        P = Persons(rows, sub, glob, hs[2], ok=mk, excl=ex)
        edges = check_all(m, hs, P, rng, what, **kw)
        if what == "both":
            check_against_the_lists(m, hs, P, edges[::8], **kw)
    # an excluded person drops, their templates' cells do not: the template form under the same list, read as template indices, still counts those cells
    person = int(hs[2][7])
    only = [np.array([person], np.int64)] * n_q
    P = Persons(rows, sub, glob, hs[2], excl=only)
    assert (P.K[:, 7] == 0).all() and np.array_equal(m.subject_score_histogram(hs, np.array([0.0], np.float32), excl=only), P.hist(np.array([0.0], np.float32), 0))
    after = m.rank_hits(NINF, 64)
    for key in ("n_hits", "idx", "score"):
        assert np.array_equal(before[key].view(np.uint32) if key == "score" else before[key], after[key].view(np.uint32) if key == "score" else after[key]), key   # the matrix is unwritten
    m.labels_free(hl)
    m.close()


def test_a_subset_listed_out_of_order(codebook_bytes, tiny):
    """The sub-shard stands in ascending global index order; persons none of whose templates the list names have no cell: axis 1 gives them empty outputs, and the
    names — subject ids, best templates — stay global."""
    G, S, n_q = 900, 300, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 21)
    sub = layout("cards", S, G, rng)
    hs = m.subjects_create(sub)
    listed = BASE + rng.permutation(G)[:331].astype(np.int64)               # any order, no repeats
    held = np.sort(listed)                                                  # the device's columns
    covered = np.isin(hs[2], sub[held - BASE])
    assert 0 < covered.sum() < S
    hsub = m.subset_create(listed)
    rows = matrix(n_q, len(held), rng)
    m.debug_rank_rows(rows, 1, subset=hsub)                                 # the matrix in the device's column order
    P = Persons(rows, sub[held - BASE], held, hs[2])
    assert (P.K[:, ~covered] == 0).all()
    check_all(m, hs, P, rng, "subset")
    st = m.subject_score_stats(hs, axis=1)
    assert (st["n"][~covered] == 0).all() and (st["n_outside"][~covered] == 0).all() and np.isposinf(st["min"][~covered]).all() and np.isneginf(st["max"][~covered]).all()
    assert (m.subject_score_histogram(hs, np.array([0.0], np.float32), axis=1)[~covered] == 0).all()
    excl = [hs[2][rng.integers(0, S, 5)] for _ in range(n_q)]
    check_all(m, hs, Persons(rows, sub[held - BASE], held, hs[2], excl=excl), rng, "subset, exclusions", excl=excl)
    m.subset_free(hsub)
    m.close()


# ---- 5: a normalised matrix; person z-norm through afis_normalize_scores --------------------------------------------------------------------------------------
def model_normalized(rows, offset, scale, axis):
    none = rows.view(np.uint32) == NO_ENTRY_WORD
    with np.errstate(invalid="ignore"):
        valued = ~none & np.isfinite(rows) & ~np.signbit(rows + np.float32(0.0)) & (rows < np.float32(65536.0))
    o = np.asarray(offset, np.float64); s = np.asarray(scale, np.float64)
    o, s = (o[:, None], s[:, None]) if axis == 0 else (o[None, :], s[None, :])
    z = ((np.where(valued, rows, 0).astype(np.float64) - o) * s).astype(np.float32)
    return np.where(valued, z.view(np.uint32), NO_ENTRY_WORD).view(np.float32)


@pytest.mark.parametrize("axis", (0, 1))
def test_person_z_norm(axis, codebook_bytes, tiny):
    """The person-level moments, afis_normalize_scores with them, and the subject hit lists at a z threshold: the model's.  On the normalised matrix the histogram and
    the entries are accepted (negative z are ordinary entries) and the statistics refused."""
    S, G, n_q = 257, 771, 17
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 31 + axis)
    sub = layout("cards", S, G, rng)
    hs = m.subjects_create(sub)
    glob = BASE + np.arange(G, dtype=np.int64)
    rows = matrix(n_q, G, rng, special=0.05)
    plant(m, rows)
    st = m.subject_score_stats(hs, axis=axis)
    mean, sd = m.score_moments(st)
    want_mean, want_sd = model_moments(Persons(rows, sub, glob, hs[2]).stats(axis))
    assert np.array_equal(mean, want_mean) and np.array_equal(sd, want_sd) and (sd > 0).all()
    if axis == 0:
        offset, scale = mean, 1.0 / sd
    else:
        offset, scale = m.expand_subject_pairs(hs, mean, 1.0 / sd)          # per person -> per column, in the search's column order
        assert len(offset) == G and np.array_equal(offset, mean[np.searchsorted(hs[2], sub)])
    z = m.normalize_scores(offset, scale, axis=axis, want_scores=True)
    want_z = model_normalized(rows, offset, scale, axis)
    assert np.array_equal(z.view(np.uint32), want_z.view(np.uint32))
    P = Persons(want_z, sub, glob, hs[2])
    assert (P.word.view(np.float32)[P.entry] < 0).any()
    for thr in (-1.0, 0.0, 1.5):
        got = m.rank_subject_hits(hs, thr, 64)
        for q in range(n_q):
            o = P.lists(q); o = o[P.K[q][o] >= edge_words([thr])[0]]
            assert got["n_hits"][q] == len(o) and np.array_equal(got["subject"][q, :min(len(o), 64)], hs[2][o[:64]]), (thr, q)
            assert np.array_equal(got["score"][q, :min(len(o), 64)].view(np.uint32), P.word[q][o[:64]])
    check_all(m, hs, P, rng, "z units", stats=False)
    edges = np.array([-2.0, -1.0, -0.0, 0.0, 1.0], np.float32)
    assert m.subject_score_histogram(hs, edges)[:, 1:3].sum() > 0            # negative z-scores are ordinary entries
    with pytest.raises(M.AfisError, match=ESTATE):
        m.subject_score_stats(hs, axis=axis)
    assert np.array_equal(m.subject_score_histogram(hs, edges), P.hist(edges, 0))   # still rankable
    m.close()


# ---- 6: refused calls -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_matrix_rankable(codebook_bytes, tiny):
    G, n_q = 65, 3
    m = tap_matcher(codebook_bytes, tiny, G)
    other = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 41)
    sub = layout("cards", 30, G, rng)
    hs = m.subjects_create(sub); foreign = other.subjects_create(sub); stale = m.subjects_create(sub)
    m.subjects_free(stale)
    rows = matrix(n_q, G, rng)
    plant(m, rows)
    before = m.rank_subject_hits(hs, NINF, 64)
    good = np.array([0.0, 1.0], np.float32)
    q0, r0 = np.zeros(1, np.int32), np.zeros(1, np.int64)
    refused = [lambda: m.subject_score_stats(hs, axis=2), lambda: m.subject_score_stats(hs, axis=-1), lambda: m.subject_score_histogram(hs, good, axis=2),
               lambda: m.subject_score_histogram(hs, np.zeros(0, np.float32)), lambda: m.subject_score_histogram(hs, np.arange(EDGES_MAX + 1, dtype=np.float32)),
               lambda: m.subject_score_histogram(hs, np.array([0.0, np.nan], np.float32)), lambda: m.subject_score_histogram(hs, np.array([1.0, 1.0], np.float32)),
               lambda: m.subject_score_histogram(hs, np.array([0.0, -0.0], np.float32)), lambda: m.subject_score_histogram(hs, good, masks=np.zeros((n_q, 3), U64)),
               lambda: m.subject_score_histogram(hs, good, n_q=n_q + 1), lambda: m.subject_score_stats(hs, n_q=n_q + 1),
               lambda: m.subject_entries_at(hs, np.array([n_q], np.int32), r0), lambda: m.subject_entries_at(hs, np.array([-1], np.int32), r0),
               lambda: m.subject_entries_at(hs, q0, np.array([-1], np.int64)), lambda: m.subject_entries_at(hs, q0, r0, n_q=n_q + 1),
               lambda: m.subject_entries_at(hs, q0, r0, excl=[np.array([-1], np.int64)] * n_q)]
    for h in (foreign, stale):
        refused += [lambda h=h: m.subject_score_stats(h), lambda h=h: m.subject_score_histogram(h, good), lambda h=h: m.subject_entries_at(h, q0, r0)]
    L = m.lib
    refused += [lambda: m._chk(L.afis_subject_score_stats(m.ctx, hs[0], 0, None, None, None, None, n_q, None)),
                lambda: m._chk(L.afis_subject_score_histogram(m.ctx, hs[0], 0, None, None, None, None, n_q, 2, None, None)),
                lambda: m._chk(L.afis_subject_entries_at(m.ctx, hs[0], None, None, None, None, n_q, 1, None, None, None, None, None, None)),
                lambda: m._chk(L.afis_subject_entries_at(m.ctx, hs[0], None, None, None, None, n_q, -1, None, None, None, None, None, None)),
                lambda: m._chk(L.afis_subject_score_stats(m.ctx, None, 0, None, None, None, None, n_q, None))]
    for i, call in enumerate(refused):
        with pytest.raises(M.AfisError, match=EINVAL):
            call()
        assert all(m.get_option(o) == 0 for o in ("subject_score_stats_us", "subject_score_histogram_us", "subject_entries_at_us")), i   # refused before anything was queued
    after = m.rank_subject_hits(hs, NINF, 64)
    for key in ("n_hits", "subject", "best_idx"):
        assert np.array_equal(before[key], after[key]), key
    check_all(m, hs, Persons(rows, sub, BASE + np.arange(G, dtype=np.int64), hs[2]), rng, "after the refusals", n_edges=2, per_row=(3,))
    other.subjects_free(foreign)
    other.close(); m.close()


def test_more_counts_than_a_call_returns(codebook_bytes, tiny):
    """outputs x (n_edges + 1) above 2^24 is refused — 16 385 queries x 1024 bins —; the same matrix at 16 bins is counted.  And the empty cases queue nothing."""
    n_q = COUNTS_MAX // (EDGES_MAX + 1) + 1
    m = tap_matcher(codebook_bytes, tiny, 1)
    hs = m.subjects_create(np.array([5], np.int64))
    rows = np.arange(n_q, dtype=np.float32).reshape(n_q, 1)
    plant(m, rows)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.subject_score_histogram(hs, np.arange(EDGES_MAX, dtype=np.float32))
    edges = np.arange(15, dtype=np.float32)
    got = m.subject_score_histogram(hs, edges)
    assert np.array_equal(got.argmax(axis=1), np.minimum(np.arange(n_q) + 1, len(edges))) and (got.sum(axis=1) == 1).all()
    m.close()
    m = tap_matcher(codebook_bytes, tiny, 5)
    nobody = m.subjects_create(np.arange(5, dtype=np.int64))
    he = m.subset_create([])                                                # a search that covered no column: empty statistics, zero counts, no entry anywhere, nothing queued
    m.debug_rank_rows(np.zeros((2, 1), np.float32), 1, subset=he)           # (two queries; the tap copies n_q x 0 cells)
    st = m.subject_score_stats(nobody, axis=1)
    assert len(st) == 5 and (st["n"] == 0).all() and np.isposinf(st["min"]).all() and len(m.subject_score_stats(nobody, axis=0)) == 2
    assert m.subject_score_histogram(nobody, np.array([0.0], np.float32), axis=1).tolist() == [[0, 0]] * 5
    got = m.subject_entries_at(nobody, np.array([0, 1], np.int32), np.array([0, 5], np.int64))
    assert got["status"].tolist() == [NO_ENTRY, NO_ENTRY] and got["subject"].tolist() == [-1, -1] and got["best_idx"].tolist() == [-1, -1] and np.isneginf(got["score"]).all()
    assert all(m.get_option(o) == 0 for o in ("subject_score_stats_us", "subject_score_histogram_us", "subject_entries_at_us"))
    m.subset_free(he)
    m.close()


# ---- 7: two contexts over two person-aligned cuts of one gallery ------------------------------------------------------------------------------------------------
def test_two_person_aligned_shards_merge_to_the_whole(codebook_bytes, tiny):
    S, G, n_q = 300, 900, 9
    rng = np.random.default_rng(SEED + 71)
    sub = layout("cards", S, G, rng)
    cut = int(np.flatnonzero(sub == sub[G // 2])[0])                        # the first template of a card: no person straddles the cut
    rows = matrix(n_q, G, rng)
    one = tap_matcher(codebook_bytes, tiny, G)
    h1 = one.subjects_create(sub)
    plant(one, rows)
    edges = edges_for(64, Persons(rows, sub, BASE + np.arange(G, dtype=np.int64), h1[2]), rng)
    whole = {(kind, axis): (one.subject_score_stats(h1, axis=axis) if kind == "stats" else one.subject_score_histogram(h1, edges, axis=axis)) for kind in ("stats", "hist") for axis in (0, 1)}
    per = {k: [] for k in whole}; ids = []
    for lo, hi in ((0, cut), (cut, G)):
        h = tap_matcher(codebook_bytes, tiny, hi - lo, lo, BASE + lo)
        hh = h.subjects_create(sub[lo:hi])
        plant(h, np.ascontiguousarray(rows[:, lo:hi]))
        ids.append(hh[2])
        for axis in (0, 1):
            per[("stats", axis)].append(h.subject_score_stats(hh, axis=axis)); per[("hist", axis)].append(h.subject_score_histogram(hh, edges, axis=axis))
        h.close()
    assert SH.merge_subject_score_stats(per[("stats", 0)], ids, 0).tobytes() == whole[("stats", 0)].tobytes()
    assert np.array_equal(SH.merge_subject_score_histograms(per[("hist", 0)], ids, 0), whole[("hist", 0)])
    names, st = SH.merge_subject_score_stats(per[("stats", 1)], ids, 1)
    assert np.array_equal(names, h1[2]) and st.tobytes() == whole[("stats", 1)].tobytes()
    names, hist = SH.merge_subject_score_histograms(per[("hist", 1)], ids, 1)
    assert np.array_equal(names, h1[2]) and np.array_equal(hist, whole[("hist", 1)])
    one.close()
