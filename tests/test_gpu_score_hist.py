"""Score distributions on the GPU: afis_score_histogram, afis_entries_at.

The yardstick is numpy, never the code under test: a cell's key is ordered((x + 0).view(u32)), an entry is a key >= the key of -inf, the bins are
np.searchsorted(edge keys, key, side="right") over the entries, the lists a lexsort on (key descending, global index ascending).  Everything is compared exactly:
counts as integers, scores as words; there is no tolerance anywhere.

Matrices are planted with the tap afis_debug_rank_hits, which leaves its matrix rankable, on a packed gallery of one-point templates (the recipe of
tests/test_gpu_score_stats.py); index_base is 1000.  The histogram kernel gives a workgroup 256 adjacent columns of a row (one column per thread), or 1024 where the row
length is a multiple of four (16-byte loads) — csrc/afis_device.h: kShChunkScalar, kShChunkVec — and walks strips of 8 rows (kFilterRows); the select's counting kernel
takes 1024 or 4096 columns (kSelChunkScalar, kSelChunkVec) and stages a row's targets 16 at a time (kSelTargetChunk): the sizes sit before, on and after those edges."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")

SEED = 9241
BASE = 1000
EINVAL = "afis error -1"
NINF = float("-inf")
NO_ENTRY_WORD = np.uint32(0xffffffff)
FLOOR = 0x007fffff                                                          # the key of -inf
LISTED, NO_ENTRY = 0, 1
U64 = np.uint64
CHUNK_SCALAR, CHUNK_VEC, STRIP, TARGETS = 256, 1024, 8, 16                  # kShChunkScalar, kShChunkVec, kFilterRows, kSelTargetChunk
SEL_SCALAR, SEL_VEC = 1024, 4096                                            # kSelChunkScalar, kSelChunkVec
EDGES_MAX, COUNTS_MAX = 1023, 1 << 24
TOP = np.uint32(0x477fffff).view(np.float32)
# before, on and after a chunk of each form and of each kernel (a row whose length is a multiple of four takes the 16-byte form), and two chunks + 1
G_SMALL = (1, 3, 4, 63, 64, 65, CHUNK_SCALAR - 1, CHUNK_SCALAR, CHUNK_SCALAR + 1, 2 * CHUNK_SCALAR + 1, CHUNK_VEC - 4, CHUNK_VEC - 1, CHUNK_VEC, CHUNK_VEC + 1, CHUNK_VEC + 4,
           SEL_VEC - 4, SEL_VEC - 1, SEL_VEC, SEL_VEC + 1, SEL_VEC + 4)
G_LARGE = (2 * SEL_SCALAR + 1, 2 * CHUNK_VEC + 4, 2 * SEL_VEC + 4, 70001)
N_Q = (1, 7, 8, 9, 17)
N_EDGES = (1, 2, 63, 64, 65, 255, 256, 1023)
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0xbf800000, 0x47800000, 0x477fffff, 0x35000000, 0x35c00000, 0xffffffff],
                   np.uint32).view(np.float32)                              # tests/test_score_stats_host.py's: +-0, +-inf, +-NaN, -1, 65536, the float below it, two small values, no entry


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """70 001 rolled templates of one minutia and one texture point each, made as one packed gallery."""
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


def key_of(x):
    with np.errstate(invalid="ignore"):
        return ordered((np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32))


def model_hist(scores, edges, axis=0, ok=None):
    """counts [rows or columns][len(edges) + 1] over the entries of ok (None: all)."""
    x = scores if axis == 0 else np.ascontiguousarray(scores.T)
    keep = np.ones(x.shape, bool) if ok is None else (ok if axis == 0 else ok.T)
    key = key_of(x); ek = key_of(edges)
    assert (np.diff(ek.astype(np.int64)) > 0).all()
    out = np.zeros((x.shape[0], len(ek) + 1), np.int64)
    for r in range(x.shape[0]):
        k = key[r][keep[r] & (key[r] >= FLOOR)]
        out[r] = np.bincount(np.searchsorted(ek, k, side="right"), minlength=len(ek) + 1)
    return out


def model_list(row, glob, ok=None):
    """The whole list of a row: the columns in rank order (key descending, equal keys by ascending global index), entries only."""
    key = key_of(row).astype(np.int64)
    o = np.lexsort((glob, -key))
    keep = key[o] >= FLOOR
    if ok is not None:
        keep &= ok[o]
    return o[keep]


def model_entries(scores, glob, query, rank, ok=None):
    lists = {q: model_list(scores[q], glob, None if ok is None else ok[q]) for q in set(int(t) for t in query)}
    st = np.full(len(query), NO_ENTRY, np.int32); ix = np.full(len(query), -1, np.int64); sc = np.full(len(query), np.float32(-np.inf).view(np.uint32), np.uint32)
    for i, (q, r) in enumerate(zip(query, rank)):
        o = lists[int(q)]
        if r < len(o):
            st[i] = LISTED; ix[i] = glob[o[r]]; sc[i] = scores[q].view(np.uint32)[o[r]]
    return st, ix, sc


def label_test(labels, masks):
    L = np.asarray(labels, U64)[None, :]; mk = np.asarray(masks, U64)
    a, b, c = mk[:, 0:1], mk[:, 1:2], mk[:, 2:3]
    return ((a == 0) | ((L & a) != 0)) & ((L & b) == b) & ((L & c) == 0)


def not_excluded(names, excl, n_q):
    ok = np.ones((n_q, len(names)), bool)
    for q in range(n_q):
        ok[q] = ~np.isin(names, np.asarray(excl[q], np.int64))
    return ok


def filter_plan(G, n_q, rng):
    labels = (U64(1) << rng.integers(0, 10, G).astype(U64)) | (U64(1) << (U64(10) + rng.integers(0, 2, G).astype(U64)))    # a finger and a sex
    masks = np.zeros((n_q, 3), U64)
    for q in range(n_q):
        kind = q % 4
        if kind == 0: masks[q] = (U64(0b11 << (q % 9)), 0, 0)
        elif kind == 1: masks[q] = (0, U64(1 << 10), 0)
        elif kind == 2: masks[q] = (0, 0, U64(0b111 << (q % 8)))
        else: masks[q] = (0, 0, 0)
    excl = [BASE + rng.integers(-5, G + 5, int(rng.integers(0, 40))).astype(np.int64) for _ in range(n_q)]   # some outside the shard, some repeated
    excl[0] = np.zeros(0, np.int64)
    return labels, masks, excl


def matrix(n_q, G, rng):
    """Rows in turn: uniform in [0, 300), every cell equal (one bin: the wave aggregation), 99 % zero with a few -1, only no-entry words, the special words sprinkled
    over both signs, keys that differ in the lowest byte only."""
    rows = np.empty((n_q, G), np.float32)
    for r in range(n_q):
        kind = r % 6
        if kind == 0: rows[r] = rng.uniform(0, 300, G)
        elif kind == 1: rows[r] = np.float32(12.5)
        elif kind == 2: rows[r] = np.where(rng.random(G) < 0.99, np.where(rng.random(G) < 0.1, -1.0, 0.0), rng.uniform(0, 300, G))
        elif kind == 3: rows[r] = NO_ENTRY_WORD.view(np.float32)
        elif kind == 4:
            rows[r] = rng.uniform(-50, 50, G)
            at = rng.random(G) < 0.4
            rows[r][at] = SPECIAL[rng.integers(0, len(SPECIAL), G)][at]
        else: rows[r] = (np.uint32(0x42c80000) + rng.integers(0, 256, G).astype(np.uint32)).view(np.float32)   # 100 and the 255 floats after it
    if n_q == 1:
        at = rng.random(G) < 0.3
        rows[0][at] = SPECIAL[rng.integers(0, len(SPECIAL), G)][at]
    return rows


def edges_for(n, rows, rng):
    """n edges, strictly ascending by key, no NaN: random values, values of the cells themselves (an edge is inclusive from below), -1, a zero of either sign and the
    two infinities."""
    cells = rows.reshape(-1)
    cells = cells[~np.isnan(cells)]
    pool = np.concatenate([rng.uniform(-60, 310, 3 * n + 8).astype(np.float32), rng.choice(cells, min(len(cells), n)) if len(cells) else np.zeros(0, np.float32),
                           (np.uint32(0x42c80000) + rng.integers(0, 256, n // 4 + 1).astype(np.uint32)).view(np.float32),
                           np.array([-1.0, -0.0 if n % 2 else 0.0, 12.5, -np.inf, np.inf], np.float32)]).astype(np.float32)
    _, first = np.unique(key_of(pool), return_index=True)
    pool = pool[first]
    must = pool[np.isin(key_of(pool), key_of(np.array([-np.inf, np.inf, 0.0, 12.5], np.float32)))] if n >= 8 else pool[:0]
    rest = pool[~np.isin(key_of(pool), key_of(must))]
    e = np.concatenate([must, rng.choice(rest, n - len(must), replace=False)])
    return e[np.argsort(key_of(e))]


def check_hist(m, rows, edges, what, axes=(0, 1), ok=None, perm=None, **kw):
    for axis in axes:
        if axis == 1 and rows.shape[1] * (len(edges) + 1) > COUNTS_MAX:
            continue
        want = model_hist(rows, edges, axis, ok)
        if axis == 1 and perm is not None:
            want = want[perm]
        got = m.score_histogram(edges, axis=axis, **kw)
        assert got.dtype == np.int64 and got.shape == want.shape, (what, axis)
        assert np.array_equal(got, want), (what, axis, len(edges), np.argwhere(got != want)[:4].tolist())
        assert m.get_option("score_histogram_us") > 0


def check_entries(m, rows, glob, query, rank, what, ok=None, **kw):
    query = np.asarray(query, np.int32); rank = np.asarray(rank, np.int64)
    st, ix, sc = model_entries(rows, glob, query, rank, ok)
    got = m.entries_at(query, rank, **kw)
    bad = np.flatnonzero((got["status"] != st) | (got["idx"] != ix) | (got["score"].view(np.uint32) != sc))
    assert len(bad) == 0, (what, len(bad), [(int(query[i]), int(rank[i]), int(got["status"][i]), int(got["idx"][i]), int(ix[i])) for i in bad[:4]])
    assert len(query) == 0 or m.get_option("entries_at_us") > 0
    return got


def rank_plan(rows, rng, per_row):
    """Targets: row r gets per_row[r % len(per_row)] of them — ranks 0, entries - 1, entries, 2^40, repeated ranks and random ones — shuffled over the rows."""
    query, rank = [], []
    for r in range(rows.shape[0]):
        n = per_row[r % len(per_row)]
        entries = int((key_of(rows[r]) >= FLOOR).sum())
        fixed = [0, max(entries - 1, 0), entries, 1 << 40, 0, entries // 2, entries // 2]
        rk = (fixed + [int(t) for t in rng.integers(0, entries + 3, max(n - len(fixed), 0))])[:n]
        query += [r] * len(rk); rank += rk
    o = rng.permutation(len(query))
    return np.asarray(query, np.int32)[o], np.asarray(rank, np.int64)[o]


PER_ROW = (0, 1, TARGETS - 1, TARGETS, TARGETS + 1, 2 * TARGETS + 1)


# ---- 1: row lengths, n_q, n_edges and matrix kinds; both axes; both calls ----------------------------------------------------------------------------------------
def lengths_case(m, G, n_q, n_edges, rng):
    rows = matrix(n_q, G, rng)
    glob = BASE + np.arange(G, dtype=np.int64)
    plant(m, rows)
    check_hist(m, rows, edges_for(n_edges, rows, rng), (G, n_q))
    query, rank = rank_plan(rows, rng, PER_ROW[n_q % 6:] + PER_ROW[:n_q % 6])
    check_entries(m, rows, glob, query, rank, (G, n_q))
    return rows


@pytest.mark.parametrize("G", G_SMALL)
def test_row_lengths(G, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    for i, n_q in enumerate(N_Q):
        lengths_case(m, G, n_q, N_EDGES[(i + G) % len(N_EDGES)], rng)
    m.close()


@pytest.mark.parametrize("n_edges", N_EDGES)
def test_edge_counts(n_edges, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, SEL_SCALAR + 1)
    rng = np.random.default_rng(SEED + 100 + n_edges)
    rows = lengths_case(m, SEL_SCALAR + 1, 9, n_edges, rng)
    cells = np.unique(rows[0])                                              # every edge a cell of the row: each one opens the bin its own cell falls into
    if len(cells) >= n_edges:
        check_hist(m, rows, cells[:: len(cells) // n_edges][:n_edges], "edges from the cells")
    m.close()


@pytest.mark.parametrize("G", G_LARGE)
def test_long_rows(G, codebook_bytes, tiny):
    """Several workgroups per row: their bins meet in the row's table.  Row 1 holds G equal cells — one bin, and for the select every key digit in one bin: the answer at
    rank r is 1000 + r, found on the position digits alone."""
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    rows = lengths_case(m, G, 9, 255 if G > 60000 else 1023, rng)
    assert (rows[1] == rows[1][0]).all() and (rows[3].view(np.uint32) == NO_ENTRY_WORD).all()
    h = m.score_histogram(np.array([12.5, 13.0], np.float32))
    assert h[1].tolist() == [0, G, 0] and h[3].tolist() == [0, 0, 0]
    rk = np.array([0, 1, 255, 256, 257, 65535 % G, G - 1, G], np.int64)
    got = m.entries_at(np.full(len(rk), 1, np.int32), rk)
    assert got["idx"].tolist() == [BASE + int(r) for r in rk[:-1]] + [-1] and got["status"].tolist() == [LISTED] * 7 + [NO_ENTRY]
    assert (m.entries_at(np.full(3, 3, np.int32), np.array([0, 1, G], np.int64))["status"] == NO_ENTRY).all()
    m.close()


def test_every_rank_and_the_round_trip(codebook_bytes, tiny):
    """Every rank 0 .. G of every row, and afis_rank_positions of what comes back: n_before is the rank."""
    G, n_q = 261, 7
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 5)
    rows = matrix(n_q, G, rng)
    rows[4][:8] = np.array([0.0, -0.0, -0.0, 0.0, np.inf, -np.inf, 1.0, -1.0], np.float32)   # the two zeros tie; a cell's own bits return
    glob = BASE + np.arange(G, dtype=np.int64)
    plant(m, rows)
    query = np.repeat(np.arange(n_q, dtype=np.int32), G + 1); rank = np.tile(np.arange(G + 1, dtype=np.int64), n_q)
    got = check_entries(m, rows, glob, query, rank, "every rank")
    assert (got["score"].view(np.uint32)[got["status"] == LISTED] == 0x80000000).any()      # -0.0 came back as -0.0
    at = got["status"] == LISTED
    back = m.rank_positions(query[at], got["idx"][at])
    assert (back["status"] == LISTED).all() and np.array_equal(back["n_before"], rank[at]) and np.array_equal(back["score"].view(np.uint32), got["score"].view(np.uint32)[at])
    none = m.entries_at(np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert none["status"].shape == (0,) and m.get_option("entries_at_us") == 0
    m.close()


# ---- 2: filters; the tail sums against the hit lists' counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (1025, SEL_VEC + 4))
def test_filters(G, codebook_bytes, tiny):
    n_q = STRIP + 4
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 11 + G)
    rows = matrix(n_q, G, rng)
    glob = BASE + np.arange(G, dtype=np.int64)
    plant(m, rows)
    labels, masks, excl = filter_plan(G, n_q, rng)
    hl = m.labels_create(labels)
    before = m.rank_hits(NINF, 64)
    ok_m, ok_e = label_test(labels, masks), not_excluded(glob, excl, n_q)
    assert not ok_m.all() and not ok_e.all()
    edges = edges_for(65, rows, rng)
    query, rank = rank_plan(rows, rng, PER_ROW)
    for what, kw, ok in (("masks", dict(labels=hl, masks=masks), ok_m), ("exclusions", dict(excl=excl), ok_e), ("both", dict(labels=hl, masks=masks, excl=excl), ok_m & ok_e),
                         ("plain, after the filtered calls", {}, None)):
        check_hist(m, rows, edges, what, ok=ok, **kw)
        check_entries(m, rows, glob, query, rank, what, ok=ok, **kw)
    # the property everything else rests on: a tail of bins is the hit lists' count at that edge, under the same filters
    for kw in ({}, dict(labels=hl, masks=masks, excl=excl)):
        counts = m.score_histogram(edges, axis=0, **kw)
        assert np.array_equal(counts.sum(axis=1), m.rank_hits_filtered(NINF, 1, **kw)["n_hits"])
        for j, e in enumerate(edges):
            assert np.array_equal(counts[:, j + 1:].sum(axis=1), m.rank_hits_filtered(float(e), 1, **kw)["n_hits"]), (j, float(e))
    after = m.rank_hits(NINF, 64)
    for key in ("n_hits", "idx", "score"):
        assert np.array_equal(before[key].view(np.uint32) if key == "score" else before[key], after[key].view(np.uint32) if key == "score" else after[key]), key   # the matrix is unwritten
    m.labels_free(hl)
    m.close()


# ---- 3: a subset listed out of order; a normalised matrix; refused calls ------------------------------------------------------------------------------------------
def test_a_subset_listed_out_of_order(codebook_bytes, tiny):
    """The sub-shard stands in ascending global index order: axis 1 returns in the caller's column order, and equal keys go by global index."""
    G, n_q = 300, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 21)
    listed = BASE + rng.permutation(G)[:131].astype(np.int64)               # any order, no repeats
    held = np.sort(listed)                                                  # the device's columns
    hs = m.subset_create(listed)
    rows = matrix(n_q, len(held), rng)
    rows[0] = np.float32(3.0)                                               # ties only
    m.debug_rank_rows(rows, 1, subset=hs)                                   # the matrix in the device's column order
    edges = edges_for(64, rows, rng)
    check_hist(m, rows, edges, "subset", perm=np.searchsorted(held, listed))
    query, rank = rank_plan(rows, rng, PER_ROW)
    check_entries(m, rows, held, query, rank, "subset")
    got = m.entries_at(np.zeros(4, np.int32), np.arange(4, dtype=np.int64))
    assert got["idx"].tolist() == held[:4].tolist()
    excl = [held[rng.integers(0, len(held), 5)] for _ in range(n_q)]
    check_entries(m, rows, held, query, rank, "subset, exclusions", ok=not_excluded(held, excl, n_q), excl=excl)
    m.subset_free(hs)
    m.close()


def test_a_normalized_matrix_is_accepted(codebook_bytes, tiny):
    G, n_q = 1025, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 31)
    rows = matrix(n_q, G, rng)
    glob = BASE + np.arange(G, dtype=np.int64)
    plant(m, rows)
    z = m.normalize_scores(np.full(n_q, 150.0), np.full(n_q, 0.01), axis=0, want_scores=True)   # z = (v - 150) / 100: most valued cells go negative
    assert (z[0] < 0).any() and (z[0] > 0).any()
    edges = np.array([-2.0, -1.5, -1.0, -0.375, -0.0, 0.25, 1.0, 1.5], np.float32)
    check_hist(m, z, edges, "z units")
    assert m.score_histogram(edges)[0][1:5].sum() > 0                      # negative z-scores are ordinary entries
    query, rank = rank_plan(z, rng, PER_ROW)
    check_entries(m, z, glob, query, rank, "z units")
    m.close()


def test_refused_calls_leave_the_matrix_rankable(codebook_bytes, tiny):
    G, n_q = 65, 3
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 41)
    rows = matrix(n_q, G, rng)
    glob = BASE + np.arange(G, dtype=np.int64)
    plant(m, rows)
    before = m.rank_hits(NINF, G)
    good = np.array([0.0, 1.0], np.float32)
    q0, r0 = np.zeros(1, np.int32), np.zeros(1, np.int64)
    refused = [lambda: m.score_histogram(good, axis=2), lambda: m.score_histogram(np.zeros(0, np.float32)), lambda: m.score_histogram(np.arange(EDGES_MAX + 1, dtype=np.float32)),
               lambda: m.score_histogram(np.array([0.0, np.nan], np.float32)), lambda: m.score_histogram(np.array([1.0, 1.0], np.float32)),
               lambda: m.score_histogram(np.array([1.0, 0.5], np.float32)), lambda: m.score_histogram(np.array([-0.0, 0.0], np.float32)),     # the two zeros are one value
               lambda: m.score_histogram(good, masks=np.zeros((n_q, 3), U64)), lambda: m.score_histogram(good, n_q=n_q + 1),
               lambda: m.entries_at(np.array([n_q], np.int32), r0), lambda: m.entries_at(np.array([-1], np.int32), r0), lambda: m.entries_at(q0, np.array([-1], np.int64)),
               lambda: m.entries_at(q0, r0, masks=np.zeros((n_q, 3), U64)), lambda: m.entries_at(q0, r0, n_q=n_q + 1)]
    L = m.lib
    refused += [lambda: m._chk(L.afis_score_histogram(m.ctx, 0, None, None, None, None, n_q, 2, None, None)),
                lambda: m._chk(L.afis_entries_at(m.ctx, None, None, None, None, n_q, 1, None, None, None, None, None)),
                lambda: m._chk(L.afis_entries_at(m.ctx, None, None, None, None, n_q, -1, None, None, None, None, None))]
    for i, call in enumerate(refused):
        with pytest.raises(M.AfisError, match=EINVAL):
            call()
        assert m.get_option("score_histogram_us") == 0 and m.get_option("entries_at_us") == 0, i   # refused before anything was queued
    after = m.rank_hits(NINF, G)
    for key in ("n_hits", "idx", "score"):
        assert np.array_equal(before[key].view(np.uint32) if key == "score" else before[key], after[key].view(np.uint32) if key == "score" else after[key]), key
    check_hist(m, rows, good, "after the refusals")
    check_entries(m, rows, glob, *rank_plan(rows, rng, (3,)), "after the refusals")
    m.close()


def test_more_counts_than_a_call_returns(codebook_bytes, tiny):
    """outputs x (n_edges + 1) above 2^24 is refused; just below it is counted."""
    G = max(G_LARGE)
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 51)
    rows = matrix(2, G, rng)
    plant(m, rows)
    n_fit = COUNTS_MAX // G - 1                                             # G x (n_fit + 1) <= 2^24 < G x (n_fit + 2)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.score_histogram(np.arange(n_fit + 1, dtype=np.float32), axis=1)
    check_hist(m, rows, np.arange(n_fit, dtype=np.float32), "the most counts", axes=(1,))
    m.close()


# ---- 4: real scores -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_set(cb):
    lats = S.make_latents(93, 3)
    gal = S.make_packed_gallery(93, 300, cb)
    S.plant_mates(93, gal, cb, lats)
    return lats, gal


def test_real_searches(codebook_bytes, planted_set):
    lats, gal = planted_set
    G = gal.G
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal); m.gallery_commit(BASE)
    listed = np.array([BASE + g for g in range(G - 2, 3, -3)], np.int64)   # a subset with the indices in descending order
    hs = m.subset_create(listed)
    rng = np.random.default_rng(SEED + 61)
    for what, search, glob in (("full", lambda: m.search(lats, k=8, want_scores=True), BASE + np.arange(G, dtype=np.int64)), ("subset", lambda: m.search_subset(hs, lats, k=8, want_scores=True), listed)):
        sc = search()["scores"]                                             # columns in the caller's order
        assert (sc > 0).any()
        edges = edges_for(64, sc, rng)
        check_hist(m, sc, edges, what)                                      # (axis 1 in the caller's column order: the model's)
        query = np.repeat(np.arange(len(lats), dtype=np.int32), sc.shape[1] + 1); rank = np.tile(np.arange(sc.shape[1] + 1, dtype=np.int64), len(lats))
        check_entries(m, sc, glob, query, rank, what)
    he = m.subset_create([])                                                # a search that covered no column: zero counts, no entry anywhere, nothing queued
    m.search_subset(he, lats[:2], k=0, want_scores=False)
    assert m.score_histogram(np.array([0.0, 1.0], np.float32)).tolist() == [[0, 0, 0], [0, 0, 0]] and m.score_histogram(np.array([0.0], np.float32), axis=1).shape == (0, 2)
    got = m.entries_at(np.array([0, 1], np.int32), np.array([0, 5], np.int64))
    assert got["status"].tolist() == [NO_ENTRY, NO_ENTRY] and got["idx"].tolist() == [-1, -1] and np.isneginf(got["score"]).all()
    assert m.get_option("score_histogram_us") == 0 and m.get_option("entries_at_us") == 0
    m.subset_free(hs); m.subset_free(he)
    m.close()


# ---- 5: two contexts over the two cuts of one gallery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", (SEL_SCALAR + 1, 700))
def test_two_shards_add_up(cut, codebook_bytes, tiny):
    G, n_q = 2 * SEL_SCALAR + 1, STRIP + 1
    rng = np.random.default_rng(SEED + 71 + cut)
    rows = matrix(n_q, G, rng)
    labels, masks, excl = filter_plan(G, n_q, rng)
    edges = edges_for(255, rows, rng)
    one = tap_matcher(codebook_bytes, tiny, G)
    plant(one, rows)
    h1 = one.labels_create(labels)
    whole = one.score_histogram(edges, labels=h1, masks=masks, excl=excl)
    ok = label_test(labels, masks) & not_excluded(BASE + np.arange(G), excl, n_q)
    assert np.array_equal(whole, model_hist(rows, edges, 0, ok))
    per = []
    for lo, hi in ((0, cut), (cut, G)):
        h = tap_matcher(codebook_bytes, tiny, hi - lo, lo, BASE + lo)
        plant(h, np.ascontiguousarray(rows[:, lo:hi]))
        hl = h.labels_create(labels[lo:hi])
        per.append(h.score_histogram(edges, labels=hl, masks=masks, excl=excl))   # the same edges and exclusion lists go to every rank
        h.labels_free(hl); h.close()
    merged = SH.merge_score_histograms(per)
    assert np.array_equal(merged, whole)                                    # bit for bit, wherever the gallery was cut
    # the bracket of a global rank: the bin holds the entry that stands there
    rank = np.array([min(int(t), 4000) for t in whole.sum(axis=1) // 3], np.int64)
    b, res = SH.histogram_rank_bin(merged, rank)
    got = one.entries_at(np.arange(n_q, dtype=np.int32), rank, labels=h1, masks=masks, excl=excl)
    ek = key_of(edges)
    for q in range(n_q):
        if got["status"][q] == LISTED:
            assert np.searchsorted(ek, key_of(got["score"][q:q + 1])[0], side="right") == b[q] and 0 <= res[q] < merged[q, b[q]]
        else:
            assert b[q] == -1
    one.labels_free(h1); one.close()
