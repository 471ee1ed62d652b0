"""Reverse search on the GPU: query handles that survive gallery edits (afis_queries_upload_reserved), the column hit lists (afis_rank_latent_hits) and the parity tap
afis_debug_rank_latent_hits.

The yardstick is numpy, compared bit for bit.  A column list is, per template the last search covered, the search's queries in rank-list order — key = the ordered bits
of (score + 0.0f), descending, equal keys by ascending query position; min_score gets the same + 0.0f — cut to the entries whose key reaches min_score's, and to cap;
n_hits, every entry (latent_base + position, the score's raw word) and every padding entry (-1, -inf) must be equal.

The device transposes the matrix in 64 x 64 tiles and ranks a transposed row with one 1024-thread workgroup over strips of 4096 entries, sorting at most 4096
composites: the tap's shapes sit on, one before and one after the tile / wave (64), the workgroup (1024) and the strip / AFIS_HITS_MAX (4096) edges in the query
dimension, on the tile edge and past two tiles (130) in the template dimension; 9001 spans three strips, 70001 would wrap a 16-bit counter."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")

SEED = 4211
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NEG_INF = np.float32(-np.inf).view(np.uint32)
F32 = np.float32
HAIR = F32(np.nextafter(F32(0), F32(1)))                                    # the smallest positive float
CAPS = (1, 64, 100, 4096)
BASES = (0, 5_000_000_000)
PAIRS = ((1, 1), (1, 4097), (2, 63), (2, 70001), (63, 64), (63, 1025), (64, 64), (64, 4096), (65, 65), (65, 1023), (65, 9001), (130, 1), (130, 1024), (130, 4095))   # (templates, queries)
SPECIAL = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x3fc00000, 0xbf800000, 0x40500000], np.uint32).view(np.float32)   # +-inf, +-0, +-NaN, 1.5, -1, 3.25
KINDS = 9


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """130 rolled templates of one minutia and one texture point each (tests/test_gpu_rank_hits.py's tap gallery), as one packed gallery."""
    G = max(n for n, _ in PAIRS)
    rng = np.random.default_rng(SEED)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    return S.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
                           off.copy(), rng.integers(0, 30, G).astype(np.int16), rng.integers(0, 30, G).astype(np.int16), rng.uniform(-1.5, 1.5, G).astype(np.float32),
                           rng.integers(0, cb.K, (G, cb.M)).astype(np.uint8))


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def template_key(x):
    """k_topk's key word (minu.hip): the ordered bits of score + 0.0f."""
    return ordered((np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32))


class ColumnModel:
    """scores [n_q][n]: per column the query positions in rank-list order and their keys, so that a (min_score, cap, latent_base) triple costs one search in a sorted array."""

    def __init__(self, scores):
        self.cols = np.ascontiguousarray(np.asarray(scores, np.float32).T)
        self.words = self.cols.view(np.uint32)
        self.order, self.neg_key = [], []
        for j in range(self.cols.shape[0]):
            key = template_key(self.cols[j]).astype(np.int64)
            o = np.lexsort((np.arange(len(key)), -key))                     # key descending, query position ascending
            self.order.append(o); self.neg_key.append(-key[o])

    def hits(self, min_score, cap, latent_base=0):
        thr = int(template_key(np.array([min_score], np.float32))[0])
        n_t = len(self.order)
        n = np.empty(n_t, np.int64); idx = np.full((n_t, cap), -1, np.int64); sc = np.full((n_t, cap), NEG_INF, np.uint32)
        for j in range(n_t):
            n[j] = np.searchsorted(self.neg_key[j], -thr, side="right")     # keys >= thr: a prefix of the rank list
            take = self.order[j][:min(int(n[j]), cap)]
            idx[j, :len(take)] = latent_base + take; sc[j, :len(take)] = self.words[j, take]
        return {"n_hits": n, "latent": idx, "score": sc}


def as_words(r):
    return {k: (v.view(np.uint32) if k == "score" and v.dtype != np.uint32 else v) for k, v in r.items() if v is not None}


def assert_same(got, want, what=""):
    got = as_words(got); want = as_words(want)
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].tolist(), got[key].ravel()[:8].tolist(), want[key].ravel()[:8].tolist())


# ---- the tap's matrices ---------------------------------------------------------------------------------------------------------------------------------
def column(kind, n_q, rng):
    """The row kinds of tests/test_gpu_rank_hits.py::matrix, one at a time: 0 all-distinct values (integers around zero), 1 nine distinct values, 2 all +0.0,
    3 search-like (-1, 0 and a few positives), 4-7 words that differ in exactly one byte — byte 0, 1, 2, 3 of the float — and 8 infinities, both zeros and quiet NaNs of
    both signs among plain values."""
    if kind == 0:
        return rng.permutation(n_q).astype(np.float32) - np.float32(n_q // 3)
    if kind == 1:
        return np.round(rng.random(n_q) * 8).astype(np.float32)
    if kind == 2:
        return np.zeros(n_q, np.float32)
    if kind == 3:
        u = rng.random(n_q)
        return np.where(u < 0.05, -1.0, np.where(u < 0.07, rng.random(n_q) * 5 + 0.01, 0.0)).astype(np.float32)
    if kind < 8:
        b = kind - 4
        byte = rng.integers(0, 256, n_q).astype(np.uint32) if b < 3 else rng.choice(np.r_[1:0x80, 0x81:0xff], n_q).astype(np.uint32)   # (no zero exponent: no subnormal, no zero)
        return ((np.uint32(0x40404040) & ~np.uint32(0xff << (8 * b))) | (byte << np.uint32(8 * b))).view(np.float32)
    return SPECIAL[rng.integers(0, len(SPECIAL), n_q)]


def matrix(n_q, n, first_kind, rng):
    """[n_q][n]: column j is of kind (first_kind + j) % 9."""
    m = np.empty((n_q, n), np.float32)
    for j in range(n):
        m[:, j] = column((first_kind + j) % KINDS, n_q, rng)
    return m


@pytest.mark.parametrize("n,n_q", PAIRS)
def test_tap_sweep(n, n_q, codebook_bytes, tiny):
    """Every column kind x every cap x every threshold x both latent bases.  Fewer than nine templates: one matrix per first kind, so that every kind is met at every shape.
    The tap uploads a matrix once; it stays rankable, and the product entry point answers the other combinations."""
    m = M.Matcher(codebook_bytes, taps=True)
    m.gallery_add_packed(tiny.slice(0, n)); m.gallery_commit(BASE)
    rng = np.random.default_rng(SEED + 131 * n + n_q)
    seen = set()
    for first_kind in range(0, KINDS if n < KINDS else 1, max(n, 1)):
        sc = matrix(n_q, n, first_kind, rng)
        seen |= {(first_kind + j) % KINDS for j in range(n)}
        model = ColumnModel(sc)
        finite = np.unique(sc[np.isfinite(sc)])
        present = finite[len(finite) // 2] if len(finite) else F32(1.5)        # a value from the matrix (a 1 x 1 matrix may hold an infinity or a NaN alone)
        thrs = [F32(-np.inf), F32(-1.0), F32(0.0), HAIR, present, F32(np.inf)]
        assert_same(m.debug_rank_latent_hits(sc, float(thrs[0]), CAPS[0], BASES[1]), model.hits(thrs[0], CAPS[0], BASES[1]), (n, n_q, first_kind, "tap"))
        assert m.get_option("rank_latents_us") > 0 and m.transpose_stats()[1] == n * n_q * 8
        for t in thrs:
            for cap in CAPS:
                for base in BASES:
                    assert_same(m.rank_latent_hits(float(t), cap, base), model.hits(t, cap, base), (n, n_q, first_kind, float(t), cap, base))
        full = m.rank_latent_hits(float("-inf"), 4096)
        neg_nan = (sc.view(np.uint32) == 0xffc00000).sum(axis=0)
        assert np.array_equal(full["n_hits"], n_q - neg_nan)                # everything reaches -inf but a NaN with the sign set
        top = m.rank_latents(100)
        assert np.array_equal(top["latent"], full["latent"][:, :100]) and np.array_equal(top["score"].view(np.uint32), full["score"][:, :100].view(np.uint32))
    assert seen == set(range(KINDS))
    m.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------
N_POOL, N_LAT, N_NEW = 60, 40, 5
MATED = (7, 31)                                                             # the latents whose mates are enrolled later


@pytest.fixture(scope="module")
def world(cb):
    """40 latents, a pool of 60 rolled templates, and a card of five new ones of which two are mates of latents 7 and 31."""
    lats = S.make_latents(91, N_LAT, n_tex_lo=400, n_tex_hi=600)
    pool = [S.make_rolled(np.random.default_rng([91, 5, i]), cb) for i in range(N_POOL)]
    new = [S.make_rolled(np.random.default_rng([91, 6, i]), cb) for i in range(N_NEW)]
    new[1] = S.make_mate(np.random.default_rng([91, 7, 1]), cb, lats[MATED[0]])
    new[3] = S.make_mate(np.random.default_rng([91, 7, 3]), cb, lats[MATED[1]])
    return lats, pool, new


@pytest.fixture(scope="module")
def fresh_scores(codebook_bytes, world):
    """The scores of a context freshly committed with all 65 templates: [40][65]."""
    lats, pool, new = world
    f = M.Matcher(codebook_bytes)
    f.gallery_add(pool + new); f.gallery_commit(BASE)
    sc = f.search(lats, k=0, want_scores=True)["scores"].copy()
    f.close()
    sc.setflags(write=False)
    return sc


def test_end_to_end(codebook_bytes, world, fresh_scores):
    lats, pool, new = world
    m = M.Matcher(codebook_bytes)
    m.gallery_add(pool); m.gallery_commit(BASE)
    m.set_option("query_batch", 16)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.upload_queries(lats, reserve=0)
    qr = m.upload_queries(lats, reserve=8)                                  # while the shard holds 60: the cuts are for 8
    qp = m.upload_queries(lats)
    m.gallery_reopen(); m.gallery_add(new); m.gallery_commit(BASE)
    assert m.resident_size == N_POOL + N_NEW
    order = [3, 0, 4, 1, 2]                                                 # the card's prints in shuffled order
    listed = [BASE + N_POOL + j for j in order]
    hs = m.subset_create(listed)
    with pytest.raises(M.AfisError, match=ESTATE):                          # the plain handle: uploaded before the edit
        m.search_subset_resident(hs, qp, k=0)
    r = m.search_subset_resident(hs, qr, k=0, want_scores=True)
    assert m.timing()["launch_groups"] == 3
    want = fresh_scores[:, [N_POOL + j for j in order]]
    assert np.array_equal(r["scores"].view(np.uint32), want.view(np.uint32))
    model = ColumnModel(want)
    for t in (HAIR, F32(-np.inf)):
        for cap in (8, 100):
            assert_same(m.rank_latent_hits(float(t), cap), model.hits(t, cap), ("subset", float(t), cap))
    top = m.rank_latents(3, latent_base=500)
    assert top["latent"][order.index(1), 0] == 500 + MATED[0] and top["latent"][order.index(3), 0] == 500 + MATED[1]   # each mate's column lists its latent first
    assert (m.rank_hits(float("-inf"), 5)["n_hits"] == N_NEW).all()          # the row lists still work on the same matrix
    assert_same(m.rank_latent_hits(float(HAIR), 8), model.hits(HAIR, 8), "after afis_rank_hits")
    # a removal: another edit, a new subset, the same reserved handle
    m.gallery_remove([BASE + 2])
    with pytest.raises(M.AfisError, match=ESTATE):                          # the old subset belongs to the gallery as it was
        m.search_subset_resident(hs, qr, k=0)
    m.subset_free(hs)
    hs = m.subset_create(listed)
    r = m.search_subset_resident(hs, qr, k=0, want_scores=True)
    assert np.array_equal(r["scores"].view(np.uint32), want.view(np.uint32))
    assert_same(m.rank_latent_hits(float(HAIR), 100), model.hits(HAIR, 100), "after the removal")
    m.subset_free(hs)
    h9 = m.subset_create([BASE + g for g in range(10, 19)])
    with pytest.raises(M.AfisError, match=EINVAL + ".*9 templates.*at most 8"):
        m.search_subset_resident(h9, qr, k=0)
    m.subset_free(h9)
    with pytest.raises(M.AfisError, match=EINVAL + ".*65 templates.*at most 8"):
        m.search_resident(qr, k=0)
    m.free_queries(qr); m.free_queries(qp)
    m.close()


def test_reserved_handle_on_a_full_search(codebook_bytes, world):
    """A context of 8 templates: the reserved handle serves afis_search_resident, through a removal too; one more template and it is refused."""
    lats, pool, _ = world
    m = M.Matcher(codebook_bytes)
    m.gallery_add(pool[:8]); m.gallery_commit(BASE)
    want = m.search(lats[:6], k=0, want_scores=True)["scores"]
    qr = m.upload_queries(lats[:6], reserve=8)
    got = m.search_resident(qr, k=0, want_scores=True)["scores"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert_same(m.rank_latent_hits(float("-inf"), 6), ColumnModel(want).hits(F32(-np.inf), 6), "a full search: row j is template index_base + j")
    m.gallery_remove([BASE + 5])
    got = m.search_resident(qr, k=0, want_scores=True)["scores"]
    assert (got[:, 5] == -1).all() and np.array_equal(np.delete(got, 5, axis=1).view(np.uint32), np.delete(want, 5, axis=1).view(np.uint32))
    m.gallery_reopen(); m.gallery_add(pool[8:9]); m.gallery_commit(BASE)
    with pytest.raises(M.AfisError, match=EINVAL + ".*9 templates.*at most 8"):
        m.search_resident(qr, k=0)
    m.free_queries(qr)
    m.close()


def test_matcher_reverse_search(codebook_bytes, world, fresh_scores):
    lats, pool, new = world
    m = M.Matcher(codebook_bytes)
    m.gallery_add(pool); m.gallery_commit(BASE)
    qr = m.upload_queries(lats, reserve=8)
    idx, lists = m.reverse_search(qr, new, float(HAIR), 100, latent_base=40)
    assert idx.tolist() == [BASE + N_POOL + j for j in range(N_NEW)] and m.resident_size == N_POOL + N_NEW
    assert_same(lists, ColumnModel(fresh_scores[:, N_POOL:]).hits(HAIR, 100, 40), "reverse_search")
    assert lists["latent"][1, 0] == 40 + MATED[0] and lists["latent"][3, 0] == 40 + MATED[1]
    with pytest.raises(M.AfisError, match=ESTATE):                          # the subset is freed: its matrix went with it
        m.rank_latent_hits(0.0, 8, n_templates=N_NEW)
    m.free_queries(qr)
    m.close()


def test_two_handles(codebook_bytes, world, fresh_scores):
    """A latent file kept as two handles of 20: searched one after the other, the column lists merge with merge_hits into the one-handle lists."""
    lats, pool, new = world
    m = M.Matcher(codebook_bytes)
    m.gallery_add(pool + new); m.gallery_commit(BASE)
    hs = m.subset_create([BASE + N_POOL + j for j in range(N_NEW)])
    qa, qb, qall = m.upload_queries(lats[:20], reserve=8), m.upload_queries(lats[20:], reserve=8), m.upload_queries(lats, reserve=8)
    for t, cap in ((float(HAIR), 100), (float("-inf"), 7)):
        parts = []
        for q, base in ((qa, 0), (qb, 20)):
            m.search_subset_resident(hs, q, k=0)
            parts.append(m.rank_latent_hits(t, cap, latent_base=base))
        m.search_subset_resident(hs, qall, k=0)
        one = m.rank_latent_hits(t, cap)
        n, li, sc = SH.merge_hits(np.stack([p["n_hits"] for p in parts]), np.stack([p["latent"] for p in parts]), np.stack([p["score"] for p in parts]), cap)
        assert_same({"n_hits": n, "latent": li, "score": sc}, one, ("two handles", t, cap))
        assert_same(one, ColumnModel(fresh_scores[:, N_POOL:]).hits(F32(t), cap), ("one handle", t, cap))
    for q in (qa, qb, qall):
        m.free_queries(q)
    m.subset_free(hs)
    m.close()


# ---- contracts ------------------------------------------------------------------------------------------------------------------------------------------
def test_contracts(codebook_bytes, world):
    lats, pool, _ = world
    lats = lats[:3]
    i64p, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    m = M.Matcher(codebook_bytes)
    with pytest.raises(M.AfisError, match=ESTATE):                          # before the first commit
        m.upload_queries(lats, reserve=8)
    m.gallery_add(pool[:12]); m.gallery_commit(BASE)
    G = 12
    nh = np.zeros(G, np.int64); a = np.zeros((G, 24), np.int64); sc = np.zeros((G, 24), np.float32)
    pn, pa, ps = nh.ctypes.data_as(i64p), a.ctypes.data_as(i64p), sc.ctypes.data_as(fp)
    rl = m.lib.afis_rank_latent_hits
    assert rl(m.ctx, G, 0.0, 24, 0, pn, pa, ps) == -3                       # before any search
    scores = m.search(lats, k=0, want_scores=True)["scores"]
    model = ColumnModel(scores)
    assert rl(m.ctx, G - 1, 0.0, 24, 0, pn, pa, ps) == -1 and rl(m.ctx, G + 1, 0.0, 24, 0, pn, pa, ps) == -1 and rl(m.ctx, 3, 0.0, 24, 0, pn, pa, ps) == -1   # not the columns the search covered
    for cap in (0, -1, 4097):
        assert rl(m.ctx, G, 0.0, cap, 0, pn, pa, ps) == -1
    assert rl(m.ctx, G, float("nan"), 24, 0, pn, pa, ps) == -1
    assert rl(m.ctx, G, 0.0, 24, -1, pn, pa, ps) == -1
    assert rl(m.ctx, G, 0.0, 24, 0, None, pa, ps) == -1 and rl(m.ctx, G, 0.0, 24, 0, pn, None, ps) == -1 and rl(m.ctx, G, 0.0, 24, 0, pn, pa, None) == -1
    # the refused calls left the matrix rankable; a repeated call gives the same answer, and the row lists still work
    assert rl(m.ctx, G, 0.0, 24, 0, pn, pa, ps) == 0
    assert_same({"n_hits": nh, "latent": a, "score": sc}, model.hits(F32(0), 24), "through the C ABI")
    assert m.get_option("rank_latents_us") > 0
    first = m.rank_latent_hits(0.0, 24)
    assert_same(m.rank_latent_hits(0.0, 24), first, "a repeated call")
    assert (m.rank_hits(float("-inf"), 24)["n_hits"] == G).all()
    assert_same(m.rank_latent_hits(0.0, 24), first, "after afis_rank_hits")
    # calls that queue device work take the matrix away
    qh = m.upload_queries(lats)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_latent_hits(0.0, 24)
    m.search_resident(qh, k=0)
    assert (m.rank_latent_hits(float("-inf"), 3)["n_hits"] == 3).all()
    m.gallery_remove([BASE + 4])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_latent_hits(0.0, 24)
    # an empty subset: a search of no columns
    he = m.subset_create([])
    qr = m.upload_queries(lats, reserve=8)
    m.search_subset_resident(he, qr, k=0)
    e = m.rank_latent_hits(0.0, 24)
    assert e["n_hits"].shape == (0,) and e["latent"].shape == (0, 24)
    assert rl(m.ctx, 1, 0.0, 24, 0, pn, pa, ps) == -1
    # a search of no queries: zero counts and padding
    q0 = m.upload_queries([], reserve=16)
    m.search_resident(q0, k=0)
    z = m.rank_latent_hits(float("-inf"), 5)
    assert (z["n_hits"] == 0).all() and z["n_hits"].shape == (G,) and (z["latent"] == -1).all() and np.isneginf(z["score"]).all()
    m.free_queries(q0)
    m.subset_free(he); m.free_queries(qr); m.free_queries(qh)
    m.close()
