"""afis_score_pairs: the fused score and the four parts of a LIST of (latent, print) pairs, without a matrix.  The yardstick is afis_search's own scores / parts of the same
context — every comparison exact, bit for bit — and, for a sample, oracle.pair directly.  Tie modes of the oracle as the parity tests map them: default order 1, option
s3_tie_order 1 -> 4, option ref_tie_order 2 -> 0 (std::sort at every site)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
M = importlib.import_module("msu-latentafis_amd.host.matcher")
S = importlib.import_module("msu-latentafis_amd.host.synth")

ZERO = np.zeros(1, np.float32).view(np.uint32)[0]
NINF = np.array([-np.inf], np.float32).view(np.uint32)[0]
SEGMENT = 64                                                               # pair_tables.h::kAdcPairsSegment


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def small(cb):
    return cases.small_set(cb)


def _open(codebook_bytes, gal, index_base=0, **options):
    m = M.Matcher(codebook_bytes)
    for k, v in options.items():
        m.set_option(k, v)
    m.gallery_add(gal)
    m.gallery_commit(index_base)
    return m


def all_pairs(n_lat, n_gal):
    return np.repeat(np.arange(n_lat, dtype=np.int32), n_gal), np.tile(np.arange(n_gal, dtype=np.int64), n_lat)


def same_as_search(res, sr, query, local):
    """Every pair of a score_pairs result against the cells of a search of the same context (scores and parts asked for); local = the prints' shard-local indices."""
    q, g = np.asarray(query, np.int64), np.asarray(local, np.int64)
    assert (res["status"] == M.PAIR_OK).all()
    got, want = bits(res["score"]), bits(sr["scores"][q, g])
    assert np.array_equal(got, want), [(int(q[i]), int(g[i]), res["score"][i], sr["scores"][q[i], g[i]]) for i in np.flatnonzero(got != want)[:6]]
    got, want = bits(res["parts"]), bits(sr["parts"][q, g])
    assert np.array_equal(got, want), [(int(q[i]), int(g[i]), res["parts"][i].tolist(), sr["parts"][q[i], g[i]].tolist()) for i in np.flatnonzero((got != want).any(axis=1))[:6]]


def oracle_parts(oracle, codebook_bytes, L, R, tie_mode):
    ocb = oracle.codebook(codebook_bytes)
    rc, out = oracle.pair(ocb, oracle.latent(ocb, T.write_latent(L))[0], oracle.rolled(T.write_rolled(R))[0], tie_mode)
    assert rc == 0
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def test_all_pairs_shuffled_over_two_launch_groups_and_three_chunks(codebook_bytes, oracle, small):
    lats, gal = small
    assert all(230 <= L.tex[0].n <= 420 for L in lats) and any(L.tex[0].n % 8 for L in lats)       # above the top-200 selection, a last tile that is not full
    m = _open(codebook_bytes, gal, query_batch=2, score_pairs_per_launch=50)
    assert m.get_option("score_pairs_per_launch") == 50 and m.get_option("score_pairs_us") == 0
    qh = m.upload_queries(lats)                                            # launch groups {0, 1} and {2}
    sr = m.search_resident(qh, k=0, want_scores=True, want_parts=True)
    assert m.timing()["launch_groups"] == 2
    rng = np.random.default_rng(12)
    order = rng.permutation(len(lats) * len(gal))
    order = np.concatenate([order, rng.choice(order, 10, replace=False)])  # 130 pairs, ten of them twice: chunks of 50, 50, 30
    query, idx = (order // len(gal)).astype(np.int32), (order % len(gal)).astype(np.int64)
    res = m.score_pairs(qh, query, idx, want_parts=True)
    assert m.get_option("score_pairs_us") > 0
    same_as_search(res, sr, query, idx)
    for i in range(len(order) - 10, len(order)):                            # a repeated pair: identical bytes
        j = int(np.flatnonzero(order[:len(order) - 10] == order[i])[0])
        assert res["score"][i].tobytes() == res["score"][j].tobytes() and res["parts"][i].tobytes() == res["parts"][j].tobytes()
    # not vacuous: texture and minutiae parts that are positive, and the planted mates (prints 3 q) on top of their latent's pairs
    assert (res["parts"][:, 3] > 0).sum() >= 3 and (res["parts"][:, :3] > 0).any(axis=1).sum() >= 3
    for q in range(len(lats)):
        mine = np.flatnonzero(query == q)
        assert idx[mine[np.argmax(res["score"][mine])]] == 3 * q, q
    # a sample against the oracle itself
    for q in range(len(lats)):
        for g in (3 * q, 3 * q + 2, 20 + q):
            i = int(np.flatnonzero((query == q) & (idx == g))[0])
            want = oracle_parts(oracle, codebook_bytes, lats[q], gal[g], 1)
            assert np.array_equal(bits(res["parts"][i]), bits(want[:4])) and bits(res["score"][i]) == bits(want[4]), (q, g, res["parts"][i], res["score"][i], want)
    # without parts: the same scores
    res2 = m.score_pairs(qh, query, idx)
    assert res2["parts"] is None and res2["score"].tobytes() == res["score"].tobytes()
    m.free_queries(qh)
    m.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_every_texture_slot_and_a_latent_empty_query(codebook_bytes, cb, small):
    base, named = cases.edge_latents(cb)
    lats = list(named.values()) + [T.FPTemplate(minu=list(base.minu[:1]), tex=list(base.tex))]        # one minutiae template: texture at slot 1
    assert {len(L.minu) for L in lats} >= {0, 1, 2, 12, 27, 28, 29} and any(not L.tex for L in lats)   # texture at slots 0, 1, 2, beyond 2 (no weight), 28, and none
    mates = cases.rules_gallery(cb, base)[:2]                               # two mates of the latents' common base: the texture scorer finds something
    gal = small[1][:10] + mates + [T.FPTemplate(minu=[], tex=list(mates[0].tex)), T.FPTemplate()]     # ... a print without minutiae, an empty entry
    m = _open(codebook_bytes, gal)
    qh = m.upload_queries(lats)
    sr = m.search_resident(qh, k=0, want_scores=True, want_parts=True)
    assert (sr["status"] == 1).sum() == 1                                   # the latent-empty query
    query, idx = all_pairs(len(lats), len(gal))
    res = m.score_pairs(qh, query, idx, want_parts=True)
    same_as_search(res, sr, query, idx)
    empty_q = int(np.flatnonzero(sr["status"] == 1)[0])
    sc = res["score"].reshape(len(lats), len(gal)); pt = res["parts"].reshape(len(lats), len(gal), 4)
    assert (sc[empty_q] == -1).all() and (bits(pt[empty_q]) == ZERO).all() and (sc[:, -1] == -1).all() and (bits(pt[:, -1]) == ZERO).all()
    assert (pt[:, -2, 3] > 0).sum() >= 3 and (bits(pt[:, -2, :3]) == ZERO).all()   # the print without minutiae still has a texture score
    assert (pt[:, 10, :3] > 0).any(axis=1).sum() >= 3 and (pt[:, 10, 3] > 0).sum() >= 3
    m.free_queries(qh)
    m.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def _rows(L, n):
    t = L.tex[0]
    return T.FPTemplate(minu=list(L.minu), tex=[T.TextureTemplate(t.x[:n].copy(), t.y[:n].copy(), t.ori[:n].copy(), des=t.des[:n].copy())])


def test_tile_tails_block_tails_the_selection_boundary_and_the_clamp(codebook_bytes, cb):
    lats, gal = cases.edge_shapes_set(cb)                                   # texture beyond the 1000-point clamp on both sides, 40 .. 60 and 230 .. 260 rows, 30 .. 1900 points
    rng = np.random.default_rng(77)
    full = S.make_latent(rng, n_tex_lo=1000, n_tex_hi=1001)
    assert full.tex[0].n == 1000
    lats = list(lats) + [_rows(full, n) for n in (8, 199, 200, 201, 1000)]
    gal = list(gal) + [S.make_mate(rng, cb, full, frac=0.8, n_tex=n) for n in (1, 63, 64, 65, 1000)]
    assert [R.tex[0].n for R in gal[-5:]] == [1, 63, 64, 65, 1000]
    m = _open(codebook_bytes, gal)
    qh = m.upload_queries(lats)
    sr = m.search_resident(qh, k=0, want_scores=True, want_parts=True)
    # the hand-made latents against the hand-made prints and one print of the set; the set's latents against their own mates, the tiny and the oversized print, and two hand-made ones
    pairs = [(q, g) for q in range(3, 8) for g in list(range(8, 13)) + [0]] + [(q, g) for q in range(3) for g in (2 * q, 6, 7, 8, 12)]
    query = np.array([p[0] for p in pairs], np.int32); idx = np.array([p[1] for p in pairs], np.int64)
    res = m.score_pairs(qh, query, idx, want_parts=True)
    same_as_search(res, sr, query, idx)
    assert (res["parts"][:, 3] > 0).sum() >= 10
    m.free_queries(qh)
    m.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def _tied(cb):
    lats, R = cases.tied_row_maxima_set(cb)
    return None, lats, [R]


def _signs(cb):
    lats, gal = cases.both_signs_set(cb, n_gal=8)
    return None, lats, gal


def _nan(cb):
    lat, clean, gal = cases.nan_inf_set(cb)
    return None, [lat, clean], gal


def _off_shipped(cb):
    fcb, lats, gal = cases.family_set("duplicates", cb)                     # exact ties between codewords: the first arg-max decides
    return fcb.to_bytes(), lats, gal


@pytest.mark.parametrize("make", [_tied, _signs, _nan, _off_shipped], ids=["tied_row_maxima", "both_signs", "nan_inf", "codebook_with_duplicates"])
def test_hard_row_maxima(codebook_bytes, cb, make):
    buf, lats, gal = make(cb)
    m = _open(buf or codebook_bytes, gal)
    qh = m.upload_queries(lats)
    sr = m.search_resident(qh, k=0, want_scores=True, want_parts=True)
    query, idx = all_pairs(len(lats), len(gal))
    res = m.score_pairs(qh, query, idx, want_parts=True)
    same_as_search(res, sr, query, idx)
    m.free_queries(qh)
    m.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option, value, tie_mode", [("s3_tie_order", 1, 4), ("ref_tie_order", 2, 0), ("adc_variant", 8, 1)])
def test_options(codebook_bytes, oracle, small, option, value, tie_mode):
    lats, gal = small
    gal = gal[:16]
    m = _open(codebook_bytes, gal, **{option: value})
    qh = m.upload_queries(lats)
    sr = m.search_resident(qh, k=0, want_scores=True, want_parts=True)
    query, idx = all_pairs(len(lats), len(gal))
    res = m.score_pairs(qh, query, idx, want_parts=True)
    same_as_search(res, sr, query, idx)
    if option == "ref_tie_order":                                           # the mates, where equal scores tie at S9: the oracle's std::sort order
        for q in range(len(lats)):
            i = int(np.flatnonzero((query == q) & (idx == 3 * q))[0])
            want = oracle_parts(oracle, codebook_bytes, lats[q], gal[3 * q], tie_mode)
            assert np.array_equal(bits(res["parts"][i]), bits(want[:4])) and bits(res["score"][i]) == bits(want[4]), (q, res["parts"][i], want)
    m.free_queries(qh)
    m.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_coverage_gallery_edits_and_a_handle_of_an_older_epoch(codebook_bytes, small):
    lats, gal = small
    BASE = 1000
    m = _open(codebook_bytes, gal[:30], index_base=BASE)
    qh = m.upload_queries(lats, reserve=40)                                 # before the removal and before the appending commit
    old = m.upload_queries(lats)                                            # a plain handle of the first epoch: searches refuse it after the edits, the pair call takes it
    m.gallery_remove([BASE + 3, BASE + 7])
    m.gallery_reopen(); m.gallery_add(gal[30:36]); m.gallery_commit(BASE)
    assert m.resident_size == 36
    sr = m.search(lats, k=0, want_scores=True, want_parts=True)              # a fresh search of the shard as it stands
    local = [0, 3, 4, 7, 29, 30, 33, 35]
    outside = [BASE + 36, BASE - 1, 3, -1, 2 ** 40]                           # one past the shard, one before it, a local index, a pad, far beyond
    glob = [BASE + g for g in local] + outside
    query = np.repeat(np.arange(len(lats), dtype=np.int32), len(glob)); idx = np.tile(np.array(glob, np.int64), len(lats))
    for handle in (qh, old):
        res = m.score_pairs(handle, query, idx, want_parts=True)
        cov = np.tile(np.arange(len(glob)) < len(local), len(lats))
        assert (res["status"][~cov] == M.PAIR_NOT_COVERED).all() and (bits(res["score"][~cov]) == NINF).all() and (bits(res["parts"][~cov]) == ZERO).all()
        same_as_search({k: v[cov] for k, v in res.items()}, sr, query[cov], idx[cov] - BASE)
        sc = res["score"].reshape(len(lats), len(glob))
        assert (sc[:, [1, 3]] == -1).all() and (sc[:, [5, 6, 7]] != -1).all()   # the removed prints; the appended ones are scored
    # a list of nothing but uncovered pairs queues nothing
    res = m.score_pairs(qh, [0, 1], [-1, BASE + 36], want_parts=True)
    assert (res["status"] == M.PAIR_NOT_COVERED).all() and m.get_option("score_pairs_us") == 0
    m.free_queries(qh); m.free_queries(old)
    m.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_the_last_search_matrix_survives(codebook_bytes, small):
    lats, gal = small
    gal = gal[:20]
    m = _open(codebook_bytes, gal)
    qh = m.upload_queries(lats)
    full = m.search_resident(qh, k=0, want_scores=True, want_parts=True)
    ninf = float("-inf")
    h1 = m.rank_hits(ninf, 24)                                              # cap 24 > G = 20: four -1 pads per list
    idx = h1["idx"].reshape(-1); query = np.repeat(np.arange(len(lats), dtype=np.int32), 24)
    res = m.score_pairs(qh, query, idx, want_parts=True)
    assert (res["status"][idx == -1] == M.PAIR_NOT_COVERED).all() and np.array_equal(bits(res["score"][idx >= 0]), bits(h1["score"].reshape(-1)[idx >= 0]))
    h2 = m.rank_hits(ninf, 24)                                              # AFIS_OK, and the same lists
    for k in ("n_hits", "idx", "score"):
        assert h1[k].tobytes() == h2[k].tobytes(), k
    # after a subset search the matrix is the subset's — and idx stays resident-global
    listed = [17, 2, 9, 4]
    sub = m.subset_create(listed)
    m.search_subset_resident(sub, qh, k=0)
    s1 = m.rank_hits(ninf, 6)
    query, gidx = all_pairs(len(lats), len(gal))
    res = m.score_pairs(qh, query, gidx, want_parts=True)
    same_as_search(res, full, query, gidx)
    s2 = m.rank_hits(ninf, 6)
    for k in ("n_hits", "idx", "score"):
        assert s1[k].tobytes() == s2[k].tobytes(), k
    assert set(s2["idx"][0][:4].tolist()) == set(listed)
    m.subset_free(sub)
    # ... and after an eligible search
    labels = m.labels_create([1 if g % 2 else 2 for g in range(len(gal))])
    masks = np.tile(np.array([1, 0, 0], np.uint64), (len(lats), 1))         # odd prints only
    m.search_eligible(lats, labels, masks)
    e1 = m.rank_hits(ninf, 12)
    res = m.score_pairs(qh, query, gidx, want_parts=True)
    same_as_search(res, full, query, gidx)
    e2 = m.rank_hits(ninf, 12)
    for k in ("n_hits", "idx", "score"):
        assert e1[k].tobytes() == e2[k].tobytes(), k
    assert (e2["n_hits"] == 10).all()
    m.labels_free(labels)
    m.free_queries(qh)
    m.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_cases(codebook_bytes, cb, small):
    lats, gal = small
    _, named = cases.edge_latents(cb)
    lats = [lats[0], named["minu26_notex"]]                                 # the second is latent-empty
    m = M.Matcher(codebook_bytes)
    m.gallery_add(gal[:6])
    z32 = np.zeros(1, np.int32); z64 = np.zeros(1, np.int64); st = np.full(1, 77, np.int32); sc = np.full(1, 77, np.float32); pt = np.full(4, 77, np.float32)
    args = (M._ptr(z32, C.c_int32), M._ptr(z64, C.c_int64), M._ptr(st, C.c_int32), M._ptr(sc, C.c_float), M._ptr(pt, C.c_float))
    other = M.Matcher(codebook_bytes)                                      # no handle can be made on a context before its first commit: a real one of a second context
    other.gallery_add(gal[:2]); other.gallery_commit(0)
    oh = other.upload_queries(lats[:1])
    f = m.lib.afis_score_pairs
    assert f(m.ctx, oh[0], 1, *args) == -3                                  # AFIS_ESTATE before the first commit
    other.free_queries(oh); other.close()
    m.gallery_commit(0)
    qh = m.upload_queries(lats)
    assert f(None, qh[0], 1, *args) == -1 and f(m.ctx, None, 1, *args) == -1 and f(m.ctx, qh[0], -1, *args) == -1
    for hole in range(4):                                                   # query, idx, status, score: each required
        assert f(m.ctx, qh[0], 1, *[None if i == hole else a for i, a in enumerate(args)]) == -1, hole
    for bad in (-1, 2):
        with pytest.raises(M.AfisError, match="afis error -1"):
            m.score_pairs(qh, [0, bad], [0, 0])
    assert st[0] == 77 and sc[0] == 77 and (pt == 77).all()                 # no refused call wrote anything
    for name, bad in (("score_pairs_per_launch", 0), ("score_pairs_per_launch", (1 << 20) + 1), ("score_pairs_us", 1)):
        with pytest.raises(M.AfisError):
            m.set_option(name, bad)
    assert m.get_option("score_pairs_per_launch") == 8192
    assert f(m.ctx, qh[0], 0, None, None, None, None, None) == 0
    res = m.score_pairs(qh, [], [], want_parts=True)
    assert res["status"].shape == (0,) and res["score"].shape == (0,) and res["parts"].shape == (0, 4)
    assert f(m.ctx, qh[0], 1, *args[:4], None) == 0 and st[0] == M.PAIR_OK and sc[0] > 0 and (pt == 77).all()   # parts = NULL; the context is usable after the refused calls
    res = m.score_pairs(qh, [1] * 6 + [0], list(range(6)) + [0], want_parts=True)
    assert (res["status"] == M.PAIR_OK).all() and (res["score"][:6] == -1).all() and (bits(res["parts"][:6]) == ZERO).all() and bits(res["score"][6]) == bits(sc[0])
    m.free_queries(qh)
    m.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_one_latent_against_every_print_five_times_over(codebook_bytes, small):
    lats, gal = small
    m = _open(codebook_bytes, gal)
    qh = m.upload_queries(lats)
    sr = m.search_resident(qh, k=0, want_scores=True, want_parts=True)
    idx = np.tile(np.arange(len(gal), dtype=np.int64), 5)                   # 200 pairs of latent 1: segments of 64, 64, 64 and 8
    assert len(idx) > 3 * SEGMENT and len(idx) % SEGMENT
    query = np.ones(len(idx), np.int32)
    res = m.score_pairs(qh, query, idx, want_parts=True)
    same_as_search(res, sr, query, idx)
    # ... and exactly two full segments beside a few pairs of the other latents
    idx = np.concatenate([np.arange(len(gal), dtype=np.int64)[::-1], np.tile(np.arange(len(gal), dtype=np.int64), 4)[:2 * SEGMENT], [5, 6]])
    query = np.concatenate([np.zeros(len(gal), np.int32), np.full(2 * SEGMENT, 2, np.int32), [1, 1]]).astype(np.int32)
    res = m.score_pairs(qh, query, idx, want_parts=True)
    same_as_search(res, sr, query, idx)
    m.free_queries(qh)
    m.close()
