"""Kept matrices on the GPU: afis_matrix_keep, afis_matrix_free, afis_matrix_info, afis_matrix_read, afis_matrix_recall, afis_matrix_fuse.

The yardstick is tests/matrix_model.py — numpy, never the code under test: the cell rule spelled out per cell, SUM a float64 loop in operand order.  Everything is
compared exactly, words as integers; there is no tolerance anywhere.

Matrices are planted with the taps afis_debug_rank_hits (the whole shard) and afis_debug_rank_rows (a subset), which leave their matrix rankable, on a packed
gallery of one-point templates (the recipe of tests/test_gpu_link_groups.py); index_base is 1000.  A normalised operand is a planted matrix that went through
afis_normalize_scores (the only way to the mark); the model then folds what afis_matrix_read returns of it.  The fuse kernel gives a thread one column, or four
where the row length is a multiple of four, 256 threads a workgroup: the row lengths sit before, on and after 4, 256 and 1024; the transposition works on 64 x 64
tiles: the square sizes sit around 64 and 128."""
import ctypes
import importlib

import numpy as np
import pytest

import link_model as LM
import matrix_model as MM

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 9433
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NINF = float("-inf")
COLUMNS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2052)
N_Q = (1, 7, 8, 9)
N_OPS = (1, 2, 16)
SQUARE = (1, 63, 64, 65, 129)
G_MAX = 4097
MODES = (MM.SUM, MM.MAX, MM.MIN)


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_words(got, want, what):
    g, w = u32(got), u32(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist(), [hex(int(t)) for t in g[g != w][:6]], [hex(int(t)) for t in w[g != w][:6]])


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """4097 rolled templates of one minutia and one texture point each, made as one packed gallery."""
    G = G_MAX
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


def lists(r):
    return {k: (u32(v) if v.dtype == np.float32 else v) for k, v in r.items()}


def same_lists(a, b, what):
    a, b = lists(a), lists(b)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def weights_for(rng, n, i):
    """None, and weights with zeros, negatives and factors whose products are inexact in fp64."""
    if i % 3 == 0:
        return None
    w = rng.choice(np.array([0.1, 1.0 / 3.0, -0.7, 0.5, 1.0, 2.5, 1e-3, 7.0 / 9.0, -1.0]), n)
    if i % 3 == 2:
        w[rng.integers(0, n)] = 0.0
    return w


# ---- 1: fuse against the model: row lengths, rows, operand counts, every mode and flag, raw and normalised --------------------------------------------------
@pytest.mark.parametrize("G", COLUMNS)
def test_fuse_against_the_model(G, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    case = 0
    for n_q in N_Q:
        raw, nrm, raw_rows, nrm_rows = [], [], [], []
        for k in range(max(N_OPS)):
            rows = MM.cells(rng, (n_q, G))
            plant(m, rows)
            raw.append(m.matrix_keep()); raw_rows.append(rows)
            z = m.normalize_scores(np.full(n_q, 5.0 + k), np.full(n_q, 0.25), axis=0, want_scores=True)   # z = (v - 5 - k) / 4: negative z-scores, and every outside cell no entry
            nrm.append(m.matrix_keep()); nrm_rows.append(z)
        assert m.get_option("matrix_device_bytes") == 2 * max(N_OPS) * n_q * G * 4
        for k in (0, max(N_OPS) - 1):                                       # what a handle holds is what was planted, and what the normalisation returned
            same_words(m.matrix_read(raw[k]), raw_rows[k], (G, n_q, "read raw", k))
            same_words(m.matrix_read(nrm[k]), nrm_rows[k], (G, n_q, "read normalised", k))
            assert m.matrix_info(raw[k]) == {"n_q": n_q, "normalized": False, "columns": G, "over_subset": False, "stale": False}
            assert m.matrix_info(nrm[k])["normalized"] is True
        if n_q * G >= 10:                                                   # (MM.cells: a tenth each from ten cells on)
            assert (u32(nrm_rows[0]) == 0xffffffff).mean() >= 0.1 and (u32(raw_rows[0]) == 0xbf800000).mean() >= 0.1 and (u32(raw_rows[0]) == 0xffffffff).mean() >= 0.1
        for n in N_OPS:
            for normalized, hs, rs in ((False, raw, raw_rows), (True, nrm, nrm_rows)):
                for op in MODES:
                    for flag in (0, MM.REQUIRE_ALL):
                        case += 1
                        pick = np.arange(n) if n == max(N_OPS) else rng.integers(0, max(N_OPS), n)   # (a handle may come twice)
                        w = weights_for(rng, n, case) if op == MM.SUM else None
                        want = MM.fuse([rs[i] for i in pick], op | flag, normalized, w)
                        got = m.matrix_fuse([hs[i] for i in pick], op | flag, weights=w, want_scores=True)
                        what = (G, n_q, n, normalized, op, flag)
                        same_words(got, want, what)
                        assert m.get_option("matrix_fuse_us") > 0, what
                        if case % 4 == 0:                                   # the result is the last search's matrix: kept and read back, it is the same words
                            h = m.matrix_keep()
                            assert m.matrix_info(h) == {"n_q": n_q, "normalized": normalized, "columns": G, "over_subset": False, "stale": False}
                            same_words(m.matrix_read(h), want, (what, "keep + read"))
                            if n_q > 2:
                                same_words(m.matrix_read(h, 1, n_q - 2), want[1:n_q - 1], (what, "rows 1 .. n_q - 2"))
                            m.matrix_free(h)
        for h in raw + nrm:
            m.matrix_free(h)
        assert m.get_option("matrix_device_bytes") == 0
    m.close()


# ---- 2: transposed operands ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SQUARE)
def test_transposed_operands(n, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, n)
    rng = np.random.default_rng(SEED + 100 + n)
    a = MM.cells(rng, (n, n))
    b = MM.cells(rng, (n, n))
    plant(m, a); ha = m.matrix_keep()
    plant(m, b); hb = m.matrix_keep()
    for op in (MM.MIN, MM.MAX, MM.SUM):
        for flag in (0, MM.REQUIRE_ALL):
            got = m.matrix_fuse([ha, ha], op | flag, transposed=[0, 1], want_scores=True)
            same_words(got, MM.fuse([a, np.ascontiguousarray(a.T)], op | flag, False), (n, op, flag, "(A, A^T)"))
            assert op == MM.SUM or np.array_equal(MM.key_of(got), MM.key_of(got).T)   # MIN and MAX of a matrix with its transpose are symmetric in the key (of two zeros the first operand's stays; a sum's additions come in the other order)
    w = np.array([0.5, -0.25, 1.0 / 3.0])
    got = m.matrix_fuse([hb, ha, hb], MM.SUM, weights=w, transposed=[1, 0, 1], want_scores=True)   # one handle transposed twice: one transposition
    same_words(got, MM.fuse([np.ascontiguousarray(b.T), a, np.ascontiguousarray(b.T)], MM.SUM, False, w), (n, "(B^T, A, B^T)"))
    got = m.matrix_fuse([ha, hb], MM.MAX, transposed=[1, 1], want_scores=True)
    same_words(got, MM.fuse([np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)], MM.MAX, False), (n, "(A^T, B^T)"))
    same_words(m.matrix_read(ha), a, "the operands are unchanged")
    m.matrix_free(ha); m.matrix_free(hb)
    m.close()


def test_a_transposed_operand_needs_a_square_matrix(codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, 5)
    rng = np.random.default_rng(SEED + 200)
    rows = MM.cells(rng, (3, 5))
    plant(m, rows)
    h = m.matrix_keep()
    before = m.rank_hits(NINF, 5)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.matrix_fuse([h, h], MM.MIN, transposed=[0, 1])
    assert m.get_option("matrix_fuse_us") == 0
    same_lists(m.rank_hits(NINF, 5), before, "the matrix still ranks")
    same_words(m.matrix_fuse([h, h], MM.MIN, transposed=[0, 0], want_scores=True), MM.fuse([rows, rows], MM.MIN, False), "untransposed")
    m.close()


# ---- 3: keep and recall ----------------------------------------------------------------------------------------------------------------------------------------------
def test_keep_and_recall(codebook_bytes, tiny):
    G, n_q = 1025, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 300)
    x = MM.cells(rng, (n_q, G))
    edges = np.array([-1.0, 0.0, 0.5, 5.0, 20.0, 39.0, 65536.0], np.float32)
    plant(m, x)

    def answers():
        return m.rank_hits(NINF, 4096), m.score_stats(0), m.score_stats(1), m.score_histogram(edges), m.score_histogram(edges, axis=1)

    first = answers()
    h = m.matrix_keep()
    assert m.get_option("matrix_keep_us") > 0 and m.get_option("matrix_device_bytes") == n_q * G * 4
    same_lists(m.rank_hits(NINF, 4096), first[0], "keep leaves the matrix rankable")
    plant(m, MM.cells(rng, (n_q + 2, G)))                                   # another matrix, of another shape
    assert not np.array_equal(m.rank_hits(NINF, 16)["idx"][:n_q], first[0]["idx"][:, :16])
    m.matrix_recall(h)
    again = answers()
    same_lists(again[0], first[0], "rank_hits after the recall")
    for i in (1, 2, 3, 4):
        assert np.array_equal(again[i], first[i]), ("after the recall", i)
    # keep -> normalise -> recall: the statistics work again
    mean, sd = m.score_moments(first[1])
    z = m.normalize_scores(mean, 1.0 / sd, axis=0, want_scores=True)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.score_stats(0)
    m.matrix_recall(h)
    assert np.array_equal(m.score_stats(0), first[1]) and m.matrix_info(h)["normalized"] is False
    # S-norm
    m.normalize_scores(mean, 1.0 / sd, axis=0)
    ha = m.matrix_keep()
    m.matrix_recall(h)
    mean_t, sd_t = m.score_moments(first[2])
    sd_t = np.where(sd_t > 0, sd_t, 1.0)
    zt = m.normalize_scores(mean_t, 1.0 / sd_t, axis=1, want_scores=True)
    hb = m.matrix_keep()
    same_words(m.matrix_read(ha), z, "the row-normalised half"); same_words(m.matrix_read(hb), zt, "the column-normalised half")
    got = m.matrix_fuse([ha, hb], MM.SUM, weights=[0.5, 0.5], want_scores=True)
    want = MM.fuse([z, zt], MM.SUM, True, [0.5, 0.5])
    same_words(got, want, "S-norm")
    hs = m.matrix_keep()
    assert m.matrix_info(hs)["normalized"] is True
    with pytest.raises(M.AfisError, match=ESTATE):                          # a fused normalised matrix is a normalised matrix
        m.score_stats(0)
    for thr in (-0.5, 0.0, 1.5):                                            # min_score in the units of the result
        hits = m.rank_hits(thr, 8)
        assert hits["n_hits"].tolist() == (MM.key_of(want).astype(np.int64) >= int(MM.key_of(np.float32(thr)))).sum(axis=1).tolist(), thr
    for hh in (h, ha, hb, hs):
        m.matrix_free(hh)
    assert m.get_option("matrix_device_bytes") == 0
    m.close()


def test_subset_matrices_keep_the_callers_column_order(codebook_bytes, tiny):
    G = 300
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 350)
    listed = BASE + rng.permutation(G)[:97].astype(np.int64)                # a subset listed out of order: the device holds its columns by ascending global index
    order = np.argsort(listed)                                              # device position t is the caller's column order[t]
    sub = m.subset_create(listed)
    dev = [MM.cells(rng, (8, 97)) for _ in range(2)]
    hs = []
    for d in dev:
        m.debug_rank_rows(d, 1, subset=sub)
        hs.append(m.matrix_keep())
    caller = []
    for d in dev:
        c = np.empty_like(d); c[:, order] = d
        caller.append(c)
    assert m.matrix_info(hs[0]) == {"n_q": 8, "normalized": False, "columns": 97, "over_subset": True, "stale": False}
    same_words(m.matrix_read(hs[0]), caller[0], "read, the caller's order")
    got = m.matrix_fuse(hs, MM.SUM | MM.REQUIRE_ALL, weights=[2.0, 0.1], want_scores=True)
    same_words(got, MM.fuse(caller, MM.SUM | MM.REQUIRE_ALL, False, [2.0, 0.1]), "fuse over a subset")
    hits = m.rank_hits(NINF, 97)                                            # the result is a subset search's matrix: its lists name global indices
    want_dev = MM.fuse(dev, MM.SUM | MM.REQUIRE_ALL, False, [2.0, 0.1])
    held = np.sort(listed)
    best = np.argmax(MM.key_of(want_dev).astype(np.int64), axis=1)          # (argmax: the first of equal keys, the lowest global index)
    assert hits["idx"][:, 0].tolist() == held[best].tolist()
    plant(m, MM.cells(rng, (8, G)))
    whole = m.matrix_keep()
    with pytest.raises(M.AfisError, match=EINVAL):                          # a subset's columns and the whole shard's do not mix (nor do their shapes here)
        m.matrix_fuse([hs[0], whole], MM.MAX)
    m.subset_free(sub)
    assert m.matrix_info(hs[0])["stale"] is True and m.matrix_info(hs[0])["over_subset"] is True and m.matrix_info(whole)["stale"] is False
    for call in (lambda: m.matrix_read(hs[0]), lambda: m.matrix_recall(hs[1]), lambda: m.matrix_fuse(hs, MM.MAX)):
        with pytest.raises(M.AfisError, match=ESTATE) as e:
            call()
        assert "afis_subset_free" in str(e.value)
    for h in hs + [whole]:
        m.matrix_free(h)
    assert m.get_option("matrix_device_bytes") == 0
    m.close()


# ---- 4: one real search: a set of prints against itself, with planted near-duplicates -----------------------------------------------------------------------------
def test_symmetric_print_score_of_a_real_search(codebook_bytes, cb):
    n0 = 32
    gal = S.make_packed_gallery(SEED, n0, cb)
    copies = [2, 5, 8, 8, 11, 17, 20, 23, 27, 30]                           # ten prints enrolled again (one of them twice more)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal)
    for g in copies:
        m.gallery_add_packed(gal.slice(g, g + 1))
    m.gallery_commit(BASE)
    G = n0 + len(copies)
    idx = BASE + np.arange(G, dtype=np.int64)
    sub = m.subset_create(idx)                                              # the same set, in the same (ascending) order: row i and column i are one print
    sc = m.search_prints(idx, 1.0, 1.0, subset=sub)["scores"]
    h = m.matrix_keep()
    info = m.matrix_info(h)
    assert (info["n_q"], info["columns"], info["over_subset"]) == (G, G, True)
    down = m.matrix_read(h)
    same_words(down, sc, "the kept matrix is the search's scores")
    got = m.matrix_fuse([h, h], MM.MIN, transposed=[0, 1], want_scores=True)
    want = MM.fuse([down, np.ascontiguousarray(down.T)], MM.MIN, False)
    same_words(got, want, "min(a -> b, b -> a)")
    assert np.array_equal(MM.key_of(got), MM.key_of(got).T) and not np.array_equal(MM.key_of(down), MM.key_of(down).T)
    source = np.concatenate([np.arange(n0), copies])
    dup = (source[:, None] == source[None, :]) & ~np.eye(G, dtype=bool)
    key = MM.key_of(got).astype(np.int64)
    assert key[dup].min() > key[~dup & ~np.eye(G, dtype=bool)].max()        # the copies stand above every pair of different prints in the symmetric score too
    thr = float(got[dup][np.argmin(key[dup])])
    excl = [np.array([t], np.int64) for t in idx]
    res = m.link_groups(thr, LM.ANY, row_node=idx, excl=excl)               # link groups read the fused matrix
    model = LM.link(got, thr, idx, idx, LM.ANY, LM.not_excluded(idx, excl, G))
    assert res["n_groups"] == model["n_groups"] == len(set(copies)) and np.array_equal(res["group_off"], model["group_off"]) and np.array_equal(res["member"], model["member"])
    mut = m.link_groups(thr, LM.MUTUAL, row_node=idx, excl=excl)            # a symmetric matrix: every edge is confirmed
    assert mut["n_edges"] == res["n_edges"] and np.array_equal(mut["group_off"], res["group_off"]) and np.array_equal(mut["member"], res["member"])
    m.matrix_free(h); m.subset_free(sub)
    m.close()


# ---- 5: staleness and refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_staleness_and_refusals(codebook_bytes, tiny):
    G, n_q = 65, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    other = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 500)
    plant(other, MM.cells(rng, (n_q, G)))
    foreign = other.matrix_keep()
    plant(m, MM.cells(rng, (n_q - 1, G))); hb = m.matrix_keep()             # another shape
    plant(m, MM.cells(rng, (n_q, G)))
    m.normalize_scores(np.zeros(n_q), np.ones(n_q), axis=0); hc = m.matrix_keep()   # another kind
    rows = MM.cells(rng, (n_q, G))
    plant(m, rows)
    ha = m.matrix_keep()
    freed = m.matrix_keep(); m.matrix_free(freed)                           # (the last handle made: no later one can take its address while it is tested)
    before = m.rank_hits(NINF, G)
    nan, inf = float("nan"), float("inf")
    refused = [lambda: m.matrix_fuse([], MM.SUM), lambda: m.matrix_fuse([ha] * 17, MM.SUM), lambda: m.matrix_fuse([ha, hb], MM.SUM), lambda: m.matrix_fuse([ha, hc], MM.MAX),
               lambda: m.matrix_fuse([hc, ha], MM.MIN), lambda: m.matrix_fuse([ha, ha], MM.MAX, weights=[1.0, 1.0]), lambda: m.matrix_fuse([ha, ha], MM.MIN | MM.REQUIRE_ALL, weights=[1.0, 1.0]),
               lambda: m.matrix_fuse([ha, ha], MM.SUM, weights=[1.0, nan]), lambda: m.matrix_fuse([ha, ha], MM.SUM, weights=[inf, 1.0]), lambda: m.matrix_fuse([ha], 3),
               lambda: m.matrix_fuse([ha], 8), lambda: m.matrix_fuse([ha], -1), lambda: m.matrix_fuse([ha, foreign], MM.SUM), lambda: m.matrix_fuse([freed], MM.SUM),
               lambda: m.matrix_fuse([ha, ha], MM.MIN, transposed=[0, 1]), lambda: m.matrix_recall(foreign), lambda: m.matrix_recall(freed), lambda: m.matrix_read(foreign),
               lambda: m.matrix_info(freed), lambda: m.matrix_info(None), lambda: m.matrix_read(ha, 1, n_q), lambda: m.matrix_read(ha, -1, 1),
               lambda: m._chk(m.lib.afis_matrix_read(m.ctx, ha, 0, 1, None)), lambda: m._chk(m.lib.afis_matrix_fuse(m.ctx, None, None, None, 1, 0, None)),
               lambda: m._chk(m.lib.afis_matrix_keep(m.ctx, None)), lambda: m._chk(m.lib.afis_matrix_info(m.ctx, ha, None))]
    for i, call in enumerate(refused):
        with pytest.raises(M.AfisError, match=EINVAL):
            call()
            print("call", i, "was not refused")
        assert m.get_option("matrix_fuse_us") == 0, i                      # refused before anything was queued
        same_lists(m.rank_hits(NINF, G), before, ("the previous matrix still ranks", i))
    assert m.lib.afis_matrix_keep(None, None) == -1 and m.lib.afis_matrix_recall(None, ha) == -1
    m.matrix_free(freed); m.matrix_free(None)                               # freeing what is not live is ignored
    assert m.matrix_info(ha)["stale"] is False
    same_words(m.matrix_fuse([ha], MM.MAX, want_scores=True), MM.fuse([rows], MM.MAX, False), "one operand")
    # no last search: recall still works, keep does not
    m.subset_free(m.subset_create(BASE + np.arange(3)))                     # a call that invalidates the last search's matrix
    with pytest.raises(M.AfisError, match=ESTATE):
        m.matrix_keep()
    m.matrix_recall(ha)
    same_lists(m.rank_hits(NINF, G), before, "recalled without a last search")
    # an appending commit: every handle is the old shard's
    m.gallery_reopen(); m.gallery_add_packed(tiny.slice(G, G + 1)); m.gallery_commit(BASE)
    for call in (lambda: m.matrix_read(ha), lambda: m.matrix_recall(ha), lambda: m.matrix_fuse([ha], MM.SUM)):
        with pytest.raises(M.AfisError, match=ESTATE) as e:
            call()
        assert "the gallery was edited" in str(e.value) and "afis_gallery_commit" in str(e.value)
    assert m.matrix_info(ha)["stale"] is True and m.matrix_info(hb)["stale"] is True
    held = m.get_option("matrix_device_bytes")
    assert held == (n_q + (n_q - 1) + n_q) * G * 4
    m.matrix_free(ha)
    assert m.get_option("matrix_device_bytes") == held - n_q * G * 4
    plant(m, MM.cells(rng, (2, G + 1)))                                     # the new shard keeps and fuses
    hn = m.matrix_keep()
    assert m.matrix_info(hn) == {"n_q": 2, "normalized": False, "columns": G + 1, "over_subset": False, "stale": False}
    m.matrix_fuse([hn, hn], MM.SUM)
    m.close()                                                               # hb, hc and hn are live: afis_destroy releases them
    other.matrix_free(foreign)
    other.close()


# ---- 6: an empty matrix; afis_destroy with live handles -------------------------------------------------------------------------------------------------------------
def test_a_matrix_without_cells(codebook_bytes, cb):
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(S.make_packed_gallery(SEED, 4, cb)); m.gallery_commit(BASE)
    he = m.subset_create([])
    m.search_subset(he, S.make_latents(SEED, 2), k=0, want_scores=False)    # a search that covered no column
    h = m.matrix_keep()
    assert m.matrix_info(h) == {"n_q": 2, "normalized": False, "columns": 0, "over_subset": True, "stale": False}
    assert m.get_option("matrix_keep_us") == 0 and m.get_option("matrix_device_bytes") == 0
    assert m.matrix_read(h).shape == (2, 0)
    m.matrix_recall(h)
    assert m.matrix_fuse([h, h], MM.SUM, want_scores=True).shape == (2, 0) and m.get_option("matrix_fuse_us") == 0
    assert m.rank_hits(0.0, 4)["n_hits"].tolist() == [0, 0]
    m.matrix_free(h); m.subset_free(he)
    m.close()


def runtime_free_bytes():
    """Free bytes of device 0 by hipMemGetInfo of the HIP runtime the library is linked against (tests/test_gpu_large_shard.py's way)."""
    fn = M.load_library(M.TEST_LIB_PATH).hipMemGetInfo
    fn.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]; fn.restype = ctypes.c_int
    free_b, total_b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert fn(ctypes.byref(free_b), ctypes.byref(total_b)) == 0
    return int(free_b.value)


def test_destroy_releases_live_handles(codebook_bytes, tiny):
    n_q, G, per_round = 4096, G_MAX, 4
    rows = np.zeros((n_q, G), np.float32)
    bytes_round = per_round * n_q * G * 4                                   # 268 MB
    free_after = []
    for _ in range(3):
        m = tap_matcher(codebook_bytes, tiny, G)
        plant(m, rows)
        hs = [m.matrix_keep() for _ in range(per_round)]
        m.matrix_fuse([hs[0], hs[1]], MM.SUM, transposed=None)
        assert m.get_option("matrix_device_bytes") == bytes_round
        m.close()                                                           # nothing freed by hand
        free_after.append(runtime_free_bytes())
    assert free_after[0] - free_after[2] < bytes_round, free_after          # two rounds of leaked handles would hold 537 MB
