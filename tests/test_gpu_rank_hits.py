"""Hit lists on the GPU: afis_rank_hits / afis_rank_subject_hits, and the parity tap afis_debug_rank_hits.

The yardstick throughout is numpy.  A hit list is the longest prefix of the corresponding rank list whose entries reach min_score, "reach" decided on the rank list's own key:
  templates  key = ordered bits of (score + 0.0f), ties by ascending global index; min_score gets the same + 0.0f
  subjects   key = ordered bits of the raw score word, maximum per subject (and the lowest index that holds it), ties by ascending subject id; min_score's raw bits
(ordered: sign-magnitude order of the word: a NaN where its bits put it).  The model forms the keys, lexsorts, takes the prefix; n_hits, every entry and every padding
entry (-1, -inf, -1) must be equal, scores as raw words.

The kernel runs one 1024-thread workgroup per query over strips of 4096 positions, selects with a radix select on the key's four bytes when more than `cap` entries
qualify, and sorts at most 4096 composites: the tap's gallery sizes sit on, one before and one after the wave (64), chunk (1024) and strip / AFIS_HITS_MAX (4096) edges;
9001 spans three strips, 70001 would wrap any 16-bit counter."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 3107
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NEG_INF = np.float32(-np.inf).view(np.uint32)
F32 = np.float32
CAPS = (1, 63, 64, 65, 100, 1000, 4096)
G_TEMPLATES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 9001, 70001)
G_SUBJECTS = (65, 1025, 4099)
SPECIAL = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x3fc00000, 0xbf800000, 0x40500000], np.uint32).view(np.float32)   # +-inf, +-0, +-NaN, 1.5, -1, 3.25
ROW_SPECIAL = 8


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """70 001 rolled templates of one minutia and one texture point each (what tests/test_gpu_subject_rank.py's tap galleries hold), made as one packed gallery."""
    G = max(G_TEMPLATES)
    rng = np.random.default_rng(SEED)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    return S.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
                           off.copy(), rng.integers(0, 30, G).astype(np.int16), rng.integers(0, 30, G).astype(np.int16), rng.uniform(-1.5, 1.5, G).astype(np.float32),
                           rng.integers(0, cb.K, (G, cb.M)).astype(np.uint8))


def tap_matcher(cbb, tiny, G):
    m = M.Matcher(cbb, taps=True)
    m.gallery_add_packed(tiny.slice(0, G)); m.gallery_commit(BASE)
    return m


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def template_key(x):
    """k_topk's key word (minu.hip): the ordered bits of score + 0.0f."""
    return ordered((np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32))


def subject_key(x):
    return ordered(np.asarray(x, np.float32).view(np.uint32))


class TemplateModel:
    """One matrix: per row the positions in rank-list order and their keys, so that a (min_score, cap) pair costs one search in a sorted array."""

    def __init__(self, scores, glob):
        self.words = scores.view(np.uint32); self.glob = np.asarray(glob, np.int64)
        self.order, self.neg_key = [], []
        for q in range(scores.shape[0]):
            key = template_key(scores[q]).astype(np.int64)
            o = np.lexsort((self.glob, -key))                               # key descending, global index ascending
            self.order.append(o); self.neg_key.append(-key[o])

    def hits(self, min_score, cap):
        thr = int(template_key(np.array([min_score], np.float32))[0])
        n_q = len(self.order)
        n = np.empty(n_q, np.int64); idx = np.full((n_q, cap), -1, np.int64); sc = np.full((n_q, cap), NEG_INF, np.uint32)
        for q in range(n_q):
            n[q] = np.searchsorted(self.neg_key[q], -thr, side="right")     # keys >= thr: a prefix of the rank list
            take = self.order[q][:min(int(n[q]), cap)]
            idx[q, :len(take)] = self.glob[take]; sc[q, :len(take)] = self.words[q, take]
        return {"n_hits": n, "idx": idx, "score": sc}


class SubjectModel:
    def __init__(self, scores, glob, subject):
        """scores [n_q][n] over the columns the search covered, glob [n] their global indices, subject [n] their labels."""
        words = scores.view(np.uint32); glob = np.asarray(glob, np.int64); subject = np.asarray(subject, np.int64)
        self.rows = []
        for q in range(scores.shape[0]):
            key = subject_key(scores[q]).astype(np.int64)
            o = np.lexsort((glob, -key, subject))                           # by subject; inside one the greatest key first, equal keys by ascending index
            first = np.ones(len(o), bool); first[1:] = subject[o][1:] != subject[o][:-1]
            best = o[first]
            rank = best[np.lexsort((subject[best], -key[best]))]            # key descending, subject id ascending
            self.rows.append((-key[rank], subject[rank], words[q, rank], glob[rank]))

    def hits(self, min_score, cap):
        thr = int(subject_key(np.array([min_score], np.float32))[0])
        n_q = len(self.rows)
        n = np.empty(n_q, np.int64); ids = np.full((n_q, cap), -1, np.int64); sc = np.full((n_q, cap), NEG_INF, np.uint32); bi = np.full((n_q, cap), -1, np.int64)
        for q, (neg_key, subj, words, glob) in enumerate(self.rows):
            n[q] = np.searchsorted(neg_key, -thr, side="right")
            t = min(int(n[q]), cap)
            ids[q, :t] = subj[:t]; sc[q, :t] = words[:t]; bi[q, :t] = glob[:t]
        return {"n_hits": n, "subject": ids, "score": sc, "best_idx": bi}


def as_words(r):
    return {k: (v.view(np.uint32) if k == "score" else v) for k, v in r.items() if v is not None}


def assert_same(got, want, what=""):
    got = as_words(got)
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].tolist(), got[key].ravel()[:8].tolist(), want[key].ravel()[:8].tolist())


# ---- the tap's matrices ---------------------------------------------------------------------------------------------------------------------------------
def matrix(G, rng):
    """Nine rows: 0 all-distinct values (integers around zero), 1 nine distinct values, 2 all +0.0, 3 search-like (-1, 0 and a few positives), 4-7 words that differ in
    exactly one byte — byte 0, 1, 2, 3 of the float, so that each radix digit decides alone — and 8 infinities, both zeros and quiet NaNs of both signs among plain values."""
    rows = np.empty((9, G), np.float32)
    rows[0] = rng.permutation(G).astype(np.float32) - np.float32(G // 3)
    rows[1] = np.round(rng.random(G) * 8)
    rows[2] = 0.0
    u = rng.random(G)
    rows[3] = np.where(u < 0.05, -1.0, np.where(u < 0.07, rng.random(G) * 5 + 0.01, 0.0))
    for b in range(4):
        byte = rng.integers(0, 256, G).astype(np.uint32) if b < 3 else rng.choice(np.r_[1:0x80, 0x81:0xff], G).astype(np.uint32)   # (no zero exponent: no subnormal, no zero)
        rows[4 + b] = ((np.uint32(0x40404040) & ~np.uint32(0xff << (8 * b))) | (byte << np.uint32(8 * b))).view(np.float32)
    rows[ROW_SPECIAL] = SPECIAL[rng.integers(0, len(SPECIAL), G)]
    assert np.isfinite(rows[:ROW_SPECIAL]).all() and not (rows[:ROW_SPECIAL].view(np.uint32) == 0x80000000).any()
    return rows


def thresholds(rows):
    """-inf, -1, 0, and per row: a value present in it (the median of its distinct finite values), the value just above its finite maximum (no hits, unless the row holds
    +inf or a NaN) and a value between two present values (the middle of the widest gap between neighbours; -0.5 for a row of one value).  Every row meets every threshold."""
    out = [F32(-np.inf), F32(-1.0), F32(0.0)]
    no_hits = {}
    for r in range(rows.shape[0]):
        u = np.unique(rows[r][np.isfinite(rows[r])])
        above = np.nextafter(u[-1], F32(np.inf))
        gap = int(np.argmax(np.diff(u))) if len(u) > 1 else -1
        between = F32(u[gap] + (u[gap + 1] - u[gap]) / 2) if gap >= 0 else F32(-0.5)
        out += [u[len(u) // 2], above, between]
        no_hits[r] = above
    seen, uniq = set(), []
    for t in out:
        if t.view(np.uint32) not in seen:
            seen.add(int(t.view(np.uint32))); uniq.append(t)
    return uniq, no_hits


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", G_TEMPLATES)
def test_tap_sweep_templates(G, codebook_bytes, tiny):
    """Every matrix row x every cap x every threshold.  The tap uploads the matrix once; it stays rankable, and the product entry point answers the other combinations."""
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    rows = matrix(G, rng)
    model = TemplateModel(rows, BASE + np.arange(G))
    thrs, no_hits = thresholds(rows)
    assert_same(m.debug_rank_hits(None, rows, float(thrs[0]), CAPS[0]), model.hits(thrs[0], CAPS[0]), (G, "tap"))
    for t in thrs:
        for cap in CAPS:
            got = m.rank_hits(float(t), cap)
            assert_same(got, model.hits(t, cap), (G, float(t), cap))
            for r, above in no_hits.items():
                if r != ROW_SPECIAL and t == above:
                    assert got["n_hits"][r] == 0 and (got["idx"][r] == -1).all()
    full = m.rank_hits(float("-inf"), 4096)
    assert (full["n_hits"][:ROW_SPECIAL] == G).all()                        # everything reaches -inf but a NaN with the sign set
    assert full["n_hits"][ROW_SPECIAL] == G - int((rows[ROW_SPECIAL].view(np.uint32) == 0xffc00000).sum())
    assert m.get_option("rank_hits_us") > 0
    m.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------------
def label_plan(G, kind, rng):
    if kind == "identity":
        return 7000 + np.arange(G, dtype=np.int64)
    if kind == "half":                                                      # one subject holds the middle half of the gallery, every other template is a subject of its own
        return np.where((np.arange(G) >= G // 4) & (np.arange(G) < G // 4 + G // 2), 0, 10 + np.arange(G, dtype=np.int64))
    lengths = []                                                            # runs of 1 .. 129 templates across wave and workgroup edges, ids up to 2^40 in shuffled order
    while sum(lengths) < G:
        lengths.append(int(min(rng.choice([1, 2, 63, 64, 65, 127, 129, int(rng.integers(1, 40))]), G - sum(lengths))))
    ids = rng.permutation(np.unique(rng.integers(0, 1 << 40, 4 * len(lengths), dtype=np.int64)))[:len(lengths)]
    return np.repeat(ids, lengths)


@pytest.mark.parametrize("kind", ["runs", "half", "identity"])
@pytest.mark.parametrize("G", G_SUBJECTS)
def test_tap_sweep_subjects(G, kind, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 7 * G)
    rows = matrix(G, rng)
    subject = label_plan(G, kind, rng)
    assert len(subject) == G
    glob = BASE + np.arange(G)
    model = SubjectModel(rows, glob, subject)
    thrs, _ = thresholds(rows)
    h = m.subjects_create(subject)
    assert_same(m.debug_rank_hits(h, rows, float(thrs[0]), CAPS[0]), model.hits(thrs[0], CAPS[0]), (G, kind, "tap"))
    for t in thrs:
        for cap in CAPS:
            got = m.rank_subject_hits(h, float(t), cap)
            assert_same(got, model.hits(t, cap), (G, kind, float(t), cap))
            if kind == "identity":                                          # one person per template: the template hits, on every row that holds no -0.0
                tpl = m.rank_hits(float(t), cap)
                keep = slice(0, ROW_SPECIAL)
                assert np.array_equal(got["n_hits"][keep], tpl["n_hits"][keep]) and np.array_equal(got["best_idx"][keep], tpl["idx"][keep])
                assert np.array_equal(got["score"][keep].view(np.uint32), tpl["score"][keep].view(np.uint32))
                assert np.array_equal(np.where(got["subject"][keep] >= 0, got["subject"][keep] - 7000 + BASE, -1), tpl["idx"][keep])
    m.subjects_free(h)
    m.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def medium(cb):
    """tests/test_gpu_parity.py's medium set: 3000 templates with planted mates, six latents."""
    lats = S.make_latents(77, 6)
    gal = S.make_packed_gallery(77, 3000, cb)
    planted = S.plant_mates(77, gal, cb, lats)
    return lats, gal, planted


def test_against_the_siblings_on_a_real_search(codebook_bytes, medium):
    lats, gal, _ = medium
    G, Q = gal.G, len(lats)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal); m.gallery_commit(BASE)
    cards = np.arange(G, dtype=np.int64) // 10 * 3 + 50
    hj = m.subjects_create(cards)
    qh = m.upload_queries(lats)
    ninf = float("-inf")
    for k in (1, 24, 100, 64):                                              # 100: the search's host path; 64 last, its matrix serves the rest of the test
        r = m.search_resident(qh, k=k, want_scores=True)
        h = m.rank_hits(ninf, k)
        assert (h["n_hits"] == G).all(), k
        assert np.array_equal(h["idx"], r["topk_idx"]) and np.array_equal(h["score"].view(np.uint32), r["topk_score"].view(np.uint32)), k
    m.free_queries(qh)                                                      # (leaves the matrix alone)
    scores = r["scores"]
    assert (scores == 0).mean() > 0.3 and (scores >= 0).all()
    before = {k: m.rank_subjects(hj, Q, k) for k in (24, 64, 100)}
    for k in (24, 64, 100):                                                 # 100: afis_rank_subjects' host path
        h = m.rank_subject_hits(hj, ninf, k)
        assert (h["n_hits"] == G // 10).all()
        for key in ("subject", "score", "best_idx"):
            assert np.array_equal(h[key].view(np.uint32) if key == "score" else h[key], before[k][key].view(np.uint32) if key == "score" else before[k][key]), (k, key)
    hair = float(np.nextafter(F32(0), F32(1)))                              # a hair above 0: exactly the positive scores
    model = TemplateModel(scores, BASE + np.arange(G))
    got = m.rank_hits(hair, 4096)
    assert_same(got, model.hits(F32(hair), 4096), "hair above 0")
    for q in range(Q):
        pos = np.flatnonzero(scores[q] > 0)
        want = pos[np.lexsort((pos, -scores[q, pos].astype(np.float64)))]
        assert got["n_hits"][q] == len(pos) > 0 and np.array_equal(got["idx"][q, :len(pos)], BASE + want) and (got["idx"][q, len(pos):] == -1).all()
        assert np.array_equal(got["score"][q, :len(pos)], scores[q, want]) and np.isneginf(got["score"][q, len(pos):]).all()
    assert_same(m.rank_hits(hair, 4096), as_words(got), "a repeated call")
    assert_same(m.rank_hits(0.0, 100), model.hits(F32(0), 100), "the cut inside the tie at zero")
    assert_same(m.rank_subject_hits(hj, hair, 300), SubjectModel(scores, BASE + np.arange(G), cards).hits(F32(hair), 300), "subjects, hair above 0")
    after = m.rank_subjects(hj, Q, 24)                                      # the matrix is still rankable, and the sibling unchanged
    for key in ("subject", "score", "best_idx"):
        assert np.array_equal(after[key], before[24][key]), key
    # a latent-empty query: every score -1
    r = m.search([lats[0], T.FPTemplate()], k=24, want_scores=True)
    assert r["status"].tolist() == [0, 1] and (r["scores"][1] == -1).all()
    h = m.rank_hits(-1.0, 4096)
    assert h["n_hits"].tolist() == [G, G] and np.array_equal(h["idx"][1, :G], BASE + np.arange(G)) and (h["idx"][1, G:] == -1).all() and (h["score"][1, :G] == -1).all()
    h = m.rank_hits(0.0, 4096)
    assert h["n_hits"][1] == 0 and (h["idx"][1] == -1).all() and np.isneginf(h["score"][1]).all() and h["n_hits"][0] == G
    m.subjects_free(hj)
    m.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_subset_search(codebook_bytes, medium):
    lats, gal, planted = medium
    G = 600
    rng = np.random.default_rng(SEED + 4)
    m = M.Matcher(codebook_bytes)
    ts = [gal.template(g) for g in range(G)]
    ts[123] = T.FPTemplate()                                                # an empty entry: -1 against every latent
    m.gallery_add(ts); m.gallery_commit(BASE)
    cards = np.arange(G, dtype=np.int64) // 10 * 3 + 50
    listed = [int(g) for g in rng.permutation(np.r_[120:130, 300, 301, 305, rng.permutation(np.r_[0:120, 130:300, 310:600])[:28]])]   # card 12 whole, card 30 in part, 28 others
    assert listed != sorted(listed) and 123 in listed and len(set(listed)) == 41
    hs = m.subset_create([BASE + g for g in listed])
    hj = m.subjects_create(cards)
    r = m.search_subset(hs, lats[:3], k=24, want_scores=True)               # scores: column j belongs to listed[j]
    assert (r["scores"][:, listed.index(123)] == -1).all()
    glob = BASE + np.asarray(listed, np.int64)
    tm, sm = TemplateModel(r["scores"], glob), SubjectModel(r["scores"], glob, cards[listed])
    present = len({int(cards[g]) for g in listed})
    for t in (F32(-np.inf), F32(0.0), F32(np.nextafter(F32(0), F32(1)))):
        for cap in (24, 41, 100):                                           # below, at and above the subset's size: cap > n pads
            got = m.rank_hits(float(t), cap)
            assert_same(got, tm.hits(t, cap), ("subset", float(t), cap))
            assert np.isin(got["idx"][got["idx"] >= 0], glob).all()          # global indices of listed templates
            gs = m.rank_subject_hits(hj, float(t), cap)
            assert_same(gs, sm.hits(t, cap), ("subset subjects", float(t), cap))
    full = m.rank_hits(float("-inf"), 100)
    assert (full["n_hits"] == 41).all() and (full["idx"][:, 41:] == -1).all() and (full["idx"][:, 40] == BASE + 123).all()   # the empty entry's -1 comes last
    ties = [np.flatnonzero(full["score"][q, :41] == 0) for q in range(3)]
    assert all(len(t) > 5 and (np.diff(full["idx"][q, t]) > 0).all() for q, t in enumerate(ties))   # the zeros go by ascending GLOBAL index though the list was shuffled
    subj = m.rank_subject_hits(hj, float("-inf"), 100)
    assert (subj["n_hits"] == present).all() and (subj["subject"][:, present:] == -1).all()
    outside = sorted(set(cards.tolist()) - {int(cards[g]) for g in listed})
    assert len(outside) > 0 and not np.isin(subj["subject"], outside).any()  # a subject without a listed template neither appears nor counts
    assert np.isin(subj["best_idx"][:, :present], glob).all()
    m.subset_free(hs)
    with pytest.raises(M.AfisError, match=ESTATE):                          # the sub-shard the matrix refers to is gone
        m.rank_hits(0.0, 24)
    m.subjects_free(hj)
    m.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_states(codebook_bytes, medium):
    lats, gal, _ = medium
    lats = lats[:3]
    i64p, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal.slice(0, 150)); m.gallery_commit(BASE)
    tens = np.arange(150, dtype=np.int64) // 10
    ha = m.subjects_create(tens)
    with pytest.raises(M.AfisError, match=ESTATE):                          # before any search
        m.rank_hits(0.0, 24, n_q=3)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subject_hits(ha, 0.0, 24, n_q=3)
    full = m.search(lats, k=24, want_scores=True)
    nh = np.zeros(3, np.int64); a = np.zeros((3, 24), np.int64); sc = np.zeros((3, 24), np.float32); b = np.zeros((3, 24), np.int64)
    pn, pa, ps, pb = nh.ctypes.data_as(i64p), a.ctypes.data_as(i64p), sc.ctypes.data_as(fp), b.ctypes.data_as(i64p)
    rh, rs = m.lib.afis_rank_hits, m.lib.afis_rank_subject_hits
    nan = float("nan")
    assert rh(m.ctx, 2, 0.0, 24, pn, pa, ps) == -1 and rs(m.ctx, ha[0], 2, 0.0, 24, pn, pa, ps, pb) == -1          # n_q is not the search's
    for cap in (0, -1, 4097):
        assert rh(m.ctx, 3, 0.0, cap, pn, pa, ps) == -1 and rs(m.ctx, ha[0], 3, 0.0, cap, pn, pa, ps, pb) == -1
    assert rh(m.ctx, 3, nan, 24, pn, pa, ps) == -1 and rs(m.ctx, ha[0], 3, nan, 24, pn, pa, ps, pb) == -1
    assert rh(m.ctx, 3, 0.0, 24, None, pa, ps) == -1 and rh(m.ctx, 3, 0.0, 24, pn, None, ps) == -1 and rh(m.ctx, 3, 0.0, 24, pn, pa, None) == -1
    for args in ((None, pa, ps, pb), (pn, None, ps, pb), (pn, pa, None, pb), (pn, pa, ps, None)):
        assert rs(m.ctx, ha[0], 3, 0.0, 24, *args) == -1
    assert rs(m.ctx, None, 3, 0.0, 24, pn, pa, ps, pb) == -1
    hb = m.subjects_create(tens + 5)
    m.subjects_free(hb)
    assert rs(m.ctx, hb[0], 3, 0.0, 24, pn, pa, ps, pb) == -1               # a freed handle
    # the refused calls left the matrix rankable: both lists are right, and the option reads the call's device time
    scores = full["scores"]
    glob = BASE + np.arange(150)
    assert rh(m.ctx, 3, 0.0, 24, pn, pa, ps) == 0
    assert_same({"n_hits": nh, "idx": a, "score": sc}, TemplateModel(scores, glob).hits(F32(0), 24), "through the C ABI")
    assert m.get_option("rank_hits_us") > 0
    assert_same(m.rank_subject_hits(ha, 0.0, 24), SubjectModel(scores, glob, tens).hits(F32(0), 24))
    assert m.get_option("rank_hits_us") > 0
    assert_same(m.rank_hits(float("-inf"), 4096), TemplateModel(scores, glob).hits(F32(-np.inf), 4096), "cap 4096 over 150 templates")
    # calls that queue device work take the matrix away
    qh = m.upload_queries(lats)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_hits(0.0, 24)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subject_hits(ha, 0.0, 24)
    m.search_resident(qh, k=24)
    assert (m.rank_hits(float("-inf"), 24)["n_hits"] == 150).all()
    m.free_queries(qh)
    # a removal that changed the shard: no matrix, and after the next search the old subject handle is still refused
    m.gallery_remove([BASE + 47])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_hits(0.0, 24)
    edited = m.search(lats, k=24, want_scores=True)["scores"]
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subject_hits(ha, 0.0, 24)
    assert (edited[:, 47] == -1).all()
    got = m.rank_hits(0.0, 4096)
    assert_same(got, TemplateModel(edited, glob).hits(F32(0), 4096), "after the removal")
    assert (got["n_hits"] == 149).all() and not (got["idx"] == BASE + 47).any()
    m.subjects_free(ha)
    m.close()


def test_a_shard_of_empty_entries(codebook_bytes, medium):
    """A committed shard of empty entries only: every score is -1."""
    lats = medium[0][:3]
    e = M.Matcher(codebook_bytes)
    e.gallery_add([T.FPTemplate() for _ in range(5)]); e.gallery_commit(BASE)
    r = e.search(lats, k=3, want_scores=True)
    assert (r["scores"] == -1).all()
    h = e.rank_hits(-1.0, 8)
    assert h["n_hits"].tolist() == [5, 5, 5] and (h["idx"][:, :5] == BASE + np.arange(5)).all() and (h["idx"][:, 5:] == -1).all() and (h["score"][:, :5] == -1).all() and np.isneginf(h["score"][:, 5:]).all()
    h = e.rank_hits(0.0, 8)
    assert (h["n_hits"] == 0).all() and (h["idx"] == -1).all() and np.isneginf(h["score"]).all()
    hs = e.subjects_create([9, 9, 4, 4, 4])
    h = e.rank_subject_hits(hs, -1.0, 8)
    assert h["n_hits"].tolist() == [2, 2, 2] and h["subject"][0].tolist() == [4, 9, -1, -1, -1, -1, -1, -1] and h["best_idx"][0, :2].tolist() == [BASE + 2, BASE]
    e.subjects_free(hs)
    e.close()
