"""Subject rank lists on the GPU: afis_subjects_create / afis_subjects_free / afis_rank_subjects, and the parity tap afis_debug_rank_subjects.

The yardstick throughout is a host model over the SAME context's full-search score matrix: the uint32 words go through the ordered form of a float's bits (sign-magnitude
order: -0.0 below +0.0, a NaN where its bits put it), are grouped by subject id — the greatest key, and the lowest global index that holds it — and sorted by (key
descending, id ascending); ids, score words and indices must be equal (np.array_equal on raw words), the padding (-1, -inf, -1) included.

Gallery: the 600-template pool with planted mates and the three latents of tests/test_gpu_subset_search.py's recipe, committed at index_base 5000.  k_subject_best runs
workgroups of 256 positions (four waves of 64) and merges equal labels inside a wave only: the run lengths of the label shapes below put run ends on, one before and one
after the wave edges (63, 64, 65, 127, 128) and carry runs across the workgroup edges at 256 and 512; the tap's galleries of 1, 63, 64, 65, 1023, 1025 and 4099
templates do the same for the end of the row.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 2209
BASE = 5000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NEG_INF = np.float32(-np.inf).view(np.uint32)
MINUS1 = np.float32(-1).view(np.uint32)


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def lats():
    return S.make_latents(SEED, 3, n_tex_lo=300, n_tex_hi=520)


@pytest.fixture(scope="module")
def pool(cb, lats):
    """600 templates of one synthetic gallery; entries 310 + 20 q + {0, 1, 2} and 40 + 7 q carry mates of latent q (the recipe of tests/test_gpu_subset_search.py)."""
    pg = S.make_packed_gallery(SEED, 600, cb, n_tex_lo=300, n_tex_hi=520)
    ts = [pg.template(g) for g in range(600)]
    rng = np.random.default_rng(SEED + 1)
    for q, L in enumerate(lats):
        for j, frac in enumerate((0.8, 0.5, 0.3)):
            g = 310 + 20 * q + j
            ts[g] = S.make_mate(rng, cb, L, frac=frac, n_minu=ts[g].minu[0].n, n_tex=ts[g].tex[0].n)
        g = 40 + 7 * q
        ts[g] = S.make_mate(rng, cb, L, frac=0.6, n_minu=ts[g].minu[0].n, n_tex=ts[g].tex[0].n)
    return ts


def fresh(cbb, ts, opts=None, index_base=BASE, taps=False):
    m = M.Matcher(cbb, taps=taps)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    m.gallery_add(ts)
    m.gallery_commit(index_base)
    return m


@pytest.fixture(scope="module")
def m600(codebook_bytes, pool):
    m = fresh(codebook_bytes, pool)
    yield m
    m.close()


def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def model(words, subject, k, base=BASE, cols=None):
    """words: [n_q][G] uint32 of a full search of the shard; subject: [G] ids; cols: the shard-local columns the search covered (None: all).  -> subject, score words, best_idx [n_q][k]."""
    words = np.asarray(words, np.uint32)
    subject = np.asarray(subject, np.int64)
    cols = np.arange(words.shape[1]) if cols is None else np.asarray(cols, np.int64)
    n_q = words.shape[0]
    out_i = np.full((n_q, k), -1, np.int64); out_s = np.full((n_q, k), NEG_INF, np.uint32); out_b = np.full((n_q, k), -1, np.int64)
    subj = subject[cols]
    for q in range(n_q):
        key = ordered(words[q, cols]).astype(np.int64)
        order = np.lexsort((cols, -key, subj))                               # by subject; inside one the greatest key first, equal keys by ascending index
        first = np.ones(len(order), bool); first[1:] = subj[order][1:] != subj[order][:-1]
        best = order[first]
        rank = best[np.lexsort((subj[best], -key[best]))][:k]                # key descending, subject id ascending
        out_i[q, :len(rank)] = subj[rank]; out_s[q, :len(rank)] = words[q, cols[rank]]; out_b[q, :len(rank)] = base + cols[rank]
    return {"subject": out_i, "score": out_s, "best_idx": out_b}


def as_words(r):
    return {"subject": r["subject"], "score": r["score"].view(np.uint32), "best_idx": r["best_idx"]}


def assert_lists(got, want, what=""):
    for key in ("subject", "score", "best_idx"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].tolist(), got[key].ravel()[:8].tolist(), want[key].ravel()[:8].tolist())


def ranked(m, subject, n_q, k):
    h = m.subjects_create(subject)
    try:
        return as_words(m.rank_subjects(h, n_q, k))
    finally:
        m.subjects_free(h)


def runs(lengths, ids=None):
    ids = np.arange(len(lengths), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    return np.repeat(ids, lengths)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_identity_is_the_template_rank_list(m600, lats):
    """subject[i] = 7000 + i: entry for entry the rank list afis_search returns."""
    subject = 7000 + np.arange(600, dtype=np.int64)
    for k in (1, 24, 64):
        r = m600.search(lats, k=k, want_scores=False)
        got = ranked(m600, subject, 3, k)
        assert np.array_equal(got["subject"] - 7000 + BASE, r["topk_idx"]), k
        assert np.array_equal(got["score"], r["topk_score"].view(np.uint32)), k
        assert np.array_equal(got["best_idx"], r["topk_idx"]), k
    assert all(int(got["best_idx"][q, 0]) - BASE in (310 + 20 * q, 311 + 20 * q, 312 + 20 * q, 40 + 7 * q) for q in range(3))   # a planted mate leads


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def label_shapes():
    rng = np.random.default_rng(SEED + 11)
    lengths = []
    while sum(lengths) < 600:
        lengths.append(int(min(rng.integers(1, 40), 600 - sum(lengths))))
    wide_ids = rng.permutation(np.unique(rng.integers(0, 1 << 40, 4 * len(lengths), dtype=np.int64)))[:len(lengths)]   # distinct, up to 2^40, in shuffled order of first appearance
    return {"contiguous tens": np.arange(600, dtype=np.int64) // 10 + 100,
            "i % 60 (every neighbour differs, A B A)": np.arange(600, dtype=np.int64) % 60,
            "one subject of 400 plus singletons": np.concatenate([np.arange(100, dtype=np.int64) + 1, np.zeros(400, np.int64), np.arange(100, dtype=np.int64) + 1000]),
            "runs 63 1 64 65 127 2 128 150": runs([63, 1, 64, 65, 127, 2, 128, 150], [9, 3, 8, 1, 7, 2, 11, 5]),
            "random runs, ids up to 2^40": runs(lengths, wide_ids),
            "one subject holds everything": np.full(600, 77, np.int64)}


def test_label_shapes(m600, lats):
    full = m600.search(lats, k=24, want_scores=True)
    words = full["scores"].view(np.uint32)
    handles = {name: m600.subjects_create(subject) for name, subject in label_shapes().items()}   # several live handles, one search
    for name, subject in label_shapes().items():
        assert len(subject) == 600
        got = as_words(m600.rank_subjects(handles[name], 3, 24))
        assert_lists(got, model(words, subject, 24), name)
        if name == "one subject holds everything":
            assert (got["subject"][:, 0] == 77).all() and (got["subject"][:, 1:] == -1).all() and (got["score"][:, 1:] == NEG_INF).all() and (got["best_idx"][:, 1:] == -1).all()
            assert np.array_equal(got["best_idx"][:, 0], full["topk_idx"][:, 0])
        if name == "contiguous tens":                                       # a card with planted mates leads: latent q's are cards 31 + 2 q and (40 + 7 q) // 10
            assert all(int(got["subject"][q, 0]) in (131 + 2 * q, 100 + (40 + 7 * q) // 10) for q in range(3))
    for h in handles.values():
        m600.subjects_free(h)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
VALUES = np.array([-1.0, -0.0, 0.0, 1.5, 1.5, 3.25, np.inf, -np.inf, np.nan], np.float32)


@pytest.fixture(scope="module")
def tiny(cb):
    rng = np.random.default_rng(SEED + 12)
    return [S.make_rolled(rng, cb, n_minu=1, n_tex=1) for _ in range(4099)]


@pytest.mark.parametrize("G", [1, 63, 64, 65, 1023, 1025, 4099])
def test_tap_with_hand_made_matrices(G, codebook_bytes, tiny):
    """Scores from nine values (most subjects tie; zeros of both signs, infinities, the NaN 0x7fc00000), labels of 1-9 templates per subject, k on both paths."""
    assert VALUES.view(np.uint32)[8] == 0x7fc00000 and VALUES.view(np.uint32)[1] == 0x80000000
    m = fresh(codebook_bytes, tiny[:G], taps=True)
    rng = np.random.default_rng(SEED + 13 + G)
    for n_q in (1, 3):
        lengths = []
        while sum(lengths) < G:
            lengths.append(int(min(rng.integers(1, 10), G - sum(lengths))))
        subject = runs(lengths, rng.permutation(3 * len(lengths))[:len(lengths)])
        if n_q == 3:
            subject = subject[rng.permutation(G)]                           # the same subjects, their templates anywhere in the shard
        scores = VALUES[rng.integers(0, len(VALUES), (n_q, G))]
        if n_q == 3:
            scores[1] = -1.0
        words = scores.view(np.uint32)
        h = m.subjects_create(subject)
        for k in (24, 100):
            got = as_words(m.debug_rank_subjects(h, scores, k))
            assert_lists(got, model(words, subject, k), (G, n_q, k))
        if n_q == 3:
            n = min(24, len(lengths))
            assert np.array_equal(got["subject"][1, :n], np.unique(subject)[:n]) and (got["score"][1, :n] == MINUS1).all()
        m.subjects_free(h)
    m.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_subset_search(m600, lats):
    subject = np.arange(600, dtype=np.int64) // 10 * 3 + 50                 # cards of ten: subject 50 + 3 c
    rng = np.random.default_rng(SEED + 14)
    inside = list(range(310, 320))                                          # card 31 wholly inside (latent 0's mates)
    partly = [330, 331, 335, 339]                                           # card 33 partly (two of latent 1's three mates)
    others = [10 * c + int(rng.integers(10)) for c in (0, 2, 5, 7, 11, 12, 19, 20, 28, 34, 35, 41, 47, 52, 58, 59)]
    listed = [int(g) for g in rng.permutation(inside + partly + others)]
    assert listed != sorted(listed)
    full = m600.search(lats, k=24, want_scores=True)
    words = full["scores"].view(np.uint32)
    hs = m600.subset_create([BASE + g for g in listed])
    hj = m600.subjects_create(subject)
    m600.search_subset(hs, lats, k=24, want_scores=False)
    present = len({int(subject[g]) for g in listed})
    assert present == 18
    for k in (24, 100):                                                     # both exceed the subjects present: the padding is exact
        got = as_words(m600.rank_subjects(hj, 3, k))
        assert_lists(got, model(words, subject, k, cols=listed), k)
        assert (got["subject"][:, present:] == -1).all() and (got["subject"][:, :present] >= 0).all()
        assert np.isin(got["best_idx"][:, :present] - BASE, listed).all()
        assert not np.isin(got["subject"], subject[[400, 450, 570, 320, 329]]).any()         # cards 40, 45, 57 and 32: wholly outside the list
    assert got["subject"][:, 0].tolist()[:2] == [50 + 3 * 31, 50 + 3 * 33]  # the listed mates' cards lead
    m600.subset_free(hs)
    with pytest.raises(M.AfisError, match=ESTATE):                          # the sub-shard the matrix refers to is gone
        m600.rank_subjects(hj, 3, 24)
    m600.subjects_free(hj)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_launch_groups(codebook_bytes, cb):
    """12 000 templates x 3 latents with option query_batch 1: three launch groups write their rows of the matrix one after the other."""
    pg = S.make_packed_gallery(SEED + 5, 12000, cb)
    lats3 = S.make_latents(SEED + 5, 3)
    m = M.Matcher(codebook_bytes)
    m.set_option("query_batch", 1)
    m.gallery_add_packed(pg); m.gallery_commit(BASE)
    rng = np.random.default_rng(SEED + 15)
    lengths = []
    while sum(lengths) < 12000:
        lengths.append(int(min(rng.integers(1, 30), 12000 - sum(lengths))))
    subject = runs(lengths, rng.permutation(len(lengths)))
    full = m.search(lats3, k=24, want_scores=True)
    assert m.timing()["launch_groups"] == 3
    got = ranked(m, subject, 3, 24)
    assert_lists(got, model(full["scores"].view(np.uint32), subject, 24), "three launch groups")
    print("subject_rank_us at 3 x 12 000:", m.get_option("subject_rank_us"))
    assert m.get_option("subject_rank_us") > 0
    m.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_latent_empty_query_in_the_batch(m600, lats):
    subject = (np.arange(600, dtype=np.int64) * 7 % 45) * 11 + 4              # 45 subjects, their templates spread over the shard
    batch = [lats[0], T.FPTemplate(), lats[2]]
    full = m600.search(batch, k=24, want_scores=True)
    assert full["status"].tolist() == [0, 1, 0] and (full["scores"][1].view(np.uint32) == MINUS1).all()
    got = ranked(m600, subject, 3, 24)
    assert_lists(got, model(full["scores"].view(np.uint32), subject, 24))
    ids = np.unique(subject)[:24]
    assert np.array_equal(got["subject"][1], ids) and (got["score"][1] == MINUS1).all()
    assert got["best_idx"][1].tolist() == [BASE + int(np.flatnonzero(subject == s).min()) for s in ids]


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_state_and_errors(codebook_bytes, pool, lats):
    i64p, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    m = M.Matcher(codebook_bytes)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.subjects_create([0])                                              # before the first commit
    base_ts = pool[:150]
    m.gallery_add(base_ts); m.gallery_commit(BASE)
    tens = np.arange(150, dtype=np.int64) // 10
    h2d = m.get_option("gallery_h2d_bytes")
    for bad in (tens[:149], np.concatenate([tens, [3]]), np.where(np.arange(150) == 70, -1, tens)):        # wrong n (both ways), a negative id
        with pytest.raises(M.AfisError, match=EINVAL):
            m.subjects_create(bad)
    assert m.get_option("gallery_h2d_bytes") == h2d
    ha = m.subjects_create(tens)
    assert m.get_option("gallery_h2d_bytes") == h2d + 150 * 4 + 15 * 8      # the slots and the id table, counted as a subset's tables are
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subjects(ha, 3, 24)                                          # before any search
    full = m.search(lats, k=24, want_scores=True)
    words = full["scores"].view(np.uint32)
    sid = np.zeros((3, 24), np.int64); sc = np.zeros((3, 24), np.float32); bi = np.zeros((3, 24), np.int64)
    a, b, c = sid.ctypes.data_as(i64p), sc.ctypes.data_as(fp), bi.ctypes.data_as(i64p)
    assert m.lib.afis_rank_subjects(m.ctx, ha[0], 2, 24, a, b, c) == -1     # n_q is not the search's
    assert m.lib.afis_rank_subjects(m.ctx, ha[0], 3, 0, a, b, c) == -1
    assert m.lib.afis_rank_subjects(m.ctx, ha[0], 3, 24, None, b, c) == -1 and m.lib.afis_rank_subjects(m.ctx, ha[0], 3, 24, a, None, c) == -1 and m.lib.afis_rank_subjects(m.ctx, ha[0], 3, 24, a, b, None) == -1
    # the refused calls, a second handle's creation, options and timing leave the matrix rankable: two handles on one search both give right answers
    other = np.arange(150, dtype=np.int64) % 7 + 1000
    hb = m.subjects_create(other)
    m.timing(); m.get_option("gallery_resident"); assert m.gallery_size == 150
    assert_lists(as_words(m.rank_subjects(ha, 3, 24)), model(words, tens, 24), "first handle")
    assert_lists(as_words(m.rank_subjects(hb, 3, 24)), model(words, other, 24), "second handle")
    assert_lists(as_words(m.rank_subjects(ha, 3, 5)), model(words, tens, 5), "again, another k")
    # calls that run searches of their own
    m.correspondences(lats[0], [BASE + 40, BASE + 41])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subjects(ha, 3, 24)
    m.search(lats, k=24, want_scores=False)
    m.One2One_matching_all_templates(lats[0])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subjects(ha, 3, 24)
    # a removal: the old handles are refused whatever was searched since; a new one equals a freshly committed context's result
    m.gallery_remove([BASE + 47, BASE + 20])
    m.search(lats, k=24, want_scores=False)
    for h in (ha, hb):
        with pytest.raises(M.AfisError, match=ESTATE):
            m.rank_subjects(h, 3, 24)
    m.subjects_free(ha)                                                     # a stale handle frees cleanly
    single = np.where(np.arange(150) == 47, 999, tens)                      # a subject whose only template is an empty entry now: -1
    edited = [T.FPTemplate() if i in (47, 20) else t for i, t in enumerate(base_ts)]
    f = fresh(codebook_bytes, edited)
    f_words = f.search(lats, k=24, want_scores=True)["scores"].view(np.uint32)
    assert (f_words[:, 47] == MINUS1).all()
    want = model(f_words, single, 100)
    assert_lists(ranked(m, single, 3, 100), want, "after the removal")
    assert_lists(ranked(f, single, 3, 100), want, "the freshly committed context itself")
    at = np.argwhere(want["subject"] == 999)
    assert len(at) == 3 and (want["score"][want["subject"] == 999] == MINUS1).all()
    f.close()
    # an appending commit: the old handle is refused, one with the new n works
    hc = m.subjects_create(single)
    m.gallery_reopen(); m.gallery_add(pool[300:340]); m.gallery_commit(BASE)
    m.search(lats, k=24, want_scores=False)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subjects(hc, 3, 24)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.subjects_create(single)                                           # 150 ids for 190 templates
    grown = np.concatenate([single, np.arange(40, dtype=np.int64) // 4 + 5])   # the appended prints join subjects 5 .. 14 and so straddle the two parts
    f = fresh(codebook_bytes, edited + pool[300:340])
    f_words = f.search(lats, k=24, want_scores=True)["scores"].view(np.uint32)
    got = ranked(m, grown, 3, 24)
    assert_lists(got, model(f_words, grown, 24), "after the append")
    assert int(got["best_idx"][0, 0]) == BASE + 160                         # pool 310, latent 0's best mate
    f.close()
    m.subjects_free(hb); m.subjects_free(hc)
    left = m.subjects_create(grown)                                         # still live at close: afis_destroy releases it
    assert left[1] == 190
    m.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_search_is_left_alone(codebook_bytes, pool, lats):
    m = fresh(codebook_bytes, pool[:200])
    kw = dict(k=24, want_scores=True, want_parts=True)
    before = m.search(lats, **kw)
    tm = m.timing()
    h = m.subjects_create(np.arange(200, dtype=np.int64) // 10)
    first = as_words(m.rank_subjects(h, 3, 24))
    assert m.timing() == tm                                                 # the last SEARCH's times
    second = as_words(m.rank_subjects(h, 3, 24))
    assert_lists(first, second, "two rank calls in a row")
    host = as_words(m.rank_subjects(h, 3, 100))                             # the host's path agrees with the device's where both answer
    assert_lists({k: v[:, :20] for k, v in host.items()}, {k: v[:, :20] for k, v in first.items()}, "k = 100 against k = 24")
    after = m.search(lats, **kw)
    for key in ("scores", "parts", "topk_score"):
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key
    assert np.array_equal(before["topk_idx"], after["topk_idx"]) and np.array_equal(before["status"], after["status"])
    m.subjects_free(h)
    m.close()
