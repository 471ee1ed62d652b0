"""Eligible search on the GPU: afis_search_eligible scores a (latent, template) pair only where the template's label passes the latent's masks.

The yardstick is the FULL search of the same context, compared on raw words: an eligible cell is the full search's cell, every other cell the no-entry word
0xffffffff, and timing()["pairs"] is the number of pairs actually scored — the condition that keeps "full search plus filter" from passing.  The matrix left on the
device is read by the plain ranking calls as their _filtered forms read a full search's, and by the _filtered calls as they read a full search's.  The expand pass
(eligible_expand.hip) is swept on planted data through its parity tap, against numpy.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 3107
ESTATE, EINVAL = "afis error -3", "afis error -1"
MINUS1 = np.float32(-1).view(np.uint32)
NO_ENTRY = np.uint32(0xFFFFFFFF)
BASE = 1000
NINF = float("-inf")
ABOVE0 = float(np.nextafter(np.float32(0), np.float32(1)))
FINGERS = (1 << 10) - 1                                                     # ten one-hot finger bits; sex bits 10 and 11; one template carries bit 40
FIELDS = (1 << 12) - 1
Q0 = (0, 0, FIELDS & ~((1 << 2) | (1 << 7) | (1 << 10)))                    # fingers {2, 7} of sex bit 10, as a single none_of
MASKS7 = np.array([Q0, (0, 0, 0), (0, 1 << 50, 0), Q0, (1 << 40, 0, 0), Q0, (FINGERS, 0, 0)], np.uint64)
MATE_OF = {0: 22, 1: 15, 3: 47, 4: 33, 6: 68}                               # an eligible planted mate per latent that has one (shard-local)
INELIGIBLE_MATE = (0, 35)                                                   # a mate of latent 0 on finger 5: never scored
EMPTY = (2, 90)                                                             # empty entries: 2 is eligible for q0's class
BIT40_AT = 33
CASE_OF = [0, 0, 1, 1, 2, 2, 2]


def label_test(lab, masks):
    """[n_q][G] bool: the label test of include/afis_matcher.h."""
    L = np.asarray(lab, np.uint64)[None, :]
    a, b, c = (np.asarray(masks, np.uint64)[:, i][:, None] for i in range(3))
    return ((a == 0) | ((L & a) != 0)) & ((L & b) == b) & ((L & c) == 0)


def labels_of(G):
    i = np.arange(G)
    lab = (np.uint64(1) << (i % 10).astype(np.uint64)) | (np.uint64(1) << (10 + (i // 10) % 2).astype(np.uint64))
    if G > BIT40_AT:
        lab[BIT40_AT] |= np.uint64(1) << np.uint64(40)
    return lab


def class_pairs(ok):
    """The sum over the classes of n_c x m_c: every query of a class has the class's m eligible templates, so it is the number of eligible cells."""
    return int(ok.sum())


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def lats7():
    six = S.make_latents(SEED, 6, n_tex_lo=300, n_tex_hi=520)
    return six[:5] + [T.FPTemplate()] + six[5:]                             # q5 is latent-empty


@pytest.fixture(scope="module")
def pool(cb, lats7):
    """97 templates cut from one synthetic gallery, with the planted mates and the two empty entries."""
    pg = S.make_packed_gallery(SEED, 97, cb, n_tex_lo=300, n_tex_hi=520)
    ts = [pg.template(g) for g in range(97)]
    rng = np.random.default_rng(SEED + 1)
    for q, g in list(MATE_OF.items()) + [INELIGIBLE_MATE]:
        ts[g] = S.make_mate(rng, cb, lats7[q], frac=0.7, n_minu=ts[g].minu[0].n, n_tex=ts[g].tex[0].n)
    for g in EMPTY:
        ts[g] = T.FPTemplate()
    return ts


def fresh(cbb, ts, opts=None, taps=False):
    m = M.Matcher(cbb, taps=taps)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    m.gallery_add(ts)
    m.gallery_commit(BASE)
    return m


def same_lists(a, b, what=""):
    assert a.keys() == b.keys(), what
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape and np.array_equal(x, y), (what, key, np.argwhere(x != y)[:6].tolist() if x.shape == y.shape else (x.shape, y.shape))


def check_against_full(m, lats, lab, masks, h, what=""):
    """One full search and one eligible search on m: the words, the status and the pair count."""
    full = m.search(lats, k=0, want_scores=True)
    full_pairs = m.timing()["pairs"]
    got = m.search_eligible(lats, h, masks)
    tm = m.timing()
    ok = label_test(lab, masks)
    want = np.where(ok, full["scores"].view(np.uint32), NO_ENTRY)
    g = got["scores"].view(np.uint32)
    print(f"{what}: {len(lats)} x {len(lab)}: pairs {tm['pairs']} of the full search's {full_pairs}, classes {m.get_option('eligible_classes')}, "
          f"expand {m.get_option('eligible_expand_us')} us, total_ms {tm['total_ms']:.3f}")
    assert g.shape == want.shape and np.array_equal(g, want), (what, np.argwhere(g != want)[:8].tolist())
    assert np.array_equal(got["status"], full["status"]), what
    assert tm["pairs"] == class_pairs(ok), (what, tm["pairs"], class_pairs(ok), full_pairs)
    assert not (full["scores"].view(np.uint32) == NO_ENTRY).any()
    return full, got, tm


# ---- 1: the expand kernel through the tap, against numpy --------------------------------------------------------------------------------------------------
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFE, 0xBF800000, 0x3F800000, 0x00000001], np.uint32)


@pytest.mark.parametrize("G", [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097])
def test_expand_rows_against_numpy(G, codebook_bytes):
    m = M.Matcher(codebook_bytes, taps=True)
    rng = np.random.default_rng(SEED + G)
    for n_c in (1, 7, 65):
        n_q = 2 * n_c + 1
        row_of = np.arange(1, 2 * n_c, 2, dtype=np.int32)                   # interleaved with the rows of another class, which must come back untouched
        for mm in sorted({0, 1, G // 2, G}):
            cls = rng.integers(0, 1 << 32, (n_c, mm), dtype=np.uint64).astype(np.uint32)
            if mm:
                at = rng.random((n_c, mm)) < 0.3
                cls[at] = SPECIALS[rng.integers(0, len(SPECIALS), int(at.sum()))]
                cls[cls == NO_ENTRY] = np.uint32(0x12345678)
            prefill = rng.integers(0, 1 << 32, (n_q, G), dtype=np.uint64).astype(np.uint32)
            for sel in ([None, np.arange(G, dtype=np.int32)] if mm == G else [np.sort(rng.choice(G, mm, replace=False)).astype(np.int32)]):
                want = prefill.copy()
                want[row_of] = NO_ENTRY
                if mm:
                    want[np.ix_(row_of, np.arange(G) if sel is None else sel)] = cls
                got = m.debug_expand_rows(cls, row_of, sel, prefill)
                assert got.dtype == np.uint32 and np.array_equal(got, want), (G, n_c, mm, sel is None, np.argwhere(got != want)[:6].tolist())
    # the lists the tap refuses
    one = np.zeros((1, 1), np.uint32); out = np.zeros((2, G), np.uint32)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.debug_expand_rows(one, [2], [0], out)                             # a row outside out
    with pytest.raises(M.AfisError, match=EINVAL):
        m.debug_expand_rows(one, [0], [G], out)                             # a column outside out
    if G > 1:
        with pytest.raises(M.AfisError, match=EINVAL):
            m.debug_expand_rows(np.zeros((1, 2), np.uint32), [0], [1, 0], out)   # not ascending
        with pytest.raises(M.AfisError, match=EINVAL):
            m.debug_expand_rows(one, [0], None, out)                        # no list, and not every column
    m.close()


# ---- 2: the search ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [96, 97])
def test_eligible_cells_are_the_full_searchs(G, codebook_bytes, pool, lats7):
    m = fresh(codebook_bytes, pool[:G])
    lab = labels_of(G)
    h = m.labels_create(lab)
    ok = label_test(lab, MASKS7)
    assert ok[1].all() and ok[6].all() and not ok[2].any() and ok[4].sum() == 1 and 0 < ok[0].sum() < G and np.array_equal(ok[0], ok[3]) and np.array_equal(ok[0], ok[5])
    full, got, tm = check_against_full(m, lats7, lab, MASKS7, h, f"G = {G}")
    assert m.get_option("eligible_classes") == 5 and m.get_option("eligible_expand_us") >= 0
    assert tm["pairs"] == 3 * int(ok[0].sum()) + G + 0 + 1 + G
    g = got["scores"].view(np.uint32)
    assert got["status"][5] == 1 and (got["status"][[0, 1, 2, 3, 4, 6]] == 0).all()
    assert (g[5][ok[5]] == MINUS1).all() and (g[0, EMPTY[0]] == MINUS1) and (g[1, list(EMPTY)] == MINUS1).all() and (g[2] == NO_ENTRY).all()
    assert g[INELIGIBLE_MATE] == NO_ENTRY and full["scores"][INELIGIBLE_MATE] > 0
    lists = m.rank_hits(NINF, 5)
    for q, t in MATE_OF.items():                                            # each eligible planted mate leads its latent's list
        assert ok[q, t] and int(lists["idx"][q, 0]) == BASE + t and lists["score"][q, 0] > 0, (q, t, lists["idx"][q], lists["score"][q])
    assert lists["n_hits"][2] == 0 and (lists["idx"][2] == -1).all() and lists["n_hits"][4] == 1
    m.labels_free(h)
    m.close()


# ---- 3: the ranking family on that matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [96, 97])
def test_ranking_equivalences(G, codebook_bytes, pool, lats7):
    m = fresh(codebook_bytes, pool[:G])
    lab = labels_of(G)
    h = m.labels_create(lab)
    hj = m.subjects_create(np.arange(G) // 10)
    excl_t = [[BASE + 22], [BASE + 15, BASE + 3], [], [BASE + 47, BASE + 999999], [], [BASE + 7], [BASE + 68]]
    excl_s = [[2], [1, 0], [], [4], [], [0], [6, 12345]]
    f = dict(labels=h, masks=MASKS7)

    def filtered_family():
        out = {}
        for t in (NINF, ABOVE0):
            out["hits", t] = m.rank_hits_filtered(t, 100, **f)
            out["subject hits", t] = m.rank_subject_hits_filtered(hj, t, 100, **f)
            out["latent hits", t] = m.rank_latent_hits_filtered(t, 100, **f)
            out["hits, excl", t] = m.rank_hits_filtered(t, 100, excl=excl_t, **f)
            out["subject hits, excl", t] = m.rank_subject_hits_filtered(hj, t, 100, excl=excl_s, **f)
            out["latent hits, excl", t] = m.rank_latent_hits_filtered(t, 100, excl=excl_t, **f)
            for mode in (M.CASE_SUM, M.CASE_MAX):
                out["case hits", mode, t] = m.rank_case_hits_filtered(CASE_OF, mode, t, 100, **f)
                out["case hits, excl", mode, t] = m.rank_case_hits_filtered(CASE_OF, mode, t, 100, excl=excl_t, **f)
                out["case subject hits", mode, t] = m.rank_case_subject_hits_filtered(hj, CASE_OF, mode, t, 100, **f)
                out["case subject hits, excl", mode, t] = m.rank_case_subject_hits_filtered(hj, CASE_OF, mode, t, 100, excl=excl_s, **f)
        return out

    m.search(lats7, k=0, want_scores=False)
    want = filtered_family()
    m.search_eligible(lats7, h, MASKS7, want_scores=False)
    for t in (NINF, ABOVE0):                                                # the plain calls read the matrix as their _filtered forms read a full search's
        same_lists(m.rank_hits(t, 100), want["hits", t], ("rank_hits", t))
        same_lists(m.rank_subject_hits(hj, t, 100), want["subject hits", t], ("rank_subject_hits", t))
        same_lists(m.rank_latent_hits(t, 100), want["latent hits", t], ("rank_latent_hits", t))
    got = filtered_family()                                                 # ... and the _filtered calls return what they return after a full search
    assert got.keys() == want.keys()
    for key in want:
        same_lists(got[key], want[key], key)
    assert want["hits", NINF]["n_hits"].tolist() == label_test(lab, MASKS7).sum(axis=1).tolist()
    m.labels_free(h); m.subjects_free(hj)
    m.close()


# ---- 4: nothing of the call stays behind ------------------------------------------------------------------------------------------------------------------
def test_no_leaks(codebook_bytes, pool, lats7):
    G = 97
    m = fresh(codebook_bytes, pool[:G])
    lab = labels_of(G)
    h = m.labels_create(lab)
    idx = [BASE + g for g in (47, 3, 22, 96, 0, 68, 15)]
    hs = m.subset_create(idx)
    qh = m.upload_queries(lats7[:3])
    kw = dict(k=24, want_scores=True, want_parts=True)

    def words(r):
        return {k: (v.view(np.uint32) if v.dtype == np.float32 else v) for k, v in r.items() if v is not None}

    sub_before = words(m.search_subset_resident(hs, qh, **kw))
    full_before = words(m.search(lats7, **kw))
    held, h2d, gather = m.get_option("subset_device_bytes"), m.get_option("gallery_h2d_bytes"), m.get_option("subset_gather_us")
    assert held > 0
    first = m.search_eligible(lats7, h, MASKS7)
    pairs = m.timing()["pairs"]
    assert (m.get_option("subset_device_bytes"), m.get_option("gallery_h2d_bytes"), m.get_option("subset_gather_us")) == (held, h2d, gather)
    same_lists(words(m.search_subset_resident(hs, qh, **kw)), sub_before, "the caller's subset and query handle after an eligible search")
    second = m.search_eligible(lats7, h, MASKS7)
    same_lists(words(second), words(first), "a repeated eligible search")
    assert m.timing()["pairs"] == pairs and m.get_option("eligible_classes") == 5
    same_lists(words(m.search(lats7, **kw)), full_before, "a full search after the eligible one")
    same_lists(words(m.search_resident(qh, **kw)), {k: v[:3] for k, v in full_before.items()}, "the query handle on the resident shard")
    assert m.get_option("subset_device_bytes") == held
    m.free_queries(qh); m.subset_free(hs); m.labels_free(h)
    assert m.get_option("subset_device_bytes") == 0
    m.close()


# ---- 5: options -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G, opts", [(96, {"adc_variant": 8}), (97, {"ref_tie_order": 2})], ids=["variant8", "tie2"])
def test_options(G, opts, codebook_bytes, pool, lats7):
    m = fresh(codebook_bytes, pool[:G], opts)
    lab = labels_of(G)
    h = m.labels_create(lab)
    check_against_full(m, lats7, lab, MASKS7, h, str(opts))
    assert m.get_option("eligible_classes") == 5
    m.labels_free(h)
    m.close()


# ---- 6: one larger case -----------------------------------------------------------------------------------------------------------------------------------
def test_a_class_on_the_overlapped_schedule(codebook_bytes, cb):
    """12 000 templates, 10 latents: seven share a mask that passes 10 800 templates (75 600 pairs, above the 65 536 at which a launch group runs on the CU-masked
    streams), two a mask that passes 1 200 and one another mask that passes 1 200."""
    G = 12000
    pg = S.make_packed_gallery(SEED + 5, G, cb)
    lats = S.make_latents(SEED + 5, 10)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(pg); m.gallery_commit(BASE)
    lab = labels_of(G)
    h = m.labels_create(lab)
    wide, one, half = (0, 0, 1 << 9), (1 << 3, 0, 0), ((1 << 1) | (1 << 2), 1 << 11, 0)
    masks = np.array([wide, one, wide, wide, half, wide, wide, one, wide, wide], np.uint64)
    ok = label_test(lab, masks)
    assert ok[0].sum() == 10800 and ok[1].sum() == 1200 and ok[4].sum() == 1200
    _, _, tm = check_against_full(m, lats, lab, masks, h, "12 000 templates")
    assert tm["pairs"] == 7 * 10800 + 2 * 1200 + 1200 and m.get_option("eligible_classes") == 3
    assert tm["overlapped_groups"] >= 1 and tm["launch_groups"] >= 3, tm
    m.labels_free(h)
    m.close()


# ---- 7: life cycle ----------------------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(codebook_bytes, pool, lats7):
    G = 96
    m = fresh(codebook_bytes, pool[:G])
    lab = labels_of(G)
    h = m.labels_create(lab)
    other = fresh(codebook_bytes, pool[:G])
    h_other = other.labels_create(lab)
    empty_ctx = M.Matcher(codebook_bytes)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.search_eligible(lats7, None, MASKS7)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.search_eligible(lats7, h, None)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.search_eligible(lats7, h_other, MASKS7)                           # a handle of another context
    with pytest.raises(M.AfisError, match=ESTATE):
        empty_ctx.search_eligible(lats7, h_other, MASKS7)                   # before the first commit
    z = m.search_eligible([], h, np.zeros((0, 3), np.uint64))
    assert z["scores"].shape == (0, G) and z["status"].shape == (0,) and m.get_option("eligible_classes") == 0
    before = m.search_eligible(lats7, h, MASKS7)["scores"].view(np.uint32)
    assert before[0, 22] != MINUS1 and before[0, 22] != NO_ENTRY
    m.gallery_remove([BASE + 22])
    with pytest.raises(M.AfisError, match=ESTATE):                          # labels from before the edit
        m.search_eligible(lats7, h, MASKS7)
    m.labels_free(h)
    h = m.labels_create(lab)                                                # new labels of the shard as it stands
    after = m.search_eligible(lats7, h, MASKS7)["scores"].view(np.uint32)
    assert after[0, 22] == MINUS1 and after[3, 22] == MINUS1                # the removed template is eligible still, and an empty entry
    keep = np.ones(G, bool); keep[22] = False
    assert np.array_equal(after[:, keep], before[:, keep])
    assert int(m.rank_hits(NINF, 5)["idx"][3, 0]) == BASE + 47
    m.labels_free(h); other.labels_free(h_other)
    m.close(); other.close(); empty_ctx.close()
