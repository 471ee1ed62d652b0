"""Case lists on the GPU: afis_rank_case_hits / afis_rank_case_subject_hits fuse the queries of one case into one row and rank the fused rows.

The yardstick is numpy, compared bit for bit.  The fused value of (case, column) is folded over the case's members in ascending query position by a Python loop on
whole rows: a member takes part when template_key(v) >= template_key(+0.0); SUM is acc = (acc + row).astype(float32) from +0.0 over the members that take part, -1
where none does; MAX the value of greatest key, first member's bits.  For subjects a member's row is the per-subject maximum on the raw word's order (what
k_subject_best makes); subjects no column covers are no entries.  The fused rows are then listed as the sibling tests list a search's: lexsort on template_key
descending and the global index (or subject id) ascending, cut at min_score's key and at cap; case_id, n_hits, every entry and every padding entry (-1, -inf) must be
equal, scores as raw words.

Shapes: the fold kernel takes four columns per thread where G % 4 == 0 and one otherwise, 256 threads a workgroup; k_rank_hits works in strips of 4096 and sorts at
most 4096 composites: G sits on, before and after the wave (64), the workgroup (256), 1024 and 4096, with odd and even rows.  Case sizes 1, 2, 64, 65 and all-in-one
cross the fold loop's unroll of four."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 5309
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NEG_INF = np.float32(-np.inf).view(np.uint32)
F32 = np.float32
HAIR = F32(np.nextafter(F32(0), F32(1)))                                    # the smallest positive float
SUM, MAX = M.CASE_SUM, M.CASE_MAX
MODES = (SUM, MAX)
CAPS = (1, 100, 4096)
G_TEMPLATES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097)
N_QS = (1, 2, 65, 300)
SIZES = (1, 2, 64, 65)
S_SUBJECTS = (1, 64, 65, 1025)
G_TINY = 10250                                                              # 1025 cards of ten
SPECIAL = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x3fc00000, 0xbf800000, 0x40500000], np.uint32).view(np.float32)   # +-inf, +-0, +-NaN, 1.5, -1, 3.25
KINDS = ("search-like", "zeros", "integers", "order", "special")


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """10 250 rolled templates of one minutia and one texture point each (tests/test_gpu_rank_hits.py's tap gallery), as one packed gallery."""
    G = G_TINY
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


def unordered(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000), o ^ np.uint32(0x80000000), ~o).astype(np.uint32)


def template_key(x):
    """rank_key (csrc/rank_order.h): the ordered bits of score + 0.0f."""
    return ordered((np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32))


ZERO_KEY = template_key(np.zeros(1, np.float32))[0]


def fuse(rows, case_of, mode):
    """rows [n_q][n] -> (the distinct case ids ascending, fused [n_cases][n]): the fold of the header, member by member on whole rows."""
    case_of = np.asarray(case_of, np.int64)
    ids = np.unique(case_of)
    out = np.empty((len(ids), rows.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for r, cid in enumerate(ids):
            members = np.flatnonzero(case_of == cid)                        # ascending query position
            if mode == SUM:
                acc = np.zeros(rows.shape[1], np.float32); took = np.zeros(rows.shape[1], bool)
                for i in members:
                    row = rows[i]
                    part = template_key(row) >= ZERO_KEY
                    acc = np.where(part, (acc + row).astype(np.float32), acc); took |= part
                out[r] = np.where(took, acc, np.float32(-1.0))
            else:
                best = rows[members[0]].view(np.uint32).copy(); key = template_key(rows[members[0]])
                for i in members[1:]:
                    k = template_key(rows[i])
                    take = k > key                                          # strictly: the first member of the greatest key keeps its bits
                    best = np.where(take, rows[i].view(np.uint32), best); key = np.where(take, k, key)
                out[r] = best.view(np.float32)
    return ids, out


def subject_best(rows, subject):
    """rows [n_q][n], subject [n] labels of the columns -> (the labels present, ascending; best [n_q][S]): per query and subject the maximum on the raw word's order."""
    subject = np.asarray(subject, np.int64)
    ids, slot = np.unique(subject, return_inverse=True)
    o = np.argsort(slot, kind="stable")
    starts = np.flatnonzero(np.r_[True, slot[o][1:] != slot[o][:-1]])
    key = ordered(np.ascontiguousarray(rows).view(np.uint32))[:, o]
    return ids, unordered(np.maximum.reduceat(key, starts, axis=1)).view(np.float32)


class Lists:
    """fused [n_cases][n] with the entries' names (global indices or subject ids): per row the rank-list order and its keys; a (min_score, cap) pair is one search."""

    def __init__(self, case_ids, fused, names, what):
        self.case_ids = case_ids; self.words = np.ascontiguousarray(fused).view(np.uint32); self.names = np.asarray(names, np.int64); self.what = what
        self.order, self.neg_key = [], []
        for r in range(fused.shape[0]):
            key = template_key(fused[r]).astype(np.int64)
            o = np.lexsort((self.names, -key))                              # key descending, name ascending
            self.order.append(o); self.neg_key.append(-key[o])

    def hits(self, min_score, cap):
        thr = int(template_key(np.array([min_score], np.float32))[0])
        n_c = len(self.order)
        n = np.empty(n_c, np.int64); a = np.full((n_c, cap), -1, np.int64); sc = np.full((n_c, cap), NEG_INF, np.uint32)
        for r in range(n_c):
            n[r] = np.searchsorted(self.neg_key[r], -thr, side="right")     # keys >= thr: a prefix of the rank list
            take = self.order[r][:min(int(n[r]), cap)]
            a[r, :len(take)] = self.names[take]; sc[r, :len(take)] = self.words[r, take]
        return {"case_id": self.case_ids, "n_hits": n, self.what: a, "score": sc}


def template_lists(rows, case_of, mode, glob):
    ids, fused = fuse(rows, case_of, mode)
    return Lists(ids, fused, glob, "idx"), fused


def subject_lists(rows, case_of, mode, subject):
    """subject [n]: the labels of the columns the matrix holds (a subset: of the listed templates only — the others' subjects are no entries)."""
    sid, best = subject_best(rows, subject)
    ids, fused = fuse(best, case_of, mode)
    return Lists(ids, fused, sid, "subject"), fused


def as_words(r):
    return {k: (v.view(np.uint32) if k == "score" and v.dtype != np.uint32 else v) for k, v in r.items() if v is not None}


def assert_same(got, want, what=""):
    got = as_words(got); want = as_words(want)
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].tolist(), got[key].ravel()[:8].tolist(), want[key].ravel()[:8].tolist())


def thresholds(fused):
    finite = np.unique(fused[np.isfinite(fused)])
    inside = finite[len(finite) // 2] if len(finite) else F32(1.5)           # a value inside the data
    return (F32(-np.inf), F32(0.0), HAIR, F32(inside))


# ---- matrices and case plans ----------------------------------------------------------------------------------------------------------------------------
def matrix(kind, n_q, G, rng):
    if kind == "search-like":                                               # -1, 0 and a few positives; a latent-empty row and an empty entry's column of -1
        u = rng.random((n_q, G))
        m = np.where(u < 0.05, -1.0, np.where(u < 0.12, rng.random((n_q, G)) * 5 + 0.01, 0.0)).astype(np.float32)
        if n_q > 1:
            m[n_q // 2] = -1.0
        m[:, G // 2] = -1.0
        return m
    if kind == "zeros":
        return np.zeros((n_q, G), np.float32)
    if kind == "integers":                                                  # distinct, both signs
        return (rng.permutation(n_q * G).astype(np.float32) - np.float32(n_q * G // 3)).reshape(n_q, G)
    if kind == "order":                                                     # positives of very different magnitude with full mantissas: nearly every other order of the adds, or a tree, rounds differently
        return np.ldexp((1 + rng.random((n_q, G))).astype(np.float32), rng.integers(-8, 25, (n_q, G))).astype(np.float32)
    return SPECIAL[rng.integers(0, len(SPECIAL), (n_q, G))]


def plans(n_q, rng):
    """Two assignments of the query positions to cases: sizes 1, 2, 64, 65 in turn while they fit (then what is left), and all in one.  The members of a case are
    interleaved with the others' (a permutation deals the positions); ids are not dense and DEscend with the position of a case's first member."""
    out = []
    for sizes in ("mixed", "one"):
        case = np.empty(n_q, np.int64)
        perm = rng.permutation(n_q)
        at, k = 0, 0
        while at < n_q:
            size = n_q if sizes == "one" else min(SIZES[k % len(SIZES)], n_q - at)
            case[perm[at:at + size]] = k
            at += size; k += 1
        first = np.array([np.flatnonzero(case == c)[0] for c in range(k)])
        rank = np.argsort(np.argsort(first))                                # 0 = the case that begins first
        ids = 7 + (13 << 28) * (k - 1 - rank)                               # past 2^31 from the second case on
        out.append(ids[case])
    return out


# ---- 1: templates --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", G_TEMPLATES)
def test_template_sweep(G, codebook_bytes, tiny):
    """Every n_q x plan x matrix kind x mode x cap x threshold.  The tap uploads a matrix once; it stays rankable, and the new entry point answers everything else."""
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    glob = BASE + np.arange(G)
    sizes_seen = set()
    for n_q in N_QS:
        ps = plans(n_q, rng)
        if n_q > 1:
            assert not np.array_equal(np.argsort(ps[0], kind="stable"), np.arange(n_q))   # members interleaved
        for kind in KINDS:
            rows = matrix(kind, n_q, G, rng)
            m.debug_rank_hits(None, rows, float("-inf"), 1)
            for case_of in ps:
                sizes_seen |= set(np.unique(case_of, return_counts=True)[1].tolist())
                for mode in MODES:
                    model, fused = template_lists(rows, case_of, mode, glob)
                    for t in thresholds(fused):
                        for cap in CAPS:
                            assert_same(m.rank_case_hits(case_of, mode, float(t), cap), model.hits(t, cap), (G, n_q, kind, mode, float(t), cap))
            assert m.get_option("rank_cases_us") > 0
    assert sizes_seen >= {1, 2, 64, 65, 300}
    m.close()


def test_the_sum_is_sequential(codebook_bytes, tiny):
    """2^24, 1, 1 in one case: 2^24 in the order of the members (each 1 is half an ulp and rounds away), 2^24 + 2 for a tree or for any order that adds the ones first."""
    m = tap_matcher(codebook_bytes, tiny, 5)
    rows = np.array([[2.0 ** 24] * 5, [1] * 5, [1] * 5, [-1] * 5], np.float32)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    got = m.rank_case_hits([4, 4, 4, 4], SUM, float("-inf"), 5)
    assert got["case_id"].tolist() == [4] and got["n_hits"].tolist() == [5] and got["idx"][0].tolist() == list(range(BASE, BASE + 5)) and (got["score"] == F32(2.0 ** 24)).all()
    got = m.rank_case_hits([9, 3, 3, 9], SUM, float("-inf"), 1)             # rows: case 3 = 1 + 1, case 9 = 2^24 (the -1 stays out)
    assert got["case_id"].tolist() == [3, 9] and got["score"][:, 0].tolist() == [2.0, 2.0 ** 24]
    got = m.rank_case_hits([0, 1, 2, 3], SUM, 0.0, 2)                       # a case of one latent-empty query: -1, nothing reaches 0
    assert got["n_hits"].tolist() == [5, 5, 5, 0] and (got["idx"][3] == -1).all() and np.isneginf(got["score"][3]).all()
    m.close()


# ---- 2: identity with the siblings ---------------------------------------------------------------------------------------------------------------------
def test_identity_with_the_siblings(codebook_bytes, tiny):
    """Every query its own case, ascending ids: both modes are afis_rank_hits entry for entry, and the subject call afis_rank_subject_hits' ids and scores."""
    G, n_q = 1025, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 2)
    rows = matrix("search-like", n_q, G, rng)
    case_of = 5 + 3 * np.arange(n_q)
    h = m.subjects_create(np.arange(G, dtype=np.int64) // 10 * 7 + 1)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    for t in (float("-inf"), -1.0, 0.0, float(HAIR)):
        for cap in (1, 100, 4096):
            tpl = m.rank_hits(t, cap); sub = m.rank_subject_hits(h, t, cap)
            for mode in MODES:
                got = m.rank_case_hits(case_of, mode, t, cap)
                assert np.array_equal(got["case_id"], case_of)
                assert_same({k: got[k] for k in ("n_hits", "idx", "score")}, tpl, ("templates", mode, t, cap))
                gs = m.rank_case_subject_hits(h, case_of, mode, t, cap)
                assert_same({k: gs[k] for k in ("n_hits", "subject", "score")}, {k: sub[k] for k in ("n_hits", "subject", "score")}, ("subjects", mode, t, cap))
    m.subjects_free(h)
    m.close()


# ---- 3: subjects -----------------------------------------------------------------------------------------------------------------------------------------
def labels(n_subjects, kind, rng):
    """-> the label of every template.  cards: contiguous cards of ten; random: 3 S + 1 templates dealt at random (every subject present); half: one subject holds
    half the shard, every other template is a subject of its own."""
    if kind == "cards":
        return np.repeat(50 + 3 * np.arange(n_subjects, dtype=np.int64), 10)
    ids = rng.permutation(np.unique(rng.integers(0, 1 << 40, 4 * n_subjects + 8, dtype=np.int64)))[:n_subjects]
    if kind == "random":
        return ids[rng.permutation(np.r_[np.arange(n_subjects), rng.integers(0, n_subjects, 2 * n_subjects + 1)])]
    G = max(2 * (n_subjects - 1), 4)
    lab = np.full(G, ids[0], np.int64)
    others = np.r_[0:G // 4, G // 4 + G // 2:G][:n_subjects - 1]
    lab[others] = ids[1:]
    return lab


@pytest.mark.parametrize("kind", ["cards", "random", "half"])
@pytest.mark.parametrize("n_subjects", S_SUBJECTS)
def test_subject_sweep(n_subjects, kind, codebook_bytes, tiny):
    rng = np.random.default_rng(SEED + 11 * n_subjects + len(kind))
    subject = labels(n_subjects, kind, rng)
    G, n_q = len(subject), 67                                               # 67 queries: cases of 1, 2 and 64, or all in one
    assert len(np.unique(subject)) == n_subjects and G <= G_TINY
    m = tap_matcher(codebook_bytes, tiny, G)
    h = m.subjects_create(subject)
    ps = plans(n_q, rng)
    for mk in KINDS:
        rows = matrix(mk, n_q, G, rng)
        m.debug_rank_hits(None, rows, float("-inf"), 1)
        for case_of in ps:
            for mode in MODES:
                model, fused = subject_lists(rows, case_of, mode, subject)
                for t in thresholds(fused):
                    for cap in CAPS:
                        assert_same(m.rank_case_subject_hits(h, case_of, mode, float(t), cap), model.hits(t, cap), (n_subjects, kind, mk, mode, float(t), cap))
    m.subjects_free(h)
    m.close()


# ---- 4: subsets ------------------------------------------------------------------------------------------------------------------------------------------
def test_subsets(codebook_bytes, tiny):
    """A subset listed out of order: the lists carry global indices, and subjects without a listed template are neither counted nor listed, at -inf too."""
    G, n_q = 600, 7
    rng = np.random.default_rng(SEED + 4)
    m = tap_matcher(codebook_bytes, tiny, G)
    cards = np.arange(G, dtype=np.int64) // 10 * 3 + 50
    listed = [int(g) for g in rng.permutation(np.r_[120:130, 300, 301, 305, rng.permutation(np.r_[0:120, 130:300, 310:600])[:50]])]   # card 12 whole, card 30 in part, 50 others
    assert listed != sorted(listed) and len(set(listed)) == 63              # 63 columns: odd rows
    hs = m.subset_create([BASE + g for g in listed])
    hj = m.subjects_create(cards)
    held = np.sort(np.asarray(listed))                                      # the device holds the listed templates in ascending global order
    case_of = np.array([8, 2, 8, 8, 2, 1 << 33, 2], np.int64)
    present = np.unique(cards[held])
    for kind in KINDS:
        rows = matrix(kind, n_q, len(held), rng)
        m.debug_rank_rows(rows, 1, subset=hs)
        for mode in MODES:
            tm, fused = template_lists(rows, case_of, mode, BASE + held)
            sm, sfused = subject_lists(rows, case_of, mode, cards[held])
            for t in thresholds(fused) + thresholds(sfused)[3:]:
                for cap in (1, 63, 100):
                    got = m.rank_case_hits(case_of, mode, float(t), cap)
                    assert_same(got, tm.hits(t, cap), ("subset", kind, mode, float(t), cap))
                    assert np.isin(got["idx"][got["idx"] >= 0], BASE + held).all()
                    assert_same(m.rank_case_subject_hits(hj, case_of, mode, float(t), cap), sm.hits(t, cap), ("subset subjects", kind, mode, float(t), cap))
            full = m.rank_case_subject_hits(hj, case_of, mode, float("-inf"), 4096)
            assert (full["n_hits"] <= len(present)).all() and np.isin(full["subject"][full["subject"] >= 0], present).all()
            if kind != "special":                                           # (a NaN with the sign set lies below -inf)
                assert (full["n_hits"] == len(present)).all() and (full["subject"][:, len(present):] == -1).all()
    m.subset_free(hs)
    with pytest.raises(M.AfisError, match=ESTATE):                          # the sub-shard the matrix refers to is gone
        m.rank_case_hits(case_of, SUM, 0.0, 24)
    m.subjects_free(hj)
    m.close()


# ---- 5: a real search ------------------------------------------------------------------------------------------------------------------------------------
def test_a_real_search(codebook_bytes, cb):
    """40 templates with planted mates; six latents in three cases (3 + 2 + 1), one of them latent-empty.  The search's own outputs do not change."""
    G = 40
    lats = S.make_latents(83, 5, n_tex_lo=400, n_tex_hi=600)
    gal = S.make_packed_gallery(83, G, cb)
    S.plant_mates(83, gal, cb, lats)
    lats = lats[:2] + [T.FPTemplate()] + lats[2:]                           # position 2 is latent-empty
    case_of = np.array([30, 11, 30, 11, 5, 30], np.int64)                   # case 30: positions 0, 2 (empty), 5; case 11: 1, 3; case 5: 4
    cards = np.arange(G, dtype=np.int64) // 4 * 9 + 2
    plain = M.Matcher(codebook_bytes)
    plain.gallery_add_packed(gal); plain.gallery_commit(BASE)
    want = plain.search(lats, k=24, want_scores=True, want_parts=True)
    plain.close()
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal); m.gallery_commit(BASE)
    hj = m.subjects_create(cards)
    r = m.search(lats, k=24, want_scores=True, want_parts=True)
    scores = r["scores"]
    assert r["status"].tolist() == [0, 0, 1, 0, 0, 0] and (scores[2] == -1).all() and (scores[[0, 1, 3, 4, 5]] > 0).any(axis=1).all()
    glob = BASE + np.arange(G)
    for mode in MODES:
        tm, fused = template_lists(scores, case_of, mode, glob)
        sm, _ = subject_lists(scores, case_of, mode, cards)
        assert (fused >= 0).all()                                           # the empty latent drags no case to -1
        for t in (F32(-np.inf), F32(0.0), HAIR, F32(np.median(fused[fused > 0]))):
            for cap in (1, 24, 100):
                assert_same(m.rank_case_hits(case_of, mode, float(t), cap), tm.hits(t, cap), ("search", mode, float(t), cap))
                assert_same(m.rank_case_subject_hits(hj, case_of, mode, float(t), cap), sm.hits(t, cap), ("search subjects", mode, float(t), cap))
    again = m.search(lats, k=24, want_scores=True, want_parts=True)
    for res in (r, again):
        for key in ("scores", "parts", "status", "topk_idx", "topk_score"):
            assert np.array_equal(res[key].view(np.uint32) if res[key].dtype == np.float32 else res[key], want[key].view(np.uint32) if want[key].dtype == np.float32 else want[key]), key
    m.subjects_free(hj)
    m.close()


# ---- 6: errors and states --------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_states(codebook_bytes, tiny):
    i64p, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    G, n_q = 150, 4
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 6)
    tens = np.arange(G, dtype=np.int64) // 10
    ha = m.subjects_create(tens)
    co = np.array([7, 3, 7, 3], np.int64)
    cid = np.zeros(2, np.int64); nh = np.zeros(2, np.int64); a = np.zeros((2, 24), np.int64); sc = np.zeros((2, 24), np.float32)
    pc, pi, pn, pa, ps = co.ctypes.data_as(i64p), cid.ctypes.data_as(i64p), nh.ctypes.data_as(i64p), a.ctypes.data_as(i64p), sc.ctypes.data_as(fp)
    rc, rs = m.lib.afis_rank_case_hits, m.lib.afis_rank_case_subject_hits
    both = (lambda *x: rc(m.ctx, *x), lambda *x: rs(m.ctx, ha[0], *x))
    for f in both:
        assert f(pc, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -3            # before any search
    rows = matrix("search-like", n_q, G, rng)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    glob = BASE + np.arange(G)
    neg = np.array([7, -1, 7, 3], np.int64)
    for f in both:
        for mode in (-1, 2):
            assert f(pc, n_q, mode, 2, 0.0, 24, pi, pn, pa, ps) == -1
        assert f(neg.ctypes.data_as(i64p), n_q, SUM, 3, 0.0, 24, pi, pn, pa, ps) == -1
        assert f(None, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -1
        for args in ((None, pn, pa, ps), (pi, None, pa, ps), (pi, pn, None, ps), (pi, pn, pa, None)):
            assert f(pc, n_q, SUM, 2, 0.0, 24, *args) == -1
        for bad_q in (3, 5, -1):
            assert f(pc, bad_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -1
        for bad_c in (1, 0, 3):
            assert f(pc, n_q, SUM, bad_c, 0.0, 24, pi, pn, pa, ps) == -1
        assert "n_cases is 3" in m.lib.afis_last_error(m.ctx).decode() and "2 distinct" in m.lib.afis_last_error(m.ctx).decode()   # both numbers
        for cap in (0, -1, 4097):
            assert f(pc, n_q, SUM, 2, 0.0, cap, pi, pn, pa, ps) == -1
        assert f(pc, n_q, SUM, 2, float("nan"), 24, pi, pn, pa, ps) == -1
    assert rs(m.ctx, None, pc, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -1
    hb = m.subjects_create(tens + 5)
    m.subjects_free(hb)
    assert rs(m.ctx, hb[0], pc, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -1   # a freed handle
    # the refused calls left the matrix rankable; through the C ABI, repeated, and mixed with the four existing ranking calls
    tm = {mode: template_lists(rows, co, mode, glob)[0] for mode in MODES}
    sm = {mode: subject_lists(rows, co, mode, tens)[0] for mode in MODES}
    assert rc(m.ctx, pc, n_q, MAX, 2, 0.0, 24, pi, pn, pa, ps) == 0
    assert_same({"case_id": cid, "n_hits": nh, "idx": a, "score": sc}, tm[MAX].hits(F32(0), 24), "through the C ABI")
    assert m.get_option("rank_cases_us") > 0 and m.get_option("case_fuse_us") >= 0 and m.get_option("case_rank_us") >= 0
    before = (m.rank_hits(0.0, 24), m.rank_subject_hits(ha, 0.0, 24), m.rank_subjects(ha, n_q, 24), m.rank_latent_hits(0.0, 4))
    for mode in MODES:
        assert_same(m.rank_case_hits(co, mode, 0.0, 24), tm[mode].hits(F32(0), 24), ("mixed", mode))
        assert_same(m.rank_case_subject_hits(ha, co, mode, float(HAIR), 24), sm[mode].hits(HAIR, 24), ("mixed subjects", mode))
        assert_same(m.rank_case_hits(co, mode, 0.0, 24), tm[mode].hits(F32(0), 24), ("repeated", mode))
    after = (m.rank_hits(0.0, 24), m.rank_subject_hits(ha, 0.0, 24), m.rank_subjects(ha, n_q, 24), m.rank_latent_hits(0.0, 4))
    for b, f in zip(before, after):
        assert_same(f, as_words(b), "the siblings on the same matrix")
    assert_same(m.rank_case_hits(co, SUM, float("-inf"), 4096), tm[SUM].hits(F32(-np.inf), 4096), "after the siblings, cap 4096 over 150 templates")
    # an empty subset: a search of no columns — zero counts and padding, the rows still named
    lats = S.make_latents(83, n_q, n_tex_lo=400, n_tex_hi=500)
    he = m.subset_create([])
    qr = m.upload_queries(lats, reserve=8)
    m.search_subset_resident(he, qr, k=0)
    for got in (m.rank_case_hits(co, SUM, float("-inf"), 5), m.rank_case_subject_hits(ha, co, MAX, float("-inf"), 5)):
        assert got["case_id"].tolist() == [3, 7] and (got["n_hits"] == 0).all() and np.isneginf(got["score"]).all()
        assert (got.get("idx", got.get("subject")) == -1).all()
    assert m.get_option("rank_cases_us") == 0
    m.subset_free(he); m.free_queries(qr)
    # calls that queue device work take the matrix away; a search of no queries ranks no case
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    assert (m.rank_case_hits(co, SUM, float("-inf"), 5)["n_hits"] == G).all()
    qh = m.upload_queries(lats)
    for f in both:
        assert f(pc, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -3
    m.free_queries(qh)
    q0 = m.upload_queries([], reserve=G)
    m.search_resident(q0, k=0)
    z = m.rank_case_hits([], SUM, 0.0, 5)
    assert z["case_id"].shape == (0,) and z["idx"].shape == (0, 5)
    assert rc(m.ctx, pc, 0, SUM, 1, 0.0, 24, pi, pn, pa, ps) == -1           # no query, one case
    assert rs(m.ctx, ha[0], pc, 0, MAX, 0, 0.0, 24, pi, pn, pa, ps) == 0
    m.free_queries(q0)
    # a gallery edit: no matrix, and the subject handle belongs to the older gallery
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    m.gallery_remove([BASE + 47])
    for f in both:
        assert f(pc, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -3
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    assert rc(m.ctx, pc, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == 0
    assert rs(m.ctx, ha[0], pc, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -3
    m.subjects_free(ha)
    m.close()
