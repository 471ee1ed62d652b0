"""Filtered hit lists on the GPU: afis_labels_create, afis_rank_hits_filtered / afis_rank_subject_hits_filtered.

The yardstick is numpy, compared bit for bit.  A cell (query, column) is ELIGIBLE when the label of the column's template passes the query's masks
((any_of == 0 or L & any_of) and L & all_of == all_of and not L & none_of) and the template (its global index), or its person (the subject id), is not on the query's
exclusion list.  The model is the sibling tests' restricted to the eligible cells:
  templates  key = ordered bits of (score + 0.0f), ties by ascending global index; min_score gets the same + 0.0f
  subjects   key = ordered bits of the raw score word, maximum per subject over the ELIGIBLE cells (and the lowest index that holds it), ties by ascending subject id
The model lexsorts the eligible cells once per matrix and filter, then a (min_score, cap) pair is a search in a sorted array; n_hits, every entry and every padding entry
(-1, -inf, -1) must be equal, scores as raw words.  Matrices are planted with the existing taps: debug_rank_hits (a full search's) and debug_rank_rows(subset=...).

Shapes: k_filter_rows takes four columns per thread where G % 4 == 0 and one otherwise, 256 threads a workgroup, strips of R = 8 query rows; k_rank_hits works in
strips of 4096 and sorts at most 4096 composites: G sits on, before and after the wave (64), the workgroup (256), 1024 and 4096, with odd and even rows; n_q on, before
and after the strip, and 65 = eight strips and one row."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 7411
BASE = 1000
R = 8                                                                       # csrc/afis_device.h: kFilterRows
ESTATE, EINVAL = "afis error -3", "afis error -1"
NEG_INF = np.float32(-np.inf).view(np.uint32)
F32, U64 = np.float32, np.uint64
HAIR = F32(np.nextafter(F32(0), F32(1)))                                    # the smallest positive float
CAPS = (1, 100, 4096)
G_TEMPLATES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097)
N_QS = (1, 2, R - 1, R, R + 1, 65)
S_SUBJECTS = (1, 64, 65, 1025)
G_TINY = 10250                                                              # 1025 cards of ten
SPECIAL = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x3fc00000, 0xbf800000, 0x40500000], np.uint32).view(np.float32)   # +-inf, +-0, +-NaN, 1.5, -1, 3.25: never 0xffffffff
KINDS = ("search-like", "zeros", "special")
ALL = U64(0xffffffffffffffff)


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


def template_key(x):
    """rank_key (csrc/rank_order.h): the ordered bits of score + 0.0f."""
    return ordered((np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32))


def subject_key(x):
    return ordered(np.asarray(x, np.float32).view(np.uint32))


def label_test(labels, masks, n_q):
    """labels [n] of the matrix's columns, masks [n_q][3] or None -> [n_q][n] bool."""
    if masks is None:
        return np.ones((n_q, len(labels)), bool)
    mk = np.asarray(masks, U64).reshape(n_q, 3)
    L = np.asarray(labels, U64)[None, :]
    any_of, all_of, none_of = mk[:, 0:1], mk[:, 1:2], mk[:, 2:3]
    return ((any_of == 0) | ((L & any_of) != 0)) & ((L & all_of) == all_of) & ((L & none_of) == 0)


def not_listed(names, excl, n_q):
    """names [n] of the columns (global indices, or subject ids), excl: None or per query a sequence -> [n_q][n] bool."""
    out = np.ones((n_q, len(names)), bool)
    if excl is not None:
        for q in range(n_q):
            out[q] = ~np.isin(names, np.asarray(excl[q], np.int64))
    return out


class TemplateModel:
    """One matrix and one filter: per row the ELIGIBLE positions in rank-list order and their keys."""

    def __init__(self, scores, glob, ok):
        self.words = np.ascontiguousarray(scores).view(np.uint32); self.glob = np.asarray(glob, np.int64)
        self.order, self.neg_key = [], []
        for q in range(scores.shape[0]):
            at = np.flatnonzero(ok[q])
            key = template_key(scores[q, at]).astype(np.int64)
            o = np.lexsort((self.glob[at], -key))                           # key descending, global index ascending
            self.order.append(at[o]); self.neg_key.append(-key[o])

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
    def __init__(self, scores, glob, subject, ok):
        """scores [n_q][n] over the columns the search covered, glob [n] their global indices, subject [n] their persons, ok [n_q][n] the eligible cells (the excluded
        persons' cells taken out by the caller)."""
        words = np.ascontiguousarray(scores).view(np.uint32); glob = np.asarray(glob, np.int64); subject = np.asarray(subject, np.int64)
        self.rows = []
        for q in range(scores.shape[0]):
            at = np.flatnonzero(ok[q])
            key = subject_key(scores[q, at]).astype(np.int64)
            o = np.lexsort((glob[at], -key, subject[at]))                   # by subject; inside one the greatest key first, equal keys by ascending index
            first = np.ones(len(o), bool); first[1:] = subject[at][o][1:] != subject[at][o][:-1]
            best = o[first]
            rank = best[np.lexsort((subject[at][best], -key[best]))]        # key descending, subject id ascending
            self.rows.append((-key[rank], subject[at][rank], words[q, at[rank]], glob[at[rank]]))

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
    return {k: (v.view(np.uint32) if k == "score" and v.dtype != np.uint32 else v) for k, v in r.items() if v is not None}


def assert_same(got, want, what=""):
    got = as_words(got); want = as_words(want)
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].tolist(), got[key].ravel()[:8].tolist(), want[key].ravel()[:8].tolist())


def thresholds(rows):
    finite = np.unique(rows[np.isfinite(rows)])
    inside = finite[len(finite) // 2] if len(finite) else F32(1.5)           # a value inside the data
    return (F32(-np.inf), F32(0.0), HAIR, F32(inside))


# ---- matrices, labels, masks and exclusions -------------------------------------------------------------------------------------------------------------
def matrix(kind, n_q, G, rng):
    if kind == "search-like":                                               # about 99 % zeros, a few positives; a latent-empty row and an empty entry's column of -1
        u = rng.random((n_q, G))
        m = np.where(u < 0.004, -1.0, np.where(u < 0.012, rng.random((n_q, G)) * 5 + 0.01, 0.0)).astype(np.float32)
        if n_q > 1:
            m[n_q // 2] = -1.0
        m[:, G // 2] = -1.0
        return m
    if kind == "zeros":
        return np.zeros((n_q, G), np.float32)
    m = SPECIAL[rng.integers(0, len(SPECIAL), (n_q, G))]
    assert not (m.view(np.uint32) == 0xffffffff).any()
    return m


def make_labels(kind, G, rng):
    if kind == "cards":                                                     # ten one-hot finger bits, two for sex, a region code above; a card's prints share sex and region
        card = np.arange(G) // 10
        sex = rng.integers(0, 2, card.max() + 1)[card]; region = rng.integers(0, 6, card.max() + 1)[card]
        return (U64(1) << (np.arange(G) % 10).astype(U64)) | (U64(1) << (10 + sex).astype(U64)) | (region.astype(U64) << U64(12))
    lab = rng.integers(0, 1 << 63, G, dtype=np.int64).astype(U64) << U64(1) | rng.integers(0, 2, G).astype(U64)   # all 64 bits random
    lab &= rng.integers(0, 1 << 63, G, dtype=np.int64).astype(U64) << U64(1) | U64(1)                             # (thinned: a few bits set is the usual label)
    for j, v in enumerate((U64(0), ALL, U64(1) << U64(63), U64(1))):      # 0, all ones and bit 63 alone are always among them
        lab[(j * 7 + 1) % G] = v
    return lab


def mask_plan(label_kind, n_q, rot, rng):
    """One filter per row, the variants in turn from `rot` on: all zero, each of the three alone, combined, a row nothing passes, a row everything passes."""
    if label_kind == "cards":
        fingers = lambda allowed: U64(0x3ff) & ~U64(sum(1 << f for f in allowed))
        variants = [(0, 0, 0), (U64(0x3 << 12), 0, 0), (0, U64(1 << 11), 0), (0, 0, fingers({2, 7}) | U64(1 << 10)), (U64(0x21f), U64(1 << 10), U64(3 << 13)),
                    (0, U64(1) << U64(40), 0), (ALL, 0, U64(1) << U64(50))]
    else:
        a, b, c = (U64(int(x)) << U64(1) | U64(1) for x in rng.integers(0, 1 << 62, 3, dtype=np.int64))
        bit = lambda i: U64(1) << U64(i)
        variants = [(0, 0, 0), (a, 0, 0), (0, bit(63) | bit(3), 0), (0, 0, b & c), (a, bit(int(rng.integers(0, 64))), bit(63) | bit(int(rng.integers(0, 64)))),
                    (0, ALL, ALL), (0, 0, 0)]                               # all_of = none_of = all ones: no label passes both; all zero: every label passes
    out = np.zeros((n_q, 3), U64)
    for q in range(n_q):
        out[q] = np.array([U64(x) for x in variants[(q + rot) % len(variants)]], U64)
    return out


def excl_plan(rows, names, ok, n_q, rot, rng, key_of, outside, per_name=False):
    """One exclusion list per row, the variants in turn from `rot` on: none; the row's current best; everything that qualifies (at 0.0); names the search did not cover
    (`outside`) with the best among them; duplicates.  names [n]: the columns' global indices — or their subject ids (per_name: the best is a person's)."""
    out = []
    for q in range(n_q):
        at = np.flatnonzero(ok[q])
        key = key_of(rows[q, at]).astype(np.int64)
        best = [int(names[at[np.lexsort((names[at], -key))[0]]])] if len(at) else []
        v = (q + rot) % 5
        if v == 0: out.append([])
        elif v == 1: out.append(best)
        elif v == 2: out.append(np.unique(names[at[key >= int(key_of(np.zeros(1, F32))[0])]]).tolist())
        elif v == 3: out.append(list(outside[:2]) + best + list(outside[2:]))
        else:
            pick = names[rng.integers(0, len(names), 3)].tolist()
            out.append([pick[0], pick[0], pick[1], pick[0], pick[2], pick[1]])
    return out


def outside_templates(G):
    return [BASE - 1, 0, BASE + G, BASE + G + 5, 1 << 40, BASE - 1000 if BASE >= 1000 else 0]


def filters(label_kind, labels_cols, rows, glob, n_q, rot, rng, outside):
    """Three filters over one matrix: masks and exclusions, masks alone, exclusions alone -> (masks, excl, ok [n_q][n])."""
    mk = mask_plan(label_kind, n_q, rot, rng)
    lt = label_test(labels_cols, mk, n_q)
    ex = excl_plan(rows, glob, lt, n_q, rot + 1, rng, template_key, outside)
    ex_alone = excl_plan(rows, glob, np.ones_like(lt), n_q, rot + 2, rng, template_key, outside)
    return [(mk, ex, lt & not_listed(glob, ex, n_q)), (mk, None, lt), (None, ex_alone, not_listed(glob, ex_alone, n_q))]


# ---- 1: the model, templates ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", G_TEMPLATES)
def test_template_sweep(G, codebook_bytes, tiny):
    """Every n_q x matrix kind, label kinds in turn, three filters each, every cap x threshold.  The tap uploads a matrix once; it stays rankable through every call."""
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    glob = BASE + np.arange(G)
    handles = {}
    for kind in ("cards", "random"):
        lab = make_labels(kind, G, rng)
        handles[kind] = (lab, m.labels_create(lab))
    launched = 0
    for a, n_q in enumerate(N_QS):
        for b, kind in enumerate(KINDS):
            rows = matrix(kind, n_q, G, rng)
            m.debug_rank_hits(None, rows, float("-inf"), 1)
            label_kind = ("cards", "random")[(a + b) % 2]
            lab, h = handles[label_kind]
            plain = TemplateModel(rows, glob, np.ones(rows.shape, bool))
            for i, t in enumerate(thresholds(rows)):                        # no masks, no exclusions: the unfiltered call, word for word — with and without a handle
                cap = CAPS[(i + a + b) % len(CAPS)]
                old = m.rank_hits(float(t), cap)
                assert_same(old, plain.hits(t, cap), (G, n_q, kind, "afis_rank_hits"))
                assert_same(m.rank_hits_filtered(float(t), cap), old, (G, n_q, kind, "no filter"))
                assert_same(m.rank_hits_filtered(float(t), cap, labels=h, excl=[[]] * n_q), old, (G, n_q, kind, "a handle, no masks, empty lists"))
            for f, (mk, ex, ok) in enumerate(filters(label_kind, lab, rows, glob, n_q, a + 2 * b, rng, outside_templates(G))):
                model = TemplateModel(rows, glob, ok)
                for t in thresholds(rows):
                    for cap in CAPS:
                        assert_same(m.rank_hits_filtered(float(t), cap, labels=h if mk is not None else None, masks=mk, excl=ex), model.hits(t, cap), (G, n_q, kind, label_kind, f, float(t), cap))
                launched += 1
                us, fus = m.get_option("rank_filtered_us"), m.get_option("filter_us")
                assert us > 0 and us >= fus >= 0
            assert_same(m.rank_hits(float("-inf"), 100), plain.hits(F32(-np.inf), 100), (G, n_q, kind, "the matrix after the filtered calls"))
    assert launched == 3 * len(N_QS) * len(KINDS)
    for _, h in handles.values():
        m.labels_free(h)
    m.close()


# ---- 2: the model, subjects -----------------------------------------------------------------------------------------------------------------------------
def subject_plan(n_subjects, kind, rng):
    """-> the person of every template.  cards: contiguous cards of ten; random: 3 S + 1 templates dealt at random (every subject present); half: one subject holds
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


def subject_filters(label_kind, labels_cols, rows, subject_cols, n_q, rot, rng):
    """As filters(), the exclusions being subject ids: an excluded person's cells are no entries for that query."""
    outside = [int(subject_cols.max()) + 1, 1 << 50, int(subject_cols.max()) + 7, 0 if 0 not in subject_cols else (1 << 51)]
    mk = mask_plan(label_kind, n_q, rot, rng)
    lt = label_test(labels_cols, mk, n_q)
    ex = excl_plan(rows, subject_cols, lt, n_q, rot + 1, rng, subject_key, outside)
    ex_alone = excl_plan(rows, subject_cols, np.ones_like(lt), n_q, rot + 2, rng, subject_key, outside)
    return [(mk, ex, lt & not_listed(subject_cols, ex, n_q)), (mk, None, lt), (None, ex_alone, not_listed(subject_cols, ex_alone, n_q))]


@pytest.mark.parametrize("kind", ["cards", "random", "half"])
@pytest.mark.parametrize("n_subjects", S_SUBJECTS)
def test_subject_sweep(n_subjects, kind, codebook_bytes, tiny):
    rng = np.random.default_rng(SEED + 11 * n_subjects + len(kind))
    subject = subject_plan(n_subjects, kind, rng)
    G = len(subject)
    assert len(np.unique(subject)) == n_subjects and G <= G_TINY
    m = tap_matcher(codebook_bytes, tiny, G)
    hj = m.subjects_create(subject)
    glob = BASE + np.arange(G)
    handles = {}
    for lk in ("cards", "random"):
        lab = make_labels(lk, G, rng)
        handles[lk] = (lab, m.labels_create(lab))
    dropped_by_labels = 0
    for a, n_q in enumerate(N_QS):
        mk_kind = KINDS[a % len(KINDS)]
        rows = matrix(mk_kind, n_q, G, rng)
        m.debug_rank_hits(None, rows, float("-inf"), 1)
        label_kind = ("cards", "random")[a % 2]
        lab, h = handles[label_kind]
        plain = SubjectModel(rows, glob, subject, np.ones(rows.shape, bool))
        for i, t in enumerate(thresholds(rows)):
            cap = CAPS[(i + a) % len(CAPS)]
            old = m.rank_subject_hits(hj, float(t), cap)
            assert_same(old, plain.hits(t, cap), (n_subjects, kind, n_q, "afis_rank_subject_hits"))
            assert_same(m.rank_subject_hits_filtered(hj, float(t), cap), old, (n_subjects, kind, n_q, "no filter"))
        for f, (mk, ex, ok) in enumerate(subject_filters(label_kind, lab, rows, subject, n_q, a, rng)):
            model = SubjectModel(rows, glob, subject, ok)
            if ex is None:                                                  # persons all of whose templates fail the label test
                dropped_by_labels += sum(len(np.unique(subject)) - len(np.unique(subject[ok[q]])) for q in range(n_q))
            for t in thresholds(rows):
                for cap in CAPS:
                    assert_same(m.rank_subject_hits_filtered(hj, float(t), cap, labels=h if mk is not None else None, masks=mk, excl=ex), model.hits(t, cap),
                                (n_subjects, kind, n_q, mk_kind, label_kind, f, float(t), cap))
            us, fus = m.get_option("rank_filtered_us"), m.get_option("filter_us")
            assert us > 0 and us >= fus >= 0
        assert_same(m.rank_subject_hits(hj, float("-inf"), 100), plain.hits(F32(-np.inf), 100), (n_subjects, kind, n_q, "the matrix after the filtered calls"))
    assert dropped_by_labels > 0
    for _, h in handles.values():
        m.labels_free(h)
    m.subjects_free(hj)
    m.close()


# ---- 3: subsets ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_listed", [63, 64])
def test_subsets(n_listed, codebook_bytes, tiny):
    """A subset listed out of order (63 columns: odd rows; 64: four columns a thread): the label of a column is its listed template's, exclusions are global indices —
    those the subset does not list are ignored — and the lists carry global indices."""
    G = 600
    rng = np.random.default_rng(SEED + n_listed)
    m = tap_matcher(codebook_bytes, tiny, G)
    cards = np.arange(G, dtype=np.int64) // 10 * 3 + 50
    listed = [int(g) for g in rng.permutation(np.r_[120:130, 300, 301, 305, rng.permutation(np.r_[0:120, 130:300, 310:600])[:n_listed - 13]])]   # card 12 whole, card 30 in part
    assert listed != sorted(listed) and len(set(listed)) == n_listed
    hs = m.subset_create([BASE + g for g in listed])
    hj = m.subjects_create(cards)
    held = np.sort(np.asarray(listed))                                      # the device holds the listed templates in ascending global order
    unlisted = np.setdiff1d(np.arange(G), held)
    outside = [int(BASE + unlisted[0]), int(BASE + unlisted[5]), BASE + G, int(BASE + unlisted[-1]), BASE - 1]   # in the shard but not in the subset; beyond it; below it
    for a, n_q in enumerate((2, R + 1)):
        for b, kind in enumerate(KINDS):
            label_kind = ("cards", "random")[(a + b) % 2]
            lab = make_labels(label_kind, G, rng)
            h = m.labels_create(lab)                                        # (leaves the matrix alone; here there is none yet, or the previous round's)
            rows = matrix(kind, n_q, n_listed, rng)
            m.debug_rank_rows(rows, 1, subset=hs)
            old = m.rank_hits(float("-inf"), 100)
            assert_same(m.rank_hits_filtered(float("-inf"), 100), old, "no filter")
            assert_same(m.rank_hits_filtered(float("-inf"), 100, excl=[[outside[0], outside[3]]] * n_q), old, "only templates the subset does not list")
            for f, (mk, ex, ok) in enumerate(filters(label_kind, lab[held], rows, BASE + held, n_q, a + b, rng, outside)):
                tm = TemplateModel(rows, BASE + held, ok)
                for t in thresholds(rows):
                    for cap in (1, n_listed, 100):
                        got = m.rank_hits_filtered(float(t), cap, labels=h if mk is not None else None, masks=mk, excl=ex)
                        assert_same(got, tm.hits(t, cap), ("subset", n_q, kind, f, float(t), cap))
                        assert np.isin(got["idx"][got["idx"] >= 0], BASE + held).all()
            for f, (mk, ex, ok) in enumerate(subject_filters(label_kind, lab[held], rows, cards[held], n_q, a + b, rng)):
                sm = SubjectModel(rows, BASE + held, cards[held], ok)
                for t in thresholds(rows):
                    for cap in (1, n_listed, 100):
                        assert_same(m.rank_subject_hits_filtered(hj, float(t), cap, labels=h if mk is not None else None, masks=mk, excl=ex), sm.hits(t, cap),
                                    ("subset subjects", n_q, kind, f, float(t), cap))
            assert_same(m.rank_hits(float("-inf"), 100), old, "the matrix after the filtered calls")
            m.labels_free(h)                                                # (leaves the matrix alone too)
            assert_same(m.rank_hits(float("-inf"), 100), old, "after labels_free")
    m.subset_free(hs)
    with pytest.raises(M.AfisError, match=ESTATE):                          # the sub-shard the matrix refers to is gone
        m.rank_hits_filtered(0.0, 24)
    m.subjects_free(hj)
    m.close()


# ---- 4: the matrix is untouched --------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_is_untouched(codebook_bytes, tiny):
    """The siblings give the same outputs before and after filtered calls, and the second of two filtered calls with different filters does not see the first."""
    G, n_q = 1025, R + 1
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 3)
    rows = matrix("search-like", n_q, G, rng)
    glob = BASE + np.arange(G)
    cards = np.arange(G, dtype=np.int64) // 10 * 7 + 1
    hj = m.subjects_create(cards)
    lab = make_labels("cards", G, rng)
    h = m.labels_create(lab)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    case_of = np.arange(n_q) // 2
    siblings = lambda: (m.rank_hits(0.0, 100), m.rank_hits(float("-inf"), 4096), m.rank_subject_hits(hj, float(HAIR), 100), m.rank_subjects(hj, n_q, 24),
                        m.rank_case_hits(case_of, M.CASE_SUM, 0.0, 100), m.rank_case_subject_hits(hj, case_of, M.CASE_MAX, 0.0, 100), m.rank_latent_hits(0.0, 4))
    before = siblings()
    nothing = np.tile(np.array([0, 1 << 40, 0], U64), (n_q, 1))             # a filter nothing passes, and every template excluded on top
    got = m.rank_hits_filtered(float("-inf"), 100, labels=h, masks=nothing, excl=[glob.tolist()] * n_q)
    assert (got["n_hits"] == 0).all() and (got["idx"] == -1).all() and np.isneginf(got["score"]).all()
    got = m.rank_subject_hits_filtered(hj, float("-inf"), 100, labels=h, masks=nothing, excl=[np.unique(cards).tolist()] * n_q)
    assert (got["n_hits"] == 0).all() and (got["subject"] == -1).all() and (got["best_idx"] == -1).all() and np.isneginf(got["score"]).all()
    fa, fb = filters("cards", lab, rows, glob, n_q, 1, rng, outside_templates(G))[0], filters("cards", lab, rows, glob, n_q, 4, rng, outside_templates(G))[0]
    assert not np.array_equal(fa[2], fb[2])
    for mk, ex, ok in (fa, fb, fa):
        assert_same(m.rank_hits_filtered(0.0, 100, labels=h, masks=mk, excl=ex), TemplateModel(rows, glob, ok).hits(F32(0), 100), "one filter after another")
    sa, sb = subject_filters("cards", lab, rows, cards, n_q, 2, rng)[0], subject_filters("cards", lab, rows, cards, n_q, 5, rng)[0]
    for mk, ex, ok in (sa, sb, sa):
        assert_same(m.rank_subject_hits_filtered(hj, 0.0, 100, labels=h, masks=mk, excl=ex), SubjectModel(rows, glob, cards, ok).hits(F32(0), 100), "one subject filter after another")
    for b, f in zip(before, siblings()):
        assert_same(f, as_words(b), "the siblings on the same matrix")
    m.labels_free(h); m.subjects_free(hj)
    m.close()


# ---- 5: a real search ------------------------------------------------------------------------------------------------------------------------------------
def test_a_real_search(codebook_bytes, cb):
    """Three latents x 48 templates with planted mates: per query, the filtered rank list equals the rank list of a subset search over exactly that query's eligible
    templates — the route open before, one subset and one search per filter — indices and score bits."""
    G = 48
    lats = S.make_latents(83, 3, n_tex_lo=400, n_tex_hi=600)
    gal = S.make_packed_gallery(83, G, cb)
    S.plant_mates(83, gal, cb, lats)
    rng = np.random.default_rng(SEED + 5)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal); m.gallery_commit(BASE)
    lab = make_labels("cards", G, rng)
    h = m.labels_create(lab)
    r = m.search(lats, k=24, want_scores=True)
    scores = r["scores"]
    assert (scores > 0).any(axis=1).all()
    glob = BASE + np.arange(G)
    fingers = lambda allowed: U64(0x3ff) & ~U64(sum(1 << f for f in allowed))
    masks = np.array([[0, 0, fingers({0, 1, 2, 3, 7})], [U64(0x70), 0, 0], [0, 0, 0]], U64)   # five fingers allowed; any of three fingers; no label test
    best = [int(glob[np.argmax(scores[q])]) for q in range(3)]
    excl = [[best[0], BASE + 40, 5], [], [best[2], best[2], BASE + 1, BASE + G]]
    ok = label_test(lab, masks, 3) & not_listed(glob, excl, 3)
    assert all(3 < ok[q].sum() < G for q in range(3)) and not ok[0, best[0] - BASE]
    got = m.rank_hits_filtered(float("-inf"), G, labels=h, masks=masks, excl=excl)
    assert_same(got, TemplateModel(scores, glob, ok).hits(F32(-np.inf), G), "against the model")
    assert_same(m.rank_hits(float("-inf"), 24), {"n_hits": np.full(3, G), "idx": r["topk_idx"], "score": r["topk_score"]}, "the search's own list afterwards")
    for q in range(3):
        eligible = glob[ok[q]]
        hs = m.subset_create(rng.permutation(eligible).tolist())
        m.search_subset(hs, [lats[q]], k=24, want_scores=False)
        want = m.rank_hits(float("-inf"), G)
        assert want["n_hits"][0] == len(eligible) == got["n_hits"][q]
        assert np.array_equal(got["idx"][q], want["idx"][0]) and np.array_equal(got["score"][q].view(np.uint32), want["score"][0].view(np.uint32)), q
        m.subset_free(hs)
    m.labels_free(h)
    m.close()


# ---- 6: the refusals, the options, the live gallery --------------------------------------------------------------------------------------------------------
def test_errors_states_and_options(codebook_bytes, tiny):
    i64p, u64p, fp = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    G, n_q = 150, 4
    rng = np.random.default_rng(SEED + 6)
    tens = np.arange(G, dtype=np.int64) // 10
    lab = make_labels("cards", G, rng)
    m = M.Matcher(codebook_bytes, taps=True)
    lc, lf = m.lib.afis_labels_create, m.lib.afis_labels_free
    out = C.c_void_p()
    plab = lab.ctypes.data_as(u64p)
    m.gallery_add_packed(tiny.slice(0, G))
    assert lc(m.ctx, plab, G, C.byref(out)) == -3 and not out.value         # before the first commit
    m.gallery_commit(BASE)
    h2d = m.get_option("gallery_h2d_bytes")
    for bad_n in (G - 1, G + 1, 0, -1):
        assert lc(m.ctx, plab, bad_n, C.byref(out)) == -1 and not out.value
    assert lc(m.ctx, None, G, C.byref(out)) == -1 and lc(m.ctx, plab, G, None) == -1
    assert m.get_option("gallery_h2d_bytes") == h2d                         # a refused call uploads nothing
    ha = m.subjects_create(tens)
    h2d = m.get_option("gallery_h2d_bytes")
    hl = m.labels_create(lab)
    assert m.get_option("gallery_h2d_bytes") == h2d + G * 8
    h2 = m.labels_create(np.zeros(G, U64))                                  # several handles live at once
    nh = np.zeros(n_q, np.int64); a = np.zeros((n_q, 24), np.int64); sc = np.zeros((n_q, 24), np.float32); b = np.zeros((n_q, 24), np.int64)
    pn, pa, ps, pb = nh.ctypes.data_as(i64p), a.ctypes.data_as(i64p), sc.ctypes.data_as(fp), b.ctypes.data_as(i64p)
    mk = mask_plan("cards", n_q, 1, rng)
    off = np.array([0, 1, 1, 3, 4], np.int64); ent = np.array([BASE + 3, BASE + 9, BASE + 9, BASE + G + 4], np.int64)
    pm, po, pe = mk.ctypes.data_as(u64p), off.ctypes.data_as(i64p), ent.ctypes.data_as(i64p)
    rt = lambda *x: m.lib.afis_rank_hits_filtered(m.ctx, *x)
    rs = lambda *x: m.lib.afis_rank_subject_hits_filtered(m.ctx, ha[0], *x)
    both = ((rt, (pn, pa, ps)), (rs, (pn, pa, ps, pb)))
    for f, outs in both:
        assert f(hl[0], pm, po, pe, n_q, 0.0, 24, *outs) == -3              # before any search
    assert m.get_option("rank_filtered_us") == 0 and m.get_option("filter_us") == 0
    rows = matrix("search-like", n_q, G, rng)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    glob = BASE + np.arange(G)
    hb = m.labels_create(lab); m.labels_free(hb)                            # create and free leave the matrix rankable; the freed handle is refused below
    bad_offs = [np.array(x, np.int64) for x in ([1, 1, 1, 3, 4], [0, 2, 1, 3, 4], [0, 1, 1, 3, 2])]
    neg = np.array([BASE + 3, -1, BASE + 9, 7], np.int64)
    for f, outs in both:
        assert f(None, pm, po, pe, n_q, 0.0, 24, *outs) == -1               # masks without labels
        assert f(hb[0], pm, po, pe, n_q, 0.0, 24, *outs) == -1              # a freed handle ...
        assert f(hb[0], None, None, None, n_q, 0.0, 24, *outs) == -1        # ... also where it would not be read
        assert f(ha[0], pm, po, pe, n_q, 0.0, 24, *outs) == -1              # a subject handle is no labels handle
        for bo in bad_offs:
            assert f(hl[0], pm, bo.ctypes.data_as(i64p), pe, n_q, 0.0, 24, *outs) == -1
        assert f(hl[0], pm, po, neg.ctypes.data_as(i64p), n_q, 0.0, 24, *outs) == -1
        assert f(hl[0], pm, po, None, n_q, 0.0, 24, *outs) == -1            # offsets that list entries, no entries
        for bad_q in (3, 5, -1):
            assert f(hl[0], pm, None, None, bad_q, 0.0, 24, *outs) == -1
        for cap in (0, -1, 4097):
            assert f(hl[0], pm, po, pe, n_q, 0.0, cap, *outs) == -1
        assert f(hl[0], pm, po, pe, n_q, float("nan"), 24, *outs) == -1
        for k in range(len(outs)):
            assert f(hl[0], pm, po, pe, n_q, 0.0, 24, *[None if j == k else o for j, o in enumerate(outs)]) == -1
    assert m.lib.afis_rank_subject_hits_filtered(m.ctx, None, hl[0], pm, po, pe, n_q, 0.0, 24, pn, pa, ps, pb) == -1
    assert m.lib.afis_rank_subject_hits_filtered(m.ctx, hl[0], hl[0], pm, po, pe, n_q, 0.0, 24, pn, pa, ps, pb) == -1   # a labels handle is no subject handle
    other = tap_matcher(codebook_bytes, tiny, G)
    ho = other.labels_create(lab)
    assert rt(ho[0], pm, po, pe, n_q, 0.0, 24, pn, pa, ps) == -1            # live, but in another context
    other.close()                                                           # (afis_destroy releases the handle that is left)
    # the refused calls left the matrix rankable; through the C ABI
    ex = [ent[off[q]:off[q + 1]].tolist() for q in range(n_q)]
    ok = label_test(lab, mk, n_q)
    assert rt(hl[0], pm, po, pe, n_q, 0.0, 24, pn, pa, ps) == 0
    assert_same({"n_hits": nh, "idx": a, "score": sc}, TemplateModel(rows, glob, ok & not_listed(glob, ex, n_q)).hits(F32(0), 24), "through the C ABI")
    us, fus = m.get_option("rank_filtered_us"), m.get_option("filter_us")
    assert us > 0 and us >= fus >= 0
    sent = np.array([0, 14, 14, 10 ** 9], np.int64)
    assert rs(hl[0], pm, po, sent.ctypes.data_as(i64p), n_q, 0.0, 24, pn, pa, ps, pb) == 0
    sx = [sent[off[q]:off[q + 1]].tolist() for q in range(n_q)]
    assert_same({"n_hits": nh, "subject": a, "score": sc, "best_idx": b}, SubjectModel(rows, glob, tens, ok & not_listed(tens, sx, n_q)).hits(F32(0), 24), "subjects through the C ABI")
    assert m.get_option("rank_filtered_us") >= m.get_option("filter_us") >= 0 and m.get_option("rank_filtered_us") > 0
    assert rt(None, None, None, None, n_q, 0.0, 24, pn, pa, ps) == 0 and m.get_option("rank_filtered_us") > 0 and m.get_option("filter_us") >= 0   # no filter still launches k_rank_hits
    assert_same(m.rank_hits_filtered(0.0, 24, labels=h2, masks=np.zeros((n_q, 3), U64)), m.rank_hits(0.0, 24), "labels of zero against masks of zero")
    # calls that queue nothing: an empty subset, a search of no queries
    lats = S.make_latents(83, n_q, n_tex_lo=400, n_tex_hi=500)
    he = m.subset_create([])
    qr = m.upload_queries(lats, reserve=8)
    m.search_subset_resident(he, qr, k=0)
    for got in (m.rank_hits_filtered(float("-inf"), 5, labels=hl, masks=mk, excl=ex), m.rank_subject_hits_filtered(ha, float("-inf"), 5, labels=hl, masks=mk, excl=sx)):
        assert (got["n_hits"] == 0).all() and np.isneginf(got["score"]).all() and (got.get("idx", got.get("subject")) == -1).all()
        assert m.get_option("rank_filtered_us") == 0 and m.get_option("filter_us") == 0
    m.subset_free(he); m.free_queries(qr)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    assert rt(hl[0], pm, po, pe, n_q, 0.0, 24, pn, pa, ps) == 0 and m.get_option("rank_filtered_us") > 0
    q0 = m.upload_queries([], reserve=G)
    for f, outs in both:
        assert f(hl[0], pm, po, pe, n_q, 0.0, 24, *outs) == -3              # a call that queued device work took the matrix away
    m.search_resident(q0, k=0)
    z = m.rank_hits_filtered(0.0, 5, labels=hl, masks=np.zeros((0, 3), U64), excl=[])
    assert z["n_hits"].shape == (0,) and z["idx"].shape == (0, 5) and m.get_option("rank_filtered_us") == 0 and m.get_option("filter_us") == 0
    m.free_queries(q0)
    # the live gallery: a removal that changed the shard, then an appending commit
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    m.gallery_remove([BASE + 47])
    for f, outs in both:
        assert f(hl[0], pm, po, pe, n_q, 0.0, 24, *outs) == -3              # no matrix
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    assert rt(hl[0], pm, po, pe, n_q, 0.0, 24, pn, pa, ps) == -3            # a matrix, but the labels belong to the older gallery
    assert rt(hl[0], None, None, None, n_q, 0.0, 24, pn, pa, ps) == -3      # ... also where they would not be read
    assert "free the handle and create it again" in m.lib.afis_last_error(m.ctx).decode()
    assert rt(None, None, po, pe, n_q, 0.0, 24, pn, pa, ps) == 0            # without them the call works, and the refusals left the matrix rankable
    m.labels_free(hl); m.labels_free(h2)                                    # free still works
    assert rt(hl[0], pm, po, pe, n_q, 0.0, 24, pn, pa, ps) == -1            # freed: no longer a live handle
    hn = m.labels_create(lab)
    assert_same(m.rank_hits_filtered(0.0, 24, labels=hn, masks=mk, excl=ex), TemplateModel(rows, glob, ok & not_listed(glob, ex, n_q)).hits(F32(0), 24), "a new handle after the removal")
    m.gallery_reopen(); m.gallery_add_packed(tiny.slice(G, G + 6)); m.gallery_commit(BASE)
    rows2 = matrix("search-like", n_q, G + 6, rng)
    m.debug_rank_hits(None, rows2, float("-inf"), 1)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_hits_filtered(0.0, 24, labels=hn, masks=mk)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.labels_create(lab)                                                # the shard holds G + 6 templates now
    lab2 = make_labels("cards", G + 6, rng)
    hm = m.labels_create(lab2)
    glob2 = BASE + np.arange(G + 6)
    assert_same(m.rank_hits_filtered(0.0, 24, labels=hm, masks=mk, excl=ex), TemplateModel(rows2, glob2, label_test(lab2, mk, n_q) & not_listed(glob2, ex, n_q)).hits(F32(0), 24), "after the append")
    m.labels_free(hn)
    m.subjects_free(ha)
    m.close()                                                               # hm is still live: afis_destroy releases it
