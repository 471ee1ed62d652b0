"""Filtered case lists and filtered reverse lists on the GPU: afis_rank_case_hits_filtered / afis_rank_case_subject_hits_filtered / afis_rank_latent_hits_filtered.

The yardstick is numpy, compared bit for bit: score words as uint32, n_hits, every entry and every padding entry (-1, -inf).  A cell (query, column) is ELIGIBLE when
the label of the column's template passes the query's masks ((any_of == 0 or L & any_of) and L & all_of == all_of and not L & none_of) and the template (its global
index), or its person (the subject id), is not on the query's exclusion list.
  case lists     for (case, column) the members E that are eligible for the column, in ascending query position, are folded by a Python loop on whole rows: SUM is
                 acc = (acc + row).astype(float32) from +0.0 over the members of E that take part (template_key(v) >= template_key(+0.0)), -1 where E is not empty and
                 none does; MAX the value of greatest key, first member's bits.  E empty is NO ENTRY: the column is not in the case's list at all.  For subjects a
                 member's value is the maximum on the raw word's order over the person's templates that are eligible for that member; the member is in E when there
                 is one and the person is not on the member's exclusion list.  The entries are listed on template_key descending, name ascending
  reverse lists  per column the eligible queries on template_key descending, query position ascending, named latent_base + position
Matrices are planted with the existing taps: debug_rank_hits (a full search's) and debug_rank_rows(subset=...).

Shapes: the folds and k_filter_rows take four columns per thread where G % 4 == 0 and one otherwise, 256 threads a workgroup, the filter strips of R = 8 query rows;
the transpose works in 64 x 64 tiles: G sits on, before and after the wave (64), the workgroup (256), 1024 and 4096, with odd and even rows; n_q around the strip;
cases of one, four, five and every query cross the fold loop's unroll of four.  The sweeps take every n_q x matrix kind x filter x mode and walk the layouts, caps
and thresholds in turn, so that one test stays at about a second and the parametrised family covers the product."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 6173
BASE = 1000
R = 8                                                                       # csrc/afis_device.h: kFilterRows
ESTATE, EINVAL = "afis error -3", "afis error -1"
NEG_INF = np.float32(-np.inf).view(np.uint32)
NO_ENTRY = np.uint32(0xffffffff)
F32, U64, U32 = np.float32, np.uint64, np.uint32
HAIR = F32(np.nextafter(F32(0), F32(1)))                                    # the smallest positive float
SUM, MAX = M.CASE_SUM, M.CASE_MAX
MODES = (SUM, MAX)
CAPS = (1, 100, 4096)
G_TEMPLATES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)
N_QS = (1, 2, R - 1, R, R + 1, 65)
S_SUBJECTS = (1, 64, 65, 1025)
G_TINY = 4097
SPECIAL = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x3fc00000, 0xbf800000, 0x40500000], np.uint32).view(np.float32)   # +-inf, +-0, +-NaN, 1.5, -1, 3.25: never 0xffffffff
KINDS = ("search-like", "zeros", "special")
ALL = U64(0xffffffffffffffff)
NOTHING = (U64(0), ALL, ALL)                                                # all_of = none_of = all ones: no label passes both
LAYOUTS = ("singles", "one", "interleaved", "five", "sparse")
FILTERS = ("all-pass", "member-none", "case-none", "disjoint", "random-tenth", "exclusions", "masks+exclusions", "names-nothing")


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """4097 rolled templates of one minutia and one texture point each (tests/test_gpu_filtered_hits.py's tap gallery), as one packed gallery."""
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
    w = np.asarray(words, U32)
    return np.where(w & U32(0x80000000), ~w, w | U32(0x80000000)).astype(U32)


def unordered(o):
    o = np.asarray(o, U32)
    return np.where(o & U32(0x80000000), o ^ U32(0x80000000), ~o).astype(U32)


def template_key(x):
    """rank_key (csrc/score_order.h): the ordered bits of score + 0.0f."""
    with np.errstate(all="ignore"):
        return ordered((np.asarray(x, F32) + F32(0.0)).view(U32))


ZERO_KEY = template_key(np.zeros(1, F32))[0]


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


def fuse_eligible(rows, ok, case_of, mode):
    """rows [n_q][n] floats, ok [n_q][n] the members' eligible cells -> (the distinct case ids ascending, fused words [n_cases][n], entry [n_cases][n] bool): the fold
    of the header over E, member by member on whole rows; entry is "E is not empty"."""
    case_of = np.asarray(case_of, np.int64)
    ids = np.unique(case_of)
    n = rows.shape[1]
    fused = np.full((len(ids), n), NO_ENTRY, U32); entry = np.zeros((len(ids), n), bool)
    with np.errstate(all="ignore"):
        for r, cid in enumerate(ids):
            seen = np.zeros(n, bool)
            if mode == SUM:
                acc = np.zeros(n, F32); took = np.zeros(n, bool)
                for i in np.flatnonzero(case_of == cid):                    # ascending query position
                    part = ok[i] & (template_key(rows[i]) >= ZERO_KEY)
                    acc = np.where(part, (acc + rows[i]).astype(F32), acc); took |= part; seen |= ok[i]
                val = np.where(took, acc, F32(-1.0)).astype(F32).view(U32)
            else:
                val = np.zeros(n, U32); key = np.zeros(n, U32); have = np.zeros(n, bool)
                for i in np.flatnonzero(case_of == cid):
                    k = template_key(rows[i])
                    take = ok[i] & (~have | (k > key))                      # strictly: the first member of the greatest key keeps its bits
                    val = np.where(take, rows[i].view(U32), val); key = np.where(take, k, key); have |= take; seen |= ok[i]
            fused[r] = np.where(seen, val, NO_ENTRY); entry[r] = seen
    return ids, fused, entry


def subject_best_eligible(rows, ok, subject):
    """rows [n_q][n], ok [n_q][n], subject [n] the columns' persons -> (the ids present ascending, best [n_q][S] floats, have [n_q][S]): per query and person the maximum
    on the raw word's order over the ELIGIBLE cells; have: there is one."""
    subject = np.asarray(subject, np.int64)
    sid, slot = np.unique(subject, return_inverse=True)
    o = np.argsort(slot, kind="stable")
    starts = np.flatnonzero(np.r_[True, slot[o][1:] != slot[o][:-1]])
    key = ordered(np.ascontiguousarray(rows).view(U32))
    assert (key[ok] > 0).all()                                              # (only 0xffffffff has the ordered word 0)
    key = np.where(ok, key, U32(0))[:, o]
    best = np.maximum.reduceat(key, starts, axis=1)
    return sid, unordered(best).view(F32), best > 0


class Lists:
    """words [rows][n] with entry [rows][n] and the entries' names: per row the rank-list order of its entries and their keys; a (min_score, cap) pair is one search."""

    def __init__(self, words, entry, names, what, head=None):
        self.words = words; self.names = np.asarray(names, np.int64); self.what = what; self.head = head or {}
        self.order, self.neg_key = [], []
        for r in range(words.shape[0]):
            at = np.flatnonzero(entry[r])
            key = template_key(words[r, at].view(F32)).astype(np.int64)
            o = np.lexsort((self.names[at], -key))                          # key descending, name ascending
            self.order.append(at[o]); self.neg_key.append(-key[o])

    def hits(self, min_score, cap):
        thr = int(template_key(np.array([min_score], F32))[0])
        n_r = len(self.order)
        n = np.empty(n_r, np.int64); a = np.full((n_r, cap), -1, np.int64); sc = np.full((n_r, cap), NEG_INF, U32)
        for r in range(n_r):
            n[r] = np.searchsorted(self.neg_key[r], -thr, side="right")     # keys >= thr: a prefix of the rank list
            take = self.order[r][:min(int(n[r]), cap)]
            a[r, :len(take)] = self.names[take]; sc[r, :len(take)] = self.words[r, take]
        return dict(self.head, **{"n_hits": n, self.what: a, "score": sc})


def case_template_model(rows, ok, case_of, mode, glob):
    ids, fused, entry = fuse_eligible(rows, ok, case_of, mode)
    return Lists(fused, entry, glob, "idx", {"case_id": ids}), fused, entry


def case_subject_model(rows, ok, subject, excl, case_of, mode):
    """ok: the label test's cells; excl: None or per query the excluded subject ids."""
    sid, best, have = subject_best_eligible(rows, ok, subject)
    ids, fused, entry = fuse_eligible(best, have & not_listed(sid, excl, rows.shape[0]), case_of, mode)
    return Lists(fused, entry, sid, "subject", {"case_id": ids}), fused, entry


def latent_model(rows, ok, latent_base):
    """The column lists: rows = the columns, entries = the queries."""
    return Lists(np.ascontiguousarray(rows.T).view(U32), np.ascontiguousarray(ok.T), latent_base + np.arange(rows.shape[0]), "latent")


def as_words(r):
    return {k: (v.view(U32) if k == "score" and v.dtype != U32 else v) for k, v in r.items() if v is not None}


def assert_same(got, want, what=""):
    got = as_words(got); want = as_words(want)
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].tolist(), got[key].ravel()[:8].tolist(), want[key].ravel()[:8].tolist())


def thresholds(words, entry):
    """-inf, -1, 0, the smallest positive, a value inside the positive entries."""
    v = words[entry].view(F32)
    pos = np.unique(v[np.isfinite(v) & (v > 0)])
    inside = pos[len(pos) // 2] if len(pos) else F32(1.5)
    return (F32(-np.inf), F32(-1.0), F32(0.0), HAIR, F32(inside))


# ---- matrices, labels, layouts and filters ------------------------------------------------------------------------------------------------------------
def matrix(kind, n_q, G, rng):
    if kind == "search-like":                                               # -1, a large tie at zero, tied positives; a latent-empty row and an empty entry's column of -1
        u = rng.random((n_q, G))
        m = np.where(u < 0.15, -1.0, np.where(u < 0.35, np.round(rng.random((n_q, G)) * 8) / 2 + 0.5, 0.0)).astype(F32)
        if n_q > 1:
            m[n_q // 2] = -1.0
        m[:, G // 2] = -1.0
        return m
    if kind == "zeros":
        return np.zeros((n_q, G), F32)
    m = SPECIAL[rng.integers(0, len(SPECIAL), (n_q, G))]
    assert not (m.view(U32) == NO_ENTRY).any()
    return m


def make_labels(G, rng):
    """bits 0 .. 9: one finger position, dealt at random; bits 10 .. 41: the column's class (position % 32), one-hot; bit 63: every seventh template."""
    j = np.arange(G)
    return (U64(1) << rng.integers(0, 10, G).astype(U64)) | (U64(1) << (10 + j % 32).astype(U64)) | np.where(j % 7 == 3, U64(1) << U64(63), U64(0))


def layout(kind, n_q, rng):
    """case_of [n_q].  singles: every query its own case; one: one case holds every query; interleaved: i % C; five: a case of five members (while there are five)
    dealt over the positions, the rest in pairs; sparse: up to four cases whose ids are far apart and DEscend with the position of a case's first member."""
    i = np.arange(n_q, dtype=np.int64)
    if kind == "singles":
        return 5 + 3 * i
    if kind == "one":
        return np.full(n_q, 9, np.int64)
    if kind == "interleaved":
        return i % min(n_q, (n_q + 3) // 4)                                 # cases of four members, the last ones shorter
    perm = rng.permutation(n_q)
    case = np.empty(n_q, np.int64)
    if kind == "five":
        case[perm[:5]] = 77
        case[perm[5:]] = 100 + np.arange(max(n_q - 5, 0)) // 2
        return case
    case[perm] = np.arange(n_q) % min(4, n_q)
    first = np.array([np.flatnonzero(case == c)[0] for c in range(min(4, n_q))])
    return (7 + (13 << 28) * (len(first) - 1 - np.argsort(np.argsort(first))))[case]   # past 2^31 from the second case on


def best_names(rows, names, q, k):
    key = template_key(rows[q]).astype(np.int64)
    return [int(x) for x in names[np.lexsort((names, -key))[:k]]]


def exclusions(rows, names, n_q, outside, rng):
    """One list per query, the variants in turn: none; the row's two best; duplicates; names the search did not cover around the best; every name reaching zero."""
    out = []
    for q in range(n_q):
        v = (q + int(rng.integers(0, 5))) % 5
        if v == 0: out.append([])
        elif v == 1: out.append(best_names(rows, names, q, 2))
        elif v == 2:
            a, b, c = (int(x) for x in names[rng.integers(0, len(names), 3)])
            out.append([a, a, b, a, c, b])
        elif v == 3: out.append(list(outside[:2]) + best_names(rows, names, q, 1) + list(outside[2:]))
        else: out.append(np.unique(names[template_key(rows[q]) >= ZERO_KEY]).tolist())
    return out


def finger_masks(n_q, rng):
    """A random tenth: any_of one finger bit per query."""
    mk = np.zeros((n_q, 3), U64)
    mk[:, 0] = U64(1) << rng.integers(0, 10, n_q).astype(U64)
    return mk


def make_filter(kind, rows, labels_cols, names, case_of, outside, rng):
    """-> (masks or None, excl or None, ok [n_q][n]) over the matrix's columns."""
    n_q = rows.shape[0]
    ids, counts = np.unique(case_of, return_counts=True)
    big = ids[np.argmax(counts)]                                            # a case of the most members
    mk, ex = np.zeros((n_q, 3), U64), None
    if kind == "member-none":
        mk[np.flatnonzero(case_of == big)[-1]] = NOTHING                    # one member of a case with no eligible cell
    elif kind == "case-none":
        mk[case_of == big] = NOTHING                                        # every member: the whole row is no entry
    elif kind == "disjoint":                                                # member r of a case of k is eligible for the column classes c with c % min(k, 32) == r % min(k, 32)
        for cid, k in zip(ids, counts):
            for r, q in enumerate(np.flatnonzero(case_of == cid)):
                kk = min(int(k), 32)
                mk[q, 0] = U64(sum(1 << (10 + c) for c in range(32) if c % kk == r % kk))
    elif kind == "random-tenth":
        mk = finger_masks(n_q, rng)
    elif kind == "exclusions":
        mk, ex = None, exclusions(rows, names, n_q, outside, rng)
    elif kind == "masks+exclusions":
        mk, ex = finger_masks(n_q, rng), exclusions(rows, names, n_q, outside, rng)
        mk[:, 2] = U64(1) << U64(63)
    elif kind == "names-nothing":                                           # exclusions that name nothing the search covered, and duplicates of them
        mk, ex = None, [list(outside) + list(outside[:2]) for _ in range(n_q)]
    return mk, ex, label_test(labels_cols, mk, n_q) & not_listed(names, ex, n_q)


def outside_templates(G):
    return [BASE - 1, 0, BASE + G, BASE + G + 5, 1 << 40]


# ---- 1: the new state -------------------------------------------------------------------------------------------------------------------------------------
def test_no_entry_is_not_minus_one(codebook_bytes, tiny):
    """min_score = -inf under AFIS_CASE_SUM: a column whose eligible members all hold -1 is listed with -1.0f and counted; a column with no eligible member is absent
    and not counted.  Columns 0 .. 5 of two queries in one case; labels = the column's bit."""
    G = 6
    m = tap_matcher(codebook_bytes, tiny, G)
    h = m.labels_create(U64(1) << np.arange(G).astype(U64))
    rows = np.array([[-1, -1, 2, -1, 0, -1],
                     [-1, 3, -1, -1, -1, 5]], F32)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    #  column:  0 both eligible, both -1 -> -1   1 only query 0 eligible (-1) -> -1   2 only query 0 eligible -> 2   3 nobody -> absent   4 nobody -> absent
    #           5 only query 1 eligible -> 5
    mk = np.array([[0b000111, 0, 0], [0b100001, 0, 0]], U64)
    got = m.rank_case_hits_filtered([4, 4], SUM, float("-inf"), G, labels=h, masks=mk)
    assert got["case_id"].tolist() == [4] and got["n_hits"].tolist() == [4]
    assert got["idx"][0].tolist() == [BASE + 5, BASE + 2, BASE + 0, BASE + 1, -1, -1]
    assert got["score"][0].view(U32).tolist() == np.array([5, 2, -1, -1, -np.inf, -np.inf], F32).view(U32).tolist()
    assert m.rank_case_hits_filtered([4, 4], SUM, -1.0, G, labels=h, masks=mk)["n_hits"].tolist() == [4]      # -1 is an entry, listed when min_score <= -1
    assert m.rank_case_hits_filtered([4, 4], SUM, 0.0, G, labels=h, masks=mk)["n_hits"].tolist() == [2]
    got = m.rank_case_hits_filtered([4, 4], MAX, float("-inf"), G, labels=h, masks=mk)
    assert got["n_hits"].tolist() == [4] and got["idx"][0].tolist() == [BASE + 5, BASE + 2, BASE + 0, BASE + 1, -1, -1]
    plain = m.rank_case_hits([4, 4], SUM, float("-inf"), G)                  # the unfiltered call has no such state: six entries
    assert plain["n_hits"].tolist() == [6] and plain["score"][0].tolist() == [5, 3, 2, 0, -1, -1]
    # the same through exclusions alone, and for persons: columns (0, 1), (2, 3), (4, 5) are persons 10, 20, 30
    got = m.rank_case_hits_filtered([4, 4], SUM, float("-inf"), G, excl=[[BASE + 3, BASE + 4, BASE + 5], [BASE + 1, BASE + 2, BASE + 3, BASE + 4]])
    assert got["n_hits"].tolist() == [4] and got["idx"][0].tolist() == [BASE + 5, BASE + 2, BASE + 0, BASE + 1, -1, -1]
    hj = m.subjects_create(np.array([10, 10, 20, 20, 30, 30], np.int64))
    got = m.rank_case_subject_hits_filtered(hj, [4, 4], SUM, float("-inf"), 3, labels=h, masks=mk)
    # person 10: query 0 sees -1 (columns 0, 1), query 1 sees -1 (column 0) -> -1; person 20: query 0 sees 2 (column 2), query 1 nothing -> 2; person 30: query 1 sees 5
    assert got["n_hits"].tolist() == [3] and got["subject"][0].tolist() == [30, 20, 10] and got["score"][0].tolist() == [5, 2, -1]
    got = m.rank_case_subject_hits_filtered(hj, [4, 4], SUM, float("-inf"), 3, labels=h, masks=mk, excl=[[20], [10, 30]])
    # person 10: query 0 alone -> -1; person 20: excluded for query 0, no eligible template for query 1 -> absent; person 30: excluded for its only eligible member -> absent
    assert got["n_hits"].tolist() == [1] and got["subject"][0].tolist() == [10, -1, -1] and got["score"][0].view(U32).tolist() == np.array([-1, -np.inf, -np.inf], F32).view(U32).tolist()
    m.labels_free(h); m.subjects_free(hj)
    m.close()


# ---- 2: the model, templates ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", G_TEMPLATES)
def test_template_sweep(G, codebook_bytes, tiny):
    """Every n_q x matrix kind x filter x mode; layouts (two per matrix), thresholds and caps in turn.  All-pass masks and exclusions that name nothing equal the
    unfiltered call."""
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    glob = BASE + np.arange(G)
    lab = make_labels(G, rng)
    h = m.labels_create(lab)
    step = G_TEMPLATES.index(G)
    seen_filters, seen_layouts, absent = set(), set(), 0
    for n_q in N_QS:
        for kind in KINDS:
            rows = matrix(kind, n_q, G, rng)
            m.debug_rank_hits(None, rows, float("-inf"), 1)
            for lk in (LAYOUTS[step % len(LAYOUTS)], LAYOUTS[(step + 2) % len(LAYOUTS)]):
                case_of = layout(lk, n_q, rng)
                seen_layouts.add(lk)
                for i, fk in enumerate(FILTERS):
                    seen_filters.add(fk)
                    mk, ex, ok = make_filter(fk, rows, lab, glob, case_of, outside_templates(G), rng)
                    for mode in MODES:
                        model, fused, entry = case_template_model(rows, ok, case_of, mode, glob)
                        absent += int((~entry).sum())
                        ts = thresholds(fused, entry)
                        for j in range(3):
                            t, cap = ts[(step + i + 2 * j + mode) % len(ts)], CAPS[(step + i + j) % len(CAPS)]
                            got = m.rank_case_hits_filtered(case_of, mode, float(t), cap, labels=h if mk is not None else None, masks=mk, excl=ex)
                            assert_same(got, model.hits(t, cap), (G, n_q, kind, lk, fk, mode, float(t), cap))
                            if fk in ("all-pass", "names-nothing"):
                                assert_same(got, m.rank_case_hits(case_of, mode, float(t), cap), (G, n_q, kind, lk, fk, mode, "the unfiltered sibling"))
                        if fk == "case-none":                               # the whole row of that case is no entry
                            row = int(np.argmax(~entry.any(axis=1)))
                            assert not entry[row].any()
                            got = m.rank_case_hits_filtered(case_of, mode, float("-inf"), 100, labels=h, masks=mk)
                            assert got["n_hits"][row] == 0 and (got["idx"][row] == -1).all() and np.isneginf(got["score"][row]).all()
                    us, fus, rus = m.get_option("rank_cases_us"), m.get_option("case_fuse_us"), m.get_option("case_rank_us")
                    assert us > 0 and us >= fus >= 0 and us >= rus >= 0
            step += 1
    assert len(seen_filters) == len(FILTERS) and len(seen_layouts) == len(LAYOUTS) and absent > 0
    m.labels_free(h)
    m.close()


# ---- 3: the model, subjects -----------------------------------------------------------------------------------------------------------------------------
def subject_plan(n_subjects, rng):
    """3 S + 1 templates dealt at random over S persons (every person present): a person's templates carry different labels."""
    ids = rng.permutation(np.unique(rng.integers(0, 1 << 40, 4 * n_subjects + 8, dtype=np.int64)))[:n_subjects]
    return ids[rng.permutation(np.r_[np.arange(n_subjects), rng.integers(0, n_subjects, 2 * n_subjects + 1)])]


@pytest.mark.parametrize("n_subjects", S_SUBJECTS)
def test_subject_sweep(n_subjects, codebook_bytes, tiny):
    rng = np.random.default_rng(SEED + 11 * n_subjects)
    subject = subject_plan(n_subjects, rng)
    G = len(subject)
    assert len(np.unique(subject)) == n_subjects and G <= G_TINY
    m = tap_matcher(codebook_bytes, tiny, G)
    hj = m.subjects_create(subject)
    lab = make_labels(G, rng)
    h = m.labels_create(lab)
    sid = np.unique(subject)
    outside = [int(sid.max()) + 1, 1 << 50, int(sid.max()) + 7]
    step = S_SUBJECTS.index(n_subjects)
    split_persons = one_member_only = 0
    for n_q in N_QS:
        for kind in KINDS:
            rows = matrix(kind, n_q, G, rng)
            m.debug_rank_hits(None, rows, float("-inf"), 1)
            lk = LAYOUTS[step % len(LAYOUTS)]
            case_of = layout(lk, n_q, rng)
            _, best, _ = subject_best_eligible(rows, np.ones(rows.shape, bool), subject)
            for i, fk in enumerate(FILTERS):
                # the masks as for the templates; the exclusions name persons: made on the persons' unfiltered maxima
                mk, _, _ = make_filter(fk, rows, lab, BASE + np.arange(G), case_of, [], rng)
                ex = None
                if fk in ("exclusions", "masks+exclusions", "names-nothing"):
                    ex = [list(outside) + outside[:1] for _ in range(n_q)] if fk == "names-nothing" else exclusions(best, sid, n_q, outside, rng)
                    if fk != "names-nothing" and n_q > 1:                   # a person excluded for one member only
                        ex[0] = list(ex[0]) + [int(sid[0])]; ex[1] = [x for x in ex[1] if x != int(sid[0])]
                        one_member_only += 1
                ok = label_test(lab, mk, n_q)
                if mk is not None and n_q > 1:                              # persons whose templates are eligible for different members
                    _, _, have = subject_best_eligible(rows, ok, subject)
                    split_persons += int((have.any(axis=0) & ~have.all(axis=0)).sum())
                for mode in MODES:
                    model, fused, entry = case_subject_model(rows, ok, subject, ex, case_of, mode)
                    ts = thresholds(fused, entry)
                    for j in range(3):
                        t, cap = ts[(step + i + 2 * j + mode) % len(ts)], CAPS[(step + i + j) % len(CAPS)]
                        got = m.rank_case_subject_hits_filtered(hj, case_of, mode, float(t), cap, labels=h if mk is not None else None, masks=mk, excl=ex)
                        assert_same(got, model.hits(t, cap), (n_subjects, n_q, kind, lk, fk, mode, float(t), cap))
                        if fk in ("all-pass", "names-nothing"):
                            assert_same(got, m.rank_case_subject_hits(hj, case_of, mode, float(t), cap), (n_subjects, n_q, kind, lk, fk, mode, "the unfiltered sibling"))
            step += 1
    assert one_member_only > 0 and (split_persons > 0 or n_subjects == 1)
    m.labels_free(h); m.subjects_free(hj)
    m.close()


# ---- 4: identities with the siblings, and the matrix is unwritten ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_identities(kind, codebook_bytes, tiny):
    """Singleton cases with AFIS_CASE_MAX are afis_rank_hits_filtered (and, without -0.0 in the matrix, afis_rank_subject_hits_filtered's ids and scores); the plain
    calls on the same matrix return their unfiltered results before and after."""
    G, n_q = 1025, R + 1
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 2 + len(kind))
    rows = matrix(kind, n_q, G, rng)
    glob = BASE + np.arange(G)
    cards = np.arange(G, dtype=np.int64) // 10 * 7 + 1
    hj = m.subjects_create(cards)
    lab = make_labels(G, rng)
    h = m.labels_create(lab)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    case_of = 5 + 3 * np.arange(n_q)
    pairs = np.arange(n_q) // 2
    siblings = lambda: (m.rank_hits(0.0, 100), m.rank_hits(float("-inf"), 4096), m.rank_subject_hits(hj, float(HAIR), 100), m.rank_subjects(hj, n_q, 24),
                        m.rank_case_hits(pairs, SUM, 0.0, 100), m.rank_case_subject_hits(hj, pairs, MAX, 0.0, 100), m.rank_latent_hits(0.0, 4),
                        m.rank_hits_filtered(0.0, 100, labels=h, masks=finger_masks(n_q, np.random.default_rng(1))))
    before = siblings()
    for fk in ("random-tenth", "masks+exclusions", "exclusions", "all-pass"):
        mk, ex, ok = make_filter(fk, rows, lab, glob, case_of, outside_templates(G), rng)
        hm = h if mk is not None else None
        for t in (float("-inf"), -1.0, 0.0, float(HAIR)):
            for cap in (1, 100, 4096):
                got = m.rank_case_hits_filtered(case_of, MAX, t, cap, labels=hm, masks=mk, excl=ex)
                assert np.array_equal(got["case_id"], case_of)
                assert_same({k: got[k] for k in ("n_hits", "idx", "score")}, m.rank_hits_filtered(t, cap, labels=hm, masks=mk, excl=ex), (fk, t, cap))
        if kind != "special":                                               # (-0.0: the subject hit lists compare the raw word, the case lists rank_key)
            sx = None if ex is None else [[int(cards[g - BASE]) for g in e if BASE <= g < BASE + G] for e in ex]
            for t in (float("-inf"), 0.0, float(HAIR)):
                gs = m.rank_case_subject_hits_filtered(hj, case_of, MAX, t, 100, labels=hm, masks=mk, excl=sx)
                sub = m.rank_subject_hits_filtered(hj, t, 100, labels=hm, masks=mk, excl=sx)
                assert_same({k: gs[k] for k in ("n_hits", "subject", "score")}, {k: sub[k] for k in ("n_hits", "subject", "score")}, ("subjects", fk, t))
        assert_same(m.rank_latent_hits_filtered(0.0, 4, labels=hm, masks=mk, excl=ex), latent_model(rows, ok, 0).hits(F32(0), 4), ("columns", fk))
    for b, f in zip(before, siblings()):
        assert_same(f, as_words(b), "the siblings on the same matrix")
    m.labels_free(h); m.subjects_free(hj)
    m.close()


# ---- 5: filtered reverse lists ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 10, 63, 64, 65, 257])
def test_reverse_sweep(G, codebook_bytes, tiny):
    """n_q and G around the 64 x 64 transpose tile; all-pass filters equal the unfiltered call on every score kind; a template no query is eligible for has no hit."""
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 500 + G)
    glob = BASE + np.arange(G)
    lab = make_labels(G, rng)
    lab[G // 3] = U64(1) << U64(50)                                         # no finger bit: no any_of mask of a finger passes it
    h = m.labels_create(lab)
    step = G
    for n_q in (1, 63, 64, 65, 130):
        for kind in KINDS:
            rows = matrix(kind, n_q, G, rng)
            m.debug_rank_hits(None, rows, float("-inf"), 1)
            base = (0, 7000)[step % 2]
            singles = 5 + 3 * np.arange(n_q)
            for t in (F32(-np.inf), F32(0.0)):                              # all-pass masks, and exclusions that name nothing: the unfiltered call
                old = m.rank_latent_hits(float(t), 100, base)
                assert_same(old, latent_model(rows, np.ones(rows.shape, bool), base).hits(t, 100), (G, n_q, kind, "afis_rank_latent_hits"))
                assert_same(m.rank_latent_hits_filtered(float(t), 100, base, labels=h, masks=np.zeros((n_q, 3), U64)), old, (G, n_q, kind, "all-pass"))
                assert_same(m.rank_latent_hits_filtered(float(t), 100, base, excl=[outside_templates(G)] * n_q), old, (G, n_q, kind, "names nothing"))
                assert_same(m.rank_latent_hits_filtered(float(t), 100, base), old, (G, n_q, kind, "no filter"))
            for i in range(2):
                fk = ("random-tenth", "masks+exclusions", "exclusions", "member-none")[(step + i) % 4]
                mk, ex, ok = make_filter(fk, rows, lab, glob, singles, outside_templates(G), rng)
                model = latent_model(rows, ok, base)
                ts = thresholds(model.words, ok.T)
                for j in range(3):
                    t, cap = ts[(step + i + 2 * j) % len(ts)], CAPS[(step + j) % len(CAPS)]
                    got = m.rank_latent_hits_filtered(float(t), cap, base, labels=h if mk is not None else None, masks=mk, excl=ex)
                    assert_same(got, model.hits(t, cap), (G, n_q, kind, fk, float(t), cap))
                if fk in ("random-tenth", "masks+exclusions"):
                    assert not ok[:, G // 3].any()
                    got = m.rank_latent_hits_filtered(float("-inf"), 4, base, labels=h, masks=mk, excl=ex)
                    assert got["n_hits"][G // 3] == 0 and (got["latent"][G // 3] == -1).all() and np.isneginf(got["score"][G // 3]).all()
            assert m.get_option("rank_latents_us") > 0
            step += 1
    m.labels_free(h)
    m.close()


def test_subsets(codebook_bytes, tiny):
    """A subset listed out of order: the label of a column is its listed template's, exclusions are global indices, the case lists carry global indices and the rows of
    the column lists stand in the caller's order."""
    G, n_listed = 600, 63
    rng = np.random.default_rng(SEED + 4)
    m = tap_matcher(codebook_bytes, tiny, G)
    cards = np.arange(G, dtype=np.int64) // 10 * 3 + 50
    listed = [int(g) for g in rng.permutation(np.r_[120:130, 300, 301, 305, rng.permutation(np.r_[0:120, 130:300, 310:600])[:n_listed - 13]])]
    assert listed != sorted(listed) and len(set(listed)) == n_listed
    hs = m.subset_create([BASE + g for g in listed])
    hj = m.subjects_create(cards)
    lab = make_labels(G, rng)
    h = m.labels_create(lab)
    held = np.sort(np.asarray(listed))                                      # the device holds the listed templates in ascending global order
    back = np.searchsorted(held, np.asarray(listed))                        # the caller's row j is device column back[j]
    unlisted = np.setdiff1d(np.arange(G), held)
    outside = [int(BASE + unlisted[0]), int(BASE + unlisted[5]), BASE + G, int(BASE + unlisted[-1]), BASE - 1]
    n_q = R + 1
    case_of = layout("five", n_q, rng)
    for kind in KINDS:
        rows = matrix(kind, n_q, n_listed, rng)
        m.debug_rank_rows(rows, 1, subset=hs)
        for fk in ("random-tenth", "masks+exclusions", "exclusions"):
            mk, ex, ok = make_filter(fk, rows, lab[held], BASE + held, case_of, outside, rng)
            hm = h if mk is not None else None
            for mode in MODES:
                model, fused, entry = case_template_model(rows, ok, case_of, mode, BASE + held)
                for t in thresholds(fused, entry)[::2]:
                    got = m.rank_case_hits_filtered(case_of, mode, float(t), 100, labels=hm, masks=mk, excl=ex)
                    assert_same(got, model.hits(t, 100), ("subset", kind, fk, mode, float(t)))
                    assert np.isin(got["idx"][got["idx"] >= 0], BASE + held).all()
                sx = None if ex is None else [[int(cards[g - BASE]) for g in e if BASE <= g < BASE + G] for e in ex]
                sm, sfused, sentry = case_subject_model(rows, label_test(lab[held], mk, n_q), cards[held], sx, case_of, mode)
                for t in thresholds(sfused, sentry)[::2]:
                    assert_same(m.rank_case_subject_hits_filtered(hj, case_of, mode, float(t), 100, labels=hm, masks=mk, excl=sx), sm.hits(t, 100), ("subset subjects", kind, fk, mode, float(t)))
            want = latent_model(rows, ok, 40)
            for t in (F32(-np.inf), F32(0.0)):
                w = want.hits(t, 5)
                got = m.rank_latent_hits_filtered(float(t), 5, 40, labels=hm, masks=mk, excl=ex)
                assert_same(got, {k: v[back] for k, v in w.items()}, ("subset columns", kind, fk, float(t)))
    m.subset_free(hs)
    with pytest.raises(M.AfisError, match=ESTATE):                          # the sub-shard the matrix refers to is gone
        m.rank_case_hits_filtered(case_of, SUM, 0.0, 24)
    m.labels_free(h); m.subjects_free(hj)
    m.close()


# ---- 6: the refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(codebook_bytes, tiny):
    """One fault per call; nothing is queued, and the context answers the next correct call."""
    i64p, u64p, fp = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    G, n_q = 150, 4
    rng = np.random.default_rng(SEED + 6)
    m = tap_matcher(codebook_bytes, tiny, G)
    tens = np.arange(G, dtype=np.int64) // 10
    ha = m.subjects_create(tens)
    lab = make_labels(G, rng)
    hl = m.labels_create(lab)
    glob = BASE + np.arange(G)
    co = np.array([7, 3, 7, 3], np.int64)
    cid = np.zeros(2, np.int64); nh = np.zeros(G, np.int64); a = np.zeros((G, 24), np.int64); sc = np.zeros((G, 24), np.float32)
    pc, pi, pn, pa, ps = co.ctypes.data_as(i64p), cid.ctypes.data_as(i64p), nh.ctypes.data_as(i64p), a.ctypes.data_as(i64p), sc.ctypes.data_as(fp)
    mk = finger_masks(n_q, rng)
    off = np.array([0, 1, 1, 3, 4], np.int64); ent = np.array([BASE + 3, BASE + 9, BASE + 9, BASE + G + 4], np.int64)
    pm, po, pe = mk.ctypes.data_as(u64p), off.ctypes.data_as(i64p), ent.ctypes.data_as(i64p)
    # f(labels, masks, excl_off, excl, mode, n_cases or n_templates, min_score, cap): the three calls behind one face
    ct = lambda l, k, o, e, mode, n, t, cap: m.lib.afis_rank_case_hits_filtered(m.ctx, l, k, o, e, pc, n_q, mode, n, t, cap, pi, pn, pa, ps)
    cs = lambda l, k, o, e, mode, n, t, cap: m.lib.afis_rank_case_subject_hits_filtered(m.ctx, ha[0], l, k, o, e, pc, n_q, mode, n, t, cap, pi, pn, pa, ps)
    lt = lambda l, k, o, e, mode, n, t, cap: m.lib.afis_rank_latent_hits_filtered(m.ctx, l, k, o, e, n, t, cap, 0, pn, pa, ps)
    calls = ((ct, 2), (cs, 2), (lt, G))
    for f, n in calls:
        assert f(hl[0], pm, po, pe, SUM, n, 0.0, 24) == -3                  # no matrix to rank
    rows = matrix("search-like", n_q, G, rng)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    other = tap_matcher(codebook_bytes, tiny, G)
    ho = other.labels_create(lab)
    bad_offs = [np.array(x, np.int64) for x in ([1, 1, 1, 3, 4], [0, 2, 1, 3, 4])]
    neg = np.array([BASE + 3, -1, BASE + 9, 7], np.int64)
    for f, n in calls:
        assert f(ho[0], pm, po, pe, SUM, n, 0.0, 24) == -1                  # a labels handle of another context
        assert f(ha[0], pm, po, pe, SUM, n, 0.0, 24) == -1                  # a subject handle is no labels handle
        assert f(None, pm, po, pe, SUM, n, 0.0, 24) == -1                   # masks without labels
        for bo in bad_offs:                                                 # excl_off[0] != 0; a decreasing CSR
            assert f(hl[0], pm, bo.ctypes.data_as(i64p), pe, SUM, n, 0.0, 24) == -1
        assert f(hl[0], pm, po, neg.ctypes.data_as(i64p), SUM, n, 0.0, 24) == -1   # a negative entry
        assert f(hl[0], pm, po, None, SUM, n, 0.0, 24) == -1                # offsets that list entries, no entries
        for bad_n in (n - 1, n + 1):                                        # a wrong n_cases / n_templates
            assert f(hl[0], pm, po, pe, SUM, bad_n, 0.0, 24) == -1
        for cap in (0, 4097):
            assert f(hl[0], pm, po, pe, SUM, n, 0.0, cap) == -1
        assert f(hl[0], pm, po, pe, SUM, n, float("nan"), 24) == -1
    for f in (ct, cs):
        for mode in (-1, 2):
            assert f(hl[0], pm, po, pe, mode, 2, 0.0, 24) == -1
    assert m.lib.afis_rank_latent_hits_filtered(m.ctx, hl[0], pm, po, pe, G, 0.0, 24, -1, pn, pa, ps) == -1   # a negative latent_base
    assert m.lib.afis_rank_case_subject_hits_filtered(m.ctx, None, hl[0], pm, po, pe, pc, n_q, SUM, 2, 0.0, 24, pi, pn, pa, ps) == -1
    assert m.lib.afis_rank_case_hits_filtered(m.ctx, hl[0], pm, po, pe, pc, n_q, SUM, 2, 0.0, 24, None, pn, pa, ps) == -1   # a null output
    other.close()
    # the refused calls left the matrix rankable; through the C ABI
    ex = [ent[off[q]:off[q + 1]].tolist() for q in range(n_q)]
    ok = label_test(lab, mk, n_q)
    okx = ok & not_listed(glob, ex, n_q)
    assert ct(hl[0], pm, po, pe, MAX, 2, 0.0, 24) == 0
    assert_same({"case_id": cid, "n_hits": nh[:2], "idx": a[:2], "score": sc[:2]}, case_template_model(rows, okx, co, MAX, glob)[0].hits(F32(0), 24), "through the C ABI")
    sent = np.array([0, 14, 14, 10 ** 9], np.int64)
    sx = [sent[off[q]:off[q + 1]].tolist() for q in range(n_q)]
    assert cs(hl[0], pm, po, sent.ctypes.data_as(i64p), SUM, 2, 0.0, 24) == 0
    assert_same({"case_id": cid, "n_hits": nh[:2], "subject": a[:2], "score": sc[:2]}, case_subject_model(rows, ok, tens, sx, co, SUM)[0].hits(F32(0), 24), "subjects through the C ABI")
    assert lt(hl[0], pm, po, pe, SUM, G, 0.0, 24) == 0
    assert_same({"n_hits": nh, "latent": a, "score": sc}, latent_model(rows, okx, 0).hits(F32(0), 24), "columns through the C ABI")
    # an older gallery epoch: AFIS_ESTATE for the labels handle, with a matrix to rank
    m.gallery_remove([BASE + 47])
    rows = matrix("search-like", n_q, G, rng)
    m.debug_rank_hits(None, rows, float("-inf"), 1)
    for f, n in ((ct, 2), (lt, G)):
        assert f(hl[0], pm, po, pe, SUM, n, 0.0, 24) == -3
        assert "free the handle and create it again" in m.lib.afis_last_error(m.ctx).decode()
        assert f(None, None, po, pe, SUM, n, 0.0, 24) == 0                  # without the handle the call works: the refusals left the matrix rankable
    assert cs(None, None, po, pe, SUM, 2, 0.0, 24) == -3                    # (the subject handle is the older gallery's too)
    m.labels_free(hl); m.subjects_free(ha)
    m.close()
