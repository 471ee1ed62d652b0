"""Cascade over a part of the shard on the GPU: afis_search_cascade_eligible runs the cascade per latent over the templates its masks pass only, afis_search_cascade_subset
over the columns of a live subset.

The yardstick is always existing code on the SAME context — search_resident(k=0, want_scores, want_parts), or search_subset_resident(...) — run through the numpy
model tests/cascade_eligible_model.py (built on tests/cascade_model.py).  Every comparison is on uint32 views, exact.  The two mapped kernels are swept on planted
tables through their parity tap, against a model of the pair tables written out below.
"""
import importlib

import numpy as np
import pytest

import cases
import cascade_model as CM
import cascade_eligible_model as EM

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 3                                                                    # cases.small_set(seed 3, 3 latents, 70 prints): the set of tests/test_gpu_cascade_search.py
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NINF = float("-inf")
KEEPS = (1, 7, 14, 15, 28, 64, 65, 100)                                     # keep == |E| (14, 28), keep > |E|, the segment edge 64 / 65, each below and above G = 70
POS_LISTED, POS_NO_ENTRY, POS_NOT_COVERED = 0, 1, 2
ALL5 = 31
ONLY0 = (0, 0, ALL5 & ~1)                                                   # none_of = all but bit 0: the 14 prints of class 0
MASKS3 = np.array([ONLY0, ONLY0, ((1 << 1) | (1 << 3), 0, 0)], np.uint64)   # latents 0 and 1 share a class; latent 2: 28 prints
ZERO3 = np.zeros((3, 3), np.uint64)


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


def counts(lats):
    return [len(L.minu) for L in lats], [len(L.tex) for L in lats]


def labels5(G):
    return (np.uint64(1) << (np.arange(G) % 5).astype(np.uint64)).astype(np.uint64)


def fresh(cbb, gal, opts=None, base=BASE, taps=False):
    m = M.Matcher(cbb, taps=taps)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    m.gallery_add(gal)
    m.gallery_commit(base)
    return m


def reference(m, h):
    """The yardstick: the full search of the same context, with scores and parts."""
    return m.search_resident(h, k=0, want_scores=True, want_parts=True)


def same(got, want, what):
    """The call's five outputs against the model's, word for word."""
    assert np.array_equal(got["n_kept"], want["n_kept"]), (what, got["n_kept"], want["n_kept"])
    assert np.array_equal(got["kept_idx"], want["kept_idx"]), (what, np.argwhere(got["kept_idx"] != want["kept_idx"])[:6].tolist())
    g = got["scores"].view(np.uint32)
    assert g.shape == want["matrix"].shape and np.array_equal(g, want["matrix"]), (what, np.argwhere(g != want["matrix"])[:8].tolist())
    gp = got["kept_parts"].view(np.uint32)
    assert np.array_equal(gp, want["kept_parts"]), (what, np.argwhere(gp != want["kept_parts"])[:8].tolist())


def check(m, lats, lh, lab, masks, ref, keep, base=BASE, what=""):
    """One eligible cascade against the model of the reference search; -> (what the call returned, the model)."""
    nm, nt = counts(lats)
    want = EM.expected_eligible(ref["scores"], ref["parts"], nm, nt, lab, masks, keep, base)
    got = m.search_cascade_eligible(lats, lh, masks, keep)
    n_pairs = int(sum(int(want["n_kept"][q]) for q in range(len(lats)) if ref["status"][q] == 0))
    print(f"{what} keep {keep}: {len(lats)} x {ref['scores'].shape[1]}, |E| {want['E'].sum(axis=1).tolist()}, classes {m.get_option('eligible_classes')}, "
          f"kept pairs {m.get_option('cascade_kept_pairs')}, stage 1 {m.get_option('cascade_stage1_us')} us, select {m.get_option('cascade_select_us')} us, "
          f"stage 2 {m.get_option('cascade_stage2_us')} us")
    same(got, want, (what, keep))
    assert np.array_equal(got["status"], ref["status"])
    assert m.get_option("cascade_kept_pairs") == n_pairs
    assert m.get_option("eligible_classes") == len({tuple(int(x) for x in r) for r in np.asarray(masks, np.uint64).reshape(-1, 3)})
    tm = m.timing()
    assert tm["pairs"] == int(want["E"].sum()) and tm["adc_ms"] == 0 and tm["tex_tail_ms"] == 0 and tm["adc_lookups"] == 0     # stage 1 scored the eligible cells only
    return got, want


# ---- 1: the small set, two launch groups, chunks of 50 ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(cb, codebook_bytes):
    lats, gal = cases.small_set(cb, seed=SEED, n_lat=3, n_gal=70)
    m = fresh(codebook_bytes, gal, {"query_batch": 2, "cascade_pairs_per_launch": 50})
    h = m.upload_queries(lats)
    ref = reference(m, h)
    lab = labels5(70)
    lh = m.labels_create(lab)
    yield m, h, lats, ref, lab, lh
    m.close()


@pytest.mark.parametrize("keep", KEEPS)
def test_small_set_equals_the_model(small, keep):
    m, h, lats, ref, lab, lh = small
    got, want = check(m, lats, lh, lab, MASKS3, ref, keep, what="small set")
    assert want["E"].sum(axis=1).tolist() == [14, 14, 28]
    # the ranking family on the matrix left behind: the kept list re-ranked by final score
    cap = keep
    n_hits, idx, pos = CM.rank_rows(want["matrix"].view(np.float32), cap, BASE)
    hits = m.rank_hits(NINF, cap)
    assert np.array_equal(hits["n_hits"], got["n_kept"]) and np.array_equal(hits["n_hits"], n_hits) and np.array_equal(hits["idx"], idx)
    for q in range(3):
        assert sorted(hits["idx"][q].tolist()) == sorted(got["kept_idx"][q].tolist())
        n = int(n_hits[q])
        assert hits["score"][q, :n].view(np.uint32).tolist() == ref["scores"][q, pos[q, :n]].view(np.uint32).tolist()
    # a dropped eligible print and an ineligible print are no entries; a kept one stands where the list has it
    targets = []
    for q in range(3):
        dropped = np.flatnonzero(want["E"][q] & (want["matrix"][q] == CM.NO_ENTRY))
        targets += [(q, int(dropped[-1]), POS_NO_ENTRY, -1)] if len(dropped) else []
        targets += [(q, int(np.flatnonzero(~want["E"][q])[0]), POS_NO_ENTRY, -1), (q, int(pos[q, 0]), POS_LISTED, 0)]
    p = m.rank_positions([t[0] for t in targets], [BASE + t[1] for t in targets])
    assert p["status"].tolist() == [t[2] for t in targets] and p["n_before"].tolist() == [t[3] for t in targets]
    if keep < 14:
        assert sum(1 for t in targets if t[2] == POS_NO_ENTRY) == 6          # every latent has a dropped eligible print


def test_small_set_is_not_vacuous(small):
    """From the reference search's outputs alone: at keep 7 the eligible cascade gives latent 0 seven eligible prints where the full cascade's kept set holds fewer of
    them (its planted mates 0, 1, 2 lie in three label classes and all three are kept at keep 7); and a kept cell has a positive texture part and a final score that
    is not m."""
    m, h, lats, ref, lab, lh = small
    nm, nt = counts(lats)
    e = EM.expected_eligible(ref["scores"], ref["parts"], nm, nt, lab, MASKS3, 7, BASE)
    full = CM.expected(ref["scores"], ref["parts"], nm, nt, 7, BASE)
    E0 = set(np.flatnonzero(e["E"][0]).tolist())
    kept_e = set(e["kept_pos"][0, :e["n_kept"][0]].tolist()); kept_f = set(full["kept_pos"][0, :full["n_kept"][0]].tolist())
    assert len(kept_e) == 7 and kept_e <= E0 and len(kept_f & E0) < 7
    tex_matters = False
    for q in range(3):
        kp = e["kept_pos"][q][:e["n_kept"][q]]
        tex_matters |= bool(((ref["parts"][q, kp, 3] > 0) & (ref["scores"][q, kp].view(np.uint32) != e["m"][q, kp].view(np.uint32))).any())
    assert tex_matters


# ---- 2: classes ---------------------------------------------------------------------------------------------------------------------------------------------
def test_classes(small):
    m, h, lats, ref, lab, lh = small
    # a zero mask triple: the direct route on the resident shard — afis_search_cascade's result, word for word
    for keep in (7, 65):
        got, want = check(m, lats, lh, lab, ZERO3, ref, keep, what="zero triple")
        assert m.get_option("eligible_classes") == 1
        plain = m.search_cascade(h, keep)
        for key in ("scores", "kept_idx", "kept_parts", "n_kept", "status"):
            assert got[key].tobytes() == plain[key].tobytes(), (keep, key)
    # a triple nothing passes, a class of exactly 1 template, and a third triple: three classes
    lab1 = lab.copy(); lab1[33] |= np.uint64(1) << np.uint64(40)
    lh1 = m.labels_create(lab1)
    masks = np.array([(1 << 50, 0, 0), (1 << 40, 0, 0), ((1 << 1) | (1 << 3), 0, 0)], np.uint64)
    for keep in (1, 7):
        got, want = check(m, lats, lh1, lab1, masks, ref, keep, what="three classes")
        assert m.get_option("eligible_classes") == 3
        assert got["n_kept"].tolist() == [0, 1, min(keep, 28)]
        assert (got["scores"].view(np.uint32)[0] == CM.NO_ENTRY).all() and (got["kept_idx"][0] == -1).all() and not got["kept_parts"][0].any()
        assert got["kept_idx"][1, 0] == BASE + 33 and got["scores"].view(np.uint32)[1, 33] == ref["scores"].view(np.uint32)[1, 33]
    m.labels_free(lh1)


# ---- 3: edges: every texture slot, no texture, a latent-empty query; prints without minutiae, an empty entry, a removed one -------------------------------------
def test_edges_in_two_classes(cb, codebook_bytes):
    base_latent, named = cases.edge_latents(cb)
    lats = [base_latent] + list(named.values())
    rng = np.random.default_rng(77)
    def tex_only():
        t = S.make_rolled(rng, cb, n_tex=int(rng.integers(300, 420)))
        t.minu = []
        return t
    gal = [S.make_mate(rng, cb, base_latent, frac=0.8, n_tex=400), tex_only(), S.make_rolled(rng, cb, n_tex=350), tex_only(), T.FPTemplate(), tex_only(),
           S.make_mate(rng, cb, base_latent, frac=0.5, n_tex=380), tex_only(), S.make_rolled(rng, cb, n_tex=330), tex_only(), tex_only(), S.make_mate(rng, cb, base_latent, frac=0.3, n_tex=360)]
    m = fresh(codebook_bytes, gal, {"query_batch": 4, "cascade_pairs_per_launch": 5})
    m.gallery_remove([BASE + 8])                                            # removed after the commit
    h = m.upload_queries(lats)
    ref = reference(m, h)
    nm, nt = counts(lats)
    G = ref["scores"].shape[1]
    assert G == 12 and ref["status"].tolist().count(1) == 1                 # one latent-empty query; the removed entry is still a column
    assert np.flatnonzero(ref["scores"][0].view(np.uint32) == CM.MINUS_ONE).tolist() == [4, 8]
    assert {-1, 0, 2, 12, 27, 28, 29} <= set(CM.tex_slots(nm, nt).tolist())
    # two classes that each hold mates, prints without minutiae and a -1 entry: columns {0, 1, 4, 5, 6, 9} and {2, 3, 7, 8, 10, 11}
    lab = np.array([1, 1, 2, 2, 1, 1, 1, 2, 2, 1, 2, 2], np.uint64)
    lh = m.labels_create(lab)
    masks = np.array([((1, 0, 0) if q % 2 == 0 else (0, 0, 1)) for q in range(len(lats))], np.uint64)
    for keep in (1, 3, 5, 6, 7, 12):                                        # below, at and above |E| = 6; 5 keeps every non-empty column and one cut inside the ties
        got, want = check(m, lats, lh, lab, masks, ref, keep, what="edges")
        assert want["E"].sum(axis=1).tolist() == [6] * len(lats)
        if keep >= 6:                                                       # every eligible cell is kept: afis_search_eligible's matrix
            assert np.array_equal(got["scores"].view(np.uint32), np.where(want["E"], ref["scores"].view(np.uint32), CM.NO_ENTRY))
    m.close()


# ---- 4: the subset form -------------------------------------------------------------------------------------------------------------------------------------
def subset_lists():
    rng = np.random.default_rng(11)
    out = [np.zeros(0, np.int64), np.array([BASE + 41], np.int64), np.sort(rng.choice(70, 7, replace=False))[::-1].copy() + BASE]     # empty; one; 7 in DESCENDING order
    for n in (64, 65, 70):
        out.append(rng.permutation(70)[:n] + BASE)                          # shuffled
    return [np.ascontiguousarray(a, np.int64) for a in out]


@pytest.mark.parametrize("which", range(6), ids=["n0", "n1", "n7-descending", "n64", "n65", "n70"])
def test_subset_form_equals_the_model(small, which):
    m, h, lats, ref, lab, lh = small
    idx = subset_lists()[which]
    n = len(idx)
    nm, nt = counts(lats)
    sh = m.subset_create(idx)
    sref = m.search_subset_resident(sh, h, k=0, want_scores=True, want_parts=True)
    if n:                                                                   # (the yardstick itself: the full search's columns)
        assert np.array_equal(sref["scores"].view(np.uint32), ref["scores"].view(np.uint32)[:, idx - BASE])
    for keep in (1, 7, 64, 65, 100):
        want = EM.expected_subset(sref["scores"], sref["parts"], nm, nt, idx, keep)
        got = m.search_cascade_subset(sh, h, keep)
        same(got, want, ("subset", n, keep))
        assert np.array_equal(got["status"], ref["status"])
        assert m.get_option("cascade_kept_pairs") == (3 * min(keep, n))
        if n == 0:
            continue
        assert m.timing()["pairs"] == 3 * n
        # the ranking family names the matrix's columns by global index: the kept cells are the only entries
        hits = m.rank_hits(NINF, keep)
        assert np.array_equal(hits["n_hits"], got["n_kept"])
        for q in range(3):
            nk = int(got["n_kept"][q])
            assert sorted(hits["idx"][q, :nk].tolist()) == sorted(got["kept_idx"][q, :nk].tolist())
            order = np.lexsort((hits["idx"][q, :nk], -CM.rank_key(hits["score"][q, :nk]).astype(np.int64)))
            assert order.tolist() == list(range(nk))                        # in rank-list order: key descending, equal keys by ascending global index
            col = {int(g): j for j, g in enumerate(idx)}
            assert hits["score"][q, :nk].view(np.uint32).tolist() == [int(sref["scores"].view(np.uint32)[q, col[int(g)]]) for g in hits["idx"][q, :nk]]
        if keep < n:
            dropped = int(idx[np.flatnonzero(want["matrix"][0] == CM.NO_ENTRY)[0]])
            outside = [g for g in range(BASE, BASE + 70) if g not in set(idx.tolist())]
            p = m.rank_positions([0, 0] + ([0] if outside else []), [dropped, int(got["kept_idx"][0, 0])] + outside[:1])
            assert p["status"].tolist() == [POS_NO_ENTRY, POS_LISTED] + ([POS_NOT_COVERED] if outside else [])
    m.subset_free(sh)


# ---- 5: options -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,keep", [({"ref_tie_order": 2}, 7), ({"adc_variant": 8}, 65)], ids=["ref_tie_order2", "adc_variant8"])
def test_options_against_the_same_contexts_search(opt, keep, cb, codebook_bytes):
    lats, gal = cases.small_set(cb, seed=SEED, n_lat=3, n_gal=70)
    m = fresh(codebook_bytes, gal, dict(opt, query_batch=2, cascade_pairs_per_launch=50))
    h = m.upload_queries(lats)
    ref = reference(m, h)
    lab = labels5(70)
    lh = m.labels_create(lab)
    check(m, lats, lh, lab, MASKS3, ref, keep, what=str(opt))
    idx = np.ascontiguousarray(np.arange(69, 20, -3, dtype=np.int64) + BASE)      # 17 prints, descending
    sh = m.subset_create(idx)
    sref = m.search_subset_resident(sh, h, k=0, want_scores=True, want_parts=True)
    nm, nt = counts(lats)
    same(m.search_cascade_subset(sh, h, min(keep, 9)), EM.expected_subset(sref["scores"], sref["parts"], nm, nt, idx, min(keep, 9)), (str(opt), "subset"))
    m.close()


# ---- 6: state and arguments -------------------------------------------------------------------------------------------------------------------------------------
def test_state_and_arguments(cb, codebook_bytes):
    lats, gal = cases.small_set(cb, seed=SEED, n_lat=3, n_gal=14)
    m = M.Matcher(codebook_bytes)
    m.gallery_add(gal[:10])
    m.gallery_commit(BASE)
    h = m.upload_queries(lats)
    hr = m.upload_queries(lats, reserve=16)
    lab = labels5(10)
    lh = m.labels_create(lab)
    masks = np.array([ONLY0, (0, 0, 0), (3, 0, 0)], np.uint64)
    sh = m.subset_create([BASE + 7, BASE + 2, BASE + 5])
    before = m.search_resident(h, k=3, want_scores=True, want_parts=True)
    elig_before = m.search_eligible(lats, lh, masks)
    casc_before = m.search_cascade(h, 3)
    names = ("cascade_stage1_us", "cascade_select_us", "cascade_stage2_us", "cascade_kept_pairs")

    def refused(call, code):
        """A good call leaves a rankable matrix; the refused one leaves none, no option and nothing allocated: the full search returns the bytes it returned before."""
        m.search_cascade_eligible(lats, lh, masks, 3)
        assert m.rank_hits(NINF, 3)["n_hits"].tolist() == [2, 3, 3]
        with pytest.raises(M.AfisError, match=code):
            call()
        with pytest.raises(M.AfisError, match=ESTATE):
            m.rank_hits(NINF, 3, n_q=3)
        for name in names:
            assert m.get_option(name) == 0, name
    for bad in (0, 4097, -1):
        refused(lambda: m.search_cascade_eligible(lats, lh, masks, bad), EINVAL)
        refused(lambda: m.search_cascade_subset(sh, h, bad), EINVAL)
    refused(lambda: m.search_cascade_eligible(lats, None, masks, 3), EINVAL)
    refused(lambda: m.search_cascade_eligible(lats, lh, None, 3), EINVAL)
    dead = m.labels_create(lab); m.labels_free(dead)
    refused(lambda: m.search_cascade_eligible(lats, dead, masks, 3), EINVAL)      # not a live labels handle
    dead_s = m.subset_create([BASE + 1]); m.subset_free(dead_s)
    refused(lambda: m.search_cascade_subset(dead_s, h, 3), EINVAL)                # not a live subset
    after = m.search_resident(h, k=3, want_scores=True, want_parts=True)
    for key in ("scores", "parts", "topk_idx", "topk_score", "status"):
        assert before[key].tobytes() == after[key].tobytes(), key
    # after successful calls the two routes that existed before return the bytes they returned before
    got = m.search_cascade_eligible(lats, lh, masks, 5)
    assert got["n_kept"].tolist() == [2, 5, 4] and m.get_option("cascade_kept_pairs") == 11 and m.get_option("cascade_stage1_us") > 0 and m.get_option("cascade_stage2_us") > 0
    m.search_cascade_subset(sh, h, 2)
    assert m.get_option("cascade_kept_pairs") == 6
    elig_after = m.search_eligible(lats, lh, masks)
    casc_after = m.search_cascade(h, 3)
    for key in ("scores", "status"):
        assert elig_before[key].tobytes() == elig_after[key].tobytes(), key
    for key in ("scores", "kept_idx", "kept_parts", "n_kept", "status"):
        assert casc_before[key].tobytes() == casc_after[key].tobytes(), key
    # no queries
    out = m.search_cascade_eligible([], lh, np.zeros((0, 3), np.uint64), 4)
    assert out["scores"].shape == (0, 10) and out["kept_idx"].shape == (0, 4)
    h0 = m.upload_queries([])
    out = m.search_cascade_subset(sh, h0, 4)
    assert out["scores"].shape == (0, 3) and out["kept_idx"].shape == (0, 4) and m.get_option("cascade_kept_pairs") == 0
    # an appending commit: labels, the subset and the plain handle are stale; the reserved handle is accepted with a fresh subset
    m.gallery_reopen(); m.gallery_add(gal[10:]); m.gallery_commit(BASE)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_cascade_eligible(lats, lh, masks, 3)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_cascade_subset(sh, hr, 3)                                  # a subset from before the edit
    idx = np.array([BASE + 13, BASE + 2, BASE + 11, BASE + 5], np.int64)
    sh2 = m.subset_create(idx)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_cascade_subset(sh2, h, 3)                                  # a plain handle from before the edit
    sref = m.search_subset_resident(sh2, hr, k=0, want_scores=True, want_parts=True)
    nm, nt = counts(lats)
    for keep in (3, 4):
        same(m.search_cascade_subset(sh2, hr, keep), EM.expected_subset(sref["scores"], sref["parts"], nm, nt, idx, keep), ("reserved handle", keep))
    lab2 = labels5(14)
    lh2 = m.labels_create(lab2)
    ref = reference(m, hr)
    check(m, lats, lh2, lab2, masks, ref, 3, what="after the commit")
    m.close()
    # no gallery
    m2 = M.Matcher(codebook_bytes)
    m2.gallery_commit(BASE)
    lh0 = m2.labels_create(np.zeros(0, np.uint64))
    out = m2.search_cascade_eligible(lats, lh0, masks, 4)
    assert out["scores"].shape == (3, 0) and out["n_kept"].tolist() == [0, 0, 0] and (out["kept_idx"] == -1).all() and not out["kept_parts"].any()
    m2.close()


# ---- 7: the mapped kernels on planted tables ----------------------------------------------------------------------------------------------------------------
def pieces_of(q_slot, q_first, per_launch):
    """csrc/cascade_tables.h: a piece is the part of one launch group's slots that lies in one chunk of per_launch slots -> [(first, n, group)] in slot order."""
    out = []
    for g in range(len(q_first) - 1):
        a, g1 = int(q_slot[q_first[g]]), int(q_slot[q_first[g + 1]])
        while a < g1:
            b = min((a // per_launch + 1) * per_launch, g1)
            out.append((a, b - a, g))
            a = b
    return out


def run_mapped(m, G_res, sel, keep, n_kept, kept, has, q_first, per_launch, row_of, out_col, out_shape, base=BASE, seed=5):
    """The tap against the tables and the matrix written out here."""
    rng = np.random.default_rng(seed)
    kept = np.asarray(kept, np.int64); n_q = kept.shape[0]
    sub = np.arange(G_res) if sel is None else np.asarray(sel)
    mm = len(sub)
    inv = np.full(G_res, -1, np.int64); inv[sub] = np.arange(mm)
    q_slot = np.concatenate([[0], np.cumsum([n_kept if x else 0 for x in has])]).astype(np.int64)
    total = int(q_slot[-1])
    parts = rng.integers(0, 1 << 32, (n_q, mm, 4), dtype=np.uint64).astype(np.uint32)       # words, not numbers
    pair_score = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    out0 = rng.integers(0, 1 << 32, out_shape, dtype=np.uint64).astype(np.uint32)
    pcs = pieces_of(q_slot, q_first, per_launch)
    tab_ints = 2 * total + len(pcs) + 3
    got = m.debug_kept_cells_mapped(G_res, mm, keep, n_kept, base, kept, has, q_first, per_launch, sel, parts, pair_score, row_of, out_col, out0, tab_ints)
    # the model
    def template(q, r):
        t = int(kept[q, r]) - base
        return int(inv[t]) if 0 <= t < G_res else -1
    tab = np.full(tab_ints, -7, np.int32); pp = np.full((total, 4), 0xA5A5A5A5, np.uint32); out = out0.copy()
    for i, (first, n, g) in enumerate(pcs):
        tab[2 * first + i] = n
        for p in range(n):
            s = first + p
            q = int(np.searchsorted(q_slot, s, side="right") - 1)
            gi = template(q, s - int(q_slot[q]))
            tab[2 * first + i + 1 + 2 * p] = q - q_first[g]
            tab[2 * first + i + 2 + 2 * p] = max(gi, 0)
            pp[s] = (parts[q, gi, 0], parts[q, gi, 1], parts[q, gi, 2], 0) if gi >= 0 else (0, 0, 0, 0)
    for q in range(n_q):
        for r in range(n_kept):
            gi = template(q, r)
            if gi >= 0:
                row = q if row_of is None else int(row_of[q]); col = gi if out_col is None else int(out_col[gi])
                out[row, col] = pair_score[q_slot[q] + r] if has[q] else CM.MINUS_ONE
    assert got["n_pieces"] == len(pcs)
    assert np.array_equal(got["tab"], tab), np.argwhere(got["tab"] != tab)[:8].tolist()
    assert np.array_equal(got["pair_parts"], pp), np.argwhere(got["pair_parts"] != pp)[:8].tolist()
    assert np.array_equal(got["out"], out), np.argwhere(got["out"] != out)[:8].tolist()
    return pcs


def test_the_mapped_kernels_on_planted_tables(codebook_bytes):
    m = M.Matcher(codebook_bytes, taps=True)
    b = BASE
    # 1 query x 1 kept, a resident shard of one template, identity tables
    run_mapped(m, 1, None, 1, 1, [[b]], [1], [0, 1], 16384, None, None, (1, 1))
    # sub-shards of 1, 3 and 5 columns of a resident shard of 9: widths that are no multiple of 4; the middle query has no pairs; keep above n_kept
    for sel in ([4], [1, 4, 8], [0, 2, 3, 5, 8]):
        n = len(sel)
        kept = np.full((3, 6), -1, np.int64)
        for q in range(3):
            kept[q, :n] = np.roll(np.array(sel)[::-1], q) + b               # every listed template once, in another order per query
        run_mapped(m, 9, sel, 6, n, kept, [1, 0, 1], [0, 2, 3], 50, None, sel, (3, 9))
    # a list with -1 padding inside n_kept, an entry the map does not list, entries outside the shard; 2 groups, pieces cut inside a query's run (chunks of 3, runs of 5);
    # row_of out of order into a matrix with more rows than queries; out_col into a wider matrix
    sel = [0, 2, 3, 5, 8, 9, 12]
    kept = np.array([[b + 5, b + 0, b + 12, -1, -1, -1],
                     [b + 9, b + 4, b + 2, b + 13, b - 1, -1],               # 4: in the shard, not in sel; 13 and -1 + base: outside the shard
                     [b + 8, b + 3, b + 0, b + 2, b + 12, -1],
                     [b + 2, b + 3, b + 5, b + 8, b + 9, -1]], np.int64)
    pcs = run_mapped(m, 13, sel, 6, 5, kept, [1, 1, 0, 1], [0, 1, 4], 3, [2, 0, 4, 1], [20, 1, 7, 3, 11, 0, 16], (5, 21))
    assert len(pcs) == 6 and any(f % 5 != 0 for f, _, _ in pcs)               # 15 pairs: groups of 5 and 10 slots, chunks of 3 -> cuts inside the runs
    # the identity over a sub-shard that is the resident shard, rows mapped: the direct class of an eligible cascade
    run_mapped(m, 5, None, 4, 4, [[b + 4, b + 1, b + 0, b + 3], [b + 2, b + 3, b + 4, b + 0]], [1, 1], [0, 2], 16384, [3, 1], None, (4, 5))
    # more than one workgroup: 3 queries x 200 kept of a sub-shard of 300 of 700
    rng = np.random.default_rng(9)
    sel = np.sort(rng.choice(700, 300, replace=False))
    kept = np.stack([rng.permutation(sel)[:200] for _ in range(3)]).astype(np.int64) + b
    run_mapped(m, 700, sel.tolist(), 200, 200, kept, [1, 1, 1], [0, 2, 3], 256, None, sel.tolist(), (3, 700))
    m.close()
