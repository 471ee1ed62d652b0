"""Weighted search on the GPU: afis_search_weighted fuses any set of a latent's templates as a weighted sum on the device and leaves a full search's matrix.

1  the fold kernel through its parity tap against the numpy fold (tests/weighted_model.py), bit for bit;
2  end to end against the ORACLE's all-templates vectors (tie_mode 1), folded in numpy: scores, status and the -1 cells, bit for bit;
3  the matrix is a full search's: the ranking calls equal their numpy models on the expected matrix;
4  batching changes nothing; 5  the reference's selection lies within 2^-21 max(1, s) of afis_search; 6  refusals; 7  two contexts holding halves of the gallery.
"""
import importlib

import numpy as np
import pytest

import cases
import weighted_model as W
from test_gpu_rank_hits import TemplateModel, SubjectModel, assert_same
from test_gpu_reverse_search import ColumnModel, assert_same as assert_same_columns
from test_gpu_rank_positions import TemplateModel as PositionModel, assert_same as assert_same_positions
from test_gpu_case_lists import template_lists, assert_same as assert_same_cases, SUM

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")

ESTATE, EINVAL = "afis error -3", "afis error -1"
NINF = float("-inf")
BASE = 1000
SEL = (26, 2, 11)                                                           # the reference's selection, matcher.cpp:380


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1: the fold kernel through the tap ----------------------------------------------------------------------------------------------------------------
GARBAGE = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0xFFFFFFFF, 0x80000000, 0x00000001, 0xBF800000], np.uint32)


def tap_case(rng, G, n_q, with_empty_row):
    """qd / wtab / parts / empty for one launch: n_pq in {1, 2, 10, 85}, |A_t| in 0..2 (and, for the second query, past the four the kernel keeps), weights with zeros, 1e-30 against 1e30, the 2^24 cell, garbage in
    every slot that is not summed."""
    qd, wtab = [], []
    for q in range(n_q):
        n_pq = int(rng.choice([1, 2, 10, 85]))
        n_at = int(rng.integers(0, min(2, n_pq) + 1))
        if q == 1:                                                          # the kernel keeps four texture products in registers and walks the rest: 4, 5 and all
            n_pq, n_at = [(4, 4), (10, 5), (85, 85), (10, 7)][int(rng.integers(0, 4))]
        status = 1 if with_empty_row and q == n_q // 2 else 0
        if status and rng.random() < 0.5:
            n_pq = n_at = 0
        w = rng.random((n_pq, 4)).astype(np.float32) * 3
        w[rng.random((n_pq, 4)) < 0.4] = 0.0
        w[rng.random((n_pq, 4)) < 0.1] = -0.0
        w[n_at:, 3] = 0.0
        qd.append((len(wtab), n_pq, n_at, status)); wtab.extend(w.tolist())
    qd.append((len(wtab), 2, 0, 0)); wtab.extend([[1, 1, 1, 0], [1, 0, 0, 0]])        # the cell an fp32 accumulator gets wrong
    qd.append((len(wtab), 1, 1, 0)); wtab.append([1e-30, 1e-30, 0, 1e-30])              # tiny weights against huge values
    qd = np.array(qd, np.int32); wtab = np.array(wtab, np.float32)
    P = len(wtab)
    parts = (rng.random((P, G, 4)) * 50).astype(np.float32)
    parts[rng.random(parts.shape) < 0.3] = 0.0
    cell = qd[-2, 0]; parts[cell, :, :3] = (2.0 ** 24, 1, 1); parts[cell + 1, :, 0] = 1
    parts[qd[-1, 0]] = 1e30
    empty = (rng.random(G) < 0.25).astype(np.uint8)
    if G > 2:
        empty[0] = 0; empty[G - 1] = 1
    junk = GARBAGE[rng.integers(0, len(GARBAGE), parts.shape)].view(np.float32)
    unused = np.broadcast_to((wtab == 0)[:, None, :], parts.shape) | np.broadcast_to((empty != 0)[None, :, None], parts.shape)
    for q in range(len(qd)):
        if qd[q, 3]:
            unused = unused.copy(); unused[qd[q, 0]:qd[q, 0] + qd[q, 1]] = True
    parts = np.where(unused, junk, parts).astype(np.float32)
    return qd, wtab, parts, empty


@pytest.mark.parametrize("G", [1, 3, 4, 97, 260])
def test_fold_kernel_against_numpy(G, codebook_bytes):
    m = M.Matcher(codebook_bytes, taps=True)
    rng = np.random.default_rng(900 + G)
    for n_q in (1, 2, 3, 4, 5):
        qd, wtab, parts, empty = tap_case(rng, G, n_q, with_empty_row=n_q >= 3)
        want = W.fold(parts, qd, wtab, empty)
        got = m.debug_fold_templates(parts, qd, wtab, empty)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (G, n_q, np.argwhere(bits(got) != bits(want))[:6].tolist())
        live = np.flatnonzero(empty == 0)
        if len(live):
            assert (got[-2, live] == np.float32(16777220.0)).all()              # 2^24 + 1 + 1 + 1 in fp64, converted once
            assert (got[-1, live] == np.float32(3.0)).all()                     # 1e-30f x 1e30f three times
        assert (got[:, empty != 0] == -1).all() and not np.isnan(got).any()
        if n_q >= 3:
            assert (got[n_q // 2] == -1).all()
    # more queries than a grid's second dimension holds: the kernel walks them in a loop
    qd2 = np.array([[0, 2, 1, 0], [1, 1, 0, 0], [0, 0, 0, 1]], np.int32)
    wt2 = np.array([[1, 0.5, 0, 2], [0, 0.25, 3, 0]], np.float32)
    p2 = (rng.random((2, G, 4)) * 9).astype(np.float32)
    e2 = np.zeros(G, np.uint8); e2[G // 2] = 1
    n_big = 65535 + 70
    want = W.fold(p2, qd2, wt2, e2)[np.arange(n_big) % 3]
    got = m.debug_fold_templates(p2, qd2[np.arange(n_big) % 3], wt2, e2)
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(M.AfisError, match=EINVAL):
        m.debug_fold_templates(p2, [[1, 2, 0, 0]], wt2, e2)                  # pseudo-queries past the end of parts
    with pytest.raises(M.AfisError, match=EINVAL):
        m.debug_fold_templates(p2, [[0, 1, 2, 0]], wt2, e2)                  # more texture templates than pseudo-queries
    m.close()


# ---- the data of 2 - 7 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def world(cb, codebook_bytes, oracle):
    """cases.small_set (3 latents x 40 prints: mates of overlap 0.8 / 0.5 / 0.3 first) plus an empty print, one without minutiae and one without texture; latents
    of 28 + 1, 7 + 2, 4 + 0 and 0 templates, a 4 + 0 latent for the rows that select what it does not have, two more of 28 + 1 and one of 2 + 6 (more texture
    templates than the fold keeps in registers).  vec[q] [G][width]: the
    oracle's all-templates vectors (tie_mode 1), computed once."""
    lats, gal = cases.small_set(cb)
    rng = np.random.default_rng(77)
    two_tex = T.FPTemplate(minu=lats[0].minu[:7], tex=[lats[0].tex[0], S.make_latent(rng, n_tex_lo=200, n_tex_hi=260).tex[0]])
    no_tex = T.FPTemplate(minu=lats[1].minu[:4], tex=[])
    ghost = T.FPTemplate(minu=lats[2].minu[:4], tex=[])
    six_tex = T.FPTemplate(minu=lats[1].minu[:2], tex=[lats[1].tex[0], two_tex.tex[1], lats[2].tex[0], lats[0].tex[0], two_tex.tex[1], lats[1].tex[0]])
    L = [lats[0], two_tex, no_tex, T.FPTemplate(), ghost, lats[1], lats[2], six_tex]
    g = list(gal) + [T.FPTemplate(), T.FPTemplate(minu=gal[0].minu, tex=[]), T.FPTemplate(minu=[], tex=gal[1].tex)]
    dats = [T.write_rolled(r) for r in g]                                   # through the file format, as the oracle reads them
    ocb = oracle.codebook(codebook_bytes)
    hr = [oracle.rolled(d)[0] for d in dats]
    vec, empty = [], np.zeros(len(g), np.uint8)
    for q, lat in enumerate(L):
        width = len(lat.minu) + len(lat.tex)
        v = np.zeros((len(g), width), np.float32)
        if width:
            hl, _ = oracle.latent(ocb, T.write_latent(lat))
            for gi in range(len(g)):
                rc, v[gi] = oracle.all_templates(ocb, hl, hr[gi], width, tie_mode=1)
                if q == 0:
                    empty[gi] = rc == 2
                assert (rc == 2) == bool(empty[gi])
        vec.append(v)
    assert empty.sum() >= 1 and empty[:40].sum() == 0
    return {"lats": L, "dats": dats, "vec": vec, "empty": empty, "counts": [(len(x.minu), len(x.tex)) for x in L]}


def weight_sets(n_q):
    """name -> (w_minu [n_q][n_wm], w_tex [n_q][n_wt])"""
    rng = np.random.default_rng(4242)

    def rnd(n):
        w = rng.random((n_q, n)).astype(np.float32) * 2
        u = rng.random((n_q, n))
        w[u < 0.4] = 0.0; w[(u >= 0.4) & (u < 0.5)] = -0.0
        return w
    sel = np.zeros((n_q, 28), np.float32); sel[:, SEL] = 1.0
    per = rnd(28); per_t = rnd(2)
    per[4, :4] = 0.0; per[4, 4:] = 1.5; per_t[4] = 1.0                      # query 4 (4 + 0 templates): only templates it does not have
    per[0] = 0.0; per[0, 27] = 0.75; per_t[0] = (0.0, 2.0)                  # query 0: one minutiae template, a texture template it does not have
    return {"ones": (np.ones((n_q, 28), np.float32), np.full((n_q, 1), 0.3, np.float32)),
            "selection": (sel, np.full((n_q, 1), 0.3, np.float32)),
            "random": (rnd(28), rnd(2)),
            "short": (rnd(5), rnd(1)),
            "long": (rnd(40), rnd(4)),
            "per_query": (per, per_t),
            "minutiae_only": (rnd(28), np.zeros((n_q, 0), np.float32)),
            "texture_only": (np.zeros((n_q, 0), np.float32), np.array([[1.0, 0.5]] * n_q, np.float32)),
            "six_textures": (rnd(28), np.array([[0.3, 1.0, 0.5, 2.0, 0.25, 0.125]] * n_q, np.float32))}


def expected(world, wm, wt, cols=None):
    """The fold of the oracle's vectors in numpy.  -> (scores [n_q][G], status [n_q], cells in which two or more active templates score > 0)"""
    rows, status, multi = [], [], 0
    empty = world["empty"]
    for q, (n_minu, n_tex) in enumerate(world["counts"]):
        row, st = W.fold_vectors(world["vec"][q], n_minu, wm[q], wt[q], empty)
        rows.append(row); status.append(st)
        am, at = W.active(n_minu, wm[q]), W.active(n_tex, wt[q])
        pos = (world["vec"][q][:, list(am) + [n_minu + t for t in at]] > 0).sum(axis=1)
        multi += int(((pos >= 2) & (empty == 0)).sum())
    out = np.stack(rows)
    return (out if cols is None else out[:, cols]), np.array(status, np.int32), multi


def open_matcher(cbb, dats, base=BASE, taps=False, **options):
    m = M.Matcher(cbb, taps=taps)
    for k, v in options.items():
        m.set_option(k, v)
    for d in dats:
        m.gallery_add_dat(d)
    m.gallery_commit(base)
    return m


@pytest.fixture(scope="module")
def shared(codebook_bytes, world):
    m = open_matcher(codebook_bytes, world["dats"])
    yield m
    m.close()


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_oracle(shared, world):
    m, n_q = shared, len(world["lats"])
    G = len(world["dats"])
    multi_all = {}
    for name, (wm, wt) in weight_sets(n_q).items():
        want, status, multi = expected(world, wm, wt)
        multi_all[name] = multi
        got = m.search_weighted(world["lats"], wm, wt)
        qd, spec, _ = W.plan(world["counts"], wm, wt)
        print(f"{name}: {n_q} x {G}: pseudo-queries {m.get_option('weighted_pseudo_queries')}, fold {m.get_option('weighted_fold_us')} us, "
              f"cells with two or more positive templates {multi}, total_ms {m.timing()['total_ms']:.3f}")
        assert got["scores"].shape == (n_q, G)
        assert np.array_equal(got["status"], status), (name, got["status"], status)
        assert np.array_equal(bits(got["scores"]), bits(want)), (name, np.argwhere(bits(got["scores"]) != bits(want))[:8].tolist())
        assert np.array_equal(got["scores"] == -1, (world["empty"][None, :] != 0) | (status[:, None] != 0)), name
        assert m.get_option("weighted_pseudo_queries") == len(spec) and m.timing()["pairs"] == len(spec) * G, name
        assert status[3] == W.LATENT_EMPTY
    assert multi_all["ones"] >= 10 and multi_all["random"] >= 10 and multi_all["long"] >= 10      # otherwise the accumulation order is never exercised
    _, status, _ = expected(world, *weight_sets(n_q)["per_query"])
    assert status[4] == W.LATENT_EMPTY and status[0] == 0


def test_options_change_the_scorers_not_the_rule(codebook_bytes, world):
    """adc_variant 8 and the tie orders: v is what afis_match_all_templates gives under the same options, folded by the same rule."""
    sub = {"lats": world["lats"][:3], "counts": world["counts"][:3], "empty": world["empty"]}
    wm, wt = (w[:3] for w in weight_sets(len(world["lats"]))["random"])
    for opts in ({"adc_variant": 8}, {"ref_tie_order": 2}):
        m = open_matcher(codebook_bytes, world["dats"], **opts)
        vec = []
        for lat in sub["lats"]:
            qs, rs, sc = m.One2One_matching_all_templates(lat)
            assert np.array_equal(rs == 2, world["empty"] != 0)
            vec.append(sc)
        want, status, _ = expected(dict(sub, vec=vec), wm, wt)
        got = m.search_weighted(sub["lats"], wm, wt)
        assert np.array_equal(bits(got["scores"]), bits(want)) and np.array_equal(got["status"], status), opts
        m.close()


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_is_a_full_search(shared, world):
    m, lats = shared, world["lats"]
    n_q, G = len(lats), len(world["dats"])
    wm, wt = weight_sets(n_q)["random"]
    want, _, _ = expected(world, wm, wt)
    glob = np.arange(G, dtype=np.int64) + BASE
    subject = (np.arange(G) // 3).astype(np.int64) * 5 + 2
    sh = m.subjects_create(subject)
    qh = m.upload_queries(lats)                                             # before the search: an upload queues device work
    m.search_weighted(lats, wm, wt, want_scores=False)
    tm = TemplateModel(want, glob)
    assert_same(m.rank_hits(NINF, 8), tm.hits(NINF, 8), "rank_hits")
    assert_same(m.rank_hits(0.5, 43), tm.hits(0.5, 43), "rank_hits 0.5")
    sm = SubjectModel(want, glob, subject)
    assert_same(m.rank_subject_hits(sh, NINF, 6), sm.hits(NINF, 6), "rank_subject_hits")
    top = m.rank_subjects(sh, n_q, 3)
    assert np.array_equal(top["subject"], sm.hits(NINF, 3)["subject"]) and np.array_equal(bits(top["score"]), sm.hits(NINF, 3)["score"])
    assert_same_columns(m.rank_latent_hits(NINF, 4, latent_base=50), ColumnModel(want).hits(NINF, 4, 50), "rank_latent_hits")
    query = np.repeat(np.arange(n_q, dtype=np.int32), G); idx = np.tile(glob, n_q)
    assert_same_positions(m.rank_positions(query, idx), PositionModel(want, glob).answer(query, idx), "rank_positions")
    case_of = [0, 0, 1, 1, 2, 2, 2, 1]
    lists, _ = template_lists(want, case_of, SUM, glob)
    assert_same_cases(m.rank_case_hits(case_of, SUM, NINF, 10), lists.hits(NINF, 10), "rank_case_hits SUM")
    # pair scoring in between leaves the matrix rankable (and scores afis_search's selection, not the weighted one)
    before = m.rank_hits(NINF, 8)
    res = m.score_pairs(qh, np.zeros(5, np.int32), glob[:5])
    assert (res["status"] == M.PAIR_OK).all()
    assert_same(m.rank_hits(NINF, 8), {k: (bits(v) if k == "score" else v) for k, v in before.items()}, "after score_pairs")
    with pytest.raises(M.AfisError, match=EINVAL):
        m.rank_subjects(sh, n_q + 1, 3)                                     # not the last search's n_q
    # a following search replaces it
    full = m.search_resident(qh, k=0, want_scores=True)
    assert_same(m.rank_hits(NINF, 8), TemplateModel(full["scores"], glob).hits(NINF, 8), "after afis_search")
    assert not np.array_equal(bits(full["scores"]), bits(want))
    m.free_queries(qh); m.subjects_free(sh)


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_batching_changes_nothing(codebook_bytes, world):
    m, lats = open_matcher(codebook_bytes, world["dats"]), world["lats"]
    n_q, G = len(lats), len(world["dats"])
    wm, wt = weight_sets(n_q)["long"]
    want, status, _ = expected(world, wm, wt)
    qd, spec, _ = W.plan(world["counts"], wm, wt)
    assert len(spec) > 3 * 3 and qd[:, 1].max() > 3                         # several batches at cap 3, and a query larger than the cap
    seen = []
    for cap in (1, 3, 0):
        m.set_option("weighted_batch_pseudo", cap)
        assert m.get_option("weighted_batch_pseudo") == cap
        got = m.search_weighted(lats, wm, wt)
        tm = m.timing()
        print(f"weighted_batch_pseudo {cap}: batches {len(W.batches(qd, cap or 1 << 30))}, launch groups {tm['launch_groups']}, pairs {tm['pairs']}, total_ms {tm['total_ms']:.3f}")
        assert np.array_equal(bits(got["scores"]), bits(want)) and np.array_equal(got["status"], status), cap
        assert m.get_option("weighted_pseudo_queries") == len(spec) and tm["pairs"] == len(spec) * G, cap
        if cap:
            assert tm["launch_groups"] >= len([b for b in W.batches(qd, cap) if qd[b[0]:b[1], 1].sum() > 0])
        seen.append(bits(got["scores"]).copy())
        assert_same(m.rank_hits(NINF, 5), TemplateModel(want, np.arange(G, dtype=np.int64) + BASE).hits(NINF, 5), f"cap {cap}")
    assert all(np.array_equal(seen[0], s) for s in seen[1:])
    with pytest.raises(M.AfisError, match=EINVAL):
        m.set_option("weighted_batch_pseudo", -1)
    m.close()


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_reference_selection_against_afis_search(shared, world):
    """|weighted - afis_search| <= 2^-21 max(1, s): afis_search adds the three minutiae scores in fp32 (two roundings of partial sums, each <= 2^-24 s) and 0.3 x
    texture in fp64 before its final rounding (2^-24 s); the weighted sum rounds once (2^-24 s) and multiplies by 0.3f, which differs from 0.3 by 2^-25.4 relative:
    together below 4.5 x 2^-24 s < 2^-21 s."""
    m = shared
    lats = [world["lats"][i] for i in (0, 5, 6)]                            # the 28 + 1 latents
    sel = np.zeros(28, np.float32); sel[list(SEL)] = 1.0
    full = m.search(lats, k=0, want_scores=True)["scores"]
    got = m.search_weighted(lats, sel, np.array([0.3], np.float32))["scores"]
    assert np.array_equal(full == -1, got == -1) and (full == -1).any()
    diff = np.abs(got.astype(np.float64) - full.astype(np.float64))
    bound = 2.0 ** -21 * np.maximum(1.0, full.astype(np.float64))
    print(f"selection: max |weighted - search| {diff.max():.3e} at score {full.ravel()[diff.argmax()]:.4f}; cells differing {int((bits(got) != bits(full)).sum())} of {got.size}, max score {full.max():.3f}")
    assert (diff <= bound).all(), np.argwhere(diff > bound)[:6].tolist()
    assert full.max() > 1


# ---- 6 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(codebook_bytes, world):
    m, lats = open_matcher(codebook_bytes, world["dats"][:6]), world["lats"][:2]
    one = np.ones((2, 3), np.float32); tex = np.full((2, 1), 0.3, np.float32)

    def refused(code, *args, **kw):
        m.search(lats, k=0)                                                 # a matrix to lose
        assert m.rank_hits(NINF, 2)["n_hits"].tolist() == [6, 6]
        with pytest.raises(M.AfisError, match=code):
            m.search_weighted(*args, **kw)
        with pytest.raises(M.AfisError, match=ESTATE):                      # after any return other than AFIS_OK the last-search matrix is invalid
            m.rank_hits(NINF, 2)
        assert m.get_option("weighted_pseudo_queries") == 0 and m.get_option("weighted_fold_us") == 0
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-45):
        w = one.copy(); w[1, 2] = bad
        refused(EINVAL, lats, w, tex)
        t = tex.copy(); t[0, 0] = bad
        refused(EINVAL, lats, one, t)
    w = np.ones((2, 40), np.float32); w[1, 39] = np.nan
    refused(EINVAL, lats, w, tex)                                           # a NaN at a template no query has is refused all the same
    refused(EINVAL, lats, one, tex, n_wm=-1)
    refused(EINVAL, lats, one, tex, n_wt=-1)
    refused(EINVAL, lats, None, tex, n_wm=3)                                # a null array whose width is > 0
    refused(EINVAL, lats, one, None, n_wt=1)
    assert m.lib.afis_search_weighted(None, None, 0, None, 0, None, 0, None, None) == -1
    assert m.lib.afis_search_weighted(m.ctx, None, 2, None, 0, None, 0, None, None) == -1     # n_q > 0 with queries NULL
    assert m.lib.afis_search_weighted(m.ctx, None, -1, None, 0, None, 0, None, None) == -1
    # -0.0 is a zero, widths of 0 are fine: every row latent-empty
    r = m.search_weighted(lats, np.full((2, 3), -0.0, np.float32), None)
    assert (r["status"] == W.LATENT_EMPTY).all() and (r["scores"] == -1).all() and m.get_option("weighted_pseudo_queries") == 0
    assert m.rank_hits(NINF, 2)["n_hits"].tolist() == [6, 6] and m.timing()["pairs"] == 0
    # no query: AFIS_OK, as afis_search with none
    r = m.search_weighted([], one[:0], tex[:0])
    assert r["scores"].shape == (0, 6) and len(r["status"]) == 0
    m.close()
    fresh = M.Matcher(codebook_bytes)
    for d in world["dats"][:3]:
        fresh.gallery_add_dat(d)
    with pytest.raises(M.AfisError, match=ESTATE):                          # before the first commit
        fresh.search_weighted(lats, one, tex)
    fresh.close()


def test_only_active_views_are_validated(codebook_bytes, world):
    """A bad view of a template that no weight selects costs nothing; of an active one it is AFIS_EINVAL from the middle of the call, which then holds nothing."""
    m, lats = open_matcher(codebook_bytes, world["dats"][:6]), world["lats"][:2]
    v = M._Views(lats)
    v.arr[0].minu[1].des_len = 95                                           # minutiae template 1 of query 0
    v.arr[1].tex[1].n = 0                                                   # texture template 1 of query 1 (7 + 2 templates)

    def call(wm, wt):
        wm, wt = np.ascontiguousarray(wm, np.float32), np.ascontiguousarray(wt, np.float32)
        sc = np.empty((2, 6), np.float32); st = np.zeros(2, np.int32)
        rc = m.lib.afis_search_weighted(m.ctx, v.arr, 2, M._ptr(wm, M.C.c_float), wm.shape[1], M._ptr(wt, M.C.c_float), wt.shape[1], M._ptr(sc, M.C.c_float), M._ptr(st, M.C.c_int32))
        return rc, sc
    wm = np.ones((2, 3), np.float32); wm[0, 1] = 0.0
    wt = np.array([[0.3, 0.0], [0.3, -0.0]], np.float32)
    rc, sc = call(wm, wt)
    assert rc == 0 and np.array_equal(bits(sc), bits(m.search_weighted(lats, wm, wt)["scores"]))
    for bad_m, bad_t in ((1.0, 0.0), (0.0, 0.5)):
        m.search(lats, k=0)
        w2, t2 = wm.copy(), wt.copy()
        w2[0, 1] = bad_m; t2[1, 1] = bad_t
        rc, _ = call(w2, t2)
        assert rc == -1, (bad_m, bad_t, rc)
        with pytest.raises(M.AfisError, match=ESTATE):
            m.rank_hits(NINF, 2, n_q=2)
        assert m.get_option("weighted_pseudo_queries") == 0
    rc, sc2 = call(wm, wt)                                                  # ... and the context goes on
    assert rc == 0 and np.array_equal(bits(sc2), bits(sc))
    m.close()


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_contexts_holding_halves(codebook_bytes, world):
    lats, dats = world["lats"], world["dats"]
    n_q, G, cut, cap = len(lats), len(world["dats"]), 23, 12
    wm, wt = weight_sets(n_q)["ones"]
    whole = open_matcher(codebook_bytes, dats, base=0)
    whole.search_weighted(lats, wm, wt, want_scores=False)
    halves = [open_matcher(codebook_bytes, dats[:cut], base=0), open_matcher(codebook_bytes, dats[cut:], base=cut)]
    want_m, _, _ = expected(world, wm, wt)
    for thr in (NINF, 0.25):
        one = whole.rank_hits(thr, cap)
        per = []
        for h, cols in zip(halves, (slice(0, cut), slice(cut, G))):
            r = h.search_weighted(lats, wm, wt)
            assert np.array_equal(bits(r["scores"]), bits(want_m[:, cols]))
            per.append(h.rank_hits(thr, cap))
        n, i, s = SH.merge_hits(np.stack([p["n_hits"] for p in per]), np.stack([p["idx"] for p in per]), np.stack([p["score"] for p in per]), cap)
        assert np.array_equal(n, one["n_hits"]) and np.array_equal(i, one["idx"]) and np.array_equal(bits(s), bits(one["score"])), thr
        assert_same(one, TemplateModel(want_m, np.arange(G, dtype=np.int64)).hits(thr, cap), f"one context {thr}")
    for m in [whole] + halves:
        m.close()
