"""Print pairs on the GPU: afis_score_print_pairs and afis_correspondences_print_pairs, the pair forms for resident print pairs.  Every comparison is exact, on uint32 /
int16 views.

1  all 400 pairs of the print-search gallery against afis_search_prints' cells, the parts against afis_match_all_templates of the prints' views;
2  about 40 pairs against the ORACLE's all-templates vectors folded in numpy (tie_mode 1), pair by pair;
3  130 pairs of ONE query print; 4  the options that change the scorers; 5  the correspondences against afis_correspondences_pairs over the 27-template views and,
for the planted second impressions and the self pairs, against the oracle's stage-2 trace; 6  the last search's matrix stays; 7  coverage; 8  refusals;
9  after a removal and an appending commit.

The gallery is tests/test_gpu_print_search.py's: 20 prints at index_base 7000 (1 / 15 / 16 / 17 / 129 minutiae, 1 .. 1100 -> 1000 texture points, no minutiae, no
texture, empty, removed, four appended prints)."""
import importlib

import numpy as np
import pytest

import print_pairs_model as PM
import weighted_model as W
from test_gpu_print_search import BASE, BIG, COUNTS, EMPTY, G, NO_MINU, NO_TEX, REMOVED, WEIGHTS, World, make_prints, open_matcher

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

ESTATE, EINVAL = "afis error -3", "afis error -1"
NINF = float("-inf")
NINF_BITS, M1_BITS = 0xff800000, 0xbf800000
assert len(COUNTS) == G == 20


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pair_weights(n):
    """The four weight pairs cycle per pair."""
    return np.array([WEIGHTS[i % 4][0] for i in range(n)], np.float32), np.array([WEIGHTS[i % 4][1] for i in range(n)], np.float32)


@pytest.fixture(scope="module")
def world(oracle):
    return World("shipped", oracle)


@pytest.fixture(scope="module")
def shared(world):
    m = open_matcher(world.cbb, world.enrolled)
    yield m
    m.close()


@pytest.fixture(scope="module")
def matrices(shared, world):
    """search_prints of all 20 prints once per weight pair: [4][G][G], the yardstick of tests 1 and 3."""
    idx = np.arange(G, dtype=np.int64) + BASE
    return np.stack([shared.search_prints(idx, WEIGHTS[k][0], WEIGHTS[k][1])["scores"] for k in range(4)])


def expected_parts(m, world, a, b, wm, wt):
    """(v_m if active else +0, v_t if active else +0) from afis_match_all_templates of the print's view; +0 twice where the score is the -1."""
    vec = {}
    out = np.zeros((len(a), 2), np.float32)
    for i, (qa, qb) in enumerate(zip(a, b)):
        nm, nt = world.counts[qa]
        am, at = nm > 0 and wm[i] != 0, nt > 0 and wt[i] != 0
        if world.empty[qb] or not (am or at):
            continue
        if qa not in vec:
            vec[qa] = m.One2One_matching_all_templates(world.views[qa])[2]
        v = vec[qa][qb]
        out[i] = (v[0] if am else 0.0, v[nm] if at else 0.0)
    return out


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_all_400_pairs_against_the_print_search(shared, world, matrices):
    m = shared
    rng = np.random.default_rng(31)
    order = rng.permutation(G * G)
    order = np.concatenate([order, rng.choice(order, 10, replace=False)])
    a, b = order // G, order % G
    wm, wt = pair_weights(len(order))
    for k, v in (("score_pairs_per_launch", 50), ("print_pairs_batch_prints", 3), ("query_batch", 2)):
        m.set_option(k, v)
    try:
        got = m.score_print_pairs(a + BASE, b + BASE, wm, wt, want_parts=True)
        n_prints, us = m.get_option("print_pairs_query_prints"), m.get_option("print_pairs_us")
    finally:
        for k, v in (("score_pairs_per_launch", 8192), ("print_pairs_batch_prints", 0), ("query_batch", 0)):
            m.set_option(k, v)
    assert (got["status"] == M.PAIR_OK).all()
    want = matrices[np.arange(len(order)) % 4, a, b]
    assert np.array_equal(bits(got["score"]), bits(want)), np.flatnonzero(bits(got["score"]) != bits(want))[:8].tolist()
    parts = expected_parts(m, world, a, b, wm, wt)
    assert np.array_equal(bits(got["parts"]), bits(parts)), np.argwhere(bits(got["parts"]) != bits(parts))[:8].tolist()
    assert (want > 0).sum() >= 10 and (bits(want) == M1_BITS).sum() >= 100  # the yardstick holds both kinds of cell: scored ones, and the -1 of an empty side or of weights (0, 0)
    for i in range(len(order) - 10, len(order)):                            # a repeated pair under ITS weights: the first occurrence's bytes where the weights agree
        j = int(np.flatnonzero(order[:len(order) - 10] == order[i])[0])
        if i % 4 == j % 4:
            assert got["score"][i].tobytes() == got["score"][j].tobytes() and got["parts"][i].tobytes() == got["parts"][j].tobytes()
    active = {int(qa) for i, qa in enumerate(a) if (world.counts[qa][0] > 0 and wm[i] != 0) or (world.counts[qa][1] > 0 and wt[i] != 0)}
    assert n_prints == len(active) == G - 2 and us > 0
    model = PM.plan(a + BASE, b + BASE, BASE, world.counts, wm != 0, wt != 0, cap=3)
    assert len(model["prints"]) == n_prints and len(model["batches"]) == 6
    # identical pairs with identical weights give identical bytes, wherever they stand in the list
    twice = m.score_print_pairs(np.tile(a[:40], 2) + BASE, np.tile(b[:40], 2) + BASE, np.tile(wm[:40], 2), np.tile(wt[:40], 2), want_parts=True)
    assert twice["score"][:40].tobytes() == twice["score"][40:].tobytes() == got["score"][:40].tobytes() and twice["parts"][:40].tobytes() == twice["parts"][40:].tobytes()


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------------------------
def oracle_pair(world, qa, qb, w_m, w_t):
    """The oracle's all-templates vector of print qa's view against print qb (World.vec's route for one column), folded: the score of the pair."""
    nm, nt = world.counts[qa]
    if nm + nt == 0:
        return np.float32(-1.0)
    src = world.views[qa] if nm else T.FPTemplate(minu=[world._stand_in], tex=world.views[qa].tex)
    key = ("latent", qa)
    if key not in world._vec:
        world._vec[key] = world.oracle.latent(world.ocb, T.write_latent(src))[0]
    rc, full = world.oracle.all_templates(world.ocb, world._vec[key], world.hr[qb], len(src.minu) + nt, tie_mode=1)
    assert (rc == 2) == bool(world.empty[qb])
    v = np.array(full if nm else full[1:], np.float32)
    if nm and qb == NO_MINU:
        v[0] = 0.0                                                          # the zero the matcher leaves for a print without a minutiae template
    row, _ = W.fold_vectors(v[None, :], nm, np.array([w_m], np.float32), np.array([w_t], np.float32), world.empty[[qb]])
    return row[0]


def test_against_the_oracle_directly(shared, world):
    edge = [NO_MINU, NO_TEX, EMPTY, REMOVED]
    pairs = [(x, y) for x in edge for y in (0, 5, 13)] + [(x, y) for y in edge for x in (1, 4, 17)] + [(x, x) for x in (0, 2, 5, 7, NO_MINU, NO_TEX, EMPTY, 13, 16, 19)]
    pairs += [(3, 6), (6, 3), (15, 18), (19, 1), (14, 7), (NO_MINU, NO_TEX), (NO_TEX, NO_MINU), (EMPTY, REMOVED)]
    assert 38 <= len(pairs) <= 44
    a = np.array([p[0] for p in pairs]); b = np.array([p[1] for p in pairs])
    wm, wt = pair_weights(len(pairs))
    wm[:24:2] = 1.0; wt[:24:2] = np.float32(0.3)                            # the edge prints under full weights as well
    got = shared.score_print_pairs(a + BASE, b + BASE, wm, wt)
    want = np.array([oracle_pair(world, int(x), int(y), wm[i], wt[i]) for i, (x, y) in enumerate(pairs)], np.float32)
    assert (got["status"] == M.PAIR_OK).all()
    assert np.array_equal(bits(got["score"]), bits(want)), [(pairs[i], got["score"][i], want[i]) for i in np.flatnonzero(bits(got["score"]) != bits(want))[:8]]
    assert (want > 0).sum() >= 6 and (want == -1).sum() >= 10       # (non-mated synthetic prints score 0: the positive cells are the self pairs)


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_130_pairs_of_one_query_print(shared, matrices):
    m = shared
    b = np.arange(130) % G
    a = np.full(130, BIG)
    row = matrices[0][BIG]
    for cap in (0, 1):
        m.set_option("print_pairs_batch_prints", cap)
        got = m.score_print_pairs(a + BASE, b + BASE, WEIGHTS[0][0], WEIGHTS[0][1], want_parts=True)
        assert np.array_equal(bits(got["score"]), bits(row[b])), cap
        assert m.get_option("print_pairs_query_prints") == 1
        for j in range(G, 130):
            assert got["parts"][j].tobytes() == got["parts"][j - G].tobytes()
    m.set_option("print_pairs_batch_prints", 0)
    assert row[BIG] > 0


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{"s3_tie_order": 1}, {"ref_tie_order": 2}, {"adc_variant": 8}], ids=["s3_tie_order_1", "ref_tie_order_2", "adc_variant_8"])
def test_under_the_options_that_change_the_scorers(world, opts):
    m = open_matcher(world.cbb, world.enrolled, **opts)
    loc = np.array([BIG, 5, NO_MINU, NO_TEX, 13, 17, 0, 3])
    full = m.search_prints(loc + BASE, 1.0, np.float32(0.3))["scores"]
    rng = np.random.default_rng(5)
    qi = rng.integers(0, len(loc), 60); b = rng.integers(0, G, 60)
    got = m.score_print_pairs(loc[qi] + BASE, b + BASE, 1.0, np.float32(0.3))
    assert np.array_equal(bits(got["score"]), bits(full[qi, b])), opts
    m.close()


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------------------------
def second_impression(p, dx, dy, drop_every):
    """A copy of print p's minutiae template with shifted coordinates and every drop_every-th minutia dropped; its texture template as it is."""
    mt = p.minu[0]
    keep = np.flatnonzero(np.arange(mt.n) % drop_every != drop_every - 1)
    return T.FPTemplate(minu=[T.MinutiaeTemplate((mt.x[keep] + dx).astype(np.int16), (mt.y[keep] + dy).astype(np.int16), mt.ori[keep].copy(), mt.des[keep].copy())], tex=list(p.tex))


PLANTED = [(5, 12, -9, 4), (13, -20, 15, 3), (15, 7, 7, 5), (18, -5, -30, 2)]   # (print, dx, dy, drop every): prints 20 .. 23


def view27(world, mt):
    return T.FPTemplate(minu=[world._stand_in] * 26 + [mt], tex=[])


def test_correspondences_against_the_27_template_view(world):
    planted = [second_impression(world.enrolled[p], dx, dy, k) for p, dx, dy, k in PLANTED]
    prints = list(world.prints) + planted
    n_all = len(prints)
    m = open_matcher(world.cbb, world.enrolled, corr_pairs_per_launch=7, print_pairs_batch_prints=4)
    m.gallery_reopen(); m.gallery_add(planted); m.gallery_commit(BASE)
    mates = [(PLANTED[k][0], G + k) for k in range(4)] + [(G + k, PLANTED[k][0]) for k in range(4)]
    selfs = [(x, x) for x in (1, 4, 5, 7, 13, G + 1)]
    edge = [NO_MINU, NO_TEX, EMPTY, REMOVED, 0, 3]
    pairs = mates + selfs + [(x, y) for x in edge for y in edge] + [(5, 13), (G + 3, 15), (15, G), (19, 16)]
    a = np.array([p[0] for p in pairs]); b = np.array([p[1] for p in pairs])
    # ---- the yardstick from the oracle alone: the stage-2 trace of the 27-template view, for the planted pairs and the self pairs
    orc, ocb = world.oracle, world.ocb
    n_oracle, n_surv, n_partial = 0, 0, 0
    traced = {}
    for qa, qb in mates + selfs:
        hl = orc.latent(ocb, T.write_latent(view27(world, prints[qa].minu[0])))[0]
        hr = orc.rolled(T.write_rolled(prints[qb]))[0]
        _, li, ri = orc.trace(ocb, hl, hr, which=1, stage=2, tie_mode=1)
        lm, rm = prints[qa].minu[0], prints[qb].minu[0]
        traced[(qa, qb)] = np.stack([lm.x[li], lm.y[li], rm.x[ri], rm.y[ri]], axis=1).astype(np.int16) if len(li) else np.zeros((0, 4), np.int16)
        n_oracle += 1; n_surv += len(li) > 0; n_partial += 0 < len(li) < 120
    assert n_surv >= 8 and n_partial >= 1, (n_surv, n_partial)              # conditioned on the yardstick: the planted impressions were chosen for it on the CPU
    # ---- the device's own definition: afis_correspondences_pairs over the 27-template views, slot 0
    has_minu = [len(p.minu) > 0 and p.minu[0].n > 0 for p in prints]
    qa_list = sorted({int(x) for x in a if has_minu[x]})
    qh = m.upload_queries([view27(world, prints[x].minu[0]) for x in qa_list])
    sel = np.flatnonzero([has_minu[x] for x in a])
    ref = m.correspondences_pairs(qh, np.array([qa_list.index(int(a[i])) for i in sel], np.int32), b[sel] + BASE, want_parts=True)
    got = m.correspondences_print_pairs(a + BASE, b + BASE, want_parts=True)
    assert m.get_option("print_pairs_us") > 0 and m.get_option("print_pairs_query_prints") == len(qa_list)
    sc = m.score_print_pairs(a + BASE, b + BASE, 1.0, 0.0, want_parts=True)
    row_of = {int(i): k for k, i in enumerate(sel)}
    for i, (qa, qb) in enumerate(pairs):
        if not (has_minu[qa] and has_minu[qb]):
            assert got["counts"][i] == M.CORR_NOT_RUN and got["corr"][i] is None and not got["xy"][i].any() and bits(got["part"][i]) == 0, (i, qa, qb)
            continue
        k = row_of[i]
        assert got["counts"][i] == ref["counts"][k, 0] >= 0, (i, qa, qb)
        assert got["xy"][i].tobytes() == ref["xy"][k, 0].tobytes() and bits(got["part"][i]) == bits(ref["part"][k, 0]), (i, qa, qb)
        assert bits(got["part"][i]) == bits(sc["parts"][i, 0]), (i, qa, qb)   # the scorer's return value is the score call's minutiae part
        if (qa, qb) in traced:
            want = traced[(qa, qb)]
            assert got["counts"][i] == len(want) and np.array_equal(got["xy"][i, :len(want)], want) and not got["xy"][i, len(want):].any(), (i, qa, qb)
            assert np.array_equal(got["corr"][i], want)
    assert n_all == G + 4 and n_oracle == len(mates) + len(selfs)
    m.free_queries(qh)
    m.close()


# ---- 6 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_stays(shared, world):
    import cases
    m = shared
    idx = np.array([BIG, 13, 15, 18, NO_MINU, 5], np.int64) + BASE
    m.search_prints(idx, 1.0, np.float32(0.3), want_scores=False)
    before = m.rank_hits(NINF, 6)
    a = np.repeat(idx, 6); b = before["idx"].reshape(-1)                    # the operator opens the candidates: the flattened lists as they are
    s = m.score_print_pairs(a, b, 1.0, np.float32(0.3))
    c = m.correspondences_print_pairs(a, b)
    assert np.array_equal(bits(s["score"]), bits(before["score"].reshape(-1))) and (c["counts"] >= M.CORR_NOT_RUN).all()
    after = m.rank_hits(NINF, 6)
    for key in ("n_hits", "idx", "score"):
        assert before[key].tobytes() == after[key].tobytes(), key
    lat, _ = cases.small_set(world.cb, seed=9, n_lat=2, n_gal=1)
    qh = m.upload_queries(lat)
    r0 = m.search_resident(qh, k=3, want_scores=True)
    m.score_print_pairs(a, b, 1.0, 1.0); m.correspondences_print_pairs(a, b)
    hits = m.rank_hits(NINF, 4)                                             # ... the resident search's matrix is still there to rank
    assert hits["n_hits"].tolist() == [G, G]
    r1 = m.search_resident(qh, k=3, want_scores=True)
    assert bits(r0["scores"]).tobytes() == bits(r1["scores"]).tobytes() and r0["topk_idx"].tobytes() == r1["topk_idx"].tobytes()
    m.free_queries(qh)


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_coverage(world, matrices):
    m = open_matcher(world.cbb, world.enrolled)
    m.gallery_reopen(); m.gallery_add(world.enrolled[:2])                   # BASE + G and BASE + G + 1 are staged, not committed
    out = [-1, BASE - 1, BASE + G, BASE + G + 1, 13]                        # (13: a shard-local index is not a global one)
    inside = [BIG, 5, NO_MINU, 13]
    pairs = [(BASE + x, y) for x in inside for y in out] + [(y, BASE + x) for x in inside for y in out] + [(y, z) for y in out for z in out[:3]]
    cov = [(BASE + x, BASE + y) for x in inside for y in (0, 5, EMPTY, 13, BIG)]
    rng = np.random.default_rng(8)
    both = pairs + cov
    order = rng.permutation(len(both))
    a = np.array([both[i][0] for i in order], np.int64); b = np.array([both[i][1] for i in order], np.int64)
    is_cov = order >= len(pairs)
    assert np.array_equal(PM.covered(a, b, BASE, G), is_cov)
    s = m.score_print_pairs(a, b, 1.0, np.float32(0.3), want_parts=True)
    c = m.correspondences_print_pairs(a, b, want_parts=True)
    assert np.array_equal(s["status"] == M.PAIR_NOT_COVERED, ~is_cov) and (bits(s["score"][~is_cov]) == NINF_BITS).all() and not bits(s["parts"][~is_cov]).any()
    assert (c["counts"][~is_cov] == M.CORR_NOT_COVERED).all() and not c["xy"][~is_cov].any() and not bits(c["part"][~is_cov]).any()
    assert all(c["corr"][i] is M.NOT_COVERED for i in np.flatnonzero(~is_cov))
    # the covered pairs in the same list are unaffected: the bytes of a call that holds them alone
    alone_s = m.score_print_pairs(a[is_cov], b[is_cov], 1.0, np.float32(0.3), want_parts=True)
    alone_c = m.correspondences_print_pairs(a[is_cov], b[is_cov], want_parts=True)
    assert s["score"][is_cov].tobytes() == alone_s["score"].tobytes() and s["parts"][is_cov].tobytes() == alone_s["parts"].tobytes() and (alone_s["status"] == M.PAIR_OK).all()
    assert c["counts"][is_cov].tobytes() == alone_c["counts"].tobytes() and c["xy"][is_cov].tobytes() == alone_c["xy"].tobytes() and c["part"][is_cov].tobytes() == alone_c["part"].tobytes()
    assert np.array_equal(bits(s["score"][is_cov]), bits(matrices[0][a[is_cov] - BASE, b[is_cov] - BASE]))
    assert (c["counts"][is_cov] > 0).sum() >= 3                            # the three self pairs at least
    # nothing covered at all: AFIS_OK, nothing queued
    none = m.score_print_pairs(a[~is_cov], b[~is_cov], 1.0, 1.0)
    assert (none["status"] == M.PAIR_NOT_COVERED).all() and m.get_option("print_pairs_us") == 0 and m.get_option("print_pairs_query_prints") == 0
    m.close()


# ---- 8 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(world):
    C = M.C
    m = open_matcher(world.cbb, world.enrolled)
    a = np.array([BIG, 13], np.int64) + BASE; b = np.array([5, 13], np.int64) + BASE
    one = np.ones(2, np.float32)
    m.search_prints(a, one, one, want_scores=False)                          # a matrix that must survive every refusal
    kept = m.rank_hits(NINF, 3)

    def outputs():
        return (np.full(2, 77, np.int32), np.full(2, 5.5, np.float32), np.full((2, 2), 6.5, np.float32), np.full(2, 78, np.int32), np.full((2, 120, 4), 79, np.int16),
                np.full(2, 7.5, np.float32))

    def untouched(o):
        ref = outputs()
        return all(x.tobytes() == y.tobytes() for x, y in zip(o, ref))

    def score(n, pa, pb, pm, pt, o, ctx=None, status=True, sc=True):
        return m.lib.afis_score_print_pairs(m.ctx if ctx is None else ctx, n, pa, pb, pm, pt, M._ptr(o[0], C.c_int32) if status else None,
                                            M._ptr(o[1], C.c_float) if sc else None, M._ptr(o[2], C.c_float))

    def corr(n, pa, pb, o, counts=True, xy=True):
        return m.lib.afis_correspondences_print_pairs(m.ctx, n, pa, pb, M._ptr(o[3], C.c_int32) if counts else None, M._ptr(o[4], C.c_int16) if xy else None, M._ptr(o[5], C.c_float))
    pa, pb, pw = M._ptr(a, C.c_int64), M._ptr(b, C.c_int64), M._ptr(one, C.c_float)
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-45):
        for side in (0, 1):
            w = one.copy(); w[1] = bad
            o = outputs()
            args = (M._ptr(w, C.c_float), pw) if side == 0 else (pw, M._ptr(w, C.c_float))
            assert score(2, pa, pb, *args, o) == -1 and untouched(o), (bad, side)
            assert m.get_option("print_pairs_us") == 0 and m.get_option("print_pairs_query_prints") == 0
    o = outputs()
    assert score(2, None, pb, pw, pw, o) == -1 and score(2, pa, None, pw, pw, o) == -1 and score(2, pa, pb, None, pw, o) == -1 and score(2, pa, pb, pw, None, o) == -1
    assert score(2, pa, pb, pw, pw, o, status=False) == -1 and score(2, pa, pb, pw, pw, o, sc=False) == -1 and score(-1, pa, pb, pw, pw, o) == -1
    assert m.lib.afis_score_print_pairs(None, 2, pa, pb, pw, pw, M._ptr(o[0], C.c_int32), M._ptr(o[1], C.c_float), None) == -1
    assert corr(2, None, pb, o) == -1 and corr(2, pa, None, o) == -1 and corr(2, pa, pb, o, counts=False) == -1 and corr(2, pa, pb, o, xy=False) == -1 and corr(-1, pa, pb, o) == -1
    assert m.lib.afis_correspondences_print_pairs(None, 2, pa, pb, M._ptr(o[3], C.c_int32), M._ptr(o[4], C.c_int16), None) == -1
    assert untouched(o)
    # -0.0f is a zero, not a refusal
    zero = m.score_print_pairs(a, b, np.float32(-0.0), 1.0, want_parts=True)
    plain = m.score_print_pairs(a, b, 0.0, 1.0, want_parts=True)
    assert zero["score"].tobytes() == plain["score"].tobytes() and zero["parts"].tobytes() == plain["parts"].tobytes() and not bits(zero["parts"][:, 0]).any()
    # no pair: AFIS_OK, both read-only options 0, the outputs untouched
    m.score_print_pairs(a, b, 1.0, 1.0)
    assert m.get_option("print_pairs_us") > 0 and m.get_option("print_pairs_query_prints") == 2
    o = outputs()
    assert score(0, None, None, None, None, o) == 0 and corr(0, None, None, o) == 0 and untouched(o)
    assert m.get_option("print_pairs_us") == 0 and m.get_option("print_pairs_query_prints") == 0
    # the context is usable afterwards, and the matrix survived all of it
    again = m.rank_hits(NINF, 3)
    assert all(kept[k].tobytes() == again[k].tobytes() for k in ("n_hits", "idx", "score"))
    ok = m.score_print_pairs(a, b, 1.0, 1.0)
    assert (ok["status"] == M.PAIR_OK).all() and ok["score"][1] > 0
    for k in (-1, 1 << 31):
        with pytest.raises(M.AfisError, match=EINVAL):
            m.set_option("print_pairs_batch_prints", k)
    with pytest.raises(M.AfisError):
        m.set_option("print_pairs_us", 1)                                    # read-only
    m.close()
    fresh = M.Matcher(world.cbb)
    fresh.gallery_add(world.enrolled[:3])
    with pytest.raises(M.AfisError, match=ESTATE):                          # before the first commit
        fresh.score_print_pairs([0], [1], 1.0, 1.0)
    with pytest.raises(M.AfisError, match=ESTATE):
        fresh.correspondences_print_pairs([0], [1])
    fresh.close()


# ---- 9 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_after_a_removal_and_an_appending_commit(world):
    m = open_matcher(world.cbb, world.enrolled)
    a = np.array([5, 5, 13, 0, 13], np.int64) + BASE; b = np.array([13, 5, 0, 13, G], np.int64) + BASE
    first = m.score_print_pairs(a, b, 1.0, np.float32(0.3))
    assert first["status"].tolist() == [0, 0, 0, 0, 1]                      # BASE + G is not there yet
    m.gallery_remove([BASE + 5])
    m.gallery_reopen(); m.gallery_add(world.enrolled[13:14]); m.gallery_commit(BASE)     # a second copy of print 13 at BASE + G
    fresh = m.search_prints(np.array([5, 13, 0, G], np.int64) + BASE, 1.0, np.float32(0.3))["scores"]
    row = {5: 0, 13: 1, 0: 2, G: 3}
    now = m.score_print_pairs(a, b, 1.0, np.float32(0.3), want_parts=True)
    want = np.array([fresh[row[int(x - BASE)], int(y - BASE)] for x, y in zip(a, b)], np.float32)
    assert (now["status"] == M.PAIR_OK).all() and np.array_equal(bits(now["score"]), bits(want))
    assert bits(now["score"][:2]).tolist() == [M1_BITS, M1_BITS] and not bits(now["parts"][:2]).any()       # the removed print: nothing of a is active, and b removed
    assert bits(now["score"][2]) == bits(first["score"][2]) and now["score"][4] > 0 and bits(now["score"][4]) == bits(fresh[1, 13])      # the copy scores as the original
    c = m.correspondences_print_pairs(a, b, want_parts=True)
    assert c["counts"][:2].tolist() == [M.CORR_NOT_RUN] * 2 and c["counts"][4] > 0 and bits(c["part"][4]) == bits(now["parts"][4, 0])
    m.close()
