"""Print cascade on the GPU: afis_search_prints_cascade takes resident prints as queries, runs the minutiae scorer for every column, keeps per query the `keep` best
columns by that partial score and runs the texture scorer for those only.

The yardstick is afis_search_prints on the SAME context — existing code, itself held to the oracle — asked four times for the same query prints: the weights
(w_m, w_t) give the final cells, (w_m, 0) the stage-1 matrix m, (1, 0) the minutiae part and (0, 1) the texture part.  The numpy model
tests/print_cascade_model.py makes the kept lists, the expected matrix, n_kept and kept_parts of them.  Every comparison is on uint32 views, exact.
"""
import importlib

import numpy as np
import pytest

import cases
import cascade_model as CM
import print_cascade_model as PM
from test_gpu_rank_hits import SubjectModel, assert_same
from test_gpu_print_search import BASE as EDGE_BASE, BIG, COUNTS, EMPTY, G as EDGE_G, NO_MINU, NO_TEX, REMOVED, WEIGHTS, make_prints, open_matcher

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 3
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NINF = float("-inf")
KEEPS = (1, 7, 64, 65, 70, 100)                                             # the 64-pair segment edge (64 / 65), keep == G, keep > G; chunks of 50 cut inside a query's run
QUERIES = list(range(10)) + [20, 40]
W_M, W_T = np.float32(1.0), np.float32(0.3)
OPTIONS = ("print_cascade_stage1_us", "print_cascade_select_us", "print_cascade_stage2_us", "print_cascade_kept_pairs")
POS_LISTED, POS_NO_ENTRY = 0, 1
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def yardstick(m, idx, wm, wt):
    """The four afis_search_prints matrices of the same context, and the status for the real weights."""
    n = len(idx)
    wm = np.broadcast_to(np.asarray(wm, F), (n,)); wt = np.broadcast_to(np.asarray(wt, F), (n,))
    zero, one = np.zeros(n, F), np.ones(n, F)
    final = m.search_prints(idx, wm, wt)
    return {"final": final["scores"], "status": final["status"], "m": m.search_prints(idx, wm, zero)["scores"], "v_m": m.search_prints(idx, one, zero)["scores"],
            "v_t": m.search_prints(idx, zero, one)["scores"], "wm": wm, "wt": wt}


def model(y, has_minu, has_tex, keep, base):
    return PM.expected(y["final"], y["m"], y["v_m"], y["v_t"], has_minu, has_tex, y["wm"], y["wt"], keep, base)


def check(m, idx, y, has_minu, has_tex, keep, base, what=""):
    """One cascade call against the model of the yardstick; -> (what the call returned, the model)."""
    want = model(y, has_minu, has_tex, keep, base)
    got = m.search_prints_cascade(idx, y["wm"], y["wt"], keep)
    G = y["final"].shape[1]
    _, at = PM.active(has_minu, has_tex, y["wm"], y["wt"])
    print(f"{what} keep {keep}: {len(idx)} x {G}, kept pairs {m.get_option('print_cascade_kept_pairs')}, stage 1 {m.get_option('print_cascade_stage1_us')} us, "
          f"select {m.get_option('print_cascade_select_us')} us, stage 2 {m.get_option('print_cascade_stage2_us')} us")
    assert np.array_equal(got["n_kept"], want["n_kept"]), (what, keep, got["n_kept"], want["n_kept"])
    assert np.array_equal(got["kept_idx"], want["kept_idx"]), (what, keep, np.argwhere(got["kept_idx"] != want["kept_idx"])[:6].tolist())
    g = got["scores"].view(np.uint32)
    assert g.shape == want["matrix"].shape and np.array_equal(g, want["matrix"]), (what, keep, np.argwhere(g != want["matrix"])[:8].tolist())
    gp = got["kept_parts"].view(np.uint32)
    assert gp.shape == want["kept_parts"].shape and np.array_equal(gp, want["kept_parts"]), (what, keep, np.argwhere(gp != want["kept_parts"])[:8].tolist())
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["status"], y["status"]), (what, keep)
    assert m.get_option("print_cascade_kept_pairs") == int(at.sum()) * min(keep, G)
    tm = m.timing()
    assert tm["pairs"] == int((want["status"] == 0).sum()) * G and tm["adc_ms"] == 0 and tm["tex_tail_ms"] == 0 and tm["adc_lookups"] == 0
    return got, want


# ---- 1: the 70-print set, several launch groups, chunks of 50 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


def open_small(cb, cbb, **opts):
    _, gal = cases.small_set(cb, seed=SEED, n_lat=3, n_gal=70)
    m = M.Matcher(cbb)
    for k, v in dict(opts, query_batch=5, cascade_pairs_per_launch=50).items():
        m.set_option(k, v)
    m.gallery_add(gal); m.gallery_commit(BASE)
    return m


@pytest.fixture(scope="module")
def small(cb, codebook_bytes):
    m = open_small(cb, codebook_bytes)
    idx = np.array(QUERIES, np.int64) + BASE
    y = yardstick(m, idx, W_M, W_T)
    yield m, idx, y, np.ones(len(idx), bool)
    m.close()


@pytest.mark.parametrize("keep", KEEPS)
def test_small_set_equals_the_model(small, keep):
    m, idx, y, has = small
    check(m, idx, y, has, has, keep, BASE, what="small set")
    assert m.timing()["launch_groups"] >= 2


def test_small_set_is_not_vacuous(small):
    """From the yardstick alone: a kept cell whose texture part is positive and whose final word is not m's; and a (query, keep) whose kept set is not the final
    score's top keep — the selection is stage 1's."""
    m, idx, y, has = small
    tex_matters = selection_differs = False
    for keep in KEEPS:
        e = model(y, has, has, keep, BASE)
        _, _, full_pos = CM.rank_rows(y["final"], keep, BASE)
        for q in range(len(idx)):
            kp = e["kept_pos"][q][:e["n_kept"][q]]
            tex_matters |= bool(((y["v_t"][q, kp] > 0) & (bits(y["final"])[q, kp] != bits(y["m"])[q, kp])).any())
            selection_differs |= set(kp.tolist()) != set(full_pos[q][full_pos[q] >= 0].tolist())
    assert tex_matters and selection_differs


# ---- 2: edges: prints without minutiae, without texture, empty, removed, 1000 texture rows; the four weight pairs ------------------------------------------------
def edge_flags(loc):
    gone = (EMPTY, REMOVED)
    return (np.array([COUNTS[l][0] > 0 and l not in gone for l in loc], bool), np.array([COUNTS[l][1] > 0 and l not in gone for l in loc], bool))


def edge_weights(n, shift):
    pairs = [WEIGHTS[(i + shift) % 4] for i in range(n)]
    return np.array([p[0] for p in pairs], F), np.array([p[1] for p in pairs], F)


@pytest.mark.parametrize("name", ["shipped", "tiny"])
def test_edges(name):
    cbk = cases.shipped_codebook() if name == "shipped" else cases.family_codebook(name)
    m = open_matcher(cbk.to_bytes(), make_prints(cbk))
    loc = list(range(EDGE_G)) + [BIG]                                        # all 20 prints, and one index twice
    idx = np.array(loc, np.int64) + EDGE_BASE
    hm, ht = edge_flags(loc)
    default = m.get_option("cascade_pairs_per_launch")
    kinds = set()
    for shift in range(4):                                                  # every weight pair meets every print: (1, 0.3f), (1, 0), (0, 1), (0, 0)
        wm, wt = edge_weights(len(loc), shift)
        y = yardstick(m, idx, wm, wt)
        am, at = PM.active(hm, ht, wm, wt)
        kinds |= {(bool(a), bool(t)) for a, t in zip(am, at)}
        for keep in ((1, 5, 19, 20, 25) if name == "shipped" and shift == 0 else (5,)):
            out = []
            for per in (3, default):
                m.set_option("cascade_pairs_per_launch", per)
                got, want = check(m, idx, y, hm, ht, keep, EDGE_BASE, what=f"edges {name} shift {shift} per {per}")
                out.append(got)
            for key in ("scores", "kept_idx", "kept_parts", "n_kept", "status"):
                assert out[0][key].tobytes() == out[1][key].tobytes(), (key, keep, shift)
            blind = np.flatnonzero(~am)                                     # a row stage 1 cannot rank keeps its first columns by index
            n = min(keep, EDGE_G)
            assert (got["kept_idx"][blind, :n] == np.arange(n) + EDGE_BASE).all()
            only_m = np.flatnonzero(am & ~at)                               # a minutiae-only row: the kept cells are m
            kept = got["scores"].view(np.uint32) != CM.NO_ENTRY
            assert np.array_equal(got["scores"].view(np.uint32)[only_m][kept[only_m]], bits(y["m"])[only_m][kept[only_m]])
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    m.close()


# ---- 3: scorer options -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [{"s3_tie_order": 1}, {"ref_tie_order": 2}, {"adc_variant": 8}], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_options_against_the_same_contexts_print_search(opt, cb, codebook_bytes):
    m = open_small(cb, codebook_bytes, **opt)
    idx = np.array(QUERIES, np.int64) + BASE
    has = np.ones(len(idx), bool)
    check(m, idx, yardstick(m, idx, W_M, W_T), has, has, 7, BASE, what=str(opt))
    m.close()


# ---- 4: the matrix is a search's ---------------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_is_a_searchs(small):
    m, idx, y, has = small
    keep, n_q, G = 7, len(idx), y["final"].shape[1]
    before = m.search_prints(idx, W_M, W_T)["scores"]
    subject = (np.arange(G) // 10).astype(np.int64) * 3 + 5                 # ten prints per person
    sj = m.subjects_create(subject)
    got, want = check(m, idx, y, has, has, keep, BASE, what="family")
    mat = want["matrix"].view(F)
    n_hits, ridx, pos = CM.rank_rows(mat, keep, BASE)                       # the kept cells re-sorted by final score
    hits = m.rank_hits(NINF, keep)
    assert np.array_equal(hits["n_hits"], n_hits) and np.array_equal(hits["idx"], ridx)
    for q in range(n_q):
        assert sorted(hits["idx"][q].tolist()) == sorted(got["kept_idx"][q].tolist())
        assert hits["score"][q].view(np.uint32).tolist() == bits(y["final"])[q, pos[q]].tolist()
    # the print against itself is an ordinary kept cell; an exclusion list takes it out
    self_kept = [q for q in range(n_q) if int(idx[q]) in hits["idx"][q].tolist()]
    assert len(self_kept) >= 10
    f = m.rank_hits_filtered(NINF, keep, excl=[[int(g)] for g in idx])
    for q in self_kept:
        rest = [t for t in ridx[q].tolist() if t != int(idx[q])]
        assert f["n_hits"][q] == keep - 1 and f["idx"][q].tolist() == rest + [-1]
    # a column stage 1 dropped is no entry; a kept one stands where the list has it
    dropped = [(q, int(np.flatnonzero(want["matrix"][q] == CM.NO_ENTRY)[-1])) for q in range(n_q)]
    kept = [(q, int(pos[q, r])) for q in range(n_q) for r in (0, keep - 1)]
    p = m.rank_positions([q for q, _ in dropped + kept], [BASE + t for _, t in dropped + kept])
    assert p["status"][:n_q].tolist() == [POS_NO_ENTRY] * n_q and p["n_before"][:n_q].tolist() == [-1] * n_q
    assert p["status"][n_q:].tolist() == [POS_LISTED] * (2 * n_q) and p["n_before"][n_q:].tolist() == [0, keep - 1] * n_q
    assert p["score"][n_q:].view(np.uint32).tolist() == [int(want["matrix"][q, t]) for q, t in kept]
    # persons: only the kept cells are entries
    assert_same(m.rank_subject_hits(sj, NINF, 5), SubjectModel(mat, np.arange(G) + BASE, subject).hits(NINF, 5), "rank_subject_hits")
    # the pair call over the kept pairs gives the kept cells' scores and kept_parts; it leaves the matrix alone
    a = np.repeat(idx, keep); b = got["kept_idx"].reshape(-1)
    sp = m.score_print_pairs(a, b, W_M, W_T, want_parts=True)
    assert (sp["status"] == 0).all()
    assert np.array_equal(bits(sp["score"]), want["matrix"][np.repeat(np.arange(n_q), keep), want["kept_pos"].reshape(-1)])
    assert np.array_equal(bits(sp["parts"]).reshape(n_q, keep, 2), want["kept_parts"])
    assert np.array_equal(m.rank_hits(NINF, keep)["idx"], ridx)
    # a following afis_search_prints returns its earlier bytes
    after = m.search_prints(idx, W_M, W_T)["scores"]
    assert before.tobytes() == after.tobytes() == y["final"].tobytes()
    m.subjects_free(sj)


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    cbk = cases.shipped_codebook()
    prints = make_prints(cbk)
    m = open_matcher(cbk.to_bytes(), prints)
    idx = np.array([BIG, 13], np.int64) + EDGE_BASE
    one = np.ones(2, F)

    def refused(code, *args):
        m.search_prints_cascade(idx, one, one, 3, want_scores=False)        # a matrix to lose
        assert m.rank_hits(NINF, 3)["n_hits"].tolist() == [3, 3]
        assert m.get_option("print_cascade_kept_pairs") == 6 and m.get_option("print_cascade_stage1_us") > 0
        with pytest.raises(M.AfisError, match=code):
            m.search_prints_cascade(*args)
        with pytest.raises(M.AfisError, match=ESTATE):                      # after any return other than AFIS_OK the last-search matrix is invalid
            m.rank_hits(NINF, 3, n_q=2)
        for name in OPTIONS + ("print_gather_us", "print_h2d_bytes"):
            assert m.get_option(name) == 0, name

    for bad_keep in (0, 4097):
        refused(EINVAL, idx, one, one, bad_keep)
    refused(EINVAL, np.array([EDGE_BASE + BIG, EDGE_BASE + EDGE_G]), one, one, 3)       # outside the resident shard
    refused(EINVAL, np.array([BIG, 13]), one, one, 3)                       # shard-local indices are not global ones
    for bad in (np.nan, np.inf, -1.0):
        w = one.copy(); w[1] = bad
        refused(EINVAL, idx, w, one, 3)
        refused(EINVAL, idx, one, w, 3)
    p_idx, p_w = M._ptr(idx, M.C.c_int64), M._ptr(one, M.C.c_float)
    assert m.lib.afis_search_prints_cascade(None, p_idx, 2, p_w, p_w, 3, None, None, None, None, None) == -1
    assert m.lib.afis_search_prints_cascade(m.ctx, p_idx, -1, p_w, p_w, 3, None, None, None, None, None) == -1
    assert m.lib.afis_search_prints_cascade(m.ctx, None, 2, p_w, p_w, 3, None, None, None, None, None) == -1
    assert m.lib.afis_search_prints_cascade(m.ctx, p_idx, 2, None, p_w, 3, None, None, None, None, None) == -1
    # staged but not committed
    m.gallery_reopen(); m.gallery_add(prints[13:15])
    refused(ESTATE, np.array([EDGE_BASE + BIG, EDGE_BASE + EDGE_G + 1]), one, one, 3)
    m.gallery_commit(EDGE_BASE)
    r = m.search_prints_cascade(np.array([EDGE_BASE + EDGE_G]), 1.0, 1.0, 2)    # valid after the edit, no handle involved: a second copy of print 13 keeps itself and the first copy
    assert r["scores"].shape == (1, EDGE_G + 2) and sorted(r["kept_idx"][0].tolist()) == [EDGE_BASE + 13, EDGE_BASE + EDGE_G]
    # no query: AFIS_OK, nothing kept
    r = m.search_prints_cascade(np.zeros(0, np.int64), [], [], 4)
    assert r["scores"].shape == (0, EDGE_G + 2) and r["kept_idx"].shape == (0, 4) and len(r["status"]) == 0
    for name in OPTIONS:
        assert m.get_option(name) == 0, name
    m.close()
    fresh = M.Matcher(cbk.to_bytes())
    fresh.gallery_add(prints[:3])
    with pytest.raises(M.AfisError, match=ESTATE):                          # before the first commit
        fresh.search_prints_cascade(np.array([0]), 1.0, 1.0, 2)
    fresh.close()
