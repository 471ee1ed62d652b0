"""Print search on the GPU: afis_search_prints takes resident prints as queries, builds their query views on the device and leaves a search's matrix.

1  the gather through its parity tap against the numpy model (tests/print_model.py): every table and array byte-equal, the pad rows of a fragment tile zero;
2  end to end against the ORACLE's all-templates vectors (tie_mode 1) for the prints' views, folded in numpy: scores, status, the -1 cells, the latent-empty rows
   and the self cells, bit for bit;
3  against afis_search_weighted over host views of the same prints — the only route there was — under the options that change the scorers, and with batches of 1 and 3;
4  the subset form; 5  the matrix is a search's: the ranking calls read it; 6  print_h2d_bytes; 7  refusals.

One gallery of 20 synthetic prints (at most 16 queries per call).  A print WITHOUT a minutiae template cannot pass through the file format the oracle reads (the
writer stops after the header), so for the oracle alone print NO_MINU carries a one-minutia stand-in template: its texture entries are the oracle's — a scorer's value
depends on nothing but its (latent template, print template) — its minutiae entries are the zeros the matcher leaves for a template that is not there, and as a query
its view has no minutiae entry at all.  Test 3 holds that print's cells against the weighted route without any stand-in."""
import importlib

import numpy as np
import pytest

import cases
import print_model as P
import weighted_model as W
from test_gpu_rank_hits import TemplateModel, SubjectModel, assert_same

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

ESTATE, EINVAL = "afis error -3", "afis error -1"
NINF = float("-inf")
BASE = 7000                                                                 # index_base != 0
# (minutiae, texture points): texture 1, 7, 8, 9, 15, 16, 17, 33 and 1100 -> 1000 (the 8-row LUT tile, the 16-row tile, the clamp); minutiae 1, 15, 16, 17, 64, 129
# (the 16-descriptor fragment tile, the candidate shape classes)
COUNTS = [(1, 1), (15, 7), (16, 8), (17, 9), (64, 15), (129, 16), (30, 17), (40, 33), (80, 1100), (0, 300), (50, 0), (0, 0), (60, 200), (70, 250), (20, 120), (90, 400),
          (35, 100), (16, 64), (100, 260), (25, 31)]                        # the last four arrive by an appending commit
BIG, NO_MINU, NO_TEX, EMPTY, REMOVED, N_FIRST = 8, 9, 10, 11, 12, 16
G = len(COUNTS)
WEIGHTS = [(1.0, np.float32(0.3)), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_prints(cb):
    rng = np.random.default_rng(2026)
    out = []
    for nm, nt in COUNTS:
        t = S.make_rolled(rng, cb, max(nm, 1), max(nt, 1))
        if nm == 0:
            t.minu = []
        if nt == 0:
            t.tex = []
        out.append(t)
    out[BIG].tex[0].codes[0] = 0; out[BIG].tex[0].codes[1] = 255             # codes 0 and 255 in every sub-quantizer
    return out


def open_matcher(cbb, prints, taps=False, **options):
    """The shard as an enrolment history leaves it: a first commit, a removal, four prints by an appending commit (the device arrays grow)."""
    m = M.Matcher(cbb, taps=taps)
    for k, v in options.items():
        m.set_option(k, v)
    m.gallery_add(prints[:N_FIRST]); m.gallery_commit(BASE)
    m.gallery_remove([BASE + REMOVED])
    m.gallery_reopen(); m.gallery_add(prints[N_FIRST:]); m.gallery_commit(BASE)
    assert m.resident_size == G
    return m


class World:
    def __init__(self, name, oracle):
        self.cb = cases.shipped_codebook() if name == "shipped" else cases.family_codebook(name)
        self.cbb = self.cb.to_bytes()
        made = make_prints(self.cb)
        self.enrolled = made
        self.prints = [T.FPTemplate() if i in (EMPTY, REMOVED) else p for i, p in enumerate(made)]     # the host's copy of what is resident
        self.views = [P.view(p, self.cb.words) for p in self.prints]
        self.counts = [(len(v.minu), len(v.tex)) for v in self.views]
        self.empty = np.array([nm + nt == 0 for nm, nt in self.counts], np.uint8)
        self.glob = np.arange(G, dtype=np.int64) + BASE
        self.oracle, self.ocb, self._vec = oracle, oracle.codebook(self.cbb), {}
        stand_in = T.MinutiaeTemplate(np.array([100], np.int16), np.array([100], np.int16), np.zeros(1, np.float32), np.ones((1, 96), np.float32))
        self._stand_in = stand_in
        cols = [T.FPTemplate(minu=[stand_in], tex=p.tex) if i == NO_MINU else p for i, p in enumerate(self.prints)]
        self.hr = [oracle.rolled(T.write_rolled(c))[0] for c in cols]

    def vec(self, q):
        """[G][n_minu + n_tex] of print q's view: the oracle's all-templates vectors (tie_mode 1), computed once."""
        if q not in self._vec:
            nm, nt = self.counts[q]
            v = np.zeros((G, nm + nt), np.float32)
            if nm + nt:
                src = self.views[q] if nm else T.FPTemplate(minu=[self._stand_in], tex=self.views[q].tex)
                hl, _ = self.oracle.latent(self.ocb, T.write_latent(src))
                for g in range(G):
                    rc, full = self.oracle.all_templates(self.ocb, hl, self.hr[g], len(src.minu) + nt, tie_mode=1)
                    assert (rc == 2) == bool(self.empty[g]), (q, g, rc)
                    v[g] = full if nm else full[1:]                         # (a view without minutiae has no minutiae entry)
                if nm:
                    v[NO_MINU, 0] = 0.0                                     # the zero the matcher leaves for a print without a minutiae template
            self._vec[q] = v
        return self._vec[q]

    def expected(self, idx, wm, wt, cols=None):
        rows, status = [], []
        for i, g in enumerate(idx):
            q = int(g) - BASE
            row, st = W.fold_vectors(self.vec(q), self.counts[q][0], np.array([wm[i]], np.float32), np.array([wt[i]], np.float32), self.empty)
            rows.append(row); status.append(st)
        out = np.stack(rows)
        return (out if cols is None else out[:, cols]), np.array(status, np.int32)


@pytest.fixture(scope="module", params=["shipped", "tiny"])
def world(request, oracle):
    return World(request.param, oracle)


@pytest.fixture(scope="module")
def shared(world):
    m = open_matcher(world.cbb, world.enrolled, taps=True)
    yield m
    m.close()


def weights_for(n, k=None):
    """The four weight pairs in turn over n queries (k: one pair for all)."""
    pairs = [WEIGHTS[(i if k is None else k) % 4] for i in range(n)]
    return np.array([p[0] for p in pairs], np.float32), np.array([p[1] for p in pairs], np.float32)


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_gather_against_the_model(shared, world):
    m = shared
    rng = np.random.default_rng(17)
    lists = [(list(range(16)), None, None),                                  # the prints of the first commit, in order
             ([BIG, 0, BIG, 19, NO_MINU, 3, EMPTY, 5, 5, REMOVED, 16, NO_TEX, 1, 17, 18], None, None),  # any order, repeats, the appended prints
             (list(rng.permutation(G)[:12]), rng.integers(0, 2, 12), rng.integers(0, 2, 12)),           # what a zero weight leaves out
             ([EMPTY], None, None), ([0], None, None)]
    for loc, um, ut in lists:
        got = m.debug_print_queries(np.array(loc, np.int64) + BASE, um, ut)
        want = P.group([world.prints[i] for i in loc], world.cb.words, um, ut)
        assert set(got) == set(want)
        for key, w in want.items():
            g = got[key]
            if key == "lt_pad":
                assert g == w, (loc, key)
                continue
            assert g.shape == w.shape and g.dtype == w.dtype, (loc, key, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (loc, key, np.argwhere(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))[:6].ravel().tolist())
        # rows of lm_frag beyond the last descriptor of a template's last tile are zero
        for p in range(len(loc)):
            nm = int(got["lm_off"][3 * p + 1] - got["lm_off"][3 * p])
            if nm % 16:
                last = got["lm_frag"][got["lm_tile_off"][3 * p + 1] - 1]
                assert (last[:, (np.arange(64) & 15) >= nm % 16] == 0).all(), (loc, p)
    big = m.debug_print_queries([BASE + BIG])
    assert big["lt_des"].shape == (1000, 96) and big["lt_pad"] == 1000      # the clamp
    assert np.array_equal(bits(big["lt_des"][0]), bits(world.cb.words[:, 0].reshape(-1))) and np.array_equal(bits(big["lt_des"][1]), bits(world.cb.words[:, 255].reshape(-1)))


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_oracle(shared, world):
    m = shared
    calls = [np.arange(16), np.array([19, 18, 17, 16, BIG, BIG, NO_MINU, NO_TEX, EMPTY, REMOVED, 0, 13])]      # every print; any order, repeats
    positive_self = 0
    for k in range(4):                                                      # every weight pair for every query: (1, 0.3f), (1, 0), (0, 1), (0, 0)
        for loc in calls:
            idx = loc.astype(np.int64) + BASE
            wm, wt = weights_for(len(idx), k)
            want, status = world.expected(idx, wm, wt)
            got = m.search_prints(idx, wm, wt)
            assert got["scores"].shape == (len(idx), G)
            assert np.array_equal(got["status"], status), (k, got["status"], status)
            assert np.array_equal(bits(got["scores"]), bits(want)), (k, np.argwhere(bits(got["scores"]) != bits(want))[:8].tolist())
            assert np.array_equal(got["scores"] == -1, (world.empty[None, :] != 0) | (status[:, None] != 0)), k
            if k == 0:
                positive_self += int(sum(got["scores"][i, int(l)] > 0 for i, l in enumerate(loc)))
            expect_empty = np.array([world.empty[int(l)] or (wm[i] == 0 or world.counts[int(l)][0] == 0) and (wt[i] == 0 or world.counts[int(l)][1] == 0) for i, l in enumerate(loc)])
            assert np.array_equal(status == W.LATENT_EMPTY, expect_empty), k
            assert m.get_option("weighted_pseudo_queries") == int((status == 0).sum()) and m.timing()["pairs"] == int((status == 0).sum()) * G
    # mixed weights in one call
    idx = np.array([BIG, 13, NO_MINU, NO_TEX, 15, 18, 2, 5], np.int64) + BASE
    wm, wt = weights_for(len(idx))
    want, status = world.expected(idx, wm, wt)
    got = m.search_prints(idx, wm, wt)
    assert np.array_equal(bits(got["scores"]), bits(want)) and np.array_equal(got["status"], status)
    assert positive_self >= 10                                              # the self cells are ordinary cells, and they are scored


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_against_the_weighted_route(world):
    loc = np.array([BIG, NO_MINU, NO_TEX, EMPTY, 0, 1, 2, 3, 4, 5, 6, 7, 13, 19, 16, BIG])
    idx = loc.astype(np.int64) + BASE
    wm, wt = weights_for(len(idx))
    wm[0] = 1.0; wt[0] = np.float32(0.3); wm[1] = 0.5; wt[1] = 2.0
    views = [world.views[int(l)] for l in loc]
    seen = {}
    for opts in ({}, {"adc_variant": 8}, {"s3_tie_order": 1}, {"ref_tie_order": 2}):
        m = open_matcher(world.cbb, world.enrolled, **opts)
        for cap in ((0, 1, 3) if not opts else (0,)):
            m.set_option("weighted_batch_pseudo", cap)
            ref = m.search_weighted(views, wm[:, None], wt[:, None])
            ref_pq, ref_pairs = m.get_option("weighted_pseudo_queries"), m.timing()["pairs"]
            got = m.search_prints(idx, wm, wt)
            assert np.array_equal(bits(got["scores"]), bits(ref["scores"])), (opts, cap, np.argwhere(bits(got["scores"]) != bits(ref["scores"]))[:8].tolist())
            assert np.array_equal(got["status"], ref["status"]), (opts, cap)
            assert m.get_option("weighted_pseudo_queries") == ref_pq and m.timing()["pairs"] == ref_pairs, (opts, cap)
            seen[(tuple(opts.items()), cap)] = bits(got["scores"]).copy()
        m.close()
    assert np.array_equal(seen[((), 0)], seen[((), 1)]) and np.array_equal(seen[((), 0)], seen[((), 3)])      # batching changes nothing
    want, _ = world.expected(idx, wm, wt)
    assert np.array_equal(seen[((), 0)], bits(want))


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_subset_form(world):
    m = open_matcher(world.cbb, world.enrolled)
    loc = np.array([BIG, 13, NO_MINU, EMPTY, 17])
    idx = loc.astype(np.int64) + BASE
    wm, wt = weights_for(len(idx), 0)
    full = m.search_prints(idx, wm, wt)
    listed = np.array([18, 3, BIG, EMPTY, 0, 15, NO_TEX], np.int64)          # out of order; most query prints are not in it
    sh = m.subset_create(listed + BASE)
    got = m.search_prints(idx, wm, wt, subset=sh)
    assert got["scores"].shape == (len(idx), len(listed))
    assert np.array_equal(bits(got["scores"]), bits(full["scores"][:, listed])) and np.array_equal(got["status"], full["status"])
    want, _ = world.expected(idx, wm, wt)
    o = np.sort(listed)                                                     # the matrix on the device is a subset search's: the lists carry global indices
    assert_same(m.rank_hits(NINF, 4), TemplateModel(np.ascontiguousarray(want[:, o]), o + BASE).hits(NINF, 4), "subset rank_hits")
    asc = m.subset_create(np.sort(listed) + BASE)                           # listed in ascending order: no permutation on the way out
    got2 = m.search_prints(idx, wm, wt, subset=asc)
    assert np.array_equal(bits(got2["scores"]), bits(full["scores"][:, np.sort(listed)]))
    # a stale subset after a commit
    m.gallery_reopen(); m.gallery_add(world.enrolled[:1]); m.gallery_commit(BASE)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_prints(idx, wm, wt, subset=sh)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_hits(NINF, 4, n_q=len(idx))
    r = m.search_prints(idx, wm, wt)                                        # ... and the whole shard, one print larger, goes on
    assert r["scores"].shape == (len(idx), G + 1) and np.array_equal(bits(r["scores"][:, :G]), bits(full["scores"])) and np.array_equal(bits(r["scores"][:, G]), bits(full["scores"][:, 0]))
    m.subset_free(sh); m.subset_free(asc)
    m.close()


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_is_a_searchs(shared, world):
    m = shared
    loc = np.array([BIG, 13, 15, 18, NO_MINU, 5])
    idx = loc.astype(np.int64) + BASE
    n_q = len(idx)
    wm, wt = weights_for(n_q, 0)
    want, _ = world.expected(idx, wm, wt)
    lat, _ = cases.small_set(world.cb, seed=9, n_lat=2, n_gal=1)
    before = m.search(lat, k=0, want_scores=True)["scores"]
    subject = (np.arange(G) // 3).astype(np.int64) * 5 + 2
    sj = m.subjects_create(subject)
    m.search_prints(idx, wm, wt, want_scores=False)
    tm = TemplateModel(want, world.glob)
    hits = m.rank_hits(NINF, 6)
    assert_same(hits, tm.hits(NINF, 6), "rank_hits")
    leads = [q for q, l in enumerate(loc) if want[q, l] > 0]
    assert len(leads) >= 4
    for q in leads:
        assert hits["idx"][q, 0] == BASE + loc[q], (q, loc[q])              # a print with a positive self score leads its own list
    # ... and an exclusion list takes the self cell out: the same list without it
    filt = m.rank_hits_filtered(NINF, 6, excl=[[int(g)] for g in idx])
    wide = m.rank_hits(NINF, 7)
    for q in leads:
        assert filt["n_hits"][q] == wide["n_hits"][q] - 1 == G - 1
        assert np.array_equal(filt["idx"][q], wide["idx"][q, 1:]) and np.array_equal(bits(filt["score"][q]), bits(wide["score"][q, 1:]))
    assert_same(m.rank_subject_hits(sj, NINF, 4), SubjectModel(want, world.glob, subject).hits(NINF, 4), "rank_subject_hits")
    pos = m.rank_positions(np.arange(n_q, dtype=np.int32), idx)
    assert (pos["status"] == 0).all() and (pos["n_before"][leads] == 0).all() and np.array_equal(bits(pos["score"]), bits(want[np.arange(n_q), loc]))
    col = m.rank_latent_hits(NINF, 3)                                       # per print of the shard, the query prints that hit it
    assert col["n_hits"].tolist() == [n_q] * G
    assert_same(m.rank_hits(0.5, 9), tm.hits(0.5, 9), "rank_hits 0.5")
    # a following afis_search is unchanged
    after = m.search(lat, k=0, want_scores=True)["scores"]
    assert np.array_equal(bits(before), bits(after))
    m.subjects_free(sj)


# ---- 6 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_only_tables_cross_pcie(shared, world):
    m = shared
    for loc, cap in (([BIG] * 4, 0), ([BIG, 15, BIG, 18, BIG, 13, BIG, BIG], 1), ([BIG] * 16, 3)):
        idx = np.array(loc, np.int64) + BASE
        n_q = len(idx)
        held = sum(P.view_bytes(world.views[l]) for l in loc)
        assert held >= n_q * 100 * 1024                                     # the bound below means something: the views hold at least 100 KB per query
        m.set_option("weighted_batch_pseudo", cap)
        wm, wt = weights_for(n_q, 0)
        m.search_prints(idx, wm, wt, want_scores=False)
        h2d, us = m.get_option("print_h2d_bytes"), m.get_option("print_gather_us")
        print(f"{n_q} queries, cap {cap}: views {held} bytes, print_h2d_bytes {h2d}, print_gather_us {us}")
        assert 0 < h2d <= 256 * n_q + 4096, (h2d, n_q)
        assert us > 0
    m.set_option("weighted_batch_pseudo", 0)
    m.search_prints(np.zeros(0, np.int64), [], [])
    assert m.get_option("print_h2d_bytes") == 0 and m.get_option("print_gather_us") == 0


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(world):
    m = open_matcher(world.cbb, world.enrolled)
    idx = np.array([BIG, 13], np.int64) + BASE
    one = np.ones(2, np.float32)
    other = M.Matcher(world.cbb)
    other.gallery_add(world.enrolled[:4]); other.gallery_commit(BASE)
    foreign = other.subset_create([BASE, BASE + 1])

    def refused(code, *args, **kw):
        m.search_prints(idx, one, one, want_scores=False)                   # a matrix to lose
        assert m.rank_hits(NINF, 2)["n_hits"].tolist() == [G, G]
        with pytest.raises(M.AfisError, match=code):
            m.search_prints(*args, **kw)
        with pytest.raises(M.AfisError, match=ESTATE):                      # after any return other than AFIS_OK the last-search matrix is invalid
            m.rank_hits(NINF, 2, n_q=2)
        assert m.get_option("print_h2d_bytes") == 0 and m.get_option("print_gather_us") == 0

    def raw(*args):
        m.search_prints(idx, one, one, want_scores=False)
        rc = m.lib.afis_search_prints(*args)
        with pytest.raises(M.AfisError, match=ESTATE):
            m.rank_hits(NINF, 2, n_q=2)
        return rc
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-45):
        w = one.copy(); w[1] = bad
        refused(EINVAL, idx, w, one)
        refused(EINVAL, idx, one, w)
    refused(EINVAL, np.array([BASE + BIG, BASE + G]), one, one)             # outside the resident shard, either side
    refused(EINVAL, np.array([BASE - 1, BASE + BIG]), one, one)
    refused(EINVAL, np.array([BIG, 13]), one, one)                          # shard-local indices are not global ones
    refused(EINVAL, idx, one, one, subset=foreign)                          # a subset of another context
    p_idx, p_w = M._ptr(idx, M.C.c_int64), M._ptr(one, M.C.c_float)
    assert raw(m.ctx, None, p_idx, -1, p_w, p_w, None, None) == -1
    assert raw(m.ctx, None, None, 2, p_w, p_w, None, None) == -1
    assert raw(m.ctx, None, p_idx, 2, None, p_w, None, None) == -1
    assert raw(m.ctx, None, p_idx, 2, p_w, None, None, None) == -1
    assert m.lib.afis_search_prints(None, None, p_idx, 2, p_w, p_w, None, None) == -1
    # staged but not committed
    m.gallery_reopen(); m.gallery_add(world.enrolled[13:15])
    refused(ESTATE, np.array([BASE + BIG, BASE + G + 1]), one, one)
    refused(EINVAL, np.array([BASE + BIG, BASE + G + 2]), one, one)
    m.gallery_commit(BASE)
    r = m.search_prints(np.array([BASE + G]), 1.0, 1.0)                     # a second copy of print 13: its own cell and the first copy's hold one value
    assert r["scores"].shape == (1, G + 2) and r["scores"][0, G] > 0 and r["scores"][0, 13] == r["scores"][0, G]
    # no query: AFIS_OK
    r = m.search_prints(np.zeros(0, np.int64), [], [])
    assert r["scores"].shape == (0, G + 2) and len(r["status"]) == 0
    other.subset_free(foreign); other.close(); m.close()
    fresh = M.Matcher(world.cbb)
    fresh.gallery_add(world.enrolled[:3])
    with pytest.raises(M.AfisError, match=ESTATE):                          # before the first commit
        fresh.search_prints(np.array([0]), 1.0, 1.0)
    fresh.close()
