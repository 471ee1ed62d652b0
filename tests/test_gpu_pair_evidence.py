"""Texture correspondences and pair alignments on the GPU: afis_texture_correspondences_pairs, afis_pair_alignments and their forms for resident print pairs.  Every
comparison is exact — indices and coordinates equal, similarities and parts by their bits, moments as integers.

1  the texture export at every list length (tests/cases.py::list_length_set as tests/test_gpu_pair_forms.py::Lengths arranges it: texture lists of every length 1 .. 230,
   four geometries, every latent against its mate and ten other columns, shuffled) against the oracle's stage-2 trace of the texture scorer, in the coordinate classes
   `default` and `generic` and in ref_tie_order 0 and 2 (the oracle's tie modes 1 and 9, as test_gpu_list_lengths.py maps them); `part` against afis_score_pairs;
2  the edges in one gallery of 40 prints; 3  the moments against numpy integers over the oracle's traces and over the library's own exports, and the rigid geometry's
   exact fit; 4  the print forms on tests/test_gpu_print_search.py's world against the latent forms over the same prints' views.
The fit's arithmetic and the relation part = the fp32 sum of sim in list order are tests/test_pair_evidence_host.py's."""
import ctypes as C
import importlib
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cases
import pair_evidence_model as PE
import test_gpu_list_lengths as lengths
import test_gpu_pair_forms as forms
from test_gpu_correspondence_pairs import Expected
from test_gpu_print_search import BASE, BIG, COUNTS, EMPTY, G, NO_MINU, NO_TEX, REMOVED, World, open_matcher

T = importlib.import_module("msu-latentafis_amd.host.templates")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

CLASSES = {c[0]: c for c in lengths.COORDINATE_CLASSES}
NINF = float("-inf")
ZERO9 = (0,) * 9


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


class Evidence:
    """The list-length pair list (forms.Lengths) with the oracle's stage-2 texture traces of every pair, computed once per coordinate class and tie mode, shared, never changed."""

    def __init__(self, cb, codebook_bytes, oracle):
        self.lens = forms.Lengths(cb, codebook_bytes, oracle)
        self.oracle, self.rig = oracle, self.lens.rig
        self._handles, self._tex = {}, {}

    def handles(self, name):
        """(latents, gallery, the oracle's latent handles, its rolled handles) of a coordinate class"""
        if name not in self._handles:
            _, tex_shift, minu_shift = CLASSES[name]
            lats, gal = self.lens.shifted(tex_shift, minu_shift)
            hl, hr = (self.rig.hl, self.rig.hr) if tex_shift == 0 and minu_shift == 0 else cases.to_orc(self.oracle, self.rig.ocb, lats, gal)
            self._handles[name] = (lats, gal, hl, hr)
        return self._handles[name]

    def texture(self, name, tie_mode):
        """{(latent, print): (sim, latent rows, print points)} over the pair list"""
        if (name, tie_mode) not in self._tex:
            _, _, hl, hr = self.handles(name)
            todo = sorted({(int(q), int(g)) for q, g in zip(self.lens.query, self.lens.idx)})
            with ThreadPoolExecutor(max(1, min(16, self.oracle.lib.orc_num_threads()))) as pool:
                got = list(pool.map(lambda p: self.oracle.trace(self.rig.ocb, hl[p[0]], hr[p[1]], which=0, stage=2, tie_mode=tie_mode), todo))
            assert all(t is not None for t in got)
            self._tex[(name, tie_mode)] = dict(zip(todo, got))
        return self._tex[(name, tie_mode)]

    def close(self):
        for name, (_, _, hl, hr) in self._handles.items():
            if hl is not self.rig.hl:
                for h in hl: self.oracle.lib.orc_latent_free(h)
                for h in hr: self.oracle.lib.orc_rolled_free(h)


@pytest.fixture(scope="module")
def ev(cb, codebook_bytes, oracle):
    e = Evidence(cb, codebook_bytes, oracle)
    yield e
    e.close()


def tex_points(L, R, li, ri):
    """[n][4] block coordinates of a texture list's entries"""
    a, b = L.tex[0], R.tex[0]
    return np.stack([a.x[li], a.y[li], b.x[ri], b.y[ri]], axis=1).astype(np.int16) if len(li) else np.zeros((0, 4), np.int16)


def same_export(res, i, sim, li, ri, L, R, where):
    n = len(li)
    assert res["counts"][i] == n, (where, int(res["counts"][i]), n)
    assert np.array_equal(res["pt"][i, :n, 0], li) and np.array_equal(res["pt"][i, :n, 1], ri), where
    assert np.array_equal(bits(res["sim"][i, :n]), bits(sim)), where
    assert np.array_equal(res["xy"][i, :n], tex_points(L, R, li, ri)), where
    assert not res["xy"][i, n:].any() and not res["pt"][i, n:].any() and not bits(res["sim"][i, n:]).any(), where      # rows at or beyond counts are zero
    assert np.array_equal(res["corr"][i], res["xy"][i, :n])


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ref_tie", [0, 2])
@pytest.mark.parametrize("name", ["default", "generic"])
def test_texture_correspondences_at_every_length(codebook_bytes, ev, name, ref_tie):
    """counts, pt and sim equal the oracle's stage-2 trace entry for entry (sim as bits), xy the templates' coordinates at those indices, zeros beyond counts, part bit for
    bit afis_score_pairs' parts[:, 3]; at least 0.9 of the mated pairs leave two or more survivors."""
    t0 = time.perf_counter()
    lens, n = ev.lens, ev.lens.n
    tie_mode = lengths.TIE_MODES[ref_tie]
    lats, gal, _, _ = ev.handles(name)
    want = ev.texture(name, tie_mode)
    m = M.Matcher(codebook_bytes)
    m.set_option("ref_tie_order", ref_tie)
    m.gallery_add(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    assert m.get_option("corr_pairs_per_launch") >= len(lens.query) and m.get_option("texture_correspondences_us") == 0
    res = m.texture_correspondences_pairs(qh, lens.query, lens.idx, want_parts=True)
    assert m.get_option("texture_correspondences_us") > 0
    sc = m.score_pairs(qh, lens.query, lens.idx, want_parts=True)
    mated = 0
    for i, (q, g) in enumerate(zip(lens.query, lens.idx)):
        sim, li, ri = want[(int(q), int(g))]
        same_export(res, i, sim, li, ri, lats[q], gal[g], (name, ref_tie, ev.rig.cases[q]["geometry"], ev.rig.cases[q]["N"], int(g)))
        mated += q == g and len(li) >= 2
    diff = np.flatnonzero(bits(res["part"]) != bits(sc["parts"][:, 3]))
    assert not len(diff), (name, ref_tie, len(diff), [(int(lens.query[i]), int(lens.idx[i]), res["part"][i], sc["parts"][i, 3]) for i in diff[:6]])
    for i in range(0, len(lens.query), 7):                                  # and the relation the host test pins on the oracle: part is the sum of sim in list order
        k = int(res["counts"][i])
        assert bits(res["part"][i]) == bits(PE.sum_in_order(res["sim"][i, :k])), i
    print("mated pairs with two or more texture survivors: %d of %d; lengths %s" % (mated, n, sorted({int(c) for c in res["counts"]})[:8]))
    assert mated >= 0.9 * n, (name, ref_tie, mated, n)
    assert 200 in res["counts"] and (res["counts"] < 200).any(), name         # both sides of the 200-row cut
    m.free_queries(qh)
    m.close()
    print("texture correspondences, %s, ref_tie_order %d: %d pairs, %.1f s" % (name, ref_tie, len(lens.query), time.perf_counter() - t0))


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------------------------
EDGE_BASE = 1000


def edge_world(cb):
    lats, gal = cases.small_set(cb)
    assert len(lats) == 3 and len(gal) == 40
    lats = list(lats) + [T.FPTemplate(minu=list(lats[0].minu[:3]), tex=[]), T.FPTemplate(minu=list(lats[0].minu), tex=[])]      # 3: latent-empty, 4: without a texture template
    gal = list(gal)
    gal[5] = T.FPTemplate(minu=list(gal[5].minu), tex=[])                   # a print without a texture template
    return lats, gal, 7                                                      # ... and the print that is removed


def raw_texture(m, qh, query, idx, with_optional):
    n = len(query)
    q = np.ascontiguousarray(query, np.int32); g = np.ascontiguousarray(idx, np.int64)
    counts = np.full(n, 77, np.int32); xy = np.full((n, 200, 4), 77, np.int16); pt = np.full((n, 200, 2), 77, np.int16); sim = np.full((n, 200), 77, np.float32); part = np.full(n, 77, np.float32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    opt = (p(pt, C.c_int16), p(sim, C.c_float), p(part, C.c_float)) if with_optional else (None, None, None)
    m._chk(m.lib.afis_texture_correspondences_pairs(m.ctx, qh[0], n, p(q, C.c_int32), p(g, C.c_int64), p(counts, C.c_int32), p(xy, C.c_int16), *opt))
    return counts, xy, pt, sim, part


@pytest.mark.gpu
def test_edges(codebook_bytes, cb, oracle):
    lats, gal, removed = edge_world(cb)
    m = M.Matcher(codebook_bytes)
    m.set_option("query_batch", 2)
    m.gallery_add(gal); m.gallery_commit(EDGE_BASE)
    m.gallery_remove([EDGE_BASE + removed])
    qh = m.upload_queries(lats)                                            # launch groups {0, 1}, {2, 3}, {4}
    sr = m.search_resident(qh, k=0, want_scores=True, want_parts=True)
    assert m.timing()["launch_groups"] >= 2 and (sr["status"] == 1).sum() == 1
    before = m.rank_hits(NINF, 8)
    rng = np.random.default_rng(41)
    order = rng.permutation(len(lats) * len(gal))
    order = np.concatenate([order, rng.choice(order, 10, replace=False)])   # ten pairs twice
    query = (order // len(gal)).astype(np.int32); local = (order % len(gal)).astype(np.int64)
    outside = np.array([-1, EDGE_BASE + len(gal), EDGE_BASE - 1, 5], np.int64)     # the list calls' pad, beyond the shard, before it, a shard-local index
    query = np.concatenate([query, np.array([0, 1, 2, 4], np.int32)]); idx = np.concatenate([local + EDGE_BASE, outside])
    n_in = len(order)
    res = m.texture_correspondences_pairs(qh, query, idx, want_parts=True)
    al = m.pair_alignments(qh, query, idx)
    corr = m.correspondences_pairs(qh, query, idx)
    sc = m.score_pairs(qh, query, idx, want_parts=True)
    # ---- the yardstick: the rules for what the reference does not run, the oracle's trace for everything else
    exp = Expected(oracle, codebook_bytes, lats, gal)
    n_run = 0
    for i in range(n_in):
        q, g = int(query[i]), int(local[i])
        not_run = q == 3 or q == 4 or g == 5 or g == removed
        if not_run:
            assert res["counts"][i] == M.CORR_NOT_RUN and res["corr"][i] is None and not res["xy"][i].any() and not res["pt"][i].any() and not bits(res["sim"][i]).any() and bits(res["part"][i]) == 0, (i, q, g)
            assert PE.of_record(al["moments"][i, 3]) == ZERO9, (i, q, g)
            if g != removed:
                assert oracle.trace(exp.ocb, exp.hl[q], exp.hr[g], which=0, stage=2, tie_mode=1) is None or q == 3, (q, g)      # the oracle does not run it either
            continue
        sim, li, ri = oracle.trace(exp.ocb, exp.hl[q], exp.hr[g], which=0, stage=2, tie_mode=1)
        same_export(res, i, sim, li, ri, lats[q], gal[g], (i, q, g))
        n_run += 1
    assert n_run >= 3 * 38 and (res["counts"][:n_in] >= 2).sum() >= 3
    assert np.array_equal(bits(res["part"]), bits(sc["parts"][:, 3]))
    assert (res["counts"][n_in:] == M.CORR_NOT_COVERED).all() and all(c is M.NOT_COVERED for c in res["corr"][n_in:]) and not res["xy"][n_in:].any() and not bits(res["part"][n_in:]).any()
    assert (al["status"][:n_in] == M.PAIR_OK).all() and (al["status"][n_in:] == M.PAIR_NOT_COVERED).all() and not al["moments"][n_in:].tobytes().strip(b"\0")
    for i in range(n_in):                                                   # the moments of the library's own exports; nothing for the latent-empty query and the removed print
        q, g = int(query[i]), int(local[i])
        for s in range(3):
            n = max(int(corr["counts"][i, s]), 0)
            assert PE.of_record(al["moments"][i, s]) == PE.moments_of_xy(corr["xy"][i, s, :n]), (i, q, g, s)
        n = max(int(res["counts"][i]), 0)
        assert PE.of_record(al["moments"][i, 3]) == PE.moments_of_xy(res["xy"][i, :n], texture=True), (i, q, g)
        if q == 3 or g == removed:
            assert not al["moments"][i].tobytes().strip(b"\0"), (i, q, g)
    i = int(np.flatnonzero((query[:n_in] == 4) & (local == 0))[0])          # the latent without texture against latent 0's mate: minutiae records, no texture record
    assert al["moments"][i, 0]["n"] >= 2 and al["moments"][i, 3]["n"] == 0
    for i in range(n_in - 10, n_in):                                        # a repeated pair: identical bytes
        j = int(np.flatnonzero(order[:n_in - 10] == order[i])[0])
        for k in ("counts", "xy", "pt", "sim", "part"):
            assert res[k][i].tobytes() == res[k][j].tobytes(), (i, j, k)
        assert al["moments"][i].tobytes() == al["moments"][j].tobytes()
    # ---- chunks of 7: the same bytes
    m.set_option("corr_pairs_per_launch", 7)
    res7 = m.texture_correspondences_pairs(qh, query, idx, want_parts=True)
    al7 = m.pair_alignments(qh, query, idx)
    assert m.get_option("texture_correspondences_us") > 0 and m.get_option("pair_alignments_us") > 0
    for k in ("counts", "xy", "pt", "sim", "part"):
        assert res7[k].tobytes() == res[k].tobytes(), k
    assert al7["status"].tobytes() == al["status"].tobytes() and al7["moments"].tobytes() == al["moments"].tobytes()
    m.set_option("corr_pairs_per_launch", 8192)
    # ---- NULL optional outputs, n_pairs == 0
    counts, xy, pt, sim, part = raw_texture(m, qh, query, idx, with_optional=False)
    assert counts.tobytes() == res["counts"].tobytes() and xy.tobytes() == res["xy"].tobytes() and (pt == 77).all() and (sim == 77).all() and (part == 77).all()
    counts, xy, pt, sim, part = raw_texture(m, qh, query, idx, with_optional=True)
    assert pt.tobytes() == res["pt"].tobytes() and sim.tobytes() == res["sim"].tobytes() and part.tobytes() == res["part"].tobytes()
    none = m.texture_correspondences_pairs(qh, [], [], want_parts=True)
    assert len(none["counts"]) == 0 and m.get_option("texture_correspondences_us") == 0
    assert len(m.pair_alignments(qh, [], [])["status"]) == 0 and m.get_option("pair_alignments_us") == 0
    with pytest.raises(M.AfisError):
        m.texture_correspondences_pairs(qh, [len(lats)], [EDGE_BASE])       # a query outside the handle
    with pytest.raises(M.AfisError):
        m.pair_alignments(qh, [-1], [EDGE_BASE])
    # ---- the last search's matrix stayed: the same lists before and after
    after = m.rank_hits(NINF, 8)
    for key in ("n_hits", "idx", "score"):
        assert before[key].tobytes() == after[key].tobytes(), key
    m.free_queries(qh)
    m.close()


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "generic"])
def test_alignments_at_every_length(codebook_bytes, ev, name):
    """Every field of all four records equals the integer moments of the oracle's traces, and of the library's own exported correspondences; the rigid geometry's texture
    record fits to c == 1, s == 0, t == 16 x LIST_TEX_MOVE pixels and rms == 0.0 exactly."""
    t0 = time.perf_counter()
    lens, rig = ev.lens, ev.rig
    _, _, minu_shift = CLASSES[name]
    lats, gal, _, _ = ev.handles(name)
    tex = ev.texture(name, 1)
    exp = forms.fill(lens.expected(minu_shift), lens.query, lens.idx, 1)
    m = M.Matcher(codebook_bytes)
    m.gallery_add(gal); m.gallery_commit(0)
    qh = m.upload_queries(lats)
    al = m.pair_alignments(qh, lens.query, lens.idx)
    assert m.get_option("pair_alignments_us") > 0 and (al["status"] == M.PAIR_OK).all()
    corr = m.correspondences_pairs(qh, lens.query, lens.idx)
    own = m.texture_correspondences_pairs(qh, lens.query, lens.idx)
    n_records, n_rigid = 0, 0
    for i, (q, g) in enumerate(zip(lens.query, lens.idx)):
        q, g = int(q), int(g)
        where = (name, rig.cases[q]["geometry"], rig.cases[q]["N"], rig.cases[q]["spec"], g)
        minu = exp.pair(q, g, 1)
        for s in range(3):
            got = PE.of_record(al["moments"][i, s])
            assert got == (PE.moments_of_xy(minu[s]) if minu[s] is not None else ZERO9), (where, s)
            assert got == PE.moments_of_xy(corr["xy"][i, s, :max(int(corr["counts"][i, s]), 0)]), (where, s)
            n_records += got[0] > 0
        sim, li, ri = tex[(q, g)]
        got = PE.of_record(al["moments"][i, 3])
        assert got == PE.moments_of_xy(tex_points(lats[q], gal[g], li, ri), texture=True), where
        assert got == PE.moments_of_xy(own["xy"][i, :max(int(own["counts"][i]), 0)], texture=True), where
        n_records += got[0] > 0
        if q == g and rig.cases[q]["geometry"] == "rigid" and rig.cases[q]["N"] >= 2:
            assert got[0] == min(rig.cases[q]["N"], 200), where
            fit = m.alignment_fit(al["moments"][i, 3])
            assert fit == (1.0, 0.0, 16.0 * cases.LIST_TEX_MOVE[0], 16.0 * cases.LIST_TEX_MOVE[1], 0.0), (where, fit)
            n_rigid += 1
    assert n_rigid == len(cases.LIST_TEX_N) - 1 and n_records >= 0.9 * 4 * lens.n, (n_rigid, n_records)
    m.free_queries(qh)
    m.close()
    print("alignments, %s: %d pairs, %d records with survivors, %.1f s" % (name, len(lens.query), n_records, time.perf_counter() - t0))


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(oracle):
    return World("shipped", oracle)


def view_as_latent(world, a):
    """Print a's view as a latent whose 27th minutiae template is the print's and whose texture template is the view's (what the print forms build on the device)."""
    v = world.views[a]
    return T.FPTemplate(minu=[world._stand_in] * 26 + [v.minu[0]] if v.minu else [], tex=list(v.tex))


@pytest.mark.gpu
def test_print_pairs_equal_the_latent_forms_over_the_prints_views(world):
    m = open_matcher(world.cbb, world.enrolled, print_pairs_batch_prints=4, corr_pairs_per_launch=50)
    qs = [0, 3, 5, BIG, NO_MINU, NO_TEX, 13, 15, 17, 19]
    pairs = [(x, y) for x in qs for y in (1, 5, BIG, NO_MINU, NO_TEX, EMPTY, REMOVED, 13, 18)] + [(x, x) for x in qs] + [(EMPTY, 5), (REMOVED, 13), (EMPTY, EMPTY), (13, 15), (13, 15)]
    a = np.array([p[0] for p in pairs]); b = np.array([p[1] for p in pairs])
    order = np.random.default_rng(8).permutation(len(pairs))
    a, b = a[order], b[order]
    got = m.texture_correspondences_print_pairs(a + BASE, b + BASE, want_parts=True)
    assert m.get_option("texture_correspondences_us") > 0
    gal = m.print_pair_alignments(a + BASE, b + BASE)
    assert m.get_option("pair_alignments_us") > 0 and (gal["status"] == M.PAIR_OK).all()
    sc = m.score_print_pairs(a + BASE, b + BASE, 1.0, 1.0, want_parts=True)
    assert np.array_equal(bits(got["part"]), bits(sc["parts"][:, 1]))       # part is the score call's texture entry
    mc = m.correspondences_print_pairs(a + BASE, b + BASE)
    # ---- the latent forms over a handle uploaded from the same prints' views
    qh = m.upload_queries([view_as_latent(world, x) for x in qs])
    sel = np.flatnonzero([x in qs for x in a])
    pos = np.array([qs.index(int(a[i])) for i in sel], np.int32)
    ref = m.texture_correspondences_pairs(qh, pos, b[sel] + BASE, want_parts=True)
    ral = m.pair_alignments(qh, pos, b[sel] + BASE)
    for k in ("counts", "xy", "pt", "sim", "part"):
        assert got[k][sel].tobytes() == ref[k].tobytes(), k
    assert gal["moments"][sel][:, 0].tobytes() == ral["moments"][:, 0].tobytes() and gal["moments"][sel][:, 1].tobytes() == ral["moments"][:, 3].tobytes()
    n_self = 0
    for i, (qa, qb) in enumerate(zip(a, b)):
        qa, qb = int(qa), int(qb)
        nta, ntb = (COUNTS[x][1] if world.counts[x][1] else 0 for x in (qa, qb))   # texture points as enrolled; none for the empty and the removed entry
        if nta == 0 or ntb == 0:                                            # a or b holds no texture template (empty and removed entries included)
            assert got["counts"][i] == M.CORR_NOT_RUN and got["corr"][i] is None and not got["xy"][i].any() and bits(got["part"][i]) == 0, (qa, qb)
        else:
            assert got["counts"][i] >= 0 and got["pt"][i, :got["counts"][i], 0].max(initial=0) < min(nta, 1000) and got["pt"][i, :got["counts"][i], 1].max(initial=0) < min(ntb, 1000), (qa, qb)
        assert PE.of_record(gal["moments"][i, 1]) == PE.moments_of_xy(got["xy"][i, :max(int(got["counts"][i]), 0)], texture=True), (qa, qb)
        assert PE.of_record(gal["moments"][i, 0]) == PE.moments_of_xy(mc["xy"][i, :max(int(mc["counts"][i]), 0)]), (qa, qb)
        if qa == qb and got["counts"][i] >= 2:                              # (a, a) is an ordinary pair: every point lies on itself
            n = int(got["counts"][i])
            assert np.array_equal(got["pt"][i, :n, 0], got["pt"][i, :n, 1]) and m.alignment_fit(gal["moments"][i, 1]) == (1.0, 0.0, 0.0, 0.0, 0.0), (qa, got["pt"][i, :n].tolist())
            n_self += 1
    assert n_self >= 5, n_self
    two = np.flatnonzero((a == 13) & (b == 15))                             # a repeated pair: identical bytes
    assert len(two) == 2 and got["xy"][two[0]].tobytes() == got["xy"][two[1]].tobytes() and gal["moments"][two[0]].tobytes() == gal["moments"][two[1]].tobytes()
    # ---- a pair straddling the shard, and the pads
    sa = np.array([13, G, -1 - BASE, 13], np.int64) + BASE; sb = np.array([G, 13, 13, -1 - BASE], np.int64) + BASE
    out = m.texture_correspondences_print_pairs(sa, sb, want_parts=True)
    assert (out["counts"] == M.CORR_NOT_COVERED).all() and not out["xy"].any() and not bits(out["part"]).any()
    oal = m.print_pair_alignments(sa, sb)
    assert (oal["status"] == M.PAIR_NOT_COVERED).all() and not oal["moments"].tobytes().strip(b"\0")
    assert len(m.texture_correspondences_print_pairs([], [])["counts"]) == 0 and len(m.print_pair_alignments([], [])["status"]) == 0
    m.free_queries(qh)
    m.close()
