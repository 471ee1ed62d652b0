"""One rank-list order on every path, on the GPU: the rank list of afis_search* — k_topk (minu.hip) for k <= 64, the host's list (csrc/rank_order.h) beyond — fed
hand-made matrices through the parity tap afis_debug_rank_rows, on either side of the k = 64 | 65 switch, and held against afis_rank_hits on the same matrix.

The yardstick is numpy throughout: np.lexsort((global_index, -key.astype(np.int64))), key = the ordered bits of score + 0.0f (tests/test_gpu_rank_hits.py::template_key).
Indices and raw score words are compared with np.array_equal, padding (-1, -inf) included.

k_topk runs one 1024-thread workgroup per query in a strided pass: the gallery sizes sit on, one before and one after the wave (64) and workgroup (1024) edges, 4099
ends on a trip that is partly empty.  The galleries are one-minutia, one-texture-point templates (tests/test_gpu_rank_hits.py's tap gallery): nothing is searched but
the four-print set of the last two tests.

A hit list at min_score = -inf is the rank list short of the entries that lie BELOW -inf — NaNs with the sign set, which reach no min_score (include/afis_matcher.h, and
tests/test_gpu_rank_hits.py::test_tap_sweep_templates counts them out): on rows that hold none the two are equal entry for entry, on the others the hit list is the rank
list with those tail entries as padding.  hits_of_list states that once for every comparison below."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import test_gpu_rank_hits as RH

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 6053
BASE = 1000
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4099)
NEG_INF_WORD = np.uint32(0xff800000)
KEY_NEG_INF = int(RH.template_key(np.array([-np.inf], np.float32))[0])
QNAN, QNAN_NEG = 0x7fc00000, 0xffc00000
ROW_TWO_NANS = 9
HITS_MAX = 4096
# How many of the four pair scores of cases.nan_inf_set's NaN / inf latent are NaN or otherwise non-finite, as measured on an MI355X (test_a_real_search_with_a_nan_latent):
# none.  The fused scores were 3.561502, 1.0029199, 0.0, 271.44421 (words 4063efa6 3f805fae 00000000 4387b8dc): the NaN row maxima do not reach the pair score.
NON_FINITE_SCORES_MEASURED = 0


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """4099 rolled templates of one minutia and one texture point each, as one packed gallery."""
    G = max(SIZES)
    rng = np.random.default_rng(SEED)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    return S.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
                           off.copy(), rng.integers(0, 30, G).astype(np.int16), rng.integers(0, 30, G).astype(np.int16), rng.uniform(-1.5, 1.5, G).astype(np.float32),
                           rng.integers(0, cb.K, (G, cb.M)).astype(np.uint8))


def rows_of(n, rng):
    """The nine kinds of RH.matrix and a tenth: finite values (small integers: many ties) except one 0x7fc00000 and one 0xffc00000 at random places."""
    rows = np.empty((10, n), np.float32)
    rows[:9] = RH.matrix(n, rng)
    rows[ROW_TWO_NANS] = rng.integers(-8, 32, n).astype(np.float32)
    w = rows[ROW_TWO_NANS].view(np.uint32)
    for p, word in zip(rng.permutation(n)[:2], (QNAN, QNAN_NEG)):
        w[p] = word
    return rows


def model_lists(scores, glob, k):
    """(idx [n_q][k], score words [n_q][k]) of a matrix whose column j is template glob[j]."""
    glob = np.asarray(glob, np.int64)
    idx = np.full((scores.shape[0], k), -1, np.int64); sc = np.full((scores.shape[0], k), NEG_INF_WORD, np.uint32)
    for q in range(scores.shape[0]):
        o = np.lexsort((glob, -RH.template_key(scores[q]).astype(np.int64)))[:k]
        idx[q, :len(o)] = glob[o]; sc[q, :len(o)] = scores[q].view(np.uint32)[o]
    return idx, sc


def assert_lists(got, want, what):
    gi, gs = got["topk_idx"], got["topk_score"].view(np.uint32)
    assert gi.shape == want[0].shape and np.array_equal(gi, want[0]), (what, "idx", np.argwhere(gi != want[0])[:6].tolist(), gi.ravel()[:8].tolist(), want[0].ravel()[:8].tolist())
    assert np.array_equal(gs, want[1]), (what, "score", np.argwhere(gs != want[1])[:6].tolist())


def hits_of_list(idx, words):
    """What afis_rank_hits(-inf, cap = k) returns for a rank list of length k: its entries, those below -inf (they stand at the tail) as padding."""
    reach = RH.template_key(words.view(np.float32)).astype(np.int64) >= KEY_NEG_INF
    return np.where(reach, idx, -1), np.where(reach, words, NEG_INF_WORD), (reach & (idx >= 0)).sum(axis=1)


def assert_hits_are_the_list(m, lists, k, n_cols, what):
    h = m.rank_hits(float("-inf"), k)
    wi, ws, wn = hits_of_list(*lists)
    assert np.array_equal(h["idx"], wi) and np.array_equal(h["score"].view(np.uint32), ws), (what, "rank_hits(-inf)")
    assert np.array_equal(np.minimum(h["n_hits"], k), wn) and (h["n_hits"] <= n_cols).all(), (what, "n_hits")
    return h


def ks_for(G):
    ks = [1, 24, 64, 65, 100, G + 3]                                        # G + 3: k > G on the host's side of the switch ...
    if G + 1 <= 64:
        ks.append(G + 1)                                                    # ... and on the device's
    return sorted(set(ks))


def matrices(rows):
    """The ten kinds as matrices of one and of three queries; with three, the middle row is all -1 (a latent-empty query)."""
    n = rows.shape[1]
    minus = np.full(n, -1, np.float32)
    out = [(a, b) for a, b in ((0, 1), (2, 3), (4, 5), (6, 7), (RH.ROW_SPECIAL, ROW_TWO_NANS))]
    return [((a, -1, b), np.stack([rows[a], minus, rows[b]])) for a, b in out] + [((a,), rows[a:a + 1].copy()) for a in (RH.ROW_SPECIAL, ROW_TWO_NANS, 3)]


# ---- 1: the tap sweep -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", SIZES)
def test_tap_sweep(G, codebook_bytes, tiny):
    m = M.Matcher(codebook_bytes, taps=True)
    m.gallery_add_packed(tiny.slice(0, G)); m.gallery_commit(BASE)
    rows = rows_of(G, np.random.default_rng(SEED + G))
    glob = BASE + np.arange(G)
    seen = set()
    for kinds, mat in matrices(rows):
        seen.update(kinds)
        got64 = None
        for k in ks_for(G):
            got = m.debug_rank_rows(mat, k)
            want = model_lists(mat, glob, k)
            assert_lists(got, want, (G, kinds, k))
            if k == 64:
                got64 = got
            if k == 65:                                                     # across the switch from the device's list to the host's: one list
                assert np.array_equal(got["topk_idx"][:, :64], got64["topk_idx"]) and np.array_equal(got["topk_score"][:, :64].view(np.uint32), got64["topk_score"].view(np.uint32)), (G, kinds)
            if k <= HITS_MAX:                                               # the matrix the tap uploaded is the context's last search: the hit lists rank it
                h = assert_hits_are_the_list(m, (got["topk_idx"], got["topk_score"].view(np.uint32)), k, G, (G, kinds, k))
                clean = [q for q in range(mat.shape[0]) if not (RH.template_key(mat[q]).astype(np.int64) < KEY_NEG_INF).any()]
                assert np.array_equal(h["idx"][clean], got["topk_idx"][clean]) and np.array_equal(h["score"][clean].view(np.uint32), got["topk_score"][clean].view(np.uint32))   # entry for entry
        if len(kinds) == 3:                                                 # the latent-empty query lists ascending indices
            k = min(G, 24)
            assert np.array_equal(m.debug_rank_rows(mat, k)["topk_idx"][1], glob[:k])
    assert seen == set(range(10)) | {-1}
    m.close()


# ---- 2: a subset listed out of order ------------------------------------------------------------------------------------------------------------------------
def test_subset_leg(codebook_bytes, tiny):
    G, base = 1025, 5_000_000_000
    rng = np.random.default_rng(SEED + 2)
    m = M.Matcher(codebook_bytes, taps=True)
    m.gallery_add_packed(tiny.slice(0, G)); m.gallery_commit(base)
    listed = base + rng.permutation(G)[:203].astype(np.int64)                 # the caller's order: shuffled
    assert not (np.diff(listed) > 0).all()
    hs = m.subset_create(listed)
    held = np.sort(listed)                                                    # the order the device holds the columns in: what the tap takes
    rows = rows_of(len(listed), rng)
    mat = np.concatenate([rows, np.full((1, len(listed)), -1, np.float32)])
    lists = {}
    for k in (24, 64, 65, 100):
        got = m.debug_rank_rows(mat, k, subset=hs)
        assert_lists(got, model_lists(mat, held, k), ("subset", k))
        assert np.isin(got["topk_idx"], listed).all() and got["topk_idx"].min() >= base
        assert_hits_are_the_list(m, (got["topk_idx"], got["topk_score"].view(np.uint32)), k, len(listed), ("subset", k))
        lists[k] = got
    for a, b in ((24, 64), (64, 65), (65, 100)):                              # one list on both paths: equal keys by ascending GLOBAL index on either
        assert np.array_equal(lists[b]["topk_idx"][:, :a], lists[a]["topk_idx"]) and np.array_equal(lists[b]["topk_score"][:, :a].view(np.uint32), lists[a]["topk_score"].view(np.uint32))
    for k in (64, 100):
        assert np.array_equal(lists[k]["topk_idx"][2], held[:k]) and np.array_equal(lists[k]["topk_idx"][10], held[:k])   # all +0.0, all -1: ascending global index
    got = m.debug_rank_rows(mat, 300, subset=hs)                              # k beyond the subset: padding
    assert_lists(got, model_lists(mat, held, 300), ("subset", 300))
    assert (got["topk_idx"][:, 203:] == -1).all()
    m.subset_free(hs)
    m.close()


# ---- 3: a real search whose latent holds NaN and infinite descriptors ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nan_set(cb):
    return cases.nan_inf_set(cb)


def test_a_real_search_with_a_nan_latent(codebook_bytes, nan_set):
    """The search tests/test_gpu_parity.py::test_bound_pass_with_nan_and_inf_latent_descriptors runs, with its fused scores and rank lists read this time.
    Measured on an MI355X: none of the four fused scores is NaN or infinite (NON_FINITE_SCORES_MEASURED, with the score words) — a NaN score is a case of the
    contract (the tap sweep above), not one this latent produces.  The lists are held against the model whichever way the scores fall."""
    lat, clean, gal = nan_set
    m = M.Matcher(codebook_bytes, taps=True)
    m.gallery_add(gal); m.gallery_commit(BASE)
    glob = BASE + np.arange(len(gal))
    r24 = m.search([lat], k=24, want_scores=True)
    scores = r24["scores"]
    n_bad = int((~np.isfinite(scores)).sum())
    print("nan_inf_set: fused scores %s words %s: %d of %d NaN or non-finite (%d NaN)" % (scores[0].tolist(), ["%08x" % w for w in scores.view(np.uint32)[0].tolist()], n_bad, scores.size, int(np.isnan(scores).sum())))
    assert scores.shape == (1, 4)
    assert n_bad == NON_FINITE_SCORES_MEASURED
    h24 = m.rank_hits(float("-inf"), 24)
    r100 = m.search([lat], k=100, want_scores=True)
    assert np.array_equal(r100["scores"].view(np.uint32), scores.view(np.uint32))
    want24, want100 = model_lists(scores, glob, 24), model_lists(scores, glob, 100)
    assert_lists(r24, want24, "k = 24"); assert_lists(r100, want100, "k = 100")
    assert np.array_equal(r100["topk_idx"][:, :24], r24["topk_idx"]) and np.array_equal(r100["topk_score"][:, :24].view(np.uint32), r24["topk_score"].view(np.uint32))
    wi, ws, wn = hits_of_list(*want24)
    assert np.array_equal(h24["idx"], wi) and np.array_equal(h24["score"].view(np.uint32), ws) and np.array_equal(h24["n_hits"], wn)
    assert sorted(r24["topk_idx"][0, :4].tolist()) == glob.tolist() and (r24["topk_idx"][0, 4:] == -1).all()       # every print listed once, whatever its score holds
    # the clean twin
    c24 = m.search([clean], k=24, want_scores=True); c100 = m.search([clean], k=100, want_scores=True)
    assert np.isfinite(c24["scores"]).all() and np.array_equal(c24["scores"], c100["scores"])
    assert_lists(c24, model_lists(c24["scores"], glob, 24), "clean, k = 24"); assert_lists(c100, model_lists(c24["scores"], glob, 100), "clean, k = 100")
    assert np.array_equal(c100["topk_idx"][:, :24], c24["topk_idx"]) and np.array_equal(c100["topk_score"][:, :24].view(np.uint32), c24["topk_score"].view(np.uint32))
    m.close()


# ---- 4: `match -l` on the same latent ----------------------------------------------------------------------------------------------------------------------
def test_match_lists_every_print_of_the_nan_latent(codebook_bytes, nan_set, tmp_path):
    lat, _, gal = nan_set
    exe = os.path.join(os.path.dirname(M.LIB_PATH), "match")
    names = ["R%03d.dat" % j for j in range(len(gal))]
    box = str(tmp_path / "gal.afisgal")
    lat_dat = T.write_latent(lat)
    (tmp_path / "L0.dat").write_bytes(lat_dat)
    cbp = tmp_path / "cb.dat"; cbp.write_bytes(codebook_bytes)
    (tmp_path / "work").mkdir()
    m = M.Matcher(codebook_bytes)
    for g in gal:
        m.gallery_add_dat(T.write_rolled(g))
    m.gallery_save(box, names)                                               # a container: the CLI's gallery order is this one, not a directory listing's
    m.gallery_commit(0)
    for tie in (0, 1):
        m.set_option("ref_tie_order", tie)
        column = m.search_dat([lat_dat], k=0, want_scores=True)["scores"][0]
        want_idx, want_sc = m.rank_list(column, k=len(gal), ref_order=bool(tie))
        out_dir = tmp_path / ("o%d" % tie); out_dir.mkdir()
        o = subprocess.run([exe, "-l", str(tmp_path / "L0.dat"), "-g", box, "-c", str(cbp), "-s", str(out_dir) + "/", "-tie", str(tie)], capture_output=True, text=True, cwd=tmp_path / "work")
        assert o.returncode == 0, (tie, o.stdout[-2000:], o.stderr[-2000:])
        lines = (out_dir / "L0.csv").read_text().splitlines()
        assert lines[0] == "filename,score" and len(lines) == 1 + len(gal)
        listed = [os.path.basename(l.rsplit(",", 1)[0].split('"')[1]) for l in lines[1:]]
        assert sorted(listed) == names, (tie, listed)                        # every gallery file exactly once
        assert listed == [names[i] for i in want_idx], (tie, listed, want_idx.tolist(), column.tolist())
        for l, v in zip(lines[1:], want_sc):
            p = float(l.rsplit(",", 1)[1])
            assert (np.isnan(p) and np.isnan(v)) or p == v or abs(p - v) <= 1e-5 * abs(v), (tie, l, float(v))
    m.close()
