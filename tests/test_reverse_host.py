"""Reverse search without a GPU: the two entry points are declared, exported by both libraries and bound by the Python host; the parity taps are the test library's
alone; the kernel and the host unit are product objects; the option is documented; merge_prints_to_card is held against a brute-force model, and merge_hits against the
unsplit model on column lists whose latents are split over parts.  (What a column list holds is tests/test_gpu_reverse_search.py's.)"""
import importlib
import os
import re

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afis_queries_upload_reserved", "afis_rank_latent_hits")
TAPS = ("afis_debug_rank_latent_hits", "afis_debug_transpose_stats")


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):        # dlopen only: no device call
        for name in NEW:
            assert re.search(r"\bint\s+%s\s*\(afis_ctx\*" % name, code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert getattr(lib, name).argtypes is not None, name
    for method in ("upload_queries", "rank_latent_hits", "rank_latents", "debug_rank_latent_hits", "reverse_search"):
        assert hasattr(M.Matcher, method), method
    import inspect
    assert "reserve" in inspect.signature(M.Matcher.upload_queries).parameters
    assert inspect.signature(M.Matcher.rank_latent_hits).parameters["latent_base"].default == 0
    assert re.search(r'"rank_latents_us" \(read-only\)', hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")])
    assert "`rank_latents_us`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_taps_are_the_test_librarys_alone():
    taps = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read(), flags=re.S)
    tlib = M.load_library(M.TEST_LIB_PATH)
    for tap in TAPS:
        assert re.search(r"\bint\s+%s\s*\(afis_ctx\*" % tap, taps), tap
        assert tap in M.TAP_EXPORTS and tap not in M.EXPORTS
        assert tap not in open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
        assert not hasattr(M.load_library(), tap)
        assert hasattr(tlib, tap) and getattr(tlib, tap).argtypes is not None


def test_the_kernel_and_the_host_unit_are_product_objects():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "latent_rank.o" in objs and "afis_reverse.o" in objs
    assert re.search(r"^TEST_OBJS\s*=\s*\$\(OBJS\)", mk, flags=re.M)          # the test library is the product objects plus the taps
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "latent_rank.hip")).read()
    assert "__global__" in src and "k_transpose_scores" in src and "size_t" in src
    pitch = int(re.search(r"kTrPitch\s*=\s*kTrTile\s*\+\s*(\d+)", src).group(1)) + int(re.search(r"kTrTile\s*=\s*(\d+)", src).group(1))
    # the bank rule (ds_write_b32 / ds_read_b32: bank = dword address % 32, conflicts inside a 32-lane half): a row written by lanes = columns, a column read by lanes = rows
    for half in (0, 32):
        lanes = np.arange(half, half + 32)
        assert len(set((5 * pitch + lanes) % 32)) == 32 and len(set((lanes * pitch + 5) % 32)) == 32
    host = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "afis_reverse.cpp")).read()
    assert "launch_rank_hits" in host and "check_hits" in host and "__global__" not in host     # no second selection kernel: k_rank_hits on the transposed matrix


# ---- merge_prints_to_card against a brute-force model ---------------------------------------------------------------------------------------------
def brute_card(latent, score, cap):
    """Every (latent, score, print) entry of the input by plain loops: per latent the greatest score, on equal scores the lowest print; then score descending, latent ascending."""
    best = {}
    for p in range(latent.shape[0]):
        for r in range(latent.shape[1]):
            l, s = int(latent[p, r]), score[p, r]
            if l < 0:
                continue
            if l not in best or s > best[l][0]:                             # (equal scores keep the earlier print; -0.0 == +0.0)
                best[l] = (s, p)
    rows = sorted(best.items(), key=lambda kv: (-float(kv[1][0]), kv[0]))[:cap]
    out_l = np.full(cap, -1, np.int64); out_s = np.full(cap, -np.inf, np.float32); out_p = np.full(cap, -1, np.int64)
    for i, (l, (s, p)) in enumerate(rows):
        out_l[i], out_s[i], out_p[i] = l, s, p
    return out_l, out_s, out_p, len(best)


def print_lists(col_scores, thr, kk, latent_base=0):
    """The column lists of P prints from [P][n_lat] scores: (n_hits [P], latent [P][kk], score [P][kk]) as Matcher.rank_latent_hits gives them."""
    P, L = col_scores.shape
    nh = np.empty(P, np.int64); li = np.full((P, kk), -1, np.int64); ls = np.full((P, kk), -np.inf, np.float32)
    for p in range(P):
        at = np.flatnonzero(col_scores[p] >= thr)
        at = at[np.lexsort((at, -col_scores[p, at].astype(np.float64)))]
        nh[p] = len(at)
        li[p, :min(kk, len(at))] = latent_base + at[:kk]; ls[p, :min(kk, len(at))] = col_scores[p, at[:kk]]
    return nh, li, ls


@pytest.mark.parametrize("cap,kk", [(5, 5), (5, 12), (40, 40), (64, 300)])
def test_merge_prints_to_card_against_a_brute_force_model(cap, kk):
    """Ten prints x 200 latents, scores rounded to a few values (the tie rules decide nearly every place) with a -0.0 among the zeros; nearly every latent is present in
    several prints' lists; kk > what qualifies pads the lists, kk below it truncates them."""
    rng = np.random.default_rng(31 + cap)
    sc = np.round(rng.random((10, 200)) * 6).astype(np.float32)
    sc[rng.random(sc.shape) < 0.5] = 0.0
    sc[:, 17] = 0.0; sc[3, 17] = -0.0; sc[:, 18] = 0.0; sc[0, 18] = -0.0
    assert np.signbit(sc[3, 17]) and (sc[:, 17] <= 0).all()
    for thr in (-np.inf, 0.0, 3.0, 7.0):
        nh, li, ls = print_lists(sc, thr, kk)
        got = SH.merge_prints_to_card(nh, li, ls, cap)
        want = brute_card(li, ls, cap)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64 and got[0].shape == (cap,)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(got[2], want[2]), (thr, cap, kk)
        assert got[3] == want[3] and got[4] == bool((nh > kk).any())
        # ... and against the card's own scores, not only the lists handed over: the list is exact, cut or not; the count while no print was cut
        card = sc.max(axis=0)
        at = np.flatnonzero(card >= thr)
        at = at[np.lexsort((at, -card[at].astype(np.float64)))]
        t = min(cap, len(at))
        assert np.array_equal(got[0][:t], at[:t]) and np.array_equal(got[1][:t], card[at[:t]]) and (got[0][t:] == -1).all()
        assert np.array_equal(got[2][:t], np.argmax(sc[:, at[:t]] == card[at[:t]], axis=0))       # the lowest print position that holds the maximum
        assert got[3] == len(at) if not got[4] else got[3] <= len(at)
        if thr == 7.0:
            assert got[3] == 0 and not got[4] and np.isneginf(got[1]).all()
        if thr == -np.inf:
            assert got[4] == (kk < 200)
    # latents 17 and 18 are +-0 everywhere: they arrive from print 0 (the lowest position among equal scores) whatever sign the zeros carry, 18 with print 0's -0.0
    nh, li, ls = print_lists(sc, 0.0, 300)
    l, s, p, n, trunc = SH.merge_prints_to_card(nh, li, ls, 300)
    assert p[l.tolist().index(17)] == 0 and p[l.tolist().index(18)] == 0 and np.signbit(s[l.tolist().index(18)]) and not np.signbit(s[l.tolist().index(17)]) and not trunc and n == 200


def test_merge_hits_on_column_lists_split_by_latents():
    """One random matrix [90 latents][7 prints]; the latents split by rows into 1, 2 and 3 parts, each part's column lists carrying its latent_base: merge_hits gives
    the unsplit lists."""
    rng = np.random.default_rng(47)
    sc = np.round(rng.random((90, 7)) * 5).astype(np.float32)
    sc[rng.random(sc.shape) < 0.3] = -1.0
    for thr, cap in ((-np.inf, 10), (0.0, 64), (2.0, 10), (6.0, 10)):
        want = print_lists(np.ascontiguousarray(sc.T), thr, cap)
        for cuts in ([0, 90], [0, 31, 90], [0, 30, 30, 90]):                # (the three-part split has an empty part)
            parts = [print_lists(np.ascontiguousarray(sc[a:b].T), thr, cap, latent_base=a) for a, b in zip(cuts, cuts[1:])]
            n, li, ls = SH.merge_hits(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]), cap)
            assert np.array_equal(n, want[0]) and np.array_equal(li, want[1]) and np.array_equal(ls.view(np.uint32), want[2].view(np.uint32)), (thr, cap, cuts)
    assert "reverse search" in SH.merge_hits.__doc__ and "latent_base" in SH.merge_hits.__doc__
