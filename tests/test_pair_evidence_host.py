"""Texture correspondences and pair alignments without a GPU: the six entry points are declared, exported by both libraries, bound by the Python host and absent from the
taps header; the kernel and the host unit are product objects and share csrc/pair_moments.h; the two options are documented; afis_corr_moments_add against Python
integers; afis_alignment_fit on planted quarter turns (exact) and on random integer point sets against the same formulas evaluated exactly (tests/pair_evidence_model.py
has the bounds and how they are counted); its refusals; the two sharding merges on hand-made per-rank outputs; and, on the oracle alone, that the fp32 sum of the stage-2
texture similarities in list order IS the oracle's texture part on the list-length set — the relation of `part` and `sim` the GPU test then uses.
(What the device answers is tests/test_gpu_pair_evidence.py's.)"""
import ctypes as C
import importlib
import os
import re
from decimal import Decimal

import numpy as np
import pytest

import cases
import pair_evidence_model as PE

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
T = importlib.import_module("msu-latentafis_amd.host.templates")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NEW = {"afis_texture_correspondences_pairs": 10, "afis_texture_correspondences_print_pairs": 9, "afis_pair_alignments": 7, "afis_print_pair_alignments": 6,
       "afis_corr_moments_add": 2, "afis_alignment_fit": 6}
OPTIONS = ("texture_correspondences_us", "pair_alignments_us")
EINVAL = -1
SEED = 9107


@pytest.fixture(scope="module", params=["product", "test"])
def lib(request):
    return M.load_library() if request.param == "product" else M.load_library(M.TEST_LIB_PATH)      # dlopen only: no device call


def rec(m):
    return PE.as_record(M.CORR_MOMENTS, m)


def fit(lib, m):
    """(rc, (c, s, tx, ty, rms)) of afis_alignment_fit; the outputs start as NaN."""
    r = rec(m)
    out = [C.c_double(float("nan")) for _ in range(5)]
    rc = lib.afis_alignment_fit(C.c_void_p(r.ctypes.data), *[C.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


# ---- declared, exported, bound, built, documented ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*int64_t\s+n,\s*slx,\s*sly,\s*srx,\s*sry,\s*dot,\s*cross,\s*ll,\s*rr;\s*\}\s*afis_corr_moments;", code)
    assert re.search(r"#define\s+AFIS_TEX_CORR_MAX\s+200\b", code)
    assert M.CORR_MOMENTS.itemsize == 72 and SH.CORR_MOMENTS == M.CORR_MOMENTS and M.CORR_MOMENTS.names == PE.FIELDS and M.TEX_CORR_MAX == 200
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):
        for name, n_args in NEW.items():
            assert re.search(r"\bint\s+%s\s*\(" % name, code), name
            assert name in M.EXPORTS and name not in M.TAP_EXPORTS and hasattr(lib, name)
            assert len(getattr(lib, name).argtypes) == n_args, name
            assert name not in taps, name
    for method in ("texture_correspondences_pairs", "texture_correspondences_print_pairs", "pair_alignments", "print_pair_alignments", "alignment_fit"):
        assert hasattr(M.Matcher, method), method
    assert hasattr(SH, "merge_texture_correspondences") and hasattr(SH, "merge_pair_alignments")
    assert hdr.index("int afis_correspondences_print_pairs(") < hdr.index("int afis_texture_correspondences_pairs(") < hdr.index("int afis_pair_alignments(") < hdr.index("int afis_search_cascade(")


def test_the_kernel_and_the_host_unit_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "pair_evidence.o" in objs and "afis_evidence.o" in objs
    assert "$(OBJS)" in re.search(r"^TEST_OBJS\s*=(.*)$", mk, flags=re.M).group(1)                   # both libraries are made of them
    src = open(os.path.join(CSRC, "pair_evidence.hip")).read()
    assert "__global__" in src and "k_pair_evidence" in src and '#include "pair_moments.h"' in src and "__shfl_xor" in src
    assert "atomic" not in re.sub(r"//.*", "", src)                         # ordinary stores only
    assert '#include "pair_moments.h"' in open(os.path.join(CSRC, "afis_ctx.h")).read()             # one text for the kernel and the host units
    h = open(os.path.join(CSRC, "pair_moments.h")).read()
    assert "THE BOUND" in h and "2^29" in h and "2^50" in h and "560" in h  # the bound on every field is stated, as score_stats.h states its own
    pairs_unit = open(os.path.join(CSRC, "graph.hip")).read()
    assert "const GraphTap tap{tap_out, tap_n, 2};" in pairs_unit[pairs_unit.index("#else    // AFIS_GRAPH_PAIRS_UNIT"):]      # the pair launcher hands the kernel a real tap


def test_the_options_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only\)' % opt, hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]), opt
        assert "`%s`" % opt in integ, opt
    assert "afis_rank_hits" in integ and "afis_pair_alignments" in integ and "afis_alignment_fit" in integ


# ---- afis_corr_moments_add ---------------------------------------------------------------------------------------------------------------------------
def random_points(rng, n, whole_range):
    if whole_range:
        return tuple(rng.integers(-32768, 32768, n) for _ in range(4))
    ox, oy = rng.integers(-32768, 32768 - 50, 2)
    return tuple(rng.integers(0, 50, n) + o for o in (ox, oy, ox, oy))


def test_moments_add_against_python_integers(lib):
    rng = np.random.default_rng(SEED)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for trial in range(40):
        sizes = [int(v) for v in rng.integers(0, 121, 3)] + [int(rng.integers(0, 201))]
        parts = []
        for k, n in enumerate(sizes):
            lx, ly, rx, ry = random_points(rng, n, trial % 2 == 0)
            parts.append(PE.moments(*(PE.texture_px(v) for v in (lx, ly, rx, ry))) if k == 3 else PE.moments(lx, ly, rx, ry))
        acc, want = rec((0,) * 9), (0,) * 9
        for m in parts:
            assert PE.in_bound(m)
            assert lib.afis_corr_moments_add(p(acc), p(rec(m))) == 0
            want = PE.add(want, m)
            assert PE.of_record(acc[0]) == want
    # the extreme record: 560 points at the largest texture pixel coordinate on both sides is inside the bound, one more point is not
    far = [32767] * 560
    top = PE.moments(*(PE.texture_px(far) for _ in range(4)))
    assert PE.in_bound(top) and top[1] < 2 ** 29 and top[5] < 2 ** 50 and top[7] < 2 ** 50
    acc = rec((0,) * 9)
    assert lib.afis_corr_moments_add(p(acc), p(rec(top))) == 0 and PE.of_record(acc[0]) == top
    one = rec(PE.moments([1], [2], [3], [4]))
    before = acc.tobytes()
    assert lib.afis_corr_moments_add(p(acc), p(one)) == EINVAL and acc.tobytes() == before           # n would pass 560
    assert lib.afis_corr_moments_add(None, p(one)) == EINVAL and lib.afis_corr_moments_add(p(acc), None) == EINVAL
    bad = rec((-1, 0, 0, 0, 0, 0, 0, 0, 0))
    fresh = rec((0,) * 9)
    assert lib.afis_corr_moments_add(p(fresh), p(bad)) == EINVAL and not fresh.tobytes().strip(b"\0")


# ---- afis_alignment_fit ------------------------------------------------------------------------------------------------------------------------------
def test_planted_quarter_turns_fit_exactly(lib):
    rng = np.random.default_rng(SEED + 1)
    n_cases = 0
    for n in (2, 3, 17, 200, 560):
        for turns in range(4):
            for span in (50, 3000):
                lx, ly = rng.integers(0, span, n), rng.integers(0, span, n)
                if len({(int(a), int(b)) for a, b in zip(lx, ly)}) < 2: lx[0] += 1      # two distinct points fix the rotation
                tx, ty = int(rng.integers(-4000, 4000)), int(rng.integers(-4000, 4000))
                rx, ry, c, s = PE.rotated(lx, ly, turns, tx, ty)
                rc, got = fit(lib, PE.moments(lx, ly, rx, ry))
                assert rc == 0 and got == (float(c), float(s), float(tx), float(ty), 0.0), (n, turns, span, got, (c, s, tx, ty))
                n_cases += 1
    assert n_cases == 40


def held_to_the_bounds(lib, m, where):
    rc, got = fit(lib, m)
    want, bound = PE.exact_fit(m), PE.bounds(m)
    assert rc == 0 and want is not None, where
    for name, g, w, b in zip(("c", "s", "tx", "ty", "rms"), got, want, bound):
        err = abs(Decimal(g) - w)
        assert err <= b, (where, name, g, float(w), float(err), float(b))
    return got, want


def test_random_point_sets_against_the_exact_fit(lib):
    """n from 2 to 560, coordinates over the whole int16 range and over a 50 x 50 patch; independent point sets (a large residual) and a planted rotation by an arbitrary
    angle with rounding and jitter (a small one: the cancelling regime of rms and t).  The bounds are pair_evidence_model.py's, counted from the operations."""
    rng = np.random.default_rng(SEED + 2)
    sizes = [2, 3, 4, 5, 7, 16, 63, 64, 119, 120, 200, 321, 559, 560] + [int(v) for v in rng.integers(2, 561, 26)]
    n_sets, small_residual = 0, 0
    for n in sizes:
        for whole in (True, False):
            for planted in (False, True):
                lx, ly, rx, ry = random_points(rng, n, whole)
                if planted:
                    a = rng.uniform(-np.pi, np.pi)
                    span = 8000 if whole else 12
                    lx, ly = rng.integers(-span, span, n), rng.integers(-span, span, n)
                    rx = np.rint(np.cos(a) * lx - np.sin(a) * ly + rng.integers(-2, 3, n)).astype(np.int64) + int(rng.integers(-span, span))
                    ry = np.rint(np.sin(a) * lx + np.cos(a) * ly + rng.integers(-2, 3, n)).astype(np.int64) + int(rng.integers(-span, span))
                m = PE.moments(lx, ly, rx, ry)
                if PE.exact_fit(m) is None: continue                        # (a degenerate draw: all points of one side coincide)
                got, want = held_to_the_bounds(lib, m, (n, whole, planted))
                n_sets += 1
                small_residual += planted and float(want[4]) < 3.0
                if planted and n >= 16:
                    assert abs(got[0] - np.cos(a)) < 0.2 and abs(got[1] - np.sin(a)) < 0.2, (n, whole, got, a)     # and it is the planted rotation
    assert n_sets >= 150 and small_residual >= 40, (n_sets, small_residual)
    # texture records at the pixel scale, the largest coordinates a record can hold
    for n in (2, 200, 560):
        b = [rng.integers(32000, 32768, n) for _ in range(4)]
        m = PE.moments(*(PE.texture_px(v) for v in b))
        if PE.exact_fit(m) is not None:
            held_to_the_bounds(lib, m, ("texture scale", n))


def test_fit_refusals_leave_the_outputs_untouched(lib):
    nan = lambda got: all(g != g for g in got)
    one = PE.moments([5], [6], [7], [8])
    rc, got = fit(lib, one)
    assert rc == EINVAL and nan(got)                                        # n < 2
    rc, got = fit(lib, (0,) * 9)
    assert rc == EINVAL and nan(got)
    same_l = PE.moments([3, 3, 3], [4, 4, 4], [1, 20, 300], [9, 8, 7])      # every latent point is one point: P = Q = 0
    assert PE.exact_terms(same_l)[:2] == (0, 0)
    rc, got = fit(lib, same_l)
    assert rc == EINVAL and nan(got)
    same_r = PE.moments([1, 20, 300], [9, 8, 7], [3, 3, 3], [4, 4, 4])
    rc, got = fit(lib, same_r)
    assert rc == EINVAL and nan(got)
    beyond = PE.moments([1, 2], [3, 5], [7, 11], [13, 19])
    rc, got = fit(lib, (561,) + beyond[1:])
    assert rc == EINVAL and nan(got)                                        # outside the bound
    assert lib.afis_alignment_fit(None, None, None, None, None, None) == EINVAL
    # every output may be NULL, alone and together
    r = rec(beyond)
    assert lib.afis_alignment_fit(C.c_void_p(r.ctypes.data), None, None, None, None, None) == 0
    full = fit(lib, beyond)[1]
    for k in range(5):
        out = C.c_double(float("nan"))
        args = [None] * 5
        args[k] = C.byref(out)
        assert lib.afis_alignment_fit(C.c_void_p(r.ctypes.data), *args) == 0 and out.value == full[k], k
    assert M.alignment_fit(lib, r) == full and M.alignment_fit(lib, rec(one)) is None


# ---- the sharding merges -----------------------------------------------------------------------------------------------------------------------------
def test_merge_texture_correspondences_takes_the_owning_rank():
    rng = np.random.default_rng(SEED + 3)
    P, R = 7, 3
    owner = np.array([0, 2, -1, 1, 1, 0, -1])
    ranks = []
    for r in range(R):
        cn = np.full(P, SH.CORR_NOT_COVERED, np.int32); xy = np.zeros((P, 200, 4), np.int16); pt = np.zeros((P, 200, 2), np.int16); sim = np.zeros((P, 200), np.float32); part = np.zeros(P, np.float32)
        for i in np.flatnonzero(owner == r):
            n = [200, 0, 5, -1][int(i) % 4]                                 # a full list, an empty one, a short one, a scorer that did not run
            cn[i] = n
            if n > 0:
                xy[i, :n] = rng.integers(0, 50, (n, 4)); pt[i, :n] = rng.integers(0, 300, (n, 2)); sim[i, :n] = rng.random(n).astype(np.float32); part[i] = sim[i, :n].sum()
        ranks.append({"counts": cn, "xy": xy, "pt": pt, "sim": sim, "part": part})
    got = SH.merge_texture_correspondences(ranks)
    assert got["owner"].tolist() == owner.tolist()
    for i in range(P):
        if owner[i] < 0:
            assert got["counts"][i] == SH.CORR_NOT_COVERED and not got["xy"][i].any() and not got["pt"][i].any() and not got["sim"][i].any() and got["part"][i] == 0
            continue
        src = ranks[owner[i]]
        for k in ("counts", "xy", "pt", "sim", "part"):
            assert got[k][i].tobytes() == src[k][i].tobytes(), (i, k)
    assert (got["counts"] == SH.CORR_NOT_RUN).any() and (got["counts"] == 200).any()
    without = SH.merge_texture_correspondences([{k: v for k, v in r.items() if k != "part"} | {"part": None} for r in ranks])
    assert without["part"] is None and without["counts"].tobytes() == got["counts"].tobytes()
    ranks[1]["counts"][0] = 3                                               # two ranks claim pair 0
    with pytest.raises(ValueError):
        SH.merge_texture_correspondences(ranks)


@pytest.mark.parametrize("K", [4, 2])
def test_merge_pair_alignments_takes_the_owning_rank(K):
    rng = np.random.default_rng(SEED + 4)
    P, R = 6, 3
    owner = np.array([1, -1, 0, 2, 2, 0])
    ranks = []
    for r in range(R):
        st = np.full(P, SH.PAIR_NOT_COVERED, np.int32); mo = np.zeros((P, K), M.CORR_MOMENTS)
        for i in np.flatnonzero(owner == r):
            st[i] = SH.PAIR_OK
            for k in range(K):
                if (i + k) % 3:                                             # (some scorers leave nothing: zero records of a covered pair)
                    mo[i, k] = PE.moments(*[rng.integers(0, 500, 9) for _ in range(4)])
        ranks.append({"status": st, "moments": mo})
    got = SH.merge_pair_alignments(ranks)
    assert got["owner"].tolist() == owner.tolist() and got["moments"].shape == (P, K)
    for i in range(P):
        if owner[i] < 0:
            assert got["status"][i] == SH.PAIR_NOT_COVERED and not got["moments"][i].tobytes().strip(b"\0")
        else:
            assert got["status"][i] == SH.PAIR_OK and got["moments"][i].tobytes() == ranks[owner[i]]["moments"][i].tobytes(), i
    ranks[0]["status"][0] = SH.PAIR_OK
    with pytest.raises(ValueError):
        SH.merge_pair_alignments(ranks)


# ---- the oracle alone: part = the fp32 sum of the list's similarities, in list order --------------------------------------------------------------------
def test_the_texture_part_is_the_sum_of_the_stage_2_similarities_in_list_order(codebook_bytes, oracle):
    cb = T.Codebook.from_bytes(codebook_bytes)
    sets = cases.list_length_set(cb)
    ocb = oracle.codebook(codebook_bytes)
    hl, hr = cases.to_orc(oracle, ocb, [c["L"] for c in sets], [c["R"] for c in sets])
    n = len(sets)
    lengths, positive = set(), 0
    for tie_mode in (1, 9):
        for q in range(n):
            for g in (q, (q + 1) % n, (q + 34) % n):                        # the mate, and two lists of other lengths
                sim, li, ri = oracle.trace(ocb, hl[q], hr[g], which=0, stage=2, tie_mode=tie_mode)
                rc, part = oracle.pair(ocb, hl[q], hr[g], tie_mode)
                assert rc == 0 and part[3].view(np.uint32) == PE.sum_in_order(sim).view(np.uint32), (tie_mode, q, g, part[3], len(sim))
                assert len(li) <= 200 and (len(li) == 0 or (li.max() < sets[q]["L"].tex[0].n and ri.max() < sets[g]["R"].tex[0].n))
                lengths.add(len(li)); positive += part[3] > 0
    assert {1, 0} & lengths and max(lengths) == 200 and len(lengths) >= 60 and positive >= 0.9 * 2 * n, (sorted(lengths), positive)
