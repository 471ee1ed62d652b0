"""Print pairs without a GPU: afis_score_print_pairs and afis_correspondences_print_pairs are declared, exported by both libraries, bound by the Python host and absent
from the taps; the header carries the contract; the three options are documented; the numpy model of the plan (tests/print_pairs_model.py) on hand-made cases;
host/sharding.py's merges for the new shapes on hand-made per-rank answers; and print_pairs_plan.h — the distinct query prints, the batches, every pair's batch and
handle position — through the stand-alone program csrc/print_pairs_plan_check, built with the host sanitizers and run as a program (nothing is loaded into this
process).  What the device answers is tests/test_gpu_print_pairs.py's."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import print_pairs_model as PM

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NAMES = ("afis_score_print_pairs", "afis_correspondences_print_pairs")
OPTIONS = ("print_pairs_batch_prints", "print_pairs_us", "print_pairs_query_prints")


def _header():
    return open(os.path.join(ROOT, "include", "afis_matcher.h")).read()


def test_the_entry_points_are_declared_exported_and_bound():
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+afis_score_print_pairs\s*\(afis_ctx\*\s*ctx,\s*int64_t\s+n_pairs,\s*const int64_t\*\s*a_idx\s*,\s*const int64_t\*\s*b_idx\s*,"
                     r"\s*const float\*\s*w_minu\s*,\s*const float\*\s*w_tex\s*,\s*int32_t\*\s*status\s*,\s*float\*\s*score\s*,\s*float\*\s*parts\s*\)\s*;", code)
    assert re.search(r"\bint\s+afis_correspondences_print_pairs\s*\(afis_ctx\*\s*ctx,\s*int64_t\s+n_pairs,\s*const int64_t\*\s*a_idx\s*,\s*const int64_t\*\s*b_idx\s*,"
                     r"\s*int32_t\*\s*counts\s*,\s*int16_t\*\s*xy\s*,\s*float\*\s*part\s*\)\s*;", code)
    assert hdr.index("int afis_score_pairs(") < hdr.index("int afis_score_print_pairs(") < hdr.index("int afis_correspondences_print_pairs(") < hdr.index("int afis_search_cascade(")
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        for name, n_args in zip(NAMES, (9, 7)):
            assert name in M.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args
    assert not any(n in M.TAP_EXPORTS for n in NAMES)
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    assert "print_pairs" not in taps
    assert hasattr(M.Matcher, "score_print_pairs") and hasattr(M.Matcher, "correspondences_print_pairs")
    assert hasattr(SH, "merge_print_pair_scores") and hasattr(SH, "merge_print_correspondences")
    alone = hdr[hdr.index("leave the matrix alone") - 400:hdr.index("leave the matrix alone")]
    assert all(n in alone for n in NAMES)                                   # on the list of calls after which the ranking calls still answer


def test_the_header_carries_the_contract():
    hdr = _header()
    para = hdr[hdr.index("/* Print pairs"):hdr.index("int afis_score_print_pairs(")]
    flat = re.sub(r"\s*\n \*\s*", " ", para)
    for phrase in ("never a subset's position", "may come in any order and may repeat", "(a, a) is an ordinary pair", "BOTH indices lie in [index_base, index_base + G)",
                   "AFIS_PAIR_NOT_COVERED", "AFIS_CORR_NOT_COVERED", "AFIS_CORR_NOT_RUN", "differs on purpose from afis_search_prints", "every rank of a sharded gallery",
                   "answered by NO rank", "afis_search_weighted route over host views", "bit for bit the cell afis_search_prints writes", "w_minu[i] != 0.0f",
                   "-1.0f when b is empty or removed, or when nothing of a is active", "double acc = +0.0", "that zero is included", "-0.0f is a zero",
                   "27 minutiae templates whose 27th is a's minutiae template", "neither written nor invalidated", "AFIS_ESTATE: a call before the first commit",
                   "n_pairs == 0 is AFIS_OK", "\"search_timeout_s\"", "No handle is involved", "\"s3_tie_order\" / \"ref_tie_order\"", "\"adc_variant\" 8 and 9",
                   "k_fold_print_pairs", "csrc/print_pairs_plan.h"):
        assert phrase in flat, phrase
    prints = hdr[hdr.index("/* Print search"):hdr.index("int afis_search_prints(")]
    assert "afis_score_pairs and afis_correspondences_pairs take latents" not in prints and "afis_score_print_pairs" in prints


def test_the_options_are_documented():
    hdr = _header()
    block = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    assert '"print_pairs_batch_prints" (settable, >= 0; default 0)' in block
    assert re.search(r'"print_pairs_us" \(read-only\)', block) and re.search(r'"print_pairs_query_prints" \(read-only\)', block)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in OPTIONS + NAMES:
        assert "`%s`" % name in doc, name
    api = open(os.path.join(CSRC, "afis_api.cpp")).read()
    for name in OPTIONS:
        assert api.count('n == "%s"' % name) == (2 if name == "print_pairs_batch_prints" else 1), name      # one settable, two read-only
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert all("`%s`" % n in readme and "`%s`" % n in design for n in NAMES)


def test_the_units_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "afis_print_pairs.o" in objs and "template_fold.o" in objs
    assert re.search(r"^afis_print_pairs\.o:.*print_pairs_plan\.h", mk, flags=re.M)
    assert "print_pairs_plan_check" in re.search(r"^all:(.*)$", mk, flags=re.M).group(1).split()
    assert "print_pairs_plan_check" in mk[mk.index("\nclean:"):]
    fold = open(os.path.join(CSRC, "template_fold.hip")).read()
    k = fold[fold.index("void k_fold_print_pairs("):fold.index("hipError_t launch_fold_print_pairs")]
    assert "__shared__" not in k and "atomic" not in k and "size_t" in k and "gridDim.x" in k      # no LDS, no atomics, size_t indices, a stride loop


# ---- the model of the plan ------------------------------------------------------------------------------------------------------------------------------
COUNTS = [(5, 10), (0, 20), (30, 0), (0, 0), (16, 1000), (17, 3)]
BASE = 100


def test_the_model_on_hand_made_cases():
    none = PM.plan([], [], BASE, COUNTS, True, True)
    assert none == {"prints": [], "batches": [], "pairs": [], "planned": []}
    out = PM.plan([-1, 99, 106, 100, 100], [100, 100, 100, 106, -1], BASE, COUNTS, True, True)              # every pair uncovered
    assert out["planned"] == [] and out["batches"] == []
    assert PM.covered([100, 105, 106, 99], [105, 100, 100, 100], BASE, 6).tolist() == [True, True, False, False]
    # first appearance orders the prints; a print gathers what SOME pair of it wants and it holds; a pair with nothing active is not planned
    a = [104, 100, 104, 101, 103, 102, 100, 102]
    b = [100, 101, 102, 103, 104, 105, 100, 100]
    wm = [True, False, False, True, True, True, True, False]
    wt = [False, False, True, True, True, True, False, True]
    out = PM.plan(a, b, BASE, COUNTS, wm, wt, cap=2)
    assert out["planned"] == [0, 2, 3, 5, 6]                                # pair 1: both weights zero; 4: print 3 is empty; 7: print 2 has no texture
    assert out["prints"] == [(4, True, True), (1, False, True), (2, True, False), (0, True, False)]
    assert out["batches"] == [[0, 1], [2, 3]]
    assert out["pairs"] == [[(0, 0), (2, 0), (3, 1)], [(5, 0), (6, 1)]]
    one = PM.plan(a, b, BASE, COUNTS, wm, wt, cap=1)
    assert one["batches"] == [[0], [1], [2], [3]] and one["pairs"] == [[(0, 0), (2, 0)], [(3, 0)], [(5, 0)], [(6, 0)]]
    # automatic: consecutive prints while the views fit; a print larger than the budget is a batch of its own
    big = PM.view_bytes(16, 1000)
    assert big == 1016 * 392 + 6144 and PM.view_bytes(17, 0) == 17 * 392 + 2 * 6144 and PM.view_bytes(0, 0) == 0
    auto = PM.plan(a, b, BASE, COUNTS, wm, wt, cap=0, budget=big - 1)
    assert auto["batches"] == [[0], [1, 2, 3]]
    tight = PM.plan(a, b, BASE, COUNTS, wm, wt, cap=0, budget=PM.view_bytes(0, 20) + PM.view_bytes(30, 0))
    assert tight["batches"] == [[0], [1, 2], [3]]
    wide = PM.plan(a, b, BASE, COUNTS, wm, wt, cap=0)
    assert wide["batches"] == [[0, 1, 2, 3]] and wide["pairs"] == [[(0, 0), (2, 0), (3, 1), (5, 2), (6, 3)]]
    # the correspondence call: minutiae only
    corr = PM.plan(a, b, BASE, COUNTS, True, False)
    assert corr["prints"] == [(4, True, False), (0, True, False), (2, True, False)] and corr["planned"] == [0, 1, 2, 5, 6, 7]


# ---- the merges -------------------------------------------------------------------------------------------------------------------------------------------
def _score_answer(rng, covered, n_pairs, parts=True):
    st = np.full(n_pairs, SH.PAIR_NOT_COVERED, np.int32); sc = np.full(n_pairs, -np.inf, np.float32); pt = np.zeros((n_pairs, 2), np.float32)
    for p in covered:
        st[p] = SH.PAIR_OK
        sc[p] = -1.0 if rng.random() < 0.3 else rng.random() * 100
        pt[p] = rng.random(2)
    return {"status": st, "score": sc, "parts": pt if parts else None}


def _corr_answer(rng, covered, n_pairs):
    cn = np.full(n_pairs, SH.CORR_NOT_COVERED, np.int32); xy = np.zeros((n_pairs, 120, 4), np.int16); pt = np.zeros(n_pairs, np.float32)
    for p in covered:
        cn[p] = int(rng.integers(-1, 121))
        if cn[p] > 0:
            xy[p, :cn[p]] = rng.integers(0, 500, (cn[p], 4)); pt[p] = rng.random()
    return cn, xy, pt


def test_the_score_merge():
    rng = np.random.default_rng(51)
    owners = [0, 2, 1, -1, 0, 2, -1, 0, 1]                                  # -1: the pair's prints lie in two shards, or in none: no rank answers it
    P = len(owners)
    ranks = [_score_answer(rng, [p for p in range(P) if owners[p] == r], P) for r in range(3)]
    out = SH.merge_print_pair_scores(ranks)
    assert out["owner"].tolist() == owners and out["parts"].shape == (P, 2)
    for p in range(P):
        if owners[p] < 0:
            assert out["status"][p] == SH.PAIR_NOT_COVERED and np.isneginf(out["score"][p]) and (out["parts"][p].view(np.uint32) == 0).all()
            continue
        src = ranks[owners[p]]
        assert out["status"][p] == SH.PAIR_OK and out["score"][p].tobytes() == src["score"][p].tobytes() and out["parts"][p].tobytes() == src["parts"][p].tobytes()
    for r in ranks:
        r["parts"] = None
    out2 = SH.merge_print_pair_scores(ranks)
    assert out2["parts"] is None and out2["score"].tobytes() == out["score"].tobytes() and out2["owner"].tolist() == owners
    with pytest.raises(ValueError, match=r"covered by two ranks"):
        SH.merge_print_pair_scores([_score_answer(rng, [0, 1], 3), _score_answer(rng, [1, 2], 3)])
    with pytest.raises(ValueError):
        SH.merge_print_pair_scores([_score_answer(rng, [0], 3), _score_answer(rng, [1], 4)])


def test_the_correspondence_merge():
    rng = np.random.default_rng(52)
    owners = [1, 0, -1, 2, 2, 0, -1]
    P = len(owners)
    ans = [_corr_answer(rng, [p for p in range(P) if owners[p] == r], P) for r in range(3)]
    cn, xy, pt = (np.stack([a[k] for a in ans]) for k in range(3))
    oc, oxy, opt, owner = SH.merge_print_correspondences(cn, xy, pt)
    assert owner.tolist() == owners and oc.shape == (P,) and oxy.shape == (P, 120, 4) and opt.shape == (P,)
    for p in range(P):
        if owners[p] < 0:
            assert oc[p] == SH.CORR_NOT_COVERED and not oxy[p].any() and opt[p].view(np.uint32) == 0
            continue
        r = owners[p]
        assert oc[p] == cn[r, p] and oxy[p].tobytes() == xy[r, p].tobytes() and opt[p].tobytes() == pt[r, p].tobytes()
    oc2, oxy2, owner2 = SH.merge_print_correspondences(cn, xy)
    assert oc2.tobytes() == oc.tobytes() and oxy2.tobytes() == oxy.tobytes() and owner2.tolist() == owners
    two = np.stack([_corr_answer(rng, [0, 1], 3)[0], _corr_answer(rng, [1, 2], 3)[0]])
    with pytest.raises(ValueError, match=r"covered by two ranks"):
        SH.merge_print_correspondences(two, np.zeros((2, 3, 120, 4), np.int16))
    with pytest.raises(ValueError):
        SH.merge_print_correspondences(np.zeros((2, 3, 3), np.int32), np.zeros((2, 3, 3, 120, 4), np.int16))          # the latent call's shapes are merge_correspondences'


# ---- print_pairs_plan.h -----------------------------------------------------------------------------------------------------------------------------------
def test_print_pairs_plan_check_runs_clean_under_the_host_sanitizers():
    exe = os.path.join(CSRC, "print_pairs_plan_check")
    src = [os.path.join(CSRC, f) for f in ("print_pairs_plan_check.cpp", "print_pairs_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in src):
        subprocess.run(["make", "-s", "-C", CSRC, "print_pairs_plan_check"], check=True)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("\nprint_pairs_plan_check:"):]
    assert "-fsanitize=address,undefined" in rule[:rule.index("\n\n")] and "-fno-sanitize-recover=undefined" in rule[:rule.index("\n\n")]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"print_pairs_plan_check: \d+ cases ok", out.stdout), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert int(re.search(r"(\d+) cases ok", out.stdout).group(1)) >= 500
    hdr = open(os.path.join(CSRC, "print_pairs_plan.h")).read()
    assert not re.search(r'#include\s*[<"](hip|afis_)', hdr)                  # device-free: no runtime header, none of the project's device headers
    for case in ("no pairs", "all uncovered", "one print in every pair", "every pair a distinct print", "a print larger than the budget", "repeats", "random"):
        assert '"%s' % case in open(src[0]).read(), case
