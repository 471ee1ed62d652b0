"""Print cascade without a GPU: afis_search_prints_cascade is declared after afis_search_cascade, exported by both libraries, bound by the Python host and absent from the
taps; the new kernels and the driver are product objects, the kernels use no atomics and share one fold expression; the options are documented and the header carries
the contract; the numpy model (tests/print_cascade_model.py) is held against hand-made matrices.  What the device computes is tests/test_gpu_print_cascade.py's."""
import importlib
import os
import re

import numpy as np

import cascade_model as CM
import print_cascade_model as PM

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NAME = "afis_search_prints_cascade"
READ_ONLY = ("print_cascade_stage1_us", "print_cascade_select_us", "print_cascade_stage2_us", "print_cascade_kept_pairs")
F = np.float32


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(afis_ctx\*\s*ctx,\s*const int64_t\*\s*idx\s*,\s*int n_q,\s*const float\*\s*w_minu\s*,\s*const float\*\s*w_tex\s*,\s*int keep,\s*"
                     r"float\*\s*scores\s*,\s*int32_t\*\s*status\s*,\s*int64_t\*\s*n_kept\s*,\s*int64_t\*\s*kept_idx\s*,\s*float\*\s*kept_parts\s*\)\s*;" % NAME, code)
    assert hdr.index("int afis_search_cascade(") < hdr.index("int %s(" % NAME) < hdr.index("int afis_get_timing(")
    declared = set(re.findall(r"\b(afis_[a-z0-9_]+)\s*\(", hdr))            # comments count: every name spelled with a parenthesis is an exported function
    assert declared == set(M.EXPORTS) and NAME in declared
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    assert NAME not in taps and NAME not in M.TAP_EXPORTS
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        assert hasattr(lib, NAME) and len(getattr(lib, NAME).argtypes) == 11
    assert hasattr(M.Matcher, "search_prints_cascade")
    assert NAME in hdr[hdr.index("afis_rank_subjects   ranks the score matrix"):hdr.index("n_q must be that")]     # the list of searches that count


def test_the_kernels_and_the_driver_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "print_cascade.o" in objs and "afis_print_cascade.o" in objs
    assert re.search(r"^print_cascade\.o:\s*print_cascade\.hip.*print_fold\.h", mk, flags=re.M)
    assert re.search(r"^afis_print_cascade\.o:\s*afis_print_cascade\.cpp.*cascade_tables\.h", mk, flags=re.M)
    src = open(os.path.join(CSRC, "print_cascade.hip")).read()
    body = src.split("namespace afis {", 1)[1]                                # the code, without the header comment
    assert "atomic" not in body and "__shared__" not in body
    assert '#include "print_fold.h"' in src
    for k in ("k_print_cascade_stage1", "k_print_cascade_finish"):            # one fold expression, used by both kernels that make a cell
        kernel = body[body.index("void %s(" % k):]
        assert "fold_print_cell(" in kernel[:kernel.index("\n}\n")], k
    defs = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".cpp")) and re.search(r"float\s+fold_print_cell\s*\(", open(os.path.join(CSRC, f)).read())]
    assert defs == ["print_fold.h"]
    drv = open(os.path.join(CSRC, "afis_print_cascade.cpp")).read().split("#include", 1)[1]
    for call in ("build_print_queries(", "launch_print_cascade_stage1(", "launch_print_cascade_gather(", "launch_print_cascade_finish(", "CascadeCall", ".run("):
        assert call in drv, call                                            # the call's own: its handle and its three kernels; the rest is the cascade driver's
    run = open(os.path.join(CSRC, "afis_cascade.cpp")).read()
    run = run[run.index("int CascadeCall::run("):]
    run = run[:run.index("\n}\n")]
    for call in ("queue_minutiae_stage(", "fuse_all()", "launch_rank_hits(", "build_cascade_tables(", "gather()", "queue_texture_pairs(", "finish()"):
        assert call in run, call
    tex = open(os.path.join(CSRC, "afis_pairs.cpp")).read()
    tex = tex[tex.index("int queue_texture_pairs("):]                        # the texture stage of a pair table that run() queues per piece: the pair kernels
    tex = tex[:tex.index("\n}\n")]
    assert "launch_adc_pairs(" in tex and "launch_graph_texture_pairs(" in tex and "launch_graph_texture(" not in tex
    assert "stream_lo" not in drv and "stream_hi" not in drv and "launch_graph_texture(" not in drv and "search_shard(" not in drv
    assert "stream_lo" not in run and "stream_hi" not in run and "launch_graph_texture(" not in run and "search_shard(" not in run
    assert drv.count("wait_streams(") == 0 and run.count("wait_streams(") == 1     # after the handle's own wait: one launch sequence, one wait
    assert "launch_adc_pairs(" not in drv and "launch_minu_cands(" not in drv and "queue_minutiae_stage(" not in drv   # no launch loop of its own


def test_the_options_and_the_contract_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    block = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in READ_ONLY:
        assert re.search(r'"%s" \(read-only\)' % opt, block), opt
        assert "`%s`" % opt in integration, opt
    assert "`%s`" % NAME in integration
    api = open(os.path.join(CSRC, "afis_api.cpp")).read()
    for opt in READ_ONLY:
        assert 'n == "%s"' % opt in api, opt
    contract = re.sub(r"\s*\n \*\s+", " ", hdr[hdr.index("Print cascade (no reference counterpart"):hdr.index("int %s(" % NAME)])
    for phrase in ("1 <= keep <= AFIS_HITS_MAX", "n_kept[q] = min(keep, G)", "(w_minu[q], +0.0f)", "-1.0f for the WHOLE ROW", "(float)(+0.0 + (double)w_minu[q] * (double)v_m)",
                   "There is no special case", "belongs to afis_search_prints", "ascending GLOBAL index", "the -1 cells stand last", "padded with -1", "bit for bit",
                   "0xffffffff", "kNoEntryWord", "afis_score_print_pairs defines", "+0.0f twice", "one of the searches that count", "AFIS_POS_NO_ENTRY", "_filtered forms",
                   "afis_rank_subjects is not in this interface", "A print against itself is an ordinary kept cell", "exclusion list", "holds nothing it allocated",
                   "returns the bytes it returned before", "staged but not committed", "search_timeout_s", "is ensured before anything of the cascade is queued",
                   "[n_pseudo][G][4]", "cascade_pairs_per_launch", "print_gather_us", "print_h2d_bytes", "the texture fields are 0", "csrc/print_fold.h",
                   "profiles/print_cascade_timing.json", "profiles/print_cascade_full_search_ab.txt", "no handle is involved", "valid after any gallery edit") + READ_ONLY:
        assert phrase in contract, phrase
    left_out = contract[contract.index("Not in this interface"):]
    for phrase in ("a subset form", "a keep above AFIS_HITS_MAX", "batching over queries", "the match CLI"):
        assert phrase in left_out, phrase
    shards = contract[contract.index("Shards:"):contract.index("Not in this interface")]
    for phrase in ("only on the rank that holds it", "every rank keeps `keep` of its OWN shard", "superset"):
        assert phrase in shards, phrase
    assert "search_prints_cascade" in (SH.__doc__ or "")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "print_cascade.hip" in readme and "afis_print_cascade.cpp" in readme
    assert NAME in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- the model against hand-made matrices ---------------------------------------------------------------------------------------------------------------------
BASE = 1000


def hand():
    """Five query prints x eight columns.  Columns 0 and 7 are empty.  Row 0: both terms; columns 2 and 5 have minutiae evidence, 1, 3, 4, 6 tie at zero, texture
    alone (columns 1, 6) does not move a column in stage 1.  Row 1: no minutiae template — stage-1 blind, texture active.  Row 2: w_tex == 0 — minutiae only.
    Row 3: nothing active (both weights zero).  Row 4: w_minu == 0 with both templates — stage-1 blind."""
    v_m = np.zeros((5, 8), F); v_t = np.zeros((5, 8), F)
    v_m[0, 2] = 4; v_m[0, 5] = 9; v_t[0, 2] = 50; v_t[0, 1] = 70; v_t[0, 6] = 90
    v_m[1] = 3; v_t[1] = np.arange(8) * 2
    v_m[2] = (0, 5, 0, 5, 0, 0, 1, 0); v_t[2] = 40
    v_m[3] = 7; v_t[3] = 7
    v_m[4] = np.arange(8)[::-1]; v_t[4] = np.arange(8)
    has_minu = [1, 0, 1, 1, 1]; has_tex = [1, 1, 1, 1, 1]
    w_minu = np.array([1, 1, 2, 0, 0], F); w_tex = np.array([0.3, 0.3, 0, -0.0, 0.5], F)
    return PM.four_matrices(v_m, v_t, has_minu, has_tex, w_minu, w_tex, empty_cols=(0, 7)), has_minu, has_tex, w_minu, w_tex


def test_the_model_cuts_a_tie_by_global_index_and_keeps_minus_ones_last():
    (final, m, v_m, v_t), hm, ht, wm, wt = hand()
    assert m[0].tolist() == [-1, 0, 4, 0, 0, 9, 0, -1] and (m[1] == -1).all() and (m[3] == -1).all() and (m[4] == -1).all()
    for keep, kept0 in ((1, [5]), (2, [5, 2]), (3, [5, 2, 1]), (4, [5, 2, 1, 3]), (5, [5, 2, 1, 3, 4]), (6, [5, 2, 1, 3, 4, 6]), (7, [5, 2, 1, 3, 4, 6, 0]),
                        (8, [5, 2, 1, 3, 4, 6, 0, 7]), (11, [5, 2, 1, 3, 4, 6, 0, 7])):
        e = PM.expected(final, m, v_m, v_t, hm, ht, wm, wt, keep, BASE)
        n = min(keep, 8)
        assert e["n_kept"].tolist() == [n] * 5 and e["status"].tolist() == [0, 0, 0, 1, 0]
        assert e["kept_idx"][0].tolist() == [BASE + t for t in kept0] + [-1] * (keep - n), keep       # the cut inside the tie 1, 3, 4, 6: ascending global index; the -1 cells last
        for blind in (1, 3, 4):                                             # a row stage 1 cannot rank keeps columns 0 .. n - 1
            assert e["kept_idx"][blind].tolist() == [BASE + t for t in range(n)] + [-1] * (keep - n), (keep, blind)
        mat = e["matrix"]
        assert (mat != CM.NO_ENTRY).sum(axis=1).tolist() == [n] * 5
        assert np.array_equal(mat[0, kept0], final.view(np.uint32)[0, kept0])
        assert (mat[3, :n] == CM.MINUS_ONE).all()
        assert not e["kept_parts"][:, n:].any() and not e["kept_parts"][3].any()
    # the final score re-sorts the kept cells: column 6 (texture 90) overtakes column 5 once it is kept
    e = PM.expected(final, m, v_m, v_t, hm, ht, wm, wt, 6, BASE)
    _, idx, _ = CM.rank_rows(e["matrix"].view(F), 6, BASE)
    assert idx[0].tolist() == [BASE + 6, BASE + 1, BASE + 2, BASE + 5, BASE + 3, BASE + 4]


def test_the_model_values_and_the_activity_rule():
    (final, m, v_m, v_t), hm, ht, wm, wt = hand()
    e = PM.expected(final, m, v_m, v_t, hm, ht, wm, wt, 8, BASE)
    mat, kp = e["matrix"].view(F), e["kept_parts"].view(F)
    assert np.array_equal(e["matrix"], final.view(np.uint32))               # keep == G: every cell is kept
    # a minutiae-only row's kept cells equal m, and its texture part is +0.0f whatever the texture scorer would give
    assert np.array_equal(e["matrix"][2], m.view(np.uint32)[2])
    pos2 = e["kept_pos"][2]
    assert pos2.tolist() == [1, 3, 6, 2, 4, 5, 0, 7]
    assert kp[2, :, 0].tolist() == [5, 5, 1, 0, 0, 0, 0, 0] and not e["kept_parts"][2, :, 1].any()
    assert mat[2, 1] == 10.0 and mat[2, 6] == 2.0
    # both terms: (float)(1 x v_m + 0.3f x v_t) in fp64, minutiae first
    assert mat[0, 2] == F(np.float64(4) + np.float64(F(0.3)) * 50) and mat[0, 6] == F(np.float64(F(0.3)) * 90)
    pos0 = e["kept_pos"][0].tolist()
    assert kp[0, pos0.index(2)].tolist() == [4, 50] and kp[0, pos0.index(6)].tolist() == [0, 90] and kp[0, pos0.index(0)].tolist() == [0, 0]       # the -1 cell: +0.0f twice
    # texture only (no minutiae template; w_minu == 0): the minutiae part is +0.0f though v_m is not
    for q, w in ((1, F(0.3)), (4, F(0.5))):
        assert not e["kept_parts"][q, :, 0].any()
        assert kp[q, 1:7, 1].tolist() == v_t[q, 1:7].tolist() and mat[q, 3] == F(np.float64(w) * np.float64(v_t[q, 3]))
    assert (e["matrix"][:, [0, 7]] == CM.MINUS_ONE).all() and (e["matrix"][3] == CM.MINUS_ONE).all()
    # kept cells outside the kept set are no entries; dtype and shapes
    e3 = PM.expected(final, m, v_m, v_t, hm, ht, wm, wt, 3, BASE)
    assert e3["matrix"].dtype == np.uint32 and e3["kept_parts"].shape == (5, 3, 2) and (e3["matrix"][0, [0, 3, 4, 6, 7]] == CM.NO_ENTRY).all()
