"""Cascade search without a GPU: afis_search_cascade is declared, exported by both libraries, bound by the Python host and absent from the taps; the new kernel and
driver are product objects and the fusion expression has one definition; the options are documented and the header carries the contract; the numpy model
(tests/cascade_model.py) is held against hand-made matrices; and cascade_tables.h — the host's structure of the second stage — goes through the stand-alone program
csrc/cascade_tables_check, built with the host sanitizers and run as a program (nothing is loaded into this process).  What the device computes is
tests/test_gpu_cascade_search.py's."""
import importlib
import os
import re
import subprocess

import numpy as np

import cascade_model as CM

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NAME = "afis_search_cascade"
READ_ONLY = ("cascade_stage1_us", "cascade_select_us", "cascade_stage2_us", "cascade_kept_pairs")
F = np.float32


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(afis_ctx\*\s*ctx,\s*afis_queries\*\s*q,\s*int keep,\s*float\*\s*scores\s*,\s*int32_t\*\s*status\s*,\s*int64_t\*\s*n_kept\s*,"
                     r"\s*int64_t\*\s*kept_idx\s*,\s*float\*\s*kept_parts\s*\)\s*;" % NAME, code)
    declared = set(re.findall(r"\b(afis_[a-z0-9_]+)\s*\(", hdr))            # comments count: every name spelled with a parenthesis is an exported function
    assert declared == set(M.EXPORTS) and NAME in declared
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    assert "cascade" not in taps and not any("cascade" in t for t in M.TAP_EXPORTS)
    default = int(re.search(r"^#define\s+AFIS_CASCADE_PAIRS_PER_LAUNCH\s+(\d+)\s*$", code, flags=re.M).group(1))
    dev = open(os.path.join(CSRC, "afis_device.h")).read()
    assert default == 16384 == int(re.search(r"constexpr int kCascadePairsPerLaunch = (\d+);", dev).group(1))
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        assert hasattr(lib, NAME) and len(getattr(lib, NAME).argtypes) == 8
    assert hasattr(M.Matcher, "search_cascade")
    assert NAME in hdr[hdr.index("afis_rank_subjects   ranks the score matrix"):hdr.index("n_q must be that")]     # the list of searches that count


def test_the_kernel_and_the_driver_are_product_objects_and_the_fusion_has_one_definition():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "cascade.o" in objs and "afis_cascade.o" in objs
    assert re.search(r"^cascade\.o:\s*cascade\.hip.*fuse_cell\.h", mk, flags=re.M) and re.search(r"^minu\.o:.*fuse_cell\.h", mk, flags=re.M)
    assert re.search(r"^afis_cascade\.o:\s*afis_cascade\.cpp.*cascade_tables\.h", mk, flags=re.M)
    defs = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".cpp")) and re.search(r"float\s+fuse_cell\s*\(", open(os.path.join(CSRC, f)).read())]
    assert defs == ["fuse_cell.h"]                                          # one definition of the expression ...
    for unit, kernels in (("minu.hip", ("k_fuse", "k_fuse_pairs")), ("cascade.hip", ("k_fuse_stage1",))):
        src = open(os.path.join(CSRC, unit)).read()
        assert '#include "fuse_cell.h"' in src
        for k in kernels:                                                   # ... that every fusing kernel calls
            body = src[src.index("void %s(" % k):]
            assert "fuse_cell(" in body[:body.index("\n}\n")], k
    body = open(os.path.join(CSRC, "cascade.hip")).read().split("namespace afis {", 1)[1]
    assert body.count("__global__") == 3 and "atomic" not in body and "__shared__" not in body
    drv = open(os.path.join(CSRC, "afis_cascade.cpp")).read().split("#include", 1)[1]
    for call in ("queue_minutiae_stage(", "launch_fuse_stage1(", "launch_rank_hits(", "launch_cascade_gather(", "queue_texture_pairs(",
                 "launch_cascade_scatter(", "build_cascade_tables("):
        assert call in drv, call
    pairs = open(os.path.join(CSRC, "afis_pairs.cpp")).read()
    tex = pairs[pairs.index("int queue_texture_pairs("):]                    # the texture stage of a pair table, as the pair calls queue it: the three kernels, called nowhere else in the product
    tex = tex[:tex.index("\n}\n")]
    for call in ("launch_adc_pairs(", "launch_graph_texture_pairs(", "launch_fuse_pairs("):
        assert call in tex, call
        n_calls = {f: len(re.findall(r"\b" + re.escape(call), open(os.path.join(CSRC, f)).read())) for f in os.listdir(CSRC) if f.endswith(".cpp") and f.startswith("afis_")}
        assert {f: n for f, n in n_calls.items() if n} == {"afis_pairs.cpp": 1}, call
    assert "stream_lo" not in drv and "stream_hi" not in drv and "launch_graph_texture(" not in drv and drv.count("wait_streams(") == 1      # unconfined; one wait
    search = open(os.path.join(CSRC, "afis_search.cpp")).read()
    assert "cascade" not in search                                          # the measured launch sequence got no flag
    stage = search[search.index("int queue_minutiae_stage("):]               # the minutiae stage every driver queues: the two kernels, called nowhere else in the product
    stage = stage[:stage.index("\n}\n")]
    assert "launch_minu_cands(" in stage and "launch_graph_minutiae(" in stage
    product = [f for f in sorted(os.listdir(CSRC)) if f.endswith(".cpp") and f.startswith("afis_") and f != "afis_taps.cpp"]
    calls = {f: len(re.findall(r"\blaunch_minu_cands\(", open(os.path.join(CSRC, f)).read())) for f in product}
    assert {f: n for f, n in calls.items() if n} == {"afis_search.cpp": 1}
    tabs = open(os.path.join(CSRC, "cascade_tables.h")).read()
    assert not re.search(r'#include\s*[<"](hip|afis_)', tabs)                 # device-free


def test_the_options_and_the_contract_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    block = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r'"cascade_pairs_per_launch" \(settable, 1 \.\. 1 048 576; default AFIS_CASCADE_PAIRS_PER_LAUNCH\)', block)
    for opt in READ_ONLY:
        assert re.search(r'"%s" \(read-only\)' % opt, block), opt
    for opt in READ_ONLY + ("cascade_pairs_per_launch", NAME):
        assert "`%s`" % opt in integration, opt
    contract = re.sub(r"\s*\n \*\s+", " ", hdr[hdr.index("Cascade search (no reference counterpart"):hdr.index("int %s(" % NAME)])      # the comment's line breaks are not the contract's
    for phrase in ("1 <= keep <= AFIS_HITS_MAX", "n_kept[q] = min(keep, G)", "texture score taken as +0.0f", "csrc/fuse_cell.h", "(a0 + a1) + a2",
                   "ascending GLOBAL index", "kept only when keep exceeds", "padded with -1", "bit for bit", "0xffffffff", "kNoEntryWord", "one of the searches that count",
                   "AFIS_POS_NO_ENTRY", "_filtered forms", "afis_rank_subjects is not in this interface", "holds nothing it allocated",
                   "returns the bytes it returned before the cascade call", "afis_queries_upload_reserved", "search_timeout_s", "ensured before anything is queued",
                   "cascade_pairs_per_launch", "cascade_stage1_us", "cascade_select_us", "cascade_stage2_us", "cascade_kept_pairs", "the texture fields are 0",
                   "profiles/cascade_search_timing.json"):
        assert phrase in contract, phrase
    left_out = contract[contract.index("Not in this interface"):]
    for phrase in ("a subset form", "a host-view form", "a keep above AFIS_HITS_MAX", "a first stage other than the minutiae scorers", "the match CLI"):
        assert phrase in left_out, phrase
    shards = contract[contract.index("Shards:"):contract.index("Not in this interface")]
    for phrase in ("every rank keeps `keep` of its OWN shard", "merge_hits / merge_subject_hits input as they are", "superset of the single-context cascade"):
        assert phrase in shards, phrase
    doc = SH.__doc__ or ""
    for phrase in ("search_cascade", "keeps `keep` of its own shard", "superset"):
        assert phrase in doc, phrase
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "cascade.hip" in readme and "afis_cascade.cpp" in readme
    assert NAME in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- the model against hand-made matrices ---------------------------------------------------------------------------------------------------------------------
def hand_search(parts, n_minu, n_tex, empty_cols=(), empty_rows=()):
    """A search's scores for hand-made parts [n_q][G][4]: fuse_cell's expression, written out per cell (the -1 cells' parts are +0.0f)."""
    parts = np.array(parts, F)
    n_q, G, _ = parts.shape
    scores = np.zeros((n_q, G), F)
    for q in range(n_q):
        slot = n_minu[q] if n_tex[q] > 0 else -1
        for g in range(G):
            if q in empty_rows or g in empty_cols:
                scores[q, g] = -1.0; parts[q, g] = 0.0
                continue
            p = parts[q, g]
            a = [p[3] if slot == s else p[s] for s in range(3)]
            f = F(F(a[0] + a[1]) + a[2])
            scores[q, g] = F(np.float64(f) + (np.float64(p[3]) if slot == 28 else 0.0) * 0.3)
    return scores, parts


def test_the_model_texture_slots():
    # one print; slots 0, 1, 2, 28, beyond (29) and no texture: the slot the texture would occupy contributes zero, every other minutiae part counts
    parts = [[[1.5, 2.25, 4.0, 8.0]]] * 6
    n_minu, n_tex = [0, 1, 2, 28, 29, 28], [1, 1, 1, 1, 1, 0]
    scores, parts = hand_search(parts, n_minu, n_tex)
    assert CM.tex_slots(n_minu, n_tex).tolist() == [0, 1, 2, 28, 29, -1]
    assert scores[:, 0].tolist() == [14.25, 13.5, 11.75, F(7.75 + 8.0 * 0.3), 7.75, 7.75]
    m = CM.stage1(scores, parts, n_minu, n_tex)
    assert m[:, 0].tolist() == [6.25, 5.5, 3.75, 7.75, 7.75, 7.75]
    assert m.dtype == np.float32


def test_the_model_cuts_a_tie_by_global_index_and_keeps_minus_ones_last():
    base = 1000
    # row 0: columns 1, 3, 4, 6 tie at 0 (no minutiae evidence), 2 and 5 are positive, 0 and 7 are empty prints; row 1 is latent-empty; row 2 has its texture in slot 2
    parts = np.zeros((3, 8, 4), F)
    parts[0, 2] = (3, 0, 1, 50); parts[0, 5] = (9, 0, 0, 0); parts[0, 1, 3] = 70; parts[0, 6, 3] = 90      # texture alone does not move a print in stage 1
    parts[2, :, 2] = np.arange(8)                                            # a minutiae part in slot 2 that the texture's slot rule hides
    parts[2, :, 0] = (0, 5, 0, 5, 0, 0, 1, 0)
    scores, parts = hand_search(parts, [28, 28, 2], [1, 1, 1], empty_cols=(0, 7), empty_rows=(1,))
    for keep, kept0 in ((1, [5]), (2, [5, 2]), (3, [5, 2, 1]), (4, [5, 2, 1, 3]), (5, [5, 2, 1, 3, 4]), (6, [5, 2, 1, 3, 4, 6]), (7, [5, 2, 1, 3, 4, 6, 0]),
                        (8, [5, 2, 1, 3, 4, 6, 0, 7]), (11, [5, 2, 1, 3, 4, 6, 0, 7])):
        e = CM.expected(scores, parts, [28, 28, 2], [1, 1, 1], keep, base)
        n = min(keep, 8)
        assert e["n_kept"].tolist() == [n] * 3
        assert e["kept_idx"][0].tolist() == [base + t for t in kept0] + [-1] * (keep - n), keep       # the cut inside the tie 1, 3, 4, 6: ascending global index; the -1 cells last
        assert e["kept_idx"][1].tolist() == [base + t for t in range(n)] + [-1] * (keep - n)           # a latent-empty row: all -1, by index
        assert e["kept_idx"][2, :2].tolist() == [base + 1, base + 3][:keep]                            # slot 2 is the texture's: parts[.., 2] does not rank
        mat = e["matrix"]
        assert (mat != CM.NO_ENTRY).sum(axis=1).tolist() == [n] * 3
        assert np.array_equal(mat[0, kept0], scores.view(np.uint32)[0, kept0]) and (mat[1, :n] == CM.MINUS_ONE).all()
        kp = e["kept_parts"].view(F)
        assert np.array_equal(kp[0, :n], parts[0, kept0]) and not e["kept_parts"][1].any() and not e["kept_parts"][:, n:].any()
    # the final score re-sorts the kept cells: column 6 (texture 90 in slot 28) overtakes column 5 once it is kept
    e = CM.expected(scores, parts, [28, 28, 2], [1, 1, 1], 6, base)
    _, idx, _ = CM.rank_rows(e["matrix"].view(F), 6, base)
    assert idx[0].tolist() == [base + 6, base + 1, base + 2, base + 5, base + 3, base + 4]
    # -0.0 and +0.0 are one key; the no-entry word is no entry; NaN of either sign has its place
    row = np.array([0x80000000, 0x00000000, 0xFFFFFFFF, 0x7FC00000, 0xFFC00000, 0xFF800000], np.uint32).view(F)[None, :]
    n_hits, idx, _ = CM.rank_rows(row, 6, 0)
    assert n_hits.tolist() == [4] and idx[0].tolist() == [3, 0, 1, 5, -1, -1]


# ---- cascade_tables.h -------------------------------------------------------------------------------------------------------------------------------------------
def test_cascade_tables_check_runs_clean_under_the_host_sanitizers():
    exe = os.path.join(CSRC, "cascade_tables_check")
    src = [os.path.join(CSRC, f) for f in ("cascade_tables_check.cpp", "cascade_tables.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in src):
        subprocess.run(["make", "-s", "-C", CSRC, "cascade_tables_check"], check=True)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("\ncascade_tables_check:"):]
    assert "-fsanitize=address,undefined" in rule[:rule.index("\n\n")] and "-fno-sanitize-recover=undefined" in rule[:rule.index("\n\n")]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"cascade_tables_check: \d+ cases ok", out.stdout), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert int(re.search(r"(\d+) cases ok", out.stdout).group(1)) >= 400
    main = open(src[0]).read()
    assert "int main(" in main
    for case in ("keep : {(size_t)1", "(size_t)64, (size_t)65", "chunk boundary inside a run", "{1, 0, 1}", "group boundary"):
        assert case in main, case
