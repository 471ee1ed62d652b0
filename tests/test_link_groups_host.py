"""Link groups without a GPU: the two entry points are declared, exported by both libraries, bound by the Python host and absent from the taps header; the kernels and
the host unit are product objects; the two options are documented; csrc/link_groups.h's host half — built with g++ under the host sanitizers as link_groups_check —
passes its own checks (node tables, the arrangement, a sequential rendering of the union against a breadth-first labelling) and arranges random pair lists as the
Python model (tests/link_model.py) does; host/sharding.py::merge_link_groups over 2 and 3 column cuts of one matrix equals the model's groups of the whole matrix.
Everything is exact: integers and names.  (What the device answers is tests/test_gpu_link_groups.py's.)"""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import link_model as LM

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NEW = {"afis_link_groups": 17, "afis_link_subject_groups": 18}
OPTIONS = ("link_groups_us", "link_d2h_bytes")
SEED = 9311


# ---- declared, exported, bound, built, documented ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+AFIS_LINK_ANY\s+0\b", code) and re.search(r"#define\s+AFIS_LINK_MUTUAL\s+1\b", code)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        for name, n_args in NEW.items():
            assert re.search(r"\bint\s+%s\s*\(" % name, code), name
            assert name in M.EXPORTS and name not in M.TAP_EXPORTS and hasattr(lib, name)
            assert len(getattr(lib, name).argtypes) == n_args, name
            assert name not in taps, name
    for method in ("link_groups", "link_subject_groups"):
        assert hasattr(M.Matcher, method), method
    assert hasattr(SH, "merge_link_groups")
    assert hdr.index("int afis_entries_at(") < hdr.index("int afis_link_groups(") < hdr.index("int afis_link_subject_groups(") < hdr.index("int afis_rank_case_hits(")
    block = hdr[hdr.index("/* Link groups"):hdr.index("#define AFIS_LINK_ANY")]
    for word in ("AFIS_LINK_MUTUAL", "single linkage", "These calls do not give", "merge_link_groups", "the union did not settle", "-1 - q"):
        assert word in block, word


def test_the_kernels_and_the_host_unit_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "link_groups.o" in objs and "afis_link.o" in objs
    assert re.search(r"^all:.*\blink_groups_check\b", mk, flags=re.M) and re.search(r"^\trm -f .*\blink_groups_check\b", mk, flags=re.M)
    assert re.search(r"^link_groups_check:.*\n\tg\+\+ .*-fsanitize=address,undefined", mk, flags=re.M)
    assert re.search(r"^link_groups\.o: link_groups\.hip link_groups\.h ", mk, flags=re.M) and re.search(r"^afis_link\.o: afis_link\.cpp link_groups\.h ", mk, flags=re.M)
    src = open(os.path.join(CSRC, "link_groups.hip")).read()
    assert "__global__" in src and "k_link_scan" in src and "k_link_flatten" in src and "k_link_compact" in src and '#include "link_groups.h"' in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)", src) and "unsafeAtomicAdd" not in src   # integer atomics only
    code = src[src.index("#include"):]
    assert "cooperative" not in code.lower() and "grid.sync" not in code and "this_grid" not in code   # kernel boundaries, no grid barrier
    assert "__HIP_MEMORY_SCOPE_AGENT" in src                                # parent[] is read and written by atomics of agent scope while the hooks run
    for unit in ("afis_link.cpp", "link_groups_check.cpp"):
        assert '#include "link_groups.h"' in open(os.path.join(CSRC, unit)).read(), unit   # one text for the kernels, the host unit and the check program
    hdr = open(os.path.join(CSRC, "link_groups.h")).read()
    assert re.findall(r'#include\s+"([^"]+)"', hdr) == ["column_names.h", "score_order.h"]   # the standard library, score_order.h and the column names' view only ...
    assert not re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, "column_names.h")).read())   # ... which is the standard library alone
    dev = open(os.path.join(CSRC, "afis_device.h")).read()
    assert re.search(r"kLinkChunkScalar\s*=\s*256,\s*kLinkChunkVec\s*=\s*1024", dev) and re.search(r"kFilterRows\s*=\s*8", dev)   # what tests/test_gpu_link_groups.py sizes its cases by
    link = open(os.path.join(CSRC, "afis_link.cpp")).read()
    assert "FilterPass" in link and "check_filtered(" in link and "link_arrange(" in link   # the filtered calls' checks and filter pass, not a second definition
    assert "MatrixCall mc{ctx, who, subj, kTemplateCells, {ctx, labels, masks, subj ? no_cells : pairs, subj != nullptr}}" in link and "queue_cells(" not in link   # ... the FilterPass the matrix calls' driver holds and queues


def test_the_options_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    api = open(os.path.join(CSRC, "afis_api.cpp")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only\)' % opt, hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]), opt
        assert "`%s`" % opt in integ, opt
        assert '"%s"' % opt in api, opt
    assert "afis_link_groups" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "afis_link_groups" in design and "link_groups.hip" in design


# ---- link_groups_check ------------------------------------------------------------------------------------------------------------------------------
def tool():
    exe = os.path.join(CSRC, "link_groups_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, "link_groups_check"], check=True)
    return exe


def test_the_check_program_passes_under_its_sanitizers():
    out = subprocess.run([tool()], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "link_groups_check: ok", (out.stdout[-500:], out.stderr[-2000:])


def test_the_arrangement_against_the_model():
    """Random groupings of random node sets, pairs in random order and labelled by any member: the tool's CSR is the model's, at every cap."""
    rng = np.random.default_rng(SEED)
    for rep in range(40):
        n_col, base, n_q = int(rng.integers(1, 30)), int(rng.integers(0, 2000)), int(rng.integers(0, 12))
        row_node = np.where(rng.random(n_q) < 0.4, -1, rng.integers(max(base - 3, 0), base + n_col + 4, n_q)).astype(np.int64)
        extra = sorted(set(int(t) for t in row_node if t >= 0 and not base <= t < base + n_col))
        names = [base + p for p in range(n_col)] + extra + [-1 - q for q in range(n_q) if row_node[q] < 0]   # name of node number i
        part = rng.integers(0, max(len(names) // 2, 1), len(names))        # a random grouping of the nodes
        groups = [[i for i in range(len(names)) if part[i] == g] for g in range(int(part.max()) + 1)]
        groups = [g for g in groups if len(g) >= 2]
        pairs = [(i, min(g)) for g in groups for i in g]
        pairs = [pairs[i] for i in rng.permutation(len(pairs))]
        want_groups = sorted((sorted((names[i] for i in g), key=LM.node_key) for g in groups), key=lambda g: LM.node_key(g[0]))
        total = sum(len(g) for g in groups)
        for cg, cm in ((len(groups), total), (0, 0), (max(len(groups) - 1, 0), total), (len(groups), max(total - 1, 0)), (int(rng.integers(0, len(groups) + 2)), int(rng.integers(0, total + 2)))):
            text = "%d %d %d %s %d %s %d %d\n" % (n_col, base, n_q, " ".join(str(int(t)) for t in row_node), len(pairs), " ".join("%d %d" % p for p in pairs), cg, cm)
            out = subprocess.run([tool(), "arrange"], input=text, capture_output=True, text=True)
            assert out.returncode == 0, out.stderr[-2000:]
            lines = out.stdout.split("\n")
            n_groups, n_members, n_listed, off, member = LM.csr(want_groups, cg, cm)
            assert [int(t) for t in lines[0].split()] == [n_groups, n_members, n_listed], (rep, cg, cm)
            assert [int(t) for t in lines[1].split()] == off.tolist() and [int(t) for t in lines[2].split()] == member.tolist(), (rep, cg, cm)


# ---- merge_link_groups against the model ------------------------------------------------------------------------------------------------------------
def planted_matrix(rng, n_q, G, share):
    rows = rng.uniform(0, 1, (n_q, G)).astype(np.float32)
    rows[rng.random((n_q, G)) < share] = np.float32(5.0)
    return rows


def as_result(d):
    return {"group_off": d["group_off"], "member": d["member"]}


@pytest.mark.parametrize("cuts", ((0, 23, 60), (0, 11, 37, 60), (0, 59, 60)))
def test_merged_groups_of_column_cuts_equal_the_whole(cuts):
    G, base, thr = 60, 1000, 2.0
    rng = np.random.default_rng(SEED + len(cuts) + cuts[1])
    glob = base + np.arange(G, dtype=np.int64)
    for what, n_q, row_node, share in (("latents", 9, None, 0.02), ("prints", G, glob, 0.004), ("prints and latents", 14, np.where(np.arange(14) % 3 == 0, -1, base + 4 * np.arange(14)), 0.02)):
        rows = planted_matrix(rng, n_q, G, share)
        whole = LM.link(rows, thr, glob, row_node)
        assert whole["n_groups"] >= 1, what
        per = [LM.link(rows[:, lo:hi], thr, glob[lo:hi], row_node) for lo, hi in zip(cuts[:-1], cuts[1:])]   # every rank: its columns, all the rows, the same row names
        got = SH.merge_link_groups([as_result(p) for p in per])
        assert got["n_groups"] == whole["n_groups"] and got["n_members"] == whole["n_members"], what
        assert np.array_equal(got["group_off"], whole["group_off"]) and np.array_equal(got["member"], whole["member"]), what
        assert got["group_off"].dtype == np.int64 and got["member"].dtype == np.int64


def test_a_group_that_exists_only_through_a_shared_latent():
    """Latent 1 hits print 1003 on rank 0 and print 1031 on rank 1: each rank sees a pair, the merge one group of three through the anonymous name -2."""
    G, base = 40, 1000
    glob = base + np.arange(G, dtype=np.int64)
    rows = np.zeros((3, G), np.float32)
    rows[1, 3] = rows[1, 31] = 9.0; rows[2, 35] = 9.0
    per = [LM.link(rows[:, :20], 1.0, glob[:20]), LM.link(rows[:, 20:], 1.0, glob[20:])]
    assert [p["member"].tolist() for p in per] == [[1003, -2], [1031, -2, 1035, -3]]
    got = SH.merge_link_groups([as_result(p) for p in per])
    assert got["group_off"].tolist() == [0, 3, 5] and got["member"].tolist() == [1003, 1031, -2, 1035, -3]
    whole = LM.link(rows, 1.0, glob)
    assert np.array_equal(got["member"], whole["member"]) and np.array_equal(got["group_off"], whole["group_off"])
    # no rank, or ranks without groups: nothing
    for per in ([], [{"group_off": np.zeros(1, np.int64), "member": np.zeros(0, np.int64)}] * 2):
        none = SH.merge_link_groups(per)
        assert none["n_groups"] == 0 and none["group_off"].tolist() == [0] and len(none["member"]) == 0
    for bad in ({"group_off": [1, 3], "member": [1, 2, 3]}, {"group_off": [0, 1], "member": [5]}, {"group_off": [0, 2], "member": [5, 6, 7]}, {"group_off": [], "member": []}):
        with pytest.raises(ValueError):
            SH.merge_link_groups([bad])
