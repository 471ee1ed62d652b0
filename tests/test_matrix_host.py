"""Kept matrices without a GPU: the six entry points are declared, exported by both libraries, bound by the Python host and absent from the taps header; the kernel
and the host unit are product objects; the three options are documented; csrc/matrix_fuse.h's cell rule — built with g++ under the host sanitizers as
matrix_fuse_check — is held against tests/matrix_model.py.  Everything is exact, words as integers: there is no tolerance anywhere.
(What the device answers is tests/test_gpu_matrix.py's.)"""
import importlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import matrix_model as MM

M = importlib.import_module("msu-latentafis_amd.host.matcher")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NEW = {"afis_matrix_keep": 2, "afis_matrix_free": 2, "afis_matrix_info": 3, "afis_matrix_read": 5, "afis_matrix_recall": 2, "afis_matrix_fuse": 7}
OPTIONS = ("matrix_device_bytes", "matrix_keep_us", "matrix_fuse_us")
SEED = 9411
MODES = (MM.SUM, MM.MAX, MM.MIN)


# ---- declared, exported, bound, built, documented ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    taps = open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, value in (("AFIS_FUSE_SUM", "0"), ("AFIS_FUSE_MAX", "1"), ("AFIS_FUSE_MIN", "2"), ("AFIS_FUSE_REQUIRE_ALL", "4"), ("AFIS_FUSE_OPERANDS_MAX", "16")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert (M.FUSE_SUM, M.FUSE_MAX, M.FUSE_MIN, M.FUSE_REQUIRE_ALL, M.FUSE_OPERANDS_MAX) == (0, 1, 2, 4, 16)
    assert re.search(r"typedef struct \{ int32_t n_q; int32_t normalized; int64_t columns; int32_t over_subset; int32_t stale; \} afis_matrix_desc;", code)
    import ctypes
    assert ctypes.sizeof(M.MatrixDesc) == 24 and M.MatrixDesc.columns.offset == 8 and M.MatrixDesc.stale.offset == 20
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        for name, n_args in NEW.items():
            assert re.search(r"\b(int|void)\s+%s\s*\(" % name, code), name
            assert name in M.EXPORTS and name not in M.TAP_EXPORTS and hasattr(lib, name)
            assert len(getattr(lib, name).argtypes) == n_args, name
            assert name not in taps, name
    for method in ("matrix_keep", "matrix_free", "matrix_info", "matrix_read", "matrix_recall", "matrix_fuse"):
        assert hasattr(M.Matcher, method), method
    at = [hdr.index(s) for s in ("int afis_search_prints_cascade(", "typedef struct afis_matrix afis_matrix;", "afis_matrix_keep  (", "afis_matrix_fuse  (", "int afis_get_timing(")]
    assert at == sorted(at)                                                 # the block stands behind the print cascade and before the timing calls
    block = hdr[hdr.index("/* Kept matrices"):hdr.index("typedef struct afis_matrix afis_matrix;")]
    assert "These calls do not give" in block and "different column sets" in block and "across shards" in block and "0x7fc00000" in block
    assert "Normalising along both axes of one matrix is not offered" in hdr and "the kept matrices below" in hdr


def test_the_kernel_and_the_host_unit_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "matrix_fuse.o" in objs and "afis_matrix.o" in objs
    assert re.search(r"^all:.*\bmatrix_fuse_check\b", mk, flags=re.M) and re.search(r"^\trm -f .*\bmatrix_fuse_check\b", mk, flags=re.M)
    assert re.search(r"^matrix_fuse_check:.*\n\tg\+\+ .*-ffp-contract=off.*-fsanitize=address,undefined", mk, flags=re.M)
    src = open(os.path.join(CSRC, "matrix_fuse.hip")).read()
    assert "__global__" in src and "k_matrix_fuse" in src and '#include "matrix_fuse.h"' in src
    assert "atomic" not in src.lower().replace("no atomic", "") and "__shared__" not in src and "hipMemset" not in src   # no atomics, no LDS, no memset before the launch
    for unit in ("afis_matrix.cpp", "matrix_fuse_check.cpp"):
        assert '#include "matrix_fuse.h"' in open(os.path.join(CSRC, unit)).read(), unit               # one text for the kernel, the host unit and the check program
    rule = open(os.path.join(CSRC, "matrix_fuse.h")).read()
    assert not re.search(r'#include\s+"(?!score_order\.h)', rule) and "hip" not in rule.replace("__HIPCC__", "").lower().replace(".hip", "")   # the standard library only
    assert "fma" not in rule.replace("fused multiply-add", "").lower()


def test_the_options_are_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only\)' % opt, hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]), opt
        assert "`%s`" % opt in integ, opt
    for recipe in ("Raw scores back after a normalisation", "S-norm", "symmetric print score"):
        assert recipe in integ, recipe
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Kept matrices" in design and "k_transpose_scores" in design[design.index("Kept matrices"):]


# ---- matrix_fuse_check against the model ----------------------------------------------------------------------------------------------------------------
def tool():
    exe = os.path.join(CSRC, "matrix_fuse_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, "matrix_fuse_check"], check=True)
    return exe


def run_tool(lines):
    out = subprocess.run([tool()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def command(mode, normalized, ops, weights):
    """ops [n][n_cells] uint32"""
    n, n_cells = ops.shape
    parts = ["fuse", "%x" % mode, "%x" % int(normalized), "%x" % n, "1" if weights is not None else "0"]
    if weights is not None:
        parts += ["%x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0] for x in weights]
    parts.append("%x" % n_cells)
    parts += ["%x" % int(c) for c in ops.reshape(-1)]
    return " ".join(parts)


def operand_words(rng, n, n_cells):
    """The special words against one another in every operand, then random words."""
    sp = MM.SPECIAL.view(np.uint32)
    ops = rng.integers(0, 1 << 32, (n, n_cells), dtype=np.uint64).astype(np.uint32)
    at = rng.random((n, n_cells)) < 0.6
    ops[at] = sp[rng.integers(0, len(sp), (n, n_cells))][at]
    if n >= 2:                                                              # every pair of special words in operands 0 and 1
        pairs = np.array([(a, b) for a in sp for b in sp], np.uint32)
        ops[0, :len(pairs)] = pairs[:, 0]; ops[1, :len(pairs)] = pairs[:, 1]
        ops[2:, :len(pairs)] = np.where(rng.random((n - 2, len(pairs))) < 0.5, np.uint32(0xffffffff), ops[2:, :len(pairs)])
    else:
        ops[0, :len(sp)] = sp
    return ops


def weight_sets(rng, n):
    inexact = np.array([0.1, 1.0 / 3.0, -0.7, 1e-3, 3.0000000000000004, 0.5, -2.5, 0.0, 1e300, -1e-300, 0.30000000000000004, 7.0 / 9.0, 1.0, -1.0, 2.0 ** -30, 1e10])
    return [None, np.ones(n), np.full(n, 0.5), rng.permutation(inexact)[:n], np.where(rng.random(n) < 0.3, 0.0, rng.standard_normal(n) * 3)]


@pytest.mark.parametrize("n", (1, 2, 3, 16))
def test_rule_against_the_model(n):
    rng = np.random.default_rng(SEED + n)
    n_cells = 400
    lines, want = [], []
    for normalized in (False, True):
        for require_all in (0, MM.REQUIRE_ALL):
            for op in MODES:
                for weights in (weight_sets(rng, n) if op == MM.SUM else [None]):
                    ops = operand_words(rng, n, n_cells)
                    lines.append(command(op | require_all, normalized, ops, weights))
                    want.append(MM.fuse([o.view(np.float32) for o in ops], op | require_all, normalized, weights).view(np.uint32))
    rows = run_tool(lines)
    assert len(rows) == len(want)
    seen = set()
    for row, w in zip(rows, want):
        assert row[0] == "0"
        got = np.array([int(t, 16) for t in row[1:]], np.uint32)
        assert np.array_equal(got, w), (n, np.flatnonzero(got != w)[:8].tolist(), [hex(int(t)) for t in got[got != w][:8]], [hex(int(t)) for t in w[got != w][:8]])
        seen.update(int(t) for t in w)
    assert {0xffffffff, 0xbf800000, 0x7fc00000} <= seen                    # no entry, the -1 of "nothing takes part", a sum that is no number: all three occur


def test_rule_small_cases_by_hand():
    f = lambda *x: np.array(x, np.float32)
    ne = MM.NO_ENTRY.view(np.float32)
    a, b = np.array([3.0, -1.0, ne, -1.0, ne, -0.0, 2.0], np.float32), np.array([4.0, 5.0, 6.0, -1.0, ne, -2.0, ne], np.float32)
    u = lambda x: x.view(np.uint32).tolist()
    assert u(MM.fuse([a, b], MM.SUM, False)) == u(f(7.0, 5.0, 6.0, -1.0, ne, 0.0, 2.0))
    assert u(MM.fuse([a, b], MM.SUM | MM.REQUIRE_ALL, False)) == u(f(7.0, -1.0, ne, -1.0, ne, -1.0, ne))
    assert u(MM.fuse([a, b], MM.MIN, False)) == u(f(3.0, 5.0, 6.0, -1.0, ne, -0.0, 2.0))
    assert u(MM.fuse([a, b], MM.MAX, True)) == u(f(4.0, 5.0, 6.0, -1.0, ne, -0.0, 2.0))
    assert u(MM.fuse([a, b], MM.MIN, True)) == u(f(3.0, -1.0, 6.0, -1.0, ne, -2.0, 2.0))
    assert u(MM.fuse([a, b], MM.SUM, True, [0.5, 0.5])) == u(f(3.5, 2.0, 3.0, -1.0, ne, -1.0, 1.0))
    rows = run_tool([command(m, nz, np.stack([a, b]).view(np.uint32), None) for m in (MM.SUM, MM.SUM | MM.REQUIRE_ALL, MM.MIN) for nz in (False, True)])
    want = [MM.fuse([a, b], m, nz) for m in (MM.SUM, MM.SUM | MM.REQUIRE_ALL, MM.MIN) for nz in (False, True)]
    for row, w in zip(rows, want):
        assert [int(t, 16) for t in row[1:]] == u(w)


def test_tool_refuses_what_the_rule_does_not_take():
    one = np.zeros((1, 1), np.uint32)
    rows = run_tool([command(3, False, one, None), command(8, False, one, None), command(7, False, one, None), command(0, False, np.zeros((17, 1), np.uint32), None),
                     command(MM.MIN | MM.REQUIRE_ALL, False, one, None)])
    assert [r[0] for r in rows] == ["1", "1", "1", "1", "0"]
