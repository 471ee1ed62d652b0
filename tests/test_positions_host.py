"""Rank positions without a GPU: the three entry points and the three AFIS_POS_* values are declared, exported by both libraries and bound by the Python host; the
kernel and its host unit are product objects; the option is documented; rank_order.h::count_before — the host statement of a position — built with g++ and held against
a numpy lexsort model on rows of special words; host/sharding.py::merge_positions against a global model for 1, 2 and 8 shards.  (What the device answers is
tests/test_gpu_rank_positions.py's.)"""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NEW = ("afis_rank_positions", "afis_rank_subject_positions", "afis_count_before")
STATUS = {"AFIS_POS_LISTED": 0, "AFIS_POS_NO_ENTRY": 1, "AFIS_POS_NOT_COVERED": 2}
OPTION = "rank_positions_us"
SEED = 5309
FLOOR = 0x007fffff                                                          # the ordered word of -inf: an entry's key reaches it
NO_ENTRY_WORD = 0xffffffff
SPECIAL = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0xbf800000, 0x3fc00000, 0x40500000, NO_ENTRY_WORD], np.uint32)   # +-inf, +-0, +-NaN, -1, 1.5, 3.25, no entry
KINDS = ("random", "special", "all zero", "99 % zero")


# ---- declared, exported, bound, built, documented ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, value in STATUS.items():
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), code, flags=re.M), name
    assert (SH.POS_LISTED, SH.POS_NO_ENTRY, SH.POS_NOT_COVERED) == (0, 1, 2)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        for name in NEW:
            assert re.search(r"\bint\s+%s\s*\(afis_ctx\*" % name, code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert getattr(lib, name).argtypes is not None, name
    for method in ("rank_positions", "rank_subject_positions", "count_before"):
        assert hasattr(M.Matcher, method), method
    assert hasattr(SH, "merge_positions")
    assert hdr.index("int afis_rank_subject_hits(") < hdr.index("int afis_rank_positions(") < hdr.index("int afis_rank_case_hits(")   # after the hit lists
    block = hdr[hdr.index("/* Rank positions"):hdr.index("int afis_rank_positions(")]
    left_out = block[block.index("These calls do not give"):]                # what the interface leaves out is said where it is declared
    assert "positions in case lists" in left_out and "column (reverse) lists" in left_out and "across shards" in left_out


def test_the_kernel_and_its_host_unit_are_product_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "rank_position.o" in objs and "afis_positions.o" in objs
    src = open(os.path.join(CSRC, "rank_position.hip")).read()
    assert "__global__" in src and "k_count_before" in src and "k_position_targets" in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*float", src) and "unsafeAtomicAdd" not in src   # integer adds only


def test_the_option_is_documented():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    assert re.search(r'"%s" \(read-only\)' % OPTION, hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")])
    assert "`%s`" % OPTION in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- rank_order.h::count_before against numpy -------------------------------------------------------------------------------------------------------
def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def template_key(x):
    return ordered((np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32))


def row_of(kind, n, rng):
    if kind == "random":
        return np.round(rng.standard_normal(n) * 4).astype(np.float32) / np.float32(2)     # many ties, both signs
    if kind == "special":
        return SPECIAL[rng.integers(0, len(SPECIAL), n)].view(np.float32)
    if kind == "all zero":
        return np.zeros(n, np.float32)
    return np.where(rng.random(n) < 0.99, 0.0, rng.random(n) * 5 + 0.01).astype(np.float32)


def model_count_before(row, glob, score, idx):
    """Entries (key >= FLOOR) other than the column named idx that stand before (score, idx): key descending, equal keys by ascending global index."""
    key = template_key(row).astype(np.int64); k = int(template_key(np.array([score], np.float32))[0])
    entry = (key >= FLOOR) & (glob != idx)
    return int((entry & ((key > k) | ((key == k) & (glob < idx)))).sum())


def model_positions(row, glob):
    """Per column its position in the row's list (lexsort: key descending, global index ascending; -1 for a column that is no entry)."""
    key = template_key(row).astype(np.int64)
    o = np.lexsort((glob, -key))
    o = o[key[o] >= FLOOR]
    pos = np.full(len(row), -1, np.int64); pos[o] = np.arange(len(o))
    return pos


def tool():
    exe = os.path.join(CSRC, "count_before_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", CSRC, "count_before_check"], check=True)
    return exe


def run_tool(tmp_path, row, glob, base, targets):
    f = tmp_path / "row.txt"
    words = row.view(np.uint32).tolist()
    lines = ["%d %d %d" % (len(row), base, 0 if glob is None else 1)]
    lines += ["%08x" % w if glob is None else "%08x %d" % (w, g) for w, g in zip(words, glob if glob is not None else words)]
    lines += ["%08x %d" % (int(np.float32(s).view(np.uint32)), i) for s, i in targets]
    f.write_text("\n".join(lines) + "\n")
    out = subprocess.run([tool(), str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return np.array(out.stdout.split(), np.int64)


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 17, 700])
def test_count_before_is_the_lexsort_position(n, kind, table, tmp_path):
    rng = np.random.default_rng([SEED, n, KINDS.index(kind), int(table)])
    row = row_of(kind, n, rng)
    base = 1000
    glob = base + np.arange(n, dtype=np.int64) if not table else np.sort(rng.permutation(5 * n)[:n]).astype(np.int64)[rng.permutation(n)] + 7   # a subset's columns in the caller's order
    # every column with its own score: its position; then hypothetical entries: the special words that are numbers at covered and uncovered indices
    own = [(row[i], int(glob[i])) for i in range(n)]
    hyp = [(s, int(i)) for s in SPECIAL[:4].view(np.float32).tolist() + [-1.0, 0.5, 2.0] for i in (0, int(glob[rng.integers(n)]), int(glob.max()) + 3)]
    own = [(s, i) for s, i in own if not np.isnan(s)]                       # (a NaN score is AFIS_EINVAL at the ABI; the host statement is held on numbers)
    got = run_tool(tmp_path, row, glob if table else None, base, own + hyp)
    want = np.array([model_count_before(row, glob, s, i) for s, i in own + hyp], np.int64)
    assert np.array_equal(got, want), (n, kind, table, np.flatnonzero(got != want)[:6].tolist())
    pos = model_positions(row, glob)
    at = {int(g): int(p) for g, p in zip(glob, pos)}
    for (s, i), c in zip(own, got[:len(own)]):
        if at[i] >= 0:
            assert c == at[i], (n, kind, i)                                 # a listed column's own count IS its position in the lexsort order
    if kind == "special" and n >= 700:
        assert (pos < 0).any() and (pos >= 0).any()


# ---- merge_positions against a global model -----------------------------------------------------------------------------------------------------------
def shard_answers(row, lo, hi, targets):
    """(status, score) of Matcher.rank_positions on the shard holding templates [lo, hi) for targets [(global index)], as the ABI states them."""
    st = np.full(len(targets), 2, np.int32); sc = np.full(len(targets), -np.inf, np.float32)
    key = template_key(row)
    for t, g in enumerate(targets):
        if lo <= g < hi:
            listed = key[g] >= FLOOR
            st[t] = 0 if listed else 1
            if listed:
                sc[t] = row[g]
    return st, sc


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shards", [1, 2, 8])
def test_merge_positions_against_a_global_model(shards, kind):
    G = 403
    rng = np.random.default_rng([SEED, shards, KINDS.index(kind)])
    row = row_of(kind, G, rng)
    glob = np.arange(G, dtype=np.int64)
    cuts = np.r_[0, np.sort(rng.permutation(np.arange(1, G))[:shards - 1]), G] if shards > 1 else np.array([0, G])
    if shards == 8:
        cuts[3] = cuts[2]                                                   # an empty shard
    targets = rng.permutation(G)[:150].tolist() + [G + 5, 10 ** 9]          # two that no shard covers
    per = [shard_answers(row, int(cuts[r]), int(cuts[r + 1]), targets) for r in range(shards)]
    status = np.stack([p[0] for p in per]); score = np.stack([p[1] for p in per])
    owner_score = np.where((status != 2).any(axis=0), score[(status != 2).argmax(axis=0), np.arange(len(targets))], np.float32(0)).astype(np.float32)
    counts = np.zeros((shards, len(targets)), np.int64)
    for r in range(shards):                                                 # Matcher.count_before on rank r: its own columns only
        lo, hi = int(cuts[r]), int(cuts[r + 1])
        for t, g in enumerate(targets):
            counts[r, t] = model_count_before(row[lo:hi], glob[lo:hi], owner_score[t], g)
    st, sc, nb, owner = SH.merge_positions(status, score, counts)
    assert st.dtype == np.int32 and sc.dtype == np.float32 and nb.dtype == np.int64 and owner.dtype == np.int64
    pos = model_positions(row, glob)
    for t, g in enumerate(targets):
        if g >= G:
            assert (st[t], nb[t], owner[t]) == (2, -1, -1) and np.isneginf(sc[t]), (t, g)
            continue
        assert cuts[owner[t]] <= g < cuts[owner[t] + 1]
        if pos[g] < 0:
            assert (st[t], nb[t]) == (1, -1) and np.isneginf(sc[t]), (t, g)
        else:
            assert (st[t], nb[t]) == (0, pos[g]) and sc[t].view(np.uint32) == row[g].view(np.uint32), (t, g, int(nb[t]), int(pos[g]))
    with pytest.raises(ValueError):
        SH.merge_positions(np.zeros((2, 1), np.int32), np.zeros((2, 1), np.float32), np.zeros((2, 1), np.int64))   # two owners
