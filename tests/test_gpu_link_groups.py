"""Link groups on the GPU: afis_link_groups, afis_link_subject_groups.

The yardstick is tests/link_model.py — numpy and plain Python, never the code under test: a cell's key is ordered((x + 0).view(u32)), a cell reaches at a key >= the
key of min_score, the edges are spelled out cell by cell under both modes and both forms, the components come from a dictionary union-find.  Everything is compared
exactly: counts as integers, members as names; there is no tolerance anywhere.

Matrices are planted with the tap afis_debug_rank_hits, which leaves its matrix rankable, on a packed gallery of one-point templates (the recipe of
tests/test_gpu_score_hist.py); index_base is 1000.  The scan kernel gives a workgroup 256 adjacent columns of a row (one column per thread), or 1024 where the row length
is a multiple of four (16-byte loads) — csrc/afis_device.h: kLinkChunkScalar, kLinkChunkVec — and walks strips of 8 rows (kFilterRows): the sizes sit before, on and
after those edges."""
import importlib

import numpy as np
import pytest

import link_model as LM

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")

SEED = 9377
BASE = 1000
ESTATE, EINVAL = "afis error -3", "afis error -1"
NINF = float("-inf")
NO_ENTRY_WORD = np.uint32(0xffffffff)
U64 = np.uint64
ANY, MUTUAL = LM.ANY, LM.MUTUAL
CHUNK_SCALAR, CHUNK_VEC, STRIP = 256, 1024, 8                               # kLinkChunkScalar, kLinkChunkVec, kFilterRows
G_ALL = (1, 3, 4, 63, 64, 65, CHUNK_SCALAR - 1, CHUNK_SCALAR, CHUNK_SCALAR + 1, CHUNK_VEC - 1, CHUNK_VEC, CHUNK_VEC + 1, 2 * CHUNK_VEC + 4)
N_Q = (1, 7, 8, 9, 17)
G_MAX = 4097
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0xbf800000, 0x47800000, 0x477fffff, 0x35000000, 0x35c00000, 0xffffffff],
                   np.uint32).view(np.float32)                              # tests/test_gpu_score_hist.py's: +-0, +-inf, +-NaN, -1, 65536, the float below it, two small values, no entry
HIT, THR = np.float32(5.0), 2.0


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def tiny(cb):
    """4097 rolled templates of one minutia and one texture point each, made as one packed gallery."""
    G = G_MAX
    rng = np.random.default_rng(SEED)
    des = rng.standard_normal((G, 96)).astype(np.float32)
    des /= np.linalg.norm(des, axis=1, keepdims=True)
    off = np.arange(G + 1, dtype=np.int64)
    return S.PackedGallery(off, rng.integers(0, 500, G).astype(np.int16), rng.integers(0, 500, G).astype(np.int16), rng.uniform(-3, 3, G).astype(np.float32), des,
                           off.copy(), rng.integers(0, 30, G).astype(np.int16), rng.integers(0, 30, G).astype(np.int16), rng.uniform(-1.5, 1.5, G).astype(np.float32),
                           rng.integers(0, cb.K, (G, cb.M)).astype(np.uint8))


def tap_matcher(cbb, tiny, G, lo=0, base=BASE):
    m = M.Matcher(cbb, taps=True)
    m.gallery_add_packed(tiny.slice(lo, lo + G)); m.gallery_commit(base)
    return m


def plant(m, rows):
    """The matrix of the "last search": uploaded by the tap, which leaves it rankable."""
    m.debug_rank_hits(None, rows, NINF, 1)


def same(got, want, what):
    for key in ("n_edges", "n_groups", "n_members", "n_listed"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert got["group_off"].dtype == np.int64 and got["member"].dtype == np.int64
    assert np.array_equal(got["group_off"], want["group_off"]) and np.array_equal(got["member"], want["member"]), (what, got["member"][:12].tolist(), want["member"][:12].tolist())


def check(m, rows, glob, what, min_score=THR, row_node=None, ok=None, modes=(ANY, MUTUAL), **kw):
    """Both modes of afis_link_groups against the model, lists complete; -> the ANY result."""
    first = None
    for mode in modes:
        want = LM.link(rows, min_score, glob, row_node, mode, ok)
        got = m.link_groups(min_score, mode, row_node=row_node, **kw)
        same(got, want, (what, mode))
        assert m.get_option("link_groups_us") > 0 and m.get_option("link_d2h_bytes") == 32 + 8 * want["n_members"], (what, mode)
        first = got if first is None else first
    return first


def check_subjects(m, hs, rows, glob, ids, what, min_score=THR, row_node=None, ok=None, modes=(ANY, MUTUAL), **kw):
    """ids [columns]: the subject id of every column's template."""
    first = None
    for mode in modes:
        want = LM.link(rows, min_score, ids, row_node, mode, ok, glob=glob)
        got = m.link_subject_groups(hs, min_score, mode, row_node=row_node, **kw)
        same(got, want, (what, mode))
        first = got if first is None else first
    return first


def sparse(n_q, G, rng, per_row=2.0, special=0.1):
    """Cells uniform in [0, 1) — below THR —, about per_row cells of a row at 5.0, and the special words sprinkled over the rest."""
    rows = rng.uniform(0, 1, (n_q, G)).astype(np.float32)
    at = rng.random((n_q, G)) < special
    rows[at] = SPECIAL[rng.integers(0, len(SPECIAL), (n_q, G))][at]
    rows[rng.random((n_q, G)) < min(0.5, per_row / G)] = HIT
    return rows


def print_rows(G):
    return BASE + np.arange(G, dtype=np.int64)


# ---- 1: row lengths and rows; latents, and rows that are prints ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", G_ALL)
def test_row_lengths(G, codebook_bytes, tiny):
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + G)
    glob = print_rows(G)
    for n_q in N_Q:
        rows = sparse(n_q, G, rng)
        rows[n_q - 1, G - 1] = HIT                                          # the last cell of the matrix is an edge
        plant(m, rows)
        got = check(m, rows, glob, (G, n_q, "latents"))
        assert got["n_edges"] >= 1                                          # (the special words 65536, +inf and +NaN reach too)
        named = np.where(rng.random(n_q) < 0.3, -1, BASE + rng.integers(0, G, n_q)).astype(np.int64)   # rows that are resident prints, repeated or not, among latents
        check(m, rows, glob, (G, n_q, "prints"), row_node=named)
    m.close()


# ---- 2: graph shapes, print-search style: row i is print i -------------------------------------------------------------------------------------------------------
def shapes_matcher(codebook_bytes, tiny, G):
    return tap_matcher(codebook_bytes, tiny, G), print_rows(G), np.zeros((G, G), np.float32)


def test_no_edge_at_all(codebook_bytes, tiny):
    G = 300
    m, glob, rows = shapes_matcher(codebook_bytes, tiny, G)
    rows[np.arange(G), np.arange(G)] = HIT                                  # every print hits itself, and nothing else
    plant(m, rows)
    got = check(m, rows, glob, "self cells only", row_node=glob)
    assert got["n_edges"] == 0 and got["n_groups"] == 0 and got["group_off"].tolist() == [0] and len(got["member"]) == 0
    assert m.get_option("link_d2h_bytes") == 32                             # the counters, and no pair
    m.close()


@pytest.mark.parametrize("shape", ("path", "path, descending", "stars", "pairs", "a bridge"))
def test_graph_shapes(shape, codebook_bytes, tiny):
    G = 2049
    m, glob, rows = shapes_matcher(codebook_bytes, tiny, G)
    i = np.arange(G - 1)
    if shape == "path":                                                     # the deepest tree a hook order can build
        rows[i, i + 1] = HIT
    elif shape == "path, descending":
        rows[i + 1, i] = HIT
    elif shape == "stars":                                                  # every row at one column; one row at every column: two stars that share no node
        rows[np.arange(1, 1000), 0] = HIT; rows[1500, 1001:1400] = HIT
    elif shape == "pairs":                                                  # 1000 disjoint pairs, confirmed in both directions
        rows[2 * np.arange(1000), 2 * np.arange(1000) + 1] = HIT; rows[2 * np.arange(1000) + 1, 2 * np.arange(1000)] = HIT
    else:                                                                   # two paths, mutual ones, joined by the single cell (700, 1300)
        for a, b in ((0, 900), (1100, 2000)):
            j = np.arange(a, b); rows[j, j + 1] = HIT; rows[j + 1, j] = HIT
    plant(m, rows)
    got = check(m, rows, glob, shape, row_node=glob)
    if shape.startswith("path"):
        assert got["n_groups"] == 1 and got["n_members"] == G and got["member"].tolist() == glob.tolist() and got["n_edges"] == G - 1
        assert m.link_groups(THR, MUTUAL, row_node=glob)["n_groups"] == 0   # one direction only: nothing is confirmed
    elif shape == "stars":
        assert got["n_groups"] == 2 and got["group_off"].tolist() == [0, 1000, 1400]
    elif shape == "pairs":
        assert got["n_groups"] == 1000 and got["n_edges"] == 2000 and np.array_equal(got["group_off"], 2 * np.arange(1001)) and m.link_groups(THR, MUTUAL, row_node=glob)["n_groups"] == 1000
    else:
        assert got["n_groups"] == 2
        rows[700, 1300] = HIT
        plant(m, rows)
        got = check(m, rows, glob, "the bridge", row_node=glob)
        assert got["n_groups"] == 1 and got["n_members"] == 901 + 901
        assert m.link_groups(THR, MUTUAL, row_node=glob)["n_groups"] == 2   # the bridge is not confirmed
    m.close()


def test_every_cell_reaches(codebook_bytes, tiny):
    """Latent style, 17 x 4097: one group, every hook contending on one root."""
    n_q, G = 17, G_MAX
    m = tap_matcher(codebook_bytes, tiny, G)
    rows = np.full((n_q, G), HIT, np.float32)
    plant(m, rows)
    got = check(m, rows, print_rows(G), "all cells", modes=(ANY,))
    assert got["n_edges"] == n_q * G and got["n_groups"] == 1 and got["n_members"] == G + n_q
    assert got["member"].tolist() == print_rows(G).tolist() + [-1 - q for q in range(n_q)]
    assert m.link_groups(THR, MUTUAL)["n_groups"] == 0                      # a latent is no column: nothing can be confirmed
    m.close()


# ---- 3: bit patterns on both sides of min_score ----------------------------------------------------------------------------------------------------------------------
def test_bit_patterns(codebook_bytes, tiny):
    G, n_q = 65, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 3)
    glob = print_rows(G)
    rows = rng.uniform(-1, 1, (n_q, G)).astype(np.float32)
    at = rng.random((n_q, G)) < 0.5
    rows[at] = SPECIAL[rng.integers(0, len(SPECIAL), (n_q, G))][at]
    rows[0, :len(SPECIAL)] = SPECIAL; rows[1] = NO_ENTRY_WORD.view(np.float32); rows[2] = np.float32(-0.0); rows[3, ::2] = np.float32(0.0)
    plant(m, rows)
    named = BASE + rng.integers(0, G, n_q).astype(np.int64)
    in_matrix = float(rows[4][np.isfinite(rows[4]) & (rows[4] > 0.5)][0])
    for thr in (NINF, -0.0, 0.0, in_matrix, 65536.0, float(np.uint32(0x35000000).view(np.float32)), float("inf")):
        a = check(m, rows, glob, ("latents", thr), min_score=thr)
        check(m, rows, glob, ("prints", thr), min_score=thr, row_node=named)
        if thr == NINF:
            assert a["n_edges"] == int((LM.key_of(rows) >= LM.FLOOR).sum()) < n_q * G   # every entry, and the no-entry words and the NaNs with the sign set are none
    assert m.link_groups(-0.0)["n_edges"] == m.link_groups(0.0)["n_edges"]  # the two zeros are one value
    m.close()


# ---- 4: the node rules ----------------------------------------------------------------------------------------------------------------------------------------------
def test_node_rules(codebook_bytes, tiny):
    G = 40
    m = tap_matcher(codebook_bytes, tiny, G)
    glob = print_rows(G)
    # rows: print 1005 twice, a latent, a print of another rank (5000), a print below the base (3), print 1005's neighbour 1006, print 5000 again
    row_node = np.array([1005, 1005, -1, 5000, 3, 1006, 5000], np.int64)
    rows = np.zeros((7, G), np.float32)
    rows[0, 5] = HIT; rows[1, 5] = HIT                                      # self cells of the repeated print: no edge
    rows[0, 9] = HIT                                                        # 1005 - 1009
    rows[1, 12] = HIT                                                       # the second copy of the row is the same node: 1005 - 1012
    rows[2, 9] = HIT                                                        # the latent joins them: -3
    rows[3, 20] = HIT; rows[6, 21] = HIT                                    # 5000 - 1020, 5000 - 1021: one node, named twice
    rows[4, 30] = HIT                                                       # 3 - 1030
    rows[5, 6] = HIT                                                        # self
    plant(m, rows)
    got = check(m, rows, glob, "node rules", row_node=row_node)
    assert got["n_edges"] == 6
    assert [got["member"][a:b].tolist() for a, b in zip(got["group_off"][:-1], got["group_off"][1:])] == [[3, 1030], [1005, 1009, 1012, -3], [1020, 1021, 5000]]
    # mutual: 1005 -> 1006 and 1006 -> 1005 confirm one another through the FIRST row of 1005; 5000 is no column, so nothing of it is confirmed
    rows[0, 6] = HIT; rows[5, 5] = HIT
    plant(m, rows)
    got = check(m, rows, glob, "node rules, mutual", row_node=row_node)
    mut = m.link_groups(THR, MUTUAL, row_node=row_node)
    assert mut["n_edges"] == 2 and mut["member"].tolist() == [1005, 1006]
    rows[0, 6] = 0.0; rows[1, 6] = HIT                                      # the second row of 1005 reaches 1006, the first does not: (1, 1006) is confirmed by (row of 1006, 1005), but 1006 -> 1005 looks at the FIRST row of 1005 and is not
    plant(m, rows)
    check(m, rows, glob, "node rules, the first row counts", row_node=row_node)
    mut = m.link_groups(THR, MUTUAL, row_node=row_node)
    assert mut["n_edges"] == 1 and mut["member"].tolist() == [1005, 1006]
    m.close()


# ---- 5: mutual mode -------------------------------------------------------------------------------------------------------------------------------------------------
def test_mutual_mode(codebook_bytes, tiny):
    G = CHUNK_SCALAR + 5
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 5)
    glob = print_rows(G)
    rows = rng.uniform(0, 1, (G, G)).astype(np.float32)
    pairs = rng.permutation(G)[:120].reshape(60, 2)
    for k, (a, b) in enumerate(pairs):                                      # a third confirmed, a third forward only, a third backward only
        if k % 3 != 2: rows[a, b] = HIT
        if k % 3 != 1: rows[b, a] = HIT
    plant(m, rows)
    check(m, rows, glob, "asymmetric", row_node=glob)
    mut = m.link_groups(THR, MUTUAL, row_node=glob)
    assert mut["n_groups"] == 20 and mut["n_edges"] == 40 and m.link_groups(THR, ANY, row_node=glob)["n_groups"] == 60
    # the reverse cell removed by an exclusion list: pair 0 is confirmed until row b may not see column a
    a, b = (int(t) for t in pairs[0])
    excl = [np.zeros(0, np.int64) for _ in range(G)]
    excl[b] = np.array([BASE + a], np.int64)
    ok = LM.not_excluded(glob, excl, G)
    check(m, rows, glob, "reverse cell excluded", row_node=glob, ok=ok, excl=excl)
    assert m.link_groups(THR, MUTUAL, row_node=glob, excl=excl)["n_groups"] == 19
    # a pair whose reverse cell does not exist: only the first 100 prints are rows
    part = np.ascontiguousarray(rows[:100])
    plant(m, part)
    check(m, part, glob, "reverse row missing", row_node=glob[:100])
    # ... and rows in another order than the columns: the reverse row is found by name
    order = rng.permutation(G)
    mixed = np.ascontiguousarray(rows[order])
    plant(m, mixed)
    got = check(m, mixed, glob, "rows permuted", row_node=glob[order])
    same(m.link_groups(THR, MUTUAL, row_node=glob[order]), mut, "rows permuted, mutual")
    m.close()


# ---- 6: the subject form --------------------------------------------------------------------------------------------------------------------------------------------
def test_subject_form(codebook_bytes, tiny):
    G = CHUNK_SCALAR + 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 6)
    glob = print_rows(G)
    ids = (7000 + rng.permutation(G) // 3).astype(np.int64)                 # persons of three prints (one of fewer), scattered over the shard
    hs = m.subjects_create(ids)
    person = lambda p: np.flatnonzero(ids == p)
    # rows: one per person of the first 60 persons, named by the person; then a latent; then a person the handle does not hold
    row_node = np.concatenate([7000 + np.arange(60), [-1, 99999]]).astype(np.int64)
    n_q = len(row_node)
    rows = rng.uniform(0, 1, (n_q, G)).astype(np.float32)
    for p in range(60):
        rows[p, person(7000 + p)] = HIT                                     # two prints of one person never link: a person against their own prints
    rows[0, person(7001)[1]] = HIT; rows[1, person(7000)[-1]] = HIT         # 7000 and 7001 linked through different prints of theirs; neither reverse cell stands at the other person's FIRST column
    rows[2, person(7003)[1]] = HIT; rows[3, person(7002)[0]] = HIT          # 7002 and 7003: the reverse cell of (2, .) stands at 7002's first column
    rows[4, person(7030)[2]] = HIT                                          # 7004 -> 7030, one direction
    rows[60, person(7004)[0]] = HIT; rows[60, person(7050)[1]] = HIT        # the latent links 7004 and 7050
    rows[61, person(7050)[0]] = HIT                                         # 99999 is a node of that name
    plant(m, rows)
    got = check_subjects(m, hs, rows, glob, ids, "persons", row_node=row_node)
    assert [got["member"][a:b].tolist() for a, b in zip(got["group_off"][:-1], got["group_off"][1:])] == [[7000, 7001], [7002, 7003], [7004, 7030, 7050, 99999, -61]]
    assert got["n_edges"] == 8
    mut = m.link_subject_groups(hs, THR, MUTUAL, row_node=row_node)
    assert mut["n_edges"] == 1 and mut["group_off"].tolist() == [0, 2] and mut["member"].tolist() == [7002, 7003]   # a reverse cell at another print of the same person is not seen
    # exclusions name persons: row 60 may not see 7050 (and an id nobody holds is ignored)
    excl = [np.zeros(0, np.int64) for _ in range(n_q)]
    excl[60] = np.array([7050, 123456], np.int64); excl[3] = np.array([7002], np.int64)
    ok = LM.not_excluded(ids, excl, n_q)
    got = check_subjects(m, hs, rows, glob, ids, "persons, exclusions", row_node=row_node, ok=ok, excl=excl)
    assert [7050, 99999] in [got["member"][a:b].tolist() for a, b in zip(got["group_off"][:-1], got["group_off"][1:])]
    # latents only, and the template form of the same matrix for contrast: there two prints of one person do link
    check_subjects(m, hs, rows, glob, ids, "persons, latent rows")
    check(m, rows, glob, "the same matrix, templates")
    # a subset listed out of order: the device's columns are the listed prints by ascending global index
    listed = BASE + rng.permutation(G)[:97].astype(np.int64)
    held = np.sort(listed)
    sub = m.subset_create(listed)
    srows = sparse(12, len(held), rng, per_row=3.0)
    m.debug_rank_rows(srows, 1, subset=sub)                                 # the matrix in the device's column order
    sub_row = np.concatenate([ids[held[:5] - BASE], [-1, -1, 99999, 7000, 7001, 7002, 7003]]).astype(np.int64)
    check_subjects(m, hs, srows, held, ids[held - BASE], "persons, subset", row_node=sub_row)
    check(m, srows, held, "templates, subset", row_node=np.concatenate([held[:6], [-1, BASE + G + 3], listed[:4]]).astype(np.int64))
    m.subset_free(sub); m.subjects_free(hs)
    m.close()


# ---- 7: filters and exclusions ----------------------------------------------------------------------------------------------------------------------------------------
def test_filters(codebook_bytes, tiny):
    G, n_q = CHUNK_VEC + 4, STRIP + 4
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 7)
    glob = print_rows(G)
    rows = sparse(n_q, G, rng, per_row=6.0)
    labels = (U64(1) << rng.integers(0, 10, G).astype(U64))
    masks = np.zeros((n_q, 3), U64)
    for q in range(n_q):
        masks[q] = [(U64(0b11 << (q % 9)), 0, 0), (0, 0, U64(0b111 << (q % 8))), (0, 0, 0)][q % 3]
    excl = [BASE + rng.integers(-5, G + 5, int(rng.integers(0, 40))).astype(np.int64) for _ in range(n_q)]
    hits = [np.flatnonzero(rows[q] == HIT) for q in range(n_q)]
    excl[1] = np.concatenate([excl[1], BASE + hits[1][:1]])                 # a cell that reaches is excluded
    plant(m, rows)
    hl = m.labels_create(labels)
    before = m.rank_hits(NINF, 64)
    ok_m, ok_e = LM.label_test(labels, masks), LM.not_excluded(glob, excl, n_q)
    assert (~ok_m & (rows == HIT)).any() and (~ok_e & (rows == HIT)).any()
    named = np.where(np.arange(n_q) % 2 == 0, -1, BASE + rng.integers(0, G, n_q)).astype(np.int64)
    for what, kw, ok in (("masks", dict(labels=hl, masks=masks), ok_m), ("exclusions", dict(excl=excl), ok_e), ("both", dict(labels=hl, masks=masks, excl=excl), ok_m & ok_e),
                         ("plain, after the filtered calls", {}, None)):
        got = check(m, rows, glob, what, ok=ok, **kw)
        check(m, rows, glob, (what, "prints"), row_node=named, ok=ok, **kw)
        # the identity: in ANY mode with latent rows an edge is a hit
        for thr in (THR, 0.5, NINF):
            assert m.link_groups(thr, ANY, cap_groups=0, cap_members=0, **kw)["n_edges"] == int(m.rank_hits_filtered(thr, 1, **kw)["n_hits"].sum()), (what, thr)
    after = m.rank_hits(NINF, 64)
    for key in ("n_hits", "idx", "score"):
        assert np.array_equal(before[key].view(np.uint32) if key == "score" else before[key], after[key].view(np.uint32) if key == "score" else after[key]), key   # the matrix is unwritten
    # labels and masks that remove the one cell joining two groups
    rows2 = np.zeros((2, G), np.float32)
    rows2[0, [10, 11]] = HIT; rows2[1, [11, 12]] = HIT                      # latent 0: 1010, 1011; latent 1: 1011, 1012; column 11 joins them
    plant(m, rows2)
    assert check(m, rows2, glob, "joined", modes=(ANY,))["n_groups"] == 1
    lab2 = np.zeros(G, U64); lab2[11] = U64(1)
    h2 = m.labels_create(lab2)
    mk2 = np.array([[0, 0, 0], [0, 0, 1]], U64)                             # latent 1 may not see a column labelled 1
    got = check(m, rows2, glob, "the joining cell masked", ok=LM.label_test(lab2, mk2), labels=h2, masks=mk2, modes=(ANY,))
    assert got["n_groups"] == 2 and got["member"].tolist() == [1010, 1011, -1, 1012, -2]
    m.labels_free(hl); m.labels_free(h2)
    m.close()


# ---- 8: caps ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_caps(codebook_bytes, tiny):
    G, n_q = 200, 30
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 8)
    glob = print_rows(G)
    rows = sparse(n_q, G, rng, per_row=1.5, special=0.0)
    plant(m, rows)
    whole = LM.link(rows, THR, glob)
    ng, nm = whole["n_groups"], whole["n_members"]
    assert ng >= 4
    last = int(whole["group_off"][-1] - whole["group_off"][-2])
    for cg, cm in ((0, 0), (ng, nm), (ng - 1, nm), (ng, nm - 1), (ng + 5, nm + 5), (1, nm), (ng, int(whole["group_off"][2])), (ng, int(whole["group_off"][2]) - 1), (0, nm), (ng, 0)):
        want = LM.link(rows, THR, glob, cap_groups=cg, cap_members=cm)
        got = m.link_groups(THR, ANY, cap_groups=cg, cap_members=cm)
        same(got, want, ("caps", cg, cm))
        assert got["n_groups"] == ng and got["n_members"] == nm
    assert m.link_groups(THR, ANY, cap_groups=ng, cap_members=nm - 1)["n_listed"] == ng - 1 and last >= 2
    m.close()


# ---- 9: state, repeatability, refusals ------------------------------------------------------------------------------------------------------------------------------
def test_state_and_refusals(codebook_bytes, tiny):
    G, n_q = 65, 9
    m = tap_matcher(codebook_bytes, tiny, G)
    rng = np.random.default_rng(SEED + 9)
    glob = print_rows(G)
    rows = sparse(n_q, G, rng, per_row=3.0)
    plant(m, rows)
    before = m.rank_hits(NINF, G)
    one = check(m, rows, glob, "first call")
    two = m.link_groups(THR)
    same(two, one, "two calls are equal")
    hs = m.subjects_create(np.arange(G) // 2)
    nan = float("nan")
    rn = np.full(n_q, -1, np.int64); bad_rn = rn.copy(); bad_rn[3] = -2
    refused = [lambda: m.link_groups(nan), lambda: m.link_groups(THR, 2), lambda: m.link_groups(THR, -1), lambda: m.link_groups(THR, row_node=bad_rn),
               lambda: m.link_groups(THR, cap_groups=-1, cap_members=0), lambda: m.link_groups(THR, cap_groups=0, cap_members=-1),
               lambda: m.link_groups(THR, masks=np.zeros((n_q, 3), U64)), lambda: m.link_groups(THR, n_q=n_q + 1, row_node=np.full(n_q + 1, -1)),
               lambda: m.link_groups(THR, excl=[np.array([-4], np.int64)] + [[]] * (n_q - 1)),
               lambda: m.link_subject_groups(hs, nan), lambda: m.link_subject_groups(hs, THR, 3), lambda: m.link_subject_groups(hs, THR, row_node=bad_rn),
               lambda: m.link_subject_groups((None, 0), THR)]
    L = m.lib
    c = np.zeros(6, np.int64)
    p = [M.C.cast(c.ctypes.data + 8 * i, M.C.POINTER(M.C.c_int64)) for i in range(6)]
    for null_at in range(5):                                                # a null output: each count, and group_off
        out = [None if i == null_at else p[i] for i in range(5)]
        refused.append(lambda out=out: m._chk(L.afis_link_groups(m.ctx, None, None, None, None, n_q, None, THR, 0, 0, 0, *out, None)))
        refused.append(lambda out=out: m._chk(L.afis_link_subject_groups(m.ctx, hs[0], None, None, None, None, n_q, None, THR, 0, 0, 0, *out, None)))
    refused.append(lambda: m._chk(L.afis_link_groups(m.ctx, None, None, None, None, n_q, None, THR, 0, 1, 1, *p[:5], None)))   # member null at cap_members 1
    refused.append(lambda: m._chk(L.afis_link_subject_groups(m.ctx, None, None, None, None, None, n_q, None, THR, 0, 0, 0, *p[:5], None)))
    for i, call in enumerate(refused):
        with pytest.raises(M.AfisError, match=EINVAL):
            call()
        assert m.get_option("link_groups_us") == 0 and m.get_option("link_d2h_bytes") == 0, i   # refused before anything was queued
    assert L.afis_link_groups(None, None, None, None, None, n_q, None, THR, 0, 0, 0, *p[:5], None) == -1
    m._chk(L.afis_link_groups(m.ctx, None, None, None, None, n_q, None, THR, 0, 0, 0, *p[:5], None))   # member may be null at cap_members 0
    assert c[:4].tolist() == [one["n_edges"], one["n_groups"], one["n_members"], 0] and c[4] == 0
    after = m.rank_hits(NINF, G)
    for key in ("n_hits", "idx", "score"):
        assert np.array_equal(before[key].view(np.uint32) if key == "score" else before[key], after[key].view(np.uint32) if key == "score" else after[key]), key   # the matrix is unwritten and rankable
    same(m.link_groups(THR), one, "after the refusals")
    # a normalised matrix: min_score in z units
    z = m.normalize_scores(np.full(n_q, 2.0), np.full(n_q, 0.5), axis=0, want_scores=True)   # z = (v - 2) / 2: a 5.0 becomes 1.5, the cells in [0, 1) go negative
    check(m, z, glob, "z units", min_score=1.0)
    check(m, z, glob, "z units, negative threshold", min_score=-0.75)
    plant(m, rows)
    m.gallery_remove([BASE + 7])                                            # an edit: the matrix and the handle are the old shard's
    with pytest.raises(M.AfisError, match=ESTATE):
        m.link_groups(THR)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.link_subject_groups(hs, THR)
    m.subjects_free(hs)
    m.close()


# ---- 10: two ranks ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_merge(codebook_bytes, tiny):
    G, n_q, cut = 2 * CHUNK_SCALAR + 1, STRIP + 1, CHUNK_SCALAR + 1
    rng = np.random.default_rng(SEED + 10)
    rows = sparse(n_q, G, rng, per_row=2.0)
    rows[0, 5] = rows[0, G - 3] = HIT                                       # a group that exists only through latent 0
    one = tap_matcher(codebook_bytes, tiny, G)
    plant(one, rows)
    whole = check(one, rows, print_rows(G), "whole", modes=(ANY,))
    one.close()
    per = []
    for lo, hi in ((0, cut), (cut, G)):
        h = tap_matcher(codebook_bytes, tiny, hi - lo, lo, BASE + lo)
        plant(h, np.ascontiguousarray(rows[:, lo:hi]))
        per.append(h.link_groups(THR))
        h.close()
    got = SH.merge_link_groups(per)
    assert np.array_equal(got["group_off"], whole["group_off"]) and np.array_equal(got["member"], whole["member"])


# ---- 11: end to end: a print search over a gallery with duplicates ---------------------------------------------------------------------------------------------------
def test_end_to_end_duplicate_check(codebook_bytes, cb):
    n0 = 32
    gal = S.make_packed_gallery(SEED, n0, cb)
    twice, thrice = (2, 5, 11, 17, 23, 30), 8                               # six prints enrolled twice, one three times: 40 prints
    copies = list(twice) + [thrice, thrice]
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(gal)
    for g in copies:
        m.gallery_add_packed(gal.slice(g, g + 1))
    m.gallery_commit(BASE)
    G = n0 + len(copies)
    source = np.concatenate([np.arange(n0), copies])                        # the print every enrolled template is a copy of
    planted = sorted(sorted(BASE + np.flatnonzero(source == g)) for g in set(copies))
    rng = np.random.default_rng(SEED + 11)
    listed = BASE + rng.permutation(G)[:29].astype(np.int64)                # a subset listed out of order
    sub = m.subset_create(listed)
    for what, idx, cols, subset in (("the whole shard", BASE + np.arange(G, dtype=np.int64), BASE + np.arange(G, dtype=np.int64), None), ("a subset", listed, listed, sub)):
        sc = m.search_prints(idx, 1.0, 1.0, subset=subset)["scores"]        # columns in the caller's order
        excl = [np.array([t], np.int64) for t in idx]                       # each print's own column is out
        ok = LM.not_excluded(cols, excl, len(idx))
        dup = (source[idx - BASE][:, None] == source[cols - BASE][None, :]) & ok
        other = ~(source[idx - BASE][:, None] == source[cols - BASE][None, :])
        key = LM.key_of(sc).astype(np.int64)
        assert dup.any() and key[dup].min() > key[other].max()              # copies score above every pair of different prints
        thr = float(sc[dup][np.argmin(key[dup])])                           # the weakest planted cell: every duplicate links, and the best non-duplicate pair is just below
        below = float(sc[other][np.argmax(key[other])])                     # ... and at that score a pair of different prints links too
        for min_score in (thr, below):
            for mode in (ANY, MUTUAL):
                want = LM.link(sc, min_score, cols, idx, mode, ok)
                got = m.link_groups(min_score, mode, row_node=idx, excl=excl)
                same(got, want, (what, min_score, mode))
        got = m.link_groups(thr, MUTUAL, row_node=idx, excl=excl)
        groups = [got["member"][a:b].tolist() for a, b in zip(got["group_off"][:-1], got["group_off"][1:])]
        if subset is None:
            assert groups == planted and got["n_edges"] == 6 * 2 + 6         # six pairs and one triple, every cell confirmed
        assert m.link_groups(below, ANY, row_node=idx, excl=excl)["n_edges"] > m.link_groups(thr, ANY, row_node=idx, excl=excl)["n_edges"]
    he = m.subset_create([])                                                # a search that covered no column: counts of zero, nothing queued
    m.search_subset(he, S.make_latents(SEED, 2), k=0, want_scores=False)
    none = m.link_groups(0.0)
    assert (none["n_edges"], none["n_groups"], none["n_members"], none["n_listed"]) == (0, 0, 0, 0) and none["group_off"].tolist() == [0] and len(none["member"]) == 0
    assert m.get_option("link_groups_us") == 0 and m.get_option("link_d2h_bytes") == 0
    m.subset_free(he)
    m.subset_free(sub)
    m.close()
