"""The list kernels' slabs (graph.hip::dist_filter): S8's power iterations keep the first `capacity` neighbour values of every row in global memory and recompute what
lies beyond.  The ordinary test inputs have rows of 10-25 neighbours and never leave the slab route; these inputs are built so that rows end below, AT, one above and far above the
capacity, for minutiae and for texture lists, on the packed and on the generic arithmetic paths.

How: the compatibility matrix H has no one-to-one rule (oracle/afis_oracle.cpp, dist_filter): two list entries are neighbours whenever the distance between their latent points
and the distance between their rolled points differ by less than 30.  Latent minutiae inside a square of side 20 (diagonal 28.3) against rolled minutiae inside such a square give
lists whose entries are ALL neighbours of each other; latent points far from that cluster and from each other (>= 90 px) give entries that are neighbours of nothing but the
entries that share their latent point.  With c clustered latent points and a rolled template of r (<= 3) clustered minutiae, c * r <= 120, the clustered entries have c * r - 1
neighbours.  Texture lists the same way in block units (a one-block span is 22.6 < 30; far rows are >= 4 blocks apart: 64 - 22.6 > 30).

Every check is against the oracle, bit for bit; the row degrees of every list are computed here, on the host, from the oracle's stage-0 list and the coordinates, and the tests
assert that they land on both sides of the capacities the library reports — they cannot pass by never leaving the slab route, or by never entering it."""
import importlib
import os
import re

import numpy as np
import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SELECTED = (26, 2, 11)                      # the latent minutiae templates a search uses (matcher.cpp:380), = which 1, 2, 3 of the stage taps


def header_capacities():
    """(texture, minutiae) steps per row the slabs hold, as the device header states them (the GPU tests check that afis_get_option reports the same)."""
    with open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "afis_device.h")) as f:
        m = re.search(r"constexpr int kTexSlabSteps = (\d+), kMinuSlabSteps = (\d+);", f.read())
    return int(m.group(1)), int(m.group(2))


def _unit(rng, n):
    d = rng.standard_normal((n, 96)).astype(np.float32)
    return (d * (np.float32(T.DESCRIPTOR_NORM) / np.linalg.norm(d, axis=1, keepdims=True))).astype(np.float32)


def _minutiae(rng, n_cluster, n_far, shift=0, corner=(300, 300)):
    """n_cluster points inside a 20 x 20 square at `corner`, n_far points on a 90-px grid away from it; every coordinate moved by `shift` (beyond 2047: the generic arithmetic)."""
    cx = rng.integers(0, 21, n_cluster) + corner[0]; cy = rng.integers(0, 21, n_cluster) + corner[1]
    grid = [(gx, gy) for gx in range(30, 760, 90) for gy in range(30, 790, 90) if abs(gx - corner[0] - 10) > 80 or abs(gy - corner[1] - 10) > 80]
    assert n_far <= len(grid)
    pick = rng.permutation(len(grid))[:n_far]
    fx = np.array([grid[i][0] for i in pick], np.int64); fy = np.array([grid[i][1] for i in pick], np.int64)
    x = np.concatenate([cx, fx]) + shift; y = np.concatenate([cy, fy]) + shift
    order = rng.permutation(len(x))                                   # clustered and far points interleaved
    n = len(x)
    return T.MinutiaeTemplate(x[order].astype(np.int16), y[order].astype(np.int16), rng.uniform(-np.pi, np.pi, n).astype(np.float32), _unit(rng, n))


def _tex_points(rng, n_cluster, n_far, shift=0, corner=(20, 20)):
    """Block coordinates: n_cluster points spanning one block in x and y at `corner` (coordinates repeat), n_far points on a 4-block grid away from it."""
    cx = rng.integers(0, 2, n_cluster) + corner[0]; cy = rng.integers(0, 2, n_cluster) + corner[1]
    grid = [(gx, gy) for gx in range(0, 45, 4) for gy in range(0, 47, 4) if abs(gx - corner[0]) > 4 or abs(gy - corner[1]) > 4]
    assert n_far <= len(grid)
    pick = rng.permutation(len(grid))[:n_far]
    fx = np.array([grid[i][0] for i in pick], np.int64); fy = np.array([grid[i][1] for i in pick], np.int64)
    x = np.concatenate([cx, fx]) + shift; y = np.concatenate([cy, fy]) + shift
    order = rng.permutation(len(x))
    return x[order].astype(np.int16), y[order].astype(np.int16)


def _latent(rng, minu3, tex, shift_m=0, shift_t=0):
    """minu3: (clustered, far) for the selected templates 26, 2, 11; tex: (clustered, far) rows of the texture template."""
    t = T.FPTemplate()
    spec = dict(zip(SELECTED, minu3))
    for i in range(28):
        c, f = spec.get(i, (2, 0))
        t.minu.append(_minutiae(rng, c, f, shift_m))
    x, y = _tex_points(rng, tex[0], tex[1], shift_t)
    t.tex.append(T.TextureTemplate(x, y, rng.uniform(-np.pi / 2, np.pi / 2, len(x)).astype(np.float32), des=_unit(rng, len(x))))
    return t


def _rolled(rng, cb, n_minu, n_tex, one_point=False):
    """n_minu clustered minutiae; n_tex texture points spanning one block (or all at one coordinate)."""
    t = T.FPTemplate()
    t.minu.append(_minutiae(rng, n_minu, 0, corner=(420, 380)))
    x, y = _tex_points(rng, n_tex, 0, corner=(30, 12))
    if one_point:
        x[:] = 30; y[:] = 12
    t.tex.append(T.TextureTemplate(x, y, rng.uniform(-np.pi / 2, np.pi / 2, n_tex).astype(np.float32), codes=rng.integers(0, cb.K, (n_tex, cb.M)).astype(np.uint8)))
    return t


def slab_set(cb, cap_t, cap_m, seed=90):
    """Latents and rolled templates whose lists have longest rows of capacity - 1, capacity, capacity + 1 and far more (up to 119 / 199 neighbours)."""
    rng = np.random.default_rng(seed)
    edge = ((cap_m, 20), (cap_m + 1, 20), (cap_m + 2, 20))            # against a rolled template of ONE minutia: longest rows cap_m - 1, cap_m, cap_m + 1
    full = ((120, 0), (119, 1), (60, 60))
    lats = [_latent(rng, edge, (cap_t, 100)),                          # texture: longest row cap_t - 1
            _latent(rng, full, (cap_t + 1, 100)),                      # cap_t
            _latent(rng, edge, (cap_t + 2, 100), shift_m=2100),        # cap_t + 1; minutiae beyond 2047: the generic arithmetic
            _latent(rng, full, (200, 0), shift_m=2100),                # 199
            _latent(rng, edge, (230, 30), shift_t=60),                 # more than 200 rows: S7 picks the list; block coordinates beyond 49: the |d| < 50 test
            _latent(rng, full, (150, 50), shift_t=2100)]               # block coordinates beyond 2047: the generic arithmetic
    gal = [_rolled(rng, cb, 1, 300), _rolled(rng, cb, 2, 640, one_point=True), _rolled(rng, cb, 3, 1000), S.make_rolled(rng, cb, n_tex=400)]
    return lats, gal


def row_degrees(lx, ly, rx, ry, texture):
    """Neighbours per list entry as graph.hip counts them: in range (texture: every |d| < 50) and |d1 - d2| < 30 in the reference's float arithmetic."""
    lx, ly, rx, ry = (np.asarray(v, np.int64) for v in (lx, ly, rx, ry))
    dx1 = lx[:, None] - lx[None, :]; dy1 = ly[:, None] - ly[None, :]; dx2 = rx[:, None] - rx[None, :]; dy2 = ry[:, None] - ry[None, :]
    d1 = np.sqrt((dx1 * dx1 + dy1 * dy1).astype(np.float32)); d2 = np.sqrt((dx2 * dx2 + dy2 * dy2).astype(np.float32))
    if texture:
        ok = (np.abs(dx1) < 50) & (np.abs(dy1) < 50) & (np.abs(dx2) < 50) & (np.abs(dy2) < 50)
        near = np.float32(16.0) * np.abs(d1 - d2) < np.float32(30.0)
    else:
        ok = np.ones(d1.shape, bool)
        near = np.abs(d1 - d2) < np.float32(30.0)
    h = ok & near
    np.fill_diagonal(h, False)
    return h.sum(axis=1)


def list_degrees(L, R, which, li, ri):
    if which == 0:
        a, b = L.tex[0], R.tex[0]
    else:
        a, b = L.minu[SELECTED[which - 1]], R.minu[0]
    return row_degrees(a.x[li], a.y[li], b.x[ri], b.y[ri], which == 0)


def longest_rows(oracle, ocb, lats, gal, hl, hr, tie_mode=1):
    """{(qi, gi, which): longest row} over every list the oracle builds, and how many lists keep survivors after S8."""
    out = {}; n_surv = 0
    for qi, L in enumerate(lats):
        for gi, R in enumerate(gal):
            for which in range(4):
                tr = oracle.trace(ocb, hl[qi], hr[gi], which=which, stage=0, tie_mode=tie_mode)
                if tr is None or len(tr[1]) == 0:
                    continue
                out[(qi, gi, which)] = int(list_degrees(L, R, which, tr[1], tr[2]).max())
                s8 = oracle.trace(ocb, hl[qi], hr[gi], which=which, stage=1, tie_mode=tie_mode)
                n_surv += int(s8 is not None and len(s8[1]) > 1)
    return out, n_surv


def assert_both_sides(longest, cap_t, cap_m):
    tex = {v for (q, g, w), v in longest.items() if w == 0}; minu = {v for (q, g, w), v in longest.items() if w > 0}
    for have, cap, top in ((tex, cap_t, 199), (minu, cap_m, 119)):
        assert {cap - 1, cap, cap + 1} <= have, (cap, sorted(have))            # rows that end one below, at and one above the capacity
        assert top in have and any(v >= 2 * cap for v in have), (cap, sorted(have))   # rows far beyond it
        assert any(v < cap - 1 for v in have), (cap, sorted(have))              # and lists that never reach it


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def slab_case(cb, codebook_bytes, oracle):
    cap_t, cap_m = header_capacities()
    lats, gal = slab_set(cb, cap_t, cap_m)
    ocb = oracle.codebook(codebook_bytes)
    hl, hr = cases.to_orc(oracle, ocb, lats, gal)
    return cap_t, cap_m, lats, gal, ocb, hl, hr


def test_the_inputs_reach_both_sides_of_the_capacity(slab_case, oracle):
    """The rehearsal on the CPU: the oracle's lists on these inputs have longest rows below, at, above and far above both capacities, and S8 leaves survivors to compare."""
    cap_t, cap_m, lats, gal, ocb, hl, hr = slab_case
    assert 8 <= cap_m < 100 and 8 <= cap_t < 180
    for tie_mode in (1, 9):
        longest, n_surv = longest_rows(oracle, ocb, lats, gal, hl, hr, tie_mode)
        assert_both_sides(longest, cap_t, cap_m)
        assert n_surv >= 20, n_surv
    for qi in range(len(lats)):
        rc, sc, parts = oracle.search(ocb, hl[qi], hr, tie_mode=1, want_parts=True)
        assert rc == 0 and np.isfinite(parts).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ref_tie", [0, 2])
def test_lists_beyond_the_slab_match_the_oracle(codebook_bytes, slab_case, oracle, ref_tie):
    """Stage traces (candidates, after S8, after S9) of every list and the per-part and fused scores, bit for bit, with the kernels back to back and in the default schedule,
    in the ascending-index tie order and in std::sort's."""
    cap_t, cap_m, lats, gal, ocb, hl, hr = slab_case
    tie_mode = 9 if ref_tie == 2 else 1
    m = M.Matcher(codebook_bytes, taps=True)
    assert m.get_option("graph_slab_steps_texture") == cap_t and m.get_option("graph_slab_steps_minutiae") == cap_m
    m.gallery_add(gal); m.gallery_commit(0)
    m.set_option("ref_tie_order", ref_tie)
    longest, _ = longest_rows(oracle, ocb, lats, gal, hl, hr, tie_mode)
    assert_both_sides(longest, cap_t, cap_m)
    default_cus = m.get_option("bound_cus")
    for bc in (0, default_cus):
        m.set_option("bound_cus", bc)
        n_lists = 0
        for (qi, gi, which) in sorted(longest):
            for stage in range(3):
                want = oracle.trace(ocb, hl[qi], hr[gi], which=which, stage=stage, tie_mode=tie_mode)
                got = m.debug_stage_list(lats[qi], gi, which, stage)
                assert want is not None and got is not None, (bc, qi, gi, which, stage)
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (bc, qi, gi, which, stage, longest[(qi, gi, which)])
                assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (bc, qi, gi, which, stage)
                n_lists += 1
        assert n_lists == 3 * len(longest) and len(longest) >= 4 * len(lats) * 3
        res = m.search(lats, k=0, want_parts=True)
        for qi in range(len(lats)):
            rc, sc, parts = oracle.search(ocb, hl[qi], hr, tie_mode=tie_mode, want_parts=True)
            got = np.concatenate([res["parts"][qi], res["scores"][qi][:, None]], axis=1)
            diff = got.view(np.uint32) != parts.astype(np.float32).view(np.uint32)
            assert rc == 0 and not diff.any(), (bc, qi, np.argwhere(diff)[:4], got[diff][:4], parts[diff][:4])
    m.close()


def _packed(templates):
    mo = np.cumsum([0] + [t.minu[0].n for t in templates]).astype(np.int64); to = np.cumsum([0] + [t.tex[0].n for t in templates]).astype(np.int64)
    cat = lambda f: np.concatenate([f(t) for t in templates])
    return S.PackedGallery(mo, cat(lambda t: t.minu[0].x), cat(lambda t: t.minu[0].y), cat(lambda t: t.minu[0].ori), cat(lambda t: t.minu[0].des),
                           to, cat(lambda t: t.tex[0].x), cat(lambda t: t.tex[0].y), cat(lambda t: t.tex[0].ori), cat(lambda t: t.tex[0].codes))


@pytest.mark.gpu
def test_lists_beyond_the_slab_in_the_overlapped_schedule(codebook_bytes, cb, slab_case, oracle):
    """The default schedule runs two instances of the minutiae list kernel at once (side stream + the context's stream) on disjoint slabs, from launches of 2^16 pairs on: the
    same latents among ordinary ones against 3000 ordinary templates + the clustered ones.  Overlapped and back to back give the same bits everywhere, and the oracle's on the
    clustered templates, in both tie orders."""
    cap_t, cap_m, lats, gal, ocb, hl, hr = slab_case
    G0 = 3000
    base = S.make_packed_gallery(78, G0, cb)
    big = _packed([base.template(g) for g in range(G0)] + list(gal))
    many = []
    n_plain = 14                                                         # ordinary latents keep the group's minutiae stage light enough for the overlapped schedule (afis_search.cpp: overlap_cell_ratio)
    for r in range(2):
        many += list(lats) + S.make_latents(500 + r, n_plain)
    assert len(many) * big.G >= 65536
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(big); m.gallery_commit(0)
    default_cus = m.get_option("bound_cus")
    assert default_cus > 0
    for ref_tie, tie_mode in ((0, 1), (2, 9)):
        m.set_option("ref_tie_order", ref_tie)
        want = None
        for bc in (default_cus, 0):
            m.set_option("bound_cus", bc)
            got = m.search(many, k=24, want_parts=True)
            assert (m.timing()["overlapped_groups"] > 0) == (bc > 0), (bc, m.timing())
            if want is None: want = got
            for key in ("scores", "parts", "topk_idx", "topk_score"):
                assert np.array_equal(np.asarray(got[key]).view(np.uint8), np.asarray(want[key]).view(np.uint8)), (ref_tie, bc, key)
        for qi in range(len(lats)):
            rc, sc, parts = oracle.search(ocb, hl[qi], hr, tie_mode=tie_mode, want_parts=True)
            for copy in range(2):
                row = copy * (len(lats) + n_plain) + qi
                got = np.concatenate([want["parts"][row][G0:], want["scores"][row][G0:, None]], axis=1)
                assert np.array_equal(got.view(np.uint32), parts.astype(np.float32).view(np.uint32)), (ref_tie, qi, copy)
    m.close()
