"""Weighted search without a GPU: afis_search_weighted is declared, exported by both libraries and bound by the Python host, its kernel and its driver are product
objects, its three options are documented and the header carries the contract; the numpy model of the plan (active lists, packing, pseudo-query count) is held
against a brute-force loop, the model of the fold against a cell-by-cell Python-float loop — including a cell an fp32 accumulator gets wrong —; per-shard matrices
ranked by the list model of tests/test_eligible_host.py and merged with merge_hits equal the one-shard model.  (What the device computes is
tests/test_gpu_weighted_search.py's.)"""
import importlib
import os
import re

import numpy as np
import pytest

import weighted_model as W
from test_eligible_host import template_hits

M = importlib.import_module("msu-latentafis_amd.host.matcher")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = {"weighted_batch_pseudo": "settable", "weighted_pseudo_queries": "read-only", "weighted_fold_us": "read-only"}


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+afis_search_weighted\s*\(afis_ctx\*\s*ctx,\s*const afis_template_view\*\s*queries,\s*int n_q,\s*const float\*\s*w_minu\s*,\s*int n_wm,\s*"
                     r"const float\*\s*w_tex\s*,\s*int n_wt,\s*float\*\s*scores\s*,\s*int32_t\*\s*status\s*\)", code)
    taps = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+afis_debug_fold_templates\s*\(afis_ctx\*", taps)
    product, test = M.load_library(), M.load_library(M.TEST_LIB_PATH)       # dlopen only: no device call
    for lib in (product, test):
        assert hasattr(lib, "afis_search_weighted") and lib.afis_search_weighted.argtypes is not None
    assert "afis_search_weighted" in M.EXPORTS and "afis_debug_fold_templates" in M.TAP_EXPORTS
    assert hasattr(test, "afis_debug_fold_templates") and not hasattr(product, "afis_debug_fold_templates")
    for method in ("search_weighted", "debug_fold_templates"):
        assert hasattr(M.Matcher, method), method
    option_text = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt, kind in OPTIONS.items():
        assert re.search(r'"%s" \(%s' % (opt, kind), option_text), opt
        assert "`%s`" % opt in integration, opt
    contract = hdr[hdr.index("Weighted search (no reference counterpart"):hdr.index("int afis_search_weighted")]
    for phrase in ("ACTIVE", "post-strip", "double acc = +0.0", "bit for bit", "exact in fp64", "contracts the multiply-add", "AFIS_QUERY_LATENT_EMPTY",
                   "finite and >= 0", "-0.0f is a zero", "does NOT give afis_search's", "a full search's in every respect", "afis_rank_subjects",
                   "Not in this interface", "a subset form", "a resident query-handle form", "afis_rank_hits(-INFINITY, cap)", "the match CLI",
                   "pairs = pseudo-queries x G", "merge_hits", "weighted_batch_pseudo", "profiles/weighted_search_timing.json"):
        assert phrase in contract, phrase


def test_the_kernel_and_the_driver_are_product_objects():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "template_fold.o" in objs and "afis_weighted.o" in objs
    assert re.search(r"^TEST_OBJS\s*=\s*\$\(OBJS\)", mk, flags=re.M)          # the test library is the product objects plus the taps
    assert re.search(r"^template_fold\.o:\s*template_fold\.hip", mk, flags=re.M) and re.search(r"^afis_weighted\.o:\s*afis_weighted\.cpp", mk, flags=re.M)
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "template_fold.hip")).read()
    body = src.split("namespace afis {", 1)[1]                                # the code, without the header comment
    assert "__global__" in src and "k_fold_templates" in src and "grid_clamp" in src and "size_t" in body and "double acc" in body and "float4" in body
    assert "atomic" not in body and "__shfl" not in src and "__shared__" not in src and "hipMemset" not in src


# ---- the plan --------------------------------------------------------------------------------------------------------------------------------------
def brute_plan(counts, w_minu, w_tex):
    """Template by template: the active ones of a query fill slot after slot; a pseudo-query is opened when a list needs one more."""
    qd, spec, wtab = [], [], []
    for q, (n_minu, n_tex) in enumerate(counts):
        first = len(spec); slot = 0; n_at = 0
        for i in range(max(n_minu, 0)):
            if i < w_minu.shape[1] and float(w_minu[q, i]) != 0.0:
                if slot % 3 == 0:
                    spec.append([-1, -1, -1, -1]); wtab.append([0.0, 0.0, 0.0, 0.0])
                spec[first + slot // 3][slot % 3] = i; wtab[first + slot // 3][slot % 3] = float(w_minu[q, i]); slot += 1
        for t in range(max(n_tex, 0)):
            if t < w_tex.shape[1] and float(w_tex[q, t]) != 0.0:
                if first + n_at == len(spec):
                    spec.append([-1, -1, -1, -1]); wtab.append([0.0, 0.0, 0.0, 0.0])
                spec[first + n_at][3] = t; wtab[first + n_at][3] = float(w_tex[q, t]); n_at += 1
        n_pq = len(spec) - first
        qd.append((first, n_pq, n_at, 0 if n_pq else W.LATENT_EMPTY))
    return np.array(qd, np.int32).reshape(-1, 4), np.array(spec, np.int32).reshape(-1, 4), np.array(wtab, np.float32).reshape(-1, 4)


def random_weights(rng, n_q, n_w):
    w = rng.random((n_q, n_w)).astype(np.float32)
    u = rng.random((n_q, n_w))
    w[u < 0.35] = 0.0
    w[(u >= 0.35) & (u < 0.45)] = -0.0
    return w


@pytest.mark.parametrize("n_wm, n_wt", [(0, 0), (1, 0), (0, 1), (3, 1), (12, 2), (28, 1), (40, 5)])
def test_the_plan_against_a_template_loop(n_wm, n_wt):
    rng = np.random.default_rng(11 + 7 * n_wm + n_wt)
    for trial in range(4):
        n_q = 9
        counts = [(int(rng.integers(0, 33)), int(rng.integers(0, 4))) for _ in range(n_q)]
        counts[2] = (0, 0); counts[5] = (28, 1); counts[7] = (0, 3)          # queries with 0 templates, the reference's layout, texture only
        wm, wt = random_weights(rng, n_q, n_wm), random_weights(rng, n_q, n_wt)
        if trial == 3:
            wm[:] = 1.0; wt[:] = 0.3                                        # everything active: afis_match_all_templates' packing
        got, want = W.plan(counts, wm, wt), brute_plan(counts, wm, wt)
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        qd, spec, wtab = got
        for q, (n_minu, n_tex) in enumerate(counts):
            am = [i for i in range(min(n_minu, n_wm)) if wm[q, i] != 0]; at = [t for t in range(min(n_tex, n_wt)) if wt[q, t] != 0]
            assert qd[q, 1] == max(-(-len(am) // 3), len(at)) and qd[q, 2] == len(at) and (qd[q, 3] == W.LATENT_EMPTY) == (not am and not at)
            rows = spec[qd[q, 0]:qd[q, 0] + qd[q, 1]]
            assert [int(x) for x in rows[:, :3].reshape(-1) if x >= 0] == am and [int(x) for x in rows[:, 3] if x >= 0] == at      # ascending, none lost
            assert ((wtab[qd[q, 0]:qd[q, 0] + qd[q, 1]] != 0) == (rows >= 0)).all()                # a weight exactly where a template stands
        if trial == 3:
            assert all(qd[q, 1] == max(-(-min(c[0], n_wm) // 3), min(c[1], n_wt)) for q, c in enumerate(counts))
        assert qd[2, 3] == W.LATENT_EMPTY and qd[2, 1] == 0
        assert int(qd[-1, 0] + qd[-1, 1]) == len(spec)
        for cap in (1, 3, 1000):                                            # batches: query boundaries, the cap, nothing lost
            bs = W.batches(qd, cap)
            assert bs[0][0] == 0 and bs[-1][1] == n_q and all(a[1] == b[0] for a, b in zip(bs, bs[1:]))
            for q0, q1 in bs:
                n = int(qd[q0:q1, 1].sum())
                assert n <= cap or int((qd[q0:q1, 1] > 0).sum()) == 1
        assert len(W.batches(qd, 1 << 30)) == 1


def test_the_plan_on_a_hand_made_case():
    counts = [(5, 1), (2, 2), (4, 0)]
    wm = np.array([[1, 0, 2, -0.0, 3, 9, 9], [0.5, 0.5, 9, 9, 9, 9, 9], [0, 0, 0, 0, 0, 0, 0]], np.float32)     # a row longer than the templates; a row of zeros
    wt = np.array([[0.3], [1.0], [1.0]], np.float32)                          # a row shorter than query 1's two texture templates
    qd, spec, wtab = W.plan(counts, wm, wt)
    assert qd.tolist() == [[0, 1, 1, 0], [1, 1, 1, 0], [2, 0, 0, 1]]
    assert spec.tolist() == [[0, 2, 4, 0], [0, 1, -1, 0]]
    assert wtab.tolist() == [[1.0, 2.0, 3.0, np.float32(0.3)], [0.5, 0.5, 0.0, 1.0]]


# ---- the fold --------------------------------------------------------------------------------------------------------------------------------------
def loop_fold(parts, qd, wtab, empty):
    """Cell by cell in Python floats (IEEE doubles), in the order the header states."""
    G = len(empty)
    out = np.empty((len(qd), G), np.float32)
    for q, (first, n_pq, n_at, status) in enumerate(qd.tolist()):
        for g in range(G):
            if status or empty[g]:
                out[q, g] = -1.0
                continue
            acc = 0.0
            for j in range(n_pq):
                for s in range(3):
                    if float(wtab[first + j, s]) != 0.0:
                        acc = acc + float(wtab[first + j, s]) * float(parts[first + j, g, s])
            for j in range(n_at):
                if float(wtab[first + j, 3]) != 0.0:
                    acc = acc + float(wtab[first + j, 3]) * float(parts[first + j, g, 3])
            with np.errstate(over="ignore"):
                out[q, g] = np.float32(acc)
    return out


def test_the_fold_against_a_cell_loop():
    rng = np.random.default_rng(2024)
    for G in (1, 5, 33):
        counts = [(int(rng.integers(0, 30)), int(rng.integers(0, 3))) for _ in range(6)]
        wm, wt = random_weights(rng, 6, 28), random_weights(rng, 6, 2)
        wm[1, :3] = 1e-30; wt[3] = 1e30
        qd, spec, wtab = W.plan(counts, wm, wt)
        parts = (rng.random((len(spec), G, 4)) * 40).astype(np.float32)
        parts[rng.random(parts.shape) < 0.3] = 0.0
        parts[rng.random(parts.shape) < 0.05] = 1e30
        parts[np.broadcast_to((spec < 0)[:, None, :], parts.shape)] = np.nan  # an unused slot may hold anything
        empty = (rng.random(G) < 0.2).astype(np.uint8)
        got, want = W.fold(parts, qd, wtab, empty), loop_fold(parts, qd, wtab, empty)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert not np.isnan(got).any() and ((got == -1) | (got >= 0)).all()


def test_the_cell_an_fp32_accumulator_gets_wrong():
    """weights 1, values 2^24, 1, 1, 1: fp32 adds stay at 16777216, the fp64 sum 16777219 converts to 16777220."""
    qd = np.array([[0, 2, 0, 0]], np.int32)
    wtab = np.array([[1, 1, 1, 0], [1, 0, 0, 0]], np.float32)
    parts = np.zeros((2, 1, 4), np.float32); parts[0, 0, :3] = (2.0 ** 24, 1, 1); parts[1, 0, 0] = 1
    f32 = np.float32(0)
    for v in (2.0 ** 24, 1, 1, 1):
        f32 = np.float32(f32 + np.float32(v))
    assert float(f32) == 16777216.0
    assert float(W.fold(parts, qd, wtab, [0])[0, 0]) == 16777220.0 == float(loop_fold(parts, qd, wtab, [0])[0, 0])
    vec = np.array([[2.0 ** 24, 1, 1, 1]], np.float32)
    row, status = W.fold_vectors(vec, 4, np.ones(4, np.float32), np.zeros(0, np.float32), [0])
    assert float(row[0]) == 16777220.0 and status == 0


def test_fold_vectors_is_the_fold_of_the_packed_parts():
    """The definition on all-templates vectors equals the fold of the packed per-part scores: the packing changes no bit."""
    rng = np.random.default_rng(5)
    G, counts = 17, [(28, 1), (7, 2), (4, 0), (0, 0), (4, 0)]
    wm, wt = random_weights(rng, 5, 30), random_weights(rng, 5, 3)
    wm[4, :4] = 0                                                           # only templates the latent does not have
    qd, spec, wtab = W.plan(counts, wm, wt)
    vecs = [(rng.random((G, a + b)) * 30).astype(np.float32) for a, b in counts]
    parts = np.zeros((len(spec), G, 4), np.float32)
    for q, (a, b) in enumerate(counts):
        for j in range(qd[q, 1]):
            for s in range(4):
                t = spec[qd[q, 0] + j, s]
                if t >= 0:
                    parts[qd[q, 0] + j, :, s] = vecs[q][:, t if s < 3 else a + t]
    empty = np.zeros(G, np.uint8); empty[3] = 1
    got = W.fold(parts, qd, wtab, empty)
    for q, (a, b) in enumerate(counts):
        row, status = W.fold_vectors(vecs[q], a, wm[q], wt[q], empty)
        assert status == qd[q, 3] and np.array_equal(row.view(np.uint32), got[q].view(np.uint32))
    assert qd[3, 3] == W.LATENT_EMPTY and qd[4, 3] == W.LATENT_EMPTY and (got[3:] == -1).all()


# ---- shards ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_per_shard_weighted_matrices_merge_into_the_one_shard_model(world):
    """The columns of shards are disjoint and the weights common: the lists read from each rank's matrix are merge_hits input as they are."""
    rng = np.random.default_rng(31 + world)
    G, base, cap = 300, 7000, 16
    counts = [(28, 1), (7, 2), (0, 0), (12, 0)]
    wm, wt = random_weights(rng, 4, 28), random_weights(rng, 4, 2)
    qd, spec, wtab = W.plan(counts, wm, wt)
    parts = (np.round(rng.random((len(spec), G, 4)) * 4) / 2).astype(np.float32)      # a few values: the tie rules decide many places
    parts[rng.random(parts.shape) < 0.6] = 0.0
    empty = (rng.random(G) < 0.1).astype(np.uint8)
    glob = np.arange(G, dtype=np.int64) + base
    whole = W.fold(parts, qd, wtab, empty)
    entry = np.ones(whole.shape, bool)
    for trial in range(3):
        cuts = np.sort(rng.integers(0, G + 1, world - 1)) if trial else np.array([100, 100][:world - 1])
        bounds = list(zip(np.r_[0, cuts], np.r_[cuts, G]))
        shards = [W.fold(parts[:, lo:hi], qd, wtab, empty[lo:hi]) for lo, hi in bounds]
        assert np.array_equal(np.concatenate(shards, axis=1).view(np.uint32), whole.view(np.uint32))
        for thr in (-np.inf, float(np.nextafter(np.float32(0), np.float32(1))), 3.0):
            per = [template_hits(s, glob[lo:hi], entry[:, lo:hi], thr, cap) for s, (lo, hi) in zip(shards, bounds)]
            n, i, s = SH.merge_hits(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), cap)
            wn, wi, ws = template_hits(whole, glob, entry, thr, cap)
            assert np.array_equal(n, wn) and np.array_equal(i, wi) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), (trial, thr)
        assert wn.sum() > 0
