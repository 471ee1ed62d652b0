"""Subset search on the GPU: afis_subset_create / afis_subset_free / afis_search_subset / afis_search_subset_resident.

A score depends only on its (latent, rolled) pair, so the yardstick of every comparison is the FULL search of the same context: scores, parts and status of a subset
search must be, bit for bit (np.array_equal on the raw words), the listed columns of the full search, in the order the caller listed them, and the rank lists must be a
host-side sort of those columns — score descending, global index ascending — padded with (-1, -inf).  The planted mates are also held against the oracle.  After an
edit the yardstick is a context freshly committed with the edited gallery.

Small cases use 600 templates cut from synth.make_packed_gallery and a hand-sized gallery of 44 templates whose ranges are the shapes a gather can get wrong; one case
uses 12 000 templates (the overlapped schedule starts at 65 536 pairs) and one 10 000 (what crosses PCIe).
"""
import ctypes as C
import importlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 2209
ESTATE, EINVAL = "afis error -3", "afis error -1"
MINUS1 = np.float32(-1).view(np.uint32)


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def lats():
    return S.make_latents(SEED, 3, n_tex_lo=300, n_tex_hi=520)


@pytest.fixture(scope="module")
def pool(cb, lats):
    """600 templates of one synthetic gallery as FPTemplate objects; entries 310 + 20 q + {0, 1, 2} and 40 + 7 q carry mates of latent q (as tests/test_gpu_live_gallery.py)."""
    pg = S.make_packed_gallery(SEED, 600, cb, n_tex_lo=300, n_tex_hi=520)
    ts = [pg.template(g) for g in range(600)]
    rng = np.random.default_rng(SEED + 1)
    for q, L in enumerate(lats):
        for j, frac in enumerate((0.8, 0.5, 0.3)):
            g = 310 + 20 * q + j
            ts[g] = S.make_mate(rng, cb, L, frac=frac, n_minu=ts[g].minu[0].n, n_tex=ts[g].tex[0].n)
        g = 40 + 7 * q
        ts[g] = S.make_mate(rng, cb, L, frac=0.6, n_minu=ts[g].minu[0].n, n_tex=ts[g].tex[0].n)
    return ts


MATES = sorted([310 + 20 * q + j for q in range(3) for j in range(3)] + [40 + 7 * q for q in range(3)])


def fresh(cbb, ts, opts=None, index_base=0, taps=False):
    m = M.Matcher(cbb, taps=taps)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    m.gallery_add(ts)
    m.gallery_commit(index_base)
    return m


def words(r):
    return {"scores": r["scores"].view(np.uint32), "parts": r["parts"].view(np.uint32), "status": r["status"], "topk_idx": r["topk_idx"], "topk_score": r["topk_score"].view(np.uint32)}


def full_results(m, lats, k=24):
    return words(m.search(lats, k=k, want_scores=True, want_parts=True))


def subset_results(m, idx, lats, k=24):
    h = m.subset_create(idx)
    try:
        return words(m.search_subset(h, lats, k=k, want_scores=True, want_parts=True))
    finally:
        m.subset_free(h)


def columns_of(full, idx, k, base=0):
    """What a subset search of the global indices `idx` must return, from a full search's results: its columns, and their host-side sort."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    cols = idx - base
    sc = full["scores"][:, cols]; nq = sc.shape[0]
    ti = np.full((nq, k), -1, np.int64); ts = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        order = np.lexsort((idx, -sc[q].view(np.float32).astype(np.float64)))[:k]
        ti[q, :len(order)] = idx[order]; ts[q, :len(order)] = sc[q].view(np.float32)[order]
    return {"scores": sc, "parts": full["parts"][:, cols], "status": full["status"], "topk_idx": ti, "topk_score": ts.view(np.uint32)}


def assert_same(a, b, what=""):
    for key in ("scores", "parts", "status", "topk_idx", "topk_score"):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (what, key, np.argwhere(a[key] != b[key])[:6].tolist() if a[key].shape == b[key].shape else (a[key].shape, b[key].shape))


def oracle_scores(oracle, cbb, L, ts):
    ocb = oracle.codebook(cbb)
    hl, hr = cases.to_orc(oracle, ocb, [L], ts)
    rc, want = oracle.search(ocb, hl[0], hr, tie_mode=1)
    assert rc == 0
    return want.view(np.uint32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"adc_variant": 8}, {"ref_tie_order": 2}, {"bound_cus": 0}], ids=["default", "variant8", "tie2", "bound_cus0"])
def test_columns_of_the_full_search(opts, codebook_bytes, pool, lats, oracle):
    m = fresh(codebook_bytes, pool, opts)
    full = full_results(m, lats)
    rng = np.random.default_rng(SEED + 3)
    others = [g for g in rng.permutation(600).tolist() if g not in MATES][:97 - len(MATES)]
    asc = sorted(MATES + others)
    assert len(asc) == 97
    shuffled = rng.permutation(asc).tolist()
    assert shuffled != asc
    subsets = {"ascending": asc, "shuffled": shuffled, "all": list(range(600)), "one": [333], "first and last": [0, 599], "last and first": [599, 0], "empty": []}
    for name, idx in subsets.items():
        got = subset_results(m, idx, lats)
        assert got["scores"].shape == (3, len(idx)) and got["parts"].shape == (3, len(idx), 4)
        assert_same(got, columns_of(full, idx, 24), (opts, name))
        if name == "all":
            assert_same(got, full, (opts, "all 600 against the full search's own rank lists"))
        if name == "empty":
            assert (got["topk_idx"] == -1).all() and np.isneginf(got["topk_score"].view(np.float32)).all()
    got = subset_results(m, shuffled, lats, k=100)                          # k > 64: the host's rank lists; 100 > 97 pads
    assert_same(got, columns_of(full, shuffled, 100), (opts, "k = 100"))
    assert (got["topk_idx"][:, 97:] == -1).all() and (got["topk_idx"][:, :97] >= 0).all()
    if not opts:                                                            # the planted mates against the oracle (tie_mode 1 = the default order)
        got = subset_results(m, shuffled, lats)
        for q, L in enumerate(lats):
            mates = [310 + 20 * q + j for j in range(3)] + [40 + 7 * q]
            want = oracle_scores(oracle, codebook_bytes, L, [pool[g] for g in mates])
            at = [shuffled.index(g) for g in mates]
            assert np.array_equal(got["scores"][q, at], want) and (got["scores"][q, at].view(np.float32) > 0).all()
            assert int(got["topk_idx"][q, 0]) in mates
    assert m.get_option("subset_device_bytes") == 0
    m.close()


def test_lazy_streams_are_the_subsets_own(codebook_bytes, pool, lats):
    """The code streams laid out on first use (variant 8's; variant 7's, of the test library's direct kernels) are made per shard: a subset's on its own first use,
    beside the resident shard's, in either order of first use."""
    for variant, subset_first in ((7, True), (7, False), (8, True)):
        m = fresh(codebook_bytes, pool[:200], {"adc_variant": variant}, taps=True)
        idx = [199, 40, 47, 54, 0, 120, 3]
        if subset_first:
            got = subset_results(m, idx, lats)
            full = full_results(m, lats)
        else:
            full = full_results(m, lats)
            got = subset_results(m, idx, lats)
        assert_same(got, columns_of(full, idx, 24), (variant, subset_first))
        assert_same(full_results(m, lats), full)
        m.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def shaped_gallery(cb, pool):
    """44 templates whose ranges are the shapes a gather by template list can get wrong."""
    rng = np.random.default_rng(SEED + 4)
    r = lambda nm, nt: S.make_rolled(rng, cb, n_minu=nm, n_tex=nt)
    minu_only = lambda nm: T.FPTemplate(minu=list(r(nm, 1).minu), tex=[])
    tex_only = lambda nt: T.FPTemplate(minu=[], tex=list(r(1, nt).tex))
    ts = [T.FPTemplate(),                                                   # 0: neither
          r(1, 1), r(15, 31), r(16, 32), r(17, 33), r(63, 999), r(64, 1000), r(65, 1200),   # 7: 1 200 texture points are clamped to 1 000
          r(200, 64), r(2000, 500),                                         # 9: the any-shape candidate kernel; its descriptors span 32 gather workgroups
          minu_only(40), tex_only(700), T.FPTemplate(),                     # 12: neither
          r(1, 1), r(1, 1), r(1, 1), r(1, 1), r(1, 1), r(1, 1), r(1, 1), r(1, 1),   # 13-20: a run of 1-point templates
          minu_only(1), minu_only(1), minu_only(1), tex_only(1), tex_only(1), tex_only(1),   # 21-26
          r(33, 65), pool[40], pool[47], r(77, 1000), T.FPTemplate(),       # 28, 29: mates of latents 0 and 1; 31: neither
          r(1, 1), r(1, 1), r(1, 1), r(1, 1), r(16, 16), r(48, 96), minu_only(17), tex_only(33), r(120, 640), r(1, 999), r(199, 1), pool[54]]   # 43: a mate of latent 2
    assert len(ts) == 44
    return ts


def test_range_shapes_the_gather_can_get_wrong(codebook_bytes, cb, pool, lats):
    ts = shaped_gallery(cb, pool)
    m = fresh(codebook_bytes, ts)
    full = full_results(m, lats)
    assert (full["scores"][:, [0, 12, 31]] == MINUS1).all() and (full["scores"][0, 28].view(np.float32) > 0)
    G = len(ts)
    subsets = {"every other": list(range(0, G, 2)), "the odd ones": list(range(1, G, 2)), "reverse": list(range(G - 1, -1, -1)),
               "empty entries first, in the middle and last": [0, 9, 5, 13, 14, 12, 28, 7, 43, 31],
               "the 2 000-minutiae template between 1-point ones": [20, 9, 21, 6, 24]}
    for name, idx in subsets.items():
        assert_same(subset_results(m, idx, lats), columns_of(full, idx, 24), name)
    got = subset_results(m, [0, 9, 5, 13, 14, 12, 28, 7, 43, 31], lats)
    assert (got["scores"][:, [0, 5, 9]] == MINUS1).all()
    m.close()


# ---- 3, 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(cb):
    """12 000 templates (the headline's sizes), 8 latents and a shuffled candidate list of 9 000; latents 0 and 1 have one mate inside the list (at idx[100 + q]) and one outside."""
    pg = S.make_packed_gallery(SEED + 5, 12000, cb)
    lats8 = S.make_latents(SEED + 5, 8)
    rng = np.random.default_rng(SEED + 6)
    idx = rng.permutation(12000)[:9000]
    outside = sorted(set(range(12000)) - set(idx.tolist()))
    for q, L in enumerate(lats8[:2]):
        for g in (int(idx[100 + q]), outside[q]):
            nm = int(pg.minu_off[g + 1] - pg.minu_off[g]); nt = int(pg.tex_off[g + 1] - pg.tex_off[g])
            pg.set_template(g, S.make_mate(rng, cb, L, frac=0.7, n_minu=nm, n_tex=nt))
    return pg, lats8, idx


def test_overlapped_schedule_on_a_subset(codebook_bytes, big):
    """12 000 templates, a subset of 9 000, 8 latents: 72 000 pairs, above the 65 536 at which a launch group runs on the CU-masked streams."""
    pg, lats8, idx = big
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(pg); m.gallery_commit(0)
    r = m.search(lats8, k=24, want_scores=True)
    full = {"scores": r["scores"].view(np.uint32)}
    h = m.subset_create(idx)
    qh = m.upload_queries(lats8)
    got = m.search_subset_resident(h, qh, k=24, want_scores=True)
    tm = m.timing()
    want_sc = full["scores"][:, idx]
    assert np.array_equal(got["scores"].view(np.uint32), want_sc)
    for q in range(8):
        order = np.lexsort((idx, -want_sc[q].view(np.float32).astype(np.float64)))[:24]
        assert np.array_equal(got["topk_idx"][q], idx[order]) and np.array_equal(got["topk_score"][q].view(np.uint32), want_sc[q][order])
    assert int(got["topk_idx"][0, 0]) == int(idx[100]) and int(got["topk_idx"][1, 0]) == int(idx[101])
    assert tm["pairs"] == 8 * 9000
    assert tm["overlapped_groups"] >= 1, tm
    m.free_queries(qh); m.subset_free(h)
    m.close()


def test_nothing_of_the_gallery_is_uploaded(codebook_bytes, big):
    """subset_create of 1 000 out of 10 000 templates moves at most 64 bytes per listed template from host to device: the index and offset tables, not their 50 KB of points."""
    pg = big[0]
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(pg.slice(0, 10000)); m.gallery_commit(0)
    idx = np.random.default_rng(SEED + 7).permutation(10000)[:1000]
    before = m.get_option("gallery_h2d_bytes")
    h = m.subset_create(idx)
    grown = m.get_option("gallery_h2d_bytes") - before
    held = m.get_option("subset_device_bytes")
    points = int((np.diff(pg.minu_off)[idx] * 392).sum() + (np.diff(pg.tex_off)[idx] * 24).sum())
    print(f"subset_create of 1 000 out of 10 000: {grown} bytes host-to-device (bound {64 * 1000}); the subset holds {held} device bytes, its points are {points}; "
          f"gather launches {m.get_option('subset_gather_us')} us")
    assert 0 < grown <= 64 * 1000
    assert held >= points
    m.subset_free(h)
    assert m.get_option("subset_device_bytes") == 0
    m.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_index_base(codebook_bytes, pool, lats):
    base = 1000000
    m = fresh(codebook_bytes, pool[:120], index_base=base)
    full = full_results(m, lats)
    local = [119, 40, 47, 3, 54, 0, 77]
    idx = [base + g for g in local]
    got = subset_results(m, idx, lats)
    assert_same(got, columns_of(full, idx, 24, base=base))
    assert [int(got["topk_idx"][q, 0]) for q in range(3)] == [base + 40, base + 47, base + 54]     # rank lists carry global indices
    assert (got["topk_idx"][:, :7] >= base).all() and (got["topk_idx"][:, 7:] == -1).all()
    with pytest.raises(M.AfisError, match=EINVAL):
        m.subset_create(local)                                              # the same positions without the base lie outside the shard
    assert m.get_option("subset_device_bytes") == 0
    m.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_handles_and_edits(codebook_bytes, pool, lats):
    base_ts = pool[:150]
    m = fresh(codebook_bytes, base_ts)
    before = full_results(m, lats)
    ia, ib = [47, 3, 40, 149, 0, 54, 60], list(range(10, 70))
    ha, hb = m.subset_create(ia), m.subset_create(ib)
    qh = m.upload_queries(lats)
    kw = dict(k=24, want_scores=True, want_parts=True)
    first_a, first_b = words(m.search_subset_resident(ha, qh, **kw)), words(m.search_subset_resident(hb, qh, **kw))
    assert_same(first_a, columns_of(before, ia, 24)); assert_same(first_b, columns_of(before, ib, 24))
    for _ in range(2):                                                      # interleaved with full searches: nothing sees anything of the others
        assert_same(words(m.search_resident(qh, **kw)), before, "full search beside live subsets")
        assert_same(words(m.search_subset_resident(hb, qh, **kw)), first_b)
        assert_same(full_results(m, lats), before)
        assert_same(words(m.search_subset_resident(ha, qh, **kw)), first_a)
        assert_same(words(m.search_subset(ha, lats, **kw)), first_a)
    a = m.correspondences(lats[0], [40, 41])
    assert a[0][0] is not None
    # a removal of a listed entry: both handles are refused and free cleanly
    m.gallery_remove([47, 20])
    for h in (ha, hb):
        with pytest.raises(M.AfisError, match=ESTATE):
            m.search_subset(h, lats, **kw)
        with pytest.raises(M.AfisError, match=ESTATE):
            m.search_subset_resident(h, qh, **kw)
    m.subset_free(ha); m.subset_free(hb); m.free_queries(qh)
    assert m.get_option("subset_device_bytes") == 0
    edited = [T.FPTemplate() if i in (47, 20) else t for i, t in enumerate(base_ts)]
    f = fresh(codebook_bytes, edited)
    got = subset_results(m, ia, lats)
    assert (got["scores"][:, 0] == MINUS1).all()                            # 47 is an empty entry now
    assert_same(got, columns_of(full_results(f, lats), ia, 24), "after the removal, against a fresh commit of the edited gallery")
    f.close()
    # an appending commit: the old handle is refused, a new subset may list the appended indices
    h = m.subset_create(ia)
    m.gallery_reopen(); m.gallery_add(pool[300:340]); m.gallery_commit(0)     # 160, 161, 162: mates of latent 0 (pool 310 ...)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_subset(h, lats, **kw)
    m.subset_free(h)
    f = fresh(codebook_bytes, edited + pool[300:340])
    ic = [189, 160, 47, 150, 149, 3, 162, 161]
    got = subset_results(m, ic, lats)
    assert_same(got, columns_of(full_results(f, lats), ic, 24), "after the append, against a fresh commit")
    assert int(got["topk_idx"][0, 0]) == 160
    assert_same(full_results(m, lats), full_results(f, lats))
    m.close(); f.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_contracts(codebook_bytes, pool, lats):
    m = M.Matcher(codebook_bytes)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.subset_create([0])                                                # before the first commit
    m.gallery_add(pool[:60]); m.gallery_commit(0)
    ref = full_results(m, lats)
    keep = m.subset_create([5, 40, 7])
    held = m.get_option("subset_device_bytes")
    assert held > 0
    h2d = m.get_option("gallery_h2d_bytes")
    for bad in ([3, 4, 3], [60], [-1], [3, 1 << 40]):                       # a duplicate, out of range
        with pytest.raises(M.AfisError, match=EINVAL):
            m.subset_create(bad)
    out = C.c_void_p()
    three = np.array([1, 2, 3], np.int64)
    assert m.lib.afis_subset_create(m.ctx, three.ctypes.data_as(C.POINTER(C.c_int64)), -1, C.byref(out)) == -1 and not out.value      # a negative n
    assert m.lib.afis_subset_create(m.ctx, None, 3, C.byref(out)) == -1 and not out.value                                             # a null list with n > 0
    m.gallery_reopen(); m.gallery_add(pool[300:303])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.subset_create([1, 61])                                            # staged after reopen, not committed
    with pytest.raises(M.AfisError, match=EINVAL):
        m.subset_create([1, 63])                                            # beyond what is staged
    qh = m.upload_queries(lats)
    assert m.lib.afis_search_subset_resident(m.ctx, keep[0], qh[0], None, None, None, 5, None, None) == -1                            # k > 0 without output arrays
    v = M._Views(lats)
    assert m.lib.afis_search_subset(m.ctx, keep[0], v.arr, v.n, None, None, None, 5, None, None) == -1
    assert m.get_option("subset_device_bytes") == held and m.get_option("gallery_h2d_bytes") == h2d
    assert_same(full_results(m, lats), ref, "after the refused calls")
    assert_same(words(m.search_subset_resident(keep, qh, k=24, want_scores=True, want_parts=True)), columns_of(ref, [5, 40, 7], 24))   # between reopen and commit: the resident shard, as a full search
    r = m.search_subset_resident(keep, qh, k=0, want_scores=True)           # k = 0 skips the rank lists
    assert r["topk_idx"] is None and np.array_equal(r["scores"].view(np.uint32), ref["scores"][:, [5, 40, 7]])
    second = m.subset_create([])
    assert m.get_option("subset_device_bytes") == held                      # an empty subset holds nothing
    m.free_queries(qh); m.subset_free(second); m.subset_free(keep)
    assert m.get_option("subset_device_bytes") == 0
    left = m.subset_create([1, 2])                                          # still live at close: afis_destroy releases it
    assert m.get_option("subset_device_bytes") > 0 and left[1] == 2
    m.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_subset_search_allocates_before_it_queues_and_never_again(codebook_bytes, tmp_path):
    """The allocation rule holds for subset searches: with AFIS_ALLOC_TRACE=1 no (re)allocation of 64 MB or more follows "the search starts queuing", in
    either schedule, with the columns permuted or not; the same search again allocates nothing."""
    cbp = tmp_path / "cb.dat"; cbp.write_bytes(codebook_bytes)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import importlib, sys
        sys.path.insert(0, {root!r})
        import numpy as np
        T = importlib.import_module("msu-latentafis_amd.host.templates"); S = importlib.import_module("msu-latentafis_amd.host.synth"); M = importlib.import_module("msu-latentafis_amd.host.matcher")
        cbb = open({str(cbp)!r}, "rb").read(); cb = T.Codebook.from_bytes(cbb)
        rng = np.random.default_rng(5)
        short = [S.make_latent(rng, n_tex_lo=400, n_tex_hi=420) for _ in range(8)]
        long_ = [S.make_latent(rng, n_tex_lo=990, n_tex_hi=1000) for _ in range(8)]
        gal = S.make_packed_gallery(5, 9000, cb)
        m = M.Matcher(cbb); m.gallery_add_packed(gal); m.gallery_commit(0)
        def mark(s): sys.stderr.write("mark: " + s + "\\n"); sys.stderr.flush()
        mark("create"); h = m.subset_create(rng.permutation(9000)[:8500]); hs = m.subset_create(np.arange(100, 8600))
        mark("short"); a = m.search_subset(h, short, k=4, want_parts=True)
        mark("long"); b = m.search_subset(h, long_, k=4, want_parts=True)
        mark("long again"); b2 = m.search_subset(h, long_, k=4, want_parts=True)
        assert np.array_equal(b["scores"], b2["scores"])
        assert m.timing()["overlapped_groups"] >= 1
        mark("ascending"); m.search_subset(hs, long_, k=4)
        mark("host rank lists"); m.search_subset(h, long_, k=100, want_scores=False)
        m.set_option("bound_cus", 0)
        mark("back to back"); c = m.search_subset(h, long_, k=4, want_parts=True)
        assert np.array_equal(b["scores"], c["scores"])
        mark("full"); m.search(long_, k=4)
        mark("end"); m.subset_free(h); m.subset_free(hs); m.close()
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, AFIS_ALLOC_TRACE="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    allocs, late, queues, where, queued = {}, {}, {}, None, False
    for line in r.stderr.splitlines():
        if line.startswith("mark: "): where = line[6:]; allocs[where] = []; late[where] = []; queues[where] = 0; queued = False
        elif line.startswith("queue: "): queued = True; queues[where] += 1
        elif line.startswith("alloc: ") and where is not None: (late if queued else allocs)[where].append(line)
    assert all(v == [] for v in late.values()), late               # nothing is (re)allocated once a search has started queuing
    assert all(queues[w] == 1 for w in ("short", "long", "long again", "ascending", "host rank lists", "back to back", "full")), queues
    assert len(allocs["create"]) >= 2, allocs                      # the sub-shards' descriptors, at least
    assert len(allocs["short"]) >= 4, allocs                       # the first search of the context allocates (row maxima, records, candidate lists ...)
    assert allocs["long again"] == [] and allocs["ascending"] == [] and allocs["back to back"] == [], allocs
