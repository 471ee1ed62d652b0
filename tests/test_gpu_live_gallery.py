"""The live gallery on the GPU: afis_gallery_reopen + afis_gallery_commit (append), afis_gallery_remove, afis_gallery_export.

The yardstick of every comparison is a context FRESHLY committed with the final gallery: scores, parts, status and the rank lists' indices and scores must agree bit for
bit (np.array_equal on the raw words), whatever route the templates took into the edited context.  Planted mates inside the appended part are also held against the
oracle.  Small cases use a few hundred templates cut from synth.make_packed_gallery (whose slices are consistent with the whole); one case uses 10 000 + 500.

Query handles: a handle uploaded before an edit is REFUSED by afis_search_resident (AFIS_ESTATE) — its launch groups were cut for the shard size of that moment —
and works again only after a new upload; test_contracts checks it.

The file adds 6 s to the GPU suite (14 tests; the 10 000 + 500 case 1.5 s).
"""
import importlib
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 2209
ESTATE, EINVAL = "afis error -3", "afis error -1"


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def lats():
    return S.make_latents(SEED, 3, n_tex_lo=300, n_tex_hi=520)


@pytest.fixture(scope="module")
def pool(cb, lats):
    """600 templates of one synthetic gallery as FPTemplate objects; entries 310 + 20 q + {0, 1, 2} and 40 + 7 q carry mates of latent q."""
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


def pack(ts):
    """FPTemplate list -> synth.PackedGallery (what gallery_add_packed takes)."""
    mo, to = [0], [0]
    mx, my, mori, mdes, tx, ty, tori, tc = [], [], [], [], [], [], [], []
    for t in ts:
        if t.minu:
            m = t.minu[0]; mx.append(m.x); my.append(m.y); mori.append(m.ori); mdes.append(m.des)
        mo.append(mo[-1] + (t.minu[0].n if t.minu else 0))
        if t.tex:
            x = t.tex[0]; tx.append(x.x); ty.append(x.y); tori.append(x.ori); tc.append(x.codes)
        to.append(to[-1] + (t.tex[0].n if t.tex else 0))
    cat = lambda a, dt, shape: np.concatenate(a).astype(dt) if a else np.zeros(shape, dt)
    return S.PackedGallery(np.array(mo, np.int64), cat(mx, np.int16, 0), cat(my, np.int16, 0), cat(mori, np.float32, 0), cat(mdes, np.float32, (0, 96)),
                           np.array(to, np.int64), cat(tx, np.int16, 0), cat(ty, np.int16, 0), cat(tori, np.float32, 0), cat(tc, np.uint8, (0, 16)))


def new_matcher(cbb, opts=None, taps=False):
    m = M.Matcher(cbb, taps=taps)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    return m


def fresh(cbb, ts, opts=None, index_base=0, taps=False):
    m = new_matcher(cbb, opts, taps)
    m.gallery_add(ts)
    m.gallery_commit(index_base)
    return m


def stage(m, ts, route, cbb=None, tmp=None):
    if route == "views":
        m.gallery_add(ts)
    elif route == "dat":
        rc = m.gallery_add_dat_batch([T.write_rolled(t) for t in ts])
        assert len(rc) == len(ts)
    elif route == "packed":
        m.gallery_add_packed(pack(ts))
    elif route == "container":
        w = M.Matcher(cbb); w.gallery_add(ts); w.gallery_save(tmp); w.close()
        m.gallery_load(tmp)
    else:
        raise ValueError(route)


def append(m, ts, route="views", index_base=0, **kw):
    m.gallery_reopen()
    stage(m, ts, route, **kw)
    m.gallery_commit(index_base)


def results(m, lats, k=24):
    r = m.search(lats, k=k, want_scores=True, want_parts=True)
    return {"scores": r["scores"].view(np.uint32), "parts": r["parts"].view(np.uint32), "status": r["status"], "topk_idx": r["topk_idx"], "topk_score": r["topk_score"].view(np.uint32)}


def assert_same(a, b, what=""):
    for key in ("scores", "parts", "status", "topk_idx", "topk_score"):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (what, key, np.argwhere(a[key] != b[key])[:6].tolist() if a[key].shape == b[key].shape else (a[key].shape, b[key].shape))


def emptied(ts, gone):
    return [T.FPTemplate() if i in gone else t for i, t in enumerate(ts)]


def oracle_scores(oracle, cbb, L, ts):
    ocb = oracle.codebook(cbb)
    hl, hr = cases.to_orc(oracle, ocb, [L], ts)
    rc, want = oracle.search(ocb, hl[0], hr, tie_mode=1)
    assert rc == 0
    return want.view(np.uint32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"adc_variant": 8}, {"ref_tie_order": 2}, {"bound_cus": 0}], ids=["default", "variant8", "tie2", "bound_cus0"])
def test_append_four_routes(opts, codebook_bytes, pool, lats, oracle, tmp_path):
    """A (300 templates) committed, then B staged through views, a .dat batch, packed arrays and a container load — in one reopened staging area — and committed."""
    A, B = pool[:300], pool[300:420]
    m = fresh(codebook_bytes, A, opts)
    m.gallery_reopen()
    stage(m, B[:30], "views"); stage(m, B[30:60], "dat"); stage(m, B[60:90], "packed"); stage(m, B[90:], "container", cbb=codebook_bytes, tmp=str(tmp_path / "b.gal"))
    assert m.gallery_size == 420
    m.gallery_commit(0)
    f = fresh(codebook_bytes, A + B, opts)
    got = results(m, lats)
    assert_same(got, results(f, lats), opts)
    if not opts:                                                            # the planted mates inside B against the oracle (tie_mode 1 = the default order)
        for q, L in enumerate(lats):
            idx = [310 + 20 * q + j for j in range(3)]
            want = oracle_scores(oracle, codebook_bytes, L, [pool[g] for g in idx])
            assert np.array_equal(got["scores"][q, idx], want) and (got["scores"][q, idx].view(np.float32) > 0).all()
            assert idx[0] in got["topk_idx"][q, :2].tolist()                 # (the other candidate for rank 1: the mate at 40 + 7 q inside A)
    m.close(); f.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def edge_templates(cb, pool):
    rng = np.random.default_rng(SEED + 2)
    no_minu = T.FPTemplate(minu=[], tex=list(pool[500].tex))
    no_tex = T.FPTemplate(minu=list(pool[501].minu), tex=[])
    big_tex = S.make_rolled(rng, cb, n_minu=77, n_tex=1000)                 # 77: not a multiple of 16
    odd = S.make_rolled(rng, cb, n_minu=33, n_tex=65)
    return [T.FPTemplate(), no_minu, no_tex, big_tex, odd, T.FPTemplate(), S.make_rolled(rng, cb, n_minu=16, n_tex=64)]


def test_repeated_uneven_appends(codebook_bytes, cb, pool, lats, tmp_path):
    """1, 7, 64 and 200 templates onto 40: the device arrays outgrow their capacity several times.  Empty entries, templates without minutiae / without texture,
    1000 texture points, a minutiae count that is no multiple of 16; the last batch goes through a container into an empty staging area (the mapped fast path)."""
    edge = edge_templates(cb, pool)
    batches = [pool[40:41], edge, pool[48:112], pool[112:312]]
    m = fresh(codebook_bytes, pool[:40])
    final = list(pool[:40])
    for i, (b, route) in enumerate(zip(batches, ("views", "packed", "dat", "container"))):
        append(m, b, route, cbb=codebook_bytes, tmp=str(tmp_path / f"b{i}.gal"))
        final += b
        assert m.gallery_size == len(final)
    f = fresh(codebook_bytes, final)
    assert_same(results(m, lats), results(f, lats))
    m.close(); f.close()


# ---- 3, 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_remove(codebook_bytes, pool, lats, oracle):
    base = pool[:150]
    base = emptied(base, {70})                                              # an entry that is empty already
    m = fresh(codebook_bytes, base)
    gone = [0, 149, 60, 61, 62, 63, 70, 47, 47]                             # first, last, a run, the empty one, one index twice (47 carries a mate of latent 1)
    m.gallery_remove(gone)
    assert m.gallery_size == 150
    want = emptied(base, set(gone))
    f = fresh(codebook_bytes, want)
    got = results(m, lats)
    assert_same(got, results(f, lats))
    minus1 = np.float32(-1).view(np.uint32)
    assert (got["scores"][:, sorted(set(gone))] == minus1).all()
    ora = oracle_scores(oracle, codebook_bytes, lats[1], [want[g] for g in (0, 47, 60, 149)])
    assert (ora == minus1).all()
    m.gallery_remove([47, 70]); m.gallery_remove([])                        # empty already: nothing changes
    assert_same(results(m, lats), got)
    m.close(); f.close()


def test_interleaved_edits(codebook_bytes, pool, lats):
    m = fresh(codebook_bytes, pool[:120])
    before = results(m, lats)
    m.gallery_reopen()
    stage(m, pool[300:380], "views")
    assert m.gallery_size == 200
    assert_same(results(m, lats), before, "search between reopen and commit sees the resident shard")
    m.gallery_commit(0)
    m.gallery_remove([5, 130, 131, 199])
    append(m, pool[120:131], "packed")
    final = emptied(pool[:120] + pool[300:380], {5, 130, 131, 199}) + pool[120:131]
    f = fresh(codebook_bytes, final)
    assert_same(results(m, lats), results(f, lats))
    m.close(); f.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_other_entry_points_after_edits(codebook_bytes, pool, lats):
    m = fresh(codebook_bytes, pool[:100])
    append(m, pool[300:340], "views")                                      # 110, 111, 112: mates of latent 0 (pool 310 ...)
    m.gallery_remove([50, 51, 52, 111])
    final = emptied(pool[:100] + pool[300:340], {50, 51, 52, 111})
    f = fresh(codebook_bytes, final)
    idx = [49, 50, 52, 53, 40, 110, 111, 112, 139]
    a, b = m.correspondences(lats[0], idx), f.correspondences(lats[0], idx)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert (u is None) == (v is None) and (u is None or np.array_equal(u, v))
    assert a[1][0] is None and a[2][0] is None and a[6][0] is None and a[5][0] is not None and a[0][0] is not None
    L = T.FPTemplate(minu=lats[0].minu[:5], tex=lats[0].tex)
    qa, ra, sa = m.One2One_matching_all_templates(L)
    qb, rb, sb = f.One2One_matching_all_templates(L)
    assert qa == qb and np.array_equal(ra, rb) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
    assert list(ra[[50, 51, 52, 111]]) == [2, 2, 2, 2] and ra.sum() == 8
    m.close(); f.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [8, 7])
def test_lazy_streams_are_rebuilt(variant, codebook_bytes, pool, lats):
    """The code streams laid out on first use (variant 8's; variant 7's, of the test library's direct kernels) exist before the edits and must not survive them."""
    opts = {"adc_variant": variant}
    m = fresh(codebook_bytes, pool[:90], opts, taps=True)
    results(m, lats)
    append(m, pool[300:350], "views")
    f1 = fresh(codebook_bytes, pool[:90] + pool[300:350], opts, taps=True)
    assert_same(results(m, lats), results(f1, lats), "after append")
    m.gallery_remove([3, 100, 101])
    f2 = fresh(codebook_bytes, emptied(pool[:90] + pool[300:350], {3, 100, 101}), opts, taps=True)
    assert_same(results(m, lats), results(f2, lats), "after remove")
    m.close(); f1.close(); f2.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_export(codebook_bytes, pool, lats, tmp_path):
    m = fresh(codebook_bytes, pool[:80])
    append(m, pool[300:330], "dat")
    m.gallery_remove([0, 17, 109])
    final = emptied(pool[:80] + pool[300:330], {0, 17, 109})
    names = [f"R{i:04d}.dat" for i in range(len(final))]
    pa, pb = str(tmp_path / "edited.gal"), str(tmp_path / "staged.gal")
    m.gallery_export(pa, names)
    w = M.Matcher(codebook_bytes); w.gallery_add(final); w.gallery_save(pb, names); w.close()
    with open(pa, "rb") as fa, open(pb, "rb") as fb:
        assert fa.read() == fb.read()
    third = M.Matcher(codebook_bytes); third.gallery_load(pa); third.gallery_commit(0)
    assert third.gallery_file_names(pa) == names
    assert_same(results(third, lats), results(m, lats))
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_save(pb)
    m.close(); third.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_shard_index_base(codebook_bytes, pool, lats):
    base = 5000
    m = fresh(codebook_bytes, pool[:100], index_base=base)
    append(m, pool[300:340], "views", index_base=base)
    m.gallery_remove([base + 7, base + 112])
    f = fresh(codebook_bytes, emptied(pool[:100] + pool[300:340], {7, 112}), index_base=base)
    got = results(m, lats)
    assert_same(got, results(f, lats))
    assert base + 110 in got["topk_idx"][0, :2].tolist() and base + 130 in got["topk_idx"][1, :2].tolist()   # rank lists carry global indices
    with pytest.raises(M.AfisError, match=EINVAL):
        m.gallery_remove([7])                                               # a local index is outside the shard [5000, 5140)
    a, b = m.correspondences(lats[0], [base + 110]), f.correspondences(lats[0], [base + 110])
    assert all(np.array_equal(u, v) for u, v in zip(a[0], b[0]))
    m.close(); f.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_contracts(codebook_bytes, pool, lats, tmp_path):
    m = M.Matcher(codebook_bytes)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_reopen()                                                  # not committed
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_remove([0])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_export(str(tmp_path / "x.gal"))
    m.gallery_add(pool[:60]); m.gallery_commit(0)
    ref = results(m, lats)
    h2d = m.get_option("gallery_h2d_bytes")
    assert h2d > 0
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_add(pool[60:61])                                          # committed and not reopened: as before
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_commit(0)
    for bad in ([-1], [60], [3, 4, 1 << 40]):
        with pytest.raises(M.AfisError, match=EINVAL):
            m.gallery_remove(bad)
    assert_same(results(m, lats), ref, "after refused removals")
    handle = m.upload_queries(lats)
    old = m.search_resident(handle, k=24, want_scores=True, want_parts=True)
    m.gallery_reopen()
    m.gallery_add(pool[300:320])
    assert m.gallery_size == 80
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_remove([1])                                               # templates are staged
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_save(str(tmp_path / "y.gal"))
    with pytest.raises(M.AfisError, match=EINVAL):
        m.gallery_commit(17)                                                # not the shard's index_base
    assert m.gallery_size == 80 and m.get_option("gallery_h2d_bytes") == h2d
    assert_same(results(m, lats), ref, "after refused calls on the reopened gallery")
    r = m.search_resident(handle, k=24, want_scores=True, want_parts=True)   # nothing edited yet: the handle is still good
    assert np.array_equal(r["scores"].view(np.uint32), old["scores"].view(np.uint32))
    m.gallery_commit(0)
    # the chosen behaviour for handles uploaded before an edit: refused, and good again after a new upload
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_resident(handle, k=24)
    m.free_queries(handle)
    handle = m.upload_queries(lats)
    f = fresh(codebook_bytes, pool[:60] + pool[300:320])
    want = results(f, lats)
    r = m.search_resident(handle, k=24, want_scores=True, want_parts=True)
    assert np.array_equal(r["scores"].view(np.uint32), want["scores"]) and np.array_equal(r["topk_idx"], want["topk_idx"])
    m.gallery_remove([2])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_resident(handle, k=24)
    m.gallery_remove([2])                                                   # a no-op is no edit: a handle uploaded now stays good across it
    m.free_queries(handle)
    handle = m.upload_queries(lats)
    m.gallery_remove([2])
    m.search_resident(handle, k=24)
    m.free_queries(handle)
    m.close(); f.close()


# ---- 10, 11 -------------------------------------------------------------------------------------------------------------------------------
def test_append_at_size_uploads_only_the_new_templates(codebook_bytes, cb):
    """10 000 resident + 500 appended.  A condition, not a measurement: the append's host-to-device bytes are at most the payload of the 500 — points x (xy + ori +
    384-byte descriptors or 16-byte codes), as the container counts them — plus 64 bytes per template of the whole gallery for the offset tables.  Then bit equality
    with a fresh commit of the 10 500 for 4 latents, whose mates sit on both sides of the seam."""
    G0, G1 = 10000, 10500
    lats4 = S.make_latents(SEED + 9, 4)
    pg = S.make_packed_gallery(SEED + 9, G1, cb)
    rng = np.random.default_rng(SEED + 10)
    for q, L in enumerate(lats4):
        for g in (G0 + 10 + 100 * q, 9000 - 1000 * q):
            nm = int(pg.minu_off[g + 1] - pg.minu_off[g]); nt = int(pg.tex_off[g + 1] - pg.tex_off[g])
            pg.set_template(g, S.make_mate(rng, cb, L, frac=0.7, n_minu=nm, n_tex=nt))
    A, B = pg.slice(0, G0), pg.slice(G0, G1)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(A); m.gallery_commit(0)
    first = m.get_option("gallery_h2d_bytes")
    assert first >= int(A.minu_off[-1]) * 392 + int(A.tex_off[-1]) * 24
    m.gallery_reopen(); m.gallery_add_packed(B); m.gallery_commit(0)
    grown = m.get_option("gallery_h2d_bytes") - first
    payload = int(B.minu_off[-1]) * (4 + 4 + 384) + int(B.tex_off[-1]) * (4 + 4 + 16)
    print(f"append of 500 onto 10 000: {grown} bytes host-to-device, payload {payload}, bound {payload + 64 * G1}; first commit {first}")
    assert 0 < grown <= payload + 64 * G1
    f = M.Matcher(codebook_bytes)
    f.gallery_add_packed(pg); f.gallery_commit(0)
    got = results(m, lats4)
    assert_same(got, results(f, lats4))
    for q in range(4):
        assert {int(got["topk_idx"][q, 0]), int(got["topk_idx"][q, 1])} == {G0 + 10 + 100 * q, 9000 - 1000 * q}
    m.gallery_remove(list(range(2000, 2400)) + [G0 + 10])
    keep = np.ones(G1, bool); keep[2000:2400] = False; keep[G0 + 10] = False
    f.close()
    f = M.Matcher(codebook_bytes)
    nm = np.diff(pg.minu_off) * keep; nt = np.diff(pg.tex_off) * keep
    mk = np.repeat(keep, np.diff(pg.minu_off)); tk = np.repeat(keep, np.diff(pg.tex_off))
    cut = S.PackedGallery(np.concatenate([[0], np.cumsum(nm)]), pg.minu_x[mk], pg.minu_y[mk], pg.minu_ori[mk], pg.minu_des[mk],
                          np.concatenate([[0], np.cumsum(nt)]), pg.tex_x[tk], pg.tex_y[tk], pg.tex_ori[tk], pg.tex_codes[tk])
    f.gallery_add_packed(cut); f.gallery_commit(0)
    assert_same(results(m, lats4), results(f, lats4), "after removing 401 of 10 500")
    m.close(); f.close()
