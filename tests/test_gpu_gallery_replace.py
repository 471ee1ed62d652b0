"""Replace in place on the GPU: afis_gallery_commit_at — staged template i takes the place of resident entry idx[i]; nothing is appended, every other index stays.

The yardstick of every comparison is a context FRESHLY committed with the final list of templates, the old list with ts[idx[i] - index_base] = staged[i]: scores, the
four parts, status and the rank lists' indices and score bits at k = 24 agree bit for bit (np.array_equal on the raw words), and afis_gallery_export of the edited context is
byte for byte the file afis_gallery_save writes of the final list.  Planted mates that are replaced in are also held against the oracle.

The helpers (pack, fresh, stage, results, assert_same) restate those of tests/test_gpu_live_gallery.py.  Shards are a few hundred templates of 300-520 texture points at
most; one case uses 10 000 resident templates and replaces 500.  The point-sum limits of the call (2^31 - 1 points) cannot be met on a shard a test may build: they are
csrc/gallery_splice_plan_check's (tests/test_gallery_replace_host.py).  Every test here fails without the entry point.

The file adds 10 s to the GPU suite (25 tests; the 10 000 / 500 case 1.3 s).
"""
import importlib

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

SEED = 2311
ESTATE, EINVAL = "afis error -3", "afis error -1"
TEX_MAX = 1000                                                              # kTexMax: every staging route keeps a template's first 1000 texture points
MINUS1 = np.float32(-1).view(np.uint32)


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


def results(m, lats, k=24):
    r = m.search(lats, k=k, want_scores=True, want_parts=True)
    return {"scores": r["scores"].view(np.uint32), "parts": r["parts"].view(np.uint32), "status": r["status"], "topk_idx": r["topk_idx"], "topk_score": r["topk_score"].view(np.uint32)}


def assert_same(a, b, what=""):
    for key in ("scores", "parts", "status", "topk_idx", "topk_score"):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (what, key, np.argwhere(a[key] != b[key])[:6].tolist() if a[key].shape == b[key].shape else (a[key].shape, b[key].shape))


def oracle_scores(oracle, cbb, L, ts):
    ocb = oracle.codebook(cbb)
    hl, hr = cases.to_orc(oracle, ocb, [L], ts)
    rc, want = oracle.search(ocb, hl[0], hr, tie_mode=1)
    assert rc == 0
    return want.view(np.uint32)


# ---- this file's own helpers ---------------------------------------------------------------------------------------------------------------
def replace(m, idx, ts, route="views", **kw):
    m.gallery_reopen()
    stage(m, ts, route, **kw)
    m.gallery_commit_at(idx)


def final_list(ts, idx, new, base=0):
    out = list(ts)
    for g, t in zip(idx, new):
        out[g - base] = t
    return out


def export_bytes(m, tmp_path, tag):
    p = str(tmp_path / f"{tag}.edited.gal")
    m.gallery_export(p)
    with open(p, "rb") as f:
        return f.read()


def saved_bytes(cbb, ts, tmp_path, tag):
    p = str(tmp_path / f"{tag}.staged.gal")
    w = M.Matcher(cbb); w.gallery_add(ts); w.gallery_save(p); w.close()
    with open(p, "rb") as f:
        return f.read()


def check_against_fresh(m, cbb, final, lats, tmp_path, tag, opts=None, base=0, taps=False):
    """The edited context m against a context freshly committed with `final`: results and the exported file.  -> m's results"""
    f = fresh(cbb, final, opts, index_base=base, taps=taps)
    got = results(m, lats)
    assert m.gallery_size == len(final) and m.resident_size == len(final)
    assert_same(got, results(f, lats), tag)
    f.close()
    assert export_bytes(m, tmp_path, tag) == saved_bytes(cbb, final, tmp_path, tag), tag
    return got


def counts(t):
    return (t.minu[0].n if t.minu else 0), (min(t.tex[0].n, TEX_MAX) if t.tex else 0)


# ---- 1: moves in both directions -------------------------------------------------------------------------------------------------------------
def test_one_entry_in_the_middle(codebook_bytes, cb, pool, lats, oracle, tmp_path):
    """Entry 60 of 120 gets a template with MORE minutiae and FEWER texture points: the minutiae ranges behind it move up, the texture ranges down.  The new template
    is a mate of latent 0: the oracle's score, bit for bit, and rank 1 or 2 (the other mate: entry 40)."""
    base = pool[:120]
    nm, nt = counts(base[60])
    new = S.make_mate(np.random.default_rng(SEED + 2), cb, lats[0], frac=0.8, n_minu=nm + 37, n_tex=nt - 111)
    m = fresh(codebook_bytes, base)
    replace(m, [60], [new])
    got = check_against_fresh(m, codebook_bytes, final_list(base, [60], [new]), lats, tmp_path, "middle")
    want = oracle_scores(oracle, codebook_bytes, lats[0], [new])
    assert got["scores"][0, 60] == want[0] and want.view(np.float32)[0] > 0
    assert 60 in got["topk_idx"][0, :2].tolist()
    m.close()


# ---- 2: ends, runs, order --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_base", [0, 5000])
def test_ends_and_a_run_out_of_order(index_base, codebook_bytes, pool, lats, tmp_path):
    """Entries 0 and G - 1 and the run 70, 71, 72 in one call, listed in an order that is not the index order (staging order != index order)."""
    base = pool[:150]
    G = len(base)
    local = [71, G - 1, 70, 0, 72]
    new = [pool[400], pool[330], pool[401], pool[310], pool[402]]           # 330: a mate of latent 1, 310: of latent 0
    m = fresh(codebook_bytes, base, index_base=index_base)
    replace(m, [index_base + g for g in local], new)
    got = check_against_fresh(m, codebook_bytes, final_list(base, local, new), lats, tmp_path, f"ends{index_base}", base=index_base)
    assert index_base + 0 in got["topk_idx"][0, :2].tolist() and index_base + G - 1 in got["topk_idx"][1, :2].tolist()     # rank lists carry global indices
    m.close()


# ---- 3: tile and span borders ----------------------------------------------------------------------------------------------------------------
def test_tile_and_span_borders(codebook_bytes, cb, pool, lats, tmp_path):
    """The counts after the replacement sit on the borders of the derived layouts — 15 / 16 / 17 and 63 / 64 / 65 minutiae (fragment tiles of 16), 31 / 32 / 33 and
    63 / 64 / 65 texture points (tiles of 32, blocks of 64) —, two entries go to 2000 minutiae and 2000 texture points (of which the shard keeps 1000), and the shard is
    laid out so that the splice kernel's spans (64 points of the descriptors, 1024 of the codes, 2048 of the 4-byte arrays) both START ON the first point of a replaced
    template and start strictly INSIDE one: asserted from the final offsets."""
    rng = np.random.default_rng(SEED + 3)
    R = lambda nm, nt: S.make_rolled(rng, cb, n_minu=nm, n_tex=nt)
    # entries 0 .. 2 sum to 2048 minutiae and 2048 texture points after the edit, so that replaced entry 3 starts on a border of every span size; replaced entry 6
    # (2000, 1000) then straddles point 4096 of both kinds
    base = [pool[0], R(30, 1000), R(18, 48), pool[3], R(17, 700), R(16, 700), pool[6]] + pool[7:40]
    idx = [6, 0, 3, 10, 11, 12, 13, 14, 15]
    new = [S.make_mate(rng, cb, lats[1], frac=0.7, n_minu=2000, n_tex=2000), S.make_mate(rng, cb, lats[0], frac=0.7, n_minu=2000, n_tex=2000), R(65, 65),
           R(15, 31), R(16, 32), R(17, 33), R(63, 63), R(64, 64), R(65, 65)]
    final = final_list(base, idx, new)
    c = np.array([counts(t) for t in final])
    assert sorted(c[idx, 0].tolist()) == [15, 16, 17, 63, 64, 65, 65, 2000, 2000] and sorted(c[idx, 1].tolist()) == [31, 32, 33, 63, 64, 65, 65, 1000, 1000]
    mo, to = np.concatenate([[0], np.cumsum(c[:, 0])]), np.concatenate([[0], np.cumsum(c[:, 1])])
    for span, offs in ((64, mo), (1024, to), (2048, mo), (2048, to)):
        starts = np.arange(0, offs[-1], span)
        on = [g for g in idx if offs[g + 1] > offs[g] > 0 and offs[g] % span == 0]
        inside = [g for g in idx if ((starts > offs[g]) & (starts < offs[g + 1])).any()]
        assert on and inside, (span, on, inside)
    m = fresh(codebook_bytes, base)
    replace(m, idx, new)
    got = check_against_fresh(m, codebook_bytes, final, lats, tmp_path, "borders")
    assert 0 in got["topk_idx"][0, :2].tolist() and 6 in got["topk_idx"][1, :2].tolist()      # the 2000-point mates
    m.close()


# ---- 4: degenerate contents ------------------------------------------------------------------------------------------------------------------
def test_empty_onto_live_is_a_removal(codebook_bytes, pool, lats, tmp_path):
    base = pool[:100]
    m = fresh(codebook_bytes, base)
    replace(m, [47, 12], [T.FPTemplate(), T.FPTemplate()])                    # 47 carries a mate of latent 1
    got = check_against_fresh(m, codebook_bytes, final_list(base, [47, 12], [T.FPTemplate()] * 2), lats, tmp_path, "emptied")
    assert (got["scores"][:, [12, 47]] == MINUS1).all()
    r = fresh(codebook_bytes, base)
    r.gallery_remove([47, 12])
    assert_same(got, results(r, lats), "against afis_gallery_remove")
    assert export_bytes(r, tmp_path, "removed") == export_bytes(m, tmp_path, "emptied2")
    m.close(); r.close()


def test_live_onto_removed_and_empty_entries(codebook_bytes, pool, lats, tmp_path):
    """Re-enrolment at freed indices: entry 20 was committed empty, entry 30 was removed; both get live templates (30 a mate of latent 2)."""
    base = final_list(pool[:80], [20], [T.FPTemplate()])
    m = fresh(codebook_bytes, base)
    m.gallery_remove([30])
    new = [pool[350], pool[410]]
    replace(m, [30, 20], new)
    got = check_against_fresh(m, codebook_bytes, final_list(base, [30, 20], new), lats, tmp_path, "reenrol")
    assert 30 in got["topk_idx"][2, :2].tolist() and (got["scores"][:, [20, 30]] != MINUS1).all()
    m.close()


def test_minutiae_only_and_texture_only_in_both_directions(codebook_bytes, pool, lats, tmp_path):
    only_m = lambda t: T.FPTemplate(minu=list(t.minu), tex=[])
    only_t = lambda t: T.FPTemplate(minu=[], tex=list(t.tex))
    base = final_list(pool[:60], [10, 11, 12, 13], [only_m(pool[10]), only_t(pool[11]), only_m(pool[12]), only_t(pool[13])])
    idx = [10, 11, 12, 13, 14, 15]
    new = [only_t(pool[420]), only_m(pool[421]), pool[422], pool[423], only_m(pool[424]), only_t(pool[425])]
    m = fresh(codebook_bytes, base)
    replace(m, idx, new)
    check_against_fresh(m, codebook_bytes, final_list(base, idx, new), lats, tmp_path, "only")
    m.close()


def test_every_replaced_entry_keeps_its_counts(codebook_bytes, cb, pool, lats, tmp_path):
    """No range moves: every offset table after the edit is the one before it."""
    base = pool[:90]
    rng = np.random.default_rng(SEED + 4)
    idx = [88, 3, 44, 45]
    new = [S.make_mate(rng, cb, lats[g % 3], frac=0.7, n_minu=counts(base[g])[0], n_tex=counts(base[g])[1]) for g in idx]
    m = fresh(codebook_bytes, base)
    replace(m, idx, new)
    got = check_against_fresh(m, codebook_bytes, final_list(base, idx, new), lats, tmp_path, "kept")
    assert 88 in got["topk_idx"][88 % 3, :2].tolist()                       # (the other candidate: the mate at 40 + 7 q)
    m.close()


def test_the_whole_shard_and_a_shard_of_one(codebook_bytes, pool, lats, tmp_path):
    """n == G on 40 entries, in descending index order; then a shard of one entry."""
    base = pool[:40]
    new = pool[300:340]
    idx = list(range(39, -1, -1))
    m = fresh(codebook_bytes, base)
    replace(m, idx, new)
    got = check_against_fresh(m, codebook_bytes, final_list(base, idx, new), lats, tmp_path, "whole")
    assert int(got["topk_idx"][0, 0]) == 39 - 10                             # pool[310], the best mate of latent 0
    m.close()
    m = fresh(codebook_bytes, pool[:1])
    replace(m, [0], [pool[330]])
    check_against_fresh(m, codebook_bytes, [pool[330]], lats, tmp_path, "one")
    m.close()


# ---- 5: staging routes -----------------------------------------------------------------------------------------------------------------------
ROUTE_IDX = [55, 2, 30, 31, 79, 7]


@pytest.fixture(scope="module")
def route_case(codebook_bytes, cb, pool, lats):
    """The replacements of the route tests carry the PQ codes the DEVICE's encoder makes of fp32 descriptors near their codewords, so that the fp32 route stages the
    same templates as the others.  -> (resident list, replacements with codes, the same with fp32 descriptors, the fresh context's results)"""
    rng = np.random.default_rng(SEED + 5)
    enc = M.Matcher(codebook_bytes)
    with_codes, with_des = [], []
    for t in [pool[330], T.FPTemplate(), pool[430], T.FPTemplate(minu=list(pool[431].minu), tex=[]), pool[432], pool[433]]:       # (what a rolled .dat file can say: no texture without minutiae)
        if not t.tex:
            with_codes.append(t); with_des.append(t)
            continue
        x = t.tex[0]
        words = cb.words[np.arange(cb.M)[None, :], x.codes.astype(np.int64)].reshape(x.n, -1)
        des = np.ascontiguousarray(words + rng.standard_normal(words.shape).astype(np.float32) * 0.01, np.float32)
        with_codes.append(T.FPTemplate(minu=list(t.minu), tex=[T.TextureTemplate(x.x, x.y, x.ori, codes=enc.pq_encode(des))]))
        with_des.append(T.FPTemplate(minu=list(t.minu), tex=[T.TextureTemplate(x.x, x.y, x.ori, des=des)]))
    enc.close()
    base = pool[:80]
    f = fresh(codebook_bytes, final_list(base, ROUTE_IDX, with_codes))
    want = results(f, lats)
    f.close()
    return base, with_codes, with_des, want


@pytest.mark.parametrize("route", ["views", "views_fp32", "dat", "packed", "container_slice", "mixed"])
def test_staging_routes(route, route_case, codebook_bytes, lats, tmp_path):
    """Views with codes, views with fp32 descriptors (encoded on the device), a .dat batch, packed arrays, a first / count slice of a container that is still a pending
    mapping when the call comes, and a mixture in one staging area: one result, the fresh context's."""
    base, new, new_des, want = route_case
    m = fresh(codebook_bytes, base)
    m.gallery_reopen()
    if route == "views_fp32":
        m.gallery_add(new_des)
    elif route == "container_slice":
        p = str(tmp_path / "slice.gal")
        w = M.Matcher(codebook_bytes); w.gallery_add(base[70:73] + new + base[:2]); w.gallery_save(p); w.close()
        m.gallery_load(p, 3, len(new))
    elif route == "mixed":
        p = str(tmp_path / "mixed.gal")
        w = M.Matcher(codebook_bytes); w.gallery_add(base[:1] + new[:2]); w.gallery_save(p); w.close()
        m.gallery_load(p, 1, 2)                                             # a pending mapping that the next staging call copies into the host arrays
        m.gallery_add(new_des[2:3]); m.gallery_add_dat(T.write_rolled(new[3])); stage(m, new[4:5], "packed"); stage(m, new[5:], "dat")
    else:
        stage(m, new, route)
    assert m.gallery_size == len(base) + len(new) and m.resident_size == len(base)
    m.gallery_commit_at(ROUTE_IDX)
    assert m.gallery_size == len(base)
    assert_same(results(m, lats), want, route)
    assert export_bytes(m, tmp_path, route) == saved_bytes(codebook_bytes, final_list(base, ROUTE_IDX, new), tmp_path, route)
    m.close()


# ---- 6: layout states ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts, taps, search_first", [({}, False, False), ({}, False, True), ({"adc_variant": 8}, False, False), ({"adc_variant": 8}, False, True),
                                                      ({"adc_variant": 7}, True, True)],
                         ids=["default-before-search", "default-after-search", "variant8-before-search", "variant8-after-search", "variant7-taps-after-search"])
def test_layout_states(opts, taps, search_first, codebook_bytes, cb, pool, lats, tmp_path):
    """A replace before the first search and after searches that have built the layouts made on first use (variant 8's code stream; variant 7's, of the test library's
    direct kernels); with variant 8 selected at the commit the bound pass's stream does not exist when the replace comes, with the default it does.  The replacements are
    larger than what they replace: the derived layouts grow."""
    base = pool[:90]
    idx = [89, 20, 21]
    new = [pool[310], pool[330], pool[350]]
    rng = np.random.default_rng(SEED + 6)
    big = [S.make_rolled(rng, cb, n_minu=150 + i, n_tex=900 + i) for i in range(3)]
    m = fresh(codebook_bytes, base, opts, taps=taps)
    if search_first:
        results(m, lats)
    replace(m, idx, new)
    check_against_fresh(m, codebook_bytes, final_list(base, idx, new), lats, tmp_path, "layout", opts, taps=taps)
    if taps:                                                                # the splice launches' tap: six arrays written once each
        us, nbytes = m.compact_stats()
        c = np.array([counts(t) for t in final_list(base, idx, new)])
        assert nbytes == int(c[:, 0].sum()) * (384 + 4 + 4) + int(c[:, 1].sum()) * (16 + 4 + 4) and us > 0
    replace(m, [0, 1, 2], big)                                              # again, now with every layout of the searches above in place
    check_against_fresh(m, codebook_bytes, final_list(final_list(base, idx, new), [0, 1, 2], big), lats, tmp_path, "layout2", opts, taps=taps)
    m.close()


# ---- 7: sequences ----------------------------------------------------------------------------------------------------------------------------
def test_replace_append_remove_replace(codebook_bytes, pool, lats, oracle, tmp_path):
    base = pool[:100]                                                       # 40, 47, 54: mates of latents 0, 1, 2
    m = fresh(codebook_bytes, base)
    before = results(m, lats)
    assert int(before["topk_idx"][1, 0]) == 47
    out = pool[450]                                                         # no mate of anything
    step1 = final_list(base, [47, 5], [out, pool[330]])                      # the mate of latent 1 goes OUT at 47; a better one comes IN at 5
    replace(m, [47, 5], [out, pool[330]], "packed")
    got = check_against_fresh(m, codebook_bytes, step1, lats, tmp_path, "step1")
    want = oracle_scores(oracle, codebook_bytes, lats[1], [pool[330], out])
    assert got["scores"][1, 5] == want[0] and got["scores"][1, 47] == want[1]
    assert int(got["topk_idx"][1, 0]) == 5 and want.view(np.float32)[1] < before["scores"].view(np.float32)[1, 47]
    assert 47 not in got["topk_idx"][1, :3].tolist()
    m.gallery_reopen(); stage(m, pool[300:320], "dat"); m.gallery_commit(0)  # 110, 111, 112: mates of latent 0
    step2 = step1 + pool[300:320]
    check_against_fresh(m, codebook_bytes, step2, lats, tmp_path, "step2")
    m.gallery_remove([5, 110, 119])
    step3 = final_list(step2, [5, 110, 119], [T.FPTemplate()] * 3)
    check_against_fresh(m, codebook_bytes, step3, lats, tmp_path, "step3")
    new = [pool[310], pool[350], T.FPTemplate(), pool[451]]
    replace(m, [119, 5, 0, 111], new)                                        # two freed indices re-used, one entry emptied, a mate replaced out
    step4 = final_list(step3, [119, 5, 0, 111], new)
    got = check_against_fresh(m, codebook_bytes, step4, lats, tmp_path, "step4")
    want = oracle_scores(oracle, codebook_bytes, lats[0], [pool[310]])
    assert got["scores"][0, 119] == want[0] and int(got["topk_idx"][0, 0]) == 119
    assert 111 not in got["topk_idx"][0, :3].tolist() and (got["scores"][:, [0, 110]] == MINUS1).all()
    m.close()


# ---- 8: contracts ----------------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(codebook_bytes, pool, lats):
    """Every refused call leaves the search results, gallery_size and resident_size as they were, and the correct call that follows succeeds.  The correct calls put
    pool[330] and pool[310] at entry 9 in turn: two fresh contexts are the yardsticks of all of them."""
    base, BASE = pool[:60], 700
    G = len(base)
    alt = [pool[330], pool[310]]
    want = []
    for t in alt:
        f = fresh(codebook_bytes, final_list(base, [9], [t]), index_base=BASE)
        want.append(results(f, lats)); f.close()
    m = M.Matcher(codebook_bytes)
    m.gallery_add(base)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_commit_at([BASE + i for i in range(G)])                    # not committed
    assert m.gallery_size == G
    m.gallery_commit(BASE)
    ref = results(m, lats)
    turn = 0

    def unchanged(staged):
        assert m.gallery_size == G + staged and m.resident_size == G
        assert_same(results(m, lats), ref, "after a refused call")

    def good():
        nonlocal ref, turn
        m.gallery_commit_at([BASE + 9])
        assert m.gallery_size == G and m.resident_size == G
        ref = results(m, lats)
        assert_same(ref, want[turn], "the correct call after a refused one")
        turn ^= 1

    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_commit_at([BASE + 9])                                     # not reopened
    unchanged(0)
    m.gallery_reopen()
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_commit_at([])                                             # nothing staged
    with pytest.raises(M.AfisError, match=ESTATE):
        m.gallery_commit_at([BASE + 9])
    unchanged(0)
    m.gallery_add(alt[turn:turn + 1])
    good()
    null_idx = lambda: m._chk(m.lib.afis_gallery_commit_at(m.ctx, None, 1))
    for bad in (null_idx, [], [BASE + 9, BASE + 10], [BASE - 1], [BASE + G], [9], [1 << 40], [-1]):
        m.gallery_reopen()
        m.gallery_add(alt[turn:turn + 1])
        with pytest.raises(M.AfisError, match=EINVAL):
            bad() if callable(bad) else m.gallery_commit_at(bad)
        unchanged(1)
        good()
    m.gallery_reopen()
    m.gallery_add([alt[turn], pool[400]])
    with pytest.raises(M.AfisError, match=EINVAL):
        m.gallery_commit_at([BASE + 9, BASE + 9])                            # an index listed twice
    unchanged(2)
    with pytest.raises(M.AfisError, match=EINVAL):
        m.gallery_commit_at([BASE + 9])                                     # fewer indices than staged templates
    unchanged(2)
    # a plain commit of the same staging still appends
    m.gallery_commit(BASE)
    f = fresh(codebook_bytes, final_list(base, [9], [alt[turn ^ 1]]) + [alt[turn], pool[400]], index_base=BASE)
    assert m.gallery_size == G + 2 and m.resident_size == G + 2
    assert_same(results(m, lats), results(f, lats), "a plain commit after a refused replace")
    m.close(); f.close()


def test_handles_after_a_replace(codebook_bytes, pool, lats):
    base = pool[:60]
    G = len(base)
    m = fresh(codebook_bytes, base)
    plain, reserved = m.upload_queries(lats), m.upload_queries(lats, reserve=G)
    sub = m.subset_create([3, 9, 40])
    lab, subj = m.labels_create(np.ones(G, np.uint64)), m.subjects_create(np.arange(G) // 2)
    m.search_resident(plain, k=24)
    m.rank_hits(float("-inf"), 4)
    replace(m, [9], [pool[330]])
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_hits(float("-inf"), 4, n_q=len(lats))                         # the last search's matrix went with the edit
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_resident(plain, k=24)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.search_subset(sub, lats)
    f = fresh(codebook_bytes, final_list(base, [9], [pool[330]]))
    want = results(f, lats)
    r = m.search_resident(reserved, k=24, want_scores=True, want_parts=True)
    got = {"scores": r["scores"].view(np.uint32), "parts": r["parts"].view(np.uint32), "status": r["status"], "topk_idx": r["topk_idx"], "topk_score": r["topk_score"].view(np.uint32)}
    assert_same(got, want, "a reserved handle after the replace")
    m.rank_hits(float("-inf"), 4)                                           # there is a matrix again: what refuses the two calls below is the handles' age
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_subjects(subj, len(lats), k=5)
    with pytest.raises(M.AfisError, match=ESTATE):
        m.rank_hits_filtered(float("-inf"), 4, labels=lab, masks=np.tile(np.array([1, 0, 0], np.uint64), (len(lats), 1)))
    m.subset_free(sub); m.labels_free(lab); m.subjects_free(subj); m.free_queries(plain); m.free_queries(reserved)
    m.close(); f.close()


def test_only_the_staged_points_and_the_tables_cross_pcie(codebook_bytes, pool):
    """A condition on option gallery_h2d_bytes: over the call it grows by at most the staged templates' bytes — points x (xy + orientation + 384-byte descriptors or 16-byte
    codes) — plus the five offset tables of G + 1 int32 (minutiae, fragment tiles, texture, 64-point blocks, 32-point tiles), the G flag bytes, and the splice's own two
    device tables: the SOURCE TABLE of the minutiae arrays and the SOURCE TABLE of the texture arrays, G int32 each (csrc/gallery_splice_plan.h: where each template's range
    starts, in the resident or in the staged array).  The resident points (20 times the bound here) did not cross."""
    base = pool[:300]
    G = len(base)
    new = pool[400:410]
    m = fresh(codebook_bytes, base)
    first = m.get_option("gallery_h2d_bytes")
    m.gallery_reopen()
    m.gallery_add(new)
    assert m.get_option("gallery_h2d_bytes") == first
    m.gallery_commit_at(list(range(100, 200, 10)))
    grown = m.get_option("gallery_h2d_bytes") - first
    c = np.array([counts(t) for t in new])
    staged = int(c[:, 0].sum()) * (4 + 4 + 384) + int(c[:, 1].sum()) * (4 + 4 + 16)
    bound = staged + 5 * (G + 1) * 4 + G + 2 * G * 4
    print(f"replace of 10 in 300: {grown} bytes host-to-device, staged {staged}, bound {bound}; first commit {first}")
    assert staged <= grown <= bound and first > 20 * bound
    m.close()


# ---- 9: the medium case ----------------------------------------------------------------------------------------------------------------------
def spliced(A, B, idx):
    """PackedGallery A with entry idx[j] = entry j of B."""
    src = [(A, g) for g in range(A.G)]
    for j, g in enumerate(idx):
        src[g] = (B, j)
    mo, to = [0], [0]
    parts = [[] for _ in range(8)]
    for P, g in src:
        a, b, c, d = int(P.minu_off[g]), int(P.minu_off[g + 1]), int(P.tex_off[g]), int(P.tex_off[g + 1])
        for k, (arr, lo, hi) in enumerate(((P.minu_x, a, b), (P.minu_y, a, b), (P.minu_ori, a, b), (P.minu_des, a, b), (P.tex_x, c, d), (P.tex_y, c, d), (P.tex_ori, c, d), (P.tex_codes, c, d))):
            parts[k].append(arr[lo:hi])
        mo.append(mo[-1] + b - a); to.append(to[-1] + d - c)
    cat = [np.concatenate(p) for p in parts]
    return S.PackedGallery(np.array(mo, np.int64), cat[0], cat[1], cat[2], cat[3], np.array(to, np.int64), cat[4], cat[5], cat[6], cat[7])


def test_replace_500_of_10000(codebook_bytes, cb):
    """10 000 resident templates, 500 of them replaced in one call, in a shuffled order.  Per latent q: a mate that stays (9000 - 1000 q), a mate that is replaced IN
    (staged template 10 + 100 q) and a mate that is replaced OUT (at the index staged template 50 + 100 q goes to).  Equal to a fresh commit of the final gallery, and the
    host-to-device bytes obey the bound of the test above."""
    G0, n = 10000, 500
    lats4 = S.make_latents(SEED + 9, 4)
    pg = S.make_packed_gallery(SEED + 9, G0 + n, cb)
    rng = np.random.default_rng(SEED + 10)
    idx = rng.permutation(np.arange(n) * 20 + 3)
    plant = lambda g, L: pg.set_template(g, S.make_mate(rng, cb, L, frac=0.7, n_minu=int(pg.minu_off[g + 1] - pg.minu_off[g]), n_tex=int(pg.tex_off[g + 1] - pg.tex_off[g])))
    for q, L in enumerate(lats4):
        plant(9000 - 1000 * q, L); plant(G0 + 10 + 100 * q, L); plant(int(idx[50 + 100 * q]), L)
    A, B = pg.slice(0, G0), pg.slice(G0, G0 + n)
    m = M.Matcher(codebook_bytes)
    m.gallery_add_packed(A); m.gallery_commit(0)
    before = results(m, lats4)
    first = m.get_option("gallery_h2d_bytes")
    m.gallery_reopen(); m.gallery_add_packed(B); m.gallery_commit_at(idx)
    grown = m.get_option("gallery_h2d_bytes") - first
    staged = int(B.minu_off[-1]) * (4 + 4 + 384) + int(B.tex_off[-1]) * (4 + 4 + 16)
    assert staged <= grown <= staged + 5 * (G0 + 1) * 4 + G0 + 2 * G0 * 4
    f = M.Matcher(codebook_bytes)
    f.gallery_add_packed(spliced(A, B, idx)); f.gallery_commit(0)
    got = results(m, lats4)
    assert_same(got, results(f, lats4))
    for q in range(4):
        gone, came = int(idx[50 + 100 * q]), int(idx[10 + 100 * q])
        assert {int(before["topk_idx"][q, 0]), int(before["topk_idx"][q, 1])} == {9000 - 1000 * q, gone}
        assert {int(got["topk_idx"][q, 0]), int(got["topk_idx"][q, 1])} == {9000 - 1000 * q, came}
        assert gone not in got["topk_idx"][q, :3].tolist()
    m.close(); f.close()
