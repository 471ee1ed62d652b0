"""GPU parity at BASELINE.json's full sizes: configs[1] (1 latent x 10 000 rolled templates) and configs[2] (batch of 100
latents x 100 000 templates, one step), through the C ABI.

At these sizes the oracle cannot score everything in a test's time budget on every host, so each test combines
  * size-independent properties over ALL pairs (planted mates lead every rank list in planting order; the rank list is
    the lexsort (score descending, index ascending) of the score vector; fusion identity on every pair; -1/0 conventions;
    ADC variants give identical bits), with
  * a bit-for-bit oracle sample: every planted mate plus >= 200 random non-mates per sampled query (configs[2]), or
    every pair of the gallery (configs[1]; 10 000 oracle pairs take about a second on the GPU box's host cores).
The oracle runs in tie_mode=1 (equal keys by ascending index = what the HIP path implements) for the bit-exact checks and in
tie_mode=0 (libstdc++ std::sort order = what the reference binary executes, matcher.cpp:476, :741, :1301, :1423, :1590)
for the tolerance statistics SURVEY section 8d states: |d| <= 1e-3*max(1,|s|) for >= 99.9 % of pairs.
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


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


def _oracle_rows(oracle, ocb, latent, gal, gidx, tie_mode):
    """[len(gidx), 5] = (s0, s1, s2, tex, fused) of `latent` against gallery templates gidx, all host threads."""
    hl, _ = oracle.latent(ocb, T.write_latent(latent))
    hr = [oracle.rolled(T.write_rolled(gal.template(int(g))))[0] for g in gidx]
    rc, sc, parts = oracle.search(ocb, hl, hr, tie_mode=tie_mode, threads=oracle.lib.orc_num_threads(), want_parts=True)
    assert rc == 0
    for h in hr:
        oracle.lib.orc_rolled_free(h)
    oracle.lib.orc_latent_free(hl)
    return parts


def _got_rows(res, q, gidx):
    return np.concatenate([res["parts"][q][gidx], res["scores"][q][gidx][:, None]], axis=1)


def _check_properties(res, planted, G, k):
    Q = res["scores"].shape[0]
    p = res["parts"]
    fused = ((p[..., 0] + p[..., 1]) + p[..., 2]).astype(np.float64) + p[..., 3].astype(np.float64) * 0.3   # matcher.cpp:188
    assert np.array_equal(fused.astype(np.float32), res["scores"])
    assert (res["scores"] >= 0).all()                                   # no empty rolled template in the synthetic gallery
    ar = np.arange(G)
    for q in range(Q):
        want = [g for g, _ in planted[q]]
        assert list(res["topk_idx"][q][:len(want)]) == want, (q, res["topk_idx"][q][:6], want)
        order = np.lexsort((ar, -res["scores"][q].astype(np.float64)))[:k]                                     # matcher.cpp:306-309 + tie rule
        assert np.array_equal(res["topk_idx"][q], order), q
        assert np.array_equal(res["topk_score"][q], res["scores"][q][order]), q


def test_config1_one_latent_vs_10k(codebook_bytes, cb, oracle):
    """BASELINE.json configs[1]: every one of the 10 000 pairs against the oracle, bit for bit; tie_mode=0 within tolerance."""
    G, seed = 10000, 4101
    lats = S.make_latents(seed, 1)
    gal = S.make_packed_gallery(seed, G, cb)
    planted = S.plant_mates(seed, gal, cb, lats, G=G, n_partial=5)
    mp = M.Matcher(codebook_bytes)                                     # the product library ...
    mp.gallery_add_packed(gal); mp.gallery_commit(0)
    res = mp.search(lats, k=24, want_parts=True)
    _check_properties(res, planted, G, 24)
    mp.set_option("adc_variant", 8)
    assert np.array_equal(mp.search(lats, k=0)["scores"], res["scores"])
    mp.set_option("adc_variant", 9); mp.set_option("ref_tie_order", 2)     # equal sort keys in std::sort's order at S3, S8, S9: compared with tie mode 0 below
    res_ref = mp.search(lats, k=24, want_parts=True)
    mp.close()
    m = M.Matcher(codebook_bytes, taps=True)                            # ... and the test library with the direct reference kernels (adc_variant 1, 6, 7)
    m.gallery_add_packed(gal); m.gallery_commit(0)
    for v in (1, 6, 7, 8, 9):                                           # other ADC variants (8 / 9 = bound pass + exact evaluation), same bits
        m.set_option("adc_variant", v)
        assert np.array_equal(m.search(lats, k=0)["scores"], res["scores"]), v
    m.close()
    ocb = oracle.codebook(codebook_bytes)
    allg = np.arange(G)
    want1 = _oracle_rows(oracle, ocb, lats[0], gal, allg, 1)
    got = _got_rows(res, 0, allg)
    diff = got.view(np.uint32) != want1.view(np.uint32)
    assert not diff.any(), ("first differing pair", int(np.argwhere(diff.any(axis=1))[0, 0]), int(diff.any(axis=1).sum()))
    assert (want1[:, :4] > 0).sum() > 1000                               # the sample is not a wall of zeros
    want0 = _oracle_rows(oracle, ocb, lats[0], gal, allg, 0)
    far = np.abs(got - want0) > 1e-3 * np.maximum(1.0, np.abs(want0))
    assert far.any(axis=1).mean() <= 1e-3, far.any(axis=1).sum()        # >= 99.9 % of pairs within tolerance
    r0 = np.lexsort((allg, -want0[:, 4].astype(np.float64)))[:24]
    n_pos = int((want0[r0, 4] > 0).sum())
    assert n_pos >= 6 and np.array_equal(res["topk_idx"][0][:n_pos], r0[:n_pos])   # rank list over strictly positive scores
    # option ref_tie_order 2 against the SAME tie mode 0 (what the reference binary executes): bit for bit on all but at most two of the 10 000 pairs (S7's sort is not reproduced),
    # where the default order differs on the mates — every planted mate among the identical ones
    got_ref = _got_rows(res_ref, 0, allg)
    n_ref = int((got_ref.view(np.uint32) != want0.view(np.uint32)).any(axis=1).sum()); n_def = int((got.view(np.uint32) != want0.view(np.uint32)).any(axis=1).sum())
    assert n_ref <= 2 and n_def >= 3 and n_def > n_ref, (n_ref, n_def)                # (seed 4101: 0 and 4 — the mates)
    mates = [g for g, _f in planted[0]]
    assert np.array_equal(got_ref[mates].view(np.uint32), want0[mates].view(np.uint32))


@pytest.fixture(scope="module")
def headline(codebook_bytes, cb):
    """BASELINE.json configs[2]: 100 latents x 100 000 templates, the bench workload (same generator, another seed)."""
    G, Q, seed = 100000, 100, 909
    if os.environ.get("AFIS_TEST_SMALL_HEADLINE"):                     # local debugging only
        G, Q = 20000, 16
    lats = S.make_latents(seed, Q)
    gal = S.make_packed_gallery(seed, G, cb)
    planted = S.plant_mates(seed, gal, cb, lats, G=G)
    m = M.Matcher(codebook_bytes, taps=True)                           # the product objects + the parity taps: the bound pass's self-check counter is read below
    m.gallery_add_packed(gal); m.gallery_commit(0)
    m.set_option("mf_stats", 1)
    res = m.search(lats, k=24, want_parts=True)
    res["refine_stats"] = m.refine_stats()
    m.set_option("mf_stats", 0)
    yield lats, gal, planted, m, res
    m.close()


def test_config2_properties_all_pairs(headline):
    lats, gal, planted, m, res = headline
    _check_properties(res, planted, gal.G, 24)
    # the matrix-core bound pass's self-check over ALL 10^7 pairs: every exactly evaluated row maximum lay inside the bounds the selection used
    st = res["refine_stats"]
    assert st["pairs"] == len(lats) * gal.G and st["bound_violations"] == 0 and st["rows_evaluated"] >= 200 * st["pairs"], st
    assert all(res["topk_score"][q][0] > 50 for q in range(len(lats)))
    # a second pass over resident queries gives the same bits (idempotence), without asking for the score matrix
    qh = m.upload_queries(lats)
    r2 = m.search_resident(qh, k=24)
    m.free_queries(qh)
    assert np.array_equal(r2["topk_idx"], res["topk_idx"]) and np.array_equal(r2["topk_score"], res["topk_score"])


def test_config2_oracle_sample_bit_exact(headline, codebook_bytes, oracle):
    lats, gal, planted, m, res = headline
    G, Q = gal.G, len(lats)
    ocb = oracle.codebook(codebook_bytes)
    rng = np.random.default_rng(5)
    n_pairs = n_nz = n_far0 = 0
    for q in range(Q):
        mates = np.array([g for g, _ in planted[q]])
        gidx = mates if q % 12 else np.unique(np.concatenate([mates, rng.integers(0, G, 260), res["topk_idx"][q]]))
        want = _oracle_rows(oracle, ocb, lats[q], gal, gidx, 1)
        got = _got_rows(res, q, gidx)
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), (q, int(gidx[np.argwhere(diff.any(axis=1))[0, 0]]), got[diff.any(axis=1)][:2], want[diff.any(axis=1)][:2])
        n_pairs += len(gidx); n_nz += int((want[:, :4] > 0).sum())
        if q % 12 == 0:                                                  # the reference's own sort order: tolerance, not bits
            want0 = _oracle_rows(oracle, ocb, lats[q], gal, gidx, 0)
            n_far0 += int((np.abs(got - want0) > 1e-3 * np.maximum(1.0, np.abs(want0))).any(axis=1).sum())
    assert n_pairs >= 9 * 260 + 4 * Q * 0.9 and n_nz > 500
    assert n_far0 <= max(1, n_pairs // 1000), n_far0


def test_config2_mates_in_the_reference_sort_order(headline, codebook_bytes, oracle):
    """configs[2] under option ref_tie_order 2 (equal sort keys in std::sort's order at S3, S8, S9): every planted mate of the 100 latents — the pairs whose S9 scores tie — and the
    sampled rows of the latents the tie-mode-0 check above uses, against the oracle's tie mode 0 (std::sort at EVERY site: what the reference binary executes), bit for bit except
    for at most two pairs (S7's sort is not reproduced); with the default order dozens of the mates differ."""
    lats, gal, planted, m, res = headline
    G, Q = gal.G, len(lats)
    ocb = oracle.codebook(codebook_bytes)
    m.set_option("ref_tie_order", 2)
    try:
        r2 = m.search(lats, k=24, want_parts=True)
    finally:
        m.set_option("ref_tie_order", 0)
    rng = np.random.default_rng(5)
    n_pairs = n_ref = n_def = n_mates = n_mates_ref = 0
    for q in range(Q):
        mates = np.array([g for g, _ in planted[q]])
        gidx = mates if q % 12 else np.unique(np.concatenate([mates, rng.integers(0, G, 260), res["topk_idx"][q]]))
        want0 = _oracle_rows(oracle, ocb, lats[q], gal, gidx, 0)
        d_ref = (_got_rows(r2, q, gidx).view(np.uint32) != want0.view(np.uint32)).any(axis=1)
        d_def = (_got_rows(res, q, gidx).view(np.uint32) != want0.view(np.uint32)).any(axis=1)
        n_pairs += len(gidx); n_ref += int(d_ref.sum()); n_def += int(d_def.sum())
        is_mate = np.isin(gidx, mates)
        n_mates += int(is_mate.sum()); n_mates_ref += int(d_ref[is_mate].sum())
    assert n_pairs >= 9 * 260 + 4 * Q * 0.9 and n_mates >= 3 * Q
    print(f"configs[2], sample of {n_pairs} pairs ({n_mates} planted mates) against tie mode 0: {n_ref} differ under ref_tie_order 2 ({n_mates_ref} mates), {n_def} under the default order")
    assert n_ref <= 2 and n_mates_ref <= 1 and n_def >= 20, (n_pairs, n_ref, n_def, n_mates, n_mates_ref)


def test_config2_variants_same_bits_on_a_query_slice(headline):
    lats, gal, planted, m, res = headline
    sub = [3, 41, 77] if len(lats) > 77 else [1, 2, 3]
    for v, gen in ((0, 0), (7, 1), (8, 0), (9, 0)):                     # plain-layout ADC kernel; generic minutiae candidate kernel; the two bound + refine forms
        m.set_option("adc_variant", v); m.set_option("minu_generic", gen)
        r = m.search([lats[i] for i in sub], k=24)
        assert np.array_equal(r["scores"], res["scores"][sub]) and np.array_equal(r["topk_idx"], res["topk_idx"][sub]), (v, gen)
    m.set_option("adc_variant", 7); m.set_option("minu_generic", 0)


# ---- BASELINE.json configs[3] and configs[4] on ONE GPU by virtual shards ------------------------------------------------------------
# No 8-GPU node is available to the suite, so the per-rank work of the sharded configurations runs shard after shard on GPU 0: every
# shard is generated, planted and committed exactly as rank r of an 8-rank job would (S.make_packed_gallery(seed, G, cb, lo, hi),
# plant_mates(lo=lo), gallery_commit(lo) -> global indices), searched with the default (bit-exact) kernels, and the per-shard top-24
# lists are merged with the same merge the exchange step feeds (host/sharding.py::merge_topk == rank_exchange.cpp::merge_topk).
SH = importlib.import_module("msu-latentafis_amd.host.sharding")


def _search_shards(codebook_bytes, cb, seed, G, lats, world, k, keep=None, n_partial=3, stats=None):
    """Per-shard searches of a G-template gallery cut into `world` contiguous shards balanced by rolled texture points.
    keep: {global index} whose templates (after planting) and per-part scores are kept for the oracle sample.
    Returns merged (idx, score), the per-shard lists, planted, and {g: (template, parts[Q][4], scores[Q])} for g in keep."""
    nm_all, nt_all = S.gallery_counts(seed, G)
    bounds = SH.shard_bounds(nt_all, world)
    assert bounds[0][0] == 0 and bounds[-1][1] == G and all(bounds[r][1] == bounds[r + 1][0] for r in range(world - 1))
    per_idx, per_sc, kept, planted = [], [], {}, None
    for lo, hi in bounds:
        gal, planted, m = cases.committed_slice(codebook_bytes, cb, seed, G, lats, lo, hi, n_partial=n_partial, taps=stats is not None)
        if stats is not None: m.set_option("mf_stats", 1)                # the bound pass's self-check counters of this shard (stats: a dict that accumulates them)
        res = m.search(lats, k=k, want_parts=True)
        if stats is not None:
            for k_, v in m.refine_stats().items(): stats[k_] = stats.get(k_, 0) + v
        m.close()
        assert res["scores"].shape == (len(lats), hi - lo)
        p = res["parts"]
        fused = ((p[..., 0] + p[..., 1]) + p[..., 2]).astype(np.float64) + p[..., 3].astype(np.float64) * 0.3      # matcher.cpp:188
        assert np.array_equal(fused.astype(np.float32), res["scores"])
        ar = np.arange(lo, hi)
        for q in range(len(lats)):                                       # every shard's list is the lexsort of ITS scores, global indices
            order = np.lexsort((ar, -res["scores"][q].astype(np.float64)))[:k]
            assert np.array_equal(res["topk_idx"][q], ar[order]) and np.array_equal(res["topk_score"][q], res["scores"][q][order])
        per_idx.append(res["topk_idx"]); per_sc.append(res["topk_score"])
        for g in (keep or ()):
            if lo <= g < hi:
                kept[g] = (gal.template(g - lo), res["parts"][:, g - lo].copy(), res["scores"][:, g - lo].copy())
        del gal, res
    idx, sc = SH.merge_topk(np.stack(per_idx), np.stack(per_sc), k)
    return idx, sc, bounds, planted, kept


def test_config3_eight_virtual_shards_equal_the_single_gpu_run(headline, codebook_bytes, cb):
    """configs[3]: 100 latents x 100k gallery over 8 shards of ~12.5k (the per-rank workload at N = 8): the merged rank lists are the
    single-GPU run's, bit for bit."""
    lats, gal, planted, m, res = headline
    G = gal.G
    idx, sc, bounds, planted8, _ = _search_shards(codebook_bytes, cb, 909, G, lats, 8, 24)
    assert planted8 == planted
    sizes = [hi - lo for lo, hi in bounds]
    assert len(bounds) == 8 and max(sizes) - min(sizes) < 0.02 * G / 8    # balanced by texture points: template counts within 2 %
    assert np.array_equal(idx, res["topk_idx"]) and np.array_equal(sc, res["topk_score"])


def test_config4_one_million_templates_in_eight_virtual_shards(codebook_bytes, cb, oracle):
    """configs[4]: a 1 M-template gallery, 8 shards of ~125k, 12 latents, the default bit-exact kernels (the 16-bit bound pass + exact
    refine IS this configuration's reduced-precision-LUT kernel).  Planted mates lead every merged list in planting
    order with global indices up to 10^6; a bit-for-bit oracle sample of every mate + 200 random templates per sampled query."""
    G, Q, seed, k = 1000000, 12, 31337, 24
    if os.environ.get("AFIS_TEST_SMALL_HEADLINE"):
        G = 80000
    lats = S.make_latents(seed, Q)
    slots = S.mate_slots(seed, G, Q, 3)
    rng = np.random.default_rng(8)
    sample_q = [0, 5, 11]
    keep = set(int(g) for g in slots.ravel())
    rand = {q: rng.integers(0, G, 200) for q in sample_q}
    for q in sample_q:
        keep |= set(int(g) for g in rand[q])
    st = {}
    idx, sc, bounds, planted, kept = _search_shards(codebook_bytes, cb, seed, G, lats, 8, k, keep=keep, stats=st)
    assert st["pairs"] == Q * G and st["bound_violations"] == 0, st     # every exactly evaluated row maximum of the 1.2e7 pairs inside the bounds the selection used
    assert int(slots.max()) > 0.9 * G                                   # the planted indices do span the million
    for q in range(Q):
        want = [g for g, _ in planted[q]]
        assert list(idx[q][:len(want)]) == want, (q, idx[q][:6], want)
        assert (np.diff(sc[q].astype(np.float64)) <= 0).all() and sc[q][0] > 50
        ties = np.flatnonzero(np.diff(sc[q]) == 0)
        assert all(idx[q][t] < idx[q][t + 1] for t in ties)              # equal scores by ascending GLOBAL index
    ocb = oracle.codebook(codebook_bytes)
    n_pairs = n_nz = 0
    for q in range(Q):
        gidx = [g for g, _ in planted[q]] + (list(int(g) for g in rand[q]) if q in sample_q else [])
        hl, _ = oracle.latent(ocb, T.write_latent(lats[q]))
        hr = [oracle.rolled(T.write_rolled(kept[g][0]))[0] for g in gidx]
        rc, _, want = oracle.search(ocb, hl, hr, tie_mode=1, threads=oracle.lib.orc_num_threads(), want_parts=True)
        assert rc == 0
        got = np.array([np.concatenate([kept[g][1][q], [kept[g][2][q]]]) for g in gidx], np.float32)
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), (q, gidx[int(np.argwhere(diff.any(axis=1))[0, 0])], got[diff.any(axis=1)][:2], want[diff.any(axis=1)][:2])
        for h in hr:
            oracle.lib.orc_rolled_free(h)
        oracle.lib.orc_latent_free(hl)
        n_pairs += len(gidx); n_nz += int((want[:, :4] > 0).sum())
    assert n_pairs >= 4 * Q + 3 * 190 and n_nz > 100


def test_a_search_that_outlasts_its_deadline_returns_an_error_and_the_context_recovers(headline):
    """Every host wait of a search is bounded (option search_timeout_s / AFIS_SEARCH_TIMEOUT_S): a device that does not finish in time — here a 2 s search given 150 ms — makes
    afis_search return AFIS_EDEVICE instead of holding the caller's thread; with side streams in use the context then keeps to one stream (bound_cus reads 0) until the option
    is set again.  Once the device has drained, the context searches as before, same bits.  (No output buffer is passed to the call that times out: the device may still be writing.)"""
    import time
    lats, gal, planted, m, res = headline
    m.set_option("adc_variant", 9); m.set_option("minu_generic", 0)      # (an earlier test leaves a reference kernel selected)
    assert m.get_option("bound_cus") == 128
    qh = m.upload_queries(lats)
    m.search_resident(qh, k=0)                                           # warm: buffers allocated
    m.set_option("search_timeout_ms", 150)
    t0 = time.time()
    with pytest.raises(M.AfisError, match="did not finish"):
        m.search_resident(qh, k=0)
    assert time.time() - t0 < 2.0                                        # it came back at the deadline, not when the device was done
    assert m.get_option("bound_cus") == 0                                # the overlapped schedule is off for this context
    time.sleep(0.5)                                                      # (the next call waits for what the failed one had queued: no need to)
    m.set_option("search_timeout_s", 600)
    sub = [5, 50]
    r = m.search([lats[i] for i in sub], k=24)                           # one stream now
    assert np.array_equal(r["scores"], res["scores"][sub]) and np.array_equal(r["topk_idx"], res["topk_idx"][sub])
    m.set_option("bound_cus", 128)
    assert m.get_option("bound_cus") == 128
    r = m.search([lats[i] for i in sub], k=24)
    assert np.array_equal(r["scores"], res["scores"][sub])
    m.free_queries(qh)
