"""The recomputation kernel (k_tex_refine) at the edges of its batching: active rows are queued and turned into items 64 rows at a time; the items of a flush
are fetched 64 per load instruction, four such batches (256 items) in flight at a time, evaluated sixteen per trip, and a wave's item list holds 384 (kRfItems).  Every case is ONE (latent, rolled) pair whose
number of items is known before the GPU is involved, and the test asserts that number (refine_stats(): cells_evaluated, rows_evaluated_in_full) besides
the results, so a case that does not reach its edge fails.

How the counts are known.  A latent row that IS a rolled point's reconstruction (the point's sixteen codewords side by side) has similarity exactly 6 to
that point (every table entry is 0) and, random code vectors being far apart, at least 0.05 less to every other point: the bound pass (tolerance about
1e-3) names ONE cell.  A row whose sub-vector in one sub-quantizer is the midpoint of two codewords ties two points that differ in that sub-quantizer
only, to within rounding.  With the tied points at 0 and 1 of the template (same register group of the bound pass, accumulator slots 0 and 1) the record
names {group 0} x {slots 0, 1}: TWO cells; tied at 0 and 17 (groups 0 and 1, slots 0 and 1) it names {0, 1} x {0, 1}: FOUR cells, points 0, 1, 16, 17
(adc_mfma.hip, "Records").  A latent of at most 200 rows has every row active (matcher.cpp:736-747 keeps 200); in one of 1 000 rows the active rows are
those whose upper bound reaches the 200th largest lower bound: with at least 200 rows at exactly 6 and every other row below 5.5 (random unit
descriptors; checked on the oracle's row maxima) these are the rows at 6 and the forced rows (bounded by nothing).  Forced rows (|a| > 1000, NaN) are
evaluated over every point and add no items.  The margins themselves are checked in float64 on the CPU before anything runs on the GPU."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

TRIP, BATCH, BATCHES_IN_FLIGHT, FLUSH = 16, 64, 256, 384      # adc_refine.hip: items per trip, per load instruction, per round trip, per item list (kRfItems)
STEP = 64                                                     # active rows whose candidate cells are worked out together
MA, MB = 3, 7                                                 # the sub-quantizers in which points 1 and 17 differ from point 0


@pytest.fixture(scope="module")
def cb(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


def _same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _decode(cb, codes):
    return np.ascontiguousarray(cb.words[np.arange(cb.M), codes].reshape(-1), np.float32)


def _rolled_1000(rng, cb):
    """1 000 points with distinct random code vectors; point 1 differs from point 0 in sub-quantizer MA only, point 17 in MB only, each by the codeword farthest away."""
    r = S.make_rolled(rng, cb, n_tex=1000)
    codes = r.tex[0].codes
    for p, m in ((1, MA), (17, MB)):
        codes[p] = codes[0]
        d = ((cb.words[m].astype(np.float64) - cb.words[m, codes[0, m]].astype(np.float64)) ** 2).sum(axis=1)
        codes[p, m] = int(np.argmax(d))
    assert len({bytes(c) for c in codes}) == len(codes)
    return r


def _rows(cb, rolled, kinds):
    """Descriptors by kind: ("pt", p) the reconstruction of point p; "A" ties points 0 and 1; "B" ties points 0 and 17; ("rand", v) a given unit row;
    "big" a component beyond 1000; "nan" a NaN component (the last two: forced rows)."""
    codes = rolled.tex[0].codes
    out = []
    for k in kinds:
        if k in ("A", "B"):
            m, p = (MA, 1) if k == "A" else (MB, 17)
            d = _decode(cb, codes[0]).reshape(cb.M, -1)
            d[m] = (cb.words[m, codes[0, m]] + cb.words[m, codes[p, m]]) * np.float32(0.5)
            out.append(d.reshape(-1))
        elif k == "big":
            d = _decode(cb, codes[40]); d[11] = np.float32(1500.0); out.append(d)
        elif k == "nan":
            d = _decode(cb, codes[41]); d[50] = np.nan; out.append(d)
        elif k[0] == "pt":
            out.append(_decode(cb, codes[k[1]]))
        else:
            out.append(np.asarray(k[1], np.float32))
    return np.ascontiguousarray(np.stack(out), np.float32)


def _latent(base, des):
    lt = base.tex[0]
    n = len(des)
    return T.FPTemplate(minu=list(base.minu), tex=[T.TextureTemplate(lt.x[:n].copy(), lt.y[:n].copy(), lt.ori[:n].copy(), des=des)])


def _expected(cb, rolled, kinds, des):
    """(active rows, items, rows evaluated in full) of the pair, with the margins the argument of the module's docstring needs checked in float64."""
    b = cb.words[np.arange(cb.M)[None, :], rolled.tex[0].codes].reshape(rolled.tex[0].n, -1).astype(np.float64)
    cells = 0; full = 0; at6 = 0
    for k, a in zip(kinds, des.astype(np.float64)):
        if k in ("big", "nan"):
            full += 1; continue
        if k[0] == "rand":
            continue
        sim = np.sort(6.0 - ((a[None, :] - b) ** 2).sum(axis=1))[::-1]
        want = {"A": 2, "B": 2}.get(k, 1)                     # points within rounding of the best
        assert sim[0] - sim[want - 1] < 1e-5 and (len(sim) == want or sim[want - 1] - sim[want] > 0.05), (k, sim[:4])
        cells += {"A": 2, "B": 4}.get(k, 1); at6 += 1
    n_rand = sum(1 for k in kinds if k[0] == "rand")
    if len(kinds) <= 200:
        assert n_rand == 0
        return len(kinds), cells, full
    assert at6 >= 200 and all(k not in ("A", "B") for k in kinds)    # the 200th largest lower bound is that of a row at exactly 6
    return at6 + full, cells, full


def _check_pair(m, oracle, ocb, lat, rolled, kinds, name, parts=True):
    des = lat.tex[0].des
    active, cells, full = _expected(m.cb_, rolled, kinds, des)
    hl = oracle.latent(ocb, T.write_latent(lat))[0]; hr = oracle.rolled(T.write_rolled(rolled))[0]
    ov, oa = oracle.texture_rowmax(ocb, hl, hr)
    rand = np.array([k[0] == "rand" for k in kinds]); forced = np.array([k in ("big", "nan") for k in kinds])
    if rand.any():
        assert np.nanmax(ov[rand]) < 5.5 and (ov[~rand & ~forced] == 6.0).all(), (name, np.nanmax(ov[rand]))
    m.set_option("mf_stats", 1); m.refine_stats()
    vv, aa = m.debug_texture_rowmax(lat, 0)                   # every row (the parity tap evaluates all of them): row maxima and first arg-maxima
    assert _same_bits(ov, vv), (name, np.argwhere(ov.view(np.uint32) != vv.view(np.uint32))[:6].ravel())
    assert np.array_equal(oa, aa), (name, np.argwhere(oa != aa)[:6].ravel())
    st = m.refine_stats()
    assert st["bound_violations"] == 0 and st["rows_evaluated"] == len(kinds) and st["rows_evaluated_in_full"] >= full, (name, st)    # (a random row may have many near-best points)
    res = m.search([lat], k=0, want_parts=True)               # the selection as the search runs it
    st = m.refine_stats()
    print("%-28s rows %4d  active %4d  items %4d  in full %d   %s" % (name, len(kinds), active, cells, full, st))
    assert st["pairs"] == 1 and st["rows"] == len(kinds) and st["bound_violations"] == 0, (name, st)
    assert st["rows_evaluated"] == active and st["cells_evaluated"] == cells and st["rows_evaluated_in_full"] == full, (name, st, (active, cells, full))
    if parts:
        want = np.asarray([oracle.pair(ocb, hl, hr, 1)[1][:4]], np.float32)
        assert np.array_equal(want.view(np.uint32), res["parts"][0].view(np.uint32)), (name, want, res["parts"][0])
    else:                                                      # a NaN row maximum: the reference's S7 sort of NaN keys is undefined behaviour, there is no oracle value; the same answer twice
        assert _same_bits(res["parts"], m.search([lat], k=0, want_parts=True)["parts"]), name


def _one_template_matcher(codebook_bytes, cb, rolled):
    m = M.Matcher(codebook_bytes, taps=True)
    m.set_option("adc_variant", 9)
    m.gallery_add([rolled]); m.gallery_commit(0)
    m.cb_ = cb
    return m


def _queue_steps(kinds):
    """The kernel's row queue replayed on the CPU from the known active set: per step (the 64 rows or, at the end, the remainder whose cells are worked out together) the rows it
    takes, how many entries stay queued behind it (they wait in registers while the step may scan a full row or flush through the buffer that held them) and how many items are
    on the list when it starts.  Active rows: every row of a short latent; the rows at 6 and the forced rows of a long one (module docstring)."""
    short = len(kinds) <= 200
    active = [i for i, k in enumerate(kinds) if short or k in ("big", "nan") or k[0] == "pt"]
    cells = {i: {"A": 2, "B": 4, "big": 0, "nan": 0}.get(kinds[i], 1) for i in active}
    n_regs = (len(kinds) + 63) // 64
    queue, n_items, steps = [], 0, []
    for u in range(n_regs + 1):
        if u < n_regs:
            queue += [i for i in active if u * 64 <= i < u * 64 + 64]
        take = 64 if len(queue) >= 64 else len(queue) if u == n_regs else 0
        if take:
            rows, queue = queue[:take], queue[take:]
            steps.append({"rows": rows, "rest": len(queue), "items_pending": n_items})
            total = sum(cells[i] for i in rows)
            if n_items + total > FLUSH:
                n_items = 0
            n_items += total
    assert not queue
    return steps


def _mix(n_items):
    """Kinds of a latent of at most 200 rows with n_items items: single cells, one or two two-cell rows and the four-cell rows it takes, tie rows between ordinary ones."""
    if n_items <= 20:
        return [("pt", 100 + i) for i in range(n_items)]
    n_b = max(2, -(-(n_items - 190) // 3))                    # as few four-cell rows as keep the latent within 200 rows
    rest = n_items - 4 * n_b
    n_a = 1 if rest % 2 else 2
    ones = rest - 2 * n_a
    kinds = [("pt", 100 + i) for i in range(ones)]
    for i in range(n_b): kinds.insert((i * 7) % (len(kinds) + 1), "B")
    for i in range(n_a): kinds.insert((i * 31 + 5) % (len(kinds) + 1), "A")
    assert len(kinds) <= 200 and ones >= 0
    return kinds


def test_item_counts_around_every_batch_size(codebook_bytes, cb, oracle):
    """One below, at and one above the trip (16), the load batch (64), the batches in flight (256) and the item list (384), in a latent of at most 200 rows
    (every row active; rows of two and four cells from exact ties) and in one of 1 000 rows (selection by bounds; rows at 6 contiguous from row 0, so that the
    list fills round by round: 384 items flush at once, 385 as 384 + 1; and scattered, where the list is flushed short of its capacity)."""
    rng = np.random.default_rng(808)
    base = S.make_latent(rng, n_tex_lo=1000, n_tex_hi=1000)
    rolled = _rolled_1000(rng, cb)
    ocb = oracle.codebook(codebook_bytes)
    m = _one_template_matcher(codebook_bytes, cb, rolled)
    for edge in (TRIP, BATCH, BATCHES_IN_FLIGHT, FLUSH):
        for n in (edge - 1, edge, edge + 1):
            kinds = _mix(n)
            _check_pair(m, oracle, ocb, _latent(base, _rows(cb, rolled, kinds)), rolled, kinds, "short latent, %d items" % n)
    for edge in (STEP, 2 * STEP):                            # active rows are queued and their cells worked out 64 rows at a time: a full step and what stays queued
        for n in (edge - 1, edge, edge + 1):
            kinds = [("pt", 100 + i) for i in range(n)]
            _check_pair(m, oracle, ocb, _latent(base, _rows(cb, rolled, kinds)), rolled, kinds, "short latent, %d active rows" % n)
    unit = base.tex[0].des
    for edge in (BATCHES_IN_FLIGHT, FLUSH):
        for n in (edge - 1, edge, edge + 1):
            kinds = [("pt", 100 + i) for i in range(n)] + [("rand", unit[i]) for i in range(n, 1000)]
            _check_pair(m, oracle, ocb, _latent(base, _rows(cb, rolled, kinds)), rolled, kinds, "1000 rows, %d at 6" % n)
    for n in (FLUSH + 1, 700, 900):                          # scattered: several flushes of uneven size
        at6 = set(int(x) for x in rng.permutation(1000)[:n]); it = iter(range(60, 1000))
        kinds = [("pt", next(it)) if i in at6 else ("rand", unit[i]) for i in range(1000)]
        _check_pair(m, oracle, ocb, _latent(base, _rows(cb, rolled, kinds)), rolled, kinds, "1000 rows, %d at 6 scattered" % n)
    m.close()


def test_forced_rows_between_ordinary_rows_of_a_round(codebook_bytes, cb, oracle):
    """Rows evaluated over every point (|a| > 1000; NaN) inside 64-row rounds whose other rows put items on the list: in a short latent (with tie rows around them), in one of
    1 000 rows whose rows at 6 are contiguous, and in one whose 700 rows at 6 are scattered.  In the last the queue never empties at a step: a full-row scan runs while up to 63
    queued rows wait in registers (the scan goes through the buffer that held them) and while items of earlier steps are on the list.  That this happens is established on the
    CPU (_queue_steps) and asserted before the GPU runs, per forced kind."""
    rng = np.random.default_rng(809)
    base = S.make_latent(rng, n_tex_lo=1000, n_tex_hi=1000)
    rolled = _rolled_1000(rng, cb)
    ocb = oracle.codebook(codebook_bytes)
    m = _one_template_matcher(codebook_bytes, cb, rolled)
    unit = base.tex[0].des
    for forced, parts in ((("big",), True), (("big", "nan"), False)):
        kinds = _mix(190)
        for j, f in enumerate(forced * 3): kinds[7 + 29 * j] = f
        kinds = kinds[:200]
        _check_pair(m, oracle, ocb, _latent(base, _rows(cb, rolled, kinds)), rolled, kinds, "short latent, forced %s" % "+".join(forced), parts)
        kinds = [("pt", 100 + i) for i in range(450)] + [("rand", unit[i]) for i in range(450, 1000)]
        for j, f in enumerate(forced * 4): kinds[5 + 61 * j] = f                    # rounds 0 .. 6, all among the rows at 6
        _check_pair(m, oracle, ocb, _latent(base, _rows(cb, rolled, kinds)), rolled, kinds, "1000 rows, forced %s" % "+".join(forced), parts)
        # scattered: 700 rows at 6 anywhere among 1 000, twelve of them replaced by forced rows spread over the rounds
        at6 = sorted(int(x) for x in rng.permutation(1000)[:700]); it = iter(range(60, 1000))
        kinds = [("rand", unit[i]) for i in range(1000)]
        for i in at6: kinds[i] = ("pt", next(it))
        for j, f in enumerate(forced * (12 // len(forced))): kinds[at6[20 + 55 * j]] = f
        steps = _queue_steps(kinds)
        for f in forced:
            hit = [s_ for s_ in steps if any(kinds[i] == f for i in s_["rows"])]
            assert any(s_["rest"] > 0 and s_["items_pending"] > 0 for s_ in hit), (f, [(s_["rest"], s_["items_pending"]) for s_ in hit])
        assert len(steps) == 11, len(steps)                                             # 700 active rows: ten steps of 64 and the remainder
        _check_pair(m, oracle, ocb, _latent(base, _rows(cb, rolled, kinds)), rolled, kinds, "1000 rows scattered, forced %s" % "+".join(forced), parts)
    m.close()


def test_rolled_template_of_one_point(codebook_bytes, cb, oracle):
    """A rolled template of ONE point: every active row has the one cell; 15, 16, 17 and 200 rows (all active)."""
    rng = np.random.default_rng(810)
    base = S.make_latent(rng, n_tex_lo=1000, n_tex_hi=1000)
    rolled = S.make_rolled(rng, cb, n_tex=1)
    ocb = oracle.codebook(codebook_bytes)
    m = _one_template_matcher(codebook_bytes, cb, rolled)
    for n in (1, TRIP - 1, TRIP, TRIP + 1, BATCH + 1, 200):
        des = np.ascontiguousarray(base.tex[0].des[:n], np.float32)
        lat = _latent(base, des)
        hl = oracle.latent(ocb, T.write_latent(lat))[0]; hr = oracle.rolled(T.write_rolled(rolled))[0]
        ov, oa = oracle.texture_rowmax(ocb, hl, hr)
        m.set_option("mf_stats", 1); m.refine_stats()
        vv, aa = m.debug_texture_rowmax(lat, 0)
        assert _same_bits(ov, vv) and np.array_equal(oa, aa) and (aa == 0).all(), n
        m.refine_stats()
        res = m.search([lat], k=0, want_parts=True)
        st = m.refine_stats()
        print("one point, %3d rows: %s" % (n, st))
        assert st["pairs"] == 1 and st["rows_evaluated"] == n and st["cells_evaluated"] == n and st["rows_evaluated_in_full"] == 0 and st["bound_violations"] == 0, (n, st)   # one real point: nothing else within reach, one cell a row
        want = np.asarray([oracle.pair(ocb, hl, hr, 1)[1][:4]], np.float32)
        assert np.array_equal(want.view(np.uint32), res["parts"][0].view(np.uint32)), n
    m.close()


def test_pair_without_texture_between_two_that_have_it(codebook_bytes, cb, oracle):
    """Three templates, the middle one without a texture template: the scorer is not called for it (matcher.cpp:411) and its neighbours' results are untouched."""
    rng = np.random.default_rng(811)
    base = S.make_latent(rng, n_tex_lo=1000, n_tex_hi=1000)
    rolled = _rolled_1000(rng, cb)
    other = S.make_rolled(rng, cb, n_tex=1)
    no_tex = T.FPTemplate(minu=list(other.minu), tex=[])
    gal = [rolled, no_tex, other]
    ocb = oracle.codebook(codebook_bytes)
    m = M.Matcher(codebook_bytes, taps=True)
    m.set_option("adc_variant", 9); m.set_option("mf_stats", 1)
    m.gallery_add(gal); m.gallery_commit(0)
    kinds = _mix(FLUSH + 1)
    lat = _latent(base, _rows(cb, rolled, kinds))
    hl = oracle.latent(ocb, T.write_latent(lat))[0]
    want = [oracle.pair(ocb, hl, oracle.rolled(T.write_rolled(g))[0], 1)[1][:4] for g in gal]
    m.refine_stats()
    res = m.search([lat], k=0, want_parts=True)
    st = m.refine_stats()
    assert st["pairs"] == 2 and st["rows"] == 2 * len(kinds) and st["bound_violations"] == 0, st
    active, cells, full = _expected(cb, rolled, kinds, lat.tex[0].des)
    assert (active, cells, full) == (len(kinds), FLUSH + 1, 0)
    assert st["rows_evaluated"] == 2 * len(kinds) and st["cells_evaluated"] == cells + len(kinds) and st["rows_evaluated_in_full"] == 0, st    # the first pair's 385 items and one cell per row of the one-point template
    assert np.array_equal(np.asarray(want, np.float32).view(np.uint32), res["parts"][0].view(np.uint32)), (want, res["parts"][0])
    for g in (0, 2):
        ov, oa = oracle.texture_rowmax(ocb, hl, oracle.rolled(T.write_rolled(gal[g]))[0])
        vv, aa = m.debug_texture_rowmax(lat, g)
        assert _same_bits(ov, vv) and np.array_equal(oa, aa), g
    m.close()
