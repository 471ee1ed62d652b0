"""S7 of the texture lists (k_graph_texture, graph.hip): the compact path that ranks ALL n_in rows the recomputation passed on (200 <= n_in <= 256, four keys per lane) and
keeps the entries of rank < 200, next to the kept path (n_in > 256, and the dense form the parity taps use).  Every case is ONE (latent, rolled) pair whose n_in is known
before the GPU is involved, and the test asserts it (refine_stats(): rows_evaluated is the pair's n_in), so a case that does not reach its edge fails.

How n_in is steered.  A latent row b_p + t d (b_p the reconstruction of rolled point p, d a unit direction) has similarity 6 - t^2 to point p and far less to every other
point, so a row's maximum can be put where it is wanted.  The recomputation passes on the rows whose upper bound reaches the 200th largest lower bound (adc_refine.hip).  Rows
that share a descriptor have identical bounds: when the 200th largest maximum belongs to such a group the whole group is passed on, together with every row above it, and a
row 0.25 or more below it (the bounds are about 1e-3 wide) is not.  Rows of one point and one direction whose t^2 differ by 2e-6 ("near": maxima a few ulps apart, all
distinct) behave the same way as long as the group's spread stays far below the bounds' width.  Forced rows (NaN, infinite or |a| > 1000: bounded by nothing) are always
passed on.  _expect() derives n_in from the oracle's row maxima and checks these margins on the CPU.

What is compared.  The search's part scores (adc_variant 9: compact form, the path under test) with the oracle's (tie mode 1) and with the same search through the direct
exact kernel (adc_variant 0: dense form, the kept S7), bit for bit; and the stage-0 tap (the S7 list, content and order) with the oracle's trace.  The tap always runs the
direct kernel and the dense form (afis_taps.cpp), so the compact path's list is held to the oracle through the scores.

What the scores can and cannot see.  WHICH rows of a tie at the 200th place are listed: of the tied rows ("dup": one descriptor; "exact": maxima of exactly 6 at distinct
rolled points) only the lower half, by row, lies where its rolled point lies; the upper half has a random place and direction and does not survive S8b / S9.  Keeping the
highest rows of the tie instead of the lowest therefore changes the score, and the cases of CUT_DECIDES assert that on the CPU before the GPU runs: the oracle scores the
latent with the tied rows' records in reverse order (what a highest-rows-win kernel would in effect list) and the texture score must differ by more than 1.  Among them are
n_in 201, 255 and 256 on the compact path.  The ORDER of equal maxima inside the 200 is not visible in a score by itself: equal similarities add up to the same sum in any
order; a kernel that ordered ties by descending slot is caught through the rows it would keep at the 200th place, not through the order of the ones it lists."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")

TOP, FAST = 200, 256            # graph.hip: kTopTex, kTexFast
GAP, NEAR = 0.25, 3e-4          # a row that is not to be passed on lies GAP below the 200th maximum; a "near" group spreads over less than NEAR
N_ROLLED = 400
P_GROUP = N_ROLLED - 1          # the rolled point the "dup" and "near" groups sit at (the "high" rows take points 0, 1, ...)


def _same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _dir(rng):
    v = rng.standard_normal(96)
    return (v / np.sqrt((v * v).sum())).astype(np.float32)


class Bench:
    """One rolled template of 400 points with distinct random code vectors, its matcher (taps, mf_stats) and the oracle's handles."""
    def __init__(self, codebook_bytes, oracle):
        self.cbb = codebook_bytes
        self.cb = T.Codebook.from_bytes(codebook_bytes)
        self.oracle = oracle
        self.ocb = oracle.codebook(codebook_bytes)
        rng = np.random.default_rng(1107)
        self.base = S.make_latent(rng, n_tex_lo=1000, n_tex_hi=1000)
        self.rolled = S.make_rolled(rng, self.cb, n_tex=N_ROLLED)
        codes = self.rolled.tex[0].codes
        assert len({bytes(c) for c in codes}) == len(codes)
        self.recon = np.ascontiguousarray(self.cb.words[np.arange(self.cb.M)[None, :], codes].reshape(N_ROLLED, -1), np.float32)
        self.hr = oracle.rolled(T.write_rolled(self.rolled))[0]
        self.m = None

    def open(self):
        self.m = M.Matcher(self.cbb, taps=True)
        self.m.set_option("adc_variant", 9); self.m.set_option("mf_stats", 1)
        self.m.gallery_add([self.rolled]); self.m.gallery_commit(0)

    def latent(self, groups, seed):
        """groups: ("high", n, lo, hi) n rows at points 0 .. n-1 with maxima evenly spaced in [lo, hi]; ("exact", n) the
        reconstructions of the next n points themselves: maxima of exactly 6, every table entry being 0; ("dup", n, s[, point]) n copies of one row with maximum s;
        ("near", n, s) n rows with maxima 2e-6 apart below s; ("bad", n, scale) random descriptors of the synthetic latents times scale; ("nan" | "inf" | "big", n) forced rows.
        Rows are shuffled, so that the groups' slots interleave; a "high" row sits where its rolled point sits (shifted by a block or two): a mate-like list."""
        rng = np.random.default_rng(seed)
        rt = self.rolled.tex[0]
        unit = self.base.tex[0].des
        des, kind, pt = [], [], []
        d_grp = _dir(rng)
        nxt = 0
        for g in groups:
            name, n = g[0], g[1]
            for j in range(n):
                if name == "high":
                    s = g[2] + (g[3] - g[2]) * (j / max(n - 1, 1))
                    des.append(self.recon[nxt] + np.float32(np.sqrt(6.0 - s)) * _dir(rng)); pt.append(nxt); nxt += 1
                elif name == "exact":
                    des.append(self.recon[nxt].copy()); pt.append(nxt); nxt += 1
                elif name == "dup":
                    p = g[3] if len(g) > 3 else P_GROUP
                    des.append(self.recon[p] + np.float32(np.sqrt(6.0 - g[2])) * d_grp); pt.append(p)
                elif name == "near":
                    des.append(self.recon[P_GROUP] + np.float32(np.sqrt(6.0 - g[2] + 2e-6 * j)) * d_grp); pt.append(P_GROUP)
                elif name == "bad":
                    des.append(unit[len(des)] * np.float32(g[2])); pt.append(-1)
                else:
                    d = self.recon[300 + j].copy()
                    if name == "nan": d[(7 * j) % 96] = np.nan
                    elif name == "inf": d[(11 * j) % 96] = -np.inf if j % 2 else np.inf
                    else: d[(13 * j) % 96] = np.float32(1500.0)
                    des.append(d); pt.append(-1)
                kind.append(name)
        n = len(des)
        assert nxt <= 300 and n <= 1000
        perm = rng.permutation(n)
        des = np.ascontiguousarray(np.stack(des)[perm], np.float32); kind = [kind[i] for i in perm]; pt = np.asarray(pt)[perm]
        lt = self.base.tex[0]
        x = lt.x[:n].copy(); y = lt.y[:n].copy(); ori = lt.ori[:n].copy()
        hi = pt >= 0
        for name in ("dup", "exact"):                               # tied rows: only the lower half (by row) lies where its rolled point lies, the upper half keeps a random place and
            rows = [i for i, k in enumerate(kind) if k == name]     # direction, so that WHICH of the tied rows are listed decides what survives S8b and S9
            hi[rows[(len(rows) + 1) // 2:]] = False
        x[hi] = np.clip(rt.x[pt[hi]] + 2, 0, 49); y[hi] = np.clip(rt.y[pt[hi]] - 1, 0, 49); ori[hi] = rt.ori[pt[hi]]
        return T.FPTemplate(minu=list(self.base.minu), tex=[T.TextureTemplate(x, y, ori, des=des)]), kind

    def expect(self, lat, kind):
        """n_in of the pair from the oracle's row maxima, with the margins of the module's docstring checked."""
        hl = self.oracle.latent(self.ocb, T.write_latent(lat))[0]
        ov, _ = self.oracle.texture_rowmax(self.ocb, hl, self.hr)
        forced = np.array([k in ("nan", "inf", "big") for k in kind])
        if len(kind) <= TOP:
            return hl, ov, len(kind)
        v = ov[~forced]
        assert len(v) >= TOP and np.isfinite(v).all()
        v200 = np.sort(v)[::-1][TOP - 1]
        below = v[v < v200 - NEAR]
        assert len(below) == 0 or below.max() < v200 - GAP, (v200, below.max())
        at = v[(v >= v200 - NEAR) & (v <= v200 + NEAR)]
        assert len(np.unique(at)) == 1 or len(np.unique(at)) == len(at), "the group at the 200th place: all equal (same bounds) or all distinct (near)"
        return hl, ov, int((v >= v200 - NEAR).sum() + forced.sum())

    def highest_rows_win(self, lat, ov):
        """The latent a kernel that kept the HIGHEST rows of a tie at the 200th place would in effect score: the tied rows' records (descriptor, place, direction) in reverse
        order over the rows they occupy, so that the oracle (lowest rows win) keeps the records of the highest rows.  None when no tie straddles the 200th place."""
        fin = np.where(np.isnan(ov), -np.inf, ov)
        v200 = np.sort(fin)[::-1][TOP - 1]
        tied = np.flatnonzero(ov == v200)
        if len(tied) <= TOP - int((fin > v200).sum()):
            return None
        lt = lat.tex[0]
        x, y, ori, des = lt.x.copy(), lt.y.copy(), lt.ori.copy(), lt.des.copy()
        x[tied] = lt.x[tied[::-1]]; y[tied] = lt.y[tied[::-1]]; ori[tied] = lt.ori[tied[::-1]]; des[tied] = lt.des[tied[::-1]]
        return T.FPTemplate(minu=list(lat.minu), tex=[T.TextureTemplate(x, y, ori, des=des)])

    def check(self, name, groups, seed, n_in, ties=None, signs=False, has_oracle=True, ref_tie=0, cut_decides=False):
        lat, kind = self.latent(groups, seed)
        hl, ov, want_n = self.expect(lat, kind)
        assert want_n == n_in, (name, want_n, n_in)
        if cut_decides:                                             # the case can tell a wrong tie-break: with the highest rows of the tie kept, the texture score is another
            wrong = self.highest_rows_win(lat, ov)
            assert wrong is not None, name
            hw = self.oracle.latent(self.ocb, T.write_latent(wrong))[0]
            s_right = self.oracle.pair(self.ocb, hl, self.hr, 1)[1][3]; s_wrong = self.oracle.pair(self.ocb, hw, self.hr, 1)[1][3]
            self.oracle.lib.orc_latent_free(hw)
            assert abs(float(s_right) - float(s_wrong)) > 1.0, (name, s_right, s_wrong)
        top = np.sort(ov[~np.isnan(ov)])[::-1][:TOP]
        if ties is not None:                                        # ties among the 200 best maxima are (or are not) really there
            assert (len(np.unique(top)) < len(top)) == ties, name
        if signs:
            assert top.max() > 0 and top.min() < 0, name
        m, oracle = self.m, self.oracle
        tie_mode = 9 if ref_tie == 2 else 1
        m.set_option("ref_tie_order", ref_tie)
        m.refine_stats()
        res = m.search([lat], k=0, want_parts=True)
        st = m.refine_stats()
        print("%-44s rows %4d  n_in %4d  %s" % (name, len(kind), n_in, st))
        assert st["pairs"] == 1 and st["rows"] == len(kind) and st["bound_violations"] == 0 and st["rows_evaluated"] == n_in, (name, st, n_in)
        got = res["parts"][0]
        assert _same_bits(got, m.search([lat], k=0, want_parts=True)["parts"][0]), name
        m.set_option("adc_variant", 0)                              # the direct exact kernel: dense row maxima, the kept S7
        dense = m.search([lat], k=0, want_parts=True)["parts"][0]
        m.set_option("adc_variant", 9)
        assert _same_bits(got, dense), (name, got, dense)
        if has_oracle:                                              # (a NaN row maximum: the reference's sort of NaN keys is undefined behaviour, there is no oracle value)
            want = np.asarray([oracle.pair(self.ocb, hl, self.hr, tie_mode)[1][:4]], np.float32)
            assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), (name, want, got)
            assert want[0, 3] > 0, name                             # the texture scorer finds something: the list matters
            w0 = oracle.trace(self.ocb, hl, self.hr, which=0, stage=0, tie_mode=tie_mode)
            g0 = m.debug_stage_list(lat, 0, 0, 0)
            assert len(w0[1]) == min(len(kind), TOP), name
            assert np.array_equal(g0[1], w0[1]) and np.array_equal(g0[2], w0[2]) and np.array_equal(g0[0].view(np.uint32), w0[0].view(np.uint32)), name
            if len(kind) > TOP:                                     # equal maxima: the lowest rows first, and at the 200th place the lowest rows kept
                sim, li = w0[0], w0[1]
                assert all(li[i] < li[i + 1] for i in range(len(li) - 1) if sim[i] == sim[i + 1]), name
                cut = np.flatnonzero(ov == sim[-1])
                if len(cut) > (sim == sim[-1]).sum():
                    assert set(li[sim == sim[-1]]) == set(cut[:(sim == sim[-1]).sum()]), name
        m.set_option("ref_tie_order", 0)
        oracle.lib.orc_latent_free(hl)


@pytest.fixture(scope="module")
def bench(codebook_bytes, oracle):
    b = Bench(codebook_bytes, oracle)
    b.open()
    yield b
    b.m.close()


HIGH = ("high", 150, 5.80, 5.98)
# name: (groups, n_in, ties among the 200, maxima of both signs)
CASES = {
    "200 rows: no S7":                          ([("high", 150, 5.80, 5.98), ("dup", 50, 5.5)], 200, None, False),
    "201 rows, all passed on":                  ([HIGH, ("dup", 51, 5.5)], 201, True, False),
    "201 rows, n_in 200, no ties":              ([("high", 200, 5.70, 5.98), ("bad", 1, 1.0)], 200, False, False),
    "n_in 200, no ties":                        ([("high", 200, 5.70, 5.98), ("bad", 130, 1.0)], 200, False, False),
    "n_in 201, ties straddle the 200th place":  ([HIGH, ("dup", 51, 5.5), ("bad", 99, 1.0)], 201, True, False),
    "n_in 255, ties inside and at the cut":     ([("high", 140, 5.80, 5.98), ("exact", 10), ("dup", 105, 5.5), ("bad", 60, 1.0)], 255, True, False),
    "n_in 256, one tied row kept":              ([("high", 199, 5.70, 5.98), ("dup", 57, 5.5), ("bad", 70, 1.0)], 256, False, False),
    "n_in 256, no ties":                        ([HIGH, ("near", 106, 5.5), ("bad", 44, 1.0)], 256, False, False),
    "n_in 255, no ties":                        ([HIGH, ("near", 105, 5.5), ("bad", 77, 1.0)], 255, False, False),
    "n_in 257: the kept path":                  ([HIGH, ("dup", 107, 5.5), ("bad", 50, 1.0)], 257, True, False),
    "n_in 257, no ties: the kept path":         ([HIGH, ("near", 107, 5.5), ("bad", 50, 1.0)], 257, False, False),
    "all n_in maxima equal":                    ([("exact", 230), ("bad", 90, 1.0)], 230, True, False),
    "n_in 201, all equal, distinct points":     ([("exact", 201), ("bad", 60, 1.0)], 201, True, False),
    "n_in 255, all equal, distinct points":     ([("exact", 255), ("bad", 60, 1.0)], 255, True, False),
    "n_in 256, all equal, distinct points":     ([("exact", 256), ("bad", 60, 1.0)], 256, True, False),
    "n_in 257, all equal: the kept path":       ([("exact", 257), ("bad", 60, 1.0)], 257, True, False),
    "maxima of both signs":                     ([("high", 120, 5.80, 5.98), ("dup", 100, -1.0), ("bad", 80, 4.0)], 220, True, True),
    "1000 rows, n_in 600":                      ([("high", 100, 5.80, 5.98), ("dup", 500, 5.5), ("bad", 400, 1.0)], 600, True, False),
    "forced rows of -inf and beyond 1000":      ([HIGH, ("dup", 60, 5.5), ("inf", 3), ("big", 2), ("bad", 85, 1.0)], 215, True, False),
}
# the cases in which WHICH rows of a tie at the 200th place are listed decides the texture score (asserted on the CPU before the GPU runs: Bench.check, cut_decides)
CUT_DECIDES = {"n_in 255, ties inside and at the cut", "n_in 256, one tied row kept", "n_in 257: the kept path", "all n_in maxima equal", "1000 rows, n_in 600",
               "n_in 201, all equal, distinct points", "n_in 255, all equal, distinct points", "n_in 256, all equal, distinct points", "n_in 257, all equal: the kept path"}


@pytest.mark.parametrize("name", list(CASES))
def test_s7_list_at_the_edges_of_the_compact_path(bench, name):
    """n_lt 200 (no S7) and 201; n_in 200, 201, 255, 256 (compact path) and 257, 600 (kept path); equal maxima inside the 200, straddling the 200th place (the lowest
    slots win), all n_in equal, none equal; maxima of both signs; rows of -inf.  (In "n_in 256, one tied row kept" the 199 distinct maxima take ranks 0 .. 198 and ONE of 57
    equal rows is kept at rank 199: the 200 best are distinct, the tie is among the n_in.)  The cases of CUT_DECIDES tell a wrong choice among the tied rows by their score."""
    groups, n_in, ties, signs = CASES[name]
    bench.check(name, groups, seed=sum(map(ord, name)), n_in=n_in, ties=ties, signs=signs, cut_decides=name in CUT_DECIDES)


def test_s7_with_nan_rows(bench):
    """Rows with a NaN component (every similarity NaN: the key above every number) next to rows of -inf: no oracle value; the compact path, the same search twice and the
    dense form through the kept S7 agree bit for bit, NaN for NaN."""
    bench.check("forced rows of NaN and -inf", [HIGH, ("dup", 60, 5.5), ("nan", 3), ("inf", 2), ("bad", 85, 1.0)], seed=5, n_in=215, has_oracle=False)


@pytest.mark.parametrize("name", ["n_in 200, no ties", "n_in 256, no ties", "n_in 257, no ties: the kept path"])
def test_s7_with_the_reference_tie_order(bench, name):
    """Option ref_tie_order 2 (k_graph_texture<1>) against the oracle's tie mode 9.  The option covers S8 and S9; at S7 the device orders equal maxima by row, so the cases
    are the ones without equal maxima."""
    groups, n_in, ties, signs = CASES[name]
    bench.check(name + ", ref_tie_order 2", groups, seed=sum(map(ord, name)), n_in=n_in, ties=ties, signs=signs, ref_tie=2)


def test_s7_paths_mixed_in_one_search(bench, codebook_bytes, oracle):
    """Three latents (n_in 257, 230 all equal, 256) against 16 templates in one search: a wave that draws tasks of both paths one after the other.  Against the crafted
    template the latents have the n_in above; against the random ones, whatever the bounds give.  Scores against the oracle, and the dense form."""
    rng = np.random.default_rng(77)
    gal = [S.make_rolled(rng, bench.cb, n_tex=int(n)) for n in rng.integers(250, 600, 7)] + [bench.rolled] + [S.make_rolled(rng, bench.cb, n_tex=int(n)) for n in rng.integers(1, 300, 8)]
    lats = [bench.latent(CASES[k][0], seed=i)[0] for i, k in enumerate(("n_in 257: the kept path", "all n_in maxima equal", "n_in 256, no ties"))]
    m = M.Matcher(codebook_bytes, taps=True)
    m.set_option("adc_variant", 9); m.set_option("mf_stats", 1)
    m.gallery_add(gal); m.gallery_commit(0)
    m.refine_stats()
    res = m.search(lats, k=0, want_parts=True)
    st = m.refine_stats()
    print("mixed search:", st)
    assert st["pairs"] == len(lats) * len(gal) and st["bound_violations"] == 0 and st["rows_evaluated"] >= TOP * st["pairs"], st
    m.set_option("adc_variant", 0)
    dense = m.search(lats, k=0, want_parts=True)
    assert _same_bits(res["parts"], dense["parts"]) and _same_bits(res["scores"], dense["scores"])
    hr = [oracle.rolled(T.write_rolled(g))[0] for g in gal]
    for qi, L in enumerate(lats):
        hl = oracle.latent(bench.ocb, T.write_latent(L))[0]
        rc, sc, parts = oracle.search(bench.ocb, hl, hr, tie_mode=1, want_parts=True)
        got = np.concatenate([res["parts"][qi], res["scores"][qi][:, None]], axis=1)
        assert rc == 0 and np.array_equal(got.view(np.uint32), parts.astype(np.float32).view(np.uint32)), qi
        oracle.lib.orc_latent_free(hl)
    m.close()
