"""GPU parity on codebooks other than the shipped one: every check of the texture path and the encoder repeated over tests/cases.py's codebook family
(scaled into fp16's subnormals and up to fp16 ulps of 0.5, components beyond fp16's range, exact copies, fp16 twins, a constant sub-quantizer, every
component just under half an fp16 ulp from its rounding).

The exactness of adc_variant 9 rests on error terms derived from the codewords (k_mf_rows: Q from their fp16 rounding, N from their norms, the widening of
k_tex_refine's bounds) and the encoders' tie rules on codewords that are equal or all but equal.  Each leg compares the HIP path, through the C ABI, with the oracle
(and the encoder with scipy's vq, tests/golden/golden_pq_codebooks.npz) bit for bit; NaN counts as equal to NaN.
"""
import ctypes as C
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")
M = importlib.import_module("msu-latentafis_amd.host.matcher")
HERE = os.path.dirname(os.path.abspath(__file__))


def _same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.fixture(scope="module")
def base(codebook_bytes):
    return T.Codebook.from_bytes(codebook_bytes)


@pytest.fixture(scope="module")
def family_pq():
    return np.load(os.path.join(HERE, "golden", "golden_pq_codebooks.npz"))


def _latent_with(des, minu_from):
    n = des.shape[0]
    x = (np.arange(n) % 45).astype(np.int16); y = (np.arange(n) // 45 % 47).astype(np.int16)
    return T.FPTemplate(minu=list(minu_from.minu), tex=[T.TextureTemplate(x, y, np.linspace(-1.5, 1.5, n).astype(np.float32), des=np.ascontiguousarray(des, np.float32))])


@pytest.mark.parametrize("name", cases.CODEBOOK_FAMILY)
def test_lut_and_encoder_on_the_family(name, base, oracle, family_pq):
    """S4 (k_lut_reference_layout) against the oracle; the encoder (k_pq_encode) against vq's codes and the oracle, at tile remainders and beyond 64 x 256 points
    (the persistent tile loop runs more than once per workgroup), on NaN / inf components, and through encode_rolled_dat and gallery_add of fp32 descriptors."""
    cb = cases.family_codebook(name, base)
    buf = cb.to_bytes()
    m = M.Matcher(buf, taps=True)
    ocb = oracle.codebook(buf)
    rng = np.random.default_rng(60 + cases.CODEBOOK_FAMILY.index(name))
    filler = S.make_latent(rng, n_tex_lo=10, n_tex_hi=10)
    dl = cases.family_lut_descriptors(name, base)
    assert _same_bits(m.debug_lut(_latent_with(dl, filler)), oracle.build_lut(ocb, dl))
    des = cases.family_encoder_descriptors(name, base)
    want = family_pq["codes_" + name]
    got = m.pq_encode(des)
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8].tolist())
    assert np.array_equal(oracle.pq_encode(ocb, des), want)
    s = np.float32(cases.CODEBOOK_SCALE[name])
    for n in (1, 63, 64, 65, 64 * 256 + 777):
        d = np.resize(des, (n, 96)).copy()
        d[1::3] = (rng.standard_normal((len(d[1::3]), 96)) * 0.2 * s).astype(np.float32)
        assert np.array_equal(m.pq_encode(d), oracle.pq_encode(ocb, d)), (name, n)
    bad = des[:12].copy()
    bad[0, 0] = np.nan; bad[1, :6] = np.inf; bad[2, 7] = -np.inf; bad[3, :] = np.nan; bad[4, 50] = np.inf; bad[4, 51] = -np.inf
    bad[5, 90] = 3e38; bad[6, 13] = -3e38; bad[7, :] = 1e-42
    assert np.array_equal(m.pq_encode(bad), oracle.pq_encode(ocb, bad)), name
    src = _latent_with(des, filler)
    src = T.FPTemplate(minu=src.minu[:1], tex=src.tex)
    rc, out = m.encode_rolled_dat(T.write_latent(src))
    rrc, R = T.read_rolled(out)
    assert rc == 0 and rrc == 0 and np.array_equal(R.tex[0].codes, want)
    lat = S.make_latent(rng)
    m2 = M.Matcher(buf); m2.gallery_add([R]); m2.gallery_commit(0)
    m3 = M.Matcher(buf); m3.gallery_add([src]); m3.gallery_commit(0)
    assert _same_bits(m2.search([lat], k=0, want_parts=True)["parts"], m3.search([lat], k=0, want_parts=True)["parts"])
    m2.close(); m3.close(); m.close()


@pytest.fixture(scope="module")
def family_sets(base):
    return {name: cases.family_set(name, base) for name in cases.CODEBOOK_FAMILY}


@pytest.mark.parametrize("name", cases.CODEBOOK_FAMILY)
def test_row_maxima_and_bounds_on_the_family(name, family_sets, oracle):
    """S5 / S6 row maxima and first arg-maxima of adc_variant 9 (matrix-core bound pass + exact recomputation), 8 (16-bit table bound pass) and 7 (direct kernel)
    against the oracle, for rolled templates of 1, 33, 640 and 1 000+ points, planted mates and (duplicates, fp16_twins) templates whose codes use the LATER copy
    or twin of a row's best codeword; the bound pass's self-check silent (every exact maximum inside its bounds) for every member."""
    cb, lats, gal = family_sets[name]
    buf = cb.to_bytes()
    m = M.Matcher(buf, taps=True)
    m.gallery_add(gal); m.gallery_commit(0)
    ocb = oracle.codebook(buf)
    hl, hr = cases.to_orc(oracle, ocb, lats, gal)
    want = {(qi, g): oracle.texture_rowmax(ocb, hl[qi], hr[g]) for qi in range(len(lats)) for g in range(len(gal))}
    m.set_option("mf_stats", 1)
    for v in (9, 8, 7):
        m.set_option("adc_variant", v)
        m.refine_stats()
        for (qi, g), (ov, oa) in want.items():
            val, arg = m.debug_texture_rowmax(lats[qi], g)
            assert _same_bits(val, ov), (name, v, qi, g, np.argwhere(val.view(np.uint32) != ov.view(np.uint32))[:6].ravel())
            assert np.array_equal(arg, oa), (name, v, qi, g, np.argwhere(arg != oa)[:6].ravel())
        if v == 9:
            st = m.refine_stats()
            assert st["bound_violations"] == 0 and st["rows_evaluated"] == st["rows"] > 0, (name, st)
            if name == "overflow":                       # codewords beyond fp16 make every row's bound infinite: every row is evaluated over every point
                assert st["rows_evaluated_in_full"] == st["rows"], st
    # the search itself (rows that cannot reach a pair's top 200 are skipped): what the bound pass did, per member
    m.set_option("adc_variant", 9); m.refine_stats()
    m.search(lats, k=0)
    st = m.refine_stats()
    assert st["bound_violations"] == 0, (name, st)
    print("REFINE_STATS " + json.dumps({"member": name, **st}))
    m.close()


def _create_from_floats(words):
    """A Matcher whose context comes from afis_create on raw floats (not from the codebook file's bytes)."""
    m = M.Matcher.__new__(M.Matcher)
    m.lib = M.load_library(M.LIB_PATH); m.has_taps = False; m.gallery_files = []
    m.ctx = C.c_void_p()
    w = np.ascontiguousarray(words, np.float32)
    rc = m.lib.afis_create(C.byref(m.ctx), w.ctypes.data_as(C.POINTER(C.c_float)), 16, 256, 6, 0)
    assert rc == 0, m.lib.afis_last_error(None)
    return m


@pytest.mark.parametrize("name", cases.CODEBOOK_FAMILY)
def test_pair_scores_on_the_family(name, family_sets, oracle):
    """Pair scores and per-part scores of the default search against the oracle (tie_mode 1), and with option ref_tie_order 2 against tie_mode 9, bit for bit;
    afis_create on raw floats and afis_create_from_codebook on the file's bytes give the same bits."""
    cb, lats, gal = family_sets[name]
    buf = cb.to_bytes()
    m = M.Matcher(buf)
    m.gallery_add(gal); m.gallery_commit(0)
    ocb = oracle.codebook(buf)
    hl, hr = cases.to_orc(oracle, ocb, lats, gal)
    for opt, tm in ((0, 1), (2, 9)):
        m.set_option("ref_tie_order", opt)
        res = m.search(lats, k=0, want_parts=True)
        for qi in range(len(lats)):
            rc, sc, parts = oracle.search(ocb, hl[qi], hr, tie_mode=tm, want_parts=True)
            assert rc == 0
            got = np.concatenate([res["parts"][qi], res["scores"][qi][:, None]], axis=1)
            assert _same_bits(got, parts), (name, opt, qi, np.argwhere(got.view(np.uint32) != parts.view(np.uint32))[:6].tolist())
        if opt == 0:
            base_res = res
            assert (res["parts"][0, :2, :3] > 0).all(), (name, res["parts"][0, :2])       # the planted mates' minutiae score (the texture part is 6 - distance: at
                                                                                          # large scales it is a large negative number, the reference's arithmetic)
    m.set_option("ref_tie_order", 0)
    mf = _create_from_floats(cb.words)
    mf.gallery_add(gal); mf.gallery_commit(0)
    rf = mf.search(lats, k=0, want_parts=True)
    assert _same_bits(rf["parts"], base_res["parts"]) and _same_bits(rf["scores"], base_res["scores"])
    mf.close(); m.close()


def test_cli_with_a_retrained_codebook_file(family_sets, oracle, tmp_path):
    """The drop-in path with `-c` naming a codebook other than the shipped one (the large member, sims in the thousands): `match -l` ranks and prints what the oracle scores."""
    exe = os.path.join(os.path.dirname(M.LIB_PATH), "match")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(M.LIB_PATH), "match"], check=True)
    cb, lats, gal = family_sets["large"]
    for d in ("work", "gal", "lat", "out"):
        (tmp_path / d).mkdir()
    cbp = tmp_path / "large.dat"; cbp.write_bytes(cb.to_bytes())
    for j, g in enumerate(gal):
        (tmp_path / "gal" / f"R{j:03d}.dat").write_bytes(T.write_rolled(g))
    (tmp_path / "lat" / "L0.dat").write_bytes(T.write_latent(lats[0]))
    out = subprocess.run([exe, "-l", str(tmp_path / "lat" / "L0.dat"), "-g", str(tmp_path / "gal"), "-s", str(tmp_path / "out") + "/", "-c", str(cbp)],
                         capture_output=True, text=True, cwd=tmp_path / "work")
    assert out.returncode == 0, out.stderr
    lines = (tmp_path / "out" / "L0.csv").read_text().splitlines()
    assert lines[0] == "filename,score" and len(lines) == 1 + len(gal)
    ocb = oracle.codebook(cb.to_bytes())
    hl, _ = oracle.latent(ocb, T.write_latent(lats[0]))
    got = []
    for line in lines[1:]:
        path, score = line.split('"')[1], line.rsplit(",", 1)[1]
        hr, _ = oracle.rolled(open(path, "rb").read())
        rc, want = oracle.pair(ocb, hl, hr, 1)
        assert rc == 0 and score == "%g" % float(want[4]), (line, want)
        got.append(float(want[4]))
    assert got == sorted(got, reverse=True) and min(got) < -1000                     # ranked by the oracle's scores; the mates' texture parts at this scale
