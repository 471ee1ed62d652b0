"""Seeded test cases shared by the CPU (oracle/golden) and GPU (parity) tests."""
import importlib

import numpy as np

T = importlib.import_module("msu-latentafis_amd.host.templates")
S = importlib.import_module("msu-latentafis_amd.host.synth")


def small_set(cb, seed=1, n_lat=3, n_gal=40, tex_lo=230, tex_hi=420, rolled_tex=(300, 520)):
    """n_lat latents, n_gal rolled templates; gallery entries 0..: mates of decreasing overlap for each latent, rest random."""
    rng = np.random.default_rng(seed)
    lats = [S.make_latent(rng, n_tex_lo=tex_lo, n_tex_hi=tex_hi) for _ in range(n_lat)]
    gal = []
    for q, L in enumerate(lats):
        for frac in (0.8, 0.5, 0.3):
            gal.append(S.make_mate(rng, cb, L, frac=frac, n_tex=int(rng.integers(*rolled_tex))))
    while len(gal) < n_gal:
        gal.append(S.make_rolled(rng, cb, n_tex=int(rng.integers(*rolled_tex))))
    return lats, gal[:n_gal]


def edge_latents(cb, seed=7):
    """Latents exercising the template-selection / fusion rules of matcher.cpp:376-417 and :188."""
    rng = np.random.default_rng(seed)
    base = S.make_latent(rng, n_tex_lo=210, n_tex_hi=260)
    out = {"full28": base}
    def clone(n_minu=None, tex=True, drop_pool=False):
        t = T.FPTemplate(minu=list(base.minu if n_minu is None else base.minu[:n_minu]), tex=list(base.tex) if tex else [])
        t._pool = base._pool
        return t
    out["minu27_tex"] = clone(27)            # texture lands at score[27], score[28] is out of range -> weight 0
    out["minu29_tex"] = clone(28)
    out["minu29_tex"].minu = out["minu29_tex"].minu + [base.minu[0]]   # 29 templates: score[28] is a minutiae slot = 0
    out["minu12_tex"] = clone(12)            # only selected templates 2 and 11 exist
    out["minu2_tex"] = clone(2)              # texture lands at score[2] with weight 1
    out["minu0_tex"] = clone(0)              # texture lands at score[0]
    out["minu28_notex"] = clone(28, tex=False)
    out["minu26_notex"] = clone(26, tex=False)   # latent "empty": status 1
    out["small_tex"] = clone(28)             # fewer than 200 texture rows: no top-N sort, rows in index order
    st = out["small_tex"].tex[0]
    out["small_tex"].tex = [T.TextureTemplate(st.x[:150].copy(), st.y[:150].copy(), st.ori[:150].copy(), des=st.des[:150].copy())]
    return base, out


def to_orc(orc, ocb, lats, gal):
    hl = [orc.latent(ocb, T.write_latent(L))[0] for L in lats]
    hr = [orc.rolled(T.write_rolled(R))[0] for R in gal]
    return hl, hr


# ---- inputs of the checks against the reference's own header, argparser and JSON library (tests/test_oracle.py); their outputs on these
# inputs are recorded in tests/golden/golden_ref.json by tests/golden/make_golden_ref.py ----
REF_ARG_LINES = [["-l", "a.dat", "-g", "gal/", "-s", "out/", "-c", "cb.dat"], ["-g", "gal", "-l"], ["-l", "-g", "x"], ["-s", "1", "-s", "2"],
                 [], ["-ldir", "d", "-l", "f"], ["-c"], ["--c", "x", "-c", "y"]]
REF_ARG_OPTS = ["-l", "-ldir", "-g", "-s", "-c", "-d"]
REF_CONFIG_KEYS = ["CodebookPath", "ScorePath", "GalleryTemplateDirectory", "LatentTemplateDirectory", "MinuPath", "Absent"]
REF_CONFIG_TEXTS = [
    '{\n\t"CodebookPath": "/home/x/codebook.dat",\n\t"ScorePath": "/home/x/scores",\n\n\t"GalleryTemplateDirectory": "/g",\n'
    '\t"LatentTemplateDirectory": "/l",\n\t"MinuPath": "None"\n\n}\n',
    '{"ScorePath":"a b/c",   "CodebookPath" :\n "q\\\\r\\"s" , "Depth": 3, "Flag": true, "GalleryTemplateDirectory": "/g/"}',
    '{ "LatentTemplateDirectory": "", "ScorePath": "/s/", "Nested": {"CodebookPath": "inner"}, "List": ["x", "y"] }',
]


def ref_lut_descriptors(cb):
    """37 latent texture descriptors for the S4 look-up table; row 3 is made of exact codewords (zero distances)."""
    rng = np.random.default_rng(5)
    des = (rng.standard_normal((37, 96)) * 0.2).astype(np.float32)
    des[3] = np.concatenate([cb.words[m, (7 * m) % 256] for m in range(16)])
    return des


def ref_rolled_template():
    """A rolled template of 23 texture points with random PQ codes (and 5 minutiae, so that the writer emits the texture block)."""
    rng = np.random.default_rng(6)
    n = 23
    return T.FPTemplate(minu=[T.MinutiaeTemplate(np.arange(5, dtype=np.int16), np.arange(5, dtype=np.int16), np.zeros(5, np.float32), np.ones((5, 96), np.float32))],
                        tex=[T.TextureTemplate(rng.integers(0, 45, n).astype(np.int16), rng.integers(0, 47, n).astype(np.int16),
                                               rng.uniform(-1, 1, n).astype(np.float32), codes=rng.integers(0, 256, (n, 16)).astype(np.uint8))])
