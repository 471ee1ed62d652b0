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


# ---- a family of codebooks (tests/test_gpu_codebooks.py, the codebook checks of tests/test_oracle.py and tests/test_host.py): every member is made from the
# shipped file by scaling, copying and editing entries, so no further codebook is committed; tests/golden/golden_ref.json records each member's sha256 ----
SHIPPED_CODEBOOK = "codebook_EmbeddingSize_96_stride_16_subdim_6.dat"
CODEBOOK_SCALE = {"shipped": 1.0, "tiny": 3e-4, "large": 37.5, "huge": 1500.0, "overflow": 1.0, "duplicates": 1.0, "fp16_twins": 1.0, "flat": 1.0, "halfulp": 1.0}
CODEBOOK_FAMILY = list(CODEBOOK_SCALE)
DUPLICATE_SLOTS = [(s, 128 + s) for s in range(32)] + [(3, 255), (100, 254)]    # (earlier slot, later exact copy) in every sub-quantizer
TWIN_SLOTS = [(40 + s, 168 + s) for s in range(32)]                                         # (earlier slot, its fp16 twin): equal in fp16, 1 ulp apart in fp32
OVERFLOW_ENTRIES = [(2, 17, 3, 7e4), (2, 200, 0, -7e4), (2, 201, 5, 7e4), (9, 5, 5, 7e4), (9, 5, 1, -7e4)]   # (sub-quantizer, slot, component, value beyond fp16)
FLAT_SUBQ = 11


def shipped_codebook():
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", SHIPPED_CODEBOOK), "rb") as f:
        return T.Codebook.from_bytes(f.read())


def family_codebook(name, base=None):
    """Member `name` of the family (a T.Codebook).  tiny (x 3e-4) puts 77 % of the entries among fp16's subnormals; large and huge scale the similarities
    into the thousands and millions; overflow has components beyond fp16's range; duplicates / fp16_twins / flat plant exact and fp16-level ties; halfulp
    maximises the codewords' fp16 rounding error, all of one sign."""
    w = (base or shipped_codebook()).words.copy()
    s = CODEBOOK_SCALE[name]
    if s != 1.0:
        w = (w * np.float32(s)).astype(np.float32)
    if name == "overflow":
        for m, k, d, v in OVERFLOW_ENTRIES:
            w[m, k, d] = np.float32(v)
    elif name == "duplicates":
        for a, b in DUPLICATE_SLOTS:
            w[:, b] = w[:, a]
    elif name == "fp16_twins":
        for a, b in TWIN_SLOTS:
            t = w[:, a].copy()
            for m in range(w.shape[0]):
                d = (a + m) % 6
                for direction in (np.inf, -np.inf):                 # one fp32 ulp away, the fp16 rounding unchanged
                    x = np.nextafter(t[m, d], np.float32(direction)).astype(np.float32)
                    if np.float16(x) == np.float16(t[m, d]):
                        t[m, d] = x
                        break
            w[:, b] = t
    elif name == "flat":
        w[FLAT_SUBQ] = 0.0
    elif name == "halfulp":                                          # every component just under half an fp16 ulp ABOVE its fp16 rounding: with latent rows
        h = w.astype(np.float16)                                     # that are positive and exact in fp16 (family_set), the bound pass's whole error is the
        gap = np.nextafter(h, np.float16(np.inf)).astype(np.float32) - h.astype(np.float32)     # codewords' rounding, all of one sign (its Q term)
        v = (h.astype(np.float32) + np.float32(0.499) * gap).astype(np.float32)
        w = np.where(v.astype(np.float16) == h, v, w).astype(np.float32)
    return T.Codebook(np.ascontiguousarray(w, np.float32))


def family_lut_descriptors(name, base=None):
    """ref_lut_descriptors for a member: the shipped rows scaled by the member's factor, row 3 the member's own exact codewords."""
    base = base or shipped_codebook()
    des = (ref_lut_descriptors(base) * np.float32(CODEBOOK_SCALE[name])).astype(np.float32)
    cb = family_codebook(name, base)
    des[3] = np.concatenate([cb.words[m, (7 * m) % 256] for m in range(16)])
    return des


def family_encoder_descriptors(name, base=None):
    """128 descriptors for the encoder checks: 48 exact codewords (for duplicates / fp16_twins: of the LATER copy or twin, and of the earlier one),
    40 exact fp32 midpoints of two codewords, 40 ordinary unit-norm rows (norm 1.73) scaled to the member."""
    cb = family_codebook(name, base)
    rng = np.random.default_rng(4000 + CODEBOOK_FAMILY.index(name))
    pairs = DUPLICATE_SLOTS if name == "duplicates" else TWIN_SLOTS if name == "fp16_twins" else None
    slots = rng.integers(0, 256, (48, 16))
    if pairs is not None:
        pick = np.array(pairs)[rng.integers(0, len(pairs), (48, 16))]
        slots = np.where((np.arange(48) % 3 == 2)[:, None], pick[..., 0], pick[..., 1])        # two in three rows: the later copy / twin
    exact = np.stack([np.concatenate([cb.words[m, slots[i, m]] for m in range(16)]) for i in range(48)])
    i, j = rng.integers(0, 256, (2, 40, 16))
    mid = np.stack([np.concatenate([(cb.words[m, i[r, m]] + cb.words[m, j[r, m]]) * np.float32(0.5) for m in range(16)]) for r in range(40)])
    unit = rng.standard_normal((40, 96))
    unit = unit / np.linalg.norm(unit, axis=1, keepdims=True) * T.DESCRIPTOR_NORM * CODEBOOK_SCALE[name]
    return np.ascontiguousarray(np.concatenate([exact, mid, unit]).astype(np.float32))


def family_set(name, base=None, seed=31):
    """(member codebook, latents, gallery) for the texture and pair checks: 2 latents x 12 rolled templates, planted mates first.  For scaled members the
    latents' texture descriptors are scaled by the member's factor (so the planted mates stay mates: scaling does not move a nearest codeword), and a third,
    unscaled latent sits far from every codeword.  For halfulp the latents' texture descriptors are positive and exact in fp16.

    For duplicates / fp16_twins the last two templates plant TIED row maxima: for rows of the first latent whose best code vector names a codeword with a
    later copy / twin, two adjacent points carry that vector once through the earlier slots' bytes and once through the later ones' (the same codewords, or
    codewords equal in fp16), in both orders; the rest of the template is a mate.  Such a template records its plan in `_pairs`: rows of
    (latent row, first point, second point, 1 if the later bytes come first)."""
    base = base or shipped_codebook()
    cb = family_codebook(name, base)
    s = CODEBOOK_SCALE[name]
    rng = np.random.default_rng(seed)
    lats = [S.make_latent(rng, n_tex_lo=300, n_tex_hi=360) for _ in range(2)]
    if name == "halfulp":
        for L in lats:
            L.tex[0].des = np.abs(L.tex[0].des).astype(np.float16).astype(np.float32)
    enc_cb = base if s != 1.0 else cb
    gal = []
    for L in lats:
        for frac, n in ((0.8, 640), (0.5, 1000)):
            gal.append(S.make_mate(rng, enc_cb, L, frac=frac, n_tex=n))
    for n in (1, 33, 640, 1200, 700, 500):
        gal.append(S.make_rolled(rng, cb, n_tex=n))
    pairs = DUPLICATE_SLOTS if name == "duplicates" else TWIN_SLOTS if name == "fp16_twins" else None
    if pairs is not None:
        earlier = np.arange(256); later = np.arange(256)
        for a, b in pairs:
            earlier[b] = a; later[a] = b
        early = earlier[cb.encode(lats[0].tex[0].des)]              # each row's best code vector through the earlier slots' bytes ...
        late = later[early]                                          # ... and through the later copies' / twins'
        rows = np.flatnonzero((late != early).any(axis=1))
        for t, (n, sel) in enumerate(((640, rows[:len(rows) // 2]), (1000, rows[len(rows) // 2:][::-1]))):
            r = S.make_mate(rng, cb, lats[0], frac=0.7, n_tex=n)
            c = r.tex[0].codes
            plan = []
            for i, row in enumerate(sel[:n // 2]):
                late_first = (i + t) % 2
                c[2 * i], c[2 * i + 1] = (late[row], early[row]) if late_first else (early[row], late[row])
                plan.append((int(row), 2 * i, 2 * i + 1, late_first))
            r._pairs = np.array(plan, np.int64)
            gal.append(r)
    gal = gal[:12]
    if s != 1.0:
        for L in lats:
            L.tex[0].des = (L.tex[0].des * np.float32(s)).astype(np.float32)
        lats.append(S.make_latent(rng, n_tex_lo=300, n_tex_hi=360))
    return cb, lats, gal


def reference_similarities(lut_row, codes):
    """matcher.cpp:571-592 on one latent row's table [16][256] and code vectors [n][16]: four chains from 6 / 0 / 0 / 0, chain c subtracting the entries of
    sub-quantizers c, c + 4, c + 8, c + 12 in that order, met as (d0 + d1) + (d2 + d3); every operation rounded to fp32."""
    codes = np.asarray(codes)
    d = [np.full(len(codes), 6.0, np.float32)] + [np.zeros(len(codes), np.float32) for _ in range(3)]
    for mg in range(4):
        for c in range(4):
            m = 4 * mg + c
            d[c] = (d[c] - lut_row[m][codes[:, m]]).astype(np.float32)
    return ((d[0] + d[1]).astype(np.float32) + (d[2] + d[3]).astype(np.float32)).astype(np.float32)


# ---- inputs that several tests share and that tests/golden/make_golden_matcher_ref.py runs through the reference's own matcher.cpp ----
# Each function takes its seed as a parameter; the defaults are the seeds the GPU parity tests have always used.
def _SS():
    return importlib.import_module("msu-latentafis_amd.host.synth_structured")


STRUCTURED_CONFIGS = ((10, 4, 30, 0.3, None), (30, 2, 40, 1.0, 0.0057))      # (share of repeated code vectors in %, latents, gallery, identity weight, sigma or None = DUP_SIGMA)


def structured_set(cb, dup, n_lat, n_gal, identity_weight, sigma=None, seed=None):
    """One configuration of the structured sweep (host/synth_structured.py): latents, gallery (mates of latent q at 2q and 2q + 1, then non-mates)."""
    SS = _SS()
    sg = SS.DUP_SIGMA[dup] if sigma is None else sigma
    keep = SS.IDENTITY_WEIGHT
    SS.IDENTITY_WEIGHT = identity_weight
    try:
        rng = np.random.default_rng(600 + dup if seed is None else seed)
        lats = [SS.make_structured_latent(rng, sigma=sg) for _ in range(n_lat)]
        gal = [SS.make_structured_mate(rng, cb, L, frac=f, sigma=sg) for L in lats for f in (0.8, 0.3)]
        while len(gal) < n_gal: gal.append(SS.make_structured_rolled(rng, cb, sigma=sg))
    finally:
        SS.IDENTITY_WEIGHT = keep
    return lats, gal


def edge_shapes_set(cb, seed=42):
    """Shapes off the fast paths: > 64 latent / > 128 rolled minutiae, texture templates above the 1000-point clamp, tiny templates, duplicated points."""
    rng = np.random.default_rng(seed)
    big = S.make_latent(rng, n_tex_lo=1100, n_tex_hi=1200, n_minu_lo=90, n_minu_hi=110)        # texture > 1000 rows, minutiae > 64
    tiny = S.make_latent(rng, n_tex_lo=40, n_tex_hi=60, n_minu_lo=3, n_minu_hi=6)
    dup = S.make_latent(rng, n_tex_lo=230, n_tex_hi=260)
    t0 = dup.tex[0]
    t0.x[50:100] = t0.x[0:50]; t0.y[50:100] = t0.y[0:50]; t0.des[50:100] = t0.des[0:50]; t0.ori[50:100] = t0.ori[0:50]   # exact duplicates
    lats = [big, tiny, dup]
    gal = []
    for L in lats:
        gal.append(S.make_mate(rng, cb, L, frac=0.8, n_minu=min(300, max(8, len(L._pool[0]) * 3)), n_tex=1300 if L is big else 500))
        gal.append(S.make_mate(rng, cb, L, frac=0.4, n_minu=150, n_tex=700))
    gal.append(S.make_rolled(rng, cb, n_minu=5, n_tex=30))
    gal.append(S.make_rolled(rng, cb, n_minu=260, n_tex=1900))
    return lats, gal


def degenerate_key_pairs(cb, seed=5):
    """(latent, rolled) pairs whose S3 keys are degenerate for latent template 26: (a) fewer than 120 non-zero similarities, (b) every similarity identical,
    (c) a few levels with large blocks of exact ties straddling the 120th place."""
    rng = np.random.default_rng(seed)
    base = S.make_latent(rng)
    d = rng.standard_normal(96).astype(np.float32); d *= np.float32(1.73) / np.linalg.norm(d)
    e = rng.standard_normal(96).astype(np.float32); e -= d * (e @ d) / (d @ d); e *= np.float32(1.73) / np.linalg.norm(e)     # orthogonal to d

    def latent_with(des_rows):
        L = T.FPTemplate(minu=list(base.minu), tex=list(base.tex))
        n = len(des_rows)
        L.minu[26] = T.MinutiaeTemplate(rng.integers(50, 700, n).astype(np.int16), rng.integers(50, 700, n).astype(np.int16),
                                        rng.uniform(-3, 3, n).astype(np.float32), np.stack(des_rows).astype(np.float32))
        return L

    def rolled_with(des_rows):
        n = len(des_rows)
        R = S.make_rolled(rng, cb, n_minu=n, n_tex=300)
        R.minu[0] = T.MinutiaeTemplate(R.minu[0].x, R.minu[0].y, R.minu[0].ori, np.stack(des_rows).astype(np.float32))
        return R

    return [
        (latent_with([d] * 30), rolled_with([-d] * 37 + [d] * 3)),                      # (a) 90 non-zero of 1200
        (latent_with([d] * 32), rolled_with([d] * 40)),                                  # (b) 1280 identical keys
        (latent_with([d] * 10 + [e] * 22), rolled_with([d] * 10 + [0.5 * d + 0.5 * e] * 30)),   # (c) a few levels, large tie blocks
    ]


PACKED_PATH_OFFSETS = ((0, 0, 1), (2040, 1500, 1), (5000, 4000, 3), (30000, 250, 1))      # (latent offset, rolled offset, scale)


def packed_path_pairs(cb, seed=33):
    """(latent, rolled) pairs with minutiae pixel coordinates inside [0, 2047], straddling it, and far beyond (S8a's generic float arithmetic)."""
    rng = np.random.default_rng(seed)
    base = S.make_latent(rng, n_tex_lo=210, n_tex_hi=240)
    R0 = S.make_mate(rng, cb, base, frac=0.8, n_tex=300)
    out = []
    for off_l, off_r, scale in PACKED_PATH_OFFSETS:
        def shift(m, off):
            x = (m.x.astype(np.int64) * scale + off).astype(np.uint16).view(np.int16)
            y = (m.y.astype(np.int64) * scale + off).astype(np.uint16).view(np.int16)
            return T.MinutiaeTemplate(x, y, m.ori, m.des)
        L = T.FPTemplate(minu=[shift(m_, off_l) for m_ in base.minu], tex=list(base.tex))
        R = T.FPTemplate(minu=[shift(R0.minu[0], off_r)], tex=list(R0.tex))
        out.append((L, R))
    return out


TIED_ROW_GROUPS = ([], [(10, 40)], [(5, 330)], [(50, 90), (120, 300)])


def tied_row_maxima_set(cb, seed=33):
    """(latents, rolled): latent texture rows that share a descriptor have bit-identical similarity rows, hence equal maxima — none, inside the top 200,
    straddling the 200th place, two groups."""
    rng = np.random.default_rng(seed)
    base = S.make_latent(rng, n_tex_lo=330, n_tex_hi=360)
    R = S.make_mate(rng, cb, base, frac=0.7, n_tex=600)
    t0 = base.tex[0]
    lats = []
    for groups in TIED_ROW_GROUPS:
        des = t0.des.copy()
        for lo, hi in groups:
            des[lo:hi] = des[lo]
        lats.append(T.FPTemplate(minu=list(base.minu), tex=[T.TextureTemplate(t0.x, t0.y, t0.ori, des=des)]))
    return lats, R


def both_signs_set(cb, seed=905, n_gal=40):
    """Structured latents of 201 .. 256 texture rows against prints whose descriptors point away from theirs: the 200 best row maxima have both signs."""
    SS = _SS()
    rng = np.random.default_rng(seed)
    keep = SS.IDENTITY_WEIGHT
    SS.IDENTITY_WEIGHT = 1.0
    try:
        lats = [SS.make_structured_latent(rng, sigma=0.0095, n_tex_lo=200, n_tex_hi=260) for _ in range(2)]
        gal = [SS.make_structured_rolled(rng, cb, sigma=0.0095, n_minu=int(rng.integers(20, 128)), n_tex=300) for _ in range(n_gal)]
    finally:
        SS.IDENTITY_WEIGHT = keep
    return lats, gal


def nan_inf_set(cb, seed=404):
    """(latent with NaN / +-inf / huge / denormal texture descriptor rows, the same latent without them, gallery of 3 random prints and a mate)."""
    rng = np.random.default_rng(seed)
    base = S.make_latent(rng, n_tex_lo=300, n_tex_hi=320)
    lt = base.tex[0]
    des = lt.des.copy()
    des[3, 5] = np.nan; des[4, :] = np.nan; des[9, 0] = np.inf; des[10, 95] = -np.inf; des[11, 40] = np.inf; des[11, 41] = -np.inf
    des[20, 7] = 7e4; des[21, 8] = -3e38; des[22, :] = 1e-42; des[23, 17] = 1001.0; des[24, 17] = 999.0; des[25, :] = 0.0
    lat = T.FPTemplate(minu=list(base.minu), tex=[T.TextureTemplate(lt.x, lt.y, lt.ori, des=des)])
    gal = [S.make_rolled(rng, cb, n_tex=n) for n in (640, 33, 1)] + [S.make_mate(rng, cb, base, frac=0.6, n_tex=500)]
    clean = T.FPTemplate(minu=list(base.minu), tex=[T.TextureTemplate(lt.x, lt.y, lt.ori, des=lt.des)])
    return lat, clean, gal


def wide_slice(cb, seed=88, n_lat=2, n_gal=12):
    """A slice of the "wide" workload (host/synth.py WORKLOADS): rolled prints of 130 +- 40 minutiae, latent templates of 20 .. 150, mates planted."""
    w = S.WORKLOADS["wide"]
    lats = S.make_latents(seed, n_lat, **w["latent"])
    packed = S.make_packed_gallery(seed, n_gal, cb, **w["gallery"])
    S.plant_mates(seed, packed, cb, lats)
    return lats, [packed.template(g) for g in range(n_gal)]


TEXTURE_SPREAD = ((25, 0, 0), (25, 9000, 9000), (10, 40000, 40000), (25, 0, 8180))      # (scale in tenths, latent offset, rolled offset)


def texture_spread_pairs(cb, seed=21):
    """(latent, rolled) pairs whose texture block coordinates are spread over 0..120 (many point pairs with |dx| or |dy| of 50 and more, the range rule of
    matcher.cpp:1257, some of exactly 50), moved beyond 8191 and beyond 32767 (negative as the reference reads them)."""
    rng = np.random.default_rng(seed)
    base = S.make_latent(rng, n_tex_lo=260, n_tex_hi=300)

    def spread(t, scale, offset=0):
        x = ((t.x.astype(np.int64) * scale) // 10 + offset).astype(np.int64)
        y = ((t.y.astype(np.int64) * scale) // 10 + offset).astype(np.int64)
        return x.astype(np.uint16).view(np.int16), y.astype(np.uint16).view(np.int16)

    out = []
    for scale, off_l, off_r in TEXTURE_SPREAD:
        L = T.FPTemplate(minu=list(base.minu), tex=[T.TextureTemplate(*spread(base.tex[0], scale, off_l), base.tex[0].ori, des=base.tex[0].des)])
        R0 = S.make_mate(rng, cb, base, frac=0.7, n_tex=500)
        rx, ry = spread(R0.tex[0], scale, off_r)
        out.append((L, T.FPTemplate(minu=list(R0.minu), tex=[T.TextureTemplate(rx, ry, R0.tex[0].ori, codes=R0.tex[0].codes)])))
    return out


def s9_limit_pairs(cb, seed=17):
    """(latent, rolled) pairs planted ON the limits of the angle tests of matcher.cpp:1503-1540.  Latent template 26 and the rolled minutiae template hold two
    minutiae each, at the same coordinates on a horizontal line (the line's angle is exactly 0), with orthogonal descriptors, so that the candidate list starts with
    the two true correspondences.  The rolled orientations are 0; the latent ones make one test's angle difference exactly a chosen float (eight pairs: each of
    the four values below with the offset on either minutia):
      the second test (limit PI / 6 in double, 0.5235987666...) at float(PI / 6) = 0.52359879, which is ABOVE the double limit — the two are incompatible, but
      a comparison in float would call them compatible — and at the float just below it;
      the first test (limit PI / 4 = 0.78539815) at float(PI / 4) = 0.78539813, just below the limit, and at the float just above (a1 - b1 = +x / 2, a2 - b2 = -x / 2,
      so that the second and third test see x / 2 and pass)."""
    rng = np.random.default_rng(seed)
    base = S.make_latent(rng, n_tex_lo=210, n_tex_hi=240)
    R0 = S.make_rolled(rng, cb, n_minu=30, n_tex=300)
    e = np.zeros((2, 96), np.float32); e[0, 0] = 1.8; e[1, 1] = 1.7
    x = np.array([100, 200], np.int16); y = np.array([100, 100], np.int16)      # the distance stage hands the two over in the order (second, first): the line runs from x = 200 to x = 100, atan2f(0, 100) = 0
    PI = 3.1415926
    x6, x4 = np.float32(PI / 6.), np.float32(PI / 4.)
    lim = [(x6, 0.0), (np.nextafter(x6, np.float32(0)), 0.0), (x4 / np.float32(2), -x4 / np.float32(2)),
           (np.nextafter(x4, np.float32(1)) / np.float32(2), -np.nextafter(x4, np.float32(1)) / np.float32(2))]
    out = []
    for a1, a2 in lim + [(b, a) for a, b in lim]:                              # the offset on the first minutia (the third test sees it) and on the second (the second test does)
        L = T.FPTemplate(minu=list(base.minu), tex=list(base.tex))
        L.minu[26] = T.MinutiaeTemplate(x.copy(), y.copy(), np.array([a1, a2], np.float32), e.copy())
        R = T.FPTemplate(minu=[T.MinutiaeTemplate(x.copy(), y.copy(), np.zeros(2, np.float32), e.copy())], tex=list(R0.tex))
        out.append((L, R))
    return out


def s2_rounding_pairs(cb, seed=0, n=15, noise=1e-5, count=3):
    """(latent, rolled) pairs in which ROUNDING inside S2's row and column sums (matcher.cpp:455-456) decides the candidate list: latent template 26 and the rolled
    minutiae template hold n minutiae each whose descriptors are one direction plus noise of relative size 1e-5, so the n * n similarities — and their
    normalised values, about 1 / (2n - 1) each — agree to five digits and the 120th place is contested by values a few ulps apart.  Minutia i has the same
    coordinates and orientation on both sides, so the candidates (i, i) that make the list survive the graph stages and the score tells which ones did."""
    rng = np.random.default_rng([seed, 0x52])
    base = S.make_latent(rng, n_tex_lo=210, n_tex_hi=240)
    R0 = S.make_rolled(rng, cb, n_minu=30, n_tex=300)
    out = []
    for _ in range(count):
        d = rng.standard_normal(96); d *= 1.73 / np.linalg.norm(d)
        x = rng.integers(50, 700, n).astype(np.int16); y = rng.integers(50, 700, n).astype(np.int16); ori = rng.uniform(-3, 3, n).astype(np.float32)
        dl = (d[None, :] * (1 + noise * rng.standard_normal((n, 96)))).astype(np.float32)
        dr = (d[None, :] * (1 + noise * rng.standard_normal((n, 96)))).astype(np.float32)
        L = T.FPTemplate(minu=list(base.minu), tex=list(base.tex))
        L.minu[26] = T.MinutiaeTemplate(x, y, ori, dl)
        out.append((L, T.FPTemplate(minu=[T.MinutiaeTemplate(x.copy(), y.copy(), ori.copy(), dr)], tex=list(R0.tex))))
    return out


def rules_gallery(cb, base, seed=11):
    """Rolled templates for the selection / fusion rules: mates and a non-mate of `base` at the default sizes and at 200 / 400 / 600 minutiae, and the first
    one without its texture template.  (A rolled template without minutiae cannot be written as a file: the writer stops after the header.)"""
    gal = []
    for nm in ((None, None, None), (200, 400, 600)):
        rng = np.random.default_rng(seed)
        kw = [dict(n_minu=n) if n else {} for n in nm]
        gal += [S.make_mate(rng, cb, base, frac=0.8, n_tex=400, **kw[0]), S.make_mate(rng, cb, base, frac=0.4, n_tex=350, **kw[1]), S.make_rolled(rng, cb, n_tex=300, **kw[2])]
    rng = np.random.default_rng([seed, 1])
    gal += [S.make_mate(rng, cb, base, frac=0.6, n_tex=250), S.make_rolled(rng, cb, n_tex=1200)]
    gal.append(T.FPTemplate(minu=list(gal[0].minu), tex=[]))
    return gal


def rolled_dat_with_texture_count(R, count):
    """T.write_rolled(R) with the point count of its first texture template overwritten (2001: the loaders refuse the file with -1, matcher.cpp:966-970)."""
    import struct
    buf = bytearray(T.write_rolled(R))
    pos = 32 + 1
    for m in R.minu:
        pos += 2 + (m.n * 8 + 2 + m.n * m.des.shape[1] * 4 if m.n > 0 else 0)
    pos += 1
    assert struct.unpack_from("<H", buf, pos)[0] == R.tex[0].n
    struct.pack_into("<H", buf, pos, count)
    return bytes(buf)


def _patch_first_count(buf, pos, count):
    import struct
    b = bytearray(buf); struct.pack_into("<H", b, pos, count)
    return bytes(b)


def loader_edge_files(cb, seed=3):
    """{name: (kind, bytes)} — files at the edges of the reference's two loaders (matcher.cpp:785-884 latent, :886-983 rolled) on which their result is DEFINED:
    empty files, a rolled file of 10 bytes (the rolled loader's own limit), a point count of 2001 in the first minutiae template (code 2) and in the texture
    template (code -1, the minutiae templates stay loaded), templates with a point count of 0 (skipped: later templates move up), a missing texture template."""
    rng = np.random.default_rng(seed)
    L = S.make_latent(rng, n_tex_lo=210, n_tex_hi=230)
    R = S.make_rolled(rng, cb, n_minu=25, n_tex=260)
    none = T.MinutiaeTemplate(np.zeros(0, np.int16), np.zeros(0, np.int16), np.zeros(0, np.float32), np.zeros((0, 96), np.float32))
    lat_tex_pos = 32 + 1 + sum(2 + m.n * 8 + 2 + m.n * m.des.shape[1] * 4 for m in L.minu) + 1
    out = {
        "rolled_empty": ("rolled", b""), "rolled_10_bytes": ("rolled", T.write_rolled(R)[:10]),
        "rolled_minutiae_2001": ("rolled", _patch_first_count(T.write_rolled(R), 33, 2001)), "rolled_texture_2001": ("rolled", rolled_dat_with_texture_count(R, 2001)),
        "rolled_no_texture": ("rolled", T.write_rolled(T.FPTemplate(minu=list(R.minu), tex=[]))),
        "rolled_first_template_without_points": ("rolled", T.write_rolled(T.FPTemplate(minu=[none] + list(R.minu), tex=list(R.tex)))),
        "latent_empty": ("latent", b""),
        "latent_minutiae_2001": ("latent", _patch_first_count(T.write_latent(L), 33, 2001)), "latent_texture_2001": ("latent", _patch_first_count(T.write_latent(L), lat_tex_pos, 2001)),
        "latent_no_texture": ("latent", T.write_latent(T.FPTemplate(minu=list(L.minu), tex=[]))),
        "latent_template_5_without_points": ("latent", T.write_latent(T.FPTemplate(minu=list(L.minu[:5]) + [none] + list(L.minu[6:]), tex=list(L.tex)))),
    }
    return out, T.write_latent(L), T.write_rolled(R)


class RecordSet:
    """One input set of the reference record: .dat bytes, the pairs taken from them, and what is recorded for them."""

    def __init__(self, name, cbb, lat, rol, pairs=None, orders=(0,), mode="selected", stage_pairs=(), corr=False, list2list=None, gpu=True, lat_names=None):
        self.name, self.cbb, self.lat, self.rol = name, cbb, lat, rol
        self.pairs = [(i, j) for i in range(len(lat)) for j in range(len(rol))] if pairs is None else list(pairs)
        self.orders, self.mode, self.stage_pairs, self.corr, self.list2list, self.gpu = tuple(orders), mode, list(stage_pairs), corr, list2list, gpu
        self.lat_names = lat_names


def _dats(lats, gal):
    return [T.write_latent(L) for L in lats], [T.write_rolled(R) for R in gal]


def _golden_npz():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_pairs.npz"))


def _shipped_bytes():
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", SHIPPED_CODEBOOK), "rb") as f:
        return f.read()


def _rs_golden(cbb, cb):
    g = _golden_npz()
    lat = [g[f"latent_{i}"].tobytes() for i in range(2)]; rol = [g[f"rolled_{j}"].tobytes() for j in range(12)]
    allp = [(i, j) for i in range(2) for j in range(12)]
    return RecordSet("golden", cbb, lat, rol, orders=(0, 1, 2, 3, 4, 5), stage_pairs=allp, corr=True, list2list={"latents": [0, 1], "extra": {}})


def _rs_small(cbb, cb):
    lats, gal = small_set(cb, seed=1)
    lat, rol = _dats(lats, gal)
    extra = {"R_empty.dat": b"", "R_tex2001.dat": rolled_dat_with_texture_count(gal[3], 2001)}
    return RecordSet("small", cbb, lat, rol, orders=(0, 1), list2list={"latents": [0, 1, 2], "extra": extra})


def _rs_structured(k):
    def make(cbb, cb):
        dup, n_lat, n_gal, idw, sg = STRUCTURED_CONFIGS[k]
        lats, gal = structured_set(cb, dup, n_lat, n_gal, idw, sg)
        lat, rol = _dats(lats, gal)
        return RecordSet(f"structured{dup}", cbb, lat, rol, orders=(0, 1), stage_pairs=[(0, 0), (0, n_gal - 1), (1, n_gal - 2)])
    return make


def _rs_rules(cbb, cb):
    base, variants = edge_latents(cb)
    names = [n for n in variants if n != "minu0_tex"]          # a latent without minutiae is a header-only file: undefined in the reference (matcher.cpp:827)
    lat = [T.write_latent(variants[n]) for n in names]
    rol = [T.write_rolled(R) for R in rules_gallery(cb, base)]
    return RecordSet("rules", cbb, lat, rol, lat_names=names)


def _rs_pairs(name, fn, which_stage=False):
    def make(cbb, cb):
        prs = fn(cb)
        lat = [T.write_latent(L) for L, _ in prs]; rol = [T.write_rolled(R) for _, R in prs]
        diag = [(i, i) for i in range(len(prs))]
        return RecordSet(name, cbb, lat, rol, pairs=diag, stage_pairs=diag if which_stage else ())
    return make


def _rs_edge_shapes(cbb, cb):
    return RecordSet("shapes_edge", cbb, *_dats(*edge_shapes_set(cb)))


# The device does not reproduce std::sort's order of equal keys at S7 (matcher.cpp:741; option ref_tie_order 2 covers S3, S8 and S9: the oracle's tie mode 9), so the sets
# the GPU tests compare with the record are built from seeds at which that order does not decide a score (tests/test_reference_record.py asserts that no pair of them
# depends on it).  The same inputs at the seeds of the GPU parity tests, where it does decide some, are recorded as well and held against the oracle on the CPU.
def _rs_tied(seed, name, gpu):
    def make(cbb, cb):
        lats, R = tied_row_maxima_set(cb, seed)
        lat, rol = _dats(lats, [R])
        return RecordSet(name, cbb, lat, rol, stage_pairs=[(i, 0) for i in range(len(lats))], gpu=gpu)
    return make


def _rs_both_signs(cbb, cb):
    lats, gal = both_signs_set(cb)
    return RecordSet("shapes_both_signs", cbb, *_dats(lats, gal[:12]))


def _rs_nan(seed, name, gpu):
    def make(cbb, cb):
        lat, clean, gal = nan_inf_set(cb, seed)
        return RecordSet(name, cbb, *_dats([lat, clean], gal), gpu=gpu)
    return make


def _rs_offenv(cbb, cb):
    lats, rolled, _ = S.make_offenvelope_set(5, 3, 12, cb)
    return RecordSet("shapes_offenvelope", cbb, *_dats(lats, rolled))


def _rs_wide(cbb, cb):
    return RecordSet("shapes_wide", cbb, *_dats(*wide_slice(cb)))


def _rs_all(cbb, cb):
    lats, gal = small_set(cb, seed=5, n_lat=2, n_gal=10)
    return RecordSet("all", cbb, *_dats(lats, gal), mode="all")


def _rs_family(name, seed=31, set_name=None, gpu=True):
    def make(cbb, cb):
        fcb, lats, gal = family_set(name, cb, seed)
        return RecordSet(set_name or "family_" + name, fcb.to_bytes(), *_dats(lats, gal), gpu=gpu)
    return make


RECORD_SETS = {"golden": _rs_golden, "small": _rs_small, "structured10": _rs_structured(0), "structured30": _rs_structured(1), "rules": _rs_rules,
               "shapes_edge": _rs_edge_shapes, "shapes_degenerate_keys": _rs_pairs("shapes_degenerate_keys", degenerate_key_pairs, True),
               "shapes_packed_path": _rs_pairs("shapes_packed_path", packed_path_pairs),
               "shapes_texture_spread": _rs_pairs("shapes_texture_spread", texture_spread_pairs, True), "shapes_s9_limits": _rs_pairs("shapes_s9_limits", s9_limit_pairs, True),
               "shapes_s2_rounding": _rs_pairs("shapes_s2_rounding", lambda cb: s2_rounding_pairs(cb, seed=1), True),      # at this seed the third pair's score changes when the row sums run backwards
               "shapes_tied_maxima": _rs_tied(52, "shapes_tied_maxima", True), "shapes_tied_maxima_s7": _rs_tied(33, "shapes_tied_maxima_s7", False),
               "shapes_both_signs": _rs_both_signs, "shapes_nan_inf": _rs_nan(410, "shapes_nan_inf", True), "shapes_nan_inf_s7": _rs_nan(404, "shapes_nan_inf_s7", False), "shapes_offenvelope": _rs_offenv, "shapes_wide": _rs_wide, "all": _rs_all}
RECORD_SETS.update({"family_" + n: _rs_family(n) for n in CODEBOOK_FAMILY})
# tiny codebook: nearly every similarity is 6 minus very little, row maxima tie in every pair and S7's order of them decides one pair in ten (see the note above _rs_tied)
RECORD_SETS.update({"family_tiny": _rs_family("tiny", 55), "family_tiny_s7": _rs_family("tiny", 31, "family_tiny_s7", False)})
_record_cache = {}


def record_set(name):
    """The input set `name` of tests/golden/golden_matcher_ref.npz (built once per process)."""
    if name not in _record_cache:
        cbb = _shipped_bytes()
        _record_cache[name] = RECORD_SETS[name](cbb, T.Codebook.from_bytes(cbb))
    return _record_cache[name]


def record_latent_name(i): return f"L{i}.dat"
def record_rolled_name(j): return f"R{j:03d}.dat"


def load_reference_record():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_matcher_ref.npz"))


def record_parts(vec_bits, info, status):
    """(s0, s1, s2, texture, fused) as uint32 bit patterns from a recorded score vector of One2One_matching_selected_templates: the minutiae scores of latent
    templates 26 / 2 / 11 sit in slots 0..2 (0 where the latent lacks the template), the texture score in slot n_minu_templates, and the fused score is
    matcher.cpp:188's `score[0] + score[1] + score[2] + score[28]*0.3` (float sums, then double).  With fewer than 29 slots the reference reads beyond the
    vector there (undefined); the project's reading — an absent slot is 0 — is what this returns then.  Status 1 / 2: zeros and a fused score of -1."""
    n_lm, n_lt = int(info[2]), int(info[3])
    vec = np.asarray(vec_bits, np.uint32).view(np.float32)
    out = np.zeros(5, np.float32)
    if status != 0:
        out[4] = -1.0
        return out.view(np.uint32)
    sel = (26, 2, 11)
    for i in range(3):
        if n_lm > sel[i]: out[i] = vec[i]
    if n_lt > 0: out[3] = vec[n_lm]
    at = lambda k: vec[k] if k < n_lm + n_lt else np.float32(0)
    with np.errstate(all="ignore"):
        f = np.float32(np.float32(at(0) + at(1)) + at(2))
        out[4] = np.float32(np.float64(f) + np.float64(at(28)) * 0.3)
    return out.view(np.uint32)


# ---- one slice of a large synthetic gallery, committed the way a rank commits its shard (tests/test_gpu_fullsize.py, tests/test_gpu_large_shard.py) ----
def committed_slice(codebook_bytes, cb, seed, G, lats, lo, hi, index_base=0, n_partial=3, taps=False):
    """Templates [lo, hi) of the G-template synthetic gallery, generated, planted with the latents' mates and committed alone at index_base + lo, exactly as rank r of a sharded
    job would: -> (PackedGallery of the slice after planting, planted {latent: [(global gallery index, frac)]}, the committed Matcher; the caller closes it)."""
    M = importlib.import_module("msu-latentafis_amd.host.matcher")
    gal = S.make_packed_gallery(seed, G, cb, lo, hi)
    planted = S.plant_mates(seed, gal, cb, lats, G=G, lo=lo, n_partial=n_partial)
    m = M.Matcher(codebook_bytes, taps=taps)
    m.gallery_add_packed(gal); m.gallery_commit(index_base + lo)
    return gal, planted, m


# The sizes at which one shard's device arrays pass 4 GiB and its descriptor floats pass 2^31 (element sizes: csrc/afis_device.h — 96 fp32 per minutia, fragment tiles of
# 16 descriptors = 6 x 64 float4 = 6144 bytes, 16 code bytes per texture point, the bound pass's stream padded to tiles of 32 points).
LARGE_SHARD_LIMITS = {"minu_des_floats": 1 << 31, "minu_frag_bytes": 1 << 32, "tex_codes_bytes": 1 << 32, "codes_p_bytes": 1 << 32}


def large_shard_quantities(nm, nt):
    """The four quantities of LARGE_SHARD_LIMITS for per-template minutiae / texture point counts nm, nt."""
    nm = np.asarray(nm, np.int64); nt = np.asarray(nt, np.int64)
    return {"minu_des_floats": int(nm.sum()) * 96, "minu_frag_bytes": int(((nm + 15) // 16).sum()) * 6144,
            "tex_codes_bytes": int(nt.sum()) * 16, "codes_p_bytes": int(((nt + 31) // 32).sum()) * 32 * 16}


def large_shard_size(seed, slice_size=50000, limit=2000000):
    """The smallest multiple of slice_size for which S.gallery_counts(seed, G) passes every limit of LARGE_SHARD_LIMITS (the counts of a synthetic gallery depend on G)."""
    for G in range(slice_size, limit + 1, slice_size):
        q = large_shard_quantities(*S.gallery_counts(seed, G))
        if all(q[k] > LARGE_SHARD_LIMITS[k] for k in LARGE_SHARD_LIMITS):
            return G
    raise AssertionError("no gallery size up to %d passes the limits" % limit)


# ---- correspondence lists of every length (tests/test_gpu_list_lengths.py) ----
# The list kernels (csrc/graph.hip: dist_filter, angle_filter, sort_scores, greedy) choose nearly every branch by the LENGTH of the list they are handed: blocks of 64 rows,
# a last block of 1..8 / 9..16 / 17..32 rows that is dealt to lane groups, the parity of the length (the antipodal offset), 48 and 16 entries in the sorts.  These inputs make
# a list of exactly the wanted length and leave survivors whose number is known: a texture list has one entry per latent row (up to the 200-row cut), a minutiae list has
# min(120, latent minutiae x rolled minutiae) entries.
LIST_TEX_N = (1, 2, 3, 8, 9, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 72, 73, 80, 81, 95, 96, 97,
              127, 128, 129, 136, 137, 144, 145, 160, 161, 191, 192, 193, 199, 200, 230)
LIST_GEOMETRIES = ("rigid", "dense", "sparse", "range")
LIST_RANGE_N = tuple(n for n in LIST_TEX_N if n >= 8)                   # the |d| < 50 rule needs pairs on both of its sides
LIST_TEX_ROLLED = 300                                                   # texture points of every rolled template
LIST_TEX_MOVE = (2, -1)                                                 # the rolled copy of the latent rows, in blocks
LIST_TEX_JITTER = {"rigid": 0, "dense": 1, "sparse": 2, "range": 1}
# (rolled minutiae, minutiae of the latent templates 26 / 2 / 11): one pair gives three list lengths.  The products cover 4, 9, 16, 18, 32, 33, 36, 48, 49, 63, 64, 65, 66,
# 72, 80, 81, 96, 98, 99, 108, 119, 120 and beyond 120 (121, 144, 3200); 17 and 97 against ONE rolled minutia; the last five hand S9 about 64, 65, 96, 100 and 120 entries.
LIST_MINU_SPECS = ((2, (2, 3, 4)), (3, (3, 6, 11)), (4, (4, 8, 2)), (6, (6, 8, 11)), (7, (7, 9, 14)), (7, (17, 5, 3)), (8, (8, 9, 10)), (8, (12, 3, 5)), (9, (9, 11, 12)),
                   (13, (5, 8, 7)), (12, (10, 12, 4)), (11, (11, 6, 9)), (80, (40, 20, 10)), (1, (17, 97, 5)),
                   (64, (64, 30, 10)), (70, (65, 16, 33)), (100, (96, 48, 24)), (110, (100, 50, 72)), (120, (120, 60, 90)))
LIST_MINU_JITTER = (3, 20)                                              # pixels: every true correspondence agrees with every other / only some do
LIST_SELECTED = (26, 2, 11)
SHAPE_SWEEP_ARGS = ("5", "8", "30")                                       # tools/shape_sweep.py as tests/test_gpu_parity.py runs it ...
SHAPE_SWEEP_NONZERO = 368                                               # ... and the oracle's non-zero part scores on those 240 pairs (960 part scores)
LIST_RESEED = {}                                                        # {("texture", geometry, N) or ("minutiae", pair): n}: the n-th draw, where the first left fewer than two survivors


def list_pair_matrices(lx, ly, rx, ry, texture):
    """(in range, neighbours) of every pair of list entries as graph.hip decides them: texture pairs are in range when every |d| < 50 (matcher.cpp:1257), minutiae pairs always;
    neighbours (H != 0) are in range with |d1 - d2| < 30 px in the reference's float arithmetic (a block is 16 px).  The neighbour matrix's row sums are row_degrees of
    tests/test_gpu_graph_slab.py."""
    lx, ly, rx, ry = (np.asarray(v, np.int64) for v in (lx, ly, rx, ry))
    dx1 = lx[:, None] - lx[None, :]; dy1 = ly[:, None] - ly[None, :]; dx2 = rx[:, None] - rx[None, :]; dy2 = ry[:, None] - ry[None, :]
    d1 = np.sqrt((dx1 * dx1 + dy1 * dy1).astype(np.float32)); d2 = np.sqrt((dx2 * dx2 + dy2 * dy2).astype(np.float32))
    if texture:
        ok = (np.abs(dx1) < 50) & (np.abs(dy1) < 50) & (np.abs(dx2) < 50) & (np.abs(dy2) < 50)
        near = np.float32(16.0) * np.abs(d1 - d2) < np.float32(30.0)
    else:
        ok = np.ones(d1.shape, bool)
        near = np.abs(d1 - d2) < np.float32(30.0)
    np.fill_diagonal(ok, False)
    return ok, ok & near


def list_walk_classes(num):
    """(antipodal, wrapped): boolean [num, num] masks over i < j of the pairs the kernels' pair walk (row t visits t + d mod num, d = 1 .. num / 2) reaches at the offset
    d == num / 2 of an even list, and through the wrap past the list's end (from row j: i + num - j <= num / 2)."""
    i, j = np.triu_indices(num, 1)
    anti = np.zeros((num, num), bool); wrap = np.zeros((num, num), bool)
    anti[i, j] = (num % 2 == 0) & (2 * (j - i) == num)
    wrap[i, j] = 2 * (j - i) > num
    return anti, wrap


def _list_unit(rng, n):
    d = rng.standard_normal((n, 96)).astype(np.float32)
    return (d * (np.float32(T.DESCRIPTOR_NORM) / np.linalg.norm(d, axis=1, keepdims=True))).astype(np.float32)


def _list_texture(rng, cb, geometry, N):
    """Latent texture template of N rows on distinct cells and a rolled one of LIST_TEX_ROLLED points, N of which (at random places) are the rows moved by LIST_TEX_MOVE + jitter.
    Default window: every coordinate of both sides in [0, 49]; "range": a window of 66 blocks, so that some pairs fail |d| < 50."""
    J = LIST_TEX_JITTER[geometry]
    side = 66 if geometry == "range" else 46
    lori = rng.uniform(-np.pi / 2, np.pi / 2, N).astype(np.float32)
    des = _list_unit(rng, N)
    for _ in range(200):                                                     # dense and range: drawn until the planted pairs have the property the case is there for
        cells = rng.permutation(side * side)[:N]
        lx = cells % side; ly = cells // side + 3                           # rolled: x + 2 + j in [0, side + 3], y - 1 + j in [0, side + 3]
        if J == 1:                                                           # two points in three stay put: nearly all pairs are neighbours, with H values that differ
            jit = rng.choice([-1, 0, 0, 0, 0, 1], (N, 2))
        else:
            jit = rng.integers(-J, J + 1, (N, 2))
        px = lx + LIST_TEX_MOVE[0] + jit[:, 0]; py = ly + LIST_TEX_MOVE[1] + jit[:, 1]
        ok, near = list_pair_matrices(lx, ly, px, py, True)
        if geometry == "dense" and N >= 2 and near.sum(axis=1).min() < 0.85 * (N - 1):
            continue                                                         # (the test asks for 0.8 of the LIST's rows: of 230 rows S7 keeps 200)
        if geometry == "range" and (ok.sum() == N * (N - 1) or not near.any()):
            continue
        break
    else:
        raise AssertionError(("no draw with the wanted pairs", geometry, N))
    n_r = LIST_TEX_ROLLED
    at = rng.permutation(n_r)[:N]
    rx = rng.integers(0, side + 4, n_r); ry = rng.integers(0, side + 4, n_r)
    rori = rng.uniform(-np.pi / 2, np.pi / 2, n_r).astype(np.float32)
    codes = rng.integers(0, cb.K, (n_r, cb.M)).astype(np.uint8)
    rx[at] = px; ry[at] = py
    rori[at] = lori + (rng.standard_normal(N) * 0.05).astype(np.float32)
    codes[at] = cb.encode_fast(des + np.float32(0.04) * rng.standard_normal((N, 96)).astype(np.float32))
    return (T.TextureTemplate(lx.astype(np.int16), ly.astype(np.int16), lori, des=des),
            T.TextureTemplate(rx.astype(np.int16), ry.astype(np.int16), rori, codes=codes))


def _list_minutiae(rng, n_r, n_l3, jitter, second_jitter=None):
    """28 latent minutiae templates (the selected ones hold the first n_l3[i] points of a pool, the others two) and a rolled one of the pool's first n_r points, moved and
    jittered: min(n_l, n_r) true correspondences per list.  Pool points sit on a 110-px grid (+-8): far enough apart for the jitter not to turn the line between two of them, and spread widely enough
    for two FALSE correspondences to agree in distance (within 30 px) only rarely — the true ones have to win the power iteration even where there are only two or three.
    second_jitter: a third value, a second rolled view of the same points (its own order, noise and move, drawn after everything else) with that jitter."""
    P = max(n_r, *n_l3)
    cells = rng.permutation(16 * 17)[:P]
    px = 60 + 110 * (cells % 16) + rng.integers(-8, 9, P); py = 60 + 110 * (cells // 16) + rng.integers(-8, 9, P)   # <= 1828: with the move and the jitter inside [0, 2047]
    po = rng.uniform(-np.pi, np.pi, P).astype(np.float32)
    pd = _list_unit(rng, P)

    def view(n, sigma, move=(0, 0), jit=0, ori_sigma=0.0):
        o = rng.permutation(n)
        d = pd[o] + np.float32(sigma) * rng.standard_normal((n, 96)).astype(np.float32)
        d = (d * (np.float32(T.DESCRIPTOR_NORM) / np.linalg.norm(d, axis=1, keepdims=True))).astype(np.float32)
        x = px[o] + move[0] + rng.integers(-jit, jit + 1, n); y = py[o] + move[1] + rng.integers(-jit, jit + 1, n)
        return T.MinutiaeTemplate(x.astype(np.int16), y.astype(np.int16), (po[o] + (rng.standard_normal(n) * ori_sigma).astype(np.float32)).astype(np.float32), d)

    sizes = dict(zip(LIST_SELECTED, n_l3))
    lat = [view(sizes.get(i, min(2, P)), 0.02) for i in range(28)]
    rol = view(n_r, 0.08, (int(rng.integers(-20, 21)), int(rng.integers(-20, 21))), jitter, 0.05)
    if second_jitter is None:
        return lat, rol
    return lat, rol, view(n_r, 0.08, (int(rng.integers(-20, 21)), int(rng.integers(-20, 21))), second_jitter, 0.05)


def list_length_set(cb, seed=70):
    """One (latent, rolled) pair per texture length and geometry; pair c carries the minutiae shapes LIST_MINU_SPECS[c % 19] with jitter LIST_MINU_JITTER[c // 19 % 2].
    -> list of dicts: geometry, N, spec (rolled minutiae, latent minutiae of 26 / 2 / 11), minu_jitter, L, R."""
    out = []
    for gi, geometry in enumerate(LIST_GEOMETRIES):
        for N in (LIST_RANGE_N if geometry == "range" else LIST_TEX_N):
            c = len(out)
            n_r, n_l3 = LIST_MINU_SPECS[c % len(LIST_MINU_SPECS)]
            jitter = LIST_MINU_JITTER[c // len(LIST_MINU_SPECS) % 2]
            lt, rt = _list_texture(np.random.default_rng([seed, 0, gi, N, LIST_RESEED.get(("texture", geometry, N), 0)]), cb, geometry, N)
            lm, rm = _list_minutiae(np.random.default_rng([seed, 1, c, LIST_RESEED.get(("minutiae", c), 0)]), n_r, n_l3, jitter)
            out.append(dict(geometry=geometry, N=N, spec=(n_r, n_l3), minu_jitter=jitter, L=T.FPTemplate(minu=lm, tex=[lt]), R=T.FPTemplate(minu=[rm], tex=[rt])))
    return out


def list_length_shifted(t, tex_shift=0, minu_shift=0):
    """The template with every texture block coordinate moved by tex_shift and every minutiae pixel coordinate by minu_shift (into another arithmetic class of the list kernels)."""
    mv = lambda v, s: (v.astype(np.int64) + s).astype(np.int16)
    return T.FPTemplate(minu=[T.MinutiaeTemplate(mv(m.x, minu_shift), mv(m.y, minu_shift), m.ori, m.des) for m in t.minu],
                        tex=[T.TextureTemplate(mv(x.x, tex_shift), mv(x.y, tex_shift), x.ori, des=x.des, codes=x.codes) for x in t.tex])


# ---- the any-shape candidate kernel at its own route borders, and the pair-table forms (tests/test_gpu_pair_forms.py) ----
# k_minu_cands (csrc/minu.hip) chooses its routes by the SHAPE of a list, nL latent x nR rolled minutiae, n = nL nR similarities: the similarity matrix in LDS (nL <= 64 and
# nR <= 128) or in the workgroup's global scratch; the keys of the threshold search in 16 registers per thread (n <= 4096) or in scratch; GEMM tiles of 64 rows x 32 columns
# with tails; and, with option s3_tie_order, std::sort's arrays in LDS with 16-bit indices (n <= 8192) or in scratch with 32-bit ones.  In a search the kernel receives what
# the matrix-core classes leave over; in the pair-table calls it is the only candidate kernel, for every shape, in persistent workgroups.
# (rolled minutiae, latent minutiae of templates 26 / 2 / 11), as LIST_MINU_SPECS: n = 4095 / 4096 / 4158 / 4160 with the matrix on either side of the LDS border, 8192 / 8255 /
# 8256 / 8320, tile tails of 31 / 32 / 33, 63 / 64 / 65 and 127 / 128 / 129 points, lists of 118 .. 121 cells, and shapes that use the scratch fully (the pool of
# _list_minutiae holds 272 points).
PAIR_BORDER_SPECS = ((128, (64, 65, 63)), (129, (64, 32, 31)), (127, (64, 65, 33)), (64, (64, 65, 63)), (65, (64, 63, 62)), (63, (65, 66, 64)), (32, (128, 129, 127)),
                     (31, (132, 133, 129)), (33, (124, 125, 128)), (96, (42, 43, 86)), (160, (25, 26, 52)), (256, (16, 17, 32)), (272, (15, 16, 31)), (40, (100, 103, 102)),
                     (60, (65, 68, 69)), (200, (200, 150, 256)), (272, (272, 140, 152)), (1, (119, 120, 121)), (2, (60, 61, 59)), (120, (1, 2, 3)))
PAIR_BORDER_RESEED = {}                                                 # {spec number: n}: the n-th draw, where the first missed a condition of the rehearsal
CANDS_LDS_ROWS, CANDS_LDS_COLS, CANDS_KEY_REGS, CANDS_SORT_LDS = 64, 128, 4096, 8192      # minu.hip: kFastL, kFastR, kThreads * kKeyRegs, kFastN
CANDS_TILE_ROWS, CANDS_TILE_COLS = 64, 32                               # minu.hip: kGemmRows, kGemmCols
DEGENERATE_SHAPES = ((64, 64), (64, 65), (65, 63), (66, 63), (32, 128), (31, 129), (33, 129), (64, 128), (65, 127), (128, 64), (129, 64), (64, 129), (65, 128), (200, 272))


def cands_route(nL, nR):
    """The routes k_minu_cands takes for a list of nL x nR similarities: (matrix in "lds" / "scratch", keys in "regs" / "scratch", std::sort's arrays in "lds16" / "scratch32")."""
    n = nL * nR
    return ("lds" if nL <= CANDS_LDS_ROWS and nR <= CANDS_LDS_COLS else "scratch", "regs" if n <= CANDS_KEY_REGS else "scratch", "lds16" if n <= CANDS_SORT_LDS else "scratch32")


# every combination the three rules allow: a matrix in LDS has at most 8192 cells, keys in registers at most 4096
CANDS_ROUTES = (("lds", "regs", "lds16"), ("lds", "scratch", "lds16"), ("scratch", "regs", "lds16"), ("scratch", "scratch", "lds16"), ("scratch", "scratch", "scratch32"))


def cands_border_coverage(shapes):
    """{name: reached} for a set of (nL, nR) shapes — every route combination, both sides of every route border (within one tile of it), every tile tail class.  A pure
    function of the shapes: tests/test_gpu_pair_forms.py asserts that every entry holds for PAIR_BORDER_SPECS."""
    shapes = sorted(set(shapes))
    routes = {cands_route(*s) for s in shapes}
    out = {"route " + "/".join(r): r in routes for r in CANDS_ROUTES}
    cells = lambda lo, hi, matrix: any(lo <= nL * nR <= hi and cands_route(nL, nR)[0] == matrix for nL, nR in shapes)
    for matrix in ("lds", "scratch"):
        out["keys: %d cells or just below, matrix in %s" % (CANDS_KEY_REGS, matrix)] = cells(CANDS_KEY_REGS - 1, CANDS_KEY_REGS, matrix)
        out["keys: exactly %d cells, matrix in %s" % (CANDS_KEY_REGS, matrix)] = cells(CANDS_KEY_REGS, CANDS_KEY_REGS, matrix)
        out["keys: just beyond %d cells, matrix in %s" % (CANDS_KEY_REGS, matrix)] = cells(CANDS_KEY_REGS + 1, CANDS_KEY_REGS + CANDS_TILE_ROWS, matrix)
    out["sort arrays: exactly %d cells" % CANDS_SORT_LDS] = cells(CANDS_SORT_LDS, CANDS_SORT_LDS, "lds")
    out["sort arrays: just beyond %d cells" % CANDS_SORT_LDS] = cells(CANDS_SORT_LDS + 1, CANDS_SORT_LDS + 2 * CANDS_TILE_ROWS, "scratch")
    for name, side, unit in (("latent", 0, CANDS_TILE_ROWS), ("rolled", 1, CANDS_TILE_COLS), ("rolled", 1, CANDS_LDS_COLS)):
        for d in (-1, 0, 1):
            out["%s points: a multiple of %d %+d" % (name, unit, d)] = any(s[side] > unit // 2 and (s[side] - d) % unit == 0 for s in shapes)
    out["lists of fewer than 120 cells"] = any(nL * nR < 120 for nL, nR in shapes)
    out["lists of exactly 120 cells"] = any(nL * nR == 120 for nL, nR in shapes)
    out["the full pool on both sides"] = any(nL == 272 and nR == 272 for nL, nR in shapes)
    return out


def pair_border_shapes(specs=PAIR_BORDER_SPECS):
    return [(n_l, n_r) for n_r, n_l3 in specs for n_l in n_l3]


def pair_border_set(cb, seed=71, specs=PAIR_BORDER_SPECS):
    """Per spec one latent, its mate (jitter LIST_MINU_JITTER[0]: every true correspondence agrees with every other) and a second rolled view of the same points (jitter
    LIST_MINU_JITTER[1], its own descriptor noise: another S3 list); every template carries a small texture template (12 .. 40 latent rows), so the texture scorer runs.
    -> list of dicts: spec, L, R, R2."""
    out = []
    for i, (n_r, n_l3) in enumerate(specs):
        draw = PAIR_BORDER_RESEED.get(i, 0)
        lm, rm, rm2 = _list_minutiae(np.random.default_rng([seed, 1, i, draw]), n_r, n_l3, LIST_MINU_JITTER[0], LIST_MINU_JITTER[1])
        lt, rt = _list_texture(np.random.default_rng([seed, 0, i, draw]), cb, "dense", 12 + 7 * i % 29)
        _, rt2 = _list_texture(np.random.default_rng([seed, 2, i, draw]), cb, "sparse", 12 + 7 * i % 29)
        out.append(dict(spec=(n_r, n_l3), L=T.FPTemplate(minu=lm, tex=[lt]), R=T.FPTemplate(minu=[rm], tex=[rt]), R2=T.FPTemplate(minu=[rm2], tex=[rt2])))
    return out


def degenerate_keys_at(cb, nL, nR, seed=5):
    """The three cases of degenerate_key_pairs at the shape nL x nR (latent template 26 against the rolled minutiae template) -> [(case, latent, rolled)]: "a" fewer than 120
    non-zero similarities (k rolled descriptors point along the latent's, nL k < 120, the others away; left out where nL >= 120), "b" every similarity identical, "c" a few
    levels with large blocks of exact ties."""
    rng = np.random.default_rng([seed, nL, nR])
    base = S.make_latent(rng, n_tex_lo=40, n_tex_hi=60)
    d = rng.standard_normal(96).astype(np.float32); d *= np.float32(1.73) / np.linalg.norm(d)
    e = rng.standard_normal(96).astype(np.float32); e -= d * (e @ d) / (d @ d); e *= np.float32(1.73) / np.linalg.norm(e)     # orthogonal to d

    def latent_with(des_rows):
        L = T.FPTemplate(minu=list(base.minu), tex=list(base.tex))
        n = len(des_rows)
        L.minu[26] = T.MinutiaeTemplate(rng.integers(50, 700, n).astype(np.int16), rng.integers(50, 700, n).astype(np.int16),
                                        rng.uniform(-3, 3, n).astype(np.float32), np.stack(des_rows).astype(np.float32))
        return L

    def rolled_with(des_rows):
        n = len(des_rows)
        R = S.make_rolled(rng, cb, n_minu=n, n_tex=60)
        R.minu[0] = T.MinutiaeTemplate(R.minu[0].x, R.minu[0].y, R.minu[0].ori, np.stack(des_rows).astype(np.float32))
        return R

    out = []
    if nL < 120:
        k = min(119 // nL, nR - 1)
        assert k >= 1 and nL * k < 120
        out.append(("a", latent_with([d] * nL), rolled_with([-d] * (nR - k) + [d] * k)))
    out.append(("b", latent_with([d] * nL), rolled_with([d] * nR)))
    out.append(("c", latent_with([d] * (nL // 3) + [e] * (nL - nL // 3)), rolled_with([d] * (nR // 4) + [0.5 * d + 0.5 * e] * (nR - nR // 4))))
    return out


def degenerate_border_set(cb):
    """degenerate_keys_at over DEGENERATE_SHAPES -> list of dicts: shape, case, L, R."""
    return [dict(shape=(nL, nR), case=c, L=L, R=R) for nL, nR in DEGENERATE_SHAPES for c, L, R in degenerate_keys_at(cb, nL, nR)]
