"""Print search without a GPU: afis_search_prints and its tap are declared, exported by the right libraries and bound by the Python host, the kernel and the driver
are product objects, the two options are documented and the header carries the contract; the numpy model (tests/print_model.py) — the view, the decode, the
destination CSRs, the fragment tiles, the plan and its batches — is held against hand-made cases and loops.  (What the device computes is
tests/test_gpu_print_search.py's.)"""
import importlib
import os
import re

import numpy as np

import print_model as P
import weighted_model as W

M = importlib.import_module("msu-latentafis_amd.host.matcher")
T = importlib.import_module("msu-latentafis_amd.host.templates")
SH = importlib.import_module("msu-latentafis_amd.host.sharding")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ("print_gather_us", "print_h2d_bytes")


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+afis_search_prints\s*\(afis_ctx\*\s*ctx,\s*afis_subset\*\s*s\s*,\s*const int64_t\*\s*idx\s*,\s*int n_q,\s*const float\*\s*w_minu\s*,\s*"
                     r"const float\*\s*w_tex\s*,\s*float\*\s*scores\s*,\s*int32_t\*\s*status\s*\)", code)
    declared = set(re.findall(r"\b(afis_[a-z0-9_]+)\s*\(", hdr))            # comments count: every name spelled with a parenthesis is an exported function
    assert declared == set(M.EXPORTS) and "afis_search_prints" in declared
    taps = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afis_matcher_taps.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+afis_debug_print_queries\s*\(afis_ctx\*", taps) and "afis_debug_print_queries" in M.TAP_EXPORTS
    product, test = M.load_library(), M.load_library(M.TEST_LIB_PATH)       # dlopen only: no device call
    for lib in (product, test):
        assert hasattr(lib, "afis_search_prints") and lib.afis_search_prints.argtypes is not None
    assert hasattr(test, "afis_debug_print_queries") and not hasattr(product, "afis_debug_print_queries")
    for method in ("search_prints", "debug_print_queries"):
        assert hasattr(M.Matcher, method), method
    option_text = hdr[hdr.index("The value an option has now"):hdr.index("int afis_get_option")]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for opt in OPTIONS:
        assert re.search(r'"%s" \(read-only' % opt, option_text), opt
        assert "`%s`" % opt in integration, opt


def test_the_header_carries_the_contract():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    contract = hdr[hdr.index("Print search (no reference counterpart"):hdr.index("int afis_search_prints")]
    for phrase in ("GLOBAL indices", "repeat", "bit for bit", "des[r][6 m + k] = codewords[m][code[r][m]][k]", "no arithmetic", "n_wm = 1, n_wt = 1", "AFIS_QUERY_LATENT_EMPTY",
                   "A print against itself is an ordinary cell", "exclusion list", "exactly as afis_search_subset", "need not be in the subset", "one of the searches that count",
                   "staged but not committed", "not live in this context", "weighted_batch_pseudo", "search_timeout_s", "print_gather_us", "print_h2d_bytes",
                   "profiles/print_search_timing.json"):
        assert phrase in contract, phrase
    # the forms left out, and the rule for shards, in one "Not in this interface" sentence
    left_out = contract[contract.index("Not in this interface"):]
    for phrase in ("pair and verification forms for prints", "rolled templates beyond index 0", "the match CLI", "a print is a query only on the rank that holds it",
                   "its template must be present there", "afis_search_weighted route over host views", "merge_hits / merge_subject_hits input as they are"):
        assert phrase in left_out, phrase
    assert "afis_search_prints" in hdr[hdr.index("afis_rank_subjects   ranks the score matrix"):hdr.index("n_q must be that")]     # the list of searches that count
    doc = SH.__doc__ or ""
    for phrase in ("only on the rank that holds it", "search_weighted", "merge_hits"):
        assert phrase in doc, phrase


def test_the_kernel_and_the_driver_are_product_objects():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "print_queries.o" in objs and "afis_prints.o" in objs
    assert re.search(r"^print_queries\.o:\s*print_queries\.hip", mk, flags=re.M) and re.search(r"^afis_prints\.o:\s*afis_prints\.cpp", mk, flags=re.M)
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "print_queries.hip")).read()
    body = src.split("namespace afis {", 1)[1]                                # the code, without the header comment
    assert "__global__" in body and "grid_clamp" in body and "size_t" in body and "uint4" in body
    assert "atomic" not in body and "hipMemset" not in body and "__shared__" not in body         # every word written once; the codebook is read through L2
    drv = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "afis_prints.cpp")).read()
    assert "build_group(" not in drv.split("#include", 1)[1] and "search_shard(" in drv and "launch_fold_templates(" in drv


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------
def words_hand():
    """A codebook whose entry says where it came from: words[m][k][d] = 1000 m + k + d / 8."""
    m, k, d = np.meshgrid(np.arange(16), np.arange(256), np.arange(6), indexing="ij")
    return (1000.0 * m + k + d / 8.0).astype(np.float32)


def make_print(rng, n_minu, n_tex):
    t = T.FPTemplate()
    if n_minu:
        t.minu.append(T.MinutiaeTemplate(rng.integers(0, 700, n_minu).astype(np.int16), rng.integers(0, 700, n_minu).astype(np.int16),
                                         rng.random(n_minu).astype(np.float32), rng.standard_normal((n_minu, 96)).astype(np.float32)))
    if n_tex:
        t.tex.append(T.TextureTemplate(rng.integers(0, 48, n_tex).astype(np.int16), rng.integers(0, 50, n_tex).astype(np.int16), rng.random(n_tex).astype(np.float32),
                                       codes=rng.integers(0, 256, (n_tex, 16)).astype(np.uint8)))
    return t


def test_the_decode_on_a_hand_made_codebook():
    w = words_hand()
    codes = np.zeros((3, 16), np.uint8); codes[1] = 255; codes[2] = np.arange(16) * 16 + 3
    des = P.decode(w, codes)
    assert des.shape == (3, 96) and des.dtype == np.float32
    for r in range(3):
        for f in range(96):                                                 # float f belongs to sub-quantizer f // 6, component f % 6
            assert des[r, f] == np.float32(1000.0 * (f // 6) + int(codes[r, f // 6]) + (f % 6) / 8.0)
    # bits, not numbers: NaN payloads, both zeros and subnormals pass through
    odd = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000], np.uint32).view(np.float32)
    w2 = w.copy(); w2[5, 9] = odd
    c2 = np.zeros((1, 16), np.uint8); c2[0, 5] = 9
    assert np.array_equal(P.decode(w2, c2)[0, 30:36].view(np.uint32), odd.view(np.uint32))
    # a float4 of a row is two 8-byte halves of at most two codewords (what the kernel's select relies on)
    for j in range(24):
        halves = {((4 * j + c) // 6, ((4 * j + c) % 6) // 2) for c in range(4)}
        assert len(halves) == 2 and len({m for m, _ in halves}) <= 2 and (4 * j) % 2 == 0


def test_the_view_and_the_group_on_hand_made_prints():
    rng = np.random.default_rng(3)
    w = words_hand()
    prints = [make_print(rng, 17, 9), make_print(rng, 0, 20), make_print(rng, 5, 0), T.FPTemplate(), make_print(rng, 16, 1100)]
    v = [P.view(p, w) for p in prints]
    assert [(len(x.minu), len(x.tex)) for x in v] == [(1, 1), (0, 1), (1, 0), (0, 0), (1, 1)]
    assert v[4].tex[0].n == 1000 and np.array_equal(v[4].tex[0].des, P.decode(w, prints[4].tex[0].codes[:1000]))        # the clamp at enrolment
    assert v[0].minu[0].des is not None and np.array_equal(v[0].minu[0].des.view(np.uint32), prints[0].minu[0].des.view(np.uint32))
    assert P.view_bytes(v[4]) == 16 * 392 + 1000 * 392
    g = P.group(prints, w)
    assert g["lm_off"].tolist() == [0, 17, 17, 17, 17, 17, 17, 22, 22, 22, 22, 22, 22, 38, 38, 38]
    assert g["lm_tile_off"].tolist() == [0, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 4, 4, 4]
    assert g["lt_off"].tolist() == [0, 9, 29, 29, 29, 1029] and g["tile_off"].tolist() == [0, 2, 5, 5, 5, 130] and g["tile16_off"].tolist() == [0, 1, 3, 3, 3, 66]
    assert g["tex_slot"].tolist() == [1, 0, -1, -1, 1] and g["status"].tolist() == [0] * 5 and g["lt_pad"] == 1000
    assert g["lm_des"].shape == (38, 96) and g["lt_des"].shape == (1029, 96) and g["lm_frag"].shape == (4, 6, 64, 4)
    # the fragment layout against a loop, and the zero rows of a last tile
    des = prints[0].minu[0].des
    fr = g["lm_frag"][:2]
    for tile in range(2):
        for vv in range(6):
            for lane in range(64):
                for c in range(4):
                    row = 16 * tile + (lane & 15)
                    want = des[row, 4 * (4 * vv + c) + (lane >> 4)] if row < 17 else np.float32(0)
                    assert fr[tile, vv, lane, c] == want
    assert (fr[1][:, (np.arange(64) & 15) >= 1] == 0).all()
    # what is not used takes no room: print 0 without its minutiae, print 4 without its texture; the texture slot still counts the view's minutiae template
    g2 = P.group(prints, w, use_minu=[0, 1, 1, 1, 1], use_tex=[1, 1, 1, 1, 0])
    assert g2["lm_off"].tolist()[:4] == [0, 0, 0, 0] and g2["lt_off"].tolist() == [0, 9, 29, 29, 29, 29] and g2["tex_slot"].tolist() == [1, 0, -1, -1, -1] and g2["lt_pad"] == 24


def test_the_plan_and_its_batches():
    rng = np.random.default_rng(5)
    prints = [make_print(rng, 4, 6), make_print(rng, 0, 6), make_print(rng, 4, 0), T.FPTemplate(), make_print(rng, 3, 3), make_print(rng, 2, 2)]
    wm = np.array([1, 1, 1, 1, 0, -0.0], np.float32); wt = np.array([0.3, 0.3, 0.3, 0.3, 0, 2], np.float32)
    qd, use, wtab = P.plan(prints, wm, wt)
    assert qd.tolist() == [[0, 1, 1, 0], [1, 1, 1, 0], [2, 1, 0, 0], [3, 0, 0, 1], [3, 0, 0, 1], [3, 1, 1, 0]]      # an empty print and a print with both weights zero: latent-empty
    assert use.tolist() == [[True, True], [False, True], [True, False], [False, True]]
    assert wtab.tolist() == [[1, 0, 0, np.float32(0.3)], [0, 0, 0, np.float32(0.3)], [1, 0, 0, 0], [0, 0, 0, 2]]
    assert W.batches(qd, 1) == [(0, 1), (1, 2), (2, 5), (5, 6)] and W.batches(qd, 3) == [(0, 5), (5, 6)] and W.batches(qd, 1 << 30) == [(0, 6)]
    # the bytes that cross PCIe do not grow with the point counts: ten padded tables per group, 32 bytes per query for the fold
    one = P.h2d_bytes(qd, 1 << 30)
    assert one == 6 * 16 + 4 * 16 + 4 * (2 * 16 + 3 * 8 + 5 * 4) and one <= 256 * len(qd) + 4096
    assert P.h2d_bytes(qd, 1) == 6 * 16 + 4 * 16 + 4 * 4 * (2 * 4 + 3 * 4 + 5 * 4)
    big = [make_print(rng, 80, 1000)] * 16
    qb, _, _ = P.plan(big, np.ones(16), np.ones(16))
    assert P.h2d_bytes(qb, 1 << 30) <= 128 * 16 + 16 * 32 + 64 and sum(P.view_bytes(P.view(p, words_hand())) for p in big) >= 16 * 100 * 1024
