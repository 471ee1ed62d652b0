"""The oracle (oracle/afis_oracle.cpp) against the RECORD of the reference's own matcher.cpp (tests/golden/golden_matcher_ref.npz, made by
tests/golden/make_golden_matcher_ref.py from the reference's unmodified translation unit on the stand-in headers of oracle/standin/).

Everything here is equality of bit patterns, of index lists or of printed digits; nothing has a tolerance.  The tests read the record and regenerate the
inputs from tests/cases.py; they need neither the reference tree nor a GPU.  What the record cannot pin is Eigen's own summation order: the sums
matcher.cpp leaves to Eigen are taken by the stand-in, in the order family the oracle documents ("accumulation orders")."""
import hashlib

import numpy as np
import pytest

import cases

T = cases.T
SETS = list(cases.RECORD_SETS)
SEL = (26, 2, 11)


@pytest.fixture(scope="module")
def rec():
    return cases.load_reference_record()


_handles = {}


def _orc(oracle, name):
    """(record set, oracle codebook, latent handles + return codes, rolled handles + return codes), parsed once per set."""
    if name not in _handles:
        rs = cases.record_set(name)
        ocb = oracle.codebook(rs.cbb)
        _handles[name] = (rs, ocb, [oracle.latent(ocb, b) for b in rs.lat], [oracle.rolled(b) for b in rs.rol])
    return _handles[name]


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def test_the_record_has_every_set(rec):
    assert sorted(rec["sets"].tolist()) == sorted(SETS)
    assert sum(len(rec[f"{n}/pairs"]) for n in SETS) >= 800


@pytest.mark.parametrize("name", SETS)
def test_regenerated_inputs_have_the_recorded_sha256(rec, name):
    """A generator that drifts must be loud: the record's results belong to exactly these bytes."""
    rs = cases.record_set(name)
    assert _sha(rs.cbb) == str(rec[f"{name}/sha_cb"])
    assert [_sha(b) for b in rs.lat] == rec[f"{name}/sha_lat"].tolist()
    assert [_sha(b) for b in rs.rol] == rec[f"{name}/sha_rol"].tolist()
    assert np.array_equal(np.array(rs.pairs, np.int32).reshape(-1, 2), rec[f"{name}/pairs"]) and list(rs.orders) == rec[f"{name}/orders"].tolist()
    if rs.list2list is not None:
        assert [_sha(rs.list2list["extra"][n]) for n in sorted(rs.list2list["extra"])] == rec[f"{name}/l2l_extra_sha"].tolist()


def _expected_vector(parts, n_lm, n_lt):
    """The score vector of matcher.cpp:376-417 from the oracle's four parts: slots 0..2 where the latent has template 26 / 2 / 11, then the texture score at
    slot n_lm (written last, so it wins when n_lm <= 2)."""
    v = np.zeros(n_lm + n_lt, np.float32)
    for i in range(3):
        if n_lm > SEL[i]: v[i] = parts[i]
    if n_lt > 0: v[n_lm] = parts[3]
    return v


@pytest.mark.parametrize("name", SETS)
def test_oracle_tie_mode_0_equals_the_record(rec, oracle, name):
    """std::sort at every site (tie mode 0), every recorded accumulation order: status, loaders' return codes and template counts, the WHOLE score vector of every
    pair (so also where the texture score lands), and the fused score wherever the reference defines it (29 slots or more, matcher.cpp:188)."""
    rs, ocb, hl, hr = _orc(oracle, name)
    info, status, scores, slen = rec[f"{name}/info"], rec[f"{name}/status"], rec[f"{name}/scores"], rec[f"{name}/score_len"]
    n_fused = 0
    for k, (i, j) in enumerate(rs.pairs):
        assert (hl[i][1], hr[j][1]) == (info[k][0], info[k][1]), (name, i, j)
        assert oracle.counts(hl[i][0]) == (info[k][2], info[k][3]) and oracle.counts(hr[j][0], rolled=True) == (info[k][4], info[k][5]), (name, i, j)
        assert slen[k] == info[k][2] + info[k][3]
        for oi, order in enumerate(rs.orders):
            want = scores[oi, k, :slen[k]]
            assert not scores[oi, k, slen[k]:].any()
            if rs.mode == "all":
                rc, v = oracle.all_templates(ocb, hl[i][0], hr[j][0], int(slen[k]), tie_mode=0 | order << 4)
                assert rc == status[k]
                assert np.array_equal(v.view(np.uint32), want), (name, i, j, order, v, want.view(np.float32))
                continue
            rc, parts = oracle.pair(ocb, hl[i][0], hr[j][0], 0 | order << 4)
            assert rc == status[k], (name, i, j)
            got = _expected_vector(parts, int(info[k][2]), int(info[k][3]))
            assert np.array_equal(got.view(np.uint32), want), (name, i, j, order, got, want.view(np.float32))
            if rc == 0 and slen[k] >= 29:
                assert parts[4:5].view(np.uint32)[0] == cases.record_parts(scores[oi, k], info[k], status[k])[4], (name, i, j, order)
                n_fused += 1
    if name in ("golden", "small", "structured10", "structured30"):
        assert n_fused == len(rs.pairs) * len(rs.orders)


def test_golden_orders_are_distinguishable(rec):
    """The six accumulation orders are really different computations on the golden pairs: every order 1..5 moves at least one recorded score away from order 0."""
    s = rec["golden/scores"]
    assert rec["golden/orders"].tolist() == [0, 1, 2, 3, 4, 5]
    for oi in range(1, 6):
        assert (s[oi] != s[0]).any(), oi


def test_committed_golden_vectors_are_reference_outputs(rec):
    """tests/golden/golden_pairs.npz["parts"][0] (made by the oracle, tie mode 0) is what the reference computes on the same bytes."""
    gold = cases._golden_npz()["parts"][0].view(np.uint32)
    info, status, scores = rec["golden/info"], rec["golden/status"], rec["golden/scores"]
    for k, (i, j) in enumerate(rec["golden/pairs"]):
        assert np.array_equal(gold[i, j], cases.record_parts(scores[0, k], info[k], status[k])), (i, j)


@pytest.mark.parametrize("name", ["golden", "small"])
def test_list2list_digits(rec, oracle, name):
    """List2List_matching's score files: the digits after each rolled file name equal "%.3f" of the oracle's fused score; -1.000 for files the loader refuses
    (an empty file: code 1, no templates; a texture count of 2001: code -1, matcher.cpp:173-177)."""
    rs, ocb, hl, hr = _orc(oracle, name)
    names, digits = rec[f"{name}/l2l_names"].tolist(), rec[f"{name}/l2l_digits"]
    extra = rs.list2list["extra"]
    assert names == [cases.record_rolled_name(j) for j in range(len(rs.rol))] + sorted(extra)
    for a, i in enumerate(rec[f"{name}/l2l_latents"]):
        for b, n in enumerate(names):
            if b < len(rs.rol):
                rc, parts = oracle.pair(ocb, hl[i][0], hr[b][0], 0)
            else:
                h, lrc = oracle.rolled(extra[n])
                if lrc < 0:                                        # the reference's caller zeroes the counts (matcher.cpp:173-177); so does the project's reader
                    assert T.read_rolled(extra[n])[1].minu == [] and T.read_rolled(extra[n])[1].tex == []
                    rc = 2
                else:
                    rc, parts = oracle.pair(ocb, hl[i][0], h, 0)
                assert rc == 2, n
            want = "-1.000" if rc == 2 else "%.3f" % parts[4]
            assert digits[a, b].decode() == want, (name, i, n)
    if extra:
        assert oracle.rolled(extra["R_empty.dat"])[1] == 1 and oracle.rolled(extra["R_tex2001.dat"])[1] == -1


def _lists(rec, name):
    off, sim, li, ri = (rec[f"{name}/lists_{f}"] for f in ("off", "sim", "li", "ri"))
    get = lambda t: (sim[off[t]:off[t + 1]], li[off[t]:off[t + 1]].astype(np.int32), ri[off[t]:off[t + 1]].astype(np.int32))
    return rec[f"{name}/lists_index"], get


def _same_list(trace, want):
    return trace is not None and np.array_equal(trace[0].view(np.uint32), want[0]) and np.array_equal(trace[1], want[1]) and np.array_equal(trace[2], want[2])


@pytest.mark.parametrize("name", ["golden", "structured10", "structured30", "shapes_degenerate_keys", "shapes_tied_maxima", "shapes_tied_maxima_s7", "shapes_texture_spread", "shapes_s9_limits", "shapes_s2_rounding"])
def test_stage_lists(rec, oracle, name):
    """The reference's own LSS_R_Fast2_Dist_lookup / _eigen (S8) and LSS_R_Fast2 (S9), each fed the oracle's previous stage, return the oracle's next stage: members,
    order, similarity bits.  The record keeps the list that was fed in, so a changed S3 / S7 list shows here as such and not as a later stage's fault."""
    rs, ocb, hl, hr = _orc(oracle, name)
    index, get = _lists(rec, name)
    seen = set()
    for k, which, stage, fed, got in index:
        i, j = rs.pairs[k]
        before = oracle.trace(ocb, hl[i][0], hr[j][0], which=int(which), stage=int(stage) - 1, tie_mode=0)
        after = oracle.trace(ocb, hl[i][0], hr[j][0], which=int(which), stage=int(stage), tie_mode=0)
        assert _same_list(before, get(fed)), (name, i, j, which, stage, "the list fed to the reference is no longer the oracle's")
        assert _same_list(after, get(got)), (name, i, j, which, stage)
        seen.add((int(k), int(which)))
    assert {k for k, _ in seen} == {rs.pairs.index(p) for p in rs.stage_pairs}
    for k in {k for k, _ in seen}:                                  # every scorer the pair has: texture and the three minutiae templates where they exist
        i, j = rs.pairs[k]
        for which in range(4):
            assert ((k, which) in seen) == (oracle.trace(ocb, hl[i][0], hr[j][0], which=which, stage=0, tie_mode=0) is not None)


def _corr_text(rec, name, k, s):
    off, blob = rec[f"{name}/corr_off"], rec[f"{name}/corr_text"]
    t = 3 * k + s
    return bytes(blob[off[t]:off[t + 1]]).decode() if rec[f"{name}/corr_present"][k, s] else None


def test_correspondence_files(rec, oracle):
    """The three CSVs of matcher.cpp:497-505 (save_corr): the coordinates of the oracle's stage-2 lists, line for line."""
    name = "golden"
    rs, ocb, hl, hr = _orc(oracle, name)
    n_lines = 0
    for k, (i, j) in enumerate(rs.pairs):
        _, L = T.read_latent(rs.lat[i]); _, R = T.read_rolled(rs.rol[j])
        for s in range(3):
            tr = oracle.trace(ocb, hl[i][0], hr[j][0], which=s + 1, stage=2, tie_mode=0)
            text = _corr_text(rec, name, k, s)
            assert (tr is None) == (text is None)
            if tr is None: continue
            lm, rm = L.minu[SEL[s]], R.minu[0]
            want = "".join(f"{lm.x[a]},{lm.y[a]},{rm.x[b]},{rm.y[b]}\n" for a, b in zip(tr[1], tr[2]))
            assert text == want, (i, j, s)
            n_lines += len(tr[1])
    assert n_lines > 50


@pytest.mark.parametrize("name", SETS)
def test_tie_mode_9_equals_the_record_on_the_sets_the_gpu_tests_use(rec, oracle, name):
    """Option ref_tie_order 2 delivers the oracle's tie mode 9 (std::sort at S3, S8 and S9; ascending index at S7, whose std::sort order the device does not
    reproduce).  On every pair of every set the GPU tests hold against the record that must be the reference's result: no pair is left out.  (The sets marked
    gpu=False in tests/cases.py are the same inputs at seeds where S7's order does decide a score; they are there for the tie-mode-0 comparison above.)"""
    rs, ocb, hl, hr = _orc(oracle, name)
    info, status, scores, slen = rec[f"{name}/info"], rec[f"{name}/status"], rec[f"{name}/scores"], rec[f"{name}/score_len"]
    differs = 0
    for k, (i, j) in enumerate(rs.pairs):
        if rs.mode == "all":
            rc, v = oracle.all_templates(ocb, hl[i][0], hr[j][0], int(slen[k]), tie_mode=9)
            differs += int(rc != status[k] or not np.array_equal(v.view(np.uint32), scores[0, k, :slen[k]]))
        else:
            rc, parts = oracle.pair(ocb, hl[i][0], hr[j][0], 9)
            differs += int(rc != status[k] or not np.array_equal(_expected_vector(parts, int(info[k][2]), int(info[k][3])).view(np.uint32), scores[0, k, :slen[k]]))
    if rs.gpu:
        assert differs == 0, (name, differs)
    else:
        assert differs > 0, (name, "S7's order no longer decides a pair here: the set has lost its purpose")


@pytest.mark.parametrize("name", SETS)
def test_distance_of_the_default_order_from_the_reference_is_the_recorded_count(rec, oracle, name):
    """The default order (tie mode 1: equal keys by ascending index) is NOT the reference's; how many pairs it moves is counted by the recorder and must stay that
    count, pair by pair (the GPU tests use the mask to hold the default path against the record where the two agree)."""
    rs, ocb, hl, hr = _orc(oracle, name)
    info, status, scores, slen = rec[f"{name}/info"], rec[f"{name}/status"], rec[f"{name}/scores"], rec[f"{name}/score_len"]
    eq = np.zeros(len(rs.pairs), bool)
    for k, (i, j) in enumerate(rs.pairs):
        if rs.mode == "all":
            rc, v = oracle.all_templates(ocb, hl[i][0], hr[j][0], int(slen[k]), tie_mode=1)
            eq[k] = rc == status[k] and np.array_equal(v.view(np.uint32), scores[0, k, :slen[k]])
        else:
            rc, parts = oracle.pair(ocb, hl[i][0], hr[j][0], 1)
            eq[k] = rc == status[k] and (rc != 0 or np.array_equal(parts[:4].view(np.uint32), cases.record_parts(scores[0, k], info[k], status[k])[:4]))
    assert np.array_equal(eq, rec[f"{name}/mode1_equal"]) and int((~eq).sum()) == int(rec[f"{name}/n_mode1_differs"])


@pytest.mark.parametrize("name", ["golden", "structured10", "structured30", "shapes_degenerate_keys", "shapes_tied_maxima", "shapes_tied_maxima_s7", "shapes_texture_spread", "shapes_s9_limits", "shapes_s2_rounding"])
def test_stage_lists_under_tie_mode_9_are_flagged_pair_by_pair(rec, oracle, name):
    """Which recorded lists are also tie mode 9's (the GPU test holds the device's lists against exactly those): recomputed here, list by list.  The only lists that
    are not are texture lists (scorer 0) of the tied-row-maxima inputs, where S7's std::sort order of exactly equal keys shows in the list itself."""
    rs, ocb, hl, hr = _orc(oracle, name)
    index, get = _lists(rec, name)
    flags = rec[f"{name}/lists_mode9_equal"]
    for row, (k, which, stage, fed, got) in enumerate(index):
        i, j = rs.pairs[k]
        for col, (st, t) in enumerate(((stage - 1, fed), (stage, got))):
            assert _same_list(oracle.trace(ocb, hl[i][0], hr[j][0], which=int(which), stage=int(st), tie_mode=9), get(t)) == flags[row, col], (name, i, j, which, st)
    if not name.startswith("shapes_tied_maxima"):
        assert flags.all()
    else:
        assert flags[index[:, 1] != 0].all() and not flags.all()


def test_loaders_on_edge_files(rec, oracle):
    """Return code and template counts of the reference's own loaders on files at their edges: the oracle's parser and the Python reader (host/templates.py) say the same."""
    cbb = cases._shipped_bytes()
    files, _, _ = cases.loader_edge_files(T.Codebook.from_bytes(cbb))
    assert list(files) == rec["loaders/names"].tolist() and [_sha(b) for _, b in files.values()] == rec["loaders/sha"].tolist()
    ocb = oracle.codebook(cbb)
    for (name, (kind, b)), want in zip(files.items(), rec["loaders/rc_counts"].tolist()):
        if kind == "latent":
            h, rc = oracle.latent(ocb, b); prc, t = T.read_latent(b)
            got = [rc, *oracle.counts(h)]
        else:
            h, rc = oracle.rolled(b); prc, t = T._read(b, rolled=True)
            got = [rc, *oracle.counts(h, rolled=True)]
            if want[0] < 0:                                        # the oracle's rolled entry point includes the caller's rule (matcher.cpp:173-177): a negative code empties the template
                assert got == [want[0], 0, 0], (name, got)
                got = want
        assert got == want, (name, got, want)
        assert [prc, len(t.minu), len(t.tex)] == want, (name, prc, len(t.minu), len(t.tex), want)
    codes = {n: w[0] for n, w in zip(files, rec["loaders/rc_counts"].tolist())}
    assert codes["rolled_empty"] == 1 and codes["rolled_10_bytes"] == 1 and codes["rolled_minutiae_2001"] == 2 and codes["rolled_texture_2001"] == -1 and codes["latent_empty"] == 1
