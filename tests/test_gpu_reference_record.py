"""GPU: the HIP path against the RECORD of the reference's own matcher.cpp (tests/golden/golden_matcher_ref.npz), directly — not through the oracle.  The
reference does not exist on the GPU machine; these tests read the record and regenerate the inputs from tests/cases.py (whose bytes the CPU tests of
tests/test_reference_record.py hold to the recorded sha256).

With option ref_tie_order 2 the device takes equal sort keys in std::sort's order at S3, S8 and S9, which is the reference's result on every pair of every set
used here (tests/test_reference_record.py asserts that for the oracle's tie mode 9, with no pair left out).  Everything is equality of bit patterns or of
printed digits."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
T = cases.T
M = importlib.import_module("msu-latentafis_amd.host.matcher")
GPU_SETS = [n for n in cases.RECORD_SETS if not n.endswith("_s7")]            # the *_s7 sets are the CPU-only ones (RecordSet.gpu is False), see tests/cases.py
LIST_SETS = ["golden", "structured10", "structured30", "shapes_degenerate_keys", "shapes_tied_maxima", "shapes_texture_spread", "shapes_s9_limits", "shapes_s2_rounding"]


@pytest.fixture(scope="module")
def rec():
    return cases.load_reference_record()


def _expected(rec, name):
    info, status, scores = rec[f"{name}/info"], rec[f"{name}/status"], rec[f"{name}/scores"]
    return np.stack([cases.record_parts(scores[0, k], info[k], status[k]) for k in range(len(status))]), status


def _got(res, pairs):
    return np.stack([np.append(res["parts"][i, j], res["scores"][i, j]).astype(np.float32).view(np.uint32) for i, j in pairs])


def _loaded(rs, taps=False):
    m = M.Matcher(rs.cbb, taps=taps)
    for b in rs.rol:
        m.gallery_add_dat(b)
    m.gallery_commit(0)
    return m


@pytest.mark.parametrize("name", GPU_SETS)
def test_scores_equal_the_reference_record(rec, name):
    """Per-part and fused scores (the whole vector in all-templates mode) of every recorded pair with ref_tie_order 2; status 1 / 2 as the record's; and the default
    order on the pairs the record marks as unaffected by it."""
    rs = cases.record_set(name)
    assert rs.gpu and all(cases.record_set(n).gpu != n.endswith("_s7") for n in cases.RECORD_SETS)
    m = _loaded(rs)
    info, scores, slen, m1 = rec[f"{name}/info"], rec[f"{name}/scores"], rec[f"{name}/score_len"], rec[f"{name}/mode1_equal"]
    for tie in (0, 2):
        if tie: m.set_option("ref_tie_order", tie)
        if rs.mode == "all":
            status = rec[f"{name}/status"]
            for i in range(len(rs.lat)):
                L = T.read_latent(rs.lat[i])[1]
                qs, rst, sc = m.One2One_matching_all_templates(L)
                for k, (pi, pj) in enumerate(rs.pairs):
                    if pi != i or not (tie or m1[k]): continue
                    assert (1 if qs == 1 else int(rst[pj])) == status[k]
                    assert np.array_equal(sc[pj].view(np.uint32), scores[0, k, :slen[k]]), (name, tie, pi, pj, sc[pj], scores[0, k, :slen[k]].view(np.float32))
            continue
        want, status = _expected(rec, name)
        res = m.search_dat(rs.lat, k=0, want_parts=True)
        got = _got(res, rs.pairs)
        for k, (i, j) in enumerate(rs.pairs):
            if not (tie or m1[k]): continue
            if status[k] == 1:
                assert res["status"][i] == 1 and res["scores"][i, j] == -1.0
                continue
            assert res["status"][i] == 0, (name, i)
            if status[k] == 2:
                assert res["scores"][i, j] == -1.0
                continue
            assert np.array_equal(got[k], want[k]), (name, tie, i, j, got[k].view(np.float32), want[k].view(np.float32))
    print(f"{name}: {len(rs.pairs)} pairs against the record with ref_tie_order 2 (none left out), {int(m1.sum())} of them with the default order as well")
    m.close()


def test_every_recorded_gpu_pair_is_compared(rec):
    n = sum(len(rec[f"{s}/pairs"]) for s in GPU_SETS)
    assert n == sum(len(cases.record_set(s).pairs) for s in GPU_SETS) and n >= 780
    print("pairs compared against the record on the GPU:", n)


@pytest.mark.parametrize("name", LIST_SETS)
def test_stage_lists_equal_the_reference_record(rec, name):
    """debug_stage_list (the lists after S3 / S7, S8, S9) against the lists the reference's own stage functions were fed and returned.  Lists in which S7's order of
    exactly equal row maxima shows (flagged in the record, texture lists of the tied-row-maxima inputs only) are the one thing the device does not reproduce."""
    rs = cases.record_set(name)
    m = _loaded(rs, taps=True)
    m.set_option("ref_tie_order", 2)
    off, sim, li, ri = (rec[f"{name}/lists_{f}"] for f in ("off", "sim", "li", "ri"))
    flags = rec[f"{name}/lists_mode9_equal"]
    lat = {}
    n = 0
    for row, (k, which, stage, fed, got) in enumerate(rec[f"{name}/lists_index"]):
        i, j = rs.pairs[k]
        L = lat.setdefault(i, T.read_latent(rs.lat[i])[1])
        for col, (st, t) in enumerate(((stage - 1, fed), (stage, got))):
            if not flags[row, col]: continue
            g = m.debug_stage_list(L, int(j), int(which), int(st))
            assert g is not None, (name, i, j, which, st)
            s = slice(off[t], off[t + 1])
            assert np.array_equal(g[1], li[s]) and np.array_equal(g[2], ri[s]), (name, i, j, which, st)
            assert np.array_equal(g[0].view(np.uint32), sim[s]), (name, i, j, which, st)
            n += 1
    print(f"{name}: {n} of {2 * len(flags)} recorded lists compared")
    assert n >= 0.8 * 2 * len(flags)
    m.close()


def test_correspondence_files_equal_the_reference_record(rec):
    """The correspondence export (matcher.cpp:497-505) of the golden pairs, as the text of the reference's three CSVs per pair."""
    name = "golden"
    rs = cases.record_set(name)
    m = _loaded(rs)
    m.set_option("ref_tie_order", 2)
    offs, blob, present = rec[f"{name}/corr_off"], rec[f"{name}/corr_text"], rec[f"{name}/corr_present"]
    n_lines = 0
    for i in range(len(rs.lat)):
        got = m.correspondences(T.read_latent(rs.lat[i])[1], list(range(len(rs.rol))))
        for k, (pi, pj) in enumerate(rs.pairs):
            if pi != i: continue
            for s in range(3):
                if not present[k, s]:
                    assert got[pj][s] is None
                    continue
                t = 3 * k + s
                want = bytes(blob[offs[t]:offs[t + 1]]).decode()
                text = "".join("%d,%d,%d,%d\n" % tuple(r) for r in got[pj][s])
                assert text == want, (pi, pj, s)
                n_lines += len(got[pj][s])
    assert n_lines > 50
    m.close()


@pytest.mark.parametrize("name", ["golden", "small"])
def test_cli_directory_mode_equals_the_reference_record(rec, name, tmp_path):
    """`match -ldir ... -tie 2`: the digits after each rolled file name are those of the reference's List2List_matching score files, -1.000 for the empty file and
    for the file whose texture count is 2001 included."""
    rs = cases.record_set(name)
    exe = os.path.join(os.path.dirname(M.LIB_PATH), "match")
    for d in ("gal", "lat", "out", "work"): (tmp_path / d).mkdir()
    for j, b in enumerate(rs.rol): (tmp_path / "gal" / cases.record_rolled_name(j)).write_bytes(b)
    for n, b in rs.list2list["extra"].items(): (tmp_path / "gal" / n).write_bytes(b)
    lat_ids = rec[f"{name}/l2l_latents"].tolist()
    for i in lat_ids: (tmp_path / "lat" / cases.record_latent_name(i)).write_bytes(rs.lat[i])
    (tmp_path / "cb.dat").write_bytes(rs.cbb)
    o = subprocess.run([exe, "-ldir", str(tmp_path / "lat"), "-g", str(tmp_path / "gal"), "-c", str(tmp_path / "cb.dat"), "-s", str(tmp_path / "out") + "/", "-tie", "2"],
                       capture_output=True, text=True, cwd=tmp_path / "work", timeout=600)
    assert o.returncode == 0, o.stderr
    names, digits = rec[f"{name}/l2l_names"].tolist(), rec[f"{name}/l2l_digits"]
    for a, i in enumerate(lat_ids):
        lines = (tmp_path / "out" / (os.path.splitext(cases.record_latent_name(i))[0] + ".csv")).read_text().splitlines()
        got = {os.path.basename(l.rsplit(",", 1)[0].strip('"')): l.rsplit(",", 1)[1] for l in lines}             # keyed by file name: directory order is the file system's
        assert got == {n: digits[a, b].decode() for b, n in enumerate(names)}, (name, i)
