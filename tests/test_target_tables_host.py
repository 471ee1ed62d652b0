"""The host tables of the calls that read the last search's matrix, without a GPU: target_tables.h — the targets of a call as a CSR by row — and column_names.h — the
column a name refers to — go through the stand-alone program csrc/target_tables_check, built with the host sanitizers and run as a program (nothing is loaded into this
process); both headers are device-free, and the three host units that resolve names do it through the one view.  What the device computes from the tables is
tests/test_gpu_rank_positions.py's, test_gpu_score_hist.py's and test_gpu_link_groups.py's."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")


def test_target_tables_check_runs_clean_under_the_host_sanitizers():
    exe = os.path.join(CSRC, "target_tables_check")
    src = [os.path.join(CSRC, f) for f in ("target_tables_check.cpp", "target_tables.h", "column_names.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in src):
        subprocess.run(["make", "-s", "-C", CSRC, "target_tables_check"], check=True)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("\ntarget_tables_check:"):]
    rule = rule[:rule.index("\n\n")]
    for flag in ("-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"):
        assert flag in rule.split(), flag
    assert re.search(r"^all:.*\btarget_tables_check\b", mk, flags=re.M) and re.search(r"^\trm -f .*\btarget_tables_check\b", mk, flags=re.M)
    assert "target_tables_check" in open(os.path.join(CSRC, ".gitignore")).read().split()
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"^target_tables_check: \d+ cases ok$", out.stdout, flags=re.M), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert int(re.search(r"(\d+) cases ok", out.stdout).group(1)) >= 600      # the named cases and some hundreds of random ones
    main = open(src[0]).read()
    assert "int main(" in main
    for case in ("no targets", "one target", "every target in one row", "every row exactly one target", "repeated (row, key) pairs", "rows given in descending order",
                 "a device list that skips targets", "below base", "base + n", "absent names", "its first and last element", "an empty name list", "random "):
        assert case in main, case


def test_the_headers_are_device_free_and_the_names_have_one_resolver():
    for hdr in ("target_tables.h", "column_names.h"):
        text = open(os.path.join(CSRC, hdr)).read()
        assert not re.search(r'#include\s*[<"](hip|afis_)', text) and not re.findall(r'#include\s+"([^"]+)"', text), hdr     # the standard library only
    assert '#include "column_names.h"' in open(os.path.join(CSRC, "link_groups.h")).read()
    units = {f: open(os.path.join(CSRC, f)).read() for f in ("afis_filter.cpp", "afis_positions.cpp", "afis_link.cpp")}
    for f, text in units.items():
        assert "column_names(ctx," in text and "std::lower_bound" not in text and "std::sort(held" not in text, f
    assert len(re.findall(r"^ColumnNames column_names\(", units["afis_filter.cpp"], flags=re.M)) == 1
    for f in ("afis_positions.cpp", "afis_distribution.cpp"):
        text = open(os.path.join(CSRC, f)).read()
        assert "build_target_tables(" in text and "stable_sort" not in text, f
