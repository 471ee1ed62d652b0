"""Replace in place without a GPU: afis_gallery_commit_at is declared, exported by both libraries and bound by the Python host; the header carries the contract; the
splice kernel and its launcher are in gallery_edit.hip, beside the compaction kernel, and in the product objects; and gallery_splice_plan.h — validation, the offsets and
flags after the edit, the source tables — through the stand-alone program csrc/gallery_splice_plan_check, built with the host sanitizers and run as a program (nothing
is loaded into this process).  What the device answers is tests/test_gpu_gallery_replace.py's."""
import importlib
import os
import re
import subprocess

M = importlib.import_module("msu-latentafis_amd.host.matcher")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msu-latentafis_amd", "csrc")
NAME = "afis_gallery_commit_at"


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = _read("include", "afis_matcher.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+afis_gallery_commit_at\s*\(afis_ctx\*\s*ctx,\s*const int64_t\*\s*idx\s*,\s*int64_t\s+n\s*\)\s*;", code)
    assert hdr.index("int afis_gallery_remove(") < hdr.index("int afis_gallery_commit_at(") < hdr.index("int afis_gallery_export(")
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):         # dlopen only: no device call
        assert NAME in M.EXPORTS and hasattr(lib, NAME) and len(getattr(lib, NAME).argtypes) == 3
    assert NAME not in M.TAP_EXPORTS and hasattr(M.Matcher, "gallery_commit_at")
    taps = _read("include", "afis_matcher_taps.h")
    tap = taps[:taps.index("int afis_debug_compact_stats(")]
    assert NAME in tap[tap.rindex("/*"):]                                   # the tap's note says that it reports the splice launches too


def test_the_header_carries_the_contract():
    hdr = _read("include", "afis_matcher.h")
    para = hdr[hdr.index("/* Replace enrolled prints in place"):hdr.index("int afis_gallery_commit_at(")]
    flat = re.sub(r"\s*\n \*\s*", " ", para)
    for phrase in ("staged template i takes the place of resident entry idx[i]", "in any order", "Nothing is appended", "every other template its index",
                   "bit for bit those of a fresh commit", "byte for byte", "makes the entry an empty entry", "re-enrolment at that index", "minutiae-only and texture-only",
                   "AFIS_EINVAL, nothing changed", "idx NULL with n > 0", "n not the number of staged templates", "[index_base, index_base + G)", "an index listed twice",
                   "2^31 - 1 minutiae or texture points", "AFIS_ESTATE, nothing changed", "not committed", "not reopened", "nothing staged", "still appends what is staged",
                   "afis_queries_upload_reserved", "built again", "no longer reopened", "gallery_h2d_bytes", "csrc/gallery_edit.hip", "one array plus the staged points",
                   "before the first array has been switched the old shard is intact", "the resident shard is dropped", "profiles/gallery_replace_timing.json"):
        assert phrase in flat, phrase
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "`%s`" % NAME in _read(doc), doc
    assert "k_splice_ranges" in _read("README.md") and "k_splice_ranges" in _read("DESIGN.md")


def test_the_splice_kernel_is_in_gallery_edit_and_in_the_product():
    mk = _read("msu-latentafis_amd", "csrc", "Makefile")
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "gallery_edit.o" in objs and "afis_gallery.o" in objs
    assert re.search(r"^afis_gallery\.o:.*gallery_splice_plan\.h", mk, flags=re.M)
    edit = _read("msu-latentafis_amd", "csrc", "gallery_edit.hip")
    assert edit.index("void k_compact_ranges(") < edit.index("void k_splice_ranges(") < edit.index("hipError_t launch_splice_ranges(")
    launcher = edit[edit.index("hipError_t launch_splice_ranges("):]
    # the three element widths and points per workgroup of the compaction
    assert re.search(r"kPts = 64;.*\n.*k_splice_ranges<uint4, kDes \* 4 / 16, kPts>", launcher)
    assert re.search(r"kPts = 1024;.*\n.*k_splice_ranges<uint4, 1, kPts>", launcher)
    assert re.search(r"kPts = 2048;.*\n.*k_splice_ranges<uint32_t, 1, kPts>", launcher)
    assert "launch_splice_ranges(" in _read("msu-latentafis_amd", "csrc", "afis_device.h")
    gal = _read("msu-latentafis_amd", "csrc", "afis_gallery.cpp")
    body = gal[gal.index("int afis_gallery_commit_at("):gal.index("int afis_gallery_export(")]
    for call in ("plan_gallery_splice(", "quiesce(", "launch_splice_ranges(", "launch_fragment_tiles(", "launch_mf_tiles(", "invalidate_lazy_streams(", "++ctx->gallery_epoch",
                 "release_staging(", "ctx->compact_us ="):
        assert call in body, call
    # the removal still launches the compaction, and only it
    rem = gal[gal.index("int afis_gallery_remove("):gal.index("int afis_gallery_commit_at(")]
    assert "launch_compact_ranges(" in rem and "launch_splice_ranges(" not in rem


def test_gallery_splice_plan_check_runs_clean_under_the_host_sanitizers():
    exe = os.path.join(CSRC, "gallery_splice_plan_check")
    src = [os.path.join(CSRC, f) for f in ("gallery_splice_plan_check.cpp", "gallery_splice_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in src):
        subprocess.run(["make", "-s", "-C", CSRC, "gallery_splice_plan_check"], check=True)
    mk = _read("msu-latentafis_amd", "csrc", "Makefile")
    assert "gallery_splice_plan_check" in re.search(r"^all:(.*)$", mk, flags=re.M).group(1).split()
    assert "gallery_splice_plan_check" in mk[mk.index("\nclean:"):]
    rule = mk[mk.index("\ngallery_splice_plan_check:"):]
    assert "-fsanitize=address,undefined" in rule[:rule.index("\n\n")] and "-fno-sanitize-recover=undefined" in rule[:rule.index("\n\n")]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"gallery_splice_plan_check: \d+ cases ok", out.stdout), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert int(re.search(r"(\d+) cases ok", out.stdout).group(1)) >= 400
    hdr = open(src[1]).read()
    assert not re.search(r'#include\s*[<"](hip|afis_)', hdr)                  # device-free: no runtime header, none of the project's device headers
    prog = open(src[0]).read()
    for case in ("one in the middle", "ends and a run, not ascending", "tile borders", "empty onto live", "live onto empty", "minutiae-only <-> texture-only", "every count kept",
                 "n == G", "a shard of one entry", "null idx", "fewer indices than staged", "more indices than staged", "below the shard", "behind the shard", "twice",
                 "minutiae beyond the limit", "texture points beyond the limit", "32-point tiles beyond the limit", "random"):
        assert '"%s' % case in prog, case
