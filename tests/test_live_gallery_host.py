"""The live gallery's surface without a GPU: the three entry points are declared, exported by both libraries and bound by the Python host; the compaction
kernels are part of the product objects.  (What they compute is tests/test_gpu_live_gallery.py's.)"""
import importlib
import os
import re

M = importlib.import_module("msu-latentafis_amd.host.matcher")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["afis_gallery_reopen", "afis_gallery_remove", "afis_gallery_export"]


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "afis_matcher.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for lib in (M.load_library(), M.load_library(M.TEST_LIB_PATH)):        # dlopen only: no device call
        for name in NEW:
            assert re.search(r"\bint\s+%s\s*\(afis_ctx\*" % name, code), name
            assert name in M.EXPORTS and hasattr(lib, name)
            assert getattr(lib, name).argtypes is not None, name
    for method in ("gallery_reopen", "gallery_remove", "gallery_export", "resident_size"):
        assert hasattr(M.Matcher, method), method
    for option in ("gallery_h2d_bytes", "gallery_resident"):
        assert '"%s"' % option in hdr, option


def test_compaction_kernels_are_product_objects():
    mk = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "gallery_edit.o" in objs
    src = open(os.path.join(ROOT, "msu-latentafis_amd", "csrc", "gallery_edit.hip")).read()
    assert "__global__" in src and "launch_compact_ranges" in src
