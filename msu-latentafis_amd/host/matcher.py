"""ctypes binding of libafis_hip.so (include/afis_matcher.h) with the reference's `PQ::Matcher` surface.

Mirrors matching/matcher.h:35-51: Matcher(code_file), One2List_matching, List2List_matching, plus the in-memory
calls the C ABI adds (gallery add/commit, batched search).  There is NO CPU fallback: if the HIP library is missing
or no gfx950 device is present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .templates import Codebook, FPTemplate, read_latent, read_rolled

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libafis_hip.so")            # the product: include/afis_matcher.h, nothing else
TEST_LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libafis_hip_test.so")  # the same objects + the parity taps (include/afis_matcher_taps.h); tests only


class AfisError(RuntimeError):
    pass


CORR_NOT_RUN, CORR_NOT_COVERED = -1, -2                                     # AFIS_CORR_NOT_RUN, AFIS_CORR_NOT_COVERED (include/afis_matcher.h)
PAIR_OK, PAIR_NOT_COVERED = 0, 1                                            # AFIS_PAIR_OK, AFIS_PAIR_NOT_COVERED


class _NotCovered:
    """What correspondences_pairs lists for a pair whose template this shard does not hold (AFIS_CORR_NOT_COVERED): distinct from None, the reference's "no file"."""
    def __repr__(self):
        return "NOT_COVERED"

    def __bool__(self):
        return False


NOT_COVERED = _NotCovered()
CASE_SUM, CASE_MAX = 0, 1                                                   # AFIS_CASE_SUM, AFIS_CASE_MAX (include/afis_matcher.h)


class MinutiaeView(C.Structure):
    _fields_ = [("n", C.c_int32), ("x", C.POINTER(C.c_int16)), ("y", C.POINTER(C.c_int16)), ("ori", C.POINTER(C.c_float)),
                ("des_len", C.c_int32), ("des", C.POINTER(C.c_float))]


class TextureView(C.Structure):
    _fields_ = [("n", C.c_int32), ("x", C.POINTER(C.c_int16)), ("y", C.POINTER(C.c_int16)), ("ori", C.POINTER(C.c_float)),
                ("des_len", C.c_int32), ("des", C.POINTER(C.c_float)), ("codes", C.POINTER(C.c_uint8))]


class TemplateView(C.Structure):
    _fields_ = [("n_minu", C.c_int32), ("minu", C.POINTER(MinutiaeView)), ("n_tex", C.c_int32), ("tex", C.POINTER(TextureView))]


class Timing(C.Structure):
    _fields_ = [("lut_ms", C.c_float), ("adc_ms", C.c_float), ("tex_tail_ms", C.c_float), ("minu_ms", C.c_float), ("fuse_ms", C.c_float), ("topk_ms", C.c_float),
                ("total_ms", C.c_float), ("adc_launches", C.c_int32), ("adc_lookups", C.c_int64), ("pairs", C.c_int64), ("adc_bound_ms", C.c_float), ("adc_refine_ms", C.c_float),
                ("cands_ms", C.c_float), ("minu_graph_ms", C.c_float), ("launch_groups", C.c_int32), ("overlapped_groups", C.c_int32),
                ("minu_tasks", C.c_int64), ("minu_fallback_tasks", C.c_int64), ("minu_tasks_small", C.c_int64), ("minu_tasks_medium", C.c_int64), ("minu_tasks_large", C.c_int64),
                ("bound_clock_ghz", C.c_float), ("cands_clock_ghz", C.c_float)]


# afis_score_stat (include/afis_matcher.h), 48 bytes: what Matcher.score_stats returns and host/sharding.py::merge_score_stats / trim_score_stats take
SCORE_STAT = np.dtype([("n", "<i8"), ("n_outside", "<i8"), ("s1", "<u8"), ("s2_lo", "<u8"), ("s2_hi", "<u8"), ("min", "<f4"), ("max", "<f4")])
assert SCORE_STAT.itemsize == 48
# afis_corr_moments (include/afis_matcher.h), 72 bytes: what Matcher.pair_alignments returns and alignment_fit / host/sharding.py::merge_pair_alignments take
CORR_MOMENTS = np.dtype([(f, "<i8") for f in ("n", "slx", "sly", "srx", "sry", "dot", "cross", "ll", "rr")])
assert CORR_MOMENTS.itemsize == 72
TEX_CORR_MAX = 200
FUSE_SUM, FUSE_MAX, FUSE_MIN, FUSE_REQUIRE_ALL, FUSE_OPERANDS_MAX = 0, 1, 2, 4, 16      # AFIS_FUSE_*: afis_matrix_fuse's modes, its flag and its operand count


class MatrixDesc(C.Structure):
    """afis_matrix_desc"""
    _fields_ = [("n_q", C.c_int32), ("normalized", C.c_int32), ("columns", C.c_int64), ("over_subset", C.c_int32), ("stale", C.c_int32)]

EXPORTS = ["afis_create", "afis_create_from_codebook", "afis_device_info", "afis_destroy", "afis_last_error", "afis_gallery_add", "afis_gallery_add_dat", "afis_gallery_add_dat_batch", "afis_gallery_reserve",
           "afis_gallery_add_packed", "afis_gallery_commit", "afis_gallery_size", "afis_gallery_reopen", "afis_gallery_remove", "afis_gallery_commit_at", "afis_gallery_export", "afis_gallery_save", "afis_gallery_load",
           "afis_gallery_file_info", "afis_gallery_file_names", "afis_rank_list", "afis_search", "afis_search_dat", "afis_queries_upload",
           "afis_subset_create", "afis_subset_free", "afis_search_subset", "afis_search_subset_resident",
           "afis_subjects_create", "afis_subjects_free", "afis_rank_subjects", "afis_rank_hits", "afis_rank_subject_hits", "afis_queries_upload_reserved", "afis_rank_latent_hits",
           "afis_rank_case_hits", "afis_rank_case_subject_hits",
           "afis_labels_create", "afis_labels_free", "afis_rank_hits_filtered", "afis_rank_subject_hits_filtered",
           "afis_rank_case_hits_filtered", "afis_rank_case_subject_hits_filtered", "afis_rank_latent_hits_filtered", "afis_search_eligible", "afis_search_weighted", "afis_search_prints",
           "afis_rank_positions", "afis_rank_subject_positions", "afis_count_before", "afis_score_stats", "afis_normalize_scores", "afis_score_stat_add", "afis_score_stat_remove", "afis_score_stat_moments", "afis_score_histogram", "afis_entries_at", "afis_subject_score_stats", "afis_subject_score_histogram", "afis_subject_entries_at", "afis_link_groups", "afis_link_subject_groups",
           "afis_matrix_keep", "afis_matrix_free", "afis_matrix_info", "afis_matrix_read", "afis_matrix_recall", "afis_matrix_fuse",
           "afis_correspondences_pairs", "afis_score_pairs", "afis_score_print_pairs", "afis_correspondences_print_pairs",
           "afis_texture_correspondences_pairs", "afis_texture_correspondences_print_pairs", "afis_pair_alignments", "afis_print_pair_alignments", "afis_corr_moments_add", "afis_alignment_fit", "afis_search_cascade", "afis_search_prints_cascade", "afis_search_cascade_subset", "afis_search_cascade_eligible",
           "afis_search_resident", "afis_queries_free", "afis_correspondences", "afis_match_all_templates", "afis_pq_encode", "afis_encode_rolled_dat", "afis_pq_train", "afis_pq_train_init_points", "afis_codebook_write", "afis_get_timing", "afis_get_timing2", "afis_set_option", "afis_get_option"]
# include/afis_matcher_taps.h: exported by libafis_hip_test.so only
TAP_EXPORTS = ["afis_debug_lut", "afis_debug_texture_rowmax", "afis_debug_stage_list", "afis_debug_phase_cycles", "afis_debug_atan2_grid", "afis_debug_graph_arith", "afis_debug_refine_stats", "afis_debug_compact_stats", "afis_debug_rank_subjects", "afis_debug_rank_hits", "afis_debug_rank_latent_hits",
               "afis_debug_transpose_stats", "afis_debug_rank_rows", "afis_debug_expand_rows", "afis_debug_fold_templates", "afis_debug_print_queries", "afis_debug_kept_cells_mapped"]


def alignment_fit(lib, moments):
    """afis_alignment_fit of one CORR_MOMENTS record through `lib` (no context, no device) -> (c, s, tx, ty, rms), or None where the call answers AFIS_EINVAL."""
    rec = np.ascontiguousarray(np.asarray(moments, CORR_MOMENTS).reshape(-1)[:1])
    out = [C.c_double(0.0) for _ in range(5)]
    if lib.afis_alignment_fit(C.c_void_p(rec.ctypes.data), *[C.byref(o) for o in out]) != 0:
        return None
    return tuple(o.value for o in out)


def add_moments(lib, records):
    """The sum of CORR_MOMENTS records (afis_corr_moments_add, exact) as one record [1]; ValueError where the sum leaves the bound."""
    acc = np.zeros(1, CORR_MOMENTS)
    for r in np.asarray(records, CORR_MOMENTS).reshape(-1):
        one = np.array([r], CORR_MOMENTS)
        if lib.afis_corr_moments_add(C.c_void_p(acc.ctypes.data), C.c_void_p(one.ctypes.data)) != 0:
            raise ValueError("add_moments: a record or the sum is outside the bound of include/afis_matcher.h")
    return acc


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.exists(path):
        raise AfisError(f"{path} not found: build it with `make -C msu-latentafis_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    vp, i32p, i64p, fp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    lib.afis_create.argtypes = [C.POINTER(vp), fp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.afis_create_from_codebook.argtypes = [C.POINTER(vp), C.c_char_p, C.c_size_t, C.c_int]
    lib.afis_destroy.argtypes = [vp]; lib.afis_destroy.restype = None
    lib.afis_last_error.argtypes = [vp]; lib.afis_last_error.restype = C.c_char_p
    lib.afis_rank_list.argtypes = [C.POINTER(C.c_float), C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    lib.afis_gallery_add.argtypes = [vp, C.POINTER(TemplateView), C.c_int]
    lib.afis_gallery_add_dat.argtypes = [vp, C.c_char_p, C.c_size_t, i32p]
    lib.afis_gallery_reserve.argtypes = [vp, C.c_int64]
    if hasattr(lib, "afis_gallery_add_dat_batch"):
        lib.afis_gallery_add_dat_batch.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int64, i32p]
    lib.afis_gallery_add_packed.argtypes = [vp, C.c_int64, i64p, C.POINTER(C.c_int16), C.POINTER(C.c_int16), fp, fp,
                                            i64p, C.POINTER(C.c_int16), C.POINTER(C.c_int16), fp, C.POINTER(C.c_uint8)]
    lib.afis_gallery_commit.argtypes = [vp, C.c_int64]
    lib.afis_gallery_save.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p)]
    lib.afis_gallery_load.argtypes = [vp, C.c_char_p, C.c_int64, C.c_int64]
    lib.afis_gallery_file_info.argtypes = [C.c_char_p, i64p, i64p, i64p, i32p]
    lib.afis_gallery_file_names.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.afis_gallery_size.argtypes = [vp]; lib.afis_gallery_size.restype = C.c_int64
    if hasattr(lib, "afis_gallery_reopen"):                             # the live gallery; absent from older builds compared by tools/lib_ab.py
        lib.afis_gallery_reopen.argtypes = [vp]
        lib.afis_gallery_remove.argtypes = [vp, i64p, C.c_int64]
        lib.afis_gallery_export.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p)]
    if hasattr(lib, "afis_gallery_commit_at"):                          # (absent from older builds, as above)
        lib.afis_gallery_commit_at.argtypes = [vp, i64p, C.c_int64]
    lib.afis_search.argtypes = [vp, C.POINTER(TemplateView), C.c_int, fp, fp, i32p, C.c_int, i64p, fp]
    lib.afis_search_dat.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, fp, fp, i32p, C.c_int, i64p, fp]
    lib.afis_queries_upload.argtypes = [vp, C.POINTER(TemplateView), C.c_int, C.POINTER(vp)]
    lib.afis_search_resident.argtypes = [vp, vp, fp, fp, i32p, C.c_int, i64p, fp]
    if hasattr(lib, "afis_subset_create"):                              # subset search; absent from older builds compared by tools/lib_ab.py
        lib.afis_subset_create.argtypes = [vp, i64p, C.c_int64, C.POINTER(vp)]
        lib.afis_subset_free.argtypes = [vp, vp]; lib.afis_subset_free.restype = None
        lib.afis_search_subset.argtypes = [vp, vp, C.POINTER(TemplateView), C.c_int, fp, fp, i32p, C.c_int, i64p, fp]
        lib.afis_search_subset_resident.argtypes = [vp, vp, vp, fp, fp, i32p, C.c_int, i64p, fp]
    if hasattr(lib, "afis_subjects_create"):                            # subject rank lists; absent from older builds compared by tools/lib_ab.py
        lib.afis_subjects_create.argtypes = [vp, i64p, C.c_int64, C.POINTER(vp)]
        lib.afis_subjects_free.argtypes = [vp, vp]; lib.afis_subjects_free.restype = None
        lib.afis_rank_subjects.argtypes = [vp, vp, C.c_int, C.c_int, i64p, fp, i64p]
    if hasattr(lib, "afis_rank_hits"):                                  # hit lists; absent from older builds compared by tools/lib_ab.py
        lib.afis_rank_hits.argtypes = [vp, C.c_int, C.c_float, C.c_int, i64p, i64p, fp]
        lib.afis_rank_subject_hits.argtypes = [vp, vp, C.c_int, C.c_float, C.c_int, i64p, i64p, fp, i64p]
    if hasattr(lib, "afis_rank_latent_hits"):                           # reverse search; absent from older builds compared by tools/lib_ab.py
        lib.afis_queries_upload_reserved.argtypes = [vp, C.POINTER(TemplateView), C.c_int, C.c_int64, C.POINTER(vp)]
        lib.afis_rank_latent_hits.argtypes = [vp, C.c_int64, C.c_float, C.c_int, C.c_int64, i64p, i64p, fp]
    if hasattr(lib, "afis_rank_case_hits"):                             # case lists; absent from older builds compared by tools/lib_ab.py
        lib.afis_rank_case_hits.argtypes = [vp, i64p, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_int, i64p, i64p, i64p, fp]
        lib.afis_rank_case_subject_hits.argtypes = [vp, vp, i64p, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_int, i64p, i64p, i64p, fp]
    if hasattr(lib, "afis_rank_hits_filtered"):                         # filtered hit lists; absent from older builds compared by tools/lib_ab.py
        u64p = C.POINTER(C.c_uint64)
        lib.afis_labels_create.argtypes = [vp, u64p, C.c_int64, C.POINTER(vp)]
        lib.afis_labels_free.argtypes = [vp, vp]; lib.afis_labels_free.restype = None
        lib.afis_rank_hits_filtered.argtypes = [vp, vp, u64p, i64p, i64p, C.c_int, C.c_float, C.c_int, i64p, i64p, fp]
        lib.afis_rank_subject_hits_filtered.argtypes = [vp, vp, vp, u64p, i64p, i64p, C.c_int, C.c_float, C.c_int, i64p, i64p, fp, i64p]
    if hasattr(lib, "afis_rank_case_hits_filtered"):                    # filtered case and column lists; absent from older builds compared by tools/lib_ab.py
        lib.afis_rank_case_hits_filtered.argtypes = [vp, vp, u64p, i64p, i64p, i64p, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_int, i64p, i64p, i64p, fp]
        lib.afis_rank_case_subject_hits_filtered.argtypes = [vp, vp, vp, u64p, i64p, i64p, i64p, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_int, i64p, i64p, i64p, fp]
        lib.afis_rank_latent_hits_filtered.argtypes = [vp, vp, u64p, i64p, i64p, C.c_int64, C.c_float, C.c_int, C.c_int64, i64p, i64p, fp]
    if hasattr(lib, "afis_search_eligible"):                            # eligible search; absent from older builds compared by tools/lib_ab.py
        lib.afis_search_eligible.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.POINTER(TemplateView), C.c_int, fp, i32p]
    if hasattr(lib, "afis_search_weighted"):                            # weighted search; absent from older builds compared by tools/lib_ab.py
        lib.afis_search_weighted.argtypes = [vp, C.POINTER(TemplateView), C.c_int, fp, C.c_int, fp, C.c_int, fp, i32p]
    if hasattr(lib, "afis_search_prints"):                              # print search; absent from older builds compared by tools/lib_ab.py
        lib.afis_search_prints.argtypes = [vp, vp, i64p, C.c_int, fp, fp, fp, i32p]
    if hasattr(lib, "afis_rank_positions"):                             # rank positions; absent from older builds compared by tools/lib_ab.py
        u64p = C.POINTER(C.c_uint64)
        lib.afis_rank_positions.argtypes = [vp, vp, u64p, i64p, i64p, C.c_int, C.c_int64, i32p, i64p, i32p, i64p, fp]
        lib.afis_rank_subject_positions.argtypes = [vp, vp, vp, u64p, i64p, i64p, C.c_int, C.c_int64, i32p, i64p, i32p, i64p, fp, i64p]
        lib.afis_count_before.argtypes = [vp, vp, u64p, i64p, i64p, C.c_int, C.c_int64, i32p, fp, i64p, i64p]
    if hasattr(lib, "afis_score_stats"):                                # cohort statistics and z-normalised scores; absent from older builds compared by tools/lib_ab.py
        u64p = C.POINTER(C.c_uint64); dp = C.POINTER(C.c_double)
        lib.afis_score_stats.argtypes = [vp, C.c_int, vp, u64p, i64p, i64p, C.c_int, vp]
        lib.afis_normalize_scores.argtypes = [vp, C.c_int, C.c_int, dp, dp, fp]
        lib.afis_score_stat_add.argtypes = [vp, vp]
        lib.afis_score_stat_remove.argtypes = [vp, C.c_float]
        lib.afis_score_stat_moments.argtypes = [vp, dp, dp]
    if hasattr(lib, "afis_score_histogram"):                            # score distributions; absent from older builds compared by tools/lib_ab.py
        u64p = C.POINTER(C.c_uint64)
        lib.afis_score_histogram.argtypes = [vp, C.c_int, vp, u64p, i64p, i64p, C.c_int, C.c_int, fp, i64p]
        lib.afis_entries_at.argtypes = [vp, vp, u64p, i64p, i64p, C.c_int, C.c_int64, i32p, i64p, i32p, i64p, fp]
    if hasattr(lib, "afis_subject_score_stats"):                        # person distributions; absent from older builds compared by tools/lib_ab.py
        u64p = C.POINTER(C.c_uint64)
        lib.afis_subject_score_stats.argtypes = [vp, vp, C.c_int, vp, u64p, i64p, i64p, C.c_int, vp]
        lib.afis_subject_score_histogram.argtypes = [vp, vp, C.c_int, vp, u64p, i64p, i64p, C.c_int, C.c_int, fp, i64p]
        lib.afis_subject_entries_at.argtypes = [vp, vp, vp, u64p, i64p, i64p, C.c_int, C.c_int64, i32p, i64p, i32p, i64p, fp, i64p]
    if hasattr(lib, "afis_link_groups"):                                # link groups; absent from older builds compared by tools/lib_ab.py
        u64p = C.POINTER(C.c_uint64)
        lib.afis_link_groups.argtypes = [vp, vp, u64p, i64p, i64p, C.c_int, i64p, C.c_float, C.c_int, C.c_int64, C.c_int64, i64p, i64p, i64p, i64p, i64p, i64p]
        lib.afis_link_subject_groups.argtypes = [vp, vp, vp, u64p, i64p, i64p, C.c_int, i64p, C.c_float, C.c_int, C.c_int64, C.c_int64, i64p, i64p, i64p, i64p, i64p, i64p]
    if hasattr(lib, "afis_matrix_keep"):                                # kept matrices; absent from older builds compared by tools/lib_ab.py
        lib.afis_matrix_keep.argtypes = [vp, C.POINTER(vp)]
        lib.afis_matrix_free.argtypes = [vp, vp]; lib.afis_matrix_free.restype = None
        lib.afis_matrix_info.argtypes = [vp, vp, C.POINTER(MatrixDesc)]
        lib.afis_matrix_read.argtypes = [vp, vp, C.c_int, C.c_int, fp]
        lib.afis_matrix_recall.argtypes = [vp, vp]
        lib.afis_matrix_fuse.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int, C.c_int, fp]
    lib.afis_correspondences.argtypes = [vp, vp, i64p, C.c_int, i32p, C.POINTER(C.c_int16)]
    if hasattr(lib, "afis_correspondences_pairs"):                      # the pair-list export; absent from older builds compared by tools/lib_ab.py
        lib.afis_correspondences_pairs.argtypes = [vp, vp, C.c_int64, i32p, i64p, i32p, C.POINTER(C.c_int16), fp]
    if hasattr(lib, "afis_score_pairs"):                                # pair scoring; absent from older builds compared by tools/lib_ab.py
        lib.afis_score_pairs.argtypes = [vp, vp, C.c_int64, i32p, i64p, i32p, fp, fp]
    if hasattr(lib, "afis_score_print_pairs"):                          # print pairs; absent from older builds compared by tools/lib_ab.py
        lib.afis_score_print_pairs.argtypes = [vp, C.c_int64, i64p, i64p, fp, fp, i32p, fp, fp]
        lib.afis_correspondences_print_pairs.argtypes = [vp, C.c_int64, i64p, i64p, i32p, C.POINTER(C.c_int16), fp]
    if hasattr(lib, "afis_pair_alignments"):                            # texture correspondences and pair alignments; absent from older builds compared by tools/lib_ab.py
        i16p = C.POINTER(C.c_int16); dp = C.POINTER(C.c_double)
        lib.afis_texture_correspondences_pairs.argtypes = [vp, vp, C.c_int64, i32p, i64p, i32p, i16p, i16p, fp, fp]
        lib.afis_texture_correspondences_print_pairs.argtypes = [vp, C.c_int64, i64p, i64p, i32p, i16p, i16p, fp, fp]
        lib.afis_pair_alignments.argtypes = [vp, vp, C.c_int64, i32p, i64p, i32p, vp]
        lib.afis_print_pair_alignments.argtypes = [vp, C.c_int64, i64p, i64p, i32p, vp]
        lib.afis_corr_moments_add.argtypes = [vp, vp]
        lib.afis_alignment_fit.argtypes = [vp, dp, dp, dp, dp, dp]
    if hasattr(lib, "afis_search_cascade"):                             # cascade search; absent from older builds compared by tools/lib_ab.py
        lib.afis_search_cascade.argtypes = [vp, vp, C.c_int, fp, i32p, i64p, i64p, fp]
    if hasattr(lib, "afis_search_cascade_subset"):                      # cascade over a subset / the eligible prints; absent from older builds compared by tools/lib_ab.py
        lib.afis_search_cascade_subset.argtypes = [vp, vp, vp, C.c_int, fp, i32p, i64p, i64p, fp]
        lib.afis_search_cascade_eligible.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.POINTER(TemplateView), C.c_int, C.c_int, fp, i32p, i64p, i64p, fp]
    if hasattr(lib, "afis_search_prints_cascade"):                      # print cascade; absent from older builds compared by tools/lib_ab.py
        lib.afis_search_prints_cascade.argtypes = [vp, i64p, C.c_int, fp, fp, C.c_int, fp, i32p, i64p, i64p, fp]
    lib.afis_queries_free.argtypes = [vp, vp]; lib.afis_queries_free.restype = None
    lib.afis_match_all_templates.argtypes = [vp, vp, fp, i32p, i32p]
    lib.afis_pq_encode.argtypes = [vp, fp, C.c_int64, C.POINTER(C.c_uint8)]
    lib.afis_encode_rolled_dat.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), i32p]
    if hasattr(lib, "afis_pq_train"):
        lib.afis_pq_train.argtypes = [C.c_int, fp, C.c_int64, fp, C.c_int, fp, i64p, i64p, i32p]
        lib.afis_pq_train_init_points.argtypes = [fp, C.c_int64, C.c_uint64, fp]
        lib.afis_codebook_write.argtypes = [fp, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.afis_get_timing.argtypes = [vp, C.POINTER(Timing)]
    if hasattr(lib, "afis_get_timing2"):                                # absent from older builds compared by tools/lib_ab.py
        lib.afis_get_timing2.argtypes = [vp, C.POINTER(Timing), C.c_size_t]
    lib.afis_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    if hasattr(lib, "afis_device_info"):                                # round 5
        lib.afis_device_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, i32p]
    if hasattr(lib, "afis_get_option"):
        lib.afis_get_option.argtypes = [vp, C.c_char_p, i64p]
    if hasattr(lib, "afis_debug_stage_list"):                           # the parity taps: libafis_hip_test.so (and older builds) only
        lib.afis_debug_stage_list.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, fp, i32p, i32p, i32p]
        lib.afis_debug_lut.argtypes = [vp, C.POINTER(TemplateView), fp, i32p]
        lib.afis_debug_texture_rowmax.argtypes = [vp, C.POINTER(TemplateView), C.c_int64, fp, i32p, i32p]
        lib.afis_debug_phase_cycles.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        lib.afis_debug_atan2_grid.argtypes = [vp, C.c_int, fp]
    if hasattr(lib, "afis_debug_graph_arith"):
        lib.afis_debug_graph_arith.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    if hasattr(lib, "afis_debug_compact_stats"):
        lib.afis_debug_compact_stats.argtypes = [vp, C.POINTER(C.c_longlong)]
    if hasattr(lib, "afis_debug_refine_stats"):
        lib.afis_debug_refine_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.c_int]
    if hasattr(lib, "afis_debug_rank_subjects"):
        lib.afis_debug_rank_subjects.argtypes = [vp, vp, fp, C.c_int, C.c_int, i64p, fp, i64p]
    if hasattr(lib, "afis_debug_rank_hits"):
        lib.afis_debug_rank_hits.argtypes = [vp, vp, fp, C.c_int, C.c_float, C.c_int, i64p, i64p, fp, i64p]
    if hasattr(lib, "afis_debug_rank_latent_hits"):
        lib.afis_debug_rank_latent_hits.argtypes = [vp, fp, C.c_int, C.c_float, C.c_int, C.c_int64, i64p, i64p, fp]
        lib.afis_debug_transpose_stats.argtypes = [vp, C.POINTER(C.c_longlong)]
    if hasattr(lib, "afis_debug_rank_rows"):
        lib.afis_debug_rank_rows.argtypes = [vp, vp, fp, C.c_int, C.c_int, i64p, fp]
    if hasattr(lib, "afis_debug_expand_rows"):
        lib.afis_debug_expand_rows.argtypes = [vp, fp, C.c_int, C.c_int64, i32p, i32p, C.c_int, C.c_int64, fp]
    if hasattr(lib, "afis_debug_fold_templates"):
        lib.afis_debug_fold_templates.argtypes = [vp, fp, C.c_int64, C.c_int64, i32p, C.c_int, fp, C.POINTER(C.c_uint8), fp]
    if hasattr(lib, "afis_debug_kept_cells_mapped"):
        u8p = C.POINTER(C.c_uint8)
        lib.afis_debug_kept_cells_mapped.argtypes = [vp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, i64p, u8p, i32p, C.c_int, C.c_int, i32p, fp, fp, i32p, i32p,
                                                  C.c_int64, C.c_int64, i32p, C.c_int64, i32p, fp, fp]
    if hasattr(lib, "afis_debug_print_queries"):
        u8p, i16p = C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
        lib.afis_debug_print_queries.argtypes = [vp, i64p, C.c_int, u8p, u8p, i32p] + [i32p] * 7 + [i16p, fp, fp, fp, i16p, fp, fp]
    return lib


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(C.POINTER(t))


def _train_chk(lib, rc, who):
    if rc != 0:
        raise AfisError(f"{who} failed ({rc}): {lib.afis_last_error(None).decode()}")


def pq_train(des, init, iters: int = 20, device: int = 0, lib_path: Optional[str] = None) -> dict:
    """afis_pq_train: `iters` Lloyd steps of the codebook [16][256][6] over the points des [n][96] on the device, from `init`, in the order-independent definition
    of include/afis_matcher.h.  Returns codewords [16][256][6], counts [16][256] (the last executed assignment's), changed [iters] and iters_run."""
    lib = load_library(lib_path or LIB_PATH)
    des = np.ascontiguousarray(des, np.float32).reshape(-1, 96)
    init = np.ascontiguousarray(init, np.float32).reshape(16, 256, 6)
    cw = np.zeros((16, 256, 6), np.float32); counts = np.zeros((16, 256), np.int64); changed = np.zeros(max(int(iters), 1), np.int64); run = C.c_int32(0)
    rc = lib.afis_pq_train(device, _ptr(des, C.c_float) if len(des) else None, des.shape[0], _ptr(init, C.c_float), int(iters), _ptr(cw, C.c_float),
                           _ptr(counts, C.c_int64), _ptr(changed, C.c_int64), C.byref(run))
    _train_chk(lib, rc, "afis_pq_train")
    return {"codewords": cw, "counts": counts, "changed": changed[:max(int(iters), 0)], "iters_run": int(run.value)}


def pq_train_init_points(des, seed: int, lib_path: Optional[str] = None) -> np.ndarray:
    """afis_pq_train_init_points (host only): kmeans2's minit='points' from a seed — per sub-quantizer the sub-vectors of 256 distinct points."""
    lib = load_library(lib_path or LIB_PATH)
    des = np.ascontiguousarray(des, np.float32).reshape(-1, 96)
    init = np.zeros((16, 256, 6), np.float32)
    _train_chk(lib, lib.afis_pq_train_init_points(_ptr(des, C.c_float), des.shape[0], C.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(init, C.c_float)), "afis_pq_train_init_points")
    return init


def codebook_bytes(codewords, lib_path: Optional[str] = None) -> bytes:
    """afis_codebook_write: the codebook file afis_create_from_codebook (and Matcher) reads, for codewords [16][256][6]."""
    lib = load_library(lib_path or LIB_PATH)
    cw = np.ascontiguousarray(codewords, np.float32)
    if cw.shape != (16, 256, 6):
        raise AfisError(f"codebook_bytes: codewords must be [16][256][6], not {list(cw.shape)}")
    need = C.c_size_t(0)
    _train_chk(lib, lib.afis_codebook_write(_ptr(cw, C.c_float), 16, 256, 6, None, 0, C.byref(need)), "afis_codebook_write")
    out = C.create_string_buffer(need.value)
    _train_chk(lib, lib.afis_codebook_write(_ptr(cw, C.c_float), 16, 256, 6, out, need.value, C.byref(need)), "afis_codebook_write")
    return out.raw[:need.value]


class _Views:
    """Builds afis_template_view arrays from FPTemplate objects and keeps every backing array alive."""

    def __init__(self, templates: Sequence[FPTemplate]):
        self.keep = []
        self.arr = (TemplateView * max(1, len(templates)))()
        for i, t in enumerate(templates):
            mv = (MinutiaeView * max(1, len(t.minu)))()
            for j, m in enumerate(t.minu):
                x = np.ascontiguousarray(m.x, np.int16); y = np.ascontiguousarray(m.y, np.int16)
                o = np.ascontiguousarray(m.ori, np.float32); d = np.ascontiguousarray(m.des, np.float32)
                self.keep += [x, y, o, d]
                mv[j] = MinutiaeView(len(x), _ptr(x, C.c_int16), _ptr(y, C.c_int16), _ptr(o, C.c_float), d.shape[1] if d.ndim == 2 else 0, _ptr(d, C.c_float))
            tv = (TextureView * max(1, len(t.tex)))()
            for j, s in enumerate(t.tex):
                x = np.ascontiguousarray(s.x, np.int16); y = np.ascontiguousarray(s.y, np.int16); o = np.ascontiguousarray(s.ori, np.float32)
                self.keep += [x, y, o]
                des_p, codes_p, dl = None, None, 0
                if s.des is not None:
                    d = np.ascontiguousarray(s.des, np.float32); self.keep.append(d); des_p = _ptr(d, C.c_float); dl = d.shape[1]
                if s.codes is not None:
                    c = np.ascontiguousarray(s.codes, np.uint8); self.keep.append(c); codes_p = _ptr(c, C.c_uint8); dl = c.shape[1]
                tv[j] = TextureView(len(x), _ptr(x, C.c_int16), _ptr(y, C.c_int16), _ptr(o, C.c_float), dl, des_p, codes_p)
            self.keep += [mv, tv]
            self.arr[i] = TemplateView(len(t.minu), mv, len(t.tex), tv)
        self.n = len(templates)


class Matcher:
    """`PQ::Matcher` (matching/matcher.h:35) on one MI355X.  One instance = one device = one gallery shard."""

    def __init__(self, code_file, device: int = 0, lib_path: Optional[str] = None, taps: bool = False):
        """taps=True loads libafis_hip_test.so (the product objects + the afis_debug_* parity taps); the default is the product library."""
        self.lib = load_library(lib_path or (TEST_LIB_PATH if taps else LIB_PATH))
        self.has_taps = hasattr(self.lib, "afis_debug_stage_list")
        if isinstance(code_file, Codebook):
            buf = code_file.to_bytes()
        elif isinstance(code_file, (bytes, bytearray)):
            buf = bytes(code_file)
        else:
            with open(code_file, "rb") as f:
                buf = f.read()
        self.ctx = C.c_void_p()
        rc = self.lib.afis_create_from_codebook(C.byref(self.ctx), buf, len(buf), device)
        if rc != 0:
            self.ctx = None
            raise AfisError(f"afis_create failed ({rc}): {self.lib.afis_last_error(None).decode()}")
        self.gallery_files: List[str] = []
        self.last_n_q = 0                                                  # queries of the last search call made through this object (rank_hits / rank_subject_hits default to it)
        self.last_n_templates = 0                                          # ... and the templates (columns) it covered (rank_latent_hits' rows)
        self.index_base = 0

    def device_info(self, device: int) -> dict:
        """What the HIP runtime says about a device (afis_device_info): name, PCI bus id, UUID, compute units."""
        name = C.create_string_buffer(256); pci = C.create_string_buffer(64); uuid = C.create_string_buffer(40); ncu = C.c_int32(0)
        rc = self.lib.afis_device_info(device, name, 256, pci, 64, uuid, 40, C.byref(ncu))
        if rc != 0:
            raise AfisError(f"afis_device_info({device}) failed ({rc})")
        return {"name": name.value.decode(errors="replace"), "pci_bus_id": pci.value.decode(errors="replace"), "uuid": uuid.value.decode(errors="replace"), "compute_units": int(ncu.value)}

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.afis_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != 0:
            raise AfisError(f"afis error {rc}: {self.lib.afis_last_error(self.ctx).decode()}")

    # ---- gallery ----------------------------------------------------------------------------------------------
    def gallery_add(self, templates: Sequence[FPTemplate]):
        v = _Views(templates)
        self._chk(self.lib.afis_gallery_add(self.ctx, v.arr, v.n))

    def gallery_add_dat(self, buf: bytes) -> int:
        rc = C.c_int32(0)
        self._chk(self.lib.afis_gallery_add_dat(self.ctx, buf, len(buf), C.byref(rc)))
        return rc.value

    def gallery_add_dat_batch(self, bufs: Sequence[bytes]) -> np.ndarray:
        """n rolled .dat files at once (parsed on the host's threads); returns the reader's code per file."""
        n = len(bufs)
        arr = (C.c_char_p * max(1, n))(*bufs)
        lens = (C.c_size_t * max(1, n))(*[len(b) for b in bufs])
        rc = np.zeros(max(1, n), np.int32)
        self._chk(self.lib.afis_gallery_add_dat_batch(self.ctx, arr, lens, n, _ptr(rc, C.c_int32)))
        return rc[:n]

    def gallery_add_packed(self, g):
        mo = np.ascontiguousarray(g.minu_off, np.int64); to = np.ascontiguousarray(g.tex_off, np.int64)
        a = [np.ascontiguousarray(g.minu_x, np.int16), np.ascontiguousarray(g.minu_y, np.int16), np.ascontiguousarray(g.minu_ori, np.float32),
             np.ascontiguousarray(g.minu_des, np.float32), np.ascontiguousarray(g.tex_x, np.int16), np.ascontiguousarray(g.tex_y, np.int16),
             np.ascontiguousarray(g.tex_ori, np.float32), np.ascontiguousarray(g.tex_codes, np.uint8)]
        self._chk(self.lib.afis_gallery_add_packed(self.ctx, len(mo) - 1, _ptr(mo, C.c_int64), _ptr(a[0], C.c_int16), _ptr(a[1], C.c_int16),
                                                   _ptr(a[2], C.c_float), _ptr(a[3], C.c_float), _ptr(to, C.c_int64), _ptr(a[4], C.c_int16),
                                                   _ptr(a[5], C.c_int16), _ptr(a[6], C.c_float), _ptr(a[7], C.c_uint8)))

    def gallery_save(self, path: str, names: Sequence[str] = None):
        """Write the staged gallery as one packed container (before gallery_commit)."""
        arr = None
        if names is not None:
            arr = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        self._chk(self.lib.afis_gallery_save(self.ctx, path.encode(), arr))

    def gallery_load(self, path: str, first: int = 0, count: int = -1):
        """Append templates [first, first+count) of a packed container to the staged gallery."""
        self._chk(self.lib.afis_gallery_load(self.ctx, path.encode(), first, count))

    def gallery_file_info(self, path: str):
        """-> (G, minutiae, texture points, per-template texture point counts) of a packed container."""
        G = C.c_int64(0); nm = C.c_int64(0); nt = C.c_int64(0)
        if self.lib.afis_gallery_file_info(path.encode(), C.byref(G), C.byref(nm), C.byref(nt), None) != 0:
            raise AfisError(self.lib.afis_last_error(None).decode())
        tc = np.zeros(max(1, G.value), np.int32)
        if self.lib.afis_gallery_file_info(path.encode(), None, None, None, _ptr(tc, C.c_int32)) != 0:
            raise AfisError(self.lib.afis_last_error(None).decode())
        return G.value, nm.value, nt.value, tc[:G.value]

    def gallery_file_names(self, path: str, first: int = 0, count: int = -1) -> List[str]:
        need = C.c_size_t(0)
        if self.lib.afis_gallery_file_names(path.encode(), first, count, None, 0, C.byref(need)) != 0:
            raise AfisError(self.lib.afis_last_error(None).decode())
        buf = C.create_string_buffer(max(1, need.value))
        if self.lib.afis_gallery_file_names(path.encode(), first, count, buf, need.value, C.byref(need)) != 0:
            raise AfisError(self.lib.afis_last_error(None).decode())
        return [b.decode() for b in buf.raw[:need.value].split(b"\0")[:-1]] if need.value else []

    def gallery_reserve(self, n_templates: int):
        """Hint: the staged gallery will grow to about n_templates templates (host arrays reserve room once)."""
        self._chk(self.lib.afis_gallery_reserve(self.ctx, n_templates))

    def gallery_commit(self, index_base: int = 0):
        self._chk(self.lib.afis_gallery_commit(self.ctx, index_base))
        self.index_base = index_base                                       # the shard's: an appending commit must name it again (reverse_search does)

    def gallery_reopen(self):
        """Open a staging area beside the committed shard: the gallery_add* / gallery_load calls work again, and the next gallery_commit appends what they staged
        (indices index_base + G_old ...) without uploading the resident templates again."""
        self._chk(self.lib.afis_gallery_reopen(self.ctx))

    def gallery_remove(self, idx: Sequence[int]):
        """Turn the listed entries (global indices, as search reports them) into empty entries (score -1); every other template keeps its index."""
        a = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        self._chk(self.lib.afis_gallery_remove(self.ctx, _ptr(a, C.c_int64) if len(a) else None, len(a)))

    def gallery_commit_at(self, idx: Sequence[int]):
        """Replace in place: on a reopened gallery, staged template i takes the place of the resident entry idx[i] (global indices, in staging order, any order).  Nothing
        is appended; every other template keeps its index.  A staged empty template makes the entry an empty entry; a live one onto an empty entry re-enrols there."""
        a = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        self._chk(self.lib.afis_gallery_commit_at(self.ctx, _ptr(a, C.c_int64) if len(a) else None, len(a)))

    def gallery_export(self, path: str, names: Sequence[str] = None):
        """Write the RESIDENT shard as a packed container: the file gallery_save writes from a context staged with the same entries."""
        arr = None
        if names is not None:
            if len(names) != self.resident_size:                          # the library reads one name per resident template
                raise AfisError(f"gallery_export: {len(names)} names for {self.resident_size} resident templates")
            arr = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        self._chk(self.lib.afis_gallery_export(self.ctx, path.encode(), arr))

    @property
    def gallery_size(self) -> int:
        return int(self.lib.afis_gallery_size(self.ctx))

    @property
    def resident_size(self) -> int:
        """Templates of the committed shard — what a search scores; gallery_size also counts what is staged beside it after gallery_reopen."""
        v = C.c_int64(0)
        if self.lib.afis_get_option(self.ctx, b"gallery_resident", C.byref(v)) == 0:
            return int(v.value)
        return self.gallery_size                                          # (a build without the live gallery: nothing can be staged beside a committed shard)

    def set_option(self, name: str, value: int):
        self._chk(self.lib.afis_set_option(self.ctx, name.encode(), value))

    def get_option(self, name: str) -> int:
        v = C.c_int64(0)
        if not hasattr(self.lib, "afis_get_option"):
            return 0
        self._chk(self.lib.afis_get_option(self.ctx, name.encode(), C.byref(v)))
        return int(v.value)

    # ---- search -----------------------------------------------------------------------------------------------
    def _alloc(self, nq, k, want_scores, want_parts, G=None):
        G = self.resident_size if G is None else G
        scores = np.empty((nq, G), np.float32) if want_scores else None
        parts = np.empty((nq, G, 4), np.float32) if want_parts else None
        status = np.zeros(nq, np.int32)
        ti = np.empty((nq, k), np.int64) if k > 0 else None
        ts = np.empty((nq, k), np.float32) if k > 0 else None
        args = (_ptr(scores, C.c_float) if want_scores else None, _ptr(parts, C.c_float) if want_parts else None, _ptr(status, C.c_int32), k,
                _ptr(ti, C.c_int64) if k > 0 else None, _ptr(ts, C.c_float) if k > 0 else None)
        return scores, parts, status, ti, ts, args

    def search(self, latents: Sequence[FPTemplate], k: int = 24, want_scores: bool = True, want_parts: bool = False):
        v = _Views(latents)
        scores, parts, status, ti, ts, args = self._alloc(v.n, k, want_scores, want_parts)
        self._chk(self.lib.afis_search(self.ctx, v.arr, v.n, *args))
        self.last_n_q = v.n; self.last_n_templates = self.resident_size
        return {"scores": scores, "parts": parts, "status": status, "topk_idx": ti, "topk_score": ts}

    def search_dat(self, bufs: Sequence[bytes], k: int = 24, want_scores: bool = True, want_parts: bool = False):
        n = len(bufs)
        arr = (C.c_char_p * max(1, n))(*bufs)
        lens = (C.c_size_t * max(1, n))(*[len(b) for b in bufs])
        scores, parts, status, ti, ts, args = self._alloc(n, k, want_scores, want_parts)
        self._chk(self.lib.afis_search_dat(self.ctx, arr, lens, n, *args))
        self.last_n_q = n; self.last_n_templates = self.resident_size
        return {"scores": scores, "parts": parts, "status": status, "topk_idx": ti, "topk_score": ts}

    def rank_list(self, scores, k: int = 24, ref_order: bool = False):
        """afis_rank_list (matcher.cpp:306-309): the k best of a score column, score descending; ref_order: equal scores in the order the reference binary's std::sort leaves them
        (else by ascending index, as the search's own top-k)."""
        s = np.ascontiguousarray(scores, np.float32).reshape(-1)
        idx = np.full(max(k, 1), -1, np.int64); sc = np.zeros(max(k, 1), np.float32)
        self._chk(self.lib.afis_rank_list(_ptr(s, C.c_float) if len(s) else None, C.c_int64(len(s)), C.c_int(int(ref_order)), C.c_int(k), _ptr(idx, C.c_int64), _ptr(sc, C.c_float)))
        return idx[:k], sc[:k]

    def upload_queries(self, latents: Sequence[FPTemplate], reserve: Optional[int] = None):
        """Latents resident on the device -> handle for search_resident / search_subset_resident.  reserve=N (afis_queries_upload_reserved): the launch groups are cut for
        a shard of N templates, and the handle stays valid through gallery edits for every shard or subset of at most N templates (reverse_search)."""
        v = _Views(latents)
        h = C.c_void_p()
        if reserve is None:
            self._chk(self.lib.afis_queries_upload(self.ctx, v.arr, v.n, C.byref(h)))
        else:
            self._chk(self.lib.afis_queries_upload_reserved(self.ctx, v.arr, v.n, int(reserve), C.byref(h)))
        return (h, v.n)

    def search_resident(self, handle, k: int = 24, want_scores: bool = False, want_parts: bool = False):
        h, n = handle
        scores, parts, status, ti, ts, args = self._alloc(n, k, want_scores, want_parts)
        self._chk(self.lib.afis_search_resident(self.ctx, h, *args))
        self.last_n_q = n; self.last_n_templates = self.resident_size
        return {"scores": scores, "parts": parts, "status": status, "topk_idx": ti, "topk_score": ts}

    # ---- subset search: a candidate list of the resident shard ---------------------------------------------------
    def subset_create(self, idx: Sequence[int]):
        """Gather the listed templates (global indices as search reports them, any order, no repeats) into a device-resident sub-shard; -> handle for search_subset*.
        Nothing of the gallery is uploaded.  The handle is refused (AFIS_ESTATE) once the gallery has been edited; subset_free releases it."""
        a = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        h = C.c_void_p()
        self._chk(self.lib.afis_subset_create(self.ctx, _ptr(a, C.c_int64) if len(a) else None, len(a), C.byref(h)))
        return (h, len(a))

    def subset_free(self, handle):
        self.lib.afis_subset_free(self.ctx, handle[0])

    def search_subset(self, handle, latents: Sequence[FPTemplate], k: int = 24, want_scores: bool = True, want_parts: bool = False):
        """search() over the subset's templates only: column j of scores / parts belongs to the j-th listed index, topk_idx holds global indices."""
        h, n = handle
        v = _Views(latents)
        scores, parts, status, ti, ts, args = self._alloc(v.n, k, want_scores, want_parts, G=n)
        self._chk(self.lib.afis_search_subset(self.ctx, h, v.arr, v.n, *args))
        self.last_n_q = v.n; self.last_n_templates = n
        return {"scores": scores, "parts": parts, "status": status, "topk_idx": ti, "topk_score": ts}

    def search_subset_resident(self, handle, qhandle, k: int = 24, want_scores: bool = False, want_parts: bool = False):
        h, n = handle
        qh, nq = qhandle
        scores, parts, status, ti, ts, args = self._alloc(nq, k, want_scores, want_parts, G=n)
        self._chk(self.lib.afis_search_subset_resident(self.ctx, h, qh, *args))
        self.last_n_q = nq; self.last_n_templates = n
        return {"scores": scores, "parts": parts, "status": status, "topk_idx": ti, "topk_score": ts}

    # ---- subject rank lists: the last search's scores grouped by enrolled person ---------------------------------
    def subjects_create(self, ids: Sequence[int]):
        """One subject id (any int64 >= 0) per template of the resident shard, in shard order; -> handle for rank_subjects.  The handle is refused (AFIS_ESTATE) once
        the gallery has been edited; subjects_free releases it.  handle[2]: the distinct ids ascending — the handle's slots, the order of every per-person output;
        handle[3]: the ids as given, one per template."""
        a = np.ascontiguousarray(np.asarray(ids, np.int64).reshape(-1))
        h = C.c_void_p()
        self._chk(self.lib.afis_subjects_create(self.ctx, _ptr(a, C.c_int64) if len(a) else None, len(a), C.byref(h)))
        return (h, len(a), np.unique(a), a)

    def subjects_free(self, handle):
        self.lib.afis_subjects_free(self.ctx, handle[0])

    def _subject_lists(self, fn, n_q: int, k: int):
        sid = np.empty((n_q, max(k, 0)), np.int64); sc = np.empty((n_q, max(k, 0)), np.float32); bi = np.empty((n_q, max(k, 0)), np.int64)
        self._chk(fn(n_q, k, _ptr(sid, C.c_int64), _ptr(sc, C.c_float), _ptr(bi, C.c_int64)))
        return {"subject": sid, "score": sc, "best_idx": bi}

    def rank_subjects(self, handle, n_q: int, k: int = 24):
        """The k best subjects of every query of the LAST search (any of the search calls; n_q is that search's): subject [n_q][k] ids, score descending / id ascending,
        score [n_q][k] the best fused score among the subject's templates the search covered, best_idx [n_q][k] the global index of that template; (-1, -inf, -1) pads."""
        return self._subject_lists(lambda nq, kk, a, b, c: self.lib.afis_rank_subjects(self.ctx, handle[0], nq, kk, a, b, c), n_q, k)

    def debug_rank_subjects(self, handle, scores: np.ndarray, k: int = 24):
        """rank_subjects over a caller-made [n_q][G] score matrix for the resident shard (parity tap)."""
        s = np.ascontiguousarray(scores, np.float32)
        return self._subject_lists(lambda nq, kk, a, b, c: self._tap("afis_debug_rank_subjects")(self.ctx, handle[0], _ptr(s, C.c_float), nq, kk, a, b, c), s.shape[0], k)

    # ---- hit lists: everything of the last search that reaches a decision score -----------------------------------
    def _hit_lists(self, fn, n_q: int, cap: int, subjects: bool):
        c = max(cap, 0)
        nh = np.empty(n_q, np.int64); a = np.empty((n_q, c), np.int64); sc = np.empty((n_q, c), np.float32); b = np.empty((n_q, c), np.int64) if subjects else None
        self._chk(fn(n_q, _ptr(nh, C.c_int64), _ptr(a, C.c_int64), _ptr(sc, C.c_float), _ptr(b, C.c_int64) if subjects else None))
        return {"n_hits": nh, "subject": a, "score": sc, "best_idx": b} if subjects else {"n_hits": nh, "idx": a, "score": sc}

    def rank_hits(self, min_score: float, cap: int, n_q: Optional[int] = None):
        """Of the LAST search (n_q: its queries; default: those of the last search call made through this object), per query every template whose score reaches min_score:
        n_hits [n_q] how many (it may exceed cap), idx / score [n_q][cap] the best min(n_hits, cap) of them in the search's rank-list order, padded with (-1, -inf).
        min_score = -inf gives the search's own top-cap, for cap up to 4096 (AFIS_HITS_MAX).  The default n_q is kept by this object's search* methods and by
        debug_rank_hits only: after debug_rank_subjects, or a search made on the context by other means, pass n_q."""
        n_q = self.last_n_q if n_q is None else n_q
        return self._hit_lists(lambda nq, nh, a, sc, b: self.lib.afis_rank_hits(self.ctx, nq, min_score, cap, nh, a, sc), n_q, cap, False)

    def rank_subject_hits(self, handle, min_score: float, cap: int, n_q: Optional[int] = None):
        """rank_hits over the enrolled persons of a subjects_create handle: n_hits, and subject / score / best_idx [n_q][cap] as rank_subjects gives them."""
        n_q = self.last_n_q if n_q is None else n_q
        return self._hit_lists(lambda nq, nh, a, sc, b: self.lib.afis_rank_subject_hits(self.ctx, handle[0], nq, min_score, cap, nh, a, sc, b), n_q, cap, True)

    def debug_rank_hits(self, handle, scores: np.ndarray, min_score: float, cap: int):
        """rank_hits (handle None) or rank_subject_hits over a caller-made [n_q][G] score matrix for the resident shard (parity tap); the matrix stays rankable."""
        s = np.ascontiguousarray(scores, np.float32)
        self.last_n_q = s.shape[0]; self.last_n_templates = s.shape[1]
        return self._hit_lists(lambda nq, nh, a, sc, b: self._tap("afis_debug_rank_hits")(self.ctx, handle[0] if handle is not None else None, _ptr(s, C.c_float), nq, min_score, cap, nh, a, sc, b),
                               s.shape[0], cap, handle is not None)

    def debug_rank_rows(self, scores: np.ndarray, k: int, subset=None):
        """The rank list of search() / search_subset() over a caller-made [n_q][n] score matrix (parity tap): topk_idx / topk_score [n_q][k] by the code the search runs
        (k <= 64 the device's rank-list kernel, k > 64 the host's).  subset: a subset_create handle; the columns then stand in ascending order of the listed global
        indices, as the device holds them.  The matrix stays rankable (rank_hits, rank_subjects, rank_latent_hits)."""
        s = np.ascontiguousarray(scores, np.float32)
        ti = np.empty((s.shape[0], k), np.int64); ts = np.empty((s.shape[0], k), np.float32)
        self._chk(self._tap("afis_debug_rank_rows")(self.ctx, subset[0] if subset is not None else None, _ptr(s, C.c_float), s.shape[0], k, _ptr(ti, C.c_int64), _ptr(ts, C.c_float)))
        self.last_n_q = s.shape[0]; self.last_n_templates = s.shape[1]
        return {"topk_idx": ti, "topk_score": ts}

    # ---- filtered hit lists: only the templates a query is eligible for ---------------------------------------------
    def labels_create(self, labels: Sequence[int]):
        """One 64-bit attribute word (the bits are the caller's) per template of the resident shard, in shard order; -> handle for rank_hits_filtered /
        rank_subject_hits_filtered.  The handle is refused (AFIS_ESTATE) once the gallery has been edited; labels_free releases it."""
        a = np.ascontiguousarray(np.asarray(labels, np.uint64).reshape(-1))
        h = C.c_void_p()
        self._chk(self.lib.afis_labels_create(self.ctx, _ptr(a, C.c_uint64) if len(a) else None, len(a), C.byref(h)))
        return (h, len(a))

    def labels_free(self, handle):
        self.lib.afis_labels_free(self.ctx, handle[0])

    @staticmethod
    def _filter_args(n_q: int, masks, excl):
        """masks: None or [n_q][3] uint64 (any_of, all_of, none_of); excl: None or one sequence of int64 per query -> the C arrays (kept alive by the caller)."""
        mk = None if masks is None else np.ascontiguousarray(np.asarray(masks, np.uint64).reshape(n_q, 3))
        off = ent = None
        if excl is not None:
            if len(excl) != n_q:
                raise ValueError("one exclusion sequence per query")
            rows = [np.asarray(e, np.int64).reshape(-1) for e in excl]
            off = np.zeros(n_q + 1, np.int64); off[1:] = np.cumsum([len(r) for r in rows])
            ent = np.ascontiguousarray(np.concatenate(rows)) if rows and off[-1] else np.zeros(1, np.int64)
        return mk, off, ent

    def _filter(self, labels, masks, excl, n_q: Optional[int] = None):
        """The filter of a call on the LAST search's matrix -> (n_q — None: that search's —, _filter_args' arrays, which live as long as the caller holds them, and
        the four filter arguments of the C calls: a labels_create handle's pointer, masks, excl_off, excl)."""
        n_q = self.last_n_q if n_q is None else n_q
        keep = mk, off, ent = self._filter_args(n_q, masks, excl)
        return n_q, keep, (labels[0] if labels is not None else None, _ptr(mk, C.c_uint64) if mk is not None else None, _ptr(off, C.c_int64) if off is not None else None,
                           _ptr(ent, C.c_int64) if ent is not None else None)

    def rank_hits_filtered(self, min_score: float, cap: int, labels=None, masks=None, excl=None, n_q: Optional[int] = None):
        """rank_hits over the cells each query is eligible for.  labels: a labels_create handle (needed with masks); masks: [n_q][3] uint64, per query (any_of, all_of,
        none_of) tested against the label L of a column's template: (any_of == 0 or L & any_of) and L & all_of == all_of and not L & none_of; excl: per query a
        sequence of GLOBAL template indices that are no entries for it (what the search did not cover is ignored).  None: no label test / no exclusions."""
        n_q, keep, f = self._filter(labels, masks, excl, n_q)
        return self._hit_lists(lambda nq, nh, a, sc, b: self.lib.afis_rank_hits_filtered(self.ctx, *f, nq, min_score, cap, nh, a, sc), n_q, cap, False)

    def rank_subject_hits_filtered(self, handle, min_score: float, cap: int, labels=None, masks=None, excl=None, n_q: Optional[int] = None):
        """rank_subject_hits over the eligible cells: a person's score is the best among their eligible covered templates; excl: per query a sequence of SUBJECT ids
        that are no entries for it.  A person without an eligible covered template is neither counted nor listed."""
        n_q, keep, f = self._filter(labels, masks, excl, n_q)
        return self._hit_lists(lambda nq, nh, a, sc, b: self.lib.afis_rank_subject_hits_filtered(self.ctx, handle[0], *f, nq, min_score, cap, nh, a, sc, b), n_q, cap, True)

    # ---- rank positions: where a named template or person stands in a query's list ----------------------------------
    def _positions(self, fn, query, names, labels, masks, excl, n_q, subjects: bool, in_score=None):
        q = np.ascontiguousarray(np.asarray(query, np.int32).reshape(-1)); a = np.ascontiguousarray(np.asarray(names, np.int64).reshape(-1))
        if len(q) != len(a):
            raise ValueError("one query position per target")
        n = len(q)
        n_q, keep, flt = self._filter(labels, masks, excl, n_q)
        nb = np.empty(n, np.int64)
        pq, pa, pn = (_ptr(q, C.c_int32), _ptr(a, C.c_int64), _ptr(nb, C.c_int64)) if n else (None, None, None)
        if in_score is not None:
            sc = np.ascontiguousarray(np.asarray(in_score, np.float32).reshape(-1))
            if len(sc) != n:
                raise ValueError("one score per target")
            self._chk(fn(flt, n_q, n, pq, pa, _ptr(sc, C.c_float) if n else None, pn))
            return nb
        st = np.empty(n, np.int32); sc = np.empty(n, np.float32); bi = np.empty(n, np.int64) if subjects else None
        self._chk(fn(flt, n_q, n, pq, pa, _ptr(st, C.c_int32) if n else None, pn, _ptr(sc, C.c_float) if n else None, _ptr(bi, C.c_int64) if subjects and n else None))
        out = {"status": st, "n_before": nb, "score": sc}
        if subjects:
            out["best_idx"] = bi
        return out

    def rank_positions(self, query, idx, labels=None, masks=None, excl=None, n_q: Optional[int] = None):
        """Where named templates stand in the lists of the LAST search: target i is (query[i], idx[i]), a query position of that search and a GLOBAL template index, in
        any order, repeated or not.  -> status [n] (AFIS_POS_LISTED 0, AFIS_POS_NO_ENTRY 1, AFIS_POS_NOT_COVERED 2), n_before [n] — the target's position in the list
        rank_hits_filtered(-inf, cap, labels, masks, excl) gives its query, for every position, not only the first 4096; -1 unless listed — and score [n], the cell's own
        bits (-inf unless listed).  labels / masks / excl are rank_hits_filtered's; n_q defaults as there."""
        return self._positions(lambda f, nq, n, q, a, st, nb, sc, bi: self.lib.afis_rank_positions(self.ctx, *f, nq, n, q, a, st, nb, sc), query, idx, labels, masks, excl, n_q, False)

    def rank_subject_positions(self, handle, query, subject_id, labels=None, masks=None, excl=None, n_q: Optional[int] = None):
        """rank_positions over the enrolled persons of a subjects_create handle, against rank_subject_hits_filtered(-inf, cap): also best_idx [n], the global index of the
        person's best eligible template (-1 unless listed).  excl: per query a sequence of SUBJECT ids; an id the handle does not hold is AFIS_POS_NOT_COVERED."""
        return self._positions(lambda f, nq, n, q, a, st, nb, sc, bi: self.lib.afis_rank_subject_positions(self.ctx, handle[0], *f, nq, n, q, a, st, nb, sc, bi),
                               query, subject_id, labels, masks, excl, n_q, True)

    def count_before(self, query, score, idx, labels=None, masks=None, excl=None, n_q: Optional[int] = None):
        """The sharding primitive: n_before [n], per target the number of entries of row query[i] of the LAST search — under the same optional filters — that stand
        before a hypothetical entry (score[i], idx[i]); a column whose global index is idx[i] is never counted, and idx[i] need not be covered.  Summed over the ranks
        of a sharded gallery (host/sharding.py::merge_positions) that is the target's global position."""
        return self._positions(lambda f, nq, n, q, a, sc, nb: self.lib.afis_count_before(self.ctx, *f, nq, n, q, sc, a, nb), query, idx, labels, masks, excl, n_q, False, in_score=score)

    # ---- cohort statistics and z-normalised scores -----------------------------------------------------------------------
    def score_stats(self, axis: int = 0, labels=None, masks=None, excl=None, n_q: Optional[int] = None) -> np.ndarray:
        """Exact integer statistics of the LAST search's matrix, per query (axis 0: [n_q]) or per column (axis 1: [columns], in the order of the search's scores
        output), over the cells the filter leaves — labels / masks / excl are rank_hits_filtered's: elimination prints and a known mate go into excl.  -> a structured
        array of dtype SCORE_STAT: n valued cells, n_outside, s1 = sum q, s2 = s2_hi x 2^64 + s2_lo = sum q^2 with q = rint(score x 2^20), min, max.  Statistics of
        disjoint shards add up bit for bit (host/sharding.py::merge_score_stats); score_moments gives mean and deviation.  The matrix stays as it is."""
        n_q, keep, f = self._filter(labels, masks, excl, n_q)
        out = np.zeros(n_q if axis == 0 else self.last_n_templates, SCORE_STAT)
        self._chk(self.lib.afis_score_stats(self.ctx, axis, *f, n_q, out.ctypes.data_as(C.c_void_p) if len(out) else None))
        return out

    def normalize_scores(self, offset, scale, axis: int = 0, want_scores: bool = False, n_q: Optional[int] = None):
        """Every valued cell v of the LAST search's matrix becomes z = float32((float64(v) - offset) * scale) with its row's (axis 0) or column's (axis 1) pair, every
        other cell no entry; every ranking call then reads z-scores and takes min_score in z units.  offset finite, scale finite and > 0.  A second call, or
        score_stats, on the normalised matrix is AFIS_ESTATE until the next search.  -> the normalised matrix [n_q][columns] if want_scores, else None."""
        n_q = self.last_n_q if n_q is None else n_q
        o = np.ascontiguousarray(np.asarray(offset, np.float64).reshape(-1)); s = np.ascontiguousarray(np.asarray(scale, np.float64).reshape(-1))
        n = n_q if axis == 0 else self.last_n_templates
        if len(o) != n or len(s) != n:
            raise ValueError("one (offset, scale) pair per %s" % ("query" if axis == 0 else "column"))
        out = np.empty((n_q, self.last_n_templates), np.float32) if want_scores else None
        self._chk(self.lib.afis_normalize_scores(self.ctx, axis, n_q, _ptr(o, C.c_double) if n else None, _ptr(s, C.c_double) if n else None,
                                                 _ptr(out, C.c_float) if want_scores else None))
        return out

    def score_moments(self, stats):
        """(mean, sd) float64 arrays of a SCORE_STAT array, by afis_score_stat_moments: the population deviation from exact integers; n == 0 gives (0, 0)."""
        st = np.ascontiguousarray(np.asarray(stats, SCORE_STAT).reshape(-1))
        mean = np.zeros(len(st)); sd = np.zeros(len(st))
        m, d = C.c_double(), C.c_double()
        for i in range(len(st)):
            if self.lib.afis_score_stat_moments(C.c_void_p(st.ctypes.data + i * SCORE_STAT.itemsize), C.byref(m), C.byref(d)) != 0:
                raise AfisError("afis_score_stat_moments: statistic %d is outside the bound n <= 2^27 or inconsistent" % i)
            mean[i] = m.value; sd[i] = d.value
        return mean, sd

    # ---- score distributions: per-row histograms and the entry at any rank ------------------------------------------------
    def score_histogram(self, edges, axis: int = 0, labels=None, masks=None, excl=None, n_q: Optional[int] = None) -> np.ndarray:
        """Histograms of the LAST search's matrix, per query (axis 0: [n_q][len(edges) + 1]) or per column (axis 1: [columns][len(edges) + 1], in the order of the
        search's scores output), over the entries the filter leaves — labels / masks / excl are rank_hits_filtered's.  edges: 1 .. 1023 float32, no NaN, strictly
        ascending.  An entry goes to bin b = the number of edges <= its score (by rank key: the two zeros are one value); bin 0 lies below edges[0], the last bin
        reaches edges[-1]; the no-entry word and NaNs with the sign set are counted nowhere.  counts[r, j + 1:].sum() is rank_hits_filtered(edges[j])'s n_hits.  int64;
        histograms of disjoint shards add up (host/sharding.py::merge_score_histograms).  A normalised matrix is accepted: edges in z units.  The matrix stays as it is."""
        n_q, keep, f = self._filter(labels, masks, excl, n_q)
        e = np.ascontiguousarray(np.asarray(edges, np.float32).reshape(-1))
        out = np.zeros((n_q if axis == 0 else self.last_n_templates, len(e) + 1), np.int64)
        self._chk(self.lib.afis_score_histogram(self.ctx, axis, *f, n_q, len(e), _ptr(e, C.c_float) if len(e) else None, _ptr(out, C.c_int64) if out.size else None))
        return out

    def entries_at(self, query, rank, labels=None, masks=None, excl=None, n_q: Optional[int] = None):
        """Which entry stands at a rank of the lists of the LAST search: target i is (query[i], rank[i]), a query position of that search and a rank >= 0, in any order,
        repeated or not.  -> status [n] (AFIS_POS_LISTED 0, AFIS_POS_NO_ENTRY 1), idx [n] — the GLOBAL index of entry rank[i] of the list rank_hits_filtered(-inf, cap,
        labels, masks, excl) gives its query, for every rank, not only the first 4096; -1 where the row has no more than rank[i] entries — and score [n], the cell's
        own bits (-inf unless listed).  The inverse of rank_positions: rank_positions(query, idx)["n_before"] == rank.  labels / masks / excl are rank_hits_filtered's."""
        q = np.ascontiguousarray(np.asarray(query, np.int32).reshape(-1)); r = np.ascontiguousarray(np.asarray(rank, np.int64).reshape(-1))
        if len(q) != len(r):
            raise ValueError("one query position per rank")
        n = len(q)
        n_q, keep, f = self._filter(labels, masks, excl, n_q)
        st = np.empty(n, np.int32); ix = np.empty(n, np.int64); sc = np.empty(n, np.float32)
        self._chk(self.lib.afis_entries_at(self.ctx, *f, n_q, n, _ptr(q, C.c_int32) if n else None, _ptr(r, C.c_int64) if n else None, _ptr(st, C.c_int32) if n else None,
                                           _ptr(ix, C.c_int64) if n else None, _ptr(sc, C.c_float) if n else None))
        return {"status": st, "idx": ix, "score": sc}

    # ---- person distributions: the three calls above over enrolled persons ---------------------------------------------------------
    def subject_score_stats(self, handle, axis: int = 0, labels=None, masks=None, excl=None, n_q: Optional[int] = None) -> np.ndarray:
        """score_stats over the enrolled persons of a subjects_create handle: a person's cell is the best score among their eligible covered templates (as
        rank_subject_hits_filtered's), per query (axis 0: [n_q], the cohort of persons) or per person over the queries (axis 1: [subjects], ascending id: handle[2]).
        excl: per query a sequence of SUBJECT ids.  A person nothing covers gives the empty statistic.  AFIS_ESTATE on a normalised matrix, as score_stats."""
        n_q, keep, flt = self._filter(labels, masks, excl, n_q)
        out = np.zeros(n_q if axis == 0 else len(handle[2]), SCORE_STAT)
        self._chk(self.lib.afis_subject_score_stats(self.ctx, handle[0], axis, *flt, n_q, out.ctypes.data_as(C.c_void_p) if len(out) else None))
        return out

    def subject_score_histogram(self, handle, edges, axis: int = 0, labels=None, masks=None, excl=None, n_q: Optional[int] = None) -> np.ndarray:
        """score_histogram over the enrolled persons of a subjects_create handle, per query (axis 0: [n_q][len(edges) + 1]) or per person (axis 1: [subjects][...],
        ascending id: handle[2]).  A person's key is the RAW ordered word of their best cell, as in rank_subject_hits: -0.0 lies below +0.0, for persons and for edges,
        so (-0.0, +0.0) are two edges.  counts[q, j + 1:].sum() is rank_subject_hits_filtered(edges[j])'s n_hits.  excl: per query a sequence of SUBJECT ids."""
        n_q, keep, flt = self._filter(labels, masks, excl, n_q)
        e = np.ascontiguousarray(np.asarray(edges, np.float32).reshape(-1))
        out = np.zeros((n_q if axis == 0 else len(handle[2]), len(e) + 1), np.int64)
        self._chk(self.lib.afis_subject_score_histogram(self.ctx, handle[0], axis, *flt, n_q, len(e), _ptr(e, C.c_float) if len(e) else None, _ptr(out, C.c_int64) if out.size else None))
        return out

    def subject_entries_at(self, handle, query, rank, labels=None, masks=None, excl=None, n_q: Optional[int] = None):
        """entries_at over the enrolled persons of a subjects_create handle: -> status [n], subject [n] — the id of entry rank[i] of the list
        rank_subject_hits_filtered(-inf, cap, labels, masks, excl) gives query[i], for every rank; -1 where the row has no more than rank[i] persons —, score [n] and
        best_idx [n], the person's best score and the GLOBAL index of the template that holds it.  The inverse of rank_subject_positions."""
        n_q, keep, flt = self._filter(labels, masks, excl, n_q)
        q = np.ascontiguousarray(np.asarray(query, np.int32).reshape(-1)); r = np.ascontiguousarray(np.asarray(rank, np.int64).reshape(-1))
        if len(q) != len(r):
            raise ValueError("one query position per rank")
        n = len(q)
        st = np.empty(n, np.int32); sid = np.empty(n, np.int64); sc = np.empty(n, np.float32); bi = np.empty(n, np.int64)
        self._chk(self.lib.afis_subject_entries_at(self.ctx, handle[0], *flt, n_q, n, _ptr(q, C.c_int32) if n else None, _ptr(r, C.c_int64) if n else None, _ptr(st, C.c_int32) if n else None,
                                                   _ptr(sid, C.c_int64) if n else None, _ptr(sc, C.c_float) if n else None, _ptr(bi, C.c_int64) if n else None))
        return {"status": st, "subject": sid, "score": sc, "best_idx": bi}

    def expand_subject_pairs(self, handle, offset, scale, columns=None):
        """Per-person (offset, scale) — one pair per distinct id of the subjects_create handle, ascending: handle[2], the order of subject_score_stats(handle, axis=1) —
        as the per-column arrays normalize_scores(axis=1) takes, in the search's column order.  columns: None — a search of the whole resident shard —, or the GLOBAL
        template indices of the search's columns in the order of its scores output (a subset's list as given to subset_create).  z = (v - offset) x scale with
        scale > 0 is increasing, so after normalize_scores(*expand_subject_pairs(...), axis=1) a person's best z is the z of their best score: every subject list then
        holds person z-scores."""
        names, per_template = handle[2], handle[3]
        o = np.asarray(offset, np.float64).reshape(-1); s = np.asarray(scale, np.float64).reshape(-1)
        if len(o) != len(names) or len(s) != len(names):
            raise ValueError("one (offset, scale) pair per subject of the handle")
        local = np.arange(len(per_template)) if columns is None else np.asarray(columns, np.int64).reshape(-1) - self.index_base
        if len(local) and (local.min() < 0 or local.max() >= len(per_template)):
            raise ValueError("a column is not a template of the resident shard")
        slot = np.searchsorted(names, per_template[local])
        return o[slot], s[slot]

    # ---- link groups: the connected components rows and columns make above a decision score ----------------------------------
    def _link(self, fn, min_score, mode, row_node, labels, masks, excl, cap_groups, cap_members, n_q):
        n_q, keep, flt = self._filter(labels, masks, excl, n_q)
        rn = None if row_node is None else np.ascontiguousarray(np.asarray(row_node, np.int64).reshape(-1))
        if rn is not None and len(rn) != n_q:
            raise ValueError("one row_node per query")

        def call(cg, cm):
            cnt = np.zeros(4, np.int64)
            goff = np.zeros(max(cg, 0) + 1, np.int64); mem = np.zeros(max(cm, 1), np.int64)
            c = [C.cast(cnt.ctypes.data + 8 * i, C.POINTER(C.c_int64)) for i in range(4)]
            self._chk(fn(flt, n_q, _ptr(rn, C.c_int64) if rn is not None and n_q else None, min_score, mode, cg, cm, c[0], c[1], c[2], c[3], _ptr(goff, C.c_int64), _ptr(mem, C.c_int64)))
            return cnt, goff, mem

        if cap_groups is None or cap_members is None:                       # the counts first, then lists of exactly that size
            cnt, _, _ = call(0, 0)
            cap_groups = int(cnt[1]) if cap_groups is None else cap_groups; cap_members = int(cnt[2]) if cap_members is None else cap_members
        cnt, goff, mem = call(cap_groups, cap_members)
        listed = int(cnt[3])
        return {"n_edges": int(cnt[0]), "n_groups": int(cnt[1]), "n_members": int(cnt[2]), "n_listed": listed, "group_off": goff[:listed + 1].copy(), "member": mem[:int(goff[listed])].copy()}

    def link_groups(self, min_score: float, mode: int = 0, row_node=None, labels=None, masks=None, excl=None, cap_groups: Optional[int] = None, cap_members: Optional[int] = None,
                    n_q: Optional[int] = None):
        """The groups the LAST search's matrix makes at min_score: the connected components, of two or more nodes, of the graph whose nodes are the columns (named by GLOBAL
        template index) and the rows — row q is the node row_node[q] (a global template index: the resident print the row is; a name that is a column's is that column's
        node) or, at -1 / row_node None, a latent reported as -1 - q — and whose edges are the cells that reach min_score between different nodes (mode 0,
        AFIS_LINK_ANY), in mode 1 (AFIS_LINK_MUTUAL) only where the reverse cell reaches too.  labels / masks / excl are rank_hits_filtered's.  -> n_edges (cells that are
        edges), n_groups, n_members (true totals), n_listed, group_off [n_listed + 1], member [group_off[-1]]: a CSR over the longest prefix of the groups that fits both
        caps; members by ascending name, then latents; groups by their first member.  A cap of None: the call runs twice, the first time for the counts.  Groups of
        disjoint shards merge by name (host/sharding.py::merge_link_groups).  A normalised matrix is accepted: min_score in z units.  The matrix stays as it is."""
        return self._link(lambda f, nq, rn, ms, md, cg, cm, *out: self.lib.afis_link_groups(self.ctx, *f, nq, rn, ms, md, cg, cm, *out),
                          min_score, mode, row_node, labels, masks, excl, cap_groups, cap_members, n_q)

    def link_subject_groups(self, handle, min_score: float, mode: int = 0, row_node=None, labels=None, masks=None, excl=None, cap_groups: Optional[int] = None,
                            cap_members: Optional[int] = None, n_q: Optional[int] = None):
        """link_groups over the enrolled persons of a subjects_create handle: all columns of one person are ONE node, named by the subject id; row_node and excl hold
        SUBJECT ids (an id the handle does not hold is a node of its own name); two prints of one person never link.  Mode 1 reads the reverse cell at the person's
        first column by ascending global index."""
        return self._link(lambda f, nq, rn, ms, md, cg, cm, *out: self.lib.afis_link_subject_groups(self.ctx, handle[0], *f, nq, rn, ms, md, cg, cm, *out),
                          min_score, mode, row_node, labels, masks, excl, cap_groups, cap_members, n_q)

    # ---- kept matrices: the last search's matrix kept, read, recalled and fused on the device ------------------------------
    def matrix_keep(self):
        """A device copy of the LAST search's matrix with its record (n_q, columns, subset, gallery epoch, normalised mark) -> a handle for the calls below.  The
        matrix stays as it is.  Free it with matrix_free; close() releases what is left."""
        h = C.c_void_p()
        self._chk(self.lib.afis_matrix_keep(self.ctx, C.byref(h)))
        return h

    def matrix_free(self, handle):
        self.lib.afis_matrix_free(self.ctx, handle)

    def matrix_info(self, handle) -> dict:
        """-> {"n_q", "normalized", "columns", "over_subset", "stale"}; answers for a stale handle too."""
        d = MatrixDesc()
        self._chk(self.lib.afis_matrix_info(self.ctx, handle, C.byref(d)))
        return {"n_q": d.n_q, "normalized": bool(d.normalized), "columns": d.columns, "over_subset": bool(d.over_subset), "stale": bool(d.stale)}

    def matrix_read(self, handle, row0: int = 0, n_rows: Optional[int] = None) -> np.ndarray:
        """Rows row0 .. row0 + n_rows - 1 (default: all from row0 on) of a kept matrix -> [n_rows][columns] float32, the columns in the order of the search's scores."""
        info = self.matrix_info(handle)
        n_rows = info["n_q"] - row0 if n_rows is None else n_rows
        out = np.empty((max(n_rows, 0), info["columns"]), np.float32)
        self._chk(self.lib.afis_matrix_read(self.ctx, handle, row0, n_rows, _ptr(out, C.c_float) if out.size else None))
        return out

    def matrix_recall(self, handle):
        """The kept matrix becomes the last search's matrix again, record and normalised mark included; the handle stays usable."""
        self._chk(self.lib.afis_matrix_recall(self.ctx, handle))
        info = self.matrix_info(handle)
        self.last_n_q = info["n_q"]; self.last_n_templates = info["columns"]

    def matrix_fuse(self, handles, mode: int = FUSE_SUM, weights=None, transposed=None, want_scores: bool = False):
        """The kept matrices `handles` (1 .. 16, all of one shape, column set and kind) folded cell by cell in argument order — FUSE_SUM (fp64, with weights),
        FUSE_MAX, FUSE_MIN, FUSE_REQUIRE_ALL or-ed in — into the last search's matrix, which every ranking call then reads.  transposed[k] true reads operand k
        transposed (square matrices whose row i and column i are the same print).  -> the fused matrix [n_q][columns] if want_scores, else None."""
        hs = list(handles)
        n = len(hs)
        arr = (C.c_void_p * max(n, 1))(*[h if isinstance(h, C.c_void_p) else C.c_void_p(h) for h in hs])
        w = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1))
        t = None if transposed is None else np.ascontiguousarray(np.asarray(transposed).reshape(-1) != 0).astype(np.uint8)
        if (w is not None and len(w) != n) or (t is not None and len(t) != n):
            raise ValueError("one weight and one transposed flag per operand")
        out = None
        if want_scores and 1 <= n <= FUSE_OPERANDS_MAX:
            info = self.matrix_info(hs[0])
            out = np.empty((info["n_q"], info["columns"]), np.float32)
        self._chk(self.lib.afis_matrix_fuse(self.ctx, arr, _ptr(w, C.c_double) if w is not None and n else None, _ptr(t, C.c_uint8) if t is not None and n else None, n, mode,
                                            _ptr(out, C.c_float) if out is not None and out.size else None))
        info = self.matrix_info(hs[0])
        self.last_n_q = info["n_q"]; self.last_n_templates = info["columns"]
        return out

    # ---- eligible search: only the pairs a latent is eligible for are scored -----------------------------------------
    def search_eligible(self, latents: Sequence[FPTemplate], labels, masks, want_scores: bool = True):
        """search() that scores a (latent, template) pair only where the template's label passes the latent's masks (labels: a labels_create handle; masks [n_q][3]
        uint64 as rank_hits_filtered takes them; both required).  scores [n_q][G]: an eligible cell is search()'s value bit for bit, every other cell the no-entry
        word 0xffffffff (a NaN: compare scores.view(np.uint32)).  The matrix left on the device is read by rank_hits / rank_subject_hits / rank_latent_hits as their
        _filtered forms read a full search's; the _filtered calls (case lists: always those) return what they return after a full search.  timing()["pairs"] counts
        the pairs scored; get_option("eligible_classes") the distinct mask triples.  It pays when latents share masks."""
        v = _Views(latents)
        mk = None if masks is None else np.ascontiguousarray(np.asarray(masks, np.uint64).reshape(v.n, 3))
        if mk is not None and v.n == 0:
            mk = np.zeros((1, 3), np.uint64)                                 # (no query: the C call still wants a masks pointer)
        G = self.resident_size
        scores = np.empty((v.n, G), np.float32) if want_scores else None
        status = np.zeros(v.n, np.int32)
        self._chk(self.lib.afis_search_eligible(self.ctx, labels[0] if labels is not None else None, _ptr(mk, C.c_uint64) if mk is not None else None, v.arr, v.n,
                                                _ptr(scores, C.c_float) if want_scores else None, _ptr(status, C.c_int32)))
        self.last_n_q = v.n; self.last_n_templates = G
        return {"scores": scores, "status": status}

    def debug_expand_rows(self, cls: np.ndarray, row_of: Sequence[int], sel, out: np.ndarray) -> np.ndarray:
        """k_expand_rows on planted data (parity tap): cls [n_c][m] words of one class, row_of [n_c] its rows of out [n_q][G], sel [m] ascending columns (None: the
        identity, m == G; m == 0: no column).  -> out with the class's rows rewritten: cls[r][i] at column sel[i], 0xffffffff elsewhere.  uint32 or float32 arrays."""
        c = np.ascontiguousarray(cls).view(np.float32); o = np.array(out, copy=True, order="C").view(np.float32)
        ro = np.ascontiguousarray(np.asarray(row_of, np.int32).reshape(-1))
        se = None if sel is None else np.ascontiguousarray(np.asarray(sel, np.int32).reshape(-1))
        n_c, m = c.shape
        self._chk(self._tap("afis_debug_expand_rows")(self.ctx, _ptr(c, C.c_float) if c.size else None, n_c, m, _ptr(ro, C.c_int32), _ptr(se, C.c_int32) if se is not None and len(se) else None,
                                                      o.shape[0], o.shape[1], _ptr(o, C.c_float)))
        return o.view(np.asarray(out).dtype)

    # ---- weighted search: any set of a latent's templates, fused on the device ---------------------------------------
    def search_weighted(self, latents: Sequence[FPTemplate], w_minu, w_tex, want_scores: bool = True, n_wm=None, n_wt=None):
        """search() over ANY set of each latent's templates: w_minu [n_q][n_wm] / w_tex [n_q][n_wt] float32 weights (a 1-D row is every query's row; None with width
        0), a template being scored where its weight is not zero and it exists.  scores [n_q][G]: -1 for an empty entry and for the whole row of a latent without an
        active template (status AFIS_QUERY_LATENT_EMPTY), otherwise the fp64 sum of weight x score over the active minutiae, then texture templates, in ascending
        order, as one float32.  The matrix left on the device is a full search's: every rank_* call reads it.  n_wm / n_wt override the widths handed to the C call
        (argument tests).  timing()["pairs"] = pseudo-queries x G; get_option("weighted_pseudo_queries"), get_option("weighted_fold_us")."""
        v = _Views(latents)

        def rows(w):
            if w is None:
                return None, 0
            a = np.asarray(w, np.float32)
            if a.ndim == 1:
                a = np.broadcast_to(a, (v.n, a.shape[0]))
            a = np.ascontiguousarray(a.reshape(v.n, -1) if v.n else a.reshape(0, a.shape[-1]))
            return a, a.shape[1]
        wm, nm = rows(w_minu); wt, nt = rows(w_tex)
        G = self.resident_size
        scores = np.empty((v.n, G), np.float32) if want_scores else None
        status = np.zeros(v.n, np.int32)
        self._chk(self.lib.afis_search_weighted(self.ctx, v.arr, v.n, _ptr(wm, C.c_float) if wm is not None and wm.size else None, nm if n_wm is None else n_wm,
                                                _ptr(wt, C.c_float) if wt is not None and wt.size else None, nt if n_wt is None else n_wt,
                                                _ptr(scores, C.c_float) if want_scores else None, _ptr(status, C.c_int32)))
        self.last_n_q = v.n; self.last_n_templates = G
        return {"scores": scores, "status": status}

    # ---- print search: resident prints as queries, built on the device -----------------------------------------------
    def search_prints(self, idx, w_minu, w_tex, subset=None, want_scores: bool = True):
        """search_weighted() with RESIDENT prints as the queries: idx [n_q] global indices of the resident shard (any order, repeats allowed), w_minu / w_tex one weight
        per query (a scalar is every query's) for the print's minutiae and texture template.  The query views are built on the device from the shard — no template is
        uploaded —, cell (q, column) is bit for bit search_weighted's for that view, a print against itself included (take it out with an exclusion list).
        subset: a subset_create handle — the columns are its templates in the caller's order; otherwise the whole resident shard.  The matrix left on the device is a
        search's: every rank_* call reads it.  get_option("print_gather_us"), get_option("print_h2d_bytes")."""
        a = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        n = len(a)
        wm = np.ascontiguousarray(np.broadcast_to(np.asarray(w_minu, np.float32), (n,)))
        wt = np.ascontiguousarray(np.broadcast_to(np.asarray(w_tex, np.float32), (n,)))
        cols = subset[1] if subset is not None else self.resident_size
        scores = np.empty((n, cols), np.float32) if want_scores else None
        status = np.zeros(n, np.int32)
        self._chk(self.lib.afis_search_prints(self.ctx, subset[0] if subset is not None else None, _ptr(a, C.c_int64) if n else None, n,
                                              _ptr(wm, C.c_float) if n else None, _ptr(wt, C.c_float) if n else None,
                                              _ptr(scores, C.c_float) if want_scores else None, _ptr(status, C.c_int32)))
        self.last_n_q = n; self.last_n_templates = cols
        return {"scores": scores, "status": status}

    # ---- cascade search: minutiae for every print, texture for the best `keep` only ----------------------------------
    def search_cascade(self, handle, keep: int, want_scores: bool = True, want_kept: bool = True):
        """afis_search_cascade over an upload_queries handle: the three minutiae scorers for every cell, per latent the `keep` best by that partial score selected on the
        device, the texture scorer for those only.  A kept cell is bit for bit search()'s; every other cell of "scores" [n_q][G] holds the no-entry word 0xffffffff.
        want_kept: "n_kept" [n_q], "kept_idx" [n_q][keep] (global indices in stage-1 rank order, -1 padded) and "kept_parts" [n_q][keep][4].  The matrix left on the
        device reads as search_eligible's: rank_hits, rank_positions (a mate stage 1 dropped is POS_NO_ENTRY) and the _filtered calls see the kept cells only.
        get_option("cascade_stage1_us" / "cascade_select_us" / "cascade_stage2_us" / "cascade_kept_pairs"); set_option("cascade_pairs_per_launch", n)."""
        h, n = handle
        keep = int(keep)
        G = self.resident_size
        wide = max(keep, 1)
        scores = np.empty((n, G), np.float32) if want_scores else None
        status = np.zeros(n, np.int32)
        n_kept = np.zeros(n, np.int64) if want_kept else None
        kept_idx = np.full((n, wide), -1, np.int64) if want_kept else None
        kept_parts = np.zeros((n, wide, 4), np.float32) if want_kept else None
        self._chk(self.lib.afis_search_cascade(self.ctx, h, keep, _ptr(scores, C.c_float) if want_scores else None, _ptr(status, C.c_int32),
                                               _ptr(n_kept, C.c_int64) if want_kept else None, _ptr(kept_idx, C.c_int64) if want_kept else None,
                                               _ptr(kept_parts, C.c_float) if want_kept else None))
        self.last_n_q = n; self.last_n_templates = G
        return {"scores": scores, "status": status, "n_kept": n_kept, "kept_idx": kept_idx, "kept_parts": kept_parts}

    def _cascade_out(self, n: int, cols: int, keep: int, want_scores: bool, want_kept: bool):
        wide = max(keep, 1)
        scores = np.empty((n, cols), np.float32) if want_scores else None
        status = np.zeros(n, np.int32)
        n_kept = np.zeros(n, np.int64) if want_kept else None
        kept_idx = np.full((n, wide), -1, np.int64) if want_kept else None
        kept_parts = np.zeros((n, wide, 4), np.float32) if want_kept else None
        args = (_ptr(scores, C.c_float) if want_scores else None, _ptr(status, C.c_int32), _ptr(n_kept, C.c_int64) if want_kept else None,
                _ptr(kept_idx, C.c_int64) if want_kept else None, _ptr(kept_parts, C.c_float) if want_kept else None)
        return {"scores": scores, "status": status, "n_kept": n_kept, "kept_idx": kept_idx, "kept_parts": kept_parts}, args

    def search_cascade_subset(self, subset, handle, keep: int, want_scores: bool = True, want_kept: bool = True):
        """afis_search_cascade_subset: search_cascade() over the columns of a subset_create handle.  "scores" [n_q][n] in the caller's column order — a kept cell is bit
        for bit search_subset_resident()'s, every other the no-entry word —, "n_kept" = min(keep, n), "kept_idx" global indices in stage-1 rank order (equal keys by
        ascending global index), "kept_parts" [n_q][keep][4].  The matrix left on the device is a subset search's: the rank_* calls name its columns by global index
        and see the kept cells only.  The options are search_cascade's."""
        sh, n_cols = subset
        h, n = handle
        keep = int(keep)
        out, args = self._cascade_out(n, n_cols, keep, want_scores, want_kept)
        self._chk(self.lib.afis_search_cascade_subset(self.ctx, sh, h, keep, *args))
        self.last_n_q = n; self.last_n_templates = n_cols
        return out

    def search_cascade_eligible(self, latents: Sequence[FPTemplate], labels, masks, keep: int, want_scores: bool = True, want_kept: bool = True):
        """afis_search_cascade_eligible: search_eligible()'s arguments plus keep — per latent the cascade over the templates whose label passes its masks only.  "n_kept"
        = min(keep, eligible templates); the kept prints are the best `keep` ELIGIBLE ones by the stage-1 score; a kept cell of "scores" [n_q][G] is bit for bit
        search()'s, every other cell — dropped or not eligible — the no-entry word.  The matrix left on the device reads as search_eligible's.
        get_option("eligible_classes"); the "cascade_*" options hold the sums over the classes."""
        v = _Views(latents)
        mk = None if masks is None else np.ascontiguousarray(np.asarray(masks, np.uint64).reshape(v.n, 3))
        if mk is not None and v.n == 0:
            mk = np.zeros((1, 3), np.uint64)                                 # (no query: the C call still wants a masks pointer)
        keep = int(keep)
        G = self.resident_size
        out, args = self._cascade_out(v.n, G, keep, want_scores, want_kept)
        self._chk(self.lib.afis_search_cascade_eligible(self.ctx, labels[0] if labels is not None else None, _ptr(mk, C.c_uint64) if mk is not None else None, v.arr, v.n,
                                                        keep, *args))
        self.last_n_q = v.n; self.last_n_templates = G
        return out

    def debug_kept_cells_mapped(self, G_res: int, m: int, keep: int, n_kept: int, index_base: int, kept, has, q_first, per_launch: int, sel, parts, pair_score, row_of, out_col,
                             out: np.ndarray, tab_ints: int):
        """k_cascade_gather_mapped and k_cascade_scatter_mapped on planted tables (parity tap; include/afis_matcher_taps.h has the shapes).  sel / row_of / out_col may be
        None (the identity).  -> {"tab" [tab_ints] int32 (planted with -7 before the call), "n_pieces", "pair_parts" [pairs][4] uint32 (planted with 0xa5a5a5a5), "out"}."""
        kp = np.ascontiguousarray(np.asarray(kept, np.int64)); n_q = kp.shape[0]
        hs = np.ascontiguousarray(np.asarray(has, np.uint8)); qf = np.ascontiguousarray(np.asarray(q_first, np.int32))
        pt = np.ascontiguousarray(parts).view(np.float32).reshape(n_q, m, 4)
        ps = np.ascontiguousarray(pair_score).view(np.float32).reshape(-1)
        opt = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))
        se, ro, oc = opt(sel), opt(row_of), opt(out_col)
        p32 = lambda a: None if a is None else _ptr(a, C.c_int32)
        o = np.array(out, copy=True, order="C").view(np.float32)
        tab = np.full(tab_ints, -7, np.int32); n_pieces = np.zeros(1, np.int32)
        pp = np.full((max(len(ps), 1), 4), 0xA5A5A5A5, np.uint32)
        self._chk(self._tap("afis_debug_kept_cells_mapped")(self.ctx, n_q, G_res, m, keep, n_kept, index_base, _ptr(kp, C.c_int64), _ptr(hs, C.c_uint8), _ptr(qf, C.c_int32), len(qf) - 1,
                                                         per_launch, p32(se), _ptr(pt, C.c_float), _ptr(ps, C.c_float) if len(ps) else _ptr(pp.view(np.float32), C.c_float),
                                                         p32(ro), p32(oc), o.shape[0], o.shape[1], _ptr(tab, C.c_int32), tab_ints, _ptr(n_pieces, C.c_int32),
                                                         _ptr(pp.view(np.float32), C.c_float), _ptr(o, C.c_float)))
        return {"tab": tab, "n_pieces": int(n_pieces[0]), "pair_parts": pp[:len(ps)], "out": o.view(np.asarray(out).dtype)}

    # ---- print cascade: resident prints as queries, minutiae for every column, texture for the best `keep` only ----------
    def search_prints_cascade(self, idx, w_minu, w_tex, keep: int, want_scores: bool = True, want_kept: bool = True):
        """afis_search_prints_cascade: search_prints() with a minutiae first stage.  idx [n_q] global indices of the resident shard, w_minu / w_tex one weight per query
        (a scalar is every query's).  The print's minutiae scorer runs for every column, per query the `keep` best columns by that partial score are selected on the
        device, the texture scorer runs for those only.  A kept cell is bit for bit search_prints()' for the same weights; every other cell of "scores" [n_q][G] holds
        the no-entry word 0xffffffff.  want_kept: "n_kept" [n_q], "kept_idx" [n_q][keep] (global indices in stage-1 rank order, -1 padded) and "kept_parts"
        [n_q][keep][2] = score_print_pairs()' parts of the kept pairs.  The matrix left on the device reads as search_cascade's: rank_hits, rank_positions (a column
        stage 1 dropped is POS_NO_ENTRY) and the _filtered calls see the kept cells only; take the self cell out with an exclusion list.
        get_option("print_cascade_stage1_us" / "print_cascade_select_us" / "print_cascade_stage2_us" / "print_cascade_kept_pairs"); set_option("cascade_pairs_per_launch", n)."""
        a = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        n = len(a)
        wm = np.ascontiguousarray(np.broadcast_to(np.asarray(w_minu, np.float32), (n,)))
        wt = np.ascontiguousarray(np.broadcast_to(np.asarray(w_tex, np.float32), (n,)))
        keep = int(keep)
        G = self.resident_size
        wide = max(keep, 1)
        scores = np.empty((n, G), np.float32) if want_scores else None
        status = np.zeros(n, np.int32)
        n_kept = np.zeros(n, np.int64) if want_kept else None
        kept_idx = np.full((n, wide), -1, np.int64) if want_kept else None
        kept_parts = np.zeros((n, wide, 2), np.float32) if want_kept else None
        self._chk(self.lib.afis_search_prints_cascade(self.ctx, _ptr(a, C.c_int64) if n else None, n, _ptr(wm, C.c_float) if n else None, _ptr(wt, C.c_float) if n else None,
                                                      keep, _ptr(scores, C.c_float) if want_scores else None, _ptr(status, C.c_int32),
                                                      _ptr(n_kept, C.c_int64) if want_kept else None, _ptr(kept_idx, C.c_int64) if want_kept else None,
                                                      _ptr(kept_parts, C.c_float) if want_kept else None))
        self.last_n_q = n; self.last_n_templates = G
        return {"scores": scores, "status": status, "n_kept": n_kept, "kept_idx": kept_idx, "kept_parts": kept_parts}

    def debug_print_queries(self, idx, use_minu=None, use_tex=None) -> dict:
        """One launch group of search_prints built from the resident prints idx (parity tap) and copied back: the seven tables and the seven arrays of the group,
        as the device holds them; use_minu / use_tex [n] select what of a print is active (default: everything it has)."""
        a = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        n = len(a)
        um = np.ascontiguousarray(np.ones(n, np.uint8) if use_minu is None else np.asarray(use_minu, np.uint8).reshape(n))
        ut = np.ascontiguousarray(np.ones(n, np.uint8) if use_tex is None else np.asarray(use_tex, np.uint8).reshape(n))
        counts = np.zeros(4, np.int32)
        fn = self._tap("afis_debug_print_queries")
        head = (self.ctx, _ptr(a, C.c_int64), n, _ptr(um, C.c_uint8), _ptr(ut, C.c_uint8), _ptr(counts, C.c_int32))
        self._chk(fn(*head, *([None] * 14)))
        n_lm, n_tiles, n_lt = (int(c) for c in counts[:3])
        out = {"lm_off": np.full(3 * n + 1, -7, np.int32), "lm_tile_off": np.full(3 * n + 1, -7, np.int32), "lt_off": np.full(n + 1, -7, np.int32),
               "tile_off": np.full(n + 1, -7, np.int32), "tile16_off": np.full(n + 1, -7, np.int32), "tex_slot": np.full(n, -7, np.int32), "status": np.full(n, -7, np.int32),
               "lm_xy": np.zeros((n_lm, 2), np.int16), "lm_ori": np.zeros(n_lm, np.float32), "lm_des": np.zeros((n_lm, 96), np.float32),
               "lm_frag": np.zeros((n_tiles, 6, 64, 4), np.float32), "lt_xy": np.zeros((n_lt, 2), np.int16), "lt_ori": np.zeros(n_lt, np.float32),
               "lt_des": np.zeros((n_lt, 96), np.float32)}
        ptrs = [_ptr(out[k], C.c_int16 if k.endswith("_xy") else C.c_int32 if out[k].dtype == np.int32 else C.c_float) for k in out]
        self._chk(fn(*head, *ptrs))
        out["lt_pad"] = int(counts[3])
        return out

    def debug_fold_templates(self, parts: np.ndarray, qd, w: np.ndarray, empty) -> np.ndarray:
        """k_fold_templates on planted data (parity tap): parts [n_pseudo][G][4] float32 (any bit patterns), qd [n_q][4] int32 = (first pseudo-query, n_pq, n_at,
        status), w [n_pseudo][4] weights aligned to the part slots, empty [G] uint8.  -> out [n_q][G] float32."""
        p = np.ascontiguousarray(parts).view(np.float32); d = np.ascontiguousarray(np.asarray(qd, np.int32).reshape(-1, 4))
        ww = np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1, 4)); e = np.ascontiguousarray(np.asarray(empty, np.uint8).reshape(-1))
        n_pseudo, G = p.shape[0], len(e)
        out = np.full((len(d), G), np.float32(7.0), np.float32)             # (every word must be overwritten)
        self._chk(self._tap("afis_debug_fold_templates")(self.ctx, _ptr(p, C.c_float) if p.size else None, n_pseudo, G, _ptr(d, C.c_int32), len(d),
                                                         _ptr(ww, C.c_float) if ww.size else None, _ptr(e, C.c_uint8), _ptr(out, C.c_float)))
        return out

    # ---- case lists: the queries of one case fused into one list ----------------------------------------------------
    def _case_lists(self, fn, case_of, cap: int, subjects: bool):
        co = np.ascontiguousarray(np.asarray(case_of, np.int64).reshape(-1))
        n_cases = len(np.unique(co)); c = max(cap, 0)
        cid = np.empty(n_cases, np.int64); nh = np.empty(n_cases, np.int64); a = np.empty((n_cases, c), np.int64); sc = np.empty((n_cases, c), np.float32)
        self._chk(fn(_ptr(co, C.c_int64), len(co), n_cases, _ptr(cid, C.c_int64), _ptr(nh, C.c_int64), _ptr(a, C.c_int64), _ptr(sc, C.c_float)))
        return {"case_id": cid, "n_hits": nh, "subject" if subjects else "idx": a, "score": sc}

    def rank_case_hits(self, case_of: Sequence[int], mode: int, min_score: float, cap: int):
        """Of the LAST search, per CASE every template whose fused score reaches min_score.  case_of[i] (any int64 >= 0) is the case of query position i — all of a
        case's latents must be queries of that one search; the distinct ids in ascending order are the rows: case_id [n_cases], n_hits [n_cases] (it may exceed cap),
        idx / score [n_cases][cap] in rank-list order, padded with (-1, -inf).  mode CASE_SUM: the fp32 sum, in query order, of the members' scores that are >= 0 (-1 when
        there is none); CASE_MAX: the members' best score.  min_score = -inf gives a rank list of length cap."""
        return self._case_lists(lambda co, nq, nc, cid, nh, a, sc: self.lib.afis_rank_case_hits(self.ctx, co, nq, mode, nc, min_score, cap, cid, nh, a, sc), case_of, cap, False)

    def rank_case_subject_hits(self, handle, case_of: Sequence[int], mode: int, min_score: float, cap: int):
        """rank_case_hits over the enrolled persons of a subjects_create handle: a member's value is the subject's best score for that query; subject / score
        [n_cases][cap].  (Which template reached it is rank_subject_hits' to say, per latent, on the same matrix.)"""
        return self._case_lists(lambda co, nq, nc, cid, nh, a, sc: self.lib.afis_rank_case_subject_hits(self.ctx, handle[0], co, nq, mode, nc, min_score, cap, cid, nh, a, sc),
                                case_of, cap, True)

    def rank_case_hits_filtered(self, case_of: Sequence[int], mode: int, min_score: float, cap: int, labels=None, masks=None, excl=None):
        """rank_case_hits, every column folded over the members that are ELIGIBLE for it.  labels / masks / excl are rank_hits_filtered's, per QUERY position (a case-wide
        elimination list is that list repeated for each member).  A column no member of the case is eligible for is no entry: neither counted nor listed, whatever
        min_score is; one whose eligible members all hold -1 is CASE_SUM's -1, listed when min_score <= -1."""
        co = np.asarray(case_of, np.int64).reshape(-1)
        _, keep, f = self._filter(labels, masks, excl, len(co))
        return self._case_lists(lambda co, nq, nc, cid, nh, a, sc: self.lib.afis_rank_case_hits_filtered(self.ctx, *f, co, nq, mode, nc, min_score, cap, cid, nh, a, sc), co, cap, False)

    def rank_case_subject_hits_filtered(self, handle, case_of: Sequence[int], mode: int, min_score: float, cap: int, labels=None, masks=None, excl=None):
        """rank_case_subject_hits over the eligible members: a member's value is the person's best score among their covered templates that are eligible for that
        member; excl: per query a sequence of SUBJECT ids.  A person no member is eligible for is neither counted nor listed."""
        co = np.asarray(case_of, np.int64).reshape(-1)
        _, keep, f = self._filter(labels, masks, excl, len(co))
        return self._case_lists(lambda co, nq, nc, cid, nh, a, sc: self.lib.afis_rank_case_subject_hits_filtered(self.ctx, handle[0], *f, co, nq, mode, nc, min_score, cap, cid, nh, a, sc),
                                co, cap, True)

    # ---- reverse search: the last search's matrix ranked along its columns -----------------------------------------
    def _latent_lists(self, fn, n_templates: int, cap: int):
        c = max(cap, 0)
        nh = np.empty(n_templates, np.int64); li = np.empty((n_templates, c), np.int64); sc = np.empty((n_templates, c), np.float32)
        self._chk(fn(n_templates, _ptr(nh, C.c_int64), _ptr(li, C.c_int64), _ptr(sc, C.c_float)))
        return {"n_hits": nh, "latent": li, "score": sc}

    def rank_latent_hits(self, min_score: float, cap: int, latent_base: int = 0, n_templates: Optional[int] = None):
        """Of the LAST search, per template it covered (a subset's listed templates in the caller's order, or the resident shard's) every query whose score reaches
        min_score: n_hits [n] how many (it may exceed cap), latent / score [n][cap] the best min(n_hits, cap) of them — latent_base + the query's position, score
        descending, equal scores by ascending position — padded with (-1, -inf).  n_templates defaults to the columns of the last search call made through this object."""
        n = self.last_n_templates if n_templates is None else n_templates
        return self._latent_lists(lambda nt, nh, li, sc: self.lib.afis_rank_latent_hits(self.ctx, nt, min_score, cap, latent_base, nh, li, sc), n, cap)

    def rank_latent_hits_filtered(self, min_score: float, cap: int, latent_base: int = 0, labels=None, masks=None, excl=None, n_templates: Optional[int] = None,
                                  n_q: Optional[int] = None):
        """rank_latent_hits over the cells each query is eligible for: per covered template only the queries whose masks its label passes and that do not exclude it.
        labels / masks / excl are rank_hits_filtered's, per QUERY position of the last search (n_q defaults as there); a template no query is eligible for has
        n_hits 0 and all padding."""
        n = self.last_n_templates if n_templates is None else n_templates
        _, keep, f = self._filter(labels, masks, excl, n_q)
        return self._latent_lists(lambda nt, nh, li, sc: self.lib.afis_rank_latent_hits_filtered(self.ctx, *f, nt, min_score, cap, latent_base, nh, li, sc), n, cap)

    def rank_latents(self, k: int, latent_base: int = 0, n_templates: Optional[int] = None):
        """The k best latents of every template the last search covered: rank_latent_hits with min_score = -inf, without the counts."""
        r = self.rank_latent_hits(-np.inf, k, latent_base, n_templates)
        return {"latent": r["latent"], "score": r["score"]}

    def debug_rank_latent_hits(self, scores: np.ndarray, min_score: float, cap: int, latent_base: int = 0):
        """rank_latent_hits over a caller-made [n_q][G] score matrix for the resident shard (parity tap); the matrix stays rankable."""
        s = np.ascontiguousarray(scores, np.float32)
        self.last_n_q = s.shape[0]; self.last_n_templates = s.shape[1]
        return self._latent_lists(lambda nt, nh, li, sc: self._tap("afis_debug_rank_latent_hits")(self.ctx, _ptr(s, C.c_float), s.shape[0], min_score, cap, latent_base, nh, li, sc),
                                  s.shape[1], cap)

    def transpose_stats(self):
        """(device microseconds, bytes read and written) of the transpose of the last rank_latent_hits (parity tap)."""
        out = (C.c_longlong * 2)()
        self._chk(self._tap("afis_debug_transpose_stats")(self.ctx, out))
        return int(out[0]), int(out[1])

    def reverse_search(self, qhandle, templates: Sequence[FPTemplate], min_score: float, cap: int, latent_base: int = 0):
        """One card of the reverse search: the rolled `templates` are appended to the resident shard (reopen, add, commit with the shard's index_base), and the latents
        of `qhandle` — upload_queries(..., reserve=N) with N >= len(templates) — are searched against them alone.  -> (the new templates' global indices, the
        rank_latent_hits lists with one row per new template)."""
        first = self.index_base + self.resident_size
        self.gallery_reopen()
        self.gallery_add(templates)
        self.gallery_commit(self.index_base)
        idx = np.arange(first, first + len(templates), dtype=np.int64)
        sub = self.subset_create(idx)
        try:
            self.search_subset_resident(sub, qhandle, k=0)
            lists = self.rank_latent_hits(min_score, cap, latent_base)
        finally:
            self.subset_free(sub)
        return idx, lists

    def correspondences(self, latent: FPTemplate, gallery_idx: Sequence[int]):
        """Surviving minutiae correspondences (matcher.cpp:497-505) of one latent against each listed gallery template:
        a list (one entry per gallery index) of three int16 arrays [n_s][4] = (lx, ly, rx, ry), one per selected template
        (None where the reference does not run that scorer)."""
        v = _Views([latent])
        n = len(gallery_idx)
        gi = np.asarray(gallery_idx, np.int64).reshape(-1)
        counts = np.zeros((max(n, 1), 3), np.int32); xy = np.zeros((max(n, 1), 3, 120, 4), np.int16)
        self._chk(self.lib.afis_correspondences(self.ctx, v.arr, _ptr(gi, C.c_int64) if n else None, n, _ptr(counts, C.c_int32), _ptr(xy, C.c_int16)))
        return [[xy[i, s, :counts[i, s]].copy() if counts[i, s] >= 0 else None for s in range(3)] for i in range(n)]

    def correspondences_pairs(self, qhandle, query, idx, want_parts: bool = False):
        """The surviving minutiae correspondences of a LIST of (latent, print) pairs in one launch sequence (afis_correspondences_pairs): pair i is (query[i], idx[i]),
        a query position of the upload_queries handle — of any gallery epoch — and a GLOBAL index of the resident shard; any order, repeats allowed; the flattened idx of
        rank_hits can be passed as it is.  -> {"counts": [n][3] int32, "xy": [n][3][120][4] int16 (rows beyond counts zero), "corr": per pair a list of three arrays
        [n_s][4] = (lx, ly, rx, ry) as correspondences() gives them — None where the reference does not run that scorer (counts -1), the marker NOT_COVERED where this
        shard does not hold idx[i] (counts -2, the -1 padding of the list calls included) —, "part": [n][3] float32 with want_parts, the scorer's return value
        (search()'s parts[q][t][s] bit for bit where counts >= 0, +0.0 elsewhere), else None}.  The last search's matrix stays rankable."""
        qa = np.ascontiguousarray(np.asarray(query, np.int32).reshape(-1)); ia = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        if len(qa) != len(ia):
            raise ValueError("correspondences_pairs: query and idx must have one length")
        n = len(qa)
        counts = np.zeros((max(n, 1), 3), np.int32); xy = np.zeros((max(n, 1), 3, 120, 4), np.int16)
        part = np.zeros((max(n, 1), 3), np.float32) if want_parts else None
        self._chk(self.lib.afis_correspondences_pairs(self.ctx, qhandle[0], n, _ptr(qa, C.c_int32) if n else None, _ptr(ia, C.c_int64) if n else None,
                                                      _ptr(counts, C.c_int32), _ptr(xy, C.c_int16), _ptr(part, C.c_float) if want_parts else None))
        corr = [[xy[i, s, :counts[i, s]].copy() if counts[i, s] >= 0 else (None if counts[i, s] == CORR_NOT_RUN else NOT_COVERED) for s in range(3)] for i in range(n)]
        return {"counts": counts[:n], "xy": xy[:n], "corr": corr, "part": part[:n] if want_parts else None}

    def score_pairs(self, qhandle, query, idx, want_parts: bool = False):
        """The fused scores of a LIST of (latent, print) pairs without a matrix (afis_score_pairs): pair i is (query[i], idx[i]), a query position of the upload_queries
        handle — of any gallery epoch — and a GLOBAL index of the resident shard; any order, repeats allowed; the flattened idx of rank_hits can be passed as it is.
        -> {"status": [n] int32 — PAIR_OK, or PAIR_NOT_COVERED where this shard does not hold idx[i] (the -1 padding of the list calls included) —, "score": [n] float32,
        search()'s scores[query[i]][idx[i] - index_base] bit for bit (-1 for an empty or removed print and a latent-empty query; -inf where not covered), "parts": [n][4]
        float32 with want_parts, search()'s parts of that cell bit for bit (+0.0 where not covered), else None}.  The last search's matrix stays rankable."""
        qa = np.ascontiguousarray(np.asarray(query, np.int32).reshape(-1)); ia = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        if len(qa) != len(ia):
            raise ValueError("score_pairs: query and idx must have one length")
        n = len(qa)
        status = np.zeros(max(n, 1), np.int32); score = np.zeros(max(n, 1), np.float32)
        parts = np.zeros((max(n, 1), 4), np.float32) if want_parts else None
        self._chk(self.lib.afis_score_pairs(self.ctx, qhandle[0], n, _ptr(qa, C.c_int32) if n else None, _ptr(ia, C.c_int64) if n else None,
                                            _ptr(status, C.c_int32), _ptr(score, C.c_float), _ptr(parts, C.c_float) if want_parts else None))
        return {"status": status[:n], "score": score[:n], "parts": parts[:n] if want_parts else None}

    # ---- print pairs: scores and correspondences of (resident print, resident print) pairs ---------------------------
    def score_print_pairs(self, a_idx, b_idx, w_minu, w_tex, want_parts: bool = False):
        """The weighted scores of a LIST of (query print, column print) pairs of the resident shard without a matrix (afis_score_print_pairs): pair i is (a_idx[i],
        b_idx[i]), both GLOBAL indices of the shard as it stands; any order, repeats allowed, (a, a) an ordinary pair; w_minu / w_tex one weight per pair (a scalar is
        every pair's).  -> {"status": [n] int32 — PAIR_OK, or PAIR_NOT_COVERED where this shard does not hold both prints (the -1 padding of the list calls included)
        —, "score": [n] float32, search_prints()' cell for query a, column b and the pair's weights bit for bit (-1 for an empty or removed b and where nothing of a is
        active; -inf where not covered), "parts": [n][2] float32 with want_parts — the minutiae and the texture entry of the print's view against b, +0.0 where not
        active —, else None}.  The last search's matrix stays rankable.  get_option("print_pairs_us"), get_option("print_pairs_query_prints")."""
        a = np.ascontiguousarray(np.asarray(a_idx, np.int64).reshape(-1)); b = np.ascontiguousarray(np.asarray(b_idx, np.int64).reshape(-1))
        if len(a) != len(b):
            raise ValueError("score_print_pairs: a_idx and b_idx must have one length")
        n = len(a)
        wm = np.ascontiguousarray(np.broadcast_to(np.asarray(w_minu, np.float32), (n,)))
        wt = np.ascontiguousarray(np.broadcast_to(np.asarray(w_tex, np.float32), (n,)))
        status = np.zeros(max(n, 1), np.int32); score = np.zeros(max(n, 1), np.float32)
        parts = np.zeros((max(n, 1), 2), np.float32) if want_parts else None
        self._chk(self.lib.afis_score_print_pairs(self.ctx, n, _ptr(a, C.c_int64) if n else None, _ptr(b, C.c_int64) if n else None,
                                                  _ptr(wm, C.c_float) if n else None, _ptr(wt, C.c_float) if n else None,
                                                  _ptr(status, C.c_int32), _ptr(score, C.c_float), _ptr(parts, C.c_float) if want_parts else None))
        return {"status": status[:n], "score": score[:n], "parts": parts[:n] if want_parts else None}

    def correspondences_print_pairs(self, a_idx, b_idx, want_parts: bool = False):
        """The surviving minutiae correspondences of a LIST of (query print, column print) pairs of the resident shard (afis_correspondences_print_pairs); the pairs as
        score_print_pairs'.  -> {"counts": [n] int32, "xy": [n][120][4] int16 = (a's x, a's y, b's x, b's y), rows beyond counts zero, "corr": per pair an array
        [n_s][4] — None where a or b holds no minutiae template (counts -1), the marker NOT_COVERED where this shard does not hold both prints (counts -2) —, "part":
        [n] float32 with want_parts, the scorer's return value (score_print_pairs' parts[i][0] bit for bit where counts >= 0, +0.0 elsewhere), else None}.  The last
        search's matrix stays rankable."""
        a = np.ascontiguousarray(np.asarray(a_idx, np.int64).reshape(-1)); b = np.ascontiguousarray(np.asarray(b_idx, np.int64).reshape(-1))
        if len(a) != len(b):
            raise ValueError("correspondences_print_pairs: a_idx and b_idx must have one length")
        n = len(a)
        counts = np.zeros(max(n, 1), np.int32); xy = np.zeros((max(n, 1), 120, 4), np.int16)
        part = np.zeros(max(n, 1), np.float32) if want_parts else None
        self._chk(self.lib.afis_correspondences_print_pairs(self.ctx, n, _ptr(a, C.c_int64) if n else None, _ptr(b, C.c_int64) if n else None,
                                                            _ptr(counts, C.c_int32), _ptr(xy, C.c_int16), _ptr(part, C.c_float) if want_parts else None))
        corr = [xy[i, :counts[i]].copy() if counts[i] >= 0 else (None if counts[i] == CORR_NOT_RUN else NOT_COVERED) for i in range(n)]
        return {"counts": counts[:n], "xy": xy[:n], "corr": corr, "part": part[:n] if want_parts else None}

    # ---- the evidence of the texture scorer, and where a latent lies on a print ---------------------------------------
    def _texture_export(self, call, head, n, want_parts):
        counts = np.zeros(max(n, 1), np.int32); xy = np.zeros((max(n, 1), TEX_CORR_MAX, 4), np.int16); pt = np.zeros((max(n, 1), TEX_CORR_MAX, 2), np.int16)
        sim = np.zeros((max(n, 1), TEX_CORR_MAX), np.float32); part = np.zeros(max(n, 1), np.float32) if want_parts else None
        self._chk(call(*head, _ptr(counts, C.c_int32), _ptr(xy, C.c_int16), _ptr(pt, C.c_int16), _ptr(sim, C.c_float), _ptr(part, C.c_float) if want_parts else None))
        corr = [xy[i, :counts[i]].copy() if counts[i] >= 0 else (None if counts[i] == CORR_NOT_RUN else NOT_COVERED) for i in range(n)]
        return {"counts": counts[:n], "xy": xy[:n], "pt": pt[:n], "sim": sim[:n], "corr": corr, "part": part[:n] if want_parts else None}

    def texture_correspondences_pairs(self, qhandle, query, idx, want_parts: bool = False):
        """The surviving correspondences of the TEXTURE scorer for a LIST of (latent, print) pairs (afis_texture_correspondences_pairs); the pairs as
        correspondences_pairs'.  -> {"counts": [n] int32 (-1: the reference does not call the scorer, -2: not covered), "xy": [n][200][4] int16 = (latent x, latent y,
        rolled x, rolled y) in BLOCK units, "pt": [n][200][2] int16 = (latent texture row, rolled texture point), "sim": [n][200] float32, all in the reference's list
        order with zeros beyond counts, "corr": per pair xy[:counts] — None / NOT_COVERED as correspondences_pairs' —, "part": [n] float32 with want_parts (search()'s
        parts[q][t][3] bit for bit where counts >= 0), else None}.  The last search's matrix stays rankable.  get_option("texture_correspondences_us")."""
        qa = np.ascontiguousarray(np.asarray(query, np.int32).reshape(-1)); ia = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        if len(qa) != len(ia):
            raise ValueError("texture_correspondences_pairs: query and idx must have one length")
        n = len(qa)
        return self._texture_export(self.lib.afis_texture_correspondences_pairs, (self.ctx, qhandle[0], n, _ptr(qa, C.c_int32) if n else None, _ptr(ia, C.c_int64) if n else None), n, want_parts)

    def texture_correspondences_print_pairs(self, a_idx, b_idx, want_parts: bool = False):
        """texture_correspondences_pairs for (query print, column print) pairs of the resident shard (afis_texture_correspondences_print_pairs); the pairs as
        score_print_pairs'; pt's first component indexes a's texture points.  "part" is score_print_pairs' parts[i][1] for a non-zero w_tex."""
        a = np.ascontiguousarray(np.asarray(a_idx, np.int64).reshape(-1)); b = np.ascontiguousarray(np.asarray(b_idx, np.int64).reshape(-1))
        if len(a) != len(b):
            raise ValueError("texture_correspondences_print_pairs: a_idx and b_idx must have one length")
        n = len(a)
        return self._texture_export(self.lib.afis_texture_correspondences_print_pairs, (self.ctx, n, _ptr(a, C.c_int64) if n else None, _ptr(b, C.c_int64) if n else None), n, want_parts)

    def pair_alignments(self, qhandle, query, idx):
        """The exact moments of every scorer's surviving correspondences for a LIST of (latent, print) pairs (afis_pair_alignments); the pairs as score_pairs'.
        -> {"status": [n] int32 (PAIR_OK / PAIR_NOT_COVERED), "moments": [n][4] CORR_MOMENTS — scorers 0, 1, 2 in pixels, the texture scorer at 16 b + 24; zeros where a
        scorer did not run or left nothing}.  alignment_fit() places the latent from a record, add_moments() pools records.  get_option("pair_alignments_us")."""
        qa = np.ascontiguousarray(np.asarray(query, np.int32).reshape(-1)); ia = np.ascontiguousarray(np.asarray(idx, np.int64).reshape(-1))
        if len(qa) != len(ia):
            raise ValueError("pair_alignments: query and idx must have one length")
        n = len(qa)
        status = np.zeros(max(n, 1), np.int32); mom = np.zeros((max(n, 1), 4), CORR_MOMENTS)
        self._chk(self.lib.afis_pair_alignments(self.ctx, qhandle[0], n, _ptr(qa, C.c_int32) if n else None, _ptr(ia, C.c_int64) if n else None, _ptr(status, C.c_int32), C.c_void_p(mom.ctypes.data)))
        return {"status": status[:n], "moments": mom[:n]}

    def print_pair_alignments(self, a_idx, b_idx):
        """pair_alignments for (query print, column print) pairs of the resident shard (afis_print_pair_alignments): "moments" is [n][2] — a's minutiae template, a's
        texture template — against b."""
        a = np.ascontiguousarray(np.asarray(a_idx, np.int64).reshape(-1)); b = np.ascontiguousarray(np.asarray(b_idx, np.int64).reshape(-1))
        if len(a) != len(b):
            raise ValueError("print_pair_alignments: a_idx and b_idx must have one length")
        n = len(a)
        status = np.zeros(max(n, 1), np.int32); mom = np.zeros((max(n, 1), 2), CORR_MOMENTS)
        self._chk(self.lib.afis_print_pair_alignments(self.ctx, n, _ptr(a, C.c_int64) if n else None, _ptr(b, C.c_int64) if n else None, _ptr(status, C.c_int32), C.c_void_p(mom.ctypes.data)))
        return {"status": status[:n], "moments": mom[:n]}

    def alignment_fit(self, moments):
        """The rigid placement r ~ R l + t, R = [[c, -s], [s, c]], of one CORR_MOMENTS record (afis_alignment_fit, host only) -> (c, s, tx, ty, rms) as floats, or None
        where the record fixes none (fewer than two points, or all points of one side coincide)."""
        return alignment_fit(self.lib, moments)

    def One2One_matching_all_templates(self, latent: FPTemplate):
        """matcher.cpp:339-374 against every gallery template: (query status, rolled status [G], scores [G][n_minu + n_tex])."""
        v = _Views([latent])
        G = self.resident_size; width = len(latent.minu) + len(latent.tex)
        scores = np.zeros((max(G, 1), max(width, 1)), np.float32); rs = np.zeros(max(G, 1), np.int32); qs = C.c_int32(0)
        self._chk(self.lib.afis_match_all_templates(self.ctx, v.arr, _ptr(scores, C.c_float), _ptr(rs, C.c_int32), C.byref(qs)))
        return qs.value, rs[:G], scores[:G, :width] if width else np.zeros((G, 0), np.float32)

    def pq_encode(self, des: np.ndarray) -> np.ndarray:
        """TrainedPQEncoder.encode_multi (descriptor_PQ.py:19-27) on the device: [n][96] fp32 -> [n][16] u8."""
        des = np.ascontiguousarray(des, np.float32).reshape(-1, 96)
        codes = np.zeros((des.shape[0], 16), np.uint8)
        self._chk(self.lib.afis_pq_encode(self.ctx, _ptr(des, C.c_float), des.shape[0], _ptr(codes, C.c_uint8)))
        return codes

    def encode_rolled_dat(self, buf: bytes):
        """A template with fp32 texture descriptors (latent layout) -> (reader rc, the rolled-layout file with PQ codes)."""
        need = C.c_size_t(0); rc = C.c_int32(0)
        self._chk(self.lib.afis_encode_rolled_dat(self.ctx, buf, len(buf), None, 0, C.byref(need), C.byref(rc)))
        out = C.create_string_buffer(max(1, need.value))
        self._chk(self.lib.afis_encode_rolled_dat(self.ctx, buf, len(buf), out, need.value, C.byref(need), C.byref(rc)))
        return rc.value, out.raw[:need.value]

    def free_queries(self, handle):
        self.lib.afis_queries_free(self.ctx, handle[0])

    def timing(self) -> dict:
        t = Timing()
        if hasattr(self.lib, "afis_get_timing2"):
            self._chk(self.lib.afis_get_timing2(self.ctx, C.byref(t), C.sizeof(Timing)))
        else:
            self._chk(self.lib.afis_get_timing(self.ctx, C.byref(t)))
        return {n: getattr(t, n) for n, _ in Timing._fields_ if n != "reserved_"}

    def _tap(self, name: str):
        if not hasattr(self.lib, name):
            raise AfisError(f"{name} is a parity tap: construct Matcher(..., taps=True) (libafis_hip_test.so); the product library does not export it")
        return getattr(self.lib, name)

    def phase_cycles(self, reset: bool = True):
        out = (C.c_uint64 * 32)()
        self._chk(self._tap("afis_debug_phase_cycles")(self.ctx, out, 1 if reset else 0))
        return list(out)

    # ---- parity taps ------------------------------------------------------------------------------------------
    def debug_atan2_grid(self, R: int) -> np.ndarray:
        out = np.empty((2 * R + 1, 2 * R + 1), np.float32)
        self._chk(self._tap("afis_debug_atan2_grid")(self.ctx, R, _ptr(out, C.c_float)))
        return out

    def debug_graph_arith(self) -> list:
        out = (C.c_ulonglong * 8)()
        self._chk(self._tap("afis_debug_graph_arith")(self.ctx, out))
        return list(out)

    def refine_stats(self, reset: bool = True) -> dict:
        """adc_variant 9 with set_option("mf_stats", 1): what the selection / recomputation kernel did since the last reset."""
        out = (C.c_ulonglong * 8)()
        self._chk(self._tap("afis_debug_refine_stats")(self.ctx, out, 1 if reset else 0))
        return dict(zip(("pairs", "rows", "rows_evaluated", "cells_evaluated", "rows_evaluated_in_full", "bound_violations"), list(out)[:6]))

    def compact_stats(self):
        """(device microseconds, bytes copied) of the compaction kernels of the last gallery_remove, or of the splice kernels of the last gallery_commit_at, whichever came last."""
        out = (C.c_longlong * 2)()
        self._chk(self._tap("afis_debug_compact_stats")(self.ctx, out))
        return int(out[0]), int(out[1])

    def debug_stage_list(self, latent: FPTemplate, g: int, which: int, stage: int):
        """(sim, li, ri) of the scorer's correspondence list after a stage (None when the scorer is not run)."""
        v = _Views([latent])
        sim = np.zeros(200, np.float32); li = np.zeros(200, np.int32); ri = np.zeros(200, np.int32); n = C.c_int32(0)
        self._chk(self._tap("afis_debug_stage_list")(self.ctx, v.arr, g, which, stage, _ptr(sim, C.c_float), _ptr(li, C.c_int32), _ptr(ri, C.c_int32), C.byref(n)))
        if n.value < 0:
            return None
        return sim[:n.value], li[:n.value], ri[:n.value]

    def debug_lut(self, latent: FPTemplate) -> np.ndarray:
        v = _Views([latent])
        n = latent.tex[0].n if latent.tex else 0
        out = np.empty((max(n, 1), 16, 256), np.float32); nr = C.c_int32(0)
        self._chk(self._tap("afis_debug_lut")(self.ctx, v.arr, _ptr(out, C.c_float), C.byref(nr)))
        return out[:nr.value]

    def debug_texture_rowmax(self, latent: FPTemplate, g: int):
        v = _Views([latent])
        val = np.zeros(1000, np.float32); arg = np.zeros(1000, np.int32); nr = C.c_int32(0)
        self._chk(self._tap("afis_debug_texture_rowmax")(self.ctx, v.arr, g, _ptr(val, C.c_float), _ptr(arg, C.c_int32), C.byref(nr)))
        return val[:nr.value], arg[:nr.value]

    # ---- the reference's drivers (matching/matcher.cpp:96-337) ---------------------------------------------------
    def load_gallery_dir(self, rolled_path: str) -> List[str]:
        """Directory scan for *.dat as One2List/List2List do (matcher.cpp:120-130, directory order)."""
        if os.path.isfile(rolled_path):                   # a packed gallery container instead of a directory
            self.gallery_load(rolled_path)
            self.gallery_files = self.gallery_file_names(rolled_path)
            self.gallery_commit(0)
            return self.gallery_files
        files = [os.path.join(rolled_path, f) for f in os.listdir(rolled_path) if os.path.splitext(f)[1] == ".dat"]
        for f in files:
            with open(f, "rb") as fh:
                self.gallery_add_dat(fh.read())
        self.gallery_files = files
        self.gallery_commit(0)
        return files

    def One2List_matching(self, latent_template_file: str, score_path: str, top: int = 24) -> int:
        """matcher.cpp:216-337: rank list of the top 24 as `<rank>"<path>",<score>` under a `filename,score` header."""
        with open(latent_template_file, "rb") as f:
            buf = f.read()
        stem = os.path.splitext(os.path.basename(latent_template_file))[0]
        _, parsed = read_latent(buf)
        if not parsed.minu and not parsed.tex:                # matcher.cpp:260-268: a latent without any template gets a score file holding `0`
            with open(score_path + stem + ".csv", "w") as out:
                out.write("0\n")
        r = self.search_dat([buf], k=min(top, max(1, self.gallery_size)))
        if r["status"][0] == 1:
            return 1
        k = min(top, self.gallery_size)
        idx = [int(r["topk_idx"][0, j]) for j in range(k)]; top_sc = [r["topk_score"][0, j] for j in range(k)]
        if self.get_option("ref_tie_order") >= 1:             # the reference binary's own order of equal scores (std::sort on the score column), as `match -l -tie`
            ri, rs = self.rank_list(r["scores"][0], k, ref_order=True)
            idx = [int(g) for g in ri]; top_sc = list(rs)
        with open(score_path + stem + ".csv", "w") as out:
            out.write("filename,score\n")
            for j, g in enumerate(idx):
                out.write(f'{j + 1}"{self.gallery_files[g]}",{_cxx_float(top_sc[j])}\n')
        # correspondence files of the ranked templates (matcher.cpp:311-328, :497-505); the reference's hard-coded
        # /LatentAFIS/scores/ prefix becomes the score directory, as in the `match` CLI
        _, latent = read_latent(buf)
        for g, lists in zip(idx, self.correspondences(latent, idx)):
            rstem = os.path.splitext(os.path.basename(self.gallery_files[g]))[0]
            for i, xy in enumerate(lists):
                if xy is None:
                    continue
                with open(f"{score_path}corr{stem}_{rstem}_{i}.csv", "w") as cf:
                    for lx, ly, rx, ry in xy:
                        cf.write(f"{lx},{ly},{rx},{ry}\n")
        return 0

    def List2List_matching(self, latent_path: str, score_path: str) -> int:
        """matcher.cpp:96-214: one CSV per latent, one `"path",%.3f` line per gallery file."""
        files = [os.path.join(latent_path, f) for f in os.listdir(latent_path) if os.path.splitext(f)[1] == ".dat"]
        if not files:
            return -1
        bufs = [open(f, "rb").read() for f in files]
        r = self.search_dat(bufs, k=0)
        for i, f in enumerate(files):
            stem = os.path.splitext(os.path.basename(f))[0]
            _, parsed = read_latent(bufs[i])
            if not parsed.minu and not parsed.tex:            # matcher.cpp:153-163: `0` and on to the next latent
                with open(score_path + stem + ".csv", "w") as out:
                    out.write("0\n")
                continue
            if r["status"][i] == 1:
                continue
            with open(score_path + stem + ".csv", "w") as out:
                for j, gf in enumerate(self.gallery_files):
                    out.write(f'"{gf}",{r["scores"][i, j]:.3f}\n')
        return 0


def _cxx_float(v: float) -> str:
    """`ostream << float` with default formatting (6 significant digits, %g style)."""
    return "%g" % float(v)
