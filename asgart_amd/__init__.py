"""asgart_amd -- host-side mirror of ASGART's search-core interface over libasgart_hip.so.

The product is the HIP library (asgart_amd/csrc -> asgart_amd/libasgart_hip.so, C ABI in
include/asgart_hip.h).  This module only binds it with ctypes and mirrors the names of the
reference's operator interface for the path (reference src/bin/asgart.rs:28-31,114-259,
src/searcher.rs:94-180, src/structs.rs:36-58,418-429):

    RunSettings, ProtoSD, Strand, Searcher (new / search), SearchDuplications (Step.run)

There is no CPU fallback: importing works without a GPU (so the symbol table can be
checked), but every compute entry point raises AsgartError when the library or a gfx950
device is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

__all__ = [
    "AsgartError", "RunSettings", "ProtoSD", "Strand", "Index", "Searcher", "SearchDuplications",
    "load_library", "library_path", "ABI_SYMBOLS", "sa_build64", "search_duplications_multi", "merge_shards",
    "score_owners", "score_costs", "compute_scores_multi", "Source", "compute_scores_flags_multi", "orientation_flags",
    "export_records", "export_geometry", "f32_shortest", "f32_pow10_table", "EXPORT_FORMATS",
    "ResultScan", "result_geometry", "E_REFUSED", "Alignments", "align_geometry", "align_bytes", "align_bytes_banded",
    "paf_records", "paf_geometry", "paf_records_cs", "paf_cs_geometry", "CS_MODES",
    "AlignCounts", "alignment_stats_geometry", "sdtable_records", "sdtable_geometry",
    "Variants", "Sites", "SiteArrays", "VARIANT_DTYPE", "SITE_CLASSES", "variants_geometry", "sites_geometry",
    "variants_records_geometry", "sites_records_geometry",
]

_HERE = os.path.dirname(os.path.abspath(__file__))

ABI_SYMBOLS = (
    "asgart_sa_build64", "asgart_index_create", "asgart_index_destroy", "asgart_index_prepare",
    "asgart_search_duplications", "asgart_search_duplications_shard", "asgart_families_counts",
    "asgart_families_copy", "asgart_families_free", "asgart_searcher_cache_get",
    "asgart_searcher_search", "asgart_sa_read", "asgart_probe_hits", "asgart_get_stats",
    "asgart_last_error", "asgart_version", "asgart_compute_scores", "asgart_index_set_option",
    "asgart_index_check_sa", "asgart_index_create_trim", "asgart_index_clone",
    "asgart_search_duplications_multi", "asgart_search_duplications_ex", "asgart_search_duplications_passes",
    "asgart_search_duplications_passes_shard", "asgart_families_keys",
    "asgart_index_export", "asgart_index_create_device", "asgart_trim_cache", "asgart_post_process",
    "asgart_debug_dump_stacks", "asgart_prepare_data", "asgart_score_owners", "asgart_score_costs",
    "asgart_compute_scores_shard", "asgart_compute_scores_multi", "asgart_tier_plan",
    "asgart_source_create", "asgart_source_destroy", "asgart_extract_sequences",
    "asgart_compute_scores_flags", "asgart_compute_scores_flags_shard", "asgart_compute_scores_flags_multi",
    "asgart_fasta_read", "asgart_fasta_counts", "asgart_fasta_copy", "asgart_fasta_read_text", "asgart_fasta_index",
    "asgart_fasta_source", "asgart_fasta_free", "asgart_fasta_timings", "asgart_fasta_geometry",
    "asgart_index_set_tail_up", "asgart_tier_segments", "asgart_tier_profile",
    "asgart_fill_counts", "asgart_fill_tally", "asgart_ranked_fill_takes", "asgart_hit_rule",
    "asgart_join_cuts", "asgart_split_warm_next",
    "asgart_run_dir_info", "asgart_lookup_account", "asgart_run_dir_rule",
    "asgart_slice_families", "asgart_slice_counts", "asgart_slice_copy", "asgart_slice_timings", "asgart_slice_free",
    "asgart_plot_filter", "asgart_plot_counts", "asgart_plot_copy", "asgart_plot_timings", "asgart_plot_free",
    "asgart_plot_geometry",
    "asgart_rosary_clusters", "asgart_rosary_counts", "asgart_rosary_copy", "asgart_rosary_timings", "asgart_rosary_free",
    "asgart_rosary_geometry",
    "asgart_duplication_groups", "asgart_groups_counts", "asgart_groups_copy", "asgart_groups_timings", "asgart_groups_free",
    "asgart_groups_geometry",
    "asgart_chain_duplications", "asgart_chains_counts", "asgart_chains_copy", "asgart_chains_timings", "asgart_chains_free",
    "asgart_chain_geometry",
    "asgart_export_records", "asgart_export_size", "asgart_export_copy", "asgart_export_timings", "asgart_export_free",
    "asgart_export_geometry", "asgart_f32_shortest", "asgart_f32_pow10_table",
    "asgart_result_scan", "asgart_result_parse", "asgart_result_counts", "asgart_result_copy", "asgart_result_timings",
    "asgart_result_free", "asgart_result_geometry",
    "asgart_align_duplications", "asgart_alignment_counts", "asgart_alignment_copy", "asgart_alignment_timings",
    "asgart_alignment_free", "asgart_align_geometry", "asgart_align_bytes",
    "asgart_align_duplications_banded", "asgart_alignment_rounds", "asgart_align_bytes_banded",
    "asgart_paf_records", "asgart_paf_geometry", "asgart_paf_records_cs", "asgart_paf_cs_geometry",
    "asgart_index_read_text",
    "asgart_alignment_stats", "asgart_alignment_stats_geometry", "asgart_sdtable_records", "asgart_sdtable_geometry",
    "asgart_mask_intervals", "asgart_mask_counts", "asgart_mask_copy", "asgart_mask_timings", "asgart_mask_free",
    "asgart_mask_geometry", "asgart_fasta_write", "asgart_fasta_write_geometry",
    "asgart_alignment_variants", "asgart_variants_counts", "asgart_variants_copy", "asgart_variants_timings",
    "asgart_variants_free", "asgart_variants_geometry",
    "asgart_variant_sites", "asgart_sites_counts", "asgart_sites_copy", "asgart_sites_timings", "asgart_sites_free",
    "asgart_sites_geometry",
    "asgart_variants_records", "asgart_sites_records", "asgart_variants_records_geometry", "asgart_sites_records_geometry",
)


def merge_shards(parts) -> Tuple[np.ndarray, np.ndarray]:
    """(fam_offsets, sds, keys) of every shard of one call -> (fam_offsets, sds) of the whole call: families ordered
    by key (segment start probe, family ordinal) == reference order.  What rank 0 does after the gather."""
    keys = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, np.uint64)
    if len(keys) == 0:
        return np.zeros(1, np.uint64), np.zeros((0, 4), np.uint64)
    starts = np.concatenate([p[0][:-1].astype(np.int64) + b for p, b in
                             zip(parts, np.cumsum([0] + [len(p[1]) for p in parts[:-1]]))])
    lens = np.concatenate([np.diff(p[0].astype(np.int64)) for p in parts])
    sds = np.concatenate([p[1] for p in parts])
    order = np.argsort(keys, kind="stable")
    lens_o, starts_o = lens[order], starts[order]
    offs = np.concatenate([[0], np.cumsum(lens_o)]).astype(np.uint64)
    idx = np.repeat(starts_o - offs[:-1].astype(np.int64), lens_o) + np.arange(int(offs[-1]), dtype=np.int64)
    return offs, sds[idx]


class AsgartError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libasgart_hip error {code}: {msg}")
        self.code = code


def library_path() -> str:
    # ASGART_LIB selects a diagnostic build of the same library (profiling counters)
    return os.environ.get("ASGART_LIB") or os.path.join(_HERE, "libasgart_hip.so")


class _Settings(C.Structure):
    _fields_ = [
        ("probe_size", C.c_uint64),
        ("max_gap_size", C.c_uint32),
        ("min_duplication_length", C.c_uint64),
        ("max_cardinality", C.c_uint64),
        ("reverse", C.c_uint8),
        ("complement", C.c_uint8),
    ]


class Stats(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_search", C.c_double), ("ms_scan", C.c_double),
                ("ms_fill", C.c_double), ("ms_extend", C.c_double)] + [
        (n, C.c_uint64) for n in (
            "probes_total", "probes_n_skipped", "probes_searched", "probes_card_skipped",
            "probes_with_hits", "raw_hits", "filtered_hits", "segments", "families", "proto_sds",
            "bisect_steps", "search_launches", "overflow_segments")] + [("ms_extend_tier2", C.c_double), ("heavy_segments", C.c_uint64), ("ms_probe_count", C.c_double),
        ("search_bytes", C.c_uint64), ("probes_filter_rejected", C.c_uint64), ("search_bytes_wide_loads", C.c_uint64),
        ("ms_longest_tier", C.c_double), ("passes", C.c_uint64), ("ms_longest_segment", C.c_double),
        ("split_segments", C.c_uint64), ("split_refused", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    """dlopen libasgart_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise AsgartError(-3, f"{path} not built: run `python -c 'import __graft_entry__ as g; "
                              f"g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(path)
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    L.asgart_sa_build64.argtypes = [vp, vp, C.c_int64]
    L.asgart_sa_build64.restype = C.c_int32
    L.asgart_index_create.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int32, C.POINTER(vp)]
    L.asgart_index_create.restype = C.c_int32
    L.asgart_index_create_trim.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                           C.POINTER(vp)]
    L.asgart_index_create_trim.restype = C.c_int32
    L.asgart_index_clone.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.asgart_index_clone.restype = C.c_int32
    L.asgart_index_export.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int32)]
    L.asgart_index_export.restype = C.c_int32
    L.asgart_index_create_device.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.asgart_index_create_device.restype = C.c_int32
    L.asgart_trim_cache.argtypes = [C.c_int32]
    L.asgart_trim_cache.restype = C.c_int64
    L.asgart_prepare_data.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, vp, vp, C.c_int64, C.POINTER(C.c_int64),
                                      C.POINTER(vp)]
    L.asgart_prepare_data.restype = C.c_int32
    L.asgart_source_create.argtypes = [vp, vp, C.c_int64, C.c_int32, C.POINTER(vp)]
    L.asgart_source_create.restype = C.c_int32
    L.asgart_source_destroy.argtypes = [vp]
    L.asgart_source_destroy.restype = None
    L.asgart_extract_sequences.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, vp, C.c_uint64, vp, C.POINTER(C.c_int64)]
    L.asgart_extract_sequences.restype = C.c_int32
    L.asgart_fasta_read.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.asgart_fasta_read.restype = C.c_int32
    L.asgart_fasta_counts.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), u64p]
    L.asgart_fasta_counts.restype = C.c_int32
    L.asgart_fasta_copy.argtypes = [vp, vp, vp, vp]
    L.asgart_fasta_copy.restype = C.c_int32
    L.asgart_fasta_read_text.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.asgart_fasta_read_text.restype = C.c_int32
    L.asgart_fasta_index.argtypes = [vp, C.POINTER(vp)]
    L.asgart_fasta_index.restype = C.c_int32
    L.asgart_fasta_source.argtypes = [vp, C.POINTER(vp)]
    L.asgart_fasta_source.restype = C.c_int32
    L.asgart_fasta_free.argtypes = [vp]
    L.asgart_fasta_free.restype = None
    L.asgart_fasta_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.asgart_fasta_timings.restype = C.c_int32
    L.asgart_fasta_geometry.argtypes = [u64p, u64p, u64p]
    L.asgart_fasta_geometry.restype = None
    L.asgart_debug_dump_stacks.argtypes = []
    L.asgart_debug_dump_stacks.restype = C.c_int32
    L.asgart_post_process.argtypes = [vp, vp, C.c_uint64, vp, C.c_int32, C.POINTER(vp)]
    L.asgart_post_process.restype = C.c_int32
    L.asgart_search_duplications_multi.argtypes = [C.POINTER(vp), C.c_int32, vp, C.c_int64, C.POINTER(_Settings), vp,
                                                   C.POINTER(vp)]
    L.asgart_search_duplications_multi.restype = C.c_int32
    L.asgart_index_destroy.argtypes = [vp]
    L.asgart_index_destroy.restype = None
    L.asgart_index_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.asgart_index_set_option.restype = C.c_int32
    L.asgart_index_check_sa.argtypes = [vp]
    L.asgart_index_check_sa.restype = C.c_int64
    L.asgart_index_prepare.argtypes = [vp, C.c_uint64]
    L.asgart_index_prepare.restype = C.c_int32
    L.asgart_search_duplications.argtypes = [vp, vp, C.c_int64, C.POINTER(_Settings), vp,
                                             C.POINTER(vp)]
    L.asgart_search_duplications.restype = C.c_int32
    L.asgart_search_duplications_shard.argtypes = [vp, vp, C.c_int64, C.POINTER(_Settings),
                                                   C.c_int32, C.c_int32, C.POINTER(vp)]
    L.asgart_search_duplications_shard.restype = C.c_int32
    L.asgart_search_duplications_ex.argtypes = [vp, vp, C.c_int64, C.POINTER(_Settings), C.c_int32, C.c_int32, vp,
                                                C.POINTER(vp)]
    L.asgart_search_duplications_ex.restype = C.c_int32
    L.asgart_search_duplications_passes.argtypes = [vp, vp, C.c_int64, C.POINTER(_Settings), C.c_int32, C.POINTER(vp)]
    L.asgart_search_duplications_passes.restype = C.c_int32
    L.asgart_families_keys.argtypes = [vp, vp]
    L.asgart_families_keys.restype = None
    L.asgart_search_duplications_passes_shard.argtypes = [vp, vp, C.c_int64, C.POINTER(_Settings), C.c_int32, C.c_int32,
                                                          C.c_int32, C.POINTER(vp)]
    L.asgart_search_duplications_passes_shard.restype = C.c_int32
    L.asgart_families_counts.argtypes = [vp, u64p, u64p]
    L.asgart_families_counts.restype = None
    L.asgart_families_copy.argtypes = [vp, vp, vp]
    L.asgart_families_copy.restype = None
    L.asgart_families_free.argtypes = [vp]
    L.asgart_families_free.restype = None
    L.asgart_searcher_cache_get.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.asgart_searcher_cache_get.restype = C.c_int32
    L.asgart_searcher_search.argtypes = [vp, vp, C.c_int64, C.c_uint64, vp, vp]
    L.asgart_searcher_search.restype = C.c_int32
    L.asgart_sa_read.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.asgart_sa_read.restype = C.c_int32
    L.asgart_compute_scores.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, vp]
    L.asgart_compute_scores.restype = C.c_int32
    L.asgart_score_owners.argtypes = [vp, C.c_int64, C.c_int32, vp]
    L.asgart_score_owners.restype = C.c_int32
    L.asgart_score_costs.argtypes = [vp, C.c_int64, vp]
    L.asgart_score_costs.restype = C.c_int32
    L.asgart_tier_plan.argtypes = [C.c_int32, vp, C.c_int64, vp, C.c_double, vp, vp]
    L.asgart_tier_plan.restype = C.c_int32
    L.asgart_compute_scores_shard.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
    L.asgart_compute_scores_shard.restype = C.c_int64
    L.asgart_compute_scores_multi.argtypes = [C.POINTER(vp), C.c_int32, vp, C.c_int64, C.c_int32, C.c_int32, vp]
    L.asgart_compute_scores_multi.restype = C.c_int32
    L.asgart_compute_scores_flags.argtypes = [vp, vp, vp, C.c_int64, vp]
    L.asgart_compute_scores_flags.restype = C.c_int32
    L.asgart_compute_scores_flags_shard.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp]
    L.asgart_compute_scores_flags_shard.restype = C.c_int64
    L.asgart_compute_scores_flags_multi.argtypes = [C.POINTER(vp), C.c_int32, vp, vp, C.c_int64, vp]
    L.asgart_compute_scores_flags_multi.restype = C.c_int32
    L.asgart_probe_hits.argtypes = [vp, vp, C.c_int64, C.POINTER(_Settings), vp, vp, vp, u64p]
    L.asgart_probe_hits.restype = C.c_int64
    L.asgart_get_stats.argtypes = [vp, C.c_uint32, C.POINTER(Stats)]
    L.asgart_get_stats.restype = C.c_int32
    if hasattr(L, "asgart_tier_segments"):   # (ASGART_LIB may name an older build of the library: benchmarks against a parent)
        L.asgart_index_set_tail_up.argtypes = [vp, C.c_int32, C.c_int64]
        L.asgart_index_set_tail_up.restype = C.c_int32
        L.asgart_tier_segments.argtypes = [vp, vp]
        L.asgart_tier_segments.restype = C.c_int32
        L.asgart_tier_profile.argtypes = [vp, vp]
        L.asgart_tier_profile.restype = C.c_int32
    if hasattr(L, "asgart_join_cuts"):
        L.asgart_join_cuts.argtypes = [C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
        L.asgart_join_cuts.restype = C.c_int32
        L.asgart_split_warm_next.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
        L.asgart_split_warm_next.restype = C.c_uint32
    if hasattr(L, "asgart_fill_counts"):
        L.asgart_fill_counts.argtypes = [vp, vp]
        L.asgart_fill_counts.restype = C.c_int32
        L.asgart_fill_tally.argtypes = [vp, vp]
        L.asgart_fill_tally.restype = C.c_int32
        L.asgart_ranked_fill_takes.argtypes = [C.c_uint64, C.c_uint64, C.c_int32]
        L.asgart_ranked_fill_takes.restype = C.c_int32
    if hasattr(L, "asgart_hit_rule"):
        L.asgart_hit_rule.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]
        L.asgart_hit_rule.restype = None
    if hasattr(L, "asgart_run_dir_info"):
        L.asgart_run_dir_info.argtypes = [vp, vp]
        L.asgart_run_dir_info.restype = C.c_int32
        L.asgart_lookup_account.argtypes = [vp, vp]
        L.asgart_lookup_account.restype = C.c_int32
        L.asgart_run_dir_rule.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        L.asgart_run_dir_rule.restype = None
    if hasattr(L, "asgart_slice_families"):
        L.asgart_slice_families.argtypes = [C.c_int32, vp, C.c_int64, vp, vp, vp, vp, C.c_int64, vp, vp, C.POINTER(vp)]
        L.asgart_slice_families.restype = C.c_int32
        L.asgart_slice_counts.argtypes = [vp, u64p, u64p]
        L.asgart_slice_counts.restype = None
        L.asgart_slice_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.asgart_slice_copy.restype = None
        L.asgart_slice_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_slice_timings.restype = C.c_int32
        L.asgart_slice_free.argtypes = [vp]
        L.asgart_slice_free.restype = None
    if hasattr(L, "asgart_plot_filter"):
        L.asgart_plot_filter.argtypes = [C.c_int32, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, C.c_int64,
                                         vp, C.POINTER(C.c_int64), C.POINTER(vp)]
        L.asgart_plot_filter.restype = C.c_int32
        L.asgart_plot_counts.argtypes = [vp, u64p, u64p, u64p]
        L.asgart_plot_counts.restype = None
        L.asgart_plot_copy.argtypes = [vp, vp, vp, vp]
        L.asgart_plot_copy.restype = None
        L.asgart_plot_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_plot_timings.restype = C.c_int32
        L.asgart_plot_free.argtypes = [vp]
        L.asgart_plot_free.restype = None
        L.asgart_plot_geometry.argtypes = [u64p, u64p]
        L.asgart_plot_geometry.restype = None
    if hasattr(L, "asgart_rosary_clusters"):
        L.asgart_rosary_clusters.argtypes = [C.c_int32, vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_uint64, C.POINTER(vp)]
        L.asgart_rosary_clusters.restype = C.c_int32
        L.asgart_rosary_counts.argtypes = [vp, u64p, u64p]
        L.asgart_rosary_counts.restype = None
        L.asgart_rosary_copy.argtypes = [vp, vp, vp, vp, vp, vp]
        L.asgart_rosary_copy.restype = None
        L.asgart_rosary_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_rosary_timings.restype = C.c_int32
        L.asgart_rosary_free.argtypes = [vp]
        L.asgart_rosary_free.restype = None
        L.asgart_rosary_geometry.argtypes = [u64p]
        L.asgart_rosary_geometry.restype = None
    if hasattr(L, "asgart_duplication_groups"):
        L.asgart_duplication_groups.argtypes = [C.c_int32, vp, vp, vp, C.c_int64, C.c_int64, C.c_uint64, C.POINTER(vp)]
        L.asgart_duplication_groups.restype = C.c_int32
        L.asgart_groups_counts.argtypes = [vp, u64p, u64p, u64p]
        L.asgart_groups_counts.restype = None
        L.asgart_groups_copy.argtypes = [vp] * 14
        L.asgart_groups_copy.restype = None
        L.asgart_groups_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_groups_timings.restype = C.c_int32
        L.asgart_groups_free.argtypes = [vp]
        L.asgart_groups_free.restype = None
        L.asgart_groups_geometry.argtypes = [u64p]
        L.asgart_groups_geometry.restype = None
    if hasattr(L, "asgart_chain_duplications"):
        L.asgart_chain_duplications.argtypes = [C.c_int32, vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_uint64, C.c_int32,
                                                C.POINTER(vp)]
        L.asgart_chain_duplications.restype = C.c_int32
        L.asgart_chains_counts.argtypes = [vp, u64p, u64p, u64p, u64p]
        L.asgart_chains_counts.restype = None
        L.asgart_chains_copy.argtypes = [vp] * 8
        L.asgart_chains_copy.restype = None
        L.asgart_chains_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_chains_timings.restype = C.c_int32
        L.asgart_chains_free.argtypes = [vp]
        L.asgart_chains_free.restype = None
        L.asgart_chain_geometry.argtypes = [u64p, u64p, u64p]
        L.asgart_chain_geometry.restype = None
    if hasattr(L, "asgart_export_records"):
        L.asgart_export_records.argtypes = [C.c_int32, C.c_int32, vp, C.c_int64, vp, vp, vp, vp, vp, C.c_int64, vp, vp,
                                            C.c_int64, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(vp)]
        L.asgart_export_records.restype = C.c_int32
        L.asgart_export_size.argtypes = [vp]
        L.asgart_export_size.restype = C.c_uint64
        L.asgart_export_copy.argtypes = [vp, vp, C.c_uint64]
        L.asgart_export_copy.restype = C.c_int32
        L.asgart_export_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_export_timings.restype = C.c_int32
        L.asgart_export_free.argtypes = [vp]
        L.asgart_export_free.restype = None
        L.asgart_export_geometry.argtypes = [u64p, u64p, u64p]
        L.asgart_export_geometry.restype = None
        L.asgart_f32_shortest.argtypes = [C.c_int32, vp, C.c_int64, C.c_int32, vp, vp]
        L.asgart_f32_shortest.restype = C.c_int32
        L.asgart_f32_pow10_table.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
        L.asgart_f32_pow10_table.restype = C.c_int32
    if hasattr(L, "asgart_result_scan"):
        L.asgart_result_scan.argtypes = [C.c_int32, vp, C.c_uint64, C.POINTER(vp), u64p, u64p]
        L.asgart_result_scan.restype = C.c_int32
        L.asgart_result_parse.argtypes = [vp, vp, vp, C.c_int64]
        L.asgart_result_parse.restype = C.c_int32
        L.asgart_result_counts.argtypes = [vp, u64p, u64p, u64p, u64p]
        L.asgart_result_counts.restype = None
        L.asgart_result_copy.argtypes = [vp] * 10
        L.asgart_result_copy.restype = C.c_int32
        L.asgart_result_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_result_timings.restype = C.c_int32
        L.asgart_result_free.argtypes = [vp]
        L.asgart_result_free.restype = None
        L.asgart_result_geometry.argtypes = [u64p, u64p, u64p]
        L.asgart_result_geometry.restype = None
    if hasattr(L, "asgart_align_duplications"):
        L.asgart_align_duplications.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.c_uint64, C.POINTER(vp)]
        L.asgart_align_duplications.restype = C.c_int32
        L.asgart_alignment_counts.argtypes = [vp, u64p, u64p, u64p]
        L.asgart_alignment_counts.restype = None
        L.asgart_alignment_copy.argtypes = [vp] * 7
        L.asgart_alignment_copy.restype = C.c_int32
        L.asgart_alignment_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_alignment_timings.restype = C.c_int32
        L.asgart_alignment_free.argtypes = [vp]
        L.asgart_alignment_free.restype = None
        L.asgart_align_geometry.argtypes = [u64p, u64p, u64p]
        L.asgart_align_geometry.restype = None
        L.asgart_align_bytes.argtypes = [vp, C.c_int64, C.c_int32, vp]
        L.asgart_align_bytes.restype = C.c_int32
    if hasattr(L, "asgart_align_duplications_banded"):
        L.asgart_align_duplications_banded.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, vp, C.c_uint64, C.POINTER(vp)]
        L.asgart_align_duplications_banded.restype = C.c_int32
        L.asgart_alignment_rounds.argtypes = [vp, C.POINTER(C.c_uint32), u64p]
        L.asgart_alignment_rounds.restype = C.c_int32
        L.asgart_align_bytes_banded.argtypes = [vp, C.c_int64, C.c_int32, vp, vp]
        L.asgart_align_bytes_banded.restype = C.c_int32
    if hasattr(L, "asgart_paf_records"):
        L.asgart_paf_records.argtypes = [C.c_int32, vp, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp,
                                         C.c_int64, C.POINTER(vp)]
        L.asgart_paf_records.restype = C.c_int32
        L.asgart_paf_geometry.argtypes = [u64p, u64p, u64p]
        L.asgart_paf_geometry.restype = None
    if hasattr(L, "asgart_paf_records_cs"):
        L.asgart_paf_records_cs.argtypes = [vp, C.c_int32, vp, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp,
                                            vp, C.c_int64, C.POINTER(vp)]
        L.asgart_paf_records_cs.restype = C.c_int32
        L.asgart_paf_cs_geometry.argtypes = [u64p, u64p, u64p, u64p]
        L.asgart_paf_cs_geometry.restype = None
        L.asgart_index_read_text.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
        L.asgart_index_read_text.restype = C.c_int32
    if hasattr(L, "asgart_alignment_stats"):
        L.asgart_alignment_stats.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp, C.POINTER(C.c_double)]
        L.asgart_alignment_stats.restype = C.c_int32
        L.asgart_alignment_stats_geometry.argtypes = [u64p, u64p]
        L.asgart_alignment_stats_geometry.restype = None
        L.asgart_sdtable_records.argtypes = [C.c_int32, vp, C.c_int64, vp, vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, vp,
                                             vp, vp, vp, vp, C.c_uint64, C.POINTER(vp)]
        L.asgart_sdtable_records.restype = C.c_int32
        L.asgart_sdtable_geometry.argtypes = [u64p, u64p, u64p]
        L.asgart_sdtable_geometry.restype = None
    if hasattr(L, "asgart_mask_intervals"):
        L.asgart_mask_intervals.argtypes = [C.c_int32, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, C.c_uint64, C.c_uint32,
                                            C.POINTER(vp)]
        L.asgart_mask_intervals.restype = C.c_int32
        L.asgart_mask_counts.argtypes = [vp, u64p, u64p, u64p]
        L.asgart_mask_counts.restype = None
        L.asgart_mask_copy.argtypes = [vp, vp]
        L.asgart_mask_copy.restype = None
        L.asgart_mask_timings.argtypes = [vp, C.POINTER(C.c_double)]
        L.asgart_mask_timings.restype = C.c_int32
        L.asgart_mask_free.argtypes = [vp]
        L.asgart_mask_free.restype = None
        L.asgart_mask_geometry.argtypes = [u64p]
        L.asgart_mask_geometry.restype = None
        L.asgart_fasta_write.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.asgart_fasta_write.restype = C.c_int32
        L.asgart_fasta_write_geometry.argtypes = [u64p, u64p, u64p]
        L.asgart_fasta_write_geometry.restype = None
    if hasattr(L, "asgart_alignment_variants"):
        L.asgart_alignment_variants.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, vp, C.POINTER(vp)]
        L.asgart_alignment_variants.restype = C.c_int32
        L.asgart_variants_counts.argtypes = [vp, u64p, u64p, u64p]
        L.asgart_variants_counts.restype = None
        L.asgart_variants_copy.argtypes = [vp, vp, vp]
        L.asgart_variants_copy.restype = C.c_int32
        L.asgart_variant_sites.argtypes = [vp, C.POINTER(vp)]
        L.asgart_variant_sites.restype = C.c_int32
        L.asgart_sites_counts.argtypes = [vp, u64p, u64p]
        L.asgart_sites_counts.restype = None
        L.asgart_sites_copy.argtypes = [vp] * 7
        L.asgart_sites_copy.restype = C.c_int32
        for name in ("variants", "sites"):
            timings, free = getattr(L, f"asgart_{name}_timings"), getattr(L, f"asgart_{name}_free")
            timings.argtypes = [vp, C.POINTER(C.c_double)]
            timings.restype = C.c_int32
            free.argtypes = [vp]
            free.restype = None
            records, geometry = getattr(L, f"asgart_{name}_records"), getattr(L, f"asgart_{name}_records_geometry")
            records.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_uint64, C.POINTER(vp)]
            records.restype = C.c_int32
            geometry.argtypes = [u64p, u64p, u64p]
            geometry.restype = None
        L.asgart_variants_geometry.argtypes = [u64p, u64p]
        L.asgart_variants_geometry.restype = None
        L.asgart_sites_geometry.argtypes = [u64p]
        L.asgart_sites_geometry.restype = None
    L.asgart_last_error.argtypes = []
    L.asgart_last_error.restype = C.c_char_p
    L.asgart_version.argtypes = []
    L.asgart_version.restype = C.c_char_p
    _lib = L
    return L


def _check(rc: int):
    if rc < 0:
        raise AsgartError(int(rc), load_library().asgart_last_error().decode(errors="replace"))


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _families_out(L, h, with_keys: bool = False):
    """The arrays behind a families handle -> (fam_offsets[n_fam+1], sds[n_sd,4]), with_keys: and keys[n_fam]
    (asgart_families_keys); the handle is freed."""
    try:
        nf, ns = C.c_uint64(), C.c_uint64()
        L.asgart_families_counts(h, C.byref(nf), C.byref(ns))
        offs = np.zeros(nf.value + 1, dtype=np.uint64)
        sds = np.zeros((ns.value, 4), dtype=np.uint64)
        L.asgart_families_copy(h, _ptr(offs), _ptr(sds))
        if not with_keys:
            return offs, sds
        keys = np.zeros(nf.value, dtype=np.uint64)
        L.asgart_families_keys(h, _ptr(keys))
        return offs, sds, keys
    finally:
        L.asgart_families_free(h)


def _read_timings(fn, h, timings: Optional[list]) -> None:
    """The three millisecond figures of a result handle (fn: its asgart_*_timings) into the caller's list, if there is one."""
    if timings is not None:
        ms = (C.c_double * 3)()
        _check(fn(h, ms))
        timings[:] = list(ms)


def _as_u8(seq) -> np.ndarray:
    if isinstance(seq, np.ndarray):
        if seq.dtype != np.uint8:
            raise TypeError("text must be uint8")
        return np.ascontiguousarray(seq)
    if isinstance(seq, str):
        seq = seq.encode()
    return np.frombuffer(bytes(seq), dtype=np.uint8).copy()


@dataclass
class RunSettings:
    """reference src/structs.rs:36-58 (fields that reach the search path)."""

    probe_size: int = 20
    max_gap_size: int = 120  # gap_size + probe_size, src/bin/asgart.rs:681
    min_duplication_length: int = 1000
    max_cardinality: int = 500
    reverse: bool = False
    complement: bool = False
    skip_masked: bool = False
    trim: Optional[Tuple[int, int]] = None

    @classmethod
    def from_cli(cls, k=20, gap=100, min_length=1000, max_cardinality=500, reverse=False,
                 complement=False, skip_masked=False) -> "RunSettings":
        """`asgart -k K -g G --min-length M --max-cardinality C [-R] [-C] [-S]`
        (reference src/bin/asgart.rs:564-631,677-693)."""
        return cls(k, gap + k, min_length, max_cardinality, reverse, complement, skip_masked)

    def _c(self) -> _Settings:
        return _Settings(self.probe_size, self.max_gap_size, self.min_duplication_length,
                         self.max_cardinality, int(self.reverse), int(self.complement))


@dataclass
class ProtoSD:
    """reference src/structs.rs:418-429"""

    left: int
    right: int
    left_length: int
    right_length: int
    identity: float = 0.0
    reversed: bool = False
    complemented: bool = False

    def as_tuple(self):
        return (self.left, self.right, self.left_length, self.right_length)


ProtoSDsFamily = List[ProtoSD]


@dataclass
class Strand:
    """reference src/bin/asgart.rs:267-271 (`data` ends with '$', :430)."""

    file_names: str
    data: np.ndarray
    map: list = field(default_factory=list)


class Index:
    """Device-resident text + suffix array + search structures (one per GPU).

    Stands for what SearchDuplications::run builds before its timed part:
    `r_divsufsort(&strand.data)` and `Searcher::new(&strand.data, &sa, 0)`
    (reference src/bin/asgart.rs:141-155).
    """

    def __init__(self, text, sa: Optional[np.ndarray] = None, device: int = 0,
                 trim: Optional[Tuple[int, int]] = None):
        """trim=(start, end): the `--trim` variant (reference src/bin/asgart.rs:142-148): the suffix array
        covers data[start..end] + '$' only (entries shifted by +start) and the whole text is searched
        against it.  `sa` is then that shifted array (end - start + 1 entries) or None."""
        L = load_library()
        self.text = _as_u8(text)
        self.n = len(self.text)
        self._h = C.c_void_p()
        self.trim = trim
        sa_arr = None
        want = len(self.text) if trim is None else trim[1] - trim[0] + 1
        if sa is not None:
            sa_arr = np.ascontiguousarray(sa, dtype=np.int64)
            if len(sa_arr) != want:
                raise ValueError("suffix array length != text length (or the trimmed window + 1)")
        if trim is None:
            _check(L.asgart_index_create(_ptr(self.text), len(self.text), _ptr(sa_arr),
                                         want if sa_arr is not None else 0, device, C.byref(self._h)))
        else:
            _check(L.asgart_index_create_trim(_ptr(self.text), len(self.text), _ptr(sa_arr),
                                              want if sa_arr is not None else 0, int(trim[0]), int(trim[1]),
                                              device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load_library().asgart_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def clone(self, device: int = 0) -> "Index":
        """A replica of this index on `device` (text + suffix array copied device to device)."""
        other = Index.__new__(Index)
        other.text = self.text
        other.n = self.n
        other.trim = self.trim
        other._h = C.c_void_p()
        _check(load_library().asgart_index_clone(self._h, device, C.byref(other._h)))
        return other

    def export(self) -> Tuple[int, int, int]:
        """(device address of the text, of the suffix array, bytes per suffix-array entry): what a one-process-per-GPU
        host broadcasts to the other ranks (asgart_index_export; multi.replicate_index)."""
        t, a, w = C.c_void_p(), C.c_void_p(), C.c_int32()
        _check(load_library().asgart_index_export(self._h, C.byref(t), C.byref(a), C.byref(w)))
        return int(t.value), int(a.value), int(w.value)

    @classmethod
    def from_device(cls, d_text: int, n: int, d_sa: int, sa_entry_bytes: int, device: int = 0, text=None) -> "Index":
        """A replica from text and suffix array already in this GPU's memory (asgart_index_create_device: copied)."""
        self = cls.__new__(cls)
        self.text = text
        self.n = int(n)
        self.trim = None
        self._h = C.c_void_p()
        _check(load_library().asgart_index_create_device(C.c_void_p(d_text), n, C.c_void_p(d_sa), n, sa_entry_bytes,
                                                         device, C.byref(self._h)))
        return self

    def set_option(self, name: str, value: int):
        """Tuning / test option (include/asgart_hip.h: asgart_index_set_option)."""
        _check(load_library().asgart_index_set_option(self._h, name.encode(), int(value)))

    def set_tail_up(self, mode: int, hits: int = 0):
        """The tail rule of the placement (include/asgart_hip.h: asgart_index_set_tail_up): mode 0 off, 1 where tiers share
        a stream (the default), 2 always; hits > 0 replaces the tier table's thresholds (tests)."""
        _check(load_library().asgart_index_set_tail_up(self._h, int(mode), int(hits)))

    def tier_segments(self) -> Tuple[np.ndarray, int]:
        """-> (segments placed per tier 1..7 by the last search call as uint64[7], how many the tail rule moved up)."""
        out = np.zeros(8, dtype=np.uint64)
        _check(load_library().asgart_tier_segments(self._h, _ptr(out)))
        return out[:7].copy(), int(out[7])

    def fill_counts(self) -> np.ndarray:
        """-> uint64[6]: rows and entries read of the small, the streamed and the ranked hit-row fill of the last search call
        (asgart_fill_counts; the ranked fill is governed by ASGART_RANKED_FILL when the index is created)."""
        out = np.zeros(6, dtype=np.uint64)
        _check(load_library().asgart_fill_counts(self._h, _ptr(out)))
        return out

    def fill_tally(self) -> np.ndarray:
        """-> uint64[4, 3]: rows, interval entries and kept hits of the last search call's large hit rows, by class (asgart_fill_tally)."""
        out = np.zeros(12, dtype=np.uint64)
        _check(load_library().asgart_fill_tally(self._h, _ptr(out)))
        return out.reshape(4, 3)

    RUN_DIR_FIELDS = ("bytes", "buckets", "T", "inserted", "bucket_full", "hits", "misses", "switch")

    def run_dir_info(self) -> dict:
        """The run directory of the prepared index (asgart_run_dir_info): bytes (0: none), buckets, T, runs it holds, runs
        that found their bucket full, the lookups that hit and missed it in the last accounting pass (stats(1)), and
        ASGART_RUN_DIR as the index read it."""
        out = np.zeros(8, dtype=np.uint64)
        _check(load_library().asgart_run_dir_info(self._h, _ptr(out)))
        return {n: int(v) for n, v in zip(self.RUN_DIR_FIELDS, out)}

    LOOKUP_ACCOUNT_FIELDS = ("ptab_loads", "ptab_bytes", "keys_loads", "keys_bytes", "sa_loads", "sa_bytes", "dir_hits",
                             "dir_misses", "raw_1", "raw_2_8", "raw_9_32", "raw_33_256", "raw_above_256", "raw_0")

    def lookup_account(self) -> dict:
        """The loads of the looked-up probes by array, as the accounting pass of the last stats(1) counted them
        (asgart_lookup_account)."""
        out = np.zeros(16, dtype=np.uint64)
        _check(load_library().asgart_lookup_account(self._h, _ptr(out)))
        return {n: int(v) for n, v in zip(self.LOOKUP_ACCOUNT_FIELDS, out)}

    def check_sa(self) -> int:
        """GPU verifier of the resident suffix array: number of violating slots (0 = valid)."""
        r = int(load_library().asgart_index_check_sa(self._h))
        _check(r)
        return r

    def prepare(self, probe_size: int):
        _check(load_library().asgart_index_prepare(self._h, probe_size))

    def sa_read(self, lo: int, hi: int) -> np.ndarray:
        out = np.empty(max(0, hi - lo), dtype=np.int64)
        _check(load_library().asgart_sa_read(self._h, lo, hi, _ptr(out)))
        return out

    def read_text(self, lo: int, hi: int) -> np.ndarray:
        """The bytes [lo, hi) of the index's normalised text as uint8 (asgart_index_read_text): with the device FASTA
        reader the index holds the only copy of it."""
        out = np.empty(max(0, hi - lo), dtype=np.uint8)
        _check(load_library().asgart_index_read_text(self._h, lo, hi, _ptr(out)))
        return out

    def compute_scores(self, sds: np.ndarray, reversed_: bool = False, complemented: bool = False) -> np.ndarray:
        """ComputeScore of reference src/bin/asgart.rs:98-112 for an (n, 4) uint64 array of
        (left, right, left_length, right_length): Levenshtein identities as float32."""
        sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        out = np.empty(len(sds), dtype=np.float32)
        _check(load_library().asgart_compute_scores(self._h, _ptr(sds), len(sds), int(reversed_),
                                                    int(complemented), _ptr(out)))
        return out

    def compute_scores_shard(self, sds: np.ndarray, reversed_: bool = False, complemented: bool = False,
                             shard: int = 0, n_shards: int = 1) -> np.ndarray:
        """compute_scores for shard `shard` of `n_shards` (asgart_compute_scores_shard): `sds` is the FULL list, the
        same on every rank; the duplications score_owners(sds, n_shards) gives to `shard` are scored, bit-equal to
        compute_scores.  -> float32[len(sds)], NaN at the entries of the other shards."""
        sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        out = np.full(len(sds), np.nan, dtype=np.float32)
        _check(load_library().asgart_compute_scores_shard(self._h, _ptr(sds), len(sds), int(reversed_),
                                                          int(complemented), int(shard), int(n_shards), _ptr(out)))
        return out

    def compute_scores_flags(self, sds: np.ndarray, flags: Optional[np.ndarray]) -> np.ndarray:
        """compute_scores with one flag byte per duplication (asgart_compute_scores_flags): flags uint8[n], bit 0
        reversed, bit 1 complemented (None: all zero).  Entry q is bit-equal to compute_scores with q's two flags."""
        sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        flags = _score_flags(flags, len(sds))
        out = np.empty(len(sds), dtype=np.float32)
        _check(load_library().asgart_compute_scores_flags(self._h, _ptr(sds), _ptr(flags), len(sds), _ptr(out)))
        return out

    def align(self, sds: np.ndarray, flags: Optional[np.ndarray] = None, inclusive: bool = False, budget: int = 0,
              timings: Optional[list] = None, max_distance=None, rounds: Optional[list] = None) -> "Alignments":
        """One optimal unit-cost alignment of the two arms of every duplication (asgart_align_duplications): the
        canonical path of include/asgart_hip.h as run-length-encoded operations.  flags: as compute_scores_flags.
        inclusive: the arms are [p ..= p + length], the strings compute_scores compares, instead of [p, p + length).
        budget: device bytes the checkpoints of one batch may take (0: half of what is free); a duplication that alone
        needs more (align_bytes) is refused -- status 0, no runs, NaN identity -- and no result depends on it otherwise.
        timings: a list that receives the milliseconds of upload, forward pass, traceback + compaction and copy.
        max_distance: None walks the whole edit matrix of every duplication.  Anything else walks a diagonal corridor of it
        (asgart_align_duplications_banded; the budget is then in align_bytes_banded's bytes): an integer or a uint32 array
        bounds the edits of every duplication or of each -- one with more gets status 2, no runs, NaN identity -- and
        "auto" lets the library choose and widen the bounds until none is beyond its own.  Every status-1 entry is
        bit-equal to the entry without max_distance.
        rounds: a list that receives [passes over the list, cells of the forward passes] (asgart_alignment_rounds)."""
        L = load_library()
        sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        flags = _score_flags(flags, len(sds))
        h = C.c_void_p()
        if max_distance is None:
            _check(L.asgart_align_duplications(self._h, _ptr(sds), _ptr(flags), len(sds), int(bool(inclusive)), int(budget),
                                               C.byref(h)))
        else:
            bounds = None if isinstance(max_distance, str) and max_distance == "auto" else _bounds(max_distance, len(sds))
            _check(L.asgart_align_duplications_banded(self._h, _ptr(sds), _ptr(flags), len(sds), int(bool(inclusive)),
                                                      None if bounds is None else _ptr(bounds), int(budget), C.byref(h)))
        try:
            n, nr, nref = C.c_uint64(), C.c_uint64(), C.c_uint64()
            L.asgart_alignment_counts(h, C.byref(n), C.byref(nr), C.byref(nref))
            out = Alignments(np.zeros(n.value + 1, np.uint64), np.zeros(nr.value, np.uint32), np.zeros(nr.value, np.uint8),
                             np.zeros(n.value, np.uint32), np.zeros(n.value, np.float32), np.zeros(n.value, np.uint8))
            _check(L.asgart_alignment_copy(h, _ptr(out.run_offsets), _ptr(out.run_len), _ptr(out.run_op), _ptr(out.distance),
                                           _ptr(out.identity), _ptr(out.status)))
            if timings is not None:
                ms = (C.c_double * 4)()
                _check(L.asgart_alignment_timings(h, ms))
                timings[:] = list(ms)
            if rounds is not None:
                nr_, nc_ = C.c_uint32(), C.c_uint64()
                _check(L.asgart_alignment_rounds(h, C.byref(nr_), C.byref(nc_)))
                rounds[:] = [int(nr_.value), int(nc_.value)]
            return out
        finally:
            L.asgart_alignment_free(h)

    def alignment_stats(self, sds: np.ndarray, flags: Optional[np.ndarray], aln: "Alignments",
                        timings: Optional[list] = None) -> "AlignCounts":
        """The counts of every alignment (asgart_alignment_stats; include/asgart_hip.h states them, align.stats_host is the
        readable form): sds and flags as align took them, aln the Alignments of align(sds, flags, inclusive=False).  A
        duplication whose status is not 1 gets ten zeros.  timings: a list that receives the milliseconds of upload,
        kernels and copy back."""
        L = load_library()
        if not hasattr(L, "asgart_alignment_stats"):
            raise AsgartError(-3, f"{library_path()} has no asgart_alignment_stats: rebuild it; there is no host fallback "
                                  "behind this call (align.stats_host is the host statement)")
        sds, flags, status, run_offsets, run_len, run_op = _alignment_arrays("alignment_stats", sds, flags, aln)
        n = len(sds)
        out = np.zeros((n, len(AlignCounts.FIELDS)), dtype=np.uint64)
        ms = (C.c_double * 3)()
        _check(L.asgart_alignment_stats(self._h, _ptr(sds), _ptr(flags), _ptr(status), n, _ptr(run_offsets), _ptr(run_len),
                                        _ptr(run_op), _ptr(out), ms))
        if timings is not None:
            timings[:] = list(ms)
        return AlignCounts(out)

    def variants(self, sds: np.ndarray, flags: Optional[np.ndarray], aln: "Alignments",
                 timings: Optional[list] = None) -> "Variants":
        """The variants between the arms of every aligned duplication (asgart_alignment_variants; include/asgart_hip.h states
        the rule, align.variants_host is the readable form): one record per base of an `X` run and per `I` or `D` run, global
        forward-strand coordinates.  sds, flags and aln as alignment_stats takes them.  The records stay on the device of the
        index behind the Variants handle (sites() and the device writers of align read them there); records() copies them.
        timings: a list that receives the milliseconds of upload, kernels and copy back."""
        L = load_library()
        if not hasattr(L, "asgart_alignment_variants"):
            raise AsgartError(-3, f"{library_path()} has no asgart_alignment_variants: rebuild it; there is no host fallback "
                                  "behind this call (align.variants_host is the host statement)")
        sds, flags, status, run_offsets, run_len, run_op = _alignment_arrays("variants", sds, flags, aln)
        h = C.c_void_p()
        _check(L.asgart_alignment_variants(self._h, _ptr(sds), _ptr(flags), _ptr(status), len(sds), _ptr(run_offsets),
                                           _ptr(run_len), _ptr(run_op), C.byref(h)))
        out = Variants(h)
        _read_timings(L.asgart_variants_timings, h, timings)
        return out

    def compute_scores_flags_shard(self, sds: np.ndarray, flags: Optional[np.ndarray], shard: int = 0,
                                   n_shards: int = 1) -> np.ndarray:
        """compute_scores_shard with one flag byte per duplication (asgart_compute_scores_flags_shard): the same owners,
        NaN at the entries of the other shards."""
        sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        flags = _score_flags(flags, len(sds))
        out = np.full(len(sds), np.nan, dtype=np.float32)
        _check(load_library().asgart_compute_scores_flags_shard(self._h, _ptr(sds), _ptr(flags), len(sds), int(shard),
                                                                int(n_shards), _ptr(out)))
        return out

    def post_process(self, offs: np.ndarray, sds: np.ndarray, threads: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """FilterNs -> ReOrder -> ReduceOverlap -> Sort (reference src/bin/asgart.rs:738-747) on raw family arrays as
        search_duplications_raw returns them -> the same form (asgart_post_process: N counts on the GPU, the reduction
        on host threads)."""
        L = load_library()
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        h = C.c_void_p()
        _check(L.asgart_post_process(self._h, _ptr(offs), len(offs) - 1, _ptr(sds), threads, C.byref(h)))
        return _families_out(L, h)

    def stats(self, flags: int = 2) -> Stats:
        """Statistics of the last search call.  flags: 1 = with the yardstick / accounting passes, 2 (default) = with raw_hits
        (an untimed pass over the call's probes), 0 = what the call itself recorded; (i + 1) << 8 selects call context i."""
        st = Stats()
        _check(load_library().asgart_get_stats(self._h, flags, C.byref(st)))
        return st

    # -- SearchDuplications::run body --------------------------------------
    def search_duplications_raw(self, chunks: Sequence[Tuple[int, int]], settings: RunSettings,
                                shard: int = 0, n_shards: int = 1, progress: Optional[np.ndarray] = None,
                                with_keys: bool = False):
        """-> (fam_offsets[n_fam+1], sds[n_sd,4]) as uint64 arrays.  progress: optional uint64[n_chunks]
        the library writes each chunk's needle offset into when the call's search phases are over (see the header)."""
        L = load_library()
        ch = np.array(chunks, dtype=np.uint64).reshape(-1)
        st = settings._c()
        h = C.c_void_p()
        if progress is not None:
            assert progress.dtype == np.uint64 and len(progress) >= len(chunks)
        if n_shards == 1:
            _check(L.asgart_search_duplications(self._h, _ptr(ch), len(chunks), C.byref(st), _ptr(progress),
                                                C.byref(h)))
        elif progress is None:
            _check(L.asgart_search_duplications_shard(self._h, _ptr(ch), len(chunks), C.byref(st),
                                                      shard, n_shards, C.byref(h)))
        else:
            _check(L.asgart_search_duplications_ex(self._h, _ptr(ch), len(chunks), C.byref(st), shard, n_shards,
                                                   _ptr(progress), C.byref(h)))
        return _families_out(L, h, with_keys)

    def search_duplications_passes(self, chunks: Sequence[Tuple[int, int]], settings: Sequence[RunSettings],
                                   shard: int = 0, n_shards: int = 1, with_keys: bool = False) -> List[tuple]:
        """Several passes (one RunSettings each, e.g. the direct and the -RC run) in one call; the library pipelines
        them itself.  -> [(fam_offsets, sds)] in the order of `settings`, each as search_duplications_raw returns it."""
        L = load_library()
        ch = np.array(chunks, dtype=np.uint64).reshape(-1)
        n = len(settings)
        sts = (_Settings * max(n, 1))(*[s._c() for s in settings])
        hs = (C.c_void_p * max(n, 1))()
        if n_shards == 1:
            _check(L.asgart_search_duplications_passes(self._h, _ptr(ch), len(chunks), sts, n, hs))
        else:
            _check(L.asgart_search_duplications_passes_shard(self._h, _ptr(ch), len(chunks), sts, n, shard, n_shards, hs))
        left = list(hs)[:n]   # (a handle is freed by whoever reads it; the ones an exception leaves unread, here)
        try:
            return [_families_out(L, left.pop(0), with_keys) for _ in range(n)]
        finally:
            for h in left:
                L.asgart_families_free(h)

    def probe_hits(self, chunks: Sequence[Tuple[int, int]], settings: RunSettings):
        """Per-probe filtered hits for all chunks: (status, row_offsets, hits)."""
        L = load_library()
        ch = np.array(chunks, dtype=np.uint64).reshape(-1)
        st = settings._c()
        nh = C.c_uint64()
        n_probes = L.asgart_probe_hits(self._h, _ptr(ch), len(chunks), C.byref(st), None, None,
                                       None, C.byref(nh))
        _check(n_probes)
        status = np.zeros(n_probes, dtype=np.uint8)
        offs = np.zeros(n_probes + 1, dtype=np.uint64)
        hits = np.zeros(nh.value, dtype=np.uint64)
        _check(L.asgart_probe_hits(self._h, _ptr(ch), len(chunks), C.byref(st), _ptr(status),
                                   _ptr(offs), _ptr(hits), C.byref(nh)))
        return status, offs, hits


@dataclass
class Alignments:
    """The arrays of asgart_alignment_copy: the runs of duplication q are run_offsets[q] .. run_offsets[q + 1] of run_len
    and run_op (the bytes '=', 'X', 'I', 'D'); distance uint32, identity float32, status uint8 (1: aligned; 0: refused by
    the budget; 2: more edits than max_distance -- both without runs, distance 0xFFFFFFFF, identity NaN)."""

    run_offsets: np.ndarray
    run_len: np.ndarray
    run_op: np.ndarray
    distance: np.ndarray
    identity: np.ndarray
    status: np.ndarray

    def __len__(self) -> int:
        return len(self.distance)

    def ops(self, q: int) -> List[Tuple[int, str]]:
        """The runs of duplication q in forward order: [(length, operation)]."""
        a, b = int(self.run_offsets[q]), int(self.run_offsets[q + 1])
        return list(zip(self.run_len[a:b].tolist(), self.run_op[a:b].tobytes().decode("ascii")))

    def part(self, lo: int, hi: int) -> "Alignments":
        """The duplications lo .. hi - 1 as a result of their own."""
        a, b = int(self.run_offsets[lo]), int(self.run_offsets[hi])
        return Alignments(self.run_offsets[lo:hi + 1] - self.run_offsets[lo], self.run_len[a:b], self.run_op[a:b],
                          self.distance[lo:hi], self.identity[lo:hi], self.status[lo:hi])

    def cigar(self, q: int) -> str:
        """`812=1X40=3I...`; empty for a refused duplication and for one beyond its max_distance."""
        return "".join(f"{n}{op}" for n, op in self.ops(q))


class AlignCounts:
    """The counts of asgart_alignment_stats: `table` is uint64[n, 10], one asgart_align_counts per duplication; every field
    is also an attribute (counts.match is table[:, 0])."""

    FIELDS = ("match", "mismatch", "transition", "transversion", "ins_runs", "ins_bases", "del_runs", "del_bases",
              "longest_match", "longest_gap")

    def __init__(self, table):
        self.table = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, len(self.FIELDS))

    def __len__(self) -> int:
        return len(self.table)

    def __getattr__(self, name):
        if name in AlignCounts.FIELDS:
            return self.table[:, AlignCounts.FIELDS.index(name)]
        raise AttributeError(name)

    def __eq__(self, other):
        return isinstance(other, AlignCounts) and np.array_equal(self.table, other.table)

    def part(self, lo: int, hi: int) -> "AlignCounts":
        """The duplications lo .. hi - 1 as counts of their own."""
        return AlignCounts(self.table[lo:hi])


def alignment_stats_geometry() -> Tuple[int, int]:
    """asgart_alignment_stats_geometry: threads per workgroup, mismatch bases per workgroup of the bases kernel."""
    a, b = C.c_uint64(), C.c_uint64()
    load_library().asgart_alignment_stats_geometry(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def _alignment_arrays(who: str, sds, flags, aln: "Alignments"):
    """What Index.alignment_stats and Index.variants share on the way in -> (sds, flags, status, run_offsets, run_len,
    run_op) as the library takes them."""
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = _score_flags(flags, len(sds))
    if flags is None:
        flags = np.zeros(len(sds), dtype=np.uint8)
    status = np.ascontiguousarray(aln.status, dtype=np.uint8).reshape(-1)
    run_offsets = np.ascontiguousarray(aln.run_offsets, dtype=np.uint64).reshape(-1)
    run_len = np.ascontiguousarray(aln.run_len, dtype=np.uint32).reshape(-1)
    run_op = np.ascontiguousarray(aln.run_op, dtype=np.uint8).reshape(-1)
    n = len(sds)
    if len(status) != n or len(run_offsets) != n + 1 or len(run_len) != len(run_op):
        raise ValueError(f"{who}: the arrays differ in length")
    if len(run_len) < int(run_offsets[-1]) < 1 << 32:   # (2^32 runs and more are the library's to refuse, unread)
        raise ValueError(f"{who}: run_offsets end at {int(run_offsets[-1])}, there are {len(run_len)} runs")
    if len(run_len) == 0:
        run_len, run_op = np.zeros(1, np.uint32), np.zeros(1, np.uint8)
    return sds, flags, status, run_offsets, run_len, run_op


# asgart_variant, as a numpy record: 32 bytes
VARIANT_DTYPE = np.dtype([("left_pos", "<u8"), ("right_pos", "<u8"), ("left_len", "<u4"), ("right_len", "<u4"), ("sd", "<u4"),
                          ("op", "u1"), ("left_base", "u1"), ("right_base", "u1"), ("flag", "u1")])
SITE_CLASSES = "ACGTN"   # the classes of a site's ref and the bits of its alt_mask, in order


@dataclass
class SiteArrays:
    """The arrays of asgart_sites_copy (and of align.sites_host), one entry per site in ascending position: pos uint64; ref
    uint8, a class (an index into SITE_CLASSES); alt_mask uint8, bit c for class c; pairs uint32, the number of entries;
    sd uint32 and side uint8 (0 left, 1 right) of the first entry."""

    pos: np.ndarray
    ref: np.ndarray
    alt_mask: np.ndarray
    pairs: np.ndarray
    sd: np.ndarray
    side: np.ndarray

    def __len__(self) -> int:
        return len(self.pos)

    def __eq__(self, other):
        return isinstance(other, SiteArrays) and all(
            a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(self.columns(), other.columns()))

    def columns(self):
        return self.pos, self.ref, self.alt_mask, self.pairs, self.sd, self.side


class _Handle:
    """A result handle of the library that stays alive until close() (or the end of a `with`, or collection)."""

    _free = ""

    def __init__(self, h):
        self._h = h

    def close(self) -> None:
        if self._h:
            getattr(load_library(), self._free)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rows_file(call, who: str, h, offs, sds, flags, chr_, chr_pos, names: Sequence[bytes], prefix: bytes,
               timings: Optional[list]) -> np.ndarray:
    """What the two device writers of the variants share: the result arrays as the library takes them, the call, the file."""
    offs, sds, flags, chr_, chr_pos, name_bytes, name_off = _result_arrays(who, offs, sds, flags, chr_, chr_pos, names)
    pre = np.frombuffer(prefix or b"\0", dtype=np.uint8)
    out = C.c_void_p()
    _check(call(h, _ptr(offs), len(offs) - 1, _ptr(sds), _ptr(flags), _ptr(chr_), _ptr(chr_pos), len(sds), _ptr(name_bytes),
                _ptr(name_off), len(names), _ptr(pre), len(prefix), C.byref(out)))
    return _written_file(out, timings)


class Variants(_Handle):
    """The records of Index.variants, on the device (asgart_variants): n_sd, n_variants, n_snv; records() and var_offsets()
    copy them; sites() makes the sites of the `X` records; table() writes the pair table on the device."""

    _free = "asgart_variants_free"

    def __init__(self, h):
        super().__init__(h)
        v = [C.c_uint64() for _ in range(3)]
        load_library().asgart_variants_counts(h, *[C.byref(x) for x in v])
        self.n_sd, self.n_variants, self.n_snv = (int(x.value) for x in v)

    def __len__(self) -> int:
        return self.n_variants

    def records(self) -> np.ndarray:
        """The records as a VARIANT_DTYPE array."""
        out = np.zeros(self.n_variants, dtype=VARIANT_DTYPE)
        _check(load_library().asgart_variants_copy(self._h, _ptr(out) if len(out) else None, None))
        return out

    def var_offsets(self) -> np.ndarray:
        out = np.zeros(self.n_sd + 1, dtype=np.uint64)
        _check(load_library().asgart_variants_copy(self._h, None, _ptr(out)))
        return out

    def sites(self, timings: Optional[list] = None) -> "Sites":
        """asgart_variant_sites: the distinct positions the `X` records touch, on the device."""
        L = load_library()
        h = C.c_void_p()
        _check(L.asgart_variant_sites(self._h, C.byref(h)))
        out = Sites(h)
        _read_timings(L.asgart_sites_timings, h, timings)
        return out

    def table(self, offs, sds, flags, chr_, chr_pos, names: Sequence[bytes], prefix: bytes,
              timings: Optional[list] = None) -> np.ndarray:
        """asgart_variants_records: the pair table as uint8[size]; the arrays as sdtable_records takes them."""
        return _rows_file(load_library().asgart_variants_records, "variants_records", self._h, offs, sds, flags, chr_,
                          chr_pos, names, prefix, timings)


class Sites(_Handle):
    """The sites of Variants.sites, on the device (asgart_sites): n_sites, n_entries; arrays() copies them; vcf() writes
    the VCF body rows on the device."""

    _free = "asgart_sites_free"

    def __init__(self, h):
        super().__init__(h)
        a, b = C.c_uint64(), C.c_uint64()
        load_library().asgart_sites_counts(h, C.byref(a), C.byref(b))
        self.n_sites, self.n_entries = int(a.value), int(b.value)

    def __len__(self) -> int:
        return self.n_sites

    def arrays(self) -> SiteArrays:
        n = self.n_sites
        out = SiteArrays(np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32),
                         np.zeros(n, np.uint32), np.zeros(n, np.uint8))
        if n:
            _check(load_library().asgart_sites_copy(self._h, *[_ptr(c) for c in out.columns()]))
        return out

    def vcf(self, offs, sds, flags, chr_, chr_pos, names: Sequence[bytes], prefix: bytes,
            timings: Optional[list] = None) -> np.ndarray:
        """asgart_sites_records: the caller's header and one VCF row per site as uint8[size]."""
        return _rows_file(load_library().asgart_sites_records, "sites_records", self._h, offs, sds, flags, chr_, chr_pos,
                          names, prefix, timings)


def variants_geometry() -> Tuple[int, int]:
    """asgart_variants_geometry: threads per workgroup, records per workgroup of the records kernel."""
    a, b = C.c_uint64(), C.c_uint64()
    load_library().asgart_variants_geometry(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def sites_geometry() -> int:
    """asgart_sites_geometry: threads per workgroup of the site kernels."""
    a = C.c_uint64()
    load_library().asgart_sites_geometry(C.byref(a))
    return int(a.value)


def variants_records_geometry() -> Tuple[int, int, int]:
    """asgart_variants_records_geometry: threads per workgroup, rows per workgroup, bytes of the LDS image."""
    v = [C.c_uint64() for _ in range(3)]
    load_library().asgart_variants_records_geometry(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def sites_records_geometry() -> Tuple[int, int, int]:
    """asgart_sites_records_geometry: threads per workgroup, rows per workgroup, bytes of the LDS image."""
    v = [C.c_uint64() for _ in range(3)]
    load_library().asgart_sites_records_geometry(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def align_geometry() -> Tuple[int, int, int]:
    """(rows of one band, rows of one lane, columns of one tile W) of the alignment kernels (asgart_align_geometry)."""
    v = [C.c_uint64() for _ in range(3)]
    load_library().asgart_align_geometry(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def align_bytes(sds: np.ndarray, inclusive: bool = False) -> np.ndarray:
    """The checkpoint bytes Index.align needs for each duplication (asgart_align_bytes; host code, no device)."""
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(len(sds), dtype=np.uint64)
    _check(load_library().asgart_align_bytes(_ptr(sds), len(sds), int(bool(inclusive)), _ptr(out)))
    return out


def _bounds(max_distance, n: int) -> np.ndarray:
    """max_distance of Index.align as one uint32 per duplication: an integer for all, or an array of n."""
    if isinstance(max_distance, str):
        raise ValueError('max_distance: None, "auto", an integer or one uint32 per duplication')
    v = np.asarray(max_distance)
    if v.ndim == 0:
        v = np.full(n, v)
    if v.shape != (n,) or not np.issubdtype(v.dtype, np.integer) or (len(v) and (v.min() < 0 or v.max() > 0xFFFFFFFF)):
        raise ValueError(f"max_distance: {n} duplications need one bound, or {n}, each an integer in [0, 2^32)")
    return np.ascontiguousarray(v, dtype=np.uint32)


def align_bytes_banded(sds: np.ndarray, max_distance, inclusive: bool = False) -> np.ndarray:
    """The checkpoint bytes Index.align(max_distance=) needs for each duplication within its bound
    (asgart_align_bytes_banded; host code, no device)."""
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    bounds = _bounds(max_distance, len(sds))
    out = np.zeros(len(sds), dtype=np.uint64)
    _check(load_library().asgart_align_bytes_banded(_ptr(sds), len(sds), int(bool(inclusive)), _ptr(bounds), _ptr(out)))
    return out


class Source:
    """The raw bytes of a run's records on one GPU, what asgart-extract slices the duplicons' sequences from (reference
    src/bin/asgart-extract.rs:17-29,110-131): asgart_source_create / asgart_extract_sequences.  Unlike Index.text it is
    not normalised: soft-masked lower case and IUPAC letters stay as they are."""

    def __init__(self):
        self._h = C.c_void_p()
        self.n = 0

    @classmethod
    def from_records(cls, records, device: int = 0) -> "Source":
        """records: the sequences in order, as (name, bytes) pairs (what prep.read_records yields) or bare byte
        sequences."""
        seqs = [_as_u8(r[1] if isinstance(r, tuple) else r) for r in records]
        ptrs = (C.c_void_p * max(len(seqs), 1))(*[s_.ctypes.data for s_ in seqs])
        lens = np.array([len(s_) for s_ in seqs], dtype=np.uint64)
        self = cls()
        _check(load_library().asgart_source_create(ptrs, _ptr(lens), len(seqs), device, C.byref(self._h)))
        self.n = int(lens.sum())
        return self

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load_library().asgart_source_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def extract_piece(self, sds: np.ndarray, flags: np.ndarray, first: int, out: np.ndarray) -> Tuple[np.ndarray, int]:
        """One asgart_extract_sequences call: the duplicons from `first` on that fit whole into `out` (uint8) ->
        (end offsets in `out`, 2 per duplicon done, number done).  Raises AsgartError (ASGART_E_CAP: the first does not
        fit; its `room` is the number of bytes that duplication needs)."""
        sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        flags = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        ends = np.zeros(2 * max(len(sds) - first, 1), dtype=np.uint64)
        done = C.c_int64()
        rc = load_library().asgart_extract_sequences(self._h, _ptr(sds), _ptr(flags), len(sds), int(first), _ptr(out),
                                                     len(out), _ptr(ends), C.byref(done))
        try:
            _check(rc)
        except AsgartError as err:
            if rc == -4:
                err.room = int(ends[1])
            raise
        return ends[:2 * done.value], int(done.value)

    def extract(self, sds: np.ndarray, reversed_=False, complemented=False,
                piece_bytes: int = 1 << 30) -> Tuple[np.ndarray, np.ndarray]:
        """Both arms of every duplication of an (n, 4) uint64 array (left, right, left_length, right_length), left then
        right for each; reversed_ / complemented: one flag for all, or one per duplication (the right arm only).
        -> (ends uint64[2n]: cumulative end offsets, bytes uint8[ends[-1]]).  The library is called for pieces of at
        most piece_bytes output bytes (a larger one for a duplication that needs more)."""
        sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
        n = len(sds)
        flags = (np.broadcast_to(np.asarray(reversed_, dtype=bool), (n,)).astype(np.uint8) |
                 (np.broadcast_to(np.asarray(complemented, dtype=bool), (n,)).astype(np.uint8) << 1))
        flags = np.ascontiguousarray(flags)
        total = int(sds[:, 2].sum(dtype=np.uint64) + sds[:, 3].sum(dtype=np.uint64)) if n else 0
        data = np.empty(total, dtype=np.uint8)
        ends = np.zeros(2 * n, dtype=np.uint64)
        first = pos = 0
        while first < n:
            cap = min(max(int(piece_bytes), 1), total - pos)
            try:
                e, done = self.extract_piece(sds, flags, first, data[pos:pos + cap])
            except AsgartError as err:
                if err.code != -4:   # ASGART_E_CAP: this duplication alone needs more than a piece
                    raise
                e, done = self.extract_piece(sds, flags, first, data[pos:pos + err.room])
            if done == 0:
                raise AsgartError(-4, f"asgart_extract_sequences: no progress at duplication {first}")
            ends[2 * first:2 * (first + done)] = e + np.uint64(pos)
            pos += int(e[-1]) if done else 0
            first += done
        return ends, data


def search_duplications_multi(indices: Sequence[Index], chunks: Sequence[Tuple[int, int]],
                              settings: RunSettings) -> Tuple[np.ndarray, np.ndarray]:
    """asgart_search_duplications_multi: one shard per index replica (one per GPU), one host thread each,
    results concatenated in shard order -> (fam_offsets, sds) like Index.search_duplications_raw."""
    L = load_library()
    ch = np.array(chunks, dtype=np.uint64).reshape(-1)
    st = settings._c()
    arr = (C.c_void_p * len(indices))(*[i._h for i in indices])
    h = C.c_void_p()
    _check(L.asgart_search_duplications_multi(arr, len(indices), _ptr(ch), len(chunks), C.byref(st), None,
                                              C.byref(h)))
    return _families_out(L, h)


def score_owners(sds: np.ndarray, n_shards: int) -> np.ndarray:
    """asgart_score_owners (host code, no device needed): the shard of each duplication of an (n, 4) uint64 array under
    the cost-balanced split that Index.compute_scores_shard uses -> int32[n]."""
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(len(sds), dtype=np.int32)
    _check(load_library().asgart_score_owners(_ptr(sds), len(sds), int(n_shards), _ptr(out)))
    return out


def score_costs(sds: np.ndarray) -> np.ndarray:
    """asgart_score_costs: the cost (device wave-steps) score_owners balances, per duplication -> uint64[n]."""
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(len(sds), dtype=np.uint64)
    _check(load_library().asgart_score_costs(_ptr(sds), len(sds), _ptr(out)))
    return out


def tier_plan(budget: int, n_work, tier_order: int, est_ms, main_ms: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """asgart_tier_plan (host code, no device needed): the streams a search call puts its extension tiers on, for 7
    tiers' work counts and estimated durations (ms) -> (stream_of int32[7]: 0 = the main stream, s = tier stream s,
    -1 = no work; launch int32[7]: the tiers with work in launch order, 0 behind them)."""
    work = np.ascontiguousarray(n_work, dtype=np.uint64).reshape(7)
    est = np.ascontiguousarray(est_ms, dtype=np.float64).reshape(7)
    stream_of = np.zeros(7, dtype=np.int32)
    launch = np.zeros(7, dtype=np.int32)
    _check(load_library().asgart_tier_plan(int(budget), _ptr(work), int(tier_order), _ptr(est), float(main_ms),
                                           _ptr(stream_of), _ptr(launch)))
    return stream_of, launch


def tier_profile() -> Tuple[np.ndarray, np.ndarray]:
    """asgart_tier_profile (host code): (profile_ms float64[8]: [0] the runs over ranges, [t] tier t's estimated duration
    before a call has measurements; tail_hits uint64[8]: tier t's threshold of the tail rule, 0 = none)."""
    ms = np.zeros(8, dtype=np.float64)
    hits = np.zeros(8, dtype=np.uint64)
    _check(load_library().asgart_tier_profile(_ptr(ms), _ptr(hits)))
    return ms, hits


FIX_HELD = 0xFFFFFFFE     # join_cuts: a range's records wait for the segment's tail run
FIX_DROPPED = 0xFFFFFFFF  # ... are dropped
JOINED, TAIL_RUN, WHOLE_AGAIN = 0, 1, 2  # join_cuts: what happens to the segment


def join_cuts(cut_held, flushes, last_gave_up: bool = False, tail_gave_up: bool = False) -> dict:
    """asgart_join_cuts (host code, no device needed): what a search call decides for ONE segment cut into
    len(flushes) ranges -- cut_held[j] bit 0: cut j held; flushes[j]: the families range j flushed; last_gave_up: the run
    over the last range gave up; tail_gave_up: so did the one more run over the rest, if there is one.
    -> f: the first cut that did not hold (len(cut_held): none); action: JOINED, TAIL_RUN (ranges 0..f stand, one more
    run from range f covers the rest) or WHOLE_AGAIN; tail_base: the family-ordinal base of that run; fix uint32[R]: what
    is added to the family ordinals of each range's records before the tail run has come back (FIX_HELD: they wait,
    FIX_DROPPED: they are dropped); settled uint32[R + 1]: the same after it has, [R] the tail run's own entry;
    settled_action: the action after it has (a tail run that gave up: WHOLE_AGAIN)."""
    flush = np.ascontiguousarray(flushes, dtype=np.uint32).reshape(-1)
    held = np.ascontiguousarray(cut_held, dtype=np.uint32).reshape(-1)
    R = len(flush)
    if len(held) != max(R - 1, 0):
        raise ValueError(f"{len(held)} cut verdicts for {R} ranges")
    held = np.concatenate([held, np.zeros(1, dtype=np.uint32)])  # (never read; R = 1 has no cut)
    fix = np.zeros(max(R, 1), dtype=np.uint32)
    settled = np.zeros(R + 1, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    _check(load_library().asgart_join_cuts(R, _ptr(held), _ptr(flush), int(bool(last_gave_up)), int(bool(tail_gave_up)),
                                           _ptr(fix), _ptr(settled), _ptr(out)))
    return {"f": int(out[0]), "action": int(out[1]), "tail_base": int(out[2]), "fix": fix[:R], "settled": settled,
            "settled_action": int(out[3])}


def split_warm_next(warm_used: int, need: int, range_len: int, split_warm_max: int) -> int:
    """asgart_split_warm_next (host code): the warm-up (probes) the index remembers for a segment a cut of which did not
    hold with warm_used probes of warm-up, whose oldest arm in front of the cut was born `need` probes in front of it, in
    a call with ranges of range_len probes and option split_warm_max; 0: none, only the cuts that held are planned again."""
    return int(load_library().asgart_split_warm_next(int(warm_used), int(need), int(range_len), int(split_warm_max)))


def compute_scores_multi(indices: Sequence[Index], sds: np.ndarray, reversed_: bool = False,
                         complemented: bool = False) -> np.ndarray:
    """asgart_compute_scores_multi: one shard per index replica, one host thread each -> float32[n], the array
    Index.compute_scores gives."""
    L = load_library()
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    out = np.empty(len(sds), dtype=np.float32)
    arr = (C.c_void_p * len(indices))(*[i._h for i in indices])
    _check(L.asgart_compute_scores_multi(arr, len(indices), _ptr(sds), len(sds), int(reversed_), int(complemented),
                                         _ptr(out)))
    return out


def _score_flags(flags, n: int) -> Optional[np.ndarray]:
    """The flag bytes of a compute_scores_flags* call: uint8[n], or None."""
    if flags is None:
        return None
    flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    if len(flags) != n:
        raise ValueError(f"{len(flags)} flag bytes for {n} duplications")
    return flags


def orientation_flags(reversed_, complemented, n: Optional[int] = None) -> np.ndarray:
    """The flag bytes (bit 0 reversed, bit 1 complemented) of asgart_compute_scores_flags and asgart_extract_sequences
    for two booleans or boolean arrays; n: broadcast to that many duplications."""
    f = np.asarray(reversed_, dtype=bool).astype(np.uint8) | (np.asarray(complemented, dtype=bool).astype(np.uint8) << 1)
    return np.ascontiguousarray(np.broadcast_to(f, (n,)) if n is not None else f)


def compute_scores_flags_multi(indices: Sequence[Index], sds: np.ndarray, flags: Optional[np.ndarray]) -> np.ndarray:
    """asgart_compute_scores_flags_multi: compute_scores_multi with one flag byte per duplication -> float32[n], the
    array Index.compute_scores_flags gives."""
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = _score_flags(flags, len(sds))
    out = np.empty(len(sds), dtype=np.float32)
    arr = (C.c_void_p * len(indices))(*[i._h for i in indices])
    _check(load_library().asgart_compute_scores_flags_multi(arr, len(indices), _ptr(sds), _ptr(flags), len(sds),
                                                            _ptr(out)))
    return out


EXPORT_FORMATS = {"json": 0, "gff2": 1, "gff3": 2}   # ASGART_EXPORT_JSON / _GFF2 / _GFF3
F32_TEXT_MAX = 64                                     # ASGART_F32_TEXT_MAX


def _result_arrays(who: str, offs, sds, flags, chr_, chr_pos, names: Sequence[bytes]):
    """What the file writers share on the way in: offs, sds, flags, chr_, chr_pos as the library takes them, and the name
    table as bytes and offsets -> (offs, sds, flags, chr_, chr_pos, name_bytes, name_off)."""
    offs = np.ascontiguousarray(offs, dtype=np.uint64).reshape(-1)
    sds = np.ascontiguousarray(sds, dtype=np.uint64).reshape(-1, 4)
    flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    chr_ = np.ascontiguousarray(chr_, dtype=np.int32).reshape(-1, 2)
    chr_pos = np.ascontiguousarray(chr_pos, dtype=np.uint64).reshape(-1, 2)
    if len(offs) < 1 or not (len(flags) == len(chr_) == len(chr_pos) == len(sds)):
        raise ValueError(f"{who}: the arrays differ in length")
    name_off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in names], out=name_off[1:])
    name_bytes = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8)
    return offs, sds, flags, chr_, chr_pos, name_bytes, name_off


def _written_file(h, timings: Optional[list]) -> np.ndarray:
    """What the file writers share on the way out: the file behind the handle h as uint8[size], the call's three
    millisecond figures into timings, the handle freed."""
    L = load_library()
    try:
        out = np.empty(int(L.asgart_export_size(h)), dtype=np.uint8)
        _check(L.asgart_export_copy(h, _ptr(out), len(out)))
        _read_timings(L.asgart_export_timings, h, timings)
    finally:
        L.asgart_export_free(h)
    return out


def export_records(fmt: str, offs, sds, flags, identity, chr_, chr_pos, names: Sequence[bytes], prefix: bytes,
                   suffix: bytes, device: int = 0, timings: Optional[list] = None) -> np.ndarray:
    """asgart_export_records: the whole result file as uint8[size], written on the GPU.  fmt: "json", "gff2" or "gff3";
    offs, sds, flags, chr_, chr_pos as slice.ResultArrays holds them; identity float32[n] or None (all 0); names: the name
    table, every name as bytes in the form the format prints it (slice.export_arrays_gpu and postprocess.to_json_arrays_gpu
    prepare it); prefix / suffix: what the file holds in front of and behind the families.  timings: a list that receives
    the call's three millisecond figures (asgart_export_timings: upload, kernels, copy back)."""
    if fmt not in EXPORT_FORMATS:
        raise ValueError(f"unknown format `{fmt}` (one of {', '.join(EXPORT_FORMATS)})")
    L = load_library()
    offs, sds, flags, chr_, chr_pos, name_bytes, name_off = _result_arrays("export_records", offs, sds, flags, chr_, chr_pos, names)
    n = len(sds)
    if identity is not None:
        identity = np.ascontiguousarray(identity, dtype=np.float32).reshape(-1)
        if len(identity) != n:
            raise ValueError("export_records: the arrays differ in length")
    pre, suf = (np.frombuffer(b or b"\0", dtype=np.uint8) for b in (prefix, suffix))
    h = C.c_void_p()
    _check(L.asgart_export_records(int(device), EXPORT_FORMATS[fmt], _ptr(offs), len(offs) - 1, _ptr(sds), _ptr(flags),
                                   _ptr(identity), _ptr(chr_), _ptr(chr_pos), n, _ptr(name_bytes), _ptr(name_off),
                                   len(names), _ptr(pre), len(prefix), _ptr(suf), len(suffix), C.byref(h)))
    return _written_file(h, timings)


def export_geometry() -> Tuple[int, int, int]:
    """asgart_export_geometry: threads per workgroup, units per workgroup, bytes of the LDS image of the write stage."""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    load_library().asgart_export_geometry(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


def _paf_records(call, who: str, offs, sds, flags, status, distance, chr_, chr_pos, run_offsets, run_len, run_op,
                 names: Sequence[bytes], name_length, timings: Optional[list]) -> np.ndarray:
    """What paf_records and paf_records_cs share: the arrays as the library takes them, call(the arguments behind the
    first one or two, the handle) and the copy of the file."""
    L = load_library()
    if not hasattr(L, "asgart_" + who):
        raise AsgartError(-3, f"{library_path()} has no asgart_{who}: rebuild it; there is no host fallback behind "
                              "this call (align.paf_text is the host writer)")
    offs, sds, flags, chr_, chr_pos, name_bytes, name_off = _result_arrays(who, offs, sds, flags, chr_, chr_pos, names)
    status = np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
    distance = np.ascontiguousarray(distance, dtype=np.uint32).reshape(-1)
    run_offsets = np.ascontiguousarray(run_offsets, dtype=np.uint64).reshape(-1)
    run_len = np.ascontiguousarray(run_len, dtype=np.uint32).reshape(-1)
    run_op = np.ascontiguousarray(run_op, dtype=np.uint8).reshape(-1)
    name_length = np.ascontiguousarray(name_length, dtype=np.uint64).reshape(-1)
    n = len(sds)
    if not (len(status) == len(distance) == n) or len(run_offsets) != n + 1 or len(run_len) != len(run_op) or \
            len(name_length) != len(names):
        raise ValueError(f"{who}: the arrays differ in length")
    if len(run_len) < int(run_offsets[-1]) < 1 << 32:   # (2^32 runs and more are the library's to refuse, unread)
        raise ValueError(f"{who}: run_offsets end at {int(run_offsets[-1])}, there are {len(run_len)} runs")
    if len(run_len) == 0:
        run_len, run_op = np.zeros(1, np.uint32), np.zeros(1, np.uint8)
    h = C.c_void_p()
    _check(call(_ptr(offs), len(offs) - 1, _ptr(sds), _ptr(flags), _ptr(status), _ptr(distance), _ptr(chr_), _ptr(chr_pos), n,
                _ptr(run_offsets), _ptr(run_len), _ptr(run_op), _ptr(name_bytes), _ptr(name_off), _ptr(name_length),
                len(names), C.byref(h)))
    return _written_file(h, timings)


def paf_records(offs, sds, flags, status, distance, chr_, chr_pos, run_offsets, run_len, run_op, names: Sequence[bytes],
                name_length, device: int = 0, timings: Optional[list] = None) -> np.ndarray:
    """asgart_paf_records: the whole PAF file as uint8[size], written on the GPU (csrc/paf.hip).  offs, sds, flags, chr_,
    chr_pos as export_records takes them; status, distance, run_offsets, run_len, run_op as Alignments holds them; names: the
    name table, every name as the bytes to write; name_length: the length of the fragment behind each name.  timings: a list
    that receives the call's three millisecond figures (asgart_export_timings: upload, kernels, copy back)."""
    return _paf_records(lambda *a: load_library().asgart_paf_records(int(device), *a), "paf_records", offs, sds, flags, status,
                        distance, chr_, chr_pos, run_offsets, run_len, run_op, names, name_length, timings)


CS_MODES = {"short": 1, "long": 2}   # cs_mode of asgart_paf_records_cs


def paf_records_cs(index: "Index", cs: str, offs, sds, flags, status, distance, chr_, chr_pos, run_offsets, run_len, run_op,
                   names: Sequence[bytes], name_length, timings: Optional[list] = None) -> np.ndarray:
    """asgart_paf_records_cs: the file of paf_records with the cs:Z: column, "short" or "long" (include/asgart_hip.h states
    the rule, align.cs_text is its readable form).  The device and the bases are the index's; everything else as
    paf_records."""
    if cs not in CS_MODES:
        raise ValueError("cs: 'short' or 'long'")
    if index is None:
        raise ValueError("paf_records_cs: the cs:Z: column needs the index whose text the duplications lie in")
    return _paf_records(lambda *a: load_library().asgart_paf_records_cs(index._h, CS_MODES[cs], *a), "paf_records_cs", offs,
                        sds, flags, status, distance, chr_, chr_pos, run_offsets, run_len, run_op, names, name_length, timings)


def paf_geometry() -> Tuple[int, int, int]:
    """asgart_paf_geometry: threads per workgroup of the write stage, the most runs one workgroup's range can hold, bytes of
    the file a workgroup owns (its LDS image)."""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    load_library().asgart_paf_geometry(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


def paf_cs_geometry() -> Tuple[int, int, int, int]:
    """asgart_paf_cs_geometry: paf_geometry's three sizes and solo_bytes, the most bytes of one run's cs text inside a
    workgroup's range that one thread composes alone."""
    a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    load_library().asgart_paf_cs_geometry(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    return int(a.value), int(b.value), int(c.value), int(d.value)


def sdtable_records(offs, sds, flags, status, chr_, chr_pos, names: Sequence[bytes], counts: "AlignCounts", figures,
                    prefix: bytes, device: int = 0, timings: Optional[list] = None) -> np.ndarray:
    """asgart_sdtable_records: the whole duplication table as uint8[size], written on the GPU (csrc/sdtable.hip).  offs, sds,
    flags, chr_, chr_pos, names as export_records takes them; status: a row for every duplication where it is not 0; counts:
    the AlignCounts of the duplications; figures: the four float32 arrays of align.divergence; prefix: the header line.
    timings: a list that receives the call's three millisecond figures (asgart_export_timings: upload, kernels, copy back)."""
    L = load_library()
    if not hasattr(L, "asgart_sdtable_records"):
        raise AsgartError(-3, f"{library_path()} has no asgart_sdtable_records: rebuild it; there is no host fallback behind "
                              "this call (align.sd_table_text is the host writer)")
    offs, sds, flags, chr_, chr_pos, name_bytes, name_off = _result_arrays("sdtable_records", offs, sds, flags, chr_, chr_pos, names)
    status = np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
    table = np.ascontiguousarray(counts.table, dtype=np.uint64)
    figures = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in figures]
    n = len(sds)
    if not (len(status) == len(table) == n) or len(figures) != 4 or any(len(v) != n for v in figures):
        raise ValueError("sdtable_records: the arrays differ in length")
    pre = np.frombuffer(prefix or b"\0", dtype=np.uint8)
    h = C.c_void_p()
    _check(L.asgart_sdtable_records(int(device), _ptr(offs), len(offs) - 1, _ptr(sds), _ptr(flags), _ptr(status), _ptr(chr_),
                                    _ptr(chr_pos), n, _ptr(name_bytes), _ptr(name_off), len(names), _ptr(table),
                                    *[_ptr(v) for v in figures], _ptr(pre), len(prefix), C.byref(h)))
    return _written_file(h, timings)


def sdtable_geometry() -> Tuple[int, int, int]:
    """asgart_sdtable_geometry: threads per workgroup, rows per workgroup, bytes of the LDS image of the write stage."""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    load_library().asgart_sdtable_geometry(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


E_REFUSED = -5   # ASGART_E_REFUSED: the device reader of result files leaves the input to the host reader


class ResultScan:
    """The two calls of the device reader of result files on one handle (asgart_result_scan, asgart_result_parse; the
    accepted grammar is stated in include/asgart_hip.h).  ResultScan(data) uploads and classifies the bytes of a RunResult
    JSON file (uint8 array) and holds the span [begin, end) of the value of "families"; parse(names) takes the name table
    -- UTF-8 bytes, sorted and unique -- and returns the arrays.  A refusal is AsgartError with code E_REFUSED: the input is
    the host reader's (slice.read_arrays does all of this)."""

    def __init__(self, data: np.ndarray, device: int = 0):
        L = load_library()
        self._h = C.c_void_p()
        self._data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)   # (kept alive: the scan reads its top-level keys)
        a, b = C.c_uint64(), C.c_uint64()
        _check(L.asgart_result_scan(int(device), _ptr(self._data) if len(self._data) else None, len(self._data),
                                    C.byref(self._h), C.byref(a), C.byref(b)))
        self.begin, self.end = int(a.value), int(b.value)

    def parse(self, names: Sequence[bytes]) -> dict:
        """-> offs uint64[F + 1], sds uint64[n, 4], flags uint8[n] (bit 2: the identity is hard), identity float32[n],
        chr int32[n, 2] (index into `names`, -1: a hard name), chr_pos uint64[n, 2], first_use uint32[len(names)],
        name_spans uint32[n, 2, 2] and identity_spans uint32[n, 2] (start, length), n_hard_names, n_hard_identities."""
        L = load_library()
        name_off = np.zeros(len(names) + 1, dtype=np.uint64)
        np.cumsum([len(b) for b in names], out=name_off[1:])
        name_bytes = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8)
        _check(L.asgart_result_parse(self._h, _ptr(name_bytes), _ptr(name_off), len(names)))
        nf, n, hn, hi = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.asgart_result_counts(self._h, C.byref(nf), C.byref(n), C.byref(hn), C.byref(hi))
        n = int(n.value)
        out = {"offs": np.zeros(int(nf.value) + 1, dtype=np.uint64), "sds": np.zeros((n, 4), dtype=np.uint64),
               "flags": np.zeros(n, dtype=np.uint8), "identity": np.zeros(n, dtype=np.float32),
               "chr": np.zeros((n, 2), dtype=np.int32), "chr_pos": np.zeros((n, 2), dtype=np.uint64),
               "first_use": np.zeros(len(names), dtype=np.uint32), "name_spans": np.zeros((n, 2, 2), dtype=np.uint32),
               "identity_spans": np.zeros((n, 2), dtype=np.uint32)}
        _check(L.asgart_result_copy(self._h, *(_ptr(out[k]) for k in ("offs", "sds", "flags", "identity", "chr", "chr_pos",
                                                                       "first_use", "name_spans", "identity_spans"))))
        out["n_hard_names"], out["n_hard_identities"] = int(hn.value), int(hi.value)
        return out

    def timings(self) -> List[float]:
        """asgart_result_timings: milliseconds of the upload, the scan kernels, the parse kernels, the copy back."""
        ms = (C.c_double * 4)()
        _check(load_library().asgart_result_timings(self._h, ms))
        return list(ms)

    def close(self):
        if self._h:
            load_library().asgart_result_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def result_geometry() -> Tuple[int, int, int]:
    """asgart_result_geometry: bytes per tile of the scan, records per workgroup and bytes of the LDS stage of the record
    stage."""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    load_library().asgart_result_geometry(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


def f32_shortest(values, mode: str = "json", device: int = 0) -> List[str]:
    """asgart_f32_shortest: every value of a float32 array as text, rendered on the GPU -- mode "json": what
    postprocess.f32_repr gives (serde_json's form), "display": what slice.f32_display gives (Rust's `{}`)."""
    if mode not in ("json", "display"):
        raise ValueError("f32_shortest: mode 'json' or 'display'")
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    text = np.zeros((len(v), F32_TEXT_MAX), dtype=np.uint8)
    lens = np.zeros(len(v), dtype=np.uint8)
    _check(load_library().asgart_f32_shortest(int(device), _ptr(v), len(v), 0 if mode == "json" else 1, _ptr(text), _ptr(lens)))
    rows = text.view(f"S{F32_TEXT_MAX}").reshape(-1).tolist()   # (a rendered f32 holds no NUL: S stops at the padding)
    if any(len(r) != ln for r, ln in zip(rows, lens.tolist())):
        raise AsgartError(-2, "asgart_f32_shortest: a length does not match its text")
    return [r.decode("ascii") for r in rows]


def f32_pow10_table():
    """asgart_f32_pow10_table -> (k_min, k_max, uint64[entries, 4]): hi, lo, x (as two's complement), exact per k, with
    10^-k = (hi * 2^64 + lo) * 2^x, rounded up where exact is 0.  Needs no GPU."""
    L = load_library()
    lo, hi = C.c_int32(), C.c_int32()
    n = L.asgart_f32_pow10_table(C.byref(lo), C.byref(hi), None)
    out = np.zeros((n, 4), dtype=np.uint64)
    L.asgart_f32_pow10_table(None, None, _ptr(out))
    return int(lo.value), int(hi.value), out


def trim_cache(device: int = 0) -> int:
    """Device memory the library holds for reuse goes back to the device (asgart_trim_cache); -> bytes released."""
    r = int(load_library().asgart_trim_cache(device))
    _check(r)
    return r


def sa_build64(text) -> np.ndarray:
    """`r_divsufsort` (reference src/bin/asgart.rs:473-479) on the GPU: the suffix array of
    `text` as int64, via asgart_sa_build64 (signature-identical to divsufsort64)."""
    t = _as_u8(text)
    sa = np.empty(len(t), dtype=np.int64)
    _check(load_library().asgart_sa_build64(_ptr(t), _ptr(sa), len(t)))
    return sa


class Searcher:
    """reference src/searcher.rs:94-180: `Searcher::new(dna, sa, offset)` and `search`."""

    def __init__(self, index: Index, offset: int = 0):
        self.index = index
        self.offset = offset

    @classmethod
    def new(cls, dna, sa: np.ndarray, offset: int = 0, device: int = 0) -> "Searcher":
        return cls(Index(dna, sa, device), offset)

    def cache(self, patterns8: Sequence[bytes]) -> List[Tuple[int, int]]:
        """8-mer -> (start, end) SA interval, the entries of Searcher.cache."""
        pats = np.frombuffer(b"".join(bytes(p) for p in patterns8), dtype=np.uint8).copy()
        n = len(patterns8)
        lo = np.zeros(n, dtype=np.uint64)
        hi = np.zeros(n, dtype=np.uint64)
        _check(load_library().asgart_searcher_cache_get(self.index._h, _ptr(pats), n, _ptr(lo),
                                                        _ptr(hi)))
        return [(int(a), int(b)) for a, b in zip(lo, hi)]

    def search_ranges(self, patterns: Sequence[bytes]) -> List[Tuple[int, int]]:
        k = len(patterns[0])
        pats = np.frombuffer(b"".join(bytes(p) for p in patterns), dtype=np.uint8).copy()
        n = len(patterns)
        lo = np.zeros(n, dtype=np.uint64)
        hi = np.zeros(n, dtype=np.uint64)
        _check(load_library().asgart_searcher_search(self.index._h, _ptr(pats), n, k, _ptr(lo),
                                                     _ptr(hi)))
        return [(int(a), int(b)) for a, b in zip(lo, hi)]

    def search(self, pattern: bytes) -> List[Tuple[int, int]]:
        """-> Segments (start, end) in SA order, like Searcher::search."""
        (lo, hi), = self.search_ranges([pattern])
        starts = self.index.sa_read(lo, hi)
        k = len(pattern)
        return [(self.offset + int(x), self.offset + int(x) + k) for x in starts]


class SearchDuplications:
    """The `Step` of reference src/bin/asgart.rs:114-259.

    `run(input, strand)` ignores `input` (as the reference does, :137) and returns
    the proto-duplication families found in `chunks_to_process`.
    """

    def __init__(self, chunks_to_process: Sequence[Tuple[int, int]],
                 trim: Optional[Tuple[int, int]], settings: RunSettings,
                 suffix_array: Optional[np.ndarray] = None, device: int = 0,
                 index: Optional[Index] = None):
        self.trim = trim
        self.chunks_to_process = list(chunks_to_process)
        self.settings = settings
        self.suffix_array = suffix_array
        self.device = device
        self.index = index

    def name(self) -> str:
        return "Looking for proto-duplications"

    def run(self, _input: List[ProtoSDsFamily], strand: Strand) -> List[ProtoSDsFamily]:
        index = self.index or Index(strand.data, self.suffix_array, self.device, trim=self.trim)
        try:
            offs, sds = index.search_duplications_raw(self.chunks_to_process, self.settings)
        finally:
            if self.index is None:
                index.close()
        s = self.settings
        out: List[ProtoSDsFamily] = []
        for f in range(len(offs) - 1):
            out.append([ProtoSD(int(r[0]), int(r[1]), int(r[2]), int(r[3]), 0.0, s.reverse,
                                s.complement) for r in sds[int(offs[f]):int(offs[f + 1])]])
        return out
