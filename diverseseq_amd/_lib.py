"""ctypes binding of libdvs_hip.so (include/dvs_hip.h) -- the only compute path.

There is no CPU fallback: if the HIP library is missing or no GPU is visible the
calls raise.  Nothing here imports ``oracle`` (the CPU restatement is test
infrastructure only).
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib
import threading

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
# DVS_HIP_LIB: another build of the same library (csrc/Makefile's host-sanitizer `asan` target)
LIB_PATH = pathlib.Path(os.environ["DVS_HIP_LIB"]).resolve() if os.environ.get("DVS_HIP_LIB") else _HERE / "libdvs_hip.so"

OK, ERR_VALUE, ERR_RUNTIME, ERR_NOMEM, ERR_UNSUPPORTED, ERR_ZERODIV = range(6)
CUT_HEIGHT, CUT_NCLUSTERS = 0, 1
MODE_NMOST, MODE_MAX, MODE_SET = 0, 1, 2
STAT_STDEV, STAT_COV = 0, 1
SELECT_NO_ARBITER = 1
SELECT_STEPWISE = 2
ROW_REMOTE = 0xFFFFFFFF

# every symbol include/dvs_hip.h declares (tests/test_boundary.py checks the .so exports them)
EXPORTS = (
    "dvs_abi_version", "dvs_ctx_create", "dvs_ctx_destroy", "dvs_last_error", "dvs_ctx_sync",
    "dvs_ctx_trim", "dvs_ctx_device_info", "dvs_ctx_set_timing", "dvs_ctx_refresh_knobs", "dvs_ctx_block_stats", "dvs_matrix_build", "dvs_matrix_from_freqs", "dvs_matrix_from_device_freqs", "dvs_matrix_get_source_rows", "dvs_matrix_count_bytes",
    "dvs_matrix_destroy", "dvs_matrix_nrows", "dvs_matrix_nbins", "dvs_matrix_dev_counts",
    "dvs_matrix_dev_totals", "dvs_matrix_dev_entropy", "dvs_matrix_get_counts",
    "dvs_matrix_get_totals", "dvs_matrix_get_entropy", "dvs_kmer_counts", "dvs_select_run",
    "dvs_select_destroy", "dvs_select_get_summary", "dvs_select_get_members",
    "dvs_select_gather_members",
    "dvs_select_delta_jsd", "dvs_select_step_pack",
    "dvs_select_step_apply", "dvs_select_step_poll", "dvs_select_step_peek", "dvs_select_bench_scan", "dvs_selftest_fast_log2", "dvs_selftest_log2_acc", "dvs_selftest_log2_f32", "dvs_selftest_exact_div", "dvs_selftest_handover", "dvs_mash_sketch", "dvs_mash_distances", "dvs_sketches_build", "dvs_sketches_destroy", "dvs_sketches_get", "dvs_sketches_dev", "dvs_sketches_dev_lens", "dvs_sketches_distances",
    "dvs_sketches_from_device", "dvs_sketches_copy_to_device", "dvs_sketches_distances_device",
    "dvs_default_alphabet_lut", "dvs_seqbatch_from_fasta", "dvs_seqbatch_destroy", "dvs_seqbatch_info",
    "dvs_seqbatch_offsets", "dvs_seqbatch_header_positions", "dvs_seqbatch_dev_codes", "dvs_seqbatch_get_codes",
    "dvs_pack_sequences", "dvs_packed_destroy", "dvs_packed_info", "dvs_packed_dev_codes", "dvs_packed_dev_mask",
    "dvs_packed_get", "dvs_seqbatch_pack", "dvs_seqbatch_packed",
    "dvs_canonical_bins", "dvs_matrix_fold_canonical", "dvs_matrix_is_canonical",
    "dvs_linkage_cut", "dvs_linkage_cophenet", "dvs_nj_patristic", "dvs_pairs_destroy", "dvs_pairs_info", "dvs_pairs_get",
    # one entry per operation over the distances of a `Source`
    "dvs_distances", "dvs_linkage", "dvs_nj", "dvs_maxmin", "dvs_cross_distances", "dvs_nearest", "dvs_within",
    "dvs_cluster_scores", "dvs_cophenet", "dvs_threshold_clusters", "dvs_pcoa", "dvs_pcoa_project", "dvs_kmedoids",
    "dvs_mst", "dvs_linkage_from_mst", "dvs_permanova", "dvs_mantel",
)
WITHIN_SKIP_SELF = 1
SRC_MASH, SRC_EUCLIDEAN, SRC_JSD, SRC_GIVEN = range(4)
SEQ_HOST, SEQ_DEVICE, SEQ_PACKED, SEQ_BATCH = range(4)


class Source(C.Structure):
    """dvs_source: where an operation's distances come from"""
    _fields_ = [("kind", C.c_uint32), ("handle", C.c_void_p), ("rows", C.POINTER(C.c_uint32)), ("n", C.c_uint32),
                ("k", C.c_uint32), ("sketch_size", C.c_uint32), ("on_device", C.c_int)]


class Seqs(C.Structure):
    """dvs_seqs: where a build's sequences come from"""
    _fields_ = [("kind", C.c_uint32), ("handle", C.c_void_p), ("offsets", C.POINTER(C.c_uint64)), ("nseq", C.c_uint32)]


def make_seqs(kind: int, handle, offsets: np.ndarray | None = None, keep=None) -> Seqs:
    """the dvs_seqs of one build: `kind` (SEQ_*), the pointer or handle and, except for SEQ_BATCH, the nseq + 1 offsets
    (made contiguous uint64 here).  The offsets array and `keep`, the owner of the bytes, live as long as the structure"""
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    seqs = Seqs(kind, handle, ptr(offsets, C.c_uint64), 0 if offsets is None else offsets.size - 1)
    seqs._keep = (handle, offsets, keep)
    return seqs


class PcoaParams(C.Structure):
    """dvs_pcoa_params"""
    _fields_ = [("n_axes", C.c_uint32), ("max_basis", C.c_uint32), ("tol", C.c_double)]


class PcoaInfo(C.Structure):
    """dvs_pcoa_info"""
    _fields_ = [("trace", C.c_double), ("converged", C.c_uint32), ("basis", C.c_uint32), ("steps", C.c_uint32),
                ("products", C.c_uint64)]


class KmedoidsParams(C.Structure):
    """dvs_kmedoids_params"""
    _fields_ = [("k", C.c_uint32), ("init", C.c_uint32), ("max_swaps", C.c_uint32), ("flags", C.c_uint32)]


class KmedoidsInfo(C.Structure):
    """dvs_kmedoids_info"""
    _fields_ = [("td_init", C.c_double), ("td", C.c_double), ("n_swaps", C.c_uint32), ("stop", C.c_uint32),
                ("passes", C.c_uint32)]


KMEDOIDS_INIT_BUILD, KMEDOIDS_INIT_GIVEN = 0, 1


class PermanovaInfo(C.Structure):
    """dvs_permanova_info"""
    _fields_ = [("n_le", C.c_uint32), ("passes", C.c_uint32), ("batch", C.c_uint32)]


class MantelInfo(C.Structure):
    """dvs_mantel_info"""
    _fields_ = [("n_ge", C.c_uint32), ("n_le", C.c_uint32), ("n_abs_ge", C.c_uint32), ("passes", C.c_uint32),
                ("batch", C.c_uint32)]


class SelectParams(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("n_seed", C.c_uint32), ("max_size", C.c_uint32),
                ("stat", C.c_uint32), ("window", C.c_uint32), ("flags", C.c_uint32)]


class SelectSummary(C.Structure):
    _fields_ = [("size", C.c_uint32), ("lowest_index", C.c_uint32),
                ("total_jsd", C.c_double), ("mean_delta_jsd", C.c_double),
                ("std_delta_jsd", C.c_double), ("cov_delta_jsd", C.c_double),
                ("summed_entropies", C.c_double),
                ("rows_scored", C.c_uint64), ("rows_rechecked", C.c_uint64),
                ("n_windows", C.c_uint32), ("n_events", C.c_uint32),
                ("n_accepts", C.c_uint32), ("n_arbitrated", C.c_uint32),
                ("scan_ms", C.c_double), ("scan_launches", C.c_uint64),
                ("engine", C.c_uint32), ("rows_coarse_passed", C.c_uint32),
                ("scan_ms_last", C.c_double), ("rows_scored_last", C.c_uint64), ("arbiter_ms", C.c_double)]


class DvsLibraryMissing(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


def _preload_torch_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so.7 / libhsa-runtime64 (same SONAMEs as /opt/rocm's); if this
    library pulled in the system copy first, a later `import torch` would find no
    GPU, and device pointers could not be shared between the two.  So when torch
    is installed, its copy is loaded (RTLD_GLOBAL) before libdvs_hip.so, whose
    NEEDED libamdhip64.so.7 then resolves to it.  torch itself is not imported."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return  # already loaded its runtime
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = pathlib.Path(list(spec.submodule_search_locations)[0]) / "lib"
    for name in ("libhsa-runtime64.so", "libamd_comgr.so", "libamdhip64.so"):
        p = libdir / name
        if p.exists():
            try:
                C.CDLL(str(p), mode=C.RTLD_GLOBAL)
            except OSError:
                return


def load() -> C.CDLL:
    """dlopen libdvs_hip.so and declare the ABI; raises if it has not been built"""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not LIB_PATH.exists():
            raise DvsLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _preload_torch_hip_runtime()
        L = C.CDLL(str(LIB_PATH))
        vp, u8p, u32p, u64p, f64p = (C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_double))
        L.dvs_abi_version.restype = C.c_int
        L.dvs_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.dvs_ctx_destroy.argtypes = [vp]
        L.dvs_ctx_destroy.restype = None
        L.dvs_last_error.argtypes = [vp]
        L.dvs_last_error.restype = C.c_char_p
        L.dvs_ctx_sync.argtypes = [vp]
        L.dvs_ctx_trim.argtypes = [vp]
        L.dvs_ctx_set_timing.argtypes = [vp, C.c_int]
        L.dvs_ctx_refresh_knobs.argtypes = [vp]
        L.dvs_ctx_block_stats.argtypes = [vp, u64p]
        L.dvs_ctx_device_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), u64p]
        L.dvs_matrix_build.argtypes = [vp, C.POINTER(Seqs), C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.dvs_matrix_from_freqs.argtypes = [vp, f64p, C.c_uint32, C.c_uint64, C.POINTER(vp)]
        L.dvs_matrix_from_device_freqs.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.POINTER(vp)]
        L.dvs_select_gather_members.argtypes = [vp, vp, vp, vp, C.c_uint32]
        L.dvs_matrix_destroy.argtypes = [vp]
        L.dvs_matrix_destroy.restype = None
        L.dvs_matrix_nrows.argtypes = [vp]
        L.dvs_matrix_nrows.restype = C.c_uint32
        L.dvs_matrix_nbins.argtypes = [vp]
        L.dvs_matrix_nbins.restype = C.c_uint64
        for n in ("dvs_matrix_dev_counts", "dvs_matrix_dev_totals", "dvs_matrix_dev_entropy"):
            getattr(L, n).argtypes = [vp]
            getattr(L, n).restype = vp
        L.dvs_matrix_get_counts.argtypes = [vp, vp, C.c_uint32, C.c_uint32, u32p]
        L.dvs_matrix_get_totals.argtypes = [vp, vp, u32p]
        L.dvs_matrix_get_entropy.argtypes = [vp, vp, f64p]
        L.dvs_matrix_get_source_rows.argtypes = [vp, vp, u32p]
        L.dvs_matrix_count_bytes.argtypes = [vp]
        L.dvs_matrix_count_bytes.restype = C.c_uint32
        L.dvs_kmer_counts.argtypes = [vp, u8p, u64p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p,
                                      f64p]
        L.dvs_select_run.argtypes = [vp, vp, u32p, u32p, C.c_uint64, C.POINTER(SelectParams),
                                     C.POINTER(vp)]
        L.dvs_select_destroy.argtypes = [vp]
        L.dvs_select_destroy.restype = None
        L.dvs_select_get_summary.argtypes = [vp, vp, C.POINTER(SelectSummary)]
        L.dvs_select_get_members.argtypes = [vp, vp, u64p, u32p, f64p, f64p, f64p]
        L.dvs_select_delta_jsd.argtypes = [vp, vp, vp, u32p, f64p]
        L.dvs_select_step_pack.argtypes = [vp, vp, vp]
        L.dvs_select_step_apply.argtypes = [vp, vp, vp, C.c_uint32]
        L.dvs_select_step_poll.argtypes = [vp, vp, u32p, u64p]
        L.dvs_select_step_peek.argtypes = [vp, vp, C.c_uint32, u32p, C.POINTER(C.c_int)]
        L.dvs_select_bench_scan.argtypes = [vp, vp, C.c_int, f64p, u64p]
        L.dvs_selftest_fast_log2.argtypes = [vp, f64p]
        L.dvs_selftest_log2_acc.argtypes = [vp, f64p]
        L.dvs_selftest_log2_f32.argtypes = [vp, f64p]
        L.dvs_selftest_exact_div.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.dvs_selftest_handover.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64)]
        L.dvs_mash_sketch.argtypes = [vp, vp, C.c_int, u64p, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_int, u32p, u32p]
        L.dvs_mash_distances.argtypes = [vp, u32p, C.c_uint32, u32p, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, f64p]
        L.dvs_sketches_build.argtypes = [vp, C.POINTER(Seqs), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(vp)]
        L.dvs_sketches_destroy.argtypes = [vp]
        L.dvs_sketches_destroy.restype = None
        L.dvs_sketches_get.argtypes = [vp, vp, u32p, u32p]
        for n in ("dvs_sketches_dev", "dvs_sketches_dev_lens"):
            getattr(L, n).argtypes = [vp]
            getattr(L, n).restype = vp
        L.dvs_sketches_distances.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, f64p]
        L.dvs_sketches_from_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.dvs_sketches_copy_to_device.argtypes = [vp, vp, vp, C.c_uint32, vp]
        L.dvs_sketches_distances_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp]
        L.dvs_default_alphabet_lut.argtypes = [C.c_int, u8p]
        L.dvs_default_alphabet_lut.restype = None
        L.dvs_seqbatch_from_fasta.argtypes = [vp, vp, C.c_int, C.c_uint64, u8p, C.c_int, C.POINTER(vp)]
        L.dvs_seqbatch_destroy.argtypes = [vp]
        L.dvs_seqbatch_destroy.restype = None
        L.dvs_seqbatch_info.argtypes = [vp, u32p, u64p, u32p]
        L.dvs_seqbatch_offsets.argtypes = [vp, u64p]
        L.dvs_seqbatch_header_positions.argtypes = [vp, u64p]
        L.dvs_seqbatch_dev_codes.argtypes = [vp]
        L.dvs_seqbatch_dev_codes.restype = vp
        L.dvs_seqbatch_get_codes.argtypes = [vp, vp, u8p]
        L.dvs_pack_sequences.argtypes = [vp, vp, C.c_int, C.c_uint64, C.POINTER(vp)]
        L.dvs_packed_destroy.argtypes = [vp]
        L.dvs_packed_destroy.restype = None
        L.dvs_packed_info.argtypes = [vp, u64p, u64p]
        for n in ("dvs_packed_dev_codes", "dvs_packed_dev_mask", "dvs_seqbatch_packed"):
            getattr(L, n).argtypes = [vp]
            getattr(L, n).restype = vp
        L.dvs_packed_get.argtypes = [vp, vp, u32p, C.POINTER(C.c_uint16)]
        L.dvs_seqbatch_pack.argtypes = [vp, vp]
        u32, srcp = C.c_uint32, C.POINTER(Source)
        L.dvs_linkage_cut.argtypes = [vp, u32, u32p, f64p, C.c_int, C.c_double, u32p, u32p]
        L.dvs_linkage_cophenet.argtypes = [vp, u32, u32p, f64p, f64p]
        L.dvs_nj_patristic.argtypes = [vp, u32, u32p, f64p, f64p]
        L.dvs_canonical_bins.argtypes = [u32, u32p, u64p]
        L.dvs_matrix_fold_canonical.argtypes = [vp, vp, C.POINTER(vp)]
        L.dvs_matrix_is_canonical.argtypes = [vp]
        L.dvs_matrix_is_canonical.restype = C.c_uint32
        L.dvs_pairs_destroy.argtypes = [vp]
        L.dvs_pairs_destroy.restype = None
        L.dvs_pairs_info.argtypes = [vp, u32p, u64p]
        L.dvs_pairs_get.argtypes = [vp, u64p, u32p, f64p]
        # the operations over the distances of a source (or of two): the context, the source(s), the operation's own
        L.dvs_distances.argtypes = [vp, srcp, f64p]
        L.dvs_linkage.argtypes = [vp, srcp, C.c_int, u32p, f64p, u32p]  # method, pairs, heights, sizes
        L.dvs_nj.argtypes = [vp, srcp, u32p, f64p]  # joins, lengths
        # seeds, n_seeds, n_select, use_min_distance, min_distance, picks, radius, n_picked, owner, dist_to_owner, cover
        L.dvs_maxmin.argtypes = [vp, srcp, u32p, u32, u32, C.c_int, C.c_double, u32p, f64p, u32p, u32p, f64p, f64p]
        L.dvs_cross_distances.argtypes = [vp, srcp, srcp, f64p]
        L.dvs_nearest.argtypes = [vp, srcp, srcp, u32, u32p, f64p]  # kk, idx, dist
        L.dvs_within.argtypes = [vp, srcp, srcp, C.c_double, u32, C.c_uint64, C.POINTER(vp)]  # radius, flags, max_pairs, the dvs_pairs
        # labels, n_clusters, the five per-row outputs, medoids
        L.dvs_cluster_scores.argtypes = [vp, srcp, u32p, u32, f64p, f64p, f64p, u32p, f64p, u32p]
        L.dvs_cophenet.argtypes = [vp, srcp, u32p, f64p, f64p, f64p, f64p]  # pairs, heights, the correlation, the row sums, the matrix
        L.dvs_threshold_clusters.argtypes = [vp, srcp, C.c_double, u32p, u32p]  # radius, labels, n_clusters
        # params, values, vectors, residuals, row_means, info
        L.dvs_pcoa.argtypes = [vp, srcp, C.POINTER(PcoaParams), f64p, f64p, f64p, f64p, C.POINTER(PcoaInfo)]
        L.dvs_pcoa_project.argtypes = [vp, srcp, srcp, u32, f64p, f64p, f64p, f64p]  # n_axes, values, vectors, row_means, coords
        # params, medoids, labels, dist, second, swaps, td, info
        L.dvs_kmedoids.argtypes = [vp, srcp, C.POINTER(KmedoidsParams), u32p, u32p, f64p, f64p, u32p, f64p,
                                   C.POINTER(KmedoidsInfo)]
        L.dvs_mst.argtypes = [vp, srcp, f64p, u32p, f64p, u32p, u32p]  # core, edges, weights, n_edges, n_rounds
        L.dvs_linkage_from_mst.argtypes = [vp, u32, u32p, f64p, u32p, f64p, u32p]  # edges, weights, pairs, heights, sizes
        # labels, n_groups, perm_labels, n_perm, ss_total, ss_within, group_ss, info
        L.dvs_permanova.argtypes = [vp, srcp, u32p, u32, u32p, u32, f64p, f64p, f64p, C.POINTER(PermanovaInfo)]
        # the two sources, perms, n_perm, moments, z, info
        L.dvs_mantel.argtypes = [vp, srcp, srcp, u32p, u32, f64p, f64p, C.POINTER(MantelInfo)]
        if L.dvs_abi_version() != 5:
            raise RuntimeError("libdvs_hip.so ABI version mismatch")
        _lib = L
        return _lib


def ptr(a: np.ndarray | None, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def raise_for(rc: int, ctx) -> None:
    """map a DVS_ERR_* code to the exception the reference's binding raises"""
    if rc == OK:
        return
    msg = (load().dvs_last_error(ctx) or b"").decode(errors="replace")
    if rc == ERR_VALUE:
        raise ValueError(msg)  # panic -> ValueError, src/lib.rs:36-57
    if rc == ERR_NOMEM:
        raise MemoryError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == ERR_ZERODIV:
        raise ZeroDivisionError(msg)
    raise RuntimeError(msg)
