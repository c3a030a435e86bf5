"""ctypes binding of include/fedrann_hip.h (libfedrann_hip.so).

No fallback: if the library is missing or no GPU is visible, FedrannHipError is raised.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FEDRANN_HIP_LIB") or os.path.join(HERE, "libfedrann_hip.so")  # env: dev A/B builds

# symbols declared in include/fedrann_hip.h (tests check that the library exports every one)
SYMBOLS = (
    "fdr_create", "fdr_destroy", "fdr_last_error", "fdr_device_info", "fdr_padded_dim",
    "fdr_projection_load", "fdr_embed", "fdr_knn", "fdr_embed_knn", "fdr_embed_dev",
    "fdr_normalize_dev", "fdr_knn_workspace_bytes", "fdr_knn_dev", "fdr_timing", "fdr_timing_read",
    "fdr_last_uncertified", "fdr_set_knn_mode", "fdr_set_dedup_mode", "fdr_last_unique", "fdr_kmer_output_scan",
    "fdr_kmer_output_load", "fdr_kmer_search", "fdr_kmer_search_indices", "fdr_kmer_count",
    "fdr_kmer_count_fetch", "fdr_set_kmer_count_block", "fdr_last_kmer_count_blocks", "fdr_csr_compact", "fdr_host_register", "fdr_host_unregister",
    "fdr_overlaps_write", "fdr_last_prefilter_launches", "fdr_knn_classes_dev", "fdr_knn_unique_dev",
    "fdr_knn_expand_dev", "fdr_kmer_output_scan_range", "fdr_kmer_output_load_range",
    "fdr_kmer_count_begin", "fdr_kmer_count_add", "fdr_kmer_count_finish", "fdr_reads_scan", "fdr_reads_parse",
    "fdr_kmer_output_append", "fdr_last_query_paths", "fdr_last_knn_trace", "fdr_kmer_count_export_dev",
    "fdr_kmer_count_merge_dev", "fdr_kmer_count_merge", "fdr_set_knn_capture", "fdr_last_candidates",
    "fdr_last_range_sets", "fdr_knn_sparse", "fdr_set_live_chunks", "fdr_knn_sparse_metric",
    "fdr_set_live_skip", "fdr_last_live_stage_lists", "fdr_set_rerank_compact", "fdr_set_pass_tail",
    "fdr_sparse_index_build", "fdr_sparse_index_search", "fdr_sparse_index_info", "fdr_sparse_index_free",
    "fdr_sparse_index_query", "fdr_topk_merge", "fdr_radius_merge", "fdr_sparse_index_radius_search", "fdr_sparse_index_radius_query",
    "fdr_sparse_index_radius_fetch", "fdr_overlaps_write_csr",
    "fdr_dense_index_build", "fdr_dense_index_embed", "fdr_dense_index_radius_search", "fdr_dense_index_radius_query",
    "fdr_dense_index_radius_fetch", "fdr_dense_index_info", "fdr_dense_index_free", "fdr_sparse_rescore",
    "fdr_rescore_rows_build", "fdr_rescore_rows_info", "fdr_rescore_rows_free", "fdr_rescore_rows_knn",
    "fdr_rescore_rows_radius", "fdr_rescore_rows_radius_fetch",
    "fdr_graph_symmetrize", "fdr_graph_symmetrize_fetch", "fdr_graph_free", "fdr_graph_components",
    "fdr_graph_expand", "fdr_graph_expand_fetch", "fdr_rescore_rows_refine",
)
FDR_FAST_MAX_DIM = 512  # the reach of the fp16 passes, and so of the dense index (csrc/knn_plan.inc)
FDR_MAX_K = 128
FDR_E_ARG, FDR_E_HIP, FDR_E_NOMEM, FDR_E_STATE, FDR_E_IO = -1, -2, -4, -5, -6  # include/fedrann_hip.h: FDR_E_*
KERNELS = ("embed_csr", "normalize_rows", "knn_tile", "knn_merge", "knn_prefilter", "knn_rerank",
           "knn_dedup", "kmer_search", "kmer_compact")
FDR_MAX_DIM = 2048
TOPK_MERGE_MAX_PARTS = 64  # fdr_topk_merge: one lane of a wave per part
FDR_RESCORE_TILE = 512  # fdr_sparse_rescore: stored entries of a query row staged at once (include/fedrann_hip.h)
# fdr_last_query_paths codes (include/fedrann_hip.h: FDR_PATH_*)
PATH_CERTIFIED, PATH_RANGE, PATH_EXACT, PATH_ZERO, PATH_RANGE_OVERFLOW, PATH_GENERIC, PATH_CLASS_MEMBER = 1, 2, 3, 4, 5, 6, 0x80
# fdr_last_knn_trace (include/fedrann_hip.h: FDR_TRACE_*, FDR_FALLBACK_*)
TRACE_KINDS = ("none", "exact", "prefilter", "generic", "sparse")
FALLBACKS = ("none", "chunked", "whole")
# fdr_set_knn_capture (include/fedrann_hip.h: FDR_CAPTURE_*, FDR_RANGE_CAP)
CAPTURE_CANDIDATES, CAPTURE_RANGE, CAPTURE_LIVE_LISTS = 1, 2, 4
RANGE_CAP = 1024
# fdr_knn_sparse_metric (include/fedrann_hip.h: FDR_METRIC_*)
METRIC_COSINE, METRIC_JACCARD, METRIC_WEIGHTED_JACCARD = 0, 1, 2
SPARSE_METRICS = {"cosine": METRIC_COSINE, "jaccard": METRIC_JACCARD, "weighted_jaccard": METRIC_WEIGHTED_JACCARD}


class KnnTrace(ctypes.Structure):
    """struct fdr_knn_trace (include/fedrann_hip.h), field for field."""
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "dp", "k", "kp")] + \
        [(n, ctypes.c_int64) for n in ("queries", "targets")] + \
        [(n, ctypes.c_int32) for n in (
            "pass_waves", "pass_wps", "pass_units", "pass_list_keys", "pass_pingpong", "pass_launches", "pass_queues",
            "pass_segments", "uncertified", "zero_queries", "range_queries", "range_chunks", "range_pp_chunks",
            "range_w8_chunks", "range_overflow", "exact_fallback", "exact_calls", "exact_queries", "exact_waves",
            "exact_qsets", "generic", "exact_segments", "pass_live", "pass_live_items_2", "pass_live_items_3",
            "pass_live_items_4", "pass_live_items_5", "pass_live_items_6", "pass_live_dense_items", "skip_live")] + \
        [(n, ctypes.c_int64) for n in ("skip_stages_walked", "skip_stages_skipped", "rerank_compact_long")] + \
        [(n, ctypes.c_int32) for n in ("rerank_compact", "rerank_compact_entries", "pass_group_order",
                                       "rerank_early_queries")]


class FedrannHipError(RuntimeError):
    pass


_lib = None


def _share_torch_hip_runtime():
    """One HIP / HSA runtime per process.  A PyTorch-ROCm wheel bundles its own libamdhip64.so.7; if
    libfedrann_hip.so were loaded first it would pull in /opt/rocm's copy, and torch (imported later,
    e.g. by fedrann_amd.distributed) would start a second runtime that sees no GPU.  So map torch's copy
    first -- located without importing torch -- and let the dynamic linker resolve our DT_NEEDED
    libamdhip64.so.7 to it (same SONAME).  FEDRANN_HIP_SYSTEM_RUNTIME=1 keeps the system runtime."""
    if os.environ.get("FEDRANN_HIP_SYSTEM_RUNTIME") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except (OSError, ImportError, ValueError):
        pass  # no torch, or an unloadable copy: the system runtime is used


def load_library():
    """dlopen libfedrann_hip.so and declare the prototypes.  Needs no GPU."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FedrannHipError(
            "%s is missing: build it with `python -m fedrann_amd.build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    _share_torch_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    i32, i64, vp, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    L.fdr_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.fdr_destroy.argtypes = [vp]
    L.fdr_last_error.argtypes = []
    L.fdr_last_error.restype = ctypes.c_char_p
    L.fdr_device_info.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
    L.fdr_padded_dim.argtypes = [ctypes.c_int]
    L.fdr_projection_load.argtypes = [vp, i64, i32, vp, vp, vp]
    L.fdr_embed.argtypes = [vp, i64, vp, vp, vp]
    L.fdr_knn.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    L.fdr_embed_knn.argtypes = [vp, i64, vp, vp, i32, vp, vp, vp]
    L.fdr_knn_sparse.argtypes = [vp, i64, i64, vp, vp, vp, i32, vp, vp]
    L.fdr_knn_sparse_metric.argtypes = [vp, i32, i64, i64, vp, vp, vp, i32, vp, vp]
    L.fdr_sparse_index_build.argtypes = [vp, i32, i64, i64, vp, vp, vp]
    L.fdr_sparse_index_search.argtypes = [vp, i32, i64, i64, vp, vp]
    L.fdr_sparse_index_query.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp]
    L.fdr_sparse_index_radius_search.argtypes = [vp, ctypes.c_float, i64, i64, i64, vp]
    L.fdr_sparse_index_radius_query.argtypes = [vp, ctypes.c_float, i64, vp, vp, vp, i64, vp]
    L.fdr_sparse_index_radius_fetch.argtypes = [vp, i64, vp, vp]
    L.fdr_sparse_index_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i64),
                                        ctypes.POINTER(i64), ctypes.POINTER(sz)]
    L.fdr_sparse_index_free.argtypes = [vp]
    L.fdr_dense_index_build.argtypes = [vp, vp, i64, i32]
    L.fdr_dense_index_embed.argtypes = [vp, i64, vp, vp]
    L.fdr_dense_index_radius_search.argtypes = [vp, ctypes.c_float, i64, i64, i64, vp]
    L.fdr_dense_index_radius_query.argtypes = [vp, ctypes.c_float, i64, vp, i64, vp]
    L.fdr_dense_index_radius_fetch.argtypes = [vp, i64, vp, vp]
    L.fdr_dense_index_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(sz),
                                       ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                       ctypes.POINTER(i32)]
    L.fdr_dense_index_free.argtypes = [vp]
    L.fdr_topk_merge.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp, vp]
    L.fdr_radius_merge.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp]
    L.fdr_graph_symmetrize.argtypes = [vp, i32, i64, vp, vp, vp, i64, vp]
    L.fdr_graph_symmetrize_fetch.argtypes = [vp, i64, vp, vp]
    L.fdr_graph_free.argtypes = [vp]
    L.fdr_graph_components.argtypes = [vp, i32, i64, vp, vp, vp, ctypes.c_float, vp, vp, vp]
    L.fdr_graph_expand.argtypes = [vp, i64, vp, vp, vp, i32, i64, i64, i64, vp]
    L.fdr_graph_expand_fetch.argtypes = [vp, i64, vp]
    L.fdr_rescore_rows_refine.argtypes = [vp, ctypes.c_float, i32, vp]
    L.fdr_sparse_rescore.argtypes = [vp, i32, i64, i64, vp, vp, vp, i64, i64, i32, vp, i32, vp, vp]
    L.fdr_rescore_rows_build.argtypes = [vp, i32, i64, i64, vp, vp, vp]
    L.fdr_rescore_rows_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i64),
                                        ctypes.POINTER(sz)]
    L.fdr_rescore_rows_free.argtypes = [vp]
    L.fdr_rescore_rows_knn.argtypes = [vp, i64, i64, i32, vp, i32, vp, vp]
    L.fdr_rescore_rows_radius.argtypes = [vp, ctypes.c_float, i64, i64, vp, vp, vp]
    L.fdr_rescore_rows_radius_fetch.argtypes = [vp, i64, vp, vp]
    L.fdr_embed_dev.argtypes = [vp, i64, vp, vp, vp, vp]
    L.fdr_normalize_dev.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    L.fdr_knn_workspace_bytes.argtypes = [vp, i64, i64, i32, i32]
    L.fdr_knn_workspace_bytes.restype = sz
    L.fdr_knn_dev.argtypes = [vp, vp, vp, i64, vp, vp, i64, i64, i32, i32, vp, vp, vp, sz, vp]
    L.fdr_knn_classes_dev.argtypes = [vp, vp, vp, i64, i32, i32, i64, vp, sz, vp, ctypes.POINTER(i32)]
    L.fdr_knn_unique_dev.argtypes = [vp, i64, i64, vp, vp, vp]
    L.fdr_knn_expand_dev.argtypes = [vp, i64, i64, i64, vp, vp, i64, vp, vp, vp]
    L.fdr_last_uncertified.argtypes = [vp]
    L.fdr_last_query_paths.argtypes = [vp, vp, i64]
    L.fdr_last_knn_trace.argtypes = [vp, ctypes.POINTER(KnnTrace)]
    L.fdr_set_knn_mode.argtypes = [vp, ctypes.c_int]
    L.fdr_set_knn_capture.argtypes = [vp, ctypes.c_int]
    L.fdr_last_candidates.argtypes = [vp, vp, i64, i32, ctypes.POINTER(i32)]
    L.fdr_last_range_sets.argtypes = [vp, i64, vp, vp, vp, vp]
    L.fdr_set_dedup_mode.argtypes = [vp, ctypes.c_int]
    L.fdr_set_live_chunks.argtypes = [vp, ctypes.c_int]
    L.fdr_set_live_skip.argtypes = [vp, ctypes.c_int]
    L.fdr_set_pass_tail.argtypes = [vp, ctypes.c_int]
    L.fdr_set_rerank_compact.argtypes = [vp, ctypes.c_int]
    L.fdr_last_live_stage_lists.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), vp, vp]
    L.fdr_last_unique.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.fdr_last_prefilter_launches.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    p64 = ctypes.POINTER(ctypes.c_int64)
    L.fdr_kmer_output_scan.argtypes = [ctypes.c_char_p, p64, p64, p64]
    L.fdr_kmer_output_load.argtypes = [ctypes.c_char_p, i64, i32, i64, i64, i64, vp, vp, vp, vp]
    L.fdr_kmer_output_scan_range.argtypes = [ctypes.c_char_p, i64, i64, p64, p64, p64]
    L.fdr_kmer_output_load_range.argtypes = [ctypes.c_char_p, i64, i32, i64, i64, i64, i64, i64, vp, vp, vp, vp]
    L.fdr_kmer_output_append.argtypes = [ctypes.c_char_p, i64, vp, vp, vp, vp]
    L.fdr_reads_scan.argtypes = [vp, i64, i32, i32, i32, p64, p64, p64]
    L.fdr_reads_parse.argtypes = [vp, i64, i32, i32, i64, i64, vp, vp, vp]
    L.fdr_csr_compact.argtypes = [vp, i64, vp, vp, vp, vp, i64, i32]
    L.fdr_host_register.argtypes = [vp, vp, sz]
    L.fdr_host_unregister.argtypes = [vp, vp]
    L.fdr_overlaps_write.argtypes = [ctypes.c_char_p, i32, i32, i64, i64, i64, i32, vp, vp, vp, vp, vp, i32, p64]
    L.fdr_kmer_search.argtypes = [vp, vp, vp, i64, vp, i64, i32, vp, p64]
    L.fdr_overlaps_write_csr.argtypes = [ctypes.c_char_p, i32, i32, i64, i64, i64, vp, vp, vp, vp, vp, vp, i32, p64]
    L.fdr_kmer_search_indices.argtypes = [vp, vp]
    L.fdr_kmer_count.argtypes = [vp, vp, vp, i64, i32, i64, p64]
    L.fdr_kmer_count_fetch.argtypes = [vp, vp, vp]
    L.fdr_kmer_count_begin.argtypes = [vp, i32]
    L.fdr_kmer_count_add.argtypes = [vp, vp, vp, i64]
    L.fdr_kmer_count_finish.argtypes = [vp, i64, p64]
    L.fdr_set_kmer_count_block.argtypes = [vp, ctypes.c_int64]
    L.fdr_last_kmer_count_blocks.argtypes = [vp]
    L.fdr_kmer_count_export_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.fdr_kmer_count_merge_dev.argtypes = [vp, i32, vp, vp, vp, i64, p64, vp]
    L.fdr_kmer_count_merge.argtypes = [vp, i32, vp, vp, vp, i64, p64]
    L.fdr_timing.argtypes = [vp, ctypes.c_int]
    L.fdr_timing_read.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_float)]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if name not in ("fdr_last_error", "fdr_knn_workspace_bytes"):
            fn.restype = ctypes.c_int
    _lib = L
    return L


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _as(a, dtype, name):
    b = np.ascontiguousarray(a, dtype=dtype)
    if b.dtype != np.dtype(dtype):
        raise TypeError("%s must be %s" % (name, np.dtype(dtype)))
    return b


def kmer_output_load(path, n_features, n_threads=0):
    """output.bin -> (indptr int64 [2R+1], indices int32 ascending per row, name_off int64 [R+1],
    names uint8 buffer) through fdr_kmer_output_scan / fdr_kmer_output_load (host only, no GPU)."""
    L = load_library()
    bpath = os.fsencode(path)
    R, nnz, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = L.fdr_kmer_output_scan(bpath, ctypes.byref(R), ctypes.byref(nnz), ctypes.byref(nb))
    if rc != 0:
        raise FedrannHipError("fdr_kmer_output_scan failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    indptr = np.empty(2 * R.value + 1, dtype=np.int64)
    indices = np.empty(2 * nnz.value, dtype=np.int32)
    name_off = np.empty(R.value + 1, dtype=np.int64)
    names = np.empty(nb.value, dtype=np.uint8)
    rc = L.fdr_kmer_output_load(bpath, int(n_features), int(n_threads), R.value, nnz.value, nb.value,
                                indptr.ctypes.data, indices.ctypes.data, name_off.ctypes.data, names.ctypes.data)
    if rc != 0:
        raise FedrannHipError("fdr_kmer_output_load failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    return indptr, indices, name_off, names


def kmer_output_records(path):
    """Record count of an output.bin from its 16-byte header ('<4sB3sQ', feature_extraction.py:110-119); the
    reference's ValueError for a bad magic / version.  No record is read."""
    import struct
    with open(path, "rb") as f:
        head = f.read(16)
    if len(head) < 16:
        raise ValueError("incomplete file header")
    magic, version, _, total = struct.unpack("<4sB3sQ", head)
    if magic != b"KMER":
        raise ValueError("invalid file format (bad magic)")
    if version != 1:
        raise ValueError("unsupported version: %d" % version)
    return int(total)


def kmer_output_load_range(path, n_features, rec_lo, rec_hi, n_threads=0, with_names=True):
    """Rows of the records [rec_lo, rec_hi) of output.bin (rec_hi = None: to the end) -- a rank's block of a
    row-sharded run -- as (n_records of the file, indptr int64 [2 (hi - lo) + 1] rebased to 0, indices int32,
    name_off, names of ALL records or (None, None))."""
    L = load_library()
    bpath = os.fsencode(path)
    R, nnz, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    total = kmer_output_records(path)  # (the header's count clamps the range; one walk over the records below, not two)
    lo = max(0, min(int(rec_lo), total))
    hi = total if rec_hi is None else max(lo, min(int(rec_hi), total))
    rc = L.fdr_kmer_output_scan_range(bpath, lo, hi, ctypes.byref(R), ctypes.byref(nnz), ctypes.byref(nb))
    if rc != 0:
        raise FedrannHipError("fdr_kmer_output_scan_range failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    indptr = np.empty(2 * (hi - lo) + 1, dtype=np.int64)
    indices = np.empty(2 * nnz.value, dtype=np.int32)
    name_off = np.empty(R.value + 1, dtype=np.int64) if with_names else None
    names = np.empty(nb.value, dtype=np.uint8) if with_names else None
    rc = L.fdr_kmer_output_load_range(bpath, int(n_features), int(n_threads), R.value, lo, hi, nnz.value, nb.value,
                                      indptr.ctypes.data, indices.ctypes.data,
                                      name_off.ctypes.data if with_names else None,
                                      names.ctypes.data if with_names and names.size else None)
    if rc != 0:
        raise FedrannHipError("fdr_kmer_output_load_range failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    return R.value, indptr, indices, name_off, names


def reads_parse(buf, n, is_fastq, fastq_ids_as_fasta, eof, seq_buf=None):
    """Whole records in buf[:n] (uint8 array: the tail of the previous piece of a FASTA / FASTQ file + new bytes)
    -> (consumed bytes, ids list of bytes, seqs uint8, seq_off int64 [R + 1]) through fdr_reads_scan /
    fdr_reads_parse (host only, no GPU).  seq_buf: a uint8 array of at least n bytes to hold the sequences (seqs is
    then a view of it) instead of a fresh one."""
    L = load_library()
    used, R, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    base = buf.ctypes.data if n else None
    rc = L.fdr_reads_scan(base, int(n), int(bool(is_fastq)), int(bool(fastq_ids_as_fasta)), int(bool(eof)),
                          ctypes.byref(used), ctypes.byref(R), ctypes.byref(nb))
    if rc != 0:
        raise FedrannHipError("fdr_reads_scan failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    seqs = np.empty(nb.value, dtype=np.uint8) if seq_buf is None else seq_buf[:nb.value]
    off = np.empty(R.value + 1, dtype=np.int64)
    span = np.empty(2 * R.value, dtype=np.int64)
    rc = L.fdr_reads_parse(base, used.value, int(bool(is_fastq)), int(bool(fastq_ids_as_fasta)), R.value, nb.value,
                           seqs.ctypes.data if nb.value else None, off.ctypes.data, span.ctypes.data if R.value else None)
    if rc != 0:
        raise FedrannHipError("fdr_reads_parse failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    view = memoryview(buf)
    sp = span.tolist()
    ids = [bytes(view[sp[2 * r]:sp[2 * r + 1]]) for r in range(R.value)]
    return used.value, ids, seqs, off


def reads_consumed(buf, n, is_fastq, fastq_ids_as_fasta, eof):
    """Bytes of buf[:n] that hold whole records only (fdr_reads_scan without the parse; host only)."""
    L = load_library()
    used, R, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = L.fdr_reads_scan(buf.ctypes.data if n else None, int(n), int(bool(is_fastq)), int(bool(fastq_ids_as_fasta)),
                          int(bool(eof)), ctypes.byref(used), ctypes.byref(R), ctypes.byref(nb))
    if rc != 0:
        raise FedrannHipError("fdr_reads_scan failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    return used.value


def kmer_output_append(path, ids, indptr, indices):
    """Records of output.bin appended to `path` (fdr_kmer_output_append; host only).  ids: list of bytes."""
    L = load_library()
    name_off, names = pack_names(ids)
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    if indptr.size != len(ids) + 1:
        raise ValueError("indptr must have one entry per record + 1")
    rc = L.fdr_kmer_output_append(os.fsencode(path), len(ids), _ptr(name_off), _ptr(names) if names.size else None,
                                  _ptr(indptr), _ptr(indices) if indices.size else None)
    if rc != 0:
        msg = L.fdr_last_error().decode()
        if "non-ASCII" in msg or "bytes long" in msg:
            raise ValueError(msg)
        raise FedrannHipError("fdr_kmer_output_append failed (%d): %s" % (rc, msg))


def pack_names(read_names):
    """list of str / bytes -> (name_off int64 [n + 1], names uint8 buffer) for fdr_overlaps_write."""
    enc = [n if isinstance(n, bytes) else str(n).encode("utf-8") for n in read_names]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum([len(b) for b in enc], out=off[1:])
    return off, np.frombuffer(b"".join(enc), dtype=np.uint8)


def overlaps_write(path, idx, dist, name_off, names, strands, row0=0, append=False, header=True, n_threads=0):
    """overlaps.tsv rows of neighbour-graph rows row0 .. row0 + idx.shape[0] (host only, no GPU); returns the
    number of data lines.  strands=None: name_off / names describe the RECORDS of a fwd / rev doubled matrix (row t =
    record t >> 1, strand t & 1).  See fdr_overlaps_write."""
    L = load_library()
    idx = _as(idx, np.int32, "idx")
    dist = _as(dist, np.float32, "dist")
    if idx.ndim != 2 or dist.shape != idx.shape:
        raise ValueError("idx and dist must be [rows, k] arrays of the same shape")
    name_off = _as(name_off, np.int64, "name_off")
    names = np.ascontiguousarray(names, dtype=np.uint8)
    if strands is None:  # doubled rows: one name per RECORD, row t = record t >> 1 on strand t & 1
        n_total = 2 * (name_off.size - 1)
    else:
        strands = np.ascontiguousarray(strands, dtype=np.uint8)
        n_total = name_off.size - 1
        if strands.size != n_total:
            raise ValueError("strands must have one entry per row")
    lines = ctypes.c_int64()
    rc = L.fdr_overlaps_write(os.fsencode(path), 1 if append else 0, 1 if header else 0, n_total, int(row0),
                              idx.shape[0], idx.shape[1], _ptr(idx), _ptr(dist), _ptr(name_off),
                              names.ctypes.data if names.size else None, _ptr(strands) if strands is not None else None,
                              int(n_threads),
                              ctypes.byref(lines))
    if rc != 0:
        raise FedrannHipError("fdr_overlaps_write failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    return int(lines.value)


def overlaps_write_csr(path, indptr, idx, dist, name_off, names, strands, row0=0, append=False, header=True,
                       n_threads=0):
    """overlaps_write for ragged rows (the result of a radius search): row r's entries are idx / dist [indptr[r],
    indptr[r + 1]), indptr int64 [rows + 1]; neighbor_rank is an entry's position in its row.  See
    fdr_overlaps_write_csr.  Host only; returns the number of data lines."""
    L = load_library()
    indptr = _as(indptr, np.int64, "indptr")
    idx = _as(idx, np.int32, "idx")
    dist = _as(dist, np.float32, "dist")
    if indptr.ndim != 1 or indptr.size < 1 or idx.ndim != 1 or dist.shape != idx.shape:
        raise ValueError("indptr must be a [rows + 1] array, idx and dist 1-D arrays of the same length")
    if indptr[0] < 0 or np.any(np.diff(indptr) < 0) or indptr[-1] > idx.size:
        raise ValueError("indptr is not a row pointer of idx")
    name_off = _as(name_off, np.int64, "name_off")
    names = np.ascontiguousarray(names, dtype=np.uint8)
    if strands is None:  # doubled rows: one name per RECORD, row t = record t >> 1 on strand t & 1
        n_total = 2 * (name_off.size - 1)
    else:
        strands = np.ascontiguousarray(strands, dtype=np.uint8)
        n_total = name_off.size - 1
        if strands.size != n_total:
            raise ValueError("strands must have one entry per row")
    lines = ctypes.c_int64()
    rc = L.fdr_overlaps_write_csr(os.fsencode(path), 1 if append else 0, 1 if header else 0, n_total, int(row0),
                                  indptr.size - 1, _ptr(indptr), _ptr(idx), _ptr(dist), _ptr(name_off),
                                  names.ctypes.data if names.size else None,
                                  _ptr(strands) if strands is not None else None, int(n_threads), ctypes.byref(lines))
    if rc != 0:
        raise FedrannHipError("fdr_overlaps_write_csr failed (%d): %s" % (rc, L.fdr_last_error().decode()))
    return int(lines.value)


def _check_radius_cap(radius, max_hits, ranks):
    """What both radius checks ask of (radius, max_hits); `ranks` names the k-NN call that ranks every row instead.
    Returns (radius as float32, max_hits)."""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError("radius must be a number, got %r" % (radius,))
    r = np.float32(radius)
    if not (r >= 0 and r < 1):
        raise ValueError("need 0 <= radius < 1, got %r (every row is within 1 of every query: %s ranks them)"
                         % (radius, ranks))
    if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)) or not 1 <= int(max_hits) < 2 ** 31:
        raise ValueError("max_hits must be an integer in [1, 2^31), got %r" % (max_hits,))
    return r, int(max_hits)


def _check_block_rows(block_rows):
    """block_rows of query() / radius_query(): None (one block) or an integer >= 1."""
    if block_rows is not None and (isinstance(block_rows, bool) or not isinstance(block_rows, (int, np.integer))
                                   or int(block_rows) < 1):
        raise ValueError("block_rows must be an integer >= 1, got %r" % (block_rows,))


def check_sparse_radius(radius, max_hits=1 << 26):
    """The argument checks of SparseIndex.radius_search / radius_query that need no GPU: 0 <= radius < 1 (a real number,
    no NaN) and 1 <= max_hits < 2^31.  Returns (radius as float32, max_hits)."""
    return _check_radius_cap(radius, max_hits, "search(k)")


def check_dense_radius(n, d, radius, lo=0, hi=None, max_hits=1 << 26):
    """The argument checks of DenseIndex.radius_search that need no GPU, for an index of n rows of dimension d:
    1 <= n < 2^31, 1 <= d <= 512 (the reach of the fp16 passes), 0 <= radius < 1 (a real number, no NaN), 0 <= lo <= hi
    <= n (hi=None: n) and 1 <= max_hits < 2^31.  Returns (radius as float32, lo, hi, max_hits)."""
    for name, v in (("n", n), ("d", d), ("lo", lo)) + ((("hi", hi),) if hi is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    n, d = int(n), int(d)
    if not 1 <= n < 2 ** 31:
        raise ValueError("the dense index needs 1 <= n < 2^31 rows, got %d" % n)
    if not 1 <= d <= FDR_FAST_MAX_DIM:
        raise ValueError("the dense index needs 1 <= d <= %d (the reach of the fp16 passes), got %d"
                         % (FDR_FAST_MAX_DIM, d))
    r, max_hits = _check_radius_cap(radius, max_hits, "knn(E, k)")
    lo, hi = int(lo), int(n if hi is None else hi)
    if not 0 <= lo <= hi <= n:
        raise ValueError("need 0 <= lo <= hi <= n = %d, got [%d, %d)" % (n, lo, hi))
    return r, lo, hi, max_hits


def radius_pieces(counts, max_hits):
    """Cut rows with the hit counts `counts` into consecutive pieces whose hits fit max_hits: [(a, b), ...] covering
    [0, len(counts)); None when one row alone exceeds it.  Needs no GPU."""
    pieces, a, acc = [], 0, 0
    for i, c in enumerate(counts):
        c = int(c)
        if c > max_hits:
            return None
        if acc + c > max_hits:
            pieces.append((a, i))
            a, acc = i, 0
        acc += c
    pieces.append((a, len(counts)))
    return pieces


def sparse_metric_code(metric):
    """FDR_METRIC_* of a metric name of Context.knn_sparse; needs no GPU."""
    if not isinstance(metric, str) or metric not in SPARSE_METRICS:
        raise ValueError("metric must be 'cosine', 'jaccard' or 'weighted_jaccard', got %r" % (metric,))
    return SPARSE_METRICS[metric]


def check_sparse_rows(indptr, indices, values, n_features, k, metric="cosine"):
    """The argument checks of Context.knn_sparse (fdr_knn_sparse repeats them on the device); needs no GPU.
    metric="weighted_jaccard" also refuses a negative value and a row whose float32 mass chain is not finite.
    Returns (n, k, n_features)."""
    return _check_sparse(indptr, indices, values, n_features, k, metric)


def check_sparse_csr(indptr, indices, values, n_features, metric="cosine"):
    """The argument checks of Context.sparse_index: those of check_sparse_rows without a k, and at least one row
    (fdr_sparse_index_build repeats them on the device); needs no GPU.  Returns (n, n_features)."""
    n, _, F = _check_sparse(indptr, indices, values, n_features, None, metric)
    return n, F


def check_sparse_search(n, k, lo=0, hi=None):
    """The argument checks of SparseIndex.search on an index of n rows: 1 <= k <= min(FDR_MAX_K, n) and
    0 <= lo <= hi <= n (hi=None: n); needs no GPU.  Returns (k, lo, hi)."""
    for name, v in (("k", k), ("lo", lo), ("hi", hi)):
        if isinstance(v, bool) or not (isinstance(v, (int, np.integer)) or (name == "hi" and v is None)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    k, lo, hi = int(k), int(lo), int(n if hi is None else hi)
    if not 1 <= k <= FDR_MAX_K or k > n:
        raise ValueError("need 1 <= k <= min(%d, n = %d), got k = %d" % (FDR_MAX_K, n, k))
    if not 0 <= lo <= hi <= n:
        raise ValueError("need 0 <= lo <= hi <= n = %d, got [%d, %d)" % (n, lo, hi))
    return k, lo, hi


def check_sparse_queries(n, n_features, metric, indptr, indices, values, k):
    """The argument checks of SparseIndex.query on an index of n rows and n_features columns under `metric`
    (fdr_sparse_index_query repeats them on the device); needs no GPU.  The query CSR is checked as
    check_sparse_rows checks the indexed one (ids in [0, n_features), strictly ascending inside a row; finite values;
    metric="weighted_jaccard": none negative and a finite mass per row), but it may hold any number of rows, none
    included, and empty rows; 1 <= k <= min(FDR_MAX_K, n) as in check_sparse_search.  Returns (nq, k)."""
    sparse_metric_code(metric)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer, got %r" % (k,))
    k = check_sparse_search(int(n), k)[0]
    nq = _check_sparse(indptr, indices, values, n_features, None, metric, min_rows=0)[0]
    if nq > np.iinfo(np.int32).max or indices.size > np.iinfo(np.int32).max:
        raise ValueError("need fewer than 2^31 query rows and stored entries")
    return nq, k


def check_topk_merge(idx_parts, dist_parts, k, out=None):
    """The argument checks of Context.topk_merge (fdr_topk_merge repeats the limits); needs no GPU.  idx_parts int32
    and dist_parts float32, both C-contiguous [n_parts, nq, kp] with 1 <= n_parts <= 64 and 1 <= kp <= FDR_MAX_K;
    1 <= k <= min(FDR_MAX_K, n_parts * kp); fewer than 2^31 queries, candidates per part and results; out, if given,
    C-contiguous (int32 [nq, k], float32 [nq, k]).  What the rows hold (ascending keys, distances >= 0 and not NaN,
    indices >= 0) is checked on the device.  Returns (n_parts, nq, kp, k)."""
    for name, a, dt in (("idx_parts", idx_parts, np.int32), ("dist_parts", dist_parts, np.float32)):
        if not isinstance(a, np.ndarray) or a.dtype != dt:
            raise TypeError("%s must be a numpy %s array" % (name, np.dtype(dt)))
        if a.ndim != 3 or not a.flags.c_contiguous:
            raise ValueError("%s must be a C-contiguous [n_parts, nq, kp] array" % name)
    if idx_parts.shape != dist_parts.shape:
        raise ValueError("idx_parts %s and dist_parts %s differ in shape" % (idx_parts.shape, dist_parts.shape))
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer, got %r" % (k,))
    (n_parts, nq, kp), k = idx_parts.shape, int(k)
    if not 1 <= n_parts <= TOPK_MERGE_MAX_PARTS:
        raise ValueError("need 1 <= n_parts <= %d, got %d" % (TOPK_MERGE_MAX_PARTS, n_parts))
    if not 1 <= kp <= FDR_MAX_K:
        raise ValueError("need 1 <= kp <= %d candidates per part, got %d" % (FDR_MAX_K, kp))
    if not 1 <= k <= FDR_MAX_K or k > n_parts * kp:
        raise ValueError("need 1 <= k <= min(%d, n_parts * kp = %d), got k = %d" % (FDR_MAX_K, n_parts * kp, k))
    if nq * max(kp, k) > np.iinfo(np.int32).max:
        raise ValueError("need fewer than 2^31 candidates per part and results (nq = %d)" % nq)
    if out is not None:
        idx, dist = out
        if not (isinstance(idx, np.ndarray) and isinstance(dist, np.ndarray)) \
                or (idx.shape, dist.shape) != ((nq, k), (nq, k)) or idx.dtype != np.int32 \
                or dist.dtype != np.float32 or not (idx.flags.c_contiguous and dist.flags.c_contiguous):
            raise ValueError("out must be C-contiguous (int32 [nq, k], float32 [nq, k])")
    return n_parts, nq, kp, k


def check_rescore_args(n, candidates, k=None, metric="cosine", q_lo=0, out=None):
    """The argument checks of Context.sparse_rescore beside those of the CSR (fdr_sparse_rescore repeats the limits);
    needs no GPU.  n: the rows of the CSR.  candidates: a C-contiguous numpy int32 [nq, k_in] array with 1 <= k_in <=
    FDR_MAX_K, row r the candidates of query q_lo + r; 0 <= q_lo and q_lo + nq <= n; 1 <= k <= k_in (None: k_in); fewer
    than 2^31 candidates in all; a known metric; out, if given, C-contiguous (int32 [nq, k], float32 [nq, k]).  That
    every candidate is a row in [0, n) is checked on the device.  Returns (nq, k_in, k, q_lo)."""
    sparse_metric_code(metric)
    if not isinstance(candidates, np.ndarray) or candidates.dtype != np.int32:
        raise TypeError("candidates must be a numpy int32 array")
    if candidates.ndim != 2 or not candidates.flags.c_contiguous:
        raise ValueError("candidates must be a C-contiguous [nq, k_in] array")
    for name, v in (("n", n), ("q_lo", q_lo)) + ((("k", k),) if k is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    (nq, k_in), n, q_lo = candidates.shape, int(n), int(q_lo)
    k = k_in if k is None else int(k)
    if not 1 <= k_in <= FDR_MAX_K:
        raise ValueError("need 1 <= k_in <= %d candidates per query, got %d" % (FDR_MAX_K, k_in))
    if not 1 <= k <= k_in:
        raise ValueError("need 1 <= k <= k_in = %d, got k = %d" % (k_in, k))
    if not (0 <= q_lo and q_lo + nq <= n):
        raise ValueError("the queries [%d, %d) are no range of the n = %d rows" % (q_lo, q_lo + nq, n))
    if nq * k_in > np.iinfo(np.int32).max:
        raise ValueError("need fewer than 2^31 candidates in all (nq = %d, k_in = %d)" % (nq, k_in))
    if out is not None:
        idx, dist = out
        if not (isinstance(idx, np.ndarray) and isinstance(dist, np.ndarray)) \
                or (idx.shape, dist.shape) != ((nq, k), (nq, k)) or idx.dtype != np.int32 \
                or dist.dtype != np.float32 or not (idx.flags.c_contiguous and dist.flags.c_contiguous):
            raise ValueError("out must be C-contiguous (int32 [nq, k], float32 [nq, k])")
    return nq, k_in, k, q_lo


def check_rescore_ragged(n, cand_indptr, cand_idx, radius, q_lo=0):
    """The argument checks of RescoreRows.radius (fdr_rescore_rows_radius repeats those of the indptr and the limits);
    needs no GPU.  n: the rows of the row set.  cand_indptr int64 [nq + 1] and cand_idx int32 [cand_indptr[-1]],
    C-contiguous 1-D numpy arrays: row r holds the candidates of query q_lo + r; cand_indptr starts at 0 and never
    decreases; fewer than 2^31 candidates in all; 0 <= q_lo and q_lo + nq <= n; 0 <= radius <= 1 (a real number, no
    NaN; 1 keeps every candidate; -0.0 comes back as 0.0).  That every candidate is a row in [0, n) is checked on the device.  Returns
    (nq, radius as float32, q_lo, counts int64 [nq]: the rows' lengths)."""
    for name, a, dt in (("cand_indptr", cand_indptr, np.int64), ("cand_idx", cand_idx, np.int32)):
        if not isinstance(a, np.ndarray) or a.dtype != dt:
            raise TypeError("%s must be a numpy %s array" % (name, np.dtype(dt)))
        if a.ndim != 1 or not a.flags.c_contiguous:
            raise ValueError("%s must be a C-contiguous 1-D array" % name)
    for name, v in (("n", n), ("q_lo", q_lo)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError("radius must be a number, got %r" % (radius,))
    r = np.float32(radius)
    if not (r >= 0 and r <= 1):
        raise ValueError("need 0 <= radius <= 1, got %r" % (radius,))
    r = r + np.float32(0)  # (-0.0 is 0: the sign bit does not reach the library)
    if cand_indptr.size < 1:
        raise ValueError("cand_indptr must hold nq + 1 >= 1 elements")
    nq, n, q_lo = cand_indptr.size - 1, int(n), int(q_lo)
    if cand_indptr[0] != 0:
        raise ValueError("cand_indptr must start at 0, got %d" % int(cand_indptr[0]))
    counts = np.diff(cand_indptr)
    if np.any(counts < 0):
        raise ValueError("cand_indptr decreases at query %d" % (q_lo + int(np.argmax(counts < 0))))
    if int(cand_indptr[-1]) > np.iinfo(np.int32).max:
        raise ValueError("need fewer than 2^31 candidates in all, got %d" % int(cand_indptr[-1]))
    if cand_idx.size != cand_indptr[-1]:
        raise ValueError("cand_idx (%d) must hold the %d candidates cand_indptr states"
                         % (cand_idx.size, int(cand_indptr[-1])))
    if not (0 <= q_lo and q_lo + nq <= n):
        raise ValueError("the queries [%d, %d) are no range of the n = %d rows" % (q_lo, q_lo + nq, n))
    return nq, r, q_lo, counts


def check_radius_merge(parts):
    """The argument checks of Context.radius_merge (fdr_radius_merge repeats those of the indptrs and the limits);
    needs no GPU.  parts: a sequence of 1 .. 64 triples (indptr int64 [nq + 1], idx int32 [indptr[-1]], dist float32
    [indptr[-1]]), C-contiguous 1-D numpy arrays, the same nq in every part; each indptr starts at 0 and never
    decreases; fewer than 2^31 entries in all.  What the rows hold (ascending keys, distances >= 0 and not NaN, indices
    >= 0) is checked on the device.  Returns (n_parts, nq, counts int64 [nq]: the merged rows' lengths)."""
    try:
        parts = [tuple(p) for p in parts]
    except TypeError:
        raise TypeError("parts must be a sequence of (indptr, idx, dist) triples") from None
    if not 1 <= len(parts) <= TOPK_MERGE_MAX_PARTS:
        raise ValueError("need 1 <= n_parts <= %d, got %d" % (TOPK_MERGE_MAX_PARTS, len(parts)))
    for p, part in enumerate(parts):
        if len(part) != 3:
            raise ValueError("part %d is not an (indptr, idx, dist) triple" % p)
        for name, a, dt in zip(("indptr", "idx", "dist"), part, (np.int64, np.int32, np.float32)):
            if not isinstance(a, np.ndarray) or a.dtype != dt:
                raise TypeError("part %d: %s must be a numpy %s array" % (p, name, np.dtype(dt)))
            if a.ndim != 1 or not a.flags.c_contiguous:
                raise ValueError("part %d: %s must be a C-contiguous 1-D array" % (p, name))
    nq = parts[0][0].size - 1
    total = 0
    for p, (indptr, _, _) in enumerate(parts):
        if indptr.size != nq + 1 or nq < 0:
            raise ValueError("part %d: its indptr has %d elements, not nq + 1 = %d" % (p, indptr.size, nq + 1))
        if indptr[0] != 0 or np.any(np.diff(indptr) < 0):
            raise ValueError("part %d: its indptr must start at 0 and never decrease" % p)
        total += int(indptr[-1])
    if nq > np.iinfo(np.int32).max or total > np.iinfo(np.int32).max:
        raise ValueError("need fewer than 2^31 queries and fewer than 2^31 entries in all (got %d and %d)" % (nq, total))
    for p, (indptr, idx, dist) in enumerate(parts):
        if idx.size != indptr[-1] or dist.size != indptr[-1]:
            raise ValueError("part %d: idx (%d) and dist (%d) must hold the %d entries its indptr states"
                             % (p, idx.size, dist.size, int(indptr[-1])))
    counts = np.zeros(nq, dtype=np.int64)
    for indptr, _, _ in parts:
        counts += np.diff(indptr)
    return len(parts), nq, counts


def check_graph_symmetrize(graph, mode="union", max_entries=1 << 27):
    """The argument checks of Context.graph_symmetrize (fdr_graph_symmetrize repeats those of the indptr and the
    limits); needs no GPU.  graph: (idx int32 [n, k], dist float32 [n, k]) or (indptr int64 [n + 1], idx int32, dist
    float32), numpy arrays (graph.as_ragged); at least one row, fewer than 2^31 rows and entries; mode "union",
    "mutual" or "transpose"; 1 <= max_entries < 2^31.  All ValueError.  What the rows hold (indices in [0, n), distances
    >= 0 and not NaN, no index twice in a row) is checked on the device.  Returns (mode code, n, indptr, idx, dist)."""
    from . import graph as _graph
    code = _graph.mode_code(mode)
    if isinstance(max_entries, bool) or not isinstance(max_entries, (int, np.integer)) \
            or not 1 <= int(max_entries) < 2 ** 31:
        raise ValueError("max_entries must be an integer in [1, 2^31), got %r" % (max_entries,))
    indptr, idx, dist = _graph.as_ragged(graph)
    n = indptr.size - 1
    if not 1 <= n <= np.iinfo(np.int32).max or idx.size > np.iinfo(np.int32).max:
        raise ValueError("need 1 <= n < 2^31 rows and fewer than 2^31 entries (got %d and %d)" % (n, idx.size))
    return code, n, indptr, idx, dist


def check_graph_expand(graph, fan, lo=0, hi=None, max_entries=1 << 27):
    """The argument checks of Context.graph_expand (fdr_graph_expand repeats those of the indptr and the limits); needs
    no GPU.  graph as check_graph_symmetrize takes it; 1 <= fan <= FDR_MAX_K; 0 <= lo <= hi <= n (hi None: n); 1 <=
    max_entries < 2^31.  All ValueError.  What the rows hold (indices in [0, n), distances >= 0 and not NaN) is checked
    on the device, over the whole graph.  Returns (n, indptr, idx, dist, fan, lo, hi)."""
    from . import graph as _graph
    _, n, indptr, idx, dist = check_graph_symmetrize(graph, "union", max_entries)
    indptr, idx, dist, n, fan, lo, hi = _graph.check_expand(indptr, idx, dist, fan, lo, hi)
    return n, indptr, idx, dist, fan, lo, hi


def expand_pieces(bound, max_entries):
    """Cut rows whose expansions hold at most `bound` (int64 [nq]) entries into consecutive pieces that fit max_entries
    by those bounds: [(a, b), ...] covering [0, nq); None when one row's bound alone exceeds it.  radius_pieces without
    its walk over the rows.  Needs no GPU."""
    nq = int(bound.size)
    if nq == 0 or int(bound.sum()) <= max_entries:
        return [(0, nq)]
    if int(bound.max()) > max_entries:
        return None
    ends = np.cumsum(bound)
    pieces, a, done = [], 0, 0
    while a < nq:
        b = int(np.searchsorted(ends, done + max_entries, side="right"))
        pieces.append((a, b))
        a, done = b, int(ends[b - 1])
    return pieces


def check_graph_components(graph, mode="union", max_distance=None):
    """The argument checks of Context.graph_components (fdr_graph_components repeats those of the indptr, the mode, the
    bound and the limits); needs no GPU.  graph as check_graph_symmetrize takes it; mode "union" or "mutual"
    ("transpose" is refused: its components are the union's); max_distance None (+inf: every entry joins) or a number
    whose float32 bits are at most 0x7f800000 (NaN, negatives and -0.0 are refused).  All ValueError.  What the rows
    hold is checked on the device.  Returns (mode code, n, indptr, idx, dist, the bound as float32)."""
    from . import graph as _graph
    code = _graph.component_mode_code(mode)
    bound = np.array(_graph.bound_bits(max_distance), dtype=np.uint32).view(np.float32)
    _, n, indptr, idx, dist = check_graph_symmetrize(graph, "union")
    return code, n, indptr, idx, dist, bound


def _row_mass_overflows(indptr, values, largest):
    """Whether a row's float32 add chain over its values (all finite and >= 0, none above `largest`) reaches +inf.  A
    chain of m such terms is at most m * largest * (1 + 2^-24)^m, below 1.07e38 for m <= 2^20 and m * largest < 1e38;
    only the rows beyond that bound run the chain itself (np.cumsum in float32 adds in order)."""
    lens = np.diff(indptr)
    suspects = np.flatnonzero((lens > (1 << 20)) | (lens.astype(np.float64) * largest >= 1e38))
    with np.errstate(over="ignore"):
        for r in suspects:
            if not np.isfinite(np.cumsum(values[indptr[r]:indptr[r + 1]], dtype=np.float32)[-1]):
                return True
    return False


def _check_sparse(indptr, indices, values, n_features, k, metric="cosine", min_rows=1):
    """k=None: no k to check, but n >= min_rows."""
    for name, a, dt in (("indptr", indptr, np.int64), ("indices", indices, np.int32), ("values", values, np.float32)):
        if a is None and name == "values":
            continue
        if not isinstance(a, np.ndarray) or a.dtype != dt:
            raise TypeError("%s must be a numpy %s array" % (name, np.dtype(dt)))
        if a.ndim != 1 or not a.flags.c_contiguous:
            raise ValueError("%s must be a C-contiguous 1-D array" % name)
    if indptr.size < 1 or indptr[0] != 0 or indptr[-1] != indices.size or np.any(np.diff(indptr) < 0):
        raise ValueError("indptr is not a CSR row pointer of the indices")
    if values is not None and values.size != indices.size:
        raise ValueError("values and indices differ in length")
    n, k, F = indptr.size - 1, None if k is None else int(k), int(n_features)
    if not 1 <= F <= np.iinfo(np.int32).max:
        raise ValueError("n_features must be in [1, 2^31)")
    if k is None:
        if n < min_rows:
            raise ValueError("need at least one row")
    elif not 1 <= k <= FDR_MAX_K or k > n:
        raise ValueError("need 1 <= k <= min(%d, n = %d), got k = %d" % (FDR_MAX_K, n, k))
    if indices.size:
        if int(indices.min()) < 0 or int(indices.max()) >= F:
            raise ValueError("a feature index is outside [0, %d)" % F)
        ascending = np.diff(indices) > 0
        starts = indptr[1:-1]
        ascending[starts[(starts > 0) & (starts < indices.size)] - 1] = True  # (a row's first id follows another row)
        if not np.all(ascending):
            raise ValueError("feature indices must be strictly ascending inside each row (sorted, no duplicates)")
    if metric == "weighted_jaccard" and values is not None and values.size:
        lo, hi = float(values.min()), float(values.max())  # (two reductions without a temporary; a NaN comes through)
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("values must be finite")
        if lo < 0:
            raise ValueError("values must not be negative under metric='weighted_jaccard'")
        if _row_mass_overflows(indptr, values, hi):
            raise ValueError("a row's float32 sum of values is not finite (metric='weighted_jaccard' needs a finite "
                             "mass per row)")
    elif values is not None and not np.all(np.isfinite(values)):
        raise ValueError("values must be finite")
    return n, k, F


class Context:
    """One GPU context (= fdr_ctx).  Methods raise FedrannHipError on any non-zero return code."""

    def __init__(self, device=0):
        self._L = load_library()
        h = ctypes.c_void_p()
        rc = self._L.fdr_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise FedrannHipError("fdr_create(%d) failed (%d): %s" % (device, rc, self._err()))
        self._h = h
        self.device = int(device)
        self.n_features = 0
        self.d = 0
        self._sparse_gen = 0  # builds of the context's sparse index so far (SparseIndex: is mine still the one?)
        self._dense_gen = 0   # ... and of its dense index (DenseIndex)
        self._rescore_gen = 0  # ... and of its re-score row set (RescoreRows)

    def _err(self):
        return self._L.fdr_last_error().decode("utf-8", "replace")

    def _check(self, rc, what):
        if rc != 0:
            raise FedrannHipError("%s failed (%d): %s" % (what, rc, self._err()))

    def close(self):
        if getattr(self, "_h", None):
            self._L.fdr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- info ---------------------------------------------------------------------------------
    def device_info(self):
        buf = ctypes.create_string_buffer(256)
        self._check(self._L.fdr_device_info(self._h, buf, 256), "fdr_device_info")
        name, arch, cus, mem = buf.value.decode().split("|")
        return {"name": name, "arch": arch, "cus": int(cus), "hbm_bytes": int(mem)}

    def padded_dim(self, d):
        dp = self._L.fdr_padded_dim(int(d))
        if dp < 0:
            raise FedrannHipError("embedding dimension %d unsupported (1..%d)" % (d, FDR_MAX_DIM))
        return dp

    def set_knn_mode(self, mode):
        """mode: "auto" (default), "exact" or "prefilter" -- same results, see include/fedrann_hip.h."""
        code = {"auto": 0, "exact": 1, "prefilter": 2}[mode]
        self._check(self._L.fdr_set_knn_mode(self._h, code), "fdr_set_knn_mode")

    def set_dedup_mode(self, mode):
        """Duplicate-row classes: "auto" (default), "off", "on" (at every size) or "force" (always expand;
        tests) -- same results, see include/fedrann_hip.h."""
        code = {"auto": 0, "off": 1, "on": 2, "force": 3}[mode]
        self._check(self._L.fdr_set_dedup_mode(self._h, code), "fdr_set_dedup_mode")

    def set_live_chunks(self, mode):
        """Live-chunk candidate pass at d <= 128: "auto" (default), "off" or "force" (at every size; tests) -- same
        results, see include/fedrann_hip.h."""
        code = {"auto": 0, "off": 1, "force": 2}[mode]
        self._check(self._L.fdr_set_live_chunks(self._h, code), "fdr_set_live_chunks")

    def set_live_skip(self, mode):
        """Stage skipping of the live-chunk pass: "auto" (default: on whenever that pass runs) or "off" -- same
        results, see include/fedrann_hip.h."""
        code = {"auto": 0, "off": 1}[mode]
        self._check(self._L.fdr_set_live_skip(self._h, code), "fdr_set_live_skip")

    def set_pass_tail(self, mode):
        """The end of the live-chunk pass: "auto" (default: the groups in descending cost) or "off" (ascending NL);
        "order", "early", "early_group" force the order alone, or the order and the merge + re-rank of finished groups
        under the pass's last launches (tests, measurements) -- same results, see include/fedrann_hip.h."""
        code = {"auto": 0, "off": 1, "order": 2, "early": 3, "early_group": 4}[mode]
        self._check(self._L.fdr_set_pass_tail(self._h, code), "fdr_set_pass_tail")

    def set_rerank_compact(self, mode):
        """Re-rank from compact rows at d <= 128: "auto" (default: on unless too many rows overflow their record),
        "off" (every candidate's whole fp32 row) or "force" (on whatever the rows; tests) -- same results, see
        include/fedrann_hip.h."""
        code = {"auto": 0, "off": 1, "force": 2}[mode]
        self._check(self._L.fdr_set_rerank_compact(self._h, code), "fdr_set_rerank_compact")

    def last_live_stage_lists(self, segment):
        """Test support: (first row, lens int32 [256], lists uint16 [256, stages]) of one target segment of the last
        live-chunk pass -- the segment's first row in the scan order and, per query-block mask value, the stages of 128
        rows a block of that mask walks (0xffff behind a list's end).  Needs CAPTURE_LIVE_LISTS set during the call."""
        first, nst = ctypes.c_int32(), ctypes.c_int32()
        lens = np.empty(256, dtype=np.int32)
        self._check(self._L.fdr_last_live_stage_lists(self._h, int(segment), ctypes.byref(first), ctypes.byref(nst),
                                                      lens.ctypes.data, None), "fdr_last_live_stage_lists")
        lists = np.empty((256, nst.value), dtype=np.uint16)
        if nst.value:
            self._check(self._L.fdr_last_live_stage_lists(self._h, int(segment), None, ctypes.byref(nst), None,
                                                          lists.ctypes.data), "fdr_last_live_stage_lists")
        return first.value, lens, lists

    def kmer_search(self, seqs, seq_off, lib_codes, k):
        """Per-read ascending unique library indices: (indptr int64 [R+1], indices int32 [nnz])."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        lib_codes = np.ascontiguousarray(lib_codes, dtype=np.uint64)
        R = seq_off.size - 1
        if R < 0 or (R >= 0 and seq_off.size and int(seq_off[-1]) != seqs.size):
            raise ValueError("seq_off does not describe seqs")
        indptr = np.empty(R + 1, dtype=np.int64)
        nnz = ctypes.c_int64()
        self._check(self._L.fdr_kmer_search(self._h, seqs.ctypes.data, seq_off.ctypes.data, R,
                                            lib_codes.ctypes.data, lib_codes.size, int(k), indptr.ctypes.data,
                                            ctypes.byref(nnz)), "fdr_kmer_search")
        indices = np.empty(nnz.value, dtype=np.int32)
        self._check(self._L.fdr_kmer_search_indices(self._h, indices.ctypes.data), "fdr_kmer_search_indices")
        return indptr, indices

    def kmer_count(self, seqs, seq_off, k, min_count=1):
        """Canonical k-mers with >= min_count occurrences: (codes uint64 ascending, counts uint64)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        n = ctypes.c_int64()
        self._check(self._L.fdr_kmer_count(self._h, seqs.ctypes.data, seq_off.ctypes.data, seq_off.size - 1, int(k),
                                           int(min_count), ctypes.byref(n)), "fdr_kmer_count")
        codes = np.empty(n.value, dtype=np.uint64)
        counts = np.empty(n.value, dtype=np.uint64)
        self._check(self._L.fdr_kmer_count_fetch(self._h, codes.ctypes.data, counts.ctypes.data), "fdr_kmer_count_fetch")
        return codes, counts

    def kmer_count_begin(self, k):
        """Incremental counting for a streaming reader: begin, add whole reads piece by piece, finish."""
        self._check(self._L.fdr_kmer_count_begin(self._h, int(k)), "fdr_kmer_count_begin")

    def kmer_count_add(self, seqs, seq_off):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        self._check(self._L.fdr_kmer_count_add(self._h, seqs.ctypes.data, seq_off.ctypes.data, seq_off.size - 1),
                    "fdr_kmer_count_add")

    def kmer_count_finish(self, min_count=1):
        """(codes uint64 ascending, counts uint64) of the canonical k-mers with >= min_count occurrences in all the
        reads added since kmer_count_begin."""
        n = ctypes.c_int64()
        self._check(self._L.fdr_kmer_count_finish(self._h, int(min_count), ctypes.byref(n)), "fdr_kmer_count_finish")
        codes = np.empty(n.value, dtype=np.uint64)
        counts = np.empty(n.value, dtype=np.uint64)
        self._check(self._L.fdr_kmer_count_fetch(self._h, codes.ctypes.data, counts.ctypes.data), "fdr_kmer_count_fetch")
        return codes, counts

    def set_kmer_count_block(self, chars):
        """Characters per block of kmer_count (0 = default 2^31); small blocks exercise the merge in tests."""
        self._check(self._L.fdr_set_kmer_count_block(self._h, int(chars)), "fdr_set_kmer_count_block")

    def kmer_count_export_dev(self, d_splitters, n_parts, d_codes_out=None, d_counts_out=None, stream=None):
        """The accumulated, unthresholded table cut at n_parts - 1 splitter codes (device pointers, e.g. torch's
        data_ptr()): returns the part offsets int64 [n_parts + 1]; with d_codes_out / d_counts_out (device, at least
        part_off[-1] entries each) the table is copied there too."""
        part_off = np.empty(int(n_parts) + 1, dtype=np.int64)
        self._check(self._L.fdr_kmer_count_export_dev(self._h, d_splitters or None, int(n_parts), d_codes_out or None,
                                                      d_counts_out or None, part_off.ctypes.data, stream or None),
                    "fdr_kmer_count_export_dev")
        return part_off

    def kmer_count_merge_dev(self, run_off, d_codes, d_counts, min_count=1, stream=None):
        """Merge the runs (run_off int64 [W + 1]) of device arrays d_codes / d_counts: (codes, counts) ascending, the
        summed counts >= min_count."""
        run_off = np.ascontiguousarray(run_off, dtype=np.int64)
        n = ctypes.c_int64()
        self._check(self._L.fdr_kmer_count_merge_dev(self._h, run_off.size - 1, run_off.ctypes.data, d_codes or None,
                                                     d_counts or None, int(min_count), ctypes.byref(n), stream or None),
                    "fdr_kmer_count_merge_dev")
        return self._kmer_count_fetch(n.value)

    def kmer_count_merge(self, run_off, codes, counts, min_count=1):
        """kmer_count_merge_dev from host arrays."""
        run_off = np.ascontiguousarray(run_off, dtype=np.int64)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if codes.size != counts.size or (run_off.size and codes.size < int(run_off[-1])):
            raise ValueError("run_off does not describe codes / counts")
        n = ctypes.c_int64()
        self._check(self._L.fdr_kmer_count_merge(self._h, run_off.size - 1, run_off.ctypes.data, codes.ctypes.data,
                                                 counts.ctypes.data, int(min_count), ctypes.byref(n)),
                    "fdr_kmer_count_merge")
        return self._kmer_count_fetch(n.value)

    def _kmer_count_fetch(self, n):
        codes = np.empty(n, dtype=np.uint64)
        counts = np.empty(n, dtype=np.uint64)
        self._check(self._L.fdr_kmer_count_fetch(self._h, codes.ctypes.data, counts.ctypes.data), "fdr_kmer_count_fetch")
        return codes, counts

    def last_kmer_count_blocks(self):
        """Non-empty blocks the last kmer_count call counted."""
        return int(self._L.fdr_last_kmer_count_blocks(self._h))

    def last_unique(self):
        """(unique target rows, unique query rows) searched by the last k-NN call."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self._check(self._L.fdr_last_unique(self._h, ctypes.byref(a), ctypes.byref(b)), "fdr_last_unique")
        return int(a.value), int(b.value)

    def last_prefilter_launches(self):
        """(launches, queues) of the fp16 candidate pass of the last k-NN call (0, 0 after an exact-mode call)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self._check(self._L.fdr_last_prefilter_launches(self._h, ctypes.byref(a), ctypes.byref(b)),
                    "fdr_last_prefilter_launches")
        return int(a.value), int(b.value)

    def last_uncertified(self):
        """Prefilter mode: query rows of the last k-NN call that were searched by the exact kernel."""
        return int(self._L.fdr_last_uncertified(self._h))

    def last_query_paths(self, n_queries):
        """uint8 [n_queries]: which way every query row of the last k-NN call took to its result (PATH_* codes, bit 7 =
        member of a duplicate-row class of several rows): fdr_last_query_paths.  Diagnostics; the tests' strata."""
        out = np.empty(int(n_queries), dtype=np.uint8)
        self._check(self._L.fdr_last_query_paths(self._h, _ptr(out), int(n_queries)), "fdr_last_query_paths")
        return out

    def last_knn_trace(self):
        """dict of fdr_last_knn_trace: which kernels the last k-NN call ran ("kind" and "exact_fallback" as names).
        Diagnostics; the tests assert the variant they meant to run with it."""
        t = KnnTrace()
        self._check(self._L.fdr_last_knn_trace(self._h, ctypes.byref(t)), "fdr_last_knn_trace")
        out = {name: int(getattr(t, name)) for name, _ in KnnTrace._fields_}
        out["kind"] = TRACE_KINDS[out["kind"]]
        out["exact_fallback"] = FALLBACKS[out["exact_fallback"]]
        return out

    def set_knn_capture(self, what):
        """Or of CAPTURE_CANDIDATES / CAPTURE_RANGE / CAPTURE_LIVE_LISTS (0: off): fdr_set_knn_capture.  Test support."""
        self._check(self._L.fdr_set_knn_capture(self._h, int(what)), "fdr_set_knn_capture")

    def last_candidates(self, n_queries, kp):
        """(uint64 keys [n_queries, kp], qbits) of the last prefilter-mode call: fdr_last_candidates.  key = fp32 bits of
        d~ << 32 | global target row; unused slots all ones."""
        keys = np.empty((int(n_queries), int(kp)), dtype=np.uint64)
        qbits = ctypes.c_int32(0)
        self._check(self._L.fdr_last_candidates(self._h, _ptr(keys), int(n_queries), int(kp), ctypes.byref(qbits)),
                    "fdr_last_candidates")
        return keys, int(qbits.value)

    def last_range_sets(self, n_range):
        """(queries, theta, counts, rows [n_range, RANGE_CAP]) of the last call's range pass: fdr_last_range_sets.
        Rows are global target rows, -1 past min(count, RANGE_CAP)."""
        n = int(n_range)
        q, th, cnt = np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.int32)
        rows = np.empty((n, RANGE_CAP), np.int32)
        self._check(self._L.fdr_last_range_sets(self._h, n, _ptr(q), _ptr(th), _ptr(cnt), _ptr(rows)),
                    "fdr_last_range_sets")
        return q, th, cnt, rows

    def timing(self, enable):
        self._check(self._L.fdr_timing(self._h, 1 if enable else 0), "fdr_timing")

    def timing_read(self, which):
        """(launch count, total ms) of kernel kind `which` since the last read; KERNELS names them."""
        n, ms = ctypes.c_int(), ctypes.c_float()
        self._check(self._L.fdr_timing_read(self._h, int(which), ctypes.byref(n), ctypes.byref(ms)),
                    "fdr_timing_read")
        return int(n.value), float(ms.value)

    # -- host-pointer API -----------------------------------------------------------------------
    def projection_load(self, p_indptr, p_cols, p_vals, n_features, d):
        p_indptr = _as(p_indptr, np.int64, "p_indptr")
        p_cols = _as(p_cols, np.int32, "p_cols")
        p_vals = _as(p_vals, np.float32, "p_vals")
        if p_indptr.shape != (int(n_features) + 1,):
            raise ValueError("p_indptr must have n_features + 1 entries")
        self._check(self._L.fdr_projection_load(self._h, int(n_features), int(d), _ptr(p_indptr),
                                                _ptr(p_cols), _ptr(p_vals)), "fdr_projection_load")
        self.n_features, self.d = int(n_features), int(d)

    def csr_compact(self, a_indptr, a_indices, n_threads=0):
        """The CSR without the column ids whose projection row is empty (same E, ~10x fewer ids)."""
        a_indptr = _as(a_indptr, np.int64, "a_indptr")
        a_indices = _as(a_indices, np.int32, "a_indices")
        n = a_indptr.shape[0] - 1
        out_ip = np.empty(n + 1, dtype=np.int64)
        out_ix = np.empty(max(int(a_indices.size), 1), dtype=np.int32)
        self._check(self._L.fdr_csr_compact(self._h, n, _ptr(a_indptr), _ptr(a_indices), _ptr(out_ip),
                                            _ptr(out_ix), int(out_ix.size), int(n_threads)), "fdr_csr_compact")
        return out_ip, np.ascontiguousarray(out_ix[:int(out_ip[-1])])

    def host_register(self, *arrays):
        """Pin numpy arrays the caller keeps passing to embed / knn / embed_knn (PCIe-rate copies)."""
        for a in arrays:
            if a is not None and a.nbytes:
                self._check(self._L.fdr_host_register(self._h, a.ctypes.data, a.nbytes), "fdr_host_register")

    def host_unregister(self, *arrays):
        for a in arrays:
            if a is not None and a.nbytes:
                self._check(self._L.fdr_host_unregister(self._h, a.ctypes.data), "fdr_host_unregister")

    def embed(self, a_indptr, a_indices):
        a_indptr = _as(a_indptr, np.int64, "a_indptr")
        a_indices = _as(a_indices, np.int32, "a_indices")
        n = a_indptr.shape[0] - 1
        E = np.empty((n, self.d), dtype=np.float32)
        self._check(self._L.fdr_embed(self._h, n, _ptr(a_indptr), _ptr(a_indices), _ptr(E)),
                    "fdr_embed")
        return E

    def knn(self, E, k):
        E = _as(E, np.float32, "E")
        if E.ndim != 2:
            raise ValueError("E must be 2-D")
        n, d = E.shape
        idx = np.empty((n, k), dtype=np.int32)
        dist = np.empty((n, k), dtype=np.float32)
        self._check(self._L.fdr_knn(self._h, _ptr(E), n, d, int(k), _ptr(idx), _ptr(dist)),
                    "fdr_knn")
        return idx, dist

    def knn_sparse(self, indptr, indices, values, n_features, k, metric="cosine"):
        """Exact k-NN of the rows of a CSR.  indptr int64 [n + 1], indices int32 strictly ascending inside each row
        and in [0, n_features), values float32 (finite) or None (every stored entry 1).  Returns (idx int32 [n, k],
        dist float32 [n, k]).
        metric="cosine" (fdr_knn_sparse): the bits of knn() on the densified matrix, without densifying it.
        metric="jaccard" (fdr_knn_sparse_metric): the Jaccard distance of the rows' sets, a row's set being its stored
        entries with a value other than 0: (float32)((u - c) / u) in float64 for c shared features and a union of u,
        0 for two empty rows; ascending by (distance, index).
        metric="weighted_jaccard" (fdr_knn_sparse_metric): the weighted Jaccard (Ruzicka) distance of rows with values
        >= 0 (a stored 0 is absent; None: every entry 1): with A the float32 sum of a row's values in order, m the
        float32 sum of min(x_q, x_t) over the shared features in ascending order and u = A_q + A_t - m in float64,
        (float32)((u - m) / u), 0 for two zero-mass rows.  Negative values and a row whose mass is not finite are
        refused (ValueError).
        The call builds the context's sparse index anew (a SparseIndex of this context is stale afterwards)."""
        code = sparse_metric_code(metric)
        n, k, F = check_sparse_rows(indptr, indices, values, n_features, k, metric=metric)
        self._sparse_gen += 1
        idx = np.empty((n, k), dtype=np.int32)
        dist = np.empty((n, k), dtype=np.float32)
        if code == METRIC_COSINE:
            self._check(self._L.fdr_knn_sparse(self._h, n, F, _ptr(indptr), _ptr(indices), _ptr(values), k,
                                               _ptr(idx), _ptr(dist)), "fdr_knn_sparse")
        else:
            self._check(self._L.fdr_knn_sparse_metric(self._h, code, n, F, _ptr(indptr), _ptr(indices),
                                                      _ptr(values), k, _ptr(idx), _ptr(dist)),
                        "fdr_knn_sparse_metric")
        return idx, dist

    def sparse_index(self, indptr, indices, values, n_features, metric="cosine"):
        """The posting index of a CSR (arguments as knn_sparse, at least one row), kept on the device for any number
        of SparseIndex.search calls: fdr_sparse_index_build.  A context holds one index: this call, and every
        knn_sparse, replaces it, and a SparseIndex of the replaced one raises from then on."""
        code = sparse_metric_code(metric)
        n, F = check_sparse_csr(indptr, indices, values, n_features, metric=metric)
        self._sparse_gen += 1
        self._check(self._L.fdr_sparse_index_build(self._h, code, n, F, _ptr(indptr), _ptr(indices), _ptr(values)),
                    "fdr_sparse_index_build")
        return SparseIndex(self, n, metric, self._sparse_gen, n_features=F)

    def dense_index(self, E):
        """The dense index of the rows E float32 [n, d] (not normalised, knn()'s argument; 1 <= d <= 512), kept on the
        device for any number of DenseIndex.radius_search / radius_query calls: fdr_dense_index_build.  A context
        holds one dense index, beside its sparse one: this call and dense_index_from_csr replace it, and a DenseIndex
        of the replaced one raises from then on."""
        E = _as(E, np.float32, "E")
        if E.ndim != 2:
            raise ValueError("E must be 2-D")
        n, d = E.shape
        check_dense_radius(n, d, 0.0)
        self._dense_gen += 1
        self._check(self._L.fdr_dense_index_build(self._h, _ptr(E), n, d), "fdr_dense_index_build")
        return DenseIndex(self, n, d, self._dense_gen)

    def dense_index_from_csr(self, a_indptr, a_indices):
        """The dense index of the rows embed(a_indptr, a_indices) would return, which stay on the device:
        fdr_dense_index_embed.  Needs projection_load; the same index as dense_index(embed(...)), bit for bit."""
        a_indptr = _as(a_indptr, np.int64, "a_indptr")
        a_indices = _as(a_indices, np.int32, "a_indices")
        n = a_indptr.shape[0] - 1
        if self.d < 1:
            raise FedrannHipError("dense_index_from_csr: no projection loaded")
        check_dense_radius(n, self.d, 0.0)
        self._dense_gen += 1
        self._check(self._L.fdr_dense_index_embed(self._h, n, _ptr(a_indptr), _ptr(a_indices)), "fdr_dense_index_embed")
        return DenseIndex(self, n, self.d, self._dense_gen)

    def topk_merge(self, idx_parts, dist_parts, k, out=None):
        """The k nearest targets per query over the candidate lists of n_parts ranks: idx_parts int32 and dist_parts
        float32 [n_parts, nq, kp], part-major as a gather by source rank leaves them, each row ascending by (distance
        bits, index), the indices global and distinct across a query's parts.  Returns (idx int32 [nq, k], dist
        float32 [nq, k]): distributed.merge_sparse_topk of the parts bit for bit, merged on the GPU (fdr_topk_merge).
        A row out of order, a negative or NaN distance and a negative index are refused (FedrannHipError) with
        nothing written.  out=(idx, dist): caller-owned C-contiguous result arrays.  The context's sparse index and
        its last k-NN trace stay as they are."""
        n_parts, nq, kp, k = check_topk_merge(idx_parts, dist_parts, k, out)
        idx, dist = out if out is not None else (np.empty((nq, k), np.int32), np.empty((nq, k), np.float32))
        self._check(self._L.fdr_topk_merge(self._h, nq, n_parts, kp, k, _ptr(idx_parts), _ptr(dist_parts), _ptr(idx),
                                           _ptr(dist)), "fdr_topk_merge")
        return idx, dist

    def radius_merge(self, parts, max_entries=1 << 26):
        """The union, per query, of the ragged rows of n_parts ranks: parts is a sequence of (indptr int64 [nq + 1],
        idx int32, dist float32) as SparseIndex.radius_query returns them, each row ascending by (distance bits, index),
        the indices global and distinct across a query's parts.  Returns (indptr int64 [nq + 1], idx int32, dist
        float32): distributed.merge_sparse_radius of the parts bit for bit, merged on the GPU (fdr_radius_merge).  The
        queries go to the device in consecutive pieces whose merged rows hold at most max_entries entries (16 device
        bytes each); one query with more is a ValueError, and so are a bad indptr, 2^31 entries or more in all and
        more than 64 parts, all before the library is called.  A row out of order, a negative or NaN distance and a
        negative index are refused (FedrannHipError) by the piece that holds them.  The context's sparse index, its
        held radius result and its last k-NN trace stay as they are."""
        n_parts, nq, counts = check_radius_merge(parts)
        if isinstance(max_entries, bool) or not isinstance(max_entries, (int, np.integer)) \
                or not 1 <= int(max_entries) < 2 ** 31:
            raise ValueError("max_entries must be an integer in [1, 2^31), got %r" % (max_entries,))
        # (everything in one piece: the common case, without the walk over the counts)
        pieces = [(0, nq)] if int(counts.sum()) <= int(max_entries) else radius_pieces(counts, int(max_entries))
        if pieces is None:
            q = int(np.argmax(counts > max_entries))
            raise ValueError("query %d alone has %d entries over the parts, above max_entries = %d"
                             % (q, int(counts[q]), max_entries))
        out_ip = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum(counts, out=out_ip[1:])
        idx = np.empty(int(out_ip[-1]), dtype=np.int32)
        dist = np.empty(int(out_ip[-1]), dtype=np.float32)
        for a, b in pieces:
            ip_parts = np.stack([p[0][a:b + 1] - p[0][a] for p in parts])
            if len(pieces) == 1 and n_parts == 1:
                ix_parts, ds_parts = parts[0][1], parts[0][2]
            else:
                ix_parts = np.concatenate([p[1][p[0][a]:p[0][b]] for p in parts])
                ds_parts = np.concatenate([p[2][p[0][a]:p[0][b]] for p in parts])
            ip = np.full(b - a + 1, -1, dtype=np.int64)
            lo, hi = int(out_ip[a]), int(out_ip[b])
            self._check(self._L.fdr_radius_merge(self._h, b - a, n_parts, _ptr(ip_parts), _ptr(ix_parts), _ptr(ds_parts),
                                                 _ptr(ip), _ptr(idx[lo:hi]), _ptr(dist[lo:hi])), "fdr_radius_merge")
            if not np.array_equal(ip, out_ip[a:b + 1] - lo):
                raise FedrannHipError("fdr_radius_merge: the queries [%d, %d) came back with another indptr" % (a, b))
        return out_ip, idx, dist

    def graph_symmetrize(self, graph, mode="union", max_entries=1 << 27):
        """The union, mutual or transposed rows of a neighbour graph: graph is (idx int32 [n, k], dist float32 [n, k]),
        as knn returns them, or ragged (indptr int64 [n + 1], idx int32, dist float32), as a radius search does; an
        entry (t, d) of row q says "q lists t at distance d".  Rows need not be sorted and may hold their own index.
        mode "union": row r names every s that it lists or that lists it; "mutual": only where each lists the other;
        "transpose": every s that lists r.  Returns (indptr int64 [n + 1], idx int32, dist float32), every row
        ascending by (distance bits, index): graph.symmetrize_rows bit for bit, computed on the GPU
        (fdr_graph_symmetrize, then fdr_graph_symmetrize_fetch).  The argument checks (check_graph_symmetrize) are
        ValueErrors before the library is called; an index outside [0, n), a negative or NaN distance, an index twice
        in a row and a result of more than max_entries entries (16 device bytes each) are refused by the library
        (FedrannHipError).  The context's indexes, their held radius results and its last k-NN trace stay as they are."""
        code, n, indptr, idx, dist = check_graph_symmetrize(graph, mode, max_entries)
        out_ip = np.empty(n + 1, dtype=np.int64)
        self._check(self._L.fdr_graph_symmetrize(self._h, code, n, _ptr(indptr), _ptr(idx), _ptr(dist), int(max_entries),
                                                 _ptr(out_ip)), "fdr_graph_symmetrize")
        total = int(out_ip[-1])
        out_idx, out_dist = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.float32)
        self._check(self._L.fdr_graph_symmetrize_fetch(self._h, total, _ptr(out_idx), _ptr(out_dist)),
                    "fdr_graph_symmetrize_fetch")
        return out_ip, out_idx, out_dist

    def graph_components(self, graph, mode="union", max_distance=None):
        """The connected components of a neighbour graph (graph as graph_symmetrize takes it), cut at a distance: rows
        r != s are joined iff the symmetrised rows of `mode` ("union": either lists the other; "mutual": each lists the
        other, at the smaller distance) hold (r, s) with distance bits <= those of max_distance (None: +inf, every
        entry joins).  Returns (labels int32 [n], sizes int64 [C]), the components numbered in ascending order of
        their smallest row: graph.component_labels, array for array, computed on the GPU (fdr_graph_components).  The
        argument checks (check_graph_components) are ValueErrors before the library is called; an index outside
        [0, n), a negative or NaN distance and an index twice in a row are refused by the library (FedrannHipError).
        The context's indexes, their held radius results, a held symmetrised graph and its last k-NN trace stay as
        they are."""
        code, n, indptr, idx, dist, bound = check_graph_components(graph, mode, max_distance)
        labels, sizes, found = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int64), ctypes.c_int64(-1)
        self._check(self._L.fdr_graph_components(self._h, code, n, _ptr(indptr), _ptr(idx), _ptr(dist),
                                                 ctypes.c_float(float(bound)), _ptr(labels), _ptr(sizes),
                                                 ctypes.addressof(found)), "fdr_graph_components")
        return labels, sizes[:found.value].copy()

    def _graph_expand_held(self, n, indptr, idx, dist, fan, lo, hi, max_entries):
        """fdr_graph_expand on checked arguments: the result's row pointer; the indices stay held on the device."""
        out_ip = np.empty(hi - lo + 1, dtype=np.int64)
        self._check(self._L.fdr_graph_expand(self._h, n, _ptr(indptr), _ptr(idx), _ptr(dist), fan, lo, hi - lo,
                                             int(max_entries), _ptr(out_ip)), "fdr_graph_expand")
        return out_ip

    def graph_expand(self, graph, fan, lo=0, hi=None, max_entries=1 << 27):
        """The distinct rows within two hops of the rows [lo, hi) of a neighbour graph (graph as graph_symmetrize takes
        it) along its `fan` nearest entries: row r names every s among its first `fan` entries by (distance bits,
        index), and every s != r among the first `fan` entries of those.  Returns (indptr int64 [hi - lo + 1], idx
        int32), every row ascending by index: graph.expand_rows bit for bit, computed on the GPU (fdr_graph_expand, then
        fdr_graph_expand_fetch).  The argument checks (check_graph_expand) are ValueErrors before the library is called;
        an index outside [0, n) and a negative or NaN distance anywhere in the graph, and a result of more than
        max_entries entries, are refused by the library (FedrannHipError).  An index twice in a row takes two places
        of the fan and comes out once.  The expansion stays held in the context (RescoreRows.refine scores it there)
        until the next graph_expand or graph_free; everything else the context holds stays as it is."""
        n, indptr, idx, dist, fan, lo, hi = check_graph_expand(graph, fan, lo, hi, max_entries)
        out_ip = self._graph_expand_held(n, indptr, idx, dist, fan, lo, hi, max_entries)
        out_idx = np.empty(int(out_ip[-1]), dtype=np.int32)
        self._check(self._L.fdr_graph_expand_fetch(self._h, int(out_ip[-1]), _ptr(out_idx)), "fdr_graph_expand_fetch")
        return out_ip, out_idx

    def graph_free(self):
        """Free the device memory of graph_symmetrize, graph_components and graph_expand, a held expansion
        included (it grows with the largest graph seen):
        fdr_graph_free."""
        self._check(self._L.fdr_graph_free(self._h), "fdr_graph_free")

    def sparse_rescore(self, indptr, indices, values, n_features, candidates, k=None, metric="cosine", q_lo=0, out=None):
        """Candidate lists re-scored by exact distance on the rows of a CSR (arguments as knn_sparse): candidates int32
        [nq, k_in], row r the candidates of query q_lo + r (row numbers of the CSR, e.g. embed_knn's lists at k_in).
        Returns (idx int32 [nq, k], dist float32 [nq, k]), k = k_in by default: each query's candidates under
        `metric`, ascending by (distance bits, index), the first k.  A distance is the float32 knn_sparse reports for
        the pair under that metric, bit for bit, so knn_sparse's own lists come back unchanged (fdr_sparse_rescore).
        The query's own index is an ordinary candidate (distance 0); a repeated candidate comes out twice; one outside
        [0, n) is refused (FedrannHipError) with nothing written.  out=(idx, dist): caller-owned C-contiguous result
        arrays.  The context's sparse index, its dense index and its last k-NN trace stay as they are."""
        code = sparse_metric_code(metric)
        n, _, F = check_sparse_rows(indptr, indices, values, n_features, 1, metric=metric)
        nq, k_in, k, q_lo = check_rescore_args(n, candidates, k, metric, q_lo, out)
        idx, dist = out if out is not None else (np.empty((nq, k), np.int32), np.empty((nq, k), np.float32))
        self._check(self._L.fdr_sparse_rescore(self._h, code, n, F, _ptr(indptr), _ptr(indices), _ptr(values), q_lo, nq,
                                               k_in, _ptr(candidates), k, _ptr(idx), _ptr(dist)), "fdr_sparse_rescore")
        return idx, dist

    def rescore_rows(self, indptr, indices, values, n_features, metric="cosine"):
        """The rows of a CSR (arguments as sparse_rescore's) kept on the device for any number of RescoreRows.knn /
        RescoreRows.radius calls: fdr_rescore_rows_build, one upload and one row pass.  A context holds one row set,
        beside its sparse and its dense index: this call replaces it, and a RescoreRows of the replaced one raises
        from then on.  A row that breaks the CSR's rules is refused and leaves no row set."""
        code = sparse_metric_code(metric)
        n, _, F = check_sparse_rows(indptr, indices, values, n_features, 1, metric=metric)
        self._rescore_gen += 1
        self._check(self._L.fdr_rescore_rows_build(self._h, code, n, F, _ptr(indptr), _ptr(indices), _ptr(values)),
                    "fdr_rescore_rows_build")
        return RescoreRows(self, n, metric, self._rescore_gen)

    def embed_knn(self, a_indptr, a_indices, k, return_embedding=False, out=None):
        """out=(idx int32 [n,k], dist float32 [n,k]): caller-owned (e.g. pinned, reused) result arrays."""
        a_indptr = _as(a_indptr, np.int64, "a_indptr")
        a_indices = _as(a_indices, np.int32, "a_indices")
        n = a_indptr.shape[0] - 1
        if out is None:
            idx = np.empty((n, k), dtype=np.int32)
            dist = np.empty((n, k), dtype=np.float32)
        else:
            idx, dist = out
            if (idx.shape, dist.shape) != ((n, k), (n, k)) or idx.dtype != np.int32 or dist.dtype != np.float32 \
                    or not (idx.flags.c_contiguous and dist.flags.c_contiguous):
                raise ValueError("out must be C-contiguous (int32 [n,k], float32 [n,k])")
        E = np.empty((n, self.d), dtype=np.float32) if return_embedding else None
        self._check(self._L.fdr_embed_knn(self._h, n, _ptr(a_indptr), _ptr(a_indices), int(k),
                                          _ptr(idx), _ptr(dist), _ptr(E)), "fdr_embed_knn")
        return (idx, dist, E) if return_embedding else (idx, dist)

    # -- device-pointer API (integers are raw device addresses, e.g. torch.Tensor.data_ptr()) -----
    def embed_dev(self, n_rows, d_indptr, d_indices, d_E, stream=0):
        self._check(self._L.fdr_embed_dev(self._h, int(n_rows), d_indptr, d_indices, d_E,
                                          stream or None), "fdr_embed_dev")

    def normalize_dev(self, d_E, n_rows, d, d_Ehat, d_zero, stream=0):
        self._check(self._L.fdr_normalize_dev(self._h, d_E, int(n_rows), int(d), d_Ehat, d_zero,
                                              stream or None), "fdr_normalize_dev")

    def knn_workspace_bytes(self, nq, nt, d, k):
        return int(self._L.fdr_knn_workspace_bytes(self._h, int(nq), int(nt), int(d), int(k)))

    def knn_dev(self, d_Qhat, d_qzero, nq, d_That, d_tzero, nt, t_base, d, k, d_idx, d_dist,
                d_ws, ws_bytes, stream=0):
        self._check(self._L.fdr_knn_dev(self._h, d_Qhat, d_qzero, int(nq), d_That, d_tzero,
                                        int(nt), int(t_base), int(d), int(k), d_idx, d_dist, d_ws,
                                        int(ws_bytes), stream or None), "fdr_knn_dev")


    def knn_classes_dev(self, d_That, d_tzero, nt, d, k, nq_max, d_ws, ws_bytes, stream=0):
        """Duplicate-row classes of the target set for knn_unique_dev / knn_expand_dev; returns the number of
        unique rows (0: not worth it, use knn_dev)."""
        nu = ctypes.c_int32()
        self._check(self._L.fdr_knn_classes_dev(self._h, d_That, d_tzero, int(nt), int(d), int(k), int(nq_max), d_ws,
                                                int(ws_bytes), stream or None, ctypes.byref(nu)), "fdr_knn_classes_dev")
        return int(nu.value)

    def knn_unique_dev(self, u_lo, u_hi, d_idx_u, d_dist_u, stream=0):
        self._check(self._L.fdr_knn_unique_dev(self._h, int(u_lo), int(u_hi), d_idx_u, d_dist_u, stream or None),
                    "fdr_knn_unique_dev")

    def knn_expand_dev(self, q0, nq, t_base, d_idx_u_all, d_dist_u_all, d_idx, d_dist, stream=0, u_row_stride=0):
        self._check(self._L.fdr_knn_expand_dev(self._h, int(q0), int(nq), int(t_base), d_idx_u_all, d_dist_u_all,
                                               int(u_row_stride), d_idx, d_dist, stream or None), "fdr_knn_expand_dev")


class _HeldIndex:
    """What SparseIndex and DenseIndex share: the liveness guard of an index that lives in its context, and the radius
    calls' protocol (counts first, one refusal that leaves them, a fetch; a block over the cap cut by its counts).  A
    subclass names its kind, the context's generation counter, its fetch symbol, what max_hits counts, and whether
    the counts a refusal leaves are exact (sparse: the hits) or upper bounds of the pieces' counts (dense: the fp16
    candidates)."""
    _kind = _gen_attr = _fetch = _counted = None
    _exact_counts = True

    def _live(self, what):
        if not self._open:
            raise FedrannHipError("%s: the %s index is closed" % (what, self._kind))
        if not getattr(self._ctx, "_h", None):
            raise FedrannHipError("%s: the context of the %s index is closed" % (what, self._kind))
        if getattr(self._ctx, self._gen_attr) != self._gen:
            raise FedrannHipError("%s: the context has built another %s index since this one" % (what, self._kind))

    def _radius_call(self, what, call, nq, max_hits):
        """One raw radius call over nq queries, call(max_hits, indptr) -> rc.  Returns (indptr, idx, dist), or
        (indptr, None, None) where the total exceeds max_hits: the one refusal that leaves the counts."""
        c = self._ctx
        indptr = np.full(nq + 1, -1, dtype=np.int64)
        rc = call(max_hits, indptr)
        if rc == FDR_E_ARG and indptr[0] == 0 and indptr[-1] > max_hits:
            return indptr, None, None
        c._check(rc, what)
        total = int(indptr[-1])
        idx = np.empty(total, dtype=np.int32)
        dist = np.empty(total, dtype=np.float32)
        c._check(getattr(c._L, self._fetch)(c._h, total, _ptr(idx), _ptr(dist)), self._fetch)
        return indptr, idx, dist

    def _radius_rows(self, what, piece, nq, max_hits, first_row):
        """Rows [0, nq) through piece(a, b) -> the raw call of the rows [a, b); a block over the cap is cut by its
        counts into pieces that fit, run one by one and concatenated: the uncapped result."""
        indptr, idx, dist = self._radius_call(what, piece(0, nq), nq, max_hits)
        if idx is not None:
            return indptr, idx, dist
        counts = np.diff(indptr)
        pieces = radius_pieces(counts, max_hits)
        if pieces is None:
            q = int(np.argmax(counts > max_hits))
            raise FedrannHipError("%s: query %d alone has %d %s, above max_hits = %d"
                                  % (what, first_row + q, int(counts[q]), self._counted, max_hits))
        parts = []
        for a, b in pieces:
            ip, ix, ds = self._radius_call(what, piece(a, b), b - a, max_hits)
            got = None if ix is None else np.diff(ip)
            if got is None or (not np.array_equal(got, counts[a:b]) if self._exact_counts else np.any(got > counts[a:b])):
                raise FedrannHipError("%s: the rows [%d, %d) gave other counts on their own" % (what, a, b))
            parts.append((got, ix, ds))
        out_ip = np.zeros(nq + 1, dtype=np.int64)
        if parts:
            np.cumsum(np.concatenate([p[0] for p in parts]), out=out_ip[1:])
        return (out_ip, np.concatenate([p[1] for p in parts]) if parts else np.empty(0, np.int32),
                np.concatenate([p[2] for p in parts]) if parts else np.empty(0, np.float32))

    def _radius_blocks(self, what, piece, nq, block_rows, max_hits):
        """Query rows [0, nq) in consecutive blocks of at most block_rows rows (None: one block), each through
        _radius_rows with piece(a, b) -> the raw call of the query rows [a, b); the blocks' results concatenated."""
        step = max(nq, 1) if block_rows is None else int(block_rows)
        outs = []
        for a0 in range(0, max(nq, 1), step):  # (nq = 0: one call, which records the trace)
            b0 = min(nq, a0 + step)
            outs.append(self._radius_rows(what, lambda a, b, a0=a0: piece(a0 + a, a0 + b), b0 - a0, max_hits, a0))
        if len(outs) == 1:
            return outs[0]
        out_ip = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum(np.concatenate([np.diff(o[0]) for o in outs]), out=out_ip[1:])
        return out_ip, np.concatenate([o[1] for o in outs]), np.concatenate([o[2] for o in outs])


class SparseIndex(_HeldIndex):
    """The sparse index of a Context (Context.sparse_index): search row ranges of it, at any k, any number of times.
    The index lives in the context, which holds one: once the context has built another (sparse_index, knn_sparse),
    or after close(), search and info raise FedrannHipError."""

    _kind, _gen_attr, _fetch, _counted = "sparse", "_sparse_gen", "fdr_sparse_index_radius_fetch", "hits"

    def __init__(self, ctx, n, metric, gen, n_features=None):
        self._ctx, self.n, self.metric, self._gen = ctx, int(n), metric, gen
        self.n_features = None if n_features is None else int(n_features)  # (None: query() is not available)
        self._open = True

    def search(self, k, lo=0, hi=None, out=None):
        """Neighbours of the rows [lo, hi) (hi=None: n) among all n rows: (idx int32 [hi - lo, k], dist float32
        [hi - lo, k]), row r the query lo + r, indices global: the rows lo .. hi - 1 of knn_sparse's result, bit for
        bit.  out=(idx, dist): caller-owned C-contiguous result arrays of that shape."""
        k, lo, hi = check_sparse_search(self.n, k, lo, hi)
        nq = hi - lo
        if out is None:
            idx = np.empty((nq, k), dtype=np.int32)
            dist = np.empty((nq, k), dtype=np.float32)
        else:
            idx, dist = out
            if (idx.shape, dist.shape) != ((nq, k), (nq, k)) or idx.dtype != np.int32 or dist.dtype != np.float32 \
                    or not (idx.flags.c_contiguous and dist.flags.c_contiguous):
                raise ValueError("out must be C-contiguous (int32 [hi - lo, k], float32 [hi - lo, k])")
        self._live("SparseIndex.search")
        c = self._ctx
        c._check(c._L.fdr_sparse_index_search(c._h, k, lo, hi, _ptr(idx), _ptr(dist)), "fdr_sparse_index_search")
        return idx, dist

    def query(self, indptr, indices, values, k, out=None, block_rows=None):
        """Neighbours, among the n rows of the index, of query rows that need not be in it: a CSR of their own (indptr
        int64 [nq + 1], indices int32 in [0, n_features) ascending inside a row, values float32 or None: every stored
        entry 1, whatever the index was built with).  Returns (idx int32 [nq, k], dist float32 [nq, k]), idx holding
        rows of the index: fdr_sparse_index_query, under the rules of the index's metric with the query's norm, set
        size or mass formed as a row's of the index is, so the rows [lo, hi) of the indexed CSR give search(k, lo, hi)
        bit for bit.  A zero (empty, zero-mass) query gets the index's first k zero rows at 0, then its first other
        rows at 1.  block_rows: the queries go to the device in consecutive blocks of at most that many rows, each
        with its indptr rebased to 0 (one C call per block: the device's result buffers hold block_rows * k entries);
        the bits do not depend on it.  out=(idx, dist): caller-owned C-contiguous result arrays."""
        if self.n_features is None:
            raise ValueError("SparseIndex.query needs the index's n_features")
        nq, k = check_sparse_queries(self.n, self.n_features, self.metric, indptr, indices, values, k)
        _check_block_rows(block_rows)
        if out is None:
            idx = np.empty((nq, k), dtype=np.int32)
            dist = np.empty((nq, k), dtype=np.float32)
        else:
            idx, dist = out
            if (idx.shape, dist.shape) != ((nq, k), (nq, k)) or idx.dtype != np.int32 or dist.dtype != np.float32 \
                    or not (idx.flags.c_contiguous and dist.flags.c_contiguous):
                raise ValueError("out must be C-contiguous (int32 [nq, k], float32 [nq, k])")
        self._live("SparseIndex.query")
        c = self._ctx
        step = max(nq, 1) if block_rows is None else int(block_rows)
        for a in range(0, max(nq, 1), step):  # (nq = 0: one call, which records the trace)
            b = min(nq, a + step)
            if a == 0 and b == nq:
                ip, ix, vals = indptr, indices, values
            else:
                ip = np.ascontiguousarray(indptr[a:b + 1] - indptr[a])
                ix = indices[indptr[a]:indptr[b]]
                vals = None if values is None else values[indptr[a]:indptr[b]]
            c._check(c._L.fdr_sparse_index_query(c._h, k, b - a, _ptr(ip), _ptr(ix), _ptr(vals), _ptr(idx[a:b]),
                                                 _ptr(dist[a:b])), "fdr_sparse_index_query")
        return idx, dist

    def radius_search(self, radius, lo=0, hi=None, max_hits=1 << 26):
        """Every row of the index within distance `radius` (0 <= radius < 1) of each of the rows [lo, hi) (hi=None: n):
        (indptr int64 [hi - lo + 1], idx int32 [total], dist float32 [total]), row r's hits at [indptr[r], indptr[r + 1])
        in (distance bits, index) order, self among them: fdr_sparse_index_radius_search, the distances a search(k)
        reports, bit for bit.  max_hits caps the hits of one device call (8 bytes each, 8 more of scratch); a range
        with more is cut by its counts into pieces that fit, and the result is the same.  One row with more hits than
        max_hits raises FedrannHipError."""
        if isinstance(lo, bool) or isinstance(hi, bool) or not isinstance(lo, (int, np.integer)) \
                or not (hi is None or isinstance(hi, (int, np.integer))):
            raise ValueError("lo and hi must be integers, got %r, %r" % (lo, hi))
        lo, hi = int(lo), int(self.n if hi is None else hi)
        if not 0 <= lo <= hi <= self.n:
            raise ValueError("need 0 <= lo <= hi <= n = %d, got [%d, %d)" % (self.n, lo, hi))
        r, max_hits = check_sparse_radius(radius, max_hits)
        self._live("SparseIndex.radius_search")
        c = self._ctx

        def piece(a, b):
            return lambda cap, ip: c._L.fdr_sparse_index_radius_search(c._h, r, lo + a, lo + b, cap, _ptr(ip))
        return self._radius_rows("fdr_sparse_index_radius_search", piece, hi - lo, max_hits, lo)

    def radius_query(self, indptr, indices, values, radius, block_rows=None, max_hits=1 << 26):
        """radius_search for query rows that need not be in the index (a CSR as in query(); there is no self):
        fdr_sparse_index_radius_query.  Returns (indptr int64 [nq + 1], idx int32 [total], dist float32 [total]).  The
        index's own rows [lo, hi) give radius_search(radius, lo, hi) bit for bit.  block_rows: the queries go to the
        device in consecutive blocks of at most that many rows; max_hits as in radius_search, per block."""
        if self.n_features is None:
            raise ValueError("SparseIndex.radius_query needs the index's n_features")
        nq = check_sparse_queries(self.n, self.n_features, self.metric, indptr, indices, values, 1)[0]
        _check_block_rows(block_rows)
        r, max_hits = check_sparse_radius(radius, max_hits)
        self._live("SparseIndex.radius_query")
        c = self._ctx

        def piece(a, b):
            if a == 0 and b == nq:
                ip, ix, vals = indptr, indices, values
            else:
                ip = np.ascontiguousarray(indptr[a:b + 1] - indptr[a])
                ix = indices[indptr[a]:indptr[b]]
                vals = None if values is None else values[indptr[a]:indptr[b]]
            return lambda cap, out: c._L.fdr_sparse_index_radius_query(c._h, r, b - a, _ptr(ip), _ptr(ix), _ptr(vals),
                                                                       cap, _ptr(out))
        return self._radius_blocks("fdr_sparse_index_radius_query", piece, nq, block_rows, max_hits)

    def info(self):
        """dict of fdr_sparse_index_info: metric, n, postings (stored entries kept), zero_rows (zero rows; Jaccard:
        empty rows; weighted Jaccard: zero-mass rows), device_bytes (what the index holds on the device)."""
        self._live("SparseIndex.info")
        c = self._ctx
        m, n, p, z = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        b = ctypes.c_size_t()
        c._check(c._L.fdr_sparse_index_info(c._h, ctypes.byref(m), ctypes.byref(n), ctypes.byref(p), ctypes.byref(z),
                                            ctypes.byref(b)), "fdr_sparse_index_info")
        name = [s for s, v in SPARSE_METRICS.items() if v == m.value][0]
        return {"metric": name, "n": int(n.value), "postings": int(p.value), "zero_rows": int(z.value),
                "device_bytes": int(b.value)}

    def close(self):
        """Free the index's device memory (if it still is the context's index)."""
        c = self._ctx
        if self._open and getattr(c, "_h", None) and c._sparse_gen == self._gen:
            c._check(c._L.fdr_sparse_index_free(c._h), "fdr_sparse_index_free")
        self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DenseIndex(_HeldIndex):
    """The dense index of a Context (Context.dense_index / dense_index_from_csr): radius searches on the projected rows,
    any number of times.  The index lives in the context, which holds one: once the context has built another, or
    after close(), the calls raise FedrannHipError."""

    _kind, _gen_attr, _fetch, _counted = "dense", "_dense_gen", "fdr_dense_index_radius_fetch", "candidates"
    _exact_counts = False  # (a refusal leaves candidate counts: upper bounds of what the pieces return)

    def __init__(self, ctx, n, d, gen):
        self._ctx, self.n, self.d, self._gen = ctx, int(n), int(d), gen
        self._open = True

    def radius_search(self, radius, lo=0, hi=None, max_hits=1 << 26):
        """Every row of the index within cosine distance `radius` (0 <= radius < 1) of each of the rows [lo, hi)
        (hi=None: n): (indptr int64 [hi - lo + 1], idx int32 [total], dist float32 [total]), row r's hits at
        [indptr[r], indptr[r + 1]) in (distance bits, index) order, self among them: fdr_dense_index_radius_search, the
        distances knn(E, k) reports, bit for bit.  max_hits caps the fp16 CANDIDATES of one device call (16 bytes
        each); a range with more is cut by its candidate counts into pieces that fit, and the result is the same.  One
        row with more candidates than max_hits raises FedrannHipError."""
        r, lo, hi, max_hits = check_dense_radius(self.n, self.d, radius, lo, hi, max_hits)
        self._live("DenseIndex.radius_search")
        c = self._ctx

        def piece(a, b):
            return lambda cap, ip: c._L.fdr_dense_index_radius_search(c._h, r, lo + a, lo + b, cap, _ptr(ip))
        return self._radius_rows("fdr_dense_index_radius_search", piece, hi - lo, max_hits, lo)

    def radius_query(self, Q, radius, block_rows=None, max_hits=1 << 26):
        """radius_search for query rows Q float32 [nq, d] that need not be in the index (not normalised; there is no
        self): fdr_dense_index_radius_query.  Returns (indptr int64 [nq + 1], idx int32 [total], dist float32
        [total]).  The rows [lo, hi) of the indexed E give radius_search(radius, lo, hi) bit for bit.  block_rows: the
        queries go to the device in consecutive blocks of at most that many rows; max_hits as in radius_search, per
        block."""
        Q = _as(Q, np.float32, "Q")
        if Q.ndim != 2 or Q.shape[1] != self.d:
            raise ValueError("Q must be [nq, %d], got shape %r" % (self.d, Q.shape))
        nq = Q.shape[0]
        _check_block_rows(block_rows)
        r, _, _, max_hits = check_dense_radius(self.n, self.d, radius, 0, None, max_hits)
        self._live("DenseIndex.radius_query")
        c = self._ctx

        def piece(a, b):
            rows = Q[a:b]  # (a row block of a C-contiguous array is C-contiguous)
            return lambda cap, out: c._L.fdr_dense_index_radius_query(c._h, r, b - a, _ptr(rows) if b > a else None,
                                                                      cap, _ptr(out))
        return self._radius_blocks("fdr_dense_index_radius_query", piece, nq, block_rows, max_hits)

    def info(self):
        """dict of fdr_dense_index_info: n, d, device_bytes (what the dense index holds on the device, the radius
        calls' buffers included) and, of the last radius call, last_candidates (fp16 candidates), last_hits,
        last_query_blocks and last_segments (the grid of its range pass)."""
        self._live("DenseIndex.info")
        c = self._ctx
        n, d, b = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_size_t()
        lc, lh, qb, sg = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        c._check(c._L.fdr_dense_index_info(c._h, ctypes.byref(n), ctypes.byref(d), ctypes.byref(b), ctypes.byref(lc),
                                           ctypes.byref(lh), ctypes.byref(qb), ctypes.byref(sg)), "fdr_dense_index_info")
        return {"n": int(n.value), "d": int(d.value), "device_bytes": int(b.value), "last_candidates": int(lc.value),
                "last_hits": int(lh.value), "last_query_blocks": int(qb.value), "last_segments": int(sg.value)}

    def close(self):
        """Free the index's device memory (if it still is the context's dense index)."""
        c = self._ctx
        if self._open and getattr(c, "_h", None) and c._dense_gen == self._gen:
            c._check(c._L.fdr_dense_index_free(c._h), "fdr_dense_index_free")
        self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class RescoreRows(_HeldIndex):
    """The re-score row set of a Context (Context.rescore_rows): candidate lists, rectangular (knn) or ragged (radius),
    scored exactly on the held rows, any number of times.  The rows live in the context, which holds one set: once
    the context has built another, or after close(), the calls raise FedrannHipError."""

    _kind, _gen_attr, _fetch, _counted = "re-score row", "_rescore_gen", "fdr_rescore_rows_radius_fetch", "candidates"

    def __init__(self, ctx, n, metric, gen):
        self._ctx, self.n, self.metric, self._gen = ctx, int(n), metric, gen
        self._open = True

    def knn(self, candidates, k=None, q_lo=0, out=None):
        """Context.sparse_rescore on the held rows, without its upload: candidates int32 [nq, k_in], row r the
        candidates of query q_lo + r.  Returns (idx int32 [nq, k], dist float32 [nq, k]), the bits sparse_rescore
        gives on the same CSR (fdr_rescore_rows_knn).  A held radius result stays as it is."""
        nq, k_in, k, q_lo = check_rescore_args(self.n, candidates, k, self.metric, q_lo, out)
        idx, dist = out if out is not None else (np.empty((nq, k), np.int32), np.empty((nq, k), np.float32))
        self._live("RescoreRows.knn")
        c = self._ctx
        c._check(c._L.fdr_rescore_rows_knn(c._h, q_lo, nq, k_in, _ptr(candidates), k, _ptr(idx), _ptr(dist)),
                 "fdr_rescore_rows_knn")
        return idx, dist

    def radius(self, cand_indptr, cand_idx, radius, q_lo=0, max_entries=1 << 26):
        """Ragged candidate rows re-scored and cut by `radius` in the exact metric: row r of (cand_indptr int64
        [nq + 1], cand_idx int32) holds the candidates of query q_lo + r, rows of the set in any number and order
        (DenseIndex.radius_search's rows, for one).  Returns (indptr int64 [nq + 1], idx int32, dist float32): row r
        holds that row's candidates with distance <= radius (0 <= radius <= 1; 1 keeps them all), the distance the
        float32 sparse_rescore and knn_sparse report for the pair, in (distance bits, index) order
        (fdr_rescore_rows_radius).  The query's own index is an ordinary candidate (distance 0); a repeated candidate
        comes out as often as it goes in; one outside [0, n) is refused (FedrannHipError).  The queries go to the device
        in consecutive pieces of at most max_entries candidates (20 device bytes each); one query with more is a
        ValueError that names it."""
        nq, r, q_lo, counts = check_rescore_ragged(self.n, cand_indptr, cand_idx, radius, q_lo)
        if isinstance(max_entries, bool) or not isinstance(max_entries, (int, np.integer)) \
                or not 1 <= int(max_entries) < 2 ** 31:
            raise ValueError("max_entries must be an integer in [1, 2^31), got %r" % (max_entries,))
        max_entries = int(max_entries)
        # (everything in one piece: the common case, without the walk over the counts)
        pieces = [(0, nq)] if int(cand_indptr[-1]) <= max_entries else radius_pieces(counts, max_entries)
        if pieces is None:
            q = int(np.argmax(counts > max_entries))
            raise ValueError("query %d alone has %d candidates, above max_entries = %d"
                             % (q_lo + q, int(counts[q]), max_entries))
        self._live("RescoreRows.radius")
        c = self._ctx
        outs = []
        for a, b in pieces:
            if a == 0 and b == nq:
                ip_in, ix_in = cand_indptr, cand_idx
            else:
                ip_in = np.ascontiguousarray(cand_indptr[a:b + 1] - cand_indptr[a])
                ix_in = cand_idx[cand_indptr[a]:cand_indptr[b]]
            ip = np.full(b - a + 1, -1, dtype=np.int64)
            c._check(c._L.fdr_rescore_rows_radius(c._h, r, q_lo + a, b - a, _ptr(ip_in), _ptr(ix_in), _ptr(ip)),
                     "fdr_rescore_rows_radius")
            total = int(ip[-1])
            idx = np.empty(total, dtype=np.int32)
            dist = np.empty(total, dtype=np.float32)
            c._check(c._L.fdr_rescore_rows_radius_fetch(c._h, total, _ptr(idx), _ptr(dist)), self._fetch)
            outs.append((ip, idx, dist))
        if len(outs) == 1:
            return outs[0]
        out_ip = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum(np.concatenate([np.diff(o[0]) for o in outs]), out=out_ip[1:])
        return out_ip, np.concatenate([o[1] for o in outs]), np.concatenate([o[2] for o in outs])

    def refine(self, graph, k, fan=None, radius=1.0, reverse=False, block_rows=None, max_entries=1 << 27):
        """One refinement step of the neighbour lists `graph` (as Context.graph_symmetrize takes it, on the set's n
        rows): every row's candidates are its `fan` nearest entries and the `fan` nearest of each of those
        (Context.graph_expand), scored exactly on the held rows, cut by `radius` (0 <= radius <= 1; 1 keeps all) and to
        the k best.  Returns the ragged (indptr int64 [n + 1], idx int32, dist float32) over all rows, every row
        ascending by (distance bits, index) and of at most k entries: what radius(*graph_expand(graph, fan), radius)
        gives, each row cut to k.  The candidates never leave the device (fdr_graph_expand, fdr_rescore_rows_refine,
        fdr_rescore_rows_radius_fetch per block of rows).  fan: min(k, FDR_MAX_K) by default.  reverse=True first
        takes Context.graph_symmetrize(graph, "union"), so a row's listers are candidates too (NN-descent's reverse
        neighbours; a hub is bounded by the fan cut).  The rows go in consecutive blocks: of block_rows rows, or, by
        default, as many as keep fan-cut length * (1 + fan), an upper bound of a row's candidates that needs the row
        pointer alone, within max_entries in sum (one row above it is a ValueError).  A row's own index is a
        candidate exactly when the row lists itself inside its fan."""
        from . import graph as _graph
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) < 2 ** 31:
            raise ValueError("k must be an integer in [1, 2^31), got %r" % (k,))
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
            raise ValueError("radius must be a number, got %r" % (radius,))
        r = np.float32(radius)
        if not (r >= 0 and r <= 1):
            raise ValueError("need 0 <= radius <= 1, got %r" % (radius,))
        r = r + np.float32(0)  # (-0.0 is 0)
        _check_block_rows(block_rows)
        fan = min(int(k), FDR_MAX_K) if fan is None else fan
        n, indptr, idx, dist, fan, _, _ = check_graph_expand(graph, fan, 0, None, max_entries)
        if n != self.n:
            raise ValueError("the graph has %d rows, the re-score rows are %d" % (n, self.n))
        self._live("RescoreRows.refine")
        c = self._ctx
        if reverse:
            indptr, idx, dist = c.graph_symmetrize((indptr, idx, dist), "union", max_entries=2 ** 31 - 1)
        if block_rows is None:
            pieces = expand_pieces(_graph.expand_bound(indptr, fan), int(max_entries))
            if pieces is None:
                raise ValueError("one row alone may have more than max_entries = %d candidates at fan = %d"
                                 % (int(max_entries), fan))
        else:
            pieces = [(a, min(n, a + int(block_rows))) for a in range(0, n, int(block_rows))]
        outs = []
        for a, b in pieces:
            c._graph_expand_held(n, indptr, idx, dist, fan, a, b, max_entries)
            ip = np.full(b - a + 1, -1, dtype=np.int64)
            c._check(c._L.fdr_rescore_rows_refine(c._h, r, int(min(int(k), 2 ** 31 - 1)), _ptr(ip)),
                     "fdr_rescore_rows_refine")
            total = int(ip[-1])
            out_idx, out_dist = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.float32)
            c._check(c._L.fdr_rescore_rows_radius_fetch(c._h, total, _ptr(out_idx), _ptr(out_dist)), self._fetch)
            outs.append((ip, out_idx, out_dist))
        if len(outs) == 1:
            return outs[0]
        out_ip = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.concatenate([np.diff(o[0]) for o in outs]), out=out_ip[1:])
        return out_ip, np.concatenate([o[1] for o in outs]), np.concatenate([o[2] for o in outs])

    def info(self):
        """dict of fdr_rescore_rows_info: metric, n, stored (stored entries), device_bytes (what the row set holds on
        the device, the calls' buffers included)."""
        self._live("RescoreRows.info")
        c = self._ctx
        m, n, s, b = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
        c._check(c._L.fdr_rescore_rows_info(c._h, ctypes.byref(m), ctypes.byref(n), ctypes.byref(s), ctypes.byref(b)),
                 "fdr_rescore_rows_info")
        name = [k for k, v in SPARSE_METRICS.items() if v == m.value][0]
        return {"metric": name, "n": int(n.value), "stored": int(s.value), "device_bytes": int(b.value)}

    def close(self):
        """Free the row set's device memory (if it still is the context's row set)."""
        c = self._ctx
        if self._open and getattr(c, "_h", None) and c._rescore_gen == self._gen:
            c._check(c._L.fdr_rescore_rows_free(c._h), "fdr_rescore_rows_free")
        self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


_default_ctx = None


def default_context():
    """Process-wide context on device $FEDRANN_DEVICE (default: LOCAL_RANK, else 0)."""
    global _default_ctx
    if _default_ctx is None:
        dev = int(os.environ.get("FEDRANN_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _default_ctx = Context(dev)
    return _default_ctx
