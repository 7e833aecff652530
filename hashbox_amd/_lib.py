"""ctypes binding of libhbxgpu.so (the C-ABI declared in include/hbxgpu.h).

There is no fallback: if the library is missing or cannot load, importing the
engine raises.  Build it with ``python -m hashbox_amd.build``.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# The in-tree build only: no environment override, so a variant build can
# never stand in for the product silently (A/B runs copy a variant over this
# file explicitly, tools/gpu_ab.sh).
LIB_PATH = os.path.join(HERE, "libhbxgpu.so")

HBX_OK = 0
ERRORS = {-1: "HBX_ERR_ARG", -2: "HBX_ERR_HIP", -3: "HBX_ERR_CAPACITY", -4: "HBX_ERR_IO",
          -5: "HBX_ERR_NODEV", -6: "HBX_ERR_STATE", -7: "HBX_ERR_FORMAT", -8: "HBX_ERR_SINK", -9: "HBX_ERR_VERIFY"}

# Every symbol include/hbxgpu.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "hbx_version", "hbx_device_count", "hbx_max_chunks", "hbx_ctx_create", "hbx_ctx_destroy",
    "hbx_last_error", "hbx_chunk_hash", "hbx_chunk_hash_batch", "hbx_chunk_hash_device",
    "hbx_submit_device", "hbx_wait", "hbx_store_paths", "hbx_block_id", "hbx_md5", "hbx_arena_alloc", "hbx_arena_free",
    "hbx_memcpy_h2d", "hbx_memcpy_h2d_async", "hbx_alloc_pinned", "hbx_free_pinned", "hbx_stage_times",
    "hbx_set_tile_iters", "hbx_pending", "hbx_set_md5_slice", "hbx_stage_totals", "hbx_io_times",
    "hbx_reserve", "hbx_verify_blocks", "hbx_verify_blocks_device",
    "hbx_file_entry_size", "hbx_file_entry_serialize", "hbx_file_entry_parse",
    "hbx_chain_block_serialize", "hbx_chain_block_parse", "hbx_directory_block_size",
    "hbx_directory_block_serialize", "hbx_directory_block_parse", "hbx_directory_block_ids",
    "hbx_deflate_bound", "hbx_deflate_blocks_device", "hbx_deflate_blocks",
    "hbx_deflate_file_bound", "hbx_store_paths_z",
    "hbx_wire_encode_id", "hbx_wire_encode_block_header", "hbx_wire_parse",
    "hbx_verify_submit_device", "hbx_inflate_blocks_device", "hbx_store_paths_zcb", "hbx_after_stream",
    "hbx_set_join_lag", "hbx_set_k3_period", "hbx_k3_wave_times", "hbx_input_after_oldest", "hbx_knobs",
    "hbx_input_fence", "hbx_set_k3_probe", "hbx_store_paths_status", "hbx_plan_pipeline", "hbx_apply_plan",
    "hbx_host_call_max",
    "hbx_seg_next", "hbx_seg_open", "hbx_seg_close", "hbx_seg_submit_device", "hbx_store_file_seg",
    "hbx_idset_slots", "hbx_idset_create", "hbx_idset_destroy", "hbx_idset_insert", "hbx_idset_contains",
    "hbx_idset_stats", "hbx_idset_export", "hbx_idset_truncate", "hbx_submit_device_dd", "hbx_store_paths_dd",
    "hbx_seg_submit_device_dd", "hbx_store_file_stream",
    "hbx_restore_in_bound", "hbx_restore_blocks", "hbx_restore_file_stream",
    "hbx_restore_many_window", "hbx_restore_files_blocks", "hbx_restore_files_stream",
    "hbx_match_chains", "hbx_submit_device_match", "hbx_store_paths_match",
    "hbx_k1_summaries", "hbx_locate_ids",
    "hbx_datfile_header_parse", "hbx_datfile_entry_parse", "hbx_datfile_walk",
    "hbx_datfile_check_device", "hbx_datfile_check_path", "hbx_datfile_verify_at",
    "hbx_block_graph",
    "hbx_datfile_compact_plan", "hbx_datfile_compact_device", "hbx_datfile_compact_path",
    "hbx_index_open", "hbx_index_open_paths", "hbx_index_close", "hbx_index_sizes", "hbx_index_export",
    "hbx_index_lookup", "hbx_index_scan", "hbx_index_mark", "hbx_index_update", "hbx_index_sweep",
    "hbx_index_compact", "hbx_index_lookup_host", "hbx_index_scan_host", "hbx_index_mark_host",
    "hbx_index_update_host", "hbx_index_sweep_host", "hbx_index_compact_host",
]
# Functions returning something other than an int status.
_NON_STATUS = ("hbx_ctx_destroy", "hbx_last_error", "hbx_max_chunks", "hbx_file_entry_size",
               "hbx_directory_block_size", "hbx_deflate_bound", "hbx_deflate_file_bound", "hbx_idset_slots",
               "hbx_restore_in_bound")


class FileEntry(ctypes.Structure):
    """hbx_file_entry: hashback FileEntry (hashback/hashback.go:80-90)."""
    _fields_ = [("name", ctypes.c_void_p), ("name_len", ctypes.c_uint32), ("file_mode", ctypes.c_uint32),
                ("file_size", ctypes.c_int64), ("mod_time", ctypes.c_int64),
                ("reference_id", ctypes.c_uint8 * 16), ("content_id", ctypes.c_uint8 * 16),
                ("decrypt_key", ctypes.c_uint8 * 16), ("link", ctypes.c_void_p), ("link_len", ctypes.c_uint32),
                ("content_type", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3)]


class WireMsg(ctypes.Structure):
    """hbx_wire_msg: one parsed protocol message (pkg/core/protocol.go)."""
    _fields_ = [("num", ctypes.c_uint16), ("type", ctypes.c_uint32), ("id", ctypes.c_uint8 * 16),
                ("n_links", ctypes.c_uint32), ("links", ctypes.c_void_p), ("data_type", ctypes.c_uint8),
                ("data_len", ctypes.c_uint32), ("data", ctypes.c_void_p), ("header_len", ctypes.c_uint64),
                ("total_len", ctypes.c_uint64)]


class FileSummary(ctypes.Structure):
    _fields_ = [("content_id", ctypes.c_uint8 * 16), ("content_type", ctypes.c_int32),
                ("n_chunks", ctypes.c_uint32)]


class PlanRequest(ctypes.Structure):
    """hbx_plan_request (include/hbxgpu.h)."""
    _fields_ = [("n_files", ctypes.c_uint64), ("arena_bytes", ctypes.c_uint64), ("longest_file", ctypes.c_uint64),
                ("free_bytes", ctypes.c_uint64), ("hbm_frac", ctypes.c_double),
                ("ranks_per_device", ctypes.c_uint32), ("steps", ctypes.c_uint32), ("arenas", ctypes.c_int32),
                ("md5_slice", ctypes.c_int32), ("join_lag", ctypes.c_int32), ("lead", ctypes.c_int32),
                ("k3_period", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class PipelinePlan(ctypes.Structure):
    """hbx_pipeline_plan (include/hbxgpu.h)."""
    _fields_ = [("resident", ctypes.c_uint32), ("md5_slice", ctypes.c_uint32), ("join_lag", ctypes.c_uint32),
                ("lead", ctypes.c_uint32), ("k3_period", ctypes.c_uint32), ("launches_per_batch", ctypes.c_uint32),
                ("hbm_bytes", ctypes.c_uint64)]


PLAN_HOST_INPUT = 1
PLAN_ARENA_SLACK = 64 << 20

# hbx_batch_ready_fn (include/hbxgpu.h)
BATCH_READY = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64)

STREAM_COMPRESS = 1  # HBX_STREAM_COMPRESS


class SegChunks(ctypes.Structure):
    """hbx_seg_chunks: what one segment of hbx_store_file_stream completed."""
    _fields_ = [("first_chunk", ctypes.c_uint64), ("n_chunks", ctypes.c_uint64), ("cut_ends", ctypes.c_void_p),
                ("ids", ctypes.c_void_p), ("fresh", ctypes.c_void_p), ("z", ctypes.c_void_p),
                ("zoff", ctypes.c_void_p), ("zlen", ctypes.c_void_p), ("final", ctypes.c_int),
                ("summary", FileSummary)]


# hbx_seg_sink_fn (include/hbxgpu.h)
SEG_SINK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(SegChunks))

# hbx_block_source_fn / hbx_restore_sink_fn (include/hbxgpu.h)
BLOCK_SOURCE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8))
RESTORE_SINK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64)
# hbx_file_block_source_fn (include/hbxgpu.h)
FILE_BLOCK_SOURCE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8))


class RestoredFile(ctypes.Structure):
    """hbx_restored_file: one file's result of hbx_restore_files_stream."""
    _fields_ = [("bytes", ctypes.c_uint64), ("n_good", ctypes.c_uint64), ("bad_index", ctypes.c_uint64),
                ("first_diff", ctypes.c_uint64), ("bad_status", ctypes.c_uint32), ("err", ctypes.c_int32)]


class ChainMatch(ctypes.Structure):
    """hbx_chain_match: one file's local ID list against its stored chain (K12)."""
    _fields_ = [("n_match", ctypes.c_uint32), ("n_local", ctypes.c_uint32), ("n_expect", ctypes.c_uint32),
                ("same", ctypes.c_uint32), ("match_bytes", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class BlockLoc(ctypes.Structure):
    """hbx_block_loc: where the pool holds one wanted block ID (K13)."""
    _fields_ = [("file", ctypes.c_uint32), ("chunk", ctypes.c_uint32), ("off", ctypes.c_uint64),
                ("len", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class DatRecord(ctypes.Structure):
    """hbx_dat_record: one position of a data file as K14's parse frames it."""
    _fields_ = [("off", ctypes.c_uint64), ("size", ctypes.c_uint64), ("data_off", ctypes.c_uint64),
                ("links_off", ctypes.c_uint64), ("data_len", ctypes.c_uint32), ("n_links", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("type", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("pad", ctypes.c_uint16), ("id", ctypes.c_uint8 * 16)]


class DatEntry(ctypes.Structure):
    """hbx_dat_entry: a good entry on the walk of a data file."""
    _fields_ = [("off", ctypes.c_uint64), ("size", ctypes.c_uint64), ("data_off", ctypes.c_uint64),
                ("link_base", ctypes.c_uint64), ("n_links", ctypes.c_uint32), ("data_len", ctypes.c_uint32),
                ("plain_len", ctypes.c_uint32), ("type", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3),
                ("id", ctypes.c_uint8 * 16)]


class DatSpan(ctypes.Structure):
    """hbx_dat_span: a gap or a broken span of a data file."""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("kind", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("n_failed", ctypes.c_uint64)]


class DatSummary(ctypes.Structure):
    """hbx_dat_summary: what a check of a data file found."""
    _fields_ = [("size", ctypes.c_uint64), ("filetype", ctypes.c_uint32), ("version", ctypes.c_uint32),
                ("deadspace", ctypes.c_uint64), ("header_ok", ctypes.c_uint32), ("gap_past_eof", ctypes.c_uint32),
                ("n_candidates", ctypes.c_uint64), ("n_gap_markers", ctypes.c_uint64), ("n_valid", ctypes.c_uint64),
                ("n_unreached", ctypes.c_uint64), ("n_entries", ctypes.c_uint64), ("entry_bytes", ctypes.c_uint64),
                ("n_gaps", ctypes.c_uint64), ("gap_bytes", ctypes.c_uint64), ("n_broken", ctypes.c_uint64),
                ("broken_bytes", ctypes.c_uint64), ("n_spans", ctypes.c_uint64), ("n_links", ctypes.c_uint64),
                ("truncate_at", ctypes.c_uint64)]


class GraphSummary(ctypes.Structure):
    """hbx_graph_summary: what hbx_block_graph found (K15)."""
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "n_rows", "n_links", "n_alias", "n_missing_links", "n_roots", "n_roots_missing", "n_marked", "mark_levels",
        "n_faulty", "n_invalid", "fault_levels", "n_marked_faulty")]


class DatCompactArgs(ctypes.Structure):
    """hbx_dat_compact_args: where a compaction's outputs will lie (K16)."""
    _fields_ = [("file_no", ctypes.c_uint32), ("dst_file_no", ctypes.c_uint32), ("dst_base", ctypes.c_uint64),
                ("meta_file_no", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("meta_base", ctypes.c_uint64)]


class DatCompactSummary(ctypes.Structure):
    """hbx_dat_compact_summary: what a compaction does to a data file (K16)."""
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "n_entries", "n_stay", "n_moved", "n_dropped", "stay_end", "moved_bytes", "dropped_bytes", "deleted_bytes",
        "meta_bytes", "n_meta", "first_past_limit")]


IX_FILES_MAX = 16  # HBX_IX_FILES_MAX


class IxFileStats(ctypes.Structure):
    """hbx_ix_file_stats: what a scan of one index file found (K17)."""
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "slots", "n_live", "n_invalid", "n_empty", "n_marked", "n_nolinks", "n_misplaced", "first_misplaced",
        "trunc_point")]


class IxSummary(ctypes.Structure):
    """hbx_ix_summary: a scan's counts over all index files (K17)."""
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "n_files", "slots", "n_live", "n_invalid", "n_empty", "n_marked", "n_nolinks", "n_misplaced", "n_obsolete",
        "n_cut_off")]


class IxSweepSummary(ctypes.Structure):
    """hbx_ix_sweep_summary: what SweepIndexes did (K17)."""
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "n_live", "n_deleted", "n_stay", "n_obsolete", "n_moved", "n_abort", "first_abort", "swept_records",
        "n_grown")]


class IxCompactSummary(ctypes.Structure):
    """hbx_ix_compact_summary: what CompactIndexes did (K17)."""
    _fields_ = [("n_files", ctypes.c_uint64), ("cleared", ctypes.c_uint64), ("size", ctypes.c_uint64 * IX_FILES_MAX)]


CMP_DROP, CMP_STAY, CMP_MOVE = 0, 1, 2  # HBX_CMP_*
CMP_F_KEEP_PREFIX = 1                   # HBX_CMP_F_KEEP_PREFIX
DAT_OFFSET_LIMIT = (1 << 34) - 1        # HBX_DAT_OFFSET_LIMIT
DAT_FILE_MAX = 0x3FFF                   # HBX_DAT_FILE_MAX
IX_F_EXISTS, IX_F_NOLINKS = 1, 2        # HBX_IX_F_*
IX_F_MARKED, IX_F_INVALID = 4, 8        # HBX_IX_F_*
IX_HEADER, IX_PROBE_LIMIT = 16, 682     # HBX_IX_HEADER, HBX_IX_PROBE_LIMIT
IX_SLOTS_MAX = (1 << 24) + 682          # HBX_IX_SLOTS_MAX
IX_SWEEP_TILE = 256                     # HBX_IX_SWEEP_TILE
IX_ACT_DELETED, IX_ACT_STAY, IX_ACT_OBSOLETE, IX_ACT_MOVED, IX_ACT_ABORT = 1, 2, 3, 4, 5  # HBX_IX_ACT_*
META_HEAD, IX_ENTRY = 34, 24            # HBX_META_HEAD, HBX_IX_ENTRY
GRAPH_NONE = 0xFFFFFFFF             # HBX_GRAPH_NONE
GRAPH_LANE_MAX, GRAPH_WAVE_MAX = 16, 4096  # HBX_GRAPH_LANE_MAX, HBX_GRAPH_WAVE_MAX (hbx_knobs reports them)
DAT_HEADER, DAT_IMAGE_SLACK = 16, 64            # HBX_DAT_HEADER, HBX_DAT_IMAGE_SLACK
DAT_ST_INVALID, DAT_ST_WRONG_ID = 9, 10         # HBX_DAT_ST_*
DAT_F_MARKER, DAT_F_GAP = 1, 2                  # HBX_DAT_F_*
DAT_SPAN_GAP, DAT_SPAN_BROKEN = 0, 1            # HBX_DAT_SPAN_*
NO_FILE = 0xFFFFFFFF                # hbx_block_loc.file of an ID the pool does not hold
BLOCK_RAW, BLOCK_ZLIB = 0xFF, 0x01  # HBX_BLOCK_RAW, HBX_BLOCK_ZLIB
MAX_BLOCK = 8 << 20                 # HBX_MAX_BLOCK
ERR_IO, ERR_VERIFY = -4, -9
ERR_CAPACITY = -3
ERR_ARG, ERR_STATE, ERR_FORMAT = -1, -6, -7
NO_DIFF = (1 << 64) - 1             # first_diff when nothing differs

_lib = None


def identity() -> dict:
    """Which library this process runs: path and content hash (bench.py
    prints it in its JSON line)."""
    import hashlib
    with open(LIB_PATH, "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()[:16]
    return {"path": os.path.relpath(LIB_PATH, os.path.dirname(HERE)), "sha256_16": sha}


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64
    # (same soname libamdhip64.so.7).  Loading torch first makes our NEEDED
    # entry bind to that copy; loading ours first would put a second HIP/HSA
    # runtime in the process and torch would then see no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m hashbox_amd.build` "
                           "(the engine has no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    U64 = ctypes.c_uint64
    I = ctypes.c_int
    L.hbx_version.restype = I
    L.hbx_device_count.argtypes = [ctypes.POINTER(I)]
    L.hbx_max_chunks.argtypes = [U64]
    L.hbx_max_chunks.restype = U64
    L.hbx_ctx_create.argtypes = [I, ctypes.POINTER(P)]
    L.hbx_ctx_destroy.argtypes = [P]
    L.hbx_ctx_destroy.restype = None
    L.hbx_last_error.argtypes = [P]
    L.hbx_last_error.restype = ctypes.c_char_p
    L.hbx_chunk_hash.argtypes = [P, P, U64, P, P, U64, ctypes.POINTER(U64)]
    L.hbx_chunk_hash_batch.argtypes = [P, U64, P, P, P, P, P, P, P]
    L.hbx_chunk_hash_device.argtypes = [P, P, U64, P, P, P, P, P, P, P]
    L.hbx_submit_device.argtypes = [P, P, U64, P, P, P, P, P, P, P]
    L.hbx_wait.argtypes = [P]
    L.hbx_store_paths.argtypes = [P, U64, P, P, P, P, P, P, P, ctypes.c_uint32, U64]
    L.hbx_block_id.argtypes = [P, P, ctypes.c_uint32, P, U64, P]
    L.hbx_md5.argtypes = [P, P, U64, P]
    L.hbx_arena_alloc.argtypes = [P, U64, ctypes.POINTER(P)]
    L.hbx_arena_free.argtypes = [P, P]
    L.hbx_memcpy_h2d.argtypes = [P, P, P, U64]
    L.hbx_memcpy_h2d_async.argtypes = [P, P, P, U64]
    L.hbx_after_stream.argtypes = [P, P]
    L.hbx_alloc_pinned.argtypes = [U64, ctypes.POINTER(P)]
    L.hbx_free_pinned.argtypes = [P]
    L.hbx_stage_times.argtypes = [P, ctypes.POINTER(ctypes.c_float)]
    L.hbx_set_tile_iters.argtypes = [P, ctypes.c_uint32]
    L.hbx_pending.argtypes = [P]
    L.hbx_set_md5_slice.argtypes = [P, ctypes.c_uint32]
    L.hbx_set_join_lag.argtypes = [P, ctypes.c_uint32]
    L.hbx_set_k3_period.argtypes = [P, ctypes.c_uint32]
    L.hbx_input_after_oldest.argtypes = [P]
    L.hbx_input_fence.argtypes = [P, P]
    L.hbx_set_k3_probe.argtypes = [P, I]
    L.hbx_k3_wave_times.argtypes = [P, P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    L.hbx_k1_summaries.argtypes = [P, P, P, U64, ctypes.POINTER(U64), P, U64, ctypes.POINTER(U64)]
    L.hbx_knobs.argtypes = [P, ctypes.c_char_p, U64]
    L.hbx_stage_totals.argtypes = [P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(U64), I]
    L.hbx_io_times.argtypes = [P, ctypes.POINTER(ctypes.c_double), I]
    L.hbx_host_call_max.argtypes = [P, ctypes.POINTER(ctypes.c_double), I]
    L.hbx_reserve.argtypes = [P, ctypes.c_uint32, U64, U64]
    L.hbx_verify_blocks.argtypes = [P, U64, P, P, P, P, P, P, P, P, ctypes.POINTER(U64)]
    L.hbx_verify_blocks_device.argtypes = [P, P, U64, P, P, P, P, P, P, P, P, ctypes.POINTER(U64)]
    PU64 = ctypes.POINTER(U64)
    PU32 = ctypes.POINTER(ctypes.c_uint32)
    L.hbx_file_entry_size.argtypes = [P]
    L.hbx_file_entry_size.restype = U64
    L.hbx_file_entry_serialize.argtypes = [P, P, U64, PU64]
    L.hbx_file_entry_parse.argtypes = [P, U64, P, PU64]
    L.hbx_chain_block_serialize.argtypes = [P, P, ctypes.c_uint32, P, U64, PU64]
    L.hbx_chain_block_parse.argtypes = [P, U64, PU32, P, P, ctypes.c_uint32]
    L.hbx_directory_block_size.argtypes = [P, ctypes.c_uint32]
    L.hbx_directory_block_size.restype = U64
    L.hbx_directory_block_serialize.argtypes = [P, ctypes.c_uint32, P, U64, PU64, P, PU32]
    L.hbx_directory_block_parse.argtypes = [P, U64, P, ctypes.c_uint32, PU32]
    L.hbx_directory_block_ids.argtypes = [P, ctypes.c_uint32, P, P, P, P]
    L.hbx_deflate_bound.argtypes = [U64]
    L.hbx_deflate_bound.restype = U64
    L.hbx_deflate_blocks_device.argtypes = [P, P, U64, P, P, P, P, P, P]
    L.hbx_deflate_blocks.argtypes = [P, U64, P, P, P, P, P]
    L.hbx_deflate_file_bound.argtypes = [U64]
    L.hbx_deflate_file_bound.restype = U64
    L.hbx_wire_encode_id.argtypes = [ctypes.c_uint16, ctypes.c_uint32, P, P]
    L.hbx_wire_encode_block_header.argtypes = [ctypes.c_uint16, ctypes.c_uint32, P, P, ctypes.c_uint32,
                                               ctypes.c_uint8, ctypes.c_uint32, P, U64, PU64]
    L.hbx_wire_parse.argtypes = [P, U64, P]
    L.hbx_store_paths_zcb.argtypes = [P, U64, P, P, P, P, P, P, P, ctypes.c_uint32, U64, P, P, P, P, P, P]
    L.hbx_inflate_blocks_device.argtypes = [P, P, U64, P, P, P, P, P, P, P]
    L.hbx_verify_submit_device.argtypes = [P, P, U64, P, P, P, P, P, P, P, P, PU64]
    L.hbx_store_paths_z.argtypes = [P, U64, P, P, P, P, P, P, P, ctypes.c_uint32, U64, P, P, P, P]
    L.hbx_store_paths_status.argtypes = [P, U64, P, P, P, P, P, P, P, P, ctypes.c_uint32, U64, P, P, P, P, P, P]
    L.hbx_plan_pipeline.argtypes = [P, ctypes.POINTER(PlanRequest), ctypes.POINTER(PipelinePlan)]
    L.hbx_apply_plan.argtypes = [P, ctypes.POINTER(PipelinePlan), U64, U64]
    L.hbx_seg_next.argtypes = [U64, U64, U64, PU64, PU64]
    L.hbx_seg_open.argtypes = [P, U64, ctypes.POINTER(P)]
    L.hbx_seg_close.argtypes = [P, P]
    L.hbx_seg_submit_device.argtypes = [P, U64, P, P, P, P, P, P, P, P, P]
    L.hbx_store_file_seg.argtypes = [P, ctypes.c_char_p, U64, U64, ctypes.c_uint32, P, P, U64, P]
    L.hbx_idset_slots.argtypes = [U64]
    L.hbx_idset_slots.restype = U64
    L.hbx_idset_create.argtypes = [P, U64, ctypes.POINTER(P)]
    L.hbx_idset_destroy.argtypes = [P, P]
    L.hbx_idset_insert.argtypes = [P, P, U64, P, P]
    L.hbx_idset_contains.argtypes = [P, P, U64, P, P]
    L.hbx_idset_stats.argtypes = [P, P, PU64, PU64, PU64, PU64]
    L.hbx_idset_export.argtypes = [P, P, P, U64, PU64]
    L.hbx_idset_truncate.argtypes = [P, P, U64]
    L.hbx_submit_device_dd.argtypes = L.hbx_submit_device.argtypes + [P, P]
    L.hbx_store_paths_dd.argtypes = L.hbx_store_paths_status.argtypes + [P, P]
    L.hbx_seg_submit_device_dd.argtypes = L.hbx_seg_submit_device.argtypes + [P, P]
    L.hbx_store_file_stream.argtypes = [P, ctypes.c_char_p, U64, U64, ctypes.c_uint32, ctypes.c_uint32, P, P, P, P]
    L.hbx_restore_in_bound.argtypes = [U64]
    L.hbx_restore_in_bound.restype = U64
    L.hbx_restore_blocks.argtypes = [P, U64, P, P, P, P, P, P, P, U64, P, U64, P, U64, P, P, PU64, PU64]
    L.hbx_restore_file_stream.argtypes = [P, U64, P, P, P, U64, ctypes.c_char_p, P, ctypes.c_char_p, U64, PU64, PU64,
                                          PU32, PU64]
    L.hbx_restore_many_window.argtypes = [U64, P, U64, U64, PU64]
    L.hbx_restore_files_blocks.argtypes = [P, U64, P, P, P, P, P, P, P, P, P, U64, P, U64, P, P, P, P, P, P, P]
    L.hbx_restore_files_stream.argtypes = [P, U64, P, P, P, P, P, U64, P, P, ctypes.c_uint32, U64, P]
    L.hbx_match_chains.argtypes = [P, U64, P, P, P, P, P, P]
    L.hbx_submit_device_match.argtypes = L.hbx_submit_device.argtypes + [P, P, P]
    L.hbx_store_paths_match.argtypes = [P, U64, P, P, P, P, P, P, P, P, ctypes.c_uint32, U64, P, P, P]
    L.hbx_locate_ids.argtypes = [P, U64, P, P, P, U64, P, P, PU64]
    L.hbx_datfile_header_parse.argtypes = [P, U64, PU32, PU32, PU64]
    L.hbx_datfile_entry_parse.argtypes = [P, U64, U64, U64, ctypes.POINTER(DatRecord)]
    L.hbx_datfile_walk.argtypes = [U64, U64, P, P, U64, P, P, P, U64, P, U64, ctypes.POINTER(DatSummary)]
    L.hbx_datfile_check_device.argtypes = [P, P, U64, U64, U64, U64, P, U64, P, U64, P, U64,
                                           ctypes.POINTER(DatSummary)]
    L.hbx_datfile_check_path.argtypes = [P, ctypes.c_char_p, U64, U64, U64, P, U64, P, U64, P, U64,
                                         ctypes.POINTER(DatSummary)]
    L.hbx_datfile_verify_at.argtypes = [P, P, U64, ctypes.c_char_p, U64, P, P, I, U64, U64, P]
    L.hbx_block_graph.argtypes = [P, U64, P, P, P, U64, P, P, U64, P, P, P, P, P, P, ctypes.POINTER(GraphSummary)]
    PCA, PCS = ctypes.POINTER(DatCompactArgs), ctypes.POINTER(DatCompactSummary)
    L.hbx_datfile_compact_plan.argtypes = [U64, U64, P, P, PCA, P, P, P, PCS]
    L.hbx_datfile_compact_device.argtypes = [P, P, U64, U64, P, P, PCA, P, P, P, P, U64, P, U64, P, U64, PCS]
    L.hbx_datfile_compact_path.argtypes = [P, ctypes.c_char_p, U64, P, P, PCA, P, P, P, P, U64, P, U64, P, U64, PCS]
    U32 = ctypes.c_uint32
    L.hbx_index_open.argtypes = [P, U32, P, P, ctypes.POINTER(P)]
    L.hbx_index_open_paths.argtypes = [P, U32, P, ctypes.POINTER(P)]
    L.hbx_index_close.argtypes = [P, P]
    L.hbx_index_sizes.argtypes = [P, P, P]
    L.hbx_index_export.argtypes = [P, P, U32, P, U64, PU64]
    L.hbx_index_lookup.argtypes = [P, P, U64, P, I, P]
    L.hbx_index_scan.argtypes = [P, P, P, U64, P, ctypes.POINTER(IxSummary)]
    L.hbx_index_mark.argtypes = [P, P, U64, P, P, PU64]
    L.hbx_index_update.argtypes = [P, P, U64, P, P]
    L.hbx_index_sweep.argtypes = [P, P, P, P, U64, P, U64, ctypes.POINTER(IxSweepSummary)]
    L.hbx_index_compact.argtypes = [P, P, ctypes.POINTER(IxCompactSummary)]
    host = [U32, P, P, P]  # n_files, images, sizes, caps
    L.hbx_index_lookup_host.argtypes = host + L.hbx_index_lookup.argtypes[2:]
    L.hbx_index_scan_host.argtypes = host + L.hbx_index_scan.argtypes[2:]
    L.hbx_index_mark_host.argtypes = host + L.hbx_index_mark.argtypes[2:]
    L.hbx_index_update_host.argtypes = host + L.hbx_index_update.argtypes[2:]
    L.hbx_index_sweep_host.argtypes = host + L.hbx_index_sweep.argtypes[2:]
    L.hbx_index_compact_host.argtypes = host + L.hbx_index_compact.argtypes[2:]
    for name in EXPORTS:
        if name not in _NON_STATUS:
            getattr(L, name).restype = I
    _lib = L
    return L
