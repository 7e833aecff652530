"""Host-side mirror of Hashback's chunking + block-ID interface on libhbxgpu.

Reference interface (fredli74/hashbox):
  * ``BackupSession.storeFile(path, entry)`` — hashback/store.go:84-199: splits
    a file by the rollsum rule and stores each chunk with
    ``Client.StoreData`` (pkg/core/client.go:556-560), whose
    ``NewHashboxBlock -> HashData`` (pkg/core/block.go:39-43, 96-111) yields
    the 16-byte BlockID; then sets ``entry.ContentType`` /
    ``entry.ContentBlockID`` (store.go:187-196).
  * ``HashboxBlock.HashData`` for blocks with links (chain/directory blocks).

:class:`Engine` exposes the same results — chunk end offsets, BlockIDs,
content type and content BlockID — computed on an MI355X.  Every call goes
through the C-ABI (include/hbxgpu.h); there is no CPU fallback, and errors
raise :class:`HbxError` (the reference panics via core.Abort,
pkg/core/utils.go:22-37).
"""
from __future__ import annotations

import ctypes
import gc
import os
import sys
import time
from collections import deque
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Union

import numpy as np

from . import _lib

MIN_BLOCK_SIZE = 64 * 1024  # hashback/hashback.go:38
MAX_BLOCK_SIZE = 8 * 1024 * 1024  # hashback/hashback.go:37
CONTENT_TYPE_FILE_DATA = 2  # store.go:193
CONTENT_TYPE_FILE_CHAIN = 3  # store.go:189
ARENA_ALIGN = 16
ARENA_SLACK = 64
SEG_OVERLAP = MAX_BLOCK_SIZE  # HBX_SEG_OVERLAP
SEG_MIN_BYTES = 2 * MAX_BLOCK_SIZE  # HBX_SEG_MIN_BYTES

BytesLike = Union[bytes, bytearray, memoryview, np.ndarray]


class HbxError(RuntimeError):
    """A non-zero status from libhbxgpu."""


class RestoreError(HbxError):
    """:meth:`Engine.restore_file` / :meth:`Engine.diff_file` failed: ``code``
    is the library's status (``_lib.ERR_VERIFY`` for a bad block, with its
    ``bad_index`` and ``bad_status``; ``_lib.ERR_IO`` for a failing source,
    sink, write or local read); ``bytes`` is what was restored before it."""

    def __init__(self, msg: str, code: int, bad_index: Optional[int], bad_status: int, nbytes: int):
        super().__init__(msg)
        self.code, self.bad_index, self.bad_status, self.bytes = code, bad_index, bad_status, nbytes


@dataclass(slots=True)
class RestoredBlocks:
    """What :meth:`Engine.restore_blocks` returns (hbx_restore_blocks)."""
    data: Optional[bytes]  # the file's bytes up to the first bad block; None in diff mode
    offs: np.ndarray  # uint64 [n_good + 1]: where each good block starts; offs[-1] = bytes restored
    status: np.ndarray  # uint32 [n]: 0 ok, 1-6 inflate, 7 ID mismatch, 8 field too long / unknown type
    n_good: int  # leading blocks with status 0
    first_diff: Optional[int]  # diff mode: first differing offset, None when nothing differs


@dataclass(slots=True)
class RestoredFiles:
    """What :meth:`Engine.restore_files_blocks` returns (hbx_restore_files_blocks)."""
    data: Optional[List[bytes]]  # per file: its bytes up to its first bad block; None in diff mode
    out_offs: np.ndarray  # uint64 [n_files + 1]: where each file's bytes lie in the packed image
    blk_offs: List[np.ndarray]  # per file, uint64 per block: its offset inside the file (2**64 - 1 once bad)
    status: List[np.ndarray]  # per file, uint32 per block: as RestoredBlocks.status
    n_good: np.ndarray  # int64 [n_files]: leading blocks with status 0
    first_diff: Optional[List[Optional[int]]]  # diff mode, per file: first differing offset, None when equal


@dataclass(slots=True)
class RestoredFile:
    """One file's result of :meth:`Engine.restore_files` (hbx_restored_file)."""
    bytes: int  # the bytes of its good prefix
    n_good: int  # its leading good blocks
    bad_index: Optional[int]  # the index of its first bad block, None if every block is good
    bad_status: int
    errno: int  # of a path that could not be created, written, opened or read; else 0
    first_diff: Optional[int] = None  # diff mode


DAT_ENTRY_DTYPE = np.dtype([("off", np.uint64), ("size", np.uint64), ("data_off", np.uint64), ("link_base", np.uint64),
                            ("n_links", np.uint32), ("data_len", np.uint32), ("plain_len", np.uint32),
                            ("type", np.uint8), ("id", np.uint8, (16,))])
DAT_SPAN_DTYPE = np.dtype([("off", np.uint64), ("len", np.uint64), ("kind", np.uint32), ("status", np.uint32),
                           ("n_failed", np.uint64)])
# the same fields where hbx_dat_entry has them (64 bytes): what a call that takes entries is given
_DAT_ENTRY_C = np.dtype({"names": list(DAT_ENTRY_DTYPE.names),
                         "formats": [DAT_ENTRY_DTYPE[k] for k in DAT_ENTRY_DTYPE.names],
                         "offsets": [0, 8, 16, 24, 32, 36, 40, 44, 48], "itemsize": 64})


def _c_entries(entries) -> np.ndarray:
    e = np.asarray(entries)
    out = np.zeros(e.shape[0], _DAT_ENTRY_C)
    for name in DAT_ENTRY_DTYPE.names:
        out[name] = e[name]
    return out


@dataclass(slots=True)
class DatFileCheck:
    """What :meth:`Engine.check_datfile` returns (hbx_datfile_check_*): what
    RecoverData (pkg/storagedb/integrity.go:74-143) would find in a storage
    data file."""
    entries: np.ndarray  # DAT_ENTRY_DTYPE [n_entries]: the good entries on the walk, ascending
    spans: np.ndarray  # DAT_SPAN_DTYPE [n_spans]: gaps (kind 0) and broken spans (kind 1), ascending
    summary: dict  # hbx_dat_summary's fields; truncate_at is None when the walk did not end in damage
    links: Optional[np.ndarray]  # uint8 [summary["n_links"], 16]: entry e's are links[link_base : link_base + n_links]


@dataclass(slots=True)
class DatCompact:
    """What :meth:`Engine.compact_datfile` returns (hbx_datfile_compact_*):
    what CompactFile (pkg/storagedb/gc.go:208-318) would do to a data file, as
    bytes.  Nothing is written anywhere."""
    entries: np.ndarray  # DAT_ENTRY_DTYPE [n]: the table the call was given
    klass: np.ndarray  # uint8 [n]: 0 dropped, 1 stays where it is, 2 moved
    new_off: np.ndarray  # uint64 [n]: where the entry lies afterwards (a dropped one: 2^64 - 1)
    meta_off: np.ndarray  # uint64 [n]: where its meta record lies (a dropped one: 2^64 - 1)
    moved: Optional[bytes]  # the moved entries back to back: what is appended at dst_base
    meta: Optional[bytes]  # one StorageMetaEntry per kept entry: what is appended at meta_base
    ix: Optional[np.ndarray]  # uint8 [n_meta, 24]: one StorageIXEntry per kept entry
    summary: dict  # hbx_dat_compact_summary's fields; first_past_limit is None when nothing passes the limit
    file_no: int
    dst_file_no: int

    @property
    def stay(self) -> np.ndarray:
        return self.klass == _lib.CMP_STAY

    @property
    def moved_rows(self) -> np.ndarray:
        return self.klass == _lib.CMP_MOVE

    @property
    def relocations(self) -> list:
        """(id, file, offset) of every moved entry: changeDataLocation's arguments (gc.go:284, 303)."""
        return [(self.entries["id"][i].tobytes(), self.dst_file_no, int(self.new_off[i]))
                for i in np.flatnonzero(self.moved_rows)]


class CompactLimitError(HbxError):
    """:meth:`Engine.compact_datfile`: an offset would lie above the 16 GiB
    limit of a location (HBX_ERR_CAPACITY with ``first_past_limit``).
    ``plan`` is the :class:`DatCompact` of the call without streams (``moved``,
    ``meta`` and ``ix`` are None): its ``klass``, ``new_off``, ``meta_off`` and
    ``summary`` are complete, so the caller can cut the list at
    ``first_past_limit`` and call again with the next file as destination."""

    def __init__(self, msg: str, plan: "DatCompact"):
        super().__init__(msg)
        self.plan = plan
        self.first_past_limit = plan.summary["first_past_limit"]


GRAPH_NONE = _lib.GRAPH_NONE


@dataclass(slots=True)
class BlockGraph:
    """What :meth:`Engine.block_graph` returns (hbx_block_graph): the block
    table's links resolved to rows, the GC mark from the roots (MarkIndexes,
    pkg/storagedb/gc.go:24-69) and the block-tree check (checkBlockFromIXEntry's
    recursion, integrity.go:298-329).  ``GRAPH_NONE`` stands for no row and no
    depth."""
    rep: np.ndarray  # uint32 [n]: the lowest row carrying row i's ID
    link_row: np.ndarray  # uint32 [m]: the representative row each link names, GRAPH_NONE = missing
    root_row: np.ndarray  # uint32 [n_roots]: the same for the roots
    mark_depth: np.ndarray  # uint32 [n]: links from the nearest root, GRAPH_NONE = unreached
    fault_depth: np.ndarray  # uint32 [n]: links down to the nearest faulty row, GRAPH_NONE = the tree is valid
    summary: dict  # hbx_graph_summary's fields

    @property
    def marked(self) -> np.ndarray:
        return self.mark_depth != GRAPH_NONE

    @property
    def tree_ok(self) -> np.ndarray:
        return self.fault_depth == GRAPH_NONE

    @property
    def alias(self) -> np.ndarray:
        return self.rep != np.arange(self.rep.shape[0], dtype=np.uint32)


def max_chunks(n: int) -> int:
    return n // MIN_BLOCK_SIZE + 1


@dataclass(slots=True)
class FileChunks:
    """What storeFile records for one file."""
    cut_ends: np.ndarray  # uint64 [k]: chunk i = [cut_ends[i-1], cut_ends[i])
    ids: np.ndarray  # uint8 [k, 16]: BlockID per chunk (core.Byte128)
    content_type: int  # 2 FileData, 3 FileChain (0 for an empty file)
    content_id: bytes  # entry.ContentBlockID
    zstreams: Optional[list] = None  # zlib stream per chunk, uint8 views (store_paths(compress=True))
    errno: int = 0  # store_paths(skip_unreadable=True): the errno of a file skipped (no chunks), else 0
    # with dedup=IdSet: bool [k], True where the chunk's ID is the first occurrence of an ID the set
    # did not hold (only those chunks are compressed and need sending); None without a set
    fresh: Optional[np.ndarray] = None

    @property
    def n_chunks(self) -> int:
        return int(self.cut_ends.shape[0])

    def chunk_bounds(self):
        starts = np.concatenate([[0], self.cut_ends[:-1]]).astype(np.uint64)
        return starts, self.cut_ends


@dataclass(slots=True)
class ChainMatch:
    """One file's local block-ID list against its stored chain (hbx_chain_match,
    K12).  ``same`` means the local file equals the stored one: a block ID binds
    the block's length and bytes (block.go:96-111).  Not ``same`` means only
    that the IDs do not settle it (a chain cut by another chunker names equal
    bytes with other IDs): compare the bytes."""
    same: bool  # n_match == n_local == n_expect
    n_match: int  # length of the common prefix of the two ID lists
    n_local: int  # chunks the local file was cut into (0 for a file skipped as unreadable)
    n_expect: int  # IDs in the stored chain
    match_bytes: int  # local offset where chunk n_match starts (the file's length when n_match == n_local)
    errno: int = 0  # match_paths(skip_unreadable=True): the errno of a file skipped, else 0
    content_type: int = 0  # of the LOCAL file, as FileChunks (0 from match_chains)
    content_id: bytes = b""
    chunks: Optional[FileChunks] = None  # the local file's chunks, where they were asked for


@dataclass(slots=True)
class SegmentChunks:
    """What ``Engine.store_file(..., on_segment=...)`` hands over per segment."""
    first_chunk: int  # index in the file of this segment's first chunk
    chunks: FileChunks  # the chunks this segment completed (absolute cut ends); views, valid during the callback
    final: bool  # the file's last segment: chunks.content_type / content_id are the whole file's


def _u8(data: BytesLike) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data.reshape(-1).view(np.uint8))
    return np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)


def _p(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


def _huge_host_buffer(nbytes: int) -> np.ndarray:
    """A host byte buffer the library fills once (the compressed streams of a
    whole store_paths call): an anonymous mapping advised for transparent
    huge pages, so its first touch costs one fault per 2 MiB instead of per
    4 KiB (60 GB of 4 KiB first-touch faults cost ~1.4 s on 16 threads)."""
    import mmap
    m = mmap.mmap(-1, max(nbytes, 1), flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
    if hasattr(mmap, "MADV_HUGEPAGE"):
        try:
            m.madvise(mmap.MADV_HUGEPAGE)
        except OSError:
            pass
    return np.frombuffer(m, np.uint8)  # the array keeps the mapping alive


class SegmentedFile:
    """An open segmented file (hbx_seg_open): the handle :meth:`Engine.seg_submit_device`
    takes.  ``end`` is the file offset where the latest submitted segment
    ends (0 before the first), ``final_sent`` whether the final one went in."""

    def __init__(self, engine: "Engine", handle: int, file_len: int):
        self._engine = engine
        self._h = ctypes.c_void_p(handle)
        self.file_len = int(file_len)
        self.end = 0
        self.final_sent = False

    def next(self, segment_bytes: int):
        """(offset, length) of the next segment to submit (hbx_seg_next)."""
        return Engine.seg_next(self.file_len, segment_bytes, self.end)

    def close(self):
        """hbx_seg_close: refused (HbxError) while a segment is pending;
        before the final segment it abandons the file."""
        if self._h:
            e = self._engine
            e._check(e._L.hbx_seg_close(e._ctx, self._h), "hbx_seg_close")
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _ids_array(ids) -> np.ndarray:
    """Block IDs as a contiguous uint8 [n, 16] array: an array of that shape,
    raw bytes (16 per ID) or a sequence of 16-byte IDs."""
    if isinstance(ids, np.ndarray):
        a = np.ascontiguousarray(ids, np.uint8)
    elif isinstance(ids, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(ids), np.uint8)
    else:
        a = np.frombuffer(b"".join(bytes(x) for x in ids), np.uint8)
    if a.size % 16:
        raise ValueError("block IDs are 16 bytes each")
    return a.reshape(-1, 16)


def _chain_lists(chains) -> tuple:
    """Per-file ID lists as (first uint64 [n + 1] running counts, ids uint8 [total, 16])."""
    arrs = [_ids_array(c) if not (isinstance(c, (list, tuple)) and not c) else np.zeros((0, 16), np.uint8)
            for c in chains]
    first = np.zeros(len(arrs) + 1, np.uint64)
    if arrs:
        first[1:] = np.cumsum([a.shape[0] for a in arrs])
    ids = np.ascontiguousarray(np.concatenate(arrs)) if arrs and int(first[-1]) else np.zeros((0, 16), np.uint8)
    return first, ids


def _matches(rec, n: int) -> list:
    """hbx_chain_match records as ChainMatch objects."""
    if n == 0:
        return []
    v = np.ctypeslib.as_array(rec)[:n]
    return [ChainMatch(bool(s), int(m), int(l), int(e), int(b))
            for s, m, l, e, b in zip(v["same"].tolist(), v["n_match"].tolist(), v["n_local"].tolist(),
                                     v["n_expect"].tolist(), v["match_bytes"].tolist())]


class IdSet:
    """A set of block IDs in device memory (hbx_idset, K9): what the server
    is known to hold.  ``Engine.store_paths(dedup=set)``,
    ``Engine.store_file(segment_bytes=..., dedup=set)``, ``Engine.submit_device(dedup=set)`` and
    ``Engine.seg_submit_device(dedup=set)`` consult it in submit order, report
    per chunk whether its ID is new (``FileChunks.fresh``) and compress only
    the new ones, in place of the reference's queue-map check and allo/ACKN
    round (pkg/core/client.go:571-576, server/server.go:160-168)."""

    def __init__(self, engine: "Engine", capacity: int):
        self._engine = engine
        self._h = ctypes.c_void_p()
        engine._check(engine._L.hbx_idset_create(engine._ctx, int(capacity), ctypes.byref(self._h)),
                      "hbx_idset_create")

    def insert(self, ids) -> np.ndarray:
        """Test-and-insert, in order: True exactly for the first occurrence of
        an ID the set did not hold (hbx_idset_insert)."""
        a = _ids_array(ids)
        fresh = np.zeros(max(a.shape[0], 1), np.uint8)
        e = self._engine
        e._check(e._L.hbx_idset_insert(e._ctx, self._h, a.shape[0], _p(a), _p(fresh)), "hbx_idset_insert")
        return fresh[:a.shape[0]].astype(bool)

    def contains(self, ids) -> np.ndarray:
        """True where the ID is in the set (hbx_idset_contains); reads only."""
        a = _ids_array(ids)
        found = np.zeros(max(a.shape[0], 1), np.uint8)
        e = self._engine
        e._check(e._L.hbx_idset_contains(e._ctx, self._h, a.shape[0], _p(a), _p(found)), "hbx_idset_contains")
        return found[:a.shape[0]].astype(bool)

    def _stats(self):
        v = [ctypes.c_uint64(0) for _ in range(4)]
        e = self._engine
        e._check(e._L.hbx_idset_stats(e._ctx, self._h, *[ctypes.byref(x) for x in v]), "hbx_idset_stats")
        return [int(x.value) for x in v]

    @property
    def count(self) -> int:
        return self._stats()[0]

    @property
    def capacity(self) -> int:
        return self._stats()[1]

    @property
    def slots(self) -> int:
        return self._stats()[2]

    @property
    def dropped(self) -> int:
        """IDs not inserted because the set was full (they stay fresh)."""
        return self._stats()[3]

    def export(self) -> np.ndarray:
        """The set's IDs, uint8 [count, 16], in insertion order
        (hbx_idset_export): call / submit order across calls and batches,
        unspecified within one."""
        n = self.count
        out = np.zeros((max(n, 1), 16), np.uint8)
        got = ctypes.c_uint64(0)
        e = self._engine
        e._check(e._L.hbx_idset_export(e._ctx, self._h, _p(out), n, ctypes.byref(got)), "hbx_idset_export")
        return out[:int(got.value)]

    def truncate(self, n: int):
        """Keep the first ``n`` IDs of the export order (hbx_idset_truncate):
        roll back to a ``count`` noted before a send that failed."""
        e = self._engine
        e._check(e._L.hbx_idset_truncate(e._ctx, self._h, int(n)), "hbx_idset_truncate")

    def close(self):
        """hbx_idset_destroy: refused (HbxError) while pending batches use the set."""
        if self._h and self._engine._ctx:
            e = self._engine
            e._check(e._L.hbx_idset_destroy(e._ctx, self._h), "hbx_idset_destroy")
        self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


IX_HIT_DTYPE = np.dtype([("found", np.uint32), ("flags", np.uint32), ("file", np.uint32), ("meta_file", np.uint32),
                         ("offset", np.uint64), ("meta_off", np.uint64)])  # hbx_ix_hit
IX_LIVE_DTYPE = np.dtype([("id", np.uint8, (16,)), ("flags", np.uint32), ("ix_file", np.uint32),
                          ("ix_offset", np.uint64), ("meta_file", np.uint32), ("state", np.uint32),
                          ("meta_off", np.uint64)])  # hbx_ix_live
IX_KILLED_DTYPE = np.dtype([("id", np.uint8, (16,)), ("meta_file", np.uint32), ("reserved", np.uint32),
                            ("meta_off", np.uint64)])  # hbx_ix_killed
assert IX_HIT_DTYPE.itemsize == 32 and IX_LIVE_DTYPE.itemsize == 48 and IX_KILLED_DTYPE.itemsize == 32


def _fields(s) -> dict:
    return {k: int(getattr(s, k)) for k, _ in s._fields_}


@dataclass(slots=True)
class IndexScan:
    """What :meth:`Index.scan` returns (hbx_index_scan): the pass of
    CheckIndexes (pkg/storagedb/integrity.go:354-410) with CompactIndexes'
    counters."""
    live: np.ndarray  # IX_LIVE_DTYPE [n_live]: the live entries in (file, offset) order
    per_file: list  # hbx_ix_file_stats' fields, one dict per file; first_misplaced is None without one
    summary: dict  # hbx_ix_summary's fields


@dataclass(slots=True)
class IndexSweep:
    """What :meth:`Index.sweep` returns (hbx_index_sweep): what SweepIndexes
    (pkg/storagedb/gc.go:70-151) did, per live entry of the scan before it."""
    action: np.ndarray  # uint8 [n_live]: IX_ACT_* (1 deleted, 2 stays, 3 obsolete, 4 moved, 5 abort)
    moved_to: np.ndarray  # uint64 [n_live, 2]: (file, offset) of a moved entry, else 2^64 - 1 twice
    killed: np.ndarray  # IX_KILLED_DTYPE [n_deleted]: killMetaEntry's arguments, in live order
    summary: dict  # hbx_ix_sweep_summary's fields; first_abort is None without one


class IndexSweepError(HbxError):
    """:meth:`Index.sweep`: findIXOffset named a later place for an entry, where
    the reference aborts (gc.go:129-131; HBX_ERR_FORMAT).  ``sweep`` is the
    complete :class:`IndexSweep`; the index is unchanged."""

    def __init__(self, msg: str, sweep: "IndexSweep"):
        super().__init__(msg)
        self.sweep = sweep


class Index:
    """A store's index files (``*.idx``) in device memory (hbx_index, K17): the
    open-addressed tables of pkg/storagedb/index.go with the reference's
    operations on them.  Nothing is written to disk: :meth:`export` hands the
    images back."""

    def __init__(self, engine: "Engine", source):
        self._engine = engine
        self._h = ctypes.c_void_p()
        e = engine
        src = list(source)
        self.n_files = len(src)
        if src and all(isinstance(s, (str, os.PathLike)) for s in src):
            paths = (ctypes.c_char_p * len(src))(*[os.fsencode(s) for s in src])
            rc = e._L.hbx_index_open_paths(e._ctx, len(src), paths, ctypes.byref(self._h))
        else:
            arrs = [np.ascontiguousarray(np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray, memoryview))
                                         else np.asarray(s, np.uint8).reshape(-1)) for s in src]
            ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
            sizes = np.array([a.shape[0] for a in arrs] + [0], np.uint64)
            rc = e._L.hbx_index_open(e._ctx, len(arrs), ptrs, _p(sizes), ctypes.byref(self._h))
        e._check(rc, "hbx_index_open")

    def sizes(self) -> List[int]:
        """Each file's current size (hbx_index_sizes)."""
        e = self._engine
        out = np.zeros(_lib.IX_FILES_MAX, np.uint64)
        e._check(e._L.hbx_index_sizes(e._ctx, self._h, _p(out)), "hbx_index_sizes")
        return out[:self.n_files].tolist()

    def export(self, k: int) -> bytes:
        """File ``k``'s image as it stands (hbx_index_export)."""
        e = self._engine
        out = np.zeros(max(self.sizes()[k], 1), np.uint8)
        n = ctypes.c_uint64(0)
        e._check(e._L.hbx_index_export(e._ctx, self._h, int(k), _p(out), out.shape[0], ctypes.byref(n)),
                 "hbx_index_export")
        return out[:int(n.value)].tobytes()

    def lookup(self, ids, stop_on_free: bool = False) -> np.ndarray:
        """findIXOffset (index.go:54-107) for every ID: IX_HIT_DTYPE [n].
        ``file`` and ``offset`` are the rule's place whether found or not;
        without ``stop_on_free`` this is readIXEntry."""
        a = _ids_array(ids)
        hits = np.zeros(max(a.shape[0], 1), IX_HIT_DTYPE)
        e = self._engine
        e._check(e._L.hbx_index_lookup(e._ctx, self._h, a.shape[0], _p(a), 1 if stop_on_free else 0, _p(hits)),
                 "hbx_index_lookup")
        return hits[:a.shape[0]]

    def scan(self, live_cap: int = 0) -> IndexScan:
        """One pass over every slot of every file (hbx_index_scan).  The live
        table is sized from ``live_cap`` and, when the index holds more live
        entries, from the library's count (the call then runs once more)."""
        e = self._engine
        per = (_lib.IxFileStats * _lib.IX_FILES_MAX)()
        sm = _lib.IxSummary()
        live = np.zeros(max(int(live_cap), 1), IX_LIVE_DTYPE)
        for _ in range(2):
            rc = e._L.hbx_index_scan(e._ctx, self._h, _p(live), live.shape[0], per, ctypes.byref(sm))
            if rc != _lib.ERR_CAPACITY or int(sm.n_live) <= live.shape[0]:
                break
            live = np.zeros(int(sm.n_live), IX_LIVE_DTYPE)
        e._check(rc, "hbx_index_scan")
        files = [_fields(per[f]) for f in range(self.n_files)]
        for f in files:
            if f["first_misplaced"] == _lib.NO_DIFF:
                f["first_misplaced"] = None
        return IndexScan(live[:int(sm.n_live)], files, _fields(sm))

    def mark(self, ids) -> np.ndarray:
        """The write half of MarkIndexes (gc.go:46-54): Marked is set on the
        slot of every ID readIXEntry finds (hbx_index_mark).  Returns bool [n],
        False where the reference would abort (gc.go:36-37)."""
        a = _ids_array(ids)
        found = np.zeros(max(a.shape[0], 1), np.uint8)
        e = self._engine
        e._check(e._L.hbx_index_mark(e._ctx, self._h, a.shape[0], _p(a), _p(found), None), "hbx_index_mark")
        return found[:a.shape[0]].astype(bool)

    def update(self, recs) -> np.ndarray:
        """changeMetaLocation (meta.go:122-128) from StorageIXEntry records,
        uint8 [n, 24] as :attr:`DatCompact.ix` (hbx_index_update): the location
        and the NoLinks bit of every ID readIXEntry finds.  Returns uint8 [n]:
        0 updated, 1 not found (inserting is not done here)."""
        r = np.ascontiguousarray(np.asarray(recs, np.uint8).reshape(-1, _lib.IX_ENTRY))
        st = np.zeros(max(r.shape[0], 1), np.uint8)
        e = self._engine
        e._check(e._L.hbx_index_update(e._ctx, self._h, r.shape[0], _p(r) if r.shape[0] else None, _p(st)),
                 "hbx_index_update")
        return st[:r.shape[0]]

    def sweep(self, live_cap: int = 0) -> IndexSweep:
        """SweepIndexes (gc.go:70-151) with the Marked bits of the images
        (hbx_index_sweep).  Raises :class:`IndexSweepError` where the reference
        aborts; the index is then unchanged.  The outputs are sized from
        ``live_cap`` and, when the index holds more live entries, from the
        library's counts (a first call that changes nothing tells them)."""
        e = self._engine
        sm = _lib.IxSweepSummary()
        n_live = n_del = int(live_cap)
        for _ in range(2):
            action = np.zeros(max(n_live, 1), np.uint8)
            moved = np.zeros((max(n_live, 1), 2), np.uint64)
            killed = np.zeros(max(n_del, 1), IX_KILLED_DTYPE)
            rc = e._L.hbx_index_sweep(e._ctx, self._h, _p(action), _p(moved), n_live, _p(killed), n_del, ctypes.byref(sm))
            if rc != _lib.ERR_CAPACITY or (int(sm.n_live) <= n_live and int(sm.swept_records) <= n_del):
                break
            n_live, n_del = int(sm.n_live), int(sm.swept_records)
        summary = _fields(sm)
        if summary["first_abort"] == _lib.NO_DIFF:
            summary["first_abort"] = None
        res = IndexSweep(action[:int(sm.n_live)], moved[:int(sm.n_live)], killed[:int(sm.n_deleted)], summary)
        if rc == _lib.ERR_FORMAT:
            msg = e._L.hbx_last_error(e._ctx)
            raise IndexSweepError(f"hbx_index_sweep: HBX_ERR_FORMAT: {msg.decode() if msg else ''}", res)
        e._check(rc, "hbx_index_sweep")
        return res

    def compact(self) -> dict:
        """CompactIndexes (gc.go:153-206; hbx_index_compact): ``cleared`` and
        the new ``sizes``."""
        e = self._engine
        sm = _lib.IxCompactSummary()
        e._check(e._L.hbx_index_compact(e._ctx, self._h, ctypes.byref(sm)), "hbx_index_compact")
        return {"cleared": int(sm.cleared), "sizes": [int(sm.size[f]) for f in range(self.n_files)]}

    def close(self):
        if self._h and self._engine._ctx:
            e = self._engine
            e._check(e._L.hbx_index_close(e._ctx, self._h), "hbx_index_close")
        self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Engine:
    """One MI355X (one HIP stream) running the chunk + block-ID path."""

    def __init__(self, device: int = 0, tile_iters: Optional[int] = None,
                 md5_slice: Optional[int] = None, join_lag: Optional[int] = None,
                 k3_period: Optional[int] = None):
        self._L = _lib.load()
        self._ctx = ctypes.c_void_p()
        rc = self._L.hbx_ctx_create(int(device), ctypes.byref(self._ctx))
        if rc != 0:
            raise HbxError(f"hbx_ctx_create(device={device}) failed: {_lib.ERRORS.get(rc, rc)}")
        self.device = device
        self._pending = deque()
        self.wait_s = 0.0
        self.last_call_s = 0.0
        self.last_located = 0  # hits of the latest locate_ids (hbx_locate_ids' n_found)
        if tile_iters is not None:
            self._check(self._L.hbx_set_tile_iters(self._ctx, int(tile_iters)), "set_tile_iters")
        if md5_slice is not None:
            self.set_md5_slice(md5_slice)
        if join_lag is not None:
            self.set_join_lag(join_lag)
        if k3_period is not None:
            self.set_k3_period(k3_period)

    # ----------------------------------------------------------- plumbing --
    def _after_producer(self):
        """The engine's HIP streams do not wait for other streams: device data
        written on torch's current stream (e.g. a tensor just filled) must be
        complete before the engine reads it.  The device-pointer entry points
        call this first; the dependency is a GPU-side event wait
        (hbx_after_stream), so the host never blocks and can submit batches
        ahead of the device."""
        t = sys.modules.get("torch")
        if t is not None and t.cuda.is_initialized():
            s = t.cuda.current_stream(self.device)
            self._check(self._L.hbx_after_stream(self._ctx, ctypes.c_void_p(int(s.cuda_stream))),
                        "hbx_after_stream")

    def close(self):
        if self._ctx:
            self._L.hbx_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._L.hbx_last_error(self._ctx)
            raise HbxError(f"{what}: {_lib.ERRORS.get(rc, rc)}: "
                           f"{msg.decode() if msg else ''}")

    @staticmethod
    def _alloc_out(lens: Sequence[int]):
        caps = (np.asarray(lens, np.uint64).reshape(-1) // np.uint64(MIN_BLOCK_SIZE) + np.uint64(1)
                if len(lens) else np.zeros(0, np.uint64))
        base = np.zeros(len(lens), np.uint64)
        if len(lens):
            base[1:] = np.cumsum(caps)[:-1]
        tot = int(caps.sum()) if len(lens) else 0
        cuts = np.zeros(max(tot, 1), np.uint64)
        ids = np.zeros((max(tot, 1), 16), np.uint8)
        sums = (_lib.FileSummary * max(len(lens), 1))()
        return caps, base, cuts, ids, sums

    @staticmethod
    def _unpack(lens, caps, base, cuts, ids, sums, fresh=None) -> List[FileChunks]:
        # one structured view of the summaries; each file's cut ends and ids
        # are views into the per-call output arrays (no per-file copies:
        # 100 k files unpack in ~0.15 s instead of ~0.4 s)
        n = len(lens)
        if n == 0:
            return []
        sv = np.ctypeslib.as_array(sums)[:n]
        k = sv["n_chunks"].astype(np.int64)
        starts = base[:n].astype(np.int64).tolist()
        ks = k.tolist()
        types = sv["content_type"].tolist()
        cid = np.ascontiguousarray(sv["content_id"]).tobytes()
        # the cyclic collector would run dozens of passes over 100 k new objects
        was = gc.isenabled()
        gc.disable()
        try:
            res = [FileChunks(cuts[b:b + kk], ids[b:b + kk], t, cid[16 * f:16 * f + 16] if kk else b"")
                   for f, (b, kk, t) in enumerate(zip(starts, ks, types))]
            if fresh is not None:
                fb = fresh.astype(bool)
                for r, b, kk in zip(res, starts, ks):
                    r.fresh = fb[b:b + kk]
            return res
        finally:
            if was:
                gc.enable()

    # -------------------------------------------------------------- API ----
    def chunk_hash(self, data: BytesLike) -> FileChunks:
        """storeFile over one in-memory file (store.go:111-196)."""
        return self.chunk_hash_batch([data])[0]

    def chunk_hash_batch(self, files: Sequence[BytesLike]) -> List[FileChunks]:
        arrs = [_u8(f) for f in files]
        lens = np.array([a.size for a in arrs], np.uint64)
        ptrs = np.array([_p(a) for a in arrs], np.uint64)
        caps, base, cuts, ids, sums = self._alloc_out(lens)
        self._check(self._L.hbx_chunk_hash_batch(self._ctx, len(arrs), _p(ptrs), _p(lens),
                                                 _p(cuts), _p(ids), _p(base), _p(caps), sums),
                    "hbx_chunk_hash_batch")
        return self._unpack(lens, caps, base, cuts, ids, sums)

    def chunk_hash_device(self, d_arena: int, offs: Sequence[int], lens: Sequence[int]
                          ) -> List[FileChunks]:
        """Files resident in device memory (pointer ``d_arena``, e.g. a torch
        uint8 tensor's ``data_ptr()``).  Offsets 16-B aligned; each file must be
        followed by >= 64 readable bytes."""
        self._after_producer()
        offs = np.ascontiguousarray(offs, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint64)
        caps, base, cuts, ids, sums = self._alloc_out(lens)
        self._check(self._L.hbx_chunk_hash_device(self._ctx, ctypes.c_void_p(int(d_arena)), len(lens),
                                                  _p(offs), _p(lens), _p(cuts), _p(ids), _p(base),
                                                  _p(caps), sums), "hbx_chunk_hash_device")
        return self._unpack(lens, caps, base, cuts, ids, sums)

    def submit_device(self, d_arena: int, offs: Sequence[int], lens: Sequence[int],
                      dedup: Optional[IdSet] = None):
        """Enqueue a device-resident batch and return at once.  Any number of
        batches may be in flight; :meth:`wait` completes the oldest.  The
        arena must stay untouched until then.  With ``dedup`` the batch's
        chunk IDs are marked against that set in submit order
        (hbx_submit_device_dd) and :meth:`wait` fills ``FileChunks.fresh``."""
        self._after_producer()
        offs = np.ascontiguousarray(offs, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint64)
        t0 = time.perf_counter()
        caps, base, cuts, ids, sums = self._alloc_out(lens)
        t1 = time.perf_counter()
        self.alloc_s = t1 - t0  # (bench diagnostics: host output arrays of this submit)
        if dedup is not None:
            fresh = np.zeros(cuts.shape[0], np.uint8)
            self._check(self._L.hbx_submit_device_dd(self._ctx, ctypes.c_void_p(int(d_arena)), len(lens),
                                                     _p(offs), _p(lens), _p(cuts), _p(ids), _p(base),
                                                     _p(caps), sums, dedup._h, _p(fresh)), "hbx_submit_device_dd")
            self._pending.append((offs, lens, caps, base, cuts, ids, sums, fresh))
            return
        self._check(self._L.hbx_submit_device(self._ctx, ctypes.c_void_p(int(d_arena)), len(lens),
                                              _p(offs), _p(lens), _p(cuts), _p(ids), _p(base),
                                              _p(caps), sums), "hbx_submit_device")
        self._pending.append((offs, lens, caps, base, cuts, ids, sums))

    def submit_device_match(self, d_arena: int, offs: Sequence[int], lens: Sequence[int], chains_ids,
                            chunks: bool = True):
        """:meth:`submit_device` with each file's stored chain (a list of block
        IDs per file; hbx_submit_device_match): K12 compares them on the
        device once the batch is hashed, and :meth:`wait` returns one
        :class:`ChainMatch` per file, with the file's FileChunks in
        ``chunks``.  With ``chunks=False`` (verdict-only) the batch brings
        back 52 bytes per file instead of 24 per result slot and ``chunks`` is
        None.  The chains are copied by this call."""
        self._after_producer()
        offs = np.ascontiguousarray(offs, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint64)
        if len(chains_ids) != len(lens):
            raise ValueError("one chain per file")
        first, eids = _chain_lists(chains_ids)
        rec = (_lib.ChainMatch * max(len(lens), 1))()
        if chunks:
            out = self._alloc_out(lens)
            caps, base, cuts, ids, sums = out
            outp = (_p(cuts), _p(ids), base.ctypes.data, caps.ctypes.data)
        else:
            out, sums, outp = None, (_lib.FileSummary * max(len(lens), 1))(), (None, None, None, None)
        self._check(self._L.hbx_submit_device_match(self._ctx, ctypes.c_void_p(int(d_arena)), len(lens), _p(offs),
                                                    _p(lens), *outp, sums, first.ctypes.data, _p(eids), rec),
                    "hbx_submit_device_match")
        self._pending.append(("match", lens, out, sums, rec, offs))

    def _match_result(self, lens, out, sums, rec, status=None) -> List[ChainMatch]:
        n = len(lens)
        res = _matches(rec, n)
        if n == 0:
            return res
        sv = np.ctypeslib.as_array(sums)[:n]
        cid = np.ascontiguousarray(sv["content_id"]).tobytes()
        files = self._unpack(lens, *out) if out is not None else None
        for f, (r, t) in enumerate(zip(res, sv["content_type"].tolist())):
            r.content_type = int(t)
            r.content_id = cid[16 * f:16 * f + 16] if r.n_local else b""
            if files is not None:
                r.chunks = files[f]
            if status is not None:
                r.errno = int(status[f])
                if r.chunks is not None:
                    r.chunks.errno = r.errno
        return res

    def match_chains(self, local_ids, expect_ids, local_cut_ends=None) -> List[ChainMatch]:
        """K12 alone on ID lists the caller holds (hbx_match_chains): per file,
        the common prefix of ``local_ids[f]`` and ``expect_ids[f]`` (lists of
        16-byte IDs, or uint8 [k, 16] arrays).  ``local_cut_ends[f]`` (one per
        local ID) gives ``match_bytes``; without them it is 0."""
        if len(local_ids) != len(expect_ids):
            raise ValueError("one expected chain per local ID list")
        n = len(local_ids)
        lf, lids = _chain_lists(local_ids)
        ef, eids = _chain_lists(expect_ids)
        cuts = None
        if local_cut_ends is not None:
            if len(local_cut_ends) != n:
                raise ValueError("one list of cut ends per file")
            cuts = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint64).reshape(-1) for c in local_cut_ends])
                                        if n else np.zeros(0, np.uint64), np.uint64)
            if cuts.shape[0] != lids.shape[0]:
                raise ValueError("one cut end per local ID")
        rec = (_lib.ChainMatch * max(n, 1))()
        self._check(self._L.hbx_match_chains(self._ctx, n, lf.ctypes.data, _p(lids),
                                             _p(cuts) if cuts is not None else None, ef.ctypes.data, _p(eids), rec),
                    "hbx_match_chains")
        return _matches(rec, n)

    def locate_ids(self, pool_ids, pool_cut_ends, want_ids) -> np.ndarray:
        """K13 alone (hbx_locate_ids): where a pool of local files holds each
        wanted block ID.  ``pool_ids[f]`` and ``pool_cut_ends[f]`` are pool
        file f's chunk IDs and cut ends (as FileChunks gives them; lists of
        16-byte IDs or uint8 [k, 16] arrays), ``want_ids`` a flat list of IDs.
        Returns a structured array of one record per wanted ID (``file``,
        ``chunk``, ``off``, ``len``): the pool file with the lowest pool
        position that holds the ID, the chunk's index in it, where it starts
        and how long it is; ``file == 0xFFFFFFFF`` for an ID the pool does not
        hold.  A located chunk is a candidate, not a fact: the file may have
        changed since it was hashed, so its bytes go through VerifyBlock
        (:meth:`restore_files` with a raw block) before they are used."""
        if len(pool_ids) != len(pool_cut_ends):
            raise ValueError("one list of cut ends per pool file")
        nf = len(pool_ids)
        pf, pids = _chain_lists(pool_ids)
        cuts = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint64).reshape(-1) for c in pool_cut_ends])
                                    if nf else np.zeros(0, np.uint64), np.uint64)
        if cuts.shape[0] != pids.shape[0]:
            raise ValueError("one cut end per pool ID")
        want = _ids_array(want_ids) if len(want_ids) else np.zeros((0, 16), np.uint8)
        nw = want.shape[0]
        rec = (_lib.BlockLoc * max(nw, 1))()
        found = ctypes.c_uint64(0)
        self._check(self._L.hbx_locate_ids(self._ctx, nf, pf.ctypes.data, _p(pids), _p(cuts), nw, _p(want), rec,
                                           ctypes.byref(found)), "hbx_locate_ids")
        self.last_located = int(found.value)
        v = np.ctypeslib.as_array(rec)[:nw]
        out = np.empty(nw, np.dtype([("file", np.uint32), ("chunk", np.uint32), ("off", np.uint64), ("len", np.uint64)]))
        for name in out.dtype.names:
            out[name] = v[name]
        return out

    def block_graph(self, ids, n_links, links, roots=None, bad=None, link_base=None) -> BlockGraph:
        """K15 (hbx_block_graph): join a block table with its links on the
        device.  ``ids`` are the rows' block IDs, ``n_links`` their link counts,
        ``links`` the flat array of link IDs and ``link_base`` where each row's
        list starts in it (None: the running sum of ``n_links``); ``bad`` marks
        rows whose own check failed, ``roots`` are the IDs the GC mark starts
        from.  IDs as :meth:`locate_ids` takes them.  :func:`formats.block_table`
        makes the table from :meth:`check_datfile` results."""
        idv = _ids_array(ids) if len(ids) else np.zeros((0, 16), np.uint8)
        n = idv.shape[0]
        nl = np.ascontiguousarray(np.asarray(n_links).reshape(-1), np.uint32)
        lk = _ids_array(links) if len(links) else np.zeros((0, 16), np.uint8)
        m = lk.shape[0]
        rt = _ids_array(roots) if roots is not None and len(roots) else np.zeros((0, 16), np.uint8)
        r = rt.shape[0]
        if link_base is None:
            lb = np.zeros(n, np.uint64)
            if n > 1:
                lb[1:] = np.cumsum(nl[:-1], dtype=np.uint64)
        else:
            lb = np.ascontiguousarray(np.asarray(link_base).reshape(-1), np.uint64)
        if nl.shape[0] != n or lb.shape[0] != n:
            raise ValueError("one link count and one link base per row")
        bd = None
        if bad is not None:
            bd = np.ascontiguousarray(np.asarray(bad).reshape(-1) != 0, np.uint8)
            if bd.shape[0] != n:
                raise ValueError("one bad flag per row")
        out = BlockGraph(np.zeros(n, np.uint32), np.zeros(m, np.uint32), np.zeros(r, np.uint32),
                         np.zeros(n, np.uint32), np.zeros(n, np.uint32), {})
        sm = _lib.GraphSummary()
        # (an empty output still gets a pointer: NULL would mean "not wanted", here the mark and the check)
        ptr = lambda a: a.ctypes.data  # noqa: E731
        self._check(self._L.hbx_block_graph(self._ctx, n, _p(idv), _p(nl), _p(lb), m, _p(lk),
                                            _p(bd) if bd is not None else None, r, _p(rt), ptr(out.rep),
                                            ptr(out.link_row), ptr(out.root_row), ptr(out.mark_depth),
                                            ptr(out.fault_depth), ctypes.byref(sm)), "hbx_block_graph")
        out.summary = {k: int(getattr(sm, k)) for k, _ in _lib.GraphSummary._fields_}
        return out

    def _dat_image(self, source, size):
        """(device pointer, size, path, arena to free) of a data file given as
        a path, as bytes or as a device pointer with its size."""
        if isinstance(source, (str, os.PathLike)):
            return None, 0, os.fsencode(source), None
        if isinstance(source, int):
            if size is None:
                raise ValueError("a device pointer needs size=")
            self._after_producer()
            return ctypes.c_void_p(source), int(size), None, None
        a = _u8(source)
        n = int(a.shape[0])
        padded = np.zeros(n + _lib.DAT_IMAGE_SLACK, np.uint8)
        padded[:n] = a
        d = ctypes.c_void_p()
        self._check(self._L.hbx_arena_alloc(self._ctx, padded.shape[0], ctypes.byref(d)), "hbx_arena_alloc")
        rc = self._L.hbx_memcpy_h2d(self._ctx, d, _p(padded), padded.shape[0])
        if rc != 0:
            self._L.hbx_arena_free(self._ctx, d)
            self._check(rc, "hbx_memcpy_h2d")
        return d, n, None, d

    def check_datfile(self, source, max_block: int = 0, max_candidates: int = 0, window_bytes: int = 0,
                      links: bool = True, size: Optional[int] = None) -> DatFileCheck:
        """Check a storage data file on the device (K14 scan and parse, K8 /
        K8s inflate, K6 VerifyBlock; hbx_datfile_check_path / _device): every
        good entry RecoverData's walk finds, every gap and broken span and
        where to truncate.  ``source`` is a path, the file's bytes, or a device
        pointer (then ``size`` is required; the image needs 64 readable bytes
        behind it).  Nothing is written or repaired.  The output arrays are
        sized from a first guess and, when the file holds more, from the counts
        the library reports (the check then runs once more)."""
        d, n, path, arena = self._dat_image(source, size)
        try:
            guess = (n if path is None else os.path.getsize(path)) // 29 + 1
            ecap = scap = min(guess, 1 << 16)
            lcap = min(guess, 1 << 16) if links else 0
            cands = int(max_candidates)
            sm = _lib.DatSummary()
            for _ in range(3):
                ents = (_lib.DatEntry * max(ecap, 1))()
                spans = (_lib.DatSpan * max(scap, 1))()
                lk = np.zeros((max(lcap, 1), 16), np.uint8)
                tail = (ents, ecap, spans, scap, _p(lk) if links else None, lcap, ctypes.byref(sm))
                if path is not None:
                    rc = self._L.hbx_datfile_check_path(self._ctx, path, int(max_block), cands, int(window_bytes), *tail)
                else:
                    rc = self._L.hbx_datfile_check_device(self._ctx, d, n, int(max_block), cands, int(window_bytes), *tail)
                if rc != _lib.ERR_CAPACITY:
                    break
                # hbx_last_error names what did not fit; the summary has the counts
                need_c = max(int(sm.n_candidates), int(sm.n_gap_markers))
                if need_c > (cands or (1 << 20)):
                    if max_candidates:
                        break  # the caller set the capacity: the error is theirs
                    cands = need_c
                elif sm.n_entries > ecap or sm.n_spans > scap or (links and sm.n_links > lcap):
                    ecap, scap = max(ecap, int(sm.n_entries)), max(scap, int(sm.n_spans))
                    lcap = max(lcap, int(sm.n_links)) if links else 0
                else:
                    break
            self._check(rc, "hbx_datfile_check")
        finally:
            if arena is not None:
                self._L.hbx_arena_free(self._ctx, arena)
        ne, ns, nl = int(sm.n_entries), int(sm.n_spans), int(sm.n_links)
        ev = np.ctypeslib.as_array(ents)[:ne]
        e = np.zeros(ne, DAT_ENTRY_DTYPE)
        for name in DAT_ENTRY_DTYPE.names:
            e[name] = ev[name]
        sv = np.ctypeslib.as_array(spans)[:ns]
        s = np.zeros(ns, DAT_SPAN_DTYPE)
        for name in DAT_SPAN_DTYPE.names:
            s[name] = sv[name]
        summary = {k: int(getattr(sm, k)) for k, _ in _lib.DatSummary._fields_}
        if summary["truncate_at"] == _lib.NO_DIFF:
            summary["truncate_at"] = None
        return DatFileCheck(e, s, summary, lk[:nl].copy() if links else None)

    def verify_datfile_at(self, source, offs: Sequence[int], expect_ids, content: bool = True, max_block: int = 0,
                          window_bytes: int = 0, size: Optional[int] = None) -> np.ndarray:
        """The entries of a data file at offsets the index names
        (checkBlockFromIXEntry, integrity.go:259-296; hbx_datfile_verify_at):
        uint32 per offset, 9 = no structurally valid entry there, 10 = not the
        expected BlockID, else the VerifyBlock status (0 good) with ``content``
        or 0 for the header and ID check alone.  ``source`` as
        :meth:`check_datfile`."""
        o = np.ascontiguousarray(np.asarray(offs, np.uint64).reshape(-1))
        n = int(o.shape[0])
        want = _ids_array(expect_ids) if n else np.zeros((0, 16), np.uint8)
        if want.shape[0] != n:
            raise ValueError("one expected ID per offset")
        st = np.zeros(max(n, 1), np.uint32)
        d, sz, path, arena = self._dat_image(source, size)
        try:
            self._check(self._L.hbx_datfile_verify_at(self._ctx, d, sz, path, n, _p(o), _p(want), 1 if content else 0,
                                                      int(max_block), int(window_bytes), _p(st)),
                        "hbx_datfile_verify_at")
        finally:
            if arena is not None:
                self._L.hbx_arena_free(self._ctx, arena)
        return st[:n]

    def open_index(self, source) -> Index:
        """A store's index files 0 .. n - 1 on the device (K17; hbx_index_open /
        _open_paths): ``source`` is a sequence of paths, or of images (bytes or
        uint8 arrays).  A size that is no header and whole slots, or a header
        of another type or version, raises (HBX_ERR_FORMAT)."""
        return Index(self, source)

    def compact_datfile(self, source, entries, keep, file_no: int = 0, dst_file_no: Optional[int] = None,
                        dst_base: int = 16, keep_prefix: bool = True, meta_file_no: int = 0, meta_base: int = 16,
                        moved: bool = True, meta: bool = True, ix: bool = True,
                        size: Optional[int] = None) -> DatCompact:
        """Compact a storage data file on the device (K16; hbx_datfile_compact_path
        / _device): CompactFile (pkg/storagedb/gc.go:208-318) over the file's
        image, as bytes.  ``entries`` are :meth:`check_datfile`'s, ``keep`` one
        flag each (:func:`formats.gc_keep` makes them from a block graph).  The
        kept entries at the start of the file stay (``keep_prefix``); every other
        kept entry is packed into ``moved``, which the caller appends to data
        file ``dst_file_no`` (None: ``file_no``) at ``dst_base``; ``meta`` holds
        one StorageMetaEntry per kept entry for ``meta_file_no`` at ``meta_base``
        and ``ix`` their StorageIXEntry records.  ``source`` as
        :meth:`check_datfile`.  Nothing is written or truncated.  The buffers
        are sized from a first guess and, when the library reports larger
        sizes, from those (the call then runs once more).  An offset above the
        16 GiB limit of a location raises :class:`CompactLimitError`, which
        carries the complete plan."""
        ent = _c_entries(entries)
        n = int(ent.shape[0])
        kp = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, np.uint8)
        if kp.shape[0] != n:
            raise ValueError("one keep flag per entry")
        dst = file_no if dst_file_no is None else dst_file_no
        args = _lib.DatCompactArgs(int(file_no), int(dst), int(dst_base), int(meta_file_no),
                                   _lib.CMP_F_KEEP_PREFIX if keep_prefix else 0, int(meta_base))
        klass, new_off, meta_off = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        sm = _lib.DatCompactSummary()
        # (what the streams take if every kept entry moves; the library says if a table needs more)
        kept = kp != 0
        caps = [int(ent["size"][kept].sum()) if moved else 0,
                int((_lib.META_HEAD + 16 * ent["n_links"][kept].astype(np.uint64)).sum()) if meta else 0,
                _lib.IX_ENTRY * int(kept.sum()) if ix else 0]
        d, sz, path, arena = self._dat_image(source, size)
        try:
            for _ in range(2):
                bufs = [np.zeros(max(c, 1), np.uint8) for c in caps]
                outs = []
                for want, b, c in zip((moved, meta, ix), bufs, caps):
                    outs += [_p(b) if want else None, c]
                tail = (n, _p(ent), _p(kp), ctypes.byref(args), _p(klass), _p(new_off), _p(meta_off), *outs,
                        ctypes.byref(sm))
                if path is not None:
                    rc = self._L.hbx_datfile_compact_path(self._ctx, path, *tail)
                else:
                    rc = self._L.hbx_datfile_compact_device(self._ctx, d, sz, *tail)
                need = [int(sm.moved_bytes), int(sm.meta_bytes), _lib.IX_ENTRY * int(sm.n_meta)]
                if rc != _lib.ERR_CAPACITY or sm.first_past_limit != _lib.NO_DIFF or \
                        not any(w and x > c for w, x, c in zip((moved, meta, ix), need, caps)):
                    break
                caps = [max(c, x) if w else 0 for w, x, c in zip((moved, meta, ix), need, caps)]
            past = rc == _lib.ERR_CAPACITY and sm.first_past_limit != _lib.NO_DIFF
            if not past:
                self._check(rc, "hbx_datfile_compact")
            else:
                msg = self._L.hbx_last_error(self._ctx)
        finally:
            if arena is not None:
                self._L.hbx_arena_free(self._ctx, arena)
        summary = {k: int(getattr(sm, k)) for k, _ in _lib.DatCompactSummary._fields_}
        if summary["first_past_limit"] == _lib.NO_DIFF:
            summary["first_past_limit"] = None
        e = np.zeros(n, DAT_ENTRY_DTYPE)
        for name in DAT_ENTRY_DTYPE.names:
            e[name] = ent[name]
        if past:  # the plan is complete and nothing was packed: hand it to the caller with the error
            raise CompactLimitError(f"hbx_datfile_compact: HBX_ERR_CAPACITY: {msg.decode() if msg else ''}",
                                    DatCompact(e, klass[:n], new_off[:n], meta_off[:n], None, None, None, summary,
                                               int(file_no), int(dst)))
        return DatCompact(e, klass[:n], new_off[:n], meta_off[:n],
                          bufs[0][:need[0]].tobytes() if moved else None,
                          bufs[1][:need[1]].tobytes() if meta else None,
                          bufs[2][:need[2]].reshape(-1, _lib.IX_ENTRY).copy() if ix else None,
                          summary, int(file_no), int(dst))

    def match_paths(self, paths: Sequence[Union[str, os.PathLike]], chains_ids, io_threads: int = 16,
                    batch_bytes: int = 1 << 30, sizes: Optional[Sequence[int]] = None,
                    skip_unreadable: bool = False, chunks: bool = False) -> List[ChainMatch]:
        """Cut and hash local files as :meth:`store_paths` does and compare each
        file's block IDs with its stored chain ``chains_ids[f]`` on the device
        (hbx_store_paths_match): what diffFileData learns by fetching and
        comparing every block (restore.go:249-277), at the store path's speed
        and without a data block off the wire.  A file that is ``same`` equals
        the stored one; any other verdict leaves the question to the byte
        comparison (:meth:`diff_files`).  ``chunks=False`` is the verdict-only
        mode: 52 bytes per file come back.  ``chunks=True`` also returns each
        file's FileChunks.  ``sizes``, ``skip_unreadable`` and ``batch_bytes``
        (honoured down to 1 MiB) as in :meth:`store_paths`; the verdicts do not
        depend on the batches."""
        enc = [os.fsencode(p) for p in paths]
        if len(chains_ids) != len(enc):
            raise ValueError("one chain per path")
        if sizes is None:
            lens = np.array([os.stat(p).st_size for p in enc], np.uint64)
        else:
            lens = np.array(sizes, np.uint64).reshape(-1)
            if lens.size != len(enc):
                raise ValueError("sizes must have one entry per path")
        arr = (ctypes.c_char_p * max(len(enc), 1))(*enc)
        first, eids = _chain_lists(chains_ids)
        rec = (_lib.ChainMatch * max(len(enc), 1))()
        status = np.zeros(max(len(enc), 1), np.int32) if skip_unreadable else None
        if chunks:
            out = self._alloc_out(lens)
            caps, base, cuts, ids, sums = out
            outp = (_p(cuts), _p(ids), base.ctypes.data, caps.ctypes.data)
        else:
            out, sums, outp = None, (_lib.FileSummary * max(len(enc), 1))(), (None, None, None, None)
        t0 = time.perf_counter()
        self._check(self._L.hbx_store_paths_match(
            self._ctx, len(enc), ctypes.cast(arr, ctypes.c_void_p), _p(lens), *outp, sums,
            _p(status) if status is not None else None, int(io_threads), int(batch_bytes), first.ctypes.data,
            _p(eids), rec), "hbx_store_paths_match")
        self.last_call_s = time.perf_counter() - t0
        return self._match_result(lens, out, sums, rec, status)

    def wait(self):
        """Results of the oldest submitted batch ([] if none is pending): a
        list of FileChunks for a chunking batch, (ids, ok, n_bad) for a
        verify batch, a list of ChainMatch for a match batch."""
        if not self._pending:
            return []
        item = self._pending.popleft()
        t = time.perf_counter()
        rc = self._L.hbx_wait(self._ctx)
        self.wait_s += time.perf_counter() - t  # time inside hbx_wait (bench diagnostics)
        self._check(rc, "hbx_wait")
        if isinstance(item[0], str) and item[0] == "seg":
            _, lens, caps, base, cuts, ids, sums, keep = item
            sv = np.ctypeslib.as_array(sums)[:len(lens)]
            res = [FileChunks(cuts[b:b + k], ids[b:b + k], int(t), bytes(c.tobytes()) if t else b"")
                   for b, k, t, c in zip(base.astype(np.int64).tolist(), sv["n_chunks"].tolist(),
                                         sv["content_type"].tolist(), sv["content_id"])]
            if len(keep) > 2:  # submitted with a set: the K9 flags
                fb = keep[2].astype(bool)
                for r, b in zip(res, base.astype(np.int64).tolist()):
                    r.fresh = fb[b:b + r.n_chunks]
            return res
        if isinstance(item[0], str) and item[0] == "match":
            _, lens, out, sums, rec, _keep = item
            return self._match_result(lens, out, sums, rec)
        if isinstance(item[0], str):  # ("verify", ...)
            _, n, ids, ok, bad, keep = item
            return ids[:n], (ok[:n].astype(bool) if keep[1] is not None else None), int(bad.value)
        offs, lens, caps, base, cuts, ids, sums = item[:7]
        return self._unpack(lens, caps, base, cuts, ids, sums, item[7] if len(item) > 7 else None)

    def verify_submit_device(self, d_arena: int, offs: Sequence[int], lens: Sequence[int],
                             links: Optional[Sequence[Sequence[bytes]]] = None,
                             expect: Optional[Sequence[bytes]] = None):
        """Pipelined VerifyBlock of device-resident blocks (hbx_verify_submit_device):
        returns at once; :meth:`wait` (FIFO with chunking batches) returns
        (ids, ok, n_bad)."""
        self._after_producer()
        offs = np.ascontiguousarray(offs, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint64)
        n = int(lens.size)
        links_a, base, counts = self._links_arrays(links, n)
        ids = np.zeros((max(n, 1), 16), np.uint8)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(bytes(e) for e in expect), np.uint8))
            if exp.size != 16 * n:
                raise ValueError("expect must hold one 16-byte ID per block")
        ok = np.zeros(max(n, 1), np.uint8)
        bad = ctypes.c_uint64(0)
        self._check(self._L.hbx_verify_submit_device(
            self._ctx, ctypes.c_void_p(int(d_arena)), n, _p(offs), _p(lens),
            _p(links_a) if links_a is not None else None, _p(base) if base is not None else None,
            _p(counts) if counts is not None else None, _p(ids), _p(exp) if exp is not None else None,
            _p(ok), ctypes.byref(bad)), "hbx_verify_submit_device")
        # everything the library writes or reads until the wait stays alive here
        self._pending.append(("verify", n, ids, ok, bad, (offs, exp, lens)))

    def pending(self) -> int:
        n = self._L.hbx_pending(self._ctx)
        if n < 0:
            self._check(n, "hbx_pending")
        return int(n)

    def set_md5_slice(self, blocks: int):
        """MD5 blocks per chain per K3 launch (0 = unlimited)."""
        self._check(self._L.hbx_set_md5_slice(self._ctx, int(blocks)), "hbx_set_md5_slice")

    def input_after_oldest(self):
        """The next input copy / batch may reuse the oldest pending batch's
        device memory: a GPU-side wait for its hashing to finish
        (hbx_input_after_oldest)."""
        self._check(self._L.hbx_input_after_oldest(self._ctx), "hbx_input_after_oldest")

    def input_fence(self, stream: Optional[int] = None):
        """Enqueue the pending wait of :meth:`input_after_oldest` now, and on
        ``stream`` (a raw hipStream_t handle) too: needed before the caller
        writes the old batch's memory with its own work (hbx_input_fence)."""
        self._check(self._L.hbx_input_fence(self._ctx, ctypes.c_void_p(int(stream) if stream else 0)),
                    "hbx_input_fence")

    def set_k3_probe(self, on: bool = True):
        """Diagnostics: per-wave records of every K3 launch (hbx_set_k3_probe)."""
        self._check(self._L.hbx_set_k3_probe(self._ctx, int(bool(on))), "hbx_set_k3_probe")

    def set_join_lag(self, lag: int):
        """Submits between a batch's own and the MD5 launch its chains join
        (1..4; 2 gives a small batch's scan a whole extra step)."""
        self._check(self._L.hbx_set_join_lag(self._ctx, int(lag)), "hbx_set_join_lag")

    def set_k3_period(self, period: int):
        """One K3 launch every ``period`` submits (1..8) with ``period`` x the
        slice per chain: small batches pay the launch's start-up and tail once
        per period (hbx_set_k3_period)."""
        self._check(self._L.hbx_set_k3_period(self._ctx, int(period)), "hbx_set_k3_period")

    def k3_wave_times(self) -> np.ndarray:
        """Diagnostics (:meth:`set_k3_probe`): per-wave records of the
        latest K3 launch, shape (waves, 8): start, start-up end | XCC << 56,
        end (100 MHz ticks), R | max count << 16 | HW_ID << 32, then the
        first group's cooperative phase: s_memtime at its start and end,
        s_memrealtime at its end, blocks per chain (R - 1)."""
        n = ctypes.c_uint32(0)
        self._check(self._L.hbx_k3_wave_times(self._ctx, None, 0, ctypes.byref(n)), "hbx_k3_wave_times")
        out = np.zeros((max(n.value, 1), 8), np.uint64)
        self._check(self._L.hbx_k3_wave_times(self._ctx, _p(out), n.value, ctypes.byref(n)), "hbx_k3_wave_times")
        return out[:n.value]

    def k1_summaries(self):
        """Diagnostics: the slice summaries K1 stored for the latest
        synchronous device batch (hbx_k1_summaries).  Returns (first, count,
        pairs): per file its first slice and slice count, and pairs[j] =
        (smax, sprev) of slice j, uint32, shape (slices, 2)."""
        nf, ns = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self._L.hbx_k1_summaries(self._ctx, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(ns))
        if rc != _lib.ERR_CAPACITY:
            self._check(rc, "hbx_k1_summaries")
        first, count = np.zeros(max(nf.value, 1), np.uint64), np.zeros(max(nf.value, 1), np.uint64)
        pairs = np.zeros((max(ns.value, 1), 2), np.uint32)
        self._check(self._L.hbx_k1_summaries(self._ctx, _p(first), _p(count), nf.value, ctypes.byref(nf), _p(pairs),
                                             ns.value, ctypes.byref(ns)), "hbx_k1_summaries")
        return first[:nf.value], count[:nf.value], pairs[:ns.value]

    def knobs(self) -> dict:
        """The context's effective pipeline knobs (hbx_knobs), including
        whether HBX_* A/B switches were honoured (only with HBX_AB=1)."""
        import json
        buf = ctypes.create_string_buffer(4096)
        self._check(self._L.hbx_knobs(self._ctx, buf, len(buf)), "hbx_knobs")
        return json.loads(buf.value.decode())

    def reserve(self, batches: int, files: int, nbytes: int):
        """Pre-size the pipeline for ``batches`` batches in flight of up to
        ``files`` files / ``nbytes`` bytes each, so the steady state never
        allocates (an allocation drains both streams)."""
        self._check(self._L.hbx_reserve(self._ctx, int(batches), int(files), int(nbytes)),
                    "hbx_reserve")

    def plan_pipeline(self, **kw) -> dict:
        """hbx_plan_pipeline on this context (free_bytes=0: the device's free
        memory now); see the module function :func:`plan_pipeline`."""
        return plan_pipeline(engine=self, **kw)

    def apply_plan(self, plan: dict, files: int, nbytes: int):
        """hbx_apply_plan: the plan's slice, join lag and K3 period, and R + 2
        reserved batches of up to `files` files and `nbytes` bytes."""
        pp = _lib.PipelinePlan(**{k: int(plan[k]) for k in _PLAN_KEYS})
        self._check(self._L.hbx_apply_plan(self._ctx, ctypes.byref(pp), int(files), int(nbytes)), "hbx_apply_plan")

    def stage_totals(self, reset: bool = False):
        """Cumulative device ms and launch counts per kernel: K1, K2, plan, K3, K4."""
        ms = (ctypes.c_double * 5)()
        n = (ctypes.c_uint64 * 5)()
        self._check(self._L.hbx_stage_totals(self._ctx, ms, n, int(bool(reset))), "hbx_stage_totals")
        return np.array(list(ms), np.float64), np.array(list(n), np.int64)

    def block_id(self, data: BytesLike, links: Sequence[bytes] = ()) -> bytes:
        """HashboxBlock.HashData (pkg/core/block.go:96-111) on the device."""
        a = _u8(data)
        ln = np.frombuffer(b"".join(bytes(x) for x in links), np.uint8) if links else \
            np.zeros(0, np.uint8)
        out = np.zeros(16, np.uint8)
        self._check(self._L.hbx_block_id(self._ctx, _p(ln), len(links), _p(a), a.size, _p(out)),
                    "hbx_block_id")
        return out.tobytes()

    def md5(self, data: BytesLike) -> bytes:
        """core.Hash (pkg/core/core.go:46-48): MD5 of the raw bytes on the device."""
        a = _u8(data)
        out = np.zeros(16, np.uint8)
        self._check(self._L.hbx_md5(self._ctx, _p(a), a.size, _p(out)), "hbx_md5")
        return out.tobytes()

    def hmac(self, data: bytes, key: bytes) -> bytes:
        """core.Hmac (pkg/core/core.go:51-68) with the device MD5 as the hash."""
        k = (bytes(key) + bytes(16))[:16] + bytes(48)  # Byte128 key, zero-padded to md5.BlockSize
        inner = self.md5(bytes(b ^ 0x36 for b in k) + bytes(data))
        return self.md5(bytes(b ^ 0x5C for b in k) + inner)

    def deep_hmac(self, depth: int, data: bytes, key: bytes) -> bytes:
        """core.DeepHmac (pkg/core/core.go:70-80): depth rounds of Hmac."""
        h, d = bytes(16), bytes(data)
        for _ in range(depth):
            h = d = self.hmac(d, key)
        return h

    @staticmethod
    def _links_arrays(links_per_block: Optional[Sequence[Sequence[bytes]]], n: int):
        if not links_per_block or not any(len(x) for x in links_per_block):
            return None, None, None
        counts = np.array([len(x) for x in links_per_block], np.uint32)
        base = np.zeros(n, np.uint64)
        base[1:] = np.cumsum(counts.astype(np.uint64))[:-1]
        flat = np.frombuffer(b"".join(bytes(l) for x in links_per_block for l in x), np.uint8)
        if flat.size != 16 * int(counts.sum()):
            raise ValueError("every link must be a 16-byte block ID")
        return np.ascontiguousarray(flat), base, counts

    def _verify(self, fn, lead_args, n, links, expect):
        links_a, base, counts = self._links_arrays(links, n)
        ids = np.zeros((max(n, 1), 16), np.uint8)
        exp = None
        if expect is not None:
            exp = np.ascontiguousarray(np.frombuffer(b"".join(bytes(e) for e in expect), np.uint8))
            if exp.size != 16 * n:
                raise ValueError("expect must hold one 16-byte ID per block")
        ok = np.zeros(max(n, 1), np.uint8)
        bad = ctypes.c_uint64(0)
        self._check(fn(self._ctx, *lead_args,
                       _p(links_a) if links_a is not None else None,
                       _p(base) if base is not None else None,
                       _p(counts) if counts is not None else None,
                       _p(ids), _p(exp) if exp is not None else None, _p(ok), ctypes.byref(bad)),
                    fn.__name__)
        return ids[:n], (ok[:n].astype(bool) if expect is not None else None), int(bad.value)

    def verify_blocks(self, blocks: Sequence[BytesLike], links: Optional[Sequence[Sequence[bytes]]] = None,
                      expect: Optional[Sequence[bytes]] = None):
        """HashboxBlock.HashData / VerifyBlock (pkg/core/block.go:96-111,
        152-174) for many uncompressed blocks at once.  Returns (ids [n,16],
        ok [n] bool or None, number of mismatches)."""
        arrs = [_u8(b) for b in blocks]
        n = len(arrs)
        lens = np.array([a.size for a in arrs], np.uint64)
        ptrs = np.array([_p(a) for a in arrs], np.uint64)
        return self._verify(self._L.hbx_verify_blocks, (n, _p(ptrs), _p(lens)), n, links, expect)

    def verify_blocks_device(self, d_arena: int, offs: Sequence[int], lens: Sequence[int],
                             links: Optional[Sequence[Sequence[bytes]]] = None,
                             expect: Optional[Sequence[bytes]] = None):
        """The same for blocks resident in device memory (each followed by
        >= 64 readable bytes)."""
        self._after_producer()
        offs = np.ascontiguousarray(offs, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint64)
        n = int(lens.size)
        return self._verify(self._L.hbx_verify_blocks_device,
                            (ctypes.c_void_p(int(d_arena)), n, _p(offs), _p(lens)), n, links, expect)

    def deflate_bound(self, n: int) -> int:
        """Largest zlib stream hbx_deflate_blocks* produces for n bytes."""
        return int(self._L.hbx_deflate_bound(int(n)))

    def deflate_blocks(self, blocks: Sequence[BytesLike]) -> List[bytes]:
        """HashboxBlock.CompressData (pkg/core/block.go:133-150, 176-184) for
        many blocks at once: one zlib stream per block, coded on the device."""
        arrs = [_u8(b) for b in blocks]
        n = len(arrs)
        if n == 0:
            return []
        lens = np.array([a.size for a in arrs], np.uint64)
        caps = np.array([self.deflate_bound(int(x)) for x in lens], np.uint64)
        outs = [np.empty(int(c), np.uint8) for c in caps]
        dptr = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
        optr = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
        olen = np.zeros(n, np.uint64)
        self._check(self._L.hbx_deflate_blocks(self._ctx, n, dptr, _p(lens), optr, _p(caps), _p(olen)),
                    "hbx_deflate_blocks")
        return [o[:int(k)].tobytes() for o, k in zip(outs, olen)]

    def deflate_blocks_device(self, d_arena: int, offs: Sequence[int], lens: Sequence[int], d_out: int,
                              out_offs: Sequence[int], out_caps: Sequence[int]) -> np.ndarray:
        """Device form: block i = d_arena[offs[i] ..+lens[i]) -> zlib stream at
        d_out[out_offs[i] ..]; returns the stream lengths."""
        self._after_producer()
        offs = np.ascontiguousarray(offs, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint64)
        oo = np.ascontiguousarray(out_offs, np.uint64)
        oc = np.ascontiguousarray(out_caps, np.uint64)
        olen = np.zeros(max(lens.size, 1), np.uint64)
        self._check(self._L.hbx_deflate_blocks_device(self._ctx, ctypes.c_void_p(int(d_arena)), lens.size,
                                                      _p(offs), _p(lens), ctypes.c_void_p(int(d_out)), _p(oo),
                                                      _p(oc), _p(olen)), "hbx_deflate_blocks_device")
        return olen[:lens.size]

    def inflate_blocks_device(self, d_in: int, in_offs: Sequence[int], in_lens: Sequence[int], d_out: int,
                              out_offs: Sequence[int], out_caps: Sequence[int]):
        """HashboxBlock.UncompressData (block.go:113-131) of many zlib streams on
        the device: returns (out_lens, status) (status 0 = ok)."""
        self._after_producer()
        io = np.ascontiguousarray(in_offs, np.uint64)
        il = np.ascontiguousarray(in_lens, np.uint64)
        oo = np.ascontiguousarray(out_offs, np.uint64)
        oc = np.ascontiguousarray(out_caps, np.uint64)
        n = int(il.size)
        ol = np.zeros(max(n, 1), np.uint64)
        st = np.zeros(max(n, 1), np.uint32)
        self._check(self._L.hbx_inflate_blocks_device(self._ctx, ctypes.c_void_p(int(d_in)), n, _p(io), _p(il),
                                                      ctypes.c_void_p(int(d_out)), _p(oo), _p(oc), _p(ol),
                                                      _p(st)), "hbx_inflate_blocks_device")
        return ol[:n], st[:n]

    def inflate_blocks(self, streams: Sequence[BytesLike], caps: Sequence[int]):
        """Host convenience: inflate zlib streams on the device; returns
        (list of bytes or None per stream, status array)."""
        import torch
        arrs = [_u8(z) for z in streams]
        n = len(arrs)
        if n == 0:
            return [], np.zeros(0, np.uint32)
        io = np.zeros(n, np.uint64)
        pos = 0
        for i, a in enumerate(arrs):
            io[i] = pos
            pos += (a.size + 255) // 256 * 256
        host = np.zeros(pos + 64, np.uint8)
        for i, a in enumerate(arrs):
            host[int(io[i]):int(io[i]) + a.size] = a
        oc = np.ascontiguousarray(caps, np.uint64)
        oo = np.zeros(n, np.uint64)
        oo[1:] = np.cumsum((oc[:-1] + 255) // 256 * 256)
        dev = torch.device("cuda", self.device)  # this engine's GPU, not torch's current one
        d_in = torch.from_numpy(host).to(dev)
        d_out = torch.zeros(int(oo[-1] + oc[-1]) + 64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ol, st = self.inflate_blocks_device(d_in.data_ptr(), io, [a.size for a in arrs], d_out.data_ptr(), oo, oc)
        out = d_out.cpu().numpy()
        return [out[int(oo[i]):int(oo[i] + ol[i])].tobytes() if st[i] == 0 else None for i in range(n)], st

    # ------------------------------------------------------ restore / diff --
    def restore_blocks(self, datas: Sequence[BytesLike], types: Sequence[int], ids,
                       links: Optional[Sequence[Sequence[bytes]]] = None, local: Optional[BytesLike] = None,
                       max_block: Optional[int] = None, out: Optional[np.ndarray] = None) -> RestoredBlocks:
        """restoreFileData / diffFileData over the blocks of one chain, in file
        order (hashback/restore.go:45-66, 249-277; hbx_restore_blocks): block i
        has the data field ``datas[i]`` as read off the wire, the DataType
        ``types[i]`` (0xff raw, 0x01 zlib) and must hash, with ``links[i]``, to
        ``ids[i]``.  Every block is inflated and verified on the device as
        VerifyBlock does; the result covers the blocks before the first bad
        one.  With ``local`` (the local copy's bytes) nothing is assembled and
        ``first_diff`` is the first offset at which the two differ.  ``out``
        (a uint8 array) receives the bytes instead of a fresh buffer."""
        arrs = [_u8(d) for d in datas]
        n = len(arrs)
        ida = _ids_array(ids)
        if ida.shape[0] != n or len(types) != n:
            raise ValueError("one type and one 16-byte ID per block")
        mb = int(max_block) if max_block else _lib.MAX_BLOCK
        lens = np.array([a.size for a in arrs], np.uint64)
        ty = np.ascontiguousarray(types, np.uint8)
        ptrs = np.array([_p(a) for a in arrs], np.uint64)
        links_a, base, counts = self._links_arrays(links, n)
        offs = np.zeros(n + 1, np.uint64)
        status = np.zeros(max(n, 1), np.uint32)
        n_good, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
        loc = None
        if local is not None:
            if out is not None:
                raise ValueError("out and local exclude each other")
            loc = _u8(local)
            if loc.size == 0:  # (a NULL pointer would mean "no local copy")
                loc = np.zeros(1, np.uint8)[:0]
            out_p, out_cap = None, 0
            loc_p = ctypes.c_void_p(loc.ctypes.data)
        else:
            if out is None:  # an upper bound: deflate expands at most 1032-fold
                cap = sum(int(k) if t == _lib.BLOCK_RAW else min(mb, 1032 * int(k) + 64)
                          for k, t in zip(lens.tolist(), ty.tolist()))
                out = np.empty(max(cap, 1), np.uint8)
            out_p, out_cap, loc_p = ctypes.c_void_p(out.ctypes.data), int(out.size), None
        self._check(self._L.hbx_restore_blocks(
            self._ctx, n, _p(ptrs), _p(lens), _p(ty), _p(ida),
            _p(links_a) if links_a is not None else None, _p(base) if base is not None else None,
            _p(counts) if counts is not None else None, int(max_block or 0), out_p, out_cap,
            loc_p, int(loc.size) if loc is not None else 0, _p(offs), _p(status), ctypes.byref(n_good),
            ctypes.byref(first)), "hbx_restore_blocks")
        g = int(n_good.value)
        data = out[:int(offs[g])].tobytes() if loc is None else None
        fd = None if loc is None or first.value == _lib.NO_DIFF else int(first.value)
        return RestoredBlocks(data, offs[:g + 1].copy(), status[:n].copy(), g, fd)

    def _restore_stream(self, ids, source, out_path, on_data, local_path, window_bytes: int, max_block):
        ida = _ids_array(ids)
        n = int(ida.shape[0])
        raised = []

        def src(_user, index, dst, cap, plen, ptype):
            try:
                t, data = source(int(index))
                a = _u8(data)
                plen[0] = a.size
                ptype[0] = int(t)
                if 0 < a.size <= cap:
                    ctypes.memmove(dst, a.ctypes.data, a.size)
                return 0
            except BaseException as e:  # never unwind through C: a non-zero return, re-raised below
                raised.append(e)
                return 1

        def sink(_user, off, data, ln):
            try:
                on_data(int(off), np.frombuffer((ctypes.c_uint8 * ln).from_address(data), np.uint8) if ln
                        else np.zeros(0, np.uint8))
                return 0
            except BaseException as e:
                raised.append(e)
                return 1

        cb_src = _lib.BLOCK_SOURCE(src)
        cb_sink = _lib.RESTORE_SINK(sink) if on_data is not None else None
        nbytes, bad_i, first = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        bad_s = ctypes.c_uint32(0)
        t0 = time.perf_counter()
        rc = self._L.hbx_restore_file_stream(
            self._ctx, n, _p(ida), ctypes.cast(cb_src, ctypes.c_void_p), None, int(window_bytes),
            os.fsencode(out_path) if out_path is not None else None,
            ctypes.cast(cb_sink, ctypes.c_void_p) if cb_sink is not None else None,
            os.fsencode(local_path) if local_path is not None else None, int(max_block or 0),
            ctypes.byref(nbytes), ctypes.byref(bad_i), ctypes.byref(bad_s), ctypes.byref(first))
        self.last_call_s = time.perf_counter() - t0
        if raised:
            raise raised[0]
        if rc in (_lib.ERR_VERIFY, _lib.ERR_IO):
            msg = self._L.hbx_last_error(self._ctx)
            raise RestoreError(f"hbx_restore_file_stream: {_lib.ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}",
                               rc, int(bad_i.value) if rc == _lib.ERR_VERIFY else None, int(bad_s.value),
                               int(nbytes.value))
        self._check(rc, "hbx_restore_file_stream")
        return int(nbytes.value), int(first.value)

    def restore_file(self, ids, source: Callable[[int], tuple], out_path=None,
                     on_data: Optional[Callable[[int, np.ndarray], None]] = None, window_bytes: int = 0,
                     max_block: Optional[int] = None) -> int:
        """restoreFileData over a whole chain of any length
        (hashback/restore.go:45-66, 116-135; hbx_restore_file_stream):
        ``source(i)`` returns block i's ``(type, data field)``; the file is
        written to ``out_path``, or handed to ``on_data(file_offset, bytes)``
        window by window, in order (the array is valid during the call only).
        Host and device memory depend on ``window_bytes`` only.  Returns the
        bytes restored.  A bad block raises :class:`RestoreError` (its
        ``bad_index``, ``bad_status``); everything before it was written.
        An exception raised by ``source`` or ``on_data`` stops the call and is
        re-raised here.  Neither may call this engine."""
        if (out_path is None) == (on_data is None):
            raise ValueError("exactly one of out_path and on_data")
        return self._restore_stream(ids, source, out_path, on_data, None, window_bytes, max_block)[0]

    def diff_file(self, ids, source: Callable[[int], tuple], local_path, window_bytes: int = 0,
                  max_block: Optional[int] = None):
        """diffFileData over a whole chain (hashback/restore.go:249-277):
        every block verified, its data compared with ``local_path`` at the
        running offset on the device.  Returns ``(same, first_diff)``:
        ``first_diff`` is the first differing file offset (the shorter length
        when one side only ends early), None when the two are equal."""
        _, first = self._restore_stream(ids, source, None, None, local_path, window_bytes, max_block)
        return (True, None) if first == _lib.NO_DIFF else (False, first)

    # ------------------------------------------- restore / diff, many files --
    def restore_files_blocks(self, chains: Sequence[Sequence[tuple]], size_hints: Optional[Sequence[int]] = None,
                             local: Optional[Sequence[BytesLike]] = None, max_block: Optional[int] = None,
                             out: Optional[np.ndarray] = None) -> RestoredFiles:
        """restoreFileData / diffFileData over the chains of many files in one
        call (hashback/restore.go:45-66, 137-162, 249-277;
        hbx_restore_files_blocks): ``chains[f]`` lists file f's blocks in order
        as ``(type, data field, id[, links])``.  A directory or chain block is
        a one-block file with its links.  Windows are formed across files; the
        prefix rule holds per file.  ``size_hints[f]`` (FileEntry.FileSize, 0 =
        unknown) sizes the inflate slots and changes no result.  With ``local``
        (one local copy per file) nothing is assembled and ``first_diff[f]`` is
        the first offset at which file f differs."""
        nf = len(chains)
        first = np.zeros(nf + 1, np.uint64)
        first[1:] = np.cumsum([len(ch) for ch in chains], dtype=np.uint64)
        blocks = [b for ch in chains for b in ch]
        n = len(blocks)
        arrs = [_u8(b[1]) for b in blocks]
        ida = _ids_array([b[2] for b in blocks])
        ty = np.array([int(b[0]) for b in blocks], np.uint8)
        lens = np.array([a.size for a in arrs], np.uint64)
        ptrs = np.array([_p(a) for a in arrs], np.uint64)
        links_a, base, counts = self._links_arrays([list(b[3]) if len(b) > 3 and b[3] else [] for b in blocks], n)
        mb = int(max_block) if max_block else _lib.MAX_BLOCK
        hints = None
        if size_hints is not None:
            hints = np.ascontiguousarray(size_hints, np.uint64)
            if hints.size != nf:
                raise ValueError("one size hint per file")
        blk_offs = np.zeros(max(n, 1), np.uint64)
        status = np.zeros(max(n, 1), np.uint32)
        n_good = np.zeros(max(nf, 1), np.uint64)
        first_diff = np.zeros(max(nf, 1), np.uint64)
        out_offs = np.zeros(nf + 1, np.uint64)
        loc = loc_offs = None
        if local is not None:
            if out is not None:
                raise ValueError("out and local exclude each other")
            if len(local) != nf:
                raise ValueError("one local copy per file")
            la = [_u8(x) for x in local]
            loc_offs = np.zeros(nf + 1, np.uint64)
            loc_offs[1:] = np.cumsum([a.size for a in la], dtype=np.uint64)
            loc = np.concatenate(la + [np.zeros(1, np.uint8)])  # never NULL: that would mean "no local copy"

        def call(o):
            return self._L.hbx_restore_files_blocks(
                self._ctx, nf, _p(first), _p(ptrs), _p(lens), _p(ty), _p(ida),
                _p(links_a) if links_a is not None else None, _p(base) if base is not None else None,
                _p(counts) if counts is not None else None, _p(hints) if hints is not None else None,
                int(max_block or 0), ctypes.c_void_p(o.ctypes.data) if o is not None else None,
                int(o.size) if o is not None else 0, _p(out_offs),
                ctypes.c_void_p(loc.ctypes.data) if loc is not None else None,
                _p(loc_offs) if loc_offs is not None else None, _p(blk_offs), _p(status), _p(n_good), _p(first_diff))

        def bound(hinted):  # an upper bound of the packed image: deflate expands at most 1032-fold
            tot = 0
            for f in range(nf):
                h = int(hints[f]) if hinted and hints is not None else 0
                for i in range(int(first[f]), int(first[f + 1])):
                    k = int(lens[i])
                    tot += k if ty[i] == _lib.BLOCK_RAW else min(mb, h or 1032 * k + 64)
            return max(tot, 1)

        if loc is not None:
            rc = call(None)
        elif out is not None:
            rc = call(out)
        else:
            out = np.empty(bound(True), np.uint8)
            rc = call(out)
            if rc == _lib.ERR_CAPACITY and hints is not None:  # a hint was too small: it is never trusted
                out = np.empty(bound(False), np.uint8)
                rc = call(out)
        self._check(rc, "hbx_restore_files_blocks")
        fo = [int(x) for x in first]
        data = fds = None
        if loc is None:
            oo = [int(x) for x in out_offs]
            data = [out[oo[f]:oo[f + 1]].tobytes() for f in range(nf)]
        else:
            fds = [None if int(x) == _lib.NO_DIFF else int(x) for x in first_diff[:nf]]
        return RestoredFiles(data, out_offs, [blk_offs[fo[f]:fo[f + 1]].copy() for f in range(nf)],
                             [status[fo[f]:fo[f + 1]].copy() for f in range(nf)], n_good[:nf].astype(np.int64), fds)

    def _restore_files_stream(self, chains_ids, source, out_paths, local_paths, size_hints, window_bytes: int,
                              io_threads: int, max_block) -> List[RestoredFile]:
        nf = len(chains_ids)
        first = np.zeros(nf + 1, np.uint64)
        first[1:] = np.cumsum([len(ch) for ch in chains_ids], dtype=np.uint64)
        ida = _ids_array([i for ch in chains_ids for i in ch])
        paths = out_paths if out_paths is not None else local_paths
        if len(paths) != nf:
            raise ValueError("one path per file")
        enc = [os.fsencode(p) for p in paths]
        parr = (ctypes.c_char_p * max(nf, 1))(*enc)
        hints = None
        if size_hints is not None:
            hints = np.ascontiguousarray(size_hints, np.uint64)
            if hints.size != nf:
                raise ValueError("one size hint per file")
        raised = []

        def src(_user, f, index, dst, cap, plen, ptype):
            try:
                t, data = source(int(f), int(index))
                a = _u8(data)
                plen[0] = a.size
                ptype[0] = int(t)
                if 0 < a.size <= cap:
                    ctypes.memmove(dst, a.ctypes.data, a.size)
                return 0
            except BaseException as e:  # never unwind through C: a non-zero return, re-raised below
                raised.append(e)
                return 1

        cb = _lib.FILE_BLOCK_SOURCE(src)
        res = (_lib.RestoredFile * max(nf, 1))()
        t0 = time.perf_counter()
        rc = self._L.hbx_restore_files_stream(
            self._ctx, nf, _p(first), _p(ida), ctypes.cast(cb, ctypes.c_void_p), None,
            _p(hints) if hints is not None else None, int(window_bytes),
            parr if out_paths is not None else None, parr if local_paths is not None else None,
            int(io_threads), int(max_block or 0), res)
        self.last_call_s = time.perf_counter() - t0
        if raised:
            raise raised[0]
        if rc == _lib.ERR_IO:
            msg = self._L.hbx_last_error(self._ctx)
            raise RestoreError(f"hbx_restore_files_stream: HBX_ERR_IO: {msg.decode() if msg else ''}", rc, None, 0,
                               sum(int(res[f].bytes) for f in range(nf)))
        self._check(rc, "hbx_restore_files_stream")
        return [RestoredFile(int(r.bytes), int(r.n_good), None if r.bad_index == _lib.NO_DIFF else int(r.bad_index),
                             int(r.bad_status), int(r.err), None if r.first_diff == _lib.NO_DIFF else int(r.first_diff))
                for r in res[:nf]]

    def restore_files(self, chains_ids, source: Callable[[int, int], tuple], out_paths, size_hints=None,
                      window_bytes: int = 0, io_threads: int = 16, max_block: Optional[int] = None
                      ) -> List[RestoredFile]:
        """restoreFileData for many files in one call (restore.go:45-66,
        137-162; hbx_restore_files_stream): ``chains_ids[f]`` lists the block
        IDs of file f, ``source(f, i)`` returns its block i as ``(type, data
        field)``, ``out_paths[f]`` is created or truncated and receives the
        file's good prefix.  Windows hold blocks of many files, two in flight;
        ``io_threads`` (at most 16) writers.  Returns one :class:`RestoredFile`
        per file: a bad block (``bad_index``, ``bad_status``) or a path that
        cannot be written (``errno``) is that file's result and the others
        complete.  A failing source raises (:class:`RestoreError` with
        ``code == _lib.ERR_IO``, or the exception ``source`` raised)."""
        return self._restore_files_stream(chains_ids, source, out_paths, None, size_hints, window_bytes, io_threads,
                                          max_block)

    def diff_files(self, chains_ids, source: Callable[[int, int], tuple], local_paths, size_hints=None,
                   window_bytes: int = 0, io_threads: int = 16, max_block: Optional[int] = None):
        """diffFileData for many files in one call (restore.go:249-277,
        279-414): returns one ``(same, first_diff)`` per file, ``first_diff``
        the first differing offset inside the file (the shorter length when one
        side only ends early), None when the two are equal.  A file with a bad
        block is never the same (its good prefix is what was compared); a local
        copy that cannot be read is ``(False, None)``."""
        res = self._restore_files_stream(chains_ids, source, None, local_paths, size_hints, window_bytes, io_threads,
                                         max_block)
        return [(r.first_diff is None and r.bad_index is None and r.errno == 0, r.first_diff) for r in res]

    def memcpy_h2d_async(self, d_dst: int, h_src: int, nbytes: int):
        """Enqueue an H2D copy on this engine's stream (pinned source)."""
        self._check(self._L.hbx_memcpy_h2d_async(self._ctx, ctypes.c_void_p(int(d_dst)),
                                                 ctypes.c_void_p(int(h_src)), int(nbytes)),
                    "hbx_memcpy_h2d_async")

    def store_paths(self, paths: Sequence[Union[str, os.PathLike]], io_threads: int = 16,
                    batch_bytes: int = 1 << 30, compress: bool = False,
                    on_batch: Optional[Callable[[int, int], None]] = None,
                    on_files: Optional[Callable[[int, List[FileChunks]], None]] = None,
                    sizes: Optional[Sequence[int]] = None,
                    skip_unreadable: bool = False, dedup: Optional[IdSet] = None) -> List[FileChunks]:
        """storeFile for many files on disk, end to end: the library reads them
        into pinned memory on ``io_threads`` threads and overlaps reading the
        next batch with the copy + kernels of the current one.  With
        ``compress`` every chunk is also zlib-compressed on the device
        (HashboxBlock.CompressData, the client's send path) and returned in
        ``FileChunks.zstreams``.  ``on_batch(first, count)`` (compress only)
        runs on this thread as soon as files [first, first+count) have their
        ids, summaries and zlib streams written (hbx_store_paths_zcb), so a
        sender can ship them while later batches are still read and hashed.
        ``on_files(first, files)`` is the same callback handed the finished
        FileChunks (ids, cut ends, zlib stream views) of those files.
        ``sizes`` are the files' byte sizes when the caller already has them
        (storeFile takes the walker's FileEntry with FileSize, store.go:84,
        247); otherwise each path is stat'ed here.  A file shorter than its
        size fails the call (HBX_ERR_IO); bytes past it are not read.  With
        ``skip_unreadable`` (hbx_store_paths_status) a file the reference skips
        without stopping the walk -- open() failing (store.go:101-103,
        221-224) or a read failing with EBADF (minorPathError,
        hashback_unix.go:57-63) -- comes back with no chunks and its errno in
        ``FileChunks.errno``, and the rest of its batch is stored; any other
        read error still fails the call.  With ``dedup`` (hbx_store_paths_dd)
        every chunk's ID is marked against that set in file order:
        ``FileChunks.fresh`` says which chunks are new, only those are
        compressed (the ``zstreams`` entry of any other chunk is an empty
        view), ``batch_bytes`` is honoured down to 1 MiB, and a call that
        fails leaves the set as it was.  ``last_call_s`` holds the library
        call's wall seconds."""
        if (on_batch is not None or on_files is not None) and not compress:
            raise ValueError("on_batch / on_files need compress=True (hbx_store_paths_zcb)")
        enc = [os.fsencode(p) for p in paths]
        if sizes is None:
            lens = np.array([os.stat(p).st_size for p in enc], np.uint64)
        else:
            lens = np.array(sizes, np.uint64).reshape(-1)
            if lens.size != len(enc):
                raise ValueError("sizes must have one entry per path")
        arr = (ctypes.c_char_p * max(len(enc), 1))(*enc)
        caps, base, cuts, ids, sums = self._alloc_out(lens)
        status = np.zeros(max(len(enc), 1), np.int32) if skip_unreadable else None
        fresh = np.zeros(cuts.shape[0], np.uint8) if dedup is not None else None
        dd_status = _p(status) if status is not None else None
        dd_tail = (dedup._h, _p(fresh)) if dedup is not None else ()

        def with_status(res):
            if status is not None:
                for r, e in zip(res, status[:len(res)].tolist()):
                    r.errno = int(e)
            return res

        if not compress:
            t0 = time.perf_counter()
            if dedup is not None:
                self._check(self._L.hbx_store_paths_dd(
                    self._ctx, len(enc), ctypes.cast(arr, ctypes.c_void_p), _p(lens), _p(cuts), _p(ids), _p(base),
                    _p(caps), sums, dd_status, int(io_threads), int(batch_bytes), None, None, None, None, None,
                    None, *dd_tail), "hbx_store_paths_dd")
            elif status is None:
                self._check(self._L.hbx_store_paths(self._ctx, len(enc), ctypes.cast(arr, ctypes.c_void_p),
                                                    _p(lens), _p(cuts), _p(ids), _p(base), _p(caps), sums,
                                                    int(io_threads), int(batch_bytes)), "hbx_store_paths")
            else:
                self._check(self._L.hbx_store_paths_status(
                    self._ctx, len(enc), ctypes.cast(arr, ctypes.c_void_p), _p(lens), _p(cuts), _p(ids), _p(base),
                    _p(caps), sums, _p(status), int(io_threads), int(batch_bytes), None, None, None, None, None,
                    None), "hbx_store_paths_status")
            self.last_call_s = time.perf_counter() - t0
            return with_status(self._unpack(lens, caps, base, cuts, ids, sums, fresh))
        fb = np.array([self._L.hbx_deflate_file_bound(int(x)) for x in lens], np.uint64)
        zbase = np.zeros(max(lens.size, 1), np.uint64)
        if lens.size > 1:
            zbase[1:lens.size] = np.cumsum(fb[:-1])
        zout = _huge_host_buffer(int(fb.sum()) + 16)
        zoff = np.zeros(max(int(caps.sum()), 1), np.uint64)
        zlen = np.zeros_like(zoff)
        zargs = (self._ctx, len(enc), ctypes.cast(arr, ctypes.c_void_p), _p(lens), _p(cuts), _p(ids),
                 _p(base), _p(caps), sums, int(io_threads), int(batch_bytes), _p(zout), _p(zbase),
                 _p(zoff), _p(zlen))
        def view(f: int) -> FileChunks:  # file f's results, as soon as its batch is reported
            s = sums[f]
            k, b = int(s.n_chunks), int(base[f])
            r = FileChunks(cuts[b:b + k].copy(), ids[b:b + k].copy(), int(s.content_type),
                           bytes(s.content_id) if k else b"")
            r.zstreams = [zout[int(zoff[b + i]):int(zoff[b + i] + zlen[b + i])] for i in range(k)]
            if status is not None:  # written when the file was read, before its batch was reported
                r.errno = int(status[f])
            if fresh is not None:
                r.fresh = fresh[b:b + k].astype(bool)
            return r

        t0 = time.perf_counter()
        if status is not None:  # the same with per-file outcomes (hbx_store_paths_status)
            zargs_st = zargs[:9] + (_p(status),) + zargs[9:]
        if dedup is not None:
            zargs_st = zargs[:9] + (dd_status,) + zargs[9:]
        if on_batch is None and on_files is None:
            if dedup is not None:
                self._check(self._L.hbx_store_paths_dd(*zargs_st, None, None, *dd_tail), "hbx_store_paths_dd")
            elif status is None:
                self._check(self._L.hbx_store_paths_z(*zargs), "hbx_store_paths_z")
            else:
                self._check(self._L.hbx_store_paths_status(*zargs_st, None, None), "hbx_store_paths_status")
        else:
            raised = []

            def ready(_user, first, count):
                if raised:
                    return
                try:
                    if on_batch is not None:
                        on_batch(int(first), int(count))
                    if on_files is not None:
                        on_files(int(first), [view(f) for f in range(int(first), int(first + count))])
                except BaseException as e:  # never unwind through C
                    raised.append(e)
            cb = _lib.BATCH_READY(ready)
            if dedup is not None:
                self._check(self._L.hbx_store_paths_dd(*zargs_st, ctypes.cast(cb, ctypes.c_void_p), None, *dd_tail),
                            "hbx_store_paths_dd")
            elif status is None:
                self._check(self._L.hbx_store_paths_zcb(*zargs, ctypes.cast(cb, ctypes.c_void_p), None),
                            "hbx_store_paths_zcb")
            else:
                self._check(self._L.hbx_store_paths_status(*zargs_st, ctypes.cast(cb, ctypes.c_void_p), None),
                            "hbx_store_paths_status")
            if raised:
                raise raised[0]
        self.last_call_s = time.perf_counter() - t0
        res = with_status(self._unpack(lens, caps, base, cuts, ids, sums, fresh))
        for f, r in enumerate(res):
            b = int(base[f])
            r.zstreams = [zout[int(zoff[b + i]):int(zoff[b + i] + zlen[b + i])]  # views, no copy
                          for i in range(r.n_chunks)]
        return res

    def host_call_max(self, reset: bool = False) -> np.ndarray:
        """hbx_host_call_max: ms of the slowest single H2D copy call and the
        slowest single submit since the last reset."""
        a = (ctypes.c_double * 2)()
        self._check(self._L.hbx_host_call_max(self._ctx, a, int(reset)), "hbx_host_call_max")
        return np.array(list(a))

    def io_times(self, reset: bool = False) -> np.ndarray:
        """store_paths host seconds: reading files, waiting for batches to be
        collected (arena reuse and the final drain), waiting for a pinned
        slot's copy (cumulative)."""
        s = (ctypes.c_double * 3)()
        self._check(self._L.hbx_io_times(self._ctx, s, int(bool(reset))), "hbx_io_times")
        return np.array(list(s), np.float64)

    def store_file(self, path: Union[str, os.PathLike], segment_bytes: Optional[int] = None,
                   io_threads: int = 16, compress: bool = False, dedup: Optional[IdSet] = None,
                   on_segment: Optional[Callable[["SegmentChunks"], None]] = None) -> FileChunks:
        """storeFile(path) for a regular file on disk (store.go:84-199).  With
        ``segment_bytes`` the file streams through the pipeline in segments of
        that size (hbx_store_file_seg): host and device memory then depend on
        the segment size only, so a file may be larger than device memory.

        ``compress``, ``dedup`` and ``on_segment`` (any of them needs
        ``segment_bytes``) make it the sender's path (hbx_store_file_stream):
        with ``dedup`` every chunk is marked against that set in the segment
        that completes it (``FileChunks.fresh``), with ``compress`` every fresh
        chunk (every chunk without a set) is zlib-compressed on the device, and
        ``on_segment(seg)`` runs once per segment, in order, as soon as that
        segment's chunks are ready, while later segments are still read and
        hashed.  ``seg`` is a :class:`SegmentChunks`; the arrays of its
        ``chunks`` (cut ends, ids, ``fresh``, ``zstreams``) are views into the
        engine's buffers, valid only during the callback.  It must not call
        this engine.  An exception raised in it stops the call (no later
        segment is handed over), puts the set back to its count on entry and
        is re-raised here.
        With ``on_segment`` the returned FileChunks carries cut ends, ids,
        ``fresh`` and the content id, and ``zstreams`` is None: memory stays
        bounded by the segment size (plus 25 bytes per chunk).  Without it the
        binding copies every segment's results, and the returned FileChunks
        has ``fresh`` and ``zstreams`` for the whole file: convenient, but NOT
        memory-bounded (the compressed file is held in host memory)."""
        if compress or dedup is not None or on_segment is not None:
            if segment_bytes is None:
                raise ValueError("compress / dedup / on_segment need segment_bytes (hbx_store_file_stream)")
            return self._store_file_stream(path, int(segment_bytes), int(io_threads), bool(compress), dedup,
                                           on_segment)
        if segment_bytes is None:
            with open(path, "rb") as fh:
                data = np.fromfile(fh, dtype=np.uint8)
            return self.chunk_hash(data)
        n = os.stat(path).st_size
        cap = max_chunks(n)
        cuts = np.zeros(cap, np.uint64)
        ids = np.zeros((cap, 16), np.uint8)
        s = _lib.FileSummary()
        self._check(self._L.hbx_store_file_seg(self._ctx, os.fsencode(path), n, int(segment_bytes), int(io_threads),
                                               _p(cuts), _p(ids), cap, ctypes.byref(s)), "hbx_store_file_seg")
        k = int(s.n_chunks)
        return FileChunks(cuts[:k], ids[:k], int(s.content_type), bytes(s.content_id) if k else b"")

    def _store_file_stream(self, path, segment_bytes: int, io_threads: int, compress: bool,
                           dedup: Optional[IdSet], on_segment) -> FileChunks:
        n = os.stat(path).st_size
        cuts_l, ids_l, fresh_l, z_l = [], [], [], []
        raised = []

        def at(ptr, nbytes: int) -> np.ndarray:  # the bytes at a C pointer, not copied
            if not ptr or nbytes == 0:
                return np.zeros(0, np.uint8)
            return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(ptr), np.uint8)

        def sink(_user, p):
            if raised:
                return 1
            try:
                s = p.contents
                k = int(s.n_chunks)
                cuts = at(s.cut_ends, 8 * k).view(np.uint64)
                ids = at(s.ids, 16 * k).reshape(-1, 16)
                fresh = at(s.fresh, k).astype(bool) if dedup is not None else None
                zs = None
                if compress:
                    zoff = at(s.zoff, 8 * k).view(np.uint64).tolist()
                    zlen = at(s.zlen, 8 * k).view(np.uint64).tolist()
                    zv = at(s.z, max((o + ln for o, ln in zip(zoff, zlen)), default=0))
                    zs = [zv[o:o + ln] for o, ln in zip(zoff, zlen)]
                final = bool(s.final)
                cuts_l.append(cuts.copy())
                ids_l.append(ids.copy())
                if fresh is not None:
                    fresh_l.append(fresh)
                if on_segment is None:
                    if zs is not None:
                        z_l.extend(z.copy() for z in zs)
                    return 0
                ctype = int(s.summary.content_type) if final else 0
                cid = bytes(s.summary.content_id) if final and int(s.summary.n_chunks) else b""
                on_segment(SegmentChunks(int(s.first_chunk), FileChunks(cuts, ids, ctype, cid, zs, 0, fresh), final))
                return 0
            except BaseException as e:  # never unwind through C: a non-zero return, re-raised below
                raised.append(e)
                return 1

        cb = _lib.SEG_SINK(sink)
        s = _lib.FileSummary()
        t0 = time.perf_counter()
        rc = self._L.hbx_store_file_stream(self._ctx, os.fsencode(path), n, segment_bytes, io_threads,
                                           _lib.STREAM_COMPRESS if compress else 0,
                                           dedup._h if dedup is not None else None,
                                           ctypes.cast(cb, ctypes.c_void_p), None, ctypes.byref(s))
        self.last_call_s = time.perf_counter() - t0
        if raised:
            raise raised[0]
        self._check(rc, "hbx_store_file_stream")
        k = int(s.n_chunks)
        res = FileChunks(np.concatenate(cuts_l) if cuts_l else np.zeros(0, np.uint64),
                         np.concatenate(ids_l) if ids_l else np.zeros((0, 16), np.uint8),
                         int(s.content_type), bytes(s.content_id) if k else b"")
        if dedup is not None:
            res.fresh = np.concatenate(fresh_l) if fresh_l else np.zeros(0, bool)
        if compress and on_segment is None:
            res.zstreams = z_l
        return res

    # ---------------------------------------------------- segmented files --
    @staticmethod
    def seg_next(file_len: int, segment_bytes: int, prev_end: int = 0):
        """hbx_seg_next: (offset, length) of the segment after the one that
        ended at ``prev_end`` (0: the first).  Segments overlap by
        SEG_OVERLAP bytes; the one with offset + length == file_len is final.
        Raises ValueError for a bad segment size or when nothing is left."""
        off, ln = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = _lib.load().hbx_seg_next(int(file_len), int(segment_bytes), int(prev_end), ctypes.byref(off),
                                      ctypes.byref(ln))
        if rc != 0:
            raise ValueError(f"hbx_seg_next({file_len}, {segment_bytes}, {prev_end}): {_lib.ERRORS.get(rc, rc)}")
        return int(off.value), int(ln.value)

    def seg_open(self, file_len: int) -> SegmentedFile:
        """Open a file of ``file_len`` bytes for segmented submission."""
        h = ctypes.c_void_p()
        self._check(self._L.hbx_seg_open(self._ctx, int(file_len), ctypes.byref(h)), "hbx_seg_open")
        return SegmentedFile(self, h.value, file_len)

    def seg_submit_device(self, files: Sequence[SegmentedFile], d_arena: int, arena_offs: Sequence[int],
                          seg_lens: Sequence[int], seg_offs: Optional[Sequence[int]] = None,
                          dedup: Optional[IdSet] = None):
        """Enqueue one batch holding the next segment of each of ``files``
        (distinct open files), resident at ``d_arena + arena_offs[i]``
        (hbx_seg_submit_device).  ``seg_offs`` (optional) are the file offsets
        the caller filled the arenas from; they are checked against what each
        handle expects (ValueError).  :meth:`wait` returns one FileChunks per
        segment: absolute cut ends, this segment's chunks, content type 0 for
        a non-final segment and the whole file's type and id for the final.
        With ``dedup`` (hbx_seg_submit_device_dd) the chunks each segment
        completes are marked against that set, in one submit order with
        ``submit_device(dedup=...)`` batches, and :meth:`wait` fills
        ``FileChunks.fresh`` per segment."""
        self._after_producer()
        offs = np.ascontiguousarray(arena_offs, np.uint64)
        lens = np.ascontiguousarray(seg_lens, np.uint64)
        if not (len(files) == offs.size == lens.size):
            raise ValueError("one arena offset and one length per file")
        if seg_offs is not None:
            for f, o in zip(files, seg_offs):
                want = f.end - SEG_OVERLAP if f.end else 0
                if int(o) != want:
                    raise ValueError(f"segment offset {int(o)}: the file's next segment starts at {want}")
        caps, base, cuts, ids, sums = self._alloc_out(lens)
        hs = (ctypes.c_void_p * max(len(files), 1))(*[f._h for f in files])
        keep = (offs, hs)
        if dedup is not None:
            fresh = np.zeros(cuts.shape[0], np.uint8)
            keep = (offs, hs, fresh)
            self._check(self._L.hbx_seg_submit_device_dd(
                self._ctx, len(files), hs, ctypes.c_void_p(int(d_arena)), _p(offs), _p(lens), _p(cuts), _p(ids),
                _p(base), _p(caps), sums, dedup._h, _p(fresh)), "hbx_seg_submit_device_dd")
        else:
            self._check(self._L.hbx_seg_submit_device(self._ctx, len(files), hs, ctypes.c_void_p(int(d_arena)),
                                                      _p(offs), _p(lens), _p(cuts), _p(ids), _p(base), _p(caps),
                                                      sums), "hbx_seg_submit_device")
        for f, ln in zip(files, lens.tolist()):
            f.end = (f.end - SEG_OVERLAP if f.end else 0) + int(ln)
            f.final_sent = f.end == f.file_len
        self._pending.append(("seg", lens, caps, base, cuts, ids, sums, keep))

    def chunk_hash_segmented(self, data: BytesLike, segment_bytes: int, return_segments: bool = False):
        """storeFile over one in-memory file, streamed through a ring of three
        device arenas of ``segment_bytes`` in overlapping segments: the result
        of :meth:`chunk_hash` for a file of any size.  With
        ``return_segments`` also the number of chunks each segment completed."""
        a = _u8(data)
        n = int(a.size)
        if self._pending:
            raise HbxError("chunk_hash_segmented: batches are pending")
        self.seg_next(n, segment_bytes, 0)  # a bad segment size raises before anything is allocated
        arenas, parts = [], []
        f = self.seg_open(n)
        try:
            for _ in range(3):
                d = ctypes.c_void_p()
                self._check(self._L.hbx_arena_alloc(self._ctx, min(int(segment_bytes), n) + 1, ctypes.byref(d)),
                            "hbx_arena_alloc")
                arenas.append(d)
            k = 0
            while not f.final_sent:
                off, ln = f.next(segment_bytes)
                if k >= 3:  # the arena's previous segment must be collected
                    parts += self.wait()
                if ln:
                    self.memcpy_h2d_async(arenas[k % 3].value, a.ctypes.data + off, ln)
                self.seg_submit_device([f], arenas[k % 3].value, [0], [ln], seg_offs=[off])
                k += 1
            while self._pending:
                parts += self.wait()
        finally:
            while self._pending:  # (after a failure: nothing may stay in flight on the arenas)
                try:
                    self.wait()
                except HbxError:
                    self._pending.clear()
            f.close()
            for d in arenas:
                self._L.hbx_arena_free(self._ctx, d)
        last = parts[-1]
        cuts = np.concatenate([p.cut_ends for p in parts]) if parts else np.zeros(0, np.uint64)
        ids = np.concatenate([p.ids for p in parts]) if parts else np.zeros((0, 16), np.uint8)
        res = FileChunks(cuts, ids, last.content_type, last.content_id if cuts.size else b"")
        return (res, [p.n_chunks for p in parts]) if return_segments else res

    def stage_times(self) -> np.ndarray:
        """Device ms of the last collected batch: K1, K2, plan + first K3
        launch, later K3 launches + K4, total (synchronous calls: K3 in [2],
        K4 in [3])."""
        ms = (ctypes.c_float * 5)()
        self._check(self._L.hbx_stage_times(self._ctx, ms), "hbx_stage_times")
        return np.array(list(ms), np.float64)


_PLAN_KEYS = ("resident", "md5_slice", "join_lag", "lead", "k3_period", "launches_per_batch", "hbm_bytes")


def plan_pipeline(n_files: int, arena_bytes: int, longest_file: int, free_bytes: int = 0, hbm_frac: float = 0.95,
                  ranks_per_device: int = 1, steps: int = 0, arenas: int = 0, md5_slice: int = -1,
                  join_lag: int = 0, lead: int = -1, k3_period: int = 0, host_input: bool = False,
                  engine: Optional["Engine"] = None) -> dict:
    """The pipeline's operating point from the library (hbx_plan_pipeline,
    include/hbxgpu.h): resident batches R, MD5 slice, join lag, lead, K3
    period, launches per batch and the HBM the arenas take.  Pure host
    arithmetic when free_bytes > 0 (no GPU needed); with free_bytes=0 an
    engine must be given (its device's free memory).  Raises ValueError for
    an impossible request."""
    L = _lib.load()
    q = _lib.PlanRequest(n_files=int(n_files), arena_bytes=int(arena_bytes), longest_file=int(longest_file),
                         free_bytes=int(free_bytes), hbm_frac=float(hbm_frac),
                         ranks_per_device=int(ranks_per_device), steps=int(steps), arenas=int(arenas),
                         md5_slice=int(md5_slice), join_lag=int(join_lag), lead=int(lead),
                         k3_period=int(k3_period), flags=_lib.PLAN_HOST_INPUT if host_input else 0)
    p = _lib.PipelinePlan()
    ctx = engine._ctx if engine is not None else None
    rc = L.hbx_plan_pipeline(ctx, ctypes.byref(q), ctypes.byref(p))
    if rc != 0:
        msg = L.hbx_last_error(ctx).decode()
        raise ValueError(f"hbx_plan_pipeline: {_lib.ERRORS.get(rc, rc)}: {msg}")
    return {k: int(getattr(p, k)) for k in _PLAN_KEYS}


def device_count() -> int:
    L = _lib.load()
    n = ctypes.c_int(0)
    L.hbx_device_count(ctypes.byref(n))
    return int(n.value)


def pack_arena_layout(lens: Sequence[int], align: int = 256):
    """Offsets for packing files into one device arena (16-B aligned, with
    slack after the last file).  Returns (offsets, total_bytes_to_allocate)."""
    offs = np.zeros(len(lens), np.uint64)
    pos = 0
    for i, n in enumerate(lens):
        offs[i] = pos
        pos += (int(n) + align - 1) // align * align
    return offs, pos + max(ARENA_SLACK, align)
