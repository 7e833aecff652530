"""Hashback's per-file and per-directory block formats on
libhbxgpu, plus the tree store that ties them to the chunking engine.

Reference (fredli74/hashbox):

* ``FileEntry``, ``FileChainBlock``, ``DirectoryBlock`` and their
  ``Serialize``/``Unserialize`` — hashback/hashback.go:80-214;
* ``storeDir`` (directory block + links + id) — hashback/store.go:201-234;
* ``storePath`` (what becomes which entry type) — hashback/store.go:254-397;
* ``entryFromFileInfo`` — hashback/store.go:243-251;
* ``restoreEntry`` / ``restoreDir`` (the way back) — hashback/restore.go:68-162.

Serialization runs in the library's C++ (``hbx_file_entry_*``,
``hbx_chain_block_*``, ``hbx_directory_block_*``); directory block ids are
hashed on the device in one batch per tree level (``hbx_directory_block_ids``,
kernel K6).  Errors raise :class:`HbxError`, like the reference's panics
("corrupted FileEntry" etc.).
"""
from __future__ import annotations

import ctypes
import os
import stat
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .engine import Engine, FileChunks, HbxError, RestoreError

TYPE_EMPTY, TYPE_DIRECTORY, TYPE_FILE_DATA, TYPE_FILE_CHAIN, TYPE_SYMLINK = 0, 1, 2, 3, 4  # hashback.go:93-99

# Go io/fs FileMode bits (the FileMode that entryFromFileInfo stores)
MODE_DIR, MODE_TEMPORARY, MODE_SYMLINK, MODE_DEVICE = 1 << 31, 1 << 28, 1 << 27, 1 << 26
MODE_NAMED_PIPE, MODE_SOCKET, MODE_SETUID, MODE_SETGID = 1 << 25, 1 << 24, 1 << 23, 1 << 22
MODE_CHAR_DEVICE, MODE_STICKY = 1 << 21, 1 << 20

_ZERO16 = bytes(16)


@dataclass
class FileEntry:
    """hashback FileEntry (hashback.go:80-90), same fields."""
    file_name: bytes
    file_size: int = 0
    file_mode: int = 0
    mod_time: int = 0
    reference_id: bytes = _ZERO16
    content_type: int = TYPE_EMPTY
    content_block_id: bytes = _ZERO16
    decrypt_key: bytes = _ZERO16
    file_link: bytes = b""

    def has_content_block_id(self) -> bool:  # hashback.go:100-102
        return self.content_type in (TYPE_DIRECTORY, TYPE_FILE_DATA, TYPE_FILE_CHAIN)


def go_file_mode(st_mode: int) -> int:
    """os.FileMode of a Linux st_mode (what Go's Lstat reports)."""
    m = st_mode & 0o777
    fmt = stat.S_IFMT(st_mode)
    m |= {stat.S_IFBLK: MODE_DEVICE, stat.S_IFCHR: MODE_DEVICE | MODE_CHAR_DEVICE, stat.S_IFDIR: MODE_DIR,
          stat.S_IFIFO: MODE_NAMED_PIPE, stat.S_IFLNK: MODE_SYMLINK, stat.S_IFSOCK: MODE_SOCKET}.get(fmt, 0)
    if st_mode & stat.S_ISGID:
        m |= MODE_SETGID
    if st_mode & stat.S_ISUID:
        m |= MODE_SETUID
    if st_mode & stat.S_ISVTX:
        m |= MODE_STICKY
    return m


def entry_from_stat(name: bytes, st: os.stat_result, reference_id: bytes = _ZERO16) -> FileEntry:
    """entryFromFileInfo (store.go:243-251)."""
    return FileEntry(file_name=name, file_size=st.st_size, file_mode=go_file_mode(st.st_mode),
                     mod_time=st.st_mtime_ns, reference_id=reference_id)


def _check(rc: int, what: str):
    if rc != 0:
        raise HbxError(f"{what}: {_lib.ERRORS.get(rc, rc)}")


_ENTRY_DTYPE = np.dtype({"names": ["name", "name_len", "file_mode", "file_size", "mod_time", "reference_id",
                                    "content_id", "decrypt_key", "link", "link_len", "content_type"],
                          "formats": ["<u8", "<u4", "<u4", "<i8", "<i8", ("u1", 16), ("u1", 16), ("u1", 16),
                                      "<u8", "<u4", "u1"],
                          "offsets": [0, 8, 12, 16, 24, 32, 48, 64, 80, 88, 92], "itemsize": 96})


def _c_entries(entries: Sequence[FileEntry]):
    """hbx_file_entry[] for many entries, built column-wise (names and links
    in one byte pool).  Returns (ctypes array view, keepalive)."""
    n = len(entries)
    rec = np.zeros(max(n, 1), _ENTRY_DTYPE)
    if n:
        names = [bytes(e.file_name) for e in entries]
        links = [bytes(e.file_link) for e in entries]
        nl = np.fromiter((len(x) for x in names), np.uint64, n)
        ll = np.fromiter((len(x) for x in links), np.uint64, n)
        pool = np.frombuffer(b"".join(names) + b"".join(links) + b"\0", np.uint8)
        base = pool.ctypes.data
        noff = np.zeros(n, np.uint64)
        noff[1:] = np.cumsum(nl[:-1])
        loff = np.zeros(n, np.uint64)
        loff[1:] = np.cumsum(ll[:-1])
        loff += np.uint64(nl.sum())
        rec["name"] = np.uint64(base) + noff
        rec["name_len"] = nl
        rec["link"] = np.uint64(base) + loff
        rec["link_len"] = ll
        rec["file_mode"] = np.fromiter((int(e.file_mode) & 0xFFFFFFFF for e in entries), np.uint32, n)
        rec["file_size"] = np.fromiter((int(e.file_size) for e in entries), np.int64, n)
        rec["mod_time"] = np.fromiter((int(e.mod_time) for e in entries), np.int64, n)
        rec["content_type"] = np.fromiter((int(e.content_type) for e in entries), np.uint8, n)
        for col, attr in (("reference_id", "reference_id"), ("content_id", "content_block_id"),
                          ("decrypt_key", "decrypt_key")):
            rec[col] = np.frombuffer(b"".join(bytes(getattr(e, attr)) for e in entries), np.uint8).reshape(n, 16)
    else:
        pool = np.zeros(1, np.uint8)
    arr = (_lib.FileEntry * max(n, 1)).from_address(rec.ctypes.data)
    return arr, (rec, pool)


def _entry_ptr(arr, i: int) -> ctypes.c_void_p:
    return ctypes.c_void_p(ctypes.addressof(arr) + 96 * i)


def _py_entry(c) -> FileEntry:
    return FileEntry(file_name=ctypes.string_at(c.name, c.name_len) if c.name_len else b"",
                     file_size=c.file_size, file_mode=c.file_mode, mod_time=c.mod_time,
                     reference_id=bytes(c.reference_id), content_type=c.content_type,
                     content_block_id=bytes(c.content_id), decrypt_key=bytes(c.decrypt_key),
                     file_link=ctypes.string_at(c.link, c.link_len) if c.link_len else b"")


def serialize_entry(e: FileEntry) -> bytes:
    """FileEntry.Serialize (hashback.go:113-132)."""
    L = _lib.load()
    arr, _keep = _c_entries([e])
    n = L.hbx_file_entry_size(ctypes.byref(arr[0]))
    out = ctypes.create_string_buffer(max(n, 1))
    used = ctypes.c_uint64()
    _check(L.hbx_file_entry_serialize(ctypes.byref(arr[0]), out, n, ctypes.byref(used)), "hbx_file_entry_serialize")
    return out.raw[:used.value]


def parse_entry(buf: bytes) -> Tuple[FileEntry, int]:
    """FileEntry.Unserialize (hashback.go:133-155): (entry, bytes used)."""
    L = _lib.load()
    src = ctypes.create_string_buffer(bytes(buf), max(len(buf), 1))
    c = _lib.FileEntry()
    used = ctypes.c_uint64()
    _check(L.hbx_file_entry_parse(src, len(buf), ctypes.byref(c), ctypes.byref(used)), "corrupted FileEntry")
    return _py_entry(c), used.value


def serialize_chain_block(ids: Sequence[bytes], keys: Optional[Sequence[bytes]] = None) -> bytes:
    """FileChainBlock.Serialize (hashback.go:162-170); keys default to zero."""
    L = _lib.load()
    k = len(ids)
    idb = b"".join(bytes(i) for i in ids) or _ZERO16
    keyb = b"".join(bytes(x) for x in keys) if keys is not None else None
    out = ctypes.create_string_buffer(8 + 32 * k)
    used = ctypes.c_uint64()
    _check(L.hbx_chain_block_serialize(idb, keyb, k, out, 8 + 32 * k, ctypes.byref(used)),
           "hbx_chain_block_serialize")
    return out.raw[:used.value]


def parse_chain_block(buf: bytes) -> Tuple[List[bytes], List[bytes]]:
    """FileChainBlock.Unserialize (hashback.go:171-185): (ids, keys)."""
    L = _lib.load()
    src = ctypes.create_string_buffer(bytes(buf), max(len(buf), 1))
    k = ctypes.c_uint32()
    _check(L.hbx_chain_block_parse(src, len(buf), ctypes.byref(k), None, None, 0), "corrupted FileChainBlock")
    ids = ctypes.create_string_buffer(16 * max(k.value, 1))
    keys = ctypes.create_string_buffer(16 * max(k.value, 1))
    _check(L.hbx_chain_block_parse(src, len(buf), ctypes.byref(k), ids, keys, k.value), "corrupted FileChainBlock")
    return ([ids.raw[16 * i:16 * i + 16] for i in range(k.value)],
            [keys.raw[16 * i:16 * i + 16] for i in range(k.value)])


def serialize_directory_block(entries: Sequence[FileEntry]) -> Tuple[bytes, List[bytes]]:
    """DirectoryBlock.Serialize (hashback.go:192-199) + storeDir's links
    (store.go:221-228)."""
    L = _lib.load()
    arr, _keep = _c_entries(entries)
    n = len(entries)
    size = L.hbx_directory_block_size(arr, n)
    out = ctypes.create_string_buffer(max(size, 1))
    links = ctypes.create_string_buffer(16 * max(n, 1))
    used, nl = ctypes.c_uint64(), ctypes.c_uint32()
    _check(L.hbx_directory_block_serialize(arr, n, out, size, ctypes.byref(used), links, ctypes.byref(nl)),
           "hbx_directory_block_serialize")
    return out.raw[:used.value], [links.raw[16 * i:16 * i + 16] for i in range(nl.value)]


def parse_directory_block(buf: bytes) -> List[FileEntry]:
    """DirectoryBlock.Unserialize (hashback.go:200-214)."""
    L = _lib.load()
    src = ctypes.create_string_buffer(bytes(buf), max(len(buf), 1))
    n = ctypes.c_uint32()
    _check(L.hbx_directory_block_parse(src, len(buf), None, 0, ctypes.byref(n)), "corrupted DirectoryBlock")
    arr = (_lib.FileEntry * max(n.value, 1))()
    _check(L.hbx_directory_block_parse(src, len(buf), arr, n.value, ctypes.byref(n)), "corrupted DirectoryBlock")
    return [_py_entry(arr[i]) for i in range(n.value)]


def directory_block_ids(eng: Engine, dirs: Sequence[Sequence[FileEntry]], with_blocks: bool = False):
    """storeDir's block id (store.go:230-231) for many directories at once, on
    the device (one K6 launch).  With ``with_blocks`` also returns each
    directory's (dblk bytes, links)."""
    L = _lib.load()
    flat = [e for d in dirs for e in d]
    arr, _keep = _c_entries(flat)
    counts = np.array([len(d) for d in dirs], np.uint32)
    base = np.zeros(len(dirs), np.uint64)
    if len(dirs) > 1:
        base[1:] = np.cumsum(counts[:-1], dtype=np.uint64)
    ids = np.zeros((max(len(dirs), 1), 16), np.uint8)
    eng._check(eng._L.hbx_directory_block_ids(eng._ctx, len(dirs), arr, base.ctypes.data, counts.ctypes.data,
                                              ids.ctypes.data), "hbx_directory_block_ids")
    out = [bytes(r) for r in ids[:len(dirs)]]
    if not with_blocks:
        return out
    blocks = []
    links = ctypes.create_string_buffer(16 * max(int(counts.max()) if len(dirs) else 1, 1))
    used, nl = ctypes.c_uint64(), ctypes.c_uint32()
    for d in range(len(dirs)):
        p = _entry_ptr(arr, int(base[d]))
        size = L.hbx_directory_block_size(p, int(counts[d]))
        buf = ctypes.create_string_buffer(max(size, 1))
        _check(L.hbx_directory_block_serialize(p, int(counts[d]), buf, size, ctypes.byref(used), links,
                                               ctypes.byref(nl)), "hbx_directory_block_serialize")
        blocks.append((buf.raw[:used.value], [links.raw[16 * i:16 * i + 16] for i in range(nl.value)]))
    return out, blocks


@dataclass
class TreeStore:
    """What one ``store`` of a tree produces (the Go session would send every
    block to the server): the top entry, every directory block and every
    file's chunk list."""
    root: FileEntry
    directories: Dict[bytes, Tuple[bytes, List[bytes], bytes]] = field(default_factory=dict)  # path -> (dblk, links, id)
    files: Dict[bytes, FileChunks] = field(default_factory=dict)  # path -> chunks (FileSize > 0 only)
    skipped: List[bytes] = field(default_factory=list)
    seconds: Dict[str, float] = field(default_factory=dict)  # walk, files, directories


def store_tree(eng: Engine, root, reference_id: bytes = _ZERO16, io_threads: int = 16,
               batch_bytes: int = 1 << 30) -> TreeStore:
    """storePath(root, toplevel=True) for a fresh backup (no reference cache,
    no ignore list): store.go:254-397 + storeDir (201-234) + storeFile (84-199).

    Every regular file with FileSize > 0 goes through ``Engine.store_paths`` in
    one pipelined call; the directory blocks are then hashed on the device
    level by level, deepest first (a parent's entry holds its child's id).
    """
    root = os.fsencode(os.fspath(root))
    st = os.stat(root)  # the top level follows symbolic links (store.go:263-264)
    dirs: Dict[bytes, List[Tuple[bytes, FileEntry]]] = {}
    depth: Dict[bytes, int] = {}
    file_entries: Dict[bytes, FileEntry] = {}
    out = TreeStore(root=entry_from_stat(os.path.basename(root.rstrip(b"/")) or root, st, reference_id))

    def visit(path: bytes, entry: FileEntry, info: os.stat_result, d: int) -> bool:
        m = entry.file_mode
        if m & (MODE_TEMPORARY | MODE_DEVICE | MODE_NAMED_PIPE | MODE_SOCKET):  # store.go:284-296
            out.skipped.append(path)
            return False
        if m & MODE_SYMLINK:  # store.go:297-317
            entry.content_type, entry.file_size = TYPE_SYMLINK, 0
            entry.file_link = os.readlink(path)
        elif m & MODE_DIR:  # store.go:319-334
            entry.content_type, entry.file_size = TYPE_DIRECTORY, 0
            kids = []
            with os.scandir(path) as it:
                names = sorted(e.name for e in it)  # FileInfoSlice sorts by Name() (store.go:217)
            for name in names:
                p = os.path.join(path, name)
                ki = os.lstat(p)
                ke = entry_from_stat(name, ki, reference_id)
                if visit(p, ke, ki, d + 1):
                    kids.append((p, ke))
            dirs[path] = kids
            depth[path] = d
        elif entry.file_size > 0:  # store.go:355-356
            file_entries[path] = entry
        return True

    t0 = time.perf_counter()
    if not visit(root, out.root, st, 0):
        return out
    t1 = time.perf_counter()
    paths = list(file_entries)
    if paths:
        # sizes from the walk's Lstat (FileEntry.FileSize, store.go:247)
        res = eng.store_paths(paths, io_threads=io_threads, batch_bytes=batch_bytes,
                              sizes=[file_entries[p].file_size for p in paths])
        for p, r in zip(paths, res):
            e = file_entries[p]
            e.content_type, e.content_block_id = r.content_type, r.content_id  # store.go:187-196
            out.files[p] = r
    t2 = time.perf_counter()
    by_depth: Dict[int, List[bytes]] = {}
    for p, d in depth.items():
        by_depth.setdefault(d, []).append(p)
    dir_entry = {p: e for kids in dirs.values() for p, e in kids}
    dir_entry[root] = out.root
    for d in sorted(by_depth, reverse=True):
        level = by_depth[d]
        ids, blocks = directory_block_ids(eng, [[e for _, e in dirs[p]] for p in level], with_blocks=True)
        for p, i, (data, links) in zip(level, ids, blocks):
            out.directories[p] = (data, links, i)
            dir_entry[p].content_block_id = i
    out.seconds = {"walk": t1 - t0, "files": t2 - t1, "directories": time.perf_counter() - t2}
    return out


def block_table(checks) -> tuple:
    """The good entries of a store's data files as ONE block table for
    :meth:`Engine.block_graph`: ``checks`` are the :class:`DatFileCheck` results
    of the files in file order (checked with their links).  Returns ``(ids
    uint8 [n, 16], n_links uint32 [n], link_base uint64 [n], links uint8 [m, 16],
    file_no uint32 [n], off uint64 [n])``: each file's ``link_base`` is shifted
    by the links of the files before it, and ``file_no`` / ``off`` say where a
    row's entry lies (what an index entry holds).  With it "check every data
    file, then mark from the roots" is ``check_datfile`` per file, this, and
    ``block_graph``."""
    ids, nl, lb, lk, fno, off = [], [], [], [], [], []
    before = 0
    for f, chk in enumerate(checks):
        if chk.links is None:
            raise ValueError(f"data file {f} was checked without its links")
        e = chk.entries
        ids.append(np.ascontiguousarray(e["id"], np.uint8).reshape(-1, 16))
        nl.append(e["n_links"].astype(np.uint32))
        lb.append(e["link_base"].astype(np.uint64) + np.uint64(before))
        lk.append(np.ascontiguousarray(chk.links, np.uint8).reshape(-1, 16))
        fno.append(np.full(e.shape[0], f, np.uint32))
        off.append(e["off"].astype(np.uint64))
        before += lk[-1].shape[0]

    def cat(parts, dtype, tail=()):
        return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0,) + tail, dtype)
    return (cat(ids, np.uint8, (16,)), cat(nl, np.uint32), cat(lb, np.uint64), cat(lk, np.uint8, (16,)),
            cat(fno, np.uint32), cat(off, np.uint64))


def gc_keep(graph, file_no, force: bool = False) -> list:
    """The sweep's verdict per data file for :meth:`Engine.compact_datfile`:
    ``graph`` is the :class:`BlockGraph` of a :func:`block_table` and
    ``file_no`` that table's fifth array.  Returns one bool array per data
    file (file 0 first; a file without rows gets an empty one), True where the
    row is marked and is its ID's representative: what the roots reach, once
    per ID (``graph.marked & ~graph.alias``).  Raises if a marked tree is
    damaged (``n_marked_faulty``): sweeping then would delete what a repair
    still needs; ``force`` sweeps anyway."""
    if graph.summary["n_marked_faulty"] and not force:
        raise ValueError(f"{graph.summary['n_marked_faulty']} marked blocks have a damaged tree below them: "
                         "repair first, or pass force=True")
    fno = np.asarray(file_no).reshape(-1)
    live = np.asarray(graph.marked) & ~np.asarray(graph.alias)
    if fno.shape[0] != live.shape[0]:
        raise ValueError("one file number per row of the graph")
    n_files = int(fno.max()) + 1 if fno.shape[0] else 0
    return [live[fno == f] for f in range(n_files)]


def gc_sweep(ix, ids, g):
    """A GC run over the index files ``ix`` (:meth:`Engine.open_index`):
    MarkIndexes' writes for the rows the roots reach (``ids[g.marked]``: ``ids``
    is the block table's ID array, ``g`` its :class:`BlockGraph`), then
    SweepIndexes and CompactIndexes (pkg/storagedb/gc.go:24-206), all on the
    device.  Returns the :class:`IndexSweep`; its ``killed`` are the caller's
    killMetaEntry calls.  A marked ID the index does not hold raises, where the
    reference aborts (gc.go:36-37).  Which entries of a data file to keep
    (:meth:`Engine.compact_datfile`'s ``keep``) also needs the meta files and
    is not derived here."""
    a = np.asarray(ids, np.uint8).reshape(-1, 16)
    marked = np.asarray(g.marked)
    if a.shape[0] != marked.shape[0]:
        raise ValueError("one ID per row of the graph")
    found = ix.mark(a[marked])
    if not found.all():
        raise HbxError(f"{int((~found).sum())} marked blocks have no index entry")
    res = ix.sweep()
    ix.compact()
    return res


def _read_verified(eng: Engine, read_block, block_id: bytes, what: str) -> bytes:
    """ReadBlock + VerifyBlock of one directory or chain block: its data,
    inflated and hashed with its links on the device (Engine.restore_blocks)."""
    btype, data, links = read_block(bytes(block_id))
    r = eng.restore_blocks([data], [btype], [block_id], links=[list(links or [])])
    if r.n_good != 1:
        raise HbxError(f"{what} block {bytes(block_id).hex()} corrupted (status {int(r.status[0])})")
    return r.data


def _read_verified_many(eng: Engine, read_block, ids: Sequence[bytes], what: str) -> List[bytes]:
    """ReadBlock + VerifyBlock of many directory or chain blocks in one device
    call (Engine.restore_files_blocks, each block a one-block file with its
    links).  The first bad one raises."""
    if not ids:
        return []
    chains = []
    for bid in ids:
        btype, data, links = read_block(bytes(bid))
        chains.append([(btype, data, bytes(bid), list(links or []))])
    r = eng.restore_files_blocks(chains)
    for k, bid in enumerate(ids):
        if int(r.n_good[k]) != 1:
            raise HbxError(f"{what} block {bytes(bid).hex()} corrupted (status {int(r.status[k][0])})")
    return r.data


def _file_chains(eng: Engine, read_block, entries: Sequence[FileEntry]) -> List[List[bytes]]:
    """The data block IDs of every file entry: its FileChainBlock's list (all
    chain blocks read and verified in one call) or its one ContentBlockID."""
    chained = [k for k, e in enumerate(entries) if e.content_type == TYPE_FILE_CHAIN]
    blocks = _read_verified_many(eng, read_block, [entries[k].content_block_id for k in chained], "chain")
    ids: List[List[bytes]] = [[bytes(e.content_block_id)] if e.content_type == TYPE_FILE_DATA else [] for e in entries]
    for k, blk in zip(chained, blocks):
        ids[k] = [bytes(i) for i in parse_chain_block(blk)[0]]
    return ids


def _create_file(local: bytes, e: FileEntry) -> int:
    """Create or truncate ``local`` with the entry's mode, as OpenFile does
    (restore.go:108: the umask applies); the mode the file has afterwards."""
    fd = os.open(local, os.O_CREAT | os.O_TRUNC | os.O_WRONLY, e.file_mode & 0o777)
    mode = stat.S_IMODE(os.fstat(fd).st_mode)
    os.close(fd)
    return mode


_REUSE_FDS = 32  # pool files kept open at a time while their chunks are read back


def _sibling_temporary(local: bytes, e: FileEntry) -> Tuple[bytes, int]:
    """A fresh file beside ``local``, created with the entry's mode and O_EXCL,
    and the mode it got.  By the time this is called every entry of the
    directory exists on disk, so a name O_EXCL accepts is no entry's."""
    d = os.path.dirname(local)
    while True:
        tmp = os.path.join(d, b".hbx-restore-" + os.urandom(8).hex().encode() + b".tmp")
        try:
            fd = os.open(tmp, os.O_CREAT | os.O_EXCL | os.O_WRONLY, e.file_mode & 0o777)
        except FileExistsError:
            continue
        mode = stat.S_IMODE(os.fstat(fd).st_mode)
        os.close(fd)
        return tmp, mode


class _PoolReader:
    """Chunks of the pool's files read back by (file, offset, length), with a
    bounded number of descriptors open.  None for anything but the whole chunk:
    that block is then fetched."""

    def __init__(self, paths: Sequence[bytes]):
        self.paths = paths
        self.fds: Dict[int, int] = {}  # insertion order = least recently used first

    def read(self, f: int, off: int, n: int) -> Optional[bytes]:
        try:
            fd = self.fds.pop(f, None)
            if fd is None:
                if len(self.fds) >= _REUSE_FDS:
                    os.close(self.fds.pop(next(iter(self.fds))))
                fd = os.open(self.paths[f], os.O_RDONLY)
            self.fds[f] = fd
            data = os.pread(fd, n, off)
        except OSError:
            return None
        return data if len(data) == n else None

    def close(self):
        for fd in self.fds.values():
            os.close(fd)
        self.fds = {}


def _restore_tree_batched(eng: Engine, root_entry: FileEntry, read_block, dest: bytes, window_bytes: int,
                          io_threads: int, keep_matching: bool = False, reuse_local: bool = False,
                          reuse_paths: Sequence = ()) -> Dict[str, int]:
    stats = {"files": 0, "directories": 0, "bytes": 0}
    if keep_matching or reuse_local:
        stats["kept"] = 0
    if reuse_local:
        stats.update(blocks_reused=0, bytes_reused=0, blocks_fetched=0, reuse_retried=0)
    made_dirs: List[Tuple[bytes, int]] = []
    # entry, local path, the mode its creation gave it (None: a keep_matching candidate, not created yet)
    files: List[Tuple[FileEntry, bytes, Optional[int]]] = []
    level: List[Tuple[FileEntry, bytes]] = [(root_entry, dest)]
    while level:  # breadth-first: one device call per level of directory blocks
        want: List[Tuple[FileEntry, bytes]] = []
        for e, path in level:
            local = os.path.join(path, bytes(e.file_name))
            if e.file_mode & MODE_SYMLINK:  # restore.go:76-84
                if e.content_type != TYPE_SYMLINK:
                    raise HbxError(f"invalid ContentType for a symlink ({e.content_type})")
                os.symlink(bytes(e.file_link), local)
            elif e.file_mode & MODE_DIR:  # restore.go:85-102
                os.makedirs(local, 0o777, exist_ok=True)
                if e.content_type == TYPE_DIRECTORY:
                    want.append((e, local))
                elif e.content_type != TYPE_EMPTY:
                    raise HbxError(f"invalid ContentType for a directory ({e.content_type})")
                made_dirs.append((local, e.file_mode & 0o777))
                stats["directories"] += 1
            else:  # restore.go:103-145
                if e.content_type not in (TYPE_FILE_CHAIN, TYPE_FILE_DATA, TYPE_EMPTY):
                    raise HbxError(f"invalid ContentType for a file ({e.content_type})")
                # keep_matching: a regular file of the entry's size already there is neither created nor
                # truncated until its block IDs have been compared with its chain
                # (reuse_local: of any size, and it stays as it is until its replacement is complete)
                candidate = False
                if (keep_matching or reuse_local) and int(e.file_size) > 0 and e.content_type != TYPE_EMPTY:
                    try:
                        st = os.lstat(local)
                        candidate = stat.S_ISREG(st.st_mode) and (reuse_local or st.st_size == int(e.file_size))
                    except OSError:
                        pass
                files.append((e, local, None if candidate else _create_file(local, e)))
        blocks = _read_verified_many(eng, read_block, [e.content_block_id for e, _ in want], "directory")
        level = [(kid, local) for (_, local), blk in zip(want, blocks) for kid in parse_directory_block(blk)]
    ids = _file_chains(eng, read_block, [e for e, _, _ in files])
    if reuse_local:
        _restore_reusing(eng, read_block, files, ids, stats, window_bytes, io_threads, reuse_paths)
        return _finish_tree(files, made_dirs, stats)
    kept = set()
    cand = [k for k in range(len(files)) if files[k][2] is None]
    if cand:
        # the local files cut and hashed at the store path's speed: one whose block IDs are its chain's is
        # already right, and none of its data blocks is read
        ms = eng.match_paths([files[k][1] for k in cand], [ids[k] for k in cand], io_threads=io_threads,
                             sizes=[int(files[k][0].file_size) for k in cand], skip_unreadable=True)
        umask = os.umask(0)
        os.umask(umask)
        for k, m in zip(cand, ms):
            e, local, _ = files[k]
            if m.same and not m.errno:
                kept.add(k)
                os.chmod(local, e.file_mode & 0o777 & ~umask)  # what creating it would have given it
            else:
                files[k] = (e, local, _create_file(local, e))
        stats["kept"] = len(kept)
    with_data = [k for k in range(len(files)) if ids[k] and k not in kept]
    # (a mode without the owner's write bit, 0444: writable while written, as in the unbatched path)
    locked = [k for k in with_data if not files[k][2] & stat.S_IWUSR]
    for k in locked:
        os.chmod(files[k][1], files[k][2] | stat.S_IWUSR)
    try:
        res = eng.restore_files([ids[k] for k in with_data], lambda f, i: read_block(ids[with_data[f]][i])[:2],
                                [files[k][1] for k in with_data],
                                size_hints=[max(int(files[k][0].file_size), 0) for k in with_data],
                                window_bytes=window_bytes, io_threads=io_threads) if with_data else []
    finally:
        for k in locked:
            os.chmod(files[k][1], files[k][2])
    for k, r in zip(with_data, res):
        if r.bad_index is not None:
            raise HbxError(f"block {ids[k][r.bad_index].hex()} (block {r.bad_index} of {os.fsdecode(files[k][1])}) "
                           f"corrupted (status {r.bad_status})")
        if r.errno:
            raise HbxError(f"cannot write {os.fsdecode(files[k][1])}: {os.strerror(r.errno)}")
        stats["bytes"] += r.bytes
    return _finish_tree(files, made_dirs, stats)


def _finish_tree(files, made_dirs, stats) -> Dict[str, int]:
    now = time.time_ns()
    for e, local, _ in files:
        os.utime(local, ns=(now, int(e.mod_time)))
        stats["files"] += 1
    for local, mode in reversed(made_dirs):  # after its content (restore.go:99), children before parents
        os.chmod(local, mode)
    return stats


def _restore_reusing(eng: Engine, read_block, files, ids, stats, window_bytes: int, io_threads: int,
                     reuse_paths: Sequence):
    """The data of ``files`` (entry, local path, mode or None for a regular
    file that was there before the walk and has not been touched) with every
    block that some local file already holds taken from that file."""
    cand = [k for k in range(len(files)) if files[k][2] is None]
    # the pool: the files that were there, and what the caller adds (read only)
    pool_paths = [files[k][1] for k in cand]
    pool_sizes = []
    for p in list(pool_paths):
        try:
            pool_sizes.append(os.lstat(p).st_size)
        except OSError:
            pool_sizes.append(0)  # (gone since the walk: unreadable below)
    seen = set(pool_paths)
    for p in reuse_paths:
        p = os.fsencode(os.fspath(p))
        try:
            st = os.stat(p)
        except OSError:
            continue
        if stat.S_ISREG(st.st_mode) and p not in seen:
            seen.add(p)
            pool_paths.append(p)
            pool_sizes.append(st.st_size)
    kept = set()
    src_paths: List[bytes] = []
    src_ids, src_cuts = [], []
    if pool_paths:
        # cut and hashed at the store path's speed: a candidate whose block IDs are its chain's is already
        # right (keep_matching); every readable file's chunks are where wanted blocks may be found
        ms = eng.match_paths(pool_paths, [ids[k] for k in cand] + [[]] * (len(pool_paths) - len(cand)),
                             io_threads=io_threads, sizes=pool_sizes, skip_unreadable=True, chunks=True)
        umask = os.umask(0)
        os.umask(umask)
        for n, m in enumerate(ms):
            if n < len(cand) and m.same and not m.errno:
                e, local, _ = files[cand[n]]
                kept.add(cand[n])
                os.chmod(local, e.file_mode & 0o777 & ~umask)  # what creating it would have given it
            if not m.errno and m.chunks is not None and m.chunks.n_chunks:
                src_paths.append(pool_paths[n])
                src_ids.append(m.chunks.ids)
                src_cuts.append(m.chunks.cut_ends)
    stats["kept"] = len(kept)
    for k in cand:  # (a chain without blocks: nothing to reuse, created empty as ever)
        if k not in kept and not ids[k]:
            files[k] = (files[k][0], files[k][1], _create_file(files[k][1], files[k][0]))
    with_data = [k for k in range(len(files)) if ids[k] and k not in kept]
    if not with_data:
        return
    first = np.zeros(len(with_data) + 1, np.int64)
    first[1:] = np.cumsum([len(ids[k]) for k in with_data])
    loc = eng.locate_ids(src_ids, src_cuts, [i for k in with_data for i in ids[k]])
    loc_file, loc_off, loc_len = loc["file"].tolist(), loc["off"].tolist(), loc["len"].tolist()
    pool = _PoolReader(src_paths)
    temps: Dict[int, bytes] = {}  # a file that was there is written beside itself and renamed when it is good
    try:
        out_paths = []
        for k in with_data:
            e, local, mode = files[k]
            if mode is None:
                temps[k], mode = _sibling_temporary(local, e)
                files[k] = (e, local, mode)
            out_paths.append(temps.get(k, local))
        # (a mode without the owner's write bit, 0444: writable while written, as in the unbatched path)
        locked = [n for n, k in enumerate(with_data) if not files[k][2] & stat.S_IWUSR]
        for n in locked:
            os.chmod(out_paths[n], files[with_data[n]][2] | stat.S_IWUSR)
        hints = [max(int(files[k][0].file_size), 0) for k in with_data]

        def run(sel: List[int], reuse: bool):
            """restore_files over with_data[n] for n in sel; per file the indices of its reused blocks."""
            reused: List[Dict[int, int]] = [{} for _ in sel]

            def source(f: int, i: int):
                n = sel[f]
                j = int(first[n]) + i
                if reuse and loc_file[j] != _lib.NO_FILE:
                    data = pool.read(loc_file[j], loc_off[j], loc_len[j])
                    if data is not None:
                        reused[f][i] = len(data)
                        return _lib.BLOCK_RAW, data
                stats["blocks_fetched"] += 1
                return read_block(ids[with_data[n]][i])[:2]

            res = eng.restore_files([ids[with_data[n]] for n in sel], source, [out_paths[n] for n in sel],
                                    size_hints=[hints[n] for n in sel], window_bytes=window_bytes,
                                    io_threads=io_threads)
            return res, reused

        def check(n: int, r):
            k = with_data[n]
            if r.bad_index is not None:
                raise HbxError(f"block {ids[k][r.bad_index].hex()} (block {r.bad_index} of "
                               f"{os.fsdecode(files[k][1])}) corrupted (status {r.bad_status})")
            if r.errno:
                raise HbxError(f"cannot write {os.fsdecode(files[k][1])}: {os.strerror(r.errno)}")
            stats["bytes"] += r.bytes

        try:
            everything = list(range(len(with_data)))
            res, reused = run(everything, True)
            again = []
            for n, r, u in zip(everything, res, reused):
                if r.bad_index is not None and r.bad_index in u:
                    again.append(n)  # the local file changed after it was hashed: a reuse is never trusted
                    continue
                check(n, r)
                stats["blocks_reused"] += len(u)
                stats["bytes_reused"] += sum(u.values())
            if again:
                stats["reuse_retried"] += len(again)
                res, _ = run(again, False)  # once more, every block fetched
                for n, r in zip(again, res):
                    check(n, r)
        finally:
            for n in locked:
                try:
                    os.chmod(out_paths[n], files[with_data[n]][2])
                except OSError:
                    pass
        for k in list(temps):
            os.replace(temps[k], files[k][1])
            del temps[k]
    finally:
        pool.close()
        for tmp in temps.values():  # a failure: the old files stay as they were
            try:
                os.unlink(tmp)
            except OSError:
                pass


def restore_tree(eng: Engine, root_entry: FileEntry, read_block, dest, window_bytes: int = 0,
                 batch: bool = False, io_threads: int = 16, keep_matching: bool = False,
                 reuse_local: bool = False, reuse_paths: Sequence = ()) -> Dict[str, int]:
    """restoreEntry(root_entry, dest) (hashback/restore.go:68-162): the
    counterpart of :func:`store_tree`.  ``read_block(id)`` returns a block as
    it comes off the wire: ``(data type, data field, links)``.

    With ``batch=True`` the tree is read breadth-first with a few device calls
    instead of one round trip per block and per file: every directory block of
    a level in one ``Engine.restore_files_blocks`` call, every chain block of
    the tree's files in one more, and all file data through one
    ``Engine.restore_files`` with the entries' FileSize as size hints.  Modes,
    read-only files, symbolic links, empty files, ModTime and the directories'
    chmod after their content are as below.  The difference: the unbatched
    path stops at the first bad block in depth-first order and has written
    nothing after it; the batched path raises :class:`HbxError` for the first
    bad block in ITS order (directory blocks level by level, then chain blocks,
    then data blocks in the order the files were met), and the good files of
    the same batch have been written by then (without their ModTime).

    ``keep_matching=True`` (with ``batch=True``; a ValueError without it) is a
    restore over an existing tree: a regular-file entry of FileSize > 0 whose
    local path is already a regular file of that size is not created or
    truncated during the walk; once the chains are read, those files are cut
    and hashed by ``Engine.match_paths`` and one whose block IDs are its
    chain's is kept as it is: only its permission bits and ModTime are set, no
    data block of it is read, and it is counted in ``stats["kept"]``, not in
    ``bytes``.  Every other candidate is created or truncated and restored
    with the rest.

    ``reuse_local=True`` (with ``batch=True``; a ValueError without it)
    includes ``keep_matching`` and goes one step further, per block instead of
    per file.  Every regular file already at an entry's path (of any size) and
    every file in ``reuse_paths`` (a file's previous name, a copy elsewhere;
    only read) is cut and hashed once; ``Engine.locate_ids`` (K13) then finds,
    for each data block a file to restore needs, a local chunk with that ID,
    and the block is read from that file instead of ``read_block``: a file
    changed in one place, grown by a byte, renamed or copied fetches only the
    blocks no local file holds.  A reused chunk enters the restore as a raw
    block and is verified like a fetched one, so nothing rests on the local
    files staying as they were hashed: a file whose first bad block was a
    reused one is restored once more with every block fetched
    (``stats["reuse_retried"]``); a bad fetched block raises as ever.  A file
    that was there before is written to a temporary beside it and renamed over
    it once every file of the call is good, so no local file is truncated
    while it may still be read (two files that exchanged content restore
    correctly), and after a failure the temporaries are gone and the old files
    are as they were.  ``stats`` gains ``"kept"``, ``"blocks_reused"``,
    ``"bytes_reused"``, ``"blocks_fetched"`` (data blocks read through
    ``read_block``) and ``"reuse_retried"``; ``"bytes"`` stays the bytes written.

    Directory blocks and chain blocks are inflated and verified on the device
    with their links (``Engine.restore_blocks``), then parsed
    (``parse_directory_block`` / ``parse_chain_block``); regular files stream
    through ``Engine.restore_file`` (every data block verified, the file
    assembled on the device).  Symbolic links, empty files and directories are
    created as the reference does; a file is opened with the entry's mode and
    gets its ModTime (restore.go:108, 141), a directory is chmod-ed after its
    content (restore.go:99).  Decrypt keys are ignored, as in the reference
    (restore.go:57).  Returns the counts ``{"files", "directories", "bytes"}``.
    """
    if keep_matching and not batch:
        raise ValueError("keep_matching needs batch=True")
    if reuse_local and not batch:
        raise ValueError("reuse_local needs batch=True")
    dest = os.fsencode(os.fspath(dest))
    if batch:
        return _restore_tree_batched(eng, root_entry, read_block, dest, window_bytes, io_threads, keep_matching,
                                     reuse_local, reuse_paths)
    stats = {"files": 0, "directories": 0, "bytes": 0}

    def restore_entry(e: FileEntry, path: bytes):
        local = os.path.join(path, bytes(e.file_name))
        if e.file_mode & MODE_SYMLINK:  # restore.go:76-84
            if e.content_type != TYPE_SYMLINK:
                raise HbxError(f"invalid ContentType for a symlink ({e.content_type})")
            os.symlink(bytes(e.file_link), local)
        elif e.file_mode & MODE_DIR:  # restore.go:85-102
            os.makedirs(local, 0o777, exist_ok=True)
            if e.content_type == TYPE_DIRECTORY:
                for kid in parse_directory_block(_read_verified(eng, read_block, e.content_block_id, "directory")):
                    restore_entry(kid, local)
            elif e.content_type != TYPE_EMPTY:
                raise HbxError(f"invalid ContentType for a directory ({e.content_type})")
            os.chmod(local, e.file_mode & 0o777)
            stats["directories"] += 1
        else:  # restore.go:103-145
            if e.content_type not in (TYPE_FILE_CHAIN, TYPE_FILE_DATA, TYPE_EMPTY):
                raise HbxError(f"invalid ContentType for a file ({e.content_type})")
            # created with the entry's mode, as OpenFile does (restore.go:108: the umask applies)
            fd = os.open(local, os.O_CREAT | os.O_TRUNC | os.O_WRONLY, e.file_mode & 0o777)
            mode = stat.S_IMODE(os.fstat(fd).st_mode)
            os.close(fd)
            if e.content_type == TYPE_FILE_CHAIN:
                ids, _keys = parse_chain_block(_read_verified(eng, read_block, e.content_block_id, "chain"))
            else:
                ids = [e.content_block_id] if e.content_type == TYPE_FILE_DATA else []
            if ids:
                # The reference writes through the handle it created; the engine opens the path again, which a
                # mode without the owner's write bit (0444) would refuse: writable while written, then the mode
                # the creation gave it.
                if not mode & stat.S_IWUSR:
                    os.chmod(local, mode | stat.S_IWUSR)
                try:
                    stats["bytes"] += eng.restore_file(ids, lambda i: read_block(bytes(ids[i]))[:2], out_path=local,
                                                       window_bytes=window_bytes)
                finally:
                    if not mode & stat.S_IWUSR:
                        os.chmod(local, mode)
            os.utime(local, ns=(time.time_ns(), int(e.mod_time)))
            stats["files"] += 1

    restore_entry(root_entry, dest)
    return stats


def diff_tree(eng: Engine, root_entry: FileEntry, read_block, local_root, window_bytes: int = 0,
              io_threads: int = 16, by_id: bool = False) -> Dict[str, object]:
    """diffEntry(root_entry, local_root) with diffDir below it
    (hashback/restore.go:279-414): compare a stored tree with a local one.

    Per entry, as the reference: the local path exists; a symbolic link points
    to the same target; a directory is a directory; a file has the same size,
    permission bits and ModTime (at second precision).  The data of every file
    whose size matches is compared on the device in one ``Engine.diff_files``
    call (every block verified; a corrupted block raises :class:`HbxError`, as
    the reference panics).  Directory and chain blocks are read level by level
    in batched calls, as ``restore_tree(batch=True)`` does.  A name only one
    side has is reported for the whole of both listings (the reference's merge
    loop ends with the shorter one).  ``platformSafeFilename`` is not applied.

    With ``by_id=True`` the files whose data would be compared are first cut
    and hashed locally (``Engine.match_paths``) and their block IDs compared
    with their chains: a block ID binds the block's length and bytes
    (block.go:96-111), so a file with its chain's IDs equals the stored one and
    none of its data blocks is fetched.  Any other file (changed, or stored
    with other cuts) goes through the byte comparison above, in one call, so
    the answer never rests on how the stored chain was cut.  The result is
    that of ``by_id=False`` plus ``"matched_by_id"``, the number of files
    settled without their blocks.

    Returns ``{"files", "directories", "different"}``: the files and
    directories compared, and one ``(path, reason)`` per path that differs.
    """
    root = os.fsencode(os.fspath(local_root))
    reasons: Dict[bytes, List[str]] = {}
    order: List[bytes] = []

    def differs(path: bytes, why: str):
        if path not in reasons:
            reasons[path] = []
            order.append(path)
        reasons[path].append(why)

    out = {"files": 0, "directories": 0}
    data_files: List[Tuple[FileEntry, bytes]] = []
    level: List[Tuple[FileEntry, bytes]] = [(root_entry, root)]
    while level:
        want: List[Tuple[FileEntry, bytes]] = []
        for e, path in level:
            local = os.path.join(path, bytes(e.file_name))
            try:
                st = os.lstat(local)
            except FileNotFoundError:
                differs(local, "local path does not exist")
                continue
            if e.file_mode & MODE_SYMLINK:  # restore.go:287-303
                if e.content_type != TYPE_SYMLINK:
                    raise HbxError(f"invalid ContentType for a symlink ({e.content_type})")
                if not stat.S_ISLNK(st.st_mode):
                    differs(local, "local path is not a symlink")
                elif os.readlink(local) != bytes(e.file_link):
                    differs(local, f"symlink points to {os.fsdecode(os.readlink(local))} and not "
                                   f"{os.fsdecode(bytes(e.file_link))}")
            elif e.file_mode & MODE_DIR:  # restore.go:304-316
                if not stat.S_ISDIR(st.st_mode):
                    differs(local, "local path is not a directory")
                    continue
                if e.content_type == TYPE_DIRECTORY:
                    want.append((e, local))
                elif e.content_type != TYPE_EMPTY:
                    raise HbxError(f"invalid ContentType for a directory ({e.content_type})")
                out["directories"] += 1
            else:  # restore.go:317-367
                if e.content_type not in (TYPE_FILE_CHAIN, TYPE_FILE_DATA, TYPE_EMPTY):
                    raise HbxError(f"invalid ContentType for a file ({e.content_type})")
                if not stat.S_ISREG(st.st_mode):
                    differs(local, "local path is not a regular file")
                    continue
                if int(e.file_size) != st.st_size:
                    differs(local, f"local file size {st.st_size} and remote size {int(e.file_size)} are different")
                    continue
                if e.file_mode & 0o777 != stat.S_IMODE(st.st_mode) & 0o777:
                    differs(local, f"local permissions {stat.S_IMODE(st.st_mode) & 0o777:o} and remote "
                                   f"{e.file_mode & 0o777:o} are different")
                if int(e.mod_time) // 10**9 != st.st_mtime_ns // 10**9:
                    differs(local, "local modification time and remote are different")
                if e.content_type != TYPE_EMPTY:
                    data_files.append((e, local))
                out["files"] += 1
        blocks = _read_verified_many(eng, read_block, [e.content_block_id for e, _ in want], "directory")
        level = []
        for (_, local), blk in zip(want, blocks):  # diffDir, restore.go:372-414
            kids = parse_directory_block(blk)
            remote = {bytes(k.file_name) for k in kids}
            for name in sorted(os.listdir(local)):
                if name not in remote:
                    differs(os.path.join(local, name), "remote path does not exist")
            level.extend((kid, local) for kid in kids)
    ids = _file_chains(eng, read_block, [e for e, _ in data_files])
    rest = list(range(len(data_files)))  # the files whose bytes are compared
    why: Dict[int, str] = {}             # a file's data reason, reported in the files' order below
    if by_id:
        out["matched_by_id"] = 0
    if by_id and data_files:
        ms = eng.match_paths([p for _, p in data_files], ids, io_threads=io_threads,
                             sizes=[int(e.file_size) for e, _ in data_files], skip_unreadable=True)
        rest = []
        for k, m in enumerate(ms):
            if m.errno:
                why[k] = f"cannot read the local file: {os.strerror(m.errno)}"
            elif m.same:
                out["matched_by_id"] += 1
            else:
                rest.append(k)
    if rest:
        res = eng._restore_files_stream([ids[k] for k in rest], lambda f, i: read_block(ids[rest[f]][i])[:2], None,
                                        [data_files[k][1] for k in rest],
                                        [max(int(data_files[k][0].file_size), 0) for k in rest], window_bytes,
                                        io_threads, None)
        for k, r in zip(rest, res):
            local, chain = data_files[k][1], ids[k]
            if r.bad_index is not None:
                raise HbxError(f"block {chain[r.bad_index].hex()} (block {r.bad_index} of {os.fsdecode(local)}) "
                               f"corrupted (status {r.bad_status})")
            if r.errno:
                why[k] = f"cannot read the local file: {os.strerror(r.errno)}"
            elif r.first_diff is not None:
                why[k] = f"data is different at offset {r.first_diff}"
    for k in sorted(why):
        differs(data_files[k][1], why[k])
    out["different"] = [(os.fsdecode(p), "; ".join(reasons[p])) for p in order]
    return out
