"""Data files built to be compacted, and a pure-Python reference of the
compaction (helper, no test): CompactFile's loop, the serialisers of the meta
and index entries and sixByteLocation.Set, restated with `struct` from the Go
source lines cited beside them (file.go:lines, the rule in prose).  Every comparison in
tests/test_compact_craft.py and tests/test_gpu_compact.py has this module on
its reference side; the code under test never is.  The files themselves come
from tests/datfile_craft.py's writer.
"""
from __future__ import annotations

import random
import struct
from dataclasses import dataclass, field

from . import datfile_craft as D

DROP, STAY, MOVE = 0, 1, 2
NEVER = (1 << 64) - 1
LIMIT = (1 << 34) - 1          # storageOffsetLimit, storagedb.go:52
FILE_MAX = 0x3FFF
EXISTS, NOLINKS = 1, 2         # entryFlagExists, entryFlagNoLinks: storagedb.go:56-57
ERR_ARG, ERR_CAPACITY = -1, -3
TILES = (256, 4096, 65536)
SUMMARY_FIELDS = ("n_entries", "n_stay", "n_moved", "n_dropped", "stay_end", "moved_bytes", "dropped_bytes",
                  "deleted_bytes", "meta_bytes", "n_meta", "first_past_limit")


class PastLimit(Exception):
    """sixByteLocation.Set's second ASSERT."""


def six_byte_location(file: int, offset: int) -> bytes:
    # storagedb.go:90-101: the file must be 0..0x3fff and the offset 0..2^34 - 1 (two assertions); the value is
    # file << 34 | offset, stored big-endian in 6 bytes
    assert 0 <= file <= 0x3FFF, file
    if not 0 <= offset <= 0x3FFFFFFFF:
        raise PastLimit(offset)
    return struct.pack(">Q", file << 34 | (offset & 0x3FFFFFFFF))[2:]


def location_get(b: bytes):
    # storagedb.go:102-105: the 6 bytes read big-endian; the file is the value >> 34, the offset its low 34 bits
    v = int.from_bytes(b, "big")
    return v >> 34, v & 0x3FFFFFFFF


def meta_entry(bid: bytes, file: int, offset: int, data_size: int, links) -> bytes:
    # meta.go:29-39: the data marker as BE32, the block ID, the 6-byte location, the data size as BE32, the
    # link count as BE32, then the links
    return (D.MARK + bid + six_byte_location(file, offset) + struct.pack(">II", data_size, len(links)) +
            b"".join(links))


def ix_entry(flags: int, bid: bytes, file: int, offset: int) -> bytes:
    # index.go:33-38: the flags as BE16, the block ID, the 6-byte location
    return struct.pack(">H", flags) + bid + six_byte_location(file, offset)


def ref_meta_parse(stream: bytes) -> list:
    """StorageMetaEntry.Unserialize (meta.go:40-55) until the stream is used
    up; raises where the reference aborts (a wrong marker) or the bytes end
    inside a record."""
    out, at = [], 0
    while at < len(stream):
        if stream[at:at + 4] != D.MARK:
            raise ValueError(f"Incorrect metadata cache marker at {at}")
        if at + 34 > len(stream):
            raise ValueError(f"record at {at} is cut")
        bid, loc = stream[at + 4:at + 20], stream[at + 20:at + 26]
        data_size, n = struct.unpack_from(">II", stream, at + 26)
        if at + 34 + 16 * n > len(stream):
            raise ValueError(f"the links of the record at {at} are cut")
        f, o = location_get(loc)
        out.append(dict(id=bid, file=f, off=o, data_size=data_size, at=at,
                        links=[stream[at + 34 + 16 * k:at + 50 + 16 * k] for k in range(n)]))
        at += 34 + 16 * n
    return out


@dataclass
class Case:
    name: str
    buf: bytes
    entries: list            # dicts with off, size, n_links, data_len, id (as datfile_craft.parse_entry's)
    keep: list
    kw: dict = field(default_factory=dict)  # file_no, dst_file_no, dst_base, keep_prefix, meta_file_no, meta_base
    broken: bool = False     # the file has bytes that are neither entry nor gap

    @property
    def size(self) -> int:
        return len(self.buf)


def ref_compact(buf: bytes, entries, keep, file_no=0, dst_file_no=None, dst_base=16, keep_prefix=True,
                meta_file_no=0, meta_base=16, streams=True) -> dict:
    """CompactFile (gc.go:208-318) over the entry list, the free file being
    (dst_file_no, dst_base) and every kept entry getting the meta and index
    entry writeBlockFile gives a block (data.go:91-100)."""
    size = len(buf)
    dst_file_no = file_no if dst_file_no is None else dst_file_no
    klass, new_off, meta_off = [], [], []
    moved, meta, ix, relocations = [], [], [], []
    deleted = moved_bytes = meta_bytes = dropped_bytes = 0
    past = None
    # gc.go:244: the read offset and the high-water mark both start behind the 16-byte file header
    offset = high_water = 16
    for i, (e, k) in enumerate(zip(entries, keep)):
        # gc.go:246-249: a gap in front of the entry is skipped; its bytes count as deleted and advance the
        # offset (here: whatever lies between two entries of the list)
        deleted += e["off"] - offset
        offset = e["off"]
        # gc.go:251-253: the entry is read where the offset stands, which then advances by the entry's size
        read_offset, entry_size = offset, e["size"]
        offset += entry_size
        if not k:
            # gc.go:258-263: no index entry for the ID, or one that points elsewhere: the entry's size is deleted
            deleted += entry_size
            dropped_bytes += entry_size
            klass.append(DROP)
            new_off.append(NEVER)
            meta_off.append(NEVER)
            continue
        if keep_prefix and read_offset == high_water:
            # gc.go:266-268: the free file is not an earlier one and the entry starts at the high-water mark:
            # it stays, and the mark moves behind it
            high_water = offset
            klass.append(STAY)
            where = (file_no, read_offset)
        else:
            # gc.go:274-284: the entry is written to the free file as it is, its size counts as moved, and a
            # relocation (block ID, free file's number, offset it was written at) is noted
            klass.append(MOVE)
            where = (dst_file_no, dst_base + moved_bytes)
            moved_bytes += entry_size
            relocations.append((e["id"], where[0], where[1]))
            if streams:
                moved.append(buf[read_offset:read_offset + entry_size])
        new_off.append(where[1])
        meta_off.append(meta_base + meta_bytes)
        meta_bytes += 34 + 16 * e["n_links"]
        if past is None:
            try:
                # data.go:91-92: the meta entry holds the ID, the data entry's size and the links; its location is
                # the data file's number and offset
                links = [buf[e["off"] + 24 + 16 * j:e["off"] + 40 + 16 * j] for j in range(e["n_links"])] if streams else []
                m = meta_entry(e["id"], where[0], where[1], entry_size, links)
                # data.go:96-100: the index entry's flags are "exists", plus "no links" for a block without links;
                # its location is the meta file's number and the meta entry's offset
                x = ix_entry(EXISTS | (NOLINKS if e["n_links"] == 0 else 0), e["id"], meta_file_no, meta_off[-1])
                if streams:
                    meta.append(m)
                    ix.append(x)
            except PastLimit:
                past = i
    deleted += max(size - offset, 0) if entries else max(size - 16, 0)  # (a file that ends in a gap)
    n_stay, n_moved = klass.count(STAY), klass.count(MOVE)
    summary = dict(n_entries=len(entries), n_stay=n_stay, n_moved=n_moved, n_dropped=klass.count(DROP),
                   stay_end=high_water, moved_bytes=moved_bytes, dropped_bytes=dropped_bytes,
                   deleted_bytes=max(size - 16, 0) - (high_water - 16) - moved_bytes, meta_bytes=meta_bytes,
                   n_meta=n_stay + n_moved, first_past_limit=past)
    res = dict(rc=0 if past is None else ERR_CAPACITY, klass=klass, new_off=new_off, meta_off=meta_off,
               summary=summary, deleted=deleted, relocations=relocations)
    if streams and past is None:
        res.update(moved=b"".join(moved), meta=b"".join(meta), ix=b"".join(ix))
    return res


def ref(case: Case, streams=True) -> dict:
    return ref_compact(case.buf, case.entries, case.keep, streams=streams, **case.kw)


# ------------------------------------------------------------------- corpus --
def fake(size: int, seed, n_links: int = 0) -> bytes:
    """A raw entry of exactly `size` bytes with seeded links, data and ID (the
    ID is not the block's hash: compaction never verifies)."""
    dl = size - 29 - 16 * n_links
    assert dl >= 0, (size, n_links)
    return D.entry(D.rnd(dl, f"c-{seed}"), D.links_of(n_links, f"c-{seed}"), D.RAW, bid=D.rnd(16, f"cid-{seed}"))


def build(name, parts, kw=None, broken=False) -> Case:
    """parts: (bytes of one entry, keep) or ("raw", bytes) / ("gap", skip) as write_datfile takes them."""
    items, flags = [], []
    for p in parts:
        if p[0] in ("raw", "gap"):
            items.append(p)
            flags.append(None)
        else:
            items.append(("raw", p[0]))
            flags.append(bool(p[1]))
    buf, offs = D.write_datfile(items)
    entries, keep = [], []
    for off, k in zip(offs, flags):
        if k is None:
            continue
        _, r = D.parse_entry(buf, off, 1 << 30)
        assert r is not None, (name, off)
        entries.append(r)
        keep.append(k)
    return Case(name, buf, entries, keep, dict(kw or {}), broken)


def case_alignments() -> Case:
    """A: 256 movers of 48..63 bytes, one per pair (source offset mod 16,
    destination offset mod 16), a dropped entry in front of each setting the
    source and each mover's size the next one's destination.  Every one of them
    ends off a granule boundary with a mover behind it, so the granule across
    its END straddles; where the next pair needs destination 0, a filler mover
    takes the stream there.  The granule across a mover's START straddles for
    every destination but 0, where the mover starts a granule."""
    parts = [(fake(48, "A-first"), True)]  # (so that the first pair's mover has a neighbour in front)
    so, sp = 16 + 48, 48   # the next byte of the file / of the stream (dst_base is 16: the same mod 16)
    pairs = [(a, b) for a in range(16) for b in range(16)]
    # the first filler leaves the stream at 0 mod 16, as pair (0, 0) needs
    for k, (a, b) in enumerate(pairs):
        assert sp % 16 == b
        drop = 29 + ((a - so - 29) % 16)
        parts.append((fake(drop, f"A-d{k}"), False))
        so += drop
        nb = pairs[k + 1][1] if k + 1 < len(pairs) else 0
        size = 48 + (((nb or 7) - sp - 48) % 16)
        parts.append((fake(size, f"A-m{k}"), True))
        so += size
        sp += size
        if nb == 0:
            fill = 29 + ((0 - sp - 29) % 16)
            parts.append((fake(fill, f"A-f{k}"), True))
            so += fill
            sp += fill
    parts.append((fake(61, "A-last"), True))
    return build("A_alignments", parts, dict(keep_prefix=False))


def case_small() -> Case:
    """B: 5,000 entries of 29 bytes, every other one kept."""
    return build("B_small", [(fake(29, f"B{k}"), k % 2 == 1) for k in range(5000)])


def case_tiles() -> Case:
    """C: movers that end one byte before, on and one byte behind a tile end
    at each tile size, one of 1 KiB (four tiles of 256) and one of 200 KiB + 7."""
    parts, sp = [], 0
    for T in TILES:
        for d in (-1, 0, 1):
            target = ((sp + 29 + T) // T) * T + d
            parts.append((fake(target - sp, f"C{T}{d}"), True))
            sp = target
    parts += [(fake(1024, "C1k"), True), (fake(29, "Cdrop"), False), (fake(200 * 1024 + 7, "C200k"), True),
              (fake(33, "Cend"), True)]
    return build("C_tiles", parts, dict(keep_prefix=False))


def case_large() -> Case:
    """D: one raw entry with 8 MiB of data, from source offset 5 mod 16 to destination offset 11 mod 16."""
    first = fake(43, "D0")                    # the stream continues at 43, new_off at 16 + 43 = 11 mod 16
    drop = fake(29 + ((5 - (16 + 43 + 29)) % 16), "D1")
    return build("D_large", [(first, True), (drop, False), (fake((8 << 20) + 29, "D2"), True)], dict(keep_prefix=False))


def cases_classes() -> list:
    e = lambda k, size=100: fake(size + k, f"E{k}", k % 3)  # noqa: E731
    six = [e(k) for k in range(6)]
    c = [build("E_all_stay", [(x, True) for x in six]),
         build("E_all_move", [(x, True) for x in six], dict(keep_prefix=False)),
         build("E_first_dropped", [(x, k > 0) for k, x in enumerate(six)]),
         build("E_gap_first", [("gap", 40)] + [(x, True) for x in six]),
         build("E_drop_middle", [(x, k != 3) for k, x in enumerate(six)]),
         build("E_after_broken", [(six[0], True), (six[1], True), ("raw", b"\x01\x02\x03\x04\x05\x06\x07"),
                                  (six[2], True), (six[3], True)], broken=True),
         build("E_gap_middle", [(six[0], True), ("gap", 12), (six[1], True), (six[2], False), (six[3], True)]),
         build("E_none_kept", [(x, False) for x in six]),
         build("E_n0", []),
         build("E_n0_gap", [("gap", 64)]),
         build("E_one_stay", [(six[0], True)]),
         build("E_one_move", [(six[0], True)], dict(keep_prefix=False)),
         build("E_one_drop", [(six[0], False)]),
         build("E_ends_at_size", [(six[0], False), (six[1], True)])]
    assert c[-1].entries[-1]["off"] + c[-1].entries[-1]["size"] == c[-1].size
    return c


LINK_COUNTS = (0, 1, 4, 16, 17, 300, 5000)


def case_links(lane_max: int, wave_max: int) -> Case:
    """F: link lists on both sides of both degree thresholds: each count once
    in the staying prefix, then three times moved, each time behind a dropped
    entry whose size puts the mover at another source offset mod 16."""
    assert lane_max in LINK_COUNTS and lane_max + 1 in LINK_COUNTS and 300 <= wave_max < 5000
    parts, so = [], 16
    for k, n in enumerate(LINK_COUNTS):
        parts.append((fake(29 + 16 * n + 10 + k, f"Fs{n}", n), True))
        so += len(parts[-1][0])
    for rnd_ in range(3):
        for k, n in enumerate(LINK_COUNTS):
            want = (1 + 5 * rnd_ + 3 * k) % 16
            parts.append((fake(29 + (want - so - 29) % 16, f"Fd{rnd_}{n}"), False))
            parts.append((fake(29 + 16 * n + (3 * k + rnd_) % 11, f"Fm{rnd_}{n}", n), True))
            so += len(parts[-2][0]) + len(parts[-1][0])
            assert (so - len(parts[-1][0])) % 16 == want
    return build("F_links", parts)


def cases_locations() -> list:
    """G: file numbers, bases and the 16 GiB limit: numbers in records, over a small file."""
    parts = [(fake(60, "G0", 1), True), (fake(45, "G1"), False), (fake(77, "G2", 2), True), (fake(29, "G3"), True),
             (fake(50, "G4", 1), True)]
    c = []
    for f in (0, 1, FILE_MAX):
        c.append(build(f"G_files_{f}", parts, dict(file_no=f, dst_file_no=FILE_MAX - f, meta_file_no=f ^ 1)))
    for b in (16, 17, (1 << 32) - 3):
        c.append(build(f"G_dst_base_{b}", parts, dict(dst_base=b, meta_base=b + 5)))
    # the movers are entries 2, 3, 4: the last one starts 77 + 29 bytes behind dst_base
    c.append(build("G_dst_at_limit", parts, dict(dst_base=LIMIT - 106, dst_file_no=3)))
    c.append(build("G_dst_past_limit", parts, dict(dst_base=LIMIT - 105, dst_file_no=3)))
    # the meta records of entries 0, 2, 3 take 50 + 66 + 34 bytes: the last one's starts 150 behind meta_base
    c.append(build("G_meta_at_limit", parts, dict(meta_base=LIMIT - 150, meta_file_no=9)))
    c.append(build("G_meta_past_limit", parts, dict(meta_base=LIMIT - 149, meta_file_no=9)))
    # a stayer that lies above the limit cannot be built without a 16 GiB file: the rule is the same comparison
    return c


def corpus(lane_max: int = 16, wave_max: int = 4096) -> dict:
    cs = [case_alignments(), case_small(), case_tiles(), case_large()] + cases_classes() + \
        [case_links(lane_max, wave_max)] + cases_locations()
    return {c.name: c for c in cs}


def granules(case: Case, r: dict):
    """(stream offset, index of the mover it starts in, straddles) per 16-byte granule of the moved stream."""
    movers = [i for i, k in enumerate(r["klass"]) if k == MOVE]
    base = case.kw.get("dst_base", 16)
    out, j = [], 0
    for s in range(0, r["summary"]["moved_bytes"], 16):
        while r["new_off"][movers[j]] - base + case.entries[movers[j]]["size"] <= s:
            j += 1
        end = r["new_off"][movers[j]] - base + case.entries[movers[j]]["size"]
        out.append((s, movers[j], s + 16 > end and end < r["summary"]["moved_bytes"]))
    return out


def c_entries(entries, cls):
    """The entry dicts as an array of the ctypes structure `cls` (hbx_dat_entry)."""
    arr = (cls * max(len(entries), 1))()
    for a, e in zip(arr, entries):
        a.off, a.size, a.n_links, a.data_len = e["off"], e["size"], e["n_links"], e["data_len"]
        a.data_off, a.type = e["off"] + 29 + 16 * e["n_links"], e.get("type", D.RAW)
        a.id[:] = e["id"]
    return arr


def keep_masks(n: int, count: int, seed=16):
    r = random.Random(f"keep-{seed}")
    for k in range(count):
        p = (0.0, 1.0, 0.5, 0.7, 0.95, 0.05)[k % 6]
        yield [r.random() < p for _ in range(n)], bool(k % 5)
