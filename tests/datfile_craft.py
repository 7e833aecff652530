"""Storage data files built from seeds, and a pure-Python reference of the
check (helper, no test): the writer, the structural rules, VerifyBlock, the
walk of RecoverData and the per-offset check of checkBlockFromIXEntry, written
from the rules in include/hbxgpu.h with CPython's zlib and hashlib.  Every
comparison in tests/test_datfile_abi.py and tests/test_gpu_datfile.py has this
module on its reference side; the code under test never is.

Format (pkg/storagedb/data.go, pkg/core/block.go):
  header  BE32 "HSDB" | BE32 1 | BE64 deadspace
  entry   "hblk" | BlockID[16] | BE32 n_links | links | u8 DataType | BE32 data_len | data
  gap     "Cgap" | BE64 skip (counted from the 'C')
"""
from __future__ import annotations

import bisect
import hashlib
import random
import struct
import zlib

MARK, GAP = b"hblk", b"Cgap"
RAW, ZLIB = 0xFF, 0x01
HEADER = 16
ST_INVALID, ST_WRONG_ID = 9, 10
SPAN_GAP, SPAN_BROKEN = 0, 1
NONE = None


def header(deadspace: int = 0, filetype: int = 0x48534442, version: int = 1) -> bytes:
    return struct.pack(">IIQ", filetype, version, deadspace)


def block_id(data: bytes, links=()) -> bytes:
    """HashboxBlock.HashData (block.go:96-111)."""
    h = hashlib.md5(struct.pack(">I", len(links)))
    for ln in links:
        h.update(ln)
    h.update(struct.pack(">I", len(data)))
    h.update(data)
    return h.digest()


def entry(data: bytes, links=(), dtype: int = RAW, level: int = 6, bid: bytes = None) -> bytes:
    """One serialized entry whose block is (links, data)."""
    field = bytes(data) if dtype == RAW else zlib.compress(bytes(data), level)
    bid = block_id(data, links) if bid is None else bid
    return (MARK + bid + struct.pack(">I", len(links)) + b"".join(links) + bytes([dtype]) +
            struct.pack(">I", len(field)) + field)


def gap(skip: int, fill: bytes = b"\0") -> bytes:
    """A gap marker followed by the bytes it skips (none when skip < 12)."""
    return GAP + struct.pack(">q", skip) + fill * max(0, skip - 12)


def _flip(b: bytearray, at: int):
    b[at] ^= 0x40


def write_datfile(items, deadspace: int = 0):
    """items: (links, data, dtype, damage) tuples, or ("raw", bytes) for bytes
    put in as they are, or ("gap", skip).  damage: None, or
      "id"    one flipped byte in the BlockID        "link"  one in the first link
      "data"  one in the data field: for a raw block a data byte, for a zlib
              stream a byte of its Adler-32 trailer
      "zhdr"  the zlib stream's first byte            "type0" / "type2"  the DataType
      "nlinks_max"  n_links = 0xFFFFFFFF             "len+1" data_len one more than is there
      "len_rest"    data_len claims everything to the end of the file (patched last)
    Returns (file bytes, offset of every item)."""
    out = bytearray(header(deadspace))
    offs, rest = [], []
    for it in items:
        offs.append(len(out))
        if it[0] == "raw":
            out += it[1]
            continue
        if it[0] == "gap":
            out += gap(it[1])
            continue
        links, data, dtype, damage = it
        e = bytearray(entry(data, links, dtype))
        head = 24 + 16 * len(links)
        if damage == "id":
            _flip(e, 4 + 7)
        elif damage == "link":
            _flip(e, 24 + 3)
        elif damage == "data":
            _flip(e, len(e) - 2 if dtype == ZLIB else head + 5 + (len(e) - head - 5) // 2)
        elif damage == "zhdr":
            _flip(e, head + 5)
        elif damage == "type0":
            e[head] = 0
        elif damage == "type2":
            e[head] = 2
        elif damage == "nlinks_max":
            e[20:24] = b"\xff\xff\xff\xff"
        elif damage == "len+1":
            e[head + 1:head + 5] = struct.pack(">I", len(e) - head - 5 + 1)
        elif damage == "len_rest":
            rest.append((len(out), head))
        elif damage is not None:
            raise ValueError(damage)
        out += e
    for at, head in rest:
        out[at + head + 1:at + head + 5] = struct.pack(">I", len(out) - at - head - 5)
    return bytes(out), offs


# ---------------------------------------------------------------- reference --
def deflate_bound(n: int) -> int:
    return 11 + n + 5 * ((n + 32767) // 32768)


def in_bound(max_block: int) -> int:
    """hbx_restore_in_bound."""
    return deflate_bound(max_block) + 64


def find_all(buf: bytes, pat: bytes):
    """Every position p in [16, size - 4] where pat starts, overlapping ones too."""
    res, p = [], buf.find(pat, HEADER)
    while p >= 0:
        res.append(p)
        p = buf.find(pat, p + 1)
    return res


def parse_entry(buf: bytes, off: int, max_block: int):
    """Rule 3: (has_marker, record or None)."""
    size = len(buf)
    avail = size - off if off < size else 0
    if avail < 4 or buf[off:off + 4] != MARK:
        return False, None
    if avail < 24:
        return True, None
    nl = struct.unpack_from(">I", buf, off + 20)[0]
    head = 24 + 16 * nl + 5
    if avail < head:
        return True, None
    dtype = buf[off + head - 5]
    dl = struct.unpack_from(">I", buf, off + head - 4)[0]
    if avail - head < dl or dtype not in (RAW, ZLIB) or dl > in_bound(max_block):
        return True, None
    return True, dict(off=off, size=head + dl, data_off=off + head, links_off=off + 24, data_len=dl, n_links=nl,
                      type=dtype, id=buf[off + 4:off + 20])


_ZERR = (("incorrect header check", 1), ("unknown compression method", 1), ("invalid window size", 1),
         ("incorrect data check", 1), ("need dictionary", 1), ("invalid stored block lengths", 6),
         ("invalid distance too far back", 5))


def inflate_status(stream: bytes, max_block: int):
    """(status 0..6 as hbx_inflate_blocks_device, data).  Exact for a good
    stream, a bad header or trailer, a stream longer than max_block and a
    truncated one; a best guess from zlib's message for damaged codes, which no
    test relies on."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream, max_block + 1)
    except zlib.error as e:
        msg = str(e)
        for text, st in _ZERR:
            if text in msg:
                return st, None
        return 4, None
    if len(out) > max_block:
        return 3, None
    if not d.eof:
        return 2, None
    return 0, out


def verify_status(buf: bytes, r: dict, max_block: int):
    """(VerifyBlock status 0..7, inflated length)."""
    field = buf[r["data_off"]:r["data_off"] + r["data_len"]]
    if r["type"] == RAW:
        if len(field) > max_block:
            return 3, 0
        data = field
    else:
        st, data = inflate_status(field, max_block)
        if st:
            return st, 0
    links = [buf[r["links_off"] + 16 * k:r["links_off"] + 16 * k + 16] for k in range(r["n_links"])]
    return (0 if block_id(data, links) == r["id"] else 7), len(data)


def ref_check(buf: bytes, max_block: int) -> dict:
    """What hbx_datfile_check_* must report for the file `buf`."""
    size = len(buf)
    ft = struct.unpack_from(">I", buf, 0)[0] if size >= 4 else 0
    ver = struct.unpack_from(">I", buf, 4)[0] if size >= 8 else 0
    dead = struct.unpack_from(">Q", buf, 8)[0] if size >= 16 else 0
    marks = find_all(buf, MARK)
    gaps = find_all(buf, GAP)
    cand = {}
    n_valid = 0
    for p in marks:
        _, r = parse_entry(buf, p, max_block)
        if r is None:
            cand[p] = (ST_INVALID, None, 0)
        else:
            n_valid += 1
            st, plain = verify_status(buf, r, max_block)
            cand[p] = (st, r, plain)
    entries, spans, links = [], [], []
    reached = 0
    past = 0
    broken = first = None
    failed = 0
    offset = HEADER
    while offset < size:
        if size - offset >= 12 and buf[offset:offset + 4] == GAP:
            skip = struct.unpack_from(">q", buf, offset + 4)[0]
            if skip > 0:
                left = size - offset
                if skip > left:
                    past = 1
                spans.append(dict(off=offset, len=min(skip, left), kind=SPAN_GAP, status=0, n_failed=0))
                offset += min(skip, left)
                if offset >= size:
                    break
        block = offset
        here = block in cand
        reached += 1 if here else 0
        if here and cand[block][0] == 0:
            st, r, plain = cand[block]
            if broken is not None:
                spans.append(dict(off=broken, len=block - broken, kind=SPAN_BROKEN, status=first, n_failed=failed))
                broken = None
            entries.append(dict(off=r["off"], size=r["size"], data_off=r["data_off"], link_base=len(links),
                                n_links=r["n_links"], data_len=r["data_len"], plain_len=plain, type=r["type"],
                                id=r["id"]))
            links += [buf[r["links_off"] + 16 * k:r["links_off"] + 16 * k + 16] for k in range(r["n_links"])]
            offset = block + r["size"]
            continue
        if broken is None:
            broken, first, failed = block, (cand[block][0] if here else ST_INVALID), 0
        failed += 1 if here else 0
        k = bisect.bisect_right(marks, block)  # forwardToDataMarker from block + 1
        if k == len(marks):
            break
        offset = marks[k]
    truncate_at = None
    if broken is not None:
        spans.append(dict(off=broken, len=size - broken, kind=SPAN_BROKEN, status=first, n_failed=failed))
        truncate_at = broken
    g = [s for s in spans if s["kind"] == SPAN_GAP]
    b = [s for s in spans if s["kind"] == SPAN_BROKEN]
    summary = dict(size=size, filetype=ft, version=ver, deadspace=dead,
                   header_ok=int(size >= 16 and ft == 0x48534442 and ver == 1), gap_past_eof=past,
                   n_candidates=len(marks), n_gap_markers=len(gaps), n_valid=n_valid,
                   n_unreached=len(marks) - reached, n_entries=len(entries),
                   entry_bytes=sum(e["size"] for e in entries), n_gaps=len(g), gap_bytes=sum(s["len"] for s in g),
                   n_broken=len(b), broken_bytes=sum(s["len"] for s in b), n_spans=len(spans), n_links=len(links),
                   truncate_at=truncate_at)
    return dict(entries=entries, spans=spans, summary=summary, links=b"".join(links), cand=cand, gaps=gaps)


def ref_verify_at(buf: bytes, offs, ids, content: bool, max_block: int):
    """What hbx_datfile_verify_at must report."""
    out = []
    for off, want in zip(offs, ids):
        _, r = parse_entry(buf, int(off), max_block)
        if r is None:
            out.append(ST_INVALID)
        elif r["id"] != bytes(want):
            out.append(ST_WRONG_ID)
        else:
            out.append(verify_status(buf, r, max_block)[0] if content else 0)
    return out


def invariant(res_summary: dict) -> bool:
    s = res_summary
    return s["size"] < HEADER or HEADER + s["entry_bytes"] + s["gap_bytes"] + s["broken_bytes"] == s["size"]


# ------------------------------------------------------------------- corpus --
def rnd(n: int, seed) -> bytes:
    return random.Random(f"dat-{seed}").randbytes(n)


def text(n: int, seed) -> bytes:
    """Zipf-like words: compresses about 3:1."""
    r = random.Random(f"txt-{seed}")
    words = [bytes(r.choices(b"abcdefghijklmnopqrstuvwxyz", k=r.randint(2, 9))) for _ in range(200)]
    w = [1.0 / (k + 1) for k in range(200)]
    out = bytearray()
    while len(out) < n:
        out += b" ".join(r.choices(words, w, k=64)) + b"\n"
    return bytes(out[:n])


def links_of(n: int, seed):
    return [rnd(16, f"link-{seed}-{k}") for k in range(n)]


TINY = entry(b"")  # 29 bytes: the smallest good entry


def scan_image(size: int, positions, seed, what: bytes = TINY) -> bytes:
    """`size` seeded random bytes behind a header with `what` at each position."""
    b = bytearray(header() + rnd(size - HEADER, seed))
    for p in positions:
        b[p:p + len(what)] = what
    return bytes(b[:size])


def scan_cases(seed=1):
    """64 KiB images: name -> bytes.  Good 29-byte entries at positions chosen
    against K14's 16-byte lanes, 1 KiB waves, 4 KiB workgroups and the
    grid-stride rounds of a grid of 1 (4 KiB) and of 2 workgroups (8 KiB)."""
    S = 65536
    c = {}
    c["align"] = scan_image(S, [1024 + 80 * a + a for a in range(16)], f"{seed}a")
    c["lane"] = scan_image(S, [2048 + 48 * k + 13 + k for k in range(3)], f"{seed}l")
    c["wave"] = scan_image(S, [1024 * (3 + k) - 1 - k for k in range(3)], f"{seed}w")
    c["group"] = scan_image(S, [4096 * (2 + k) - 1 - k for k in range(3)], f"{seed}g")
    c["round"] = scan_image(S, [8192 * (2 + k) - 1 - k for k in range(3)] + [8192 * 7 - 16, 4096 * 13], f"{seed}r")
    c["first"] = scan_image(S, [16], f"{seed}f")
    c["last4"] = scan_image(S, [S - 4], f"{seed}e", MARK)
    c["size-3"] = scan_image(S, [S - 3], f"{seed}d", MARK)  # cut to "hbl": not a candidate
    c["overlap"] = scan_image(S, [5000], f"{seed}o", b"hblhblk")
    c["run4k"] = scan_image(S, [8192 + 3], f"{seed}u", MARK * 1024)
    c["end_entry"] = scan_image(S, [S - 29, S - 29 - 40], f"{seed}t")
    return c


def small_files(seed=2):
    """The header alone, and files of 17..48 bytes: random tails, and tails that start with a marker."""
    c = {"header_only": header(), "bad_type": header(filetype=0x48534443), "bad_version": header(version=2),
         "short_header": header()[:9], "empty": b""}
    for n in range(17, 49):
        c[f"rand{n}"] = (header() + rnd(n - 16, f"{seed}-{n}"))[:n]
        c[f"mark{n}"] = (header() + TINY + rnd(8, f"{seed}m{n}"))[:n]
        c[f"gap{n}"] = (header() + gap(12) + TINY)[:n]
    return c


def parse_cases(max_block: int, seed=3):
    good = lambda k, nl=0, t=RAW: (links_of(nl, f"{seed}{k}"), text(300 + 17 * k, f"{seed}{k}"), t, None)  # noqa: E731
    c = {}
    c["links014"] = write_datfile([good(0), good(1, 1), good(2, 4, ZLIB), good(3, 4)])[0]
    c["nlinks_max"] = write_datfile([good(0), (links_of(1, 5), b"abc", RAW, "nlinks_max"), good(1)])[0]
    c["len+1"] = write_datfile([good(0), ([], rnd(100, seed), RAW, "len+1")])[0]
    c["ends_at_eof"] = write_datfile([good(0, 1), good(1, 0, ZLIB)])[0]
    c["type0"] = write_datfile([good(0), good(1, 1, RAW)[:3] + ("type0",), good(2)])[0]
    c["type2"] = write_datfile([good(0), good(1, 0, ZLIB)[:3] + ("type2",), good(2)])[0]
    whole, offs = write_datfile([good(0), (links_of(1, 9), b"12345", RAW, None)])
    for k in range(1, 50):  # the last entry (50 bytes) cut by the end of the file inside each field
        c[f"cut{k:02d}"] = whole[:offs[1] + k]
    nb = in_bound(max_block)
    c["len_bound+1"] = write_datfile([good(0), ([], bytes(nb + 1), RAW, None), good(1)])[0]
    c["len_bound"] = write_datfile([good(0), ([], bytes(nb), RAW, None), good(1)])[0]  # valid, longer than max_block: 3
    return c


def verify_cases(seed=4):
    t = lambda k: text(3000 + 100 * k, f"{seed}{k}")  # noqa: E731
    items = []
    for k, (dtype, nl) in enumerate([(RAW, 0), (RAW, 3), (ZLIB, 0), (ZLIB, 2)]):
        items.append((links_of(nl, f"{seed}{k}"), t(k), dtype, None))
    items += [([], b"", RAW, None), ([], b"", ZLIB, None), (links_of(2, "e"), b"", RAW, None)]
    items += [([], bytes(65536), ZLIB, None)]  # 64 KiB in ~90 bytes: outgrows its first slot
    c = {"good": write_datfile(items)[0]}
    for damage, dtype, nl in [("data", ZLIB, 0), ("zhdr", ZLIB, 1), ("data", RAW, 0), ("id", RAW, 0), ("id", ZLIB, 2),
                              ("link", RAW, 2), ("link", ZLIB, 3)]:
        c[f"{damage}-{dtype:02x}-{nl}"] = write_datfile(
            [items[0], (links_of(nl, "d"), t(9), dtype, damage), items[3]])[0]
    return c


def walk_cases(seed=5):
    g = lambda k, nl=0, t=RAW: (links_of(nl, f"{seed}{k}"), text(200 + 31 * k, f"{seed}{k}"), t, None)  # noqa: E731
    bad = lambda k, d="id": g(k)[:3] + (d,)  # noqa: E731
    c = {}
    c["len_rest"] = write_datfile([g(0), g(1)[:3] + ("len_rest",), g(2), g(3, 2, ZLIB), g(4)])[0]
    inner = entry(text(150, "inner"))
    c["nested_good"] = write_datfile([g(0), ([], inner, RAW, None), g(1)])[0]
    c["nested_outer_bad"] = write_datfile([g(0), ([], inner, RAW, "id"), g(1)])[0]
    c["two_failures"] = write_datfile([g(0), bad(1), bad(2, "data"), g(3)])[0]
    c["short_span"] = write_datfile([g(0), ("raw", b"\x01\x02\x03\x04\x05"), g(1)])[0]
    c["damage_to_eof"] = write_datfile([g(0), g(1), bad(2)])[0]
    c["garbage_to_eof"] = write_datfile([g(0), ("raw", rnd(300, "tail"))])[0]
    c["gap12"] = write_datfile([g(0), ("gap", 12), g(1), ("gap", 12), g(2)])[0]
    c["gap_first"] = write_datfile([("gap", 100), g(0)])[0]
    c["gap_gap"] = write_datfile([g(0), ("gap", 40), ("gap", 24), g(1)])[0]
    c["gap_to_eof"] = write_datfile([g(0), ("gap", 64)])[0]
    c["gap_past_eof"] = write_datfile([g(0), ("raw", GAP + struct.pack(">q", 1000) + bytes(20))])[0]
    c["gap_skip0"] = write_datfile([g(0), ("raw", GAP + struct.pack(">q", 0)), g(1)])[0]
    c["gap_negative"] = write_datfile([g(0), ("raw", GAP + struct.pack(">q", -24)), g(1)])[0]
    c["gap_huge"] = write_datfile([g(0), ("raw", GAP + struct.pack(">q", (1 << 63) - 1)), g(1)])[0]
    c["gap_cut"] = write_datfile([g(0), ("raw", GAP + b"\0\0\0\0\0\0\0")])[0]
    c["gap_then_bad"] = write_datfile([g(0), ("gap", 30), bad(1), g(2)])[0]
    c["marker_in_tail"] = write_datfile([g(0), ("raw", b"xx" + MARK + b"yyy")])[0]
    c["all_good"] = write_datfile([g(k, k % 3, ZLIB if k % 2 else RAW) for k in range(12)], deadspace=77)[0]
    return c


def big_file(seed=6, size=8 << 20, damaged=0.03):
    """About `size` bytes, several hundred entries: data blocks of 4-64 KiB
    (Zipf text and random bytes, raw and zlib), small directory-like blocks
    with links, a few gaps; `damaged` of the entries get one flipped byte."""
    r = random.Random(f"big-{seed}")
    items, est, k = [], 16, 0
    while est < size - (80 << 10):
        k += 1
        u = r.random()
        if u < 0.04:
            skip = r.randint(12, 5000)
            items.append(("gap", skip))
            est += skip
            continue
        if u < 0.45:
            data, nl = text(r.randint(60, 600), f"{seed}d{k}"), r.randint(1, 40)
        else:
            n = r.randint(4096, 65536)
            data, nl = (text(n, f"{seed}t{k}") if r.random() < 0.7 else rnd(n, f"{seed}r{k}")), 0
        dtype = ZLIB if r.random() < 0.7 else RAW
        # ("len+1" only on raw blocks: a byte behind a zlib stream is not this feature's business)
        damage = (r.choice(["id", "data", "link" if nl else "id", "type2", "len+1" if dtype == RAW else "zhdr"])
                  if r.random() < damaged else None)
        items.append((links_of(nl, f"{seed}k{k}"), data, dtype, damage))
        est += 29 + 16 * nl + (len(data) if dtype == RAW else len(zlib.compress(data, 6))) + 1
    return write_datfile(items)
