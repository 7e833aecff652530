"""CPU: the host side of the data file check (include/hbxgpu.h:
hbx_datfile_header_parse, hbx_datfile_entry_parse, hbx_datfile_walk) against
the pure-Python reference of tests/datfile_craft.py, on the crafted corpus and
on seeded random mutations of it; the size invariant on every result; argument
and capacity errors.  No device call is made: where the device would scan, the
"hblk" and "Cgap" positions come from the reference, and where it would inflate
and hash, the statuses do."""
import ctypes
import mmap
import random
import struct

import pytest

from hashbox_amd import _lib
from . import datfile_craft as C

MB = 1 << 20  # max_block of every case


@pytest.fixture(scope="module")
def L():
    return _lib.load()


def _corpus():
    out = {}
    for fam, cases in (("scan", C.scan_cases()), ("small", C.small_files()), ("parse", C.parse_cases(MB)),
                       ("verify", C.verify_cases()), ("walk", C.walk_cases())):
        for name, buf in cases.items():
            out[f"{fam}/{name}"] = buf
    return out


CORPUS = _corpus()


class Guarded:
    """A copy of `buf` that ends exactly at an unreadable page: a read at or
    past its size faults instead of passing unseen."""

    def __init__(self, buf: bytes):
        page = mmap.PAGESIZE
        n = (len(buf) + page - 1) // page * page
        self.map = mmap.mmap(-1, n + page)
        base = ctypes.addressof(ctypes.c_char.from_buffer(self.map))
        libc = ctypes.CDLL(None, use_errno=True)
        libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert libc.mprotect(base + n, page, 0) == 0, ctypes.get_errno()  # PROT_NONE
        self.addr = base + n - len(buf)
        ctypes.memmove(self.addr, buf, len(buf))
        self.size = len(buf)


def _host_parse(L, g: Guarded, off: int):
    rec = _lib.DatRecord()
    assert L.hbx_datfile_entry_parse(g.addr, g.size, off, MB, ctypes.byref(rec)) == 0
    return rec


def _same_record(rec, ref, has_marker, off):
    assert rec.off == off and (rec.flags & _lib.DAT_F_MARKER) == (1 if has_marker else 0)
    if ref is None:
        assert rec.status == 9
        assert (rec.size, rec.data_off, rec.links_off, rec.data_len, rec.n_links, rec.type) == (0, 0, 0, 0, 0, 0)
        assert bytes(rec.id) == bytes(16)
    else:
        assert rec.status == 0
        got = dict(off=rec.off, size=rec.size, data_off=rec.data_off, links_off=rec.links_off,
                   data_len=rec.data_len, n_links=rec.n_links, type=rec.type, id=bytes(rec.id))
        assert got == ref


def _host_check(L, buf: bytes, entry_cap=None, span_cap=None):
    """Host parse + reference statuses + host walk -> (rc, entries, spans, summary dict)."""
    ref = C.ref_check(buf, MB)
    g = Guarded(buf)
    marks = sorted(ref["cand"])
    cand = (_lib.DatRecord * max(len(marks), 1))()
    plain = (ctypes.c_uint32 * max(len(marks), 1))()
    for k, p in enumerate(marks):
        rec = _host_parse(L, g, p)
        st, r, pl = ref["cand"][p]
        _same_record(rec, r, True, p)
        rec.status = st  # what the device's inflate and VerifyBlock would say
        cand[k] = rec
        plain[k] = pl
    gaps = [p for p in ref["gaps"] if len(buf) - p >= 12]
    goffs = (ctypes.c_uint64 * max(len(gaps), 1))(*gaps)
    gskip = (ctypes.c_int64 * max(len(gaps), 1))(*[struct.unpack_from(">q", buf, p + 4)[0] for p in gaps])
    ecap = len(ref["entries"]) if entry_cap is None else entry_cap
    scap = len(ref["spans"]) if span_cap is None else span_cap
    ents = (_lib.DatEntry * max(ecap, 1))()
    spans = (_lib.DatSpan * max(scap, 1))()
    sm = _lib.DatSummary()
    rc = L.hbx_datfile_walk(len(buf), len(marks), cand, plain, len(gaps), goffs, gskip, ents, ecap, spans, scap,
                            ctypes.byref(sm))
    return rc, ents, spans, sm, ref


WALK_FIELDS = ("size", "gap_past_eof", "n_candidates", "n_unreached", "n_entries", "entry_bytes", "n_gaps",
               "gap_bytes", "n_broken", "broken_bytes", "n_spans", "n_links", "truncate_at")


def _assert_same(ents, spans, sm, ref):
    s = ref["summary"]
    for k in WALK_FIELDS:
        want = s[k] if s[k] is not None else (1 << 64) - 1
        assert getattr(sm, k) == want, (k, getattr(sm, k), want)
    assert sm.n_gap_markers <= s["n_gap_markers"]  # (only markers with 12 bytes inside the file were passed)
    got_e = [dict(off=e.off, size=e.size, data_off=e.data_off, link_base=e.link_base, n_links=e.n_links,
                  data_len=e.data_len, plain_len=e.plain_len, type=e.type, id=bytes(e.id))
             for e in ents[:sm.n_entries]]
    assert got_e == ref["entries"]
    got_s = [dict(off=x.off, len=x.len, kind=x.kind, status=x.status, n_failed=x.n_failed) for x in spans[:sm.n_spans]]
    assert got_s == ref["spans"]
    assert sm.size < 16 or 16 + sm.entry_bytes + sm.gap_bytes + sm.broken_bytes == sm.size
    assert C.invariant(s)


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_host_parse_and_walk_match_the_reference(L, name):
    rc, ents, spans, sm, ref = _host_check(L, CORPUS[name])
    assert rc == 0
    _assert_same(ents, spans, sm, ref)


def test_host_parse_at_every_offset_of_small_files(L):
    """Not only at markers: every offset of a few files, and offsets at and past the end."""
    for name in ("parse/links014", "parse/nlinks_max", "walk/nested_good", "small/mark40", "parse/cut30"):
        buf = CORPUS[name]
        g = Guarded(buf)
        for off in list(range(0, len(buf) + 3)) + [len(buf) + 1000, (1 << 64) - 1, (1 << 63)]:
            has, ref = C.parse_entry(buf, off, MB)
            _same_record(_host_parse(L, g, off), ref, has, off)


@pytest.mark.parametrize("nl, dl", [(0xFFFFFFFF, 5), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x10000000, 7),
                                    (0x0FFFFFFF, 0xFFFFFFF0), (1, 0xFFFFFFFF), (2, 3)])
def test_untrusted_counts_never_read_outside_the_buffer(L, nl, dl):
    """n_links and data_len up to 2^32 - 1, in a buffer that ends exactly at
    `size` in front of an unreadable page, cut at every length."""
    e = bytearray(C.entry(b"12345", C.links_of(1, "u")))
    e[20:24] = struct.pack(">I", nl)
    whole = C.header() + bytes(e) + bytes(40)
    for size in range(16, len(whole) + 1):
        buf = whole[:size]
        g = Guarded(buf)
        has, ref = C.parse_entry(buf, 16, MB)
        _same_record(_host_parse(L, g, 16), ref, has, 16)
    # the same with data_len patched where n_links = 1 puts it
    e = bytearray(C.entry(b"12345", C.links_of(1, "u")))
    e[41:45] = struct.pack(">I", dl)
    whole = C.header() + bytes(e)
    for size in range(16, len(whole) + 1):
        g = Guarded(whole[:size])
        has, ref = C.parse_entry(whole[:size], 16, MB)
        _same_record(_host_parse(L, g, 16), ref, has, 16)


def _mutate(buf: bytes, r: random.Random) -> bytes:
    b = bytearray(buf)
    for _ in range(r.randint(1, 4)):
        kind = r.randrange(5)
        if kind == 0 and len(b) > 16:  # byte flip
            b[r.randrange(16, len(b))] ^= 1 << r.randrange(8)
        elif kind == 1 and len(b) > 17:  # truncation
            del b[r.randrange(17, len(b)):]
        elif kind == 2:  # an inserted marker
            at = r.randrange(16, len(b) + 1)
            b[at:at] = r.choice([C.MARK, C.GAP, C.TINY, C.GAP + struct.pack(">q", r.randint(-5, 300))])
        elif kind == 3 and len(b) > 20:  # a marker written over what is there
            at = r.randrange(16, len(b) - 3)
            b[at:at + 4] = r.choice([C.MARK, C.GAP])
        elif kind == 4 and len(b) > 30:  # a 32-bit field made huge
            at = r.randrange(16, len(b) - 3)
            b[at:at + 4] = r.choice([b"\xff\xff\xff\xff", b"\x7f\xff\xff\xff", b"\x00\x00\x00\x00"])
    return bytes(b)


def test_seeded_mutations_match_the_reference(L):
    """Three hundred mutations of the small corpus files: flips, truncations,
    inserted and overwritten markers, huge counts."""
    names = [n for n in sorted(CORPUS) if len(CORPUS[n]) < 20000]
    r = random.Random("datfile-mutations")
    for k in range(300):
        buf = _mutate(CORPUS[names[k % len(names)]], r)
        rc, ents, spans, sm, ref = _host_check(L, buf)
        assert rc == 0, k
        _assert_same(ents, spans, sm, ref)


def test_header_parse(L):
    ft, ver, dead = ctypes.c_uint32(9), ctypes.c_uint32(9), ctypes.c_uint64(9)
    h = C.header(deadspace=0x0102030405060708)
    args = (ctypes.byref(ft), ctypes.byref(ver), ctypes.byref(dead))
    assert L.hbx_datfile_header_parse(h, 16, *args) == 0
    assert (ft.value, ver.value, dead.value) == (0x48534442, 1, 0x0102030405060708)
    assert L.hbx_datfile_header_parse(h, 16, None, None, None) == 0
    for bad in (C.header(filetype=0x48534443), C.header(version=2), h[:15], h[:8], h[:3], b""):
        g = Guarded(bad)
        assert L.hbx_datfile_header_parse(g.addr if bad else None, len(bad), *args) == -7  # HBX_ERR_FORMAT
        assert ft.value == (struct.unpack(">I", bad[:4])[0] if len(bad) >= 4 else 0)
        assert ver.value == (struct.unpack(">I", bad[4:8])[0] if len(bad) >= 8 else 0)
        assert dead.value == (struct.unpack(">Q", bad[8:16])[0] if len(bad) >= 16 else 0)
    assert L.hbx_datfile_header_parse(None, 16, *args) == -1


def test_walk_capacities_report_the_needed_counts(L):
    buf = CORPUS["walk/two_failures"]
    rc, ents, spans, sm, ref = _host_check(L, buf)
    assert rc == 0 and sm.n_entries == 2 and sm.n_spans == 1
    rc, ents, spans, sm, _ = _host_check(L, buf, entry_cap=1)
    assert rc == _lib.ERR_CAPACITY and sm.n_entries == 2 and sm.n_spans == 1 and ents[0].off == ref["entries"][0]["off"]
    buf = CORPUS["walk/gap_gap"]
    rc, ents, spans, sm, ref = _host_check(L, buf, span_cap=1)
    assert rc == _lib.ERR_CAPACITY and sm.n_spans == 2 and sm.n_entries == 2 and spans[0].off == ref["spans"][0]["off"]
    rc, ents, spans, sm, ref = _host_check(L, buf, entry_cap=0, span_cap=0)
    assert rc == _lib.ERR_CAPACITY and (sm.n_entries, sm.n_spans, sm.entry_bytes) == (2, 2, ref["summary"]["entry_bytes"])


def test_argument_errors_without_a_device(L):
    sm = _lib.DatSummary()
    rec = _lib.DatRecord()
    one = (_lib.DatRecord * 2)()
    one[0].off, one[1].off = 50, 40  # descending
    offs = (ctypes.c_uint64 * 2)(30, 20)
    skips = (ctypes.c_int64 * 2)(12, 12)
    assert L.hbx_datfile_walk(100, 0, None, None, 0, None, None, None, 0, None, 0, None) == -1
    assert L.hbx_datfile_walk(100, 1, None, None, 0, None, None, None, 0, None, 0, ctypes.byref(sm)) == -1
    assert L.hbx_datfile_walk(100, 0, None, None, 1, None, None, None, 0, None, 0, ctypes.byref(sm)) == -1
    assert L.hbx_datfile_walk(100, 0, None, None, 0, None, None, None, 1, None, 0, ctypes.byref(sm)) == -1
    assert L.hbx_datfile_walk(100, 2, one, None, 0, None, None, None, 0, None, 0, ctypes.byref(sm)) == -1
    assert L.hbx_datfile_walk(100, 0, None, None, 2, offs, skips, None, 0, None, 0, ctypes.byref(sm)) == -1
    assert L.hbx_datfile_walk(100, 0, None, None, 0, None, None, None, 0, None, 0, ctypes.byref(sm)) == _lib.ERR_CAPACITY
    assert (sm.n_spans, sm.n_broken, sm.broken_bytes, sm.truncate_at) == (1, 1, 84, 16)  # nothing but garbage
    assert L.hbx_datfile_entry_parse(None, 10, 0, 0, ctypes.byref(rec)) == -1
    assert L.hbx_datfile_entry_parse(b"x" * 10, 10, 0, 0, None) == -1
    assert L.hbx_datfile_entry_parse(b"x" * 10, 10, 0, (1 << 30) + 1, ctypes.byref(rec)) == -1
    # the device calls reject their arguments before they touch a context or a device
    assert L.hbx_datfile_check_device(None, None, 0, 0, 0, 0, None, 0, None, 0, None, 0, ctypes.byref(sm)) == -1
    assert L.hbx_datfile_check_path(None, b"/nonexistent", 0, 0, 0, None, 0, None, 0, None, 0, ctypes.byref(sm)) == -1
    assert L.hbx_datfile_verify_at(None, None, 0, b"/nonexistent", 0, None, None, 1, 0, 0, None) == -1


def test_python_names_and_layouts(L):
    import inspect

    import hashbox_amd
    from hashbox_amd.engine import Engine
    assert [ctypes.sizeof(t) for t in (_lib.DatRecord, _lib.DatEntry, _lib.DatSpan, _lib.DatSummary)] == [64, 64, 32, 136]
    for name in ("hbx_datfile_header_parse", "hbx_datfile_entry_parse", "hbx_datfile_walk", "hbx_datfile_check_device",
                 "hbx_datfile_check_path", "hbx_datfile_verify_at"):
        assert name in _lib.EXPORTS and getattr(L, name).restype is ctypes.c_int
    assert list(inspect.signature(Engine.check_datfile).parameters)[:2] == ["self", "source"]
    assert list(inspect.signature(Engine.verify_datfile_at).parameters)[:4] == ["self", "source", "offs", "expect_ids"]
    assert hashbox_amd.DatFileCheck is hashbox_amd.engine.DatFileCheck
    assert L.hbx_restore_in_bound(MB) == C.in_bound(MB)


def test_k14_is_built_like_the_other_kernels():
    import os

    from hashbox_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "hbx_datfile.hip" in build.SOURCES and "hbx_datfile.h" in build.SOURCES
    eng = open(os.path.join(root, "hashbox_amd", "csrc", "hbx_engine.hip")).read()
    assert '#include "hbx_datfile.hip"' in eng and '#include "hbx_datfile.h"' in eng
    k14 = open(os.path.join(root, "hashbox_amd", "csrc", "hbx_datfile.hip")).read()
    assert "hbx_k14_scan" in k14 and "hbx_k14_parse" in k14 and "__shared__" not in k14 and "asm" not in k14


def test_k14_kernels_use_no_scratch(tmp_path):
    """The compiler's metadata for gfx950: neither K14 kernel spills or has a private segment."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "k14.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(root, "hashbox_amd", "csrc", "hbx_datfile.hip")], check=True, capture_output=True,
                   timeout=600)
    isa = out.read_text()
    for name in ("hbx_k14_scan", "hbx_k14_parse"):
        i = isa.index(f".name:           {name}\n")
        blk = isa[isa.rfind("  - .", 0, i):isa.find("  - .", i) if isa.find("  - .", i) > 0 else len(isa)]
        get = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))  # noqa: E731
        assert get("vgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
        assert get("group_segment_fixed_size") == 0 and get("vgpr_count") <= 64, name
