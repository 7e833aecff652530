"""CPU: the plan of a data file compaction on the host
(hbx_datfile_compact_plan, include/hbxgpu.h "Compact a storage data file")
against the pure-Python restatement of CompactFile in tests/compact_craft.py,
what the crafted corpus covers (asserted on the reference), the argument rules,
and formats.gc_keep."""
import ctypes
import os
import re

import numpy as np
import pytest

from hashbox_amd import _lib
from . import compact_craft as C
from . import datfile_craft as D

CORPUS = C.corpus(_lib.GRAPH_LANE_MAX, _lib.GRAPH_WAVE_MAX)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hbxgpu.h")


def make_args(kw) -> _lib.DatCompactArgs:
    f = kw.get("file_no", 0)
    dst = kw.get("dst_file_no")
    return _lib.DatCompactArgs(f, f if dst is None else dst, kw.get("dst_base", 16), kw.get("meta_file_no", 0),
                               _lib.CMP_F_KEEP_PREFIX if kw.get("keep_prefix", True) else 0, kw.get("meta_base", 16))


def summary_dict(sm) -> dict:
    s = {k: int(getattr(sm, k)) for k in C.SUMMARY_FIELDS}
    if s["first_past_limit"] == C.NEVER:
        s["first_past_limit"] = None
    return s


def plan(size, entries, keep, kw):
    """hbx_datfile_compact_plan: (rc, klass, new_off, meta_off, summary)."""
    n = len(entries)
    ent = C.c_entries(entries, _lib.DatEntry)
    kp = np.array([1 if k else 0 for k in keep] + [0], np.uint8)
    klass, no, mo = np.full(n + 1, 9, np.uint8), np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    sm = _lib.DatCompactSummary()
    args = make_args(kw)
    rc = _lib.load().hbx_datfile_compact_plan(size, n, ent, kp.ctypes.data, ctypes.byref(args), klass.ctypes.data,
                                              no.ctypes.data, mo.ctypes.data, ctypes.byref(sm))
    return rc, klass[:n].tolist(), no[:n].tolist(), mo[:n].tolist(), summary_dict(sm)


def check_plan(name, got, want):
    rc, klass, no, mo, sm = got
    assert rc == want["rc"], f"{name}: rc {rc}, expected {want['rc']}"
    for what, g, w in (("klass", klass, want["klass"]), ("new_off", no, want["new_off"]), ("meta_off", mo, want["meta_off"])):
        assert len(g) == len(w)
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"case {name}: {what}[{i}] expected {b}, got {a}"
    for k in C.SUMMARY_FIELDS:
        assert sm[k] == want["summary"][k], f"case {name}: summary {k} expected {want['summary'][k]}, got {sm[k]}"


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_plan_equals_the_reference(name):
    case = CORPUS[name]
    want = C.ref(case)
    check_plan(name, plan(case.size, case.entries, case.keep, case.kw), want)
    s = want["summary"]
    assert s["n_stay"] + s["n_moved"] + s["n_dropped"] == s["n_entries"] == len(case.entries)
    if not case.broken:
        assert s["deleted_bytes"] == want["deleted"], name  # the reference's `deleted` (gc.go:248, 260, 263, 317)
    if want["rc"] == 0:
        assert len(want["moved"]) == s["moved_bytes"] and len(want["meta"]) == s["meta_bytes"]
        assert len(want["ix"]) == 24 * s["n_meta"]
        got = C.ref_meta_parse(want["meta"])
        kept = [i for i, k in enumerate(want["klass"]) if k != C.DROP]
        assert [m["at"] + case.kw.get("meta_base", 16) for m in got] == [want["meta_off"][i] for i in kept]
        assert [(m["id"], m["off"], m["data_size"]) for m in got] == \
            [(case.entries[i]["id"], want["new_off"][i], case.entries[i]["size"]) for i in kept]


def test_plan_on_seeded_keep_masks():
    buf, _offs = D.big_file()
    entries = D.ref_check(buf, 8 << 20)["entries"]
    assert len(entries) > 200 and len(buf) > 7 << 20
    n = 0
    for keep, prefix in C.keep_masks(len(entries), 300):
        kw = dict(keep_prefix=prefix, dst_base=16 + 1000 * n, meta_base=16 + n, dst_file_no=n % 7)
        want = C.ref_compact(buf, entries, keep, streams=False, **kw)
        check_plan(f"mask {n}", plan(len(buf), entries, keep, kw), want)
        n += 1
    assert n == 300


def test_corpus_covers_what_it_claims():
    # A: every pair (source offset mod 16, destination offset mod 16) with a granule inside the entry; and the
    # two roles a mover can have in a straddling granule counted apart: the entry the granule STARTS in (all 256
    # pairs) and the entry it ENDS in (the 240 pairs whose destination is not 0 mod 16: a mover at 0 starts a granule)
    case = CORPUS["A_alignments"]
    r = C.ref(case)
    inside, starts_in, ends_in = set(), set(), set()
    pair = lambda i: (case.entries[i]["off"] % 16, r["new_off"][i] % 16)  # noqa: E731
    movers = [i for i, k in enumerate(r["klass"]) if k == C.MOVE]
    nxt = dict(zip(movers, movers[1:]))
    for _s, i, across in C.granules(case, r):
        if across:
            starts_in.add(pair(i))
            ends_in.add(pair(nxt[i]))
        else:
            inside.add(pair(i))
    assert min(case.entries[i]["size"] for i in movers) >= 29 and sum(case.entries[i]["size"] >= 48 for i in movers) >= 256
    every = {(a, b) for a in range(16) for b in range(16)}
    assert inside == every and starts_in == every
    assert ends_in == {(a, b) for a, b in every if b != 0}
    # B: 29-byte entries: a granule lies inside one only if it starts in its first 14 bytes, so more than half
    # of them straddle; 2,259 entries per default tile
    case = CORPUS["B_small"]
    r = C.ref(case)
    assert r["summary"]["n_moved"] == 2500 and all(e["size"] == 29 for e in case.entries)
    g = C.granules(case, r)
    assert sum(1 for x in g if not x[2]) <= len(g) // 2 and 65536 // 29 == 2259 and r["summary"]["moved_bytes"] > 65536
    # C: tile edges
    case = CORPUS["C_tiles"]
    r = C.ref(case)
    ends = [(r["new_off"][i] - 16, r["new_off"][i] - 16 + case.entries[i]["size"], case.entries[i]["size"])
            for i, k in enumerate(r["klass"]) if k == C.MOVE]
    for T in C.TILES:
        for d in (-1, 0, 1):
            assert any(e % T == d % T for _a, e, _s in ends), (T, d)
    assert any(s == 1024 and (e - 1) // 256 - a // 256 >= 3 for a, e, s in ends)
    assert any(s == 200 * 1024 + 7 and (e - 1) // 65536 - a // 65536 >= 3 for a, e, s in ends)
    assert r["summary"]["moved_bytes"] % 16 != 0  # the last granule is partial
    # D: 8 MiB of data from 5 mod 16 to 11 mod 16
    case = CORPUS["D_large"]
    r = C.ref(case)
    assert case.entries[2]["data_len"] == 8 << 20 and case.entries[2]["off"] % 16 == 5 and r["new_off"][2] % 16 == 11
    # F: both sides of both degree thresholds, staying and moved, at several source alignments
    case = CORPUS["F_links"]
    r = C.ref(case)
    for n in C.LINK_COUNTS:
        rows = [i for i, e in enumerate(case.entries) if e["n_links"] == n and r["klass"][i] != C.DROP]
        assert {r["klass"][i] for i in rows} == {C.STAY, C.MOVE}
        assert len({case.entries[i]["off"] % 16 for i in rows}) >= 3, n
    assert {_lib.GRAPH_LANE_MAX, _lib.GRAPH_LANE_MAX + 1} <= set(C.LINK_COUNTS)
    assert min(x for x in C.LINK_COUNTS if x > _lib.GRAPH_LANE_MAX + 1) <= _lib.GRAPH_WAVE_MAX < max(C.LINK_COUNTS)
    # G: the limit from both sides, for both bases
    for what in ("dst", "meta"):
        at, past = C.ref(CORPUS[f"G_{what}_at_limit"]), C.ref(CORPUS[f"G_{what}_past_limit"])
        assert at["rc"] == 0 and past["rc"] == C.ERR_CAPACITY and past["summary"]["first_past_limit"] == 4
        assert max(at["new_off"][4], at["meta_off"][4]) == C.LIMIT
        assert max(past["new_off"][4], past["meta_off"][4]) == C.LIMIT + 1
    files = {C.location_get(m[20:26])[0] for m in [C.ref(CORPUS["G_files_16383"])["meta"]]}
    assert files == {C.FILE_MAX}  # (the first record's: the stayer in file 0x3fff)
    total = sum(c.size for c in CORPUS.values())
    assert 8 << 20 < total < 14 << 20  # (the 8 MiB entry and about a megabyte of everything else)


def test_struct_sizes_and_constants_match_the_header():
    text = open(HEADER).read()
    assert ctypes.sizeof(_lib.DatCompactArgs) == 32 and ctypes.sizeof(_lib.DatCompactSummary) == 88
    assert re.search(r"\} hbx_dat_compact_args;\s*/\* 32 bytes \*/", text)
    assert re.search(r"\} hbx_dat_compact_summary;\s*/\* 88 bytes \*/", text)

    def define(name):
        m = re.search(rf"#define {name} (0x[0-9A-Fa-f]+|\d+)u?(ll)?\b", text)
        assert m, name
        return int(m.group(1), 0)
    assert define("HBX_DAT_OFFSET_LIMIT") == _lib.DAT_OFFSET_LIMIT == C.LIMIT == (1 << 34) - 1
    assert define("HBX_DAT_FILE_MAX") == _lib.DAT_FILE_MAX == C.FILE_MAX
    assert (define("HBX_CMP_DROP"), define("HBX_CMP_STAY"), define("HBX_CMP_MOVE")) == \
        (_lib.CMP_DROP, _lib.CMP_STAY, _lib.CMP_MOVE) == (C.DROP, C.STAY, C.MOVE)
    assert define("HBX_CMP_F_KEEP_PREFIX") == _lib.CMP_F_KEEP_PREFIX == 1
    assert (define("HBX_IX_F_EXISTS"), define("HBX_IX_F_NOLINKS")) == (_lib.IX_F_EXISTS, _lib.IX_F_NOLINKS) == (1, 2)
    assert (define("HBX_META_HEAD"), define("HBX_IX_ENTRY")) == (_lib.META_HEAD, _lib.IX_ENTRY) == (34, 24)
    fields = re.search(r"typedef struct \{([^}]*)\} hbx_dat_compact_summary;", text).group(1)
    assert re.findall(r"\b([a-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields)) == list(C.SUMMARY_FIELDS)
    assert [k for k, _ in _lib.DatCompactSummary._fields_] == list(C.SUMMARY_FIELDS)


def test_argument_rules():
    case = CORPUS["G_files_0"]
    size, ent, keep = case.size, case.entries, case.keep
    ok = lambda entries=ent, kw=case.kw, size_=size, keep_=keep: plan(size_, entries, keep_, kw)[0]  # noqa: E731
    assert ok() == 0

    def changed(i, **f):
        out = [dict(e) for e in ent]
        out[i].update(f)
        return out
    assert ok(entries=[ent[1], ent[0]] + ent[2:]) == C.ERR_ARG                        # do not ascend
    assert ok(entries=changed(1, off=ent[1]["off"] - 1)) == C.ERR_ARG                  # overlap
    assert ok(entries=changed(0, off=15)) == C.ERR_ARG                                 # starts inside the header
    assert ok(size_=size - 1) == C.ERR_ARG                                             # ends past size
    assert ok(entries=changed(4, off=size)) == C.ERR_ARG
    assert ok(entries=changed(2, data_len=ent[2]["data_len"] + 1)) == C.ERR_ARG        # size != 29 + 16 n + len
    assert ok(entries=changed(2, n_links=ent[2]["n_links"] + 1)) == C.ERR_ARG
    assert ok(entries=changed(2, size=ent[2]["size"] - 1)) == C.ERR_ARG
    # a size above 2^32 - 1 (DataSize is a uint32): 2^28 - 1 links make 2^32 + 13 bytes, one link fewer 2^32 - 3
    far = [dict(ent[0], n_links=(1 << 28) - 1, data_len=0, size=(1 << 32) + 13)]
    assert plan((1 << 33), far, [True], {})[0] == C.ERR_ARG
    fits = [dict(ent[0], n_links=(1 << 28) - 2, data_len=0, size=(1 << 32) - 3)]
    assert plan((1 << 33), fits, [True], {})[0] == 0
    for key in ("file_no", "dst_file_no", "meta_file_no"):
        assert ok(kw={key: 0x4000}) == C.ERR_ARG and ok(kw={key: 0x3FFF}) == 0
    for key in ("dst_base", "meta_base"):
        assert ok(kw={key: 15}) == C.ERR_ARG and ok(kw={key: 16}) == 0
        assert ok(kw={key: (1 << 64) - 1}) == C.ERR_ARG
    # NULL arguments
    L = _lib.load()
    e, kp = C.c_entries(ent, _lib.DatEntry), np.ones(len(ent), np.uint8)
    sm, a = _lib.DatCompactSummary(), make_args({})
    tail = (None, None, None)
    assert L.hbx_datfile_compact_plan(size, len(ent), e, kp.ctypes.data, ctypes.byref(a), *tail, ctypes.byref(sm)) == 0
    assert L.hbx_datfile_compact_plan(size, len(ent), e, kp.ctypes.data, ctypes.byref(a), *tail, None) == C.ERR_ARG
    assert L.hbx_datfile_compact_plan(size, len(ent), e, kp.ctypes.data, None, *tail, ctypes.byref(sm)) == C.ERR_ARG
    assert L.hbx_datfile_compact_plan(size, len(ent), None, kp.ctypes.data, ctypes.byref(a), *tail, ctypes.byref(sm)) == C.ERR_ARG
    assert L.hbx_datfile_compact_plan(size, len(ent), e, None, ctypes.byref(a), *tail, ctypes.byref(sm)) == C.ERR_ARG
    assert L.hbx_datfile_compact_plan(size, 1 << 31, e, kp.ctypes.data, ctypes.byref(a), *tail, ctypes.byref(sm)) == C.ERR_ARG
    assert L.hbx_datfile_compact_plan(size, 0, None, None, ctypes.byref(a), *tail, ctypes.byref(sm)) == 0
    assert summary_dict(sm)["deleted_bytes"] == size - 16 and sm.stay_end == 16


def test_reference_serialisers():
    """The reference against bytes worked out by hand from the Go source."""
    assert C.six_byte_location(0, 16).hex() == "000000000010"
    assert C.six_byte_location(1, 0).hex() == "000400000000"        # 1 << 34
    assert C.six_byte_location(0x3FFF, C.LIMIT).hex() == "ffffffffffff"
    assert C.location_get(C.six_byte_location(77, 12345678901)) == (77, 12345678901)
    with pytest.raises(C.PastLimit):
        C.six_byte_location(0, C.LIMIT + 1)
    bid = bytes(range(16))
    m = C.meta_entry(bid, 2, 0x123, 1000, [b"L" * 16])
    assert m == b"hblk" + bid + bytes.fromhex("000800000123") + bytes.fromhex("000003e8") + bytes.fromhex("00000001") + b"L" * 16
    assert C.ix_entry(3, bid, 0, 16) == bytes.fromhex("0003") + bid + bytes.fromhex("000000000010")
    assert C.ref_meta_parse(m + m)[1] == dict(id=bid, file=2, off=0x123, data_size=1000, at=50, links=[b"L" * 16])
    for bad in (m[:-1], b"hblx" + m[4:], m + b"h"):
        with pytest.raises(ValueError):
            C.ref_meta_parse(bad)


def test_gc_keep_on_a_hand_made_graph():
    from hashbox_amd import BlockGraph, GRAPH_NONE, formats as F
    N = GRAPH_NONE
    # rows 0..5: file 0 holds rows 0, 1, 2, file 2 rows 3, 4, 5 (file 1 holds no good entry); row 4 is an alias of row 1
    rep = np.array([0, 1, 2, 3, 1, 5], np.uint32)
    mark = np.array([0, 1, N, N, 1, 2], np.uint32)
    g = BlockGraph(rep, np.zeros(0, np.uint32), np.zeros(0, np.uint32), mark, np.full(6, N, np.uint32),
                   {"n_marked_faulty": 0})
    file_no = np.array([0, 0, 0, 2, 2, 2], np.uint32)
    keep = F.gc_keep(g, file_no)
    assert [k.tolist() for k in keep] == [[True, True, False], [], [False, False, True]]
    assert all(k.dtype == bool for k in keep)
    g.summary["n_marked_faulty"] = 2
    with pytest.raises(ValueError, match="2 marked blocks"):
        F.gc_keep(g, file_no)
    assert [k.tolist() for k in F.gc_keep(g, file_no, force=True)] == [k.tolist() for k in keep]
    with pytest.raises(ValueError):
        F.gc_keep(g, file_no[:-1], force=True)
    empty = BlockGraph(*(np.zeros(0, np.uint32),) * 5, {"n_marked_faulty": 0})
    assert F.gc_keep(empty, np.zeros(0, np.uint32)) == []
