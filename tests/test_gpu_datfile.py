"""GPU: a storage data file checked on the device (K14 scan and parse, K8 / K8s
inflate and K6 VerifyBlock in place; hbx_datfile_check_device / _path,
hbx_datfile_verify_at) against the pure-Python reference of
tests/datfile_craft.py: entries, spans, summary and links must be equal,
field by field.  Images of at most 8 MiB, max_block 1 MiB."""
import ctypes
import os

import numpy as np
import pytest

from hashbox_amd import Engine, HbxError, _lib
from . import datfile_craft as C

pytestmark = pytest.mark.gpu

MB = 1 << 20
SCAN = C.scan_cases()
SMALL = C.small_files()
PARSE = C.parse_cases(MB)
VERIFY = C.verify_cases()
WALK = C.walk_cases()
_refs = {}


def _ref(buf: bytes):
    key = (len(buf), hash(buf))
    if key not in _refs:
        _refs[key] = C.ref_check(buf, MB)
    return _refs[key]


def _assert_equal(res, ref):
    s = ref["summary"]
    assert res.summary == s, {k: (res.summary[k], s[k]) for k in s if res.summary[k] != s[k]}
    got_e = [dict(off=int(e["off"]), size=int(e["size"]), data_off=int(e["data_off"]), link_base=int(e["link_base"]),
                  n_links=int(e["n_links"]), data_len=int(e["data_len"]), plain_len=int(e["plain_len"]),
                  type=int(e["type"]), id=e["id"].tobytes()) for e in res.entries]
    assert got_e == ref["entries"]
    got_s = [dict(off=int(x["off"]), len=int(x["len"]), kind=int(x["kind"]), status=int(x["status"]),
                  n_failed=int(x["n_failed"])) for x in res.spans]
    assert got_s == ref["spans"]
    assert res.links.tobytes() == ref["links"]
    assert C.invariant(res.summary)


def _check(eng, buf: bytes, **kw):
    res = eng.check_datfile(buf, max_block=MB, **kw)
    _assert_equal(res, _ref(buf))
    return res


@pytest.fixture(scope="module", params=[0, 1, 2], ids=["grid-default", "grid-1", "grid-2"])
def scan_engine(request, engine):
    """The session's engine, and engines whose K14 grid is one and two
    workgroups: a 64 KiB image then takes 16 and 8 grid-stride rounds."""
    if request.param == 0:
        yield engine
        return
    old = {k: os.environ.get(k) for k in ("HBX_AB", "HBX_K14_WGS")}
    os.environ.update(HBX_AB="1", HBX_K14_WGS=str(request.param))
    try:
        eng = Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert eng.knobs()["k14_wgs"] == request.param
    yield eng
    eng.close()


def test_knob_needs_ab(engine):
    assert engine.knobs()["k14_wgs"] == 0


@pytest.mark.parametrize("name", sorted(SCAN))
def test_scan(scan_engine, name):
    """Entries of 29 bytes at every alignment mod 16 and across the borders of
    a lane's 16 bytes, a wave's 1 KiB, a workgroup's 4 KiB and the grid-stride
    rounds; a marker at 16, in the last 4 bytes and cut by the end; overlapping
    text; 1,024 markers in 4 KiB from one workgroup."""
    res = _check(scan_engine, SCAN[name])
    if name == "run4k":
        assert res.summary["n_candidates"] == 1024 and int(res.spans[0]["n_failed"]) == 1024
    if name == "align":
        assert sorted(int(o) % 16 for o in res.entries["off"]) == list(range(16))


def _raw_check(eng, d, size, max_candidates=0, entry_cap=4096, span_cap=4096, link_cap=4096):
    ents, spans = (_lib.DatEntry * max(entry_cap, 1))(), (_lib.DatSpan * max(span_cap, 1))()
    links = np.zeros((max(link_cap, 1), 16), np.uint8)
    sm = _lib.DatSummary()
    rc = eng._L.hbx_datfile_check_device(eng._ctx, d, size, MB, max_candidates, 0, ents, entry_cap, spans, span_cap,
                                         links.ctypes.data, link_cap, ctypes.byref(sm))
    return rc, ents, spans, sm


def test_candidate_capacity_one_too_small(scan_engine):
    buf = SCAN["run4k"]
    d, n, _, arena = scan_engine._dat_image(buf, None)
    try:
        rc, _, _, sm = _raw_check(scan_engine, d, n, max_candidates=1023)
        assert rc == _lib.ERR_CAPACITY and sm.n_candidates == 1024 and sm.n_entries == 0
        rc, _, _, sm = _raw_check(scan_engine, d, n, max_candidates=1024)
        assert rc == 0 and sm.n_candidates == 1024 and sm.n_broken == 1
        # the context is usable after the failure, and output capacities report what is needed
        good = WALK["all_good"]
    finally:
        scan_engine._L.hbx_arena_free(scan_engine._ctx, arena)
    d, n, _, arena = scan_engine._dat_image(good, None)
    try:
        ref = _ref(good)["summary"]
        rc, ents, _, sm = _raw_check(scan_engine, d, n, entry_cap=5)
        assert rc == _lib.ERR_CAPACITY and (sm.n_entries, sm.n_links) == (ref["n_entries"], ref["n_links"])
        assert [e.off for e in ents[:5]] == [e["off"] for e in _ref(good)["entries"][:5]]
        rc, _, _, sm = _raw_check(scan_engine, d, n, link_cap=ref["n_links"] - 1)
        assert rc == _lib.ERR_CAPACITY and sm.n_links == ref["n_links"]
        rc, _, _, sm = _raw_check(scan_engine, d, n, link_cap=ref["n_links"])
        assert rc == 0
    finally:
        scan_engine._L.hbx_arena_free(scan_engine._ctx, arena)


def test_bytes_behind_size_decide_nothing(scan_engine):
    """The image is longer than the file says: a 'k' right behind `size`
    completes no marker, and an entry cut by `size` is cut although its bytes
    are there."""
    S = 65536
    cut = SCAN["size-3"]
    whole, offs = C.write_datfile([([], C.text(300, "b0"), C.RAW, None), (C.links_of(1, "b1"), b"12345", C.RAW, None)])
    for image, sizes in ((cut + b"k" + bytes(63), [S]), (whole + C.rnd(64, "slack"), range(offs[1] + 1, len(whole) + 1))):
        d, _, _, arena = scan_engine._dat_image(image, None)
        try:
            for size in sizes:
                res = scan_engine.check_datfile(d.value, max_block=MB, size=size)
                _assert_equal(res, _ref(image[:size]))
        finally:
            scan_engine._L.hbx_arena_free(scan_engine._ctx, arena)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_files(engine, name):
    """The header alone (right, wrong, cut) and files of 17..48 bytes."""
    _check(engine, SMALL[name])


@pytest.mark.parametrize("name", sorted(PARSE))
def test_parse(engine, name):
    """n_links 0, 1, 4 and 2^32 - 1; data_len one past the end; an entry ending
    at the end; the end inside every field; DataType 0 and 2; data_len at and
    one above hbx_restore_in_bound(max_block)."""
    _check(engine, PARSE[name])


@pytest.mark.parametrize("name", sorted(VERIFY))
def test_verify(engine, name):
    """Raw and zlib, with and without links, empty data; one flipped byte in a
    zlib stream, a raw block, an ID, a link."""
    _check(engine, VERIFY[name])
    if name == "good":  # 64 KiB of zeros outgrew min(max_block, 8 len + 4096) and was inflated again
        assert engine.knobs()["datfile"][1] >= 1


@pytest.mark.parametrize("name", sorted(WALK))
def test_walk(engine, name):
    res = _check(engine, WALK[name])
    if name == "nested_good":
        assert res.summary["n_unreached"] == 1 and res.summary["n_entries"] == 3
    if name == "nested_outer_bad":
        assert res.summary["n_unreached"] == 0 and int(res.spans[0]["len"]) == 29
    if name == "gap_past_eof":
        assert res.summary["gap_past_eof"] == 1


def test_windows_change_nothing(engine):
    """A window of 64 KiB of slots: many windows, the same result."""
    buf = WALK["all_good"] + VERIFY["good"][16:]
    _check(engine, buf)
    one = engine.knobs()["datfile"][0]
    _check(engine, buf, window_bytes=65536)
    assert engine.knobs()["datfile"][0] > one


def test_verify_at(engine, tmp_path):
    buf, offs = C.write_datfile([([], C.text(900, "m0"), C.RAW, None), (C.links_of(2, "m1"), C.text(5000, "m1"), C.ZLIB, None),
                                 ([], C.text(700, "m2"), C.ZLIB, "data"), (C.links_of(1, "m3"), C.text(300, "m3"), C.RAW, "link"),
                                 ([], C.text(100, "m4"), C.RAW, "id"), ([], C.text(100, "m5"), C.RAW, "type2")])
    ids = [buf[o + 4:o + 20] for o in offs]
    true4 = C.block_id(C.text(100, "m4"))
    at = offs + [offs[1] + 1, offs[0] - 1, offs[1], len(buf) - 3, len(buf) + 100, offs[4]]
    want = ids + [ids[1], ids[0], ids[0], ids[0], ids[0], true4]
    p = tmp_path / "b.dat"
    p.write_bytes(buf)
    for content in (True, False):
        ref = C.ref_verify_at(buf, at, want, content, MB)
        assert ref == ([0, 0, 1, 7, 7, 9, 9, 9, 10, 9, 9, 10] if content else [0, 0, 0, 0, 0, 9, 9, 9, 10, 9, 9, 10])
        assert engine.verify_datfile_at(buf, at, want, content=content, max_block=MB).tolist() == ref
        assert engine.verify_datfile_at(str(p), at, want, content=content, max_block=MB).tolist() == ref
    assert engine.verify_datfile_at(buf, [], []).tolist() == []


def test_errors_leave_the_context_usable(engine, tmp_path):
    sm = _lib.DatSummary()
    L = engine._L
    missing = os.fsencode(tmp_path / "missing.dat")
    assert L.hbx_datfile_check_path(engine._ctx, missing, MB, 0, 0, None, 0, None, 0, None, 0, ctypes.byref(sm)) == _lib.ERR_IO
    assert b"missing.dat" in L.hbx_last_error(engine._ctx)
    with pytest.raises(HbxError):
        engine.verify_datfile_at(str(tmp_path / "missing.dat"), [16], [bytes(16)])
    d, n, _, arena = engine._dat_image(WALK["all_good"], None)
    try:
        assert L.hbx_datfile_check_device(engine._ctx, d.value + 1, n - 1, MB, 0, 0, None, 0, None, 0, None, 0,
                                          ctypes.byref(sm)) == -1  # unaligned image
        assert L.hbx_datfile_check_device(engine._ctx, d, n, (1 << 30) + 1, 0, 0, None, 0, None, 0, None, 0,
                                          ctypes.byref(sm)) == -1
    finally:
        L.hbx_arena_free(engine._ctx, arena)
    _check(engine, WALK["two_failures"])


def test_refused_while_batches_are_pending():
    import torch
    t = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    with Engine(0) as e:
        e.submit_device(t.data_ptr(), [0], [1 << 20])
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):
            e.check_datfile(WALK["all_good"], max_block=MB)
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):
            e.verify_datfile_at(WALK["all_good"], [16], [bytes(16)])
        e.wait()
        _check(e, WALK["all_good"])


def test_path_and_device_agree_on_8mib_and_the_engine_goes_on(engine, oracle, tmp_path):
    """One file of 8 MiB, several hundred entries, about 3 % damaged, with
    gaps: from a path and device-resident; then a plain chunk_hash on the same
    context, nothing pending."""
    buf, _ = C.big_file()
    assert 7 << 20 <= len(buf) <= 8 << 20
    ref = C.ref_check(buf, MB)
    assert ref["summary"]["n_entries"] > 300 and ref["summary"]["n_broken"] > 3 and ref["summary"]["n_gaps"] > 3
    p = tmp_path / "big.dat"
    p.write_bytes(buf)
    a = engine.check_datfile(str(p), max_block=MB)
    b = engine.check_datfile(buf, max_block=MB)
    c = engine.check_datfile(buf, max_block=MB, window_bytes=2 << 20, links=False)
    for res in (a, b):
        _assert_equal(res, ref)
    assert c.links is None and c.summary == ref["summary"] and np.array_equal(c.entries, a.entries)
    assert np.array_equal(a.entries, b.entries) and np.array_equal(a.spans, b.spans) and np.array_equal(a.links, b.links)
    at = [e["off"] for e in ref["entries"]]
    assert not engine.verify_datfile_at(str(p), at, [e["id"] for e in ref["entries"]], max_block=MB).any()
    assert engine._L.hbx_pending(engine._ctx) == 0
    data = oracle.random_bytes(1 << 20, 5)
    got, want = engine.chunk_hash(data), oracle.store_file(data, fast=True)
    assert np.array_equal(got.cut_ends, want.cut_ends) and np.array_equal(got.ids, want.ids)
    assert got.content_id == want.content_id
    assert engine._L.hbx_pending(engine._ctx) == 0
