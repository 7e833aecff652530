"""GPU: a data file compacted on the device (K16, hbx_datfile_compact_device /
_path: the plan, the moved stream packed by destination tiles, the meta and
index records) against the pure-Python restatement of CompactFile in
tests/compact_craft.py: every output of every case must be equal byte for
byte, at tiles of 256, 4,096 and 65,536 bytes.  The largest case moves one
entry of 8 MiB."""
import ctypes
import os

import numpy as np
import pytest

from hashbox_amd import CompactLimitError, DatCompact, Engine, HbxError, _lib
from . import compact_craft as C
from . import datfile_craft as D
from .test_compact_craft import make_args, summary_dict
from .test_gpu_graph import _datfiles, store  # noqa: F401  (the stored tree of the block graph's end-to-end test)

pytestmark = pytest.mark.gpu

CORPUS = C.corpus(_lib.GRAPH_LANE_MAX, _lib.GRAPH_WAVE_MAX)
REFS = {}
OUTPUTS = ("klass", "new_off", "meta_off", "moved", "meta", "ix")
DEFAULT_TILE = 65536


def ref_of(name):
    if name not in REFS:
        REFS[name] = C.ref(CORPUS[name])
    return REFS[name]


def _first_diff(a: bytes, b: bytes) -> int:
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    n = min(x.size, y.size)
    d = np.flatnonzero(x[:n] != y[:n])
    return int(d[0]) if d.size else n


def compare(name, case, got, want, tile=DEFAULT_TILE, outputs=OUTPUTS, summary=True):
    """got: a dict of the outputs (bytes / lists) and "summary".  A failure
    names case, output, entry, and for a stream's byte its tile, its granule
    and whether that granule straddled two entries."""
    for f in ("klass", "new_off", "meta_off"):
        if f not in outputs:
            continue
        g, w = [int(x) for x in got[f]], want[f]
        assert len(g) == len(w), f"case {name}: {f} has {len(g)} entries, expected {len(w)}"
        for i, (a, b) in enumerate(zip(g, w)):
            if a != b:
                pytest.fail(f"case {name}: output {f}, entry {i}: expected {b}, got {a}")
    kept = [i for i, k in enumerate(want["klass"]) if k != C.DROP]
    if "moved" in outputs and bytes(got["moved"]) != want["moved"]:
        at = _first_diff(bytes(got["moved"]), want["moved"])
        gr = {s: (i, across) for s, i, across in C.granules(case, want)}
        i, across = gr.get(at - at % 16, (None, None))
        pytest.fail(f"case {name}: output moved, byte {at} of {len(want['moved'])} (got {len(got['moved'])} bytes): "
                    f"entry {i}, tile {at // tile} of {tile} bytes, granule {at // 16}, "
                    f"{'straddles two entries' if across else 'inside one entry'}")
    if "meta" in outputs and bytes(got["meta"]) != want["meta"]:
        at = _first_diff(bytes(got["meta"]), want["meta"])
        base = case.kw.get("meta_base", 16)
        i = max([k for k in kept if want["meta_off"][k] - base <= at], default=None)
        pytest.fail(f"case {name}: output meta, byte {at} of {len(want['meta'])} (got {len(got['meta'])} bytes): "
                    f"entry {i}, byte {at - (want['meta_off'][i] - base) if i is not None else at} of its record")
    if "ix" in outputs and bytes(got["ix"]) != want["ix"]:
        at = _first_diff(bytes(got["ix"]), want["ix"])
        pytest.fail(f"case {name}: output ix, byte {at}: record {at // 24} (entry {kept[at // 24] if at // 24 < len(kept) else None}), "
                    f"byte {at % 24} of it")
    if summary:
        for k in C.SUMMARY_FIELDS:
            assert got["summary"][k] == want["summary"][k], \
                f"case {name}: summary {k} expected {want['summary'][k]}, got {got['summary'][k]}"


def as_dict(r: DatCompact) -> dict:
    return dict(klass=r.klass.tolist(), new_off=r.new_off.tolist(), meta_off=r.meta_off.tolist(), moved=r.moved,
                meta=r.meta, ix=None if r.ix is None else r.ix.tobytes(), summary=r.summary)


def run(eng, case, **kw) -> DatCompact:
    return eng.compact_datfile(case.buf, _entries_array(case), case.keep, **{**case.kw, **kw})


def _entries_array(case):
    from hashbox_amd.engine import DAT_ENTRY_DTYPE
    e = np.zeros(len(case.entries), DAT_ENTRY_DTYPE)
    for i, x in enumerate(case.entries):
        e[i]["off"], e[i]["size"], e[i]["n_links"], e[i]["data_len"] = x["off"], x["size"], x["n_links"], x["data_len"]
        e[i]["data_off"], e[i]["type"] = x["off"] + 29 + 16 * x["n_links"], x.get("type", D.RAW)
        e[i]["id"] = np.frombuffer(x["id"], np.uint8)
    return e


def raw(eng, case, absent=(), short=None, path=None):
    """The C call: outputs in `absent` are NULL with capacity 0; `short` names
    a stream whose capacity is one byte less than it needs.  Returns (rc, dict);
    every array is filled with 7 before the call."""
    want = ref_of(case.name)
    n = len(case.entries)
    s = want["summary"]
    sizes = dict(moved=s["moved_bytes"], meta=s["meta_bytes"], ix=24 * s["n_meta"])
    arr = dict(klass=np.full(n + 1, 7, np.uint8), new_off=np.full(n + 1, 7, np.uint64), meta_off=np.full(n + 1, 7, np.uint64))
    buf = {k: np.full(v + 16, 7, np.uint8) for k, v in sizes.items()}
    cap = {k: (v - 1 if k == short else v) for k, v in sizes.items()}
    p = lambda k, a: None if k in absent else a.ctypes.data  # noqa: E731
    ent = C.c_entries(case.entries, _lib.DatEntry)
    kp = np.array([1 if k else 0 for k in case.keep] + [0], np.uint8)
    args, sm = make_args(case.kw), _lib.DatCompactSummary()
    tail = [n, ent, kp.ctypes.data, ctypes.byref(args), p("klass", arr["klass"]), p("new_off", arr["new_off"]),
            p("meta_off", arr["meta_off"])]
    for k in ("moved", "meta", "ix"):
        tail += [p(k, buf[k]), 0 if k in absent else cap[k]]
    tail.append(ctypes.byref(sm))
    if path is not None:
        rc = eng._L.hbx_datfile_compact_path(eng._ctx, os.fsencode(path), *tail)
    else:
        d, size, _path, arena = eng._dat_image(case.buf, None)
        try:
            rc = eng._L.hbx_datfile_compact_device(eng._ctx, d, size, *tail)
        finally:
            eng._L.hbx_arena_free(eng._ctx, arena)
    out = {k: v[:n].tolist() for k, v in arr.items()}
    out.update({k: v[:sizes[k]].tobytes() for k, v in buf.items()})
    out["summary"] = summary_dict(sm)
    out["_raw"] = {**arr, **buf}
    return rc, out


@pytest.fixture(scope="module", params=C.TILES, ids=[f"tile-{t}" for t in C.TILES])
def tile_engine(request, engine):
    """The session's engine (the default tile), and engines whose K16 tiles
    are 256 and 4,096 bytes: a small stream then spans many tiles."""
    if request.param == DEFAULT_TILE:
        assert engine.knobs()["k16_tile"] == DEFAULT_TILE
        yield engine, DEFAULT_TILE
        return
    old = {k: os.environ.get(k) for k in ("HBX_AB", "HBX_K16_TILE")}
    os.environ.update(HBX_AB="1", HBX_K16_TILE=str(request.param))
    try:
        eng = Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert eng.knobs()["k16_tile"] == request.param
    yield eng, request.param
    eng.close()


def test_the_tile_knob_needs_ab(engine):
    old = {k: os.environ.pop(k, None) for k in ("HBX_AB", "HBX_K16_TILE")}
    os.environ["HBX_K16_TILE"] = "256"
    try:
        with Engine(0) as e:
            assert e.knobs()["k16_tile"] == DEFAULT_TILE and e.knobs()["ab_env"] == 0
    finally:
        os.environ.pop("HBX_K16_TILE", None)
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_case(tile_engine, name):
    eng, tile = tile_engine
    case, want = CORPUS[name], ref_of(name)
    if want["rc"] == 0:
        r = run(eng, case)
        compare(name, case, as_dict(r), want, tile)
        assert r.stay.tolist() == [k == C.STAY for k in want["klass"]]
        assert r.moved_rows.tolist() == [k == C.MOVE for k in want["klass"]]
        assert r.relocations == want["relocations"]
        return
    # past the 16 GiB limit: the plan and the summary are complete, nothing is packed
    with pytest.raises(CompactLimitError, match="HBX_ERR_CAPACITY") as err:
        run(eng, case)
    assert isinstance(err.value, HbxError) and err.value.first_past_limit == want["summary"]["first_past_limit"]
    plan = err.value.plan  # what a caller cuts the list by
    assert plan.moved is None and plan.meta is None and plan.ix is None
    compare(name, case, as_dict(plan), want, tile, outputs=("klass", "new_off", "meta_off"))
    rc, out = raw(eng, case)
    assert rc == C.ERR_CAPACITY and out["summary"]["first_past_limit"] == want["summary"]["first_past_limit"]
    compare(name, case, out, want, tile, outputs=("klass", "new_off", "meta_off"))
    for k in ("moved", "meta", "ix"):
        assert (out["_raw"][k] == 7).all(), k


def test_path_equals_device(engine, tmp_path):
    for name in ("C_tiles", "F_links", "E_n0"):
        case = CORPUS[name]
        p = tmp_path / f"{name}.dat"
        p.write_bytes(case.buf)
        r = engine.compact_datfile(p, _entries_array(case), case.keep, **case.kw)
        compare(f"{name} by path", case, as_dict(r), ref_of(name))
        compare(f"{name} path against device", case, as_dict(r), as_dict(run(engine, case)))
        rc, out = raw(engine, case, path=p)
        assert rc == 0
        compare(f"{name} by path, C call", case, out, ref_of(name))
    case = CORPUS["C_tiles"]
    rc, _ = raw(engine, case, path=tmp_path / "missing.dat")
    assert rc == _lib.ERR_IO
    short = tmp_path / "short.dat"
    short.write_bytes(case.buf[:-1])  # the last entry ends past this file's size
    assert raw(engine, case, path=short)[0] == C.ERR_ARG
    compare("C_tiles after the errors", case, as_dict(run(engine, case)), ref_of("C_tiles"))


@pytest.mark.parametrize("name", ["A_alignments", "F_links", "E_drop_middle", "E_all_stay", "E_none_kept"])
@pytest.mark.parametrize("absent", OUTPUTS + ("all",))
def test_outputs_not_wanted(engine, name, absent):
    """Each output absent in turn, and all of them: the others and the summary do not change."""
    case, want = CORPUS[name], ref_of(name)
    gone = OUTPUTS if absent == "all" else (absent,)
    rc, out = raw(engine, case, gone)
    assert rc == 0
    compare(f"{name} without {absent}", case, out, want, outputs=[f for f in OUTPUTS if f not in gone])
    for f in gone:
        assert (out["_raw"][f] == 7).all()  # not written
    for f in ("moved", "meta", "ix"):  # nothing behind an output's end either
        assert (out["_raw"][f][len(want[f]):] == 7).all()


@pytest.mark.parametrize("short", ["moved", "meta", "ix"])
def test_capacity_one_byte_short(engine, short):
    case, want = CORPUS["F_links"], ref_of("F_links")
    rc, out = raw(engine, case, short=short)
    assert rc == C.ERR_CAPACITY
    assert "do not fit" in engine._L.hbx_last_error(engine._ctx).decode()
    for k in C.SUMMARY_FIELDS:  # the needed sizes: moved_bytes, meta_bytes, 24 n_meta
        assert out["summary"][k] == want["summary"][k], k
    for f in OUTPUTS:
        assert (out["_raw"][f] == 7).all(), f  # untouched
    compare("F_links afterwards", case, as_dict(run(engine, case)), want)


def test_nine_calls_on_one_context():
    """Small files after large ones: every call finds the leftovers of the one before in the kept buffers."""
    with Engine(0) as e:
        for name in ("D_large", "E_one_move", "B_small", "E_n0", "C_tiles", "E_all_stay", "F_links", "G_dst_base_17",
                     "A_alignments"):
            compare(name, CORPUS[name], as_dict(run(e, CORPUS[name])), ref_of(name))


def test_refused_while_batches_are_pending_then_chunk_hash(oracle):
    import torch
    t = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    case = CORPUS["E_drop_middle"]
    with Engine(0) as e:
        e.submit_device(t.data_ptr(), [0], [1 << 20])
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):
            run(e, case)
        e.wait()
        compare(case.name, case, as_dict(run(e, case)), ref_of(case.name))
        assert e._L.hbx_pending(e._ctx) == 0
        data = oracle.random_bytes(1 << 20, 16)
        got, want = e.chunk_hash(data), oracle.store_file(data, fast=True)
        assert np.array_equal(got.cut_ends, want.cut_ends) and np.array_equal(got.ids, want.ids)
        assert got.content_id == want.content_id
        assert e._L.hbx_pending(e._ctx) == 0


def test_argument_errors_leave_the_context_usable(engine):
    case = CORPUS["E_drop_middle"]
    L, c = engine._L, engine._ctx
    n = len(case.entries)
    ent, kp = C.c_entries(case.entries, _lib.DatEntry), np.ones(n, np.uint8)
    args, sm = make_args({}), _lib.DatCompactSummary()
    d, size, _p, arena = engine._dat_image(case.buf, None)
    try:
        def call(c_=c, d_=d, a_=ctypes.byref(args), sm_=ctypes.byref(sm), moved=(None, 0)):
            return L.hbx_datfile_compact_device(c_, d_, size, n, ent, kp.ctypes.data, a_, None, None, None, *moved,
                                                None, 0, None, 0, sm_)
        assert call() == 0
        assert call(c_=None) == -1 and call(d_=None) == -1 and call(a_=None) == -1 and call(sm_=None) == -1
        assert call(d_=ctypes.c_void_p(d.value + 1)) == -1   # an unaligned image
        assert call(moved=(None, 5)) == -1                   # a capacity without an array
        assert call() == 0
        bad = make_args({"dst_base": 15})
        assert call(a_=ctypes.byref(bad)) == -1
        assert "out of range" in L.hbx_last_error(c).decode()  # (the rejection has a text of its own)
    finally:
        L.hbx_arena_free(c, arena)
    with pytest.raises(ValueError):
        engine.compact_datfile(case.buf, _entries_array(case), case.keep[:-1])
    compare(case.name, case, as_dict(run(engine, case)), ref_of(case.name))


# -------------------------------------------------------------- round trips --
@pytest.fixture(scope="module")
def real_file(engine):
    """A file of real blocks (IDs that verify), some damaged, checked on the device."""
    buf, _offs = D.big_file(seed=16, size=1 << 20, damaged=0.05)
    chk = engine.check_datfile(buf)
    assert chk.summary["n_entries"] > 40 and chk.summary["n_broken"] > 0 and int(chk.entries["n_links"].max()) > 16
    return buf, chk


@pytest.mark.parametrize("share", [0.7, 1.0])
def test_the_moved_stream_is_a_data_file(engine, real_file, share):
    buf, chk = real_file
    n = chk.entries.shape[0]
    keep = np.random.default_rng(16).random(n) < share
    r = engine.compact_datfile(buf, chk.entries, keep, keep_prefix=False, dst_base=16, file_no=3, meta_file_no=5)
    entries = [dict(off=int(e["off"]), size=int(e["size"]), n_links=int(e["n_links"]), data_len=int(e["data_len"]),
                    id=e["id"].tobytes()) for e in chk.entries]
    case = C.Case("real", buf, entries, keep.tolist(), dict(keep_prefix=False, file_no=3, meta_file_no=5))
    compare("real", case, as_dict(r), C.ref(case))
    # header + moved stream: a data file that holds exactly the kept entries at new_off, and no span
    new = D.header() + r.moved
    again = engine.check_datfile(new)
    kept = np.flatnonzero(keep)
    assert again.summary["n_entries"] == kept.size and again.summary["n_spans"] == 0
    assert again.entries["off"].tolist() == r.new_off[kept].tolist()
    assert again.entries["id"].tobytes() == chk.entries["id"][kept].tobytes()
    assert again.entries["size"].tolist() == chk.entries["size"][kept].tolist()
    assert (engine.verify_datfile_at(new, r.new_off[kept], chk.entries["id"][kept]) == 0).all()
    # the meta stream, consumed whole by Unserialize's rules
    metas = C.ref_meta_parse(r.meta)
    assert len(metas) == kept.size
    for m, i in zip(metas, kept):
        e = chk.entries[i]
        assert (m["id"], m["file"], m["off"], m["data_size"]) == (e["id"].tobytes(), 3, int(r.new_off[i]), int(e["size"]))
        assert b"".join(m["links"]) == chk.links[int(e["link_base"]):int(e["link_base"]) + int(e["n_links"])].tobytes()
        assert m["at"] + 16 == int(r.meta_off[i])
    # the index records point at the meta records
    for x, i in zip(r.ix, kept):
        x = x.tobytes()
        assert x[:2] == bytes([0, 1 | (2 if chk.entries[i]["n_links"] == 0 else 0)]) and x[2:18] == chk.entries[i]["id"].tobytes()
        assert C.location_get(x[18:]) == (5, int(r.meta_off[i]))


def test_check_mark_sweep_compact(engine, store):  # noqa: F811
    """check_datfile -> block_table -> block_graph -> gc_keep -> compact_datfile
    per file into new files; checked and graphed again, the new files hold
    the live tree and nothing else."""
    from hashbox_amd import formats as F
    blocks, orphans = store["blocks"], store["orphans"]
    old = _datfiles(store)
    checks = [engine.check_datfile(buf) for buf in old]
    ids, nl, base, links, file_no, _off = F.block_table(checks)
    g = engine.block_graph(ids, nl, links, roots=[store["root"]], link_base=base)
    keeps = F.gc_keep(g, file_no)
    assert len(keeps) == 2 and sum(int(k.sum()) for k in keeps) == len(blocks)
    new, relocated = [], 0
    for f, (buf, chk, keep) in enumerate(zip(old, checks, keeps)):
        r = engine.compact_datfile(buf, chk.entries, keep, file_no=f, dst_file_no=f + 2, keep_prefix=False)
        assert r.summary["n_dropped"] == int((~keep).sum()) > 0 and r.summary["n_moved"] == int(keep.sum())
        assert r.summary["deleted_bytes"] == int(chk.entries["size"][~keep].sum())
        assert [x[1] for x in r.relocations] == [f + 2] * int(keep.sum())
        relocated += len(r.relocations)
        new.append(D.header() + r.moved)
        assert len(C.ref_meta_parse(r.meta)) == int(keep.sum())
    assert relocated == len(blocks)
    checks = [engine.check_datfile(buf) for buf in new]
    assert all(c.summary["n_spans"] == 0 for c in checks)
    ids, nl, base, links, _f, _o = F.block_table(checks)
    assert {ids[i].tobytes() for i in range(ids.shape[0])} == set(blocks)
    g = engine.block_graph(ids, nl, links, roots=[store["root"]], link_base=base)
    assert g.summary["n_marked"] == ids.shape[0] == len(blocks) and g.summary["n_alias"] == 0
    assert g.tree_ok.all() and g.marked.all()
    # a damaged live tree: gc_keep refuses to sweep
    checks = [engine.check_datfile(buf) for buf in _datfiles(store, damaged=store["victim"])]
    ids, nl, base, links, file_no, _o = F.block_table(checks)
    g = engine.block_graph(ids, nl, links, roots=[store["root"]], link_base=base)
    with pytest.raises(ValueError, match="damaged tree"):
        F.gc_keep(g, file_no)
    assert sum(int(k.sum()) for k in F.gc_keep(g, file_no, force=True)) == len(blocks) - 1


def test_a_failure_names_what_differs():
    """The report of compare(): case, output, entry, tile, granule, straddling."""
    case, want = CORPUS["B_small"], ref_of("B_small")
    good = dict(want)
    bad = dict(good, moved=good["moved"][:4120] + bytes([good["moved"][4120] ^ 1]) + good["moved"][4121:])
    with pytest.raises(pytest.fail.Exception) as e:
        compare("B_small", case, bad, want, tile=4096)
    # granule 257 (bytes 4112..4127) starts at byte 23 of the 142nd mover (entry 283) and ends in the 143rd
    assert "case B_small: output moved, byte 4120" in str(e.value) and "entry 283, tile 1 of 4096 bytes" in str(e.value)
    assert "granule 257, straddles two entries" in str(e.value)
    bad = dict(good, moved=good["moved"][:4100] + bytes([good["moved"][4100] ^ 1]) + good["moved"][4101:])
    with pytest.raises(pytest.fail.Exception, match="entry 283, tile 0 of 65536 bytes, granule 256, inside one entry"):
        compare("B_small", case, bad, want)
    bad = dict(good, new_off=good["new_off"][:7] + [5] + good["new_off"][8:])
    with pytest.raises(pytest.fail.Exception, match="case B_small: output new_off, entry 7: expected"):
        compare("B_small", case, bad, want)
    bad = dict(good, meta=good["meta"][:35] + b"\0" + good["meta"][36:])
    with pytest.raises(pytest.fail.Exception, match="output meta, byte 35 .*entry 3, byte 1 of its record"):
        compare("B_small", case, bad, want)
    bad = dict(good, ix=good["ix"][:49] + b"\xff" + good["ix"][50:])
    with pytest.raises(pytest.fail.Exception, match=r"output ix, byte 49: record 2 \(entry 5\), byte 1 of it"):
        compare("B_small", case, bad, want)
