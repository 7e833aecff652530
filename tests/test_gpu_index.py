"""GPU: the index files as a device-resident object (K17, hbx_index_*): the
cases of tests/test_index_craft.py through the handle, against the pure-Python
restatement in tests/index_craft.py, every image byte for byte and every output
word for word; the argument, state and capacity errors; the files read from
disk; and gc_sweep behind a block graph."""
import ctypes

import numpy as np
import pytest

from hashbox_amd import Engine, HbxError, IndexSweepError, _lib, formats
from hashbox_amd.engine import IX_KILLED_DTYPE, IX_LIVE_DTYPE
from . import index_craft as C
from . import test_index_craft as T

pytestmark = pytest.mark.gpu

CODES = {v: k for k, v in _lib.ERRORS.items()}


def code_of(ex) -> int:
    return next(c for name, c in CODES.items() if name in str(ex))


class GpuIndex:
    """hashbox_amd.Index behind the interface of test_index_craft.HostIndex."""

    def __init__(self, eng, files):
        self.ix = eng.open_index([bytes(f) for f in files])

    def images(self):
        return [self.ix.export(k) for k in range(self.ix.n_files)]

    def lookup(self, ids, stop_on_free):
        return 0, T.hits_list(self.ix.lookup(ids, stop_on_free))

    def scan(self):
        r = self.ix.scan()
        per = [dict(p, first_misplaced=C.NONE if p["first_misplaced"] is None else p["first_misplaced"]) for p in r.per_file]
        return 0, T.live_list(r.live), per, r.summary

    def mark(self, ids):
        found = self.ix.mark(ids)
        return 0, found.astype(np.uint8).tolist(), int((~found).sum())

    def update(self, recs):
        try:
            return 0, self.ix.update(np.frombuffer(b"".join(recs), np.uint8)).tolist()
        except HbxError as ex:
            return code_of(ex), None

    def sweep(self):
        try:
            r, rc = self.ix.sweep(), 0
        except IndexSweepError as ex:
            r, rc = ex.sweep, C.ERR_FORMAT
        sm = dict(r.summary, first_abort=C.NONE if r.summary["first_abort"] is None else r.summary["first_abort"])
        return dict(rc=rc, action=r.action.tolist(), moved_to=[tuple(int(x) for x in m) for m in r.moved_to],
                    killed=T.killed_list(r.killed), summary=sm)

    def compact(self):
        r = self.ix.compact()
        assert r["sizes"] == self.ix.sizes()
        return 0, r["cleared"], r["sizes"]

    def close(self):
        self.ix.close()


@pytest.fixture
def gpu(engine):
    return lambda files: GpuIndex(engine, files)


@pytest.mark.parametrize("name", sorted(T.LOOKUP))
def test_lookup(gpu, name):
    T.check_lookup(gpu, name)


@pytest.mark.parametrize("name", sorted(T.SWEEP))
def test_sweep(gpu, name):
    T.check_sweep(gpu, name, T.SWEEP[name])


@pytest.mark.parametrize("seed", T.SEEDS)
def test_random_store(gpu, seed):
    files, _ids = T.random_store(seed)
    T.check_scan(gpu, f"random {seed}", files)
    T.check_sweep(gpu, f"random {seed}", files)


def test_scan(gpu):
    for what, files in (("short", T.LOOKUP["short"][0]), ("duplicate", T.SWEEP["duplicate_earlier_marked"]),
                        ("misplaced", T.SWEEP["abort_below_home"]), ("two files", T.SWEEP["file1_home_past_file0_end"]),
                        ("full run", T.LOOKUP["full_run_found_in_file_1"][0]), ("compact store", T.compact_store())):
        T.check_scan(gpu, what, files)


def test_mark(gpu):
    T.check_mark(gpu)


def test_update(gpu):
    T.check_update(gpu)


def test_compact(gpu):
    T.check_compact(gpu)


def test_pipeline(gpu):
    T.check_pipeline(gpu)


def test_sweep_twice_and_after_growth(gpu):
    """A sweep that lengthens file 0, lookups and marks in the grown file, a
    second sweep in which the marked entries stay and a third, without marks,
    in which they go."""
    files = T.copy(T.SWEEP["file1_home_past_file0_end"])
    ix = gpu(files)
    ref = T.copy(files)
    want = C.ref_sweep(ref)
    got = ix.sweep()
    assert got["action"] == want["action"] and got["summary"]["n_grown"] == 1
    ids = [C.mk_id(50, 1), C.mk_id(52, 2), C.mk_id(51, 9)]
    for sof in (False, True):
        assert ix.lookup(ids, sof)[1] == C.ref_lookup(ref, ids, sof)
    assert ix.mark(ids[:2])[1] == C.ref_mark(ref, ids[:2])
    want = C.ref_sweep(ref)
    got = ix.sweep()
    assert got["action"] == want["action"] == [C.STAY, C.STAY]  # (their old slots in file 1 are Invalid now)
    T.same_images("second sweep", ix.images(), ref)
    want = C.ref_sweep(ref)
    got = ix.sweep()
    assert got["action"] == want["action"] == [C.DELETED, C.DELETED] and got["killed"] == want["killed"]
    T.same_images("third sweep", ix.images(), ref)
    ix.close()


def test_open_paths_and_sizes(engine, tmp_path):
    files = T.SWEEP["file1_stays_and_moves_within"]
    paths = []
    for k, f in enumerate(files):
        p = tmp_path / f"{k:08X}.idx"
        p.write_bytes(bytes(f))
        paths.append(str(p))
    with engine.open_index(paths) as ix:
        assert ix.sizes() == [len(f) for f in files]
        assert [ix.export(k) for k in range(2)] == [bytes(f) for f in files]
        assert T.live_list(ix.scan().live) == C.ref_scan(files)[0]
    with pytest.raises(HbxError, match="HBX_ERR_IO"):
        engine.open_index([str(tmp_path / "none.idx")])
    (tmp_path / "odd.idx").write_bytes(bytes(files[1]) + b"\0")
    with pytest.raises(HbxError, match="HBX_ERR_FORMAT"):
        engine.open_index([paths[0], str(tmp_path / "odd.idx")])


def test_gc_sweep_behind_a_block_graph(engine):
    """formats.gc_sweep: the IDs of the rows the graph marks are marked, the index swept and compacted."""
    files, ids = T.random_store(2)
    for f in files:
        for o in range(C.HEADER, len(f), C.SLOT):
            f[o + 1] &= ~C.M
    rows = list(dict.fromkeys(b for b in ids if C.find(files, b, False)[0]))[:600]
    idv = np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 16)
    # row i links to row i + 1 inside groups of three; the roots are the first rows of two groups in three
    links = [[rows[i + 1]] if i % 3 != 2 and i + 1 < len(rows) else [] for i in range(len(rows))]
    roots = [rows[i] for i in range(0, len(rows), 3) if (i // 3) % 3 != 2]
    g = engine.block_graph(idv, [len(x) for x in links], [b for x in links for b in x], roots)
    assert 100 < g.summary["n_marked"] < len(rows)
    ref = T.copy(files)
    assert all(C.ref_mark(ref, [rows[i] for i in np.flatnonzero(g.marked)]))
    want = C.ref_sweep(ref)
    C.ref_compact(ref)
    with engine.open_index([bytes(f) for f in files]) as ix:
        res = formats.gc_sweep(ix, idv, g)
        assert res.action.tolist() == want["action"] and T.killed_list(res.killed) == want["killed"]
        T.same_images("gc_sweep", [ix.export(0)], ref)
        assert ix.sizes() == [len(ref[0])]
    with engine.open_index([bytes(C.new_file(8))]) as ix, pytest.raises(HbxError, match="no index entry"):
        formats.gc_sweep(ix, idv, g)


def test_errors_leave_the_context_usable(engine):
    L, c = engine._L, engine._ctx
    good = bytes(T.SWEEP["cascade"][0])

    def open_raw(images, n=None):
        bufs = [np.frombuffer(bytes(b) + bytes(8), np.uint8) for b in images]
        ptrs = (ctypes.c_void_p * max(len(bufs), 1))(*[b.ctypes.data for b in bufs])
        sizes = np.array([len(b) for b in images] + [0], np.uint64)
        h = ctypes.c_void_p()
        rc = L.hbx_index_open(c, len(images) if n is None else n, ptrs, sizes.ctypes.data, ctypes.byref(h))
        assert (rc == 0) == bool(h)
        return rc, h

    assert open_raw([], 0)[0] == C.ERR_ARG
    assert open_raw([good] * (_lib.IX_FILES_MAX + 1))[0] == C.ERR_ARG
    assert L.hbx_index_open(c, 1, None, None, None) == C.ERR_ARG
    assert open_raw([good + b"\0"])[0] == C.ERR_FORMAT
    assert open_raw([good[:8]])[0] == C.ERR_FORMAT
    assert open_raw([good, C.header(filetype=0x48534442) + bytes(24)])[0] == C.ERR_FORMAT
    assert open_raw([C.header(version=2) + bytes(24)])[0] == C.ERR_FORMAT
    rc, many = open_raw([good] * _lib.IX_FILES_MAX)
    assert rc == 0 and L.hbx_index_close(c, many) == 0
    rc, h = open_raw([good])
    assert rc == 0
    sm, n = _lib.IxSweepSummary(), ctypes.c_uint64(0)
    act, mv = np.zeros(8, np.uint8), np.zeros(16, np.uint64)
    kl = np.zeros(8, IX_KILLED_DTYPE)
    out = np.zeros(len(good), np.uint8)

    def sweep(live_cap, killed_cap):
        return L.hbx_index_sweep(c, h, act.ctypes.data, mv.ctypes.data, live_cap, kl.ctypes.data, killed_cap, ctypes.byref(sm))

    assert sweep(2, 8) == C.ERR_CAPACITY and (sm.n_live, sm.swept_records, sm.n_moved) == (3, 1, 0)
    assert sweep(8, 0) == C.ERR_CAPACITY and (sm.n_live, sm.n_deleted) == (3, 1)
    assert L.hbx_index_sweep(c, h, None, None, 8, None, 8, ctypes.byref(sm)) == C.ERR_ARG
    assert L.hbx_index_sweep(c, h, act.ctypes.data, mv.ctypes.data, 8, kl.ctypes.data, 8, None) == C.ERR_ARG
    assert L.hbx_index_export(c, h, 0, out.ctypes.data, len(good) - 1, ctypes.byref(n)) == C.ERR_CAPACITY and n.value == len(good)
    assert L.hbx_index_export(c, h, 1, out.ctypes.data, len(good), ctypes.byref(n)) == C.ERR_ARG
    live, ss = np.zeros(2, IX_LIVE_DTYPE), _lib.IxSummary()
    assert L.hbx_index_scan(c, h, live.ctypes.data, 2, None, ctypes.byref(ss)) == C.ERR_CAPACITY and ss.n_live == 3
    assert T.live_list(live) == C.ref_scan(T.SWEEP["cascade"])[0][:2]
    assert L.hbx_index_scan(c, h, None, 0, None, ctypes.byref(ss)) == 0 and ss.n_live == 3  # only counted
    assert L.hbx_index_lookup(c, h, 0, None, 0, None) == 0 and L.hbx_index_mark(c, h, 0, None, None, None) == 0
    assert L.hbx_index_update(c, h, 0, None, None) == 0
    assert L.hbx_index_lookup(c, h, 1, None, 0, None) == C.ERR_ARG
    assert L.hbx_index_lookup(None, h, 0, None, 0, None) == C.ERR_ARG
    # a handle of another context
    with Engine(0) as other:
        assert L.hbx_index_sizes(other._ctx, h, out.ctypes.data) == C.ERR_ARG
        assert L.hbx_index_compact(other._ctx, h, ctypes.byref(_lib.IxCompactSummary())) == C.ERR_ARG
        assert L.hbx_index_close(other._ctx, h) == C.ERR_ARG
    # nothing of that changed the index: it still sweeps as the reference does
    assert L.hbx_index_export(c, h, 0, out.ctypes.data, len(good), ctypes.byref(n)) == 0 and out.tobytes() == good
    assert sweep(8, 8) == 0 and act[:3].tolist() == [C.DELETED, C.MOVED, C.MOVED]
    assert L.hbx_index_close(c, h) == 0
    assert L.hbx_index_close(c, h) == C.ERR_ARG
    assert engine.md5(b"abc").hex() == "900150983cd24fb0d6963f7d28e17f72"


def test_refused_while_batches_are_pending():
    import torch
    t = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    files = T.SWEEP["cascade"]
    with Engine(0) as e:
        ix = e.open_index([bytes(f) for f in files])
        e.submit_device(t.data_ptr(), [0], [1 << 20])
        for call in (ix.sweep, ix.scan, ix.compact, ix.sizes, lambda: ix.lookup([C.mk_id(0, 1)]),
                     lambda: ix.mark([C.mk_id(0, 1)]), lambda: ix.export(0)):
            with pytest.raises(HbxError, match="HBX_ERR_STATE"):
                call()
        e.wait()
        ref = T.copy(files)
        want = C.ref_sweep(ref)
        assert ix.sweep().action.tolist() == want["action"]
        assert ix.export(0) == bytes(ref[0])
        ix.close()
