"""CPU: the index files' operations on the host (hbx_index_*_host,
include/hbxgpu.h "Index files") against the pure-Python restatement in
tests/index_craft.py: every image byte for byte, every output word for word.
What the crafted and random stores cover is asserted on the reference first,
so no comparison can pass by covering nothing.  tests/test_gpu_index.py runs
the same checks through the device handle."""
import ctypes

import numpy as np
import pytest

from hashbox_amd import _lib
from hashbox_amd.engine import IX_HIT_DTYPE, IX_KILLED_DTYPE, IX_LIVE_DTYPE
from . import index_craft as C

LOOKUP = {name: (files, ids) for name, files, ids in C.lookup_cases()}
SWEEP = C.sweep_cases(_lib.IX_SWEEP_TILE)
SEEDS = (1, 2, 3)
RANDOM = {}


def random_store(seed):
    if seed not in RANDOM:
        RANDOM[seed] = C.random_store(seed)
    files, ids = RANDOM[seed]
    return [bytearray(f) for f in files], ids


def copy(files):
    return [bytearray(f) for f in files]


def hits_list(h):
    return [tuple(int(h[k][i]) for k in ("found", "flags", "file", "meta_file", "offset", "meta_off"))
            for i in range(h.shape[0])]


def live_list(v):
    return [(v["id"][i].tobytes(),) + tuple(int(v[k][i]) for k in ("flags", "ix_file", "ix_offset", "meta_file", "state",
                                                                  "meta_off")) for i in range(v.shape[0])]


def killed_list(k):
    return [(k["id"][i].tobytes(), int(k["meta_file"][i]), int(k["meta_off"][i])) for i in range(k.shape[0])]


def fields(s):
    return {k: int(getattr(s, k)) for k, _ in s._fields_}


class HostIndex:
    """hbx_index_*_host over buffers with room to grow; behind each size they
    hold 0xAA, so a file that grows shows whether the bytes between are zeroed."""

    def __init__(self, files):
        self.n = len(files)
        cap = C.off(max((len(f) - C.HEADER) // C.SLOT for f in files) + 1400)
        self.bufs = [np.full(cap, 0xAA, np.uint8) for _ in files]
        for b, f in zip(self.bufs, files):
            b[:len(f)] = np.frombuffer(bytes(f), np.uint8)
        self.ptrs = (ctypes.c_void_p * self.n)(*[b.ctypes.data for b in self.bufs])
        self.size = np.array([len(f) for f in files], np.uint64)
        self.caps = np.full(self.n, cap, np.uint64)
        self.L = _lib.load()

    def head(self):
        return self.n, self.ptrs, self.size.ctypes.data, self.caps.ctypes.data

    def images(self):
        return [b[:int(s)].tobytes() for b, s in zip(self.bufs, self.size)]

    def lookup(self, ids, stop_on_free):
        a = np.frombuffer(b"".join(ids), np.uint8)
        h = np.zeros(len(ids), IX_HIT_DTYPE)
        rc = self.L.hbx_index_lookup_host(*self.head(), len(ids), a.ctypes.data, 1 if stop_on_free else 0, h.ctypes.data)
        return rc, hits_list(h)

    def scan(self, live_cap=None):
        sm, per = _lib.IxSummary(), (_lib.IxFileStats * _lib.IX_FILES_MAX)()
        live = np.zeros(1 << 14 if live_cap is None else max(live_cap, 1), IX_LIVE_DTYPE)
        rc = self.L.hbx_index_scan_host(*self.head(), live.ctypes.data, live.shape[0] if live_cap is None else live_cap,
                                        per, ctypes.byref(sm))
        n = min(int(sm.n_live), live.shape[0] if live_cap is None else live_cap)
        return rc, live_list(live[:n]), [fields(per[f]) for f in range(self.n)], fields(sm)

    def mark(self, ids):
        a = np.frombuffer(b"".join(ids), np.uint8)
        found, miss = np.full(len(ids) + 1, 9, np.uint8), ctypes.c_uint64(77)
        rc = self.L.hbx_index_mark_host(*self.head(), len(ids), a.ctypes.data, found.ctypes.data, ctypes.byref(miss))
        return rc, found[:len(ids)].tolist(), int(miss.value)

    def update(self, recs):
        a = np.frombuffer(b"".join(recs), np.uint8)
        st = np.full(len(recs) + 1, 9, np.uint8)
        rc = self.L.hbx_index_update_host(*self.head(), len(recs), a.ctypes.data, st.ctypes.data)
        return rc, st[:len(recs)].tolist()

    def sweep(self, live_cap=1 << 14, killed_cap=1 << 14):
        action, moved = np.zeros(max(live_cap, 1), np.uint8), np.zeros((max(live_cap, 1), 2), np.uint64)
        killed, sm = np.zeros(max(killed_cap, 1), IX_KILLED_DTYPE), _lib.IxSweepSummary()
        rc = self.L.hbx_index_sweep_host(*self.head(), action.ctypes.data, moved.ctypes.data, live_cap, killed.ctypes.data,
                                         killed_cap, ctypes.byref(sm))
        n = min(int(sm.n_live), live_cap)
        return dict(rc=rc, action=action[:n].tolist(), moved_to=[tuple(int(x) for x in r) for r in moved[:n]],
                    killed=killed_list(killed[:min(int(sm.n_deleted), killed_cap)]), summary=fields(sm))

    def compact(self):
        sm = _lib.IxCompactSummary()
        rc = self.L.hbx_index_compact_host(*self.head(), ctypes.byref(sm))
        return rc, int(sm.cleared), [int(sm.size[f]) for f in range(self.n)]

    def close(self):
        pass


# ------------------------------------------------- the checks both suites run --
def same_images(what, got, want):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), f"{what}: file {f} has {len(g)} bytes, expected {len(w)}"
        if bytes(g) != bytes(w):
            at = next(i for i in range(len(w)) if g[i] != w[i])
            pytest.fail(f"{what}: file {f} differs at byte {at}: slot {(at - 16) // 24}, byte {(at - 16) % 24} of it")


def same_list(what, got, want):
    assert len(got) == len(want), f"{what}: {len(got)} entries, expected {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}[{i}]: expected {w}, got {g}"


def check_lookup(open_ix, name):
    files, ids = LOOKUP[name]
    ix = open_ix(files)
    for sof in (False, True):
        rc, got = ix.lookup(ids, sof)
        assert rc == 0
        same_list(f"lookup {name} stop_on_free={sof}", got, C.ref_lookup(files, ids, sof))
    same_images(f"lookup {name}", ix.images(), files)
    ix.close()


def check_scan(open_ix, what, files):
    ix = open_ix(files)
    live, per, sm = C.ref_scan(files)
    rc, glive, gper, gsm = ix.scan()
    assert rc == 0
    same_list(f"scan {what} live", glive, live)
    same_list(f"scan {what} per_file", gper, per)
    assert gsm == sm, f"scan {what}: summary {gsm}, expected {sm}"
    same_images(f"scan {what}", ix.images(), files)
    ix.close()
    return live, per, sm


def check_sweep(open_ix, what, files, then_compact=True):
    """The sweep, and CompactIndexes behind it; returns the reference's result and files."""
    ref = copy(files)
    want = C.ref_sweep(ref)
    ix = open_ix(files)
    got = ix.sweep()
    assert got["rc"] == want["rc"], f"sweep {what}: rc {got['rc']}, expected {want['rc']}"
    same_list(f"sweep {what} action", got["action"], want["action"])
    same_list(f"sweep {what} moved_to", got["moved_to"], want["moved_to"])
    same_list(f"sweep {what} killed", got["killed"], want["killed"])
    assert got["summary"] == want["summary"], f"sweep {what}: summary {got['summary']}, expected {want['summary']}"
    same_images(f"sweep {what}", ix.images(), ref)
    if then_compact:
        cleared, sizes = C.ref_compact(ref)
        rc, gc, gs = ix.compact()
        assert (rc, gc, gs) == (0, cleared, sizes), f"compact after sweep {what}"
        same_images(f"compact after sweep {what}", ix.images(), ref)
    ix.close()
    return want, ref


def check_mark(open_ix):
    files, ids = LOOKUP["short"]
    ids = ids + ids[:3] + [C.mk_id(77, 123)]  # IDs again, and one more the index does not hold
    ref = copy(files)
    want = C.ref_mark(ref, ids)
    assert want.count(0) >= 3 and want.count(1) >= 6
    ix = open_ix(files)
    rc, found, missing = ix.mark(ids)
    assert rc == 0 and missing == want.count(0)
    same_list("mark found", found, want)
    same_images("mark", ix.images(), ref)
    assert ref != files
    ix.close()


def short_records():
    files, ids = LOOKUP["short"]
    recs = []
    for k, bid in enumerate(dict.fromkeys(ids)):
        recs.append(C.slot_bytes(C.E | (C.N if k % 2 else 0) | C.M | C.I, bid, 9 + k % 3, 5000 + 17 * k))
    return files, recs


def check_update(open_ix):
    files, recs = short_records()
    ref = copy(files)
    rc, want = C.ref_update(ref, recs)
    assert rc == 0 and want.count(0) >= 6 and want.count(1) >= 3
    ix = open_ix(files)
    rc, status = ix.update(recs)
    assert rc == 0
    same_list("update status", status, want)
    same_images("update", ix.images(), ref)
    # an ID twice in one call: refused before anything is written
    rc, _ = ix.update(recs + [recs[2]])
    assert rc == C.ERR_ARG
    same_images("update after a refused call", ix.images(), ref)
    ix.close()


def compact_store():
    s = [C.new_file(16), C.new_file(6), C.new_file(4)]
    for k in range(4):
        C.put(s, 0, k, C.E | (C.I if k == 1 else 0), C.mk_id(0, k), 1, k)
    for k in range(4, 10):  # a trailing run of Invalid slots
        C.put(s, 0, k, (C.E if k % 2 else 0) | C.I | C.M, C.mk_id(4, k), 1, k)
    C.put(s, 0, 12, C.N | C.M, C.mk_id(12, 1), 2, 2)  # Exists clear: neither cleared nor kept
    C.put(s, 1, 5, C.E, C.mk_id(5, 1))
    C.put(s, 2, 1, C.E | C.I, C.mk_id(1, 1))  # a file that becomes empty
    return s


def check_compact(open_ix):
    files = compact_store()
    ref = copy(files)
    cleared, sizes = C.ref_compact(ref)
    assert cleared == 8 and sizes == [C.off(4), C.off(6), C.off(0)]
    ix = open_ix(files)
    assert ix.compact() == (0, cleared, sizes)
    same_images("compact", ix.images(), ref)
    ix.close()


def check_pipeline(open_ix, seed=1):
    """writer -> mark -> sweep -> compact -> export against the reference's
    three loops; then every surviving ID is found and every deleted one is not."""
    files, ids = random_store(seed)
    for f in files:  # the writer's store, without a mark
        for o in range(C.HEADER, len(f), C.SLOT):
            f[o + 1] &= ~C.M
    keep = ids[::3] + ids[1::3]
    ref = copy(files)
    fw = C.ref_mark(ref, keep)
    sw = C.ref_sweep(ref)
    assert sw["rc"] == 0 and sw["summary"]["n_deleted"] > 100 and sw["summary"]["n_moved"] > 100
    cleared, sizes = C.ref_compact(ref)
    ix = open_ix(files)
    rc, found, _ = ix.mark(keep)
    assert rc == 0
    same_list("pipeline mark", found, fw)
    got = ix.sweep()
    for k in ("rc", "action", "moved_to", "killed", "summary"):
        assert got[k] == sw[k], f"pipeline sweep {k}"
    assert ix.compact() == (0, cleared, sizes)
    same_images("pipeline", ix.images(), ref)
    dead = [k[0] for k in sw["killed"]]
    alive = [b for b, w in zip(keep, fw) if w]
    rc, hits = ix.lookup(alive + dead, False)
    assert rc == 0
    same_list("pipeline lookup", hits, C.ref_lookup(ref, alive + dead, False))
    still = {b for b in alive if C.find(ref, b, False)[0]}
    assert all(h[0] == 1 for h in hits[:len(alive)]) and len(still) == len(set(alive))
    # a deleted ID is found only if a valid duplicate of it was kept
    assert all(h[0] == 0 for b, h in zip(dead, hits[len(alive):]) if b not in still)
    assert sum(1 for b in dead if b not in still) > 100
    ix.close()


# ------------------------------------------------------------------ the tests --
def host(files):
    return HostIndex(files)


@pytest.mark.parametrize("name", sorted(LOOKUP))
def test_lookup(name):
    check_lookup(host, name)


def test_lookup_cases_cover_what_they_name():
    files, ids = LOOKUP["short"]
    r0, r1 = C.ref_lookup(files, ids, False), C.ref_lookup(files, ids, True)
    at = {bid: k for k, bid in enumerate(ids)}
    hit = lambda r, home, tag, mid=0: r[at[C.mk_id(home, tag, mid)]]  # noqa: E731
    assert hit(r0, 2, 1)[:3] == (1, C.E | C.N, 0) and hit(r0, 2, 1)[4] == C.off(2)
    assert hit(r0, 10, 2)[4] == C.off(15) == hit(r1, 10, 2)[4]
    assert hit(r0, 20, 3)[0] == 1 and hit(r1, 20, 3)[0] == 0 and hit(r1, 20, 3)[4] == C.off(20)
    assert hit(r0, 30, 4)[0] == 0 == hit(r1, 30, 4)[0] and hit(r0, 30, 4)[4] == C.off(30)
    assert hit(r0, 40, 5)[0] == 0 and hit(r0, 40, 5)[4] == C.off(40)
    assert hit(r0, 50, 6)[0] == 0 and hit(r0, 50, 6)[4] == C.off(50)
    assert [hit(r0, 60, 7, k)[5] for k in range(4)] == [1000, 1001, 1002, 1003] and hit(r0, 60, 7, 4)[0] == 0
    assert hit(r0, 115, 8)[2:5:2] == (0, len(files[0]))  # the file ends inside the run
    assert hit(r0, 120, 9)[4] == len(files[0]) and hit(r0, 121, 10)[4] == C.off(121) > len(files[0])
    one = C.ref_lookup(*LOOKUP["full_run_one_file"], False)
    assert one[0][0] == 0 and one[0][2] == 1 == len(LOOKUP["full_run_one_file"][0])  # ran out of index files
    two = C.ref_lookup(*LOOKUP["full_run_found_in_file_1"], False)
    assert two[0][:3] == (1, C.E | C.N, 1) and two[1][:3] == (0, 0, 1)
    for name in ("full_run_remembered_free", "full_run_remembered_free_one_file"):
        assert C.ref_lookup(*LOOKUP[name], False)[0][2:5:2] == (0, C.off(5 + 300))
        assert C.ref_lookup(*LOOKUP[name], True)[0][2:5:2] == (0, C.off(5 + 300))


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_sweep(name):
    check_sweep(host, name, SWEEP[name])


def test_sweep_cases_cover_what_they_name():
    D, S, O, Mv, A = C.DELETED, C.STAY, C.OBSOLETE, C.MOVED, C.ABORT
    none = (C.NONE, C.NONE)
    r = {name: C.ref_sweep(copy(f)) for name, f in SWEEP.items()}
    assert r["unmarked_alone"]["action"] == [D] and r["marked_at_home"]["action"] == [S]
    assert r["cascade"]["action"] == [D, Mv, Mv] and r["cascade"]["moved_to"] == [none, (0, 16), (0, 40)]
    assert r["cascade_middle_at_home"]["action"] == [D, S, Mv]
    assert r["cascade_middle_at_home"]["moved_to"][2] == (0, 16)
    assert r["invalid_in_front"]["action"] == [Mv] and r["marked_invalid_skipped"]["action"] == []
    assert r["garbage_without_exists"]["action"] == [Mv]
    assert r["duplicate_earlier_marked"]["action"] == [S, O]
    assert r["duplicate_earlier_unmarked"]["action"] == [D, Mv]
    assert r["file1_into_slot_freed_in_file0"]["moved_to"][-1] == (0, C.off(3 + 681))
    assert r["file1_stays_and_moves_within"]["action"][-2:] == [S, Mv]
    assert r["file1_stays_and_moves_within"]["moved_to"][-1] == (1, C.off(4))
    f = copy(SWEEP["file1_home_past_file0_end"])
    g = C.ref_sweep(f)
    assert g["moved_to"] == [(0, C.off(50)), (0, C.off(52))] and len(f[0]) == C.off(53) and g["summary"]["n_grown"] == 1
    assert bytes(f[0][C.off(10):C.off(50)]) == bytes(C.off(50) - C.off(10))
    for name in ("abort_below_home", "abort_beyond_reach"):
        f = copy(SWEEP[name])
        g = C.ref_sweep(f)
        assert g["rc"] == C.ERR_FORMAT and g["action"].count(A) == 1 and f == SWEEP[name]
        assert len(set(g["action"])) > 1  # the sweep went on
    assert r["run_683"]["summary"]["n_live"] == 683 and r["run_683"]["rc"] == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_random_store(seed):
    files, _ids = random_store(seed)
    want = C.ref_sweep(copy(files))
    s = want["summary"]
    assert want["rc"] == 0 and min(s["n_deleted"], s["n_stay"], s["n_moved"], s["n_obsolete"]) >= 10, s
    assert want["into_vacated"] >= 1
    live, _per, sm = check_scan(host, f"random {seed}", files)
    assert sm["n_obsolete"] >= 10 and sm["n_invalid"] > 100
    check_sweep(host, f"random {seed}", files)


def test_scan_states_and_misplaced():
    live, _per, sm = check_scan(host, "short", LOOKUP["short"][0])
    assert sm["n_cut_off"] >= 2 and {e[5] for e in live} == {0, 2}
    live, _per, sm = check_scan(host, "duplicate", SWEEP["duplicate_earlier_marked"])
    assert [e[5] for e in live] == [0, 1] and sm["n_obsolete"] == 1
    _live, per, sm = check_scan(host, "misplaced", SWEEP["abort_below_home"])
    assert sm["n_misplaced"] == 1 and per[0]["first_misplaced"] == C.off(2)
    _live, per, _sm = check_scan(host, "two files", SWEEP["file1_home_past_file0_end"])
    assert [p["n_live"] for p in per] == [0, 2] and per[1]["trunc_point"] == C.off(53) and per[0]["trunc_point"] == 16
    check_scan(host, "compact store", compact_store())


def test_mark():
    check_mark(host)


def test_update():
    check_update(host)


def test_compact():
    check_compact(host)


def test_pipeline():
    check_pipeline(host)


def test_capacities_and_bad_files():
    files = SWEEP["cascade"]
    ix = HostIndex(files)
    g = ix.sweep(live_cap=2)
    assert g["rc"] == C.ERR_CAPACITY and g["summary"]["n_live"] == 3 and g["summary"]["swept_records"] == 1
    g = ix.sweep(killed_cap=0)
    assert g["rc"] == C.ERR_CAPACITY and g["summary"]["n_deleted"] == 1
    same_images("a sweep without room", ix.images(), files)
    rc, live, _per, sm = ix.scan(live_cap=2)
    assert rc == C.ERR_CAPACITY and sm["n_live"] == 3 and live == C.ref_scan(files)[0][:2]
    ix.caps[:] = ix.size  # no room to grow
    far = HostIndex(SWEEP["file1_home_past_file0_end"])
    far.caps[:] = far.size
    assert far.sweep()["rc"] == C.ERR_CAPACITY
    same_images("a sweep that cannot grow", far.images(), SWEEP["file1_home_past_file0_end"])
    L = _lib.load()
    sm = _lib.IxCompactSummary()
    for bad, rc in ((bytearray(C.header() + bytes(25)), C.ERR_FORMAT), (bytearray(C.header()[:12]), C.ERR_FORMAT),
                    (bytearray(C.header(filetype=0x48534442) + bytes(24)), C.ERR_FORMAT),
                    (bytearray(C.header(version=2) + bytes(24)), C.ERR_FORMAT)):
        h = HostIndex([bytearray(C.new_file(2))])
        buf = np.frombuffer(bytes(bad) + bytes(64), np.uint8).copy()
        ptrs = (ctypes.c_void_p * 1)(buf.ctypes.data)
        size = np.array([len(bad)], np.uint64)
        assert L.hbx_index_compact_host(1, ptrs, size.ctypes.data, None, ctypes.byref(sm)) == rc
        assert h.compact()[0] == 0
    h = HostIndex([C.new_file(2)])
    assert L.hbx_index_compact_host(0, h.ptrs, h.size.ctypes.data, None, ctypes.byref(sm)) == C.ERR_ARG
    assert L.hbx_index_compact_host(_lib.IX_FILES_MAX + 1, h.ptrs, h.size.ctypes.data, None, ctypes.byref(sm)) == C.ERR_ARG


def test_header_states_the_rule():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hbxgpu.h")).read()
    for name, val in (("HBX_IX_F_MARKED", "4u"), ("HBX_IX_F_INVALID", "8u"), ("HBX_IX_HEADER", "16u"),
                      ("HBX_IX_PROBE_LIMIT", "682u"), ("HBX_IX_SWEEP_TILE", f"{_lib.IX_SWEEP_TILE}u")):
        assert re.search(rf"#define {name} {val}\b", src), name
    assert "findIXOffset(id, stop_on_free)" in src and "If o > size[f]: stop" in src
