"""GPU: the block graph on the device (K15, hbx_block_graph: links resolved by
128-bit key, the GC mark from the roots, the block-tree check over the
transposed graph) against the pure-Python reference of tests/graph_craft.py:
every array and every summary field of every case must be equal.  The largest
tables are one row of 100,000 links and a DAG of 50,000 rows."""
import ctypes
import os

import numpy as np
import pytest

from hashbox_amd import BlockGraph, Engine, HbxError, _lib
from . import datfile_craft as D
from . import graph_craft as G

pytestmark = pytest.mark.gpu

NONE = G.NONE
CORPUS = G.corpus(_lib.GRAPH_LANE_MAX, _lib.GRAPH_WAVE_MAX)
ARRAYS = ("rep", "link_row", "root_row", "mark_depth", "fault_depth")
TREE_FIELDS = ("n_faulty", "n_invalid", "fault_levels", "n_marked_faulty")
MARK_FIELDS = ("n_marked", "mark_levels", "n_marked_faulty")


def _compare(name, got, want, summary=None, arrays=ARRAYS):
    """A failure names case, row, field, expected and got."""
    for f in arrays:
        g, w = got[f] if isinstance(got, dict) else getattr(got, f), want[f]
        assert g.shape == w.shape, f"{name}: {f} has shape {g.shape}, expected {w.shape}"
        wrong = np.flatnonzero(g != w)
        if wrong.size:
            i = int(wrong[0])
            pytest.fail(f"case {name}: {f}[{i}] expected {int(w[i])}, got {int(g[i])} ({wrong.size} rows differ)")
    s = got["summary"] if isinstance(got, dict) else got.summary
    w = want["summary"] if summary is None else summary
    assert set(s) == set(G.SUMMARY_FIELDS)
    for k in G.SUMMARY_FIELDS:
        assert s[k] == w[k], f"case {name}: summary {k} expected {w[k]}, got {s[k]}"


def _run(eng, case) -> BlockGraph:
    return eng.block_graph(case.ids, case.n_links, case.links, roots=case.roots, bad=case.bad,
                           link_base=case.link_base)


def _raw(eng, case, absent=()):
    """The C call with some output arrays not wanted (NULL)."""
    n, m, r = case.n, case.m, case.roots.shape[0]
    out = {"rep": np.full(n, 7, np.uint32), "link_row": np.full(m, 7, np.uint32), "root_row": np.full(r, 7, np.uint32),
           "mark_depth": np.full(n, 7, np.uint32), "fault_depth": np.full(n, 7, np.uint32)}
    p = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    sm = _lib.GraphSummary()
    ptrs = [None if f in absent else out[f].ctypes.data for f in ARRAYS]
    nl, lb = np.ascontiguousarray(case.n_links, np.uint32), np.ascontiguousarray(case.link_base, np.uint64)
    rc = eng._L.hbx_block_graph(eng._ctx, n, p(case.ids), p(nl), p(lb), m, p(case.links), p(case.bad), r, p(case.roots),
                                *ptrs, ctypes.byref(sm))
    out["summary"] = {k: int(getattr(sm, k)) for k in G.SUMMARY_FIELDS}
    return rc, out


@pytest.fixture(scope="module", params=[0, 1, 2], ids=["grid-default", "grid-1", "grid-2"])
def grid_engine(request, engine):
    """The session's engine, and engines whose K15 grids are one and two
    workgroups: every table of more than 256 or 512 items then takes several
    grid-stride rounds."""
    if request.param == 0:
        yield engine
        return
    old = {k: os.environ.get(k) for k in ("HBX_AB", "HBX_K15_WGS")}
    os.environ.update(HBX_AB="1", HBX_K15_WGS=str(request.param))
    try:
        eng = Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert eng.knobs()["k15_wgs"] == request.param
    yield eng
    eng.close()


def test_knobs_report_grid_and_thresholds(engine):
    k = engine.knobs()
    assert k["k15_wgs"] == 0  # the knob needs HBX_AB=1
    assert (k["k15_lane_max"], k["k15_wave_max"]) == (_lib.GRAPH_LANE_MAX, _lib.GRAPH_WAVE_MAX)


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_case(grid_engine, name):
    case = CORPUS[name]
    _compare(name, _run(grid_engine, case), G.ref(case))


def test_properties(engine):
    case = CORPUS["keys_alias"]
    g, r = _run(engine, case), G.ref(case)
    assert g.marked.tolist() == (r["mark_depth"] != NONE).tolist()
    assert g.tree_ok.tolist() == (r["fault_depth"] == NONE).tolist()
    assert g.alias.tolist() == [False, False, False, True, False, False, False, True, True]
    # link_base=None is the running sum of n_links
    h = engine.block_graph(case.ids, case.n_links, case.links, roots=case.roots, bad=case.bad)
    _compare("keys_alias/no base", h, r)


@pytest.mark.parametrize("name", ["keys_alias", "deg_thresholds", "fault_unreached", "edge_no_roots", "fault_none"])
@pytest.mark.parametrize("absent", ARRAYS + ("all",))
def test_outputs_not_wanted(engine, name, absent):
    """Each output array absent in turn, and all of them: the others and the
    summary do not change, but a stage that does not run reports 0."""
    case, want = CORPUS[name], G.ref(CORPUS[name])
    gone = ARRAYS if absent == "all" else (absent,)
    rc, out = _raw(engine, case, gone)
    assert rc == 0
    s = dict(want["summary"])
    if "fault_depth" in gone:
        s.update({k: 0 for k in TREE_FIELDS})
    if "mark_depth" in gone and case.roots.shape[0] == 0:
        s.update({k: 0 for k in MARK_FIELDS})
    _compare(f"{name} without {absent}", out, want, summary=s, arrays=[f for f in ARRAYS if f not in gone])
    for f in gone:
        assert (out[f] == 7).all()  # not written


def test_twice_on_one_context():
    """The second and third call find the first's leftovers in the kept
    buffers: a small table after a large one, then the large one again."""
    with Engine(0) as e:
        for name in ("deg_100k", "fault_unreached", "random_dag", "edge_one_row", "edge_n0", "keys_alias", "deg_100k",
                     "fault_none", "random_dag"):
            _compare(name, _run(e, CORPUS[name]), G.ref(CORPUS[name]))


def test_argument_errors_leave_the_context_usable(engine):
    case = CORPUS["keys_alias"]
    L, c = engine._L, engine._ctx
    n, m, r = case.n, case.m, case.roots.shape[0]
    sm = _lib.GraphSummary()
    ids, lk, rt = case.ids.ctypes.data, case.links.ctypes.data, case.roots.ctypes.data
    nl = np.ascontiguousarray(case.n_links, np.uint32)
    lb = np.ascontiguousarray(case.link_base, np.uint64)
    tail = (None, None, None, None, None)

    def call(n_=n, ids_=ids, nl_=nl.ctypes.data, lb_=lb.ctypes.data, m_=m, lk_=lk, r_=r, rt_=rt, sm_=ctypes.byref(sm)):
        return L.hbx_block_graph(c, n_, ids_, nl_, lb_, m_, lk_, None, r_, rt_, *tail, sm_)
    assert call() == 0
    assert call(sm_=None) == -1
    assert call(ids_=None) == -1 and call(nl_=None) == -1 and call(lb_=None) == -1
    assert call(lk_=None) == -1 and call(rt_=None) == -1
    assert call(n_=1 << 31) == -1
    assert call(m_=m - 1) == -1  # the last row's list now ends behind the links
    for base, count in ((m, 1), (m + 1, 0), ((1 << 64) - 1, 2), (m - 1, 2)):
        lb2, nl2 = lb.copy(), nl.copy()
        lb2[4], nl2[4] = base, count
        assert call(nl_=nl2.ctypes.data, lb_=lb2.ctypes.data) == -1, (base, count)
    lb2, nl2 = lb.copy(), nl.copy()
    lb2[5], nl2[5] = m, 0  # an empty list at the very end is inside
    assert call(nl_=nl2.ctypes.data, lb_=lb2.ctypes.data) == 0
    with pytest.raises(ValueError):
        engine.block_graph(case.ids, case.n_links[:-1], case.links)
    with pytest.raises(ValueError):
        engine.block_graph(case.ids, case.n_links, case.links, bad=[1])
    _compare("keys_alias", _run(engine, case), G.ref(case))


def test_refused_while_batches_are_pending_then_chunk_hash(oracle):
    import torch
    t = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    case = CORPUS["front_diamond"]
    with Engine(0) as e:
        e.submit_device(t.data_ptr(), [0], [1 << 20])
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):
            _run(e, case)
        e.wait()
        _compare(case.name, _run(e, case), G.ref(case))
        _compare("random_dag", _run(e, CORPUS["random_dag"]), G.ref(CORPUS["random_dag"]))
        # a plain batch afterwards, nothing pending
        assert e._L.hbx_pending(e._ctx) == 0
        data = oracle.random_bytes(1 << 20, 15)
        got, want = e.chunk_hash(data), oracle.store_file(data, fast=True)
        assert np.array_equal(got.cut_ends, want.cut_ends) and np.array_equal(got.ids, want.ids)
        assert got.content_id == want.content_id
        assert e._L.hbx_pending(e._ctx) == 0


# ------------------------------------------------------------- end to end --
@pytest.fixture(scope="module")
def store(engine, tmp_path_factory):
    """A small tree (nested directories, a file of several chunks, two
    identical files) stored; its blocks as ID -> (links, data, DataType), and
    three orphan blocks."""
    from hashbox_amd import formats as F
    src = tmp_path_factory.mktemp("graph") / "src"
    (src / "a" / "b").mkdir(parents=True)
    rng = np.random.default_rng(15)
    twin = bytes(rng.integers(0, 256, 70_000, dtype=np.uint8))
    files = {"top.txt": bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), "a/twin1": twin, "a/b/twin2": twin,
             "a/big": bytes(rng.integers(0, 256, 5 * (1 << 20) // 2 + 17, dtype=np.uint8)),
             "a/b/small": bytes(rng.integers(0, 256, 100, dtype=np.uint8))}
    for rel, data in files.items():
        (src / rel).write_bytes(data)
    t = F.store_tree(engine, src)
    blocks = {}
    for _p, (dblk, links, bid) in t.directories.items():
        blocks[bytes(bid)] = ([bytes(x) for x in links], dblk, D.ZLIB)
    big_chunks = None
    for path, r in t.files.items():
        data = open(path, "rb").read()
        ends = [int(x) for x in r.cut_ends]
        for k, (a, b, cid) in enumerate(zip([0] + ends[:-1], ends, r.ids)):
            blocks[bytes(cid)] = ([], data[a:b], D.ZLIB if k % 2 else D.RAW)
        if r.content_type == F.TYPE_FILE_CHAIN:
            chain = [bytes(x) for x in r.ids]
            blocks[bytes(r.content_id)] = (chain, F.serialize_chain_block(chain), D.RAW)
            big_chunks = chain
    assert big_chunks and len(big_chunks) > 2
    for bid, (links, data, _t) in blocks.items():
        assert D.block_id(data, links) == bid
    o0, o1 = D.rnd(500, "orphan0"), D.rnd(900, "orphan1")
    orphans = {D.block_id(o0): ([], o0, D.RAW), D.block_id(o1): ([], o1, D.ZLIB)}
    o2 = D.rnd(300, "orphan2")
    orphans[D.block_id(o2, [D.block_id(o0)])] = ([D.block_id(o0)], o2, D.RAW)
    return {"blocks": blocks, "orphans": orphans, "root": bytes(t.root.content_block_id), "victim": big_chunks[1]}


def _datfiles(store, damaged=None):
    """Two data files holding every block once, orphans among them."""
    every = list(store["blocks"].items()) + list(store["orphans"].items())
    order = np.random.default_rng(16).permutation(len(every))
    files = ([], [])
    for k, at in enumerate(order):
        bid, (links, data, dtype) = every[int(at)]
        files[k % 2].append((links, data, dtype, "data" if bid == damaged else None))
    return [D.write_datfile(items)[0] for items in files]


def _ancestors(blocks, victim):
    """Block ID -> the length of the shortest link path down to `victim`'s parent."""
    dist = {bid: 0 for bid, (links, _d, _t) in blocks.items() if victim in links}
    todo = list(dist)
    while todo:
        nxt = []
        for x in todo:
            for bid, (links, _d, _t) in blocks.items():
                if x in links and bid not in dist:
                    dist[bid] = dist[x] + 1
                    nxt.append(bid)
        todo = nxt
    return dist


def test_check_datfiles_then_mark_from_the_root(engine, store):
    from hashbox_amd import formats as F
    blocks, orphans = store["blocks"], store["orphans"]
    checks = [engine.check_datfile(buf) for buf in _datfiles(store)]
    assert sum(c.summary["n_entries"] for c in checks) == len(blocks) + len(orphans)
    assert all(c.summary["n_broken"] == 0 for c in checks)
    ids, nl, base, links, file_no, _off = F.block_table(checks)
    assert set(file_no.tolist()) == {0, 1} and int(nl.max()) > 2
    g = engine.block_graph(ids, nl, links, roots=[store["root"]], link_base=base)
    _compare("store", g, G.reference(G.Case("store", ids, nl, base, links, [store["root"]])))
    row_id = [ids[i].tobytes() for i in range(ids.shape[0])]
    assert {row_id[i] for i in np.flatnonzero(g.marked)} == set(blocks)
    assert {row_id[i] for i in np.flatnonzero(~g.marked)} == set(orphans)
    assert g.tree_ok.all() and g.summary["n_missing_links"] == 0 and g.summary["n_marked_faulty"] == 0
    assert not g.alias.any()

    # one data block damaged in its stream's Adler-32 trailer: it is no entry any more, so its parents miss a link
    victim = store["victim"]
    assert blocks[victim][2] == D.ZLIB
    checks = [engine.check_datfile(buf) for buf in _datfiles(store, damaged=victim)]
    assert sum(c.summary["n_broken"] for c in checks) == 1
    ids, nl, base, links, _f, _o = F.block_table(checks)
    assert ids.shape[0] == len(blocks) + len(orphans) - 1
    g = engine.block_graph(ids, nl, links, roots=[store["root"]], link_base=base)
    _compare("store damaged", g, G.reference(G.Case("store damaged", ids, nl, base, links, [store["root"]])))
    above = _ancestors(blocks, victim)
    assert store["root"] in above and 3 <= len(above) < len(blocks) // 2
    row_id = [ids[i].tobytes() for i in range(ids.shape[0])]
    got = {row_id[i]: int(g.fault_depth[i]) for i in np.flatnonzero(~g.tree_ok)}
    assert got == above
    assert g.summary["n_marked_faulty"] == len(above) == g.summary["n_invalid"] and g.summary["n_faulty"] == 1
    assert g.summary["n_marked"] == len(blocks) - 1 and g.summary["n_missing_links"] == 1
