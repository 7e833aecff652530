"""CPU: the reference side of the block graph tests (tests/graph_craft.py) is
held against restatements of the reference server's two loops, the corpus is
shown to contain what it claims, and the host-only pieces of the feature
(struct size, constants, formats.block_table, argument checks before a device
is touched) are checked."""
import ctypes
import os
import re

import numpy as np
import pytest

from hashbox_amd import _lib
from hashbox_amd.engine import DAT_ENTRY_DTYPE, DatFileCheck
from . import graph_craft as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = G.NONE
LANE, WAVE = _lib.GRAPH_LANE_MAX, _lib.GRAPH_WAVE_MAX
CORPUS = G.corpus(LANE, WAVE)
ACYCLIC = sorted(k for k, c in CORPUS.items() if not c.cyclic)


def _header() -> str:
    with open(os.path.join(ROOT, "include", "hbxgpu.h")) as f:
        return f.read()


def test_binding_mirrors_the_header():
    h = _header()
    assert int(re.search(r"\} hbx_graph_summary;\s*/\* (\d+) bytes \*/", h).group(1)) == \
        ctypes.sizeof(_lib.GraphSummary) == 8 * len(G.SUMMARY_FIELDS)
    body = re.search(r"typedef struct \{([^}]*)\} hbx_graph_summary;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [x.strip() for decl in body.split(";") for x in decl.replace("uint64_t", "").split(",") if x.strip()]
    assert fields == [n for n, _ in _lib.GraphSummary._fields_] == list(G.SUMMARY_FIELDS)
    assert int(re.search(r"#define HBX_GRAPH_LANE_MAX (\d+)u", h).group(1)) == LANE <= 64
    assert int(re.search(r"#define HBX_GRAPH_WAVE_MAX (\d+)u", h).group(1)) == WAVE > LANE
    assert re.search(r"#define HBX_GRAPH_NONE 0xFFFFFFFFu", h) and _lib.GRAPH_NONE == NONE


def test_argument_checks_without_device():
    L = _lib.load()
    sm = _lib.GraphSummary()
    buf = (ctypes.c_uint8 * 64)()
    assert L.hbx_block_graph(None, 0, None, None, None, 0, None, None, 0, None, None, None, None, None, None,
                             ctypes.byref(sm)) == -1
    assert L.hbx_block_graph(None, 1, buf, buf, buf, 0, None, None, 0, None, None, None, None, None, None, None) == -1


@pytest.mark.parametrize("name", ACYCLIC)
def test_reference_agrees_with_the_restated_loops(name):
    case, r = CORPUS[name], G.ref(CORPUS[name])
    reps = {i for i in range(case.n) if int(r["rep"][i]) == i}
    marked = {i for i in reps if r["mark_depth"][i] != NONE}
    assert marked == G.mark_indexes_restated(case)
    valid = G.check_tree_restated(case)
    assert set(valid) == reps
    wrong = [i for i in reps if bool(r["fault_depth"][i] == NONE) != valid[i]]
    assert not wrong, wrong[:10]
    s = r["summary"]
    assert s["n_marked"] == len(marked) and s["n_invalid"] == sum(not v for v in valid.values())


def test_every_case_is_cyclic_exactly_where_it_says():
    for name, case in CORPUS.items():
        r = G.ref(case)
        adj = {i: [int(t) for t in r["link_row"][int(case.link_base[i]):int(case.link_base[i]) + int(case.n_links[i])]
                   if t != NONE] for i in range(case.n) if int(r["rep"][i]) == i}
        indeg = {i: 0 for i in adj}
        for i in adj:
            for t in adj[i]:
                indeg[t] += 1
        ready = [i for i in adj if not indeg[i]]
        seen = 0
        while ready:
            i = ready.pop()
            seen += 1
            for t in adj[i]:
                indeg[t] -= 1
                if not indeg[t]:
                    ready.append(t)
        assert (seen < len(adj)) == case.cyclic, name


def test_edges_of_the_call():
    c = CORPUS["edge_n0"]
    assert c.n == 0 and c.m == 3 and G.ref(c)["summary"]["n_roots_missing"] == 2
    assert CORPUS["edge_one_row"].n == 1 and CORPUS["edge_one_row"].m == 0
    assert CORPUS["edge_no_roots"].roots.shape[0] == 0
    c, r = CORPUS["edge_roots"], G.ref(CORPUS["edge_roots"])
    assert r["root_row"].tolist() == [NONE, 0, 0, 1] and r["rep"].tolist() == [0, 1, 0, 3]
    assert r["mark_depth"].tolist() == [0, 0, 0, NONE]  # the alias's link to C is not followed
    c, r = CORPUS["edge_unowned"], G.ref(CORPUS["edge_unowned"])
    owned = set()
    for i in range(c.n):
        owned |= set(range(int(c.link_base[i]), int(c.link_base[i]) + int(c.n_links[i])))
    free = sorted(set(range(c.m)) - owned)
    assert free and any(r["link_row"][e] != NONE for e in free) and any(r["link_row"][e] == NONE for e in free)
    assert r["summary"]["n_missing_links"] == 3 and r["summary"]["n_faulty"] == 0
    c = CORPUS["edge_overlap"]
    spans = [(int(b), int(b) + int(k)) for b, k in zip(c.link_base, c.n_links) if k]
    assert any(a < d and c_ < b for (a, b) in spans for (c_, d) in spans if (a, b) != (c_, d))
    assert list(c.link_base[:3]) == sorted(c.link_base[:3], reverse=True)


def test_degrees_present():
    want = G.degree_list(LANE, WAVE)
    assert {LANE - 1, LANE, LANE + 1, WAVE - 1, WAVE, WAVE + 1, 0, 1, 2, 63, 64, 65, 127, 128, 129, 5000} == set(want)
    c, r = CORPUS["deg_thresholds"], G.ref(CORPUS["deg_thresholds"])
    assert sorted(set(c.n_links[1:1 + len(want)].tolist())) == want
    # the last link of every row alone leads to its own leaf: dropping it leaves that leaf unmarked
    for i in range(1, 1 + len(want)):
        k = int(c.n_links[i])
        if k:
            last = int(r["link_row"][int(c.link_base[i]) + k - 1])
            assert int((r["link_row"] == last).sum()) == 1 and r["mark_depth"][last] == 2
    c, r = CORPUS["deg_100k"], G.ref(CORPUS["deg_100k"])
    assert sorted(c.n_links.tolist())[-2:] == [5000, 100000]
    for row in (1, 2):
        last = int(r["link_row"][int(c.link_base[row]) + int(c.n_links[row]) - 1])
        assert int((r["link_row"] == last).sum()) == 1 and r["mark_depth"][last] == 2
    c, r = CORPUS["deg_same_target"], G.ref(CORPUS["deg_same_target"])
    assert c.n_links[0] == 1000 and set(r["link_row"][:1000].tolist()) == {1}


def test_frontiers_present():
    r = G.ref(CORPUS["front_chain70"])
    assert r["mark_depth"].tolist() == list(range(71)) and r["summary"]["mark_levels"] == 71 > 64
    r = G.ref(CORPUS["front_star1000"])
    assert np.bincount(r["mark_depth"]).tolist() == [1, 1000]
    for size in G.LEVEL_SIZES:
        r = G.ref(CORPUS[f"front_level{size}"])
        assert np.bincount(r["mark_depth"]).tolist() == [1, size, size]
    assert G.LEVEL_SIZES == (63, 64, 65, 255, 256, 257)
    c, r = CORPUS["front_diamond"], G.ref(CORPUS["front_diamond"])
    assert r["mark_depth"][6] == 2 and r["mark_depth"][4] == 4  # the bottom: 2 by the short way, 5 by the long one
    assert r["fault_depth"].tolist() == [2, 4, 3, 2, 1, 1, 0]
    r = G.ref(CORPUS["front_parents300"])
    assert r["summary"]["n_marked"] == 302 and int((r["link_row"] == 301).sum()) == 300


def test_cycles_present():
    for kind in ("self", "two", "three"):
        clean, faulty = G.ref(CORPUS[f"cycle_{kind}_clean"]), G.ref(CORPUS[f"cycle_{kind}_faulty"])
        assert clean["summary"]["n_invalid"] == 0 and faulty["summary"]["n_invalid"] >= 2
        assert CORPUS[f"cycle_{kind}_clean"].cyclic and CORPUS[f"cycle_{kind}_faulty"].cyclic
    r = G.ref(CORPUS["cycle_three_faulty"])
    assert r["fault_depth"].tolist() == [2, 1, 0, 2, NONE] and r["mark_depth"].tolist() == [0, 1, 2, 3, NONE]


def test_keys_present():
    ids = G.home_ids()
    assert len(set(ids)) == 64 and len({i[:15] for i in ids}) == 1  # one home slot: LE64(id[0..8]) is shared
    c, r = CORPUS["keys_home"], G.ref(CORPUS["keys_home"])
    assert c.ids.tobytes() == b"".join(ids) and r["summary"]["n_marked"] == 64 and r["summary"]["n_missing_links"] == 0
    c, r = CORPUS["keys_near"], G.ref(CORPUS["keys_near"])
    x = c.ids[2].tobytes()
    mid = c.links[2:19]
    diff = [[p for p in range(16) if mid[k].tobytes()[p] != x[p]] for k in range(17)]
    assert sorted(d[0] for d in diff if d) == list(range(16)) and all(len(d) <= 1 for d in diff)
    assert r["summary"]["n_missing_links"] == 16 and r["link_row"][2 + 8] == 2
    c, r = CORPUS["keys_alias"], G.ref(CORPUS["keys_alias"])
    assert r["rep"].tolist() == [0, 1, 2, 1, 4, 5, 6, 2, 1]
    assert r["mark_depth"].tolist() == [0, 1, 1, 1, 0, 2, NONE, 1, 1]  # d is reached through aliases only: unmarked
    assert r["fault_depth"].tolist() == [NONE] * 6 + [0, NONE, NONE]  # the aliases' bad flags count for nothing


def test_faults_present():
    r = G.ref(CORPUS["fault_chain40"])
    assert r["fault_depth"].tolist() == list(range(40, -1, -1))
    c, r = CORPUS["fault_missing_mid"], G.ref(CORPUS["fault_missing_mid"])
    assert c.n_links[1] == 5000 and np.flatnonzero(r["link_row"] == NONE).tolist() == [1 + 2500]
    assert r["fault_depth"][:2].tolist() == [1, 0]
    r = G.ref(CORPUS["fault_unreached"])
    assert r["fault_depth"].tolist() == [1, 0, 0, 0, 1] and r["mark_depth"].tolist() == [0, 1, 2, NONE, NONE]
    c, r = CORPUS["fault_none"], G.ref(CORPUS["fault_none"])
    assert c.bad is not None and not c.bad.any() and r["summary"]["n_faulty"] == 0
    s = G.ref(CORPUS["fault_orphan"])["summary"]
    assert s["n_marked_faulty"] == 0 and s["n_invalid"] == 2 and s["n_marked"] == 2


def test_random_dag_is_what_it_says():
    c, r = CORPUS["random_dag"], G.ref(CORPUS["random_dag"])
    s = r["summary"]
    assert c.n == 50000 and 200000 <= c.m <= 400000 and s["n_roots"] == 20
    assert s["n_alias"] == 1000 or 900 <= s["n_alias"] <= 1000
    assert 0.005 * c.m <= s["n_missing_links"] <= 0.015 * c.m and 350 <= int(c.bad.sum()) <= 650
    assert int(c.n_links.max()) > WAVE and int((c.n_links > 64).sum()) > 100
    assert s["n_marked"] > 10000 and s["n_marked_faulty"] > 100 and s["n_invalid"] > s["n_faulty"] > 0
    targets, counts = np.unique(r["link_row"][r["link_row"] != NONE], return_counts=True)
    assert int(counts.max()) >= 10 and float(np.mean(counts > 1)) > 0.5  # shared leaves: most have several parents
    again = G.random_dag()
    assert again.ids.tobytes() == c.ids.tobytes() and again.links.tobytes() == c.links.tobytes()


def _check_of(rows, links):
    e = np.zeros(len(rows), DAT_ENTRY_DTYPE)
    for k, (bid, off, base, nl) in enumerate(rows):
        e[k]["id"] = np.frombuffer(bid, np.uint8)
        e[k]["off"], e[k]["link_base"], e[k]["n_links"] = off, base, nl
    lk = np.frombuffer(b"".join(links), np.uint8).reshape(-1, 16).copy() if links else np.zeros((0, 16), np.uint8)
    return DatFileCheck(e, np.zeros(0), {"n_links": len(links)}, lk)


def test_block_table_joins_files():
    from hashbox_amd import formats
    a, b, c, d, x = (G.mk_id("bt", k) for k in "abcdx")
    one = _check_of([(a, 16, 0, 2), (b, 100, 2, 0), (c, 200, 2, 1)], [b, c, x])
    two = _check_of([(d, 16, 0, 1), (x, 90, 1, 2)], [a, b, c])
    ids, nl, base, links, file_no, off = formats.block_table([one, two])
    assert ids.dtype == np.uint8 and ids.tobytes() == a + b + c + d + x
    assert nl.dtype == np.uint32 and nl.tolist() == [2, 0, 1, 1, 2]
    assert base.dtype == np.uint64 and base.tolist() == [0, 2, 2, 3, 4]
    assert links.tobytes() == b + c + x + a + b + c
    assert file_no.tolist() == [0, 0, 0, 1, 1] and off.tolist() == [16, 100, 200, 16, 90]
    case = G.Case("bt", ids, nl, base, links, [d])
    r = G.ref(case)
    assert r["mark_depth"].tolist() == [1, 2, 2, 0, 3] and r["summary"]["n_missing_links"] == 0
    empty = formats.block_table([])
    assert [v.shape for v in empty] == [(0, 16), (0,), (0,), (0, 16), (0,), (0,)]
    with pytest.raises(ValueError):
        formats.block_table([DatFileCheck(one.entries, one.spans, one.summary, None)])
