"""Block tables built from seeds, and a pure-Python reference of the block
graph (helper, no test), written from the semantics in include/hbxgpu.h: a
dict from ID to lowest row, a deque BFS from the roots for mark_depth, a BFS
over reversed edges from the faulty rows for fault_depth.  It knows nothing of
the kernels.  Beside it stand restatements, in this project's words, of the two
loops of the reference server that the call replaces: MarkIndexes' queue and
visited set (pkg/storagedb/gc.go:24-69) and checkBlockFromIXEntry's recursion
with verifiedBlocks (integrity.go:298-329); tests/test_graph_craft.py holds the
BFS reference against them on every acyclic case.

IDs are hashlib.md5 of a label, except where a case designs them."""
from __future__ import annotations

import hashlib
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF
SUMMARY_FIELDS = ("n_rows", "n_links", "n_alias", "n_missing_links", "n_roots", "n_roots_missing", "n_marked",
                  "mark_levels", "n_faulty", "n_invalid", "fault_levels", "n_marked_faulty")


def mk_id(*label) -> bytes:
    return hashlib.md5(repr(label).encode()).digest()


def _ids(list_of_ids) -> np.ndarray:
    return np.frombuffer(b"".join(list_of_ids), np.uint8).reshape(-1, 16).copy()


class Case:
    """One input of the call: arrays as the C-ABI takes them."""

    def __init__(self, name, ids, n_links, link_base, links, roots, bad=None, cyclic=False):
        self.name, self.cyclic = name, cyclic
        self.ids = ids if isinstance(ids, np.ndarray) else _ids(ids)
        self.n_links = np.asarray(n_links, np.uint32).reshape(-1)
        self.link_base = np.asarray(link_base, np.uint64).reshape(-1)
        self.links = links if isinstance(links, np.ndarray) else _ids(links)
        self.roots = roots if isinstance(roots, np.ndarray) else _ids(roots)
        self.bad = None if bad is None else np.asarray(bad, np.uint8).reshape(-1)
        assert self.ids.shape[0] == self.n_links.shape[0] == self.link_base.shape[0]
        assert self.bad is None or self.bad.shape[0] == self.ids.shape[0]

    @property
    def n(self):
        return self.ids.shape[0]

    @property
    def m(self):
        return self.links.shape[0]

    def row_links(self, i):
        b, k = int(self.link_base[i]), int(self.n_links[i])
        lk = self._link_keys()
        return lk[b:b + k]

    def _link_keys(self):
        if not hasattr(self, "_lk"):
            raw = self.links.tobytes()
            self._lk = [raw[16 * e:16 * e + 16] for e in range(self.m)]
        return self._lk

    def id_keys(self):
        if not hasattr(self, "_ik"):
            raw = self.ids.tobytes()
            self._ik = [raw[16 * i:16 * i + 16] for i in range(self.n)]
        return self._ik

    def root_keys(self):
        raw = self.roots.tobytes()
        return [raw[16 * q:16 * q + 16] for q in range(self.roots.shape[0])]


class Table:
    """Rows added one by one, links laid out one list after the other."""

    def __init__(self, name):
        self.name, self.rows, self.roots = name, [], []

    def id(self, *label) -> bytes:
        return mk_id(self.name, *label)

    def row(self, bid: bytes, links=(), bad=False) -> int:
        self.rows.append((bid, list(links), bool(bad)))
        return len(self.rows) - 1

    def case(self, cyclic=False, with_bad=None) -> Case:
        ids = [r[0] for r in self.rows]
        nl = [len(r[1]) for r in self.rows]
        base = np.zeros(len(nl), np.uint64)
        if nl:
            base[1:] = np.cumsum(nl[:-1])
        links = [x for r in self.rows for x in r[1]]
        bad = [r[2] for r in self.rows]
        if with_bad is None:
            with_bad = any(bad)
        return Case(self.name, _ids(ids) if ids else np.zeros((0, 16), np.uint8), nl, base,
                    _ids(links) if links else np.zeros((0, 16), np.uint8),
                    _ids(self.roots) if self.roots else np.zeros((0, 16), np.uint8), bad if with_bad else None, cyclic)


# ---------------------------------------------------------------- reference --
def index_of(case: Case) -> dict:
    """ID -> its lowest row."""
    idx = {}
    for i, k in enumerate(case.id_keys()):
        idx.setdefault(k, i)
    return idx


def reference(case: Case) -> dict:
    n, m = case.n, case.m
    idx = index_of(case)
    keys = case.id_keys()
    rep = np.array([idx[k] for k in keys], np.uint32) if n else np.zeros(0, np.uint32)
    link_row = np.array([idx.get(k, NONE) for k in case._link_keys()], np.uint32) if m else np.zeros(0, np.uint32)
    root_row = np.array([idx.get(k, NONE) for k in case.root_keys()], np.uint32)
    lr = link_row.tolist()
    is_rep = [int(rep[i]) == i for i in range(n)]
    adj = [lr[int(case.link_base[i]):int(case.link_base[i]) + int(case.n_links[i])] if is_rep[i] else []
           for i in range(n)]
    # mark: breadth-first from the roots
    mark = [NONE] * n
    q = deque()
    for t in root_row.tolist():
        if t != NONE and mark[t] == NONE:
            mark[t] = 0
            q.append(t)
    while q:
        i = q.popleft()
        for t in adj[i]:
            if t != NONE and mark[t] == NONE:
                mark[t] = mark[i] + 1
                q.append(t)
    # tree check: breadth-first over reversed edges from the faulty rows
    fault = [NONE] * n
    radj = [[] for _ in range(n)]
    for i in range(n):
        for t in adj[i]:
            if t != NONE:
                radj[t].append(i)
    for i in range(n):
        if is_rep[i] and ((case.bad is not None and case.bad[i]) or NONE in adj[i]):
            fault[i] = 0
            q.append(i)
    n_faulty = len(q)
    while q:
        i = q.popleft()
        for s in radj[i]:
            if fault[s] == NONE:
                fault[s] = fault[i] + 1
                q.append(s)
    reps = [i for i in range(n) if is_rep[i]]
    summary = dict(
        n_rows=n, n_links=m, n_alias=n - len(reps), n_missing_links=int((link_row == NONE).sum()),
        n_roots=int(root_row.shape[0]), n_roots_missing=int((root_row == NONE).sum()),
        n_marked=sum(mark[i] != NONE for i in reps),
        mark_levels=max((mark[i] + 1 for i in reps if mark[i] != NONE), default=0),
        n_faulty=n_faulty, n_invalid=sum(fault[i] != NONE for i in reps),
        fault_levels=max((fault[i] + 1 for i in reps if fault[i] != NONE), default=0),
        n_marked_faulty=sum(mark[i] != NONE and fault[i] != NONE for i in reps))
    for i in range(n):  # an alias row's depths are copies of its representative's
        if not is_rep[i]:
            mark[i], fault[i] = mark[int(rep[i])], fault[int(rep[i])]
    return dict(rep=rep, link_row=link_row, root_row=root_row, mark_depth=np.array(mark, np.uint32).reshape(-1),
                fault_depth=np.array(fault, np.uint32).reshape(-1), summary=summary)


def ref(case: Case) -> dict:
    """reference(case), computed once and shared (do not change it)."""
    if not hasattr(case, "_ref"):
        case._ref = reference(case)
    return case._ref


def mark_indexes_restated(case: Case) -> set:
    """MarkIndexes in this project's words: a queue of IDs, seeded with the
    roots; an ID taken from the queue is looked up in the index; one already
    visited is dropped, otherwise it is marked and its links join the queue.
    (Where the reference aborts on an ID the index does not hold, this skips
    it, as the call under test does.)  Returns the rows marked."""
    idx = index_of(case)
    visited, queue = set(), deque(case.root_keys())
    while queue:
        row = idx.get(queue.popleft())
        if row is None or row in visited:
            continue
        visited.add(row)
        queue.extend(case.row_links(row))
    return visited


def check_tree_restated(case: Case) -> dict:
    """checkBlockFromIXEntry's recursion in this project's words: a block is
    valid if its own check passed and every link exists and is valid; the
    verdict of a block is kept in verifiedBlocks and not computed twice.  Only
    for tables without link cycles (the reference does not return on one).
    Returns row -> valid for every representative row."""
    assert not case.cyclic
    idx = index_of(case)
    verified = {}

    def check(row: int) -> bool:
        if row in verified:
            return verified[row]
        ok = not (case.bad is not None and case.bad[row])
        for k in case.row_links(row):
            t = idx.get(k)
            if t is None or not check(t):
                ok = False
        verified[row] = ok
        return ok

    return {row: check(row) for row in sorted(set(idx.values()))}


# ------------------------------------------------------------------- corpus --
def _edges() -> list:
    out = []
    out.append(Case("edge_n0", np.zeros((0, 16), np.uint8), [], [], [mk_id("n0", k) for k in range(3)],
                    [mk_id("n0", "r", k) for k in range(2)]))
    t = Table("edge_one_row")
    t.row(t.id(0))
    t.roots = [t.id(0)]
    out.append(t.case())
    t = Table("edge_no_roots")
    t.row(t.id(0), [t.id(1), t.id(2)])
    t.row(t.id(1))
    t.row(t.id(2), [t.id("gone")])
    out.append(t.case())
    # a root not in the table, the same root twice, a root whose ID an alias row carries too
    t = Table("edge_roots")
    t.row(t.id("A"), [t.id("B")])
    t.row(t.id("B"))
    t.row(t.id("A"), [t.id("C")], bad=True)  # alias of row 0
    t.row(t.id("C"))
    t.roots = [t.id("X"), t.id("A"), t.id("A"), t.id("B")]
    out.append(t.case())
    # link slots no row owns: before, between and behind the lists; one of them names a row, the others nothing
    name = "edge_unowned"
    ids = [mk_id(name, k) for k in range(4)]
    links = [ids[3], mk_id(name, "u0"), ids[1], ids[2], mk_id(name, "u1"), ids[0], ids[3], mk_id(name, "u2")]
    out.append(Case(name, ids, [2, 0, 1, 0], [2, 0, 6, 8], links, [ids[0]]))
    # overlapping lists, bases in descending order, an empty list at the very end
    name = "edge_overlap"
    ids = [mk_id(name, k) for k in range(6)]
    links = [ids[5], ids[4], ids[3], ids[2], ids[5]]
    out.append(Case(name, ids, [2, 3, 3, 0, 1, 0], [3, 2, 0, 5, 0, 5], links, [ids[0]], bad=[0, 0, 0, 0, 0, 1]))
    return out


def degree_list(lane_max: int, wave_max: int) -> list:
    return sorted({0, 1, 2, lane_max - 1, lane_max, lane_max + 1, 63, 64, 65, 127, 128, 129, wave_max - 1, wave_max,
                   wave_max + 1, 5000})


def _degrees(lane_max: int, wave_max: int) -> list:
    """A root over one row per degree; a row's links go to a pool of shared
    leaves but for its LAST one, which alone leads to a leaf of its own."""
    out = []
    t = Table("deg_thresholds")
    degs = degree_list(lane_max, wave_max)
    pool = [t.id("pool", k) for k in range(97)]
    t.row(t.id("root"), [t.id("deg", d) for d in degs])
    for d in degs:
        t.row(t.id("deg", d), [pool[(k * 31 + d) % 97] for k in range(d - 1)] + ([t.id("own", d)] if d else []))
    for p in pool:
        t.row(p)
    for d in degs:
        if d:
            t.row(t.id("own", d))
    t.roots = [t.id("root")]
    out.append(t.case())
    t = Table("deg_100k")
    pool = [t.id("pool", k) for k in range(1000)]
    t.row(t.id("root"), [t.id("big"), t.id("mid")])
    t.row(t.id("big"), [pool[k % 1000] for k in range(99999)] + [t.id("last")])
    t.row(t.id("mid"), [pool[(k * 7) % 1000] for k in range(4999)] + [t.id("mid_last")])
    for p in pool:
        t.row(p)
    t.row(t.id("last"))
    t.row(t.id("mid_last"), bad=True)
    t.roots = [t.id("root")]
    out.append(t.case())
    t = Table("deg_same_target")
    t.row(t.id("root"), [t.id("one")] * 1000)
    t.row(t.id("one"), [t.id("leaf")])
    t.row(t.id("leaf"), bad=True)
    t.roots = [t.id("root")]
    out.append(t.case())
    return out


LEVEL_SIZES = (63, 64, 65, 255, 256, 257)


def _frontiers() -> list:
    out = []
    t = Table("front_chain70")
    for k in range(71):
        t.row(t.id(k), [t.id(k + 1)] if k < 70 else [])
    t.roots = [t.id(0)]
    out.append(t.case())
    t = Table("front_star1000")
    t.row(t.id("hub"), [t.id(k) for k in range(1000)])
    for k in range(1000):
        t.row(t.id(k))
    t.roots = [t.id("hub")]
    out.append(t.case())
    for size in LEVEL_SIZES:  # levels of 1, size and size rows
        t = Table(f"front_level{size}")
        t.row(t.id("top"), [t.id("a", k) for k in range(size)])
        for k in range(size):
            t.row(t.id("a", k), [t.id("b", k)])
        for k in range(size):
            t.row(t.id("b", k), bad=(k == size - 1))
        t.roots = [t.id("top")]
        out.append(t.case())
    t = Table("front_diamond")  # the bottom at depths 2 and 5
    t.row(t.id("top"), [t.id("long", 0), t.id("short")])
    for k in range(4):
        t.row(t.id("long", k), [t.id("long", k + 1) if k < 3 else t.id("bottom")])
    t.row(t.id("short"), [t.id("bottom")])
    t.row(t.id("bottom"), bad=True)
    t.roots = [t.id("top")]
    out.append(t.case())
    t = Table("front_parents300")
    t.row(t.id("top"), [t.id("p", k) for k in range(300)])
    for k in range(300):
        t.row(t.id("p", k), [t.id("child")])
    t.row(t.id("child"), bad=True)
    t.roots = [t.id("top")]
    out.append(t.case())
    return out


def _cycles() -> list:
    out = []
    for faulty in (False, True):
        tag = "faulty" if faulty else "clean"
        t = Table(f"cycle_self_{tag}")
        t.row(t.id("root"), [t.id("s")])
        t.row(t.id("s"), [t.id("s")], bad=faulty)  # the member itself
        t.row(t.id("other"))
        t.roots = [t.id("root")]
        out.append(t.case(cyclic=True, with_bad=True))
        t = Table(f"cycle_two_{tag}")
        t.row(t.id("a"), [t.id("b")])
        t.row(t.id("b"), [t.id("a")] + ([t.id("hang")] if faulty else []))
        t.row(t.id("hang"), [t.id("gone")] if faulty else [])  # a faulty row hanging off the cycle
        t.roots = [t.id("a")]
        out.append(t.case(cyclic=True, with_bad=True))
        t = Table(f"cycle_three_{tag}")
        t.row(t.id("root"), [t.id("x")])
        t.row(t.id("x"), [t.id("y")])
        t.row(t.id("y"), [t.id("z")], bad=faulty)
        t.row(t.id("z"), [t.id("x")])
        t.row(t.id("apart"))
        t.roots = [t.id("root")]
        out.append(t.case(cyclic=True, with_bad=True))
    return out


def home_ids() -> list:
    """64 IDs with one home slot (K9's rule: LE64 of id[0..8]) that differ in id[15] only."""
    head = mk_id("keys_home")[:15]
    return [head + bytes([k]) for k in range(64)]


def _keys() -> list:
    out = []
    name = "keys_home"
    ids = home_ids()
    t = Table(name)
    for k in range(64):
        t.row(ids[k], [ids[(k + 1) % 64], ids[(k * 7 + 3) % 64]] if k < 63 else [])
    t.roots = [ids[0]]
    out.append(t.case(cyclic=True))
    # links equal to an existing ID in 15 of its 16 bytes, one per position: all missing
    t = Table("keys_near")
    x = t.id("x")
    near = [x[:p] + bytes([x[p] ^ 0x01]) + x[p + 1:] for p in range(16)]
    t.row(t.id("top"), [t.id("mid"), x])
    t.row(t.id("mid"), near[:8] + [x] + near[8:])
    t.row(x)
    t.roots = [t.id("top")] + near[:2]
    out.append(t.case())
    # alias rows before and after the rows that link to their ID, with other links and another bad flag
    t = Table("keys_alias")
    a, b, c, d = t.id("a"), t.id("b"), t.id("c"), t.id("d")
    t.row(t.id("p"), [a])       # 0 links to a before any a
    t.row(a, [b])               # 1 THE a
    t.row(b, [c], bad=False)    # 2 THE b
    t.row(a, [d], bad=True)     # 3 alias of 1: its bad and its link to d are ignored
    t.row(t.id("q"), [a, b])    # 4 links after the alias
    t.row(c)                    # 5
    t.row(d, [t.id("gone")])    # 6 faulty, reached by nobody that counts
    t.row(b, [d], bad=True)     # 7 alias of 2
    t.row(a)                    # 8 alias of 1 again
    t.roots = [t.id("p"), t.id("q")]
    out.append(t.case())
    return out


def _faults() -> list:
    out = []
    t = Table("fault_chain40")
    for k in range(41):
        t.row(t.id(k), [t.id(k + 1)] if k < 40 else [], bad=(k == 40))
    t.roots = [t.id(0)]
    out.append(t.case())
    t = Table("fault_missing_mid")
    leaves = [t.id("leaf", k) for k in range(50)]
    t.row(t.id("top"), [t.id("wide")])
    t.row(t.id("wide"), [leaves[k % 50] if k != 2500 else t.id("gone") for k in range(5000)])
    for x in leaves:
        t.row(x)
    t.roots = [t.id("top")]
    out.append(t.case())
    t = Table("fault_unreached")
    t.row(t.id("top"), [t.id("f1")])
    t.row(t.id("f1"), [t.id("f2")], bad=True)
    t.row(t.id("f2"), bad=True)         # reached only through another faulty row
    t.row(t.id("lost"), bad=True)       # bad and unreached
    t.row(t.id("above_lost"), [t.id("lost")])
    t.roots = [t.id("top")]
    out.append(t.case())
    t = Table("fault_none")  # the skip path, with a bad array of zeros
    t.row(t.id("top"), [t.id("a"), t.id("b")])
    t.row(t.id("a"), [t.id("b")])
    t.row(t.id("b"))
    t.row(t.id("orphan"), [t.id("b")])
    t.roots = [t.id("top")]
    out.append(t.case(with_bad=True))
    t = Table("fault_orphan")  # the only fault where the mark does not come
    t.row(t.id("top"), [t.id("a")])
    t.row(t.id("a"))
    t.row(t.id("orphan"), [t.id("orphan_leaf")])
    t.row(t.id("orphan_leaf"), bad=True)
    t.roots = [t.id("top")]
    out.append(t.case())
    return out


def random_dag(seed=15, rows=50000, roots=20) -> Case:
    """A layered DAG: Zipf out-degrees, leaves shared by many rows, 1 % of the
    links missing, 1 % of the rows bad, 2 % alias rows (another row's ID with
    links and a flag of their own), the rows in random order."""
    rng = np.random.default_rng(seed)
    n_alias = rows // 50
    nodes = rows - n_alias
    sizes = [roots, 200, 2000, 6000]
    sizes.append(nodes - sum(sizes))  # the leaves
    layer = np.repeat(np.arange(len(sizes)), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)])
    ids = np.frombuffer(b"".join(hashlib.md5(b"dag%d" % k).digest() for k in range(nodes)), np.uint8).reshape(-1, 16)
    # the rows of the table: every node once, then the aliases (a node of an inner layer each)
    node_of = np.concatenate([np.arange(nodes), rng.integers(0, first[-2], n_alias)])
    inner = layer[node_of] < len(sizes) - 1
    deg = np.where(inner, np.minimum(rng.zipf(1.7, rows), 5000), 0)
    order = rng.permutation(rows)
    node_of, deg = node_of[order], deg[order]
    m = int(deg.sum())
    src_layer = np.repeat(layer[node_of], deg)
    # a link goes to the next layer, or (one in four) straight to a leaf
    to_leaf = (rng.random(m) < 0.25) | (src_layer == len(sizes) - 2)
    tl = np.where(to_leaf, len(sizes) - 1, src_layer + 1)
    target = first[tl] + (rng.random(m) * (first[tl + 1] - first[tl])).astype(np.int64)
    links = ids[target].copy()
    gone = rng.random(m) < 0.01
    links[gone] = rng.integers(0, 256, (int(gone.sum()), 16), dtype=np.uint8)
    base = np.zeros(rows, np.uint64)
    base[1:] = np.cumsum(deg[:-1])
    bad = (rng.random(rows) < 0.01).astype(np.uint8)
    return Case("random_dag", ids[node_of].copy(), deg, base, links, ids[:roots].copy(), bad)


_corpus = {}


def corpus(lane_max: int, wave_max: int) -> dict:
    """name -> Case; the degree cases move with the kernels' two thresholds."""
    key = (lane_max, wave_max)
    if key not in _corpus:
        cases = _edges() + _degrees(lane_max, wave_max) + _frontiers() + _cycles() + _keys() + _faults() + [random_dag()]
        _corpus[key] = {c.name: c for c in cases}
        assert len(_corpus[key]) == len(cases)
    return _corpus[key]
