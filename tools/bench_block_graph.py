#!/usr/bin/env python3
"""The block graph of one synthetic store table on the device (K15,
Engine.block_graph) beside a one-thread numpy yardstick; one JSON object to
--out (default profiles/block_graph.json) and stdout.

The table (--rows, default 8 Mi, from --seed) is shaped like a backup store:
a few hundred roots (dataset states) over three levels of directories whose
link counts are Zipf-distributed up to 100,000 (one directory has exactly
that many), chain blocks of 2 to 2,000 links (log-uniform), and leaf data
blocks, which are most of the rows; links pick their targets at random in the
layer below, so leaves are shared and some are garbage.  IDs are random 16
bytes.  Two legs:

  clean    no fault: the tree check ends after its seeding pass
  faulty   0.01 % of the leaves are bad: the transposed graph is built

  device   the wall time of Engine.block_graph (hbx_block_graph through the
           binding, copies included): one warm-up, the median of --runs (3)
  host     a numpy level-synchronous BFS over the same arrays on one thread:
           IDs resolved by sorting a 16-byte view and searchsorted; timed once
           per leg (it is deterministic and takes a while)

Every device run is asserted equal to the host result, array by array and
field by field.  No bar is set for the times.  The kernels' own times are not
taken here: run with --device-only --runs 1 under
`rocprofv3 --kernel-trace --stats` for the split.

Run on the GPU box: python tools/bench_block_graph.py
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

NONE = 0xFFFFFFFF
FIELDS = ("n_rows", "n_links", "n_alias", "n_missing_links", "n_roots", "n_roots_missing", "n_marked", "mark_levels",
          "n_faulty", "n_invalid", "fault_levels", "n_marked_faulty")


def make_table(rows: int, seed: int):
    rng = np.random.default_rng(seed)
    n_root, n_d1, n_d2 = 300, max(rows // 2800, 30), max(rows // 140, 300)
    n_chain = max(rows // 210, 100)
    sizes = np.array([n_root, n_d1, n_d2, n_chain, rows - n_root - n_d1 - n_d2 - n_chain])
    first = np.concatenate([[0], np.cumsum(sizes)])
    layer = np.repeat(np.arange(5), sizes)
    deg = np.zeros(rows, np.int64)
    deg[:first[1]] = rng.integers(1, 4, n_root)
    for lv in (1, 2):
        deg[first[lv]:first[lv + 1]] = np.minimum(rng.zipf(1.5, sizes[lv]), 100_000)
    deg[first[1]] = 100_000
    deg[first[3]:first[4]] = np.floor(2 ** rng.uniform(1, np.log2(2001), n_chain)).astype(np.int64)
    order = rng.permutation(rows)  # the rows of a store lie in no order
    ids = rng.integers(0, 256, (rows, 16), dtype=np.uint8)
    m = int(deg.sum())
    src_layer = np.repeat(layer, deg)
    # a root links directories of level 1; a directory the level below or (half of level 2's links) leaves; a chain leaves
    r = rng.random(m)
    tl = np.where(src_layer == 0, 1, np.where(src_layer == 1, 2, np.where(src_layer == 2, np.where(r < 0.5, 3, 4), 4)))
    target = first[tl] + (rng.random(m) * sizes[tl]).astype(np.int64)
    place = np.empty(rows, np.int64)
    place[order] = np.arange(rows)  # node k is row place[k]
    base_node = np.concatenate([[0], np.cumsum(deg)[:-1]])
    table_ids = np.ascontiguousarray(ids[order])
    nl = deg[order].astype(np.uint32)
    base = base_node[order].astype(np.uint64)  # the lists stay where they are: bases in no order
    links = np.ascontiguousarray(ids[target])
    roots = np.ascontiguousarray(ids[:n_root])
    leaves = place[first[4]:]
    bad = np.zeros(rows, np.uint8)
    bad[rng.choice(leaves, max(1, len(leaves) // 10_000), replace=False)] = 1
    return table_ids, nl, base, links, roots, bad


def host_graph(ids, nl, base, links, roots, bad):
    """The yardstick: numpy on one thread."""
    n, m = ids.shape[0], links.shape[0]
    key = np.ascontiguousarray(ids).view("S16").ravel()
    order = np.argsort(key, kind="stable")
    skey = key[order]

    def resolve(q):
        q = np.ascontiguousarray(q).view("S16").ravel()
        at = np.minimum(np.searchsorted(skey, q, side="left"), n - 1)
        return np.where(skey[at] == q, order[at], NONE).astype(np.uint32)
    rep, link_row, root_row = resolve(ids), resolve(links), resolve(roots)
    is_rep = rep == np.arange(n, dtype=np.uint32)
    nl64 = np.where(is_rep, nl, 0).astype(np.int64)
    base64 = base.astype(np.int64)

    def lists(rows_, start, count, adj):
        c = count[rows_]
        tot = int(c.sum())
        if not tot:
            return np.zeros(0, np.int64), np.zeros(0, np.uint32)
        ends = np.cumsum(c)
        at = np.repeat(start[rows_] - (ends - c), c) + np.arange(tot)
        return np.repeat(rows_, c), adj[at]

    def sweep(seeds, start, count, adj):
        depth = np.full(n, NONE, np.uint32)
        front = np.unique(seeds).astype(np.int64)
        depth[front] = 0
        level = 0
        while front.size:
            _, t = lists(front, start, count, adj)
            t = t[t != NONE]
            t = np.unique(t[depth[t] == NONE]).astype(np.int64)
            depth[t] = level + 1
            front, level = t, level + 1
        return depth, level
    mark, mark_levels = sweep(root_row[root_row != NONE], base64, nl64, link_row)
    miss = np.concatenate([[0], np.cumsum(link_row == NONE)])
    faulty = is_rep & ((bad != 0) | (miss[base64 + nl64] - miss[base64] > 0))
    fault, fault_levels = np.full(n, NONE, np.uint32), 0
    if faulty.any():
        src, t = lists(np.flatnonzero(is_rep), base64, nl64, link_row)
        ok = t != NONE
        src, t = src[ok], t[ok].astype(np.int64)
        by_target = np.argsort(t, kind="stable")
        rsrc = src[by_target].astype(np.uint32)
        rcount = np.bincount(t, minlength=n).astype(np.int64)
        rstart = np.cumsum(rcount) - rcount
        fault, fault_levels = sweep(np.flatnonzero(faulty), rstart, rcount, rsrc)
    summary = dict(n_rows=n, n_links=m, n_alias=int((~is_rep).sum()), n_missing_links=int((link_row == NONE).sum()),
                   n_roots=int(roots.shape[0]), n_roots_missing=int((root_row == NONE).sum()),
                   n_marked=int((is_rep & (mark != NONE)).sum()), mark_levels=mark_levels,
                   n_faulty=int(faulty.sum()), n_invalid=int((is_rep & (fault != NONE)).sum()), fault_levels=fault_levels,
                   n_marked_faulty=int((is_rep & (mark != NONE) & (fault != NONE)).sum()))
    mark, fault = mark[rep], fault[rep]  # aliases copy their representative's depths
    return dict(rep=rep, link_row=link_row, root_row=root_row, mark_depth=mark, fault_depth=fault, summary=summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_graph.json"))
    ap.add_argument("--rows", type=int, default=8 << 20)
    ap.add_argument("--seed", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="no host leg and no comparison (for a profiler run)")
    a = ap.parse_args()
    from hashbox_amd import Engine, _lib
    t0 = time.perf_counter()
    ids, nl, base, links, roots, bad = make_table(a.rows, a.seed)
    print(f"table of {ids.shape[0]} rows and {links.shape[0]} links built in {time.perf_counter() - t0:.1f} s; "
          f"largest list {int(nl.max())}", file=sys.stderr, flush=True)
    legs = {"clean": None, "faulty": bad}
    result = {"table": f"{ids.shape[0]} rows, {links.shape[0]} links, {roots.shape[0]} roots, seed {a.seed}; largest "
                       f"list {int(nl.max())}; faulty leg: {int(bad.sum())} bad leaves",
              "lib": _lib.identity(), "legs": {}}
    with Engine(0) as eng:
        for leg, flags in legs.items():
            want, host_s = None, None
            if not a.device_only:
                t0 = time.perf_counter()
                want = host_graph(ids, nl, base, links, roots, flags if flags is not None else np.zeros(ids.shape[0], np.uint8))
                host_s = round(time.perf_counter() - t0, 4)
                print(leg, "host", host_s, want["summary"], file=sys.stderr, flush=True)
            runs = []
            for k in range(a.runs + 1):  # the first is the warm-up
                t0 = time.perf_counter()
                got = eng.block_graph(ids, nl, links, roots=roots, bad=flags, link_base=base)
                el = round(time.perf_counter() - t0, 4)
                if want is not None:
                    for f in ("rep", "link_row", "root_row", "mark_depth", "fault_depth"):
                        assert np.array_equal(getattr(got, f), want[f]), (leg, f)
                    assert got.summary == want["summary"], (got.summary, want["summary"])
                if k:
                    runs.append(el)
                print(leg, "device", el, file=sys.stderr, flush=True)
            dev = float(np.median(runs))
            result["legs"][leg] = {"device_s": runs, "device_median_s": round(dev, 4), "host_s": host_s,
                                   "host_over_device": round(host_s / dev, 2) if host_s else None,
                                   "summary": got.summary}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({leg: {k: v[k] for k in ("device_median_s", "host_s", "host_over_device")}
                      for leg, v in result["legs"].items()}))


if __name__ == "__main__":
    main()
