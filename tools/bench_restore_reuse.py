#!/usr/bin/env python3
"""restore_tree over an existing tree: reuse_local (K13, Engine.locate_ids)
against keep_matching; one JSON object to --out (default
profiles/restore_reuse.json) and stdout.

Tree and store: tools/bench_diff_tree.py's (bench_restore_many.py's set, --gib
GiB, default 2, in one directory under --dir; the block store in memory, every
data block as the engine's own K7 zlib stream).  Before every run the local
tree, which equals the stored one, gets one of three changes in every hundredth
file:

  (i)   flip    one byte flipped in the middle (size and ModTime kept)
  (ii)  insert  one byte inserted at the front (the size changes)
  (iii) rename  the file moved out of the tree; reuse_local gets the moved
                copies through reuse_paths

and is restored over with keep_matching=True and with reuse_local=True.  After
every run the changed files are compared with their stored bytes.  One warm-up
of each, then --runs (default 3) alternating rounds: the medians in seconds,
and the data blocks fetched per run.  The block counts are exact and are
asserted against a model: the chains of the changed files (with repeats),
minus, for reuse_local, every ID some pool file holds, the changed files' IDs
coming from the CPU oracle's chunking.  No bar is set for the times.

Run on the GPU box: python tools/bench_restore_reuse.py
"""
import argparse
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

GIB = 1 << 30
RAW, ZLIB = 0xFF, 0x01
CASES = ("flip", "insert", "rename")
MODES = ("keep_matching", "reuse_local")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_reuse.json"))
    ap.add_argument("--dir", default="/dev/shm/hbx_restore_reuse")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    from bench_restore_many import make_set
    from hashbox_amd import Engine, _lib, formats as F
    from oracle import oracle as O
    O.lib()
    dest, moved = os.path.join(a.dir, "dest"), os.path.join(a.dir, "moved")
    names = [f"{c}_{m}" for c in CASES for m in MODES]
    runs = {n: [] for n in names}
    try:
        paths, sizes = make_set(os.path.join(dest, "tree"), int(a.gib * GIB), 11)
        os.makedirs(moved)
        nbytes = sum(sizes)
        with Engine(0) as eng:
            t = F.store_tree(eng, os.path.join(dest, "tree"), io_threads=a.threads)
            blocks = {bytes(bid): (RAW, dblk, list(links)) for dblk, links, bid in t.directories.values()}
            res = eng.store_paths(paths, a.threads, 1 << 30, compress=True, sizes=sizes)
            data_ids, chains = set(), []
            for r in res:
                chain = [bytes(x) for x in r.ids]
                for cid, z in zip(chain, r.zstreams):
                    blocks[cid] = (ZLIB, bytes(z), [])
                data_ids.update(chain)
                chains.append(chain)
                if r.content_type == F.TYPE_FILE_CHAIN:
                    blocks[bytes(r.content_id)] = (RAW, F.serialize_chain_block(chain), chain)
            del res
            changed = list(range(0, len(paths), 100))
            original = {k: open(paths[k], "rb").read() for k in changed}
            aside = {k: os.path.join(moved, os.path.basename(paths[k])) for k in changed}

            def variant(case, k):
                data = original[k]
                if case == "flip":
                    at = len(data) // 2
                    return data[:at] + bytes([data[at] ^ 0x01]) + data[at + 1:]
                return b"\x5a" + data if case == "insert" else data

            def prepare(case):
                for k in changed:
                    if case == "rename":
                        os.replace(paths[k], aside[k])
                        continue
                    st = os.lstat(paths[k])
                    with open(paths[k], "wb") as fh:
                        fh.write(variant(case, k))
                    os.utime(paths[k], ns=(st.st_atime_ns, st.st_mtime_ns))

            # the model: what each mode must fetch, from the stored chains and the oracle's chunking of the
            # changed files (an unchanged file's IDs are its chain's)
            unchanged = {i for k, ch in enumerate(chains) if k not in original for i in ch}
            model = {}
            for case in CASES:
                local = {k: [bytes(x) for x in O.store_file(np.frombuffer(variant(case, k), np.uint8), fast=True).ids]
                         for k in changed}
                assert case == "rename" or all(local[k] != chains[k] for k in changed)
                pool = unchanged | {i for ids in local.values() for i in ids}
                model[f"{case}_keep_matching"] = sum(len(chains[k]) for k in changed)
                model[f"{case}_reuse_local"] = sum(i not in pool for k in changed for i in chains[k])
            fetched = [0]

            def read_block(bid):
                if bid in data_ids:
                    fetched[0] += 1
                return blocks[bid]

            def run(name):
                case, mode = name.split("_", 1)
                prepare(case)
                kw = {"keep_matching": True} if mode == "keep_matching" else {
                    "reuse_local": True, "reuse_paths": list(aside.values()) if case == "rename" else ()}
                fetched[0] = 0
                t0 = time.perf_counter()
                st = F.restore_tree(eng, t.root, read_block, dest, batch=True, io_threads=a.threads, **kw)
                el = time.perf_counter() - t0
                for k in changed:
                    with open(paths[k], "rb") as fh:
                        assert fh.read() == original[k], paths[k]
                assert st["kept"] == len(paths) - len(changed), st
                assert fetched[0] == model[name], (name, fetched[0], model[name])
                return {"seconds": round(el, 4), "data_blocks_fetched": fetched[0], "bytes_written": st["bytes"],
                        "blocks_reused": st.get("blocks_reused"), "reuse_retried": st.get("reuse_retried")}
            for name in names:  # warm-up: every buffer sized
                run(name)
            for _ in range(a.runs):
                for name in names:
                    runs[name].append(run(name))
                    print(name, runs[name][-1], file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    med = {n: float(np.median([r["seconds"] for r in runs[n]])) for n in names}
    summary = {"seconds": {n: round(v, 4) for n, v in med.items()},
               "data_blocks_fetched": {n: runs[n][0]["data_blocks_fetched"] for n in names},
               "data_blocks_model": model,
               "reuse_over_keep": {c: round(med[f"{c}_reuse_local"] / med[f"{c}_keep_matching"], 4) for c in CASES}}
    result = {"set": f"{len(sizes)} files, {nbytes / GIB:.3f} GiB, log-uniform 4 KiB..4 MiB, text and random mixed, "
                     f"{len(data_ids)} distinct data blocks as K7 streams, {len(changed)} files changed per case, "
                     f"{a.threads} threads",
              "files": len(sizes), "bytes": nbytes, "lib": _lib.identity(), "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
