#!/usr/bin/env python3
"""diff_tree by block ID (K12, Engine.match_paths) against diff_tree as it is;
one JSON object to --out (default profiles/diff_by_id.json) and stdout.

Tree: tools/bench_restore_many.py's set (BASELINE configs[4]'s shape: sizes
log-uniform in 4 KiB..4 MiB, text and random bytes mixed, --gib GiB, default 2)
in one directory under --dir (default under /dev/shm), stored with store_tree;
the block store is in memory and holds every data block as the engine's own K7
zlib stream.  The local side is that tree, and a second copy with one byte
flipped (size and ModTime kept) in every hundredth file:

  (a) diff_tree as it is, on the unchanged tree: every data block fetched,
      inflated, verified and compared
  (b) diff_tree(by_id=True) on the unchanged tree: the local files cut and
      hashed, no data block fetched; bounded below by reading the local files
      (store_paths over the same files is reported beside it)
  (c) diff_tree(by_id=True) on the copy with 1 % of the files changed: those
      files alone go through the byte comparison

One warm-up of each, then --runs (default 3) alternating rounds; the medians as
seconds per GiB of the tree, and the data blocks fetched per run.  No ratio is
fixed in advance.

Run on the GPU box: python tools/bench_diff_tree.py
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diff_by_id.json"))
    ap.add_argument("--dir", default="/dev/shm/hbx_diff_tree")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    from bench_restore_many import make_set
    from hashbox_amd import Engine, _lib, formats as F
    same_root, changed_root = os.path.join(a.dir, "same"), os.path.join(a.dir, "changed")
    names = ["a_diff_tree", "b_by_id_unchanged", "c_by_id_1pct_changed"]
    runs = {n: [] for n in names}
    store_s = []
    try:
        paths, sizes = make_set(os.path.join(same_root, "tree"), int(a.gib * GIB), 11)
        nbytes = sum(sizes)
        with Engine(0) as eng:
            t = F.store_tree(eng, os.path.join(same_root, "tree"), io_threads=a.threads)
            blocks = {bytes(bid): (RAW, dblk, list(links)) for dblk, links, bid in t.directories.values()}
            res = eng.store_paths(paths, a.threads, 1 << 30, compress=True, sizes=sizes)
            data_ids = set()
            for r in res:
                chain = [bytes(x) for x in r.ids]
                for cid, z in zip(chain, r.zstreams):
                    blocks[cid] = (ZLIB, bytes(z), [])
                data_ids.update(chain)
                if r.content_type == F.TYPE_FILE_CHAIN:
                    blocks[bytes(r.content_id)] = (RAW, F.serialize_chain_block(chain), chain)
            del res
            shutil.copytree(same_root, changed_root, symlinks=True)
            changed = paths[::100]
            for p in changed:
                q = os.path.join(changed_root, os.path.relpath(p, same_root))
                st = os.lstat(q)
                with open(q, "r+b") as fh:
                    fh.seek(st.st_size // 2)
                    b = fh.read(1)
                    fh.seek(st.st_size // 2)
                    fh.write(bytes([b[0] ^ 0x01]))
                os.utime(q, ns=(st.st_atime_ns, st.st_mtime_ns))
            fetched = [0]

            def read_block(bid):
                if bid in data_ids:
                    fetched[0] += 1
                return blocks[bid]

            def run(name):
                root, by_id = (changed_root, True) if name.startswith("c_") else (same_root, name.startswith("b_"))
                fetched[0] = 0
                t0 = time.perf_counter()
                d = F.diff_tree(eng, t.root, read_block, root, io_threads=a.threads, by_id=by_id)
                el = time.perf_counter() - t0
                assert len(d["different"]) == (len(changed) if name.startswith("c_") else 0), d["different"][:3]
                return {"seconds": round(el, 4), "data_blocks_fetched": fetched[0],
                        "matched_by_id": d.get("matched_by_id")}
            for name in names:  # warm-up: every buffer sized
                run(name)
            for _ in range(a.runs):
                for name in names:
                    runs[name].append(run(name))
                    print(name, runs[name][-1], file=sys.stderr, flush=True)
                # what reading, cutting and hashing the local files costs alone: (b)'s floor
                eng.store_paths(paths, a.threads, 1 << 30, sizes=sizes)
                store_s.append(round(eng.last_call_s, 4))
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    med = {n: float(np.median([r["seconds"] for r in runs[n]])) for n in names}
    summary = {"seconds_per_gib": {n: round(v / (nbytes / GIB), 4) for n, v in med.items()},
               "data_blocks_fetched": {n: runs[n][0]["data_blocks_fetched"] for n in names},
               "store_paths_seconds_per_gib": round(float(np.median(store_s)) / (nbytes / GIB), 4),
               "b_over_a": round(med["b_by_id_unchanged"] / med["a_diff_tree"], 4),
               "c_over_a": round(med["c_by_id_1pct_changed"] / med["a_diff_tree"], 4)}
    result = {"set": f"{len(sizes)} files, {nbytes / GIB:.3f} GiB, log-uniform 4 KiB..4 MiB, text and random mixed, "
                     f"{len(data_ids)} distinct data blocks as K7 streams, {len(changed)} files changed in (c), "
                     f"{a.threads} threads",
              "files": len(sizes), "bytes": nbytes, "lib": _lib.identity(), "summary": summary, "runs": runs,
              "store_paths_seconds": store_s}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
