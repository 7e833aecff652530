#!/usr/bin/env python3
"""Restore of many small files in one call (hbx_restore_files_stream, K11)
against one call per file and against the CPU; one JSON object to --out
(default profiles/restore_many.json) and stdout.

Set: BASELINE configs[4]'s shape, sizes log-uniform in 4 KiB..4 MiB, every
other file Zipf-word text and the rest random bytes, as many files as fit
--gib (default 4).  The set is stored with store_paths(compress=True) and then
restored from the blocks held in memory (the engine's own K7 streams), once
with a discarding writer (every path /dev/null) and once to files in --dir
(default under /dev/shm):

  (a) the way before hbx_restore_files_stream: one Engine.restore_file per file
  (b) Engine.restore_files, size hints from the file sizes
  (c) CPython zlib.decompress + hashlib.md5 on --threads (16) threads

One warm-up pass of (a) and (b), then --runs (default 3) alternating runs per
leg and target; the medians as seconds per GiB and files per second.  K11's
share of (b) comes from hbx_knobs' restore_ms: the host milliseconds spent in
VerifyBlock beside K11 over the call's time.  No ratio is fixed in advance: the
result to read is (b) against (a) on the same set in the same run.

--lib PATH runs with another build of the library (a variant compiled with
-DHBX_PIECE_MANY=<bytes>); --piece-libs 4096=PATH,65536=PATH runs leg (b) again
in a child process per variant and reports them beside the product's value.

Run on the GPU box: python tools/bench_restore_many.py
"""
import argparse
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

GIB = 1 << 30
ZLIB = 0x01


def make_set(d, total, seed):
    """Files of log-uniform size 4 KiB..4 MiB up to `total` bytes: (paths, sizes)."""
    from bench_deflate import text_corpus
    rng = np.random.default_rng(seed)
    text = text_corpus(64 << 20, seed).tobytes()
    noise = rng.integers(0, 256, 64 << 20, dtype=np.uint8).tobytes()
    os.makedirs(d, exist_ok=True)
    paths, sizes, used = [], [], 0
    while True:
        n = int(np.exp(rng.uniform(np.log(4 << 10), np.log(4 << 20))))
        if used + n > total:
            break
        base = text if len(paths) % 2 == 0 else noise
        o = int(rng.integers(0, len(base) - n))
        p = os.path.join(d, f"{len(paths):06d}.bin")
        with open(p, "wb") as fh:
            fh.write(base[o:o + n])
        paths.append(p)
        sizes.append(n)
        used += n
    return paths, sizes


def leg_per_file(eng, ids, streams, sizes, outs):
    t0 = time.perf_counter()
    got = 0
    for f in range(len(ids)):
        z = streams[f]
        if outs is None:
            got += eng.restore_file(ids[f], lambda i: (ZLIB, z[i]), on_data=lambda off, a: None)
        else:
            got += eng.restore_file(ids[f], lambda i: (ZLIB, z[i]), out_path=outs[f])
    el = time.perf_counter() - t0
    assert got == sum(sizes)
    return {"seconds": round(el, 4)}


def leg_many(eng, ids, streams, sizes, outs, threads):
    paths = outs if outs is not None else ["/dev/null"] * len(ids)
    t0 = time.perf_counter()
    res = eng.restore_files(ids, lambda f, i: (ZLIB, streams[f][i]), paths, size_hints=sizes, io_threads=threads)
    el = time.perf_counter() - t0
    assert all(r.bad_index is None and r.errno == 0 for r in res) and sum(r.bytes for r in res) == sum(sizes)
    k = eng.knobs()
    ms = k["restore_ms"]
    return {"seconds": round(el, 4), "inflate_ms": ms[1], "verify_k11_ms": ms[2], "emit_ms": ms[3],
            "k11_share": round(ms[2] / 1e3 / el, 4), "windows": k["restore_many"][0], "retries": k["restore_many"][2]}


def leg_cpu(ids, streams, sizes, outs, threads):
    def one(f):
        parts = []
        for z, want in zip(streams[f], ids[f]):
            d = zlib.decompress(z)
            assert hashlib.md5(struct.pack(">II", 0, len(d)) + d).digest() == want
            parts.append(d)
        if outs is not None:
            with open(outs[f], "wb") as fh:
                for d in parts:
                    fh.write(d)
        return sum(len(d) for d in parts)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        got = sum(ex.map(one, range(len(ids))))
    el = time.perf_counter() - t0
    assert got == sum(sizes)
    return {"seconds": round(el, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_many.json"))
    ap.add_argument("--dir", default="/dev/shm/hbx_restore_many")
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libhbxgpu.so (a kPieceMany variant)")
    ap.add_argument("--piece-libs", default="", help="BYTES=PATH,...: leg (b) again per variant, in child processes")
    ap.add_argument("--only-many", action="store_true", help="leg (b) only (what a --piece-libs child runs)")
    a = ap.parse_args()
    from hashbox_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from hashbox_amd import Engine
    total = int(a.gib * GIB)
    names = ["b_restore_files"] if a.only_many else ["a_restore_file_each", "b_restore_files", "c_cpu_threads"]
    targets = ("discard", "shm")
    legs = {t: {n: [] for n in names} for t in targets}
    src_dir, out_dir = os.path.join(a.dir, "src"), os.path.join(a.dir, "out")
    try:
        paths, sizes = make_set(src_dir, total, 11)
        nbytes = sum(sizes)
        with Engine(0) as eng:
            res = eng.store_paths(paths, a.threads, 1 << 30, compress=True, sizes=sizes)
            ids = [[bytes(x) for x in r.ids] for r in res]
            streams = [[bytes(z) for z in r.zstreams] for r in res]
            del res
            shutil.rmtree(src_dir, ignore_errors=True)
            os.makedirs(out_dir, exist_ok=True)
            outs = [os.path.join(out_dir, f"{k:06d}.bin") for k in range(len(paths))]

            def run(target, name):
                o = outs if target == "shm" else None
                if name == "a_restore_file_each":
                    return leg_per_file(eng, ids, streams, sizes, o)
                if name == "b_restore_files":
                    return leg_many(eng, ids, streams, sizes, o, a.threads)
                return leg_cpu(ids, streams, sizes, o, a.threads)
            for name in names:  # warm-up: every buffer sized
                if name != "c_cpu_threads":
                    run("discard", name)
            for _ in range(a.runs):
                for target in targets:
                    for name in names:
                        legs[target][name].append(run(target, name))
                        print(target, name, legs[target][name][-1]["seconds"], file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    summary = {}
    for t in targets:
        med = {n: float(np.median([r["seconds"] for r in legs[t][n]])) for n in names}
        summary[t] = {"seconds_per_gib": {n: round(v / (nbytes / GIB), 4) for n, v in med.items()},
                      "files_per_second": {n: round(len(sizes) / v, 1) for n, v in med.items()},
                      "b_k11_share": float(np.median([r["k11_share"] for r in legs[t]["b_restore_files"]])),
                      "b_windows": legs[t]["b_restore_files"][0]["windows"]}
        if not a.only_many:
            summary[t]["b_over_a"] = round(med["b_restore_files"] / med["a_restore_file_each"], 4)
    result = {"set": f"{len(sizes)} files, {nbytes / GIB:.3f} GiB, log-uniform 4 KiB..4 MiB, text and random mixed, "
                     f"{sum(len(c) for c in ids)} blocks, K7 streams, {a.threads} threads",
              "files": len(sizes), "bytes": nbytes, "lib": _lib.identity(), "summary": summary, "runs": legs}
    if a.piece_libs:
        result["piece_many"] = {}
        for item in a.piece_libs.split(","):
            size, path = item.split("=", 1)
            tmp = a.out + f".piece{size}.json"
            subprocess.run([sys.executable, os.path.abspath(__file__), "--only-many", "--lib", path, "--out", tmp,
                            "--dir", a.dir, "--gib", str(a.gib), "--threads", str(a.threads), "--runs", str(a.runs)],
                           check=True, stdout=subprocess.DEVNULL)
            with open(tmp) as fh:
                sub = json.load(fh)
            os.remove(tmp)
            result["piece_many"][size] = {t: {"seconds_per_gib": sub["summary"][t]["seconds_per_gib"]["b_restore_files"],
                                              "k11_share": sub["summary"][t]["b_k11_share"]} for t in targets}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["summary"]))


if __name__ == "__main__":
    main()
