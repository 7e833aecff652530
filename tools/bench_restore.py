#!/usr/bin/env python3
"""A file's block chain back into its bytes (hbx_restore_blocks,
hbx_restore_file_stream) against the primitives it is built from and against
the CPU; one JSON object to --out (default profiles/restore.json) and stdout.

Corpus: --gib GiB (default 1) of Zipf-word text laid out as tools/bench_dedup.py
does, cut and hashed by the engine (hbx_store_paths_z), every chunk once as the
engine's own K7 stream and once as a CPython zlib -6 stream (the stand-in for
Go's compress/zlib).  One process, one warm-up pass over every leg, then --runs
(default 3) alternating runs per leg and stream kind:

  (a) hbx_restore_blocks from host memory into a host buffer (inflated sizes
      unknown to the caller); its phases from hbx_knobs' restore_ms
  (b) hbx_restore_file_stream, default windows, a sink that discards
  (c) the primitives called separately with EXACT capacities, streams already in
      device memory: hbx_inflate_blocks_device then hbx_verify_blocks_device
  (d) CPython zlib.decompress + hashlib.md5 on 16 threads

Expectation: the device part of (a) (inflate + verify beside K10) is within 5 %
of (c): the gather moves two bytes per output byte at HBM rates beside an
inflate at a few GB/s.

Run on the GPU box: python tools/bench_restore.py
"""
import argparse
import hashlib
import json
import os
import shutil
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

GIB = 1 << 30
PIECE = 128 << 20
ZLIB = 0x01


def leg_blocks(eng, streams, ids, out, total):
    t0 = time.perf_counter()
    r = eng.restore_blocks(streams, [ZLIB] * len(streams), ids, out=out)
    el = time.perf_counter() - t0
    assert r.n_good == len(streams) and int(r.offs[-1]) == total
    ms = eng.knobs()["restore_ms"]
    return {"seconds": round(el, 4), "gibs": round(total / el / GIB, 3),
            "stage_in_ms": ms[0], "inflate_ms": ms[1], "verify_k10_ms": ms[2], "copy_out_ms": ms[3],
            "device_seconds": round((ms[1] + ms[2]) / 1e3, 4)}


def leg_stream(eng, streams, ids, total):
    seen = [0]

    def sink(off, a):
        seen[0] += a.size
    t0 = time.perf_counter()
    n = eng.restore_file(ids, lambda i: (ZLIB, streams[i]), on_data=sink)
    el = time.perf_counter() - t0
    assert n == total == seen[0]
    ms = eng.knobs()["restore_ms"]
    return {"seconds": round(el, 4), "gibs": round(total / el / GIB, 3), "inflate_ms": ms[1], "verify_k10_ms": ms[2]}


def leg_primitives(eng, d_in, in_offs, in_lens, d_out, out_offs, lens, ids, total):
    t0 = time.perf_counter()
    ol, st = eng.inflate_blocks_device(d_in.data_ptr(), in_offs, in_lens, d_out.data_ptr(), out_offs, lens)
    t1 = time.perf_counter()
    _, ok, bad = eng.verify_blocks_device(d_out.data_ptr(), out_offs, ol, None, ids)
    t2 = time.perf_counter()
    assert not st.any() and bad == 0 and int(ol.sum()) == total
    return {"seconds": round(t2 - t0, 4), "gibs": round(total / (t2 - t0) / GIB, 3),
            "inflate_ms": round((t1 - t0) * 1e3, 3), "verify_ms": round((t2 - t1) * 1e3, 3)}


def leg_cpu(streams, ids, total, threads):
    def one(k):
        d = zlib.decompress(streams[k])
        return hashlib.md5(struct.pack(">II", 0, len(d)) + d).digest() == ids[k], len(d)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        res = list(ex.map(one, range(len(streams))))
    el = time.perf_counter() - t0
    assert all(ok for ok, _ in res) and sum(n for _, n in res) == total
    return {"seconds": round(el, 4), "gibs": round(total / el / GIB, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore.json"))
    ap.add_argument("--dir", default="/dev/shm/hbx_restore")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import torch
    from bench_dedup import text_zipf_files
    from hashbox_amd import Engine, pack_arena_layout
    pieces = max(1, int(a.gib * GIB) // PIECE)
    total = pieces * PIECE
    kinds = ("zlib6", "k7")
    names = ["a_restore_blocks", "b_restore_file_stream", "c_inflate_then_verify", "d_cpu_16_threads"]
    legs = {k: {n: [] for n in names} for k in kinds}
    try:
        paths = text_zipf_files(a.dir, pieces, PIECE, 7)
        with Engine(0) as eng:
            res = eng.store_paths(paths, a.threads, 1 << 30, compress=True, sizes=[PIECE] * pieces)
            ids, chunks, streams = [], [], {"zlib6": [], "k7": []}
            for p, r in zip(paths, res):
                data = np.fromfile(p, np.uint8)
                ends = [int(x) for x in r.cut_ends]
                chunks += [data[s:e].tobytes() for s, e in zip([0] + ends[:-1], ends)]
                ids += [bytes(x) for x in r.ids]
                streams["k7"] += [bytes(z) for z in r.zstreams]
            del res
            with ThreadPoolExecutor(a.threads) as ex:
                streams["zlib6"] = list(ex.map(lambda c: zlib.compress(c, 6), chunks))
            lens = [len(c) for c in chunks]
            del chunks
            out = np.zeros(total, np.uint8)  # touched once: no first-touch faults inside a timed copy
            dev = torch.device("cuda", 0)
            out_offs, out_total = pack_arena_layout(lens)
            d_out = torch.empty(int(out_total) + 65536, dtype=torch.uint8, device=dev)
            staged = {}
            for kind in kinds:
                zl = [len(z) for z in streams[kind]]
                io, it = pack_arena_layout(zl)
                host = np.zeros(int(it), np.uint8)
                for o, z in zip(io, streams[kind]):
                    host[int(o):int(o) + len(z)] = np.frombuffer(z, np.uint8)
                staged[kind] = (torch.from_numpy(host).to(dev), io, zl)
            torch.cuda.synchronize(dev)

            def run(kind, name):
                if name == names[0]:
                    return leg_blocks(eng, streams[kind], ids, out, total)
                if name == names[1]:
                    return leg_stream(eng, streams[kind], ids, total)
                if name == names[2]:
                    d_in, io, zl = staged[kind]
                    return leg_primitives(eng, d_in, io, zl, d_out, out_offs, lens, ids, total)
                return leg_cpu(streams[kind], ids, total, a.threads)
            for kind in kinds:  # warm-up: every buffer sized
                for name in names[:3]:
                    run(kind, name)
            for _ in range(a.runs):
                for kind in kinds:
                    for name in names:
                        legs[kind][name].append(run(kind, name))
            knobs = eng.knobs()
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    summary = {}
    for kind in kinds:
        med = {n: float(np.median([r["seconds"] for r in legs[kind][n]])) for n in names}
        a_dev = float(np.median([r["device_seconds"] for r in legs[kind][names[0]]]))
        summary[kind] = {"compressed_bytes": sum(len(z) for z in streams[kind]),
                         "median_seconds": {n: round(v, 4) for n, v in med.items()},
                         "median_gibs": {n: round(total / v / GIB, 3) for n, v in med.items()},
                         "a_device_seconds": round(a_dev, 4),
                         "a_device_over_c": round(a_dev / med[names[2]], 4)}
    result = {"corpus": f"{total / GIB:g} GiB Zipf text, {len(ids)} blocks cut by the engine, {a.threads} CPU threads",
              "blocks": len(ids), "summary": summary, "runs": legs,
              "k8_split_streams": knobs["k8_split_streams"], "k8_split_fallbacks": knobs["k8_split_fallbacks"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["summary"]))


if __name__ == "__main__":
    main()
