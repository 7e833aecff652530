#!/usr/bin/env python3
"""The block-ID set (K9, hbx_idset_*) measured three ways; one JSON object to
--out (default profiles/dedup.json) and to stdout.

  (a) compressed disk path   store_paths(compress=True) over a corpus that is
      duplicate-heavy AND compressible, read from tmpfs: Zipf-distributed words
      (tools/bench_deflate.py text_corpus) laid out by oracle.zipf_corpus's
      scheme (a pool of 64 segments of 64 KiB..4 MiB, drawn Zipf(1.1)).  A run
      with a fresh set against a run with dedup=None (the yardstick: what the
      call did before the set existed), alternating, three each: GiB/s, the
      fresh fraction, compressed bytes produced, hbx_io_times.
  (b) device-resident pipeline   the schedule of tests/test_gpu_fullsize.py
      (_run_schedule: 64 x 128 MiB random per batch, R batches in flight, join
      lag 2, lead 2) with a set attached against set = NULL, alternating:
      the ratio beside the spread of the NULL runs.
  (c) mark rate   hbx_idset_insert of n = 1e5 and 1e6 new random IDs into a set
      of capacity 4e6 (host list in, flags out: the copies are in the time),
      and of the same IDs again (all seen).

Run on the GPU box: python tools/bench_dedup.py
"""
import argparse
import json
import os
import shutil
import sys
import time
from collections import deque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

GIB = 1 << 30


def text_zipf_files(d, n_files, file_bytes, seed):
    """n_files files of file_bytes each: segments drawn Zipf(1.1) from a pool of
    64 text segments of 64 KiB..4 MiB (oracle.zipf_corpus's scheme; the
    segments are slices of one 64 MiB text at random offsets)."""
    from bench_deflate import text_corpus
    g = np.random.Generator(np.random.PCG64(seed))
    base = text_corpus(64 << 20, seed)
    sizes = g.integers(64 * 1024, 4 * 1024 * 1024 + 1, 64)
    offs = [int(g.integers(0, base.size - int(s))) for s in sizes]
    segs = [base[o:o + int(s)] for o, s in zip(offs, sizes)]
    os.makedirs(d, exist_ok=True)
    paths = []
    for f in range(n_files):
        out = np.empty(file_bytes, np.uint8)
        pos = 0
        while pos < file_bytes:
            s = segs[int(min(g.zipf(1.1), 64)) - 1]
            take = min(s.size, file_bytes - pos)
            out[pos:pos + take] = s[:take]
            pos += take
        p = os.path.join(d, f"z{f:04d}.txt")
        out.tofile(p)
        paths.append(p)
    return paths


def leg_compressed(eng, paths, sizes, io_threads, batch_bytes, dedup):
    eng.io_times(reset=True)
    t0 = time.perf_counter()
    res = eng.store_paths(paths, io_threads, batch_bytes, compress=True, sizes=sizes, dedup=dedup)
    el = time.perf_counter() - t0
    io = eng.io_times()
    n = sum(r.n_chunks for r in res)
    zbytes = sum(int(z.size) for r in res for z in r.zstreams)
    out = {"seconds": round(el, 4), "gibs": round(sum(sizes) / el / GIB, 3), "chunks": n, "compressed_bytes": zbytes,
           "io_times_s": {"read_files": round(float(io[0]), 4), "wait_collect": round(float(io[1]), 4),
                          "wait_h2d": round(float(io[2]), 4)}}
    if dedup is not None:
        fresh_chunks = sum(int(r.fresh.sum()) for r in res)
        fresh_bytes = 0
        for r in res:
            starts, ends = r.chunk_bounds()
            fresh_bytes += int((ends - starts)[r.fresh].sum())
        out["fresh_chunk_fraction"] = round(fresh_chunks / max(n, 1), 4)
        out["fresh_byte_fraction"] = round(fresh_bytes / max(sum(sizes), 1), 4)
    return out


def part_a(a):
    from hashbox_amd import Engine, IdSet
    d = os.path.join(a.dir, "text")
    paths = text_zipf_files(d, a.files, a.file_mib << 20, 7)
    sizes = [a.file_mib << 20] * a.files
    legs = {"none": [], "set": []}
    try:
        with Engine(0) as eng:
            # warm-up: one whole pass (the first read of files just written is the slow one)
            eng.store_paths(paths, a.io_threads, a.batch_mib << 20, compress=True, sizes=sizes)
            for _ in range(a.runs):
                legs["none"].append(leg_compressed(eng, paths, sizes, a.io_threads, a.batch_mib << 20, None))
                with IdSet(eng, 1 << 20) as s:
                    legs["set"].append(leg_compressed(eng, paths, sizes, a.io_threads, a.batch_mib << 20, s))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    med = {k: float(np.median([r["gibs"] for r in v])) for k, v in legs.items()}
    return {"corpus": f"{a.files} x {a.file_mib} MiB Zipf text from tmpfs, batch {a.batch_mib} MiB, "
                      f"{a.io_threads} io threads",
            "runs": legs, "median_gibs": med, "gain": round(med["set"] / med["none"], 4),
            "compressed_bytes_ratio": round(legs["set"][-1]["compressed_bytes"] /
                                            max(legs["none"][-1]["compressed_bytes"], 1), 4)}


def run_schedule(arenas, offs, lens, steps, R, with_set, lag=2, lead=2):
    """tests/test_gpu_fullsize.py _run_schedule at lead == lag, timed."""
    import torch
    from hashbox_amd import Engine, IdSet
    nfull = ((8 << 20) + 8) >> 6
    B = -(-nfull // (R - lead))
    order = deque()
    got = []  # (counted after the clock stops: both legs do the same host work inside it)
    with Engine(0, md5_slice=B, join_lag=lag) as e:
        e.reserve(R + 2, len(lens), int(sum(lens)))
        s = IdSet(e, 1 << 20) if with_set else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(steps):
            if len(order) >= R:
                e.input_after_oldest()
            e.submit_device(arenas[j % len(arenas)].data_ptr(), offs, lens, dedup=s)
            order.append(j)
            if len(order) > R:
                order.popleft()
                got.append(e.wait())
        while order:
            order.popleft()
            got.append(e.wait())
        el = time.perf_counter() - t0
        total = sum(r.n_chunks for b in got for r in b)
        fresh = sum(int(r.fresh.sum()) for b in got for r in b) if with_set else 0
        count = s.count if with_set else None
        if s is not None:
            s.close()
    out = {"seconds": round(el, 4), "gibs": round(steps * sum(lens) / el / GIB, 1), "chunks": total}
    if with_set:
        out.update(fresh_chunks=fresh, set_count=count)
    return out


def part_b(a):
    import torch
    import workloads as W
    lens = [128 << 20] * 64
    offs, total = W.pack_layout(lens)
    arenas = W.random_arenas(3, total, 1000, torch.device("cuda", 0))
    run_schedule(arenas, offs, lens, a.steps, a.resident, False)  # warm-up
    legs = {"null": [], "set": []}
    for _ in range(a.runs):
        legs["null"].append(run_schedule(arenas, offs, lens, a.steps, a.resident, False))
        legs["set"].append(run_schedule(arenas, offs, lens, a.steps, a.resident, True))
    del arenas
    torch.cuda.empty_cache()
    nul = [r["gibs"] for r in legs["null"]]
    med = {k: float(np.median([r["gibs"] for r in v])) for k, v in legs.items()}
    return {"schedule": f"64 x 128 MiB random per batch, {a.steps} steps, R = {a.resident}, join lag 2, lead 2, "
                        "fill and drain included", "runs": legs, "median_gibs": med,
            "ratio_set_over_null": round(med["set"] / med["null"], 4),
            "null_spread": round((max(nul) - min(nul)) / med["null"], 4)}


def part_c(a):
    from hashbox_amd import Engine, IdSet
    out = {}
    with Engine(0) as eng:
        L = eng._L
        for n in (100_000, 1_000_000):
            new, seen = [], []
            for run in range(a.runs + 1):  # (run 0 warms the staging buffers up)
                ids = np.random.Generator(np.random.PCG64(100 + run)).integers(0, 256, (n, 16), dtype=np.uint8)
                flags = np.zeros(n, np.uint8)
                with IdSet(eng, 4_000_000) as s:
                    for dst in (new, seen):
                        t0 = time.perf_counter()
                        rc = L.hbx_idset_insert(eng._ctx, s._h, n, ids.ctypes.data, flags.ctypes.data)
                        dt = time.perf_counter() - t0
                        eng._check(rc, "hbx_idset_insert")
                        assert int(flags.sum()) == (n if dst is new else 0)
                        if run:
                            dst.append(n / dt)
            out[str(n)] = {"new_ids_per_s": [round(x) for x in new], "seen_ids_per_s": [round(x) for x in seen],
                           "median_new_ids_per_s": round(float(np.median(new))),
                           "median_seen_ids_per_s": round(float(np.median(seen)))}
    return {"set_capacity": 4_000_000, "what": "hbx_idset_insert wall time: H2D of the IDs, one mark, D2H of the flags",
            "n": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup.json"))
    ap.add_argument("--dir", default="/dev/shm/hbx_dedup")
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--file-mib", type=int, default=64)
    ap.add_argument("--batch-mib", type=int, default=1024)
    ap.add_argument("--io-threads", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--resident", type=int, default=33)
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: see hashbox_amd/_lib.py)
    res = {}
    if "a" in a.parts:
        res["compressed_path"] = part_a(a)
    if "b" in a.parts:
        res["device_pipeline"] = part_b(a)
    if "c" in a.parts:
        res["mark_rate"] = part_c(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
