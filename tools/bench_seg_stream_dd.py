#!/usr/bin/env python3
"""One file of any size through hbx_store_file_stream (segments + ID set +
compression + sink) against the paths it is built beside; one JSON object to
--out (default profiles/seg_stream_dd.json) and to stdout.

Corpus, on tmpfs: --gib GiB (default 8) of Zipf-word text laid out as
tools/bench_dedup.py does (a pool of 64 text segments drawn Zipf(1.1)), once as
ONE file and once as the same bytes cut into 128 MiB files.  One process, one
warm-up pass over every leg, then --runs (default 3) alternating runs per leg,
512 MiB segments and 16 reader threads:

  (a) hbx_store_file_seg                       the yardstick of the plain path
  (b) hbx_store_file_stream, no set, no compression, a sink that only counts
  (c) hbx_store_file_stream, HBX_STREAM_COMPRESS and a fresh set; the sink
      adds up the stream bytes (it reads zlen, not the streams)
  (d) hbx_store_paths_dd, compression and a fresh set, over the 128 MiB files
      (1 GiB batches): the yardstick of the compressed path

Per leg: GiB/s of file bytes, chunks, fresh share, stream bytes, hbx_io_times.
Expectation: (b) within the spread of (a); (c) >= (1 - OVERLAP/seg) x (d) less
(d)'s spread.

Run on the GPU box: python tools/bench_seg_stream_dd.py
"""
import argparse
import ctypes
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
PIECE = 128 << 20


def io_dict(eng):
    io = eng.io_times()
    return {"read_files": round(float(io[0]), 4), "wait_collect": round(float(io[1]), 4),
            "wait_h2d": round(float(io[2]), 4)}


def leg_seg(eng, path, n, seg, threads):
    eng.io_times(reset=True)
    t0 = time.perf_counter()
    r = eng.store_file(path, segment_bytes=seg, io_threads=threads)
    el = time.perf_counter() - t0
    return {"seconds": round(el, 4), "gibs": round(n / el / GIB, 3), "chunks": r.n_chunks, "io_times_s": io_dict(eng)}


def leg_stream(eng, path, n, seg, threads, compress, idset):
    from hashbox_amd import _lib
    tot = {"segments": 0, "chunks": 0, "fresh": 0, "zbytes": 0}

    def sink(_user, p):
        s = p.contents
        k = int(s.n_chunks)
        tot["segments"] += 1
        tot["chunks"] += k
        if k and s.fresh:
            tot["fresh"] += int(np.frombuffer((ctypes.c_uint8 * k).from_address(s.fresh), np.uint8).sum())
        if k and s.zlen:
            tot["zbytes"] += int(np.frombuffer((ctypes.c_uint64 * k).from_address(s.zlen), np.uint64).sum())
        return 0

    cb = _lib.SEG_SINK(sink)
    summ = _lib.FileSummary()
    eng.io_times(reset=True)
    t0 = time.perf_counter()
    rc = eng._L.hbx_store_file_stream(eng._ctx, os.fsencode(path), n, seg, threads,
                                      _lib.STREAM_COMPRESS if compress else 0, idset._h if idset else None,
                                      ctypes.cast(cb, ctypes.c_void_p), None, ctypes.byref(summ))
    el = time.perf_counter() - t0
    eng._check(rc, "hbx_store_file_stream")
    assert tot["chunks"] == summ.n_chunks
    out = {"seconds": round(el, 4), "gibs": round(n / el / GIB, 3), "chunks": tot["chunks"],
           "segments": tot["segments"], "io_times_s": io_dict(eng)}
    if idset is not None:
        out["fresh_chunk_fraction"] = round(tot["fresh"] / max(tot["chunks"], 1), 4)
    if compress:
        out["compressed_bytes"] = tot["zbytes"]
    return out


def leg_paths(eng, paths, sizes, threads, batch, idset):
    eng.io_times(reset=True)
    t0 = time.perf_counter()
    res = eng.store_paths(paths, threads, batch, compress=True, sizes=sizes, dedup=idset)
    el = time.perf_counter() - t0
    n = sum(r.n_chunks for r in res)
    return {"seconds": round(el, 4), "gibs": round(sum(sizes) / el / GIB, 3), "chunks": n,
            "fresh_chunk_fraction": round(sum(int(r.fresh.sum()) for r in res) / max(n, 1), 4),
            "compressed_bytes": sum(int(z.size) for r in res for z in r.zstreams), "io_times_s": io_dict(eng)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_stream_dd.json"))
    ap.add_argument("--dir", default="/dev/shm/hbx_seg_stream_dd")
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--seg-mib", type=int, default=512)
    ap.add_argument("--batch-mib", type=int, default=1024)
    ap.add_argument("--io-threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: see hashbox_amd/_lib.py)
    from bench_dedup import text_zipf_files
    from hashbox_amd import SEG_OVERLAP, Engine, IdSet
    pieces = max(1, int(a.gib * GIB) // PIECE)
    n = pieces * PIECE
    seg = a.seg_mib << 20
    try:
        paths = text_zipf_files(os.path.join(a.dir, "pieces"), pieces, PIECE, 7)
        one = os.path.join(a.dir, "one.txt")
        with open(one, "wb") as out:
            for p in paths:
                with open(p, "rb") as fh:
                    shutil.copyfileobj(fh, out, 16 << 20)
        sizes = [PIECE] * pieces
        names = ["a_store_file_seg", "b_stream_plain", "c_stream_compress_set", "d_store_paths_dd"]
        legs = {k: [] for k in names}
        with Engine(0) as eng:
            def run(name):
                if name == names[0]:
                    return leg_seg(eng, one, n, seg, a.io_threads)
                if name == names[1]:
                    return leg_stream(eng, one, n, seg, a.io_threads, False, None)
                with IdSet(eng, 1 << 20) as s:
                    if name == names[2]:
                        return leg_stream(eng, one, n, seg, a.io_threads, True, s)
                    return leg_paths(eng, paths, sizes, a.io_threads, a.batch_mib << 20, s)
            for name in names:  # warm-up: the first read of files just written, every buffer sized
                run(name)
            for _ in range(a.runs):
                for name in names:
                    legs[name].append(run(name))
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    g = {k: [r["gibs"] for r in v] for k, v in legs.items()}
    med = {k: float(np.median(v)) for k, v in g.items()}
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in g.items()}
    res = {"corpus": f"{n / GIB:g} GiB Zipf text on tmpfs as one file ({a.seg_mib} MiB segments) and as {pieces} x "
                     f"128 MiB files ({a.batch_mib} MiB batches), {a.io_threads} io threads",
           "runs": legs, "median_gibs": med, "spread": spread,
           "b_over_a": round(med[names[1]] / med[names[0]], 4),
           "c_over_d": round(med[names[2]] / med[names[3]], 4),
           "expected_c_over_d": round(1 - SEG_OVERLAP / seg, 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
