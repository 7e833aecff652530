#!/usr/bin/env python3
"""Check one synthetic storage data file on the device (K14 + K8 / K8s + K6,
Engine.check_datfile): device-resident and from a path, beside a CPU baseline;
one JSON object to --out (default profiles/datfile_check.json) and stdout.

The file (--gib GiB, default 2, from --seed): entries whose data are Zipf text
(slices of a 32 MiB seeded pool, 70 %) or random bytes, data blocks of
64 KiB-8 MiB (log-uniform, 70 % zlib at level 6, else raw) mixed with small
directory-like blocks of 60-600 bytes with 1-40 links (half of the entries, a
sliver of the bytes), a gap every 25th item; 1 % of the entries get one
flipped byte (ID, data field, link) or a DataType of 2.  It is built in memory
by tests/datfile_craft.py's writer and checked once by its pure-Python
reference; EVERY timed run's result is asserted equal to that reference.

  device   the image already in HBM (hbx_datfile_check_device)
  path     the file under --dir, default /dev/shm (hbx_datfile_check_path)
  cpu      the CPU baseline: --threads (16) host threads doing zlib.decompress
           + hashlib.md5 over the same entries at offsets the reference found
           (no scan, no walk: it is told where the entries are)

One warm-up of each, then --runs (3) alternating rounds; medians in seconds and
GiB/s of file bytes.  No bar is set for the times.  K14's own kernel times are
not taken here: run this tool with --device-only --runs 1 under
`rocprofv3 --kernel-trace --stats` for them.

Run on the GPU box: python tools/bench_datfile_check.py
"""
import argparse
import hashlib
import json
import os
import random
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GIB = 1 << 30
MB = 8 << 20


def make_file(total: int, seed: int, threads: int):
    from tests import datfile_craft as C
    r = random.Random(f"bench-dat-{seed}")
    pool = C.text(32 << 20, f"pool-{seed}")
    specs, est, k = [], 16, 0
    while est < total:
        k += 1
        if k % 25 == 0:
            specs.append(("gap", r.randint(12, 1 << 16)))
            est += specs[-1][1]
            continue
        if k % 2:
            n, nl = r.randint(60, 600), r.randint(1, 40)
        else:
            n, nl = int(2 ** r.uniform(16, 23)), 0
        dtype = C.ZLIB if r.random() < 0.7 else C.RAW
        damage = r.choice(["id", "data", "link" if nl else "id", "type2"]) if r.random() < 0.01 else None
        specs.append((n, nl, r.random() < 0.7, r.randrange(len(pool) - (8 << 20)), dtype, damage))
        est += n // (3 if dtype == C.ZLIB else 1) + 29 + 16 * nl

    def build(spec):
        if spec[0] == "gap":
            return C.gap(spec[1])
        n, nl, is_text, at, dtype, damage = spec
        data = pool[at:at + n] if is_text else np.random.default_rng([seed, at, n]).integers(0, 256, n, np.uint8).tobytes()
        links = [hashlib.md5(struct.pack(">QI", at, j)).digest() for j in range(nl)]
        return C.write_datfile([(links, data, dtype, damage)])[0][16:]
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(build, specs))
    return C.header() + b"".join(parts), C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "datfile_check.json"))
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=14)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="no path and no cpu leg (for a profiler run)")
    a = ap.parse_args()
    from hashbox_amd import Engine, _lib
    t0 = time.perf_counter()
    buf, C = make_file(int(a.gib * GIB), a.seed, a.threads)
    t_make = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = C.ref_check(buf, MB)
    t_ref = time.perf_counter() - t0
    s = ref["summary"]
    assert C.invariant(s)
    print(f"file {len(buf) / GIB:.3f} GiB built in {t_make:.1f} s, reference in {t_ref:.1f} s: {s}", file=sys.stderr, flush=True)
    path = os.path.join(a.dir, f"hbx_datfile_check_{os.getpid()}.dat")
    want_e = np.array([e["off"] for e in ref["entries"]], np.uint64)
    want_s = [(x["off"], x["len"], x["kind"], x["status"], x["n_failed"]) for x in ref["spans"]]

    def same(res):
        assert res.summary == s, {k: (res.summary[k], s[k]) for k in s if res.summary[k] != s[k]}
        assert np.array_equal(res.entries["off"], want_e)
        assert res.entries["id"].tobytes() == b"".join(e["id"] for e in ref["entries"])
        assert [int(p) for p in res.entries["plain_len"]] == [e["plain_len"] for e in ref["entries"]]
        assert [tuple(int(x[f]) for f in ("off", "len", "kind", "status", "n_failed")) for x in res.spans] == want_s
        assert res.links.tobytes() == ref["links"]

    def cpu_entry(e):
        field = buf[e["data_off"]:e["data_off"] + e["data_len"]]
        data = zlib.decompress(field) if e["type"] == C.ZLIB else field
        lo = e["off"] + 24
        h = hashlib.md5(struct.pack(">I", e["n_links"]))
        h.update(buf[lo:lo + 16 * e["n_links"]])
        h.update(struct.pack(">I", len(data)))
        h.update(data)
        return h.digest() == e["id"]

    legs = ["device"] if a.device_only else ["device", "path", "cpu"]
    runs = {n: [] for n in legs}
    try:
        with Engine(0) as eng, ThreadPoolExecutor(a.threads) as ex:
            d, n, _, arena = eng._dat_image(buf, None)
            if "path" in legs:
                with open(path, "wb") as fh:
                    fh.write(buf)

            def run(leg):
                t0 = time.perf_counter()
                if leg == "device":
                    res = eng.check_datfile(d.value, max_block=MB, size=n)
                elif leg == "path":
                    res = eng.check_datfile(path, max_block=MB)
                else:
                    assert all(ex.map(cpu_entry, ref["entries"], chunksize=64))
                el = time.perf_counter() - t0
                if leg != "cpu":
                    same(res)
                return round(el, 4)
            for leg in legs:
                run(leg)
            for _ in range(a.runs):
                for leg in legs:
                    runs[leg].append(run(leg))
                    print(leg, runs[leg][-1], eng.knobs()["datfile"], file=sys.stderr, flush=True)
            knobs = eng.knobs()
            eng._L.hbx_arena_free(eng._ctx, arena)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    med = {n: float(np.median(runs[n])) for n in legs}
    summary = {"seconds": {n: round(v, 4) for n, v in med.items()},
               "gib_per_s": {n: round(len(buf) / GIB / v, 3) for n, v in med.items()},
               "windows_retries": knobs["datfile"]}
    result = {"file": f"{len(buf) / GIB:.3f} GiB, seed {a.seed}: {s['n_candidates']} markers, {s['n_entries']} good entries "
                      f"({s['entry_bytes']} bytes), {s['n_gaps']} gaps, {s['n_broken']} broken spans "
                      f"({s['broken_bytes']} bytes), {s['n_links']} links; max_block 8 MiB; {a.threads} threads",
              "bytes": len(buf), "reference": s, "lib": _lib.identity(), "summary": summary, "runs": runs,
              "cpu_baseline": "zlib.decompress + hashlib.md5 over the good entries at known offsets"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
