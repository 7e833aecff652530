#!/usr/bin/env python3
"""Compact two synthetic storage data files on the device (K16,
Engine.compact_datfile) beside a device-to-device copy and a one-thread host
join; one JSON object to --out (default profiles/datfile_compact.json) and
stdout.

  large   the file of tools/bench_datfile_check.py (--gib 2, --seed 14: data
          blocks of 64 KiB-8 MiB mixed with small blocks of 1-40 links); its
          entries are those the device check finds
  small   --small (8 Mi) entries of 29 bytes to 2 KiB (log-uniform, raw, no
          links, --small-seed 16) back to back behind the header, built with
          numpy; the table is known from the construction

Both with a seeded keep mask of --keep (0.7) and without KEEP_PREFIX, so every
kept entry moves.  Per image, with the image resident in device memory:

  call    the wall time of Engine.compact_datfile with every output (the plan,
          the three device streams and their copies to host memory): one
          warm-up, the median of --runs (3)
  plan    the same call with no stream wanted: the plan alone
  copy    a device-to-device copy of moved_bytes (torch's copy_ between two
          contiguous uint8 tensors, timed with events on the current stream; it
          may run as a copy kernel, not as the runtime's hipMemcpy path): the
          yardstick for hbx_k16_pack, which reads and writes the same bytes
  host    the reference's join on one host thread: b"".join over memoryview
          slices of the file

EVERY timed result is asserted equal to the reference: tests/compact_craft.py's
ref_compact for the large image, a numpy restatement of the same rules for the
small one (a Python loop over 8 Mi entries would outlast the run).  No bar is
set.  The kernels' own times are not taken here: run with --device-only
--runs 1 --images large (then small) under `rocprofv3 --kernel-trace --stats`
and give each kernel statistics file to --kernel-stats IMAGE=FILE on the timed
run: it adds every K16 kernel's time and hbx_k16_pack's GB/s, read plus
written, per launch of that run.  --cache DIR keeps the built images between
runs.

Run on the GPU box: python tools/bench_datfile_compact.py
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

GIB = 1 << 30


def small_image(n: int, seed: int):
    """The file (a uint8 array) of n raw entries without links."""
    rng = np.random.default_rng(seed)
    size = np.floor(29 * (2048 / 29) ** rng.random(n)).astype(np.int64)
    off = 16 + np.concatenate([[0], np.cumsum(size)[:-1]])
    total = int(off[-1] + size[-1])
    buf = np.frombuffer(rng.bytes(total), np.uint8).copy()
    buf[:16] = np.frombuffer(b"HSDB\0\0\0\1" + bytes(8), np.uint8)
    dl = (size - 29).astype(">u4").view(np.uint8).reshape(n, 4)
    for j, b in enumerate(b"hblk"):
        buf[off + j] = b
    for j in range(4):
        buf[off + 20 + j] = 0          # n_links
        buf[off + 25 + j] = dl[:, j]   # data_len
    buf[off + 24] = 0xFF               # DataType raw
    return buf


def numpy_reference(buf, e, keep, join=True):
    """ref_compact's rules for a table without links, no KEEP_PREFIX, bases 16, files 0."""
    n = e.shape[0]
    size = e["size"].astype(np.int64)
    msz = np.where(keep, size, 0)
    new_off = np.where(keep, 16 + np.cumsum(msz) - msz, -1).astype(np.uint64)
    meta_off = np.where(keep, 16 + 34 * (np.cumsum(keep) - keep), -1).astype(np.uint64)
    kept = np.flatnonzero(keep)

    def loc(off):  # sixByteLocation of file 0
        return off.astype(">u8").view(np.uint8).reshape(-1, 8)[:, 2:]
    meta = np.zeros((kept.size, 34), np.uint8)
    meta[:, :4] = np.frombuffer(b"hblk", np.uint8)
    meta[:, 4:20] = e["id"][kept]
    meta[:, 20:26] = loc(new_off[kept])
    meta[:, 26:30] = size[kept].astype(">u4").view(np.uint8).reshape(-1, 4)
    ix = np.zeros((kept.size, 24), np.uint8)
    ix[:, 1] = 3  # Exists | NoLinks
    ix[:, 2:18] = e["id"][kept]
    ix[:, 18:] = loc(meta_off[kept])
    moved_bytes = int(msz.sum())
    summary = dict(n_entries=n, n_stay=0, n_moved=int(kept.size), n_dropped=n - int(kept.size), stay_end=16,
                   moved_bytes=moved_bytes, dropped_bytes=int(size.sum()) - moved_bytes,
                   deleted_bytes=buf.shape[0] - 16 - moved_bytes, meta_bytes=34 * int(kept.size), n_meta=int(kept.size),
                   first_past_limit=None)
    out = dict(klass=np.where(keep, 2, 0).astype(np.uint8), new_off=new_off, meta_off=meta_off, meta=meta.tobytes(),
               ix=ix.tobytes(), summary=summary)
    if join:
        t0 = time.perf_counter()
        out["moved"] = host_join(buf, e["off"][kept], size[kept])
        out["join_s"] = time.perf_counter() - t0
    return out


def host_join(buf, offs, sizes) -> bytes:
    mv = memoryview(buf)
    return b"".join([mv[o:o + s] for o, s in zip(offs.tolist(), sizes.tolist())])


def pack_from_stats(path):
    """{kernel: (calls, total ns)} of the hbx_k16_* kernels from a rocprofv3 kernel statistics CSV."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            if row["Name"].startswith(("hbx_k16_", "hbx_k15_scan")):
                out[row["Name"]] = (int(row["Calls"]), int(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "datfile_compact.json"))
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=14)
    ap.add_argument("--small", type=int, default=8 << 20)
    ap.add_argument("--small-seed", type=int, default=16)
    ap.add_argument("--keep", type=float, default=0.7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--images", default="large,small")
    ap.add_argument("--cache", default=None, help="a directory that keeps the built images between runs")
    ap.add_argument("--device-only", action="store_true", help="one untimed-by-host leg per image (for a profiler run)")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="IMAGE=FILE",
                    help="rocprofv3's kernel statistics CSV of a --device-only --runs 1 --images IMAGE run")
    a = ap.parse_args()
    import torch
    from hashbox_amd import Engine, _lib
    from tests import compact_craft as C
    import bench_datfile_check as B
    result = {"lib": _lib.identity(), "keep": a.keep, "images": {}}
    stats = {x.split("=", 1)[0]: pack_from_stats(x.split("=", 1)[1]) for x in a.kernel_stats}

    def cached(name, make):
        p = os.path.join(a.cache, name + ".npy") if a.cache else None
        if p and os.path.exists(p):
            return np.load(p)
        v = make()
        if p:
            os.makedirs(a.cache, exist_ok=True)
            np.save(p, v)
        return v

    with Engine(0) as eng:
        for image in a.images.split(","):
            t0 = time.perf_counter()
            if image == "large":
                buf = cached(f"large-{a.gib}-{a.seed}", lambda: np.frombuffer(B.make_file(int(a.gib * GIB), a.seed, a.threads)[0], np.uint8))
            else:
                buf = cached(f"small-{a.small}-{a.small_seed}", lambda: small_image(a.small, a.small_seed))
            d, n, _, arena = eng._dat_image(buf, None)
            if image == "large":
                entries = eng.check_datfile(d.value, max_block=8 << 20, size=n, links=False).entries
            else:
                entries = small_image_entries(buf, a.small, a.small_seed)
            keep = np.random.default_rng([a.seed, 70]).random(entries.shape[0]) < a.keep
            print(f"{image}: {n / GIB:.3f} GiB, {entries.shape[0]} entries ready in {time.perf_counter() - t0:.1f} s",
                  file=sys.stderr, flush=True)
            kw = dict(keep_prefix=False, size=n)
            if a.device_only:
                for _ in range(a.runs + 1):
                    r = eng.compact_datfile(d.value, entries, keep, **kw)
                result["images"][image] = {"summary": r.summary}
                eng._L.hbx_arena_free(eng._ctx, arena)
                continue
            # the reference, and the host join's time
            if image == "large":
                ents = [dict(off=int(x["off"]), size=int(x["size"]), n_links=int(x["n_links"]), data_len=int(x["data_len"]),
                             id=x["id"].tobytes()) for x in entries]
                mv = memoryview(buf)
                want = C.ref_compact(mv, ents, keep.tolist(), keep_prefix=False)
                want = {**want, "klass": np.array(want["klass"], np.uint8), "new_off": np.array(want["new_off"], np.uint64),
                        "meta_off": np.array(want["meta_off"], np.uint64)}
                kept = np.flatnonzero(keep)
                t0 = time.perf_counter()
                joined = host_join(buf, entries["off"][kept], entries["size"][kept])
                join_s = time.perf_counter() - t0
                assert joined == want["moved"]
                del joined
            else:
                want = numpy_reference(buf, entries, keep)
                join_s = want["join_s"]

            def same(r, streams=True):
                assert np.array_equal(r.klass, want["klass"]) and np.array_equal(r.new_off, want["new_off"])
                assert np.array_equal(r.meta_off, want["meta_off"])
                assert r.summary == want["summary"], (r.summary, want["summary"])
                if streams:
                    assert r.meta == want["meta"] and r.ix.tobytes() == want["ix"]
                    assert r.moved == want["moved"]
            call, plan = [], []
            for k in range(a.runs + 1):  # the first is the warm-up
                t0 = time.perf_counter()
                r = eng.compact_datfile(d.value, entries, keep, **kw)
                el = time.perf_counter() - t0
                same(r)
                del r
                t0 = time.perf_counter()
                r = eng.compact_datfile(d.value, entries, keep, moved=False, meta=False, ix=False, **kw)
                pl = time.perf_counter() - t0
                same(r, streams=False)
                if k:
                    call.append(round(el, 4))
                    plan.append(round(pl, 4))
                print(image, "call", round(el, 4), "plan", round(pl, 4), file=sys.stderr, flush=True)
            # the ceiling: the moved bytes copied device to device
            mb = want["summary"]["moved_bytes"]
            src = torch.empty(mb, dtype=torch.uint8, device="cuda:0").random_(0, 256)
            dst = torch.empty_like(src)
            copy = []
            for k in range(a.runs + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                dst.copy_(src)
                ev[1].record()
                torch.cuda.synchronize()
                if k:
                    copy.append(round(ev[0].elapsed_time(ev[1]) / 1e3, 6))
            del src, dst
            torch.cuda.empty_cache()
            copy_s = float(np.median(copy))
            leg = {"bytes": n, "n_entries": int(entries.shape[0]), "summary": want["summary"],
                   "call_s": call, "call_median_s": float(np.median(call)), "plan_s": plan,
                   "plan_median_s": float(np.median(plan)), "copy_s": copy,
                   "copy_gb_per_s_read_plus_written": round(2 * mb / copy_s / 1e9, 1),
                   "host_join_s": round(join_s, 4), "host_join_gb_per_s_read_plus_written": round(2 * mb / join_s / 1e9, 2)}
            if image in stats:
                st = stats[image]
                leg["kernels_ms_per_launch"] = {k: round(ns / c / 1e6, 4) for k, (c, ns) in sorted(st.items())}
                if "hbx_k16_pack" in st:
                    c, ns = st["hbx_k16_pack"]
                    leg["pack_gb_per_s_read_plus_written"] = round(2 * mb / (ns / c), 1)
                    leg["pack_ns_per_moved_entry"] = round(ns / c / max(want["summary"]["n_moved"], 1), 3)
                    leg["pack_over_copy"] = round((2 * mb / (ns / c)) / (2 * mb / copy_s / 1e9), 3)
            result["images"][image] = leg
            eng._L.hbx_arena_free(eng._ctx, arena)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: {f: v.get(f) for f in ("call_median_s", "plan_median_s", "copy_gb_per_s_read_plus_written",
                                                "host_join_s")} for k, v in result["images"].items()}))


def small_image_entries(buf, n, seed):
    """The table of small_image(n, seed) again (the sizes come from the seed, the IDs from the image)."""
    from hashbox_amd.engine import DAT_ENTRY_DTYPE
    rng = np.random.default_rng(seed)
    size = np.floor(29 * (2048 / 29) ** rng.random(n)).astype(np.int64)
    off = 16 + np.concatenate([[0], np.cumsum(size)[:-1]])
    e = np.zeros(n, DAT_ENTRY_DTYPE)
    e["off"], e["size"], e["data_off"], e["data_len"], e["type"] = off, size, off + 29, size - 29, 0xFF
    for j in range(16):
        e["id"][:, j] = buf[off + 4 + j]
    return e


if __name__ == "__main__":
    main()
