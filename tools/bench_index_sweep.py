#!/usr/bin/env python3
"""The index files on the device (K17, Engine.open_index) at full size: one
index file of 2^24 + 682 slots with --entries (8 Mi) entries; lookup of every
ID, scan, sweep and compact timed beside two baselines.  One JSON object to
--out (default profiles/index_sweep.json) and stdout.

The file is laid out with numpy as linear probing lays it out: the IDs sorted
by home, slot = maximum.accumulate(home - rank) + rank.  10 % of the entries
are Invalid beforehand and 60 % of the rest Marked (--invalid, --marked).

  device  the wall time of the Index call (its kernels, and the copies of its
          results to host memory): one warm-up, the median of --runs (3).  A
          sweep changes the index, so every round opens it again.
  host    hbx_index_*_host on one thread over a host copy of the image.  The
          reference is one goroutine that also pays a seek and a read per probe.
  copy    a device-to-device copy of the image (torch's copy_, timed with
          events): the bandwidth floor of a pass that reads and writes it once.

The IDs are looked up in a seeded random order, as a mark meets them.

EVERY device result is asserted equal to the host call's.  No bar is set.  The
kernels' own times are not taken here: run once more with --runs 1 under
`rocprofv3 --kernel-trace --stats` and give the kernel statistics file to
--kernel-stats on the timed run: it adds every K17 kernel's time per launch.

Run on the GPU box: python tools/bench_index_sweep.py
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

E, N, M, I = 1, 2, 4, 8
HOMES, PROBES = 1 << 24, 682


def build(n: int, seed: int, invalid: float, marked: float):
    """(image, ids): the file as a uint8 array and the IDs of its entries, uint8 [n, 16], in slot order."""
    rng = np.random.default_rng(seed)
    ids = np.frombuffer(rng.bytes(16 * n), np.uint8).reshape(n, 16)
    home = (ids[:, 13].astype(np.int64) << 16) | (ids[:, 14].astype(np.int64) << 8) | ids[:, 15]
    order = np.argsort(home, kind="stable")
    ids, home = ids[order], home[order]
    rank = np.arange(n, dtype=np.int64)
    slot = np.maximum.accumulate(home - rank) + rank
    assert int((slot - home).max()) < PROBES and int(slot[-1]) < HOMES + PROBES
    flags = np.full(n, E, np.uint8) | np.where(rng.random(n) < 0.5, N, 0).astype(np.uint8)
    inv = rng.random(n) < invalid
    flags |= np.where(inv, I, 0).astype(np.uint8)
    flags |= np.where(~inv & (rng.random(n) < marked), M, 0).astype(np.uint8)
    rec = np.zeros((n, 24), np.uint8)
    rec[:, 1] = flags
    rec[:, 2:18] = ids
    loc = ((rng.integers(0, 4, n).astype(np.uint64) << np.uint64(34)) | (np.uint64(16) + np.uint64(34) * rank.astype(np.uint64)))
    rec[:, 18:] = loc.astype(">u8").view(np.uint8).reshape(n, 8)[:, 2:]
    image = np.zeros(16 + 24 * (HOMES + PROBES), np.uint8)
    image[:16] = np.frombuffer(b"HSIX\0\0\0\1" + bytes(8), np.uint8)
    image[16:].reshape(-1, 24)[slot] = rec
    return image, np.ascontiguousarray(ids)


class Host:
    """hbx_index_*_host over one image, in place."""

    def __init__(self, L, image):
        self.L, self.buf = L, image
        self.ptrs = (ctypes.c_void_p * 1)(image.ctypes.data)
        self.size = np.array([image.shape[0]], np.uint64)
        self.caps = np.array([image.shape[0]], np.uint64)

    def head(self):
        return 1, self.ptrs, self.size.ctypes.data, self.caps.ctypes.data


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_sweep.json"))
    ap.add_argument("--entries", type=int, default=8 << 20)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--invalid", type=float, default=0.10)
    ap.add_argument("--marked", type=float, default=0.60)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's kernel statistics CSV of a --runs 1 run")
    a = ap.parse_args()
    import torch
    from hashbox_amd import Engine, _lib
    from hashbox_amd.engine import IX_HIT_DTYPE, IX_KILLED_DTYPE, IX_LIVE_DTYPE
    L = _lib.load()
    t, (image, ids) = timed(lambda: build(a.entries, a.seed, a.invalid, a.marked))
    n = ids.shape[0]
    ids = np.ascontiguousarray(ids[np.random.default_rng([a.seed, 1]).permutation(n)])
    print(f"image of {image.shape[0]} bytes with {n} entries built in {t:.1f} s", file=sys.stderr, flush=True)
    res = {"lib": _lib.identity(), "bytes": int(image.shape[0]), "entries": n, "invalid": a.invalid, "marked": a.marked,
           "host_s": {}, "device_s": {}}

    # ---- the host calls: the baseline, and what the device must give
    h = Host(L, image.copy())
    hits = np.zeros(n, IX_HIT_DTYPE)
    res["host_s"]["lookup"], rc = timed(lambda: L.hbx_index_lookup_host(*h.head(), n, ids.ctypes.data, 0, hits.ctypes.data))
    assert rc == 0
    live, ssum = np.zeros(n, IX_LIVE_DTYPE), _lib.IxSummary()
    res["host_s"]["scan"], rc = timed(lambda: L.hbx_index_scan_host(*h.head(), live.ctypes.data, n, None, ctypes.byref(ssum)))
    assert rc == 0
    n_live = int(ssum.n_live)
    act, mv = np.zeros(n_live, np.uint8), np.zeros((n_live, 2), np.uint64)
    kl, wsum = np.zeros(n_live, IX_KILLED_DTYPE), _lib.IxSweepSummary()
    res["host_s"]["sweep"], rc = timed(lambda: L.hbx_index_sweep_host(*h.head(), act.ctypes.data, mv.ctypes.data, n_live,
                                                                    kl.ctypes.data, n_live, ctypes.byref(wsum)))
    assert rc == 0, rc
    swept = h.buf.copy()
    csum = _lib.IxCompactSummary()
    res["host_s"]["compact"], rc = timed(lambda: L.hbx_index_compact_host(*h.head(), ctypes.byref(csum)))
    assert rc == 0
    res["scan_summary"] = {k: int(getattr(ssum, k)) for k, _ in ssum._fields_}
    res["sweep_summary"] = {k: int(getattr(wsum, k)) for k, _ in wsum._fields_}
    res["compact"] = {"cleared": int(csum.cleared), "size": int(csum.size[0])}
    print("host", res["host_s"], res["sweep_summary"], file=sys.stderr, flush=True)

    # ---- the device
    legs = {k: [] for k in ("open", "lookup", "scan", "sweep", "compact", "export")}
    with Engine(0) as eng:
        for k in range(a.runs + 1):  # the first round is the warm-up
            t_open, ix = timed(lambda: eng.open_index([image]))
            t_lookup, g_hits = timed(lambda: ix.lookup(ids))
            t_scan, g_scan = timed(lambda: ix.scan(n))
            t_sweep, g_sweep = timed(lambda: ix.sweep(n))
            assert ix.export(0) == swept.tobytes()
            t_compact, g_c = timed(ix.compact)
            t_export, out = timed(lambda: ix.export(0))
            ix.close()
            assert g_hits.tobytes() == hits.tobytes()
            assert g_scan.live.tobytes() == live[:n_live].tobytes() and g_scan.summary == res["scan_summary"]
            assert g_sweep.action.tobytes() == act.tobytes() and g_sweep.moved_to.tobytes() == mv.tobytes()
            assert g_sweep.killed.tobytes() == kl[:int(wsum.n_deleted)].tobytes()
            assert g_c == {"cleared": res["compact"]["cleared"], "sizes": [res["compact"]["size"]]}
            assert out == h.buf[:int(h.size[0])].tobytes()
            del g_hits, g_scan, g_sweep, out
            row = dict(open=t_open, lookup=t_lookup, scan=t_scan, sweep=t_sweep, compact=t_compact, export=t_export)
            print("device", {x: round(v, 4) for x, v in row.items()}, file=sys.stderr, flush=True)
            if k:
                for x, v in row.items():
                    legs[x].append(round(v, 5))
    res["device_s"] = {x: {"runs": v, "median": float(np.median(v))} for x, v in legs.items()}
    # ---- the floor: the image copied device to device
    src = torch.empty(image.shape[0], dtype=torch.uint8, device="cuda:0").random_(0, 256)
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
    res["copy_s"] = {"runs": copy, "median": float(np.median(copy))}
    res["host_over_device"] = {x: round(res["host_s"][x] / res["device_s"][x]["median"], 1) for x in res["host_s"]}
    if a.kernel_stats:
        with open(a.kernel_stats, newline="") as fh:
            res["kernels_ms_per_launch"] = {r["Name"]: [int(r["Calls"]), round(int(r["TotalDurationNs"]) / int(r["Calls"]) / 1e6, 4)]
                                            for r in csv.DictReader(fh) if r["Name"].startswith(("hbx_k17_", "hbx_k15_scan"))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"host_s": {x: round(v, 3) for x, v in res["host_s"].items()},
                      "device_s": {x: v["median"] for x, v in res["device_s"].items()}, "copy_s": res["copy_s"]["median"]}))


if __name__ == "__main__":
    main()
