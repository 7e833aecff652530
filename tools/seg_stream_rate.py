#!/usr/bin/env python3
"""Rate of one file streamed through the pipeline in segments (hbx_seg_*),
against the same bytes submitted as independent single-file batches.

Device-resident over aliased read-only arenas, as bench.py and
tests/test_gpu_fullsize._run_schedule run: every segment of the synthetic
file reads one of a few random arenas (the kernels do the work of a real
file; the carry still goes from each segment's cut kernel to the next), under
the schedule hbx_plan_pipeline gives for one file per batch.  The yardstick
leg submits the same arenas with hbx_submit_device, the path this feature
leaves as it was.  GiB/s counts FILE bytes: the overlap once.

Legs (each in a child process of its own, under its own time limit):
  stream  <seg GiB>   segmented and independent, alternating, `--repeats` each
  disk                hbx_store_file_seg of one file vs hbx_store_paths of the
                      same bytes as 128 MiB files
  k5                  the block-id kernel's rate (the final FileChainBlock id)
The parent collects their JSON lines into --out (profiles/seg_stream.json).

    python tools/seg_stream_rate.py --out profiles/seg_stream.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GiB = 1 << 30
OVERLAP = 8 << 20


def leg_stream(seg_bytes: int, segments: int, repeats: int) -> dict:
    import numpy as np
    import torch
    import workloads as W
    from hashbox_amd import Engine
    dev = torch.device("cuda", 0)
    n_arenas = 3
    arenas = W.random_arenas(n_arenas, seg_bytes + 65536, 4242, dev)
    torch.cuda.synchronize()
    file_len = segments * seg_bytes - (segments - 1) * OVERLAP
    out = {"seg_bytes": seg_bytes, "segments": segments, "file_bytes": file_len, "seg": [], "independent": []}
    with Engine(0) as e:
        # the plan for R aliased arenas of one file each (bench.py --alias-depth: R is not bounded by HBM here)
        plan = e.plan_pipeline(n_files=1, arena_bytes=seg_bytes + 64, longest_file=seg_bytes, arenas=33,
                               free_bytes=256 * GiB, steps=segments)
        e.apply_plan(plan, 1, seg_bytes)
        out["plan"] = plan
        R, lag, lead = plan["resident"], plan["join_lag"], plan["lead"]

        def run(segmented: bool) -> float:
            order = 0
            f = e.seg_open(file_len) if segmented else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(segments):
                if order >= R and lead > lag:  # (as tests/test_gpu_fullsize._run_schedule)
                    e.wait()
                    order -= 1
                elif order >= R:
                    e.input_after_oldest()
                a = arenas[j % n_arenas].data_ptr()
                if segmented:
                    _, ln = f.next(seg_bytes)
                    e.seg_submit_device([f], a, [0], [ln])
                else:
                    e.submit_device(a, [0], [seg_bytes])
                order += 1
                if order > R:
                    e.wait()
                    order -= 1
            last = None
            while order:
                last = e.wait()
                order -= 1
            dt = time.perf_counter() - t0
            if segmented:
                assert f.final_sent and last[0].content_type == 3
                f.close()
            return dt

        run(True)  # warm-up: buffers sized, streams and SDMA engines created
        run(False)
        for _ in range(repeats):
            out["seg"].append(round(file_len / run(True) / GiB, 1))
            # the same arenas as independent files: segments x seg_bytes are hashed, and counted
            out["independent"].append(round(segments * seg_bytes / run(False) / GiB, 1))
    med = lambda v: float(np.median(v))
    out["seg_gibs"], out["independent_gibs"] = med(out["seg"]), med(out["independent"])
    out["ratio"] = round(out["seg_gibs"] / out["independent_gibs"], 4)
    out["expected_ratio"] = round(1 - OVERLAP / seg_bytes, 4)
    out["independent_spread"] = round((max(out["independent"]) - min(out["independent"])) / out["independent_gibs"], 4)
    return out


def leg_disk(file_bytes: int, seg_bytes: int, io_threads: int) -> dict:
    import numpy as np
    from hashbox_amd import Engine
    rng = np.random.default_rng(7)
    piece = 128 << 20
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as d:
        big = os.path.join(d, "big.bin")
        paths = []
        with open(big, "wb") as fb:
            for i in range(file_bytes // piece):
                buf = rng.integers(0, 256, piece, dtype=np.uint8).tobytes()
                fb.write(buf)
                p = os.path.join(d, f"part{i:04d}.bin")
                with open(p, "wb") as fp:
                    fp.write(buf)
                paths.append(p)
        out = {"file_bytes": file_bytes, "seg_bytes": seg_bytes, "io_threads": io_threads, "seg": [], "paths": []}
        with Engine(0) as e:
            e.store_file(big, segment_bytes=seg_bytes, io_threads=io_threads)  # warm-up (and the page cache)
            e.store_paths(paths, io_threads=io_threads, batch_bytes=seg_bytes)
            for _ in range(3):
                t0 = time.perf_counter()
                r = e.store_file(big, segment_bytes=seg_bytes, io_threads=io_threads)
                out["seg"].append(round(file_bytes / (time.perf_counter() - t0) / GiB, 2))
                t0 = time.perf_counter()
                e.store_paths(paths, io_threads=io_threads, batch_bytes=seg_bytes)
                out["paths"].append(round(file_bytes / (time.perf_counter() - t0) / GiB, 2))
            out["chunks"] = r.n_chunks
    out["seg_gibs"], out["paths_gibs"] = float(np.median(out["seg"])), float(np.median(out["paths"]))
    return out


def leg_k5() -> dict:
    """hbx_block_id over a FileChainBlock of 230 k chunks (a 1 TiB file): an 11 MB message."""
    import numpy as np
    from hashbox_amd import Engine
    k = 230_000
    ids = np.random.default_rng(3).integers(0, 256, (k, 16), dtype=np.uint8)
    body = b"fchn" + k.to_bytes(4, "big") + b"".join(bytes(i) + bytes(16) for i in ids)
    links = [bytes(i) for i in ids]
    with Engine(0) as e:
        e.block_id(body[:4096], links[:16])
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            e.block_id(body, links)
            ts.append(time.perf_counter() - t0)
    msg = 16 + 48 * k
    return {"chunks": k, "message_bytes": msg, "seconds": round(min(ts), 4), "mb_per_s": round(msg / min(ts) / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["stream", "disk", "k5"])
    ap.add_argument("--seg-gib", type=float, default=8.0)
    ap.add_argument("--segments", type=int, default=68)  # >= 33; a multiple of the K3 period the plan picks (4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--disk-gib", type=float, default=2.0)
    ap.add_argument("--disk-seg-mib", type=int, default=512)
    ap.add_argument("--io-threads", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_stream.json"))
    a = ap.parse_args()
    if a.leg == "stream":
        print(json.dumps(leg_stream(int(a.seg_gib * GiB), a.segments, a.repeats)))
        return
    if a.leg == "disk":
        print(json.dumps(leg_disk(int(a.disk_gib * GiB), a.disk_seg_mib << 20, a.io_threads)))
        return
    if a.leg == "k5":
        print(json.dumps(leg_k5()))
        return
    res = {}
    common = ["--segments", str(a.segments), "--repeats", str(a.repeats)]
    legs = [("stream_8GiB", ["--leg", "stream", "--seg-gib", "8"] + common),
            ("stream_1GiB", ["--leg", "stream", "--seg-gib", "1"] + common),
            ("k5_chain_id", ["--leg", "k5"]),
            ("disk", ["--leg", "disk", "--disk-gib", str(a.disk_gib), "--disk-seg-mib", str(a.disk_seg_mib),
                      "--io-threads", str(a.io_threads)])]
    for name, args in legs:  # a fresh child per leg; a leg that fails or runs out of time ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                           timeout=a.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"leg {name} failed with status {p.returncode}")
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(name, json.dumps(res[name]), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
