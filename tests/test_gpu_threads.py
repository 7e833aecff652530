"""GPU: the threading contract of include/hbxgpu.h ("a context is safe to call
from many threads; distinct contexts run concurrently"; INTEGRATION.md
"Errors, ownership, threading") with several host threads inside the library
at once.

Each scenario runs in a fresh child process (tests/threads_child.py), one at a
time, under a 120 s watchdog: a deadlock ends as a failed test with the child
killed, and the child itself gives up after 90 s with every thread's stack on
stderr.  The child computes every expected value before it starts a thread
(oracle.store_file(fast=True), hashlib, CPython zlib, dict and list models),
compares exactly inside the workers and prints one JSON document: per worker
the number of comparisons made and the text of every one that failed.  The
asserts below are on that document; the counts they demand are derived from
the scenario, so a worker that skipped work fails as well.

Two threads sharing one context's PIPELINE (submit on one, wait on the other)
are driven from plain C (tests/c/abi_threads.c): the Python Engine keeps a
FIFO of its own, the C-ABI has no binding state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "threads_child.py")
ROUNDS = 20
MIX_A_CHECKS = ROUNDS * 5 + 1  # per batch: 4 files came back + each file exact; then nothing is left pending


def run_child(scenario: str) -> dict:
    r = subprocess.run([sys.executable, CHILD, scenario], cwd=ROOT, capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines and lines[-1].startswith("{"), (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    doc = json.loads(lines[-1])
    print(f"{scenario}: threads ran {doc['wall_s']:.2f} s")
    assert doc["scenario"] == scenario and doc["hung"] == [], (doc["hung"], r.stderr[-6000:])
    errors = {k: w["errors"] for k, w in doc["workers"].items() if w["errors"]}
    assert not errors, (errors, r.stderr[-3000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return doc


def checks(doc) -> dict:
    return {k: w["checks"] for k, w in doc["workers"].items()}


def test_distinct_contexts_different_work():
    """Four threads, a context each: two pipelines (join lag 2 and 1, other
    slices, other bytes), hashes + zlib round trips, ID set + chain match +
    restore.  20 rounds each, every result exact."""
    doc = run_child("distinct_mixed")
    assert doc["disjoint"] is True
    # C: per round 4 hash comparisons + 2 zlib ones; D: per round 4, and the set at the end
    assert checks(doc) == {"A": MIX_A_CHECKS, "B": MIX_A_CHECKS, "C": ROUNDS * 6, "D": ROUNDS * 4 + 1}
    assert doc["workers"]["A"]["foreign"] == 0 and doc["workers"]["B"]["foreign"] == 0


def test_distinct_contexts_four_pipelines():
    """Four pipelines side by side on four corpora that share no chunk: four K1
    gates and four one-workgroup-per-CU MD5 launches at once.  No ID of
    another thread's corpus may appear."""
    doc = run_child("distinct_pipelines")
    assert doc["disjoint"] is True
    assert checks(doc) == {f"A{i}": MIX_A_CHECKS for i in range(4)}
    assert [doc["workers"][f"A{i}"]["foreign"] for i in range(4)] == [0] * 4
    assert [doc["workers"][f"A{i}"]["batches"] for i in range(4)] == [ROUNDS] * 4


def test_contexts_created_and_destroyed_beside_pipelines():
    """hbx_ctx_create (its process-wide SDMA warm-up included) and
    hbx_ctx_destroy 30 times, and 30 ID sets created, filled, exported and
    closed on a fourth context, while two pipelines run."""
    doc = run_child("create_destroy")
    assert doc["disjoint"] is True
    assert checks(doc) == {"A": MIX_A_CHECKS, "B": MIX_A_CHECKS, "contexts": 30, "sets": 60}


def test_one_context_six_threads_synchronous():
    """Six threads on one context, synchronous calls only: serialised by the
    context's lock, so every result is exact and nothing is refused."""
    doc = run_child("shared_sync")
    assert checks(doc) == {f"T{t}": 50 * 5 for t in range(6)}  # chunk_hash + 4 hash comparisons per round


def test_one_context_pipeline_and_synchronous_callers():
    """A pipeline thread and three synchronous callers on one context: the
    pipeline's results are exact; a call hbxgpu.h refuses while batches are
    pending gives HBX_ERR_STATE or the exact result, and both were seen; the
    calls it does not refuse are always exact; hbx_last_error(NULL) is per
    thread."""
    doc = run_child("shared_pipeline")
    c = checks(doc)
    assert c["P"] == ROUNDS * 5 + ROUNDS // 4 + 1  # the pipeline drains every 4 batches; + the refusal it waited for
    assert doc["workers"]["P"]["foreign"] == 0 and doc["workers"]["P"]["batches"] == ROUNDS
    its = {k: doc["workers"][k]["iterations"] for k in ("S0", "S1", "S2")}
    assert c["S0"] == 50 + 3 * its["S0"] and c["S1"] == 50 + 4 * its["S1"] and c["S2"] == 2 * its["S2"]
    out = doc["outcomes"]
    print("refused / exact per call:", out)
    assert set(out) == {"chunk_hash", "verify_blocks", "set_md5_slice", "inflate_blocks_device", "idset_insert"}
    assert all(v["exact"] >= 1 for v in out.values()), out  # (each goes through once the pipeline is done)
    assert any(v["refused"] >= 1 and v["exact"] >= 1 for v in out.values()), out


def test_one_id_set_many_inserters():
    """Four threads insert overlapping draws into one set while a fifth reads:
    each distinct ID is fresh exactly once over all calls, at its lowest index
    within the call; count and export() are the distinct IDs drawn; contains
    never reports an ID before an insert call holding it had been started."""
    doc = run_child("shared_idset")
    c = checks(doc)
    assert [c[f"I{t}"] for t in range(4)] == [1, 0, 0, 0]  # (I0 waited for the reader half way)
    inv = doc["workers"]["invariant"]
    assert inv["reads"] >= 1 and inv["found_during_run"] >= 1
    assert 10_000 < inv["distinct"] <= 20_000
    assert inv["checks"] == 1 + 160 + 2 + 160 + inv["reads"] + 3


# ------------------------------------------------ the plain-C threaded driver --
K, SPAN_STEP = 24, 65552


def _span(pair, i):
    """abi_threads.c's batch_span."""
    return (i * SPAN_STEP, 200_000 + 4099 * i) if pair == 0 else ((K - 1 - i) * SPAN_STEP + 32, 150_001 + 8191 * i)


def test_plain_c_producer_and_consumer_threads(oracle, tmp_path):
    """One thread submits 24 batches (4 outstanding), another waits 24 times,
    on one context and then on two contexts at once: the i-th wait filled
    batch i's arrays with the oracle's cuts and IDs."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), f"OUT={tmp_path}"], check=True)
    data = oracle.random_bytes(2 * 1024 * 1024, 4242)
    data[300_000:900_000] = 0x41  # some batches hold a run that never cuts
    f = tmp_path / "in.bin"
    data.tofile(f)
    want = {}
    for pair in (0, 1):
        lines = []
        for i in range(K):
            off, n = _span(pair, i)
            ref = oracle.store_file(data[off:off + n], fast=True)
            lines += [f"ctx {pair} batch {i}: {int(c)} {bytes(x).hex()}" for c, x in zip(ref.cut_ends, ref.ids)]
            lines.append(f"ctx {pair} batch {i}= {ref.content_type} {ref.content_id.hex()} {ref.n_chunks}")
        want[pair] = lines
    assert len(set(want[0]) | set(want[1])) == len(want[0]) + len(want[1])  # no two batches give the same lines
    r = subprocess.run([str(tmp_path / "abi_threads"), str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = r.stdout.split("\n")
    assert "ok" in got
    assert [x[2:] for x in got if x.startswith("a ")] == want[0]
    assert [x[2:] for x in got if x.startswith("b ctx 0")] == want[0]
    assert [x[2:] for x in got if x.startswith("b ctx 1")] == want[1]
