"""Child program of tests/test_gpu_threads.py: one scenario of concurrent
callers of libhbxgpu per process.

    python tests/threads_child.py <scenario>

Every expected value is computed on this (the main) thread before a worker
starts: oracle.store_file(fast=True) for cut ends and block IDs, hashlib for
MD5 and HashData, CPython zlib for streams, plain dicts and list prefixes for
the ID set and the chain match.  The workers start together behind a
threading.Barrier (ctypes releases the GIL during a call, so they really are
inside the library at once), compare every result exactly and count what they
compared.  The process prints ONE JSON document as its last line of stdout:

    {"scenario": ..., "wall_s": ..., "workers": {name: {"checks": n, "errors": [...], ...}}, ...}

A worker that does not come back within JOIN_TIMEOUT_S is reported with every
thread's stack (faulthandler) on stderr, and the process exits with status 3
at once: no further GPU work is started after a hang."""
import faulthandler
import hashlib
import json
import os
import sys
import threading
import time
import traceback
import zlib
from collections import deque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MIN = 64 * 1024
Mi = 1 << 20
JOIN_TIMEOUT_S = 90.0
ROUNDS = 20
A_LENS = (3 * MIN + 17, 131_073, Mi + 5, 9 * Mi + 7)  # the last one holds an 8 MiB chunk: the longest MD5 chain
A_SLICE, B_SLICE = 8192, 16384  # MD5 blocks per launch: the 8 MiB chain (131,072 blocks) takes 16 and 8 launches


# ------------------------------------------------------------- plumbing --
class Worker:
    def __init__(self, name, fn):
        self.name, self.fn = name, fn
        self.checks = 0
        self.errors = []
        self.extra = {}

    def eq(self, ok, what):
        """One exact comparison: counted, and described if it failed."""
        self.checks += 1
        if not ok and len(self.errors) < 8:
            self.errors.append(str(what() if callable(what) else what))
        return ok

    def fail(self, what):
        if len(self.errors) < 8:
            self.errors.append(str(what))

    def report(self):
        return dict(checks=self.checks, errors=self.errors, **self.extra)


def run_workers(scenario, workers, more=None):
    """Start the workers together, join them under one deadline, print the document."""
    barrier = threading.Barrier(len(workers))

    def body(w):
        try:
            barrier.wait(JOIN_TIMEOUT_S)
            w.fn(w)
        except BaseException:
            w.fail(traceback.format_exc())

    threads = [threading.Thread(target=body, args=(w,), name=w.name, daemon=True) for w in workers]
    t0 = time.monotonic()
    for t in threads:
        t.start()
    deadline = t0 + JOIN_TIMEOUT_S
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    wall = time.monotonic() - t0
    hung = [t.name for t in threads if t.is_alive()]
    doc = dict(scenario=scenario, wall_s=round(wall, 3), hung=hung, workers={w.name: w.report() for w in workers})
    if hung:  # which thread is inside which call; then out, with no further GPU work
        faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
        sys.stderr.flush()
        print(json.dumps(doc), flush=True)
        os._exit(3)
    if more:
        more(doc)  # what the scenario adds once every worker is back
    print(json.dumps(doc), flush=True)
    return 1 if any(w["errors"] for w in doc["workers"].values()) else 0


def same_file(g, r) -> bool:
    return (np.array_equal(g.cut_ends, r.cut_ends) and np.array_equal(g.ids, r.ids)
            and g.content_id == r.content_id and g.content_type == r.content_type)


def rows(a) -> list:
    return [bytes(x) for x in np.asarray(a, np.uint8).reshape(-1, 16)]


def random_ids(n, seed) -> np.ndarray:
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, 16), dtype=np.uint8)


# ----------------------------------------------- mix A: a pipeline of batches --
class MixA:
    """Three device arenas, each holding the four files of A_LENS in another
    order and with bytes of its own; batches of them pipelined, up to three in
    flight.  `corpus` numbers the mix: no two mixes of a process share a byte
    pattern, hence (asserted by disjoint()) no chunk ID."""

    def __init__(self, corpus: int):
        import torch
        from hashbox_amd import pack_arena_layout
        from oracle import oracle as O
        self.lens, self.offs, self.refs, self.dev = [], [], [], []
        self.id_set = set()
        for k in range(3):
            order = [(f + k) % 4 for f in range(4)]
            lens = [A_LENS[f] for f in order]
            offs, total = pack_arena_layout(lens)
            host = np.zeros(total, np.uint8)
            refs = []
            for o, f in zip(offs.tolist(), order):
                n = A_LENS[f]
                # the 9 MiB file is one byte value (no cut before MAX: one 8 MiB chunk); the others are random
                data = (np.full(n, 1 + 3 * corpus + k, np.uint8) if f == 3
                        else O.random_bytes(n, 1000 * corpus + 10 * k + f))
                host[o:o + n] = data
                r = O.store_file(data, fast=True)
                if f == 3:
                    assert int(r.cut_ends[0]) == 8 * Mi, "the 9 MiB file must start with an 8 MiB chunk"
                refs.append(r)
                self.id_set.update(rows(r.ids))
            self.lens.append(lens)
            self.offs.append(offs)
            self.refs.append(refs)
            self.dev.append(torch.from_numpy(host).to("cuda:0"))
        self.others = set()  # chunk IDs of every other mix of the process

    @staticmethod
    def disjoint(mixes) -> bool:
        """No two corpora share a chunk (checked on the oracle's IDs); each mix learns the others' IDs."""
        ok = True
        for a in mixes:
            a.others = set().union(*[b.id_set for b in mixes if b is not a]) if len(mixes) > 1 else set()
            ok = ok and not (a.id_set & a.others)
        return ok

    def check(self, w, got, k):
        w.eq(len(got) == 4, lambda: f"arena {k}: {len(got)} files came back")
        for f, (g, r) in enumerate(zip(got, self.refs[k])):
            if not w.eq(same_file(g, r), lambda: f"arena {k} file {f} ({self.lens[k][f]} B): cuts/IDs differ from the "
                                                 f"oracle: got {g.n_chunks} chunks {g.content_id.hex()}, want "
                                                 f"{r.n_chunks} {r.content_id.hex()}"):
                w.extra["foreign"] = w.extra.get("foreign", 0) + sum(1 for i in rows(g.ids) if i in self.others)

    def run(self, w, e, rounds=ROUNDS, burst=None, after_first_submit=None):
        """`rounds` batches, each compared; the pipeline drains every `burst` batches (default: at the end)."""
        w.extra.setdefault("foreign", 0)
        burst = burst or rounds
        done = 0
        while done < rounds:
            n, sub, fl = min(burst, rounds - done), 0, deque()
            for _ in range(n):
                while len(fl) < 3 and sub < n:
                    k = (done + sub) % 3
                    e.submit_device(self.dev[k].data_ptr(), self.offs[k], self.lens[k])
                    fl.append(k)
                    sub += 1
                    if after_first_submit is not None:
                        after_first_submit()
                        after_first_submit = None
                k = fl.popleft()
                self.check(w, e.wait(), k)
            done += n
            w.eq(e.pending() == 0, "batches left pending after a drain")
        w.extra["batches"] = done


def mix_a_worker(mix, md5_slice, join_lag, rounds=ROUNDS):
    def fn(w):
        from hashbox_amd import Engine
        with Engine(0, md5_slice=md5_slice, join_lag=join_lag) as e:
            mix.run(w, e, rounds)
    return fn


# ------------------------------------------------ mix C: hashes and zlib --
class MixC:
    def __init__(self, seed):
        from tests.test_gpu_restore import _text, block_id
        rng = np.random.default_rng(seed)
        lens = list(range(201)) + [70_001]
        self.blocks = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lens]
        self.links = [rows(random_ids((0, 1, 4, 9)[i % 4], seed * 1000 + i)) for i in range(len(lens))]
        self.ids = [block_id(b, l) for b, l in zip(self.blocks, self.links)]
        self.expect = [bytes(x ^ 0x80 for x in i) if k % 7 == 3 else i for k, i in enumerate(self.ids)]
        self.ok = [k % 7 != 3 for k in range(len(lens))]
        self.single = []  # (data, links, HashData, MD5) per round: 0..4 links
        for r in range(ROUNDS):
            d, l = self.blocks[(37 * r + 5) % len(lens)], rows(random_ids(r % 5, seed * 77 + r))
            self.single.append((d, l, block_id(d, l), hashlib.md5(d).digest()))
        self.text = [_text(MIN, seed * 10 + i) for i in range(3)]

    def hashes(self, w, e, r, stride=1):
        """verify_blocks, block_id and md5 of round r.  stride > 1: every stride-th block, starting at r, and the
        70,001-byte one (every length and link count then comes round within `stride` rounds)."""
        n = len(self.blocks)
        pick = list(range(n)) if stride == 1 else sorted(set(range(r % stride, n, stride)) | {n - 1})
        ids, ok, bad = e.verify_blocks([self.blocks[i] for i in pick], [self.links[i] for i in pick],
                                       [self.expect[i] for i in pick])
        w.eq(rows(ids) == [self.ids[i] for i in pick], f"round {r}: verify_blocks IDs differ from hashlib")
        want_ok = [self.ok[i] for i in pick]
        w.eq(ok.tolist() == want_ok and bad == want_ok.count(False), f"round {r}: verify_blocks ok flags / n_bad")
        d, l, want_id, want_md5 = self.single[r % len(self.single)]
        w.eq(e.block_id(d, l) == want_id, f"round {r}: block_id with {len(l)} links")
        w.eq(e.md5(d) == want_md5, f"round {r}: md5 of {len(d)} bytes")

    def zlib_round_trip(self, w, e, r):
        zs = e.deflate_blocks(self.text)
        w.eq([zlib.decompress(z) for z in zs] == self.text, f"round {r}: CPython zlib does not inflate K7's streams")
        out, st = e.inflate_blocks(zs, [MIN] * len(zs))
        w.eq(st.tolist() == [0] * len(zs) and out == self.text, f"round {r}: inflate_blocks_device of K7's streams")

    def worker(self):
        def fn(w):
            from hashbox_amd import Engine
            with Engine(0) as e:
                for r in range(ROUNDS):
                    self.hashes(w, e, r)
                    self.zlib_round_trip(w, e, r)
        return fn


# ------------------------------------ mix D: ID set, chain match, restore --
class MixD:
    def __init__(self, seed):
        from tests.test_gpu_idset import _model_insert
        from tests.test_gpu_match import _record, _synthetic_cases
        from tests.test_gpu_restore import edge_chain, wire
        g = np.random.Generator(np.random.PCG64(seed))
        pool = g.integers(0, 256, (1500, 16), dtype=np.uint8)
        model = {}
        self.draws, self.fresh, self.probe, self.found = [], [], [], []
        for r in range(ROUNDS):
            d = pool[g.integers(0, pool.shape[0], 600)]
            self.draws.append(d)
            self.fresh.append(_model_insert(model, d))
            p = pool[g.integers(0, pool.shape[0], 400)]
            self.probe.append(p)
            self.found.append([x.tobytes() in model for x in p])
        self.count = len(model)
        self.exported = set(model)
        self.cases = _synthetic_cases()
        rng = np.random.default_rng(seed)
        self.cuts = [np.cumsum(rng.integers(1, 1 << 40, len(loc), dtype=np.uint64)) for loc, _ in self.cases]
        self.records = [_record(loc, exp, c) for (loc, exp), c in zip(self.cases, self.cuts)]
        blocks, self.chain_ids = edge_chain()
        self.chain_bytes = b"".join(blocks)
        self.datas, self.types = wire(blocks, "rz")
        self.chain_offs = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).tolist()

    def worker(self):
        def fn(w):
            from hashbox_amd import Engine, IdSet
            with Engine(0) as e:
                s = IdSet(e, 4096)
                for r in range(ROUNDS):
                    w.eq(np.array_equal(s.insert(self.draws[r]), self.fresh[r]), f"round {r}: IdSet.insert vs the dict")
                    w.eq(s.contains(self.probe[r]).tolist() == self.found[r], f"round {r}: IdSet.contains vs the dict")
                    got = e.match_chains([l for l, _ in self.cases], [x for _, x in self.cases], self.cuts)
                    w.eq([(m.same, m.n_match, m.n_local, m.n_expect, m.match_bytes) for m in got] == self.records,
                         f"round {r}: match_chains records")
                    x = e.restore_blocks(self.datas, self.types, self.chain_ids)
                    w.eq(x.status.tolist() == [0] * len(self.datas) and x.data == self.chain_bytes
                         and x.offs.tolist() == self.chain_offs, f"round {r}: restore_blocks of the edge chain")
                w.eq(s.count == self.count and {i.tobytes() for i in s.export()} == self.exported,
                     "IdSet count / export at the end")
                s.close()
        return fn


# ------------------------------------------------------------ scenarios --
def scenario_distinct_mixed():
    """1a: four contexts, one thread each, four different mixes."""
    a, b = MixA(0), MixA(1)
    ok = MixA.disjoint([a, b])
    c, d = MixC(3), MixD(4)
    return run_workers("distinct_mixed", [Worker("A", mix_a_worker(a, A_SLICE, 2)),
                                          Worker("B", mix_a_worker(b, B_SLICE, 1)),
                                          Worker("C", c.worker()), Worker("D", d.worker())],
                       lambda doc: doc.update(disjoint=ok))


def scenario_distinct_pipelines():
    """1b: four contexts all running mix A on four corpora: four K1 gates and K3 launches side by side."""
    mixes = [MixA(10 + i) for i in range(4)]
    ok = MixA.disjoint(mixes)
    return run_workers("distinct_pipelines",
                       [Worker(f"A{i}", mix_a_worker(m, (A_SLICE, B_SLICE, 4096, 12_000)[i], 2 if i % 2 == 0 else 1))
                        for i, m in enumerate(mixes)], lambda doc: doc.update(disjoint=ok))


def scenario_create_destroy():
    """2: contexts and ID sets come and go while two pipelines run."""
    from oracle import oracle as O
    a, b = MixA(20), MixA(21)
    ok = MixA.disjoint([a, b])
    small = [O.random_bytes(n, 500 + i) for i, n in enumerate((5, MIN + 1, 3 * MIN + 17))]
    small_refs = [O.store_file(x, fast=True) for x in small]
    pool = random_ids(700, 31)
    draws = [pool[np.random.Generator(np.random.PCG64(40 + i)).integers(0, 700, 1000)] for i in range(30)]
    distinct = [{x.tobytes() for x in d} for d in draws]

    def contexts(w):
        from hashbox_amd import Engine
        for i in range(30):
            with Engine(0) as e:
                w.eq(same_file(e.chunk_hash(small[i % 3]), small_refs[i % 3]), f"context {i}: chunk_hash of a small file")

    def sets(w):
        from hashbox_amd import Engine, IdSet
        from tests.test_gpu_idset import _model_insert
        with Engine(0) as e:
            for i in range(30):
                with IdSet(e, 2000) as s:
                    w.eq(np.array_equal(s.insert(draws[i]), _model_insert({}, draws[i])), f"set {i}: insert vs the dict")
                    w.eq(s.count == len(distinct[i]) and {x.tobytes() for x in s.export()} == distinct[i],
                         f"set {i}: count / export")

    return run_workers("create_destroy", [Worker("A", mix_a_worker(a, A_SLICE, 2)), Worker("B", mix_a_worker(b, B_SLICE, 1)),
                                          Worker("contexts", contexts), Worker("sets", sets)], lambda doc: doc.update(disjoint=ok))


def scenario_shared_sync():
    """3: six threads, one context, synchronous calls only: serialised, never refused."""
    from hashbox_amd import Engine, HbxError
    from oracle import oracle as O
    from tests.test_gpu_parity import EDGE_SIZES
    sizes = [n for n in EDGE_SIZES if n <= 2 * MIN + 2]
    eng = Engine(0)
    workers = []
    for t in range(6):
        files = [O.random_bytes(n, 9000 + 100 * t + i) for i, n in enumerate(sizes[t::6] + [9 * Mi + t])]
        refs = [O.store_file(x, fast=True) for x in files]
        c = MixC(60 + t)

        def fn(w, files=files, refs=refs, c=c):
            for r in range(50):
                try:
                    k = r % len(files)
                    w.eq(same_file(eng.chunk_hash(files[k]), refs[k]), f"round {r}: chunk_hash of {files[k].size} bytes")
                    c.hashes(w, eng, r, stride=5)
                except HbxError as ex:  # nothing may be refused: every call is synchronous
                    w.fail(f"round {r}: {ex}")
        workers.append(Worker(f"T{t}", fn))
    rc = run_workers("shared_sync", workers)
    eng.close()
    return rc


def scenario_shared_pipeline():
    """4: one context; P runs mix A, three threads make synchronous calls.  Per
    hbxgpu.h, refused while batches are pending: hbx_chunk_hash, hbx_verify_blocks,
    hbx_inflate_blocks_device, hbx_idset_insert, hbx_set_md5_slice.  Never
    refused: hbx_md5, hbx_block_id, hbx_pending, hbx_knobs."""
    import ctypes
    import torch
    from hashbox_amd import Engine, HbxError, IdSet, _lib
    from oracle import oracle as O
    from tests.test_gpu_idset import _model_insert
    from tests.test_gpu_restore import _text
    eng = Engine(0, md5_slice=A_SLICE, join_lag=2)
    mix = MixA(30)
    small = O.random_bytes(2 * MIN + 2, 77)
    small_ref = O.store_file(small, fast=True)
    c = MixC(70)
    # zlib -6 streams of three text blocks, resident on the device
    text = [_text(n, 80 + i) for i, n in enumerate((MIN, 70_001, 1))]
    zs = [zlib.compress(x, 6) for x in text]
    z_offs = np.cumsum([0] + [(len(z) + 255) // 256 * 256 for z in zs])
    zhost = np.zeros(int(z_offs[-1]) + 64, np.uint8)
    for o, z in zip(z_offs, zs):
        zhost[int(o):int(o) + len(z)] = np.frombuffer(z, np.uint8)
    d_in = torch.from_numpy(zhost).to("cuda:0")
    o_caps = [len(x) for x in text]
    o_offs = np.cumsum([0] + [(n + 255) // 256 * 256 for n in o_caps])
    d_out = torch.zeros(int(o_offs[-1]) + 64, dtype=torch.uint8, device="cuda:0")
    # an ID set no batch uses, and the dict's answers for its j-th insert that goes through
    idset = IdSet(eng, 8192)
    pool = random_ids(3000, 90)
    g = np.random.Generator(np.random.PCG64(91))
    draws = [pool[g.integers(0, 3000, 200)] for _ in range(400)]
    model = {}
    draws_fresh = [_model_insert(model, d) for d in draws]
    torch.cuda.synchronize()

    p_done = threading.Event()
    seen_refusal = threading.Event()
    outcomes = {}
    lock = threading.Lock()

    def attempt(w, name, call, exact, final):
        """A refusable call: HBX_ERR_STATE (not once the pipeline thread is done) or the exact result."""
        try:
            got = call()
        except HbxError as ex:
            refused = f": {_lib.ERRORS[-6]}:" in str(ex)
            w.eq(refused and not final, f"{name}: {ex}" + (" (after the last batch was collected)" if refused else ""))
            if refused:
                seen_refusal.set()
            with lock:
                outcomes.setdefault(name, [0, 0])[0] += 1
            return False
        w.eq(exact(got), f"{name}: went through with a wrong result")
        with lock:
            outcomes.setdefault(name, [0, 0])[1] += 1
        return True

    def always(w, name, call, exact):
        """A call the header does not refuse: always the exact result."""
        try:
            w.eq(exact(call()), f"{name}: wrong result")
        except HbxError as ex:
            w.fail(f"{name} must never be refused: {ex}")

    def pipeline(w):
        def hold():  # one batch is pending and this thread is outside the library: every refusable call is refused
            w.eq(seen_refusal.wait(30.0), "no synchronous call was refused while a batch was pending")
        try:
            mix.run(w, eng, ROUNDS, burst=4, after_first_submit=hold)
        finally:
            p_done.set()

    # hbx_last_error(NULL) is per thread: two threads fail hbx_plan_pipeline(NULL, ...) with different messages
    L = _lib.load()
    pair = threading.Barrier(2)

    def own_last_error(w, which):
        want, other = (b"join lag", b"K3 period") if which == 0 else (b"K3 period", b"join lag")
        for r in range(50):
            q = _lib.PlanRequest(n_files=8, arena_bytes=Mi, longest_file=Mi, free_bytes=1 << 30)
            if which == 0:
                q.join_lag = 9
            else:
                q.k3_period = 99
            rc = L.hbx_plan_pipeline(None, ctypes.byref(q), ctypes.byref(_lib.PipelinePlan()))
            pair.wait(20.0)  # both have failed before either reads
            msg = L.hbx_last_error(None)
            w.eq(rc == -1 and want in msg and other not in msg, f"hbx_last_error(NULL) round {r}: rc {rc}, {msg!r}")
            pair.wait(20.0)

    def loop(w, body):
        n = 0
        while not p_done.is_set():
            body(w, False)
            n += 1
        body(w, True)  # the pipeline is drained: nothing is refused any more
        w.extra["iterations"] = n + 1

    def s0(w):
        own_last_error(w, 0)

        def body(w, final):
            attempt(w, "chunk_hash", lambda: eng.chunk_hash(small), lambda got: same_file(got, small_ref), final)
            always(w, "md5", lambda: eng.md5(small), lambda got: got == hashlib.md5(small.tobytes()).digest())
            always(w, "pending", eng.pending, (lambda got: got == 0) if final else (lambda got: 0 <= got <= 3))
        loop(w, body)

    def s1(w):
        own_last_error(w, 1)
        d, l, want_id, _ = c.single[3]

        def body(w, final):
            attempt(w, "verify_blocks", lambda: eng.verify_blocks(c.blocks, c.links, c.expect),
                    lambda got: rows(got[0]) == c.ids and got[1].tolist() == c.ok and got[2] == c.ok.count(False), final)
            always(w, "block_id", lambda: eng.block_id(d, l), lambda got: got == want_id)
            attempt(w, "set_md5_slice", lambda: eng.set_md5_slice(A_SLICE), lambda got: True, final)
            always(w, "knobs", eng.knobs, lambda k: k["md5_slice"] == A_SLICE and k["join_lag"] == 2)
        loop(w, body)

    def s2(w):
        state = {"j": 0}

        def inflate():
            d_out.zero_()
            return eng.inflate_blocks_device(d_in.data_ptr(), z_offs[:-1], [len(z) for z in zs], d_out.data_ptr(),
                                             o_offs[:-1], o_caps)

        def inflated(got):
            out = d_out.cpu().numpy()
            return (got[0].tolist() == o_caps and got[1].tolist() == [0, 0, 0]
                    and [out[int(o):int(o) + n].tobytes() for o, n in zip(o_offs, o_caps)] == text)

        def body(w, final):
            attempt(w, "inflate_blocks_device", inflate, inflated, final)
            j = min(state["j"], len(draws) - 1)
            want = draws_fresh[j] if state["j"] < len(draws) else np.zeros(200, bool)
            if attempt(w, "idset_insert", lambda: idset.insert(draws[j]), lambda got: np.array_equal(got, want), final):
                state["j"] += 1
        loop(w, body)

    rc = run_workers("shared_pipeline", [Worker("P", pipeline), Worker("S0", s0), Worker("S1", s1), Worker("S2", s2)],
                     lambda doc: doc.update(outcomes={k: dict(refused=v[0], exact=v[1]) for k, v in outcomes.items()}))
    idset.close()
    eng.close()
    return rc


def scenario_shared_idset():
    """5: four inserters and one reader on one ID set of one context."""
    from hashbox_amd import Engine, IdSet
    pool = random_ids(20_000, 5)
    assert len({x.tobytes() for x in pool}) == pool.shape[0]
    picks = [np.random.Generator(np.random.PCG64(100 + t)).integers(0, pool.shape[0], (40, 500)) for t in range(4)]
    probes = np.random.Generator(np.random.PCG64(200)).integers(0, pool.shape[0], (4000, 300))
    drawn = np.unique(np.concatenate([p.reshape(-1) for p in picks]))
    eng = Engine(0)
    s = IdSet(eng, 60_000)
    calls = []  # (start ns, end ns, pool indices, fresh) per insert call
    reads = []  # (end ns, pool indices, found) per contains call
    lock = threading.Lock()
    left = [4]
    half, read_after_half = threading.Event(), threading.Event()

    def inserter(t):
        def fn(w):
            try:
                for j in range(40):
                    if t == 0 and j == 20:  # half way: go on once a contains call that began after this has returned
                        half.set()
                        w.eq(read_after_half.wait(30.0), "the reader made no contains call during the run")
                    idx = picks[t][j]
                    ids = pool[idx]
                    t0 = time.monotonic_ns()  # before the call: the ID may be in the set from here on
                    fresh = s.insert(ids)
                    t1 = time.monotonic_ns()
                    with lock:
                        calls.append((t0, t1, idx, fresh))
            finally:
                with lock:
                    left[0] -= 1
        return fn

    def reader(w):
        after_half = 0
        for idx in probes:
            if left[0] == 0:
                break
            was_half = half.is_set()
            found = s.contains(pool[idx])
            with lock:
                reads.append((time.monotonic_ns(), idx, found))
            after_half += was_half
            if after_half:
                read_after_half.set()

    def invariant(doc):
        """The set's invariant over all calls (main thread, every worker back)."""
        w = Worker("invariant", None)
        n = pool.shape[0]
        w.eq(len(calls) == 160, f"{len(calls)} insert calls were recorded")
        times_fresh = np.zeros(n, np.int64)
        first_start = np.full(n, np.iinfo(np.int64).max)  # earliest start of an insert call holding the ID
        first_end = np.full(n, np.iinfo(np.int64).max)  # earliest end of one
        fresh_start = np.zeros(n, np.int64)  # start of the call in which the ID was fresh
        for t0, t1, idx, fresh in calls:
            np.add.at(times_fresh, idx[fresh], 1)
            np.minimum.at(first_start, idx, t0)
            np.minimum.at(first_end, idx, t1)
            fresh_start[idx[fresh]] = t0
            _, lowest = np.unique(idx, return_index=True)
            w.eq(np.isin(np.flatnonzero(fresh), lowest).all(), "an ID was fresh at an index that is not its lowest in the call")
        w.eq(bool((times_fresh[drawn] == 1).all()) and int(times_fresh.sum()) == drawn.size,
             lambda: f"each ID must be fresh exactly once; (times, IDs): {np.unique(times_fresh[drawn], return_counts=True)}")
        # the calls are serialised: the fresh call started before any other call holding the ID had ended, and a
        # call that saw the ID at its lowest index as not fresh ended after the fresh call had started
        w.eq((fresh_start[drawn] <= first_end[drawn]).all(), "an ID was fresh after a call holding it had returned")
        for t0, t1, idx, fresh in calls:
            _, lowest = np.unique(idx, return_index=True)
            seen = lowest[~fresh[lowest]]
            w.eq((fresh_start[idx[seen]] < t1).all(), "an ID was reported seen before the call that inserted it had started")
        n_found = 0
        for t_end, idx, found in reads:
            n_found += int(found.sum())
            w.eq((first_start[idx[found]] < t_end).all(), "contains reported an ID no insert call had yet been started with")
        w.extra.update(reads=len(reads), found_during_run=n_found, distinct=int(drawn.size))
        w.eq(s.count == drawn.size, lambda: f"count {s.count}, distinct IDs drawn {drawn.size}")
        w.eq({x.tobytes() for x in s.export()} == {x.tobytes() for x in pool[drawn]}, "export() is not the set of IDs drawn")
        w.eq(s.contains(pool).tolist() == np.isin(np.arange(n), drawn).tolist(), "contains(pool) after the run")
        doc["workers"]["invariant"] = w.report()

    rc = run_workers("shared_idset", [Worker(f"I{t}", inserter(t)) for t in range(4)] + [Worker("reader", reader)], invariant)
    s.close()
    eng.close()
    return rc


SCENARIOS = dict(distinct_mixed=scenario_distinct_mixed, distinct_pipelines=scenario_distinct_pipelines,
                 create_destroy=scenario_create_destroy, shared_sync=scenario_shared_sync,
                 shared_pipeline=scenario_shared_pipeline, shared_idset=scenario_shared_idset)

if __name__ == "__main__":
    sys.exit(SCENARIOS[sys.argv[1]]())
