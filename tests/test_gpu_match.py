"""GPU: the match by block ID (K12, hbx_match.hip) through hbx_match_chains,
hbx_store_paths_match and hbx_submit_device_match.

Every expected record is the common prefix of two ID lists, computed below in
plain Python; the ID lists of files come from the oracle's chunking.  Nothing
comes from the code under test, and every comparison is exact."""
import errno
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Mi = 1 << 20


# ------------------------------------------------------------- the model --
def _prefix(a, b) -> int:
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def _record(local, expect, cut_ends=None):
    """(same, n_match, n_local, n_expect, match_bytes) of two lists of 16-byte IDs."""
    m = _prefix(local, expect)
    mb = int(cut_ends[m - 1]) if cut_ends is not None and m else 0
    return (m == len(local) == len(expect), m, len(local), len(expect), mb)


def _got(r):
    return (r.same, r.n_match, r.n_local, r.n_expect, r.match_bytes)


def _rows(a) -> list:
    return [bytes(x) for x in np.asarray(a, np.uint8).reshape(-1, 16)]


def _random_ids(n, seed) -> list:
    return _rows(np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, 16), dtype=np.uint8))


def _flip(i: bytes, byte: int, bit: int) -> bytes:
    b = bytearray(i)
    b[byte] ^= 1 << bit
    return bytes(b)


# ---------------------------------------------------------- direct calls --
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)


def _synthetic_cases():
    """(local, expect) pairs: the smallest shapes at which the wave loop can go wrong."""
    cases = []
    for n in COUNTS:
        loc = _random_ids(n, 100 + n)
        cases.append((loc, list(loc)))  # a mismatch nowhere
        for at in sorted({0, 62, 63, 64, 65, n - 1}):
            if 0 <= at < n:
                exp = list(loc)
                exp[at] = _flip(exp[at], at % 16, at % 8)
                cases.append((loc, exp))
                # (and everything after the first mismatch different too)
                cases.append((loc, exp[:at + 1] + _random_ids(n - at - 1, 7000 + n + at)))
        if n:
            cases.append((loc, loc[:-1]))  # the expected chain one shorter
            cases.append((loc, []))        # non-empty against empty
        cases.append((loc, loc + _random_ids(1, 900 + n)))  # one longer (for n == 0: empty against non-empty)
    one = _random_ids(1, 5)[0]
    for word in range(4):  # exactly one of the four 32-bit words differs
        for nbits in (1, 32):
            other = bytearray(one)
            for k in range(4 if nbits == 32 else 1):
                other[4 * word + k] ^= 0xFF if nbits == 32 else 0x10
            cases.append(([one], [bytes(other)]))
            cases.append((_random_ids(70, 6) + [one], _random_ids(70, 6) + [bytes(other)]))
    cases.append(([one], [_flip(one, 0, 0)]))    # bit 0 of byte 0 alone
    cases.append(([one], [_flip(one, 15, 7)]))   # bit 7 of byte 15 alone
    return cases


def test_direct_synthetic(engine):
    cases = _synthetic_cases()
    rng = np.random.default_rng(3)
    cuts = [np.cumsum(rng.integers(1, 1 << 40, len(loc), dtype=np.uint64)) for loc, _ in cases]  # ascending
    want = [_record(loc, exp, c) for (loc, exp), c in zip(cases, cuts)]
    assert {w[0] for w in want} == {True, False}
    got = engine.match_chains([l for l, _ in cases], [e for _, e in cases], cuts)
    assert [_got(r) for r in got] == want
    # without cut ends match_bytes is 0
    got = engine.match_chains([l for l, _ in cases], [e for _, e in cases])
    assert [_got(r) for r in got] == [w[:4] + (0,) for w in want]
    # each case alone gives the same record (a file's record depends on nothing but its two lists)
    for k in (0, 1, len(cases) // 2, len(cases) - 1):
        loc, exp = cases[k]
        assert _got(engine.match_chains([loc], [exp], [cuts[k]])[0]) == want[k]


def test_direct_more_files_than_cus_and_none(engine):
    n = 3000
    loc = _random_ids(n, 11)
    exp = [i if k % 3 else _flip(i, k % 16, k % 8) for k, i in enumerate(loc)]
    got = engine.match_chains([[i] for i in loc], [[i] for i in exp])
    assert [_got(r) for r in got] == [_record([a], [b]) for a, b in zip(loc, exp)]
    assert sum(r.same for r in got) == n - n // 3
    assert engine.match_chains([], []) == []
    # n_files == 0 straight through the C-ABI
    assert engine._L.hbx_match_chains(engine._ctx, 0, None, None, None, None, None, None) == 0


# -------------------------------------------------------------- pipeline --
SIZES = (0, 1, 65_535, 65_536, 131_072, 131_073, 24 * Mi + 12_345)


@pytest.fixture(scope="module")
def corpus(oracle, tmp_path_factory):
    """Files in a temporary directory: per original size its local variants,
    each with the oracle's chunking of the original (the expected chain) and of
    the variant (the local ID list)."""
    tmp = tmp_path_factory.mktemp("match")
    rng = np.random.default_rng(2024)
    files = []  # dicts: path, data, expect (IDs), local (oracle FileResult), name
    for size in SIZES:
        orig = rng.integers(0, 256, size, dtype=np.uint8)
        o = oracle.store_file(orig, fast=True)
        ends = [int(x) for x in o.cut_ends]
        variants = {"identical": orig}
        if size:
            mid = len(ends) // 2  # a byte inside a middle chunk
            at = ((ends[mid - 1] if mid else 0) + ends[mid]) // 2
            for name, pos in (("first", 0), ("last", size - 1), ("middle", at)):
                v = orig.copy()
                v[pos] ^= 0x01
                variants[name] = v
            variants["shorter"] = orig[:-1]
        variants["longer"] = np.concatenate([orig, np.array([0x5A], np.uint8)])
        for name, v in variants.items():
            p = tmp / f"{size}_{name}"
            p.write_bytes(v.tobytes())
            files.append({"path": p, "size": int(v.size), "expect": _rows(o.ids), "name": f"{size}_{name}",
                          "local": oracle.store_file(v, fast=True), "data": v})
    assert max(len(f["expect"]) for f in files) >= 3  # several chunks
    return files


def _want(corpus):
    return [_record(_rows(f["local"].ids), f["expect"], f["local"].cut_ends) for f in corpus]


def test_corpus_model_is_not_trivial(corpus):
    want = dict(zip((f["name"] for f in corpus), _want(corpus)))
    big = SIZES[-1]
    assert want[f"{big}_identical"][0] and want[f"{big}_identical"][4] == big
    assert not want[f"{big}_first"][0] and want[f"{big}_first"][1] == 0
    assert not want[f"{big}_last"][0] and want[f"{big}_last"][1] >= 1
    assert not want[f"{big}_middle"][0] and not want[f"{big}_shorter"][0] and not want[f"{big}_longer"][0]
    assert want["0_identical"] == (True, 0, 0, 0, 0) and want["0_longer"] == (False, 0, 1, 0, 0)
    assert sum(w[0] for w in want.values()) == len(SIZES)


@pytest.mark.parametrize("batch_bytes,io_threads", [(1 * Mi, 16), (8 * Mi, 16), (1 << 30, 16), (1 << 30, 1)])
def test_paths_verdicts(engine, corpus, batch_bytes, io_threads):
    got = engine.match_paths([f["path"] for f in corpus], [f["expect"] for f in corpus], io_threads=io_threads,
                             batch_bytes=batch_bytes)
    assert [_got(r) for r in got] == _want(corpus)
    for r, f in zip(got, corpus):
        assert r.chunks is None and r.errno == 0
        assert (r.content_type, r.content_id) == (f["local"].content_type, f["local"].content_id), f["name"]


def test_paths_with_chunks_and_push_bytes(engine, corpus):
    paths, chains = [f["path"] for f in corpus], [f["expect"] for f in corpus]
    n = len(paths)
    k0 = engine.knobs()["match_push_bytes"]
    lean = engine.match_paths(paths, chains)  # one batch: the corpus is far below the default batch_bytes
    k1 = engine.knobs()["match_push_bytes"]
    full = engine.match_paths(paths, chains, chunks=True)
    k2 = engine.knobs()["match_push_bytes"]
    assert 0 < k1 - k0 <= 52 * n + 768
    assert k2 - k1 > 52 * n + 768
    assert [_got(r) for r in full] == [_got(r) for r in lean] == _want(corpus)
    stored = engine.store_paths(paths)
    for r, s, f in zip(full, stored, corpus):
        assert np.array_equal(r.chunks.cut_ends, s.cut_ends) and np.array_equal(r.chunks.ids, s.ids), f["name"]
        assert np.array_equal(s.cut_ends, f["local"].cut_ends) and np.array_equal(s.ids, f["local"].ids), f["name"]
        assert (r.content_type, r.content_id) == (s.content_type, s.content_id)
    # a plain store pushes nothing that counts as a match push
    assert engine.knobs()["match_push_bytes"] == k2


def test_paths_unreadable_file(engine, corpus, tmp_path):
    small = [f for f in corpus if f["size"] < Mi]
    paths = [f["path"] for f in small]
    chains = [f["expect"] for f in small]
    sizes = [f["size"] for f in small]
    at = 3
    paths.insert(at, tmp_path / "not_there")
    chains.insert(at, _random_ids(2, 1))
    sizes.insert(at, 70_000)
    for chunks in (False, True):
        got = engine.match_paths(paths, chains, sizes=sizes, skip_unreadable=True, chunks=chunks)
        assert got[at].errno == errno.ENOENT and got[at].n_local == 0 and not got[at].same
        rest = got[:at] + got[at + 1:]
        assert all(r.errno == 0 for r in rest)
        assert [_got(r) for r in rest] == _want(small)


def test_foreign_chain(engine, oracle, tmp_path):
    """A valid chain that is not the engine's cuts: the IDs do not settle it."""
    data = np.random.default_rng(77).integers(0, 256, 300 * 1024, dtype=np.uint8)
    p = tmp_path / "f"
    p.write_bytes(data.tobytes())
    pieces = [oracle.block_id(data[k:k + 100 * 1024]) for k in range(0, data.size, 100 * 1024)]
    assert len(pieces) == 3
    local = oracle.store_file(data, fast=True)
    r = engine.match_paths([p], [pieces])[0]
    assert _got(r) == _record(_rows(local.ids), pieces, local.cut_ends) and not r.same
    assert engine.match_paths([p], [_rows(local.ids)])[0].same


# ----------------------------------------------------------- device form --
def _device_batch(files):
    import torch
    from hashbox_amd import pack_arena_layout
    lens = [f["size"] for f in files]
    offs, total = pack_arena_layout(lens)
    host = np.zeros(total, np.uint8)
    for f, o in zip(files, offs):
        host[int(o):int(o) + f["size"]] = f["data"]
    arena = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    return arena, offs, lens


@pytest.mark.parametrize("join_lag", [1, 2, 3])
def test_device_form_pipelined(corpus, join_lag):
    from hashbox_amd import Engine
    big = [f for f in corpus if f["size"] > Mi]
    small = [f for f in corpus if f["size"] <= Mi]
    groups = [big[:3] + small[:5], small[5:20], small[::2], small[20:], big[3:] + small[1::3]]  # M P M P M
    is_match = [True, False, True, False, True]
    with Engine(0, md5_slice=64, join_lag=join_lag, k3_period=4) as e:
        batches = [_device_batch(g) for g in groups]
        # the plain batches alone
        alone = []
        for k in (1, 3):
            arena, offs, lens = batches[k]
            e.submit_device(arena.data_ptr(), offs, lens)
            alone.append(e.wait())
        for verdict_only in (False, True):
            for k, (arena, offs, lens) in enumerate(batches):
                if is_match[k]:
                    e.submit_device_match(arena.data_ptr(), offs, lens, [f["expect"] for f in groups[k]],
                                          chunks=not verdict_only)
                else:
                    e.submit_device(arena.data_ptr(), offs, lens)
            assert e.pending() == 5
            out = [e.wait() for _ in range(5)]  # FIFO
            assert e.pending() == 0
            for k in (0, 2, 4):
                assert [_got(r) for r in out[k]] == _want(groups[k]), (k, verdict_only)
                for r, f in zip(out[k], groups[k]):
                    assert (r.content_type, r.content_id) == (f["local"].content_type, f["local"].content_id)
                    if verdict_only:
                        assert r.chunks is None
                    else:
                        assert np.array_equal(r.chunks.ids, f["local"].ids)
                        assert np.array_equal(r.chunks.cut_ends, f["local"].cut_ends)
            for k, ref in zip((1, 3), alone):
                assert len(out[k]) == len(ref)
                for a, b in zip(out[k], ref):
                    assert np.array_equal(a.cut_ends, b.cut_ends) and np.array_equal(a.ids, b.ids)
                    assert (a.content_type, a.content_id) == (b.content_type, b.content_id)


def test_direct_call_refused_while_pending(engine, corpus):
    from hashbox_amd import HbxError
    small = [f for f in corpus if 0 < f["size"] <= Mi][:4]
    arena, offs, lens = _device_batch(small)
    engine.submit_device_match(arena.data_ptr(), offs, lens, [f["expect"] for f in small])
    try:
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):
            engine.match_chains([_random_ids(1, 1)], [_random_ids(1, 1)])
    finally:
        got = engine.wait()
    assert [_got(r) for r in got] == _want(small)
