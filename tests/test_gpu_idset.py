"""GPU: the block-ID set (K9, hbx_dedup.hip) through hbx_idset_*.  Every
comparison is exact equality against the dict / set model below.

THE INVARIANT under test: an ID comes back seen (fresh = False) only if an
equal 16-byte ID was inserted before it, in an earlier call or at a lower
index of the same call.  The shapes are the smallest that can break the
kernels: races on one slot across a wave boundary and across workgroups,
probe runs that share the hashed bytes, a run that wraps past the last slot,
and a full table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ids(rows) -> np.ndarray:
    return np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).reshape(-1, 16).copy()


def _model_insert(model: dict, ids: np.ndarray) -> np.ndarray:
    """fresh[i] = ids[i] is not in the model yet; then it is (insertion order kept)."""
    out = np.zeros(ids.shape[0], bool)
    for i, row in enumerate(ids):
        k = row.tobytes()
        if k not in model:
            model[k] = len(model)
            out[i] = True
    return out


def _random_ids(n, seed) -> np.ndarray:
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, 16), dtype=np.uint8)


@pytest.fixture()
def make_set(engine):
    from hashbox_amd import IdSet
    made = []

    def make(capacity):
        made.append(IdSet(engine, capacity))
        return made[-1]
    yield make
    for s in made:
        s.close()


def test_empty_and_single(make_set):
    s = make_set(100)
    assert s.insert(np.zeros((0, 16), np.uint8)).shape == (0,)
    assert s.contains(np.zeros((0, 16), np.uint8)).shape == (0,)
    assert (s.count, s.capacity, s.slots, s.dropped) == (0, 100, 256, 0)
    assert s.export().shape == (0, 16)
    one = _random_ids(1, 1)
    assert s.contains(one).tolist() == [False]
    assert s.insert(one).tolist() == [True]
    assert s.contains(one).tolist() == [True]
    assert s.insert(one).tolist() == [False]
    assert s.count == 1 and np.array_equal(s.export(), one)


@pytest.mark.parametrize("n", [65, 1000])
def test_copies_of_one_id(make_set, n):
    """Every thread of the mark meets the same scratch slot (atomicMin across a
    wave boundary at 65, across workgroups at 1000): only index 0 is fresh."""
    s = make_set(64)
    ids = np.repeat(_random_ids(1, 2), n, axis=0)
    fresh = s.insert(ids)
    assert fresh[0] and not fresh[1:].any()
    assert s.count == 1
    assert not s.insert(ids).any()


def test_shared_first_eight_bytes(make_set):
    """200 IDs with one home slot that differ only in byte 15: the whole 16
    bytes are compared, and the probe run is 200 slots long."""
    base = _random_ids(1, 3)[0]
    ids = np.repeat(base[None, :], 200, axis=0)
    ids[:, 15] = np.arange(200, dtype=np.uint8)
    s = make_set(1000)
    assert s.insert(ids).all()
    assert s.count == 200 and s.contains(ids).all()
    other = ids[:50].copy()
    other[:, 15] = np.arange(200, 250, dtype=np.uint8)
    assert not s.contains(other).any()
    model = {r.tobytes(): i for i, r in enumerate(ids)}
    again = np.concatenate([other, ids[::-1], other])
    assert np.array_equal(s.insert(again), _model_insert(model, again))
    assert {r.tobytes() for r in s.export()} == set(model)


def test_one_home_slot_across_workgroups(make_set):
    """4,096 distinct IDs with one LE64(id[0..8]): one home slot in the set
    (16,384 slots) and one in the mark's scratch table, so both probe runs are
    4,096 long.  Each ID occurs three times in one insert of 12,288, once in
    each third under another permutation: the three copies always lie in three
    different 256-thread workgroups of the mark (16 workgroups per third)."""
    n = 4096
    base = _random_ids(1, 9)[0]
    ids = np.repeat(base[None, :], n, axis=0)
    ids[:, 8:] = np.random.Generator(np.random.PCG64(10)).permutation(1 << 16)[:n].astype("<u8").view(np.uint8) \
        .reshape(n, 8)
    assert len({r.tobytes() for r in ids}) == n and len({r[:8].tobytes() for r in ids}) == 1
    g = np.random.Generator(np.random.PCG64(11))
    where = np.stack([g.permutation(n) + k * n for k in range(3)], axis=1)  # [id, copy] -> index in the call
    assert len({tuple(sorted(set((where[j] // 256).tolist()))) for j in range(n)}) > 1
    assert all(len(set((where[j] // 256).tolist())) == 3 for j in range(n))
    call = np.zeros((3 * n, 16), np.uint8)
    for k in range(3):
        call[where[:, k]] = ids
    s = make_set(2 * n)
    assert s.slots == 4 * n
    model = {}
    want = _model_insert(model, call)
    assert int(want.sum()) == n and want[:n].all() and not want[n:].any()
    assert np.array_equal(s.insert(call), want)
    assert (s.count, s.dropped) == (n, 0)
    assert s.contains(ids).all()
    order = s.export()
    assert {r.tobytes() for r in order} == set(model)
    s.truncate(1000)
    assert s.count == 1000
    assert s.contains(order[:1000]).all() and not s.contains(order[1000:]).any()
    assert np.array_equal(s.export(), order[:1000])


def test_all_zero_and_all_ff_are_ordinary_keys(make_set):
    s = make_set(16)
    ids = _ids([bytes(16), b"\xff" * 16])
    assert s.contains(ids).tolist() == [False, False]
    assert s.insert(ids[:1]).tolist() == [True]
    assert s.contains(ids).tolist() == [True, False]
    assert s.insert(ids).tolist() == [False, True]
    assert s.contains(ids).tolist() == [True, True] and s.count == 2


def test_probe_run_wraps_past_the_last_slot(make_set, engine):
    """Capacity 32 has S = 64 slots; five IDs with LE64(id[0..8]) = 63 take
    slots 63, 0, 1, 2, 3."""
    s = make_set(32)
    assert s.slots == 64
    ids = np.zeros((5, 16), np.uint8)
    ids[:, 0] = 63
    ids[:, 8] = np.arange(1, 6)
    assert s.insert(ids).all()
    assert s.contains(ids).all() and s.count == 5
    # one at a time as well (each call finds the run the earlier ones left)
    t = make_set(32)
    for i in range(5):
        assert t.insert(ids[i:i + 1]).tolist() == [True]
    assert t.contains(ids).all() and not t.insert(ids).any()
    # the same home slot in a larger table does not wrap, and is not confused
    miss = ids.copy()
    miss[:, 8] += 100
    assert not s.contains(miss).any()


def test_full_set_degrades_to_fresh(make_set):
    s = make_set(32)
    ids = _random_ids(33, 4)
    assert s.insert(ids[:32]).all()
    assert (s.count, s.dropped) == (32, 0)
    extra = ids[32:33]
    assert s.insert(extra).tolist() == [True]
    assert (s.count, s.dropped, s.capacity) == (32, 1, 32)
    assert s.contains(extra).tolist() == [False]
    assert s.insert(extra).tolist() == [True]  # never seen: it was not inserted
    assert (s.count, s.dropped) == (32, 2)
    assert s.contains(ids[:32]).all() and not s.insert(ids[:32]).any()
    assert {r.tobytes() for r in s.export()} == {r.tobytes() for r in ids[:32]}
    # several over the brim in one call, with a repeat among them
    t = make_set(4)
    more = _random_ids(7, 5)
    more[6] = more[5]
    assert t.insert(more).tolist() == [True] * 6 + [False]
    assert (t.count, t.dropped) == (4, 2)
    kept = {r.tobytes() for r in t.export()}
    assert len(kept) == 4 and kept <= {r.tobytes() for r in more}
    assert t.contains(more).tolist() == [r.tobytes() in kept for r in more]


def test_random_draws_match_the_model(make_set):
    """200,000 draws from a pool of 50,000 IDs over four inserts."""
    g = np.random.Generator(np.random.PCG64(6))
    pool = g.integers(0, 256, (50_000, 16), dtype=np.uint8)
    draws = pool[g.integers(0, pool.shape[0], 200_000)]
    s = make_set(60_000)
    model = {}
    total = 0
    for part in np.split(draws, [30_000, 100_000, 100_001]):
        fresh = s.insert(part)
        assert np.array_equal(fresh, _model_insert(model, part))
        total += int(fresh.sum())
        assert s.count == len(model)
    assert 0 < total < draws.shape[0] and total == len(model)
    exported = s.export()
    assert exported.shape[0] == len(model)
    assert {r.tobytes() for r in exported} == set(model)
    assert s.contains(pool).tolist() == [r.tobytes() in model for r in pool]
    assert s.dropped == 0


def test_truncate_to_a_checkpoint(make_set):
    from hashbox_amd import HbxError
    s = make_set(5000)
    ids = _random_ids(3000, 7)
    assert s.insert(ids[:1000]).all()
    mark = s.count
    assert mark == 1000
    assert s.insert(ids[1000:]).all() and s.count == 3000
    s.truncate(mark)
    assert s.count == mark
    assert s.contains(ids[:1000]).all()
    assert not s.contains(ids[1000:]).any()
    assert {r.tobytes() for r in s.export()} == {r.tobytes() for r in ids[:1000]}
    assert s.insert(ids[1000:]).all() and not s.insert(ids).any()
    with pytest.raises(HbxError, match="HBX_ERR_ARG"):
        s.truncate(3001)
    s.truncate(0)
    assert s.count == 0 and not s.contains(ids).any()


def test_refusals(make_set, engine):
    import torch
    from hashbox_amd import Engine, HbxError, IdSet, pack_arena_layout
    s = make_set(1000)
    ids = _random_ids(4, 8)
    # a set of another context
    with Engine(0) as other:
        with pytest.raises(HbxError, match="HBX_ERR_ARG"):
            other._check(other._L.hbx_idset_insert(other._ctx, s._h, 4, ids.ctypes.data, None), "hbx_idset_insert")
        mine = IdSet(other, 10)
        with pytest.raises(HbxError, match="HBX_ERR_ARG"):
            engine.submit_device(0, [], [], dedup=mine)
        mine.close()
    # a direct call, and a destroy, while a batch is pending
    lens = [300_000, 70_000]
    offs, total = pack_arena_layout(lens)
    arena = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.submit_device(arena.data_ptr(), offs, lens, dedup=s)
    try:
        for call in (lambda: s.insert(ids), lambda: s.contains(ids), lambda: s.count, s.export,
                     lambda: s.truncate(0), s.close):
            with pytest.raises(HbxError, match="HBX_ERR_STATE"):
                call()
    finally:
        got = engine.wait()
    model = {}
    for g in got:
        assert np.array_equal(g.fresh, _model_insert(model, g.ids))
    assert s.count == len(model) >= 2
