"""GPU: the block locator (K13, hbx_locate.hip) through hbx_locate_ids.

Every expected record comes from plain Python below: a dict of the first
occurrence of each pool ID, and the chunk's place computed from the cut ends.
Nothing comes from the code under test, and every comparison is exact."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
MISS = (NONE, 0, 0, 0)


# ------------------------------------------------------------- the model --
def _slots(n: int) -> int:
    """The scratch table of n pool IDs: the smallest power of two >= 2 n, at least 64."""
    s = 64
    while s < 2 * n:
        s <<= 1
    return s


def _model(pool_ids, pool_cuts, want):
    """pool_ids / pool_cuts: one list per pool file; (file, chunk, off, len) per wanted ID."""
    first, place = {}, []
    for f, (ids, cuts) in enumerate(zip(pool_ids, pool_cuts)):
        assert len(ids) == len(cuts)
        for c, i in enumerate(ids):
            off = int(cuts[c - 1]) if c else 0
            first.setdefault(bytes(i), len(place))
            place.append((f, c, off, int(cuts[c]) - off))
    return [place[first[bytes(w)]] if bytes(w) in first else MISS for w in want]


def _got(rec):
    return [tuple(int(x) for x in r) for r in zip(rec["file"].tolist(), rec["chunk"].tolist(), rec["off"].tolist(),
                                                   rec["len"].tolist())]


def _check(engine, pool_ids, pool_cuts, want):
    want = list(want)
    exp = _model(pool_ids, pool_cuts, want)
    rec = engine.locate_ids(pool_ids, pool_cuts, want)
    assert rec.shape == (len(want),)
    assert _got(rec) == exp
    if want:
        assert engine.last_located == sum(e != MISS for e in exp)
    return exp


def _rows(a) -> list:
    return [bytes(x) for x in np.asarray(a, np.uint8).reshape(-1, 16)]


def _random_ids(n, seed) -> list:
    return _rows(np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, 16), dtype=np.uint8))


def _split(ids, seed, empty_files=True):
    """A flat ID list as pool files: random chunk counts (files without chunks among them) and cut ends."""
    rng = np.random.default_rng(seed)
    files, cuts, at = [], [], 0
    while at < len(ids):
        k = int(rng.integers(0, 40)) if empty_files else int(rng.integers(1, 40))
        k = min(k, len(ids) - at)
        files.append(ids[at:at + k])
        cuts.append(np.cumsum(rng.integers(1, 1 << 33, k, dtype=np.uint64)).tolist())
        at += k
    return files, cuts


def _id_at(home: int, slots: int, seed: int) -> bytes:
    """An ID whose home slot in a table of `slots` is `home`: LE64(id[0..8]) & (slots - 1)."""
    rng = np.random.default_rng(seed)
    lo = (int(rng.integers(0, 1 << 62)) & ~(slots - 1)) | home
    return lo.to_bytes(8, "little") + bytes(rng.integers(0, 256, 8, dtype=np.uint8))


# ------------------------------------------------------------------ sizes --
POOLS = (0, 1, 31, 32, 33, 255, 256, 257, 1000)
WANTS = (0, 1, 255, 256, 257)


@pytest.mark.parametrize("np_", POOLS)
def test_sizes_and_hit_miss_mix(engine, np_):
    assert (_slots(32), _slots(33)) == (64, 128)
    pool = _random_ids(np_, 10 + np_)
    files, cuts = _split(pool, np_)
    rng = np.random.default_rng(500 + np_)
    for nw in WANTS:
        absent = _random_ids(nw, 9000 + np_ + nw)
        hits = [pool[int(k)] for k in rng.integers(0, np_, nw)] if np_ else absent  # in random order, with repeats
        mixed = [h if rng.integers(0, 2) else a for h, a in zip(hits, absent)]
        for want in (hits, absent, mixed):
            exp = _check(engine, files, cuts, want)
            if want is absent or not np_:
                assert all(e == MISS for e in exp)
            elif want is hits:
                assert all(e != MISS for e in exp)


def test_every_pool_id_finds_itself(engine):
    pool = _random_ids(1000, 3)
    files, cuts = _split(pool, 3)
    exp = _check(engine, files, cuts, pool)
    assert len(set(exp)) == 1000 and MISS not in exp


# ------------------------------------------------------------- duplicates --
def test_duplicates_lowest_index_wins(engine):
    pool = _random_ids(300, 21)
    pool[-1] = pool[0]  # one ID at indices {0, last}
    files, cuts = _split(pool, 21, empty_files=False)
    exp = _check(engine, files, cuts, [pool[0], pool[-1], pool[150]])
    assert exp[0] == exp[1] and exp[0][:3] == (0, 0, 0)

    one = _random_ids(1, 22)[0]  # 1,000 copies of one ID: one contended slot takes every atomic min
    files, cuts = _split([one] * 1000, 22, empty_files=False)
    exp = _check(engine, files, cuts, [one] * 70 + _random_ids(3, 23))
    assert exp[0] == (0, 0, 0, int(cuts[0][0])) and exp[-1] == MISS

    ids = _random_ids(400, 24)  # every ID present twice, in two different orders
    rng = np.random.default_rng(24)
    pool = [ids[int(k)] for k in rng.permutation(400)] + [ids[int(k)] for k in rng.permutation(400)]
    files, cuts = _split(pool, 25)
    exp = _check(engine, files, cuts, ids)
    flat_first = {}
    for k, i in enumerate(pool):
        flat_first.setdefault(i, k)
    assert all(flat_first[i] < 400 for i in ids) and MISS not in exp


# -------------------------------------------------------------- collisions --
def test_crafted_collisions(engine):
    # 40 distinct IDs sharing one home slot (a table of 128)
    s = _slots(40)
    assert s == 128
    run = [_id_at(5, s, 100 + k) for k in range(40)]
    assert len(set(run)) == 40
    files, cuts = _split(run, 31)
    # wanted IDs that share the whole probe run with pool IDs and are absent: homes at its start, inside and end
    absent = [_id_at(5, s, 900), _id_at(20, s, 901), _id_at(44, s, 902), _id_at(45, s, 903)]
    exp = _check(engine, files, cuts, run[::-1] + absent)
    assert exp[-4:] == [MISS] * 4 and MISS not in exp[:-4]

    # a run whose home is the last slot: probing wraps around
    s = _slots(50)
    wrap = [_id_at(s - 1, s, 200 + k) for k in range(12)]
    pool = _random_ids(38, 32) + wrap
    files, cuts = _split(pool, 33)
    exp = _check(engine, files, cuts, wrap + [_id_at(s - 1, s, 950), _id_at(3, s, 951)])
    assert exp[-2] == MISS and MISS not in exp[:12]

    # equal in the first 8 bytes (so in the home slot), different in the last 8 ...
    base = _random_ids(30, 34)
    twins = [b[:8] + bytes(x ^ 0xFF for x in b[8:]) for b in base]
    # ... and equal in the last 12 bytes, different in word 0
    cousins = [bytes(x ^ 0x5A for x in b[:4]) + b[4:] for b in base]
    pool = base + twins[:15] + cousins[:15]
    files, cuts = _split(pool, 35)
    exp = _check(engine, files, cuts, base + twins + cousins)
    assert all(e != MISS for e in exp[:45]) and exp[45:60] == [MISS] * 15
    assert all(e != MISS for e in exp[60:75]) and exp[75:] == [MISS] * 15
    # one bit anywhere makes another ID
    one = base[0]
    others = [bytes(x ^ (1 << (k % 8)) if n == k // 8 else x for n, x in enumerate(one)) for k in range(128)]
    assert _check(engine, [[one]], [[77]], others + [one]) == [MISS] * 128 + [(0, 0, 0, 77)]


# ---------------------------------------------------------- record fields --
def test_record_fields_and_files_without_chunks(engine):
    ids = _random_ids(12, 41)
    # files without chunks at the start, adjacent in the middle, and at the end; a one-chunk file
    files = [[], [], ids[0:1], ids[1:5], [], [], ids[5:6], [], ids[6:12], [], []]
    cuts = [[], [], [65_536], [70_000, 140_000, 140_001, 1 << 33], [], [], [1], [],
            [1 << 32, (1 << 32) + 5, 1 << 40, (1 << 40) + 1, 1 << 41, 1 << 42], [], []]
    want = ids[::-1] + _random_ids(2, 42)
    exp = _check(engine, files, cuts, want)
    assert exp[11] == (2, 0, 0, 65_536)                       # the one-chunk file: off 0
    assert exp[10] == (3, 0, 0, 70_000) and exp[7] == (3, 3, 140_001, (1 << 33) - 140_001)
    assert exp[6] == (6, 0, 0, 1)
    assert exp[0] == (8, 5, 1 << 41, 1 << 41) and exp[5] == (8, 0, 0, 1 << 32)

    # pool_first[0] != 0, and n_found, straight through the C-ABI
    from hashbox_amd import _lib
    lead = 7
    first = np.cumsum([lead] + [len(f) for f in files]).astype(np.uint64)
    flat = np.frombuffer(b"".join(_random_ids(lead, 43) + ids), np.uint8)
    fcuts = np.array([999] * lead + [c for f in cuts for c in f], np.uint64)
    w = np.frombuffer(b"".join(want), np.uint8)
    rec = (_lib.BlockLoc * len(want))()
    found = ctypes.c_uint64(123)
    rc = engine._L.hbx_locate_ids(engine._ctx, len(files), first.ctypes.data, flat.ctypes.data, fcuts.ctypes.data,
                                  len(want), w.ctypes.data, rec, ctypes.byref(found))
    assert rc == 0 and found.value == 12
    assert [(r.file, r.chunk, r.off, r.len, r.reserved) for r in rec] == [e + (0,) for e in exp]
    # n_found may be NULL; n_want == 0 is HBX_OK
    assert engine._L.hbx_locate_ids(engine._ctx, len(files), first.ctypes.data, flat.ctypes.data, fcuts.ctypes.data,
                                    len(want), w.ctypes.data, rec, None) == 0
    assert engine._L.hbx_locate_ids(engine._ctx, 0, None, None, None, 0, None, None, None) == 0
    # an empty pool given as files without chunks
    assert _check(engine, [[], []], [[], []], ids[:3]) == [MISS] * 3


# ----------------------------------------------------------- repeat calls --
def test_repeat_calls_clear_the_table(engine):
    big = _random_ids(700, 51)
    small = big[100:120]
    bf, bc = _split(big, 51)
    sf, sc = _split(small, 52)
    want = big[:200]
    first = _check(engine, bf, bc, want)
    second = _check(engine, sf, sc, want)  # what only the larger pool held is a miss now
    assert MISS not in first and [e != MISS for e in second] == [100 <= k < 120 for k in range(200)]
    assert _check(engine, bf, bc, want) == first


# ---------------------------------------------------------- pending batch --
def test_refused_while_a_batch_is_pending(engine):
    import torch
    from hashbox_amd import HbxError, pack_arena_layout
    lens = [70_000, 5]
    offs, total = pack_arena_layout(lens)
    arena = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.submit_device(arena.data_ptr(), offs, lens)
    try:
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):
            engine.locate_ids([_random_ids(1, 1)], [[5]], _random_ids(1, 2))
    finally:
        assert len(engine.wait()) == 2
    assert _check(engine, [_random_ids(1, 1)], [[5]], _random_ids(1, 1)) == [(0, 0, 0, 5)]
