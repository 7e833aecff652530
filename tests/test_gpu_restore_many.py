"""GPU: the chains of many files back into their bytes, or compared with local
copies, in one call (hbx_restore_files_blocks, hbx_restore_files_stream, K11;
restoreDir / restoreFileData and diffDir / diffEntry / diffFileData,
hashback/restore.go:45-66, 137-162, 249-277, 279-414).  Expected bytes are
always the original bytes, with hashlib for the IDs and CPython's zlib for the
streams (the helpers of tests/test_gpu_restore.py); only a bad block's status
is compared with what Engine.restore_blocks gives for that block alone.
"""
import errno
import os
import stat
import zlib

import numpy as np
import pytest

from tests.test_restore_many_abi import window_end
from tests.test_gpu_restore import RAW, ZLIB, _corruptions, _inflates_to, _text, block_id, chain8, edge_chain, wire

pytestmark = pytest.mark.gpu

PM = 16384  # hbxm::kPieceMany: bytes per K11 wave
P10 = 65536  # hbxr::kPiece, the P of edge_chain()
Mi = 1 << 20
ERR_IO = -4
NO_OFF = 2**64 - 1

_cache = {}


def edge_chain_pm():
    """edge_chain()'s lengths with P = kPieceMany."""
    if "edge_pm" not in _cache:
        P = PM
        lens = [0, 1, 15, 16, 17, 63, 64, 65, P - 1, P, P + 1] + [1] * 13 + [17, P + 1, 0, 15, P - 1, 63, 3, P, 5,
                                                                          P + 1, 2, P - 1]
        rng = np.random.default_rng(98)
        blocks = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) if i % 2 else _text(n, 400 + i)
                  for i, n in enumerate(lens)]
        _cache["edge_pm"] = (blocks, [block_id(b) for b in blocks])
    return _cache["edge_pm"]


def deal(items, sizes=(0, 1, 2, 3, 5)):
    """The items dealt in order into groups of 0, 1, 2, 3, 5, 0, 1, ... items."""
    out, at, k = [], 0, 0
    while at < len(items):
        n = sizes[k % len(sizes)]
        out.append(items[at:at + n])
        at += n
        k += 1
    return out


def text_pool():
    """4 MiB of text that small text files are cut from."""
    if "pool" not in _cache:
        _cache["pool"] = _text(4 * Mi, 77)
    return _cache["pool"]


def knobs_many(engine):
    w, p, r = engine.knobs()["restore_many"]
    return {"windows": w, "passes": p, "retries": r}


# ----------------------------------------------------------------- edges --
@pytest.mark.parametrize("mode", ["z", "r", "zr", "rz"])
@pytest.mark.parametrize("piece", [P10, PM])
def test_gather_edges_across_files_with_canaries(engine, mode, piece):
    """Files of 0, 1, 2, 3 and 5 blocks; in the packed image every destination
    offset mod 16 occurs, with block lengths around 16, 64 and the piece size
    (K10's and K11's).  64 canary bytes on each side of out stay untouched."""
    blocks, ids = edge_chain() if piece == P10 else edge_chain_pm()
    want = b"".join(blocks)
    datas, types = wire(blocks, mode)
    chains = deal(list(zip(types, datas, ids)))
    files = deal(blocks)
    assert [len(c) for c in chains[:5]] == [0, 1, 2, 3, 5] and sum(len(c) for c in chains) == len(blocks)
    dst = np.concatenate([[0], np.cumsum([len(b) for b in blocks])])[:-1]
    assert set(int(o) % 16 for o in dst) == set(range(16))
    buf = np.full(64 + len(want) + 64, 0xA5, np.uint8)
    r = engine.restore_files_blocks(chains, out=buf[64:64 + len(want)])
    assert [s.tolist() for s in r.status] == [[0] * len(c) for c in chains]
    assert r.n_good.tolist() == [len(c) for c in chains]
    assert r.data == [b"".join(f) for f in files]
    assert buf[64:64 + len(want)].tobytes() == want
    assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all()
    assert r.out_offs.tolist() == np.concatenate([[0], np.cumsum([sum(len(b) for b in f) for f in files])]).tolist()
    for f, bo in zip(files, r.blk_offs):
        assert bo.tolist() == np.concatenate([[0], np.cumsum([len(b) for b in f])])[:-1].astype(int).tolist()
    assert knobs_many(engine) == {"windows": 1, "passes": 1, "retries": 0}


def test_no_files_and_files_without_blocks(engine):
    r = engine.restore_files_blocks([])
    assert r.data == [] and r.out_offs.tolist() == [0]
    r = engine.restore_files_blocks([[], []])
    assert r.data == [b"", b""] and r.n_good.tolist() == [0, 0] and r.out_offs.tolist() == [0, 0, 0]
    d = engine.restore_files_blocks([[], []], local=[b"", b"abc"])
    assert d.first_diff == [None, 0] and d.data is None


# ----------------------------------------------------------- prefix rule --
def _four_files():
    blocks, ids, zs = chain8()
    rot = lambda x, k: x[k:] + x[:k]  # noqa: E731
    return [(rot(blocks, k), rot(ids, k), rot(zs, k)) for k in (0, 3, 5, 6)]


@pytest.mark.parametrize("kind", ["truncated", "middle_byte", "adler", "wrong_id"])
def test_prefix_rule_per_file(engine, kind):
    files = _four_files()
    b1, i1, z1 = files[1]
    if kind == "wrong_id":
        bad_z, bad_id = z1[2], block_id(b1[2] + b"x")
    else:
        bad_z, bad_id = _corruptions(z1[2])[kind], i1[2]
        assert _inflates_to(bad_z) != b1[2], "the corruption changes nothing: the case would prove nothing"
    chains = [[(ZLIB, z, i) for z, i in zip(zs, ids)] for _, ids, zs in files]
    chains[1][2] = (ZLIB, bad_z, bad_id)
    want = [b"".join(b) for b, _, _ in files]
    want[1] = b1[0] + b1[1]
    total = sum(len(w) for w in want)
    buf = np.full(total + 64, 0xA5, np.uint8)
    r = engine.restore_files_blocks(chains, out=buf)
    assert r.n_good.tolist() == [8, 2, 8, 8]
    assert r.data == want
    assert r.out_offs.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()  # packed
    assert buf[:total].tobytes() == b"".join(want) and (buf[total:] == 0xA5).all()
    alone = engine.restore_blocks([bad_z], [ZLIB], [bad_id])
    assert int(alone.status[0]) != 0
    for f in (0, 2, 3):
        assert r.status[f].tolist() == [0] * 8
    assert r.status[1].tolist() == [0, 0, int(alone.status[0]), 0, 0, 0, 0, 0]  # every block gets its own status
    if kind == "adler":
        assert int(r.status[1][2]) == 1
    if kind == "wrong_id":
        assert int(r.status[1][2]) == 7
    assert r.blk_offs[1].tolist() == [0, len(b1[0])] + [NO_OFF] * 6


# ----------------------------------------------------------------- hints --
def test_size_hints_change_no_result(engine):
    blocks, ids, _ = chain8()
    pool = text_pool()
    small = [pool[1000 * k:1000 * k + 300 + 37 * k] for k in range(5)]
    files = [blocks[:3], [small[0]], blocks[3:5], [small[1]], [small[2]], blocks[5:], [small[3]], [small[4]]]
    sizes = [sum(len(b) for b in f) for f in files]
    chains = [[(ZLIB, zlib.compress(b, 6), block_id(b)) for b in f] for f in files]
    chains[2][0] = (RAW, files[2][0], block_id(files[2][0]))
    want = [b"".join(f) for f in files]
    retries = {}
    for name, hints in (("exact", sizes), ("zero", [0] * 8), ("one", [1] * 8), ("ten", [10 * s for s in sizes]),
                        ("null", None)):
        r = engine.restore_files_blocks(chains, size_hints=hints)
        assert r.data == want, name
        assert r.n_good.tolist() == [len(f) for f in files], name
        assert [s.tolist() for s in r.status] == [[0] * len(f) for f in files], name
        assert r.out_offs.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist(), name
        retries[name] = knobs_many(engine)["retries"]
    # with hints of 1 every zlib block but the one of a single byte outgrew its slot and was inflated again
    assert retries == {"exact": 0, "zero": 0, "one": 11, "ten": 0, "null": 0}
    # a stream that outgrows max_block too fails with status 3, whatever the hint
    for hints in ([1], [0], None):
        r = engine.restore_files_blocks([[(ZLIB, zlib.compress(blocks[0], 6), ids[0])]], size_hints=hints,
                                        max_block=len(blocks[0]) - 1)
        assert r.status[0].tolist() == [3] and r.data == [b""]


# ------------------------------------------------------------------ diff --
def _three_files():
    blocks, ids, zs = chain8()
    groups = [(2, 5), (0, 2), (5, 8)]  # the middle file starts with the block of nine K11 pieces
    files = [blocks[a:b] for a, b in groups]
    chains = [[(ZLIB, z, i) for z, i in zip(zs[a:b], ids[a:b])] for a, b in groups]
    return files, chains


def test_diff_identical_and_lengths(engine):
    files, chains = _three_files()
    local = [b"".join(f) for f in files]
    r = engine.restore_files_blocks(chains, local=local)
    assert r.first_diff == [None, None, None] and r.data is None and r.n_good.tolist() == [3, 2, 3]
    mid = local[1]
    for other, want in ((mid[:-1], len(mid) - 1), (mid + b"!", len(mid)), (b"", 0)):
        r = engine.restore_files_blocks(chains, local=[local[0], other, local[2]])
        assert r.first_diff == [None, want, None], len(other)
    # raw blocks, whose staged source is unaligned
    raw = [[(RAW, b, i) for b, (_, _, i) in zip(f, c)] for f, c in zip(files, chains)]
    assert engine.restore_files_blocks(raw, local=local).first_diff == [None, None, None]


def test_diff_single_flips_in_the_middle_file(engine):
    files, chains = _three_files()
    local = [b"".join(f) for f in files]
    n0 = len(files[1][0])
    assert n0 > 9 * PM
    borders = [k * PM for k in range(1, 10)] + [n0]  # K11's piece borders in block 0, and the block border
    at = sorted({0, len(local[1]) - 1} | {b + d for b in borders for d in (-1, 0, 1)})
    for pos in at:
        mid = bytearray(local[1])
        mid[pos] ^= 0x01
        r = engine.restore_files_blocks(chains, local=[local[0], bytes(mid), local[2]])
        assert r.first_diff == [None, pos, None], pos


def test_diff_flips_in_two_files_at_once(engine):
    files, chains = _three_files()
    local = [bytearray(b"".join(f)) for f in files]
    local[0][70_003] ^= 0x80
    local[0][150_000] ^= 0x80
    local[2][len(local[2]) - 1] ^= 0x80
    local[2][PM + 5] ^= 0x80
    r = engine.restore_files_blocks(chains, local=[bytes(x) for x in local])
    assert r.first_diff == [70_003, None, PM + 5]
    # a difference before the shorter end still wins; only the good prefix is compared
    r = engine.restore_files_blocks(chains, local=[bytes(local[0][:-1]), bytes(local[1]), bytes(local[2])])
    assert r.first_diff == [70_003, None, PM + 5]
    bad = [list(c) for c in chains]
    bad[2][1] = (ZLIB, bad[2][1][1][:40], bad[2][1][2])
    end = len(files[2][0])
    assert PM + 5 < end
    r = engine.restore_files_blocks(bad, local=[bytes(x) for x in local])
    assert r.n_good.tolist() == [3, 2, 1] and r.first_diff == [70_003, None, PM + 5]
    whole = b"".join(files[2])
    r = engine.restore_files_blocks(bad, local=[bytes(local[0]), bytes(local[1]), whole[:end + 9] + b"?" + whole[end + 10:]])
    assert r.first_diff == [70_003, None, end]  # the lengths differ there


# --------------------------------------------------------------- windows --
def _window_set():
    """Twenty small files, one 3 MiB file of six 512 KiB blocks, twenty more."""
    if "wset" not in _cache:
        pool = text_pool()
        rng = np.random.default_rng(21)
        small = [pool[int(o):int(o) + int(n)] for o, n in zip(rng.integers(0, 3 * Mi, 40), rng.integers(1, 3000, 40))]
        big_blocks = [_text(512 * 1024, 600 + k) if k % 2 == 0 else
                      bytes(np.random.default_rng(600 + k).integers(0, 256, 512 * 1024, dtype=np.uint8)) for k in range(6)]
        files = [[s] for s in small[:20]] + [big_blocks] + [[s] for s in small[20:]]
        wired = [[(RAW, b) if (k + j) % 4 == 3 else (ZLIB, zlib.compress(b, 6)) for j, b in enumerate(f)]
                 for k, f in enumerate(files)]
        _cache["wset"] = (files, wired, [[block_id(b) for b in f] for f in files])
    return _cache["wset"]


def test_windows_across_files_to_paths_and_diff(engine, tmp_path):
    files, wired, ids = _window_set()
    mb = 528 * 1024  # (zlib -6 stores a random 512 KiB block in a little more than 512 KiB)
    wb = 2 * (mb + 512) + 4096  # two blocks of the big file per window; a window holds all twenty small files
    sizes = [sum(len(b) for b in f) for f in files]
    caps = [len(d) if t == RAW else min(mb, sizes[f]) for f, w in enumerate(wired) for t, d in w]
    ends, owner = [0], [f for f, w in enumerate(wired) for _ in w]
    while ends[-1] < len(caps):
        ends.append(window_end(caps, wb, ends[-1]))
    in_window = [set(owner[a:b]) for a, b in zip(ends, ends[1:])]
    assert sum(20 in w for w in in_window) >= 3 and any(len(w) >= 10 for w in in_window)
    paths = [tmp_path / f"f{k:02d}.bin" for k in range(len(files))]
    res = engine.restore_files(ids, lambda f, i: wired[f][i], paths, size_hints=sizes, window_bytes=wb,
                               io_threads=4, max_block=mb)
    k = knobs_many(engine)
    assert k == {"windows": len(in_window), "passes": len(in_window), "retries": 0} and k["windows"] >= 4
    for f, (p, r) in enumerate(zip(paths, res)):
        assert p.read_bytes() == b"".join(files[f]), f
        assert (r.bytes, r.n_good, r.bad_index, r.errno) == (sizes[f], len(files[f]), None, 0), f
    src = lambda f, i: wired[f][i]  # noqa: E731
    assert engine.diff_files(ids, src, paths, size_hints=sizes, window_bytes=wb, io_threads=4, max_block=mb) == \
        [(True, None)] * len(files)
    # a flip in the big file's third window, one in a small file behind it, one file a byte short
    big = bytearray(b"".join(files[20]))
    at = 4 * mb + 12_345
    big[at] ^= 0x04
    paths[20].write_bytes(bytes(big))
    s30 = bytearray(b"".join(files[30]))
    s30[len(s30) - 1] ^= 0x04
    paths[30].write_bytes(bytes(s30))
    paths[5].write_bytes(b"".join(files[5])[:-1])
    got = engine.diff_files(ids, src, paths, size_hints=sizes, window_bytes=wb, io_threads=4, max_block=mb)
    want = [(True, None)] * len(files)
    want[20], want[30], want[5] = (False, at), (False, len(s30) - 1), (False, sizes[5] - 1)
    assert got == want
    # without hints every zlib block takes a max_block slot: more windows, the same files
    out2 = [tmp_path / f"g{k:02d}.bin" for k in range(len(files))]
    engine.restore_files(ids, src, out2, window_bytes=wb, io_threads=4, max_block=mb)
    assert knobs_many(engine)["windows"] > k["windows"]
    assert all(p.read_bytes() == b"".join(f) for p, f in zip(out2, files))
    # hints of one byte: every longer zlib block is inflated again into a max_block slot, and a staged window then
    # runs as several passes, none holding more than window_bytes of corrected capacities
    out3 = [tmp_path / f"h{k:02d}.bin" for k in range(len(files))]
    res = engine.restore_files(ids, src, out3, size_hints=[1] * len(files), window_bytes=wb, io_threads=4, max_block=mb)
    k3 = knobs_many(engine)
    n_zlib_longer = sum(1 for w, f in zip(wired, files) for (t, _), b in zip(w, f) if t == ZLIB and len(b) > 1)
    assert k3["retries"] == n_zlib_longer and k3["passes"] > k3["windows"], k3
    assert all(r.bad_index is None and r.errno == 0 for r in res)
    assert all(p.read_bytes() == b"".join(f) for p, f in zip(out3, files))
    assert engine.diff_files(ids, src, out3, size_hints=[1] * len(files), window_bytes=wb, io_threads=4,
                             max_block=mb) == [(True, None)] * len(files)


# ------------------------------------------------------------------ many --
def test_ten_thousand_small_files_in_one_window(engine, tmp_path):
    """10,000 text files of 200-3,000 bytes, one zlib block each: with exact
    hints they share one window, and the inflate call sees >= 8,192 short
    compressible streams (the condition for K8's lane-per-stream kernel)."""
    pool = text_pool()
    rng = np.random.default_rng(31)
    n = 10_000
    lens = rng.integers(200, 3001, n)
    offs = rng.integers(0, len(pool) - 3001, n)
    files = [pool[int(o):int(o) + int(k)] for o, k in zip(offs, lens)]
    zs = [zlib.compress(f, 6) for f in files]
    ids = [[block_id(f)] for f in files]
    assert 10 * sum(len(z) for z in zs) < 7 * int(lens.sum())  # compressible enough for the lane kernel
    paths = [tmp_path / f"{k:05d}.txt" for k in range(n)]
    res = engine.restore_files(ids, lambda f, i: (ZLIB, zs[f]), paths, size_hints=lens.tolist(),
                               window_bytes=64 * Mi, io_threads=16)
    assert knobs_many(engine) == {"windows": 1, "passes": 1, "retries": 0}
    assert all(r.bad_index is None and r.errno == 0 for r in res)
    assert [r.bytes for r in res] == lens.tolist()
    for k, p in enumerate(paths):
        assert p.read_bytes() == files[k], k
    # the same set through the blocks call
    r = engine.restore_files_blocks([[(ZLIB, z, i[0])] for z, i in zip(zs, ids)], size_hints=lens.tolist())
    assert r.data == files and knobs_many(engine)["windows"] == 1


# ---------------------------------------------------------------- stream --
def _stream_set():
    """300 files of 0-200 KB, cut into blocks of at most 60,000 bytes, text and
    random data mixed, zlib and raw mixed."""
    if "sset" not in _cache:
        pool = text_pool()
        rng = np.random.default_rng(41)
        noise = bytes(rng.integers(0, 256, Mi, dtype=np.uint8))
        sizes = [int(x) for x in rng.integers(0, 200_001, 300)]
        sizes[0] = sizes[7] = sizes[299] = 0
        files, wired, ids = [], [], []
        for f, n in enumerate(sizes):
            base = pool if f % 3 else noise
            o = int(rng.integers(0, len(base) - 200_001))
            data = base[o:o + n]
            blocks = [data[a:a + 60_000] for a in range(0, n, 60_000)]
            files.append(data)
            wired.append([(RAW, b) if (f + j) % 5 == 0 else (ZLIB, zlib.compress(b, 1)) for j, b in enumerate(blocks)])
            ids.append([block_id(b) for b in blocks])
        _cache["sset"] = (files, wired, ids)
    return _cache["sset"]


def test_stream_to_paths_with_a_bad_path_and_a_failing_source(engine, tmp_path):
    files, wired, ids = _stream_set()
    sizes = [len(f) for f in files]
    paths = [tmp_path / f"s{k:03d}.bin" for k in range(300)]
    paths[100] = tmp_path / "missing" / "dir" / "s100.bin"
    assert sizes[100] > 0
    res = engine.restore_files(ids, lambda f, i: wired[f][i], paths, size_hints=sizes, window_bytes=8 * Mi,
                               io_threads=4)
    assert knobs_many(engine)["windows"] >= 2
    for f in range(300):
        if f == 100:
            assert res[f].errno == errno.ENOENT and not paths[f].exists()
            assert (res[f].bytes, res[f].bad_index) == (sizes[f], None)
            continue
        assert res[f].errno == 0 and res[f].bad_index is None and res[f].bytes == sizes[f], f
        assert paths[f].read_bytes() == files[f], f
    assert paths[0].exists() and paths[0].read_bytes() == b""  # a file without blocks is created empty

    class SourceDown(Exception):
        pass

    def failing(f, i):
        if f == 150:
            raise SourceDown("file 150")
        return wired[f][i]
    again = [tmp_path / f"t{k:03d}.bin" for k in range(300)]
    with pytest.raises(SourceDown):
        engine.restore_files(ids, failing, again, size_hints=sizes, window_bytes=8 * Mi, io_threads=4)
    # the library's own status for a failing source
    import ctypes
    from hashbox_amd import _lib
    first = np.concatenate([[0], np.cumsum([len(c) for c in ids])]).astype(np.uint64)
    ida = np.frombuffer(b"".join(i for c in ids for i in c), np.uint8)
    parr = (ctypes.c_char_p * 300)(*[os.fsencode(p) for p in again])
    out = (_lib.RestoredFile * 300)()
    cb = _lib.FILE_BLOCK_SOURCE(lambda user, f, i, dst, cap, ln, ty: 1 if f == 150 else _deliver(wired, f, i, dst, cap, ln, ty))
    rc = engine._L.hbx_restore_files_stream(engine._ctx, 300, first.ctypes.data, ida.ctypes.data,
                                            ctypes.cast(cb, ctypes.c_void_p), None, None, 8 * Mi, parr, None, 4, 0, out)
    assert rc == ERR_IO
    assert engine.pending() == 0
    # afterwards the same engine restores the set
    res = engine.restore_files(ids, lambda f, i: wired[f][i], again, size_hints=sizes, window_bytes=8 * Mi,
                               io_threads=4)
    assert all(r.errno == 0 and r.bad_index is None for r in res)
    assert all(p.read_bytes() == f for p, f in zip(again, files))
    # a bad block is its file's result; the others complete
    broken = [list(c) for c in wired]
    victim = next(f for f in range(300) if len(wired[f]) >= 3 and wired[f][1][0] == ZLIB)
    broken[victim][1] = (ZLIB, wired[victim][1][1][:20])
    third = [tmp_path / f"u{k:03d}.bin" for k in range(300)]
    res = engine.restore_files(ids, lambda f, i: broken[f][i], third, size_hints=sizes, window_bytes=8 * Mi,
                               io_threads=4)
    assert res[victim].bad_index == 1 and 1 <= res[victim].bad_status <= 7 and res[victim].n_good == 1
    assert third[victim].read_bytes() == files[victim][:60_000]
    assert all(third[f].read_bytes() == files[f] and res[f].bad_index is None for f in range(300) if f != victim)


def _deliver(wired, f, i, dst, cap, ln, ty):
    import ctypes
    t, data = wired[f][i]
    ln[0] = len(data)
    ty[0] = t
    if 0 < len(data) <= cap:
        ctypes.memmove(dst, data, len(data))
    return 0


# ----------------------------------------------------------------- trees --
@pytest.fixture(scope="module")
def tree(engine, tmp_path_factory):
    """The tree of tests/test_gpu_restore.py::test_restore_tree, stored, with
    every block of the backup by its ID as (DataType, data field, links)."""
    from hashbox_amd import formats as F
    tmp = tmp_path_factory.mktemp("many_tree")
    rng = np.random.default_rng(12)
    src = tmp / "src"
    (src / "a" / "b").mkdir(parents=True)
    big = bytes(rng.integers(0, 256, 5 * Mi // 2, dtype=np.uint8))
    mid = _text(70 * 1024, 8)
    ro = _text(3000, 9)
    (src / "a" / "big.bin").write_bytes(big)
    (src / "a" / "b" / "mid.txt").write_bytes(mid)
    (src / "empty").write_bytes(b"")
    os.symlink("a/b/mid.txt", src / "link")
    (src / "a" / "readonly.txt").write_bytes(ro)
    os.chmod(src / "a" / "readonly.txt", 0o444)
    os.utime(src / "a" / "readonly.txt", ns=(1_600_000_000 * 10**9, 1_200_000_003 * 10**9))
    os.chmod(src / "a" / "big.bin", 0o600)
    os.chmod(src / "a" / "b" / "mid.txt", 0o640)
    os.chmod(src / "a" / "b", 0o750)
    os.utime(src / "a" / "big.bin", ns=(1_600_000_000 * 10**9, 1_500_000_123 * 10**9 + 456))
    os.utime(src / "a" / "b" / "mid.txt", ns=(1_600_000_000 * 10**9, 1_400_000_001 * 10**9))
    os.utime(src / "empty", ns=(1_600_000_000 * 10**9, 1_300_000_002 * 10**9))
    t = F.store_tree(engine, src)
    raw_blocks = [(bid, dblk, links) for _p, (dblk, links, bid) in t.directories.items()]
    for path, r in t.files.items():
        data = open(path, "rb").read()
        ends = [int(x) for x in r.cut_ends]
        for a, b, cid in zip([0] + ends[:-1], ends, r.ids):
            raw_blocks.append((bytes(cid), data[a:b], []))
        if r.content_type == F.TYPE_FILE_CHAIN:
            chain_ids = [bytes(x) for x in r.ids]
            raw_blocks.append((r.content_id, F.serialize_chain_block(chain_ids), chain_ids))
    assert any(r.content_type == F.TYPE_FILE_CHAIN for r in t.files.values())
    server = {}
    for k, (bid, d, links) in enumerate(raw_blocks):
        assert block_id(d, links) == bytes(bid)  # the IDs are hashlib's
        server[bytes(bid)] = (RAW, d, links) if k % 5 == 4 else (ZLIB, zlib.compress(d, 6), links)
    return {"src": src, "t": t, "server": server, "big": big, "mid": mid, "ro": ro, "tmp": tmp}


def test_restore_tree_batched_and_diff_tree(engine, tree):
    from hashbox_amd import formats as F
    src, t, server = tree["src"], tree["t"], tree["server"]
    big, mid, ro = tree["big"], tree["mid"], tree["ro"]
    asked = []

    def read_block(bid):
        asked.append(bid)
        return server[bid]
    dest = tree["tmp"] / "dest"
    dest.mkdir()
    stats = F.restore_tree(engine, t.root, read_block, dest, window_bytes=64 * Mi, batch=True)
    got = dest / "src"
    assert stats == {"files": 4, "directories": 3, "bytes": len(big) + len(mid) + len(ro)}
    assert (got / "a" / "readonly.txt").read_bytes() == ro
    assert stat.S_IMODE(os.lstat(got / "a" / "readonly.txt").st_mode) == 0o444
    assert (got / "a" / "big.bin").read_bytes() == big
    assert (got / "a" / "b" / "mid.txt").read_bytes() == mid
    assert (got / "empty").read_bytes() == b"" and (got / "empty").is_file()
    assert os.readlink(got / "link") == "a/b/mid.txt"
    for rel in ("a/big.bin", "a/b/mid.txt", "a/readonly.txt", "empty", "a", "a/b"):
        s0, s1 = os.lstat(src / rel), os.lstat(got / rel)
        assert stat.S_IMODE(s0.st_mode) == stat.S_IMODE(s1.st_mode), rel
        if stat.S_ISREG(s0.st_mode):
            assert int(s0.st_mtime) == int(s1.st_mtime), rel
    assert set(asked) == set(server) and len(asked) == len(server)  # every block of the backup was read, once

    d = F.diff_tree(engine, t.root, read_block, dest, window_bytes=64 * Mi)
    assert d == {"files": 4, "directories": 3, "different": []}
    # one flipped byte (size and ModTime kept), one chmod, one deleted file: exactly those three
    p = got / "a" / "b" / "mid.txt"
    st = os.lstat(p)
    flipped = bytearray(mid)
    flipped[50_000] ^= 0x20
    p.write_bytes(bytes(flipped))
    os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns))
    os.chmod(got / "a" / "big.bin", 0o644)
    os.remove(got / "empty")
    d = F.diff_tree(engine, t.root, read_block, dest, window_bytes=64 * Mi)
    assert d["files"] == 3 and d["directories"] == 3
    diff = dict(d["different"])
    assert len(d["different"]) == 3 and set(diff) == {str(p), str(got / "a" / "big.bin"), str(got / "empty")}
    assert diff[str(p)] == "data is different at offset 50000"
    assert "permissions" in diff[str(got / "a" / "big.bin")] and "data" not in diff[str(got / "a" / "big.bin")]
    assert diff[str(got / "empty")] == "local path does not exist"
    # a file only the local side has
    (got / "a" / "extra").write_bytes(b"x")
    d = F.diff_tree(engine, t.root, read_block, dest, window_bytes=64 * Mi)
    assert (str(got / "a" / "extra"), "remote path does not exist") in d["different"] and len(d["different"]) == 4


def test_restore_tree_batched_names_the_bad_block(engine, tree):
    from hashbox_amd import HbxError, formats as F
    t, server = tree["t"], dict(tree["server"])
    victim = bytes(t.files[os.fsencode(tree["src"] / "a" / "big.bin")].ids[1])
    ty, data, links = server[victim]
    server[victim] = (ty, data[:len(data) // 2], links)
    dest = tree["tmp"] / "dest_bad"
    dest.mkdir()
    with pytest.raises(HbxError, match=victim.hex()):
        F.restore_tree(engine, t.root, lambda bid: server[bid], dest, window_bytes=64 * Mi, batch=True)
    # the good files of the same batch have been written
    assert (dest / "src" / "a" / "b" / "mid.txt").read_bytes() == tree["mid"]
    assert (dest / "src" / "a" / "readonly.txt").read_bytes() == tree["ro"]
