"""Files streamed through the engine in overlapping segments (hbx_seg_*,
hbx_store_file_seg) against oracle.store_file over the whole file: the cases
of tests/test_segmented.py (whose per-segment chunk counts come from the
oracle), odd arena offsets, segments of several files and ordinary batches
interleaved in one FIFO, the refusals, and the disk path.
"""
import numpy as np
import pytest

from .test_segmented import CASES, MAX, MIN, Mi, make_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def whole(oracle):
    """(input bytes, oracle.store_file of the whole file) per case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            kind, n, _, _, _ = CASES[name]
            data = make_input(oracle, kind, n)
            data.flags.writeable = False
            cache[name] = (data, oracle.store_file(data))
        return cache[name]
    return get


def same(got, ref):
    assert np.array_equal(got.cut_ends, ref.cut_ends)
    assert np.array_equal(got.ids, ref.ids)
    assert got.content_type == ref.content_type
    assert got.content_id == ref.content_id


def join(parts):
    """One file's per-segment results as (cut ends, ids, final part)."""
    return (np.concatenate([p.cut_ends for p in parts]), np.concatenate([p.ids for p in parts]), parts[-1])


@pytest.mark.parametrize("name", list(CASES))
def test_cases_match_oracle_and_whole_file_engine(engine, whole, name):
    _, _, seg_bytes, chunks, per_seg = CASES[name]
    data, ref = whole(name)
    assert ref.n_chunks == chunks
    got, counts = engine.chunk_hash_segmented(data, seg_bytes, return_segments=True)
    same(got, ref)
    assert counts == per_seg
    same(engine.chunk_hash(data), ref)


def run_on_torch_arenas(e, data, seg_bytes, arena_off):
    """The segment loop a device-side producer runs: a ring of three arenas,
    each segment at byte `arena_off` of its arena.  Returns the per-segment
    results."""
    import torch
    n = data.size
    arenas = [torch.zeros(arena_off + min(seg_bytes, n) + 64, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    parts, k = [], 0
    with e.seg_open(n) as f:
        while not f.final_sent:
            off, ln = f.next(seg_bytes)
            if k >= 3:
                parts += e.wait()
            a = arenas[k % 3]
            a[arena_off:arena_off + ln].copy_(torch.from_numpy(data[off:off + ln]))
            e.seg_submit_device([f], a.data_ptr(), [arena_off], [ln], seg_offs=[off])
            k += 1
        while e.pending():
            parts += e.wait()
    return parts


def test_arena_offsets_of_16_but_not_256(engine, whole):
    _, _, seg_bytes, _, per_seg = CASES["random_40Mi+1"]
    data, ref = whole("random_40Mi+1")
    parts = run_on_torch_arenas(engine, np.array(data), seg_bytes, 48)
    cuts, ids, last = join(parts)
    assert np.array_equal(cuts, ref.cut_ends) and np.array_equal(ids, ref.ids)
    assert [p.n_chunks for p in parts] == per_seg
    # a non-final segment's summary is empty; the final one carries the file's
    assert [p.content_type for p in parts[:-1]] == [0] * (len(parts) - 1)
    assert all(p.content_id == b"" for p in parts[:-1])
    assert (last.content_type, last.content_id) == (ref.content_type, ref.content_id) and ref.content_type == 3


def test_one_chunk_file_is_file_data(engine, oracle):
    data = oracle.random_bytes(MIN, 21)
    ref = oracle.store_file(data)
    got, counts = engine.chunk_hash_segmented(data, 16 * Mi, return_segments=True)
    same(got, ref)
    assert counts == [1] and got.content_type == 2 and got.content_id == got.ids[0].tobytes()


def test_interleaved_files_and_batches_in_one_fifo(oracle, whole):
    """Two open files and an ordinary batch, all in flight at once at join
    lag 2, K3 period 4 and a 64-block slice (chains span many launches, and a
    file's next K2 is enqueued long before its previous segment is
    collected), collected by wait in submit order."""
    import torch
    from hashbox_amd import Engine
    (da, ra), (db, rb) = whole("random_40Mi+1"), whole("tiled_36Mi+777")
    seg = 16 * Mi
    small = [oracle.random_bytes(n, 70 + i) for i, n in enumerate([3 * Mi + 5, 200001, 0, 9 * Mi])]
    small_refs = [oracle.store_file(x, fast=True) for x in small]
    # one device buffer: file A | file B | the small files, each 256-aligned;
    # a segment is read in place at its file offset (a multiple of 16)
    lens = [da.size, db.size] + [x.size for x in small]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += (n + 255) // 256 * 256
    host = np.zeros(pos + 64, np.uint8)
    for o, x in zip(offs, [da, db] + small):
        host[o:o + x.size] = x
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    base = dev.data_ptr()
    with Engine(0, md5_slice=64, join_lag=2, k3_period=4) as e:
        fa, fb = e.seg_open(da.size), e.seg_open(db.size)

        def sub(files):
            nxt = [f.next(seg) for f in files]
            e.seg_submit_device(files, base, [offs[0 if f is fa else 1] + o for f, (o, _) in zip(files, nxt)],
                                [ln for _, ln in nxt], seg_offs=[o for o, _ in nxt])
            return files

        order = [sub([fa, fb]), sub([fa])]
        e.submit_device(base, np.array(offs[2:], np.uint64), lens[2:])
        order.append(None)
        order.append(sub([fb]))
        while not (fa.final_sent and fb.final_sent):  # alternate until both files are through
            for f in (fa, fb):
                if not f.final_sent:
                    order.append(sub([f]))
        assert e.pending() == len(order) == 1 + 4 + 3 + 1  # A has 5 segments, B 4, one shared batch
        parts = {id(fa): [], id(fb): []}
        for files in order:
            res = e.wait()
            if files is None:
                for g, r in zip(res, small_refs):
                    assert np.array_equal(g.cut_ends, r.cut_ends) and np.array_equal(g.ids, r.ids)
                    assert (g.content_type, g.content_id) == (r.content_type, r.content_id)
                continue
            assert len(res) == len(files)
            for f, p in zip(files, res):
                parts[id(f)].append(p)
        assert e.pending() == 0
        fa.close()
        fb.close()
    for f, ref, name in ((fa, ra, "random_40Mi+1"), (fb, rb, "tiled_36Mi+777")):
        cuts, ids, last = join(parts[id(f)])
        assert np.array_equal(cuts, ref.cut_ends) and np.array_equal(ids, ref.ids)
        assert [p.n_chunks for p in parts[id(f)]] == CASES[name][4]
        assert (last.content_type, last.content_id) == (ref.content_type, ref.content_id)


def test_refusals(whole):
    import torch
    from hashbox_amd import Engine, HbxError
    data, ref = whole("zeros_32Mi")
    dev = torch.zeros(32 * Mi + 64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = dev.data_ptr()
    with Engine(0) as e:
        f = e.seg_open(32 * Mi)
        with pytest.raises(ValueError):  # the first segment starts at 0
            e.seg_submit_device([f], p, [16], [16 * Mi], seg_offs=[16])
        for bad in (16 * Mi - 16,   # a non-final segment below HBX_SEG_MIN_BYTES
                    16 * Mi + 8,    # non-final, not a multiple of HBX_ARENA_ALIGN
                    32 * Mi + 16):  # longer than the file
            with pytest.raises(HbxError):
                e.seg_submit_device([f], p, [0], [bad])
        with pytest.raises(HbxError):  # two segments of one file in a batch
            e.seg_submit_device([f, f], p, [0, 8 * Mi], [16 * Mi, 16 * Mi])
        assert e.pending() == 0 and f.end == 0
        e.seg_submit_device([f], p, [0], [16 * Mi], seg_offs=[0])
        with pytest.raises(HbxError):  # a segment is pending
            f.close()
        with pytest.raises(ValueError):  # the next segment starts at 8 MiB
            e.seg_submit_device([f], p, [16 * Mi], [16 * Mi], seg_offs=[16 * Mi])
        e.seg_submit_device([f], p, [8 * Mi], [16 * Mi], seg_offs=[8 * Mi])
        e.seg_submit_device([f], p, [16 * Mi], [16 * Mi], seg_offs=[16 * Mi])
        assert f.final_sent and e.pending() == 3
        with pytest.raises(HbxError):  # after the final segment
            e.seg_submit_device([f], p, [16 * Mi], [16 * Mi])
        assert e.pending() == 3
        parts = e.wait() + e.wait() + e.wait()
        f.close()
        cuts, ids, last = join(parts)
        assert np.array_equal(cuts, ref.cut_ends) and np.array_equal(ids, ref.ids)
        assert (last.content_type, last.content_id) == (ref.content_type, ref.content_id)


def test_abandoned_file_leaves_the_context_usable(engine, oracle, whole):
    import torch
    dev = torch.zeros(16 * Mi + 64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    f = engine.seg_open(64 * Mi)
    engine.seg_submit_device([f], dev.data_ptr(), [0], [16 * Mi])
    (part,) = engine.wait()
    assert part.n_chunks == 2 and part.content_type == 0
    f.close()  # before the final segment: the file is abandoned
    data, ref = whole("random_40Mi+1")
    same(engine.chunk_hash_segmented(data, 16 * Mi), ref)
    small = oracle.random_bytes(3 * Mi + 1, 31)
    same(engine.chunk_hash(small), oracle.store_file(small))


def test_store_file_segmented_from_disk(engine, whole, tmp_path):
    data, ref = whole("random_40Mi+1")
    path = tmp_path / "big.bin"
    data.tofile(path)
    same(engine.store_file(path, segment_bytes=16 * Mi), ref)
    same(engine.store_file(path, segment_bytes=16 * Mi, io_threads=3), ref)
    same(engine.store_file(path), ref)


def test_store_file_segmented_short_file_is_io_error(engine, tmp_path):
    import ctypes
    from hashbox_amd import _lib
    path = tmp_path / "short.bin"
    path.write_bytes(bytes(MAX))
    s = _lib.FileSummary()
    cap = 1024
    cuts = np.zeros(cap, np.uint64)
    ids = np.zeros((cap, 16), np.uint8)
    rc = engine._L.hbx_store_file_seg(engine._ctx, str(path).encode(), 20 * Mi, 16 * Mi, 4, cuts.ctypes.data,
                                      ids.ctypes.data, cap, ctypes.byref(s))
    assert rc == -4  # HBX_ERR_IO
    assert engine.pending() == 0


def test_store_file_segmented_empty_file(engine, tmp_path):
    path = tmp_path / "empty.bin"
    path.write_bytes(b"")
    got = engine.store_file(path, segment_bytes=16 * Mi)
    assert got.n_chunks == 0 and got.content_type == 0 and got.content_id == b""
