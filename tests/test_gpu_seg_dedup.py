"""Segments with an ID set (hbx_seg_submit_device_dd) and the disk-to-sender
stream (hbx_store_file_stream) on the GPU, against the oracle and the model of
tests/test_seg_stream_abi.py (never against the engine itself): a chunk is
fresh where its ID occurs for the first time in submit order, marked in the
segment that completes it, and every fresh chunk's zlib stream inflates to the
chunk's bytes.  Inputs are at most 50 MiB in 16 MiB segments.
"""
import ctypes
import zlib

import numpy as np
import pytest

from .test_seg_stream_abi import FLAGS, SEG, first_occurrence, input_bytes, per_segment, whole
from .test_segmented import Mi

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_IO, ERR_SINK = -1, -4, -8


def run_segments(e, data, arena_off, idset):
    """The segment loop of a device-side producer with a set: a ring of three
    arenas, each segment at byte `arena_off` of its arena.  Per-segment results."""
    import torch
    n = data.size
    arenas = [torch.zeros(arena_off + min(SEG, n) + 64, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    parts, k = [], 0
    with e.seg_open(n) as f:
        while not f.final_sent:
            off, ln = f.next(SEG)
            if k >= 3:
                parts += e.wait()
            a = arenas[k % 3]
            a[arena_off:arena_off + ln].copy_(torch.from_numpy(np.array(data[off:off + ln])))
            e.seg_submit_device([f], a.data_ptr(), [arena_off], [ln], seg_offs=[off], dedup=idset)
            k += 1
        while e.pending():
            parts += e.wait()
    return parts


def check_parts(parts, ref, counts, flags):
    assert [p.n_chunks for p in parts] == counts
    assert np.array_equal(np.concatenate([p.cut_ends for p in parts]), ref.cut_ends)
    assert np.array_equal(np.concatenate([p.ids for p in parts]), ref.ids)
    assert (parts[-1].content_type, parts[-1].content_id) == (ref.content_type, ref.content_id)
    assert all(p.fresh is not None and p.fresh.shape == (p.n_chunks,) for p in parts)
    assert np.concatenate([p.fresh for p in parts]).astype(int).tolist() == flags


# ------------------------------------------------ 1. flags per segment --
@pytest.mark.parametrize("name,arena_off", [(n, 0) for n in FLAGS] + [("zeros_32Mi", 48)])
def test_flags_per_segment(engine, oracle, name, arena_off):
    from hashbox_amd import IdSet
    data, ref = input_bytes(oracle, name), whole(oracle, name)
    with IdSet(engine, 64) as s:
        parts = run_segments(engine, data, arena_off, s)
        check_parts(parts, ref, per_segment(oracle, name), FLAGS[name])
        assert s.count == len({bytes(x) for x in ref.ids}) == sum(FLAGS[name])
        assert s.dropped == 0


# ------------------------------------------------------ 2. seeded set --
def test_seeded_set_and_a_second_pass(engine, oracle):
    from hashbox_amd import IdSet
    data, ref = input_bytes(oracle, "rep4"), whole(oracle, "rep4")
    seed = ref.ids[[1, 12]]
    want = first_occurrence(ref.ids, seen=seed)
    assert want[1] == 0 and want[12] == 0 and want != FLAGS["rep4"]
    assert [w for i, w in enumerate(want) if i not in (1, 12)] == [w for i, w in enumerate(FLAGS["rep4"])
                                                                   if i not in (1, 12)]
    with IdSet(engine, 64) as s:
        assert s.insert(seed).tolist() == [True, True]
        check_parts(run_segments(engine, data, 0, s), ref, per_segment(oracle, "rep4"), want)
        count = s.count
        assert count == 2 + sum(want)
        check_parts(run_segments(engine, data, 0, s), ref, per_segment(oracle, "rep4"), [0] * 16)
        assert s.count == count and s.dropped == 0


# ------------------------ 3. one order for segment and ordinary batches --
def test_segments_and_ordinary_batches_share_one_order(oracle):
    """Segment 0 of file B, then an ordinary batch with a whole copy of B (8 MiB
    chunks: far more MD5 launches than the segments behind it, which the
    hold-back keeps from marking first) and two small files, then B's other
    segments interleaved with file A's; all in flight at once."""
    import torch
    from hashbox_amd import Engine, IdSet
    da, ra = input_bytes(oracle, "random_40Mi+1"), whole(oracle, "random_40Mi+1")
    db, rb = input_bytes(oracle, "tiled_36Mi+777"), whole(oracle, "tiled_36Mi+777")
    small = [oracle.random_bytes(n, 90 + i) for i, n in enumerate([3 * Mi + 5, 200001])]
    small_refs = [oracle.store_file(x, fast=True) for x in small]
    lens = [db.size, da.size] + [x.size for x in small]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += (n + 255) // 256 * 256
    host = np.zeros(pos + 64, np.uint8)
    for o, x in zip(offs, [db, da] + small):
        host[o:o + x.size] = x
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    base = dev.data_ptr()
    with Engine(0, md5_slice=64, join_lag=2, k3_period=4) as e, IdSet(e, 256) as s:
        fb, fa = e.seg_open(db.size), e.seg_open(da.size)

        def sub(f):
            o, ln = f.next(SEG)
            e.seg_submit_device([f], base, [offs[0 if f is fb else 1] + o], [ln], seg_offs=[o], dedup=s)
            return f

        order = [sub(fb)]
        e.submit_device(base, np.array([offs[0], offs[2], offs[3]], np.uint64), [lens[0], lens[2], lens[3]], dedup=s)
        order.append(None)
        while not (fa.final_sent and fb.final_sent):
            for f in (fb, fa):
                if not f.final_sent:
                    order.append(sub(f))
        assert e.pending() == len(order) == 1 + 1 + 3 + 5
        ids, fresh, parts = [], [], {id(fa): [], id(fb): []}
        for f in order:
            res = e.wait()
            if f is None:
                for g, r in zip(res, [rb] + small_refs):
                    assert np.array_equal(g.cut_ends, r.cut_ends) and np.array_equal(g.ids, r.ids)
            else:
                assert len(res) == 1
                parts[id(f)].append(res[0])
            for g in res:
                ids.append(g.ids)
                fresh.append(g.fresh)
        assert e.pending() == 0
        fa.close()
        fb.close()
        for f, ref, name in ((fa, ra, "random_40Mi+1"), (fb, rb, "tiled_36Mi+777")):
            ps = parts[id(f)]
            assert [p.n_chunks for p in ps] == per_segment(oracle, name)
            assert np.array_equal(np.concatenate([p.ids for p in ps]), ref.ids)
            assert np.array_equal(np.concatenate([p.cut_ends for p in ps]), ref.cut_ends)
            assert (ps[-1].content_type, ps[-1].content_id) == (ref.content_type, ref.content_id)
        all_ids = np.concatenate(ids)
        want = first_occurrence(all_ids)
        assert np.concatenate(fresh).astype(int).tolist() == want
        # B's first two chunks are fresh in its segment 0, so the whole copy behind it finds them seen
        assert want[:2] == [1, 1] and want[2:8] == [0, 0, 0, 0, 1, 1]
        assert s.count == sum(want) and s.dropped == 0


def test_two_files_in_one_segment_batch_are_marked_in_segment_order(engine, oracle):
    """Two open files with the same bytes, their segments side by side in each
    batch: within a batch the first segment's chunks come first."""
    import torch
    from hashbox_amd import IdSet
    name = "tiled_36Mi+777"
    data, ref = input_bytes(oracle, name), whole(oracle, name)
    dev = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to("cuda:0")
    torch.cuda.synchronize()
    with IdSet(engine, 64) as s, engine.seg_open(data.size) as f1, engine.seg_open(data.size) as f2:
        while not f1.final_sent:
            o, ln = f1.next(SEG)
            engine.seg_submit_device([f1, f2], dev.data_ptr(), [o, o], [ln, ln], seg_offs=[o, o], dedup=s)
        ids, fresh, counts = [], [], []
        while engine.pending():
            a, b = engine.wait()
            assert np.array_equal(a.ids, b.ids) and np.array_equal(a.cut_ends, b.cut_ends)
            counts.append(a.n_chunks)
            ids += [a.ids, b.ids]
            fresh += [a.fresh, b.fresh]
        assert counts == per_segment(oracle, name)
        assert np.array_equal(np.concatenate(ids[0::2]), ref.ids)
        want = first_occurrence(np.concatenate(ids))
        assert np.concatenate(fresh).astype(int).tolist() == want
        assert not np.concatenate(fresh[1::2]).any()  # the second file's chunks were all seen in the first's
        assert np.concatenate(fresh[0::2]).astype(int).tolist() == FLAGS[name]
        assert s.count == sum(FLAGS[name])


# ------------------------------------------- 4. from disk, the sender path --
@pytest.fixture(scope="module")
def on_disk(oracle, tmp_path_factory):
    """name -> path of the input written once."""
    d = tmp_path_factory.mktemp("seg_stream")
    paths = {}

    def get(name):
        if name not in paths:
            paths[name] = d / (name.replace("+", "_") + ".bin")
            input_bytes(oracle, name).tofile(paths[name])
        return paths[name]
    return get


def check_streams(data, start, chunks, flags):
    """Every chunk flagged fresh has a stream that inflates to its bytes; every
    other chunk has an empty one.  Returns where the next chunk starts."""
    assert len(chunks.zstreams) == chunks.n_chunks == len(flags)
    for end, z, fr in zip(chunks.cut_ends.tolist(), chunks.zstreams, flags):
        if fr:
            assert zlib.decompress(z.tobytes()) == data[start:end].tobytes()
        else:
            assert z.size == 0
        start = end
    return start


class Sender:
    """An on_segment callback that checks each segment as a sender would use it."""

    def __init__(self, data, compress=True, flags=None):
        self.data, self.compress, self.flags = data, compress, flags
        self.calls, self.next_chunk, self.start = [], 0, 0
        self.cuts, self.ids, self.fresh, self.last = [], [], [], None

    def __call__(self, seg):
        ch = seg.chunks
        assert self.last is None or not self.last.final, "a call after the final segment"
        assert seg.first_chunk == self.next_chunk
        self.next_chunk += ch.n_chunks
        self.calls.append(ch.n_chunks)
        fl = ch.fresh.astype(int).tolist() if ch.fresh is not None else [1] * ch.n_chunks
        if self.compress:
            self.start = check_streams(self.data, self.start, ch, fl)
        else:
            assert not ch.zstreams
        self.cuts.append(ch.cut_ends.copy())
        self.ids.append(ch.ids.copy())
        self.fresh += fl
        self.last = seg
        if not seg.final:
            assert ch.content_type == 0 and ch.content_id == b""

    def check(self, ref, counts, flags):
        assert self.calls == counts
        assert self.last.final
        assert (self.last.chunks.content_type, self.last.chunks.content_id) == (ref.content_type, ref.content_id)
        assert np.array_equal(np.concatenate(self.cuts), ref.cut_ends)
        assert np.array_equal(np.concatenate(self.ids), ref.ids)
        assert self.fresh == flags


def same_file(got, ref):
    assert np.array_equal(got.cut_ends, ref.cut_ends) and np.array_equal(got.ids, ref.ids)
    assert (got.content_type, got.content_id) == (ref.content_type, ref.content_id)


@pytest.mark.parametrize("name", ["rep4", "tiled_36Mi+777"])
def test_stream_from_disk_with_set_and_compression(engine, oracle, on_disk, name):
    from hashbox_amd import IdSet
    data, ref, counts = input_bytes(oracle, name), whole(oracle, name), per_segment(oracle, name)
    with IdSet(engine, 64) as s:
        cb = Sender(data)
        got = engine.store_file(on_disk(name), segment_bytes=SEG, compress=True, dedup=s, on_segment=cb)
        cb.check(ref, counts, FLAGS[name])
        same_file(got, ref)
        assert got.fresh.astype(int).tolist() == FLAGS[name] and got.zstreams is None
        assert s.count == sum(FLAGS[name])
        again = Sender(data)  # the same file on the same set: nothing is fresh, nothing is compressed
        got = engine.store_file(on_disk(name), segment_bytes=SEG, compress=True, dedup=s, on_segment=again)
        again.check(ref, counts, [0] * ref.n_chunks)
        assert not got.fresh.any() and s.count == sum(FLAGS[name])
    assert engine.pending() == 0


def test_stream_compression_without_a_set(engine, oracle, on_disk):
    name = "tiled_36Mi+777"
    data, ref = input_bytes(oracle, name), whole(oracle, name)
    cb = Sender(data)
    got = engine.store_file(on_disk(name), segment_bytes=SEG, compress=True, on_segment=cb)
    cb.check(ref, per_segment(oracle, name), [1] * ref.n_chunks)  # (no flags: every chunk has a stream)
    assert cb.last.chunks.fresh is None and got.fresh is None
    same_file(got, ref)


def test_stream_set_without_compression(engine, oracle, on_disk):
    from hashbox_amd import IdSet
    name = "tiled_36Mi+777"
    data, ref = input_bytes(oracle, name), whole(oracle, name)
    with IdSet(engine, 64) as s:
        cb = Sender(data, compress=False)
        got = engine.store_file(on_disk(name), segment_bytes=SEG, dedup=s, on_segment=cb)
        cb.check(ref, per_segment(oracle, name), FLAGS[name])
        same_file(got, ref)
        assert got.fresh.astype(int).tolist() == FLAGS[name] and not got.zstreams


def test_stream_without_a_callback_returns_the_whole_file(engine, oracle, on_disk):
    from hashbox_amd import IdSet
    data, ref = input_bytes(oracle, "rep4"), whole(oracle, "rep4")
    with IdSet(engine, 64) as s:
        got = engine.store_file(on_disk("rep4"), segment_bytes=SEG, compress=True, dedup=s)
        same_file(got, ref)
        assert got.fresh.astype(int).tolist() == FLAGS["rep4"]
        assert check_streams(data, 0, got, FLAGS["rep4"]) == data.size


def test_stream_with_three_reader_threads(engine, oracle, on_disk):
    from hashbox_amd import IdSet
    name = "tiled_36Mi+777"
    data, ref = input_bytes(oracle, name), whole(oracle, name)
    with IdSet(engine, 64) as s:
        cb = Sender(data)
        same_file(engine.store_file(on_disk(name), segment_bytes=SEG, io_threads=3, compress=True, dedup=s,
                                    on_segment=cb), ref)
        cb.check(ref, per_segment(oracle, name), FLAGS[name])


def test_stream_empty_and_one_chunk_files(engine, oracle, tmp_path):
    from hashbox_amd import IdSet
    empty, one = tmp_path / "empty.bin", tmp_path / "one.bin"
    empty.write_bytes(b"")
    data = oracle.random_bytes(64 * 1024, 23)
    data.tofile(one)
    with IdSet(engine, 64) as s:
        segs = []
        got = engine.store_file(empty, segment_bytes=SEG, compress=True, dedup=s,
                                on_segment=lambda seg: segs.append((seg.first_chunk, seg.chunks.n_chunks, seg.final,
                                                                    seg.chunks.content_type)))
        assert segs == [(0, 0, True, 0)]
        assert got.n_chunks == 0 and got.content_type == 0 and got.content_id == b"" and s.count == 0
        ref = oracle.store_file(data)
        cb = Sender(data)
        got = engine.store_file(one, segment_bytes=SEG, compress=True, dedup=s, on_segment=cb)
        cb.check(ref, [1], [1])
        same_file(got, ref)
        assert got.content_type == 2 and got.content_id == ref.ids[0].tobytes() and s.count == 1


# ---------------------- 5. failures leave the set and the context as they were --
def test_exception_in_the_callback_rolls_the_set_back(engine, oracle, on_disk):
    from hashbox_amd import IdSet
    name = "rep4"
    data, ref = input_bytes(oracle, name), whole(oracle, name)
    seed = oracle.random_bytes(48, 7).reshape(3, 16)

    class Boom(Exception):
        pass

    seen = []

    def cb(seg):
        seen.append(seg.first_chunk)
        if len(seen) == 3:  # segment 2
            raise Boom("sender lost its connection")

    with IdSet(engine, 64) as s:
        s.insert(seed)
        with pytest.raises(Boom):
            engine.store_file(on_disk(name), segment_bytes=SEG, compress=True, dedup=s, on_segment=cb)
        assert len(seen) == 3  # no segment reached the callback after the failure
        assert s.count == 3 and engine.pending() == 0
        ok = Sender(data)
        same_file(engine.store_file(on_disk(name), segment_bytes=SEG, compress=True, dedup=s, on_segment=ok), ref)
        ok.check(ref, per_segment(oracle, name), FLAGS[name])
        assert s.count == 3 + sum(FLAGS[name])


def test_short_read_and_failing_sink_through_the_raw_binding(engine, oracle, on_disk):
    from hashbox_amd import IdSet, _lib
    name = "rep4"
    data = input_bytes(oracle, name)
    path = str(on_disk(name)).encode()
    calls = []

    def count(_user, seg):
        calls.append(int(seg.contents.n_chunks))
        return 0

    with IdSet(engine, 64) as s:
        s.insert(oracle.random_bytes(32, 8).reshape(2, 16))
        L, summ = engine._L, _lib.FileSummary()
        sink = _lib.SEG_SINK(count)
        rc = L.hbx_store_file_stream(engine._ctx, path, data.size + 4 * Mi, SEG, 4, _lib.STREAM_COMPRESS, s._h,
                                     ctypes.cast(sink, ctypes.c_void_p), None, ctypes.byref(summ))
        assert rc == ERR_IO
        assert engine.pending() == 0 and s.count == 2
        bad = _lib.SEG_SINK(lambda _user, seg: 1)
        rc = L.hbx_store_file_stream(engine._ctx, path, data.size, SEG, 4, _lib.STREAM_COMPRESS, s._h,
                                     ctypes.cast(bad, ctypes.c_void_p), None, ctypes.byref(summ))
        assert rc == ERR_SINK
        assert b"sink" in L.hbx_last_error(engine._ctx)
        assert engine.pending() == 0 and s.count == 2
        del calls[:]
        rc = L.hbx_store_file_stream(engine._ctx, path, data.size, SEG, 4, 0, s._h,
                                     ctypes.cast(sink, ctypes.c_void_p), None, ctypes.byref(summ))
        assert rc == 0 and calls == per_segment(oracle, name) and summ.n_chunks == 16 and summ.content_type == 3
        assert s.count == 2 + sum(FLAGS[name])


def test_a_full_set_keeps_every_chunk_fresh(engine, oracle, on_disk):
    from hashbox_amd import IdSet
    name = "random_40Mi+1"
    data, ref = input_bytes(oracle, name), whole(oracle, name)
    with IdSet(engine, 2) as s:
        cb = Sender(data)
        got = engine.store_file(on_disk(name), segment_bytes=SEG, compress=True, dedup=s, on_segment=cb)
        cb.check(ref, per_segment(oracle, name), [1] * 13)  # (and every stream inflated to its chunk)
        same_file(got, ref)
        assert got.fresh.all() and s.count == 2 and s.dropped == 11


# -------------------------------------------------------------- 6. refusals --
def test_refusals(oracle, on_disk):
    import torch
    from hashbox_amd import Engine, HbxError, IdSet, _lib
    dev = torch.zeros(32 * Mi + 64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = dev.data_ptr()
    with Engine(0) as e, Engine(0) as other:
        s, foreign = IdSet(e, 64), IdSet(other, 64)
        f = e.seg_open(32 * Mi)
        one = (ctypes.c_uint64 * 1)(0)
        ln = (ctypes.c_uint64 * 1)(SEG)
        cap = (ctypes.c_uint64 * 1)(SEG // 65536 + 1)
        hs = (ctypes.c_void_p * 1)(f._h)
        cuts = np.zeros(cap[0], np.uint64)
        ids = np.zeros((cap[0], 16), np.uint8)
        rc = e._L.hbx_seg_submit_device_dd(e._ctx, 1, hs, ctypes.c_void_p(p), one, ln, cuts.ctypes.data,
                                           ids.ctypes.data, one, cap, None, s._h, None)  # a set, no flags array
        assert rc == ERR_ARG and e.pending() == 0
        with pytest.raises(HbxError, match="HBX_ERR_ARG"):  # a set of another engine
            e.seg_submit_device([f], p, [0], [SEG], dedup=foreign)
        with pytest.raises(HbxError, match="HBX_ERR_ARG"):
            e.store_file(on_disk("zeros_32Mi"), segment_bytes=SEG, dedup=foreign)
        with pytest.raises(ValueError):  # the new arguments need segments
            e.store_file(on_disk("zeros_32Mi"), dedup=s)
        sink = _lib.SEG_SINK(lambda _user, seg: 0)
        path = str(on_disk("zeros_32Mi")).encode()
        for seg_bytes, flags, snk in ((SEG - 16, 0, sink), (SEG + 8, 0, sink), (SEG, _lib.STREAM_COMPRESS, None),
                                      (SEG, 2, sink)):
            rc = e._L.hbx_store_file_stream(e._ctx, path, 32 * Mi, seg_bytes, 4, flags, s._h,
                                            ctypes.cast(snk, ctypes.c_void_p) if snk else None, None, None)
            assert rc == ERR_ARG
        assert e.pending() == 0 and f.end == 0 and s.count == 0
        e.seg_submit_device([f], p, [0], [SEG], seg_offs=[0], dedup=s)
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):  # a segment batch with the set is pending
            s.close()
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):  # batches are pending
            e.store_file(on_disk("zeros_32Mi"), segment_bytes=SEG, dedup=s)
        assert e.pending() == 1
        (part,) = e.wait()
        assert part.n_chunks == 2 and part.fresh.tolist() == [True, False]
        f.close()  # abandoned before its final segment: what it inserted stays in the set
        assert e.pending() == 0 and s.count == 1
        s.close()
        foreign.close()
