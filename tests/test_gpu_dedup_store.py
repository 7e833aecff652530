"""GPU: the pipeline with a block-ID set (hbx_store_paths_dd,
hbx_submit_device_dd): exactly one chunk per distinct ID is fresh, the first in
submit order, however the files fall into batches; only fresh chunks are
compressed; a failed call leaves the set as it was.  Flags are compared for
equality with the dict model below over the IDs in file order; ids and cut
ends with the run without a set."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20


def _model(model: dict, files) -> list:
    """Per file, fresh[q] = the chunk's ID is not in the model yet (then it is)."""
    out = []
    for f in files:
        flags = np.zeros(f.ids.shape[0], bool)
        for q, row in enumerate(f.ids):
            k = row.tobytes()
            if k not in model:
                model[k] = len(model)
                flags[q] = True
        out.append(flags)
    return out


def _same_chunks(got, plain):
    assert len(got) == len(plain)
    for g, p in zip(got, plain):
        assert np.array_equal(g.cut_ends, p.cut_ends) and np.array_equal(g.ids, p.ids)
        assert g.content_id == p.content_id and g.content_type == p.content_type


def _flags_equal(got, want):
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.fresh is not None and g.fresh.dtype == bool
        assert np.array_equal(g.fresh, w), f


@pytest.fixture(scope="module")
def corpus(engine, tmp_path_factory):
    """24 random files of 256 KiB to 3 MiB: files 20-22 are copies of files 2,
    9 and 15, files 18 and 19 share their first MiB with files 4 and 11."""
    g = np.random.Generator(np.random.PCG64(2024))
    sizes = g.integers(256 * KIB, 3 * MIB + 1, 24)
    sizes[4] = sizes[11] = 2 * MIB + 12345  # long enough to have a 1 MiB prefix
    sizes[18], sizes[19] = 1 * MIB + 300 * KIB + 1, 2 * MIB + 777
    datas = [g.integers(0, 256, int(n), dtype=np.uint8) for n in sizes]
    for dst, src in ((20, 2), (21, 9), (22, 15)):
        datas[dst] = datas[src].copy()
    for dst, src in ((18, 4), (19, 11)):
        datas[dst][:MIB] = datas[src][:MIB]
    d = tmp_path_factory.mktemp("dedup")
    paths = []
    for i, x in enumerate(datas):
        p = d / f"f{i:02d}.bin"
        x.tofile(p)
        paths.append(str(p))
    plain = engine.store_paths(paths, io_threads=4)
    assert all(f.fresh is None for f in plain)
    want = _model({}, plain)
    # both classes occur, and every copied file has a chunk that is not fresh
    assert any(w.any() for w in want)
    for dst in (20, 21, 22):
        assert plain[dst].n_chunks >= 1 and not want[dst].any()
    return {"paths": paths, "datas": datas, "plain": plain, "want": want, "copies": (20, 21, 22)}


@pytest.mark.parametrize("batch_bytes", [1 << 30, 4 * MIB])
def test_store_paths_flags(engine, corpus, batch_bytes):
    """One batch, and batches of 4 MiB: the same flags."""
    from hashbox_amd import IdSet
    with IdSet(engine, 4096) as s:
        got = engine.store_paths(corpus["paths"], io_threads=4, batch_bytes=batch_bytes, dedup=s)
        _same_chunks(got, corpus["plain"])
        _flags_equal(got, corpus["want"])
        distinct = {r.tobytes() for f in got for r in f.ids}
        assert s.count == len(distinct) == sum(int(w.sum()) for w in corpus["want"])
        assert {r.tobytes() for r in s.export()} == distinct
        # a second pass over the same files: nothing is fresh
        again = engine.store_paths(corpus["paths"], io_threads=4, batch_bytes=batch_bytes, dedup=s)
        _same_chunks(again, corpus["plain"])
        assert not any(f.fresh.any() for f in again) and s.count == len(distinct)


def test_store_paths_compress_only_fresh(engine, corpus):
    from hashbox_amd import IdSet
    batches = []
    base = engine.store_paths(corpus["paths"], io_threads=4, compress=True)
    with IdSet(engine, 4096) as s:
        got = engine.store_paths(corpus["paths"], io_threads=4, batch_bytes=4 * MIB, compress=True, dedup=s,
                                 on_batch=lambda first, count: batches.append((first, count)))
    assert len(batches) > 1 and sum(c for _, c in batches) == len(got)  # several batches
    _same_chunks(got, corpus["plain"])
    _flags_equal(got, corpus["want"])
    n_fresh = n_seen = 0
    for f, x in zip(got, corpus["datas"]):
        starts, ends = f.chunk_bounds()
        assert len(f.zstreams) == f.n_chunks
        for q in range(f.n_chunks):
            if f.fresh[q]:
                assert zlib.decompress(f.zstreams[q].tobytes()) == x[int(starts[q]):int(ends[q])].tobytes()
                n_fresh += 1
            else:
                assert f.zstreams[q].size == 0
                n_seen += 1
    assert n_fresh and n_seen
    total = sum(z.size for f in got for z in f.zstreams)
    assert total < sum(z.size for f in base for z in f.zstreams)
    for dst in corpus["copies"]:
        assert all(z.size == 0 for z in got[dst].zstreams)


def test_seeded_set(engine, corpus):
    """A set seeded with one file's IDs (a previous backup's list): none of
    that file's chunks is fresh, whichever batch it falls into."""
    from hashbox_amd import IdSet
    seed = 7
    with IdSet(engine, 4096) as s:
        assert s.insert(corpus["plain"][seed].ids).all()
        model = {r.tobytes(): i for i, r in enumerate(corpus["plain"][seed].ids)}
        want = _model(model, corpus["plain"])
        assert not want[seed].any()
        got = engine.store_paths(corpus["paths"], io_threads=4, batch_bytes=4 * MIB, dedup=s)
        _flags_equal(got, want)
        assert not got[seed].fresh.any() and s.count == len(model)


def test_failed_call_rolls_the_set_back(engine, corpus, tmp_path):
    from hashbox_amd import HbxError, IdSet
    with IdSet(engine, 4096) as s:
        s.insert(corpus["plain"][0].ids)
        before = s.count
        kept = s.export().copy()
        paths = corpus["paths"][1:12] + [str(tmp_path / "gone.bin")]
        sizes = [x.size for x in corpus["datas"][1:12]] + [4096]
        with pytest.raises(HbxError, match="gone.bin"):
            engine.store_paths(paths, sizes=sizes, io_threads=4, batch_bytes=4 * MIB, dedup=s)
        assert s.count == before and np.array_equal(s.export(), kept)
        assert not s.contains(corpus["plain"][1].ids).any()
        # and both work afterwards
        got = engine.store_paths(corpus["paths"], io_threads=4, batch_bytes=4 * MIB, dedup=s)
        model = {r.tobytes(): i for i, r in enumerate(corpus["plain"][0].ids)}
        _flags_equal(got, _model(model, corpus["plain"]))


def test_submit_device_in_submit_order(corpus):
    """Three batches in flight with a 64 KiB MD5 slice.  Batch 0 holds a 3 MiB
    file (48 launches), batch 1 only files under 128 KiB (2 launches: hashed
    long before batch 0) of which one repeats a file of batch 0, batch 2
    repeats batch 0 with one file changed.  The first occurrence in SUBMIT
    order is the fresh one.  A verify batch in between never touches the set."""
    import torch
    from hashbox_amd import Engine, IdSet, pack_arena_layout
    g = np.random.Generator(np.random.PCG64(99))
    big = g.integers(0, 256, 3 * MIB, dtype=np.uint8)
    mid = corpus["datas"][0]
    small, small2 = (g.integers(0, 256, n, dtype=np.uint8) for n in (100 * KIB, 90 * KIB))
    changed = small.copy()
    changed[50_000] ^= 1
    batches = [[big, mid, small], [small, small2], [big, mid, changed]]
    dev = torch.device("cuda", 0)

    def resident(files):
        lens = [int(x.size) for x in files]
        offs, total = pack_arena_layout(lens)
        host = np.zeros(total, np.uint8)
        for o, x in zip(offs, files):
            host[int(o):int(o) + x.size] = x
        return torch.from_numpy(host).to(dev), offs, lens

    arenas = [resident(b) for b in batches]
    torch.cuda.synchronize(dev)
    with Engine(0, md5_slice=1024) as e:
        plain = [e.chunk_hash_batch(b) for b in batches]
        with IdSet(e, 1000) as s:
            for i, (a, offs, lens) in enumerate(arenas):
                e.submit_device(a.data_ptr(), offs, lens, dedup=s)
                if i == 1:  # blocks that are no chunk of any file: their IDs must not reach the set
                    e.verify_submit_device(arenas[0][0].data_ptr(), [0, 4096], [100_000, 50_000])
            assert e.pending() == 4
            got = [e.wait() for _ in range(4)]
            verify_ids = got.pop(2)[0]
            model = {}
            for gb, pb in zip(got, plain):
                _same_chunks(gb, pb)
                _flags_equal(gb, _model(model, pb))
            assert got[0][2].fresh.all() and not got[1][0].fresh.any() and got[1][1].fresh.all()
            assert not got[2][0].fresh.any() and not got[2][1].fresh.any() and got[2][2].fresh.any()
            assert s.count == len(model)
            assert {r.tobytes() for r in s.export()} == set(model)
            assert not s.contains(verify_ids).any()
            # submit order is also the export order: batch 0's IDs come first
            n0 = sum(f.n_chunks for f in got[0])
            assert {r.tobytes() for r in s.export()[:n0]} == {r.tobytes() for f in got[0] for r in f.ids}
