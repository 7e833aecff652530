"""The crafted cut-rule inputs (tests/cut_craft.py) through K1 + K2, bit-exact
against the oracle: maxima at every edge of the candidate range, of a slice,
of K1's runs, iterations and tiles; edge-slice summaries that overstate the
in-range maximum; exact ties between and inside K2's three sources.
tests/test_cut_craft.py shows on the CPU that the cases have those
properties.  A failure names the case, the chunk and where the reference's
answer lies.
"""
import numpy as np
import pytest

from . import cut_craft as cc

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cc.CASES]


@pytest.fixture(scope="module")
def refs(oracle):
    """oracle.store_file of every case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle.store_file(cc.build(name), fast=True)
        return cache[name]
    return get


def differences(oracle, name, got, ref):
    """[] if `got` is `ref` bit for bit, else one line per wrong chunk with
    the reference's classification of it."""
    if (np.array_equal(got.cut_ends, ref.cut_ends) and np.array_equal(got.ids, ref.ids)
            and got.content_type == ref.content_type and got.content_id == ref.content_id):
        return []
    x = cc.build(name)
    D = oracle.digest_all(x)
    out = []
    starts = [0] + [int(c) for c in ref.cut_ends[:-1]]
    for i, (s, want) in enumerate(zip(starts, ref.cut_ends)):
        have = int(got.cut_ends[i]) if i < got.n_chunks else None
        same_id = have == int(want) and np.array_equal(got.ids[i], ref.ids[i])
        if not same_id:
            r = cc.Range(D, s, x.size)
            where = r.src if r.none else "%s, slice %d position %d, %d tied, max %#010x" % (
                r.src, r.slice_of(r.win) - r.ja, r.pos_of(r.win), r.tied.size, r.max)
            out.append("%s chunk %d (s=%d): cut %s, reference %d (%s)%s" % (
                name, i, s, have, int(want), where, "" if have != int(want) else ", block id differs"))
            if have != int(want):
                break  # the chain after a wrong cut is another file's
    if not out:
        out.append("%s: %d chunks for %d, or the content id differs" % (name, got.n_chunks, ref.n_chunks))
    return out


def check_all(oracle, refs, results):
    bad = [line for name, got in zip(NAMES, results) for line in differences(oracle, name, got, refs(name))]
    assert not bad, "\n".join(bad)


def test_all_cases_in_one_batch(engine, oracle, refs):
    check_all(oracle, refs, engine.chunk_hash_batch([cc.build(n) for n in NAMES]))


@pytest.mark.parametrize("name", NAMES)
def test_each_case_alone(engine, oracle, refs, name):
    bad = differences(oracle, name, engine.chunk_hash(cc.build(name)), refs(name))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("swz", ["0", "1"])
@pytest.mark.parametrize("tile_iters", [1, 3, 16])
def test_batch_at_tile_sizes(oracle, refs, monkeypatch, tile_iters, swz):
    """K1 tiles of 1, 3 and 16 iterations, both LDS images: the maxima placed
    at the first and last position of an iteration and of a tile are then at
    a workgroup's first and last position."""
    from hashbox_amd import Engine
    monkeypatch.setenv("HBX_AB", "1")
    monkeypatch.setenv("HBX_K1_SWZ", swz)
    with Engine(0, tile_iters=tile_iters) as e:
        assert e.knobs()["k1_swz"] == int(swz)
        check_all(oracle, refs, e.chunk_hash_batch([cc.build(n) for n in NAMES]))


def test_batch_device_resident_pipelined(oracle, refs):
    """The packed batch submitted three times on the pipelined path, the MD5
    stage in 64-block slices, chunks joining two submits late."""
    import torch
    from hashbox_amd import Engine, pack_arena_layout
    files = [cc.build(n) for n in NAMES]
    sizes = [f.size for f in files]
    offs, total = pack_arena_layout(sizes)
    host = np.zeros(total, np.uint8)
    for o, f in zip(offs, files):
        host[int(o):int(o) + f.size] = f
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    with Engine(0, md5_slice=64, join_lag=2) as e:
        for _ in range(3):
            e.submit_device(dev.data_ptr(), offs, sizes)
        assert e.pending() == 3
        for _ in range(3):
            check_all(oracle, refs, e.wait())
        assert e.pending() == 0
