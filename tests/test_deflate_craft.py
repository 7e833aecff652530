"""CPU: the hand-built deflate streams of tests/deflate_craft.py against
CPython's zlib, which this makes the reference for every case's verdict and
bytes; test_gpu_inflate_crafted.py then compares the device with the table.
"""
import zlib

import pytest

from oracle import deflate as OD
from tests import deflate_craft as C

FAMILIES = [C.copy_grid, C.chains, C.far, C.structure, C.rejections, C.split_good, C.split_short,
            C.split_may_fall_back]


def test_writer_and_expand():
    w = C.BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    w.code(0b0110001, 7)  # reversed: first bit of the code first
    assert w.tell() == 10 and w.getvalue() == bytes([0b00110011, 0b10])
    assert C.expand([1, 2, 3, (5, 2), b"xy", (2, 7)]) == bytes([1, 2, 3, 2, 3, 2, 3, 2]) + b"xy" + bytes([2, 3])
    with pytest.raises(ValueError):
        C.expand([1, (3, 2)])
    lens = C.huffman_lens({0: 5, 1: 1, 2: 1, 7: 3}, 8)
    assert sum(2.0 ** -k for k in lens if k) == 1.0 and lens[0] == 1
    # the builder reproduces a stream zlib itself inflates, block kinds mixed
    data = C.expand([b"abcabc", (200, 3), 0, (258, 1)])
    z = C.zwrap([C.stored(b"abc", False), C.fixed([b"abc", (200, 3)], False), C.dynamic([0, (258, 1)], True)], data)
    assert zlib.decompress(z) == data


def test_case_names_are_unique():
    names = [c.name for f in FAMILIES for c in f()]
    assert len(names) == len(set(names))
    assert len(C.copy_grid()) == len(C.GRID_D) * len(C.GRID_L) * 2 == 1440


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_cases_agree_with_zlib(family):
    for c in family():
        if c.status == 0:
            got = zlib.decompress(c.stream) if c.name in C.TRAILING else OD.inflate_strict(c.stream)
            assert got == c.expected, c.name
            assert c.min_cap == len(c.expected), c.name
        elif c.status == 3:
            # a valid stream: the verdict comes from the capacity, one byte short
            assert len(OD.inflate_strict(c.stream)) == c.min_cap + 1, c.name
        else:
            assert c.expected is None and (c.status == C.ANY_ERROR or 1 <= c.status <= 6), c.name
            with pytest.raises(zlib.error):
                zlib.decompress(c.stream)
                pytest.fail(f"zlib accepts {c.name}")


def test_the_cases_reach_what_they_aim_at():
    """The properties the families are built for, read back from the streams."""
    far = {c.name: c for c in C.far()}
    assert len(far["far_D32768_L258"].expected) == 32768 + 70 + 258 + 1
    mx = [c for c in C.structure() if c.name == "hlit_286_hdist_30"][0]
    assert len(mx.stream) > 270  # a header of about 280 bytes
    t = C.three_block_stream()
    assert 150 <= len(t.stream) <= 260
    for c in C.split_good():
        assert len(c.stream) >= 2 * C.REGION, c.name
    by = {c.name: c for c in C.split_good() + C.split_short()}
    assert len(by["split_len_65535"].stream) == 65535 and len(by["split_len_65536"].stream) == 65536
    assert len(by["split_fixed_sync_5_regions"].stream) >= 5 * C.REGION
    assert len(by["split_final_block_in_last_bytes"].stream) == 3 * C.REGION
    for c in C.split_may_fall_back():
        assert len(c.stream) >= 3 * C.REGION, c.name
    chain = [c for c in C.chains() if c.name == "chain_dynamic_1000_to_1"][0]
    assert len(chain.expected) > 900 * len(chain.stream)
