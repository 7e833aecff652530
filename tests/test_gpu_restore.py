"""GPU: a file's block chain back into its bytes, or compared with a local
copy (hbx_restore_blocks, hbx_restore_file_stream, K10; restoreFileData and
diffFileData, hashback/restore.go:45-66, 249-277).  The blocks go in as they
come off the wire (data field, DataType, expected BlockID); the expected value
is always the original bytes, with hashlib for the IDs and CPython's zlib as
the stand-in for Go's compress/zlib.  No reference binary is involved.
"""
import hashlib
import os
import stat
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, ZLIB = 0xFF, 0x01
P = 65536  # hbxr::kPiece: bytes per K10 workgroup
Mi = 1 << 20
STRIDE = 8 * Mi + 256  # one inflate slot at the default max_block
ERR_IO, ERR_VERIFY = -4, -9


def _text(n, seed):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 10, 300)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.zipf(1.3)) % len(words)] + b" "
    return bytes(out[:n])


def block_id(data: bytes, links=()) -> bytes:
    """HashboxBlock.HashData (pkg/core/block.go:96-111)."""
    return hashlib.md5(struct.pack(">I", len(links)) + b"".join(links) + struct.pack(">I", len(data)) + data).digest()


def wire(blocks, mode):
    """(data fields, types) of the blocks: 'z' every block a zlib -6 stream,
    'r' every block raw, 'zr' / 'rz' alternating."""
    datas, types = [], []
    for i, b in enumerate(blocks):
        t = mode[i % len(mode)]
        datas.append(zlib.compress(b, 6) if t == "z" else b)
        types.append(ZLIB if t == "z" else RAW)
    return datas, types


# ---------------------------------------------------------------- inputs --
_cache = {}


def round_trip_file():
    """3 MiB + 13 bytes of text, random data and text again."""
    if "file" not in _cache:
        n = 3 * Mi + 13
        rnd = np.random.default_rng(7).integers(0, 256, Mi, dtype=np.uint8).tobytes()
        _cache["file"] = _text(Mi, 1) + rnd + _text(n - 2 * Mi, 2)
    return _cache["file"]


@pytest.fixture(scope="module")
def stored(engine, tmp_path_factory):
    """The round-trip file cut, hashed and compressed by the engine itself:
    (bytes, chunks, ids, K7 streams)."""
    data = round_trip_file()
    path = tmp_path_factory.mktemp("restore") / "file.bin"
    path.write_bytes(data)
    r = engine.store_file(path, segment_bytes=16 * Mi, compress=True)
    ends = [int(x) for x in r.cut_ends]
    chunks = [data[a:b] for a, b in zip([0] + ends[:-1], ends)]
    assert r.n_chunks >= 4 and b"".join(chunks) == data
    return data, chunks, [bytes(x) for x in r.ids], [bytes(z) for z in r.zstreams]


def chain8():
    """Eight text blocks of odd lengths; block 0 spans more than two pieces."""
    if "chain8" not in _cache:
        lens = [2 * P + 18_929, 70_001, 1, 99_999, 123_457, 65_537, 80_000, 31]
        blocks = [_text(n, 50 + i) for i, n in enumerate(lens)]
        _cache["chain8"] = (blocks, [block_id(b) for b in blocks], [zlib.compress(b, 6) for b in blocks])
    return _cache["chain8"]


def edge_chain():
    """Lengths 0, 1, 15, 16, 17, 63, 64, 65, P-1, P, P+1 and fillers, ordered
    so that every destination offset mod 16 occurs."""
    if "edge" not in _cache:
        lens = [0, 1, 15, 16, 17, 63, 64, 65, P - 1, P, P + 1] + [1] * 13 + [17, P + 1, 0, 15, P - 1, 63, 3, P, 5,
                                                                          P + 1, 2, P - 1]
        rng = np.random.default_rng(99)
        blocks = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) if i % 2 else _text(n, 300 + i)
                  for i, n in enumerate(lens)]
        offs = np.concatenate([[0], np.cumsum(lens)])
        assert set(int(o) % 16 for o in offs[:-1]) == set(range(16))
        _cache["edge"] = (blocks, [block_id(b) for b in blocks])
    return _cache["edge"]


# ------------------------------------------------------------ round trip --
def test_round_trip_k7_streams(engine, stored):
    data, chunks, ids, zs = stored
    r = engine.restore_blocks(zs, [ZLIB] * len(zs), ids)
    assert r.status.tolist() == [0] * len(zs) and r.n_good == len(zs)
    assert r.data == data
    assert r.offs.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).tolist()
    assert r.first_diff is None


def test_round_trip_zlib6_streams(engine, stored):
    data, chunks, ids, _ = stored
    datas, types = wire(chunks, "z")
    r = engine.restore_blocks(datas, types, ids)
    assert r.n_good == len(chunks) and r.data == data


@pytest.mark.parametrize("mode", ["zr", "rz", "r"])
def test_round_trip_with_raw_blocks(engine, stored, mode):
    data, chunks, ids, zs = stored
    datas, types = wire(chunks, mode)
    datas = [z if t == ZLIB else d for d, t, z in zip(datas, types, zs)]  # the zlib ones as K7 wrote them
    r = engine.restore_blocks(datas, types, ids)
    assert r.status.tolist() == [0] * len(chunks) and r.data == data


def test_empty_chain(engine):
    r = engine.restore_blocks([], [], [])
    assert r.n_good == 0 and r.data == b"" and r.offs.tolist() == [0]
    d = engine.restore_blocks([], [], [], local=b"abc")
    assert d.first_diff == 0 and d.data is None
    assert engine.restore_blocks([], [], [], local=b"").first_diff is None


# ---------------------------------------------------------- gather edges --
@pytest.mark.parametrize("mode", ["z", "r", "zr", "rz"])
def test_gather_edges_with_canaries(engine, mode):
    """Every destination offset mod 16; as raw blocks the source is unaligned
    too (raw data fields are staged byte-packed).  64 canary bytes on each side
    of the output stay as they were."""
    blocks, ids = edge_chain()
    want = b"".join(blocks)
    datas, types = wire(blocks, mode)
    buf = np.full(64 + len(want) + 64, 0xA5, np.uint8)
    r = engine.restore_blocks(datas, types, ids, out=buf[64:64 + len(want)])
    assert r.status.tolist() == [0] * len(blocks)
    assert r.data == want
    assert buf[64:64 + len(want)].tobytes() == want
    assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all()
    assert r.offs.tolist() == np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).tolist()


@pytest.mark.parametrize("mode", ["z", "rz"])
def test_gather_edges_through_the_pinned_sink(engine, mode):
    """The same chain through hbx_restore_file_stream: K10 writes pinned host
    memory, five blocks per window."""
    blocks, ids = edge_chain()
    want = b"".join(blocks)
    datas, types = wire(blocks, mode)
    got, spans = bytearray(), []

    def on_data(off, a):
        spans.append((off, a.size))
        got.extend(a.tobytes())
    mb = P + 1
    n = engine.restore_file(ids, lambda i: (types[i], datas[i]), on_data=on_data, window_bytes=5 * (mb + 511),
                            max_block=mb)
    assert n == len(want) and bytes(got) == want
    assert len(spans) >= 4


# ----------------------------------------------------------- long stream --
_CHILD = r"""
import sys, zlib, hashlib, struct
import numpy as np
sys.path.insert(0, %r)
from tests.test_gpu_restore import _text, block_id
from hashbox_amd import Engine
d = _text(1 << 20, 77)
z = zlib.compress(d, 6)
assert len(z) >= 65536
with Engine(0) as e:
    assert e.knobs()["ab_env"]
    r = e.restore_blocks([z, d[:1000], z], [1, 0xFF, 1], [block_id(d), block_id(d[:1000]), block_id(d)])
    assert r.status.tolist() == [0, 0, 0], r.status
    assert r.data == d + d[:1000] + d
    k = e.knobs()
print("OK", k["k8_split_streams"], k["k8_split_fallbacks"])
"""


@pytest.mark.parametrize("mode", ["wave", "lane", "split"])
def test_long_stream_under_each_decoder(mode):
    """A 1 MiB text block whose zlib -6 stream is over 64 KiB (K8s takes it),
    under each HBX_K8_MODE, each in a fresh process."""
    env = dict(os.environ, HBX_AB="1", HBX_K8_MODE=mode)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.strip().splitlines()[-1].split()
    assert out[0] == "OK"
    if mode == "split":
        assert int(out[1]) == 2, out  # both long streams went through K8s


# ----------------------------------------------------------- prefix rule --
def _inflates_to(z: bytes):
    """What CPython's zlib makes of a stream: the bytes, or None if it fails
    (an incomplete stream counts as failing)."""
    try:
        o = zlib.decompressobj()
        out = o.decompress(z)
        return out if o.eof else None
    except zlib.error:
        return None


def _corruptions(z: bytes):
    mid = len(z) // 2
    return {"truncated": z[:mid],
            "middle_byte": z[:mid] + bytes([z[mid] ^ 0x5A]) + z[mid + 1:],
            "adler": z[:-4] + bytes(b ^ 0xFF for b in z[-4:])}


@pytest.mark.parametrize("kind", ["truncated", "middle_byte", "adler"])
def test_prefix_rule_corrupt_stream(engine, kind):
    blocks, ids, zs = chain8()
    bad = _corruptions(zs[5])[kind]
    assert _inflates_to(bad) != blocks[5], "the corruption changes nothing: the case would prove nothing"
    datas = zs[:5] + [bad] + zs[6:]
    want = b"".join(blocks)
    buf = np.full(len(want) + 64, 0xA5, np.uint8)
    r = engine.restore_blocks(datas, [ZLIB] * 8, ids, out=buf)
    assert r.n_good == 5
    assert 1 <= int(r.status[5]) <= 7, r.status
    if kind == "adler":
        assert int(r.status[5]) == 1
    assert r.status[:5].tolist() == [0] * 5 and r.status[6:].tolist() == [0, 0]  # every block gets its own status
    end = int(r.offs[5])
    assert end == sum(len(b) for b in blocks[:5]) and len(r.offs) == 6
    assert r.data == want[:end] and buf[:end].tobytes() == want[:end]
    assert (buf[end:] == 0xA5).all(), "written past the good prefix"


def test_prefix_rule_wrong_id(engine):
    blocks, ids, zs = chain8()
    wrong = ids[:2] + [block_id(blocks[2] + b"x")] + ids[3:]
    want = b"".join(blocks)
    buf = np.full(len(want) + 64, 0xA5, np.uint8)
    r = engine.restore_blocks(zs, [ZLIB] * 8, wrong, out=buf)
    assert r.n_good == 2 and int(r.status[2]) == 7
    end = len(blocks[0]) + len(blocks[1])
    assert r.data == want[:end] and (buf[end:] == 0xA5).all()
    # the same as raw blocks
    r = engine.restore_blocks(blocks, [RAW] * 8, wrong)
    assert r.n_good == 2 and int(r.status[2]) == 7 and r.data == want[:end]


def test_oversized_stream_and_unknown_type(engine):
    blocks, ids, zs = chain8()
    zeros = bytes(9 * Mi)
    z = zlib.compress(zeros, 6)
    r = engine.restore_blocks([zs[0], z, zs[2]], [ZLIB] * 3, [ids[0], block_id(zeros), ids[2]])
    assert r.status.tolist() == [0, 3, 0] and r.n_good == 1 and r.data == blocks[0]
    # with room for it, the same stream is fine
    r = engine.restore_blocks([z], [ZLIB], [block_id(zeros)], max_block=9 * Mi)
    assert r.status.tolist() == [0] and r.data == zeros
    r = engine.restore_blocks([zs[0], zs[1]], [ZLIB, 0x02], ids[:2])
    assert r.status.tolist() == [0, 8] and r.n_good == 1 and r.data == blocks[0]
    # a data field longer than the bound; a raw block longer than max_block
    r = engine.restore_blocks([bytes(70_000)], [ZLIB], [bytes(16)], max_block=60_000)
    assert r.status.tolist() == [8] and r.n_good == 0 and r.data == b""
    r = engine.restore_blocks([blocks[1]], [RAW], [ids[1]], max_block=70_000)
    assert r.status.tolist() == [3]
    r = engine.restore_blocks([blocks[1]], [RAW], [ids[1]], max_block=70_001)
    assert r.status.tolist() == [0] and r.data == blocks[1]


def test_crafted_streams_restore_and_verify(engine, oracle):
    """Hand-built streams (tests/deflate_craft.py) through the whole restore:
    a match at the full window distance, stored blocks whose payload is itself
    zlib streams, and a 1000:1 chain of overlapping copies, which outgrows the
    size the restore path guesses from the compressed length.  The IDs are the
    oracle's.  Then a chain whose second block carries an incomplete Huffman
    code, which zlib refuses: the prefix rule stops there."""
    from tests import deflate_craft as C
    by = {c.name: c for c in C.far() + C.split_may_fall_back() + C.chains() + C.rejections()}
    cases = [by["far_D32768_L258"], by["stored_payload_of_zlib_streams"], by["chain_dynamic_1000_to_1"]]
    ids = [oracle.block_id(np.frombuffer(c.expected, np.uint8)) for c in cases]
    assert ids == [block_id(c.expected) for c in cases]
    r = engine.restore_blocks([c.stream for c in cases], [ZLIB] * 3, ids)
    assert r.status.tolist() == [0, 0, 0] and r.n_good == 3
    assert r.data == b"".join(c.expected for c in cases)
    bad = by["incomplete_litlen_code"]
    r = engine.restore_blocks([cases[0].stream, bad.stream, cases[2].stream], [ZLIB] * 3, [ids[0], bytes(16), ids[2]])
    assert r.n_good == 1 and int(r.status[1]) != 0 and int(r.status[0]) == 0
    assert r.data == cases[0].expected


def test_out_cap_smaller_than_the_prefix_is_an_argument_error(engine):
    from hashbox_amd import HbxError
    blocks, ids, zs = chain8()
    with pytest.raises(HbxError, match="HBX_ERR_ARG"):
        engine.restore_blocks(zs[:2], [ZLIB] * 2, ids[:2], out=np.zeros(len(blocks[0]) + 5, np.uint8))
    assert engine.restore_blocks(zs[:2], [ZLIB] * 2, ids[:2]).data == blocks[0] + blocks[1]


# ----------------------------------------------------------------- links --
def test_directory_block_with_links(engine):
    from hashbox_amd import formats as F
    rng = np.random.default_rng(4)
    entries = [F.FileEntry(file_name=b"name%d" % i, file_size=1000 + i, file_mode=0o644, mod_time=10**18 + i,
                           content_type=F.TYPE_FILE_DATA,
                           content_block_id=bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for i in range(40)]
    dblk, links = F.serialize_directory_block(entries)
    assert len(links) == 40
    bid = block_id(dblk, links)
    z = zlib.compress(dblk, 6)
    r = engine.restore_blocks([z, dblk], [ZLIB, RAW], [bid, bid], links=[links, links])
    assert r.status.tolist() == [0, 0] and r.data == dblk + dblk
    assert [e.file_name for e in F.parse_directory_block(r.data[:len(dblk)])] == [e.file_name for e in entries]
    altered = links[:7] + [bytes(16)] + links[8:]
    r = engine.restore_blocks([z, dblk], [ZLIB, RAW], [bid, bid], links=[altered, links])
    assert r.status.tolist() == [7, 0] and r.n_good == 0 and r.data == b""
    r = engine.restore_blocks([z], [ZLIB], [bid])  # without its links the ID differs too
    assert r.status.tolist() == [7]


# ------------------------------------------------------------------ diff --
def _diff_positions():
    blocks, _, _ = chain8()
    total = sum(len(b) for b in blocks)
    b1 = len(blocks[0])
    return {"first": 0, "at15": 15, "at16": 16, "last_of_block0": b1 - 1, "first_of_block1": b1,
            "before_piece": P - 1, "after_piece": P, "piece_in_block1_before": b1 + P - 1, "piece_in_block1": b1 + P,
            "last": total - 1}


@pytest.mark.parametrize("mode", ["z", "rz"])
def test_diff_identical(engine, mode):
    blocks, ids, _ = chain8()
    datas, types = wire(blocks, mode)
    r = engine.restore_blocks(datas, types, ids, local=b"".join(blocks))
    assert r.n_good == 8 and r.first_diff is None and r.data is None


@pytest.mark.parametrize("where", list(_diff_positions()))
def test_diff_single_flip(engine, where):
    blocks, ids, zs = chain8()
    at = _diff_positions()[where]
    local = bytearray(b"".join(blocks))
    local[at] ^= 0x01
    r = engine.restore_blocks(zs, [ZLIB] * 8, ids, local=bytes(local))
    assert r.first_diff == at and r.n_good == 8


def test_diff_two_flips_and_lengths(engine):
    blocks, ids, zs = chain8()
    whole = b"".join(blocks)
    local = bytearray(whole)
    local[200_000] ^= 0x80
    local[70_003] ^= 0x80
    datas, types = wire(blocks, "rz")
    assert engine.restore_blocks(datas, types, ids, local=bytes(local)).first_diff == 70_003
    total = len(whole)
    assert engine.restore_blocks(zs, [ZLIB] * 8, ids, local=whole[:-1]).first_diff == total - 1
    assert engine.restore_blocks(zs, [ZLIB] * 8, ids, local=whole + b"!").first_diff == total
    # a difference before the shorter end still wins
    assert engine.restore_blocks(zs, [ZLIB] * 8, ids, local=bytes(local[:-1])).first_diff == 70_003
    # only the good prefix is compared: a flip behind the bad block is not seen
    bad = zs[:3] + [zs[3][:50]] + zs[4:]
    r = engine.restore_blocks(bad, [ZLIB] * 8, ids, local=bytes(local))
    end = sum(len(b) for b in blocks[:3])
    assert r.n_good == 3 and 200_000 < end and r.first_diff == 70_003
    local2 = bytearray(whole)
    local2[end + 10] ^= 1
    assert engine.restore_blocks(bad, [ZLIB] * 8, ids, local=bytes(local2)).first_diff == end  # lengths differ there


# ------------------------------------------------------------- streaming --
def test_stream_to_a_file_and_a_sink(engine, stored, tmp_path):
    data, chunks, ids, zs = stored
    out = tmp_path / "restored.bin"
    n = engine.restore_file(ids, lambda i: (ZLIB, zs[i]), out_path=out, window_bytes=2 * STRIDE)
    assert n == len(data) and out.read_bytes() == data
    spans, got = [], bytearray()

    def on_data(off, a):
        spans.append((off, a.size))
        got.extend(a.tobytes())
    datas, types = wire(chunks, "zr")
    n = engine.restore_file(ids, lambda i: (types[i], datas[i]), on_data=on_data, window_bytes=2 * STRIDE)
    assert n == len(data) and bytes(got) == data
    assert len(spans) == (len(chunks) + 1) // 2  # two blocks per window
    pos = 0
    for off, ln in spans:  # contiguous, ordered, covering the file once
        assert off == pos and ln > 0
        pos += ln
    assert pos == len(data)
    # an empty chain is an empty file
    empty = tmp_path / "empty.bin"
    assert engine.restore_file([], lambda i: (RAW, b""), out_path=empty) == 0 and empty.read_bytes() == b""


def test_stream_diff(engine, stored, tmp_path):
    data, chunks, ids, zs = stored
    src = lambda i: (ZLIB, zs[i])  # noqa: E731
    same = tmp_path / "same.bin"
    same.write_bytes(data)
    assert engine.diff_file(ids, src, same, window_bytes=2 * STRIDE) == (True, None)
    for at in (0, len(chunks[0]) + len(chunks[1]) + 77, len(data) - 1):  # first window, second window, last byte
        flipped = bytearray(data)
        flipped[at] ^= 0x10
        other = tmp_path / "other.bin"
        other.write_bytes(bytes(flipped))
        assert engine.diff_file(ids, src, other, window_bytes=2 * STRIDE) == (False, at)
    short = tmp_path / "short.bin"
    short.write_bytes(data[:-1])
    assert engine.diff_file(ids, src, short, window_bytes=2 * STRIDE) == (False, len(data) - 1)
    longer = tmp_path / "long.bin"
    longer.write_bytes(data + b"?")
    assert engine.diff_file(ids, src, longer, window_bytes=2 * STRIDE) == (False, len(data))
    tiny = tmp_path / "tiny.bin"
    tiny.write_bytes(data[:1000])  # the local copy ends inside the first window
    assert engine.diff_file(ids, src, tiny, window_bytes=2 * STRIDE) == (False, 1000)


def test_stream_failures_leave_the_engine_usable(engine, stored, tmp_path):
    from hashbox_amd import RestoreError
    data, chunks, ids, zs = stored
    assert len(chunks) >= 4
    off3 = sum(len(c) for c in chunks[:3])

    def check_usable():
        out = tmp_path / "again.bin"
        assert engine.pending() == 0
        assert engine.restore_file(ids, lambda i: (ZLIB, zs[i]), out_path=out, window_bytes=2 * STRIDE) == len(data)
        assert out.read_bytes() == data

    class SourceDown(Exception):
        pass

    def failing(i):
        if i == 3:
            raise SourceDown("block 3")
        return ZLIB, zs[i]
    seen = []
    with pytest.raises(SourceDown):
        engine.restore_file(ids, failing, on_data=lambda off, a: seen.append((off, a.size)), window_bytes=2 * STRIDE)
    assert all(off + ln <= off3 for off, ln in seen)
    check_usable()

    bad = zs[3][:len(zs[3]) // 2]
    assert _inflates_to(bad) is None
    seen = []
    with pytest.raises(RestoreError) as ei:
        engine.restore_file(ids, lambda i: (ZLIB, bad if i == 3 else zs[i]),
                            on_data=lambda off, a: seen.append((off, a.size)), window_bytes=2 * STRIDE)
    assert ei.value.code == ERR_VERIFY and ei.value.bad_index == 3 and 1 <= ei.value.bad_status <= 7
    assert ei.value.bytes == off3
    assert seen and all(off + ln <= off3 for off, ln in seen), seen  # nothing at or past block 3
    assert sum(ln for _, ln in seen) == off3  # ... and everything before it
    check_usable()

    # a wrong ID is a bad block too; to a file, the blocks before it are written
    wrong = ids[:1] + [bytes(16)] + ids[2:]
    part = tmp_path / "part.bin"
    with pytest.raises(RestoreError) as ei:
        engine.restore_file(wrong, lambda i: (ZLIB, zs[i]), out_path=part, window_bytes=2 * STRIDE)
    assert (ei.value.code, ei.value.bad_index, ei.value.bad_status) == (ERR_VERIFY, 1, 7)
    assert part.read_bytes() == chunks[0]
    check_usable()

    class SinkDown(Exception):
        pass

    def sink(off, a):
        if off > 0:
            raise SinkDown()
    with pytest.raises(SinkDown):
        engine.restore_file(ids, lambda i: (ZLIB, zs[i]), on_data=sink, window_bytes=2 * STRIDE)
    check_usable()
    with pytest.raises(RestoreError) as ei:  # a file that cannot be created
        engine.restore_file(ids, lambda i: (ZLIB, zs[i]), out_path=tmp_path / "no" / "such" / "dir.bin")
    assert ei.value.code == ERR_IO
    check_usable()


# ------------------------------------------------------------------ tree --
def test_restore_tree(engine, tmp_path):
    from hashbox_amd import formats as F
    rng = np.random.default_rng(12)
    src = tmp_path / "src"
    (src / "a" / "b").mkdir(parents=True)
    big = bytes(rng.integers(0, 256, 5 * Mi // 2, dtype=np.uint8))
    mid = _text(70 * 1024, 8)
    (src / "a" / "big.bin").write_bytes(big)
    (src / "a" / "b" / "mid.txt").write_bytes(mid)
    (src / "empty").write_bytes(b"")
    os.symlink("a/b/mid.txt", src / "link")
    ro = _text(3000, 9)
    (src / "a" / "readonly.txt").write_bytes(ro)  # no write bit: the reference writes through the handle it created
    os.chmod(src / "a" / "readonly.txt", 0o444)
    os.utime(src / "a" / "readonly.txt", ns=(1_600_000_000 * 10**9, 1_200_000_003 * 10**9))
    os.chmod(src / "a" / "big.bin", 0o600)
    os.chmod(src / "a" / "b" / "mid.txt", 0o640)
    os.chmod(src / "a" / "b", 0o750)
    os.utime(src / "a" / "big.bin", ns=(1_600_000_000 * 10**9, 1_500_000_123 * 10**9 + 456))
    os.utime(src / "a" / "b" / "mid.txt", ns=(1_600_000_000 * 10**9, 1_400_000_001 * 10**9))
    os.utime(src / "empty", ns=(1_600_000_000 * 10**9, 1_300_000_002 * 10**9))

    t = F.store_tree(engine, src)
    # the server: every block of the backup by its ID, as (DataType, data field, links)
    server = {}
    raw_blocks = []  # (id, data, links)
    for _path, (dblk, links, bid) in t.directories.items():
        raw_blocks.append((bid, dblk, links))
    for path, r in t.files.items():
        data = open(path, "rb").read()
        ends = [int(x) for x in r.cut_ends]
        for a, b, cid in zip([0] + ends[:-1], ends, r.ids):
            raw_blocks.append((bytes(cid), data[a:b], []))
        if r.content_type == F.TYPE_FILE_CHAIN:
            chain_ids = [bytes(x) for x in r.ids]
            raw_blocks.append((r.content_id, F.serialize_chain_block(chain_ids), chain_ids))
    assert any(r.content_type == F.TYPE_FILE_CHAIN for r in t.files.values())
    assert any(r.content_type == F.TYPE_FILE_DATA for r in t.files.values())
    zs = engine.deflate_blocks([d for _, d, _ in raw_blocks])
    for k, ((bid, d, links), z) in enumerate(zip(raw_blocks, zs)):
        server[bytes(bid)] = (RAW, d, links) if k % 5 == 4 else (ZLIB, z, links)
    asked = []

    def read_block(bid):
        asked.append(bid)
        return server[bid]
    dest = tmp_path / "dest"
    dest.mkdir()
    stats = F.restore_tree(engine, t.root, read_block, dest, window_bytes=2 * STRIDE)
    got = dest / "src"
    assert stats["files"] == 4 and stats["directories"] == 3 and stats["bytes"] == len(big) + len(mid) + len(ro)
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
    assert set(asked) == set(server)  # every block of the backup was read
    # a corrupted block anywhere stops the restore
    from hashbox_amd import HbxError
    victim = bytes(t.files[os.fsencode(src / "a" / "big.bin")].ids[1])
    ty, d, links = server[victim]
    server[victim] = (ty, d[:len(d) // 2], links)
    dest2 = tmp_path / "dest2"
    dest2.mkdir()
    with pytest.raises(HbxError):
        F.restore_tree(engine, t.root, read_block, dest2, window_bytes=2 * STRIDE)
