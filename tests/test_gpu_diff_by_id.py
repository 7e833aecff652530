"""GPU: diff_tree(by_id=True) and restore_tree(keep_matching=True): the files
whose local block IDs are their stored chain's are settled without reading a
data block; every other file goes through the byte comparison, so the answer is
that of the existing diff for every input.  The block store counts what is
read per ID."""
import hashlib
import os
import shutil
import stat
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Mi = 1 << 20
RAW, ZLIB = 0xFF, 0x01


def block_id(data: bytes, links=()) -> bytes:
    """HashboxBlock.HashData (block.go:96-111)."""
    return hashlib.md5(struct.pack(">I", len(links)) + b"".join(links) + struct.pack(">I", len(data)) + data).digest()


class Store:
    """An in-memory block store; read_block counts the calls per ID."""

    def __init__(self, blocks):
        self.blocks = dict(blocks)
        self.reads = {}

    def read_block(self, bid):
        bid = bytes(bid)
        self.reads[bid] = self.reads.get(bid, 0) + 1
        return self.blocks[bid]

    def reset(self):
        self.reads = {}


def _text(n, seed):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 9, 400)]
    out = b" ".join(words[int(i)] for i in rng.integers(0, len(words), n // 4 + 8))
    return out[:n]


@pytest.fixture(scope="module")
def tree(engine, tmp_path_factory):
    """A few dozen small files plus two multi-chunk ones, stored; every block
    by its ID as (DataType, data field, links), and per file its data blocks."""
    from hashbox_amd import formats as F
    tmp = tmp_path_factory.mktemp("by_id")
    rng = np.random.default_rng(31)
    src = tmp / "src"
    (src / "d1" / "d2").mkdir(parents=True)
    (src / "d3").mkdir()
    content = {}
    for k in range(36):
        sub = ("", "d1", "d1/d2", "d3")[k % 4]
        size = (1, 100, 4000, 65_535, 65_536, 70_001, 131_072, 200_000)[k % 8] + k
        content[os.path.join(sub, f"f{k:02d}")] = _text(size, k) if k % 3 else bytes(rng.integers(0, 256, size,
                                                                                                  dtype=np.uint8))
    content["d1/big_a.bin"] = bytes(rng.integers(0, 256, 5 * Mi // 2 + 17, dtype=np.uint8))
    content["d3/big_b.bin"] = bytes(rng.integers(0, 256, 3 * Mi + 1, dtype=np.uint8))
    content["empty"] = b""
    for k, (rel, data) in enumerate(content.items()):
        (src / rel).write_bytes(data)
        os.chmod(src / rel, (0o644, 0o600, 0o640)[k % 3])
        os.utime(src / rel, ns=(1_600_000_000 * 10**9, (1_500_000_000 + 1000 * k) * 10**9 + k))
    os.symlink("d1/f01", src / "link")
    t = F.store_tree(engine, src)
    blocks, data_ids = {}, {}
    for _p, (dblk, links, bid) in t.directories.items():
        blocks[bytes(bid)] = (ZLIB, zlib.compress(dblk, 6), list(links))
    for path, r in t.files.items():
        data = open(path, "rb").read()
        ends = [int(x) for x in r.cut_ends]
        rel = os.path.relpath(os.fsdecode(path), src)
        data_ids[rel] = [bytes(c) for c in r.ids]
        for n, (a, b, cid) in enumerate(zip([0] + ends[:-1], ends, r.ids)):
            assert block_id(data[a:b]) == bytes(cid)
            blocks[bytes(cid)] = (RAW, data[a:b], []) if n % 2 else (ZLIB, zlib.compress(data[a:b], 1), [])
        if r.content_type == F.TYPE_FILE_CHAIN:
            chain = [bytes(x) for x in r.ids]
            blocks[bytes(r.content_id)] = (RAW, F.serialize_chain_block(chain), chain)
    assert len(data_ids["d1/big_a.bin"]) > 1 and len(data_ids["d3/big_b.bin"]) > 1
    all_data = {i for ids in data_ids.values() for i in ids}
    return {"src": src, "t": t, "store": Store(blocks), "content": content, "data_ids": data_ids,
            "all_data": all_data, "tmp": tmp}


def _copy(tree, name):
    """A local copy of the stored tree with modes and ModTimes kept: <tmp>/<name>/src."""
    root = tree["tmp"] / name
    shutil.copytree(tree["src"], root / "src", symlinks=True)
    return root


def _rewrite(p, data):
    """New bytes with the size's owner, mode and ModTime kept."""
    st = os.lstat(p)
    p.write_bytes(data)
    os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns))


def _flip(data: bytes, at: int) -> bytes:
    b = bytearray(data)
    b[at] ^= 0x40
    return bytes(b)


def _both(engine, tree, root):
    """diff_tree both ways; what each read of the data blocks."""
    from hashbox_amd import formats as F
    s = tree["store"]
    s.reset()
    plain = F.diff_tree(engine, tree["t"].root, s.read_block, root, window_bytes=64 * Mi)
    s.reset()
    by_id = F.diff_tree(engine, tree["t"].root, s.read_block, root, window_bytes=64 * Mi, by_id=True)
    data_read = {i for i in s.reads if i in tree["all_data"]}
    assert "matched_by_id" not in plain
    matched = by_id.pop("matched_by_id")
    assert by_id == plain
    return plain, matched, data_read


N_DATA_FILES = 38  # 36 small files of size > 0 and the two big ones


def test_unchanged_copy_reads_no_data_block(engine, tree):
    plain, matched, data_read = _both(engine, tree, _copy(tree, "same"))
    assert plain["different"] == [] and plain["files"] == N_DATA_FILES + 1
    assert matched == N_DATA_FILES and data_read == set()
    # the plain diff did read them all
    from hashbox_amd import formats as F
    s = tree["store"]
    s.reset()
    F.diff_tree(engine, tree["t"].root, s.read_block, tree["tmp"] / "same", window_bytes=64 * Mi)
    assert {i for i in s.reads if i in tree["all_data"]} == tree["all_data"]


@pytest.mark.parametrize("rel", ["d1/d2/f06", "d1/big_a.bin"])
def test_one_byte_changed_reads_only_that_file(engine, tree, rel):
    root = _copy(tree, "flip_" + rel.replace("/", "_"))
    data = tree["content"][rel]
    at = len(data) * 2 // 3
    _rewrite(root / "src" / rel, _flip(data, at))
    plain, matched, data_read = _both(engine, tree, root)
    assert plain["different"] == [(str(root / "src" / rel), f"data is different at offset {at}")]
    assert matched == N_DATA_FILES - 1
    assert data_read and data_read <= set(tree["data_ids"][rel])


def test_size_missing_extra_mode_symlink(engine, tree):
    root = _copy(tree, "various")
    got = root / "src"
    (got / "d3" / "f03").write_bytes(tree["content"]["d3/f03"] + b"!")   # a size change
    os.remove(got / "d1" / "f05")                                         # a missing file
    (got / "d1" / "d2" / "extra").write_bytes(b"x")                       # an extra file
    os.chmod(got / "f04", 0o755)                                          # a mode change
    os.remove(got / "link")
    os.symlink("d3/f03", got / "link")                                    # a symlink retargeted
    plain, matched, data_read = _both(engine, tree, root)
    diff = dict(plain["different"])
    assert set(diff) == {str(got / "d3" / "f03"), str(got / "d1" / "f05"), str(got / "d1" / "d2" / "extra"),
                         str(got / "f04"), str(got / "link")}
    assert "size" in diff[str(got / "d3" / "f03")] and "permissions" in diff[str(got / "f04")]
    # the size change and the missing file never reach the data comparison; the chmod-ed file matches by ID
    assert matched == N_DATA_FILES - 2 and data_read == set()


def test_corrupt_block_of_a_changed_file_raises(engine, tree):
    from hashbox_amd import HbxError, formats as F
    rel = "d3/big_b.bin"
    root = _copy(tree, "corrupt")
    _rewrite(root / "src" / rel, _flip(tree["content"][rel], 5))
    victim = tree["data_ids"][rel][1]
    blocks = dict(tree["store"].blocks)
    ty, data, links = blocks[victim]
    blocks[victim] = (ty, data[:len(data) // 2], links)
    for by_id in (False, True):
        with pytest.raises(HbxError, match=victim.hex()):
            F.diff_tree(engine, tree["t"].root, Store(blocks).read_block, root, window_bytes=64 * Mi, by_id=by_id)
    # the same corrupt block behind an unchanged file is never fetched by ID
    same = tree["tmp"] / "same2"
    shutil.copytree(tree["src"], same / "src", symlinks=True)
    d = F.diff_tree(engine, tree["t"].root, Store(blocks).read_block, same, window_bytes=64 * Mi, by_id=True)
    assert d["different"] == [] and d["matched_by_id"] == N_DATA_FILES


def test_foreign_chain_compares_equal_through_the_bytes(engine, tmp_path):
    """A hand-built tree whose one file is chained in fixed 100 KiB blocks:
    valid, but not the engine's cuts."""
    from hashbox_amd import formats as F
    data = bytes(np.random.default_rng(5).integers(0, 256, 300 * 1024, dtype=np.uint8))
    (tmp_path / "top").mkdir()
    p = tmp_path / "top" / "file"
    p.write_bytes(data)
    pieces = [data[k:k + 100 * 1024] for k in range(0, len(data), 100 * 1024)]
    ids = [block_id(x) for x in pieces]
    blocks = {i: (RAW, x, []) for i, x in zip(ids, pieces)}
    chain = F.serialize_chain_block(ids)
    fe = F.entry_from_stat(b"file", os.lstat(p))
    fe.content_type, fe.content_block_id = F.TYPE_FILE_CHAIN, block_id(chain, ids)
    blocks[fe.content_block_id] = (RAW, chain, ids)
    dblk, links = F.serialize_directory_block([fe])
    root = F.entry_from_stat(b"top", os.lstat(tmp_path / "top"))
    root.content_type, root.file_size, root.content_block_id = F.TYPE_DIRECTORY, 0, block_id(dblk, links)
    blocks[root.content_block_id] = (RAW, dblk, list(links))
    s = Store(blocks)
    plain = F.diff_tree(engine, root, s.read_block, tmp_path, window_bytes=64 * Mi)
    s.reset()
    by_id = F.diff_tree(engine, root, s.read_block, tmp_path, window_bytes=64 * Mi, by_id=True)
    assert plain == {"files": 1, "directories": 1, "different": []}
    assert by_id == dict(plain, matched_by_id=0)
    assert all(s.reads.get(i) == 1 for i in ids)  # settled by its bytes
    # and a changed byte is found there
    _rewrite(p, _flip(data, 150_000))
    by_id = F.diff_tree(engine, root, s.read_block, tmp_path, window_bytes=64 * Mi, by_id=True)
    assert by_id["different"] == [(str(p), "data is different at offset 150000")] and by_id["matched_by_id"] == 0


def _snapshot(root):
    out = {}
    for d, _dirs, names in os.walk(root):
        for n in names + _dirs:
            p = os.path.join(d, n)
            st = os.lstat(p)
            rel = os.path.relpath(p, root)
            if stat.S_ISLNK(st.st_mode):
                out[rel] = ("link", os.readlink(p))
            elif stat.S_ISDIR(st.st_mode):
                out[rel] = ("dir", stat.S_IMODE(st.st_mode))
            else:
                out[rel] = ("file", stat.S_IMODE(st.st_mode), st.st_mtime_ns, open(p, "rb").read())
    return out


def test_restore_keep_matching(engine, tree):
    from hashbox_amd import formats as F
    s, t = tree["store"], tree["t"]
    fresh = tree["tmp"] / "fresh"
    fresh.mkdir()
    s.reset()
    st0 = F.restore_tree(engine, t.root, s.read_block, fresh, window_bytes=64 * Mi, batch=True)
    assert "kept" not in st0 and st0["files"] == N_DATA_FILES + 1
    assert {i for i in s.reads if i in tree["all_data"]} == tree["all_data"]

    over = tree["tmp"] / "over"
    over.mkdir()
    F.restore_tree(engine, t.root, s.read_block, over, window_bytes=64 * Mi, batch=True)
    got = over / "src"
    modified, deleted, chmodded = "d1/big_a.bin", "d3/f07", "d1/d2/f10"
    _rewrite(got / modified, _flip(tree["content"][modified], 1_000_000))
    os.remove(got / deleted)
    os.chmod(got / chmodded, 0o777)
    os.remove(got / "link")  # (a symlink is created, never overwritten: as in any restore over a tree)
    inodes = {rel: os.lstat(got / rel).st_ino for rel in tree["data_ids"] if rel != deleted}

    s.reset()
    st1 = F.restore_tree(engine, t.root, s.read_block, over, window_bytes=64 * Mi, batch=True, keep_matching=True)
    assert _snapshot(over) == _snapshot(fresh)
    assert st1["kept"] == N_DATA_FILES - 2
    assert st1["files"] == st0["files"] and st1["directories"] == st0["directories"]
    assert st1["bytes"] == len(tree["content"][modified]) + len(tree["content"][deleted])
    for rel, ino in inodes.items():
        if rel != modified:
            assert os.lstat(got / rel).st_ino == ino, rel
    assert {i for i in s.reads if i in tree["all_data"]} == set(tree["data_ids"][modified]) | set(
        tree["data_ids"][deleted])

    # keep_matching=False over the same tree reads every data block, as ever
    os.remove(got / "link")
    s.reset()
    st2 = F.restore_tree(engine, t.root, s.read_block, over, window_bytes=64 * Mi, batch=True)
    assert "kept" not in st2 and st2["bytes"] == st0["bytes"]
    assert {i for i in s.reads if i in tree["all_data"]} == tree["all_data"]
    assert _snapshot(over) == _snapshot(fresh)
