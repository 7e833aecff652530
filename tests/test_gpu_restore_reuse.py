"""GPU: restore_tree(batch=True, reuse_local=True): a restore over an existing
tree fetches only the data blocks no local file holds (K13, Engine.locate_ids).

The block store counts what is read per ID.  The model of what must be read
comes from the oracle's chunking of the local files alone: the IDs of the
chains of the files that are not already right, minus the IDs of every chunk of
every pool file.  After every case the restored tree equals a fresh restore in
bytes, modes, ModTimes and symlinks, and no temporary file is left."""
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
BIG_A, BIG_B = "d1/big_a.bin", "d3/big_b.bin"


def block_id(data: bytes, links=()) -> bytes:
    """HashboxBlock.HashData (block.go:96-111)."""
    return hashlib.md5(struct.pack(">I", len(links)) + b"".join(links) + struct.pack(">I", len(data)) + data).digest()


class Store:
    """An in-memory block store; read_block counts the calls per ID.  `hook`
    (an ID -> a callable) runs once, before that ID's first read returns."""

    def __init__(self, blocks):
        self.blocks = dict(blocks)
        self.reads = {}
        self.hook = {}

    def read_block(self, bid):
        bid = bytes(bid)
        self.reads[bid] = self.reads.get(bid, 0) + 1
        if bid in self.hook:
            self.hook.pop(bid)()
        return self.blocks[bid]


@pytest.fixture(scope="module")
def tree(engine, tmp_path_factory):
    """A dozen small files plus two multi-chunk ones (at most 3 MiB), stored;
    every block by its ID as (DataType, data field, links), per file its data
    blocks, and a fresh restore to compare against."""
    from hashbox_amd import formats as F
    tmp = tmp_path_factory.mktemp("reuse")
    rng = np.random.default_rng(31)
    src = tmp / "src"
    (src / "d1" / "d2").mkdir(parents=True)
    (src / "d3").mkdir()
    content = {}
    for k in range(12):
        sub = ("", "d1", "d1/d2", "d3")[k % 4]
        size = (1, 100, 4000, 65_535, 65_536, 70_001, 131_072, 200_000)[k % 8] + k
        content[os.path.join(sub, f"f{k:02d}")] = bytes(rng.integers(0, 256, size, dtype=np.uint8))
    content[BIG_A] = bytes(rng.integers(0, 256, 5 * Mi // 2 + 17, dtype=np.uint8))
    content[BIG_B] = bytes(rng.integers(0, 256, 3 * Mi - 5, dtype=np.uint8))
    content["empty"] = b""
    for k, (rel, data) in enumerate(content.items()):
        (src / rel).write_bytes(data)
        os.chmod(src / rel, (0o644, 0o444, 0o640, 0o600)[k % 4])  # (BIG_B and three small files read-only)
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
    assert len(data_ids[BIG_A]) > 2 and len(data_ids[BIG_B]) > 2
    all_data = {i for ids in data_ids.values() for i in ids}
    assert sum(len(ids) for ids in data_ids.values()) == len(all_data)  # no ID twice: a read names its file
    fresh = tmp / "fresh"
    fresh.mkdir()
    st0 = F.restore_tree(engine, t.root, Store(blocks).read_block, fresh, window_bytes=64 * Mi, batch=True)
    return {"src": src, "t": t, "blocks": blocks, "content": content, "data_ids": data_ids, "all_data": all_data,
            "tmp": tmp, "fresh": _snapshot(fresh), "st0": st0, "n_data_files": len(data_ids)}


def _snapshot(root):
    out = {}
    for d, dirs, names in os.walk(root):
        for n in names + dirs:
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


def _copy(tree, name):
    """A local copy of the stored tree with modes and ModTimes kept, <tmp>/<name>/src, without the symlink (a
    symlink is created, never overwritten: as in any restore over a tree)."""
    root = tree["tmp"] / name
    shutil.copytree(tree["src"], root / "src", symlinks=True)
    os.remove(root / "src" / "link")
    return root


def _rewrite(p, data):
    """New bytes with the mode and ModTime kept."""
    st = os.lstat(p)
    os.chmod(p, 0o600)
    p.write_bytes(data)
    os.chmod(p, stat.S_IMODE(st.st_mode))
    os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns))


def _flip(data: bytes, at: int) -> bytes:
    b = bytearray(data)
    b[at] ^= 0x40
    return bytes(b)


def _oracle_ids(oracle, path):
    return [bytes(x) for x in oracle.store_file(np.fromfile(path, np.uint8), fast=True).ids]


def _model(oracle, tree, root, reuse_paths=()):
    """(the files already right, the data block IDs that must be fetched), from the oracle's chunking of the
    local files: the chains of the files that are not right, minus every chunk of every pool file."""
    pool, kept, needed = set(), set(), set()
    for rel, chain in tree["data_ids"].items():
        p = root / "src" / rel
        ids = _oracle_ids(oracle, p) if p.is_file() else None
        if ids == chain:
            kept.add(rel)
        else:
            needed.update(chain)
        pool.update(ids or ())
    for p in reuse_paths:
        pool.update(_oracle_ids(oracle, p))
    return kept, needed - pool


def _restore(engine, tree, root, store=None, **kw):
    from hashbox_amd import formats as F
    s = store or Store(tree["blocks"])
    stats = F.restore_tree(engine, tree["t"].root, s.read_block, root, window_bytes=64 * Mi, batch=True, **kw)
    return stats, {i for i in s.reads if i in tree["all_data"]}, s


def _check_tree(tree, root):
    assert _snapshot(root) == tree["fresh"]  # bytes, modes, ModTimes, symlinks; and no other name is there


def test_unchanged_copy_reads_nothing(engine, oracle, tree):
    root = _copy(tree, "same")
    kept, fetch = _model(oracle, tree, root)
    assert len(kept) == tree["n_data_files"] and fetch == set()
    inodes = {rel: os.lstat(root / "src" / rel).st_ino for rel in tree["data_ids"]}
    stats, data_read, _ = _restore(engine, tree, root, reuse_local=True)
    assert data_read == set()
    assert stats["kept"] == tree["n_data_files"] and stats["blocks_reused"] == stats["blocks_fetched"] == 0
    assert stats["bytes"] == stats["bytes_reused"] == stats["reuse_retried"] == 0
    assert stats["files"] == tree["st0"]["files"] and stats["directories"] == tree["st0"]["directories"]
    assert {rel: os.lstat(root / "src" / rel).st_ino for rel in inodes} == inodes
    _check_tree(tree, root)


def test_one_byte_flipped_fetches_one_block(engine, oracle, tree):
    root = _copy(tree, "flip")
    data = tree["content"][BIG_A]
    _rewrite(root / "src" / BIG_A, _flip(data, len(data) * 2 // 3))
    kept, fetch = _model(oracle, tree, root)
    chain = tree["data_ids"][BIG_A]
    assert len(kept) == tree["n_data_files"] - 1 and len(fetch) == 1 and fetch < set(chain)
    inodes = {rel: os.lstat(root / "src" / rel).st_ino for rel in kept}
    stats, data_read, s = _restore(engine, tree, root, reuse_local=True)
    assert data_read == fetch and all(s.reads[i] == 1 for i in fetch)
    assert stats["kept"] == len(kept) and stats["blocks_fetched"] == 1 and stats["reuse_retried"] == 0
    assert stats["blocks_reused"] == len(chain) - 1 and stats["bytes"] == len(data)
    assert stats["bytes_reused"] == len(data) - len(_block_bytes(tree, next(iter(fetch))))
    assert {rel: os.lstat(root / "src" / rel).st_ino for rel in kept} == inodes  # the others are untouched
    _check_tree(tree, root)
    # keep_matching alone fetches the whole file
    root2 = _copy(tree, "flip_km")
    _rewrite(root2 / "src" / BIG_A, _flip(data, len(data) * 2 // 3))
    _stats, data_read, _ = _restore(engine, tree, root2, keep_matching=True)
    assert data_read == set(chain)


def _block_bytes(tree, bid) -> bytes:
    ty, data, _links = tree["blocks"][bid]
    return data if ty == RAW else zlib.decompress(data)


def test_one_byte_inserted_at_the_front(engine, oracle, tree):
    root = _copy(tree, "insert")
    data = tree["content"][BIG_B]
    _rewrite(root / "src" / BIG_B, b"\x5a" + data)
    chain = tree["data_ids"][BIG_B]
    # the oracle confirms that the cuts resynchronise: the local file still holds most of the chain's blocks
    local = _oracle_ids(oracle, root / "src" / BIG_B)
    assert local != chain and 0 < len(set(chain) - set(local)) < len(chain) // 2
    kept, fetch = _model(oracle, tree, root)
    assert BIG_B not in kept and fetch == set(chain) - set(local)
    stats, data_read, _ = _restore(engine, tree, root, reuse_local=True)
    assert data_read == fetch and len(data_read) < len(chain)
    assert stats["blocks_fetched"] == len(fetch) and stats["blocks_reused"] == len(chain) - len(fetch)
    assert stats["kept"] == tree["n_data_files"] - 1 and stats["bytes"] == len(data)
    _check_tree(tree, root)


def test_deleted_file_with_a_copy_elsewhere(engine, oracle, tree):
    root = _copy(tree, "moved")
    aside = tree["tmp"] / "aside.bin"
    os.replace(root / "src" / BIG_A, aside)
    other = tree["tmp"] / "unrelated.bin"
    other.write_bytes(b"nothing the tree holds" * 5000)
    before = (aside.read_bytes(), os.lstat(aside).st_mtime_ns)
    extras = [aside, other, tree["tmp"] / "not_there"]
    kept, fetch = _model(oracle, tree, root, extras[:2])
    assert len(kept) == tree["n_data_files"] - 1 and fetch == set()
    stats, data_read, _ = _restore(engine, tree, root, reuse_local=True, reuse_paths=extras)
    assert data_read == set()
    assert stats["blocks_fetched"] == 0 and stats["blocks_reused"] == len(tree["data_ids"][BIG_A])
    assert stats["bytes"] == stats["bytes_reused"] == len(tree["content"][BIG_A])
    assert (aside.read_bytes(), os.lstat(aside).st_mtime_ns) == before  # only read
    _check_tree(tree, root)
    # without the copy the whole file is fetched
    root2 = _copy(tree, "moved_plain")
    os.remove(root2 / "src" / BIG_A)
    _stats, data_read, _ = _restore(engine, tree, root2, reuse_local=True)
    assert data_read == set(tree["data_ids"][BIG_A])
    _check_tree(tree, root2)


def test_two_files_with_exchanged_contents(engine, oracle, tree):
    root = _copy(tree, "swap")
    _rewrite(root / "src" / BIG_A, tree["content"][BIG_B])
    _rewrite(root / "src" / BIG_B, tree["content"][BIG_A])
    kept, fetch = _model(oracle, tree, root)
    assert len(kept) == tree["n_data_files"] - 2 and fetch == set()
    stats, data_read, _ = _restore(engine, tree, root, reuse_local=True)
    assert data_read == set()
    assert stats["blocks_fetched"] == 0
    assert stats["blocks_reused"] == len(tree["data_ids"][BIG_A]) + len(tree["data_ids"][BIG_B])
    assert stats["bytes"] == len(tree["content"][BIG_A]) + len(tree["content"][BIG_B])
    _check_tree(tree, root)


def test_local_file_rewritten_after_hashing(engine, oracle, tree):
    """The store rewrites a later file (same size) during the first data-block
    read of an earlier one: the later file's reused chunks no longer carry
    their IDs, VerifyBlock refuses them, and that file is restored from the
    store."""
    root = _copy(tree, "stale")
    early, late = "f00", BIG_B  # a file of the top directory comes before any file of a directory below it
    _rewrite(root / "src" / early, _flip(tree["content"][early], 0))
    _rewrite(root / "src" / late, _flip(tree["content"][late], 0))
    s = Store(tree["blocks"])
    junk = bytes(np.random.default_rng(9).integers(0, 256, len(tree["content"][late]), dtype=np.uint8))
    s.hook[tree["data_ids"][early][0]] = lambda: _rewrite(root / "src" / late, junk)
    stats, data_read, _ = _restore(engine, tree, root, store=s, reuse_local=True)
    assert not s.hook  # it ran
    assert stats["reuse_retried"] == 1 and stats["kept"] == tree["n_data_files"] - 2
    assert data_read == set(tree["data_ids"][early]) | set(tree["data_ids"][late])
    assert stats["bytes"] == len(tree["content"][early]) + len(tree["content"][late])
    assert stats["blocks_reused"] == 0  # only what ended up in a good file counts
    _check_tree(tree, root)


def test_corrupt_fetched_block_leaves_the_old_files(engine, oracle, tree):
    from hashbox_amd import HbxError
    root = _copy(tree, "corrupt")
    data = tree["content"][BIG_A]
    _rewrite(root / "src" / BIG_A, _flip(data, len(data) * 2 // 3))
    _rewrite(root / "src" / BIG_B, b"\x5a" + tree["content"][BIG_B])
    _kept, fetch = _model(oracle, tree, root)
    victim = next(i for i in tree["data_ids"][BIG_A] if i in fetch)
    blocks = dict(tree["blocks"])
    ty, blob, links = blocks[victim]
    blocks[victim] = (ty, blob[:len(blob) // 2], links)
    before = _snapshot(root)
    with pytest.raises(HbxError, match=victim.hex()):
        _restore(engine, tree, root, store=Store(blocks), reuse_local=True)
    after = _snapshot(root)
    assert after.pop("src/link") == ("link", "d1/f01")  # (made during the walk, before any data is read)
    # (an entry of FileSize 0 is created in the walk, as in every restore: its bytes and mode stay, its time moves)
    assert after["src/empty"][:2] + after["src/empty"][3:] == before["src/empty"][:2] + before["src/empty"][3:]
    after["src/empty"] = before["src/empty"]
    assert after == before  # old content, old ModTimes, no temporaries
    os.remove(root / "src" / "link")
    # and with the good store the same tree restores
    _stats, data_read, _ = _restore(engine, tree, root, reuse_local=True)
    assert data_read == fetch
    _check_tree(tree, root)


def test_defaults_unchanged(engine, tree):
    from hashbox_amd import formats as F
    with pytest.raises(ValueError, match="batch"):
        F.restore_tree(engine, tree["t"].root, Store(tree["blocks"]).read_block, tree["tmp"] / "nowhere",
                       reuse_local=True)
    assert not (tree["tmp"] / "nowhere").exists()
    root = _copy(tree, "defaults")
    data = tree["content"][BIG_A]
    _rewrite(root / "src" / BIG_A, _flip(data, 5))
    stats, data_read, _ = _restore(engine, tree, root, keep_matching=True)
    assert set(stats) == {"files", "directories", "bytes", "kept"}
    assert data_read == set(tree["data_ids"][BIG_A]) and stats["kept"] == tree["n_data_files"] - 1
    _check_tree(tree, root)
    plain = tree["tmp"] / "defaults_plain"
    plain.mkdir()
    stats, data_read, s = _restore(engine, tree, plain)
    assert stats == tree["st0"] and set(stats) == {"files", "directories", "bytes"}
    assert data_read == tree["all_data"] and all(s.reads[i] == 1 for i in tree["all_data"])
    _check_tree(tree, plain)
