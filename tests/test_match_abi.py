"""CPU: the C-ABI and the Python names of the match by block ID (K12,
include/hbxgpu.h: hbx_match_chains, hbx_submit_device_match,
hbx_store_paths_match).  No compute call is made: every call here is refused
for its arguments before a context is touched."""
import ctypes
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBX_ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    from hashbox_amd import _lib
    return _lib.load()


def test_declared_exported_and_bound(L):
    from hashbox_amd import _lib
    src = open(os.path.join(ROOT, "include", "hbxgpu.h")).read()
    for name in ("hbx_match_chains", "hbx_submit_device_match", "hbx_store_paths_match"):
        assert f"int {name}(" in src, name
        assert name in _lib.EXPORTS, name
        assert getattr(L, name).restype is ctypes.c_int
        # each names what it short-cuts in the reference
        at = src.index(f"int {name}(")
        comment = src[src.rindex("/*", 0, at):at]
        assert "restore.go:249-277, 317-367" in comment and "diffFileData / diffEntry" in comment, name
    assert len(L.hbx_match_chains.argtypes) == 8
    assert len(L.hbx_submit_device_match.argtypes) == len(L.hbx_submit_device.argtypes) + 3
    assert len(L.hbx_store_paths_match.argtypes) == len(L.hbx_store_paths_status.argtypes) - 6 + 3
    assert "match_push_bytes" in src


def test_record_layout():
    from hashbox_amd import _lib
    R = _lib.ChainMatch
    assert ctypes.sizeof(R) == 32
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == [
        ("n_match", 0, 4), ("n_local", 4, 4), ("n_expect", 8, 4), ("same", 12, 4), ("match_bytes", 16, 8),
        ("reserved", 24, 8)]
    src = open(os.path.join(ROOT, "include", "hbxgpu.h")).read()
    body = src[src.index("typedef struct {\n  uint32_t n_match;"):src.index("} hbx_chain_match;")]
    assert [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln] == [
        "n_match", "n_local", "n_expect", "same", "match_bytes", "reserved"]


def test_null_context_is_an_argument_error(L):
    from hashbox_amd import _lib
    one = np.array([0, 1], np.uint64)
    ids = np.zeros((1, 16), np.uint8)
    rec = (_lib.ChainMatch * 1)()
    p = lambda a: a.ctypes.data
    assert L.hbx_match_chains(None, 1, p(one), p(ids), None, p(one), p(ids), rec) == HBX_ERR_ARG
    assert L.hbx_match_chains(None, 0, None, None, None, None, None, None) == HBX_ERR_ARG
    sums = (_lib.FileSummary * 1)()
    lens = np.array([10], np.uint64)
    offs = np.array([0], np.uint64)
    # with every other argument in order, without a match array, without the IDs, with a chain of 2^32 IDs
    huge = np.array([0, 1 << 32], np.uint64)
    for first, eids, match in ((one, ids, rec), (one, ids, None), (one, None, rec), (huge, ids, rec),
                               (None, None, None)):
        args = (p(first) if first is not None else None, p(eids) if eids is not None else None, match)
        assert L.hbx_submit_device_match(None, None, 1, p(offs), p(lens), None, None, None, None, sums,
                                         *args) == HBX_ERR_ARG
        path = (ctypes.c_char_p * 1)(b"/nonexistent")
        assert L.hbx_store_paths_match(None, 1, ctypes.cast(path, ctypes.c_void_p), p(lens), None, None, None, None,
                                       sums, None, 4, 1 << 20, *args) == HBX_ERR_ARG


def test_python_names():
    import hashbox_amd
    from hashbox_amd import ChainMatch, Engine, formats
    assert "ChainMatch" in hashbox_amd.__all__
    assert ChainMatch.__slots__ == ("same", "n_match", "n_local", "n_expect", "match_bytes", "errno", "content_type",
                                    "content_id", "chunks")
    assert list(inspect.signature(Engine.match_chains).parameters) == ["self", "local_ids", "expect_ids",
                                                                       "local_cut_ends"]
    mp = inspect.signature(Engine.match_paths).parameters
    assert list(mp) == ["self", "paths", "chains_ids", "io_threads", "batch_bytes", "sizes", "skip_unreadable",
                        "chunks"]
    assert (mp["io_threads"].default, mp["batch_bytes"].default, mp["sizes"].default,
            mp["skip_unreadable"].default, mp["chunks"].default) == (16, 1 << 30, None, False, False)
    assert list(inspect.signature(Engine.submit_device_match).parameters)[:5] == ["self", "d_arena", "offs", "lens",
                                                                                  "chains_ids"]
    assert inspect.signature(formats.diff_tree).parameters["by_id"].default is False
    assert inspect.signature(formats.restore_tree).parameters["keep_matching"].default is False


def test_keep_matching_needs_batch(tmp_path):
    from hashbox_amd import formats
    root = formats.FileEntry(file_name=b"x")
    with pytest.raises(ValueError, match="batch"):
        formats.restore_tree(None, root, lambda bid: None, tmp_path, keep_matching=True)
    assert not os.listdir(tmp_path)  # refused before anything is created


def test_listed_in_the_build_sources():
    from hashbox_amd import build
    assert "hbx_match.hip" in build.SOURCES
    eng = open(os.path.join(ROOT, "hashbox_amd", "csrc", "hbx_engine.hip")).read()
    assert '#include "hbx_match.hip"' in eng
