"""CPU: the C-ABI and the Python names of the block locator (K13,
include/hbxgpu.h: hbx_locate_ids, hbx_block_loc).  No compute call is made:
every call here is refused for its arguments before a context is touched."""
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
    assert "int hbx_locate_ids(" in src
    assert "hbx_locate_ids" in _lib.EXPORTS
    assert L.hbx_locate_ids.restype is ctypes.c_int
    assert len(L.hbx_locate_ids.argtypes) == 9
    at = src.index("int hbx_locate_ids(")
    decl = src[at:src.index(");", at)]
    assert decl.count(",") == 8
    # the header states the device memory the call takes
    comment = src[src.rindex("/*", 0, at):at]
    assert "16 (np + nw) + 8 np + 8 (n_pool_files + 1) + 4 S + 32 nw" in comment


def test_record_layout():
    from hashbox_amd import _lib
    R = _lib.BlockLoc
    assert ctypes.sizeof(R) == 32
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == [
        ("file", 0, 4), ("chunk", 4, 4), ("off", 8, 8), ("len", 16, 8), ("reserved", 24, 8)]
    src = open(os.path.join(ROOT, "include", "hbxgpu.h")).read()
    body = src[src.index("typedef struct {\n  uint32_t file;"):src.index("} hbx_block_loc;")]
    assert [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln] == [
        "file", "chunk", "off", "len", "reserved"]
    assert _lib.NO_FILE == 0xFFFFFFFF


def test_argument_errors_with_a_null_context(L):
    from hashbox_amd import _lib
    p = lambda a: a.ctypes.data
    first = np.array([0, 1], np.uint64)
    ids = np.zeros((1, 16), np.uint8)
    cuts = np.array([10], np.uint64)
    rec = (_lib.BlockLoc * 1)()
    found = ctypes.c_uint64(77)
    fb = ctypes.byref(found)
    call = L.hbx_locate_ids
    # a NULL context, with everything else in order; with nothing to do; with n_found NULL
    assert call(None, 1, p(first), p(ids), p(cuts), 1, p(ids), rec, fb) == HBX_ERR_ARG
    assert call(None, 0, None, None, None, 0, None, None, None) == HBX_ERR_ARG
    assert call(None, 1, p(first), p(ids), p(cuts), 1, p(ids), rec, None) == HBX_ERR_ARG
    # a NULL required array while its count is non-zero
    assert call(None, 1, None, p(ids), p(cuts), 1, p(ids), rec, fb) == HBX_ERR_ARG
    assert call(None, 1, p(first), None, p(cuts), 1, p(ids), rec, fb) == HBX_ERR_ARG
    assert call(None, 1, p(first), p(ids), None, 1, p(ids), rec, fb) == HBX_ERR_ARG
    assert call(None, 1, p(first), p(ids), p(cuts), 1, None, rec, fb) == HBX_ERR_ARG
    # a NULL loc with n_want > 0
    assert call(None, 1, p(first), p(ids), p(cuts), 1, p(ids), None, fb) == HBX_ERR_ARG
    # running counts that decrease
    down = np.array([0, 2, 1], np.uint64)
    two = np.zeros((2, 16), np.uint8)
    assert call(None, 2, p(down), p(two), p(np.array([1, 2], np.uint64)), 1, p(ids), rec, fb) == HBX_ERR_ARG
    # more than 2^31 - 1 pool files, more than 2^30 pool IDs, more than 2^32 - 1 wanted IDs (nothing is read
    # past the counts' own arrays before the refusal)
    assert call(None, 1 << 31, p(first), p(ids), p(cuts), 1, p(ids), rec, fb) == HBX_ERR_ARG
    huge = np.array([0, (1 << 30) + 1], np.uint64)
    assert call(None, 1, p(huge), p(ids), p(cuts), 1, p(ids), rec, fb) == HBX_ERR_ARG
    assert call(None, 1, p(first), p(ids), p(cuts), 1 << 32, p(ids), rec, fb) == HBX_ERR_ARG
    assert found.value == 77  # never written


def test_python_names():
    from hashbox_amd import Engine, formats
    assert list(inspect.signature(Engine.locate_ids).parameters) == ["self", "pool_ids", "pool_cut_ends", "want_ids"]
    rp = inspect.signature(formats.restore_tree).parameters
    assert rp["reuse_local"].default is False and tuple(rp["reuse_paths"].default) == ()
    assert rp["keep_matching"].default is False and rp["batch"].default is False


def test_reuse_local_needs_batch(tmp_path):
    from hashbox_amd import formats
    root = formats.FileEntry(file_name=b"x")
    with pytest.raises(ValueError, match="batch"):
        formats.restore_tree(None, root, lambda bid: None, tmp_path, reuse_local=True)
    assert not os.listdir(tmp_path)  # refused before anything is created


def test_listed_in_the_build_sources():
    from hashbox_amd import build
    assert "hbx_locate.hip" in build.SOURCES
    eng = open(os.path.join(ROOT, "hashbox_amd", "csrc", "hbx_engine.hip")).read()
    assert '#include "hbx_locate.hip"' in eng
    k13 = open(os.path.join(ROOT, "hashbox_amd", "csrc", "hbx_locate.hip")).read()
    assert '#include "hbx_dedup.hip"' in k13 and "hbx_k13_build" in k13 and "hbx_k13_lookup" in k13
