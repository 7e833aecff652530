"""CPU: the block-ID set's C-ABI (include/hbxgpu.h, hbx_idset_*): the pure
slot-count helper, the argument checks that need no device, and the Python
name.  The kernels are checked on a GPU by tests/test_gpu_idset.py."""
import ctypes

import pytest

ERR_ARG = -1


def _L():
    from hashbox_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("capacity,slots", [(1, 64), (31, 64), (32, 64), (33, 128), (1 << 20, 1 << 21),
                                            (1 << 31, 1 << 32), ((1 << 31) + 1, 0), (1 << 40, 0)])
def test_idset_slots(capacity, slots):
    """S = the smallest power of two >= 2 C, at least 64; 0 above 2^31."""
    assert _L().hbx_idset_slots(capacity) == slots


def test_null_context_is_an_argument_error():
    L = _L()
    h = ctypes.c_void_p()
    n = ctypes.c_uint64(0)
    buf = (ctypes.c_uint8 * 16)()
    flag = (ctypes.c_uint8 * 1)()
    some = ctypes.c_void_p(1)  # never dereferenced: the context is checked first
    assert L.hbx_idset_create(None, 16, ctypes.byref(h)) == ERR_ARG
    assert L.hbx_idset_destroy(None, some) == ERR_ARG
    assert L.hbx_idset_insert(None, some, 1, buf, flag) == ERR_ARG
    assert L.hbx_idset_contains(None, some, 1, buf, flag) == ERR_ARG
    assert L.hbx_idset_stats(None, some, ctypes.byref(n), None, None, None) == ERR_ARG
    assert L.hbx_idset_export(None, some, buf, 1, ctypes.byref(n)) == ERR_ARG
    assert L.hbx_idset_truncate(None, some, 0) == ERR_ARG
    assert L.hbx_submit_device_dd(None, None, 0, None, None, None, None, None, None, None, some, flag) == ERR_ARG
    assert L.hbx_store_paths_dd(None, 0, None, None, None, None, None, None, None, None, 1, 0, None, None, None,
                                None, None, None, some, flag) == ERR_ARG


def test_python_name():
    from hashbox_amd import IdSet, FileChunks
    assert callable(IdSet.insert) and callable(IdSet.contains) and callable(IdSet.export)
    assert "fresh" in FileChunks.__slots__
