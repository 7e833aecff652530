"""Restore and diff of a block chain (hbx_restore_blocks,
hbx_restore_file_stream): the parts that need no GPU.  The ABI surface, the
argument checks that return before the context is touched, and the bound on a
block's data field.  tests/test_gpu_restore.py runs the path on the device.
"""
import ctypes
import inspect
import os
import re
import subprocess

from hashbox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NEW_FUNCTIONS = ["hbx_restore_in_bound", "hbx_restore_blocks", "hbx_restore_file_stream"]


def test_header_declares_the_restore_interface():
    src = open(os.path.join(ROOT, "include", "hbxgpu.h")).read()
    assert re.search(r"\buint64_t\s+hbx_restore_in_bound\s*\(\s*uint64_t\s+max_block\s*\)", src)
    for name in NEW_FUNCTIONS[1:]:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert re.search(r"#define\s+HBX_BLOCK_RAW\s+0xff\b", src)
    assert re.search(r"#define\s+HBX_BLOCK_ZLIB\s+0x01\b", src)
    assert re.search(r"#define\s+HBX_MAX_BLOCK\s+\(8u\s*<<\s*20\)", src)
    assert re.search(r"#define\s+HBX_ERR_VERIFY\s+\(-9\)", src)
    assert re.search(r"typedef\s+int\s*\(\*hbx_block_source_fn\)\(void\s*\*user,\s*uint64_t\s+index,\s*uint8_t\s*\*dst,"
                     r"\s*uint64_t\s+cap,\s*uint64_t\s*\*len,\s*uint8_t\s*\*type\)", src)
    assert re.search(r"typedef\s+int\s*\(\*hbx_restore_sink_fn\)\(void\s*\*user,\s*uint64_t\s+file_off,"
                     r"\s*const\s+uint8_t\s*\*data,\s*uint64_t\s+len\)", src)
    # the inflate call's comment points to the call that needs no sizes in advance
    inflate_doc = src.split("int hbx_inflate_blocks_device(")[0].rsplit("/*", 1)[1]
    assert "hbx_restore_blocks" in inflate_doc
    # every entry point names the reference lines it replaces
    restore_doc = src.split("uint64_t hbx_restore_in_bound(")[0].rsplit("#define HBX_BLOCK_RAW", 1)[0][-2000:]
    assert "restore.go:45-66" in restore_doc and "restore.go:249-277" in restore_doc


def test_library_exports_and_binding_lists_them():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = set(re.findall(r"\sT\s+(hbx_[a-z0-9_]+)$", out, flags=re.M))
    L = _lib.load()
    for name in NEW_FUNCTIONS:
        assert name in exported, name
        assert name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    assert _lib.ERRORS[-9] == "HBX_ERR_VERIFY"
    assert (_lib.BLOCK_RAW, _lib.BLOCK_ZLIB, _lib.MAX_BLOCK) == (0xFF, 0x01, 8 << 20)
    assert len(L.hbx_restore_blocks.argtypes) == 18 and len(L.hbx_restore_file_stream.argtypes) == 14


def test_k10_is_part_of_the_build():
    from hashbox_amd import build
    assert "hbx_restore.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "hbx_restore.hip"))
    eng = open(os.path.join(build.CSRC, "hbx_engine.hip")).read()
    assert '#include "hbx_restore.hip"' in eng
    k10 = open(os.path.join(build.CSRC, "hbx_restore.hip")).read()
    for kernel in ("hbx_k10_gather", "hbx_k10_diff"):
        assert re.search(r"__global__[^;{]*\b%s\b" % kernel, k10), kernel
        assert kernel in eng, kernel


def test_in_bound():
    L = _lib.load()
    assert L.hbx_restore_in_bound(0) == L.hbx_restore_in_bound(_lib.MAX_BLOCK)
    assert L.hbx_restore_in_bound(0) >= L.hbx_deflate_bound(_lib.MAX_BLOCK)
    for mb in (1, 65536, 1 << 20, _lib.MAX_BLOCK):
        assert L.hbx_restore_in_bound(mb) >= max(mb, L.hbx_deflate_bound(mb))
    assert L.hbx_restore_in_bound(65536) < L.hbx_restore_in_bound(1 << 20)


def test_python_mirror():
    from hashbox_amd import Engine, RestoredBlocks, RestoreError, HbxError, formats
    p = inspect.signature(Engine.restore_blocks).parameters
    assert list(p)[:4] == ["self", "datas", "types", "ids"]
    assert [p[k].default for k in ("links", "local", "max_block")] == [None, None, None]
    p = inspect.signature(Engine.restore_file).parameters
    assert list(p)[:3] == ["self", "ids", "source"]
    assert [p[k].default for k in ("out_path", "on_data", "window_bytes")] == [None, None, 0]
    assert list(inspect.signature(Engine.diff_file).parameters)[:4] == ["self", "ids", "source", "local_path"]
    assert list(inspect.signature(formats.restore_tree).parameters)[:4] == ["eng", "root_entry", "read_block", "dest"]
    assert [f for f in RestoredBlocks.__dataclass_fields__] == ["data", "offs", "status", "n_good", "first_diff"]
    assert issubclass(RestoreError, HbxError)


def test_contradictory_arguments_return_before_the_context_is_touched():
    """out and local both set, no target at all, and (for the stream) two
    targets are HBX_ERR_ARG whatever the context is: the checks read no byte
    of it (the stand-in context here is a zeroed buffer, never a real one)."""
    L = _lib.load()
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    buf = ctypes.create_string_buffer(64)
    bufp = ctypes.cast(buf, ctypes.c_void_p)
    offs = (ctypes.c_uint64 * 2)()
    status = (ctypes.c_uint32 * 1)()
    good, first = ctypes.c_uint64(), ctypes.c_uint64()

    def blocks(c, out, local):
        return L.hbx_restore_blocks(c, 0, None, None, None, None, None, None, None, 0, out, 64 if out else 0,
                                    local, 64 if local else 0, offs, status, ctypes.byref(good), ctypes.byref(first))
    assert blocks(None, bufp, None) == ERR_ARG  # NULL context
    assert blocks(ctx, bufp, bufp) == ERR_ARG  # both
    assert blocks(ctx, None, None) == ERR_ARG  # neither
    # blocks without their arrays
    assert L.hbx_restore_blocks(ctx, 1, None, None, None, None, None, None, None, 0, bufp, 64, None, 0, offs, status,
                                ctypes.byref(good), ctypes.byref(first)) == ERR_ARG
    # a max_block whose lengths would not fit the kernels' 32-bit fields
    assert L.hbx_restore_blocks(ctx, 0, None, None, None, None, None, None, None, 1 << 40, bufp, 64, None, 0, offs,
                                status, ctypes.byref(good), ctypes.byref(first)) == ERR_ARG

    src = _lib.BLOCK_SOURCE(lambda user, i, dst, cap, ln, ty: 1)
    sink = _lib.RESTORE_SINK(lambda user, off, data, ln: 1)
    srcp, sinkp = ctypes.cast(src, ctypes.c_void_p), ctypes.cast(sink, ctypes.c_void_p)
    n = ctypes.c_uint64()

    def stream(c, out_path, sk, local_path, source=srcp, ids=bufp):
        return L.hbx_restore_file_stream(c, 1, ids, source, None, 0, out_path, sk, local_path, 0, ctypes.byref(n),
                                         None, None, ctypes.byref(first))
    assert stream(None, b"/nonexistent/x", None, None) == ERR_ARG
    assert stream(ctx, None, None, None) == ERR_ARG  # no target
    assert stream(ctx, b"/nonexistent/x", sinkp, None) == ERR_ARG  # two targets
    assert stream(ctx, b"/nonexistent/x", None, b"/nonexistent/y") == ERR_ARG
    assert stream(ctx, None, sinkp, b"/nonexistent/y") == ERR_ARG
    assert stream(ctx, b"/nonexistent/x", sinkp, b"/nonexistent/y") == ERR_ARG
    assert stream(ctx, None, sinkp, None, source=None) == ERR_ARG  # blocks without a source
    assert stream(ctx, None, sinkp, None, ids=None) == ERR_ARG
    assert fake.raw == bytes(1 << 16)
    assert not os.path.exists("/nonexistent")
