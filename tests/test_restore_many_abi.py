"""Restore and diff of many files in one call (hbx_restore_many_window,
hbx_restore_files_blocks, hbx_restore_files_stream, K11): the parts that need
no GPU.  The ABI surface, K11's place in the build, the window rule against a
Python restatement, and the argument checks that return before the context is
touched.  tests/test_gpu_restore_many.py runs the path on the device.
"""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hashbox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ERR_ARG = -1
NEW_FUNCTIONS = ["hbx_restore_many_window", "hbx_restore_files_blocks", "hbx_restore_files_stream"]
Mi = 1 << 20


def test_header_declares_the_interface():
    src = open(os.path.join(ROOT, "include", "hbxgpu.h")).read()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert re.search(r"typedef\s+int\s*\(\*hbx_file_block_source_fn\)\(void\s*\*user,\s*uint64_t\s+file,"
                     r"\s*uint64_t\s+index,\s*uint8_t\s*\*dst,\s*uint64_t\s+cap,\s*uint64_t\s*\*len,"
                     r"\s*uint8_t\s*\*type\)", src)
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*hbx_restored_file\s*;", src)
    assert struct
    fields = re.findall(r"\b(u?int\d+_t)\s+(\w+)\s*;", struct.group(1))
    assert fields == [("uint64_t", "bytes"), ("uint64_t", "n_good"), ("uint64_t", "bad_index"),
                      ("uint64_t", "first_diff"), ("uint32_t", "bad_status"), ("int32_t", "err")]
    # the binding's struct has the same layout
    assert [(n, ctypes.sizeof(t)) for n, t in _lib.RestoredFile._fields_] == \
        [(n, int(re.search(r"\d+", t).group()) // 8) for t, n in fields]
    assert ctypes.sizeof(_lib.RestoredFile) == 40
    # the entry points name the reference lines they replace, and the memory formula is stated
    doc = src.split("int hbx_restore_many_window(")[0][-4000:]
    assert "restore.go:137-162" in doc and "restore.go:279-414" in doc
    stream_doc = src.split("int hbx_restore_files_stream(")[0][-2500:]
    assert "Memory depends on window_bytes" in stream_doc and "pinned" in stream_doc


def test_library_exports_and_binding_lists_them():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = set(re.findall(r"\sT\s+(hbx_[a-z0-9_]+)$", out, flags=re.M))
    L = _lib.load()
    for name in NEW_FUNCTIONS:
        assert name in exported, name
        assert name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.hbx_restore_many_window.argtypes) == 5
    assert len(L.hbx_restore_files_blocks.argtypes) == 21
    assert len(L.hbx_restore_files_stream.argtypes) == 13


@pytest.fixture(scope="module")
def engine_isa(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_many") / "engine.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(ROOT, "hashbox_amd", "csrc", "hbx_engine.hip")],
                   check=True, capture_output=True, timeout=900)
    return out.read_text()


def test_k11_is_part_of_the_build(engine_isa):
    from hashbox_amd import build
    assert "hbx_restore_many.hip" in build.SOURCES
    eng = open(os.path.join(build.CSRC, "hbx_engine.hip")).read()
    assert '#include "hbx_restore_many.hip"' in eng
    k11 = open(os.path.join(build.CSRC, "hbx_restore_many.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", k11)  # plain HIP C++
    assert re.findall(r"\batomic\w+", re.sub(r"//.*", "", k11)) == ["atomicMin"]
    for kernel in ("hbx_k11_gather", "hbx_k11_diff"):
        assert re.search(r"__global__[^;{]*\b%s\b" % kernel, k11), kernel
        assert kernel in eng, kernel
        i = engine_isa.index(f".name:           {kernel}\n")
        blk = engine_isa[engine_isa.rfind("  - .", 0, i):engine_isa.find("  - .", i)]
        get = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))  # noqa: E731
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, kernel
        assert get("sgpr_spill_count") == 0 and get("group_segment_fixed_size") == 0, kernel  # no LDS either
    # K10 is still there
    assert ".name:           hbx_k10_gather\n" in engine_isa and ".name:           hbx_k10_diff\n" in engine_isa


def window_end(caps, window_bytes, start):
    """The rule restated: block i takes caps[i] rounded up to 256, + 256; the
    window holds what fits window_bytes (0 = 1 GiB), at least one block."""
    wb = window_bytes or (1 << 30)
    total, e = 0, start
    while e < len(caps):
        share = (int(caps[e]) + 255) // 256 * 256 + 256
        if e > start and total + share > wb:
            break
        total += share
        e += 1
    return e


def _windows(L, caps, window_bytes):
    a = np.ascontiguousarray(caps, np.uint64)
    got, start = [], 0
    end = ctypes.c_uint64()
    while start < len(caps):
        assert L.hbx_restore_many_window(len(caps), a.ctypes.data, window_bytes, start, ctypes.byref(end)) == 0
        got.append(int(end.value))
        assert int(end.value) == window_end(caps, window_bytes, start), (start, window_bytes)
        assert int(end.value) > start
        start = int(end.value)
    return got


def test_window_rule_against_a_restatement():
    L = _lib.load()
    ones = [1] * 1000
    assert _windows(L, ones, 0) == [1000]  # 512 bytes each: one window by far
    assert _windows(L, ones, 512 * 100) == list(range(100, 1001, 100))
    assert _windows(L, ones, 512 * 100 + 511) == list(range(100, 1001, 100))
    assert _windows(L, ones, 1) == list(range(1, 1001))  # nothing fits: a block per window
    rng = np.random.default_rng(5)
    mixed = [int(x) for x in rng.integers(1 * Mi, 8 * Mi + 1, 200)]
    for wb in (0, 1 << 30, 64 * Mi, 17 * Mi + 3, 8 * Mi + 512, 8 * Mi):
        ends = _windows(L, mixed, wb)
        assert ends[-1] == 200
    assert len(_windows(L, mixed, 1 << 30)) < len(_windows(L, mixed, 64 * Mi)) < 200
    # one capacity larger than the window: a window of that one block, its neighbours unaffected
    caps = [1000, 1000, 5 * Mi, 1000, 1000]
    assert _windows(L, caps, 1 * Mi) == [2, 3, 5]
    assert _windows(L, [5 * Mi], 1 * Mi) == [1]
    assert _windows(L, [2**64 - 1, 1], 1 * Mi) == [1, 2]  # no overflow in the rounding
    # start == n, and arguments
    a = np.ascontiguousarray(caps, np.uint64)
    end = ctypes.c_uint64(77)
    assert L.hbx_restore_many_window(5, a.ctypes.data, 1 * Mi, 5, ctypes.byref(end)) == 0 and end.value == 5
    assert L.hbx_restore_many_window(0, None, 0, 0, ctypes.byref(end)) == 0 and end.value == 0
    assert L.hbx_restore_many_window(5, a.ctypes.data, 1 * Mi, 6, ctypes.byref(end)) == ERR_ARG
    assert L.hbx_restore_many_window(5, a.ctypes.data, 1 * Mi, 0, None) == ERR_ARG
    assert L.hbx_restore_many_window(5, None, 1 * Mi, 0, ctypes.byref(end)) == ERR_ARG


def test_python_mirror():
    from hashbox_amd import Engine, RestoredFile, RestoredFiles, formats
    p = inspect.signature(Engine.restore_files_blocks).parameters
    assert list(p)[:2] == ["self", "chains"]
    assert [p[k].default for k in ("size_hints", "local", "max_block")] == [None, None, None]
    p = inspect.signature(Engine.restore_files).parameters
    assert list(p)[:4] == ["self", "chains_ids", "source", "out_paths"]
    assert [p[k].default for k in ("size_hints", "window_bytes", "io_threads", "max_block")] == [None, 0, 16, None]
    assert list(inspect.signature(Engine.diff_files).parameters)[:4] == ["self", "chains_ids", "source", "local_paths"]
    p = inspect.signature(formats.restore_tree).parameters
    assert p["batch"].default is False
    assert list(inspect.signature(formats.diff_tree).parameters)[:4] == ["eng", "root_entry", "read_block",
                                                                         "local_root"]
    assert list(RestoredFiles.__dataclass_fields__) == ["data", "out_offs", "blk_offs", "status", "n_good",
                                                        "first_diff"]
    assert list(RestoredFile.__dataclass_fields__) == ["bytes", "n_good", "bad_index", "bad_status", "errno",
                                                       "first_diff"]


def test_contradictory_arguments_return_before_the_context_is_touched():
    """out and local both set or both missing, block lists without their
    arrays, a `first` that does not start at 0 or decreases, two path lists or
    none, more than 16 writers: HBX_ERR_ARG whatever the context is.  The
    stand-in context is a zeroed buffer that must stay zeroed."""
    L = _lib.load()
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    buf = ctypes.create_string_buffer(64)
    bufp = ctypes.cast(buf, ctypes.c_void_p)
    first0 = np.zeros(2, np.uint64)  # one file without blocks
    first1 = np.array([0, 1], np.uint64)  # one file of one block
    offs = np.zeros(2, np.uint64)
    good, fd, st, bo = np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint64)

    def blocks(c, out, local, first=first0, n_files=1, arrays=None, max_block=0, out_offs=offs, local_offs=offs,
               first_diff=fd):
        a = arrays if arrays is not None else (None, None, None, None)
        return L.hbx_restore_files_blocks(
            c, n_files, first.ctypes.data if first is not None else None, a[0], a[1], a[2], a[3], None, None, None,
            None, max_block, out, 64 if out else 0, out_offs.ctypes.data if out_offs is not None else None,
            local, local_offs.ctypes.data if local_offs is not None else None, bo.ctypes.data, st.ctypes.data,
            good.ctypes.data, first_diff.ctypes.data if first_diff is not None else None)
    assert blocks(None, bufp, None) == ERR_ARG  # NULL context
    assert blocks(ctx, bufp, bufp) == ERR_ARG  # both
    assert blocks(ctx, None, None) == ERR_ARG  # neither
    assert blocks(ctx, bufp, None, out_offs=None) == ERR_ARG
    assert blocks(ctx, None, bufp, local_offs=None) == ERR_ARG
    assert blocks(ctx, None, bufp, first_diff=None) == ERR_ARG
    assert blocks(ctx, bufp, None, first=None) == ERR_ARG
    assert blocks(ctx, bufp, None, first=np.array([1, 1], np.uint64)) == ERR_ARG  # does not start at 0
    assert blocks(ctx, bufp, None, first=np.array([0, 2, 1], np.uint64), n_files=2) == ERR_ARG  # decreases
    assert blocks(ctx, bufp, None, first=first1) == ERR_ARG  # a block without its arrays
    assert blocks(ctx, bufp, None, max_block=1 << 40) == ERR_ARG
    assert blocks(ctx, None, bufp, local_offs=np.array([5, 1], np.uint64)) == ERR_ARG

    src = _lib.FILE_BLOCK_SOURCE(lambda user, f, i, dst, cap, ln, ty: 1)
    srcp = ctypes.cast(src, ctypes.c_void_p)
    paths = (ctypes.c_char_p * 1)(b"/nonexistent/x")
    nulls = (ctypes.c_char_p * 1)(None)
    res = (_lib.RestoredFile * 1)()

    def stream(c, out_paths, local_paths, first=first1, ids=bufp, source=srcp, io_threads=4, max_block=0,
               results=res):
        return L.hbx_restore_files_stream(c, 1, first.ctypes.data if first is not None else None, ids, source, None,
                                          None, 0, out_paths, local_paths, io_threads, max_block, results)
    assert stream(None, paths, None) == ERR_ARG
    assert stream(ctx, None, None) == ERR_ARG  # no target
    assert stream(ctx, paths, paths) == ERR_ARG  # two targets
    assert stream(ctx, paths, None, source=None) == ERR_ARG  # blocks without a source
    assert stream(ctx, paths, None, ids=None) == ERR_ARG
    assert stream(ctx, paths, None, first=None) == ERR_ARG
    assert stream(ctx, paths, None, first=np.array([3, 4], np.uint64)) == ERR_ARG
    assert stream(ctx, paths, None, io_threads=17) == ERR_ARG
    assert stream(ctx, paths, None, max_block=1 << 40) == ERR_ARG
    assert stream(ctx, paths, None, results=None) == ERR_ARG
    assert stream(ctx, nulls, None) == ERR_ARG  # a file without its path
    assert fake.raw == bytes(1 << 16)
    assert not os.path.exists("/nonexistent")
