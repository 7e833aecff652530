"""Segments with an ID set and the disk-to-sender stream
(hbx_seg_submit_device_dd, hbx_store_file_stream): the parts that need no GPU.
The ABI surface, the argument checks that return before the context is
touched, and the model the GPU tests compare against: a chunk is fresh where
its ID occurs for the first time in oracle.store_file(data).ids, and a
segment completes the chunks tests/test_segmented.model_segmented gives it.
tests/test_gpu_seg_dedup.py runs the same inputs through the engine.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from hashbox_amd import _lib

from .test_segmented import CASES, Mi, make_input, model_segmented

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SEG = 16 * Mi  # HBX_SEG_MIN_BYTES: every test here cuts its file into segments of this size

NEW_FUNCTIONS = ["hbx_seg_submit_device_dd", "hbx_store_file_stream"]

# name -> the K9 flags of the whole file in chunk order (first occurrence of each ID)
FLAGS = {
    "zeros_32Mi": [1, 0, 0, 0],
    "zeros_32Mi+1": [1, 0, 0, 0, 1],
    "tiled_36Mi+777": [1, 1, 0, 0, 1, 1],
    "random_40Mi+1": [1] * 13,
    "rep4": [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1],
}
REP4_BYTES = 50_332_980

_inputs, _whole, _per_seg = {}, {}, {}


def input_bytes(O, name: str) -> np.ndarray:
    """The input's bytes (read-only), made once per process."""
    if name not in _inputs:
        if name == "rep4":
            data = np.concatenate([O.random_bytes(12 * Mi + 333, 41)] * 4)
        else:
            kind, n, seg_bytes, _, _ = CASES[name]
            assert seg_bytes == SEG
            data = make_input(O, kind, n)
        data.flags.writeable = False
        _inputs[name] = data
    return _inputs[name]


def whole(O, name: str):
    """oracle.store_file of the whole input, computed once per process."""
    if name not in _whole:
        _whole[name] = O.store_file(input_bytes(O, name))
    return _whole[name]


def per_segment(O, name: str):
    """Chunks each 16 MiB segment completes."""
    if name not in _per_seg:
        _per_seg[name] = CASES[name][4] if name in CASES else model_segmented(O, input_bytes(O, name), SEG)[1]
    return _per_seg[name]


def first_occurrence(ids: np.ndarray, seen=()) -> list:
    """1 where ids[i] is the first occurrence of an ID not in `seen`."""
    have = {bytes(x) for x in seen}
    out = []
    for row in np.asarray(ids, np.uint8).reshape(-1, 16):
        key = row.tobytes()
        out.append(0 if key in have else 1)
        have.add(key)
    return out


# ------------------------------------------------------------------- ABI --
def test_header_declares_the_stream_interface():
    src = open(os.path.join(ROOT, "include", "hbxgpu.h")).read()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert re.search(r"#define\s+HBX_ERR_SINK\s+\(-8\)", src)
    assert re.search(r"#define\s+HBX_STREAM_COMPRESS\s+1u\b", src)
    assert re.search(r"\}\s*hbx_seg_chunks\s*;", src)
    assert re.search(r"typedef\s+int\s*\(\*hbx_seg_sink_fn\)\(void\s*\*user,\s*const\s+hbx_seg_chunks\s*\*seg\)", src)
    for field in ("first_chunk", "n_chunks", "cut_ends", "ids", "fresh", "zoff", "zlen", "final", "summary"):
        assert re.search(r"\b%s\b" % field, src.split("} hbx_seg_chunks;")[0].rsplit("typedef struct {", 1)[1]), field
    assert "segment batches never touch a set" not in src


def test_library_exports_and_binding_lists_them():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = set(re.findall(r"\sT\s+(hbx_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW_FUNCTIONS:
        assert name in exported, name
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.load(), name).argtypes is not None, name
    assert _lib.ERRORS[-8] == "HBX_ERR_SINK"
    assert _lib.STREAM_COMPRESS == 1


def test_binding_struct_matches_the_header_layout():
    # 8 pointers / u64, an int padded to 8, then the 24-byte summary
    S = _lib.SegChunks
    assert ctypes.sizeof(S) == 8 * 8 + 8 + 24
    assert S.final.offset == 64 and S.summary.offset == 68
    assert ctypes.sizeof(_lib.FileSummary) == 24


def test_python_mirror_takes_the_new_arguments():
    import inspect
    from hashbox_amd import Engine, SegmentChunks
    p = inspect.signature(Engine.store_file).parameters
    assert [p[k].default for k in ("compress", "dedup", "on_segment")] == [False, None, None]
    assert inspect.signature(Engine.seg_submit_device).parameters["dedup"].default is None
    assert [f for f in SegmentChunks.__dataclass_fields__] == ["first_chunk", "chunks", "final"]
    assert "not memory-bounded" in " ".join(Engine.store_file.__doc__.lower().split())


def test_null_arguments_return_before_any_device_call():
    L = _lib.load()
    one = (ctypes.c_uint64 * 1)(0)
    s = _lib.FileSummary()
    assert L.hbx_seg_submit_device_dd(None, 1, None, None, one, one, None, None, one, one, None, None, None) == ERR_ARG
    assert L.hbx_store_file_stream(None, b"/nonexistent", 0, SEG, 1, 0, None, None, None, ctypes.byref(s)) == ERR_ARG


def test_stream_argument_checks_come_before_the_context_is_touched():
    """A NULL path, a bad segment size, unknown flags and compression without a
    sink are HBX_ERR_ARG whatever the context is: the checks read no byte of
    it (the stand-in context here is a zeroed buffer, never a real one)."""
    L = _lib.load()
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    sink = _lib.SEG_SINK(lambda user, seg: 0)
    sinkp = ctypes.cast(sink, ctypes.c_void_p)
    call = L.hbx_store_file_stream
    assert call(ctx, None, 0, SEG, 1, 0, None, sinkp, None, None) == ERR_ARG
    for bad in (SEG - 16, 0, SEG + 8):  # below HBX_SEG_MIN_BYTES; not a multiple of 16
        assert call(ctx, b"/nonexistent", 64 * Mi, bad, 1, 0, None, sinkp, None, None) == ERR_ARG
    assert call(ctx, b"/nonexistent", 64 * Mi, SEG, 1, _lib.STREAM_COMPRESS, None, None, None, None) == ERR_ARG
    assert call(ctx, b"/nonexistent", 64 * Mi, SEG, 1, 2, None, sinkp, None, None) == ERR_ARG
    assert fake.raw == bytes(1 << 16)


# -------------------------------------------------------------- the model --
@pytest.mark.parametrize("name", list(FLAGS))
def test_model_flags_and_segment_counts(oracle, name):
    data, ref = input_bytes(oracle, name), whole(oracle, name)
    assert first_occurrence(ref.ids) == FLAGS[name]
    counts = per_segment(oracle, name)
    assert sum(counts) == ref.n_chunks == len(FLAGS[name])
    if name in CASES:
        assert counts == CASES[name][4] and data.size == CASES[name][1]
    else:
        assert data.size == REP4_BYTES and ref.n_chunks == 16
        cuts, _ = model_segmented(oracle, data, SEG)
        assert np.array_equal(cuts, ref.cut_ends)


def test_the_inputs_cover_the_duplicate_kinds(oracle):
    """Duplicates inside one segment, across segments, and of real content."""
    def seg_of_chunk(name):
        return [j for j, k in enumerate(per_segment(oracle, name)) for _ in range(k)]
    z = seg_of_chunk("zeros_32Mi")  # [0, 0, 1, 2]: chunk 1 repeats chunk 0 within segment 0
    assert z[:2] == [0, 0] and FLAGS["zeros_32Mi"][:2] == [1, 0]
    assert z[2] != z[0] and FLAGS["zeros_32Mi"][2] == 0  # ... and chunk 2 repeats it from another segment
    r = seg_of_chunk("rep4")
    ids = whole(oracle, "rep4").ids
    dup = [i for i, f in enumerate(FLAGS["rep4"]) if not f]
    first = {bytes(x): i for i, x in reversed(list(enumerate(ids)))}
    assert dup and any(r[first[bytes(ids[i])]] < r[i] for i in dup)  # random content, seen in an earlier segment
