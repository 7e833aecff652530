"""Files larger than a batch, streamed in overlapping segments (hbx_seg_*):
the parts that need no GPU.  The ABI surface, the segment layout
(hbx_seg_next), the argument checks that return before any HIP call, and the
segmenting rule itself: a pure-Python model of what the segment cut kernel
does (layout from hbx_seg_next, each cut from the oracle over file[s : s+L]
as store.go:111-166 decides it, the stop rule, the carry) must equal
oracle.store_file over the whole file.  tests/test_gpu_segmented.py runs the
same cases through the engine.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from hashbox_amd import _lib

from . import cut_craft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Mi = 1 << 20
MIN = 64 * 1024
MAX = 8 * Mi
ERR_ARG = -1

NEW_SYMBOLS = ["hbx_seg_next", "hbx_seg_open", "hbx_seg_close", "hbx_seg_submit_device", "hbx_store_file_seg"]

# name -> (input kind, file bytes, segment bytes, chunks, chunks completed per segment);
# the counts were computed from the oracle with the model below
CASES = {
    "zeros_32Mi": ("zeros", 32 * Mi, 16 * Mi, 4, [2, 1, 1]),
    "zeros_32Mi+1": ("zeros", 32 * Mi + 1, 16 * Mi, 5, [2, 1, 1, 1]),
    "zeros_16Mi+1": ("zeros", 16 * Mi + 1, 16 * Mi, 3, [2, 1]),
    "zeros_24Mi+1": ("zeros", 24 * Mi + 1, 16 * Mi, 4, [2, 1, 1]),
    "zeros_24Mi+MIN": ("zeros", 24 * Mi + MIN, 16 * Mi, 4, [2, 1, 1]),
    "zeros_24Mi+2MIN": ("zeros", 24 * Mi + 2 * MIN, 16 * Mi, 4, [2, 1, 1]),
    "zeros_24Mi+2MIN+1": ("zeros", 24 * Mi + 2 * MIN + 1, 16 * Mi, 4, [2, 1, 1]),
    "random_40Mi+1": ("random11", 40 * Mi + 1, 16 * Mi, 13, [3, 1, 1, 3, 5]),
    "random_50Mi+12345": ("random12", 50 * Mi + 12345, 24 * Mi + 4096, 16, [4, 4, 8]),
    "tiled_36Mi+777": ("tiled5", 36 * Mi + 777, 16 * Mi, 6, [2, 1, 1, 2]),
    # zeros with designed cuts (tests/cut_craft.py SEG_FILES; what each achieves: CRAFTED below)
    "craft_exact": ("craft_exact", 24 * Mi + 3 * MIN, 16 * Mi, 6, [2, 1, 3]),
    "craft_slice": ("craft_slice", 26 * Mi + 5, 16 * Mi, 6, [2, 2, 2]),
    "craft_skew": ("craft_skew", 26 * Mi + 5, 16 * Mi + 48, 6, [2, 2, 2]),
}


def make_input(O, kind: str, n: int) -> np.ndarray:
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind.startswith("random"):
        return O.random_bytes(n, int(kind[6:]))
    if kind.startswith("craft"):
        size, build, _ = cut_craft.SEG_FILES[kind]
        assert size == n
        return build()
    assert kind == "tiled5"
    tile = O.random_bytes(4096, 5)
    return np.tile(tile, n // 4096 + 1)[:n].copy()


def seg_layout(file_len: int, seg_bytes: int):
    """Every (offset, length) hbx_seg_next gives for the file."""
    L = _lib.load()
    out, prev = [], 0
    while True:
        off, ln = ctypes.c_uint64(), ctypes.c_uint64()
        assert L.hbx_seg_next(file_len, seg_bytes, prev, ctypes.byref(off), ctypes.byref(ln)) == 0
        out.append((off.value, ln.value))
        prev = off.value + ln.value
        if prev == file_len:
            return out


def model_segmented(O, data: np.ndarray, seg_bytes: int):
    """The rule: per segment (an arena holding file[off : off+len)), start at
    carry - off, cut while s < len and (final or s + MAX <= len), each cut
    being the first cut the oracle makes of arena[s : s + min(MAX, len - s)];
    then carry = off + s.  Returns (absolute cut ends, chunks per segment)."""
    n = data.size
    carry, cuts, per_seg = 0, [], []
    for off, ln in seg_layout(n, seg_bytes):
        arena = data[off:off + ln]
        final = off + ln == n
        s, k = carry - off, 0
        assert 0 <= s <= ln
        if off:
            assert 0 < s <= MAX, "the carried start lies strictly inside the overlap"
        while s < ln and (final or s + MAX <= ln):
            window = arena[s:s + min(MAX, ln - s)]
            s += int(O.store_file(window).cut_ends[0])
            cuts.append(off + s)
            k += 1
        carry = off + s
        per_seg.append(k)
    assert carry == n
    return np.array(cuts, np.uint64), per_seg


# ------------------------------------------------------------------- ABI --
def test_header_declares_the_segment_interface():
    src = open(os.path.join(ROOT, "include", "hbxgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert re.search(r"#define\s+HBX_SEG_OVERLAP\s+HBX_MAX_BLOCK_SIZE\b", src)
    assert re.search(r"#define\s+HBX_SEG_MIN_BYTES\s+\(2u?\s*\*\s*HBX_MAX_BLOCK_SIZE\)", src)
    assert "typedef struct hbx_seg hbx_seg;" in src


def test_library_exports_and_binding_lists_them():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = set(re.findall(r"\sT\s+(hbx_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.load(), name).argtypes is not None, name


def test_python_constants_match_the_header():
    from hashbox_amd import SEG_MIN_BYTES, SEG_OVERLAP
    assert SEG_OVERLAP == MAX and SEG_MIN_BYTES == 2 * MAX


# ---------------------------------------------------------- hbx_seg_next --
def test_seg_next_layouts():
    assert seg_layout(32 * Mi, 16 * Mi) == [(0, 16 * Mi), (8 * Mi, 16 * Mi), (16 * Mi, 16 * Mi)]
    assert seg_layout(16 * Mi + 1, 16 * Mi) == [(0, 16 * Mi), (8 * Mi, 8 * Mi + 1)]
    assert seg_layout(16 * Mi, 16 * Mi) == [(0, 16 * Mi)]
    assert seg_layout(12345, 16 * Mi) == [(0, 12345)]
    assert seg_layout(0, 16 * Mi) == [(0, 0)]
    assert seg_layout(50 * Mi + 12345, 24 * Mi + 4096) == [
        (0, 24 * Mi + 4096), (16 * Mi + 4096, 24 * Mi + 4096), (32 * Mi + 8192, 18 * Mi + 12345 - 8192)]


def test_seg_next_through_the_engine_class():
    from hashbox_amd import Engine
    assert Engine.seg_next(32 * Mi, 16 * Mi) == (0, 16 * Mi)
    assert Engine.seg_next(32 * Mi, 16 * Mi, 16 * Mi) == (8 * Mi, 16 * Mi)
    with pytest.raises(ValueError):
        Engine.seg_next(32 * Mi, 16 * Mi, 32 * Mi)


@pytest.mark.parametrize("file_len,seg_bytes,prev_end", [
    (64 * Mi, 16 * Mi - 16, 0),   # below HBX_SEG_MIN_BYTES
    (64 * Mi, 0, 0),
    (64 * Mi, 16 * Mi + 8, 0),    # not a multiple of HBX_ARENA_ALIGN
    (32 * Mi, 16 * Mi, 32 * Mi),  # nothing is left
    (32 * Mi, 16 * Mi, 33 * Mi),
])
def test_seg_next_refusals(file_len, seg_bytes, prev_end):
    L = _lib.load()
    off, ln = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.hbx_seg_next(file_len, seg_bytes, prev_end, ctypes.byref(off), ctypes.byref(ln)) == ERR_ARG


def test_null_arguments_return_before_any_device_call():
    L = _lib.load()
    off = ctypes.c_uint64()
    h = ctypes.c_void_p()
    one = (ctypes.c_uint64 * 1)(0)
    s = _lib.FileSummary()
    assert L.hbx_seg_next(32 * Mi, 16 * Mi, 0, None, ctypes.byref(off)) == ERR_ARG
    assert L.hbx_seg_next(32 * Mi, 16 * Mi, 0, ctypes.byref(off), None) == ERR_ARG
    assert L.hbx_seg_open(None, 32 * Mi, ctypes.byref(h)) == ERR_ARG
    assert L.hbx_seg_close(None, None) == ERR_ARG
    assert L.hbx_seg_submit_device(None, 1, None, None, one, one, None, None, one, one, None) == ERR_ARG
    assert L.hbx_store_file_seg(None, b"/nonexistent", 0, 16 * Mi, 1, None, None, 0, ctypes.byref(s)) == ERR_ARG


# ---------------------------------------------------------------- the rule --
@pytest.fixture(scope="module")
def whole(oracle):
    """oracle.store_file of each case's whole file, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            kind, n, _, _, _ = CASES[name]
            cache[name] = oracle.store_file(make_input(oracle, kind, n))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_segment_rule_equals_whole_file(oracle, whole, name):
    kind, n, seg_bytes, chunks, per_seg = CASES[name]
    want = whole(name)
    assert want.n_chunks == chunks
    cuts, got_per_seg = model_segmented(oracle, make_input(oracle, kind, n), seg_bytes)
    assert np.array_equal(cuts, want.cut_ends)
    assert got_per_seg == per_seg
    assert sum(per_seg) == chunks


# what the crafted files are designed to achieve, per chunk: chunk index ->
# (segment it is cut in, properties); a chunk's slices are relative to the
# arena of the segment that cuts it
CRAFTED = {
    "craft_exact": {1: (0, ["starts at len - MAX: continue", "qb+1 peak in the next segment's bytes"]),
                    3: (2, ["previous start one past len - MAX: stop and carry", "resumed", "winner at qa = MIN"])},
    "craft_slice": {2: (1, ["resumed", "winner at slice position 0"]),
                    4: (2, ["resumed", "winner at slice position 4095"])},
    "craft_skew": {2: (1, ["resumed", "winner at slice position 0", "arena slices skewed"]),
                   4: (2, ["resumed", "winner at slice position 4095", "arena slices skewed"])},
}


@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_segment_cases_achieve_what_they_state(oracle, whole, name):
    kind, n, seg_bytes, _, per_seg = CASES[name]
    data = make_input(oracle, kind, n)
    cuts = [int(c) for c in whole(name).cut_ends]
    assert cuts == list(cut_craft.SEG_FILES[kind][2]), "not the designed cuts"
    layout = seg_layout(n, seg_bytes)
    first = np.cumsum([0] + per_seg)  # index of the first chunk each segment cuts
    D = oracle.digest_all(data)
    starts = [0] + cuts[:-1]
    for i, (seg, props) in CRAFTED[name].items():
        off, ln = layout[seg]
        assert first[seg] <= i < first[seg + 1]
        r = cut_craft.Range(D[:off + ln], starts[i], off + ln if seg + 1 < len(layout) else n, off)
        assert r.cut == cuts[i] and r.tied.size == 1 and r.cut != r.s + r.L
        for p in props:
            if p == "resumed":
                assert i == first[seg] and seg > 0 and 0 < r.s - off <= MAX
            elif p == "starts at len - MAX: continue":
                assert r.s - off == ln - MAX and i > first[seg] and seg + 1 < len(layout)
            elif p == "qb+1 peak in the next segment's bytes":
                assert r.qb + 1 == off + ln and int(D[r.qb + 1]) > r.max and layout[seg + 1][0] <= r.qb + 1
            elif p == "previous start one past len - MAX: stop and carry":
                poff, pln = layout[seg - 1]
                assert r.s - poff == pln - MAX + 1 and first[seg] == i
            elif p == "winner at qa = MIN":
                assert r.win == r.qa == off + MIN
            elif p == "winner at slice position 0":
                assert r.pos_of(r.win) == 0
            elif p == "winner at slice position 4095":
                assert r.pos_of(r.win) == 4095
            elif p == "arena slices skewed":
                assert off % cut_craft.SLICE == 48 * seg and r.win % cut_craft.SLICE != r.pos_of(r.win)
            else:
                raise AssertionError(p)
