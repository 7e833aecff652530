"""Designed inputs for K1's slice summaries (hbx_k1_digest_scan_dma, k1_prime,
k1_iteration, digest_pass_sdwa in hashbox_amd/csrc/hbx_kernels.hip) and
their reference.

K1 stores one ``{smax, sprev}`` pair per 4,096 window positions of a file
with split candidates.  K2 reads almost none of them exactly,
so the cut tests cannot see a wrong word that loses.  Here every word has a
reference, from ``oracle.digest_all`` alone:

* ``smax[j] = max D[4096 j : min(4096 (j + 1), N)]``;
* ``sprev[j] = D[4096 j - 1]``, and ``0x80000000`` for ``j = 0`` (nothing
  rolled in: ``s1 = 0``, ``s2 = 2^15`` of the virtual zeros).

The corpus is one arena of non-zero filler (as tests/md5_craft.py builds
them): files at 16-byte-aligned offsets that are not all multiples of 64, at
least ``GAP`` filler bytes after each and 64 KiB after the last.  K1's buffer
descriptor rounds a tile up to 16 bytes, so up to 15 filler bytes after a
file are really loaded, and zeros after a file whose length is a multiple of
16; most random files and the byte after them are chosen so that a digest
computed one position past the end, from what K1 would load there, beats the
last slice's maximum.

MIRRORED quotes the K1 source lines the reference restates;
tests/test_k1_craft.py fails if one no longer occurs in the source, and
asserts on the reference that the corpus has the properties claimed below.

Nothing here needs a GPU.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from oracle import oracle as O

from . import cut_craft as cc

MIN = O.MIN_BLOCK_SIZE
SLICE = 4096           # kSlice
WAVES = MIN // SLICE   # slices (waves) per 64 KiB iteration
STREAM = 32            # positions per SDWA stream: a lane's run is two of them
ARENA_SLACK = 64       # HBX_ARENA_SLACK (include/hbxgpu.h)
GAP = 128              # least filler after a file
HEAD = 256             # filler before the first file
END = 64 << 10         # filler after the last file
START = 0x80000000     # sprev of slice 0
TILES = (1, 3, 16)     # the tile lengths the GPU test sets (0, the default, gives 16 at this size)
MAX_CORPUS = 40 << 20
# what the corpus holds, as DESIGN.md §2 states it (tests/test_k1_craft.py asserts each on the reference)
STATED = {"tail": 24, "tail_masked": 24, "tail0": 5, "tail0_masked": 4, "last": 9, "wave_up": 13, "wave_down": 9,
          "masked_up": 9, "masked_down": 6, "tile_first": {1: 330, 3: 101, 16: 5}}

# hashbox_amd/csrc/hbx_kernels.hip (white space is collapsed before the comparison)
MIRRORED = [
    "st.s2c = 0x8000u;",                                         # sprev[0], and every D through it
    "st.s2c = 0x8000u - readlane(sC, 15);",                      # a later tile's start state (k1_prime's halo path)
    "const bool ok = qs + (uint64_t)w * kSlice < N;",            # which slices exist: ceil(N / 4096)
    "sprev = readlane((s2_t << 16) | (S1_t & 0xffffu), 0);",     # D just before the wave's first position
    "DA = (e_l + 4u * k + B < lim) ? DA : 0u;",                  # smax stops at N - 1 (stream A)
    "DB = (e_l + 32u + 4u * k + B < lim) ? DB : 0u;",            # ... (stream B)
    "M = digest_pass_sdwa<true>(cur, out, XA, XB, e_l, (uint32_t)(N - qs));",  # lim = N - iteration start
    "if (qs + kMinBlock <= N) {",                                # only a file's last, partial iteration is masked
]
MIRRORED_ENGINE = [
    "return N > 2ull * HBX_MIN_BLOCK_SIZE ? (N + HBX_MIN_BLOCK_SIZE - 1) / HBX_MIN_BLOCK_SIZE : 0;",  # scan_iters
    "slices += (N + kSlice - 1) / kSlice;",
]


# ------------------------------------------------------------- reference --
def n_slices(n: int) -> int:
    """`scan_iters(N)` non-zero: `slices += (N + kSlice - 1) / kSlice`."""
    return (n + SLICE - 1) // SLICE if n > 2 * MIN else 0


def summaries(x: np.ndarray) -> np.ndarray:
    """[slices, 2] uint32 {smax, sprev} of one file, from digest_all alone."""
    n, k = x.size, n_slices(x.size)
    out = np.zeros((k, 2), np.uint32)
    if not k:
        return out
    D = O.digest_all(x)
    pad = np.zeros(k * SLICE, np.uint32)  # D >= 0: a zero never raises a maximum
    pad[:n] = D
    out[:, 0] = pad.reshape(k, SLICE).max(axis=1)
    out[0, 1] = START
    out[1:, 1] = D[SLICE * np.arange(1, k) - 1]
    return out


def rollsum_digest(x: np.ndarray, q: int) -> int:
    """D[q] by the Python Rollsum of oracle/oracle.py: Init, then the window's
    MIN bytes rolled in, zeros standing for the bytes before the file."""
    r = O._Rollsum()
    for c in [0] * max(0, MIN - 1 - q) + x[max(0, q - MIN + 1):q + 1].tolist():
        r.rollin(c)
    assert r.count == MIN
    return r.digest()


def s1_wraps(x: np.ndarray):
    """(up, down): at which positions the true window sum S1 passes a multiple
    of 2^16 upwards / downwards, i.e. where the 16-bit s1 wraps."""
    c = np.concatenate([[0], np.cumsum(x, dtype=np.int64)])
    S1 = c[1:] - c[np.maximum(np.arange(1, x.size + 1) - MIN, 0)]
    hi = np.concatenate([[0], S1 >> 16])
    return hi[1:] > hi[:-1], hi[1:] < hi[:-1]


def wrap_slices(x: np.ndarray):
    """The slices whose maximum lies in a 32-position stream at or after a
    wrap of s1 in that stream: ([slices after a wrap up], [... down]).  A carry
    that leaks between the halves of the digest register changes these."""
    D = O.digest_all(x)
    up, down = s1_wraps(x)
    ups, downs = [], []
    for j in range(n_slices(x.size)):
        lo, hi = SLICE * j, min(SLICE * (j + 1), x.size)
        p = lo + int(np.argmax(D[lo:hi]))
        m0 = p - p % STREAM
        if up[m0:p + 1].any():
            ups.append(j)
        if down[m0:p + 1].any():
            downs.append(j)
    return ups, downs


# ------------------------------------------------------------ file values --
def _steer(x: np.ndarray, at: int, lo: int, fine: int, first_free: int):
    """Make s2 = 0xFFFF at position `at` of x (which may hold one byte past
    the file) by the byte 256 before it (weight 257 in s2) and the byte
    `fine` before it (weight fine + 1, kept >= first_free), then check that
    D[at] is above every D in [lo, at).  Bytes further back are stepped until
    that holds."""
    w = fine + 1
    for _ in range(256):
        s2 = int(O.digest_all(x)[at]) >> 16
        t0, b0 = int(x[at - 256]), int(x[at - fine])
        for t in range(256):
            r = ((0xFFFF - s2) - 257 * (t - t0)) & 0xFFFF
            for r in (r, r - 65536):
                if r % w == 0 and first_free <= b0 + r // w <= 255:
                    y = x.copy()
                    y[at - 256], y[at - fine] = t, b0 + r // w
                    D = O.digest_all(y)
                    if D[at] >> 16 == 0xFFFF and (at == lo or int(D[at]) > int(D[lo:at].max())):
                        return y
        x = x.copy()
        x[at - 300] += 1
    raise AssertionError("no steering found")


@dataclass
class File:
    name: str
    family: str
    data: np.ndarray
    # "tail": D one past the end, over file + filler, beats the last slice; "tail0": the same with a zero byte
    # there, which is what K1 loads past a file whose length is a multiple of 16 (its descriptor ends with the
    # file); "last": D[N-1] is the last slice's maximum
    kind: str = ""
    after: Optional[int] = None   # the first filler byte after the file ("tail")

    @property
    def n(self) -> int:
        return int(self.data.size)


def _random_file(name: str, n: int, seed: int, kind: str) -> File:
    x = O.random_bytes(n, seed)
    if n <= 2 * MIN:
        return File(name, "lengths", x)
    lo = (n - 1) // SLICE * SLICE
    if kind == "tail" and n % 16:
        y = _steer(np.concatenate([x, np.array([1], np.uint8)]), n, lo, 0, 1)
        return File(name, "lengths", y[:n].copy(), "tail", int(y[n]))
    if kind == "tail":  # the byte at N stays zero: the file's last byte (weight 2) does the fine step
        y = _steer(np.concatenate([x, np.array([0], np.uint8)]), n, lo, 1, 0)
        assert y[n] == 0
        return File(name, "lengths", y[:n].copy(), "tail0")
    y = _steer(x, n - 1, lo, 0, 0)
    return File(name, "lengths", y, "last")


def length_list() -> List[int]:
    ns = [2 * MIN, 2 * MIN + 1]
    ns += [k * MIN + d for k in (3, 4) for d in (-1, 0, 1)]
    ns += [3 * MIN + SLICE * j + d for j in (0, 1, 15) for d in (-1, 0, 1, 63, 64, 65)]
    ns += [3 * MIN + 7 * SLICE + 1600 + r for r in range(16)]  # every N mod 16, ending inside a wave's slice
    out = []
    for n in ns:
        if n not in out:
            out.append(n)
    return out


def block_wave(n: int, seed: int) -> np.ndarray:
    """MIN bytes from 0xC0..0xFF, then MIN bytes from 0x00..0x3F, repeated:
    the window sum falls and rises by about 192 per position, so the 16-bit
    s1 wraps every ~340 positions, in both directions."""
    g = np.random.default_rng(seed)
    x = g.integers(0, 0x40, n, dtype=np.uint8)
    high = (np.arange(n) // MIN) % 2 == 0
    x[high] += 0xC0
    return x


CUT_CASES = ("u_end_mid-slice_N-1", "u_end_16_N-1", "u_end_64_N-2", "u_end_4096_N-1", "u_slice_pos_0",
             "u_slice_pos_4095", "u_run_residue_31", "u_run_residue_32", "u_iter_first", "u_iter_last",
             "u_tile3_first", "u_tile3_last", "u_tile16_first", "comb_8_per_slice", "tie_all_three",
             "plateau_six_slices")
WAVE_N, WAVE_SEED = 2 * (1 << 20) + 777, 1
WAVE_TAILS = 8           # per direction: short block waves whose last, masked iteration holds 15.5 slices
NTILE = 37 * MIN + 999
NO_SLICES = (0, 1, MIN, 2 * MIN)


def _ramp() -> np.ndarray:
    """0xFF from the file start for 1.5 MIN (s1 and s2 climb from the virtual
    zeros' s1 = 0, s2 = 2^15 with the largest step), zeros, then random."""
    x = np.zeros(4 * MIN + 5 * SLICE + 333, np.uint8)
    x[:MIN + MIN // 2] = 0xFF
    x[3 * MIN:] = O.random_bytes(x.size - 3 * MIN, 77)
    return x


@functools.lru_cache(maxsize=None)
def files() -> List[File]:
    out = []
    for i, n in enumerate(length_list()):
        out.append(_random_file("len_%d" % n, n, 9000 + i, "last" if i % 4 == 3 else "tail"))
    nv = 4 * MIN + 3 * SLICE + 777
    for v in (0x00, 0x5A, 0xFF):
        out.append(File("const_%02x" % v, "values", np.full(nv, v, np.uint8)))
    out.append(File("ramp_ff", "values", _ramp()))
    for name in CUT_CASES:
        out.append(File("cut_" + name, "values", np.array(cc.build(name))))
    out.append(File("block_wave", "wave", block_wave(WAVE_N, WAVE_SEED)))
    # the masked pass (digest_pass_sdwa<true>) is other code than the full one: block waves that end in the
    # falling (3 MIN + ...) and in the rising (4 MIN + ...) half of the wave
    for k in (3, 4):
        for i in range(WAVE_TAILS):
            n = k * MIN + 15 * SLICE + 2049 + 17 * i
            out.append(File("wave_tail_%d_%d" % (k, i), "wave_tail", block_wave(n, 10 * k + i)))
    out.append(File("tiles_37", "tiles", O.random_bytes(NTILE, 501)))
    out.append(File("tiles_12", "tiles", O.random_bytes(NTILE // 3, 502)))
    for n in NO_SLICES:
        out.append(File("none_%d" % n, "none", O.random_bytes(n, 600 + n % 7)))
    return out


# ------------------------------------------------------------- the arena --
def filler(n: int, seed: int) -> np.ndarray:
    return np.random.Generator(np.random.PCG64(seed)).integers(1, 256, n, dtype=np.uint8)


@dataclass
class Corpus:
    files: List[File]
    host: np.ndarray
    offs: np.ndarray   # uint64
    lens: np.ndarray   # uint64
    _ref: Optional[List[np.ndarray]] = None

    def data(self, f: int) -> np.ndarray:
        o = int(self.offs[f])
        return self.host[o:o + int(self.lens[f])]

    def ref(self) -> List[np.ndarray]:
        """summaries() of every file, computed once."""
        if self._ref is None:
            self._ref = [summaries(self.data(f)) for f in range(len(self.files))]
        return self._ref

    def extended(self, f: int, more: int = 16) -> np.ndarray:
        """D over the file and what K1 loads after it: the `more` arena bytes
        that follow, or zeros where the file's length is a multiple of 16
        (K1's descriptor ends with the file)."""
        o, n = int(self.offs[f]), int(self.lens[f])
        x = self.host[o:o + n + more].copy()
        if n % 16 == 0:
            x[n:] = 0
        return O.digest_all(x)


def build(fs: List[File], seed: int = 4242) -> Corpus:
    """Lay the files out in order: file i at the next address that is i + 1
    sixteenths past a multiple of 64 (16, 32, 48, 0, ...) and leaves >= GAP
    filler after the previous one."""
    offs, pos = [], HEAD
    for i, f in enumerate(fs):
        o = pos + ((16 * ((i + 1) % 4) - pos) % 64)
        offs.append(o)
        pos = o + f.n + GAP
    host = filler(pos + END, seed)
    for f, o in zip(fs, offs):
        host[o:o + f.n] = f.data
        if f.after is not None:
            host[o + f.n] = f.after
    return Corpus(list(fs), host, np.array(offs, np.uint64), np.array([f.n for f in fs], np.uint64))


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    """Every file, the ones without slices spread among the others."""
    fs = [f for f in files() if f.family != "none"]
    for k, f in enumerate(f for f in files() if f.family == "none"):
        fs.insert(3 + 11 * k, f)
    return build(fs)


def batch_indices(c: Corpus) -> List[int]:
    """About 40 files of the corpus in another order: every family, the files
    without slices between them, so that the per-file slice bases differ from
    the whole corpus's."""
    by: Dict[str, List[int]] = {}
    for i, f in enumerate(c.files):
        by.setdefault(f.family, []).append(i)
    idx = by["lengths"][::2][:16] + by["values"][::2] + by["wave"] + by["wave_tail"][::4] + by["tiles"]
    idx = idx[::-1]
    for k, i in enumerate(by["none"]):
        idx.insert(2 + 9 * k, i)
    return idx


def tile_first_slices(c: Corpus, tile: int) -> List[tuple]:
    """(file, slice) of every tile's first slice but the file's first: there
    `sprev`, and the state everything after it builds on, comes from
    k1_prime's halo path.  k1_tiles: a tile starts every `tile` iterations."""
    return [(f, WAVES * tile * k) for f in range(len(c.files))
            for k in range(1, (n_slices(int(c.lens[f])) + WAVES * tile - 1) // (WAVES * tile))]


def describe(c: Corpus, f: int, j: int, tile: int) -> str:
    it = j // WAVES
    return "%s (file %d, %d bytes, offset %% 64 = %d) slice %d of %d: tile %d (of %d iterations), iteration %d, wave %d" % (
        c.files[f].name, f, int(c.lens[f]), int(c.offs[f]) % 64, j, n_slices(int(c.lens[f])), it // tile, tile, it,
        j % WAVES)
