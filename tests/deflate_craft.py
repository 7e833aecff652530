"""Hand-built deflate / zlib streams for the inflate tests (RFC 1950/1951).

The device inflate is fed by CPython's zlib and by the device deflate in the
rest of the suite; neither emits a distance above window - 262 on purpose, a
15-bit code, a block header at a chosen bit, or one specific invalid stream.
This module builds such streams bit by bit, and the families of named cases
(``Case``) the CPU and GPU tests share:

* ``test_deflate_craft.py`` checks every case against CPython's zlib (the
  verdict and the bytes), which makes zlib the reference;
* ``test_gpu_inflate_crafted.py`` compares the device with the table.

Blocks are values: ``stored``, ``fixed`` and ``dynamic`` return a function
that writes the block into a ``BitWriter``, so blocks can follow each other at
any bit offset; ``deflate(blocks)`` strings them together and ``zwrap`` adds
the zlib header and the Adler-32.

Tokens: an ``int`` is a literal, ``bytes`` a run of literals, ``(L, D)`` a
match, ``("sym", code, nbits)`` a raw Huffman code (first bit of the code
first, for symbols no encoder may send) and ``("bits", value, nbits)`` raw
extra bits (LSB first).

Go's compress/flate is the producer of the streams in the field.  It agrees
with zlib on every case here; the two known differences are left out on
purpose: a code-length code made of a single 1-bit code (zlib rejects it, Go
accepts it) and distances beyond the window a CINFO < 7 header announces
(zlib rejects them when told the window, Go ignores CINFO).

No dependence on the GPU.
"""
from __future__ import annotations

import functools
import heapq
import struct
import zlib
from collections import namedtuple

import numpy as np

# expected_status: 0, a documented inflate status (include/hbxgpu.h: 1 header
# or Adler, 2 input, 3 output capacity, 4 code, 5 distance, 6 stored length),
# or ANY_ERROR for "non-zero".  min_cap: the output capacity the stream is
# given (for a good stream exactly its inflated length).
Case = namedtuple("Case", "name stream expected status min_cap")
ANY_ERROR = -1
# good cases that zlib.decompress (not the strict oracle) is the reference for
TRAILING = frozenset(["trailing_bytes_after_adler"])

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30
# a complete code-length code that can send every length and every repeat
DEFAULT_CL = [5] * 16 + [2, 3, 3]


class BitWriter:
    """LSB-first bit writer (RFC 1951 §3.1.1)."""

    def __init__(self):
        self._buf = bytearray()
        self._acc = 0
        self._n = 0

    def bits(self, value: int, nbits: int) -> None:
        self._acc |= (value & ((1 << nbits) - 1)) << self._n
        self._n += nbits
        if self._n >= 512:
            nb = self._n >> 3
            self._buf += (self._acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
            self._acc >>= 8 * nb
            self._n -= 8 * nb

    def code(self, code: int, nbits: int) -> None:
        """A Huffman code: its first (most significant) bit goes out first."""
        self.bits(_rev(code, nbits), nbits)

    def align(self) -> None:
        self.bits(0, -self._n & 7)

    def raw(self, data: bytes) -> None:
        assert self._n & 7 == 0
        for k in range(0, len(data), 4096):
            piece = data[k:k + 4096]
            self.bits(int.from_bytes(piece, "little"), 8 * len(piece))

    def tell(self) -> int:
        """Bits written so far."""
        return 8 * len(self._buf) + self._n

    def getvalue(self) -> bytes:
        nb = (self._n + 7) >> 3
        return bytes(self._buf) + self._acc.to_bytes(nb, "little")


def _rev(code: int, nbits: int) -> int:
    r = 0
    for _ in range(nbits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lens):
    """symbol -> (code, nbits) of the canonical code with these lengths (RFC
    1951 §3.2.2), whatever the lengths: an over-subscribed set gives codes
    that overflow their length, which only the header of an invalid stream
    ever carries."""
    codes, code = {}, 0
    for nbits in range(1, 16):
        for s, k in enumerate(lens):
            if k == nbits:
                codes[s] = (code, nbits)
                code += 1
        code <<= 1
    return codes


def _stream_codes(lens):
    return {s: (_rev(c, n), n) for s, (c, n) in canonical(lens).items()}


def huffman_lens(freq, n, maxbits=15):
    """Code lengths of a complete Huffman code over the symbols of ``freq``
    (one used symbol gets the single 1-bit code zlib and Go allow)."""
    lens = [0] * n
    used = [s for s in range(n) if freq.get(s, 0) > 0]
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    f = {s: freq[s] for s in used}
    while used:
        lens = [0] * n
        heap = [(f[s], s, [s]) for s in used]
        heapq.heapify(heap)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(lens) <= maxbits:
            break
        f = {s: max(1, v >> 1) for s, v in f.items()}  # flatter, until it fits
    return lens


_LEN_SYM = {}
for _i in range(29):
    for _e in range(1 << LEN_EXTRA[_i]):
        _LEN_SYM.setdefault(LEN_BASE[_i] + _e, (257 + _i, _e, LEN_EXTRA[_i]))
_LEN_SYM[258] = (285, 0, 0)


def len_symbol(L):
    """(symbol, extra value, extra bits) of match length L, 258 as symbol 285."""
    return _LEN_SYM[L]


def dist_symbol(D):
    s = max(k for k in range(30) if DIST_BASE[k] <= D)
    return s, D - DIST_BASE[s], DIST_EXTRA[s]


def _emit(w, tokens, lcodes, dcodes):
    for t in tokens:
        if isinstance(t, int):
            w.bits(*lcodes[t])
        elif isinstance(t, (bytes, bytearray)):
            for b in t:
                w.bits(*lcodes[b])
        elif t[0] == "sym":
            w.code(t[1], t[2])
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        else:
            s, e, k = len_symbol(t[0])
            w.bits(*lcodes[s])
            w.bits(e, k)
            s, e, k = dist_symbol(t[1])
            w.bits(*dcodes[s])
            w.bits(e, k)


def _frequencies(tokens):
    lf, df = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            lf[t] = lf.get(t, 0) + 1
        elif isinstance(t, (bytes, bytearray)):
            for b in t:
                lf[b] = lf.get(b, 0) + 1
        elif isinstance(t[0], int):
            s = len_symbol(t[0])[0]
            lf[s] = lf.get(s, 0) + 1
            s = dist_symbol(t[1])[0]
            df[s] = df.get(s, 0) + 1
    return lf, df


def expand(tokens) -> bytes:
    """The plain LZ77 expansion: the bytes a stream of these tokens inflates
    to (raw tokens stand for nothing)."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, (bytes, bytearray)):
            out += t
        elif isinstance(t[0], int):
            L, D = t
            if D > len(out) or D < 1:
                raise ValueError(f"distance {D} with {len(out)} bytes written")
            at = len(out) - D
            if D >= L:
                out += out[at:at + L]
            else:  # the copy overlaps itself: the last D bytes, repeated
                out += (bytes(out[at:]) * (L // D + 1))[:L]
    return bytes(out)


_FIXED_L = _stream_codes(FIXED_LITLEN)
_FIXED_D = _stream_codes(FIXED_DIST)


def fixed_code(sym):
    """The raw token of literal/length symbol ``sym`` (0..287) in a fixed block."""
    c, n = canonical(FIXED_LITLEN)[sym]
    return ("sym", c, n)


def stored(data: bytes, final: bool, nlen=None):
    """A stored block (RFC 1951 §3.2.4); ``nlen`` replaces the complement."""
    assert len(data) <= 65535

    def block(w):
        w.bits(1 if final else 0, 1)
        w.bits(0, 2)
        w.align()
        w.bits(len(data), 16)
        w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        w.raw(bytes(data))
    return block


def fixed(tokens, final: bool, eob=True):
    def block(w):
        w.bits(1 if final else 0, 1)
        w.bits(1, 2)
        _emit(w, tokens, _FIXED_L, _FIXED_D)
        if eob:
            w.bits(*_FIXED_L[256])
    return block


def cl_ops_for(lens, use16=True, use17=True):
    """Code-length alphabet operations that send ``lens``: runs of zeros by
    17/18 and repeats by 16 (RFC 1951 §3.2.7), where allowed."""
    ops, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= (3 if use17 else 11):
            k = min(run, 138)
            ops.append((18, k - 11) if k >= 11 else (17, k - 3))
            i += k
        elif v != 0 and run >= 4 and use16:
            ops.append((v,))
            k = min(run - 1, 6)
            ops.append((16, k - 3))
            i += 1 + k
        else:
            ops.append((v,))
            i += 1
    return ops


def run_cl_ops(ops):
    """The code lengths a decoder reads from these operations."""
    lens = []
    for op in ops:
        if op[0] < 16:
            lens.append(op[0])
        elif op[0] == 16:
            lens += [lens[-1]] * (3 + op[1])
        elif op[0] == 17:
            lens += [0] * (3 + op[1])
        else:
            lens += [0] * (11 + op[1])
    return lens


def dynamic(tokens, final: bool, litlen_lens=None, dist_lens=None, cl_lens=None, raw_header=None, hclen=None,
            eob=True):
    """A dynamic block (RFC 1951 §3.2.7).  Lengths left out are a Huffman
    code of the tokens; lengths given are sent as given, invalid ones
    included (HLIT = len(litlen_lens), HDIST = len(dist_lens)).  ``cl_lens``
    are the 19 lengths of the code-length code by symbol and ``hclen`` how
    many of them are sent.  ``raw_header = (hlit_field, hdist_field, ops)``
    dictates the two 5-bit fields and the code-length operations themselves
    (``(length,)``, ``(16, extra)``, ``(17, extra)``, ``(18, extra)``); the
    tokens are then coded with ``litlen_lens`` / ``dist_lens``, which the
    caller keeps consistent with the operations where the block is valid."""
    lf, df = _frequencies(tokens)
    if litlen_lens is None:
        litlen_lens = huffman_lens(lf, 286)
        while len(litlen_lens) > 257 and litlen_lens[-1] == 0:
            litlen_lens.pop()
    if dist_lens is None:
        dist_lens = huffman_lens(df, 30)
        while len(dist_lens) > 1 and dist_lens[-1] == 0:
            dist_lens.pop()
    if raw_header is None:
        raw_header = (len(litlen_lens) - 257, len(dist_lens) - 1, cl_ops_for(list(litlen_lens) + list(dist_lens)))
    hlit, hdist, ops = raw_header
    cl = list(DEFAULT_CL if cl_lens is None else cl_lens)
    if hclen is None:
        hclen = 19
        while hclen > 4 and cl[ORDER[hclen - 1]] == 0:
            hclen -= 1
    clcodes = _stream_codes(cl)
    lcodes, dcodes = _stream_codes(litlen_lens), _stream_codes(dist_lens)

    def block(w):
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        w.bits(hlit, 5)
        w.bits(hdist, 5)
        w.bits(hclen - 4, 4)
        for k in range(hclen):
            w.bits(cl[ORDER[k]], 3)
        for op in ops:
            w.bits(*clcodes[op[0]])
            if op[0] == 16:
                w.bits(op[1], 2)
            elif op[0] == 17:
                w.bits(op[1], 3)
            elif op[0] == 18:
                w.bits(op[1], 7)
        _emit(w, tokens, lcodes, dcodes)
        if eob and 256 in lcodes:
            w.bits(*lcodes[256])
    return block


def sync_flush():
    """The empty stored block of a sync flush: 00 00 FF FF once aligned."""
    return stored(b"", False)


def deflate(blocks) -> bytes:
    w = BitWriter()
    for b in blocks:
        b(w)
    return w.getvalue()


def header(cinfo=7, cm=8, flevel=2, fdict=0, fcheck=None) -> int:
    """CMF/FLG as one 16-bit number, with correct check bits unless given."""
    v = ((cinfo << 4 | cm) << 8) | (flevel << 6) | (fdict << 5)
    return v + ((31 - v % 31) % 31 if fcheck is None else fcheck)


def zwrap(body, data: bytes, cmf_flg=0x789C, adler=None, trailer=b"") -> bytes:
    """RFC 1950 around a deflate body (bytes or a list of blocks): header,
    body, the Adler-32 of ``data`` (or the number given)."""
    if not isinstance(body, (bytes, bytearray)):
        body = deflate(body)
    a = zlib.adler32(data) if adler is None else adler
    return struct.pack(">H", cmf_flg) + bytes(body) + struct.pack(">I", a & 0xFFFFFFFF) + trailer


def good(name, blocks_tokens, **kw):
    """A good case from [(kind, tokens, extra), ...]: kind "s" stored (tokens
    = bytes), "f" fixed, "d" dynamic (extra = dynamic()'s keywords); the last
    block is final."""
    blocks, alltok = [], []
    for i, bt in enumerate(blocks_tokens):
        kind, toks = bt[0], bt[1]
        extra = bt[2] if len(bt) > 2 else {}
        fin = i == len(blocks_tokens) - 1
        if kind == "s":
            blocks.append(stored(toks, fin))
            alltok.append(bytes(toks))
        elif kind == "f":
            blocks.append(fixed(toks, fin))
            alltok += list(toks)
        else:
            blocks.append(dynamic(toks, fin, **extra))
            alltok += list(toks)
    data = expand(alltok)
    return Case(name, zwrap(blocks, data, **kw), data, 0, len(data))


def _rng(seed):
    return np.random.default_rng(seed)


def _rand(n, seed):
    return _rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text(n, seed):
    """Word soup that deflate compresses about 3:1."""
    rng = _rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 10, 300)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.zipf(1.3)) % len(words)] + b" "
    return bytes(out[:n])


# ---------------------------------------------------------------- copy grid --
GRID_D = tuple(range(1, 67)) + (127, 128, 129, 255, 256, 257)
GRID_L = (3, 4, 63, 64, 65, 127, 128, 129, 257, 258)


@functools.lru_cache(None)
def copy_grid():
    """One fixed block each: P random literals, one match, 5 literals, for
    every short distance (the periodic copy below 64, the lane kernel's 16-byte
    steps from 16), lengths around the 64-lane steps, and two lane phases."""
    rnd = _rand(400, 1)
    cases = []
    for D in GRID_D:
        for L in GRID_L:
            for P in (D, D + 61):
                cases.append(good(f"grid_D{D}_L{L}_P{P}", [("f", [rnd[:P], (L, D), rnd[300:305]])]))
    return cases


def chain_tokens(n):
    return [0x37] + [(258, 1)] * n + [(258, 2), (258, 63), (258, 64)]


@functools.lru_cache(None)
def chains():
    """Long overlapping copies at a few bits per match; the capacity is exact,
    so the last match ends at the last byte of the slot."""
    out = [good("chain_fixed", [("f", chain_tokens(40))]),
           good("chain_dynamic", [("d", chain_tokens(40))]),
           good("chain_dynamic_1000_to_1", [("d", chain_tokens(4000))])]
    lit = [1, 2, 3]
    out.append(good("len258_as_285", [("f", lit + [(258, 3), 9])]))
    # 284 with extra 31 is 227 + 31 = 258 too (zlib and Go accept it)
    toks = lit + [fixed_code(284), ("bits", 31, 5), ("sym", 2, 5), 9]  # distance symbol 2 = 3
    data = expand(lit + [(258, 3), 9])
    out.append(Case("len258_as_284_extra31", zwrap([fixed(toks, True)], data), data, 0, len(data)))
    return out


# ------------------------------------------------------------ far distances --
FAR_D = (16383, 16384, 16385, 16447, 16448, 32505, 32506, 32507, 32767, 32768)


@functools.lru_cache(None)
def far():
    """Matches at and around the split decoder's ring (16,384 symbols) and up
    to the full window, which zlib never emits (it stops at window - 262) but
    Go's flate and the device deflate do; then distances equal to and one past
    the bytes written."""
    pre = _rand(32768 + 70, 2)
    cases = []
    for D in FAR_D:
        for L in (3, 258):
            cases.append(good(f"far_D{D}_L{L}", [("s", pre), ("f", [(L, D), 7])]))
    cases.append(good("far_all_in_one_block", [("s", pre), ("f", [t for D in FAR_D for t in ((3, D), (258, D), 5)])]))
    lits = _rand(300, 3)
    short = _rand(20070, 4)
    for name, blocks, n in (("first_block", [], 300), ("after_prefix", [("s", short)], 20070 + 300)):
        for L in (3, 258):
            cases.append(good(f"dist_equals_written_{name}_L{L}", blocks + [("f", [lits, (L, n), 1])]))
            body = [stored(b[1], False) for b in blocks] + [fixed([lits, (L, n + 1), 1], True)]
            cases.append(Case(f"dist_one_past_written_{name}_L{L}", zwrap(body, b""), None, 5, n + L + 1))
    return cases


# ---------------------------------------------------------- block structure --
def _maximal_dynamic():
    """286 literal/length and 30 distance lengths, each sent on its own with a
    code-length code that spends 7 bits on the common ones: a header of about
    280 bytes, the longest a valid block has."""
    ll = [8] * 226 + [9] * 60            # 226 / 256 + 60 / 512 = 1
    dl = [4] * 2 + [5] * 28              # 2 / 16 + 28 / 32 = 1
    cl = [0] * 19
    for s, k in ((8, 7), (9, 7), (4, 6), (5, 5), (0, 4), (1, 3), (2, 2), (3, 1)):
        cl[s] = k
    ops = [(v,) for v in ll + dl]
    return dict(litlen_lens=ll, dist_lens=dl, cl_lens=cl, raw_header=(29, 29, ops), hclen=19)


HEADER_AT = (3583, 3584, 3585, 4080, 4095, 4096, 4097, 8191)


@functools.lru_cache(None)
def structure():
    cases = []
    # a stored block after 3 + 9k + 7 bits of fixed block: its header starts at
    # each of the eight bit offsets
    for k in range(8):
        for name, payload in (("empty", b""), ("one", b"\x5a")):
            cases.append(good(f"stored_{name}_after_{k}_nine_bit_literals",
                              [("f", [200] * k), ("s", payload), ("f", [65])]))
    for n in (0, 1, 8, 9, 65535):
        cases.append(good(f"stored_len_{n}", [("f", [1]), ("s", _rand(n, 10 + n)), ("s", _rand(n, 11 + n))]))
    cases.append(good("final_empty_stored", [("f", [1, 2, 3, (3, 3)]), ("s", b"")]))
    # 300 blocks in turn, with matches into the blocks before
    rnd = _rand(6000, 5)
    blocks = []
    for i in range(300):
        piece = rnd[20 * i:20 * i + 20]
        toks = [piece] + ([(5 + i % 200, 1 + (7 * i) % (20 * i))] if i else [])
        blocks.append(("s", piece) if i % 3 == 0 else ("f", toks) if i % 3 == 1 else ("d", toks))
    cases.append(good("300_blocks_alternating", blocks))
    # headers across the 4 KiB input staging of the wave decoders: LEN/NLEN of
    # a stored block at stream offset X, and a maximal dynamic header whose
    # first bit is bit 2 (bit 3 with one 9-bit literal) of offset X
    mx = _maximal_dynamic()
    body = [_rand(150, 6), (258, 150), (3, 1), (200, 30)]
    pad = _rand(9000, 7)
    pad8 = bytes(b % 144 for b in pad)  # 8-bit literals: one stream byte each
    for X in HEADER_AT:
        cases.append(good(f"stored_header_at_{X}", [("f", [pad8[:X - 4]]), ("s", _rand(77, X)), ("f", [(9, 50)])]))
        cases.append(good(f"max_dynamic_header_at_{X}_bit2", [("f", [pad8[:X - 3]]), ("d", body, mx)]))
        cases.append(good(f"max_dynamic_header_at_{X}_bit3", [("f", [pad8[:X - 4], 200]), ("d", body, mx)]))
    # code lengths 1..15 in both codes, the 15-bit codes used
    ls = [256, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 257, 77, 285, 65]
    ll = [0] * 286
    for i, s in enumerate(ls):
        ll[s] = min(i + 1, 15)
    dl = [min(i + 1, 15) for i in range(16)]
    toks = [bytes(range(65, 78)) * 20]
    for ds in range(16):
        toks += [(3, DIST_BASE[ds]), (258, DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1), 65]
    cases.append(good("lengths_1_to_15", [("d", toks, dict(litlen_lens=ll, dist_lens=dl))]))
    # codes of exactly 9 and 10 bits, either side of the 9-bit first-level table:
    # 1/2 + 240/512 + 32/1024 = 1
    ll = [0] * 286
    for s in range(240):
        ll[s] = 9
    for s in range(240, 256):
        ll[s] = 10
    ll[256] = 1
    for s in range(257, 273):
        ll[s] = 10
    toks = [bytes(range(256)), (3, 256), (18, 1), bytes(range(255, 200, -1))]
    cases.append(good("codes_of_9_and_10_bits", [("d", toks, dict(litlen_lens=ll))]))
    cases.append(good("hlit_286_hdist_30", [("d", body, mx)]))
    # 8 code-length code lengths sent (HCLEN field 4): 16, 17, 18, 0, 8, 7, 9, 6.
    # (4 sent, the field at 0, cannot be valid: see rejections().)
    ll = [7] * 64 + [8] * 64 + [0] * 128 + [6] * 16   # 1/2 + 1/4 + 1/4
    cl = [0] * 19
    for s, k in ((0, 2), (6, 2), (7, 2), (8, 3), (18, 3)):
        cl[s] = k
    cases.append(good("hclen_8_lengths", [("d", [bytes(range(128)) * 2],
                                           dict(litlen_lens=ll, dist_lens=[0], cl_lens=cl,
                                                raw_header=(len(ll) - 257, 0, cl_ops_for(ll + [0], False, False))))]))
    # a 16 that repeats the last literal/length length into the distance lengths;
    # 18 with its longest run of 138
    # 254 zeros, a 2 for symbol 254, six more for 255, 256, 257 and three distance lengths, the fourth
    ops = [(18, 127), (18, 105), (2,), (16, 3), (2,)]
    ll = run_cl_ops(ops)[:258]
    assert ll == [0] * 254 + [2] * 4 and run_cl_ops(ops)[258:] == [2] * 4
    cases.append(good("repeat_16_crosses_into_distances",
                      [("d", [254, 255, 254, 255, 254, (3, 1), (3, 2), (3, 3), (3, 4)],
                        dict(litlen_lens=ll, dist_lens=[2] * 4, raw_header=(1, 3, ops)))]))
    ll = [0] * 138 + [2, 2, 2] + [0] * 115 + [2]
    assert (18, 127) in cl_ops_for(ll)
    cases.append(good("repeat_18_of_138", [("d", [138, 139, 140, 138], dict(litlen_lens=ll, dist_lens=[0]))]))
    cases.append(good("one_distance_code_of_length_1", [("d", [9, (200, 1)], dict(dist_lens=[1]))]))
    cases.append(good("no_distance_codes", [("d", [b"literals only"], dict(dist_lens=[0]))]))
    cases.append(good("cinfo_6_short_distances", [("f", [_rand(100, 8), (50, 100), (258, 1)])],
                      cmf_flg=header(cinfo=6)))
    data = text(500, 9)
    cases.append(Case("trailing_bytes_after_adler", zlib.compress(data, 6) + b"after the stream", data, 0, len(data)))
    return cases


# --------------------------------------------------------------- rejections --
def three_block_stream():
    toks = [text(60, 12), (30, 20), (258, 1)]
    return good("three_blocks", [("d", toks), ("s", _rand(40, 13)), ("f", [_rand(30, 14), (100, 90)])])


@functools.lru_cache(None)
def rejections():
    def bad(name, body, status, cap=4096, **kw):
        return Case(name, zwrap(body, b"", **kw) if not isinstance(body, bytes) else body, None, status, cap)

    def raw_block(bits):  # a block given as (value, nbits) fields
        def block(w):
            for v, k in bits:
                w.bits(v, k)
        return block

    cases = [bad("btype_3", [fixed([1], False), raw_block([(1, 1), (3, 2)])], 4)]
    for s in (286, 287):
        cases.append(bad(f"fixed_litlen_symbol_{s}", [fixed([65, fixed_code(s)], True)], 4))
    for s in (30, 31):
        cases.append(bad(f"fixed_distance_symbol_{s}", [fixed([65, 65, 65, fixed_code(257), ("sym", s, 5)], True)], 4))
    ok_ll = [0] * 65 + [1] + [0] * 190 + [1]  # 'A' and end of block
    hdr = lambda hlit, hdist: raw_block([(1, 1), (2, 2), (hlit, 5), (hdist, 5), (15, 4)] + [(4, 3)] * 19)
    cases += [bad("hlit_287", [hdr(30, 0)], 4), bad("hlit_288", [hdr(31, 0)], 4),
              bad("hdist_31", [hdr(0, 30)], 4), bad("hdist_32", [hdr(0, 31)], 4)]
    A = [65, 65]
    one_two = [0] * 65 + [1] + [0] * 190  # 'A' in one bit; end of block and 257 follow in two

    def dyn(name, *args, tokens=A, **kw):
        return bad(name, [dynamic(tokens, True, *args, **kw)], 4)

    cases += [
        dyn("oversubscribed_code_length_code", ok_ll, [1], cl_lens=[1, 1, 1] + [0] * 16,
            raw_header=(0, 0, [(v,) for v in ok_ll + [1]])),
        dyn("oversubscribed_litlen_code", [0] * 65 + [1, 1] + [0] * 189 + [1], [1]),
        dyn("oversubscribed_distance_code", ok_ll, [1, 1, 1]),
        # the three incomplete codes; none of the streams uses a missing code
        dyn("incomplete_code_length_code", ok_ll, [1], cl_lens=[2, 2] + [0] * 16 + [2]),
        dyn("incomplete_litlen_code", one_two + [2], [1]),
        dyn("incomplete_distance_code", one_two + [2, 2], [2, 2, 2], tokens=A + [(3, 1)]),
        dyn("repeat_16_first", ok_ll, [1], raw_header=(0, 0, [(16, 0)] + cl_ops_for(ok_ll[3:] + [1]))),
        dyn("repeat_past_the_lengths", ok_ll, [1], raw_header=(0, 0, cl_ops_for(ok_ll) + [(17, 0)])),
        dyn("no_end_of_block_code", [0] * 65 + [1, 1] + [0] * 190, [1], eob=False),
        # 4 code-length code lengths sent (16, 17, 18, 0) can only spell zeros
        dyn("hclen_4_lengths", [0] * 257, [0], cl_lens=[1] + [0] * 17 + [1], hclen=4, eob=False, tokens=[]),
        bad("stored_len_nlen_mismatch", [fixed([1], False), stored(b"abc", True, nlen=0xFFFD)], 6),
    ]
    d = b"header and trailer"
    z = zlib.compress(d, 6)
    cases += [bad(name, struct.pack(">H", h) + z[2:], 1)
              for name, h in (("cm_7", header(cm=7)), ("cinfo_8", header(cinfo=8)),
                              ("bad_fcheck", header(fcheck=0) + 1), ("fdict", header(fdict=1)))]
    cases += [bad("wrong_adler", z[:-4] + struct.pack(">I", zlib.adler32(d) ^ 0x10000), 1),
              bad("wrong_adler_low", z[:-1] + bytes([z[-1] ^ 1]), 1)]
    # capacity exact and one short, for a stream that ends in a literal, a match, a stored block
    r = _rand(100, 15)
    for name, blocks in (("literal", [("f", [r, (40, 7), 1, 2])]), ("match", [("f", [r, (258, 100)])]),
                         ("stored", [("f", [r]), ("s", r[:50])]), ("stored_only", [("s", r)])):
        c = good(f"cap_exact_ends_in_{name}", blocks)
        cases += [c, Case(f"cap_one_short_ends_in_{name}", c.stream, None, 3, c.min_cap - 1)]
    t = three_block_stream()
    cases.append(t)
    for k in range(len(t.stream)):
        cases.append(Case(f"prefix_{k}_of_{len(t.stream)}", t.stream[:k], None, ANY_ERROR, t.min_cap))
    return cases


# --------------------------------------------------------------- split path --
REGION = 32768  # compressed bytes per region of the split decoder (kSplitRegion)
RING = 16384    # symbols of history it keeps in LDS (kRing)


def _split_stream(name, seed, kind="fixed", target_len=None, tail=None, first_ops=None, n_regions=3,
                  bad_region1=False, blk=3000):
    """A stream of blocks of random literals over several regions.  kind
    "fixed": fixed blocks, a sync flush after each (block starts at byte
    boundaries, found by the flush marker); "dynamic": dynamic blocks, no
    flush (block starts at any bit, found by their headers).  The first block
    that starts inside a region k >= 1 opens with matches that reach before
    the region (markers): first_ops[k], then 63 and 64 symbols before it, the
    whole window (or all the output), and a copy of those copies.  Once the
    region holds more than 16,448 symbols a block opens with matches across
    the LDS ring's edge.  target_len: the exact compressed length; tail:
    "last_bytes" ends in an empty final block in the stream's last 6 bytes."""
    rng = _rng(seed)
    w = BitWriter()
    w.bits(0x78, 8)
    w.bits(0x9C, 8)
    toks_all = []
    total = 0          # bytes of output so far
    region = 0
    region_out = 0     # output at the region's first block start
    ring_done = True
    first_ops = first_ops or {}
    # blk literals per block: 3,000 are about 3,170 bytes
    if target_len is None and kind == "fixed":
        target_len = n_regions * REGION + 4000
    while True:
        at = w.tell() >> 3  # (fixed: byte-aligned here, after the flush)
        if kind == "fixed" and at + blk + 600 > target_len:
            break
        if kind == "dynamic" and at > n_regions * REGION + 1000:
            break
        toks = []
        k = at // REGION
        if k > region:
            region, region_out, ring_done = k, total, False
            r = 0  # symbols of the region so far
            for L, back in list(first_ops.get(k, [(5, 1)])) + [(20, 63), (20, 64)]:
                toks.append((L, r + back))  # a source that starts `back` symbols before the region
                r += L
            far_d = min(32768, total + r)
            if bad_region1 and k == 1:
                assert far_d < 32768
                far_d += 1  # one byte before the start of the output
            toks += [(258, far_d), (100, 50), (30, r + 358 + 1)]  # (100, 50) copies copies of markers
        elif not ring_done and total - region_out > RING + 200:
            ring_done = True
            for D in (16383, 16384, 16385, 16447, 16448):
                toks += [(3, D), (258, D), (70, D)]
        toks.append(rng.integers(0, 256, blk, dtype=np.uint8).tobytes())
        if kind == "fixed":
            fixed(toks, False)(w)
            sync_flush()(w)
        else:
            dynamic(toks, False)(w)
        total += expand_len(toks)
        toks_all += toks
    if kind == "fixed":
        # 8-bit literals, one stream byte each, to land on the exact length: a
        # fixed block of n of them is n + 2 bytes, a flush after it 4 more (its
        # header shares the block's last byte), the empty final block 2, Adler 4
        at = w.tell() >> 3
        n = target_len - at - 2 - 4 - (6 if tail == "last_bytes" else 0)
        lit = bytes(b % 144 for b in rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        toks_all.append(lit)
        if tail == "last_bytes":
            fixed([lit], False)(w)
            sync_flush()(w)
            fixed([], True)(w)
        else:
            fixed([lit], True)(w)
    else:
        lit = rng.integers(0, 256, 500, dtype=np.uint8).tobytes()
        dynamic([lit], True)(w)
        toks_all.append(lit)
    body = w.getvalue()
    if bad_region1:
        return Case(name, body + bytes(4), None, 5, 1 << 20)
    data = expand(toks_all)
    z = body + struct.pack(">I", zlib.adler32(data))
    assert target_len is None or len(z) == target_len, (len(z), target_len)
    return Case(name, z, data, 0, len(data))


def expand_len(toks):
    """The length of expand(toks)."""
    n = 0
    for t in toks:
        n += len(t) if isinstance(t, (bytes, bytearray)) else t[0] if isinstance(t, tuple) else 1
    return n


@functools.lru_cache(None)
def split_good():
    """Streams the split path must resolve itself."""
    # what each region's first block opens with: (L, symbols before the region)
    ops = {1: [(5, 1)], 2: [(258, 32768)], 3: [(70, 63)], 4: [(70, 64)]}
    return [
        _split_stream("split_fixed_sync_5_regions", 31, "fixed", first_ops=ops, n_regions=5),
        _split_stream("split_dynamic_no_flush_5_regions", 31, "dynamic", first_ops=ops, n_regions=5),
        _split_stream("split_len_65536", 33, "fixed", target_len=65536),
        _split_stream("split_final_block_in_last_bytes", 34, "fixed", target_len=3 * REGION, tail="last_bytes"),
        _split_stream("split_final_block_alone_in_last_region", 35, "fixed", target_len=2 * REGION + 6,
                      tail="last_bytes"),
    ]


@functools.lru_cache(None)
def split_short():
    """One byte under the two regions the split path starts at."""
    return [_split_stream("split_len_65535", 32, "fixed", target_len=65535)]


@functools.lru_cache(None)
def split_may_fall_back():
    """Streams the split path may hand back to the wave kernel (false block
    starts inside stored payloads), which must come out exact all the same."""
    cases = []
    noise = bytearray(_rand(4 * REGION, 41))
    for k in range(1, 4):  # a flush marker, then noise, where each region starts looking
        noise[k * REGION + 10:k * REGION + 14] = b"\x00\x00\xff\xff"
    cases.append(good("stored_payload_with_flush_markers",
                      [("s", bytes(noise[i:i + 30000])) for i in range(0, len(noise), 30000)]))
    inner = b""
    while len(inner) < 3 * REGION + 2000:
        inner += zlib.compress(text(40_000, 50 + len(inner)), 6)
    cases.append(good("stored_payload_of_zlib_streams",
                      [("s", inner[i:i + 65535]) for i in range(0, len(inner), 65535)]))
    cases.append(_split_stream("region_1_match_before_output_start", 36, "fixed", bad_region1=True, blk=1000))
    return cases
