"""A structural zlib decoder for the deflate tests (RFC 1950/1951), and the
length-limited optimum the device's code lengths are measured against.

``parse(stream)`` reads a zlib stream bit by bit and keeps what an inflater
throws away: where each block starts and ends, a dynamic block's HLIT, HDIST,
HCLEN, code-length code, the header operations as sent (literal lengths and
the 16/17/18 repeats) and the two length arrays they spell, and every token
with its symbols and extra values.  It is strict: anything the RFCs forbid
raises ``ParseError`` (over-subscribed and incomplete codes, a repeat with
nothing to repeat, a distance before the start of the output, a wrong Adler).
Like zlib it lets pass the two incomplete codes an encoder may need: a
literal/length or distance code of a single 1-bit code, and no distance code
at all.  Bytes after the Adler-32 are kept in ``Stream.trailing``.

``test_deflate_parse.py`` checks it against CPython's zlib and against the
streams ``deflate_craft`` dictated; ``test_gpu_deflate_structure.py`` reads
the device deflate's streams with it.

No dependence on the GPU.
"""
from __future__ import annotations

import heapq
import zlib

from tests.deflate_craft import (DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LITLEN, LEN_BASE, LEN_EXTRA, ORDER, _rev,
                                 canonical, expand)


class ParseError(ValueError):
    pass


class Match(tuple):
    """``(length, distance)`` (so ``deflate_craft.expand`` takes it) with the
    symbols and extra values it was sent as."""
    def __new__(cls, length, distance, lsym, lextra, dsym, dextra):
        m = tuple.__new__(cls, (length, distance))
        m.lsym, m.lextra, m.dsym, m.dextra = lsym, lextra, dsym, dextra
        return m

    length = property(lambda s: s[0])
    distance = property(lambda s: s[1])


class Block:
    """One deflate block.  ``start``/``end``: bit offsets in the zlib stream
    (bit 0 = the first bit of CMF) of BFINAL and of the bit after the block.
    ``tokens``: ints (literals), ``Match``es, or for a stored block one
    ``bytes``.  ``out_start``/``out_len``: the output bytes it produces."""

    def __init__(self):
        self.btype = self.bfinal = self.start = self.end = None
        self.hlit = self.hdist = self.hclen = None
        self.cl_lens = self.ops = self.litlen_lens = self.dist_lens = None
        self.tokens = []
        self.out_start = self.out_len = 0

    def litlen_counts(self):
        """symbol -> uses, the end of block included."""
        f = {256: 1}
        for t in self.tokens:
            s = t if isinstance(t, int) else t.lsym
            f[s] = f.get(s, 0) + 1
        return f

    def dist_counts(self):
        f = {}
        for t in self.tokens:
            if not isinstance(t, int):
                f[t.dsym] = f.get(t.dsym, 0) + 1
        return f

    def op_counts(self):
        f = {}
        for op in self.ops:
            f[op[0]] = f.get(op[0], 0) + 1
        return f


class Stream:
    def __init__(self):
        self.cmf = self.flg = self.adler = None
        self.blocks = []
        self.trailing = b""

    def expand(self) -> bytes:
        toks = []
        for b in self.blocks:
            toks += b.tokens
        return expand(toks)


class _Bits:
    def __init__(self, data, pos):
        self.d = data
        self.p = pos   # next byte to load
        self.acc = 0
        self.n = 0

    def need(self, k):
        while self.n < k:
            if self.p >= len(self.d):
                raise ParseError("the stream ends inside a block")
            self.acc |= self.d[self.p] << self.n
            self.p += 1
            self.n += 8

    def take(self, k):
        if k == 0:
            return 0
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def tell(self):
        return 8 * self.p - self.n


def kraft(lens, unit=15):
    """Sum of 2^-len over the used symbols, in units of 2^-unit."""
    return sum(1 << (unit - k) for k in lens if k)


def _table(lens, what, allow_single):
    """Decoding table of the canonical code: entry ``sym << 4 | nbits`` at
    every ``maxbits``-bit value whose low bits are the (bit-reversed) code, or
    -1.  Raises unless the code is complete (or one of zlib's exceptions)."""
    used = [k for k in lens if k]
    if not used:
        return None, 0
    if max(used) > 15:
        raise ParseError(f"{what}: a length above 15")
    k = kraft(lens)
    if k > 1 << 15:
        raise ParseError(f"over-subscribed {what} code")
    if k < 1 << 15 and not (allow_single and len(used) == 1 and used[0] == 1):
        raise ParseError(f"incomplete {what} code")
    mx = max(used)
    tab = [-1] * (1 << mx)
    for s, (c, n) in canonical(lens).items():
        tab[_rev(c, n)::1 << n] = [s << 4 | n] * (1 << (mx - n))
    return tab, mx


_FIXED_LL = _table(FIXED_LITLEN, "fixed", False)
_FIXED_D = _table(FIXED_DIST + [5, 5], "fixed", False)  # 30 and 31 have codes, and are invalid


def _symbol(br, tab, mx, what):
    if tab is None:
        raise ParseError(f"a {what} symbol in a block without {what} codes")
    if br.n < mx:  # near the end of the stream fewer bits may be left than the longest code
        while br.n < mx and br.p < len(br.d):
            br.acc |= br.d[br.p] << br.n
            br.p += 1
            br.n += 8
    e = tab[br.acc & ((1 << mx) - 1)]
    if e < 0:
        raise ParseError(f"an unused {what} code")
    n = e & 15
    if n > br.n:
        raise ParseError("the stream ends inside a block")
    br.acc >>= n
    br.n -= n
    return e >> 4


def _dynamic_header(br, b):
    b.hlit = br.take(5) + 257
    b.hdist = br.take(5) + 1
    b.hclen = br.take(4) + 4
    if b.hlit > 286 or b.hdist > 30:
        raise ParseError(f"HLIT {b.hlit} / HDIST {b.hdist}")
    cl = [0] * 19
    for k in range(b.hclen):
        cl[ORDER[k]] = br.take(3)
    b.cl_lens = cl
    tab, mx = _table(cl, "code-length", False)
    if tab is None:
        raise ParseError("incomplete code-length code")
    lens, ops = [], []
    total = b.hlit + b.hdist
    while len(lens) < total:
        s = _symbol(br, tab, mx, "code-length")
        if s < 16:
            ops.append((s,))
            lens.append(s)
            continue
        x = br.take((2, 3, 7)[s - 16])
        ops.append((s, x))
        if s == 16:
            if not lens:
                raise ParseError("a repeat of the length before the first")
            lens += [lens[-1]] * (3 + x)
        else:
            lens += [0] * ((3, 11)[s - 17] + x)
    if len(lens) > total:
        raise ParseError("a repeat runs past the lengths")
    b.ops = ops
    b.litlen_lens, b.dist_lens = lens[:b.hlit], lens[b.hlit:]
    if b.litlen_lens[256] == 0:
        raise ParseError("no end-of-block code")
    return _table(b.litlen_lens, "literal/length", True), _table(b.dist_lens, "distance", True)


def parse(stream) -> Stream:
    data = bytes(stream)
    st = Stream()
    if len(data) < 2:
        raise ParseError("no zlib header")
    st.cmf, st.flg = data[0], data[1]
    if st.cmf & 15 != 8 or st.cmf >> 4 > 7 or (st.cmf << 8 | st.flg) % 31 or st.flg & 0x20:
        raise ParseError("zlib header")
    br = _Bits(data, 2)
    written = 0
    while True:
        b = Block()
        b.start = br.tell()
        b.bfinal = br.take(1)
        b.btype = br.take(2)
        b.out_start = written
        if b.btype == 3:
            raise ParseError("BTYPE 3")
        if b.btype == 0:
            br.take(br.n & 7)
            n, nn = br.take(16), br.take(16)
            if n ^ nn != 0xFFFF:
                raise ParseError("stored LEN / NLEN")
            at = br.p - (br.n >> 3)  # whole bytes are buffered here
            if at + n > len(data):
                raise ParseError("the stream ends inside a stored block")
            b.tokens = [data[at:at + n]] if n else []
            br.p, br.acc, br.n = at + n, 0, 0
            written += n
        else:
            if b.btype == 1:
                (lt, lm), (dt, dm) = _FIXED_LL, _FIXED_D
            else:
                (lt, lm), (dt, dm) = _dynamic_header(br, b)
            toks = b.tokens
            while True:
                s = _symbol(br, lt, lm, "literal/length")
                if s < 256:
                    toks.append(s)
                    written += 1
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise ParseError(f"literal/length symbol {s}")
                lx = br.take(LEN_EXTRA[s - 257])
                ds = _symbol(br, dt, dm, "distance")
                if ds > 29:
                    raise ParseError(f"distance symbol {ds}")
                dx = br.take(DIST_EXTRA[ds])
                m = Match(LEN_BASE[s - 257] + lx, DIST_BASE[ds] + dx, s, lx, ds, dx)
                if m[1] > written:
                    raise ParseError(f"distance {m[1]} with {written} bytes written")
                toks.append(m)
                written += m[0]
        b.end = br.tell()
        b.out_len = written - b.out_start
        st.blocks.append(b)
        if b.bfinal:
            break
    at = br.p - (br.n >> 3)
    if at + 4 > len(data):
        raise ParseError("no Adler-32")
    st.adler = int.from_bytes(data[at:at + 4], "big")
    st.trailing = data[at + 4:]
    if st.adler != zlib.adler32(st.expand()):
        raise ParseError("wrong Adler-32")
    return st


# ------------------------------------------------------- reference lengths --
def _freqs(freq):
    return sorted(int(f) for f in (freq.values() if isinstance(freq, dict) else freq) if f > 0)


def huffman_cost(freq) -> int:
    """sum(freq * length) of an unlimited Huffman code (one symbol: 1 bit)."""
    h = _freqs(freq)
    if len(h) == 1:
        return h[0]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        s = heapq.heappop(h) + heapq.heappop(h)
        cost += s
        heapq.heappush(h, s)
    return cost


def unlimited_depth(freq) -> int:
    """The longest code of the plain Huffman tree of these counts; among equal
    weights a leaf is taken before a merged node and the older node first (the
    two-queue rule, which gives the shallowest of the optimal trees)."""
    h = [(f, 0, i, 0) for i, f in enumerate(_freqs(freq))]  # weight, merged?, age, height
    if len(h) <= 1:
        return len(h)
    heapq.heapify(h)
    age = len(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], 1, age, max(a[3], b[3]) + 1))
        age += 1
    return h[0][3]


def optimal_limited_lengths(freq, maxbits):
    """Package-merge (Larmore and Hirschberg 1990): code lengths, none above
    ``maxbits``, of least sum(freq * length).  ``freq``: a dict or a list;
    returns the same shape, 0 for unused symbols.  One used symbol gets one
    bit."""
    items = list(freq.items()) if isinstance(freq, dict) else list(enumerate(freq))
    used = sorted((int(f), s) for s, f in items if f > 0)
    out = {s: 0 for s, _ in items}
    n = len(used)
    if n == 1:
        out[used[0][1]] = 1
    elif n > 1:
        if n > 1 << maxbits:
            raise ValueError("more symbols than codes")
        leaves = [(f, (i,)) for i, (f, _) in enumerate(used)]
        prev = list(leaves)
        for _ in range(maxbits - 1):
            pk = [(prev[k][0] + prev[k + 1][0], prev[k][1] + prev[k + 1][1]) for k in range(0, len(prev) - 1, 2)]
            prev = sorted(leaves + pk, key=lambda x: x[0])
        depth = [0] * n
        for _, members in prev[:2 * n - 2]:
            for i in members:
                depth[i] += 1
        for i, (_, s) in enumerate(used):
            out[s] = depth[i]
    return out if isinstance(freq, dict) else [out[s] for s, _ in items]


def coded_cost(freq, lens) -> int:
    get = lens.__getitem__ if not isinstance(lens, dict) else (lambda s: lens.get(s, 0))
    items = freq.items() if isinstance(freq, dict) else enumerate(freq)
    return sum(f * get(s) for s, f in items if f > 0)
