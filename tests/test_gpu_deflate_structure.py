"""GPU: the structure of the device deflate's streams (K7, hbx_deflate.hip),
read back with tests/deflate_parse.py.

test_gpu_deflate.py checks that zlib inflates every stream to its input.
That can fail only on a branch some input reaches; here every stream is also
decoded structurally, checked against the invariants the kernel's own design
states (``check_stream``), and a set of seeded inputs is built to drive K7h's
code construction down each of its branches, with the branch taken asserted
from the decoded stream: the length limit of the literal/length and distance
codes (one rebuild and more than one), the length limit of the code-length
code, no / one distance symbol, the header's run-length coder at its edges,
the widest token, every length and distance symbol at both ends of its extra
bits, and a group member whose bits do not fit its image.

Coded cost against the optimum.  sum(count * emitted length) over a code's
symbols cannot be below the same sum under package-merge's lengths (limit
15).  K7h builds a Huffman tree of count | 1, and while it is deeper than 15
rebuilds it from (count >> shift) | 1, which is not optimal.  Two assertions:

* every dynamic block, whatever the parse made of it (``tie_allowance``):
  the excess in bits is at most what the rule can cost.  With no rebuild the
  emitted code is optimal for count | 1, so against any other code it loses
  at most that code's lengths summed over the symbols of even count; after
  ``shift`` rebuilds the weights are off by at most 2^shift per symbol, so
  it loses at most 2^shift times both codes' lengths summed.  This bound
  does not depend on which matches the parse found (K7a's candidate search
  races inside a round, so the small blocks of the mixed batch give other
  counts, and ratios of 1.001 to 1.006, from run to run);
* the inputs whose counts are dictated (deep_litlen, deep_dist, deep_cl and
  the literal-only header cases, ``dictated=True``): the ratio of the two
  sums over both codes.  The largest measured on the MI355X is
  RATIO_MEASURED (below): 6 bits in 620,624 at deep_dist, 3 in 793,044 at
  deep_litlen's twice rebuilt code, none elsewhere.  The tests assert that
  plus a quarter of its excess over 1 (7 bits at deep_dist): a change to
  the halving heuristic that costs more must fail here.
"""
import functools

import numpy as np
import pytest

from oracle import deflate as OD
from tests import deflate_parse as P
from tests.deflate_craft import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, ORDER
from tests.test_gpu_deflate import _check, _text

pytestmark = pytest.mark.gpu

SEG = 32768      # kSeg: bytes per segment
GROUP = 4        # kGroup: segments that may share one code
FAR4 = 1024      # kFar4: the farthest 4-byte match kept
ROUND = 512      # kRound: positions K7a looks up and inserts between two barriers
IMG_BYTES = 4 * ((SEG + 16) // 4 + 4)  # 4 * kImgWords: a member's image
RATIO_MEASURED = 620630 / 620624  # 1.00001, deep_dist; deep_litlen's twice rebuilt code: 793047 / 793044
RATIO_BOUND = RATIO_MEASURED + (RATIO_MEASURED - 1.0) / 4
WORST = {"ratio": 1.0, "where": None}  # the largest dictated ratio seen in this session (printed as it grows)


# ------------------------------------------------------------- invariants --
def fixed_code_bits(tokens):
    """Bits of these tokens under the fixed code (RFC 1951 §3.2.6), without
    the block header and the end of block."""
    bits = 0
    for t in tokens:
        if isinstance(t, int):
            bits += 8 if t < 144 else 9
        else:
            bits += (7 if t.lsym < 280 else 8) + LEN_EXTRA[t.lsym - 257] + 5 + DIST_EXTRA[t.dsym]
    return bits


def header_ops(seq):
    """The run-length coding of the code lengths as K7h states it (zlib's
    order): zeros in runs of 11-138 (18), then one of 3-10 (17), then single
    zeros; a length once, then repeats of 3-6 (16), then the length again."""
    ops, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        cur, r = seq[i], j - i
        if cur == 0:
            while r >= 11:
                q = min(r, 138)
                ops.append((18, q - 11))
                r -= q
            if r >= 3:
                ops.append((17, r - 3))
                r = 0
        else:
            ops.append((cur,))
            r -= 1
            while r >= 3:
                q = min(r, 6)
                ops.append((16, q - 3))
                r -= q
        ops += [(cur,)] * r
        i = j
    return ops


def partner(x):
    """The second 1-bit distance code K7h sends beside the only used symbol x
    (or beside none: symbols 0 and 1), so that the code is complete."""
    lens = [0] * (max(x, 1) + 1)
    lens[x] = lens[0 if x else 1] = 1
    return lens


def halved(freq, shift):
    """The weights K7h builds a tree from: shift 0 first, then one more for
    every tree that came out too deep."""
    return {s: (f >> shift) | 1 for s, f in freq.items()}


def rebuilds(freq, limit=15):
    """How often K7h rebuilds the tree of these counts: its two-queue merge
    takes a leaf before a merged node of the same weight, which gives the
    shallowest Huffman tree, as P.unlimited_depth does."""
    shift = 0
    while P.unlimited_depth(halved(freq, shift)) > limit:
        shift += 1
    return shift


def k7h_lengths(freq, limit=15):
    """Code lengths by K7h's stated rule, which the counts determine: symbols
    in the order of count << 9 | symbol, a two-queue Huffman merge of
    (count >> shift) | 1 that takes a leaf before a merged node of the same
    weight, rebuilt with the next shift while deeper than the limit."""
    keys = sorted((f << 9) | s for s, f in freq.items())
    m = len(keys)
    if m == 1:
        return {keys[0] & 511: 1}
    for shift in range(32):
        w = [((k >> 9) >> shift) | 1 for k in keys] + [0] * (m - 1)
        par = [0] * (2 * m - 1)
        i, j = 0, m
        for k in range(m, 2 * m - 1):
            for _ in range(2):
                if i < m and (j >= k or w[i] <= w[j]):
                    a, i = i, i + 1
                else:
                    a, j = j, j + 1
                w[k] += w[a]
                par[a] = k
        depth = [0] * (2 * m - 1)
        for k in range(2 * m - 3, -1, -1):
            depth[k] = depth[par[k]] + 1
        if max(depth[:m]) <= limit:
            return {keys[t] & 511: depth[t] for t in range(m)}


def tie_allowance(freq, lens, opt):
    """The most bits K7h's code ``lens`` can cost over the code ``opt`` (see
    the module's docstring).  No allowance for fewer than two symbols."""
    if len(freq) < 2:
        return 0
    shift = rebuilds(freq)
    if shift == 0:
        return sum(opt[s] for s, f in freq.items() if f % 2 == 0)
    return (1 << shift) * sum(lens[s] + opt[s] for s in freq)


def check_codes(b, where, dictated=False):
    lf, df = b.litlen_counts(), b.dist_counts()
    assert max(b.litlen_lens + b.dist_lens) <= 15, where
    # a code for every symbol used and for no other
    assert {s for s, k in enumerate(b.litlen_lens) if k} == set(lf), where
    assert len(lf) >= 2 and P.kraft(b.litlen_lens) == 1 << 15, where
    assert b.hlit == max(257, max(lf) + 1), where
    if len(df) >= 2:
        assert {s for s, k in enumerate(b.dist_lens) if k} == set(df), where
        assert P.kraft(b.dist_lens) == 1 << 15, where
    else:
        assert b.dist_lens == partner(min(df) if df else 0), (where, b.dist_lens)
    of = b.op_counts()
    used = {s for s, k in enumerate(b.cl_lens) if k}
    assert max(b.cl_lens) <= 7, where
    if len(of) >= 2:
        assert used == set(of) and P.kraft(b.cl_lens, 7) == 1 << 7, (where, b.cl_lens)
    else:
        x = min(of)
        assert used == {x, 0 if x else 1} and all(b.cl_lens[s] == 1 for s in used), (where, b.cl_lens)
    assert b.hclen == max(4, max(ORDER.index(s) for s in used) + 1), where
    assert b.ops == header_ops(b.litlen_lens + b.dist_lens), where
    # coded cost against the length-limited optimum
    cost = best = 0
    for f, lens in ((lf, b.litlen_lens), (df, b.dist_lens)):
        opt = P.optimal_limited_lengths(f, 15)
        c, o = P.coded_cost(f, lens), P.coded_cost(f, opt)
        assert 0 <= c - o <= tie_allowance(f, lens, opt), (where, c, o, tie_allowance(f, lens, opt), f)
        cost, best = cost + c, best + o
    if dictated:
        ratio = cost / best
        if ratio > WORST["ratio"]:
            WORST.update(ratio=ratio, where=where)
            print(f"coded cost / optimum: {ratio:.6f} ({cost} / {best}) at {where}")
        assert ratio <= RATIO_BOUND, (where, ratio, cost, best)


def check_stream(data, z, name="", dictated=False):
    """Every exact invariant of one stream; returns the parsed stream."""
    st = P.parse(z)
    assert st.trailing == b"" and st.expand() == bytes(data), name
    n, blocks = len(data), st.blocks
    nseg = -(-n // SEG)
    # layout: non-final pieces, then 01 00 00 FF FF and the Adler-32
    last = blocks[-1]
    assert bytes(z[-9:-4]) == b"\x01\x00\x00\xff\xff" and last.start == 8 * (len(z) - 9), name
    assert (last.bfinal, last.btype, last.out_len) == (1, 0, 0), name
    assert all(b.bfinal == 0 for b in blocks[:-1]), name
    covered, i = 0, 0
    while i < len(blocks) - 1:
        b = blocks[i]
        where = f"{name} block {i} at output {b.out_start}"
        assert b.start % 8 == 0 and b.out_start == covered and covered % SEG == 0, where
        s0 = covered // SEG
        if b.btype == 0:
            k, piece = 1, (b.end - b.start) // 8
            assert b.out_len == min(SEG, n - covered) > 0 and piece == 5 + b.out_len, where
            i += 1
        else:
            flush = blocks[i + 1]
            assert i + 1 < len(blocks) - 1, where
            assert (flush.btype, flush.out_len) == (0, 0) and flush.end % 8 == 0 and flush.end - b.end <= 3 + 7 + 32, where
            piece = (flush.end - b.start) // 8
            k = -(-b.out_len // SEG)
            assert b.out_len > 0 and (b.out_len % SEG == 0 or covered + b.out_len == n), where
            if k > 1:  # a shared code: the whole group, dynamic
                g0 = s0 - s0 % GROUP
                assert b.btype == 2 and s0 == g0 and k == min(GROUP, nseg - g0), where
            # tokens: none across a segment's end; the parse's limits
            pos = covered
            seg_tok = [[] for _ in range(k)]
            for t in b.tokens:
                ln = 1 if isinstance(t, int) else t.length
                assert pos // SEG == (pos + ln - 1) // SEG, (where, pos, t)
                if ln > 1:
                    assert 4 <= ln <= 258 and 1 <= t.distance <= 32768, (where, pos, t)
                    assert ln > 4 or t.distance <= FAR4, (where, pos, t)
                    assert LEN_BASE[t.lsym - 257] + t.lextra == ln and t.lsym == (285 if ln == 258 else t.lsym), (where, t)
                    assert t.lsym != 284 or t.lextra < 31, (where, pos, t)  # 258 goes as 285
                seg_tok[pos // SEG - s0].append(t)
                pos += ln
            # size: smaller than its segments' fixed-or-stored pieces (K7h's decision rule)
            alone = []
            for m in range(k):
                nm = min(SEG, n - (s0 + m) * SEG)
                fm = ((3 + fixed_code_bits(seg_tok[m]) + 7 + 3 + 7) >> 3) + 4
                alone.append((5 + nm, fm))
            if b.btype == 1:
                assert piece == alone[0][1] < alone[0][0], (where, piece, alone)
            else:
                assert piece < sum(min(a) for a in alone), (where, piece, alone)
                check_codes(b, where, dictated)
            i += 2
        covered += b.out_len
    assert covered == n, name
    return st


def verify(engine, blocks, names=None, dictated=()):
    """dictated: True, or the names of the blocks whose counts the input dictates."""
    outs = _check(engine, blocks)  # strict inflate by zlib, deflate_bound, 78 9C
    names = names or [f"block {i}" for i in range(len(blocks))]
    return [check_stream(b, z, nm, dictated is True or nm in dictated) for b, z, nm in zip(blocks, outs, names)]


def dynamic_blocks(st):
    return [b for b in st.blocks if b.btype == 2]


# ------------------------------------------------------------- generators --
def _rng(seed):
    return np.random.default_rng(seed)


def chain(below, n, slack=0.04):
    """n counts that continue the counts ``below`` as a chain: the Huffman
    tree of below + chain has one level per count, because each count exceeds
    the sum of all counts before its predecessor (by ``slack`` and a little,
    so that a few stray symbols do not break it).  Fibonacci numbers are the
    tight case and do not do: K7h weighs a count as count | 1, which breaks
    their ties, and so does the end of block's count of 1.  All odd."""
    seq = list(below)
    for _ in range(n):
        seq.append(max(seq[-1], int(sum(seq[:-1]) * (1 + slack)) + 2) | 1)
    return seq[len(below):]


def _zhash(buf):
    """K7a's bucket of the 4 bytes at each position (2,048 buckets of the 16
    latest positions): used to place a far source where its bucket is quiet."""
    a = np.frombuffer(bytes(buf) + bytes(3), np.uint8).astype(np.uint64)
    x = a[:-3] | (a[1:-2] << np.uint64(8)) | (a[2:-1] << np.uint64(16)) | (a[3:] << np.uint64(24))
    return ((x * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(21)


def spread(counts, seed, unique4=True):
    """Bytes with exactly these counts in a random order in which (unique4) no
    4-byte string occurs twice, so that the parse finds no match and the
    block's literal counts are these."""
    rng = _rng(seed)
    arr = np.repeat(np.array(list(counts), np.uint8), list(counts.values()))
    rng.shuffle(arr)
    for _ in range(2000 if unique4 else 0):
        a = arr.astype(np.uint32)
        g = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)
        order = np.argsort(g, kind="stable")
        dup = order[1:][g[order][1:] == g[order][:-1]]
        if dup.size == 0:
            break
        for i in dup:
            k, j = int(i) + int(rng.integers(0, 4)), int(rng.integers(0, arr.size))
            arr[k], arr[j] = arr[j], arr[k]
    else:
        assert not unique4, "no order without a repeated 4-byte string found"
    return arr.tobytes()


def deep_litlen(n, slack, rare_high, seed):
    """Four segments of literals and no match: 64 equally frequent byte values
    (a subtree 6 deep) over ``n`` rare values whose counts form a chain above
    the end of block: unlimited depth n + 7.  rare_high: the rare values are
    9-bit literals of the fixed code and the frequent ones 8-bit, or the
    other way round."""
    rare = list(range(160, 160 + n)) if rare_high else list(range(3, 3 + n))
    flat = list(range(40, 104)) if rare_high else list(range(150, 214))
    counts = dict(zip(rare, chain([1], n, slack)))
    rest = GROUP * SEG - sum(counts.values())
    assert rest // 64 > 1.1 * max(counts.values())
    for i, v in enumerate(flat):
        counts[v] = rest // 64 + (1 if i < rest % 64 else 0)
    return spread(counts, seed)


def dyadic(lens, L, seed):
    """A block of 2^L - 1 literals in which byte v occurs 2^(L - lens[v])
    times and no 4-byte string twice: with the end of block (once, L bits) the
    counts are exact powers of two that sum to 2^L, so every Huffman code of
    them has exactly these lengths."""
    assert sum(1 << (L - k) for k in lens.values()) == (1 << L) - 1, "not a complete code with the end of block"
    return spread({v: 1 << (L - k) for v, k in lens.items()}, seed)


def alphabet(tail, L=12, lead=256, core_len=4):
    """Code lengths by byte value for ``dyadic``: ``tail`` dictates the
    lengths of the last byte values as runs [(length or 0, count), ...]; the
    values before them are filled so that the whole code is complete: a few
    single lengths, a zero, a core of core_len-bit values, a zero, and runs of
    (L-1)-bit and L-bit values that take what is left.  Returns {value: length}; the
    tail starts at value 256 - sum of its counts."""
    tail_seq = [k for k, c in tail for _ in range(c)]
    room = lead - len(tail_seq)
    used = sum(1 << (L - k) for k in tail_seq if k) + 1  # + the end of block
    for core in range((1 << core_len) - 1, 1 << (core_len - 1), -1):
        for deep in range(0, room):
            for absorb in range(1, room):
                rest = (1 << L) - used - core * (1 << (L - core_len)) - 2 * deep - absorb
                if rest < 0 or rest >> (L - core_len):
                    continue
                fill = [L - i for i in range(L - core_len) if rest >> i & 1]  # distinct lengths, by binary digits
                head = sorted(fill) + [0] + [core_len] * core + [0] + [L - 1] * deep + [L] * absorb
                if len(head) == room and tail_seq[0] != L:
                    return {v: k for v, k in enumerate(head + tail_seq) if k}
    raise AssertionError("no complete alphabet for this tail")


def one_distance_far(dist, n, seed):
    """Random bytes over 200 values with period ``dist`` > 512: every match
    lies ``dist`` back (a nearer copy does not exist, a farther one is never
    longer and loses the tie)."""
    per = _rng(seed).integers(0, 200, dist, dtype=np.uint8).tobytes()
    return (per * (n // dist + 1))[:n]


class Builder:
    """Data built token by token: fresh random bytes and copies of earlier
    bytes at dictated distances.  A source starts with four fresh bytes, two
    or more from any other source's start (two copies then share four bytes
    at most, too few for a candidate), so the dictated distance is the only
    candidate of full length; no copy crosses a segment's end.  In K7a's
    rounds of 512 positions every position reads its bucket and then inserts
    itself, with a barrier only between rounds: a later position of the round
    may or may not see an earlier one, so a source is seen for certain only if
    it starts in an earlier round, and a copy from less than 512 back is put
    early enough in its round."""

    def __init__(self, seed, values=200):
        self.rng = _rng(seed)
        self.values = values
        self.out = bytearray()
        self.clean = bytearray()  # 1: a fresh byte; 2: one a copy's source starts at

    def fresh(self, k, value=None):
        b = bytes([value]) * k if value is not None else self.rng.integers(0, self.values, k, dtype=np.uint8).tobytes()
        self.out += b
        self.clean += b"\x01" * k

    def room(self, length):
        """Fresh bytes up to the segment's end when ``length`` more would cross it."""
        p = len(self.out)
        if p % SEG + length > SEG:
            self.fresh(SEG - p % SEG)

    def copy(self, length, dists, lead=3, quiet=None, pad=True):
        """``lead`` or more fresh bytes, then ``length`` bytes from one of the
        distances ``dists`` (an int or a range) back.  quiet: also require
        that fewer than this many later positions share the source's hash
        bucket (a far source must still be among the bucket's 16 latest)."""
        if isinstance(dists, int):
            dists = range(dists, dists + 1)
        if pad:
            self.fresh(max(lead, dists[0] if dists[0] < length else 0))
        for _ in range(4000):
            self.room(length)
            p = len(self.out)
            for dist in (dists if len(dists) == 1 else self.rng.integers(dists[0], dists[-1] + 1, 48).tolist()):
                q = p - dist
                ok = q >= 0 and q // ROUND < p // ROUND and (
                    dist < length or (all(self.clean[q:q + 4]) and 2 not in self.clean[max(q - 1, 0):q + 2]))
                if ok and quiet is not None:
                    h = _zhash(self.out[q:])
                    ok = int((h[1:] == h[0]).sum()) < quiet
                if ok:
                    break
            if ok:
                break
            self.fresh(1)
        else:
            raise AssertionError(f"no place for a copy of {length} from {dists} back")
        if self.clean[q]:
            self.clean[q] = 2
        for k in range(length):
            self.out.append(self.out[q + k])
        self.clean += bytes(length)
        return dist


def one_distance(dist, length, k, seed):
    """k copies of ``length`` bytes from ``dist`` back between fresh bytes
    (for dist < length: of the last ``dist`` bytes, over and over), each where
    its source lies in an earlier round, so that ``dist`` is the only distance."""
    b = Builder(seed, values=100)
    b.fresh(ROUND)
    for i in range(k):
        if dist == 1:  # a run byte of its own for every run (the fresh bytes are below 100), on a round's last byte
            b.fresh((-len(b.out) - 1) % ROUND + (ROUND if (-len(b.out) - 1) % ROUND < 3 else 0))
            b.fresh(1, 100 + i)
        b.copy(length, dist, pad=dist > 1)
    b.fresh(9)
    return bytes(b.out)


@functools.lru_cache(None)
def across_hlit():
    """Four segments of fresh bytes, then 15 KiB of a fifth (coded alone) of
    matches only, round by round: 258 bytes from 1 back (symbol 285, distance
    symbol 0; left out of two rounds) and two copies of 127 bytes from the
    fourth segment (symbol 280; distance symbols 28 and 29).  28 + 30 + 30 uses
    give distance symbol 0 two bits, 1 + 28 + 64 uses give symbol 285 two
    bits: the run 2, 2 lies across HLIT = 286."""
    b = Builder(17, values=100)
    b.fresh(4 * SEG)
    far = [range(DIST_BASE[28], DIST_BASE[29]), range(DIST_BASE[29], 32769)]
    for r in range(30):
        if r in (10, 20):
            b.copy(131, far[0], lead=0, quiet=12, pad=False)
            b.copy(127, far[1], lead=0, quiet=12, pad=False)
        else:
            b.copy(258, 1, pad=False)
        b.copy(127, far[0], lead=0, quiet=12, pad=False)
        b.copy(127, far[1], lead=0, quiet=12, pad=False)
        assert len(b.out) == 4 * SEG + (r + 1) * ROUND, "a copy did not fit where it was meant to go"
    return bytes(b.out)


def length_of(sym, extra):
    return LEN_BASE[sym - 257] + extra


DEEP_DIST_SYMBOLS = 18


@functools.lru_cache(None)
def deep_dist():
    """One group: copies of 5 bytes over 18 distance symbols used 1, 1, 3, 5,
    7, 13, 19, ... 4,343 times (a chain: unlimited depth 17): 29, 28, 27, 26,
    then 12..17 (from less than 512 back: few, and placed at the start of a
    round), then 25 down to 18.  Between them six fresh bytes each over 230
    values, with rarer values in chained counts under them, which puts the
    length symbols 281-284 (one use each) 13 or more bits deep.  The two
    farthest copies are the widest tokens: 162 = symbol 281 + extra 31 at
    24,576 = symbol 28 + extra 8,191 and 257 = symbol 284 + extra 30 at 32,768
    = symbol 29 + extra 8,191.  (19 symbols do not fit: the chain has to be a
    little steeper than Fibonacci's, see chain(), and a copy with the fresh
    bytes that keep its source unique takes 11 bytes of the group's 131,072.)"""
    b = Builder(77, values=230)
    rng = b.rng
    b.fresh(400)
    order = [27, 26, 12, 13, 14, 15, 16, 17, 25, 24, 23, 22, 21, 20, 19, 18]
    counts = dict(zip(order, chain([1, 1], DEEP_DIST_SYMBOLS - 2, slack=0.03)))
    plan = [s for s in order if s >= 18 for _ in range(counts[s])]
    near = [s for s in order if s < 18 for _ in range(counts[s])]
    rng.shuffle(plan)
    rng.shuffle(near)
    rare = [230 + i for i, c in enumerate(chain([1, 1, 1, 1, 1, 2], 8)) for _ in range(c)]
    rng.shuffle(rare)
    long_ones = {27: length_of(282, 0), 26: length_of(283, 31)}  # 163 and 226 bytes, once each
    stride, waiting, i, done = len(plan) // len(rare), {}, 0, 0  # waiting: symbol -> copies put off
    while i < len(plan) or waiting or near:
        fits = [s for s in waiting if DIST_BASE[s] + 300 <= len(b.out)]  # (a dozen keys at most)
        if near and len(b.out) > 600 and (len(b.out) + 6) % ROUND < 80:
            s = near.pop()  # early in a round: any source 97 or more back lies in an earlier one
        elif fits:
            s = fits[0]
            waiting[s] -= 1
            if not waiting[s]:
                del waiting[s]
        elif i == len(plan):
            b.fresh(64)
            continue
        else:
            s = plan[i]
            i += 1
            if DIST_BASE[s] + 300 > len(b.out):
                waiting[s] = waiting.get(s, 0) + 1  # too early for a source that far back
                continue
        done += 1
        if rare and done % stride == 0:
            b.fresh(1, rare.pop())
        hi = min(DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1, len(b.out))
        b.copy(long_ones.pop(s, None) or 5, range(DIST_BASE[s], hi + 1), lead=6)
    while rare:
        b.fresh(1, rare.pop())
        b.fresh(3)
    assert not long_ones
    b.copy(length_of(281, 31), 24576, lead=6, quiet=9)
    b.copy(length_of(284, 30), 32768, lead=6, quiet=9)
    assert len(b.out) <= GROUP * SEG, len(b.out)
    return bytes(b.out)


@functools.lru_cache(None)
def len_dist_extremes():
    """A few segments: fresh bytes, then copies for every length symbol
    258..285 and every distance symbol 0..29 at extra value 0 and at its
    largest (4-byte copies only at 1,024 or nearer, which the parse keeps)."""
    lengths = []
    for i in range(1, 29):
        lengths += sorted({LEN_BASE[i], LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1})
    lengths[lengths.index(258)] = 257  # symbol 284 ends at extra 30; 258 is symbol 285
    dists = []
    for s in range(30):
        dists += sorted({DIST_BASE[s], DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1})
    b = Builder(91)
    b.fresh(SEG + 600)
    k = 0
    for rep in range(2):  # every distance meets two lengths, every length several distances
        for d in dists:
            ln = lengths[k % len(lengths)]
            k += 1
            if ln == 4 and d > FAR4:
                ln = 5
            b.copy(ln, d, lead=3, quiet=9 if d > 12000 else None)
    for ln in lengths:  # every length once more at a near distance, whatever the pairing above did
        b.copy(ln, 600 + ln, lead=3)
    b.fresh(50)
    assert len(b.out) <= 4 * SEG
    return bytes(b.out)


@functools.lru_cache(None)
def deep_cl():
    """4,095 literals whose code lengths, in byte order, cost the header 1, 1,
    2, 3, 7, 9, 17, 25, 43 and 67 operations of ten kinds (18, 17, the two
    1-bit distance codes, 0, 16, and the lengths 5, 7, 10, 8, 12): each count
    exceeds the sum of all before the one before it, also as K7h weighs them
    (count | 1), so the code-length code is a chain 9 deep before its limit
    of 7.  21 values of 5 bits (four runs of four), 17 of 7, 25 of 10, 43 of 8
    and 75 of 12 (three runs of four; the end of block is the 76th): 21/32 +
    17/128 + 25/1024 + 43/256 + 76/4096 = 1."""
    items = [[5] * 4] * 4 + [[12] * 4] * 3 + [[5]] * 5 + [[7]] * 17 + [[10]] * 25 + [[8]] * 43 + [[12]] * 63
    seq, prev, placed = [], 0, 0
    while items:  # the kind with most items left that differs from the one before
        kinds = sorted({it[0] for it in items if it[0] != prev}, key=lambda k: (-sum(it[0] == k for it in items), k))
        it = max((it for it in items if it[0] == kinds[0]), key=len)
        items.remove(it)
        placed += 1
        if placed in (20, 50, 80):
            seq.append(0)       # three single zeros
        elif placed == 110:
            seq += [0] * 10     # a run of ten: 17
        seq += it
        prev = it[0]
    assert len(seq) == 194
    lens = {v: k for v, k in enumerate(seq) if k}  # 62 zeros follow: 18
    return dyadic(lens, 12, 5)


RLE_TAILS = {
    # value 63 opens 138 zeros (the next run starts three 64-bit words on); zeros of 10 and 11; equal runs of 3, 4, 7, 8
    "start_63": [(0, 138), (9, 1), (0, 10), (9, 1), (0, 11), (9, 1), (10, 3), (9, 1), (10, 4), (9, 1), (10, 7), (9, 1),
                 (10, 8), (9, 1), (10, 1), (9, 1), (10, 1), (9, 1), (11, 1)],
    "start_127": [(0, 129)],               # zeros from 127 to the end of block
    "start_191": [(0, 65)],                # zeros from 191: the next run starts at 256 = 191 + 65
    "start_255": [(9, 1), (12, 1)],        # value 255 and the end of block: one run from lane 63 into the fifth word
    "zeros_139": [(0, 139), (9, 1)],       # 18 for 138, then a single zero
    "zeros_160": [(0, 160), (9, 1)],       # two 18s
}
assert 256 - sum(c for _, c in RLE_TAILS["start_63"]) == 63


@functools.lru_cache(None)
def rle_cases():
    cases = {name: dyadic(alphabet(tail), 12, 300 + i) for i, (name, tail) in enumerate(sorted(RLE_TAILS.items()))}
    cases["across_hlit"] = across_hlit()
    cases["far_period"] = one_distance_far(30000, 2 * SEG, 8)   # HDIST 30
    cases["length_15"] = dyadic(alphabet([(9, 1)], L=15, core_len=6), 15, 9)  # a 15-bit code: HCLEN 19
    return cases


def header_features(b):
    """What the header of one dynamic block shows of the run-length coder's
    edges, from the decoded lengths (which check_codes ties to the operations)."""
    f = set()
    seq = b.litlen_lens + b.dist_lens
    i = 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        r = j - i
        if seq[i] == 0:
            if r in (10, 11, 138, 139):
                f.add(f"zeros_{r}")
            if r >= 149:
                f.add("zeros_149_or_more")
        elif r in (3, 4, 7, 8):
            f.add(f"equal_{r}")
        if i < b.hlit < j:
            f.add("run_across_hlit")
        if i in (63, 127, 191) and j >= i + 65:
            f.add(f"start_{i}_next_65_later")
        if i == 255 and j > 256:
            f.add("start_255_into_next_word")
        i = j
    f.add(f"hlit_{b.hlit}")
    f.add(f"hdist_{b.hdist}")
    f.add(f"hclen_{b.hclen}")
    # what the operations themselves say
    ops = b.ops
    for k, op in enumerate(ops):
        if op == (18, 127) and k + 1 < len(ops) and ops[k + 1][0] == 18:
            f.add("two_18s")
        if op == (18, 127) and k + 1 < len(ops) and ops[k + 1] == (0,):
            f.add("18_then_zero")
        if op[0] == 16 and op[1] == 3 and k + 1 < len(ops) and ops[k + 1] == ops[k - 1]:
            f.add("16_then_remainder")
        if op in ((17, 7), (18, 0)):
            f.add("17_18_switch_%d" % op[0])
    return f


# feature -> the case of rle_cases() that shows it.  (HCLEN 4 is left out: a
# valid block sends a length other than 0, and the first of those in the
# header's order, 8, is the fifth entry; with K7h's 1-bit distance codes for
# no or one distance symbol HCLEN is 18, or 19 once a 15-bit code exists.)
FEATURES = {
    "zeros_10": "start_63", "zeros_11": "start_63", "zeros_138": "start_63", "zeros_139": "zeros_139",
    "zeros_149_or_more": "zeros_160", "two_18s": "zeros_160", "18_then_zero": "zeros_139",
    "17_18_switch_17": "start_63", "17_18_switch_18": "start_63",
    "equal_3": "start_63", "equal_4": "start_63", "equal_7": "start_63", "equal_8": "start_63",
    "16_then_remainder": "start_63",
    "run_across_hlit": "across_hlit",
    "start_63_next_65_later": "start_63", "start_127_next_65_later": "start_127",
    "start_191_next_65_later": "start_191", "start_255_into_next_word": "start_255",
    "hlit_257": "start_63", "hlit_286": "across_hlit", "hdist_30": "far_period",
    "hclen_18": "start_63", "hclen_19": "length_15",
}
# (HDIST 1 cannot occur either: K7h always sends two distance lengths or more.)


# ------------------------------------------------------------------ tests --
def test_mixed_batch_inputs_hold_the_invariants(engine):
    """The inputs of test_gpu_deflate.test_mixed_batch, built the same way."""
    rng = np.random.default_rng(7)
    blocks = []
    for i in range(400):
        n = int(rng.choice([0, 1, 17, 4096, 16384, 40000, 70000, 200000]))
        kind = i % 4
        if kind == 0:
            blocks.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        elif kind == 1:
            blocks.append(_text(n, i))
        elif kind == 2:
            blocks.append(bytes([i & 255]) * n)
        else:
            per = rng.integers(0, 256, 37, dtype=np.uint8).tobytes()
            blocks.append((per * (n // 37 + 1))[:n])
    sts = verify(engine, blocks)
    assert sum(len(dynamic_blocks(st)) for st in sts) > 100


def test_shared_code_group_inputs_hold_the_invariants(engine):
    """The small blocks of test_gpu_deflate.test_shared_code_groups."""
    seg = SEG
    t = _text(12 * seg, 3)
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 256, seg, dtype=np.uint8).tobytes()
    blocks = [t[:n] for n in (seg + 1, seg + 3, 2 * seg + 5, 3 * seg + 1, 4 * seg, 4 * seg + 3, 5 * seg + 17,
                              9 * seg + 100)]
    blocks.append(t[: seg - 4] + b"wxyz" + b"wxyz")
    blocks.append(t[:seg] + bytes(seg) + t[seg: 3 * seg])
    blocks.append(t[:seg] + rnd + t[seg: 3 * seg])
    blocks.append(rnd + t[: 3 * seg] + rnd + t[3 * seg: 6 * seg])
    blocks.append(rng.integers(0, 128, 4 * seg + 7, dtype=np.uint8).tobytes())
    sts = verify(engine, blocks)
    # groups do share: the 4-segment text is one dynamic block, 9 segments are 4 + 4 + 1
    assert [b.out_len for b in dynamic_blocks(sts[4])] == [4 * seg]
    assert [b.out_len for b in dynamic_blocks(sts[7])] == [4 * seg, 4 * seg, seg + 100]


@pytest.mark.parametrize("rare_high", [True, False], ids=["rare_9bit", "rare_8bit"])
@pytest.mark.parametrize("n,slack,halvings", [(9, 0.0, 1), (12, 0.04, 2)], ids=["one_rebuild", "more_rebuilds"])
def test_deep_litlen(engine, n, slack, halvings, rare_high):
    """The literal/length code's limit: an unlimited tree deeper than 15 comes
    out exactly 15 deep.  one_rebuild: the counts halved once already fit;
    more_rebuilds: the tree is 18 or more deep and the halved counts' tree is
    still deeper than 15, so K7h halves again."""
    (st,) = verify(engine, [deep_litlen(n, slack, rare_high, 11 * n + rare_high)], dictated=True)
    hit = []
    for b in dynamic_blocks(st):
        f = b.litlen_counts()
        d0, d1 = P.unlimited_depth(halved(f, 0)), P.unlimited_depth(halved(f, 1))  # the trees K7h builds
        print(f"deep_litlen: block of {b.out_len}: {len(f)} symbols, depth {P.unlimited_depth(f)}, of count | 1 {d0}, "
              f"halved once {d1}, "
              f"emitted {max(b.litlen_lens)}")
        if d0 > 15 and P.unlimited_depth(f) > 15:
            assert max(b.litlen_lens) == 15
            hit.append((d0, d1))
    assert hit, "the input no longer makes a literal/length tree deeper than 15: reshape it"
    if halvings == 1:
        assert any(d1 <= 15 for _, d1 in hit), f"no tree fits after one halving {hit}: reshape the input"
    else:
        assert any(d0 >= 18 and d1 > 15 for d0, d1 in hit), f"no tree needs a second halving {hit}: reshape the input"


def test_deep_dist_and_the_widest_token(engine):
    """The distance code's limit (18 symbols in chained counts: 17 deep, 15
    sent), and a token of 13+ code bits + 5 extra bits, then 13+ code bits +
    13 extra bits, with all the extra bits set."""
    (st,) = verify(engine, [deep_dist()], dictated=True)
    deep, widest = False, []
    for b in dynamic_blocks(st):
        f = b.dist_counts()
        d0 = min(P.unlimited_depth(f), P.unlimited_depth(halved(f, 0)))  # the counts' tree and the one K7h builds
        print(f"deep_dist: block of {b.out_len}: distance counts {sorted(f.items())}, depth {d0}, "
              f"emitted {max(b.dist_lens)}; literal/length depth {P.unlimited_depth(b.litlen_counts())}, "
              f"emitted {max(b.litlen_lens)}")
        if d0 > 15:
            assert max(b.dist_lens) == 15 and len(f) >= DEEP_DIST_SYMBOLS
            deep = True
        for t in b.tokens:
            if not isinstance(t, int) and LEN_EXTRA[t.lsym - 257] == 5 and DIST_EXTRA[t.dsym] == 13:
                print(f"  {tuple(t)}: symbol {t.lsym} in {b.litlen_lens[t.lsym]} bits + extra {t.lextra}, "
                      f"distance symbol {t.dsym} in {b.dist_lens[t.dsym]} bits + extra {t.dextra}")
                if b.litlen_lens[t.lsym] >= 13 and b.dist_lens[t.dsym] >= 13:
                    widest.append(t)
    assert deep, "the input no longer makes a distance tree deeper than 15: reshape it"
    assert widest, "no token of 13 + 5 + 13 + 13 bits or more: reshape the input"
    assert any(t.lextra == 31 or (t.lsym, t.lextra) == (284, 30) for t in widest)
    assert any(t.dextra == 8191 for t in widest)


def test_deep_code_length_code(engine):
    (st,) = verify(engine, [deep_cl()], dictated=True)
    (b,) = dynamic_blocks(st)
    f = b.op_counts()
    print(f"deep_cl: operations {sorted(f.items(), key=lambda x: x[1])}, lengths {b.cl_lens}")
    assert not [t for t in b.tokens if not isinstance(t, int)], "a match: the counts are no longer the dictated ones"
    assert len(f) >= 9 and min(P.unlimited_depth(f), P.unlimited_depth(halved(f, 0))) > 7, \
        "the header's operations no longer make a tree deeper than 7 (as counts and as K7h weighs them, count | 1)"
    assert max(b.cl_lens) == 7


def test_no_match(engine):
    """200 equally likely values in one segment: no distance symbol, so K7h
    sends the 1-bit codes of distance symbols 0 and 1 (RFC 1951 §3.2.7)."""
    data = np.random.default_rng(3).integers(0, 200, SEG, dtype=np.uint8).tobytes()
    (st,) = verify(engine, [data])
    (b,) = dynamic_blocks(st)
    assert not b.dist_counts() and b.hdist == 2 and b.dist_lens == [1, 1] and b.hlit == 257


@pytest.mark.parametrize("k", [20, 150], ids=["one_segment", "three_segments"])
def test_one_distance_symbol_0(engine, k):
    """Runs of 259 equal bytes that start on a round's last byte: every match
    lies 1 back; symbol 1 gets the second code.  (A plain run of one byte
    value does not do: the byte before a position is in the same round and
    not seen for certain, and the parse takes what the bucket holds.)"""
    (st,) = verify(engine, [one_distance(1, 258, k, 40 + k)])
    dyn = [b for b in dynamic_blocks(st) if b.dist_counts()]
    assert dyn, "no match: reshape the input"
    for b in dyn:
        assert set(b.dist_counts()) == {0}, f"matches at other distances {b.dist_counts()}: reshape the input"
        assert b.dist_lens == [1, 1] == partner(0)
    assert sum(b.dist_counts()[0] for b in dyn) >= k - 3


@pytest.mark.parametrize("dist", [6, 400, 30000])
def test_one_distance_symbol_far(engine, dist):
    """Every match at one distance, in symbol 4, 17 or 29: that symbol and
    symbol 0 get the two 1-bit codes, HDIST reaches the symbol."""
    sym = {6: 4, 400: 17, 30000: 29}[dist]
    data = one_distance_far(dist, 2 * SEG, dist) if dist > ROUND else one_distance(dist, 100, 40, dist)
    (st,) = verify(engine, [data])
    hit = 0
    for b in dynamic_blocks(st):
        f = b.dist_counts()
        if f:
            assert set(f) == {sym}, f"matches at other distances {f}: reshape the input"
            assert all(t.distance == dist for t in b.tokens if not isinstance(t, int))
            assert b.hdist == sym + 1 and b.dist_lens == [1] + [0] * (sym - 1) + [1] == partner(sym)
            hit += f[sym]
    assert hit >= 30, "too few matches: reshape the input"


def test_rle_edges(engine):
    """The header's run-length coder at its edges: every feature of FEATURES
    is shown by the header of the case named there."""
    cases = rle_cases()
    names = sorted(cases)
    sts = verify(engine, [cases[k] for k in names], names, dictated=set(RLE_TAILS) | {"length_15"})
    shown = {}
    for name, st in zip(names, sts):
        shown[name] = set()
        for b in dynamic_blocks(st):
            shown[name] |= header_features(b)
        print(f"rle_edges: {name}: {sorted(shown[name])}")
    missing = {f: c for f, c in FEATURES.items() if f not in shown[c]}
    assert not missing, f"not shown by their cases (reshape the inputs): {missing}"
    assert len(FEATURES) == 24


def test_len_dist_extremes(engine):
    """Every length symbol 258..285 and every distance symbol 0..29, each
    with extra value 0 and with its largest."""
    (st,) = verify(engine, [len_dist_extremes()])
    seen_l, seen_d = set(), set()
    for b in st.blocks:
        for t in b.tokens:
            if not isinstance(t, (int, bytes)):
                seen_l.add((t.lsym, t.lextra))
                seen_d.add((t.dsym, t.dextra))
    want_l = {(s, x) for s in range(258, 286) for x in (0, (1 << LEN_EXTRA[s - 257]) - 1)} - {(284, 31)} | {(284, 30)}
    want_d = {(s, x) for s in range(30) for x in (0, (1 << DIST_EXTRA[s]) - 1)}
    assert not want_l - seen_l, f"lengths not reached (reshape the input): {sorted(want_l - seen_l)}"
    assert not want_d - seen_d, f"distances not reached (reshape the input): {sorted(want_d - seen_d)}"


def test_member_overflows_image(engine):
    """text, text, text, X in one group, X random bytes with one planted
    256-byte repeat (so K7e lets it through to the parse).  The group must
    not share, by the fallback at `il + 8 > 4 * kImgWords` and not because
    sharing would not pay: the members come out coded alone, and the code
    K7h's rule makes of the four members' pooled counts (the decoded tokens
    are the parse's, whichever code they were sent in) puts X's bits past
    its image, while the shared piece would have been smaller than the
    members' fixed-or-stored sizes."""
    rng = np.random.default_rng(23)
    x = bytearray(rng.integers(0, 256, SEG, dtype=np.uint8).tobytes())
    x[20000:20256] = x[1000:1256]
    t = _text(3 * SEG, 4)
    (st,) = verify(engine, [t + bytes(x)])
    pieces = [b for b in st.blocks[:-1] if b.out_len]
    assert [(b.btype, b.out_len) for b in pieces[:3]] == [(2, SEG)] * 3
    assert len(pieces) == 4 and pieces[3].out_len == SEG  # (stored, or a code of its own that gains from the repeat)
    # the shared code K7h built first
    members = [list(b.tokens[0]) if b.btype == 0 else b.tokens for b in pieces]  # (X stored: its bytes as literals)
    lf, df = {256: 1}, {}
    for toks in members:
        for tk in toks:
            s = tk if isinstance(tk, int) else tk.lsym
            lf[s] = lf.get(s, 0) + 1
            if not isinstance(tk, int):
                df[tk.dsym] = df.get(tk.dsym, 0) + 1
    ll = k7h_lengths(lf)
    dl = k7h_lengths(df) if len(df) >= 2 else dict(enumerate(partner(min(df) if df else 0)))
    bits = [sum(ll[tk] if isinstance(tk, int) else ll[tk.lsym] + LEN_EXTRA[tk.lsym - 257] + dl[tk.dsym]
                + DIST_EXTRA[tk.dsym] for tk in toks) for toks in members]
    print(f"member_overflows_image: bits per member under the shared code {bits}, X {bits[3] / SEG:.2f} per byte")
    # X's image (it starts at bit S mod 8 >= 0): il = ((S mod 8 + bits + end of block + 3 + 7) >> 3) + 4
    il = ((bits[3] + ll[256] + 3 + 7) >> 3) + 4
    assert il + 8 > IMG_BYTES, f"X fits its image under the shared code ({il} bytes): reshape the input"
    # and sharing would have paid: the piece, with a header at its largest (every operation 7 + 7 bits), against
    # the members alone
    header = 17 + 3 * 19 + 14 * len(header_ops([ll.get(s, 0) for s in range(max(257, max(ll) + 1))]
                                               + [dl.get(s, 0) for s in range(max(dl) + 1)]))
    total = (header + sum(bits) + ll[256] + 3 + 7) // 8 + 5
    alone = sum(min(5 + SEG, ((3 + fixed_code_bits(toks) + 7 + 3 + 7) >> 3) + 4) for toks in members)
    assert total < alone, f"the shared piece would not have been smaller ({total} against {alone}): reshape the input"
    # and without X the three do share
    (st,) = verify(engine, [t])
    assert [(b.btype, b.out_len) for b in st.blocks[:-1] if b.out_len] == [(2, 3 * SEG)]


def test_output_canary(engine):
    """test_device_odd_offsets with the output filled with 0xA5 (a stray zero
    byte shows) and odd capacities, twice on one engine with different blocks,
    so that the scratch slots hold the first call's images the second time."""
    import torch
    rng = np.random.default_rng(9)
    first = [_text(50_000, 1), rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes(), bytes(33_333), b"x",
             _text(4 * SEG + 5, 2)]
    second = [bytes(40_001), _text(70_001, 3), b"", rng.integers(0, 200, 33_333, dtype=np.uint8).tobytes(),
              _text(3 * SEG - 1, 4)[::-1]]
    for datas in (first, second):
        offs, pos = [], 3
        for d in datas:
            offs.append(pos)
            pos += len(d) + 7
        host = np.zeros(pos + 64, np.uint8)
        for o, d in zip(offs, datas):
            host[o:o + len(d)] = np.frombuffer(d, np.uint8)
        src = torch.from_numpy(host).to("cuda:0")
        caps = [(engine.deflate_bound(len(d)) + 2 * i) | 1 for i, d in enumerate(datas)]
        out_offs, q = [], 1
        for c in caps:
            out_offs.append(q)
            q += c + 5 + (c & 1)
        dst = torch.full((q + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        lens = engine.deflate_blocks_device(src.data_ptr(), offs, [len(d) for d in datas], dst.data_ptr(), out_offs,
                                            caps)
        out = dst.cpu().numpy()
        mask = np.ones(out.size, bool)
        for d, o, k in zip(datas, out_offs, lens):
            z = out[o:o + int(k)].tobytes()
            # what _check asserts (it goes through deflate_blocks itself), on this slice
            assert z[:2] == b"\x78\x9c" and len(z) <= engine.deflate_bound(len(d))
            assert OD.inflate_strict(z) == d
            check_stream(d, z)
            mask[o:o + int(k)] = False
        assert (out[mask] == 0xA5).all(), np.flatnonzero(mask & (out != 0xA5))[:10]
