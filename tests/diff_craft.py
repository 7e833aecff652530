"""Designed inputs for the byte comparison behind ``diff`` (hbx_k10_diff in
hashbox_amd/csrc/hbx_restore.hip, hbx_k11_diff in hbx_restore_many.hip, and
the host code that cuts their pieces and merges their words: restore_window,
many_pass, hbx_restore_blocks, hbx_restore_file_stream, hbx_restore_files_*
in hbx_engine.hip), their reference and a model of the path a byte takes.

Both kernels are a cascade of "smallest of several candidates": the first
differing byte of a 16-byte granule (``first_diff16``), a lane's first hit
over its iterations, the wave's minimum by six ``__shfl_xor`` steps, K10's
four ``wmin`` slots, ``atomicMin`` on one word per call (K10) or per file of
a pass (K11), and the host's merge over passes and windows beside the prefix
rule and the length rule.  One flipped bit gives every level one candidate.
Here every level gets competing candidates, and every local alignment of
``local + dst`` and every block length 1..48 is met.

* **Reference** (:func:`reference`): ``np.flatnonzero(a[:m] != b[:m])`` over
  the good prefix, else ``min(len_local, len_restored)`` when the lengths
  differ, else none.  It knows nothing of pieces.
* **Model** (:func:`k11_layout`, :func:`k10_layout`, :func:`locate`): the
  host's piece cutting, where a block's source and its local bytes lie, and
  for a byte of a piece its region (head, vector, tail), granule, word, byte,
  lane, iteration and wave.  MIRRORED quotes the source lines it restates;
  tests/test_diff_craft.py fails if one no longer occurs in the source and
  asserts each family's coverage on the model.

The bases the model takes as 16-byte aligned: every DevBuf comes from
``hipMalloc`` (hbx_engine.hip, ``DevBuf::ensure``), K10's local image is
``d_rimg`` at offset 0 (``*d = c->d_rimg.as<uint8_t>();`` in
hbx_restore_blocks and hbx_restore_file_stream), K11's is ``d_rimg`` at
offset 0 too (the hbx_k11_diff launch in many_pass), the staged input starts
at ``d_rin[k]`` and the inflate slots at multiples of 256 from ``d_rslots``.
None of them carries an offset.

Nothing here needs a GPU.
"""
from __future__ import annotations

import functools
import hashlib
import struct
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

RAW, ZLIB = 0xFF, 0x01
PIECE = 65536        # hbxr::kPiece: K10, one piece per 256-thread workgroup
PIECE_MANY = 16384   # hbxm::kPieceMany: K11, one piece per wave
T10, T11 = 256, 64   # lanes that share a piece's granules
WAVES = 4            # K11: pieces per workgroup; K10: wmin slots
MAX_BLOCK = 65536    # max_block of the K11 call (size hints keep the slots small)
XORS = (0x01, 0x80, 0xFF)
G_ALIGNS = (0, 5, 11)
HT_LENS = tuple(range(1, 49))
HT_WAYS = ("same", "first", "last", "both")
K10_HT_LENS = (1, 15, 16, 17, 33, 48)
K10_HT_ZLENS = (1, 17)
# what the corpus holds, as DESIGN.md §2 states it (tests/test_diff_craft.py asserts each on the model)
STATED = {"G": 1206, "L": 36, "W": 456, "HT": 3092, "S": 11, "F": 65, "k11_cases": 4866,
          "k10": {"L": 18, "W": 122, "WG": 16, "S": 11, "HT": 512, "G": 121}}

MIRRORED = {
    "hbx_restore.hip": [
        "constexpr uint32_t kPiece = 65536;",
        "constexpr uint32_t kThreads = 256;",
        "const uint8_t* loc = local + p.dst;",                                     # K10: dst is the file offset
        "const uint32_t head = min(len, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(loc) & 15u)) & 15u);",
        "const uint32_t nvec = (len - head) >> 4;",
        "const uint32_t tail0 = head + (nvec << 4);",
        "if (t < head && src[t] != loc[t]) best = t;",                             # head: byte t is lane t's
        "for (uint32_t v = t; v < nvec; v += kThreads) {",                         # K10: granule v, lane v % 256
        "const uint32_t at = head + 16u * v;",
        "if (x0) return (uint32_t)__builtin_ctz(x0) >> 3;",                        # word, then byte in the word
        "return 12u + ((uint32_t)__builtin_ctz(x3) >> 3);",
        "if (t < len - tail0 && src[tail0 + t] != loc[tail0 + t]) best = min(best, tail0 + t);",
        "for (int m = 32; m >= 1; m >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, m, 64));",
        "if ((t & 63u) == 0u) wmin[t >> 6] = best == 0xFFFFFFFFu ? kNoDiff : p.dst + best;",  # wave = lane / 64
        "for (uint32_t w = 1; w < kThreads / 64; w++) m = wmin[w] < m ? wmin[w] : m;",
    ],
    "hbx_restore_many.hip": [
        "#define HBX_PIECE_MANY 16384",
        "const uint32_t i = blockIdx.x * kWaves + (threadIdx.x >> 6);",            # piece i: workgroup i / 4, wave i % 4
        "for (uint32_t v = t; v < nvec; v += 64u) {",                              # K11: granule v, lane v % 64
        "if (t == 0 && best != 0xFFFFFFFFu) atomicMin(&first[p.file], (unsigned long long)(p.foff + best));",
    ],
    "hbx_engine.hip": [
        "hipError_t e = hipMalloc(&p, want);",                                     # every base is aligned
        "*d = c->d_rimg.as<uint8_t>();",                                           # K10's local image: offset 0
        "(uint32_t)pieces.size(), c->d_rimg.as<uint8_t>(), c->d_rword.as<unsigned long long>());",  # K11's
        "inline uint64_t restore_stride(uint64_t mb) { return (mb + 256ull + 255ull) & ~255ull; }",
        "out_offs.push_back((zi.size() - 1) * stride);",                           # K10's inflate slots
        "return ((std::min<uint64_t>(cap, 1ull << 62) + 255ull) & ~255ull) + 256ull;",  # many_slot
        "slots += many_slot(S.caps[i]);",                                          # K11's inflate slots
        "if (types[i] == HBX_BLOCK_ZLIB) pos = (pos + 15) & ~15ull;",              # hbx_restore_blocks: raw is packed
        "if (pre[i] == 0 && types[i] == HBX_BLOCK_ZLIB) pos = (pos + 15) & ~15ull;",  # hbx_restore_files_blocks
        "const uint64_t cover = diff ? avail : (image ? total : 0);",
        "const uint64_t len = std::min(dlen[i], cover - w.offs[i]);",
        "pieces.push_back(hbxr::Piece{addr[i] + p, w.offs[i] + p, (uint32_t)std::min<uint64_t>(hbxr::kPiece, len - p), 0u});",
        "if (word < w.offs[w.n_good]) w.first_diff = word;",                       # K10's prefix rule
        "if (w.first_diff != hbxr::kNoDiff && found == hbxr::kNoDiff) found = base + w.first_diff;",
        "sg.have = (sg.was_bad || llen <= sg.foff0) ? 0 : std::min(sg.bytes, llen - sg.foff0);",
        "sg.loff = pos;",
        "const uint64_t cover = R.diff ? std::min(g.have, g.bytes) : g.bytes;",
        "const uint64_t at = bfoff[i - s] - g.foff0;",
        "if (at >= cover) break;",
        "const uint64_t dst = R.diff ? g.loff + at : bimg[i - s];",
        "(uint32_t)std::min<uint64_t>(hbxm::kPieceMany, len - p), (uint32_t)k});",
        "if (R.diff && words[k] < g.foff0 + g.good) R.found[f] = std::min(R.found[f], words[k]);",
        "if (e > start && (s > wb || sum > wb - s)) break;",                       # many_window_end
        "const uint64_t per = std::min<uint64_t>(std::max<uint64_t>(1, window_bytes / stride), std::max<uint64_t>(n_blocks, 1));",
    ],
}


# ------------------------------------------------------------- reference --
def reference(restored: bytes, local: bytes) -> Optional[int]:
    """diffFileData's answer for a file whose good prefix is `restored`."""
    a, b = np.frombuffer(restored, np.uint8), np.frombuffer(local, np.uint8)
    m = min(a.size, b.size)
    d = np.flatnonzero(a[:m] != b[:m])
    if d.size:
        return int(d[0])
    return m if a.size != b.size else None


def block_id(data: bytes, links=()) -> bytes:
    """HashboxBlock.HashData (pkg/core/block.go:96-111)."""
    return hashlib.md5(struct.pack(">I", len(links)) + b"".join(links) + struct.pack(">I", len(data)) + data).digest()


# ----------------------------------------------------------------- model --
@dataclass
class Blk:
    """One block as the model needs it."""
    type: int
    field_len: int       # the data field on the wire
    plain_len: int       # what it inflates to
    inflates: bool = True
    id_ok: bool = True


@dataclass
class Piece:
    index: int           # in the launch: K10 workgroup `index`; K11 workgroup index / 4, wave index % 4
    file: int
    block: int           # in its file
    foff: int            # file offset of its first byte
    len: int
    src16: int           # source address mod 16
    loc16: int           # local address mod 16

    @property
    def head(self) -> int:   # `head = min(len, (16 - (loc & 15)) & 15)`
        return min(self.len, (16 - self.loc16) & 15)

    @property
    def nvec(self) -> int:   # `nvec = (len - head) >> 4`
        return (self.len - self.head) >> 4

    @property
    def tail0(self) -> int:  # `tail0 = head + (nvec << 4)`
        return self.head + (self.nvec << 4)


def cut(at: int, length: int, piece: int):
    """`for (p = 0; p < len; p += kPiece) ... min(kPiece, len - p)`"""
    return [(at + p, min(piece, length - p)) for p in range(0, length, piece)]


def stage(blks: Sequence[Blk], pos: int = 0):
    """hbx_restore_blocks / hbx_restore_files_blocks: zlib streams at 16-byte
    boundaries, raw blocks packed byte by byte behind what precedes them.
    Returns (positions, end)."""
    at = []
    for b in blks:
        if b.type == ZLIB:
            pos = (pos + 15) & ~15
        at.append(pos)
        pos += b.field_len
    return at, pos


@dataclass
class Seg:
    file: int
    index: int      # the segment's index in the pass: the word it owns
    loff: int       # where its local bytes start in the packed local image
    have: int       # local bytes compared
    bytes: int      # the blocks before the first that does not inflate
    good: int       # the bytes of its leading verified blocks
    n_good: int
    status: List[bool] = field(default_factory=list)  # per block: status == 0


@dataclass
class Layout:
    pieces: List[Piece]
    segs: Dict[int, Seg]       # by file (files without blocks have none)
    src_at: List[List[int]]    # per file, per block: staged position of a raw block (zlib: of its stream)
    by_file: Dict[int, List[Piece]]


def k11_layout(files: Sequence[Sequence[Blk]], local_lens: Sequence[int]) -> Layout:
    """One window, one pass of hbx_restore_files_blocks in diff mode (what the
    GPU test asserts through `knobs()["restore_many"]`)."""
    pieces, segs, src_at, by_file = [], {}, [], {}
    pos = loff = 0
    for f, blks in enumerate(files):
        at, pos = stage(blks, pos)
        src_at.append(at)
        if not blks:
            continue
        live = 0
        while live < len(blks) and blks[live].inflates:
            live += 1
        ok = 0
        while ok < len(blks) and blks[ok].inflates and blks[ok].id_ok:
            ok += 1
        nbytes = sum(b.plain_len for b in blks[:live])
        have = min(nbytes, local_lens[f])  # foff0 = 0: one pass
        sg = Seg(f, len(segs), loff, have, nbytes, sum(b.plain_len for b in blks[:ok]), ok,
                 [b.inflates and b.id_ok for b in blks])
        segs[f] = sg
        off = 0
        for k, b in enumerate(blks[:live]):
            if off >= have:  # `if (at >= cover) break;`
                break
            n = min(b.plain_len, have - off)
            src = at[k] if b.type == RAW else 0  # an inflate slot is aligned
            for o, ln in cut(off, n, PIECE_MANY):
                p = Piece(len(pieces), f, k, o, ln, (src + o - off) & 15, (loff + o) & 15)
                pieces.append(p)
                by_file.setdefault(f, []).append(p)
            off += b.plain_len
        loff += have
    return Layout(pieces, segs, src_at, by_file)


def k10_layout(blks: Sequence[Blk], local_len: int) -> Layout:
    """hbx_restore_blocks in diff mode, one window (every chain here is far
    below the slot budget): local + dst is the file offset in the image."""
    at, _ = stage(blks)
    live = 0
    while live < len(blks) and blks[live].inflates:
        live += 1
    ok = 0
    while ok < len(blks) and blks[ok].inflates and blks[ok].id_ok:
        ok += 1
    total = sum(b.plain_len for b in blks[:live])
    cover = min(total, local_len)
    pieces, off = [], 0
    for k, b in enumerate(blks[:live]):
        if off >= cover:
            break
        n = min(b.plain_len, cover - off)
        src = at[k] if b.type == RAW else 0
        for o, ln in cut(off, n, PIECE):
            pieces.append(Piece(len(pieces), 0, k, o, ln, (src + o - off) & 15, o & 15))
        off += b.plain_len
    sg = Seg(0, 0, 0, cover, total, sum(b.plain_len for b in blks[:ok]), ok, [b.inflates and b.id_ok for b in blks])
    return Layout(pieces, {0: sg}, [at], {0: pieces})


def locate(pieces: Sequence[Piece], x: int, threads: int) -> Optional[dict]:
    """The path of the file's byte x: its piece, region, granule, word, byte
    in the word, lane, iteration and wave.  None: no piece covers it (it lies
    behind `cover`)."""
    for p in pieces:
        if p.foff <= x < p.foff + p.len:
            o = x - p.foff
            out = {"piece": p.index, "block": p.block, "at": o, "loc16": p.loc16, "src16": p.src16}
            if o < p.head:       # `if (t < head && ...) best = t`
                out.update(region="head", lane=o, iter=None, granule=None)
            elif o < p.tail0:    # `for (v = t; v < nvec; v += T)`, `at = head + 16 v`
                v, r = divmod(o - p.head, 16)
                out.update(region="vector", granule=v, lane=v % threads, iter=v // threads, word=r // 4, byte=r % 4)
            else:                # `if (t < len - tail0 && ...)`
                out.update(region="tail", lane=o - p.tail0, iter=None, granule=None)
            if threads == T10:
                out.update(workgroup=p.index, wave=out["lane"] // 64)
            else:
                out.update(workgroup=p.index // WAVES, wave=p.index % WAVES)
            return out
    return None


def window_end(caps: Sequence[int], wb: int, start: int) -> int:
    """many_window_end: the blocks from `start` whose shares fit wb, at least one."""
    total, e = 0, start
    while e < len(caps):
        s = ((caps[e] + 255) & ~255) + 256  # many_slot
        if e > start and (s > wb or total > wb - s):
            break
        total += s
        e += 1
    return e


def restore_stride(mb: int) -> int:
    return (mb + 256 + 255) & ~255


def verdict(pieces: Sequence[Piece], threads: int, restored: bytes, local: bytes, want: Optional[int],
            got: Optional[int]) -> str:
    """What a wrong answer looks like to the model: where the expected byte
    lies, and which candidate the kernel seems to have taken."""
    def path(x):
        w = locate(pieces, x, threads)
        if w is None:
            return "offset %d: in no piece (behind what is compared)" % x
        s = "offset %d: piece %d (workgroup %d, wave %d; local %% 16 = %d, source %% 16 = %d) %s" % (
            x, w["piece"], w["workgroup"], w["wave"], w["loc16"], w["src16"], w["region"])
        if w["region"] == "vector":
            s += " granule %d word %d byte %d, lane %d iteration %d" % (w["granule"], w["word"], w["byte"], w["lane"],
                                                                         w["iter"])
        else:
            s += " lane %d" % w["lane"]
        return s
    a, b = np.frombuffer(restored, np.uint8), np.frombuffer(local, np.uint8)
    m = min(a.size, b.size)
    cand = np.flatnonzero(a[:m] != b[:m]).tolist()
    out = []
    if want is not None and want < m and cand and want == cand[0]:
        out.append("expected " + path(want))
    elif want is not None:
        out.append("expected %d by the length rule (%d restored, %d local)" % (want, a.size, b.size))
    else:
        out.append("expected no difference")
    if got is None:
        out.append("got none: every candidate was lost (%d differing bytes)" % len(cand))
    elif got in cand:
        out.append("got candidate %d of %d, %s" % (cand.index(got), len(cand), path(got)))
    elif got == m and a.size != b.size:
        out.append("got the length rule's %d: every candidate before it was lost" % got)
    else:
        out.append("got %d, which is no differing byte%s" % (got, "; " + path(got) if got < m else " (outside)"))
    return "; ".join(out)


# ------------------------------------------------------------------ bytes --
@functools.lru_cache(maxsize=None)
def _pool() -> np.ndarray:
    """2 MiB of letters a..p: zlib codes them, and no XOR of XORS keeps one."""
    return np.random.Generator(np.random.PCG64(1249)).integers(97, 113, 2 << 20, dtype=np.uint8)


_seq = [0]


def fresh(n: int) -> np.ndarray:
    """The next n bytes of the pool (wrapping), never the same run twice in a row."""
    p = _pool()
    o = (_seq[0] * 7919) % (p.size - max(n, 1))
    _seq[0] += 1
    return p[o:o + n].copy()


@dataclass
class Case:
    name: str
    family: str
    blocks: List[bytes]              # the file's blocks, plain
    local: bytes
    want: Optional[int]
    tag: tuple = ()                  # what the case covers, for the CPU assertions
    bad: Optional[Tuple[int, str]] = None  # (block, "truncated" | "wrong_id")
    align: Optional[int] = None      # K11: local address mod 16 of the file's first byte
    rel: int = 0                     # K11, raw blocks: (source - local) mod 16
    guard: bool = False              # the bytes just outside it differ between the packed neighbours

    @property
    def data(self) -> bytes:
        return b"".join(self.blocks)

    def restored(self) -> bytes:
        """The good prefix: the blocks before the bad one."""
        return self.data if self.bad is None else b"".join(self.blocks[:self.bad[0]])


def wire(case: Case, mode: str):
    """[(type, data field, id)] of a case's blocks: mode 'r' raw, 'z' zlib -6;
    a "truncated" block is half a zlib stream in both modes."""
    out = []
    for k, b in enumerate(case.blocks):
        t, fld, bid = (RAW, b, block_id(b)) if mode == "r" else (ZLIB, zlib.compress(b, 6), block_id(b))
        if case.bad is not None and case.bad[0] == k:
            if case.bad[1] == "truncated":
                z = zlib.compress(b, 6)
                t, fld = ZLIB, z[:max(2, len(z) // 2)]
            else:
                bid = block_id(b + b"x")
        out.append((t, fld, bid))
    return out


def blks_of(case: Case, chain) -> List[Blk]:
    return [Blk(t, len(fld), len(b), not (case.bad is not None and case.bad == (k, "truncated")),
                not (case.bad is not None and case.bad == (k, "wrong_id")))
            for k, ((t, fld, _), b) in enumerate(zip(chain, case.blocks))]


def flipped(x: np.ndarray, at: Sequence[int], xor: int = 0xFF) -> bytes:
    y = x.copy()
    for a in at:
        y[a] ^= xor
    return y.tobytes()


def _one(name, family, x: np.ndarray, at: Sequence[int], xor=0xFF, **kw) -> Case:
    """A one-block file whose local copy differs at `at`."""
    at = sorted(set(at))  # (first and last are one byte in a file of one)
    return Case(name, family, [x.tobytes()], flipped(x, at, xor), min(at) if len(at) else None, **kw)


# --------------------------------------------------------- K11's families --
def family_g() -> List[Case]:
    """Every pair of differing bytes of one granule, each XOR value, three
    local alignments; the same pairs in the last whole granule before a tail;
    granules that differ in all 16 bytes."""
    out = []
    pairs = [(i, j) for i in range(16) for j in range(i + 1, 16)]
    for a in G_ALIGNS:
        h = (16 - a) & 15
        for i, j in pairs:
            for x in XORS:
                f = fresh(h + 48 + 5)
                out.append(_one("G_a%d_%d_%d_%02x" % (a, i, j, x), "G", f, [h + 16 + i, h + 16 + j], x,
                                tag=("pair", a, i, j, x), align=a, rel=(i + j) & 15))
    for k, (i, j) in enumerate(pairs):
        a, x = G_ALIGNS[k % 3], XORS[(k // 3) % 3]
        h = (16 - a) & 15
        f = fresh(h + 48 + 5)
        out.append(_one("G_last_a%d_%d_%d_%02x" % (a, i, j, x), "G", f, [h + 32 + i, h + 32 + j], x,
                        tag=("pair_last", a, i, j, x), align=a, rel=k & 15))
    for a in G_ALIGNS:
        h = (16 - a) & 15
        for g in (1, 2):
            f = fresh(h + 48 + 5)
            out.append(_one("G_all16_a%d_g%d" % (a, g), "G", f, range(h + 16 * g, h + 16 * g + 16),
                            tag=("all16", a, g), align=a, rel=a))
    return out


def _granule_case(name, family, threads, piece, a, hits, tag, **kw) -> Case:
    """A one-piece file at local alignment a with one differing byte in each
    granule of `hits` [(lane, iteration)]; `n` whole granules plus a tail."""
    h = (16 - a) & 15
    gran = [it * threads + lane for lane, it in hits]
    n = kw.pop("n")
    f = fresh(n)
    assert h + 16 * (max(gran) + 1) <= n <= piece
    at = [h + 16 * g + (5 * g + 3) % 16 for g in gran]
    return _one(name, family, f, at, tag=tag, align=a, **kw)


def family_l(threads=T11, piece=PIECE_MANY, aligns=(0, 7), lanes=(0, 17, 62)) -> List[Case]:
    """Granules v and v + T of one lane, and v + T only, at iterations 0, 1
    and 15 (the pairs 0/1, 1/2, 14/15)."""
    out = []
    for a in aligns:
        for lane in lanes:
            for it in (0, 1, 14):
                for kind, hits in (("both", [(lane, it), (lane, it + 1)]), ("later", [(lane, it + 1)])):
                    out.append(_granule_case("L_a%d_l%d_i%d_%s" % (a, lane, it, kind), "L", threads, piece, a, hits,
                                             ("lane", a, lane, it, kind), n=piece, rel=(lane + it) & 15))
    return out


def family_w(threads=T11, piece=PIECE_MANY, pair_lanes=None, lane_of=lambda k: k, ab_base=0, aligns=True) -> List[Case]:
    """Each lane 0..63 the only holder; for each shuffle distance m the lanes
    (l, l ^ m) with the smaller offset once in each; lane a in iteration 1
    against lane b > a in iteration 0, and the reverse."""
    out = []
    n1, n2 = 16 * threads + 16 + 3, 32 * threads + 16 + 3
    for k in range(64):
        lane, a = lane_of(k), (5 * k) & 15 if aligns else 0
        out.append(_granule_case("W_only_l%d" % lane, "W", threads, piece, a, [(lane, 0)], ("only", lane), n=n1,
                                 rel=(3 * k) & 15))
    for m in (1, 2, 4, 8, 16, 32):
        for l0 in (pair_lanes if pair_lanes is not None else range(64)):
            if l0 & m:
                continue
            lo, hi = lane_of(l0), lane_of(l0) ^ m
            a = (l0 + m) & 15 if aligns else 0
            out.append(_granule_case("W_m%d_l%d_lo" % (m, lo), "W", threads, piece, a, [(lo, 0), (hi, 1)],
                                     ("xor", m, lo, hi, lo), n=n2, rel=l0 & 15))
            out.append(_granule_case("W_m%d_l%d_hi" % (m, lo), "W", threads, piece, a, [(lo, 1), (hi, 0)],
                                     ("xor", m, lo, hi, hi), n=n2, rel=(l0 + 9) & 15))
    for lo, hi in ((3, 40), (0, 63), (31, 32), (62, 63)):
        lo, hi = ab_base + lo, ab_base + hi
        a = 9 if aligns else 0
        out.append(_granule_case("W_ab_%d_%d_b" % (lo, hi), "W", threads, piece, a, [(lo, 1), (hi, 0)],
                                 ("ab", lo, hi, hi), n=n2, rel=lo & 15))
        out.append(_granule_case("W_ab_%d_%d_a" % (lo, hi), "W", threads, piece, a, [(lo, 0), (hi, 1)],
                                 ("ab", lo, hi, lo), n=n2, rel=hi & 15))
    return out


def family_ht() -> List[Case]:
    """Blocks of 1..48 bytes at each local alignment, four ways each, every
    one between neighbours that differ just outside it; head against vector
    and vector against tail in pieces of kPieceMany - 1, kPieceMany and
    kPieceMany + 1 bytes."""
    out = []
    for n in HT_LENS:
        for a in range(16):
            for w, way in enumerate(HT_WAYS):
                at = {"same": [], "first": [0], "last": [n - 1], "both": [0, n - 1]}[way]
                out.append(_one("HT_n%d_a%d_%s" % (n, a, way), "HT", fresh(n), at, tag=("ht", n, a, way), align=a,
                                rel=(n + 3 * a + 5 * w) & 15, guard=True))
    for n in (PIECE_MANY - 1, PIECE_MANY, PIECE_MANY + 1):
        for a in (3, 0):
            p = Piece(0, 0, 0, 0, min(n, PIECE_MANY), 0, a)
            h, t0 = p.head, p.tail0
            ats = []
            if h:
                ats += [("head_vs_vector", [h - 1, h]), ("vector_first", [h])]
            if t0 < p.len:
                ats += [("vector_vs_tail", [t0 - 1, t0]), ("tail_first", [t0])]
            else:
                ats += [("vector_last", [t0 - 1])]
            if n > PIECE_MANY:
                ats += [("piece_vs_next", [PIECE_MANY - 1, PIECE_MANY]), ("next_piece", [PIECE_MANY])]
            for what, at in ats:
                out.append(_one("HT_p%d_a%d_%s" % (n, a, what), "HT", fresh(n), at, tag=("edge", n, a, what), align=a,
                                rel=7, guard=True))
    return out


def suffix_points(pieces: Sequence[Piece], ends: Sequence[int], total: int) -> Dict[str, int]:
    """The x classes of family S, read off the model: `ends` are the blocks'
    ends.  The piece taken for head, vector and tail is the first that has
    both a head and a tail."""
    p = next(q for q in pieces if q.head and q.tail0 < q.len and q.nvec)
    nxt = pieces[pieces.index(p) + 1]
    assert nxt.foff == p.foff + p.len and nxt.block == p.block
    return {"zero": 0, "in_head": p.foff + p.head // 2, "vector_first": p.foff + p.head,
            "vector_last": p.foff + p.tail0 - 1, "in_tail": p.foff + p.tail0 + (p.len - p.tail0) // 2,
            "piece_last": p.foff + p.len - 1, "next_piece_first": p.foff + p.len, "block_last": ends[0] - 1,
            "next_block_first": ends[0], "file_last": total - 1, "second_block_last": ends[1] - 1}


def family_s(piece=PIECE_MANY, align=5) -> List[Case]:
    """The local copy differs in EVERY byte from x on, in a file of three
    blocks of three pieces each: every later granule, lane, wave, piece and
    block competes for the word."""
    n = 2 * piece + 5000
    blocks = [fresh(n) for _ in range(3)]
    whole = np.concatenate(blocks)
    # (the pieces of a file at local alignment `align`; K10: block 0 at 0, so `align` is 0 there)
    lay = k10_layout([Blk(RAW, n, n)] * 3, 3 * n) if piece == PIECE else None
    if lay is None:
        pieces, off = [], 0
        for k in range(3):
            for o, ln in cut(off, n, piece):
                pieces.append(Piece(len(pieces), 0, k, o, ln, 0, (align + o) & 15))
            off += n
    else:
        pieces = lay.pieces
    out = []
    for what, x in suffix_points(pieces, [n, 2 * n], 3 * n).items():
        loc = whole.copy()
        loc[x:] ^= 0xFF
        out.append(Case("S_%s" % what, "S", [b.tobytes() for b in blocks], loc.tobytes(), x, tag=("suffix", what, x),
                        align=align if piece == PIECE_MANY else None, rel=11))
    return out


def family_f() -> List[Case]:
    """Small files that share workgroups, differing and identical in turn,
    files of no blocks between them; local copies shorter and longer than the
    file; files with a bad block."""
    out = []
    k = 0
    for rnd in range(2):
        for j in range(16):
            n = 200 + 37 * j
            f = fresh(n)
            at = [] if j % 2 else [n // 2 + j]
            out.append(_one("F_wg%d_%02d_%s" % (rnd, j, "same" if j % 2 else "diff"), "F", f, at,
                            tag=("wg", rnd, j, bool(at))))
            if j % 3 == 2:
                k += 1
                loc = b"" if k % 2 else b"abc"
                out.append(Case("F_empty_%d" % k, "F", [], loc, 0 if loc else None, tag=("empty", len(loc))))
        if rnd == 0:  # one more one-piece file: the second round's files sit one wave further
            out.append(_one("F_wg_shift", "F", fresh(300), [], tag=("shift",)))
    two = [fresh(20000), fresh(20000)]
    whole = np.concatenate(two)
    blocks = [b.tobytes() for b in two]
    n = whole.size
    for c in (0, 1, PIECE_MANY + 1000, 20000 + 5, n - 1):
        out.append(Case("F_short_%d" % c, "F", blocks, whole[:c].tobytes(), c, tag=("short", c, "none")))
        if c:
            out.append(Case("F_short_%d_flip" % c, "F", blocks, flipped(whole[:c], [c - 1]), c - 1,
                            tag=("short", c, "before")))
    more = fresh(40)
    longer = np.concatenate([whole, more])
    out.append(Case("F_long", "F", blocks, longer.tobytes(), n, tag=("long", "none")))
    out.append(Case("F_long_flip_last", "F", blocks, flipped(longer, [n - 1]), n - 1, tag=("long", "before")))
    out.append(Case("F_long_flip_behind", "F", blocks, flipped(longer, [n, n + 7]), n, tag=("long", "behind")))
    # a file whose block 2 is bad: the prefix is blocks 0 and 1
    four = [fresh(m) for m in (PIECE_MANY + 77, 3000, 5000, 900)]
    w4 = np.concatenate(four)
    b4 = [b.tobytes() for b in four]
    pre = four[0].size + four[1].size
    for kind in ("truncated", "wrong_id"):
        for what, at, want in (("before", [pre - 1], pre - 1), ("behind", [pre, pre + 10, pre + 5100], pre),
                               ("both", [PIECE_MANY + 80, pre + 3], PIECE_MANY + 80), ("none", [], pre)):
            out.append(Case("F_bad_%s_%s" % (kind, what), "F", b4, flipped(w4, at), want, tag=("bad", kind, what),
                            bad=(2, kind)))
        out.append(Case("F_bad_%s_prefix_only" % kind, "F", b4, w4[:pre].tobytes(), None, tag=("bad", kind, "exact"),
                        bad=(2, kind)))
    return out


# ------------------------------------------------------------ K11's corpus --
@dataclass
class Corpus:
    cases: List[Case]        # in file order, fillers included (family "filler")

    def chains(self, mode: str):
        return [wire(c, mode) for c in self.cases]

    def locals(self):
        return [c.local for c in self.cases]

    def layout(self, mode: str, chains=None) -> Layout:
        chains = chains if chains is not None else self.chains(mode)
        return k11_layout([blks_of(c, ch) for c, ch in zip(self.cases, chains)], [len(c.local) for c in self.cases])


def _filler(k: int, fa: int, fb: int) -> Case:
    """A raw-mode spacer: a file of fa bytes whose local copy is fb <= fa bytes
    that all differ from the file's, the last one from the file's last byte too."""
    f = fresh(fa)
    loc = f[:fb] ^ 0xFF  # (the pool holds 0x61..0x70: a complement equals no pool byte, the file's last included)
    return Case("filler_%d" % k, "filler", [f.tobytes()], loc.tobytes(), reference(f.tobytes(), loc.tobytes()),
                tag=("filler", fa, fb))


def lay_out(cases: Sequence[Case]) -> Corpus:
    """One chain list: before every case that names an alignment, a filler of
    at least one byte that puts the case's local bytes at `align` mod 16 and,
    with raw blocks, its source `rel` further (mod 16); one filler at the end.
    Every such case lies between two fillers, whose bytes just outside it
    differ."""
    out, pos, loff = [], 0, 0

    def put(c):
        nonlocal pos, loff
        ch = wire(c, "r")
        blks = blks_of(c, ch)
        _, pos = stage(blks, pos)
        live = 0
        while live < len(blks) and blks[live].inflates:
            live += 1
        loff += min(sum(b.plain_len for b in blks[:live]), len(c.local))
        out.append(c)

    for c in cases:
        if c.align is not None:
            fb = ((c.align - loff) & 15) or 16
            fa = fb + ((c.align + c.rel - pos - fb) & 15)
            put(_filler(len(out), fa, fb))
        put(c)
    put(_filler(len(out), 16, 16))
    return Corpus(out)


@functools.lru_cache(maxsize=None)
def k11_corpus() -> Corpus:
    _seq[0] = 0
    return lay_out(family_f() + family_g() + family_l() + family_w() + family_s() + family_ht())


# --------------------------------------------------- windows and passes (X) --
X_MB = 8192
X_BLOCKS = (5000, 8000, 6111, 7001, 4097, 8192)
X_WB = 2 * 8448 + 6 * 512  # window_bytes of the diff_files run: two max_block shares and six small files' more


@dataclass
class XSet:
    blocks: List[bytes]
    wired: List[tuple]                 # (type, field) per block: zlib and raw in turn
    ids: List[bytes]
    locals: Dict[str, Tuple[bytes, Optional[int]]]  # name -> (local copy, expected)
    flips: Dict[str, List[int]]


@functools.lru_cache(maxsize=None)
def x_set() -> XSet:
    """A file of six blocks, two per window, with a flip in the second window
    only, the third only, the first and third, and each."""
    _seq[0] = 100000
    bl = [fresh(n) for n in X_BLOCKS]
    whole = np.concatenate(bl)
    offs = np.concatenate([[0], np.cumsum(X_BLOCKS)]).tolist()
    at = {0: offs[1] - 1, 1: offs[2] + 6000, 2: offs[5] + 17}  # one designed offset per window
    flips = {"same": [], "second": [at[1]], "third": [at[2]], "first_third": [at[0], at[2]],
             "each": [at[0], at[1], at[2]]}
    locs = {k: (flipped(whole, v, 0x20), min(v) if v else None) for k, v in flips.items()}
    blocks = [b.tobytes() for b in bl]
    wired = [(ZLIB, zlib.compress(b, 6)) if k % 2 == 0 else (RAW, b) for k, b in enumerate(blocks)]
    return XSet(blocks, wired, [block_id(b) for b in blocks], locs, flips)


def x_window_of(x: int, per: int = 2) -> int:
    """hbx_restore_file_stream: `per` blocks a window."""
    offs = np.concatenate([[0], np.cumsum(X_BLOCKS)])
    return (int(np.searchsorted(offs, x, side="right")) - 1) // per


def x_files(n_small: int = 20):
    """The X file between twenty small one-block files (ten before, ten
    behind): (plain blocks per file, wired per file, ids per file)."""
    xs = x_set()
    _seq[0] = 200000
    small = [fresh(100 + 13 * k).tobytes() for k in range(n_small)]
    files = [[s] for s in small[:n_small // 2]] + [xs.blocks] + [[s] for s in small[n_small // 2:]]
    wired = [[(RAW, s)] if k % 3 else [(ZLIB, zlib.compress(s, 6))] for k, s in enumerate(small[:n_small // 2])]
    wired += [xs.wired]
    wired += [[(RAW, s)] if k % 3 else [(ZLIB, zlib.compress(s, 6))] for k, s in enumerate(small[n_small // 2:])]
    return files, wired, [[block_id(b) for b in f] for f in files]


def x_passes(files, wired, wb: int, mb: int = X_MB):
    """The windows of hbx_restore_files_stream with exact size hints (a zlib
    block's capacity is min(max_block, file size), a raw block's its length)
    as lists of (file, block); one pass per window (no stream outgrows its
    slot)."""
    caps = [min(mb, sum(len(b) for b in f)) if t == ZLIB else len(d) for f, w in zip(files, wired) for t, d in w]
    owner = [(f, k) for f, w in enumerate(wired) for k in range(len(w))]
    out, s = [], 0
    while s < len(caps):
        e = window_end(caps, wb, s)
        out.append(owner[s:e])
        s = e
    return out


# ------------------------------------------------------------ K10's calls --
@dataclass
class Call:
    """One hbx_restore_blocks call in diff mode."""
    case: Case
    mode: str            # 'r' or 'z' for the case's own blocks
    pre: bytes = b""     # a raw block before them (identical in the local copy): the local alignment

    def chain(self):
        ch = wire(self.case, self.mode)
        if self.pre:
            ch = [(RAW, self.pre, block_id(self.pre))] + ch
        return ch

    def local(self) -> bytes:
        return self.pre + self.case.local

    def want(self) -> Optional[int]:
        return None if self.case.want is None else self.case.want + len(self.pre)

    def restored(self) -> bytes:
        return self.pre + self.case.restored()

    def layout(self, chain=None) -> Layout:
        ch = chain if chain is not None else self.chain()
        blks = blks_of(self.case, ch[1:] if self.pre else ch)
        if self.pre:
            blks = [Blk(RAW, len(self.pre), len(self.pre))] + blks
        return k10_layout(blks, len(self.local()))


def k10_wave_lane(k: int) -> int:
    """Lane k of wave k % 4: the 64 only-holder cases visit every wave."""
    return 64 * (k % 4) + k


@functools.lru_cache(maxsize=None)
def k10_calls() -> List[Call]:
    _seq[0] = 300000
    out = []
    for c in family_l(T10, PIECE, aligns=(0,), lanes=(0, 100, 255)):
        out.append(Call(c, "r"))
    for c in family_w(T10, PIECE, pair_lanes=(0, 5, 10, 23, 36, 49, 58, 63), lane_of=k10_wave_lane,
                      ab_base=128, aligns=False):  # (no block in front: the piece lies at local offset 0)
        out.append(Call(c, "r"))
    for c in family_s(PIECE):
        out.append(Call(c, "r"))
    # WG: each wave the only holder; each pair of waves with the smaller offset once in each
    n2 = 32 * T10 + 16 + 3
    for w in range(4):
        out.append(Call(_granule_case("WG_only_w%d" % w, "WG", T10, PIECE, 0, [(64 * w + 11 * w + 7, 0)],
                                      ("only", w), n=n2), "r"))
    for a in range(4):
        for b in range(a + 1, 4):
            la, lb = 64 * a + 50 - 9 * a, 64 * b + 3 + 5 * b
            out.append(Call(_granule_case("WG_%d_%d_a" % (a, b), "WG", T10, PIECE, 0, [(la, 0), (lb, 0)],
                                          ("pair", a, b, a), n=n2), "r"))
            out.append(Call(_granule_case("WG_%d_%d_b" % (a, b), "WG", T10, PIECE, 0, [(la, 1), (lb, 0)],
                                          ("pair", a, b, b), n=n2), "r"))
    for lens, mode in ((K10_HT_LENS, "r"), (K10_HT_ZLENS, "z")):
        for n in lens:
            for a in range(16):
                pre = fresh(a).tobytes()
                for way in HT_WAYS:
                    at = {"same": [], "first": [0], "last": [n - 1], "both": [0, n - 1]}[way]
                    out.append(Call(_one("HT_%s_n%d_a%d_%s" % (mode, n, a, way), "HT", fresh(n), at,
                                         tag=("ht", mode, n, a, way)), mode, pre))
    pre = fresh(16 + 9).tobytes()  # local alignment 9: a head of 7, then the granule
    for i in range(16):
        for j in range(i + 1, 16):
            x = XORS[(i + j) % 3]
            out.append(Call(_one("G_%d_%d_%02x" % (i, j, x), "G", fresh(7 + 48 + 5), [7 + 16 + i, 7 + 16 + j], x,
                                 tag=("pair", 9, i, j, x)), "r", pre))
    out.append(Call(_one("G_all16", "G", fresh(7 + 48 + 5), range(7 + 16, 7 + 32), tag=("all16", 9, 1)), "r", pre))
    return out
