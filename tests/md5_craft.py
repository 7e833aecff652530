"""Designed inputs for the block-MD5 chains (md5_run, md5_tail, msg_word,
md5_block_at, md5_coop, k3p_produce / k3p_consume, the mixed-count rounds of
k3_body, K6 and K6p in hashbox_amd/csrc/hbx_kernels.hip).

Three parts:

* the reference: ``ref_id`` = hashlib.md5(BE32(n_links) || links || BE32(len)
  || data), nothing else;
* the arena builder: blocks at chosen byte addresses in an arena whose every
  other byte is non-zero filler, so a kernel that hashes one byte outside
  [src, src + len) gets another ID;
* the path model: a restatement of the few expressions that decide which code
  a chain runs through.  Every piece quotes the kernel expression it mirrors,
  and MIRRORED lists those expressions: tests/test_md5_craft.py asserts that
  each still occurs in the source, so an edit of one of these lines fails
  there and sends its author here (a rule rewritten elsewhere in the kernel
  is only seen by the GPU witnesses: the probe and the launch counts).  It
  also asserts on the model that the families below reach the branches they
  claim.

Nothing here needs a GPU.
"""
from __future__ import annotations

import hashlib
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ARENA_SLACK = 64       # HBX_ARENA_SLACK (include/hbxgpu.h)
GAP = 128              # least filler between two blocks
HEAD = 256             # filler before the first block
TAIL = ARENA_SLACK + 64 + 896  # filler after the last block (>= HBX_ARENA_SLACK + 64)
COOP_MIN = 8           # kCoopMinBudget
BPS = 4                # Coop<16>::BPS, message blocks per stage
PLAN_BINS = 1024       # kPlanBins
MAX_BLOCK = 8 << 20    # kMaxBlock
BUDGET_ALL = 0xFFFFFFFF  # kBudgetAll (a drain)


# The source lines the model restates, by file under hashbox_amd/csrc (white
# space is collapsed before the comparison).
MIRRORED = {
    "hbx_device.h": ["constexpr uint32_t kMaxBlock = 8388608u;"],
    "hbx_kernels.hip": [
        "constexpr uint32_t kCoopMinBudget = 8u;",
        "constexpr uint32_t kPlanBins = 1024u;",
        "constexpr uint32_t kBudgetAll = 0xFFFFFFFFu;",
        "static constexpr uint32_t BPS = G / 4u;",
        "#define HBX_SLICE_REM_FIRST 1",
        "#define HBX_MD5_RING 8",
        "md5_run<PROD ? 4 : HBX_MD5_RING>(src, len, h, pos, rem, finish);",
        "md5_run<PROD ? 4 : HBX_MD5_RING>(src, len, h, b0, cnt, finish);",
        # chain_path
        "const uint32_t p = 8u + 16u * nl;",
        "const uint64_t T = (uint64_t)len + p;",
        "const uint32_t nfull = (uint32_t)(T >> 6);",
        "const uint32_t hb = (p + 63u) >> 6;",
        "const bool fast = nfull >= hb;",
        "const uint32_t cnt = fast ? nfull - hb : 0u;",
        "const uint32_t ntail = finish ? ((rem + 9u > 64u) ? 2u : 1u) : 0u;",
        "rem = ((len + 8u) >> 6) + 1u;",
        "ch.next = hb;",
        "rem = nfull - hb + 1u;",
        # slice_cnt, order_bin, plan_bin
        "if (left <= budget) return left;",
        "return HBX_SLICE_REM_FIRST ? (left - 1u) % budget + 1u : budget;",
        "const uint32_t ref = min(budget, (uint32_t)(kMaxBlock >> 6) + 1u);",
        "return (ref - c) * (kPlanBins - 1u) / ref;",
        "if (cnt == budget) return (uint32_t)((reinterpret_cast<const Chain*>(o.chain)->src >> ashift) % abins);",
        "return abins + (ref - c) * (kPlanBins - 1u - abins) / ref;",
        # k3_wave, k3q_parts
        "if constexpr (!ITEMS) return ~wave_max_all(L.live ? ~L.cnt : 0u);",
        "const uint32_t m = wave_max_all((L.cnt || L.finish) ? ~L.cnt : 0u);",
        "if (R >= kCoopMinBudget) { // wave-uniform",
        "k3p_consume(wl, flags, S, R - 1u, h, polls, spin);",
        "md5_coop<16>(wl, src, h, L.next + 1u, R - 1u);",
        "const uint32_t nst = (4u * Rr + 15u) / 16u;",
        "for (uint32_t u = 1; 4u * (nst - 1u) + u < Rr; u++) {",
        "uint32_t pos = b0 + R, rem = cnt ? cnt - R : 0u;",
        "for (int round = 0; round < 4; round++) {",
        "if (mx == 0u || ~mx < kCoopMinBudget) break;",
        "const uint32_t nmax = wave_max_all(cnt);",
        "pR = R;",
        "pmax = wave_max_all(cnt);",
        "p[3] = (uint64_t)min(pR, 0xffffu) | ((uint64_t)min(pmax, 0xffffu) << 16) | ((uint64_t)hw << 32);",
        "const uint32_t per_part = ITEMS ? (budget == kBudgetAll ? kBudgetAll : (budget + Q.parts - 1u) / Q.parts) : 0u;",
        "const uint32_t hi = (uint64_t)lo + per_part < total ? lo + per_part : total;",
        "if (L.cnt == 0u && !L.finish) {",
        # k6_wave
        "const uint32_t R = ~wave_max_all(active ? ~cnt : 0u);",
        "const uint32_t Rc = R >= kCoopMinBudget ? R : 0u;",
        "const uint32_t rest = cnt - Rc;",
    ],
    "hbx_engine.hip": [
        # k6_waves
        "std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });",
        # k3_need, k3_launches, k3q_parts
        "longest = std::max<uint64_t>(longest, (lens[i] + 8ull + 16ull * nl) >> 6);",
        "b->need = budget == kBudgetAll ? 1u : (uint32_t)std::max<uint64_t>(1, (longest + lb - 1) / lb);",
        "uint64_t k = size + older >= c->join_lag ? size + older + 1 - c->join_lag : 0;",
        "if (drain) k = std::max<uint64_t>(k, 1);",
        "return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, size), kMaxFresh);",
        "if (!live) return HBX_OK;",
        "const bool hashed = budget == kBudgetAll || b->done >= b->need;",
        "const uint32_t parts = c->k3_items && budget != kBudgetAll && budget >= 64u * c->k3_items ? c->k3_items : 0u;",
    ],
}


# ------------------------------------------------------------- reference --
def ref_id(data, links: Sequence[bytes] = ()) -> bytes:
    """HashboxBlock.HashData: MD5(BE32(n_links) || links || BE32(len) || data)."""
    d = bytes(data)
    return hashlib.md5(struct.pack(">I", len(links)) + b"".join(links) + struct.pack(">I", len(d)) + d).digest()


# ------------------------------------------------------------ path model --
@dataclass(frozen=True)
class ChainPath:
    """What one block's message looks like to K6 / K6p / K3."""
    L: int
    length: int
    p: int        # prefix bytes          `p = 8u + 16u * nl`
    T: int        # message bytes         `T = (uint64_t)len + p`
    full: int     # full message blocks   `nfull = (uint32_t)(T >> 6)`
    residue: int  # bytes in the tail     md5_tail: `rem = T - 64u * nfull`
    tails: int    # padded tail blocks    md5_tail: `(rem + 9u > 64u) ? 2u : 1u`
    hb: int       # blocks with prefix    `hb = (p + 63u) >> 6`
    fast: bool    # `fast = nfull >= hb` (else K6 / K6p finish it byte by byte)
    k6_cnt: int   # hbx_k6_hash_blocks: `cnt = fast ? nfull - hb : 0u`
    k3_next: Optional[int]  # hbx_k6p_verify_chains: `ch.next` (None: finished in K6p)
    k3_left: Optional[int]  # ... `rem - 1`: full blocks K3 still hashes


def chain_path(L: int, length: int) -> ChainPath:
    p = 8 + 16 * L
    T = p + length
    full = T >> 6
    residue = T & 63
    tails = 2 if residue + 9 > 64 else 1
    hb = (p + 63) >> 6
    fast = full >= hb
    if L == 0:          # `if (nl == 0u) { ch.next = 0u; rem = ((len + 8u) >> 6) + 1u; }`
        nxt, left = 0, full
    elif fast:          # `ch.next = hb; rem = nfull - hb + 1u;`
        nxt, left = hb, full - hb
    else:               # `if (!fast) { ... return; }`
        nxt, left = None, None
    return ChainPath(L, length, p, T, full, residue, tails, hb, fast, full - hb if fast else 0, nxt, left)


def length_for(L: int, count: int, residue: int, door: str = "k3") -> int:
    """Data bytes of a block with `count` blocks on the streaming path and
    `residue` message bytes in its tail.  door "k3": count = K3's `left`
    (L == 0: every full block; L > 0: the blocks after the prefix blocks);
    door "k6": count = K6's `cnt` (the blocks after the prefix blocks)."""
    p = 8 + 16 * L
    hb = (p + 63) >> 6
    full = count if (door == "k3" and L == 0) else hb + count
    n = 64 * full + residue - p
    if n < 0:
        raise ValueError("no such block: L=%d count=%d residue=%d" % (L, count, residue))
    return n


def slice_cnt(left: int, budget: int) -> int:
    """slice_cnt(): `if (left <= budget) return left;
    return HBX_SLICE_REM_FIRST ? (left - 1u) % budget + 1u : budget;`"""
    if left <= budget:
        return left
    return (left - 1) % budget + 1


def launch_counts(left: int, budget: int) -> List[int]:
    """The blocks a chain hashes in each of its launches (the planner's
    `o.rem - slice_cnt(o.rem - 1u, bprev)`), remainder first."""
    out = []
    while True:
        c = slice_cnt(left, budget)
        out.append(c)
        left -= c
        if left == 0:
            return out


def order_bin(cnt: int, budget: int) -> int:
    """order_bin(): `ref = min(budget, (kMaxBlock >> 6) + 1); c = min(cnt, ref);
    return (ref - c) * (kPlanBins - 1u) / ref;`"""
    ref = min(budget, (MAX_BLOCK >> 6) + 1)
    c = min(cnt, ref)
    return (ref - c) * (PLAN_BINS - 1) // ref


def plan_bin(cnt: int, budget: int, abins: int = 512, src: int = 0, ashift: int = 29) -> int:
    """plan_bin() for a chain whose launch count is `cnt`: full slices by
    address (`(src >> ashift) % abins`), the rest by descending count in
    `abins + (ref - c) * (kPlanBins - 1u - abins) / ref`."""
    if not abins:
        return order_bin(cnt, budget)
    if cnt == budget:
        return (src >> ashift) % abins
    ref = min(budget, (MAX_BLOCK >> 6) + 1)
    c = min(cnt, ref)
    return abins + (ref - c) * (PLAN_BINS - 1 - abins) // ref


@dataclass
class K3Wave:
    """One K3 group (k3_body) given its live lanes' launch counts."""
    R: int                 # k3_wave_R: the smallest count over the live lanes
    coop: bool             # `if (R >= kCoopMinBudget)`
    coop_blocks: int = 0   # after md5_block_at: `R - 1u` blocks from stages
    stages: int = 0        # k3p_consume: `nst = (4u * Rr + 15u) / 16u`
    last_stage: int = 0    # blocks hashed from the last stage (1..4)
    rounds: List[int] = field(default_factory=list)  # R2 of each mixed round
    run: List[int] = field(default_factory=list)     # per lane: what md5_run gets
    nmax: int = 0          # md5_run: `nmax = wave_max_all(cnt)`
    probe_R: int = 0       # probe word 3 bits 0..15 (`pR`, 0 on the lane path)
    probe_max: int = 0     # probe word 3 bits 16..31 (`pmax`)


def k3_wave(counts: Sequence[int]) -> K3Wave:
    counts = list(counts)
    R = min(counts)        # `~wave_max_all(L.live ? ~L.cnt : 0u)`
    if R < COOP_MIN:       # the lane path: `md5_run(src, len, h, b0, cnt, finish)`
        return K3Wave(R, False, run=counts, nmax=max(counts))
    w = K3Wave(R, True, coop_blocks=R - 1, stages=(4 * (R - 1) + 15) // 16)
    w.last_stage = (R - 1) - BPS * (w.stages - 1)
    rem = [c - R for c in counts]          # `rem = cnt ? cnt - R : 0u`
    for _ in range(4):                     # `for (int round = 0; round < 4; round++)`
        nz = [r for r in rem if r]
        if not nz or min(nz) < COOP_MIN:   # `if (mx == 0u || ~mx < kCoopMinBudget) break;`
            break
        R2 = min(nz)
        w.rounds.append(R2)
        rem = [r - R2 if r else 0 for r in rem]
    w.run, w.nmax = rem, max(rem)          # `md5_run(src, len, h, pos, rem, finish)`
    w.probe_R, w.probe_max = min(R, 0xFFFF), min(max(counts), 0xFFFF)
    return w


def k3q_parts(counts: Sequence[int], budget: int, items: int) -> List[List[int]]:
    """K3Q: the blocks each lane hashes in each item (part) of its group's
    launch.  md5_launch: `parts = k3_items && budget != kBudgetAll && budget
    >= 64u * k3_items ? k3_items : 0u` (0: the K3P kernel, one part);
    k3_body: `per_part = (budget + Q.parts - 1u) / Q.parts`; k3_lane<true>:
    `lo = part * per_part`, `hi = min(lo + per_part, total)`.  A lane with
    nothing in a part (`L.cnt == 0u && !L.finish`) shadows the lane with the
    most blocks there and is not counted in that part's R."""
    parts = items if items and budget != BUDGET_ALL and budget >= 64 * items else 0
    if not parts:
        return [list(counts)]
    per = (budget + parts - 1) // parts
    return [[max(0, min(c, (h + 1) * per) - h * per) for c in counts] for h in range(parts)]


@dataclass
class K6Wave:
    Rc: int          # `Rc = R >= kCoopMinBudget ? R : 0u`
    rest: List[int]  # `rest = cnt - Rc`
    nmax: int


def k6_wave(counts: Sequence[int]) -> K6Wave:
    R = min(counts)  # `R = ~wave_max_all(active ? ~cnt : 0u)`
    Rc = R if R >= COOP_MIN else 0
    rest = [c - Rc for c in counts]
    return K6Wave(Rc, rest, max(rest))


def k6_waves(lengths: Sequence[int]) -> List[List[int]]:
    """verify_device: `std::stable_sort(perm, lens[a] > lens[b])`, wave w =
    sorted blocks [64 w, 64 w + 64).  Returns the block indices of each wave."""
    perm = np.argsort(-np.asarray(lengths, np.int64), kind="stable").tolist()
    return [perm[i:i + 64] for i in range(0, len(perm), 64)]


def k3_need(paths: Sequence[ChainPath], budget: int) -> int:
    """submit_verify: `longest = max((lens[i] + 8 + 16 nl) >> 6)`,
    `b->need = max(1, (longest + lb - 1) / lb)`: the launches after which the
    batch counts as hashed."""
    longest = max([c.full for c in paths] or [0])
    return 1 if budget == BUDGET_ALL else max(1, (longest + budget - 1) // budget)


def k3_launches(needs_and_sizes: Sequence[Tuple[int, int]], join_lag: int) -> int:
    """K3 launches of a run that submits the batches (need, n) in order and
    then waits for all of them in FIFO order (md5_step, joiners, md5_launch,
    wait_oldest; K3 period 1, join lag 1 or 2).  It holds for an engine that
    has only seen verify batches: there plan_mode_of() is 0 or 1 and no launch
    is planned ahead.  Once submit_device has created the cut stream, lag 2
    with the default plan_cut plans one launch ahead (mode 3, preplan), which
    this model does not restate."""
    pend, unjoined, launches = [], [], 0

    def step(drain):
        nonlocal launches
        size = len(unjoined)
        k = size + 1 - join_lag if size >= join_lag else 0  # joiners(c, 0, drain)
        if drain:
            k = max(k, 1)
        k = min(k, size, 8)
        if not k and not any(b["joined"] and not b["fin"] for b in pend):
            return                                           # `if (!live) return HBX_OK;`
        for _ in range(k):
            unjoined.pop(0)["joined"] = True
        launches += 1
        for b in pend:                                       # md5_launch
            if b["joined"] and not b["fin"]:
                b["done"] += 1
                b["fin"] = drain or b["done"] >= b["need"]

    for need, n in needs_and_sizes:
        step(False)                                          # `md5_step(c, budget)` comes first
        b = dict(need=need, joined=False, done=0, fin=n == 0)
        pend.append(b)
        if n:
            unjoined.append(b)
    for b in pend:                                           # wait_oldest
        while not b["fin"]:
            step(True)
    return launches


# ------------------------------------------------------------- the arena --
@dataclass
class Spec:
    """One designed block: n_links, data bytes, byte address mod 64, and the
    name of the lane class it stands for."""
    L: int
    length: int
    amod: int
    cls: str


@dataclass
class CaseSet:
    """Blocks placed in one arena.  `groups` names index ranges that go
    through a door together (one call, or one batch)."""
    name: str
    specs: List[Spec]
    offs: np.ndarray
    host: np.ndarray
    links: List[List[bytes]]
    groups: Dict[str, List[int]]
    _ref: Optional[List[bytes]] = None
    _paths: Optional[List[ChainPath]] = None

    @property
    def lens(self) -> np.ndarray:
        return np.array([s.length for s in self.specs], np.uint64)

    @property
    def paths(self) -> List[ChainPath]:
        if self._paths is None:
            self._paths = [chain_path(s.L, s.length) for s in self.specs]
        return self._paths

    def data(self, i: int) -> np.ndarray:
        o = int(self.offs[i])
        return self.host[o:o + self.specs[i].length]

    def ref(self) -> List[bytes]:
        """ref_id of every block, computed once."""
        if self._ref is None:
            self._ref = [ref_id(self.data(i).tobytes(), self.links[i]) for i in range(len(self.specs))]
        return self._ref

    def k3_counts(self, idx: Sequence[int], budget: int = BUDGET_ALL) -> List[int]:
        """First-launch counts of the chains of `idx` that reach K3."""
        return [slice_cnt(self.paths[i].k3_left, budget) for i in idx if self.paths[i].k3_left is not None]

    def describe(self, i: int) -> str:
        s, c = self.specs[i], self.paths[i]
        return "%s[%d] %s: L=%d len=%d addr%%64=%d sh=%d full=%d residue=%d tails=%d k6_cnt=%d k3_left=%s" % (
            self.name, i, s.cls, s.L, s.length, s.amod, s.amod & 3, c.full, c.residue, c.tails, c.k6_cnt, c.k3_left)


def filler(n: int, seed: int) -> np.ndarray:
    """Non-zero pseudo-random bytes that are never 0x80 either: in place of a
    pad byte (0x80, then zeros) or OR-ed into it, every one changes the ID."""
    v = np.random.Generator(np.random.PCG64(seed)).integers(1, 255, n, dtype=np.uint8)  # 1..254
    v[v == 0x80] = 0xFF
    return v


def build(name: str, specs: Sequence[Spec], groups: Dict[str, List[int]], seed: int) -> CaseSet:
    """Lay the blocks out in order, each at the next address with the wanted
    residue mod 64 that leaves >= GAP filler bytes after the previous one;
    the arena's base is taken as 64-aligned (the GPU test checks the
    tensor's).  Data and links come from a generator of their own."""
    offs, pos = [], HEAD
    for s in specs:
        o = pos + ((s.amod - pos) % 64)
        offs.append(o)
        pos = o + s.length + GAP
    host = filler(pos + TAIL, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    data = rng.integers(0, 256, sum(s.length for s in specs), dtype=np.uint8)
    at = 0
    for s, o in zip(specs, offs):
        host[o:o + s.length] = data[at:at + s.length]
        at += s.length
    links = [[rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(s.L)] for s in specs]
    return CaseSet(name, list(specs), np.array(offs, np.uint64), host, links, groups)


# ----------------------------------------------------------- the families --
A_LINKS = (0, 1, 2, 3, 4)
A_LENS = range(0, 192)


def family_a() -> CaseSet:
    """Every residue at every alignment, short: prefixes 8..72, data 0..191
    bytes (three message blocks, one and two tail blocks, fast both ways),
    every address mod 16.  All waves on the lane path."""
    specs = [Spec(L, n, a16 + 16 * ((n + L) & 3), "A L=%d" % L)
             for L in A_LINKS for n in A_LENS for a16 in range(16)]
    return build("A", specs, {"all": list(range(len(specs)))}, 1001)


B_LINKS = (0, 1, 4)
B_COUNTS = range(7, 35)  # K6 data-block counts (K3: the same for L > 0, one more for L == 0)


def b_amod(lane: int, c: int) -> int:
    """Address mod 64 of lane `lane` of class `c`: a permutation of 0..63 per
    class (37 is odd), shifted per class so that one residue meets every sh."""
    return (37 * lane + 5 * c + 11) % 64


def family_b() -> CaseSet:
    """Uniform waves: per L and K6 count c one class of 64 blocks, residue =
    lane, address residues a permutation of the lanes.  Class lengths do not
    interleave within one L (64 consecutive lengths per class), so sorted by
    length each wave is one class."""
    specs, groups = [], {}
    for L in B_LINKS:
        idx = []
        for c in B_COUNTS:
            for lane in range(64):
                idx.append(len(specs))
                specs.append(Spec(L, length_for(L, c, lane, "k6"), b_amod(lane, c), "B L=%d c=%d" % (L, c)))
        groups["L%d" % L] = idx
    return build("B", specs, groups, 2002)


C_LINKS = (0, 1)
NMAX_EDGES = (3, 4, 5, 7, 8, 9, 16, 17)  # around md5_run's rings of 4 (K3P) and 8 (K3, K6)


def c_compositions() -> Dict[str, List[int]]:
    """K3 launch counts per lane of each designed group (one batch each)."""
    comp = {
        "40x63+39": [40] * 63 + [39],
        "40x63+32": [40] * 63 + [32],
        "40x63+8": [40] * 63 + [8],
        "40x63+7": [40] * 63 + [7],        # the whole wave to the lane path
        "40x63+0": [40] * 63 + [0],        # a lane that only finishes
        "40+9x63": [40] + [9] * 63,
        "steps8": [8 * (1 + j // 8) for j in range(64)],  # four rounds, then a remainder
        "rounds2": [8 * (1 + j % 3) for j in range(64)],  # two rounds, nothing left
        "rounds3": [8 * (1 + j % 4) for j in range(64)],  # three rounds, nothing left
        "8to15": [8 + j % 8 for j in range(64)],          # first remainder below 8: no round
        "n1": [40],
        "n2": [40, 12],
        "n63": [24 + 6 * (j & 1) for j in range(63)],
        "n65": [40] * 65,                  # a second group of one
        "64x64": [64] * 64,                # a whole slice of 64 for every lane
        # counts past a K3Q part of 64 blocks (budget 128 / 2 items, 256 / 4): chains cross parts
        "parts-lane": [100] * 32 + [70] * 16 + [127] * 8 + [65] * 8,  # part 1: 36, 6, 63, 1: the lane path
        "parts-coop": [120] * 63 + [80],                              # part 1: 63x56 + 16: a mixed round
        "parts-shadow": [127] * 32 + [40] * 32,                       # part 1: half the lanes only shadow
    }
    for m in NMAX_EDGES:
        comp["coop-nmax%d" % m] = [20] * 62 + [21, 20 + m]  # remainders 1 and m: no round, md5_run
        comp["lane-nmax%d" % m] = [2] * 62 + [1, m]         # lane path
    return comp


def family_c() -> CaseSet:
    """Designed mixed groups; residues and addresses mixed as in B."""
    specs, groups = [], {}
    for L in C_LINKS:
        for k, (name, counts) in enumerate(c_compositions().items()):
            idx = []
            for j, cnt in enumerate(counts):
                r = (29 * j + 7 * k + 3) % 64
                if L == 0 and cnt == 0:
                    r = 8 + r % 56         # the message holds at least the 8 prefix bytes
                idx.append(len(specs))
                specs.append(Spec(L, length_for(L, cnt, r, "k3"), (37 * j + 13 * k + 5) % 64,
                                  "C %s L=%d" % (name, L)))
            groups["%s/L%d" % (name, L)] = idx
    return build("C", specs, groups, 3003)


D_SLICES = (3, 9, 12, 64)
D_B_CLASSES = (7, 8, 20, 24, 34)


def d_groups(b: CaseSet, c: CaseSet) -> List[Tuple[CaseSet, str, List[int]]]:
    """The batches family D slices: every group of C, a few classes of B."""
    out = [(c, g, idx) for g, idx in c.groups.items()]
    for L in B_LINKS:
        for cc in D_B_CLASSES:
            at = (cc - B_COUNTS[0]) * 64
            out.append((b, "B L=%d c=%d" % (L, cc), b.groups["L%d" % L][at:at + 64]))
    return out


def family_e(b: CaseSet) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The chunking door: one-chunk files of B's L = 0 lengths at offsets that
    are 16-aligned but not 64-aligned, in a filler arena.  Returns (host,
    offs, lens)."""
    lens = [b.specs[i].length for i in b.groups["L0"]]
    specs = [Spec(0, n, 16 * (1 + i % 3), "E") for i, n in enumerate(lens)]
    e = build("E", specs, {}, 5005)
    return e.host, e.offs, e.lens


F_MSG = range(48, 201)
F_LINKS = (0, 1, 3, 4)
