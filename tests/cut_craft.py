"""Hand-built inputs for the cut rule (store.go:111-166, K1 + K2).

The cut of the chunk starting at ``s`` is the LAST position of the maximum
window digest over ``q in [qa, qb] = [s+MIN-1, s+L-1]`` (``q`` the last byte
of a window, the cut ``q+1``).  K2 decides it from one summary per 4,096
positions with three comparison rules (first edge slice ``>``, interior
slices the last ``>=``, last edge slice ``>=``) and a bounded re-scan; random
bytes never tie, so none of that is reached by the rest of the suite.  Under
assumption A1 the digest is a closed form in the bytes (``s1`` the byte sum,
``s2 = 0x8000 + sum (k+1) x[q-k]``, both mod 2^16, ``D = s2 << 16 | s1``), so
maxima and exact ties can be put at chosen file positions:

* ``marker``: one byte ``v`` (odd) on a constant background peaks exactly
  once, ``D = 0xFFFF0000 | v`` at ``k(v)`` positions after the byte; equal
  ``v`` tie, different ``v`` order strictly; nothing else reaches
  ``0xFFFF0000`` while the bytes stay MIN apart.
* ``comb``: a byte ``v = 2^j`` peaks ``v`` times, ``MIN / v`` apart, all tied.
* ``plateau``: on a background of ones, ``+1`` at ``p`` and ``-1`` at ``p+d``
  give ``D = d << 16`` on every ``q`` in ``[p+d, p+MIN-1]``; the position
  before it is higher, so it is a range's maximum only when it starts at
  ``qa``, which the previous cut is designed for.
* ``periodic``: a random tile repeated; ``D`` has the tile's period.

``CASES`` names one input per property (built on demand) with the cuts it is
designed to produce and a check of the property on ``digest_all`` alone;
``classify`` and ``chain`` restate the rule from ``digest_all`` and say which
of K2's three sources the answer lies in.  ``test_cut_craft.py`` holds the
table against the oracle, ``test_gpu_cut_crafted.py`` the device against it,
``test_segmented.py`` takes ``SEG_FILES``.

No dependence on the GPU.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle as O

MIN, MAX = O.MIN_BLOCK_SIZE, O.MAX_BLOCK_SIZE
SLICE_SHIFT = 12
SLICE = 1 << SLICE_SHIFT
Mi = 1 << 20
FIRST, INTERIOR, LAST, NONE = "first edge", "interior", "last edge", "no candidate"
SOURCES = (FIRST, INTERIOR, LAST)
HALF = 0x80000000

# bullet names of the case list (the issue's), each needs a named case
BULLETS = (
    "unique: qa", "unique: qa+1", "unique: qb-1", "unique: qb", "unique: slice position 0",
    "unique: slice position 4095", "unique: run residue 0", "unique: run residue 31", "unique: run residue 32",
    "unique: run residue 63", "unique: iteration first", "unique: iteration last", "unique: tile of 3 first",
    "unique: tile of 3 last", "unique: N-1, end mid-slice", "unique: N-2, end mid-slice", "unique: N-1, end 16",
    "unique: N-2, end 16", "unique: N-1, end 64", "unique: N-2, end 64", "unique: N-1, end 4096",
    "unique: N-2, end 4096",
    "narrowest: qa", "narrowest: qb", "narrowest: middle", "narrowest: no candidate",
    "overstated: qa-1, winner elsewhere", "overstated: qb+1, winner elsewhere",
    "overstated: qa-1, winner in the same slice", "overstated: qb+1, winner in the same slice",
    "sources: first = interior", "sources: first = last", "sources: interior = last",
    "sources: first strictly greater", "sources: first greater by v only",
    "interior: same lane, different loads", "interior: same load, different lanes",
    "interior: earlier in higher lane and lower load", "interior: earlier in lower lane and lower load",
    "interior: three or more",
    "in-slice: plateau ends in the first edge slice", "in-slice: plateau ends at position 4095",
    "in-slice: plateau ends at position 0 of the next slice", "in-slice: plateau over several slices",
    "in-slice: short period",
    "sign: all below 0x80000000", "sign: straddles 0x80000000",
    "chain",
)


# ------------------------------------------------------------ constructions --
@functools.lru_cache(maxsize=None)
def k_of(v: int, bg: int = 0, top: int = 0xFFFF) -> int:
    """The smallest k at which a byte ``bg + v`` at p, alone on a background of
    constant ``bg``, gives ``s2 == top`` at ``q = p + k``.  Found by search over
    the closed form ``s2 = s2(background) + (k+1) v``."""
    base = 0x8000 if bg % 2 == 0 else 0  # 0x8000 + bg * MIN (MIN+1) / 2 mod 2^16
    s2 = (base + np.arange(1, MIN + 1, dtype=np.int64) * v) & 0xFFFF
    hit = np.flatnonzero(s2 == top)
    assert hit.size, (v, bg, hex(top))
    return int(hit[0])


def peak(v: int) -> int:
    return 0xFFFF0000 | v


def marker(x: np.ndarray, q: int, v: int, bg: int = 0) -> int:
    """Make ``D[q] = 0xFFFF0000 | v`` the one peak of a byte ``bg + v``.
    Returns the byte's position."""
    p = q - k_of(v, bg)
    assert 0 <= p and q < x.size and x[p] == bg, (q, v, p)
    x[p] = bg + v
    return p


def comb(x: np.ndarray, q: int, v: int) -> list:
    """A byte ``v = 2^j`` on zeros: ``D = (0x10000 - v) << 16 | v`` at q and
    every ``MIN / v`` after it, v times in all.  Returns the tied positions
    inside the file."""
    assert v & (v - 1) == 0 and 1 < v < 256
    p = q - k_of(v, 0, 0x10000 - v)
    assert 0 <= p and x[p] == 0
    x[p] = v
    return [t for t in range(q, q + MIN, MIN // v) if t - p < MIN and t < x.size]


def plateau(x: np.ndarray, q0: int, n: int, bg: int = 1) -> int:
    """``D = d << 16`` (d = MIN - n) on ``[q0, q0 + n - 1]`` of a background
    of ones; ``D[q0 - 1] = d << 16 | 1`` is higher.  Returns the value."""
    d = MIN - n
    p = q0 - d
    assert bg == 1 and 1 <= n < MIN and p >= 0 and x[p] == bg and x[q0] == bg
    x[p] = bg + 1
    x[q0] = bg - 1
    return d << 16


def periodic(n: int, period: int, seed: int) -> np.ndarray:
    return np.tile(O.random_bytes(period, seed), n // period + 1)[:n].copy()


# ---------------------------------------------------------- reference side --
class Range:
    """The candidate range of the chunk starting at s, read off D alone.
    ``origin``: file offset of the arena's byte 0 (segmented path), which the
    4,096-position slices are relative to."""

    def __init__(self, D: np.ndarray, s: int, N: int, origin: int = 0):
        self.D, self.s, self.N, self.origin = D, s, N, origin
        self.L = min(MAX, N - s)
        self.none = self.L <= 2 * MIN
        if self.none:
            self.cut, self.src = s + self.L, NONE
            return
        self.qa, self.qb = s + MIN - 1, s + self.L - 1
        self.ja, self.jb = self.slice_of(self.qa), self.slice_of(self.qb)
        seg = D[self.qa:self.qb + 1]
        self.max = int(seg.max())
        self.tied = self.qa + np.flatnonzero(seg == self.max)  # every position holding the maximum
        self.win = int(self.tied[-1])
        self.cut = self.win + 1
        j = self.slice_of(self.win)
        self.src = FIRST if j == self.ja else LAST if j == self.jb else INTERIOR

    def slice_of(self, q):
        return (q - self.origin) >> SLICE_SHIFT

    def pos_of(self, q):
        return (q - self.origin) & (SLICE - 1)

    def source_of(self, q):
        j = self.slice_of(q)
        return FIRST if j == self.ja else LAST if j == self.jb else INTERIOR

    def lane_load(self, q):
        """Which lane and which of its 32 loads holds q's interior slice in K2."""
        i = self.slice_of(q) - self.ja - 1
        return i % 64, i // 64


def classify(D: np.ndarray, s: int, N: int, origin: int = 0):
    """(reference cut, K2 source the answer lies in) of the chunk starting at s."""
    r = Range(D, s, N, origin)
    return r.cut, r.src


def chain(x: np.ndarray):
    """Walk the file with ``classify``: [(start, cut, source)]."""
    D = O.digest_all(x)
    out, s = [], 0
    while s < x.size:
        cut, src = classify(D, s, x.size)
        out.append((s, cut, src))
        s = cut
    return out


# ----------------------------------------------------------------- cases ----
# name; bullets it stands for; bytes (a function: built on demand); the cut
# ends it is designed to produce; the chunks designed (indices); check(Range
# of each designed chunk ...) asserts the property on D
Case = namedtuple("Case", "name bullets n build cuts subjects check")
CASES = []

C1 = 66770               # the designed first cut: every second chunk starts unaligned
QA = C1 + MIN - 1        # = 132,305: slice 32, position 1,233
N4 = 4 * MIN - 1500      # qb = 260,643: slice 63, position 2,595
N5 = 5 * MIN - 1500
NBIG = C1 + MAX + 3000   # second chunk has L = MAX and the file continues
QBX = C1 + MAX - 1       # its qb: slice 2,064, position 1,233
VTOP = 235               # the first chunk's winner: above every other marker


def _add(name, bullets, n, build, cuts, check, subjects=(1,)):
    assert all(b in BULLETS for b in bullets), bullets
    assert not any(c.name == name for c in CASES), name
    cuts = tuple(int(c) for c in cuts)
    assert list(cuts) == sorted(set(cuts)) and cuts[-1] == n, (name, cuts)
    CASES.append(Case(name, tuple(bullets), n, build, cuts, tuple(subjects), check))


def _std(name, bullets, peaks, cuts, check, n=N4, more=None, subjects=(1,)):
    """Zeros; a first chunk cut at C1 by a VTOP marker; then ``peaks``."""
    def build():
        x = np.zeros(n, np.uint8)
        marker(x, C1 - 1, VTOP)
        for q, v in peaks:
            marker(x, q, v)
        if more:
            more(x)
        return x
    _add(name, bullets, n, build, (C1,) + tuple(cuts), check, subjects)


def _ends(win, n):
    return (win + 1,) if win + 1 == n else (win + 1, n)


def _unique(name, bullet, q, n=N4, also=None):
    def check(r):
        assert r.tied.size == 1 and r.win == q and r.max == peak(1)
        if also:
            assert also(r), name
    assert n - (q + 1) <= 2 * MIN
    _std(name, [bullet], [(q, 1)], _ends(q, n), check, n)


_unique("u_qa", "unique: qa", QA, also=lambda r: r.win == r.qa and r.src == FIRST)
_unique("u_qa+1", "unique: qa+1", QA + 1, also=lambda r: r.win == r.qa + 1)
_unique("u_qb-1", "unique: qb-1", N4 - 2, also=lambda r: r.win == r.qb - 1 and r.src == LAST)
_unique("u_qb", "unique: qb", N4 - 1, also=lambda r: r.win == r.qb and r.cut == r.s + r.L)
_unique("u_slice_pos_0", "unique: slice position 0", 40 << 12, also=lambda r: r.pos_of(r.win) == 0)
_unique("u_slice_pos_4095", "unique: slice position 4095", (40 << 12) + 4095,
        also=lambda r: r.pos_of(r.win) == 4095)
for _r in (0, 31, 32, 63):
    _unique("u_run_residue_%d" % _r, "unique: run residue %d" % _r, 169984 + _r,
            also=lambda r, _r=_r: r.win % 64 == _r and r.src == INTERIOR)
# K1 walks a file in 64 KiB iterations, a tile of t iterations per workgroup:
# the rollsum state crosses an iteration inside a tile, and is primed anew at
# a tile's first position
_unique("u_iter_last", "unique: iteration last", 4 * MIN - 1, N5, also=lambda r: r.win % MIN == MIN - 1)
_unique("u_iter_first", "unique: iteration first", 4 * MIN, N5, also=lambda r: r.win % MIN == 0)
_unique("u_tile3_last", "unique: tile of 3 last", 3 * MIN - 1, also=lambda r: r.win % (3 * MIN) == 3 * MIN - 1)
_unique("u_tile3_first", "unique: tile of 3 first", 3 * MIN, also=lambda r: r.win % (3 * MIN) == 0)
_unique("u_tile16_last", "unique: iteration last", 16 * MIN - 1, 16 * MIN + 100000,
        also=lambda r: r.win % (16 * MIN) == 16 * MIN - 1)
_unique("u_tile16_first", "unique: iteration first", 16 * MIN, 16 * MIN + 100000,
        also=lambda r: r.win % (16 * MIN) == 0)
for _n, _what, _ok in ((N4, "mid-slice", N4 % 16 != 0), (260624, "16", 260624 % 16 == 0 and 260624 % 32 != 0),
                       (260672, "64", 260672 % 64 == 0 and 260672 % 128 != 0), (63 * SLICE, "4096", True)):
    assert _ok
    for _back in (1, 2):
        _unique("u_end_%s_N-%d" % (_what, _back), "unique: N-%d, end %s" % (_back, _what), _n - _back, _n,
                also=lambda r, _back=_back: r.win == r.N - _back and r.src == LAST)

# the narrowest range, N - s = 2 MIN + 1, and one byte less: no candidate
NNARROW = C1 + 2 * MIN + 1
for _name, _q in (("qa", QA), ("qb", NNARROW - 1), ("middle", QA + MIN // 2)):
    _unique("narrow_" + _name, "narrowest: " + _name, _q, NNARROW,
            also=lambda r: r.L == 2 * MIN + 1 and r.qb - r.qa == MIN + 1)


def _check_none(r):
    assert r.none and r.L == 2 * MIN and r.cut == r.N
    assert int(r.D[r.s + MIN - 1:].max()) == peak(1)  # a peak a candidate range would have taken


_std("narrow_none", ["narrowest: no candidate"], [(QA + 30000, 1)], (C1 + 2 * MIN,), _check_none, C1 + 2 * MIN)


# a slice summary that overstates the in-range maximum of an edge slice
def _overstated(name, bullet, out, win, n, cuts, same):
    (qo, vo), (qw, vw) = out, win

    def check(r):
        edge = r.ja if qo < r.qa else r.jb
        assert qo in (r.qa - 1, r.qb + 1) and r.slice_of(qo) == edge  # outside the range, inside the edge slice
        assert int(r.D[qo]) == peak(vo) > r.max == peak(vw)
        assert r.tied.size == 1 and r.win == qw and r.cut != r.s + r.L
        assert (r.slice_of(qw) == edge) == same
    _std(name, [bullet], [out, win], cuts, check, n)


_overstated("ov_first_elsewhere", "overstated: qa-1, winner elsewhere", (QA - 1, 3), (QA + MIN + 500, 1), N4,
            _ends(QA + MIN + 500, N4), False)
_overstated("ov_first_same_slice", "overstated: qa-1, winner in the same slice", (QA - 1, 157), (QA + 1699, 151), N4,
            _ends(QA + 1699, N4), True)
# (the chunk after the winner takes the qb+1 peak: cut QBX + 2)
_overstated("ov_last_elsewhere", "overstated: qb+1, winner elsewhere", (QBX + 1, 7), (QA + 3 * MIN + 77, 1), NBIG,
            (QA + 3 * MIN + 78, QBX + 2, NBIG), False)
_overstated("ov_last_same_slice", "overstated: qb+1, winner in the same slice", (QBX + 1, 217), (QBX - 599, 99), NBIG,
            (QBX - 598, NBIG), True)


# ties between K2's three sources
def _sources(name, bullet, peaks, want_src, n, cuts, tied_srcs, more=None, value=1):
    def check(r):
        assert r.max == peak(value) and r.src == want_src and r.cut == cuts[0]
        assert [r.source_of(int(q)) for q in r.tied] == tied_srcs
        assert r.cut != r.s + r.L
    _std(name, [bullet], peaks, cuts, check, n, more)


_FE, _IN, _LA4, _LA5 = QA + 100, QA + 100 + MIN + 10, N4 - 51, N5 - 51
_sources("tie_first_interior", "sources: first = interior", [(_FE, 1), (_IN, 1)], INTERIOR, N4, _ends(_IN, N4),
         [FIRST, INTERIOR])
_sources("tie_first_last", "sources: first = last", [(_FE, 1), (_LA4, 1)], LAST, N4, _ends(_LA4, N4), [FIRST, LAST])
_sources("tie_interior_last", "sources: interior = last", [(QA + 5000, 1), (_LA4, 1)], LAST, N4, _ends(_LA4, N4),
         [INTERIOR, LAST])
_sources("tie_all_three", "sources: first = last", [(_FE, 1), (_IN, 1), (_LA5, 1)], LAST, N5, _ends(_LA5, N5),
         [FIRST, INTERIOR, LAST])
# first edge 0xFFFF0003 against 0xFFFF0001 in an interior and in the last edge
# slice; the chunk after it sees those two tied
_sources("first_greater_by_v", "sources: first greater by v only", [(_FE, 3), (_IN, 1), (_LA5, 1)], FIRST, N5,
         (_FE + 1, _LA5 + 1, N5), [FIRST], value=3)

# first edge 0xFFFF0063 against a comb of two, 0xFFFE0002 in an interior and in
# the last edge slice
_NSTRICT = QA + 40000 + MIN // 2 + 31


def _check_strict(r):
    assert r.max == peak(99) and r.src == FIRST and r.tied.size == 1
    rest = r.D[r.win + 1:r.qb + 1]
    top = np.flatnonzero(rest == rest.max()) + r.win + 1
    assert int(rest.max()) == 0xFFFE0002 and [r.source_of(int(q)) for q in top] == [INTERIOR, LAST]
    assert r.cut != r.s + r.L


_std("first_strictly_greater", ["sources: first strictly greater"], [(_FE, 99)], (_FE + 1, _NSTRICT), _check_strict,
     _NSTRICT, more=lambda x: comb(x, QA + 40000, 2))


# ties among the interior slices of one 8 MiB range: slice ja+1+i is held by
# lane i % 64 as its load i / 64
def _interior(name, bullet, idxs, ok):
    qs = [((QA >> SLICE_SHIFT) + 1 + i << SLICE_SHIFT) + 777 for i in idxs]
    n = C1 + MAX

    def check(r):
        assert r.L == MAX and r.max == peak(1) and list(r.tied) == qs and r.src == INTERIOR
        ll = [r.lane_load(q) for q in qs]
        assert [64 * ld + ln for ln, ld in ll] == list(idxs) and ok(ll), ll
        assert r.cut != r.s + r.L
    _std(name, [bullet], [(q, 1) for q in qs], (qs[-1] + 1, n), check, n)


_interior("il_same_lane", "interior: same lane, different loads", (5, 5 + 64 * 3),
          lambda ll: ll[0][0] == ll[1][0] and ll[0][1] < ll[1][1])
_interior("il_same_load", "interior: same load, different lanes", (64 * 2 + 7, 64 * 2 + 40),
          lambda ll: ll[0][1] == ll[1][1] and ll[0][0] < ll[1][0])
_interior("il_earlier_higher_lane", "interior: earlier in higher lane and lower load", (64 + 50, 64 * 4 + 3),
          lambda ll: ll[0][0] > ll[1][0] and ll[0][1] < ll[1][1])
_interior("il_earlier_lower_lane", "interior: earlier in lower lane and lower load", (64 + 3, 64 * 4 + 50),
          lambda ll: ll[0][0] < ll[1][0] and ll[0][1] < ll[1][1])
_interior("il_fourteen", "interior: three or more",
          (10, 74, 300, 481, 700, 905, 1100, 1290, 1500, 1699, 1800, 1930, 1990, 2030),
          lambda ll: len(ll) == 14 and ll[0][0] == ll[1][0] and ll[-1] == (46, 31))

# ties inside a slice: plateaus from qa on a background of ones (the first
# chunk is cut at C1 by a +1 marker, 0xFFFF0001, above any plateau)
NPLAT = C1 + 3 * MIN - 2000


def _plateau(name, bullets, length, ok):
    def build():
        x = np.ones(NPLAT, np.uint8)
        marker(x, C1 - 1, 1, bg=1)
        plateau(x, QA, length)
        return x

    def check(r):
        val = (MIN - length) << 16
        assert r.max == val and list(r.tied) == list(range(r.qa, r.qa + length))
        assert int(r.D[r.qa - 1]) == val | 1  # just outside, higher, in the same slice
        assert r.slice_of(r.qa - 1) == r.ja and ok(r) and r.cut != r.s + r.L
    _add(name, bullets, NPLAT, build, (C1, QA + length, NPLAT), check)


_plateau("plateau_in_first_edge", ["in-slice: plateau ends in the first edge slice"], 1000,
         lambda r: r.src == FIRST and r.pos_of(r.win) == 2232)
_plateau("plateau_to_4095", ["in-slice: plateau ends at position 4095"], 2863,
         lambda r: r.src == FIRST and r.pos_of(r.win) == 4095)
_plateau("plateau_to_next_0", ["in-slice: plateau ends at position 0 of the next slice"], 2864,
         lambda r: r.src == INTERIOR and r.pos_of(r.win) == 0 and r.slice_of(r.win) == r.ja + 1)
_plateau("plateau_six_slices", ["in-slice: plateau over several slices"], 2864 + 5 * SLICE + 321,
         lambda r: r.slice_of(r.win) == r.ja + 6 and r.max >= HALF)
_plateau("plateau_below_half", ["sign: all below 0x80000000", "in-slice: plateau over several slices"], 40000,
         lambda r: r.max < HALF and int(r.D[r.qa:r.qb + 1].max()) < HALF and r.slice_of(r.win) == r.ja + 10)


def _check_straddle(r):
    seg = r.D[r.qa:r.qb + 1]
    assert r.max == peak(5) and r.tied.size == 1 and (seg >= HALF).sum() > 1000 and (seg < HALF).sum() > 1000


_std("sign_straddle", ["sign: straddles 0x80000000"], [(QA + 20000, 5)], _ends(QA + 20000, N4), _check_straddle)


# combs: eight tied positions per slice over 16 slices; one per slice at the
# same position in the first edge slice and the 15 after it; and a comb across
# qb, whose out-of-range teeth tie the winner inside the last edge slice
def _comb_case(name, bullets, q0, v, n, cuts, ok):
    def check(r):
        assert r.max == (0x10000 - v) << 16 | v and r.tied.size >= 2 and ok(r) and r.cut != r.s + r.L
    _std(name, bullets, [], cuts, check, n, more=lambda x: comb(x, q0, v))


_comb_case("comb_8_per_slice", ["in-slice: short period"], QA + 300, 128, N4, _ends(QA + 300 + 127 * 512, N4),
           lambda r: r.tied.size == 128 and (np.diff(r.tied) == 512).all() and r.src == INTERIOR)
_comb_case("comb_column_first_to_interior", ["sources: first = interior"], QA + 50, 16, N4,
           _ends(QA + 50 + 15 * SLICE, N4),
           lambda r: r.tied.size == 16 and (np.diff(r.tied) == SLICE).all() and r.source_of(int(r.tied[0])) == FIRST
           and r.src == INTERIOR)
_comb_case("comb_across_qb", ["overstated: qb+1, winner in the same slice"], QBX - 200 - 100 * 512, 128, NBIG,
           (QBX - 199, NBIG),
           lambda r: r.src == LAST and r.win == r.qb - 200 and int(r.D[r.qb + 312]) == r.max
           and r.slice_of(r.qb + 312) == r.jb)


# short periods: D has the tile's period from q = MIN - 1 on, so the cut is the
# last position of the range at a phase holding the period's maximum
def _periodic_cuts(period, seed, n):
    tile = O.random_bytes(period, seed)
    Dp = O.digest_all(np.tile(tile, (MIN + 2 * period) // period + 1))[MIN - 1:MIN - 1 + period]
    phases = np.flatnonzero(Dp == Dp.max())  # D[q] is the maximum iff (q - (MIN-1)) % period is one of these
    cuts, s = [], 0
    while s < n:
        L = min(MAX, n - s)
        if L <= 2 * MIN:
            cuts.append(s + L)
        else:
            qb = s + L - 1
            back = min((qb - (MIN - 1) - int(ph)) % period for ph in phases)
            assert qb - back >= s + MIN - 1
            cuts.append(qb - back + 1)
        s = cuts[-1]
    return cuts


def _periodic(period):
    n, seed = N4, 100 + period

    def check(*rs):
        for r in rs:
            if not r.none:  # one tie per period at least, the last of them the winner
                assert r.tied.size >= (r.qb - r.qa + 1) // period >= 1 and (np.diff(r.tied) <= period).all()
                assert r.qb - r.win < period
        assert not rs[0].none and (period > SLICE // 2 or (rs[0].tied >> SLICE_SHIFT == rs[0].win >> SLICE_SHIFT).sum() > 1)
    cuts = _periodic_cuts(period, seed, n)
    _add("period_%d" % period, ["in-slice: short period"], n, lambda: periodic(n, period, seed), cuts, check,
         subjects=range(len(cuts)))


for _p in (1, 2, 3, 64, 1000, 4095, 4097):
    _periodic(_p)

# markers of falling value whose k falls too: in file order their bytes are
# at least as far apart as their peaks, and each chunk's winner is above
# everything after it
LADDER = (193, 169, 167, 163, 145, 141, 135, 133, 109, 103, 91, 89, 81, 67, 53, 49, 39, 31)
assert all(a > b and k_of(a) > k_of(b) for a, b in zip(LADDER, LADDER[1:]))


def _chain_zero():
    """Six chunks: cut at c1; first = interior tie; a peak at qa-1 with the
    winner interior; the winner at qa; interior = last tie; the tail."""
    v = LADDER
    c1 = 70001
    qa1 = c1 + MIN - 1
    peaks = [(c1 - 1, v[0]), (qa1 + 100, v[1]), (qa1 + 100 + MIN + 10, v[1])]
    c2 = peaks[-1][0] + 1
    qa2 = c2 + MIN - 1
    peaks += [(qa2 - 1, v[2]), (qa2 + MIN + 500, v[3])]
    c3 = peaks[-1][0] + 1
    peaks += [(c3 + MIN - 1, v[4])]
    c4 = c3 + MIN
    qa4 = c4 + MIN - 1
    peaks += [(qa4 + 5000, v[5]), (qa4 + 5000 + MIN + 3000, v[5])]
    c5 = peaks[-1][0] + 1
    n = c5 + 50

    def build():
        x = np.zeros(n, np.uint8)
        for q, val in peaks:
            marker(x, q, val)
        return x

    def check(r0, r1, r2, r3, r4):
        assert r0.s == 0 and r0.tied.size == 1
        assert [r.source_of(int(q)) for r in (r1,) for q in r.tied] == [FIRST, INTERIOR]
        assert int(r2.D[r2.qa - 1]) == peak(v[2]) > r2.max == peak(v[3]) and r2.src == INTERIOR
        assert r3.win == r3.qa and r3.max == peak(v[4])
        assert [r4.source_of(int(q)) for q in r4.tied] == [INTERIOR, LAST] and r4.max == peak(v[5])
        assert all(r.s % 16 for r in (r1, r2, r3, r4))
    _add("chain_zero_six", ["chain"], n, build, (c1, c2, c3, c4, c5, n), check, subjects=(0, 1, 2, 3, 4))


_chain_zero()


def _chain_ones():
    """Five chunks on ones: cut at C1, then four plateaus of growing length,
    each starting at the qa the one before it designed."""
    lengths = (700, 2864 + SLICE, 12000, 40000)
    starts, s = [], C1
    for ln in lengths:
        starts.append(s + MIN - 1)
        s = s + MIN - 1 + ln
    n = s + 40000  # the last plateau's chunk is longer than 2 MIN, the tail is not

    def build():
        x = np.ones(n, np.uint8)
        marker(x, C1 - 1, 1, bg=1)
        for q0, ln in zip(starts, lengths):
            plateau(x, q0, ln)
        return x

    def check(*rs):
        for r, ln in zip(rs, lengths):
            assert r.max == (MIN - ln) << 16 and list(r.tied) == list(range(r.qa, r.qa + ln)) and r.s % 16
        assert rs[0].src == FIRST and rs[1].pos_of(rs[1].win) != 0 and rs[3].max < HALF
    cuts = [C1] + [q0 + ln for q0, ln in zip(starts, lengths)] + [n]
    _add("chain_ones_plateaus", ["chain"], n, build, cuts, check, subjects=(1, 2, 3, 4))


_chain_ones()


def _chain_big():
    """Four designed chunks across 19 MiB: cut at c1 = 5 MiB + 124; L = MAX
    with a peak at qb+1 and the winner interior; the chunk after it takes
    that peak; then two interior slices tied in one lane, 5 loads apart."""
    v = LADDER
    c1 = 5 * Mi + 124
    qb1 = c1 + MAX - 1
    w1 = c1 + 3 * Mi + 333
    c3 = qb1 + 2
    ja3 = (c3 + MIN - 1) >> SLICE_SHIFT
    t1, t2 = (ja3 + 1 + 9 << SLICE_SHIFT) + 4095, (ja3 + 1 + 9 + 64 * 5 << SLICE_SHIFT)
    n = c3 + 6 * Mi + 17
    peaks = [(c1 - 1, v[0]), (w1, v[2]), (qb1 + 1, v[1]), (t1, v[3]), (t2, v[3])]

    def build():
        x = np.zeros(n, np.uint8)
        for q, val in peaks:
            marker(x, q, val)
        return x

    def check(r0, r1, r2, r3):
        assert r0.win == c1 - 1 and r0.L == MAX
        assert r1.L == MAX and int(r1.D[r1.qb + 1]) == peak(v[1]) > r1.max == peak(v[2]) and r1.src == INTERIOR
        assert r1.slice_of(r1.qb + 1) == r1.jb
        assert r2.win == qb1 + 1 and r2.tied.size == 1
        assert list(r3.tied) == [t1, t2] and r3.lane_load(t1) == (9, 0) and r3.lane_load(t2) == (9, 5)
        assert all(r.s % 16 for r in (r1, r2, r3))
    _add("chain_big_four", ["chain"], n, build, (c1, w1 + 1, c3, t2 + 1, n), check, subjects=(0, 1, 2, 3))


_chain_big()

BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _built(name):
    x = BY_NAME[name].build()
    x.flags.writeable = False
    return x


def build(name: str) -> np.ndarray:
    """The case's bytes (read-only, kept: 99 MiB for the whole list)."""
    return _built(name)


# ------------------------------------------------------- segmented inputs ---
# Zero-background files for 16 MiB segments (segment k holds file bytes
# [8 MiB k, 8 MiB k + 16 MiB)): name -> (bytes, builder, designed cuts).  The
# per-segment counts are the model's, and what each file achieves is asserted
# there too (tests/test_segmented.py).
def _seg_file(n, peaks):
    def build():
        x = np.zeros(n, np.uint8)
        for q, v in peaks:
            marker(x, q, v)
        return x
    return build


# chunk 1 starts at exactly len - MAX of segment 0 (continue), has L = MAX and
# a peak at qb+1 = 16 MiB, the first byte segment 0 does not hold; chunk 3
# starts one past len - MAX of segment 1 (stop and carry) and is resumed at
# arena byte 1 of segment 2, its winner at qa = arena position MIN
_XA = 24 * Mi + 3 * MIN
_SEG_EXACT = (_XA, _seg_file(_XA, [(8 * Mi - 1, 3), (12 * Mi + 777, 1), (16 * Mi, 7), (16 * Mi + MIN, 5),
                                   (20 * Mi + 100, 1)]),
              (8 * Mi, 12 * Mi + 778, 16 * Mi + 1, 16 * Mi + MIN + 1, 20 * Mi + 101, _XA))
# resumed chunks whose winners sit at arena-relative slice positions 0 and 4095
_XB = 26 * Mi + 5
_SEG_SLICE = (_XB, _seg_file(_XB, [(5 * Mi + 123, 1), (10 * Mi + 4097, 1), (14 * Mi, 5), (18 * Mi + 500, 3),
                                   (21 * Mi + 4095, 1)]),
              (5 * Mi + 124, 10 * Mi + 4098, 14 * Mi + 1, 18 * Mi + 501, 21 * Mi + 4096, _XB))
# the same at segments of 16 MiB + 48: arena slices no longer line up with the
# file's, so the winners are placed by arena position (segment k at k (8 MiB + 48))
_XC = 26 * Mi + 5
_OFF1, _OFF2 = 8 * Mi + 48, 16 * Mi + 96
_SEG_SKEW = (_XC, _seg_file(_XC, [(5 * Mi + 123, 1), (10 * Mi + 4097, 1), (_OFF1 + 6 * Mi, 5), (18 * Mi + 500, 3),
                                  (_OFF2 + 5 * Mi + 4095, 1)]),
             (5 * Mi + 124, 10 * Mi + 4098, _OFF1 + 6 * Mi + 1, 18 * Mi + 501, _OFF2 + 5 * Mi + 4096, _XC))
SEG_FILES = {"craft_exact": _SEG_EXACT, "craft_slice": _SEG_SLICE, "craft_skew": _SEG_SKEW}
