"""The crafted cut-rule inputs (tests/cut_craft.py) against the CPU oracle.

For every case the closed-form oracle, the literal loop (store.go:141-165),
``cut_craft.chain`` (the rule restated on ``digest_all``) and the cuts the
case was designed for are the same; on the cases up to 4 MIN the pure-Python
transliteration agrees too.  Each case's stated property is asserted on
``digest_all`` alone, and the list as a whole must reach each of K2's three
sources and every bullet of the case list: what the GPU tests
(test_gpu_cut_crafted.py) then run is known to exercise the tie rules and
the bounded edge re-scans, not assumed to.
"""
import collections

import numpy as np
import pytest

from . import cut_craft as cc

NAMES = [c.name for c in cc.CASES]


@pytest.fixture(scope="module")
def table(oracle):
    """name -> (chain from digest_all, Range of every chunk), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            x = cc.build(name)
            D = oracle.digest_all(x)
            ch, s = [], 0
            while s < x.size:
                r = cc.Range(D, s, x.size)
                ch.append(r)
                s = r.cut
            cache[name] = ch
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_oracle_chain_and_design_agree(oracle, table, name):
    case = cc.BY_NAME[name]
    x = cc.build(name)
    assert x.size == case.n
    ranges = table(name)
    cuts = [r.cut for r in ranges]
    assert cuts == list(case.cuts), "classify's chain is not the designed one"
    assert [(r.s, r.cut, r.src) for r in ranges] == cc.chain(x)
    fast = oracle.store_file(x, fast=True)
    assert [int(c) for c in fast.cut_ends] == cuts
    lit = oracle.store_file(x, fast=False)
    assert np.array_equal(lit.cut_ends, fast.cut_ends) and np.array_equal(lit.ids, fast.ids)
    assert (lit.content_type, lit.content_id) == (fast.content_type, fast.content_id)


@pytest.mark.parametrize("name", [c.name for c in cc.CASES if c.n <= 4 * cc.MIN])
def test_python_literal_loop_agrees(oracle, name):
    x = cc.build(name)
    cuts, ids, ctype, cid = oracle.py_store_file_literal(x.tobytes())
    ref = oracle.store_file(x, fast=True)
    assert cuts == [int(c) for c in ref.cut_ends] == list(cc.BY_NAME[name].cuts)
    assert ids == [i.tobytes() for i in ref.ids] and (ctype, cid) == (ref.content_type, ref.content_id)


@pytest.mark.parametrize("name", NAMES)
def test_stated_property_holds_on_the_digests(table, name):
    case = cc.BY_NAME[name]
    ranges = table(name)
    case.check(*[ranges[i] for i in case.subjects])
    # a chunk after the first starts where a designed cut put it: unaligned
    # (the periodic files' cuts fall where their random tiles put them)
    for i in case.subjects:
        if i and not name.startswith("period_"):
            assert ranges[i].s % 16, (name, i)


def designed_chunks(table):
    for c in cc.CASES:
        ranges = table(c.name)
        for i in c.subjects:
            yield c, i, ranges[i]


def test_every_bullet_has_a_case():
    have = collections.Counter(b for c in cc.CASES for b in c.bullets)
    assert [b for b in cc.BULLETS if not have[b]] == []


def test_each_source_decides_at_least_five_chunks(table):
    n = collections.Counter(r.src for _, _, r in designed_chunks(table))
    assert all(n[src] >= 5 for src in cc.SOURCES), n
    assert n[cc.NONE] >= 1


def test_clamp_cannot_hide_a_wrong_edge_or_tie(table):
    """A cut outside [s+MIN, s+L] becomes s+L in K2: no overstated-edge or tie
    case may have s+L as its answer (but a tie whose designed winner is qb)."""
    seen = 0
    for c, i, r in designed_chunks(table):
        if r.none or not any(b.startswith(("overstated", "sources", "interior", "in-slice")) for b in c.bullets):
            continue
        if c.name.startswith("period_") and r.win == r.qb:
            continue
        assert r.cut != r.s + r.L, (c.name, i)
        seen += 1
    assert seen >= 25


def test_sizes_stay_small():
    assert sum(c.n for c in cc.CASES) < 200 * cc.Mi
    assert sum(1 for c in cc.CASES if c.n > cc.Mi + cc.MAX // 8) <= 12


def test_marker_offsets_are_found_by_search(oracle):
    """k(v) of the issue's table, and the closed form behind it, on the oracle."""
    assert [cc.k_of(v) for v in (1, 3, 5, 7)] == [32766, 54612, 45874, 4680]
    x = np.zeros(3 * cc.MIN, np.uint8)
    q = cc.MIN - 1 + 5000
    p = cc.marker(x, q, 7)
    D = oracle.digest_all(x)
    assert (p, int(D[q]), int(D[q - 1])) == (q - 4680, 0xFFFF0007, 0xFFF80007) and int(D[q + 1]) < 0x10000000
    assert int(D.max()) == 0xFFFF0007 and (D == D.max()).sum() == 1
    assert [int(c) for c in oracle.store_file(x, fast=True).cut_ends] == [q + 1, 3 * cc.MIN]
    y = np.ones(3 * cc.MIN, np.uint8)
    val = cc.plateau(y, 65535, 4096)
    D = oracle.digest_all(y)
    assert val == 61440 << 16 and (D[65535:69631] == val).all() and int(D[69631]) < val
    assert [int(c) for c in oracle.store_file(y, fast=True).cut_ends] == [69631, 3 * cc.MIN]
    y = np.ones(3 * cc.MIN, np.uint8)
    val = cc.plateau(y, 100000, 4096)  # with whole windows before it: the position before a plateau is higher
    D = oracle.digest_all(y)
    assert (D[100000:104096] == val).all() and int(D[99999]) == val | 1 == int(D[65535:].max())


def summary(table):
    """Chunks per K2 source and per bullet, as the pull request reports them."""
    src, bul = collections.Counter(), collections.Counter()
    for c, _, r in designed_chunks(table):
        src[r.src] += 1
        for b in c.bullets:
            bul[b] += 1
    return src, bul
