"""CPU checks of the crafted MD5 chains (tests/md5_craft.py): the arenas are
what they claim (filler everywhere, blocks apart), the reference agrees with
the oracle, and the path model says that the families reach every lane class
tests/test_gpu_md5_crafted.py relies on, as explicit sets."""
import itertools

import numpy as np
import pytest

from . import md5_craft as mc


@pytest.fixture(scope="module")
def fam():
    return {"A": mc.family_a(), "B": mc.family_b(), "C": mc.family_c()}


def test_reference_is_the_oracles_block_id(oracle, fam):
    rng = np.random.default_rng(5)
    for L, n in [(0, 0), (0, 5), (1, 0), (3, 55), (4, 56), (9, 1000), (2, 70000)]:
        d = rng.integers(0, 256, n, dtype=np.uint8)
        links = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(L)]
        assert mc.ref_id(d.tobytes(), links) == oracle.block_id(d, links)
    assert mc.ref_id(b"hello").hex() == "9e06002f060f42397d3862c8777fb39b"
    c = fam["C"]
    for i in range(0, len(c.specs), 97):
        assert c.ref()[i] == oracle.block_id(c.data(i), c.links[i])


@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_arena_is_filler_with_blocks_apart(fam, name):
    if name == "E":
        host, offs, lens = mc.family_e(fam["B"])
        assert all(int(o) % 16 == 0 and int(o) % 64 != 0 for o in offs)
    else:
        cs = fam[name]
        host, offs, lens = cs.host, cs.offs, cs.lens
        assert [int(o) % 64 for o in offs] == [s.amod for s in cs.specs]
    offs, lens = offs.astype(np.int64), lens.astype(np.int64)
    order = np.argsort(offs)
    starts, ends = offs[order], offs[order] + lens[order]
    assert starts[0] >= 128
    assert (starts[1:] - ends[:-1] >= 128).all(), "blocks overlap or lie closer than 128 bytes"
    assert host.size - ends[-1] >= mc.ARENA_SLACK + 64
    inside = np.zeros(host.size, bool)
    for s, e in zip(starts, ends):
        inside[s:e] = True
    fill = host[~inside]
    assert fill.size and (fill != 0).all() and (fill != 0x80).all()
    # the filler is not the block data: the bytes on both sides of a block's
    # end differ from what a correct message holds there (0x80, then zeros)
    assert (host[ends] != 0x80).all() and (host[ends] != 0).all()
    assert host.size < (8 << 20)


def test_chain_path_restates_the_framing():
    for L, n in itertools.product(range(6), range(0, 400)):
        c = mc.chain_path(L, n)
        msg_blocks = (c.T + 9 + 63) // 64           # RFC 1321 padding
        assert c.full + c.tails == msg_blocks
        assert c.fast == (64 * c.hb <= c.T - c.residue)
        if c.fast:                                   # the streaming path starts inside the data
            assert 64 * c.hb >= c.p and c.k6_cnt == c.full - c.hb
        assert (c.k3_left is None) == (L > 0 and not c.fast)
        for door in ("k3", "k6"):
            cnt = c.k3_left if door == "k3" else (c.k6_cnt if c.fast else None)
            if cnt is not None:
                assert mc.length_for(L, cnt, c.residue, door) == n
    assert [mc.slice_cnt(x, 9) for x in (0, 1, 9, 10, 18, 19, 27)] == [0, 1, 9, 1, 9, 1, 9]
    assert mc.launch_counts(40, 9) == [4, 9, 9, 9, 9] and mc.launch_counts(64, 64) == [64]
    assert mc.launch_counts(7, mc.BUDGET_ALL) == [7]


def test_family_a_lane_path_classes(fam):
    a = fam["A"]
    assert len(a.specs) == 5 * 192 * 16
    p = a.paths
    assert {c.p for c in p} == {8, 24, 40, 56, 72}
    assert {s.amod % 16 for s in a.specs} == set(range(16))
    assert {c.full for c in p} == {0, 1, 2, 3, 4} and {c.tails for c in p} == {1, 2}
    assert {c.fast for c in p} == {True, False}
    # K6: sorted by length, every wave stays on the lane path
    for w in mc.k6_waves(a.lens):
        assert mc.k6_wave([p[i].k6_cnt for i in w]).Rc == 0
    assert mc.k3_wave(a.k3_counts(a.groups["all"])).coop is False
    # every (sh, residue) on the lane path, for a fast chain (md5_tail with
    # msg_word's 0..3-byte mask) and with both tail-block counts
    fast = {(s.amod & 3, c.residue) for s, c in zip(a.specs, p) if c.fast}
    assert fast == set(itertools.product(range(4), range(64)))
    assert {(s.amod & 3, c.residue & 3, c.tails) for s, c in zip(a.specs, p) if c.fast} == \
        set(itertools.product(range(4), range(4), (1, 2)))
    # md5_run from block 0 (`b0 == 0`, any_first) at every sh: L == 0 chains with full blocks
    assert {s.amod & 3 for s, c in zip(a.specs, p) if s.L == 0 and c.full} == {0, 1, 2, 3}


def test_family_b_uniform_waves(fam):
    b = fam["B"]
    p = b.paths
    assert len(b.specs) == 3 * 28 * 64
    coop_pairs, lane_pairs, s16 = set(), set(), set()
    for L in mc.B_LINKS:
        idx = b.groups["L%d" % L]
        lens = [b.specs[i].length for i in idx]
        waves = mc.k6_waves(lens)
        assert len(waves) == len(mc.B_COUNTS)
        seen = []
        for w in waves:                              # K6: a wave is a class
            cls = {b.specs[idx[i]].cls for i in w}
            cnts = {p[idx[i]].k6_cnt for i in w}
            assert len(cls) == 1 and len(cnts) == 1
            k6 = mc.k6_wave([p[idx[i]].k6_cnt for i in w])
            assert k6.Rc == (cnts.copy().pop() if min(cnts) >= 8 else 0) and k6.nmax == (0 if k6.Rc else 7)
            seen.append(min(cnts))
            assert {p[idx[i]].residue for i in w} == set(range(64))
            assert {b.specs[idx[i]].amod for i in w} == set(range(64))
            for i in w:
                s, c = b.specs[idx[i]], p[idx[i]]
                (coop_pairs if k6.Rc else lane_pairs).add((s.amod & 3, c.residue))
                if k6.Rc:                            # md5_coop: `S = c + 64 * b1 - 8`, c = data - 16 L
                    s16.add((s.amod - 16 * L + 64 * c.hb - 8) % 16)
        assert seen == list(reversed(mc.B_COUNTS))   # the 7 / 8 / 9 threshold
    assert coop_pairs == set(itertools.product(range(4), range(64)))
    assert {sh for sh, _ in lane_pairs} == {0, 1, 2, 3}
    assert s16 == set(range(16))


@pytest.mark.parametrize("budget,items", [(64, 0), (128, 2), (256, 4)])
def test_family_b_k3_groups_are_the_classes(fam, budget, items):
    """At these budgets every class falls into a bin of its own (both bin
    rules), bins run by descending count and every class holds exactly 64
    chains, so group g of the launch is class g whatever the order inside a
    bin; a K3Q part (`per_part = ceil(budget / parts)`) holds a whole slice."""
    b = fam["B"]
    for L in mc.B_LINKS:
        idx = b.groups["L%d" % L]
        assert all(b.paths[i].k3_left is not None for i in idx)
        by_cls = {}
        for i in idx:
            by_cls.setdefault(b.specs[i].cls, set()).add(mc.slice_cnt(b.paths[i].k3_left, budget))
        assert all(len(v) == 1 for v in by_cls.values())
        counts = [v.pop() for v in by_cls.values()]
        assert counts == [c + (L == 0) for c in mc.B_COUNTS] and max(counts) < budget
        for rule in (lambda c: mc.order_bin(c, budget), lambda c: mc.plan_bin(c, budget)):
            bins = [rule(c) for c in counts]
            assert len(set(bins)) == len(bins) and bins == sorted(bins, reverse=True)
        if items:
            assert max(counts) <= (budget + items - 1) // items
        assert mc.k3_need([b.paths[i] for i in idx], budget) == 1


def test_family_b_k3_stage_classes(fam):
    b = fam["B"]
    waves = []
    for L in mc.B_LINKS:
        idx = b.groups["L%d" % L]
        for g in range(len(mc.B_COUNTS)):
            waves.append(mc.k3_wave(b.k3_counts(idx[64 * g:64 * g + 64])))
    coop = [w for w in waves if w.coop]
    assert {w.R for w in waves} >= {7, 8, 9} and not all(w.coop for w in waves)
    assert {w.stages for w in coop} == set(range(2, 10))
    assert {w.coop_blocks % 4 for w in coop} == {0, 1, 2, 3}
    assert {w.last_stage for w in coop} == {1, 2, 3, 4}
    assert {w.stages % 3 for w in coop} == {0, 1, 2}          # each arm of the three-set producer
    assert {w.stages % 2 for w in coop} == {0, 1}
    assert all(not w.rounds and w.nmax == 0 for w in coop)
    # one workgroup (HBX_K3_WGS=1): MD5 wave w walks groups w, w + 4, ..; a
    # group starts in LDS half `S & 1` of the stages before it: both occur
    for L in mc.B_LINKS:
        idx = b.groups["L%d" % L]
        order = sorted(range(len(mc.B_COUNTS)), key=lambda g: -mc.B_COUNTS[g])  # descending count
        halves = set()
        for w0 in range(4):
            S = 0
            for g in order[w0::4]:
                kw = mc.k3_wave(b.k3_counts(idx[64 * g:64 * g + 64]))
                if kw.coop:
                    halves.add(S & 1)
                    S += kw.stages
        assert halves == {0, 1}


def test_family_c_mixed_groups(fam):
    c = fam["C"]
    comp = mc.c_compositions()
    waves = {}
    for L in mc.C_LINKS:
        for name, counts in comp.items():
            idx = c.groups["%s/L%d" % (name, L)]
            assert len(idx) == len(counts) <= 65
            got = c.k3_counts(idx)
            assert got == counts, (name, L)
            waves[name, L] = mc.k3_wave(got[:64])
            # residues and addresses are mixed inside a group
            if len(idx) >= 63:
                assert len({c.paths[i].residue for i in idx}) >= 56
                assert {c.specs[i].amod & 3 for i in idx} == {0, 1, 2, 3}
                assert len({c.specs[i].amod % 16 for i in idx}) == 16
    for L in mc.C_LINKS:
        w = lambda n: waves[n, L]  # noqa: E731
        assert (w("40x63+39").R, w("40x63+39").rounds, w("40x63+39").nmax) == (39, [], 1)
        assert (w("40x63+32").R, w("40x63+32").rounds, w("40x63+32").nmax) == (32, [8], 0)
        assert (w("40x63+8").R, w("40x63+8").rounds) == (8, [32])
        assert not w("40x63+7").coop and w("40x63+7").nmax == 40
        assert not w("40x63+0").coop and w("40x63+0").R == 0
        assert (w("40+9x63").R, w("40+9x63").rounds) == (9, [31])
        assert w("steps8").rounds == [8, 8, 8, 8] and sorted(set(w("steps8").run)) == [0, 8, 16, 24]
        assert w("8to15").coop and w("8to15").rounds == [] and sorted(set(w("8to15").run)) == list(range(8))
        assert w("n1").R == 40 and w("n2").rounds == [28] and w("n63").rounds == [] and w("n63").nmax == 6
        for m in mc.NMAX_EDGES:
            assert w("coop-nmax%d" % m).coop and w("coop-nmax%d" % m).rounds == []
            assert not w("lane-nmax%d" % m).coop
    allw = list(waves.values())
    assert {len(w.rounds) for w in allw} == {0, 1, 2, 3, 4}
    for L in mc.C_LINKS:
        assert waves["rounds2", L].rounds == [8, 8] and waves["rounds2", L].nmax == 0
        assert waves["rounds3", L].rounds == [8, 8, 8] and waves["rounds3", L].nmax == 0
    assert {w.nmax for w in allw if w.coop} >= set(mc.NMAX_EDGES)
    assert {w.nmax for w in allw if not w.coop} >= set(mc.NMAX_EDGES)
    # K6 on the same groups: L = 1 keeps the counts, L = 0 hashes block 0 byte by byte
    for name, counts in comp.items():
        idx = c.groups["%s/L1" % name]
        assert sorted(c.paths[i].k6_cnt for i in idx) == sorted(counts)
        idx0 = c.groups["%s/L0" % name]
        assert sorted(c.paths[i].k6_cnt for i in idx0) == sorted(max(k - 1, 0) for k in counts)


def _d_first_waves(fam):
    """Per (slice, batch): every chain's blocks per launch."""
    out = {}
    for budget in mc.D_SLICES:
        for cs, name, idx in mc.d_groups(fam["B"], fam["C"]):
            sched = [mc.launch_counts(cs.paths[i].k3_left, budget) for i in idx if cs.paths[i].k3_left is not None]
            out[budget, name] = sched
    return out


def test_family_d_slices(fam):
    d = _d_first_waves(fam)
    first, finish_in = {}, set()
    for (budget, name), sched in d.items():
        first.setdefault(budget, set()).update(s[0] for s in sched)
        finish_in.add(len({len(s) for s in sched}))
    # the remainder slice: 1 and 7 (lane path), 8 and the whole budget (cooperative)
    assert first[3] == {0, 1, 2, 3}
    for budget in (9, 12, 64):
        assert first[budget] >= {1, 7, 8, budget}, (budget, sorted(first[budget]))
    assert max(finish_in) >= 2                                  # chains of one group finish in different launches
    # and per wave: a batch of at most 64 chains is one group in its first
    # launch, whose R is the smallest first slice
    for budget in (9, 12, 64):
        waves = {(w.R, w.coop) for w in (mc.k3_wave([s[0] for s in sched]) for (b, _), sched in d.items()
                                         if b == budget and len(sched) <= 64)}
        assert waves >= {(1, False), (7, False), (8, True), (budget, True)}, (budget, sorted(waves))
    # a launch of a sliced group may be cooperative, on the lane path, or both in turn
    kinds = set()
    for (budget, name), sched in d.items():
        if len(sched) <= 64:
            kinds.add(frozenset(mc.k3_wave([s[j] for s in sched if j < len(s)]).coop
                                for j in range(max(len(s) for s in sched))))
    assert kinds == {frozenset([True]), frozenset([False]), frozenset([True, False])}


def test_k3q_parts(fam):
    """K3Q engages at the variants' budgets only, a part is 64 blocks there,
    and the parts-* groups of C cross it: part 1 on the lane path, with a
    mixed round, and with half the lanes only shadowing."""
    comp = mc.c_compositions()
    assert mc.k3q_parts([40], 64, 2) == [[40]] and mc.k3q_parts([40], mc.BUDGET_ALL, 4) == [[40]]
    for budget, items in ((128, 2), (256, 4)):
        assert max(max(c) for c in comp.values()) <= 127 < budget   # one launch hashes every group
        for name, counts in comp.items():
            parts = mc.k3q_parts(counts, budget, items)
            assert len(parts) == items and [sum(x) for x in zip(*parts)] == counts
            if not name.startswith("parts-"):
                assert parts[1:] == [[0] * len(counts)] * (items - 1)
        live = lambda part: [c for c in part if c]  # noqa: E731
        p = mc.k3q_parts(comp["parts-lane"], budget, items)
        assert set(p[0]) == {64} and sorted(set(p[1])) == [1, 6, 36, 63] and not mc.k3_wave(live(p[1])).coop
        p = mc.k3q_parts(comp["parts-coop"], budget, items)
        w = mc.k3_wave(live(p[1]))
        assert (w.R, w.rounds) == (16, [40])
        p = mc.k3q_parts(comp["parts-shadow"], budget, items)
        w0, w1 = mc.k3_wave(p[0]), mc.k3_wave(live(p[1]))
        assert (w0.R, w0.rounds) == (40, [24]) and p[1].count(0) == 32 and (w1.R, w1.coop) == (63, True)


def test_model_lines_still_stand_in_the_source():
    """Every source line the model quotes still occurs, white space aside:
    whoever edits one of them is sent to md5_craft.py."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hashbox_amd", "csrc")
    ws = lambda t: re.sub(r"\s+", " ", t)  # noqa: E731
    missing = []
    for name, lines in mc.MIRRORED.items():
        with open(os.path.join(csrc, name)) as fh:
            src = ws(fh.read())
        missing += ["%s: %s" % (name, ln) for ln in lines if ws(ln) not in src]
    assert not missing, "md5_craft.py restates lines that changed:\n" + "\n".join(missing)
    assert (mc.COOP_MIN, mc.PLAN_BINS, mc.BPS, mc.MAX_BLOCK, mc.BUDGET_ALL) == (8, 1024, 16 // 4, 8388608, 0xFFFFFFFF)


def test_launch_schedule_model():
    # lag 1: the batch joins the next submit's launch and takes `need` launches
    assert mc.k3_launches([(5, 64)] + [(1, 0)] * 6, 1) == 5
    assert mc.k3_launches([(5, 64)] + [(1, 0)] * 2, 1) == 3   # two slices, then the drain
    assert mc.k3_launches([(1, 64)], 1) == 1                    # submit + wait: one drain
    assert mc.k3_launches([(1, 0)] * 3, 1) == 0
    # lag 2: empty batches do not age the FIFO; the wait drains
    assert mc.k3_launches([(5, 64)] + [(1, 0)] * 6, 2) == 1
    assert mc.k3_launches([(2, 64), (1, 1), (1, 1), (1, 1)], 2) == 4
