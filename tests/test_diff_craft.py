"""CPU checks of the byte-diff corpus (tests/diff_craft.py): every case's
designed answer is the plain reference's, and each family covers what
tests/test_gpu_diff_crafted.py relies on, asserted on the model alone."""
import collections
import os
import re

import numpy as np
import pytest

from . import diff_craft as dc

PM, P10 = dc.PIECE_MANY, dc.PIECE


@pytest.fixture(scope="module")
def corpus():
    return dc.k11_corpus()


@pytest.fixture(scope="module")
def raw(corpus):
    """(chains, layout) with raw blocks."""
    ch = corpus.chains("r")
    return ch, corpus.layout("r", ch)


@pytest.fixture(scope="module")
def zl(corpus):
    ch = corpus.chains("z")
    return ch, corpus.layout("z", ch)


def diffs(restored: bytes, local: bytes):
    a, b = np.frombuffer(restored, np.uint8), np.frombuffer(local, np.uint8)
    m = min(a.size, b.size)
    return np.flatnonzero(a[:m] != b[:m]).tolist()


def by_family(corpus, fam):
    return [(f, c) for f, c in enumerate(corpus.cases) if c.family == fam]


# ------------------------------------------------------------- reference --
def test_reference_restates_the_definition():
    r = dc.reference
    assert r(b"", b"") is None and r(b"abc", b"abc") is None
    assert r(b"abc", b"abd") == 2 and r(b"abc", b"xbd") == 0
    assert r(b"abc", b"ab") == 2 and r(b"ab", b"abc") == 2 and r(b"", b"abc") == 0 and r(b"abc", b"") == 0
    assert r(b"abc", b"xb") == 0 and r(b"abcd", b"abXd!") == 2


def test_every_case_answers_the_reference(corpus):
    for c in corpus.cases:
        assert c.want == dc.reference(c.restored(), c.local), c.name
    for k in dc.k10_calls():
        assert k.want() == dc.reference(k.restored(), k.local()), k.case.name
    xs = dc.x_set()
    for name, (loc, want) in xs.locals.items():
        assert want == dc.reference(b"".join(xs.blocks), loc), name
    names = [c.name for c in corpus.cases]
    assert len(set(names)) == len(names)
    assert len({k.case.name for k in dc.k10_calls()}) == len(dc.k10_calls())


def test_stated_counts(corpus):
    n = collections.Counter(c.family for c in corpus.cases)
    for fam in ("G", "L", "W", "HT", "S", "F"):
        assert n[fam] == dc.STATED[fam], (fam, n[fam])
    assert len(corpus.cases) - n["filler"] == dc.STATED["k11_cases"]
    assert dict(collections.Counter(k.case.family for k in dc.k10_calls())) == dc.STATED["k10"]
    assert sum(len(c.data) for c in corpus.cases) < 6 << 20
    assert max((len(b) for c in corpus.cases for b in c.blocks), default=0) <= dc.MAX_BLOCK


# ----------------------------------------------------- the model's pieces --
def test_model_cuts_pieces_as_the_host_does():
    B = dc.Blk
    # K10: raw blocks packed, a zlib stream staged at the next multiple of 16, its slot aligned
    lay = dc.k10_layout([B(dc.RAW, 5, 5), B(dc.ZLIB, 30, 70000), B(dc.RAW, 9, 9)], 5 + 70000 + 9)
    assert lay.src_at[0] == [0, 16, 46]
    assert [(p.block, p.foff, p.len, p.src16, p.loc16) for p in lay.pieces] == [
        (0, 0, 5, 0, 0), (1, 5, P10, 0, 5), (1, 5 + P10, 70000 - P10, 0, 5), (2, 70005, 9, 14, 5)]
    p = lay.pieces[1]
    assert (p.head, p.nvec, p.tail0) == (11, 4095, 11 + 65520)
    # a local copy that ends inside block 1 cuts the last piece at `cover`
    lay = dc.k10_layout([B(dc.RAW, 5, 5), B(dc.ZLIB, 30, 70000), B(dc.RAW, 9, 9)], 100)
    assert [(p.foff, p.len) for p in lay.pieces] == [(0, 5), (5, 95)]
    # a piece shorter than its head
    p = dc.Piece(0, 0, 0, 0, 3, 0, 9)
    assert (p.head, p.nvec, p.tail0) == (3, 0, 3)
    # K11: loff is the running sum of `have`; a file of no blocks has no segment; a truncated stream ends `bytes`
    files = [[B(dc.RAW, 20, 20)], [], [B(dc.RAW, 7, 7), B(dc.ZLIB, 11, 40, inflates=False), B(dc.RAW, 3, 3)],
             [B(dc.RAW, PM + 1, PM + 1, id_ok=False)], [B(dc.RAW, 2, 2)]]
    lay = dc.k11_layout(files, [18, 0, 50, PM + 1, 2])
    assert 1 not in lay.segs and [lay.segs[f].index for f in (0, 2, 3, 4)] == [0, 1, 2, 3]
    assert [(lay.segs[f].loff, lay.segs[f].have, lay.segs[f].bytes, lay.segs[f].good, lay.segs[f].n_good)
            for f in (0, 2, 3, 4)] == [(0, 18, 20, 20, 1), (18, 7, 7, 7, 1), (25, PM + 1, PM + 1, 0, 0),
                                       (26 + PM, 2, 2, 2, 1)]
    assert lay.src_at == [[0], [], [20, 32, 43], [46], [47 + PM]]
    assert [(p.file, p.foff, p.len, p.src16, p.loc16) for p in lay.pieces] == [
        (0, 0, 18, 0, 0), (2, 0, 7, 4, 2), (3, 0, PM, 14, 9), (3, PM, 1, 14, 9), (4, 0, 2, 15, (26 + PM) % 16)]
    w = dc.locate(lay.by_file[3], 7 + 16 * 70 + 6, dc.T11)
    assert (w["region"], w["granule"], w["lane"], w["iter"], w["word"], w["byte"]) == ("vector", 70, 6, 1, 1, 2)
    assert (w["workgroup"], w["wave"]) == (0, 2)
    assert dc.locate(lay.by_file[3], 3, dc.T11)["region"] == "head"
    assert dc.locate(lay.by_file[0], 17, dc.T11)["region"] == "tail" and dc.locate(lay.by_file[0], 18, dc.T11) is None


def test_cases_lie_where_they_ask_to(corpus, raw, zl):
    rels = set()
    for (_, lay), mode in ((raw, "r"), (zl, "z")):
        for f, c in enumerate(corpus.cases):
            if c.align is None:
                continue
            p = lay.by_file[f][0]
            assert p.loc16 == c.align and p.foff == 0, c.name
            if mode == "r":
                assert (p.src16 - p.loc16) & 15 == c.rel, c.name
                rels.add(c.rel)
            else:
                assert p.src16 == 0
    assert rels == set(range(16))
    # the whole corpus is one launch of a few thousand workgroups
    assert 9000 < len(raw[1].pieces) < 12000 and len(raw[1].pieces) == len(zl[1].pieces)


# ----------------------------------------------------------------- G ------
def test_g_every_pair_of_a_granule(corpus, raw):
    _, lay = raw
    want = {("pair", a, i, j, x) for a in dc.G_ALIGNS for i in range(16) for j in range(i + 1, 16) for x in dc.XORS}
    got, last = set(), set()
    for f, c in by_family(corpus, "G"):
        d = diffs(c.data, c.local)
        w = [dc.locate(lay.by_file[f], x, dc.T11) for x in d]
        p = lay.by_file[f][0]
        assert len({x["granule"] for x in w}) == 1 and all(x["region"] == "vector" for x in w), c.name
        assert p.tail0 < p.len and p.nvec == 3 and p.loc16 == c.tag[1]
        if c.tag[0] == "all16":
            assert len(d) == 16 and c.want == d[0] and w[0]["granule"] == c.tag[2]
            continue
        _, a, i, j, x = c.tag
        assert len(d) == 2 and c.want == d[0]
        assert [(4 * y["word"] + y["byte"]) for y in w] == [i, j]
        loc = np.frombuffer(c.local, np.uint8)
        assert all(int(loc[q]) ^ c.data[q] == x for q in d)
        if c.tag[0] == "pair":
            assert w[0]["granule"] == 1
            got.add(c.tag)
        else:
            assert w[0]["granule"] == p.nvec - 1  # the last whole granule: a tail follows
            last.add((i, j))
    assert got == want and len(want) == 1080
    assert last == {(i, j) for i in range(16) for j in range(i + 1, 16)} and len(last) == 120
    assert {c.tag[1:] for _, c in by_family(corpus, "G") if c.tag[0] == "all16"} == {(a, g) for a in dc.G_ALIGNS
                                                                                     for g in (1, 2)}


# ----------------------------------------------------------------- L ------
def check_l(cases, threads, aligns, lanes):
    seen = set()
    for c, pieces in cases:
        _, a, lane, it, kind = c.tag
        w = [dc.locate(pieces, x, threads) for x in diffs(c.data, c.local)]
        assert all(x["region"] == "vector" and x["lane"] == lane and x["piece"] == w[0]["piece"] for x in w), c.name
        assert [x["iter"] for x in w] == ([it, it + 1] if kind == "both" else [it + 1]), c.name
        assert dc.locate(pieces, c.want, threads)["iter"] == (it if kind == "both" else it + 1)
        seen.add((a, lane, it, kind))
    assert seen == {(a, lane, it, k) for a in aligns for lane in lanes for it in (0, 1, 14) for k in ("both", "later")}


def test_l_two_iterations_of_one_lane(corpus, raw):
    _, lay = raw
    check_l([(c, lay.by_file[f]) for f, c in by_family(corpus, "L")], dc.T11, (0, 7), (0, 17, 62))


# ----------------------------------------------------------------- W ------
def check_w(cases, threads, pair_count):
    only, xor, ab = set(), collections.defaultdict(set), set()
    for c, pieces in cases:
        d = diffs(c.data, c.local)
        w = [dc.locate(pieces, x, threads) for x in d]
        assert all(x["region"] == "vector" and x["piece"] == w[0]["piece"] for x in w), c.name
        if c.tag[0] == "only":
            assert len(w) == 1 and w[0]["lane"] == c.tag[1] and w[0]["iter"] == 0
            only.add(c.tag[1])
            continue
        kind, *rest = c.tag
        lo, hi, holder = rest[-3:]
        assert len(w) == 2 and {x["lane"] for x in w} == {lo, hi}
        assert w[0]["lane"] == holder and w[0]["iter"] == 0 and w[1]["iter"] == 1  # the minimum is by value
        assert lo // 64 == hi // 64  # one wave
        if kind == "xor":
            assert lo ^ hi == rest[0]
            xor[rest[0]].add((lo, holder))
        else:
            assert lo < hi
            ab.add((lo, hi, holder))
    assert set(xor) == {1, 2, 4, 8, 16, 32}
    for m, s in xor.items():
        assert len(s) == 2 * pair_count[m], (m, len(s))
        assert all((lo, lo) in s and (lo, lo ^ m) in s for lo, _ in s)
    assert len(ab) == 8 and {h == lo for lo, hi, h in ab} == {True, False}
    return only


def test_w_every_lane_and_every_shuffle_distance(corpus, raw):
    _, lay = raw
    only = check_w([(c, lay.by_file[f]) for f, c in by_family(corpus, "W")], dc.T11, dict.fromkeys((1, 2, 4, 8, 16, 32), 32))
    assert only == set(range(64))


# ---------------------------------------------------------------- HT ------
def test_ht_every_length_at_every_alignment(corpus, raw, zl):
    chains, lay = raw
    seen, rel, short = set(), set(), 0
    for f, c in by_family(corpus, "HT"):
        if c.tag[0] != "ht":
            continue
        _, n, a, way = c.tag
        (p,) = lay.by_file[f]
        assert (p.len, p.loc16) == (n, a) and p.head == min(n, (16 - a) & 15)
        short += p.len < ((16 - a) & 15)
        rel.add((p.src16 - p.loc16) & 15)
        seen.add((n, a, way))
        d = diffs(c.data, c.local)
        assert d == {"same": [], "first": [0], "last": [n - 1], "both": sorted({0, n - 1})}[way]
        (q,) = zl[1].by_file[f]
        assert (q.len, q.loc16, q.src16) == (n, a, 0)
    assert seen == {(n, a, w) for n in range(1, 49) for a in range(16) for w in dc.HT_WAYS} and len(seen) == 3072
    assert rel == set(range(16))
    assert short >= 4 * 100  # pieces that end inside their head: `head = min(len, ...)`
    # every region holds the first and the last byte of some case
    first, last = collections.Counter(), collections.Counter()
    for f, c in by_family(corpus, "HT"):
        if c.tag[0] == "ht":
            first[dc.locate(lay.by_file[f], 0, dc.T11)["region"]] += 1
            last[dc.locate(lay.by_file[f], len(c.data) - 1, dc.T11)["region"]] += 1
    assert set(first) == set(last) == {"head", "vector", "tail"}  # (a piece of no whole granule at alignment 0 is all tail)


def test_ht_piece_edges(corpus, raw):
    _, lay = raw
    seen = set()
    for f, c in by_family(corpus, "HT"):
        if c.tag[0] != "edge":
            continue
        _, n, a, what = c.tag
        w = [dc.locate(lay.by_file[f], x, dc.T11) for x in diffs(c.data, c.local)]
        reg = [x["region"] for x in w]
        if what == "head_vs_vector":
            assert reg == ["head", "vector"] and w[1]["granule"] == 0
        elif what == "vector_vs_tail":
            assert reg == ["vector", "tail"] and w[1]["lane"] == 0
        elif what == "piece_vs_next":
            assert w[0]["piece"] + 1 == w[1]["piece"] and w[1]["at"] == 0
        elif what == "next_piece":
            assert len(w) == 1 and w[0]["at"] == 0 and lay.by_file[f][1].len == 1
        seen.add((n, a, what))
    for n in (PM - 1, PM, PM + 1):
        assert (n, 3, "head_vs_vector") in seen
    assert {(PM - 1, 3, "vector_vs_tail"), (PM - 1, 0, "vector_vs_tail"), (PM, 3, "vector_vs_tail"),
            (PM + 1, 3, "vector_vs_tail"), (PM, 0, "vector_last"), (PM + 1, 0, "piece_vs_next"),
            (PM + 1, 3, "piece_vs_next")} <= seen


def test_identical_cases_lie_between_bytes_that_differ(corpus, raw):
    """In the packed source (raw blocks) and the packed local image, the byte
    just before and the byte just behind every guarded case differ: a
    comparison one byte wide of [0, len) reports a difference."""
    chains, lay = raw
    end = max(a + len(fld) for at, ch in zip(lay.src_at, chains) for a, (_, fld, _) in zip(at, ch))
    staged = np.zeros(end, np.uint8)
    total = max(s.loff + s.have for s in lay.segs.values())
    limg = np.zeros(total, np.uint8)
    for f, (c, ch) in enumerate(zip(corpus.cases, chains)):
        for a, (t, fld, _) in zip(lay.src_at[f], ch):
            staged[a:a + len(fld)] = np.frombuffer(fld, np.uint8)
        if f in lay.segs:
            s = lay.segs[f]
            limg[s.loff:s.loff + s.have] = np.frombuffer(c.local, np.uint8)[:s.have]
    n = 0
    for f, c in enumerate(corpus.cases):
        if not c.guard:
            continue
        a, s, ln = lay.src_at[f][0], lay.segs[f], len(c.data)
        assert s.have == ln and len(c.blocks) == 1
        assert np.array_equal(staged[a:a + ln], np.frombuffer(c.data, np.uint8))
        assert staged[a - 1] != limg[s.loff - 1] and staged[a + ln] != limg[s.loff + ln], c.name
        n += c.want is None
    assert n == 48 * 16


# ----------------------------------------------------------------- S ------
def check_s(cases, threads):
    seen = {}
    for c, pieces in cases:
        _, what, x = c.tag
        d = diffs(c.data, c.local)
        assert d == list(range(x, len(c.data))) and c.want == x
        assert len(pieces) == 9 and len(c.blocks) == 3 and len({p.block for p in pieces}) == 3
        seen[what] = dc.locate(pieces, x, threads)
        seen[what]["x"] = x
        k = next(k for k, p in enumerate(pieces) if p.index == seen[what]["piece"])
        seen[what].update(piece=k, piece_len=pieces[k].len)  # (the piece's place in its file: each case is a file)
    s = seen
    assert s["zero"]["x"] == 0
    assert s["in_head"]["region"] == "head" and 0 < s["in_head"]["lane"]
    assert s["vector_first"]["region"] == "vector" and s["vector_first"]["granule"] == 0 and s["vector_first"]["word"] == 0
    assert s["vector_last"]["region"] == "vector" and (s["vector_last"]["word"], s["vector_last"]["byte"]) == (3, 3)
    assert s["vector_last"]["x"] + 1 == s["in_tail"]["x"] - s["in_tail"]["lane"]
    assert s["in_tail"]["region"] == "tail" and s["in_tail"]["lane"] > 0
    assert s["piece_last"]["at"] == s["piece_last"]["piece_len"] - 1
    assert s["next_piece_first"]["at"] == 0 and s["next_piece_first"]["piece"] == s["piece_last"]["piece"] + 1
    assert s["next_piece_first"]["block"] == s["piece_last"]["block"]
    assert s["next_block_first"]["at"] == 0 and s["next_block_first"]["block"] == s["block_last"]["block"] + 1
    assert s["block_last"]["x"] + 1 == s["next_block_first"]["x"]
    assert s["file_last"]["block"] == 2 and s["second_block_last"]["block"] == 1
    assert len(seen) == 11


def test_s_suffixes(corpus, raw):
    _, lay = raw
    check_s([(c, lay.by_file[f]) for f, c in by_family(corpus, "S")], dc.T11)


# ----------------------------------------------------------------- F ------
def test_f_files_share_workgroups(corpus, raw, zl):
    for _, lay in (raw, zl):
        wg_of = collections.defaultdict(set)
        for p in lay.pieces:
            wg_of[p.index // dc.WAVES].add(p.file)
        pos = {True: set(), False: set()}
        for f, c in by_family(corpus, "F"):
            if c.tag[0] != "wg":
                continue
            (p,) = lay.by_file[f]
            pos[c.tag[3]].add(p.index % dc.WAVES)
            assert len(wg_of[p.index // dc.WAVES]) == 4  # four files in its workgroup
            assert (c.want is not None) == c.tag[3]
        assert pos[True] == {0, 1, 2, 3} and pos[False] == {0, 1, 2, 3}
    fam = by_family(corpus, "F")
    empt = [k for k, (f, c) in enumerate(fam) if c.tag[0] == "empty"]
    assert len(empt) == 10 and all(fam[k - 1][1].tag[0] == "wg" and fam[k + 1][1].tag[0] in ("wg", "shift") for k in empt)
    assert {c.tag[1] for _, c in fam if c.tag[0] == "empty"} == {0, 3}
    assert all(f not in raw[1].segs for f, c in fam if c.tag[0] == "empty")


def test_f_lengths_and_bad_blocks(corpus, raw, zl):
    for _, lay in (raw, zl):
        cuts = set()
        for f, c in by_family(corpus, "F"):
            if c.tag[0] == "short":
                cutat = c.tag[1]
                ps = lay.by_file.get(f, [])
                assert sum(p.len for p in ps) == cutat == len(c.local)
                if c.tag[2] == "before":
                    assert c.want == cutat - 1 and dc.locate(ps, cutat - 1, dc.T11) is not None
                    assert dc.locate(ps, cutat, dc.T11) is None
                cuts.add(cutat % PM)
            elif c.tag[0] == "long":
                ps = lay.by_file[f]
                assert sum(p.len for p in ps) == len(c.data) < len(c.local)
                if c.tag[1] == "behind":  # differing bytes no piece covers
                    a, b = np.frombuffer(c.local, np.uint8), np.frombuffer(c.data, np.uint8)
                    assert c.want == len(c.data) and a[len(c.data)] != 0 and np.array_equal(a[:b.size], b)
            elif c.tag[0] == "bad":
                s = lay.segs[f]
                pre = len(c.restored())
                assert s.n_good == 2 and s.good == pre and s.status == [True, True, False, True]
                covered = sum(p.len for p in lay.by_file[f])
                if c.tag[2] == "exact":
                    assert covered == pre and c.want is None
                elif c.tag[1] == "truncated":
                    assert covered == pre == s.bytes
                else:  # a wrong ID: the blocks behind it are compared and their word is dropped by the prefix rule
                    assert covered == len(c.data) > pre
                if c.tag[2] == "behind":
                    assert min(diffs(c.data, c.local)) == pre == c.want
        assert len(cuts - {0}) >= 3  # pieces cut at `cover`, away from a piece boundary
    kinds = {c.tag[1:] for _, c in by_family(corpus, "F") if c.tag[0] == "bad"}
    assert kinds == {(k, w) for k in ("truncated", "wrong_id") for w in ("before", "behind", "both", "none", "exact")}


# ----------------------------------------------------------------- X ------
def test_x_windows_and_passes():
    xs = dc.x_set()
    assert dc.restore_stride(dc.X_MB) == 8448 and (2 * 8448) // 8448 == 2  # diff_file: two blocks a window
    win = {k: [dc.x_window_of(x) for x in v] for k, v in xs.flips.items()}
    assert win == {"same": [], "second": [1], "third": [2], "first_third": [0, 2], "each": [0, 1, 2]}
    assert all(len(z) <= dc.X_MB and len(b) <= dc.X_MB for b, (_, z) in zip(xs.blocks, xs.wired))
    files, wired, ids = dc.x_files()
    passes = dc.x_passes(files, wired, dc.X_WB)
    big = 10
    assert len(files) == 21 and len(files[big]) == 6
    with_big = [k for k, p in enumerate(passes) if any(f == big for f, _ in p)]
    assert len(passes) == 4 and with_big == [0, 1, 2, 3]
    # the first pass holds ten small files before the big one's first block (its segment index and loff are not
    # zero there); in the last pass the big file continues (foff0 > 0) in front of the ten small files behind it
    assert passes[0] == [(f, 0) for f in range(10)] + [(big, 0)]
    assert passes[1] == [(big, 1), (big, 2)] and passes[2] == [(big, 3), (big, 4)]
    assert passes[3] == [(big, 5)] + [(f, 0) for f in range(11, 21)]
    offs = np.concatenate([[0], np.cumsum(dc.X_BLOCKS)])
    blk = {k: [int(np.searchsorted(offs, x, side="right")) - 1 for x in v] for k, v in xs.flips.items()}
    assert blk["each"] == [0, 2, 5]  # passes 0, 1 and 3


# --------------------------------------------------------------- K10 ------
@pytest.fixture(scope="module")
def k10():
    return [(k, k.layout()) for k in dc.k10_calls()]


def shifted(k, lay):
    """The case with the pieces' offsets taken back by the block in front."""
    n = len(k.pre)
    return [dc.Piece(p.index, 0, p.block, p.foff - n, p.len, p.src16, p.loc16) for p in lay.pieces if p.foff >= n]


def test_k10_lanes_waves_and_workgroups(k10):
    fam = collections.defaultdict(list)
    for k, lay in k10:
        assert not k.pre or k.case.family in ("HT", "G")
        fam[k.case.family].append((k.case, shifted(k, lay)))
    check_l(fam["L"], dc.T10, (0,), (0, 100, 255))
    lanes = (0, 5, 10, 23, 36, 49, 58, 63)  # of wave l % 4 each
    only = check_w(fam["W"], dc.T10, {m: sum(not l & m for l in lanes) for m in (1, 2, 4, 8, 16, 32)})
    assert len(only) == 64 and {x // 64 for x in only} == {0, 1, 2, 3} and {x % 64 for x in only} == set(range(64))
    check_s(fam["S"], dc.T10)
    solo, pairs = set(), set()
    for c, pieces in fam["WG"]:
        w = [dc.locate(pieces, x, dc.T10) for x in diffs(c.data, c.local)]
        assert len(pieces) == 1 and all(x["region"] == "vector" for x in w)
        if c.tag[0] == "only":
            assert [x["wave"] for x in w] == [c.tag[1]]
            solo.add(c.tag[1])
        else:
            _, a, b, holder = c.tag
            assert {x["wave"] for x in w} == {a, b} and w[0]["wave"] == holder and len(w) == 2
            pairs.add((a, b, holder))
    assert solo == {0, 1, 2, 3}
    assert pairs == {(a, b, h) for a in range(4) for b in range(a + 1, 4) for h in (a, b)}
    # no W or WG call is longer than one piece
    assert all(len(k.local()) <= P10 for k, _ in k10 if k.case.family in ("W", "WG", "L"))


def test_k10_heads_tails_and_granules(k10):
    seen, pairs = set(), set()
    for k, lay in k10:
        c = k.case
        if c.family == "HT":
            _, mode, n, a, way = c.tag
            p = lay.pieces[-1]
            assert (p.len, p.loc16, p.foff) == (n, a, a) and len(lay.pieces) == (2 if a else 1)
            assert p.src16 == (a if mode == "r" else 0)
            assert k.want() == (None if way == "same" else a + (n - 1 if way == "last" else 0))
            seen.add((mode, n, a, way))
        elif c.family == "G" and c.tag[0] == "pair":
            _, a, i, j, x = c.tag
            w = [dc.locate(lay.pieces, q + len(k.pre), dc.T10) for q in diffs(c.data, c.local)]
            assert [(y["region"], y["granule"], 4 * y["word"] + y["byte"]) for y in w] == [("vector", 1, i), ("vector", 1, j)]
            assert w[0]["loc16"] == a == 9
            pairs.add((i, j))
    assert seen == {(m, n, a, w) for m, lens in (("r", dc.K10_HT_LENS), ("z", dc.K10_HT_ZLENS)) for n in lens
                    for a in range(16) for w in dc.HT_WAYS}
    assert len(pairs) == 120


# ------------------------------------------------------------- reporting --
def test_verdict_names_the_level(corpus, raw):
    _, lay = raw
    f, c = next((f, c) for f, c in by_family(corpus, "W") if c.tag[0] == "xor" and c.tag[1] == 32)
    other = max(diffs(c.data, c.local))
    v = dc.verdict(lay.by_file[f], dc.T11, c.restored(), c.local, c.want, other)
    assert "expected offset %d" % c.want in v and "got candidate 1 of 2" in v
    assert "lane %d iteration 0" % c.tag[4] in v and "iteration 1" in v
    assert "every candidate was lost" in dc.verdict(lay.by_file[f], dc.T11, c.restored(), c.local, c.want, None)
    assert "no differing byte" in dc.verdict(lay.by_file[f], dc.T11, c.restored(), c.local, c.want, c.want + 1)


def test_model_quotes_the_source():
    """Every source line the model restates still occurs in the kernels and
    the engine (white space collapsed): an edit of one of them fails here and
    sends its author to diff_craft.py."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hashbox_amd", "csrc")
    ws = lambda t: re.sub(r"\s+", " ", t)  # noqa: E731
    missing = []
    for name, lines in dc.MIRRORED.items():
        with open(os.path.join(csrc, name)) as fh:
            src = ws(fh.read())
        missing += ["%s: %s" % (name, ln) for ln in lines if ws(ln) not in src]
    assert not missing, "diff_craft.py restates lines that changed:\n" + "\n".join(missing)
