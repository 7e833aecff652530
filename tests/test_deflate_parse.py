"""CPU: the structural decoder of tests/deflate_parse.py against CPython's
zlib (every stream must expand to what zlib inflates) and against the headers
tests/deflate_craft.py dictated, and its package-merge against brute force.
"""
import itertools
import zlib

import numpy as np
import pytest

from tests import deflate_craft as C
from tests import deflate_parse as P
from tests.test_deflate_craft import FAMILIES
from tests.test_gpu_deflate import _text


@pytest.fixture(scope="module")
def crafted():
    """Every family rebuilt with ``dynamic`` wrapped, so that each stream's
    dictated headers are on record: {deflate body: [(bit offset, header)]}."""
    reg = {}
    orig_dyn, orig_get = C.dynamic, C.BitWriter.getvalue

    def dynamic(tokens, final, litlen_lens=None, dist_lens=None, cl_lens=None, raw_header=None, hclen=None,
                eob=True):
        blk = orig_dyn(tokens, final, litlen_lens, dist_lens, cl_lens, raw_header, hclen, eob)
        lf, df = C._frequencies(tokens)  # the defaults, as dynamic() resolves them
        ll = list(litlen_lens) if litlen_lens is not None else C.huffman_lens(lf, 286)
        while litlen_lens is None and len(ll) > 257 and ll[-1] == 0:
            ll.pop()
        dl = list(dist_lens) if dist_lens is not None else C.huffman_lens(df, 30)
        while dist_lens is None and len(dl) > 1 and dl[-1] == 0:
            dl.pop()
        hlit, hdist, ops = raw_header or (len(ll) - 257, len(dl) - 1, C.cl_ops_for(ll + dl))
        cl = list(C.DEFAULT_CL if cl_lens is None else cl_lens)
        hc = hclen
        if hc is None:
            hc = 19
            while hc > 4 and cl[C.ORDER[hc - 1]] == 0:
                hc -= 1
        rec = dict(hlit=hlit + 257, hdist=hdist + 1, hclen=hc, ops=[tuple(o) for o in ops], litlen=ll, dist=dl,
                   cl=[cl[s] if C.ORDER.index(s) < hc else 0 for s in range(19)])

        def block(w):
            w.__dict__.setdefault("dictated", []).append((w.tell(), rec))
            blk(w)
        return block

    def getvalue(self):
        v = orig_get(self)
        reg[v] = list(self.__dict__.get("dictated", []))
        return v

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(C, "dynamic", dynamic)
        mp.setattr(C.BitWriter, "getvalue", getvalue)
        cases = {f.__name__: f.__wrapped__() for f in FAMILIES}
    return reg, cases


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_good_cases_parse_to_their_bytes_and_headers(crafted, family):
    reg, cases = crafted
    n_dyn = 0
    for c in cases[family.__name__]:
        if c.status not in (0, 3):
            continue
        st = P.parse(c.stream)
        data = st.expand()
        assert data == zlib.decompress(c.stream), c.name
        if c.status == 0:
            assert data == c.expected, c.name
        assert (st.trailing != b"") == (c.name in C.TRAILING), c.name
        assert sum(b.out_len for b in st.blocks) == len(data) and st.blocks[-1].bfinal == 1, c.name
        assert all(b.out_start == sum(x.out_len for x in st.blocks[:i]) for i, b in enumerate(st.blocks)), c.name
        # the writer's record of this stream: the body alone (zwrap) or with the zlib header (the split streams)
        body = c.stream[:len(c.stream) - len(st.trailing) - 4]
        base, rec = (0, reg[body]) if body in reg else (16, reg.get(body[2:]))
        if rec is None:
            assert c.name in C.TRAILING, c.name  # zlib's own stream
            continue
        dyn = [b for b in st.blocks if b.btype == 2]
        assert len(dyn) == len(rec), c.name
        for b, (at, want) in zip(dyn, rec):
            n_dyn += 1
            assert b.start == at + base, c.name
            assert (b.hlit, b.hdist, b.hclen) == (want["hlit"], want["hdist"], want["hclen"]), c.name
            assert b.ops == want["ops"], c.name
            assert b.cl_lens == want["cl"], c.name
            assert b.litlen_lens == want["litlen"] and b.dist_lens == want["dist"], c.name
            assert C.run_cl_ops(b.ops) == b.litlen_lens + b.dist_lens, c.name
    if family in (C.chains, C.structure, C.rejections, C.split_good):
        assert n_dyn > 0  # the comparison ran


def test_block_fields(crafted):
    by = {c.name: c for c in crafted[1]["structure"]}
    st = P.parse(by["stored_one_after_3_nine_bit_literals"].stream)
    f, s, g = st.blocks
    assert (f.btype, s.btype, g.btype) == (1, 0, 1) and (f.bfinal, s.bfinal, g.bfinal) == (0, 0, 1)
    assert f.start == 16 and f.end == 16 + 3 + 3 * 9 + 7 == s.start
    assert s.end == g.start and s.end % 8 == 0 and s.end - s.start == 3 + (-(s.start + 3) % 8) + 32 + 8
    assert f.tokens == [200] * 3 and s.tokens == [b"\x5a"] and (s.out_start, s.out_len) == (3, 1)
    st = P.parse(by["lengths_1_to_15"].stream)
    (b,) = st.blocks
    m = [t for t in b.tokens if not isinstance(t, int)]
    assert max(b.litlen_lens) == 15 and max(b.dist_lens) == 15
    for ds in range(16):
        lo, hi = m[2 * ds], m[2 * ds + 1]
        assert (lo.length, lo.lsym, lo.lextra, lo.dsym, lo.dextra) == (3, 257, 0, ds, 0)
        assert (hi.length, hi.lsym, hi.lextra, hi.dsym, hi.dextra) == (258, 285, 0, ds, (1 << C.DIST_EXTRA[ds]) - 1)
        assert hi.distance == C.DIST_BASE[ds] + hi.dextra
    assert b.litlen_counts()[285] == 16 and b.dist_counts()[15] == 2 and b.op_counts()[18] >= 1
    st = P.parse([c for c in crafted[1]["chains"] if c.name == "len258_as_284_extra31"][0].stream)
    m = [t for t in st.blocks[0].tokens if not isinstance(t, int)][0]
    assert (m.length, m.lsym, m.lextra) == (258, 284, 31)


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_structural_rejections_raise(crafted, family):
    n = 0
    for c in crafted[1][family.__name__]:
        if c.status in (0, 3):  # 3: a valid stream given too small an output
            continue
        n += 1
        with pytest.raises(P.ParseError):
            P.parse(c.stream)
            pytest.fail(f"parse accepts {c.name}")
    assert n > 0 or family is not C.rejections


def test_more_rejections():
    ok = C.good("x", [("d", [b"abc", (5, 2)])]).stream
    P.parse(ok)
    for bad in (ok[:-4] + bytes(4), ok[:1], b"", ok[:-5]):
        with pytest.raises(P.ParseError):
            P.parse(bad)
    # a single literal/length code of one bit is zlib's one allowed incomplete code; of two bits it is not
    one = C.zwrap([C.dynamic([], True, litlen_lens=[0] * 256 + [1], dist_lens=[0])], b"")
    assert zlib.decompress(one) == b"" and P.parse(one).expand() == b""
    two = C.zwrap([C.dynamic([], True, litlen_lens=[0] * 256 + [2], dist_lens=[0])], b"")
    with pytest.raises(zlib.error):
        zlib.decompress(two)
    with pytest.raises(P.ParseError):
        P.parse(two)
    # a distance before the start of the output
    with pytest.raises(P.ParseError):
        P.parse(C.zwrap([C.fixed([1, 2, (3, 3)], True)], b""))


def _inputs():
    rng = np.random.default_rng(3)
    return [("text", _text(100_001, 5)), ("random", rng.integers(0, 256, 70_001, dtype=np.uint8).tobytes()),
            ("zero", bytes(100_001)), ("empty", b"")]


@pytest.mark.parametrize("strategy", [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY],
                         ids=["default", "fixed", "huffman_only"])
@pytest.mark.parametrize("level", [1, 6, 9])
def test_zlib_streams_parse_exactly(level, strategy):
    for name, data in _inputs():
        co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        z = co.compress(data) + co.flush()
        st = P.parse(z)
        assert st.expand() == data, name
        assert st.trailing == b"" and st.adler == zlib.adler32(data) and (st.cmf, st.flg) == (z[0], z[1]), name
        assert st.blocks[-1].end <= 8 * (len(z) - 4) < st.blocks[-1].end + 8, name
        for b in st.blocks:
            if strategy == zlib.Z_FIXED:
                assert b.btype != 2, name  # (zlib still stores what the fixed code would grow)
            if strategy == zlib.Z_HUFFMAN_ONLY:
                assert all(isinstance(t, (int, bytes)) for t in b.tokens), name
            if b.btype == 2:  # zlib's codes are complete and within the limits
                assert P.kraft(b.litlen_lens) == 1 << 15 and max(b.cl_lens) <= 7, name
                f, lens = b.litlen_counts(), b.litlen_lens
                assert all(lens[s] for s in f), name
                # zlib's own limited code against the optimum under the same limit
                opt = P.optimal_limited_lengths(f, 15)
                assert P.coded_cost(f, opt) <= P.coded_cost(f, lens), name


# ------------------------------------------------------------ package-merge --
def _complete_sets(n, maxbits):
    return [ls for ls in itertools.product(range(1, maxbits + 1), repeat=n)
            if sum(1 << (maxbits - k) for k in ls) == 1 << maxbits]


def _freq_sets(n):
    rng = np.random.default_rng(100 + n)
    fib = [1, 1, 2, 3, 5, 8, 13, 21][:n]
    out = [fib, fib[::-1], [1] * n, [1 << k for k in range(n)], [1] * (n - 1) + [1000], [7] * (n - 1) + [8]]
    out += [list(map(int, rng.integers(1, 10, n))) for _ in range(25)]
    out += [list(map(int, rng.zipf(1.5, n) % 5000 + 1)) for _ in range(25)]
    return out


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_package_merge_is_the_brute_force_optimum(n):
    for maxbits in range(max(1, (n - 1).bit_length()), 7):
        sets = _complete_sets(n, maxbits)
        assert sets
        for f in _freq_sets(n):
            best = min(sum(a * b for a, b in zip(f, ls)) for ls in sets)
            lens = P.optimal_limited_lengths(f, maxbits)
            assert max(lens) <= maxbits and min(lens) >= 1, (f, maxbits, lens)
            assert sum(1 << (maxbits - k) for k in lens) == 1 << maxbits, (f, maxbits, lens)
            assert P.coded_cost(f, lens) == best, (f, maxbits, lens)
            if maxbits >= n - 1:  # no limit in effect
                assert best == P.huffman_cost(f), (f, maxbits)


def test_package_merge_shapes_and_large_alphabets():
    assert P.optimal_limited_lengths({5: 9}, 15) == {5: 1}
    assert P.optimal_limited_lengths([0, 4, 0], 15) == [0, 1, 0]
    assert P.optimal_limited_lengths({}, 15) == {}
    with pytest.raises(ValueError):
        P.optimal_limited_lengths([1] * 5, 2)
    rng = np.random.default_rng(8)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for f in (fib, [int(x) for x in rng.zipf(1.2, 286) % 100_000 + 1], [1 << k for k in range(25)], [3] * 286):
        f = {s: v for s, v in enumerate(f)}
        huff = P.huffman_cost(f)
        assert P.coded_cost(f, P.optimal_limited_lengths(f, 40)) == huff
        prev = None
        for mb in (9, 12, 15):
            lens = P.optimal_limited_lengths(f, mb)
            cost = P.coded_cost(f, lens)
            assert max(lens.values()) <= mb and P.kraft(lens.values(), 40) == 1 << 40
            assert cost >= huff and (prev is None or cost <= prev)  # a looser limit never costs more
            assert cost <= P.coded_cost(f, C.huffman_lens(f, len(f), mb))  # nor more than the halving heuristic
            prev = cost


def test_unlimited_depth():
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    for n in (2, 3, 10, 17, 24):
        assert P.unlimited_depth(fib[:n]) == n - 1
        assert P.unlimited_depth({s: v for s, v in enumerate(fib[:n])}) == n - 1
    assert P.unlimited_depth([]) == 0 and P.unlimited_depth([9]) == 1 and P.unlimited_depth([0, 9, 0]) == 1
    for k in range(1, 9):
        assert P.unlimited_depth([5] * (1 << k)) == k
    assert P.unlimited_depth([1 << k for k in range(20)]) == 19
    # ties: 1 1 2 2 has optimal trees of depth 2 and 3; the two-queue rule builds the shallow one
    assert P.unlimited_depth([1, 1, 2, 2]) == 2
