"""CPU checks of the K1 summary corpus (tests/k1_craft.py): the reference
rests on two implementations of the digest, the arena is what it claims, and
the corpus has every property tests/test_gpu_k1_summaries.py relies on,
asserted on the reference alone."""
import os
import re

import numpy as np
import pytest

from . import k1_craft as kc

MIN, SLICE = kc.MIN, kc.SLICE


@pytest.fixture(scope="module")
def corpus():
    return kc.corpus()


def test_digest_all_agrees_with_the_python_rollsum(oracle, corpus):
    """The closed form of oracle/hbx_oracle.c against Init + 65,536 Rollins of
    the Python class, before, at and after the first full window, at a tile
    start and at the last position."""
    f = next(i for i, x in enumerate(corpus.files) if x.name == "tiles_12")
    x = corpus.data(f)
    D = oracle.digest_all(x)
    for q in (0, 1, 31, MIN - 2, MIN - 1, MIN, 3 * MIN - 1, 3 * MIN, x.size - 1):
        assert kc.rollsum_digest(x, q) == int(D[q]), q
    ramp = next(x.data for x in corpus.files if x.name == "ramp_ff")
    Dr = oracle.digest_all(ramp)
    for q in (0, 255, 257):  # the ramp from the virtual zeros: s1 = 255 (q + 1), s2 = 2^15 + 255 (q + 1)(q + 2) / 2
        want = ((0x8000 + 255 * (q + 1) * (q + 2) // 2) & 0xFFFF) << 16 | (255 * (q + 1)) & 0xFFFF
        assert int(Dr[q]) == want == kc.rollsum_digest(ramp, q)


def test_summaries_restate_the_definition(oracle):
    x = oracle.random_bytes(2 * MIN + SLICE + 5, 3)
    D = oracle.digest_all(x)
    s = kc.summaries(x)
    assert s.shape == (34, 2) and s.dtype == np.uint32
    for j in (0, 1, 32, 33):
        assert int(s[j, 0]) == int(D[SLICE * j:min(SLICE * (j + 1), x.size)].max())
        assert int(s[j, 1]) == (int(D[SLICE * j - 1]) if j else 0x80000000)
    assert int(s[33, 0]) == int(D[-5:].max())
    assert [kc.n_slices(n) for n in (0, 1, MIN, 2 * MIN, 2 * MIN + 1, 3 * MIN, 3 * MIN + 1)] == [0, 0, 0, 0, 33, 48, 49]


def test_arena_is_filler_with_files_apart(corpus):
    offs, lens = corpus.offs.astype(np.int64), corpus.lens.astype(np.int64)
    assert (offs % 16 == 0).all() and {int(o) % 64 for o in offs} == {0, 16, 32, 48}
    assert offs[0] >= 128 and (np.diff(offs) > 0).all()
    ends = offs + lens
    assert (offs[1:] - ends[:-1] >= kc.GAP).all() and kc.GAP >= kc.ARENA_SLACK
    assert corpus.host.size - ends[-1] >= 64 << 10
    inside = np.zeros(corpus.host.size, bool)
    for s, e in zip(offs, ends):
        inside[s:e] = True
    assert (corpus.host[~inside] != 0).all()
    assert corpus.host.size <= kc.MAX_CORPUS
    assert max(f.n for f in corpus.files) < 4 << 20
    for i, f in enumerate(corpus.files):
        assert np.array_equal(corpus.data(i), f.data), f.name


def test_lengths_cover_the_run_slice_and_iteration_ends(corpus):
    ns = {f.n for f in corpus.files if f.family == "lengths"}
    assert {2 * MIN, 2 * MIN + 1} <= ns
    assert {k * MIN + d for k in (3, 4) for d in (-1, 0, 1)} <= ns
    assert {3 * MIN + SLICE * j + d for j in (0, 1, 15) for d in (-1, 0, 1, 63, 64, 65)} <= ns
    scanning = [f for f in corpus.files if kc.n_slices(f.n)]
    assert {f.n % 16 for f in scanning if f.family == "lengths"} == set(range(16))
    assert {f.n for f in corpus.files if f.family == "none"} == {0, 1, MIN, 2 * MIN}
    assert all(kc.n_slices(f.n) == 0 for f in corpus.files if f.family == "none")
    # slices that hold 1, 63, 64, 65 and 4,095 positions, and files that end with an iteration
    last = {f.n - SLICE * (kc.n_slices(f.n) - 1) for f in scanning}
    assert {1, 63, 64, 65, 4095, 4096} <= last
    assert any(f.n % MIN == 0 for f in scanning) and any(f.n % MIN == 1 for f in scanning)


def test_tail_property(oracle, corpus):
    """"tail" files (N no multiple of 16, so K1's descriptor reaches into the
    filler): over file + filler, D one position past the end is above the
    last slice's true maximum (so is the maximum over [slice start, N + 16)):
    a mask one position, or one 16-byte load, too wide changes smax.
    "tail0" files (N a multiple of 16: K1 loads zeros past the file): the same
    for D[N] computed with a zero byte at N.  "last" files: D[N - 1] alone
    holds the last slice's maximum: a mask one position too narrow changes
    it."""
    n_of = dict.fromkeys(("tail", "tail_masked", "tail0", "tail0_masked", "last"), 0)
    for i, f in enumerate(corpus.files):
        if not f.kind:
            continue
        n = f.n
        lo = (n - 1) // SLICE * SLICE
        D = corpus.extended(i)
        true_max = int(D[lo:n].max())
        assert true_max == int(corpus.ref()[i][-1, 0])
        n_of[f.kind] += 1
        if f.kind == "tail":
            assert n % 16 and int(D[n]) > true_max and int(D[lo:n + 16].max()) > true_max, f.name
            assert int(corpus.host[int(corpus.offs[i]) + n]) == f.after != 0
            n_of["tail_masked"] += n % MIN != 0  # the file's last iteration is partial: digest_pass_sdwa<true>
        elif f.kind == "tail0":
            D0 = oracle.digest_all(np.concatenate([f.data, np.zeros(16, np.uint8)]))
            assert np.array_equal(D, D0)  # extended() puts zeros there, as K1's loads do
            assert n % 16 == 0 and int(D0[n]) > true_max and int(D0[lo:n + 16].max()) > true_max, f.name
            assert corpus.host[int(corpus.offs[i]) + n] != 0  # the arena still holds filler there
            n_of["tail0_masked"] += n % MIN != 0
        else:
            assert int(D[n - 1]) == true_max and (n - 1 == lo or int(D[lo:n - 1].max()) < true_max), f.name
    assert n_of == {k: kc.STATED[k] for k in n_of}


def test_block_wave_wraps(corpus):
    """At least 8 slices per direction whose maximum lies in a 32-position
    stream at or after a wrap of the 16-bit s1 in that stream (the figures are
    the ones DESIGN.md states); in the masked pass of the short waves, which
    handles 16 slices a file, 9 and 6 (each one shows a leak that is there)."""
    w = next(f for f in corpus.files if f.family == "wave")
    assert w.n == 2 * (1 << 20) + 777
    lo_half, hi_half = w.data[MIN:2 * MIN], w.data[:MIN]
    assert lo_half.max() <= 0x3F and hi_half.min() >= 0xC0
    up, down = kc.wrap_slices(w.data)
    assert len(up) >= 8 and len(down) >= 8, (len(up), len(down))
    assert (len(up), len(down)) == (kc.STATED["wave_up"], kc.STATED["wave_down"])
    tup = tdown = 0
    for f in corpus.files:
        if f.family == "wave_tail":
            assert f.n % MIN > 15 * SLICE
            first = kc.WAVES * (f.n // MIN)  # the first slice of the masked iteration
            u, d = kc.wrap_slices(f.data)
            tup += sum(j >= first for j in u)
            tdown += sum(j >= first for j in d)
    assert (tup, tdown) == (kc.STATED["masked_up"], kc.STATED["masked_down"])
    # random bytes hardly do this: the reason the family exists
    r = next(f for f in corpus.files if f.name == "tiles_37")
    ru, rd = kc.wrap_slices(r.data)
    assert len(ru) + len(rd) <= 4


def test_values_families(oracle, corpus):
    by = {f.name: f for f in corpus.files}
    for v in (0x00, 0x5A, 0xFF):
        assert (by["const_%02x" % v].data == v).all()
    assert (by["ramp_ff"].data[:MIN] == 0xFF).all()
    for name in kc.CUT_CASES:  # sparse single bytes on a constant background
        x = by["cut_" + name].data
        bg = np.bincount(x).argmax()
        assert (x != bg).sum() <= 4 and kc.n_slices(x.size), name
    # maxima at the last positions of a file, at both ends of a slice and of a tile of 3 and 16
    D = oracle.digest_all(by["cut_u_end_mid-slice_N-1"].data)
    assert int(np.flatnonzero(D == D[(D.size - 1) // SLICE * SLICE:].max())[-1]) == D.size - 1


def test_tiles(corpus):
    """Several tiles per file at every tile length the GPU test sets; every
    tile's first slice takes sprev from k1_prime's halo path."""
    ns = {f.name: f.n for f in corpus.files}
    assert ns["tiles_37"] == 37 * MIN + 999 and ns["tiles_12"] == (37 * MIN + 999) // 3
    for tile in kc.TILES:
        firsts = kc.tile_first_slices(corpus, tile)
        assert len(firsts) == kc.STATED["tile_first"][tile], (tile, len(firsts))
        assert all(j % (kc.WAVES * tile) == 0 and 0 < j < kc.n_slices(int(corpus.lens[f])) for f, j in firsts)
        multi = {f for f, _ in firsts}
        assert {i for i, f in enumerate(corpus.files) if f.family == "tiles"} <= multi or tile == 16
        # a tile that ends the file short of its length, and one that is whole
        assert any((kc.n_slices(int(corpus.lens[f])) - j) < kc.WAVES * tile for f, j in firsts)
    f37 = next(i for i, f in enumerate(corpus.files) if f.name == "tiles_37")
    assert [j for f, j in kc.tile_first_slices(corpus, 16) if f == f37] == [256, 512]
    # the reference's sprev at a tile start is the digest of the window the halo holds
    ref = corpus.ref()[f37]
    assert int(ref[256, 1]) == kc.rollsum_digest(corpus.data(f37), 256 * SLICE - 1)


def test_batch_mixes_the_families(corpus):
    idx = kc.batch_indices(corpus)
    assert 35 <= len(idx) <= 45 and len(set(idx)) == len(idx)
    fam = [corpus.files[i].family for i in idx]
    assert set(fam) == {"lengths", "values", "wave", "wave_tail", "tiles", "none"} and fam.count("none") == 4
    assert idx != sorted(idx)
    # the slice bases differ from the whole corpus's for the files after the first
    base = np.cumsum([0] + [kc.n_slices(int(corpus.lens[i])) for i in idx])[:-1]
    whole = np.cumsum([0] + [kc.n_slices(int(n)) for n in corpus.lens])[:-1]
    assert sum(int(base[k]) != int(whole[i]) for k, i in enumerate(idx)) >= len(idx) - 2
    # a file without slices shares its base with the next file
    k = fam.index("none")
    assert base[k] == base[k + 1]


def test_model_quotes_the_source():
    """Every source line the reference restates still occurs in the kernel
    and the engine (white space collapsed): an edit of one of them fails here
    and sends its author to k1_craft.py."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hashbox_amd", "csrc")
    ws = lambda t: re.sub(r"\s+", " ", t)  # noqa: E731
    missing = []
    for name, lines in (("hbx_kernels.hip", kc.MIRRORED), ("hbx_engine.hip", kc.MIRRORED_ENGINE)):
        with open(os.path.join(csrc, name)) as fh:
            src = ws(fh.read())
        missing += ["%s: %s" % (name, ln) for ln in lines if ws(ln) not in src]
    assert not missing, "k1_craft.py restates lines that changed:\n" + "\n".join(missing)
    with open(os.path.join(csrc, "hbx_device.h")) as fh:
        assert "constexpr uint32_t kSlice = 4096u;" in ws(fh.read())
