"""Every slice summary K1 stores, read back through hbx_k1_summaries and
compared word for word with the per-position reference of tests/k1_craft.py
(oracle.digest_all alone): smax and sprev of all slices of the corpus, at K1
tiles of the default length, 1, 3 and 16 iterations with both LDS images, with
one DMA statement per piece and with the first DMA after the halo's loads, and
as a batch of about 40 files in another order.  The same call's cuts and IDs
are held against oracle.store_file as the parity tests do.
tests/test_k1_craft.py shows on the CPU that the corpus has the lengths,
tails, wraps and tile starts this relies on.  A failure names file, slice,
tile, iteration and wave, the word that differs, and for smax whether the
device's value is the maximum over a range one position or 16 bytes longer.

Out of scope here: the pipelined and the segment paths run the same kernel
from the same plan and keep their cut-level tests (hbx_k1_summaries answers
for synchronous batches only); files past 2^32 bytes would make the corpus
4 GiB (test_one_file_past_4_gib stays their witness); the K1 variants under
tools/variants/ were removed from the product.
"""
import numpy as np
import pytest

from . import k1_craft as kc

pytestmark = pytest.mark.gpu


class Dev:
    """The corpus on the device, its reference summaries and store_file results."""

    def __init__(self, oracle):
        import torch
        self.c = kc.corpus()
        self.t = torch.from_numpy(self.c.host).to("cuda:0")
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 64 == 0, "the designed offsets assume a 64-aligned arena"
        self.ptr = self.t.data_ptr()
        self.ref = self.c.ref()
        self.store = [oracle.store_file(self.c.data(f), fast=True) for f in range(len(self.c.files))]


@pytest.fixture(scope="module")
def dev(oracle):
    d = Dev(oracle)
    yield d
    d.t = None


def differences(dev, e, idx, tile):
    """Run files `idx` of the corpus as one synchronous device batch on engine
    `e`; [] if every summary word, cut and ID is the reference's."""
    c = dev.c
    got = e.chunk_hash_device(dev.ptr, c.offs[idx], c.lens[idx])
    first, count, pairs = e.k1_summaries()
    lines = []
    want_count = [kc.n_slices(int(c.lens[f])) for f in idx]
    want_first = np.cumsum([0] + want_count)[:-1]
    if count.tolist() != want_count or first.tolist() != want_first.tolist() or pairs.shape != (sum(want_count), 2):
        return ["slice bookkeeping: %d files, counts %s..., firsts %s..., %d pairs; expected %d files, %s..., %s..., %d" % (
            len(count), count.tolist()[:8], first.tolist()[:8], pairs.shape[0], len(idx), want_count[:8],
            want_first.tolist()[:8], sum(want_count))]
    wrong = 0
    for k, f in enumerate(idx):
        g, r = got[k], dev.store[f]
        if not (np.array_equal(g.cut_ends, r.cut_ends) and np.array_equal(g.ids, r.ids)
                and g.content_id == r.content_id and g.content_type == r.content_type):
            lines.append("%s: cuts or ids differ from oracle.store_file" % c.files[f].name)
        have = pairs[int(first[k]):int(first[k]) + want_count[k]]
        bad = np.argwhere(have != dev.ref[f])
        wrong += len(bad)
        ext = None
        for j, word in bad.tolist():
            if len(lines) >= 12:
                break
            line = "%s: %s expected %#010x got %#010x" % (kc.describe(c, f, j, tile), ("smax", "sprev")[word],
                                                          int(dev.ref[f][j, word]), int(have[j, word]))
            if word == 0:
                ext = c.extended(f) if ext is None else ext
                lo, hi = kc.SLICE * j, min(kc.SLICE * (j + 1), int(c.lens[f]))
                if int(have[j, 0]) == int(ext[lo:hi + 1].max()):
                    line += " = the maximum over one position more"
                elif int(have[j, 0]) == int(ext[lo:hi + 16].max()):
                    line += " = the maximum over 16 bytes more"
            lines.append(line)
    if wrong:
        lines.append("%d summary words differ in all" % wrong)
    return lines


def open_engine(monkeypatch, tile_iters, **env):
    from hashbox_amd import Engine
    monkeypatch.setenv("HBX_AB", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    e = Engine(0, tile_iters=tile_iters)
    k = e.knobs()
    assert k["ab_env"] == 1 and k["tile_iters"] == tile_iters
    assert k["k1_swz"] == int(env.get("HBX_K1_SWZ", 1)) and k["k1_dma4"] == int(env.get("HBX_K1_DMA4", 1))
    assert k["k1_early"] == int(env.get("HBX_K1_EARLY", 1))
    return e


def check(lines):
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("swz", [0, 1])
@pytest.mark.parametrize("tile_iters", [0, 1, 3, 16])
def test_every_summary_at_tile_sizes(monkeypatch, dev, tile_iters, swz):
    """The whole corpus in one call.  Tile length 0 sizes tiles per batch: 16
    iterations, the least, for a corpus this small."""
    with open_engine(monkeypatch, tile_iters, HBX_K1_SWZ=swz) as e:
        check(differences(dev, e, list(range(len(dev.c.files))), tile_iters or 16))


@pytest.mark.parametrize("switch", ["HBX_K1_DMA4", "HBX_K1_EARLY"])
def test_every_summary_with_a_dma_switch_off(monkeypatch, dev, switch):
    with open_engine(monkeypatch, 3, **{switch: 0}) as e:
        check(differences(dev, e, list(range(len(dev.c.files))), 3))


def test_batch_of_forty_in_another_order(monkeypatch, dev):
    """A fresh engine at the defaults (asserted: no K1 switch of the
    environment applies): files of every family and files without slices in
    another order, so each file's slice base is another than in the corpus;
    then the corpus and the reversed batch on the same context (the other
    summary slot, other bases again)."""
    from hashbox_amd import Engine
    monkeypatch.setenv("HBX_AB", "1")
    for name in ("HBX_K1_SWZ", "HBX_K1_DMA4", "HBX_K1_EARLY"):
        monkeypatch.delenv(name, raising=False)
    idx = kc.batch_indices(dev.c)
    with Engine(0) as e:
        k = e.knobs()
        assert k["ab_env"] == 1 and k["tile_iters"] == 0
        assert (k["k1_swz"], k["k1_dma4"], k["k1_early"]) == (1, 1, 1)
        check(differences(dev, e, idx, 16))
        check(differences(dev, e, list(range(len(dev.c.files))), 16))
        check(differences(dev, e, idx[::-1], 16))
