"""The crafted MD5 chains (tests/md5_craft.py) through every door of the
block-ID code, bit-exact against hashlib: K6 (verify_blocks_device), K6p and
K3 / K3P / K3Q (verify_submit_device), the chunking path (submit_device) and
K5 / K5r (block_id, md5).  Blocks lie at every byte alignment in arenas of
non-zero filler, waves are composed by design (tests/test_md5_craft.py shows
on the CPU which lane classes each family reaches), and where a batch is one
group hashed in one launch the K3 probe confirms the wave's R and largest
count.  Every designed chain is compared in every run; a failure names the
lane classes that broke.
"""
import hashlib

import numpy as np
import pytest

from . import md5_craft as mc

pytestmark = pytest.mark.gpu


class Dev:
    """A case set with its arena on the device."""

    def __init__(self, cs):
        import torch
        self.cs = cs
        self.t = torch.from_numpy(cs.host).to("cuda:0")
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 64 == 0, "the designed addresses assume a 64-aligned arena"
        self.ptr = self.t.data_ptr()
        self.ref = cs.ref()

    def args(self, idx):
        cs = self.cs
        return (self.ptr, cs.offs[idx], cs.lens[idx], [cs.links[i] for i in idx])

    def bad(self, idx, ids, door):
        """[] if ids (one row per block of idx) are the reference's, else a
        summary by lane class and the first wrong blocks in full."""
        assert len(ids) == len(idx)
        wrong = [i for k, i in enumerate(idx) if ids[k].tobytes() != self.ref[i]]
        if not wrong:
            return []
        by = {}
        for i in wrong:
            by[self.cs.specs[i].cls] = by.get(self.cs.specs[i].cls, 0) + 1
        out = ["%s: %d of %d block ids differ" % (door, len(wrong), len(idx))]
        out += ["  %s: %d wrong" % kv for kv in sorted(by.items())[:32]]
        out += ["  " + self.cs.describe(i) for i in wrong[:8]]
        return out


@pytest.fixture(scope="module")
def dev():
    d = {"A": Dev(mc.family_a()), "B": Dev(mc.family_b()), "C": Dev(mc.family_c())}
    yield d
    d.clear()


def check(lines):
    assert not lines, "\n".join(lines)


# ------------------------------------------------------------------- K6 --
def test_k6_every_residue_at_every_alignment(engine, dev):
    a = dev["A"]
    idx = a.cs.groups["all"]
    ids, ok, bad = engine.verify_blocks_device(*a.args(idx), expect=[a.ref[i] for i in idx])
    check(a.bad(idx, ids, "K6 family A"))
    assert ok.all() and bad == 0


@pytest.mark.parametrize("L", mc.B_LINKS)
def test_k6_uniform_waves(engine, dev, L):
    b = dev["B"]
    idx = b.cs.groups["L%d" % L]
    ids, _, _ = engine.verify_blocks_device(*b.args(idx))
    check(b.bad(idx, ids, "K6 family B"))


def test_k6_mixed_groups(engine, dev):
    c = dev["C"]
    lines = []
    for g, idx in c.cs.groups.items():
        ids, ok, bad = engine.verify_blocks_device(*c.args(idx), expect=[c.ref[i] for i in idx])
        lines += c.bad(idx, ids, "K6 group " + g)
        assert bad == int((~ok).sum())
    check(lines)


# ------------------------------------------------------------------- K3 --
VARIANTS = {
    #                 PROD PSETS SPIN ITEMS WGS lag
    "k3":            (0, 2, 0, 0, 0, 1),
    "k3-wgs1-lag2":  (0, 2, 0, 0, 1, 2),
    "p2":            (1, 2, 0, 0, 0, 1),
    "p2-wgs1-lag2":  (1, 2, 0, 0, 1, 2),
    "p3":            (1, 3, 0, 0, 0, 1),
    "p3-wgs1":       (1, 3, 0, 0, 1, 1),
    "p3-spin-wgs1":  (1, 3, 1, 0, 1, 1),
    "q2":            (1, 2, 0, 2, 0, 1),
    "q4-wgs1-lag2":  (1, 2, 0, 4, 1, 2),
}


def open_engine(monkeypatch, variant, md5_slice):
    from hashbox_amd import Engine
    prod, psets, spin, items, wgs, lag = VARIANTS[variant]
    monkeypatch.setenv("HBX_AB", "1")
    monkeypatch.setenv("HBX_K3_PROD", str(prod))
    monkeypatch.setenv("HBX_K3_PSETS", str(psets))
    monkeypatch.setenv("HBX_K3_SPIN", str(spin))
    monkeypatch.setenv("HBX_K3_ITEMS", str(items))
    if wgs:
        monkeypatch.setenv("HBX_K3_WGS", str(wgs))
    e = Engine(0, md5_slice=md5_slice, join_lag=lag)
    k = e.knobs()
    assert k["ab_env"] == 1 and k["k3_prod"] == prod and k["k3_psets"] == psets and k["k3_spin"] == spin
    assert k["k3_items"] == items and k["join_lag"] == lag and k["md5_slice"] == md5_slice
    assert not wgs or k["md5_wgs"] == wgs
    return e


def launches(e):
    import torch
    torch.cuda.synchronize()
    return int(e.stage_totals()[1][3])


def pace(e, a, lag):
    """One more submit, so that the next K3 launch happens: at join lag 1 a
    batch of no blocks, at lag 2 (where only batches with chains age the
    queue) one tiny block.  Returns (need, n) for the schedule model."""
    if lag == 1:
        e.verify_submit_device(a.ptr, [], [])
        return (1, 0)
    e.verify_submit_device(*a.args([0]))
    return (1, 1)


def test_k3_family_a_through_the_lane_path(engine, dev):
    """K6p finishes the blocks whose tail holds prefix bytes; the rest are K3
    chains of at most 4 blocks: md5_run from block 0 and from block hb, and
    md5_tail, at every alignment."""
    a = dev["A"]
    idx = a.cs.groups["all"]
    engine.verify_submit_device(*a.args(idx))
    ids, _, _ = engine.wait()
    check(a.bad(idx, ids, "K6p + K3 family A"))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_k3_uniform_waves_and_mixed_groups(monkeypatch, dev, variant):
    """B: the three L sets as three batches, each hashed by one launch at a
    budget that bins every class apart, so a K3 group is a class (with one
    workgroup, a wave walks seven of them: both LDS halves, every arm of the
    producer's loop).  A: one drained batch, all on the lane path.  C: each
    designed group as a batch of its own, hashed by one launch: the drain
    (unlimited budget), or for the K3Q variants, whose kernel only runs below
    that, a paced launch at the variant's budget (parts of 64 blocks, which
    the parts-* groups cross).  The probe's R and largest count of wave 0
    must be the model's for the first part; n65 (two groups, their order the
    planner's) has no such witness."""
    items, lag = VARIANTS[variant][3], VARIANTS[variant][5]
    budget = 64 * max(1, items)
    a, b, c = dev["A"], dev["B"], dev["C"]
    lines = []
    with open_engine(monkeypatch, variant, budget) as e:
        e.set_k3_probe(True)
        n0 = launches(e)
        sched = []
        for L in mc.B_LINKS:
            idx = b.cs.groups["L%d" % L]
            e.verify_submit_device(*b.args(idx))
            sched.append((mc.k3_need([b.cs.paths[i] for i in idx], budget), len(idx)))
        for _ in range(lag):
            sched.append(pace(e, a, lag))
        for L in mc.B_LINKS:
            idx = b.cs.groups["L%d" % L]
            lines += b.bad(idx, e.wait()[0], "K3 %s family B" % variant)
        for _ in range(lag):
            e.wait()
        assert e.pending() == 0
        assert launches(e) - n0 == mc.k3_launches(sched, lag)
        idx = a.cs.groups["all"]
        e.verify_submit_device(*a.args(idx))
        lines += a.bad(idx, e.wait()[0], "K3 %s family A" % variant)
        for g, idx in c.cs.groups.items():
            n0, sched = launches(e), [(mc.k3_need([c.cs.paths[i] for i in idx], budget), len(idx))]
            e.verify_submit_device(*c.args(idx))
            if items:
                assert sched[0][0] == 1
                sched += [pace(e, a, lag) for _ in range(lag)]
            ids, _, _ = e.wait()
            lines += c.bad(idx, ids, "K3 %s group %s" % (variant, g))
            if len(idx) <= 64:  # before the pacing batches' drains write the probe again
                w = mc.k3_wave(mc.k3q_parts(c.cs.k3_counts(idx), budget, items)[0])
                word = int(e.k3_wave_times()[0][3])
                got = (word & 0xFFFF, (word >> 16) & 0xFFFF)
                if got != (w.probe_R, w.probe_max):
                    lines.append("K3 %s group %s: wave 0 ran R=%d max=%d, designed R=%d max=%d" % (
                        (variant, g) + got + (w.probe_R, w.probe_max)))
            while e.pending():
                e.wait()
            if items and launches(e) - n0 != mc.k3_launches(sched, lag):
                lines.append("K3 %s group %s: %d K3 launches, the model says %d" % (
                    variant, g, launches(e) - n0, mc.k3_launches(sched, lag)))
    check(lines)


@pytest.mark.parametrize("variant", ["k3", "p2", "p3", "p3-spin-wgs1"])
@pytest.mark.parametrize("md5_slice", mc.D_SLICES)
def test_k3_slices(monkeypatch, dev, md5_slice, variant):
    """D: the groups of C and a few classes of B time-sliced: the remainder
    slice first (1 and 7 blocks on the lane path, 8 and a whole slice
    cooperative), chains of one group finishing in different launches.
    Submits of no blocks pace the launches; their number must be the
    model's.  (K3Q needs a slice of 64 blocks per item, so it is not here.)"""
    a = dev["A"]
    lines = []
    with open_engine(monkeypatch, variant, md5_slice) as e:
        for cs, name, idx in mc.d_groups(dev["B"].cs, dev["C"].cs):
            d = dev[cs.name]
            need = mc.k3_need([cs.paths[i] for i in idx], md5_slice)
            n0 = launches(e)
            e.verify_submit_device(*d.args(idx))
            sched = [(need, len(idx))] + [pace(e, a, 1) for _ in range(need + 1)]
            ids, _, _ = e.wait()
            while e.pending():
                e.wait()
            lines += d.bad(idx, ids, "K3 %s slice %d %s" % (variant, md5_slice, name))
            got, want = launches(e) - n0, mc.k3_launches(sched, 1)
            assert want == need
            if got != want:
                lines.append("slice %d %s: %d K3 launches, the model says %d" % (md5_slice, name, got, want))
    check(lines)


# ------------------------------------------------------ the chunking door --
@pytest.mark.parametrize("md5_slice", [0, 64])
def test_chunking_door_agrees(oracle, dev, md5_slice):
    """E: what the store path can produce: one-chunk files at 16-aligned,
    not 64-aligned offsets, here in a filler arena; against oracle.store_file
    and against the reference the verify door is held to."""
    import torch
    from hashbox_amd import Engine
    host, offs, lens = mc.family_e(dev["B"].cs)
    t = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 64 == 0
    with Engine(0, md5_slice=md5_slice) as e:
        e.submit_device(t.data_ptr(), offs, lens)
        if md5_slice:
            e.verify_submit_device(t.data_ptr(), [], [])  # the launch at this slice
        got = e.wait()
        while e.pending():
            e.wait()
    lines = []
    for k, (o, n, g) in enumerate(zip(offs.tolist(), lens.tolist(), got)):
        f = host[o:o + n]
        r = oracle.store_file(f, fast=True)
        same = (np.array_equal(g.cut_ends, r.cut_ends) and np.array_equal(g.ids, r.ids)
                and g.content_id == r.content_id and g.content_type == r.content_type)
        if not same or g.ids[0].tobytes() != mc.ref_id(f.tobytes()):
            lines.append("file %d (offset %d, %d bytes, %s): differs" % (k, o, n, mc.chain_path(0, n)))
    check(lines[:12])


# ---------------------------------------------------------------- K5, K5r --
def test_block_id_and_md5_sweeps(engine):
    """F: hbx_block_id at every message length 48..200 (K5 below 64 bytes,
    K5r with md5_run's tail from there) and hbx_md5 at every length 0..200."""
    rng = np.random.default_rng(606)
    lines = []
    for L in mc.F_LINKS:
        links = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(L)]
        for msg in mc.F_MSG:
            n = msg - 8 - 16 * L
            if n < 0:
                continue
            d = rng.integers(1, 256, n, dtype=np.uint8)
            if engine.block_id(d, links) != mc.ref_id(d.tobytes(), links):
                lines.append("block_id: L=%d len=%d (message %d bytes) differs" % (L, n, msg))
    for n in range(0, 201):
        d = rng.integers(1, 256, n, dtype=np.uint8)
        if engine.md5(d) != hashlib.md5(d.tobytes()).digest():
            lines.append("md5: %d bytes differs" % n)
    check(lines[:12])
