"""GPU: the device inflate (K8: a wave per stream, a lane per stream, and the
split path) on hand-built deflate streams: distances up to the full window,
copies at every short distance and lane phase, block headers at chosen bits
and across the input staging, code lengths up to 15 bits, and one specific
invalid stream per documented status (include/hbxgpu.h).

tests/deflate_craft.py builds the cases and test_deflate_craft.py holds them
against CPython's zlib, so here the device is only compared with the table:
status, length and bytes, all exact.  Every stream has its own output slot in
an arena filled with 0xA5, and no byte outside the length a stream reports
may change, for good and bad streams alike.
"""
import numpy as np
import pytest

from tests import deflate_craft as C

pytestmark = pytest.mark.gpu

CANARY = 0xA5


@pytest.fixture(autouse=True, params=["wave", "lane", "split"])
def k8_mode(request, monkeypatch):
    """Every decoder (as in test_gpu_inflate.py): split takes every stream of
    at least two regions, the wave kernel the rest."""
    monkeypatch.setenv("HBX_AB", "1")
    monkeypatch.setenv("HBX_K8_MODE", request.param)
    return request.param


def inflate_cases(engine, cases):
    """One inflate_blocks_device call over the cases; checks every case and
    the arena around every slot."""
    import torch
    n = len(cases)
    in_lens = np.array([len(c.stream) for c in cases], np.uint64)
    in_offs = np.zeros(n, np.uint64)
    in_offs[1:] = np.cumsum((in_lens[:-1] + 255) // 256 * 256)
    host = np.zeros(int(in_offs[-1] + in_lens[-1]) + 64, np.uint8)
    for c, o in zip(cases, in_offs.tolist()):
        host[o:o + len(c.stream)] = np.frombuffer(c.stream, np.uint8)
    caps = np.array([c.min_cap for c in cases], np.uint64)
    out_offs = np.zeros(n, np.uint64)
    out_offs[1:] = np.cumsum((caps[:-1] + 255) // 256 * 256 + 256)  # at least 256 canary bytes between slots
    out_offs += 256
    total = int(out_offs[-1] + caps[-1]) + 256
    dev = torch.device("cuda", engine.device)
    d_in = torch.from_numpy(host).to(dev)
    d_out = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    out_lens, st = engine.inflate_blocks_device(d_in.data_ptr(), in_offs, in_lens, d_out.data_ptr(), out_offs, caps)
    out = d_out.cpu().numpy()
    untouched = np.ones(total, bool)  # where the canary must still stand
    wrong = []
    for c, o, ln, s, cap in zip(cases, out_offs.tolist(), out_lens.tolist(), st.tolist(), caps.tolist()):
        if ln > cap:
            wrong.append(f"{c.name}: reports {ln} bytes in a slot of {cap}")
            continue
        untouched[o:o + ln] = False
        if c.status == C.ANY_ERROR:
            if s == 0:
                wrong.append(f"{c.name}: status 0, want an error")
        elif s != c.status:
            wrong.append(f"{c.name}: status {s}, want {c.status}")
        elif s == 0 and (ln != len(c.expected) or out[o:o + ln].tobytes() != c.expected):
            wrong.append(f"{c.name}: {ln} bytes, want {len(c.expected)}" if ln != len(c.expected)
                         else f"{c.name}: bytes differ")
    assert not wrong, f"{len(wrong)} of {n}: " + "; ".join(wrong[:12])
    spoiled = np.flatnonzero(untouched & (out != CANARY))
    if spoiled.size:
        at = int(spoiled[0])
        k = int(np.searchsorted(out_offs, at, side="right")) - 1
        pytest.fail(f"{spoiled.size} bytes written outside the reported output, the first at slot offset "
                    f"{at - int(out_offs[k])} of {cases[k].name} (reports {int(out_lens[k])}, cap {int(caps[k])})")
    return out_lens, st


def test_copy_grid_and_chains(engine):
    inflate_cases(engine, C.copy_grid() + C.chains())


def test_far_distances(engine):
    inflate_cases(engine, C.far())


def test_block_structure(engine):
    inflate_cases(engine, C.structure())


def test_rejections_have_the_documented_status(engine):
    inflate_cases(engine, C.rejections())


def test_split_resolves_crafted_streams(engine, k8_mode):
    """Matches that reach before their region, across the LDS ring's edge, and
    block starts at every bit offset: exact in every mode, and in split mode
    decoded by the split path itself (the engine's counters), not handed back."""
    cases = C.split_good()
    k0 = engine.knobs()
    inflate_cases(engine, cases + C.split_short())
    k1 = engine.knobs()
    if k8_mode == "split":
        assert k1["k8_split_streams"] - k0["k8_split_streams"] == len(cases)
        assert k1["k8_split_fallbacks"] - k0["k8_split_fallbacks"] == 0, (k0, k1)


def test_split_may_fall_back_but_stays_exact(engine):
    inflate_cases(engine, C.split_may_fall_back())
