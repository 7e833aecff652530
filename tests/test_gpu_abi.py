"""GPU: the C-ABI from plain C (tests/c/abi_driver.c mirrors INTEGRATION.md's
cgo stub) and the ABI's state rules, bit-exact against the oracle."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["random", "constant", "tiny"])
def test_plain_c_driver_matches_oracle(oracle, tmp_path, kind):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), f"OUT={tmp_path}"], check=True)
    data = {"random": oracle.random_bytes(21 * 1024 * 1024 + 77, 91),
            "constant": np.full(17 * 1024 * 1024 + 5, 0x33, np.uint8),
            "tiny": np.frombuffer(b"hello", np.uint8)}[kind]
    f = tmp_path / "in.bin"
    data.tofile(f)
    r = subprocess.run([str(tmp_path / "abi_driver"), str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert "ok" in lines
    ref = oracle.store_file(data, fast=True)
    want = [f"{int(c)} {bytes(i).hex()}" for c, i in zip(ref.cut_ends, ref.ids)]
    assert [x[5:] for x in lines if x.startswith("sync ")] == want
    assert [x[6:] for x in lines if x.startswith("async ")] == want
    assert f"content {ref.content_type} {ref.content_id.hex()}" in lines


def test_state_rules(oracle):
    """The slice is fixed while batches are pending (their launch counts were
    set at submit); a refused submit leaves nothing pending; the pipeline
    keeps going afterwards."""
    import torch
    from hashbox_amd import Engine, HbxError
    sizes = [3 << 20, 9 << 20, 131073]
    files = [oracle.random_bytes(n, 60 + i) for i, n in enumerate(sizes)]
    offs = np.array([0, 4 << 20, 14 << 20], np.uint64)
    host = np.zeros(16 << 20, np.uint8)
    for o, f in zip(offs, files):
        host[int(o):int(o) + f.size] = f
    dev = torch.from_numpy(host).to("cuda:0")
    refs = [oracle.store_file(f, fast=True) for f in files]
    with Engine(0, md5_slice=64) as e:
        e.submit_device(dev.data_ptr(), offs, sizes)
        with pytest.raises(HbxError):
            e.set_md5_slice(3)
        with pytest.raises(HbxError):  # the probe is fixed while batches are pending
            e.set_k3_probe(True)
        with pytest.raises(HbxError):  # offset not 16-byte aligned
            e.submit_device(dev.data_ptr(), offs + np.uint64(4), sizes)
        assert e.pending() == 1
        e.submit_device(dev.data_ptr(), offs, sizes)
        got = [e.wait(), e.wait()]
        assert e.pending() == 0
        e.set_md5_slice(3)  # allowed once drained
        e.set_k3_probe(True)
        e.submit_device(dev.data_ptr(), offs, sizes)
        got.append(e.wait())
        w = e.k3_wave_times()  # the probe's per-wave records of the latest K3 launch
        assert w.shape[1] == 8 and (w[:, 2] >= w[:, 0]).all()
        coop = w[w[:, 7] > 0]  # waves whose first group ran the cooperative phase: cycles advance
        assert (coop[:, 5] >= coop[:, 4]).all() and (coop[:, 6] >= (coop[:, 1] & ((1 << 56) - 1))).all()
        e.set_k3_probe(False)
        assert e.knobs()["k3_probe"] == 0
    for g in got:
        for a, r in zip(g, refs):
            assert np.array_equal(a.cut_ends, r.cut_ends) and np.array_equal(a.ids, r.ids)
            assert a.content_id == r.content_id


def test_ab_switches_need_hbx_ab(monkeypatch):
    """HBX_* A/B switches change nothing unless HBX_AB=1 (a caller's stray
    environment must not change the schedule): HBX_JOIN_LAG=3 and
    HBX_LEAN_MARKS=0 alone keep join lag 1 and lean marks."""
    from hashbox_amd import Engine
    monkeypatch.delenv("HBX_AB", raising=False)
    monkeypatch.setenv("HBX_LEAN_MARKS", "0")
    monkeypatch.setenv("HBX_JOIN_LAG", "3")
    with Engine(0) as e:
        k = e.knobs()
    assert k["ab_env"] == 0 and k["lean_marks"] == 1 and k["join_lag"] == 1, k
    monkeypatch.setenv("HBX_AB", "1")
    with Engine(0) as e:
        k = e.knobs()
    # lag 3: the next launch is preplanned on the cut stream (plan_cut 2, mode 3)
    assert k["ab_env"] == 1 and k["lean_marks"] == 0 and k["join_lag"] == 3 and k["plan_mode"] == 3, k


def test_k1_summaries_state_and_argument_rules(oracle):
    """hbx_k1_summaries answers for the latest synchronous batch only: not
    before one, not while or after a pipelined batch or a reserve; it reports
    the needed counts with HBX_ERR_CAPACITY and refuses null outputs."""
    import ctypes
    import torch
    from hashbox_amd import Engine, HbxError, _lib
    MIN = oracle.MIN_BLOCK_SIZE
    sizes = [3 * MIN + 5, 100, 2 * MIN, 2 * MIN + 1]
    offs = np.array([0, 1 << 20, 2 << 20, 3 << 20], np.uint64)
    host = np.zeros(4 << 20, np.uint8)
    for i, (o, n) in enumerate(zip(offs, sizes)):
        host[int(o):int(o) + n] = oracle.random_bytes(n, 40 + i)
    dev = torch.from_numpy(host).to("cuda:0")
    want_count = [49, 0, 0, 33]
    ERR_ARG, ERR_STATE = -1, -6
    with Engine(0) as e:
        L, ctx = e._L, e._ctx
        nf, ns = ctypes.c_uint64(5), ctypes.c_uint64(5)

        def call(first, count, max_files, pairs, max_slices, pnf=ctypes.byref(nf), pns=ctypes.byref(ns)):
            return L.hbx_k1_summaries(ctx, first, count, max_files, pnf, pairs, max_slices, pns)

        assert call(None, None, 0, None, 0) == ERR_STATE and (nf.value, ns.value) == (0, 0)  # no batch yet
        with pytest.raises(HbxError, match="HBX_ERR_STATE"):
            e.k1_summaries()
        e.chunk_hash_device(dev.data_ptr(), offs, sizes)
        assert call(None, None, 0, None, 0) == _lib.ERR_CAPACITY and (nf.value, ns.value) == (4, 82)
        first, count = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        pairs = np.full((83, 2), 0xAAAAAAAA, np.uint32)
        fp, cp, pp = first.ctypes.data, count.ctypes.data, pairs.ctypes.data
        assert call(fp, cp, 4, pp, 81) == _lib.ERR_CAPACITY and (nf.value, ns.value) == (4, 82)
        assert call(fp, cp, 3, pp, 82) == _lib.ERR_CAPACITY and (pairs == 0xAAAAAAAA).all()
        assert call(None, cp, 4, pp, 82) == ERR_ARG and call(fp, None, 4, pp, 82) == ERR_ARG
        assert call(fp, cp, 4, None, 82) == ERR_ARG
        assert call(fp, cp, 4, pp, 82, pnf=None) == ERR_ARG and call(fp, cp, 4, pp, 82, pns=None) == ERR_ARG
        assert call(fp, cp, 4, pp, 82) == 0 and (nf.value, ns.value) == (4, 82)
        assert count.tolist() == want_count and first.tolist() == [0, 49, 49, 49]
        assert (pairs[82] == 0xAAAAAAAA).all()  # nothing behind the last slice: the dummy slot stays on the device
        assert pairs[0, 1] == pairs[49, 1] == 0x80000000
        D = oracle.digest_all(host[:sizes[0]])
        assert int(pairs[48, 0]) == int(D[48 * 4096:].max()) and int(pairs[48, 1]) == int(D[48 * 4096 - 1])
        f2, c2, p2 = e.k1_summaries()  # the binding, and a second read of the same slot
        assert np.array_equal(f2, first) and np.array_equal(c2, count) and np.array_equal(p2, pairs[:82])
        e.submit_device(dev.data_ptr(), offs, sizes)
        assert call(fp, cp, 4, pp, 82) == ERR_STATE and (nf.value, ns.value) == (0, 0)  # pending
        e.wait()
        assert call(fp, cp, 4, pp, 82) == ERR_STATE  # a pipelined batch's summaries are not offered
        e.chunk_hash(host[:sizes[3]])  # hbx_chunk_hash_batch: one file
        f3, c3, p3 = e.k1_summaries()
        assert c3.tolist() == [33] and f3.tolist() == [0] and p3.shape == (33, 2)
        e.chunk_hash(host[:100])  # a batch without a slice is a batch: counts, no pairs
        f4, c4, p4 = e.k1_summaries()
        assert c4.tolist() == [0] and f4.tolist() == [0] and p4.shape == (0, 2)
        e.chunk_hash(host[:sizes[3]])
        e.reserve(2, 8, 8 << 20)  # may move the summary slots
        assert call(fp, cp, 4, pp, 82) == ERR_STATE
