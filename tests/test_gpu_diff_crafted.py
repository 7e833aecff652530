"""GPU: the byte comparison behind diff (hbx_k10_diff, hbx_k11_diff and the
host code that merges their words) on the designed corpus of
tests/diff_craft.py: competing differences inside a granule, a lane, a wave,
a workgroup, a file, a pass and a window, every local alignment and every
block length 1..48.  The expected answer is the plain numpy reference's
(diffFileData, hashback/restore.go:249-277); tests/test_diff_craft.py holds
the corpus against it and asserts what each family covers.

Every case is compared in every run.  With each answer the per-block status
and the number of good blocks are asserted, so that no answer passes because
nothing was compared.  A failure lists the cases that broke, at most a
dozen, with the model's verdict: where the expected byte lies and which
candidate the kernel seems to have taken instead.

formats.diff_tree hands every file whose size matches to Engine.diff_files
and adds no path of its own to the comparison, so it is not run here.
"""
import collections

import numpy as np
import pytest

from . import diff_craft as dc

pytestmark = pytest.mark.gpu

SHOWN = 12


@pytest.fixture(scope="module")
def corpus():
    return dc.k11_corpus()


def fail_report(what, broken, total):
    if not broken:
        return
    per = collections.Counter(b[0] for b in broken)
    lines = ["%s: %d of %d cases broke (%s)" % (what, len(broken), total,
                                               ", ".join("%s %d" % kv for kv in sorted(per.items())))]
    for fam, name, text in broken[:SHOWN]:
        lines.append("  [%s] %s: %s" % (fam, name, text))
    pytest.fail("\n".join(lines), pytrace=False)


def status_problem(seg, case, status, n_good):
    """The per-block status and n_good against the model: None if right."""
    want_ok = seg.status if seg is not None else []
    got = [int(s) for s in status]
    if [s == 0 for s in got] != want_ok or int(n_good) != (seg.n_good if seg is not None else 0):
        return "status %s n_good %d, expected ok=%s n_good %d" % (got, int(n_good), want_ok, seg.n_good if seg else 0)
    if case.bad is not None:
        s = got[case.bad[0]]
        if (case.bad[1] == "wrong_id" and s != 7) or (case.bad[1] == "truncated" and not 1 <= s <= 6):
            return "block %d (%s) has status %d" % (case.bad[0], case.bad[1], s)
    return None


# ------------------------------------------------------------------ K11 ---
@pytest.mark.parametrize("mode", ["r", "z"])
def test_k11_whole_corpus_in_one_call(engine, corpus, mode):
    """Every family in one hbx_restore_files_blocks call: one window, one
    pass, one hbx_k11_diff launch, one word per file."""
    chains = corpus.chains(mode)
    lay = corpus.layout(mode, chains)
    hints = [len(c.data) for c in corpus.cases]  # (exact: small inflate slots, no stream outgrows its own)
    r = engine.restore_files_blocks(chains, size_hints=hints, local=corpus.locals(), max_block=dc.MAX_BLOCK)
    w, p, again = engine.knobs()["restore_many"]
    # (a truncated stream may run into the end of its hinted slot and is then inflated again at max_block)
    assert (w, p) == (1, 1) and again <= sum(c.bad is not None and c.bad[1] == "truncated" for c in corpus.cases), \
        "the model lays out one pass"
    assert r.data is None and len(r.first_diff) == len(corpus.cases)
    broken = []
    for f, c in enumerate(corpus.cases):
        seg = lay.segs.get(f)
        bad = status_problem(seg, c, r.status[f], r.n_good[f])
        got = r.first_diff[f]
        if bad is None and got == c.want:
            continue
        text = "expected %s, got %s" % (c.want, got)
        if got != c.want:
            text += "; " + dc.verdict(lay.by_file.get(f, []), dc.T11, c.restored(), c.local, c.want, got)
        if bad:
            text += "; " + bad
        broken.append((c.family, c.name, text))
    fail_report("K11, %s blocks" % ("raw" if mode == "r" else "zlib"), broken, len(corpus.cases))


def _files_stream(engine, wired, ids, paths, hints, wb, mb):
    """Engine.diff_files with each file's n_good, bytes and bad block."""
    return engine._restore_files_stream(ids, lambda f, i: wired[f][i][:2], None, paths, hints, wb, 4, mb)


def test_f_on_real_files_through_diff_files(engine, corpus, tmp_path):
    """Family F (files sharing workgroups, files of no blocks, shorter and
    longer local copies, bad blocks) as files on disk through
    hbx_restore_files_stream, raw and zlib files in turn."""
    cases = [c for c in corpus.cases if c.family == "F"]
    wired = [dc.wire(c, "rz"[k % 2]) for k, c in enumerate(cases)]
    lay = dc.k11_layout([dc.blks_of(c, w) for c, w in zip(cases, wired)], [len(c.local) for c in cases])
    paths = []
    for k, c in enumerate(cases):
        paths.append(tmp_path / ("f%03d.bin" % k))
        paths[-1].write_bytes(c.local)
    ids = [[b[2] for b in w] for w in wired]
    hints = [len(c.data) for c in cases]
    res = _files_stream(engine, wired, ids, paths, hints, 16 << 20, dc.MAX_BLOCK)
    broken = []
    for f, (c, r) in enumerate(zip(cases, res)):
        seg = lay.segs.get(f)
        want = (c.want, seg.n_good if seg else 0, len(c.restored()), c.bad[0] if c.bad else None, 0)
        got = (r.first_diff, r.n_good, r.bytes, r.bad_index, r.errno)
        if got != want:
            broken.append((c.family, c.name, "expected (first_diff, n_good, bytes, bad_index, errno) %s, got %s; %s" % (
                want, got, dc.verdict(lay.by_file.get(f, []), dc.T11, c.restored(), c.local, c.want, r.first_diff))))
    fail_report("F through diff_files", broken, len(cases))
    same = engine.diff_files(ids, lambda f, i: wired[f][i][:2], paths, size_hints=hints, window_bytes=16 << 20,
                             io_threads=4, max_block=dc.MAX_BLOCK)
    assert same == [(c.want is None and c.bad is None, c.want) for c in cases]


# -------------------------------------------------- windows and passes ---
def test_x_windows_through_diff_file(engine, tmp_path):
    """Two blocks a window: a flip in the second window only, the third only,
    the first and third, and each.  The first window that differs wins, and
    the call compared everything before it."""
    xs = dc.x_set()
    wb = 2 * dc.restore_stride(dc.X_MB)
    offs = np.concatenate([[0], np.cumsum(dc.X_BLOCKS)]).tolist()
    src = lambda i: xs.wired[i]  # noqa: E731
    broken = []
    for name, (loc, want) in xs.locals.items():
        path = tmp_path / (name + ".bin")
        path.write_bytes(loc)
        got = engine.diff_file(xs.ids, src, path, window_bytes=wb, max_block=dc.X_MB)
        nbytes, _ = engine._restore_stream(xs.ids, src, None, None, path, wb, dc.X_MB)
        done = offs[-1] if want is None else offs[2 * dc.x_window_of(want) + 2]  # through the window that differs
        if got != (want is None, want) or nbytes != done:
            broken.append(("X", name, "expected %s after %d bytes, got %s after %d (flips in windows %s)" % (
                want, done, got[1], nbytes, [dc.x_window_of(x) for x in xs.flips[name]])))
    fail_report("X through diff_file", broken, len(xs.locals))


def test_x_passes_through_diff_files(engine, tmp_path):
    """The same file between twenty small ones, four passes: its first block
    behind ten files of the first pass (segment index and loff not zero), its
    last in front of ten others (foff0 not zero beside them); flips in the
    small files of both passes compete for their own words only."""
    xs = dc.x_set()
    files, wired, ids = dc.x_files()
    wb = dc.X_WB
    passes = dc.x_passes(files, wired, wb)
    hints = [sum(len(b) for b in f) for f in files]
    whole = [b"".join(f) for f in files]
    big = 10
    paths = [tmp_path / ("x%02d.bin" % k) for k in range(len(files))]
    broken = []
    for name, (loc, want) in xs.locals.items():
        local = list(whole)
        local[big] = loc
        wants = [None] * len(files)
        wants[big] = want
        if name != "same":  # small files of the first and the last pass, and one a byte short
            for f, at in ((3, 0), (7, len(whole[7]) - 1), (12, 17), (20, len(whole[20]) - 1)):
                local[f] = dc.flipped(np.frombuffer(whole[f], np.uint8), [at], 0x40)
                wants[f] = at
            local[15] = whole[15][:-1]
            wants[15] = len(whole[15]) - 1
        for p, b in zip(paths, local):
            p.write_bytes(b)
        res = _files_stream(engine, wired, ids, paths, hints, wb, dc.X_MB)
        w, p, again = engine.knobs()["restore_many"]
        assert (w, p, again) == (len(passes), len(passes), 0) and len(passes) == 4
        for f, r in enumerate(res):
            got = (r.first_diff, r.n_good, r.bytes, r.bad_index, r.errno)
            exp = (wants[f], len(files[f]), len(whole[f]), None, 0)
            if got != exp:
                broken.append(("X", "%s, file %d" % (name, f), "expected %s, got %s (flips %s)" % (
                    exp, got, xs.flips[name] if f == big else "")))
    fail_report("X through diff_files", broken, 5 * len(files))


# ------------------------------------------------------------------ K10 ---
@pytest.mark.parametrize("family", ["L", "W", "WG", "S", "HT", "G"])
def test_k10_calls(engine, family):
    """One hbx_restore_blocks call per case: K10 has one word per call."""
    calls = [k for k in dc.k10_calls() if k.case.family == family]
    assert len(calls) == dc.STATED["k10"][family]
    broken = []
    for k in calls:
        chain = k.chain()
        r = engine.restore_blocks([b[1] for b in chain], [b[0] for b in chain], [b[2] for b in chain], local=k.local())
        want = k.want()
        ok = r.n_good == len(chain) and r.status.tolist() == [0] * len(chain) and r.data is None
        if ok and r.first_diff == want:
            continue
        lay = k.layout(chain)
        text = "expected %s, got %s; %s" % (want, r.first_diff, dc.verdict(lay.pieces, dc.T10, k.restored(), k.local(),
                                                                          want, r.first_diff))
        if not ok:
            text += "; status %s n_good %d" % (r.status.tolist(), r.n_good)
        broken.append((family, k.case.name, text))
    fail_report("K10 family %s" % family, broken, len(calls))


def test_k10_bad_block_and_lengths(engine, corpus):
    """Family F's shorter and longer local copies and bad blocks through
    hbx_restore_blocks: `cover` cuts the last piece, the prefix rule drops a
    word from behind the bad block, the length rule answers otherwise."""
    cases = [c for c in corpus.cases if c.family == "F" and c.tag[0] in ("short", "long", "bad")]
    assert len(cases) == 22
    broken = []
    for n, c in enumerate(cases):
        chain = dc.wire(c, "rz"[n % 2])
        lay = dc.k10_layout(dc.blks_of(c, chain), len(c.local))
        r = engine.restore_blocks([b[1] for b in chain], [b[0] for b in chain], [b[2] for b in chain], local=c.local,
                                  max_block=dc.MAX_BLOCK)
        bad = status_problem(lay.segs[0], c, r.status, r.n_good)
        if bad is None and r.first_diff == c.want:
            continue
        broken.append((c.family, c.name, "expected %s, got %s; %s; %s" % (
            c.want, r.first_diff, dc.verdict(lay.pieces, dc.T10, c.restored(), c.local, c.want, r.first_diff), bad)))
    fail_report("K10, lengths and bad blocks", broken, len(cases))
