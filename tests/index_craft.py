"""The store's index files (*.idx) in pure Python: the reference side of the
K17 tests.  Written from the rules in include/hbxgpu.h ("Index files"), never
the code under test: the format, THE RULE (findIXOffset), a writer that places
an ID where the rule says, restatements of the lookup, scan, mark, update,
sweep and compact loops over a list of bytearrays (one per index file, its
length is its size), and the crafted and random stores the tests run."""
import random
import struct

E, N, M, I = 1, 2, 4, 8  # Exists, NoLinks, Marked, Invalid
HEADER, SLOT, PROBES = 16, 24, 682
HOMES = 1 << 24
SLOTS_MAX = HOMES + PROBES
NONE = (1 << 64) - 1
DELETED, STAY, OBSOLETE, MOVED, ABORT = 1, 2, 3, 4, 5
OK, ERR_ARG, ERR_CAPACITY, ERR_FORMAT = 0, -1, -3, -7


def header(filetype=0x48534958, version=1) -> bytes:
    return struct.pack(">IIQ", filetype, version, 0)


def new_file(slots=0) -> bytearray:
    return bytearray(header() + bytes(SLOT * slots))


def mk_id(home: int, tag: int, mid: int = 0) -> bytes:
    """A 16-byte ID: 8 bytes of tag, 5 bytes of mid (byte 12 is its last), the home in the last three."""
    return tag.to_bytes(8, "big") + mid.to_bytes(5, "big") + home.to_bytes(3, "big")


def home(bid: bytes) -> int:
    return bid[13] << 16 | bid[14] << 8 | bid[15]


def off(slot: int) -> int:
    return HEADER + SLOT * slot


def location(mfile: int, moff: int) -> bytes:
    return ((mfile << 34) | moff).to_bytes(6, "big")


def slot_bytes(flags: int, bid: bytes, mfile: int = 0, moff: int = 0) -> bytes:
    return struct.pack(">H", flags) + bid + location(mfile, moff)


def read_slot(f: bytearray, o: int):
    """(flags, id, meta_file, meta_off) of the slot at offset o."""
    l = int.from_bytes(f[o + 18:o + 24], "big")
    return struct.unpack_from(">H", f, o)[0], bytes(f[o + 2:o + 18]), l >> 34, l & ((1 << 34) - 1)


def is_live(flags: int) -> bool:
    return bool(flags & E) and not flags & I


def put(files, f: int, s: int, flags: int, bid: bytes, mfile: int = 0, moff: int = 0):
    """Write a slot where the test wants it, lengthening the file with zeros."""
    o = off(s)
    if len(files[f]) < o + SLOT:
        files[f].extend(bytes(o + SLOT - len(files[f])))
    files[f][o:o + SLOT] = slot_bytes(flags, bid, mfile, moff)


def find(files, bid: bytes, stop_on_free: bool):
    """THE RULE: (found, file, offset)."""
    base = off(home(bid))
    f, o = 0, base
    free = None
    stop = False
    while not stop:
        if f >= len(files):
            break
        size = len(files[f])
        if o > size:
            break
        for _ in range(PROBES):
            if o >= size:
                stop = True
                break
            flags, sid = struct.unpack_from(">H", files[f], o)[0], files[f][o + 2:o + 18]
            if is_live(flags):
                if sid == bid:
                    return True, f, o
            else:
                if free is None:
                    free = (f, o)
                if stop_on_free or not flags & E:
                    stop = True
                    break
            o += SLOT
        if stop:
            break
        f += 1
        o = base
    if free is not None:
        return False, free[0], free[1]
    return False, f, o


def insert(files, bid: bytes, flags: int = E, mfile: int = 0, moff: int = 0):
    """The writer: the ID goes where findIXOffset(id, False) says, a new file
    or a longer one as writeIXEntry makes them (index.go:117-132).  Returns
    (file, offset)."""
    _found, f, o = find(files, bid, False)
    while f >= len(files):
        files.append(new_file())
    if len(files[f]) < o + SLOT:
        files[f].extend(bytes(o + SLOT - len(files[f])))
    files[f][o:o + SLOT] = slot_bytes(flags, bid, mfile, moff)
    return f, o


def ref_lookup(files, ids, stop_on_free):
    out = []
    for bid in ids:
        found, f, o = find(files, bid, stop_on_free)
        if found:
            flags, _id, mf, mo = read_slot(files[f], o)
            out.append((1, flags, f, mf, o, mo))
        else:
            out.append((0, 0, f, 0, o, 0))
    return out


STAT_FIELDS = ("slots", "n_live", "n_invalid", "n_empty", "n_marked", "n_nolinks", "n_misplaced", "first_misplaced",
               "trunc_point")
SUM_FIELDS = ("n_files", "slots", "n_live", "n_invalid", "n_empty", "n_marked", "n_nolinks", "n_misplaced",
              "n_obsolete", "n_cut_off")


def ref_scan(files):
    """(live, per_file, summary): live as tuples (id, flags, ix_file, ix_offset, meta_file, state, meta_off)."""
    live, per = [], []
    sm = dict.fromkeys(SUM_FIELDS, 0)
    sm["n_files"] = len(files)
    for f, img in enumerate(files):
        st = dict.fromkeys(STAT_FIELDS, 0)
        st["slots"] = (len(img) - HEADER) // SLOT
        st["first_misplaced"] = NONE
        st["trunc_point"] = HEADER
        for o in range(HEADER, len(img), SLOT):
            flags, bid, mf, mo = read_slot(img, o)
            if flags & I:
                st["n_invalid"] += 1
            elif not flags & E:
                st["n_empty"] += 1
            else:
                st["n_live"] += 1
                st["n_marked"] += 1 if flags & M else 0
                st["n_nolinks"] += 1 if flags & N else 0
                st["trunc_point"] = o + SLOT
                if o < off(home(bid)):
                    st["n_misplaced"] += 1
                    if st["first_misplaced"] == NONE:
                        st["first_misplaced"] = o
                found, pf, po = find(files, bid, False)
                state = 2 if not found else 0 if (pf, po) == (f, o) else 1
                sm["n_obsolete"] += state == 1
                sm["n_cut_off"] += state == 2
                live.append((bid, flags, f, o, mf, state, mo))
        per.append(st)
        for k in ("slots", "n_live", "n_invalid", "n_empty", "n_marked", "n_nolinks", "n_misplaced"):
            sm[k] += st[k]
    return live, per, sm


def ref_mark(files, ids):
    found = []
    for bid in ids:
        ok, f, o = find(files, bid, False)
        if ok:
            flags = struct.unpack_from(">H", files[f], o)[0]
            struct.pack_into(">H", files[f], o, flags | M)
        found.append(1 if ok else 0)
    return found


def ref_update(files, recs):
    """recs: 24-byte StorageIXEntry records.  (rc, status)."""
    ids = [bytes(r[2:18]) for r in recs]
    if len(set(ids)) != len(ids):
        return ERR_ARG, None
    status = []
    for r in recs:
        ok, f, o = find(files, bytes(r[2:18]), False)
        if ok:
            flags = struct.unpack_from(">H", files[f], o)[0]
            rflags = struct.unpack_from(">H", r, 0)[0]
            struct.pack_into(">H", files[f], o, (flags & ~N) | (rflags & N))
            files[f][o + 18:o + 24] = r[18:24]
        status.append(0 if ok else 1)
    return OK, status


SWEEP_FIELDS = ("n_live", "n_deleted", "n_stay", "n_obsolete", "n_moved", "n_abort", "first_abort", "swept_records",
                "n_grown")


def ref_sweep(files):
    """SweepIndexes over `files`, in place.  A dict: rc, action, moved_to,
    killed [(id, meta_file, meta_off)], summary, into_vacated (moves whose
    target an earlier step of this sweep vacated).  With an ABORT the files are
    put back."""
    saved = [bytearray(f) for f in files]
    action, moved_to, killed = [], [], []
    vacated, into_vacated = set(), 0
    for f in range(len(files)):
        size = len(files[f])
        for o in range(HEADER, size, SLOT):
            flags, bid, mf, mo = read_slot(files[f], o)
            if flags & I or not flags & E:
                continue
            to = (NONE, NONE)
            if not flags & M:
                killed.append((bid, mf, mo))
                flags |= I
                act = DELETED
            else:
                flags &= ~M
                found, pf, po = find(files, bid, True)
                if (pf, po) == (f, o):
                    act = STAY
                elif found:
                    flags |= I
                    act = OBSOLETE
                elif pf < f or (pf == f and po < o):
                    if len(files[pf]) < po + SLOT:
                        files[pf].extend(bytes(po + SLOT - len(files[pf])))
                    files[pf][po:po + SLOT] = files[f][o:o + SLOT]
                    struct.pack_into(">H", files[pf], po, flags)
                    into_vacated += (pf, po) in vacated
                    to = (pf, po)
                    flags |= I
                    act = MOVED
                else:
                    action.append(ABORT)
                    moved_to.append(to)
                    continue
            struct.pack_into(">H", files[f], o, flags)
            if flags & I:
                vacated.add((f, o))
            action.append(act)
            moved_to.append(to)
    sm = dict(n_live=len(action), n_deleted=action.count(DELETED), n_stay=action.count(STAY),
              n_obsolete=action.count(OBSOLETE), n_moved=action.count(MOVED), n_abort=action.count(ABORT),
              first_abort=action.index(ABORT) if ABORT in action else NONE, swept_records=action.count(DELETED),
              n_grown=sum(len(a) > len(b) for a, b in zip(files, saved)))
    rc = OK
    if sm["n_abort"]:
        rc = ERR_FORMAT
        sm["n_grown"] = 0
        for f in range(len(files)):
            files[f][:] = saved[f]
    return dict(rc=rc, action=action, moved_to=moved_to, killed=killed, summary=sm, into_vacated=into_vacated)


def ref_compact(files):
    """CompactIndexes over `files`, in place: (cleared, sizes)."""
    cleared = 0
    for img in files:
        trunc = HEADER
        for o in range(HEADER, len(img), SLOT):
            flags = struct.unpack_from(">H", img, o)[0]
            if flags & I:
                img[o:o + SLOT] = bytes(SLOT)
                cleared += 1
            elif flags & E:
                trunc = o + SLOT
        del img[trunc:]
    return cleared, [len(f) for f in files]


# ---------------------------------------------------------------- lookup cases --
def _strangers(files, f, h, first, count, flags=E, tag0=1000):
    """`count` valid entries of home h with IDs of their own in slots first .. of file f."""
    for k in range(count):
        put(files, f, first + k, flags, mk_id(h, tag0 + first + k), 1, 100 + k)


def lookup_cases():
    """[(name, files, ids)]: every case runs with both stop_on_free values."""
    cases = []
    # one store for the short cases, each at a home of its own
    f0 = [new_file(120)]
    ids = []
    a = mk_id(2, 1)
    put(f0, 0, 2, E | N, a, 3, 777)  # a hit at home
    ids.append(a)
    b = mk_id(10, 2)
    _strangers(f0, 0, 10, 10, 5)
    put(f0, 0, 15, E, b, 1, 5)  # behind 5 valid others
    ids.append(b)
    c = mk_id(20, 3)
    put(f0, 0, 20, E | I, mk_id(20, 99))  # Exists|Invalid in front of the hit
    put(f0, 0, 21, E | M, c, 2, 9)
    ids.append(c)
    d = mk_id(30, 4)
    put(f0, 0, 30, I, mk_id(30, 98))  # Invalid without Exists stops both
    put(f0, 0, 31, E, d)
    ids.append(d)
    e = mk_id(40, 5)
    put(f0, 0, 41, E, e)  # an empty slot in front
    ids.append(e)
    g = mk_id(50, 6)
    put(f0, 0, 50, E | I, g)  # the ID itself, invalid: no hit
    ids.append(g)
    # IDs that share the home and the first 8 bytes and differ only in byte 12
    for k in range(4):
        put(f0, 0, 60 + k, E, mk_id(60, 7, k), 0, 1000 + k)
    ids += [mk_id(60, 7, k) for k in (3, 0, 2, 1, 4)]
    # the file ends inside the run; base == size; base > size
    _strangers(f0, 0, 115, 115, 5)
    ids += [mk_id(115, 8), mk_id(120, 9), mk_id(121, 10), mk_id(5000, 11)]
    ids.append(mk_id(100, 12))  # nothing at its home
    cases.append(("short", f0, ids))
    # 682 valid strangers, then the ID in slot 683 of file 0
    h = 5
    x = mk_id(h, 50)
    one = [new_file(h + PROBES + 4)]
    _strangers(one, 0, h, h, PROBES)
    put(one, 0, h + PROBES, E, x)
    cases.append(("full_run_one_file", one, [x, mk_id(h, 51)]))  # the place is file == n_files
    two = [bytearray(one[0]), new_file(h + 8)]
    put(two, 1, h, E | N, x, 7, 70)
    cases.append(("full_run_found_in_file_1", two, [x, mk_id(h, 51)]))  # the other: file 1's empty home
    free = [bytearray(one[0]), new_file(h + 8)]
    put(free, 0, h + 300, E | I, mk_id(h, 52))  # a remembered free slot in file 0
    cases.append(("full_run_remembered_free", free, [x, mk_id(h, 51)]))
    free1 = [bytearray(free[0])]
    cases.append(("full_run_remembered_free_one_file", free1, [x, mk_id(h, 51)]))
    return cases


# ----------------------------------------------------------------- sweep cases --
def _run(files, f, h, first, count, unmarked=lambda i: i % 3 == 1, tag0=5000):
    for i in range(count):
        put(files, f, first + i, E if unmarked(i) else E | M, mk_id(h, tag0 + first + i), i % 3, 64 + i)


def sweep_cases(tile=256):
    """{name: files}."""
    c = {}
    s = [new_file(8)]
    put(s, 0, 3, E, mk_id(3, 1), 1, 2)
    c["unmarked_alone"] = s
    s = [new_file(8)]
    put(s, 0, 3, E | M | N, mk_id(3, 1), 1, 2)
    c["marked_at_home"] = s
    s = [new_file(8)]
    put(s, 0, 0, E, mk_id(0, 1), 0, 10)
    put(s, 0, 1, E | M, mk_id(0, 2), 0, 20)
    put(s, 0, 2, E | M | N, mk_id(0, 3), 0, 30)
    c["cascade"] = s
    s = [new_file(8)]
    put(s, 0, 0, E, mk_id(0, 1), 0, 10)
    put(s, 0, 1, E | M, mk_id(1, 2), 0, 20)
    put(s, 0, 2, E | M, mk_id(0, 3), 0, 30)
    c["cascade_middle_at_home"] = s
    s = [new_file(8)]
    put(s, 0, 0, E | I, mk_id(0, 1))
    put(s, 0, 1, E | M, mk_id(0, 2), 2, 5)
    c["invalid_in_front"] = s
    s = [new_file(8)]
    put(s, 0, 2, E | M | I, mk_id(2, 1), 1, 1)
    put(s, 0, 3, M | I, mk_id(2, 2), 1, 1)
    c["marked_invalid_skipped"] = s
    s = [new_file(12)]
    for k, fl in enumerate((0, N, M, N | M)):
        put(s, 0, 2 * k, fl, mk_id(2 * k, 77, k), 3, 3)
    put(s, 0, 9, 0, mk_id(9, 78), 1, 1)
    put(s, 0, 10, E | M, mk_id(9, 79), 1, 1)  # moves onto the garbage in front of it
    c["garbage_without_exists"] = s
    s = [new_file(8)]
    put(s, 0, 4, E | M, mk_id(4, 1), 0, 10)
    put(s, 0, 5, E | M, mk_id(4, 1), 0, 20)
    c["duplicate_earlier_marked"] = s
    s = [new_file(8)]
    put(s, 0, 4, E, mk_id(4, 1), 0, 10)
    put(s, 0, 5, E | M, mk_id(4, 1), 0, 20)
    c["duplicate_earlier_unmarked"] = s
    # two files: file 0's run of 682 is full
    h = 3
    s = [new_file(h + PROBES + 2), new_file(h + 6)]
    _run(s, 0, h, h, PROBES, unmarked=lambda i: i == 0)
    put(s, 1, h, E | M, mk_id(h, 1), 1, 1)
    c["file1_into_slot_freed_in_file0"] = s
    s = [new_file(h + PROBES + 2), new_file(h + 6)]
    _run(s, 0, h, h, PROBES, unmarked=lambda i: False)
    put(s, 1, h, E | M, mk_id(h, 1), 1, 1)
    put(s, 1, h + 2, E | M, mk_id(h, 2), 1, 2)  # one slot after a free slot of file 1: moves within file 1
    c["file1_stays_and_moves_within"] = s
    s = [new_file(10), new_file(60)]
    put(s, 1, 50, E | M, mk_id(50, 1), 2, 2)
    put(s, 1, 52, E | M, mk_id(52, 2), 2, 3)
    c["file1_home_past_file0_end"] = s
    s = [new_file(12)]
    put(s, 0, 2, E | M, mk_id(5, 1), 1, 1)
    put(s, 0, 7, E, mk_id(7, 2), 1, 1)
    put(s, 0, 8, E | M, mk_id(7, 3), 1, 1)
    c["abort_below_home"] = s
    s = [new_file(h + PROBES + 4)]
    _run(s, 0, h, h, PROBES, unmarked=lambda i: False)
    put(s, 0, h + PROBES, E | M, mk_id(h, 1), 1, 1)
    put(s, 0, 1, E, mk_id(1, 2), 1, 1)
    c["abort_beyond_reach"] = s
    for n in (1, 63, 64, 65, 683):
        s = [new_file(n + 20)]
        _run(s, 0, 7, 7, n)
        c[f"run_{n}"] = s
    s = [new_file(30)]
    _run(s, 0, 0, 0, 10, unmarked=lambda i: i % 2 == 0)
    _run(s, 0, 11, 11, 10, unmarked=lambda i: i % 2 == 0)
    c["two_runs_one_empty_between"] = s
    s = [new_file(40)]
    _run(s, 0, 30, 30, 10)
    c["run_to_the_file_end"] = s
    s = [new_file(2 * tile + 10)]
    _run(s, 0, tile - 5, tile - 5, 11)
    _run(s, 0, 2 * tile - 1, 2 * tile - 1, 3)
    c["run_across_the_tile"] = s
    return c


# --------------------------------------------------------------- random stores --
def random_store(seed, slots=4096, homes=3000, load=0.7, invalid=0.10, dup=0.01, marked=0.60):
    """(files, ids): a store built by the writer to `load` of `slots`, 10 % of
    its entries invalidated, duplicates injected behind their runs, 60 % of the
    valid entries marked.  ids: every ID inserted."""
    rng = random.Random(seed)
    files = [new_file(slots)]
    ids = []
    for k in range(int(slots * load)):
        bid = rng.randbytes(13) + rng.randrange(homes).to_bytes(3, "big")
        insert(files, bid, E | (N if rng.random() < 0.5 else 0), rng.randrange(4), 16 + 34 * k)
        ids.append(bid)
    where = []
    for f, img in enumerate(files):
        where += [(f, o) for o in range(HEADER, len(img), SLOT) if struct.unpack_from(">H", img, o)[0] & E]
    rng.shuffle(where)
    n_inv = int(len(where) * invalid)
    for f, o in where[:n_inv]:
        struct.pack_into(">H", files[f], o, struct.unpack_from(">H", files[f], o)[0] | I)
    valid = where[n_inv:]
    for f, o in valid[:int(len(where) * dup)]:  # a later valid copy, in the first slot without Exists behind it
        t = o
        while t < len(files[f]) and struct.unpack_from(">H", files[f], t)[0] & E:
            t += SLOT
        if t < len(files[f]):
            files[f][t:t + SLOT] = files[f][o:o + SLOT]
            files[f][t + 18:t + 24] = location(5, t)
            valid.append((f, t))
    for f, o in valid:
        if rng.random() < marked:
            struct.pack_into(">H", files[f], o, struct.unpack_from(">H", files[f], o)[0] | M)
    return files, ids
