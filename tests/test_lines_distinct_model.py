"""The passes of the line distinct (sre_hip_distinct_lines) on the CPU: tests/lines_distinct_sim.cpp compiles the rules the
kernels compile (sregex_amd/csrc/sre_lines_distinct.h) and runs them behind the tally model's insert
(tests/lines_tally_sim.cpp, under its four schedules and with the hash whole and masked to 0, 1 and 2 bits).  Whatever the
schedule, every key's first line, last line and count must be those of a Python dict; the `last` pass must send exactly one
atomic per distinct slot of a wave; the pick pass must leave exactly the lines the rule, the range and the flag select, count
the qualifying keys, and drop a line without a slot without a read of the table.  The values it leaves then go through the
filter's gather model (tests/lines_gather_sim.cpp, unchanged) at cuts need, need - 1, one line and 0.  A case is a list of
lines as in tests/test_lines_tally_model.py: a tuple of K field texts (None: an unset field) or None (a line without a
key)."""
import ctypes
import random

import pytest

from test_lines_tally_model import SCHEDULES, _build, entry_table, insert, key_of, tsim      # noqa: F401  (tsim: a fixture)
from test_lines_keyset_model import gather_all_cuts

_u64, _u32, _i64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
_p64, _p32, _p8, _pi64 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(_i64)
FIRST, LAST, EVERY = 0, 1, 2
HASH_BITS = (64, 0, 1, 2)


@pytest.fixture(scope="module")
def dsim():
    L = _build("liblinesdistinctsim.so", "lines_distinct_sim.cpp",
               ["sre_lines_distinct.h", "sre_lines_tally.h", "sre_lines_route.h", "sre_lines_gather.h"])
    L.ldsim_threads.restype = _u32
    L.ldsim_range_ok.argtypes = [_u64, _u64]
    L.ldsim_picks.argtypes = [ctypes.c_int, _u64, _u64, ctypes.c_int, _u64, _u64, _u64, _u64]
    L.ldsim_last.restype = None
    L.ldsim_last.argtypes = [_p32, _u64, _u64, ctypes.c_int, _u64, _p64, _p64]
    L.ldsim_pick.restype = None
    L.ldsim_pick.argtypes = [_p32, _u64, _u64, _p64, _p64, _p64, ctypes.c_int, _u64, _u64, ctypes.c_int, _p64, _p64]
    L.ldsim_perline.restype = _u64
    L.ldsim_perline.argtypes = [_p32, _u64, _p64, _p64, _p64, _u64, _pi64, _u64]
    return L


@pytest.fixture(scope="module")
def gsim():
    """the filter's gather model, as tests/test_lines_gather_model.py builds it (a library of its own here)"""
    L = _build("liblinesgathersim_distinct.so", "lines_gather_sim.cpp", ["sre_lines_gather.h"])
    L.lgsim_gather.restype = _u64
    L.lgsim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32, _p64, _p64]
    return L


def per_key(lines):
    """{key: [first line, last line, count]}"""
    d = {}
    for i, ln in enumerate(lines):
        if ln is not None:
            e = d.setdefault(key_of(ln), [i, i, 0])
            e[1] = i
            e[2] += 1
    return d


def ranges(lines):
    """the ranges every case runs: all keys, unique keys, repeated keys, a band, and one nothing reaches"""
    most = max([e[2] for e in per_key(lines).values()] or [0])
    return [(1, 0), (1, 1), (2, 0), (2, 3), (most + 1, 0)]


def picked(which, lo, hi, line, first, last, count):
    named = line == first if which == FIRST else line == last if which == LAST else True
    return named and lo <= count and (hi == 0 or count <= hi)


def line_values(buf, lines):
    """the source's line ends and the filter's per-line values in mode 0 (len + 1 of a keyed line, else 0)"""
    ends = [i for i, b in enumerate(buf) if b == 0x0A]
    assert len(ends) == len(lines)
    starts = [0] + [e + 1 for e in ends[:-1]]
    return ends, [0 if ln is None else e - s + 1 for ln, s, e in zip(lines, starts, ends)]


def check(tsim, dsim, gsim, lines, K, hash_bits=64, schedule=0, seed=1, gather=True):
    n, want = len(lines), per_key(lines)
    buf, _, _, tab, cnt, lslot, words, nslots = insert(tsim, lines, K, max(len(want), 1), hash_bits, schedule, seed)
    ctx = (n, K, hash_bits, schedule, seed)
    assert words[2] == 0 and words[1] == len(want) and words[6] == 0, (words, ctx)
    NONE = tsim.ltsim_none()
    slot_of = {key_of(ln): lslot[i] for i, ln in enumerate(lines) if ln is not None}
    assert all((lslot[i] == NONE) == (ln is None) for i, ln in enumerate(lines)), ctx
    # the last pass: one atomic per distinct slot of a wave, the slot's final word the key's highest line
    lastrun, lw = (_u64 * nslots)(), (_u64 * 4)()
    dsim.ldsim_last(lslot, n, nslots, schedule, seed, lastrun, lw)
    waves = sum(len({lslot[i] for i in range(b, min(b + 64, n)) if lslot[i] != NONE}) for b in range(0, n, 64))
    assert lw[2] == 0 and lw[0] == lw[1] == lw[3] == waves, (list(lw), waves, ctx)
    for key, (first, last, count) in want.items():
        s = slot_of[key]
        assert (tab[s], lastrun[s], cnt[s]) == (first, last, count), (key, ctx)
    used = set(slot_of.values())
    assert all(lastrun[s] == 0 for s in range(nslots) if s not in used), ctx
    # the per-line arrays, whole and cut
    for kc, kl in ((n, n), (n // 2, 0), (0, (n + 1) // 2)):
        keycount, keyline = (_u64 * (n + 1))(*([99] * (n + 1))), (_i64 * (n + 1))(*([-99] * (n + 1)))
        assert dsim.ldsim_perline(lslot, nslots, tab, cnt, keycount, kc, keyline, kl) == 0, ctx
        assert list(keycount) == [0 if ln is None else want[key_of(ln)][2] for ln in lines[:kc]] + [99] * (n + 1 - kc), ctx
        assert list(keyline) == [-1 if ln is None else want[key_of(ln)][0] for ln in lines[:kl]] + [-99] * (n + 1 - kl), ctx
    # the pick pass: every which x invert x range
    ends, fval0 = line_values(buf, lines)
    threads = dsim.ldsim_threads()
    for which in (FIRST, LAST, EVERY):
        for invert in (0, 1):
            for lo, hi in ranges(lines):
                fval, pw = (_u64 * (n + 1))(*(fval0 + [7])), (_u64 * 4)()
                dsim.ldsim_pick(lslot, n, nslots, tab, cnt, lastrun if which == LAST else None, which, lo, hi, invert, fval, pw)
                sel = [ln is not None and picked(which, lo, hi, i, *want[key_of(ln)]) != bool(invert) for i, ln in enumerate(lines)]
                c2 = ctx + (which, invert, lo, hi)
                assert list(fval) == [v if s else 0 for v, s in zip(fval0, sel)] + [7], c2
                kept = [e[0] for e in want.values() if lo <= e[2] and (hi == 0 or e[2] <= hi)]
                assert pw[0] == len(kept) and pw[2] == 0, (list(pw), len(kept), c2)
                assert pw[3] == len({f // threads for f in kept}), ("one add per workgroup", list(pw), c2)
                nkeyed = sum(1 for ln in lines if ln is not None)
                assert pw[1] == nkeyed * (3 if which == LAST else 2), ("reads through the slots of the keyed lines only", c2)
                if which != EVERY and not invert:
                    assert sum(sel) == len(kept), ("nselected == nkeys_kept", c2)
                if gather and n and (lo, hi) in ((1, 0), (2, 0)):
                    gather_all_cuts(gsim, buf, ends, list(fval)[:n], lines)


def make_lines(rng, n, K, nkeys, unkeyed=0.15):
    pool = [tuple(None if rng.random() < 0.1 else bytes(rng.choice(b"abc") for _ in range(rng.randrange(0, 4))) for _ in range(K))
            for _ in range(nkeys)]
    return [None if rng.random() < unkeyed else rng.choice(pool) for _ in range(n)]


def test_the_rule_itself(dsim):
    assert [dsim.ldsim_range_ok(a, b) for a, b in ((0, 0), (0, 5), (1, 0), (1, 1), (2, 1), (3, 2), (2, 3))] == [0, 0, 1, 1, 0, 0, 1]
    for which in (FIRST, LAST, EVERY):
        for lo, hi in ((1, 0), (1, 1), (2, 0), (2, 3), (5, 0)):
            for count in (1, 2, 3, 4, 5):
                for line, first, last in ((3, 3, 3), (3, 3, 9), (9, 3, 9), (5, 3, 9)):
                    if count == 1 and first != last:
                        continue
                    for invert in (0, 1):
                        want = picked(which, lo, hi, line, first, last, count) != bool(invert)
                        assert bool(dsim.ldsim_picks(which, lo, hi, invert, line, first, last, count)) == want


@pytest.mark.parametrize("hash_bits", HASH_BITS)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_first_last_count_and_pick_under_every_schedule(tsim, dsim, gsim, schedule, hash_bits):
    rng = random.Random(1000 * schedule + hash_bits)
    for n, K, nkeys in ((1, 1, 1), (63, 1, 3), (64, 2, 40), (65, 1, 65), (257, 2, 9), (600, 1, 120)):
        check(tsim, dsim, gsim, make_lines(rng, n, K, nkeys), K, hash_bits, schedule, seed=n, gather=hash_bits == 64)


def test_one_key_and_all_distinct_and_no_key(tsim, dsim, gsim):
    check(tsim, dsim, gsim, [(b"k",)] * 300, 1, schedule=1)
    check(tsim, dsim, gsim, [(b"%d" % i,) for i in range(300)], 1, schedule=2)
    check(tsim, dsim, gsim, [None] * 70, 1)
    check(tsim, dsim, gsim, [None, (b"", None), (None, b""), None, (b"ab", b"c"), (b"a", b"bc"), (b"ab", b"c")], 2, schedule=3)


def test_a_stopped_search_is_dropped_without_a_table_read(tsim, dsim):
    """more keys than max_keys: the insert raises its flag and leaves lines without a slot (SRE_LT_NONE); pick clears them
    and reads nothing through them, whatever stands in the table"""
    lines = [(b"%d" % (i % 200),) for i in range(520)]
    buf, _, _, tab, cnt, lslot, words, nslots = insert(tsim, lines, 1, 8, 64, 0, 1)
    assert words[2] != 0
    NONE = tsim.ltsim_none()
    stopped = [i for i in range(len(lines)) if lslot[i] == NONE]
    assert stopped
    for which in (FIRST, LAST, EVERY):
        for invert in (0, 1):
            n = len(lines)
            fval, pw = (_u64 * n)(*([5] * n)), (_u64 * 4)()
            lastrun = (_u64 * nslots)()
            dsim.ldsim_pick(lslot, n, nslots, tab, cnt, lastrun, which, 1, 0, invert, fval, pw)
            assert pw[2] == 0 and all(fval[i] == 0 for i in stopped)
            assert pw[1] == (n - len(stopped)) * (3 if which == LAST else 2)
