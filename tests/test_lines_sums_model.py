"""The sums kernel of the line tally (sre_hip_tally_sums_lines) on the CPU: tests/lines_sums_sim.cpp runs the lanes of all
waves as sre_k_tally_sums does, with the rules the kernel compiles (sregex_amd/csrc/sre_lines_sums.h), and applies every
atomic through a Mem that logs (wave, aggregate, quantity).  Whatever the order of the waves, the aggregates must equal a
Python dict, a wave must send at most one atomic per key, column and quantity and none for a column in which its lines of
the key hold no number, and nothing at or beyond row min(sums_cap, nkeys) may change; and all of that whether the waves
send to the caller's rows or to copies of them that are merged at the end.  A case is a list of lines, each
None (a line without a key) or (key, [text of every value column, None: an unset group])."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import sregex_amd as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
_p64, _p32 = ctypes.POINTER(_u64), ctypes.POINTER(_u32)
FILL = 0xA5
LAST, UNSET, FIRST = 1 << 63, 1 << 62, 1 << 61
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
IDENTITY = (0, INT64_MAX, INT64_MIN, 0)
QUANTITIES = 4

LINE_ORDER, RANDOM, REVERSED = 0, 1, 2
SCHEDULES = (LINE_ORDER, RANDOM, REVERSED)

NINES = b"9" * 18
# the table of tests/test_tally_sums_abi.py
NUMBERS = [(b"0", 0), (b"-0", 0), (b"007", 7), (NINES, 10 ** 18 - 1), (b"-" + NINES, -(10 ** 18 - 1))]
NOT_NUMBERS = [b"", b"-", b"--1", b"+1", b"1 ", b" 1", b"12a", b"1-", b"1" * 19, b"-" + b"1" * 19, b"1" * 18 + b"\0"]


@pytest.fixture(scope="module")
def sim():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "liblinessumssim.so")
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, "lines_sums_sim.cpp")] + [os.path.join(csrc, h) for h in (
        "sre_lines_sums.h", "sre_lines_tally.h", "sre_lines_route.h", "sre_lines_gather.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    L = ctypes.CDLL(so)
    L.lssim_none.restype = _u32
    L.lssim_max_values.restype = _u32
    L.lssim_agg_bytes.restype = _u32
    L.lssim_number.restype = ctypes.c_int
    L.lssim_number.argtypes = [ctypes.c_char_p, _u64, ctypes.POINTER(_i64)]
    L.lssim_sums.restype = _u64
    L.lssim_sums.argtypes = [ctypes.c_char_p, _p64, _p64, _u64, _u32, _p32, _p64, _u64, ctypes.c_void_p, _u32, ctypes.c_int, _u64,
                             _p64, _u64, _p64]
    L.lssim_copies.restype = _u32
    L.lssim_copies.argtypes = [_u64, _u32]
    return L


def number(text):
    """the number rule in Python"""
    return int(text) if text is not None and re.fullmatch(rb"-?[0-9]{1,18}", text, re.DOTALL) else None


def wrap(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def model_number(sim, text):
    v = _i64(-12345)
    if sim.lssim_number(text, len(text), ctypes.byref(v)) != 1:
        assert v.value == -12345, "the value of a text that is not a number was written"
        return None
    return v.value


def test_number_rule_is_the_librarys(sim):
    assert sim.lssim_agg_bytes() == ctypes.sizeof(S.TallySumStruct) == 32
    assert sim.lssim_max_values() == S.HIP_TALLY_MAX_VALUES
    for text, want in NUMBERS:
        assert model_number(sim, text) == S.tally_number(text) == number(text) == want, text
    for text in NOT_NUMBERS:
        assert model_number(sim, text) is None and S.tally_number(text) is None and number(text) is None, text
    rng = random.Random(3)
    for _ in range(3000):
        text = bytes(rng.choice(b"0123456789-+ a\0") for _ in range(rng.randrange(22)))
        if rng.random() < 0.5:
            text = rng.choice([b"", b"-"]) + bytes(rng.choice(b"0123456789") for _ in range(rng.randrange(1, 21)))
        assert model_number(sim, text) == S.tally_number(text) == number(text), text


def test_copies_rule(sim):
    """as many copies as fit 8 MiB, at most 64, and the caller's rows themselves when one copy is too large"""
    assert sim.lssim_copies(0, 1) == 1 and sim.lssim_copies(1, 1) == 64 and sim.lssim_copies(4096, 8) == 8
    assert sim.lssim_copies(1 << 18, 1) == 1 and sim.lssim_copies((1 << 18) + 1, 1) == 1 and sim.lssim_copies(1 << 30, 8) == 1
    assert sim.lssim_copies(1 << 17, 1) == 2 and sim.lssim_copies(4096, 1) == 64 and sim.lssim_copies(4097, 1) == 63


def value_table(lines, V):
    """(source bytes, vval, vstart) as the extract's select pass leaves them over the value groups"""
    buf, val, start = bytearray(), [], []
    for ln in lines:
        st = len(buf)
        for c in range(V):
            flags = (FIRST if c == 0 else 0) | (LAST if c + 1 == V else 0)
            fld = None if ln is None else ln[1][c]
            if fld is None:
                val.append(0 if ln is None else 1)
                start.append(st | UNSET | flags)
            else:
                val.append(len(fld) + 1)
                start.append(len(buf) | flags)
                buf += fld + b";"
        buf += b"\n"
    return bytes(buf), val, start


def expected(lines, V):
    """{key: [aggregate of every column]} in first-occurrence order"""
    d = {}
    for ln in lines:
        if ln is None:
            continue
        row = d.setdefault(ln[0], [list(IDENTITY) for _ in range(V)])
        for c in range(V):
            x = number(ln[1][c])
            if x is not None:
                a = row[c]
                a[0], a[1], a[2], a[3] = wrap(a[0] + x), min(a[1], x), max(a[2], x), a[3] + 1
    return d


def run(sim, lines, V, sums_cap=None, schedule=LINE_ORDER, seed=1, spare_rows=3):
    """under the rule's number of copies, then with the waves sending to the caller's rows, then with three copies"""
    res = [run_copies(sim, lines, V, copies, sums_cap, schedule, seed, spare_rows) for copies in (0, 1, 3)]
    assert all(bytes(r[1]) == bytes(res[0][1]) and r[2] == res[0][2] for r in res), "the copies show in the result"
    return res[0]


def run_copies(sim, lines, V, copies, sums_cap, schedule, seed, spare_rows):
    n = len(lines)
    want = expected(lines, V)
    nkeys = len(want)
    rows = nkeys if sums_cap is None else min(sums_cap, nkeys)
    buf, val, start = value_table(lines, V)
    a_val, a_start = (_u64 * max(n * V, 1))(*val), (_u64 * max(n * V, 1))(*start)
    # slots in an order of their own, so that a slot number is never a key number by accident
    keyno = {key: k for k, key in enumerate(want)}
    nslots = max(2 * nkeys, 8)
    slots = random.Random(nkeys).sample(range(nslots), nkeys)
    cnt = (_u64 * nslots)(*([0xDEAD] * nslots))
    for key, k in keyno.items():
        cnt[slots[k]] = k
    NONE = sim.lssim_none()
    lslot = (_u32 * max(n, 1))(*[NONE if ln is None else slots[keyno[ln[0]]] for ln in lines])
    alloc = (rows + spare_rows) * V
    sums = (S.TallySumStruct * alloc)()
    ctypes.memset(sums, FILL, ctypes.sizeof(sums))
    log_cap = 4 * V * max(n, 1)
    log, words = (_u64 * (3 * log_cap))(), (_u64 * 4)()
    made = sim.lssim_sums(buf, a_val, a_start, n, V, lslot, cnt, rows, ctypes.addressof(sums), copies, schedule, seed, log,
                          log_cap, words)
    ctx = (n, V, copies, sums_cap, schedule, seed)
    assert words[3] == (copies or sim.lssim_copies(rows, V)) >= 1
    assert made == words[0] <= log_cap and words[1] == 0, ("an atomic outside the rows", list(words), ctx)
    # the result is the dict's
    for k, (key, row) in enumerate(want.items()):
        if k >= rows:
            break
        for c in range(V):
            a = sums[k * V + c]
            assert (a.sum, a.min, a.max, a.n) == tuple(row[c]), (key, c, ctx)
    # nothing at or beyond row min(sums_cap, nkeys)
    tail = bytes(sums)[rows * V * 32:]
    assert tail == bytes([FILL]) * len(tail), ctx
    # at most one atomic per (wave, key, column, quantity), none where the wave's lines of the key hold no number
    seen = set()
    for q in range(made):
        rec = (log[3 * q], log[3 * q + 1], log[3 * q + 2])
        assert rec not in seen, ("two atomics of one wave on one quantity", rec, ctx)
        seen.add(rec)
    keys = list(want)
    holds = set()       # (wave, aggregate) with a number
    for i, ln in enumerate(lines):
        if ln is None or keyno[ln[0]] >= rows:
            continue
        for c in range(V):
            if number(ln[1][c]) is not None:
                holds.add((i // 64, keyno[ln[0]] * V + c))
    assert {(w, idx) for w, idx, _ in seen} == holds, ctx
    assert made == QUANTITIES * len(holds), ctx
    # the grouping loop: a turn per distinct key of a wave that takes part
    turns = sum(len({keyno[ln[0]] for ln in lines[w:w + 64] if ln is not None and keyno[ln[0]] < rows}) for w in range(0, n, 64))
    assert words[2] == turns, ctx
    return keys, sums, made


def num(x):
    return b"%d" % x


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_one_key_in_300_lines(sim, schedule):
    lines = [(b"k", [num(i - 150)]) for i in range(300)]
    _, sums, made = run(sim, lines, 1, schedule=schedule)
    a = sums[0]
    assert (a.sum, a.min, a.max, a.n) == (sum(range(-150, 150)), -150, 149, 300)
    assert made == QUANTITIES * 5, "five waves, one key: one atomic per wave and quantity"


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_64_distinct_keys_in_one_wave(sim, schedule):
    lines = [(b"k%d" % i, [num(i * 7 - 100)]) for i in range(64)]
    _, _, made = run(sim, lines, 1, schedule=schedule)
    assert made == QUANTITIES * 64


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("V", (1, 3))
def test_three_keys_interleaved_lane_by_lane(sim, schedule, V):
    lines = [(b"abc"[i % 3:i % 3 + 1], [num(i), b"x", num(-i)][:V]) for i in range(200)]
    _, _, made = run(sim, lines, V, schedule=schedule)
    assert made == QUANTITIES * 3 * 4 * (1 if V == 1 else 2), "four waves, three keys, the columns that hold numbers"


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_a_wave_whose_lanes_mostly_sit_out(sim, schedule):
    lines = [None] * 130
    lines[3] = (b"a", [b"5"])
    lines[60] = (b"a", [b"-7"])
    lines[61] = (b"b", [b"nope"])
    lines[129] = (b"a", [b"1"])
    _, sums, made = run(sim, lines, 1, schedule=schedule)
    assert (sums[0].sum, sums[0].min, sums[0].max, sums[0].n) == (-1, -7, 5, 3)
    assert (sums[1].sum, sums[1].min, sums[1].max, sums[1].n) == IDENTITY
    assert made == QUANTITIES * 2
    run(sim, [None] * 70, 2, schedule=schedule)
    run(sim, [], 1, schedule=schedule)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("V", (1, 3))
def test_sums_cap_below_the_number_of_keys(sim, schedule, V):
    rng = random.Random(V)
    lines = [(b"k%d" % rng.randrange(40), [num(rng.randrange(-50, 50)) for _ in range(V)]) for _ in range(500)]
    for cap in (0, 1, 5, 39, 40, 43):
        run(sim, lines, V, sums_cap=cap, schedule=schedule, seed=cap)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_wrapping_sum_and_the_number_table(sim, schedule):
    lines = [(b"p", [NINES]) for _ in range(12)] + [(b"m", [b"-" + NINES]) for _ in range(12)]
    lines += [(b"t", [t]) for t, _ in NUMBERS] + [(b"t", [t]) for t in NOT_NUMBERS] + [(b"t", [None])]
    _, sums, _ = run(sim, lines * 4, 1, schedule=schedule)
    assert sums[0].sum == wrap(48 * (10 ** 18 - 1)) and sums[0].n == 48 and sums[0].sum < 0
    assert sums[1].sum == wrap(-48 * (10 ** 18 - 1)) and sums[1].sum > 0
    assert (sums[2].sum, sums[2].min, sums[2].max, sums[2].n) == (4 * 7, -(10 ** 18 - 1), 10 ** 18 - 1, 4 * len(NUMBERS))


VALUES = (b"", None, b"x1", b"-", NINES, b"1" * 19, b"-" + NINES)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("n", (1, 63, 64, 65, 300, 1500))
@pytest.mark.parametrize("V", (1, 3, 8))
def test_random_mixes(sim, schedule, n, V):
    rng = random.Random(n * 10 + V)
    for nkeys in (1, 7, 200):
        lines = []
        for _ in range(n):
            if rng.random() < 0.15:
                lines.append(None)
                continue
            vals = [rng.choice(VALUES) if rng.random() < 0.3 else num(rng.randrange(-1000, 1000)) for _ in range(V)]
            lines.append((b"key%d" % rng.randrange(nkeys), vals))
        run(sim, lines, V, schedule=schedule, seed=n + nkeys)
        run(sim, lines, V, sums_cap=max(nkeys // 2, 1), schedule=schedule, seed=n)
