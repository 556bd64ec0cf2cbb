"""The insert of the line tally (sre_hip_tally_lines) on the CPU: tests/lines_tally_sim.cpp runs every lane as the state
machine the kernel compiles (sregex_amd/csrc/sre_lines_tally.h), one atomic access a step, under schedules that put lanes
to sleep between any two accesses; of the 64 lines of a wave only the lowest line of every key searches the table.
Whatever the schedule, each key must sit in exactly one slot, the slot's final word must be the key's lowest line, the
counts must be the exact multiplicities, and a wave must issue one add per distinct slot it holds.  The keep pass then
leaves an entry table that, fed through the extract's gather model (tests/lines_extract_sim.cpp, unchanged), writes every
output byte exactly once.  A case is a list of lines, each a tuple of K field texts (None: an unset field) or None (an
unselected line); the expected result is a Python dict in first-occurrence order."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32 = ctypes.c_uint64, ctypes.c_uint32
_p64, _p32, _p8 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_uint8)
FILL = 0xA5
DELIM, FSEP = 0x0A, 0x09
LAST, UNSET, FIRST = 1 << 63, 1 << 62, 1 << 61

SEQUENTIAL, RANDOM, HOLD_MIN, ROUND_ROBIN = 0, 1, 2, 3
SCHEDULES = (SEQUENTIAL, RANDOM, HOLD_MIN, ROUND_ROBIN)


def _build(name, source, headers):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, source)] + [os.path.join(csrc, h) for h in headers]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def tsim():
    L = _build("liblinestallysim.so", "lines_tally_sim.cpp", ["sre_lines_tally.h", "sre_lines_route.h", "sre_lines_gather.h"])
    L.ltsim_empty.restype = _u64
    L.ltsim_none.restype = _u32
    L.ltsim_nslots.restype = _u64
    L.ltsim_nslots.argtypes = [_u64]
    L.ltsim_flag_every.restype = _u32
    L.ltsim_hash.restype = _u64
    L.ltsim_hash.argtypes = [ctypes.c_char_p, _p64, _p64, _u32, _u64]
    L.ltsim_insert.restype = _u64
    L.ltsim_insert.argtypes = [ctypes.c_char_p, _p64, _p64, _u64, _u32, _u64, ctypes.c_int, ctypes.c_int, _u64, _p64, _p64, _p32,
                               _p64]
    L.ltsim_keep.restype = None
    L.ltsim_keep.argtypes = [_p64, _u64, _u32, _p64, _p32]
    return L


@pytest.fixture(scope="module")
def gsim():
    """the extract's gather model, as tests/test_lines_extract_model.py builds it (a library of its own here)"""
    L = _build("liblinesextractsim_tally.so", "lines_extract_sim.cpp", ["sre_lines_gather.h"])
    L.lesim_cut.restype = _u64
    L.lesim_cut.argtypes = [_p64, _u64, _u64, _u64]
    L.lesim_gather.restype = _u64
    L.lesim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32,
                               _p64, _p64]
    return L


def entry_table(lines, K, src_off=0):
    """(source bytes, val, start) as the extract's select pass leaves them: the fields of a line lie in its text in order,
    separated by '|'; an unset field has the line's start under UNSET"""
    buf, val, start = bytearray(), [], []
    for ln in lines:
        st = len(buf)
        for f in range(K):
            flags = (FIRST if f == 0 else 0) | (LAST if f + 1 == K else 0)
            fld = None if ln is None else ln[f]
            if fld is None:
                val.append(0 if ln is None else 1)
                start.append(st | UNSET | flags)
            else:
                val.append(len(fld) + 1)
                start.append(len(buf) | flags)
                buf += fld + b"|"
        buf += b"\n"
    return bytes(buf), val, start


def key_of(ln):
    return tuple(b"" if f is None else f for f in ln)


def first_occurrence(lines):
    """{key: [first line, count]} in first-occurrence order"""
    d = {}
    for i, ln in enumerate(lines):
        if ln is None:
            continue
        d.setdefault(key_of(ln), [i, 0])[1] += 1
    return d


def insert(tsim, lines, K, max_keys, hash_bits=64, schedule=SEQUENTIAL, seed=1):
    n = len(lines)
    buf, val, start = entry_table(lines, K)
    a_val, a_start = (_u64 * max(n * K, 1))(*val), (_u64 * max(n * K, 1))(*start)
    nslots = tsim.ltsim_nslots(max_keys)
    assert nslots >= 1024 and nslots >= 2 * max_keys and nslots & (nslots - 1) == 0 and (nslots == 1024 or nslots < 4 * max_keys)
    tab, cnt = (_u64 * nslots)(*([tsim.ltsim_empty()] * nslots)), (_u64 * nslots)()
    lslot, words = (_u32 * max(n, 1))(), (_u64 * 9)()
    tsim.ltsim_insert(buf, a_val, a_start, n, K, max_keys, hash_bits, schedule, seed, tab, cnt, lslot, words)
    return buf, a_val, a_start, tab, cnt, lslot, list(words), nslots


def check(tsim, lines, K, hash_bits=64, schedule=SEQUENTIAL, seed=1, max_keys=None):
    """one insert without overflow, asserted in full; returns what the keep pass needs"""
    n = len(lines)
    want = first_occurrence(lines)
    mk = max(len(want), 1) if max_keys is None else max_keys
    buf, a_val, a_start, tab, cnt, lslot, words, nslots = insert(tsim, lines, K, mk, hash_bits, schedule, seed)
    tsel, tclaims, tover, ncas, nmin, nadds, bad, _, turns = words
    ctx = (n, K, hash_bits, schedule, seed, mk)
    assert bad == 0, ctx
    assert tover == 0 and tclaims == len(want), (words, len(want), ctx)
    assert tsel == sum(1 for ln in lines if ln is not None), ctx
    NONE, EMPTY = tsim.ltsim_none(), tsim.ltsim_empty()
    slot_of = {}
    for i, ln in enumerate(lines):
        if ln is None:
            assert lslot[i] == NONE, (i, ctx)
            continue
        assert lslot[i] != NONE and lslot[i] < nslots
        assert slot_of.setdefault(key_of(ln), lslot[i]) == lslot[i], ("a key in two slots", i, ctx)
    assert len(set(slot_of.values())) == len(slot_of), ("two keys in one slot", ctx)
    for key, (first, count) in want.items():
        s = slot_of[key]
        assert tab[s] == first, ("the slot's final word is the key's lowest line", key, tab[s], first, ctx)
        assert cnt[s] == count, (key, cnt[s], count, ctx)
    used = set(slot_of.values())
    assert all(tab[s] == EMPTY and cnt[s] == 0 for s in range(nslots) if s not in used), ctx
    # the wave rule: one turn of the grouping loop, one search and one add per distinct key (= slot) of a wave
    groups = sum(len({lslot[i] for i in range(w, min(w + 64, n))} - {NONE}) for w in range(0, n, 64))
    assert groups == sum(len({key_of(ln) for ln in lines[w:w + 64] if ln is not None}) for w in range(0, n, 64))
    assert nadds == groups and turns == groups, ctx
    # every group makes at least one CAS; a minimum only follows a CAS that saw a higher line of the key
    assert ncas >= groups and nmin <= groups - len(want)
    return buf, a_val, a_start, tab, lslot, want


def make_lines(rng, n, K, nkeys, unselected=0.1, unset=0.1, longest=12):
    pool = []
    while len(pool) < nkeys:
        pool.append(tuple(None if rng.random() < unset else bytes(rng.choice(b"abc\t") for _ in range(rng.randrange(longest + 1)))
                          for _ in range(K)))
    return [None if rng.random() < unselected else rng.choice(pool) for _ in range(n)]


SIZES = (0, 1, 63, 64, 65, 300, 1500)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("K", (1, 2, 3))
def test_random_keys(tsim, schedule, n, K):
    rng = random.Random(n * 10 + K)
    for nkeys in (1, 7, 200):
        check(tsim, make_lines(rng, n, K, nkeys), K, schedule=schedule, seed=n + nkeys)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("bits", (0, 1, 2))
def test_masked_hash_forces_probe_chains(tsim, schedule, bits):
    """every key starts its search at one of 2^bits words: chains as long as the keys are many"""
    rng = random.Random(bits)
    for n, nkeys in ((200, 3), (600, 90), (65, 65)):
        check(tsim, make_lines(rng, n, 2, nkeys), 2, hash_bits=bits, schedule=schedule, seed=bits * 7 + n)


@pytest.mark.parametrize("seed", range(20))
def test_all_lanes_of_a_key_stopped_between_cas_and_min(tsim, seed):
    """one key, the highest line first (round robin) or in random order with every lane that has seen the key asleep in
    front of its minimum until all searches are over: the word must still fall to line 0"""
    lines = [(b"same", b"key")] * 500
    for schedule in (HOLD_MIN, ROUND_ROBIN):
        *_, words, _ = insert(tsim, lines, 2, 1, schedule=schedule, seed=seed)
        check(tsim, lines, 2, schedule=schedule, seed=seed)
        if schedule == ROUND_ROBIN:
            assert words[4] > 0, "no lane went through the minimum: the schedule tests nothing"


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("seed", range(10))
def test_two_keys_race_for_one_empty_slot(tsim, schedule, seed):
    rng = random.Random(seed)
    lines = [rng.choice([(b"ab", b"c"), (b"a", b"bc")]) for _ in range(130)]
    buf, val, start, tab, lslot, want = check(tsim, lines, 2, hash_bits=0, schedule=schedule, seed=seed)
    assert len(want) == 2 and sorted(set(lslot)) == [0, 1]      # the loser of slot 0 moved on to slot 1


def test_hash_mixes_the_lengths_in(tsim):
    lines = [(b"ab", b"c"), (b"a", b"bc"), (b"abc", b""), (b"", b"abc"), (b"abc", None), (b"ab", b"c")]
    buf, val, start = entry_table(lines, 2)
    a_val, a_start = (_u64 * len(val))(*val), (_u64 * len(start))(*start)
    h = [tsim.ltsim_hash(buf, a_val, a_start, 2, i) for i in range(len(lines))]
    assert h[0] == h[5] and len(set(h[:4])) == 4
    assert h[2] == h[4]                                         # an unset field is an empty field


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_claims_beyond_max_keys_raise_the_flag(tsim, schedule):
    rng = random.Random(9)
    for n, nkeys, bits in ((300, 40, 64), (300, 40, 1), (2000, 1500, 64), (64, 2, 0), (5, 1, 64)):
        lines = make_lines(rng, n, 2, nkeys, unselected=0.0)
        distinct = len(first_occurrence(lines))
        check(tsim, lines, 2, hash_bits=bits, schedule=schedule, max_keys=distinct)         # nkeys == max_keys succeeds
        if distinct > 1:
            *_, words, _ = insert(tsim, lines, 2, distinct - 1, bits, schedule)
            assert words[2] == 1 and words[6] == 0, (words, distinct)
            assert words[0] == n, "the selected lines are counted whether or not the call overflows"


def test_a_full_table_raises_the_flag(tsim):
    """max_keys = 1 gives 1024 slots; with the claims counted wave by wave, 64 lanes of 3000 distinct keys can fill them
    before any wave has settled: the search that has gone round the table must end and raise the flag"""
    lines = [(b"k%d" % i,) for i in range(3000)]
    for schedule in (RANDOM, ROUND_ROBIN):
        *_, words, nslots = insert(tsim, lines, 1, 1, 64, schedule)
        assert nslots == 1024 and words[2] == 1 and words[6] == 0


# ------------------------------------------------------------------ keep, then the extract's gather

def rows_of(want, fsep=FSEP, delim=DELIM):
    return [bytes([fsep]).join(key) + bytes([delim]) for key in want]


CAPS = (None, lambda need, rows: need - 1, lambda need, rows: rows[0] if rows else 0, lambda need, rows: 0)


def gather(tsim, gsim, lines, K, schedule, seed, src_off, dst_off, hash_bits=64):
    n = len(lines)
    buf, a_val, a_start, tab, lslot, want = check(tsim, lines, K, hash_bits=hash_bits, schedule=schedule, seed=seed)
    tsim.ltsim_keep(a_val, n, K, tab, lslot)
    firsts = {first for first, _ in want.values()}
    for i in range(n):
        for f in range(K):
            kept = a_val[i * K + f] != 0
            assert kept == (i in firsts), ("keep selects exactly the first line of every key", i, f)
    nent = n * K
    off = (_u64 * (nent + 1))()
    for e in range(nent):
        off[e + 1] = off[e] + a_val[e]
    texts = rows_of(want)
    need = sum(len(t) for t in texts)
    assert off[nent] == need
    src_len = (src_off + len(buf) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
    for cap in CAPS:
        cap = need if cap is None else cap(need, [len(t) for t in texts])
        if cap < 0:
            continue
        out, k = b"", 0
        for t in texts:
            if len(out) + len(t) > cap:
                break
            out += t
            k += 1
        cut = gsim.lesim_cut(off, n, K, cap)
        out_bytes = off[cut * K]
        assert out_bytes == len(out) <= cap, (cap, cut, k)
        if out_bytes == 0:
            continue        # (the call launches no gather)
        dst_len = (dst_off + out_bytes + 15) // 16 * 16
        dst = (ctypes.c_uint8 * dst_len)(*([FILL] * dst_len))
        reads, writes = (_u32 * max(src_len, 1))(), (_u32 * dst_len)()
        win, glo = _u64(), _u64()
        bad = gsim.lesim_gather(off, a_start, nent, out_bytes, src_off, dst_off, DELIM, FSEP, src, src_len, dst, dst_len, reads,
                                writes, ctypes.byref(win), ctypes.byref(glo))
        ctx = (n, K, schedule, src_off, dst_off, cap, out_bytes)
        assert bad == 0, ("accesses outside the aligned extents", bad, ctx)
        got = bytes(dst)
        assert got[dst_off:dst_off + out_bytes] == out, ctx
        w = list(writes)
        assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes, ("every output byte exactly once", ctx)
        assert not any(w[:dst_off]) and not any(w[dst_off + out_bytes:]), ("a write outside [out, out + out_bytes)", ctx)
        assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + out_bytes:] == bytes([FILL]) * (dst_len - dst_off - out_bytes)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("n", (1, 65, 700, 2100))
@pytest.mark.parametrize("K", (1, 2))
def test_keep_then_gather_writes_every_byte_once(tsim, gsim, schedule, n, K):
    rng = random.Random(n * 3 + K)
    for nkeys in (1, 20, 400):
        lines = make_lines(rng, n, K, nkeys)
        if lines[0] is None:
            lines[0] = (b"first",) * K          # (one row is then a real capacity)
        gather(tsim, gsim, lines, K, schedule, n + nkeys, rng.randrange(16), rng.randrange(16))


def test_keep_then_gather_with_long_chains(tsim, gsim):
    rng = random.Random(4)
    gather(tsim, gsim, make_lines(rng, 900, 2, 120), 2, RANDOM, 5, 3, 11, hash_bits=1)
    gather(tsim, gsim, [None] * 200, 2, RANDOM, 5, 3, 11)
