"""The key set and the lookup's probe (sre_hip_keyset_create, sre_hip_lookup_lines) on the CPU: tests/lines_keyset_sim.cpp
runs the text the kernels compile (sregex_amd/csrc/sre_lines_keyset.h, sre_lines_tally.h).  The dictionary's field rule
is checked against a Python split; the insert runs under the tally model's four schedules with the hash whole and masked,
and each key must end in one slot whose word is the key's lowest row; equal tuples must hash alike whether a line or a
row carries them; the probe is checked against a Python dict for key ids, selection and counts under both flags, and the
per-line values it leaves go through the filter's gather model (tests/lines_gather_sim.cpp, unchanged).  A dictionary is
a list of rows, each a tuple of K field texts; a line is a tuple of K field texts (None: an unset field) or None (a line
without a match)."""
import ctypes
import os
import random
import subprocess

import pytest

import sregex_amd as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
_p64, _p32, _p8, _pi64 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(_i64)
FILL = 0xA5
DELIM, FSEP = 0x0A, 0x09
LAST, UNSET, FIRST = 1 << 63, 1 << 62, 1 << 61
SEQUENTIAL, RANDOM, HOLD_MIN, ROUND_ROBIN = 0, 1, 2, 3
SCHEDULES = (SEQUENTIAL, RANDOM, HOLD_MIN, ROUND_ROBIN)
HASH_BITS = (64, 0, 1, 2)
HEADERS = ["sre_lines_keyset.h", "sre_lines_tally.h", "sre_lines_route.h", "sre_lines_gather.h"]


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
def ksim():
    L = _build("liblineskeysetsim.so", "lines_keyset_sim.cpp", HEADERS)
    for name in ("lksim_empty", "lksim_no_row", "lksim_max_rows"):
        getattr(L, name).restype = _u64
    L.lksim_nslots.restype = _u64
    L.lksim_nslots.argtypes = [_u64]
    L.lksim_fields.restype = _u64
    L.lksim_fields.argtypes = [ctypes.c_char_p, _p64, _u64, _u32, _u32, _p64, _p64]
    L.lksim_hash_row.restype = _u64
    L.lksim_hash_row.argtypes = [ctypes.c_char_p, _p64, _p64, _u32, _u64]
    L.lksim_hash_line.restype = _u64
    L.lksim_hash_line.argtypes = [ctypes.c_char_p, _p64, _p64, _u32, _u64]
    L.lksim_insert.restype = None
    L.lksim_insert.argtypes = [ctypes.c_char_p, _p64, _p64, _u64, _u32, _u64, ctypes.c_int, ctypes.c_int, _u64, _p64, _p64]
    L.lksim_probe.restype = _u64
    L.lksim_probe.argtypes = [ctypes.c_char_p, _p64, _p64, _u64, _u32, ctypes.c_char_p, _p64, _p64, _p64, _u64, ctypes.c_int,
                              ctypes.c_int, _p64, _pi64, _u64, _p64]
    return L


@pytest.fixture(scope="module")
def gsim():
    """the filter's gather model, as tests/test_lines_gather_model.py builds it (a library of its own here)"""
    L = _build("liblinesgathersim_keyset.so", "lines_gather_sim.cpp", ["sre_lines_gather.h"])
    L.lgsim_gather.restype = _u64
    L.lgsim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32, _p64, _p64]
    return L


def arr(values, ctype=_u64):
    return (ctype * max(len(values), 1))(*values)


# ------------------------------------------------------------------ the dictionary rule

def split_ends(text, delim=DELIM):
    """the row ends by the split rule of line mode: a final row without delim is a row, nothing follows a final delim"""
    ends, start = [], 0
    while start < len(text):
        e = text.find(bytes([delim]), start)
        if e < 0:
            ends.append(len(text))
            break
        ends.append(e)
        start = e + 1
    return ends


def py_rows(text, K, fsep=FSEP, delim=DELIM):
    """[tuple of K fields, or None for a row that breaks the field rule]"""
    out, start = [], 0
    for e in split_ends(text, delim):
        row = text[start:e]
        fields = (row,) if K == 1 else tuple(row.split(bytes([fsep])))
        out.append(fields if len(fields) == K else None)
        start = e + 1
    return out


def sim_rows(ksim, text, K, fsep=FSEP, delim=DELIM):
    """(rows as py_rows gives them read back through fstart / flen, lowest bad row or None, arrays)"""
    ends = split_ends(text, delim)
    n = len(ends)
    fstart, flen = arr([2 ** 64 - 1] * (n * K)), arr([2 ** 64 - 1] * (n * K))
    bad = ksim.lksim_fields(text, arr(ends), n, K, fsep, fstart, flen)
    rows = []
    for r in range(n):
        ok = all(flen[r * K + f] != 2 ** 64 - 1 for f in range(K))
        rows.append(tuple(text[fstart[r * K + f]:fstart[r * K + f] + flen[r * K + f]] for f in range(K)) if ok else None)
    return rows, (None if bad == ksim.lksim_no_row() else bad), fstart, flen


DICTS = [
    (b"", 1), (b"", 3), (b"one", 1), (b"one\n", 1), (b"a\nb", 1), (b"a\nb\n", 1), (b"\n", 1), (b"\n\n", 1), (b"a\n\nb\n", 1),
    (b"a\tb\n\t\nc\t", 2), (b"\t", 2), (b"\t\t\n", 3), (b"a\tb\tc\nd\te\tf", 3), (b"with\ttabs\tinside\nsecond\t\n", 1),
    (b"x|y\nz|", 2),
]


@pytest.mark.parametrize("text,K", DICTS, ids=[str(i) for i in range(len(DICTS))])
def test_dictionary_rows_and_fields(ksim, text, K):
    fsep = ord("|") if b"|" in text else FSEP
    want = py_rows(text, K, fsep)
    got, bad, _, _ = sim_rows(ksim, text, K, fsep)
    assert None not in want and got == want and bad is None, (text, K, got, want)


@pytest.mark.parametrize("K", (2, 3))
def test_the_lowest_bad_row_is_reported(ksim, K):
    good = b"\t".join([b"f"] * K)
    few, many = b"\t".join([b"f"] * (K - 1)), b"\t".join([b"f"] * (K + 1))
    for rows, lowest in (([good, few, good, many], 1), ([many, few], 0), ([good, good, b""], 2), ([good] * 70 + [many] + [few] * 9, 70),
                         ([good, good], None)):
        text = b"\n".join(rows) + b"\n"
        want = py_rows(text, K)
        got, bad, _, _ = sim_rows(ksim, text, K)
        bad_rows = [r for r, w in enumerate(want) if w is None]
        assert bad == lowest == (bad_rows[0] if bad_rows else None), (rows, bad, bad_rows)
        # a row with too many separators writes nothing beyond its own K entries: every good row reads back whole
        assert got == want


# ------------------------------------------------------------------ the insert

def build(ksim, rows, K, hash_bits=64, schedule=SEQUENTIAL, seed=1):
    """the dictionary of the rows and its table, asserted: each key in one slot, the slot's word the key's lowest row"""
    text = b"".join(bytes([FSEP]).join(r) + b"\n" for r in rows)
    got, bad, fstart, flen = sim_rows(ksim, text, K)
    assert bad is None and got == [tuple(r) for r in rows]
    n = len(rows)
    nslots = ksim.lksim_nslots(n)
    assert nslots >= 1024 and nslots >= 2 * n and nslots & (nslots - 1) == 0 and (nslots == 1024 or nslots < 4 * n)
    EMPTY = ksim.lksim_empty()
    tab, words = arr([EMPTY] * nslots), (_u64 * 5)()
    ksim.lksim_insert(text, fstart, flen, n, K, nslots, hash_bits, schedule, seed, tab, words)
    ids = {}
    for r, row in enumerate(rows):
        ids.setdefault(tuple(row), r)
    claims, ncas, nmin, bad, _ = words
    ctx = (n, K, hash_bits, schedule, seed)
    assert bad == 0 and claims == len(ids), (list(words), len(ids), ctx)
    held = [w for w in tab if w != EMPTY]
    assert sorted(held) == sorted(ids.values()), ("each key in one slot, holding its lowest row", ctx)
    assert ncas >= n and nmin <= n - len(ids)
    mask = (1 << hash_bits) - 1 if hash_bits < 64 else 2 ** 64 - 1
    for s in range(nslots):
        if tab[s] != EMPTY:
            home = ksim.lksim_hash_row(text, fstart, flen, K, tab[s]) & mask & (nslots - 1)
            # linear probing: no empty word between a key's home and its slot
            assert all(tab[(home + d) % nslots] != EMPTY for d in range((s - home) % nslots)), (s, home, ctx)
    return text, fstart, flen, tab, nslots, ids


def make_rows(rng, n, K, nkeys, longest=10):
    pool = [tuple(bytes(rng.choice(b"abc") for _ in range(rng.randrange(longest + 1))) for _ in range(K)) for _ in range(nkeys)]
    return [rng.choice(pool) for _ in range(n)]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("bits", HASH_BITS)
def test_insert_under_every_schedule(ksim, schedule, bits):
    rng = random.Random(bits * 4 + schedule)
    for n, K, nkeys in ((0, 1, 1), (1, 1, 1), (64, 2, 5), (300, 2, 90), (700, 1, 700), (513, 3, 40)):
        if bits != 64 and n > 300:
            continue        # (chains of hundreds of keys under a random schedule take a while and test nothing more)
        build(ksim, make_rows(rng, n, K, nkeys), K, hash_bits=bits, schedule=schedule, seed=n + bits)


@pytest.mark.parametrize("seed", range(5))
def test_one_key_many_rows_falls_to_row_zero(ksim, seed):
    for schedule in (HOLD_MIN, ROUND_ROBIN):
        *_, tab, nslots, ids = build(ksim, [(b"same", b"key")] * 300, 2, schedule=schedule, seed=seed)
        assert ids == {(b"same", b"key"): 0}


# ------------------------------------------------------------------ one hash through two Keys types

def entry_table(lines, K):
    """(source bytes, val, start, line ends, per-line filter values) as the select passes leave them: the fields of a
    line lie in its text in order, each followed by '|'; an unset field has the line's start under UNSET; a line
    without a match has val 0 in every entry and filter value 0"""
    buf, val, start, ends, fval = bytearray(), [], [], [], []
    for ln in lines:
        st = len(buf)
        for f in range(K):
            flags = (FIRST if f == 0 else 0) | (LAST if f + 1 == K else 0)
            fld = None if ln is None else ln[f]
            if fld is None:
                val.append(0 if ln is None else 1)
                start.append(st | UNSET | flags)
                if ln is None:
                    buf += b"no match "
            else:
                val.append(len(fld) + 1)
                start.append(len(buf) | flags)
                buf += fld + b"|"
        ends.append(len(buf))
        fval.append(0 if ln is None else len(buf) - st + 1)
        buf += b"\n"
    return bytes(buf), val, start, ends, fval


def key_of(ln):
    return tuple(b"" if f is None else f for f in ln)


def test_equal_tuples_hash_alike_through_both_key_types(ksim):
    tuples = [(b"ab", b"c"), (b"a", b"bc"), (b"abc", b""), (b"", b"abc"), (b"", b""), (b"10.0.0.1", b"GET")]
    text, fstart, flen, *_ = build(ksim, tuples, 2)
    lines = list(tuples) + [(b"abc", None), (None, None)]
    src, val, start, _, _ = entry_table(lines, 2)
    hr = [ksim.lksim_hash_row(text, fstart, flen, 2, r) for r in range(len(tuples))]
    hl = [ksim.lksim_hash_line(src, arr(val), arr(start), 2, i) for i in range(len(lines))]
    assert hl[:len(tuples)] == hr and len(set(hr)) == len(tuples)
    assert hl[6] == hr[2] and hl[7] == hr[4]                    # an unset field is an empty field
    for t, h in zip(tuples, hr):
        assert h == S.keyset_hash(b"\t".join(t), 2), t          # ... and the host hash is the same one


def test_host_hash_equals_the_model(ksim):
    rng = random.Random(5)
    for K in (1, 2, 5):
        rows = make_rows(rng, 40, K, 40, longest=30)
        text, fstart, flen, *_ = build(ksim, rows, K)
        for r, row in enumerate(rows):
            assert S.keyset_hash(b"\t".join(row), K) == ksim.lksim_hash_row(text, fstart, flen, K, r)


# ------------------------------------------------------------------ the probe

def probe(ksim, gsim, rows, lines, K, hash_bits=64, schedule=RANDOM, keyid_n=None, gather=True):
    """the probe of every line against the set of the rows under both flags, asserted against a dict; returns the
    members' ids and the model's words"""
    text, fstart, flen, tab, nslots, ids = build(ksim, rows, K, hash_bits, schedule)
    src, val, start, ends, fval0 = entry_table(lines, K)
    n = len(lines)
    want_ids = [-2 if ln is None else ids.get(key_of(ln), -1) for ln in lines]
    nkeyed, nmembers = sum(1 for v in want_ids if v != -2), sum(1 for v in want_ids if v >= 0)
    kn = n if keyid_n is None else min(keyid_n, n)
    out = None
    for invert in (0, 1):
        fval, keyid, words = arr(fval0 + [7]), arr([-99] * (n + 1), _i64), (_u64 * 5)()
        twice = ksim.lksim_probe(src, arr(val), arr(start), n, K, text, fstart, flen, tab, nslots, hash_bits, invert, fval, keyid, kn,
                                 words)
        ctx = (len(rows), n, K, hash_bits, invert)
        assert twice == 0, ("a step made two table reads", ctx)
        assert words[3] == 0, ("a read outside the table", ctx)
        assert (words[0], words[1]) == (nkeyed, nmembers), (list(words), nkeyed, nmembers, ctx)
        assert list(keyid)[:kn] == want_ids[:kn] and list(keyid)[kn:n + 1] == [-99] * (n + 1 - kn), ctx
        want_val = [v if w != -2 and ((w >= 0) != bool(invert)) else 0 for v, w in zip(fval0, want_ids)]
        assert list(fval)[:n] == want_val and fval[n] == 7, ctx
        assert words[2] <= nkeyed * nslots and words[4] <= nslots
        if gather:
            gather_all_cuts(gsim, src, ends, want_val, lines)
        out = words
    return want_ids, list(out)


def gather_all_cuts(gsim, src_text, ends, vals, lines, src_off=3, dst_off=5):
    """the per-line values through the filter's scan (a prefix sum), its cut at need, need - 1, one line and 0, and the
    gather model: the selected lines whole, every output byte once, nothing else touched"""
    n = len(vals)
    off = [0]
    for v in vals:
        off.append(off[-1] + v)
    need = off[n]
    texts = [src_text[(ends[i - 1] + 1 if i else 0):ends[i]] + b"\n" for i in range(n) if vals[i]]
    assert need == sum(len(t) for t in texts)
    src_len = (src_off + len(src_text) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + src_text + bytes([0xEE]) * (src_len - src_off - len(src_text))
    for cap in {need, need - 1, len(texts[0]) if texts else 0, 0}:
        if cap < 0:
            continue
        want = b""
        for t in texts:
            if len(want) + len(t) > cap:
                break
            want += t
        out_bytes = len(want)
        if out_bytes == 0:
            continue            # (the call launches no gather)
        dst_len = (dst_off + out_bytes + 15) // 16 * 16
        dst = (ctypes.c_uint8 * dst_len)(*([FILL] * dst_len))
        reads, writes = (_u32 * src_len)(), (_u32 * dst_len)()
        win, glo = _u64(), _u64()
        bad = gsim.lgsim_gather(arr(off), arr(ends), n, out_bytes, src_off, dst_off, DELIM, src, src_len, dst, dst_len, reads, writes,
                                ctypes.byref(win), ctypes.byref(glo))
        assert bad == 0, ("accesses outside the aligned extents", bad, cap)
        got, w = bytes(dst), list(writes)
        assert got[dst_off:dst_off + out_bytes] == want, cap
        assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes and not any(w[:dst_off]) and not any(w[dst_off + out_bytes:])
        assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + out_bytes:] == bytes([FILL]) * (dst_len - dst_off - out_bytes)


def make_lines(rng, n, K, keys, foreign, unkeyed=0.15):
    out = []
    for _ in range(n):
        x = rng.random()
        out.append(None if x < unkeyed else rng.choice(keys) if x < 0.6 else rng.choice(foreign))
    return out


@pytest.mark.parametrize("n", (1, 63, 64, 65, 3 * 1024 + 17))
@pytest.mark.parametrize("K", (1, 2))
def test_probe_against_a_dict(ksim, gsim, n, K):
    rng = random.Random(n + K)
    rows = make_rows(rng, 150, K, 60)
    foreign = [tuple(b"zz" + f for f in r) for r in make_rows(rng, 30, K, 30)]
    lines = make_lines(rng, n, K, rows, foreign)
    if n == 1:
        lines = [rows[7]]
    ids, words = probe(ksim, gsim, rows, lines, K)
    if n >= 63:
        assert -2 in ids and -1 in ids and max(ids) >= 0
    probe(ksim, gsim, rows, lines, K, keyid_n=n // 2, gather=False)


def test_unset_against_empty_and_empty_set(ksim, gsim):
    rows = [(b"a", b""), (b"", b""), (b"", b"b")]
    lines = [(b"a", None), (b"a", b""), (None, None), (None, b"b"), (b"a", b"b"), None, (b"", b"")]
    ids, _ = probe(ksim, gsim, rows, lines, 2)
    assert ids == [0, 0, 1, 2, -1, -2, 1]
    ids, words = probe(ksim, gsim, [], lines, 2)
    assert ids == [-1, -1, -1, -1, -1, -2, -1] and words[1] == 0 and words[2] == 6      # one read each: an empty word


def test_a_chain_across_the_end_of_the_table(ksim, gsim):
    """keys chosen by the model's hash (the host hash is the same) so that home >= slots - 2: the chains wrap to word 0"""
    tail, i = [], 0
    while len(tail) < 10:
        key = (b"key%d" % i,)
        if S.keyset_hash(key[0]) & 1023 >= 1022:
            tail.append(key)
        i += 1
    rows, foreign = tail[:7], tail[7:]
    text, fstart, flen, tab, nslots, _ = build(ksim, rows, 1)
    assert nslots == 1024 and tab[0] != ksim.lksim_empty() and tab[1] != ksim.lksim_empty(), "the chain does not wrap"
    ids, words = probe(ksim, gsim, rows, rows[::-1] + foreign + [None], 1)
    assert ids == list(range(6, -1, -1)) + [-1, -1, -1, -2]
    assert words[4] >= 6                # the longest walk passed the table's end


@pytest.mark.parametrize("bits", (0, 2))
def test_a_non_member_walks_a_long_chain(ksim, gsim, bits):
    rows = [(b"k%d" % i,) for i in range(200)]
    lines = [(b"k%d" % i,) for i in range(0, 400, 2)] + [None, (b"absent",)]
    ids, words = probe(ksim, gsim, rows, lines, 1, hash_bits=bits)
    assert ids[:100] == list(range(0, 200, 2)) and ids[100:200] == [-1] * 100 and ids[200:] == [-2, -1]
    # a non-member walks its whole home chain to the first empty word
    assert words[4] >= 200 >> bits
    if bits == 0:
        assert words[4] == 201
