"""The key map and the line join (sre_hip_keyset_create_map, sre_hip_join_lines) on the CPU: tests/lines_join_sim.cpp runs
the rules the kernels compile (sregex_amd/csrc/sre_lines_join.h, sre_lines_keyset.h and the join table of
sre_lines_gather.h): the split of a map's rows into key fields and value columns, the join pass line by line, and the
gather over the join table, tile by tile with the kernel's table slices and LDS window rule, counting every byte read from
the source and from the map's copy of the dictionary and every output byte written.  Expected values are a Python dict
join and Python-built rows."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
_p64, _p32, _p8, _pi64 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(_i64)
_cp, _int = ctypes.c_char_p, ctypes.c_int
FILL = 0xA5
NO_ROW = (1 << 64) - 1
VALUE_LENGTHS = (0, 1, 15, 16, 17, 40)


@pytest.fixture(scope="module")
def jsim():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "liblinesjoinsim.so")
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, "lines_join_sim.cpp")] + [os.path.join(csrc, h) for h in (
        "sre_lines_join.h", "sre_lines_keyset.h", "sre_lines_tally.h", "sre_lines_gather.h", "sre_lines_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    L = ctypes.CDLL(so)
    L.ljsim_window.restype = L.ljsim_max_values.restype = _u32
    for f in (L.ljsim_flag_last, L.ljsim_flag_unset, L.ljsim_flag_first, L.ljsim_flag_literal):
        f.restype = _u64
    L.ljsim_nslots.restype = _u64
    L.ljsim_nslots.argtypes = [_u64]
    L.ljsim_fields.restype = _u64
    L.ljsim_fields.argtypes = [_cp, _p64, _u64, _u32, _u32, _u32, _p64, _p64, _p64, _p64]
    L.ljsim_insert.restype = _u64
    L.ljsim_insert.argtypes = [_cp, _p64, _p64, _u64, _u32, _u64, _int, _p64]
    L.ljsim_join.restype = None
    L.ljsim_join.argtypes = [_cp, _p64, _p64, _p64, _u64, _u32, _cp, _p64, _p64, _p64, _p64, _u32, _p64, _u64, _int, _p32, _u32,
                             _int, _p64, _p64, _pi64, _pi64, _u64, _p64]
    L.ljsim_cut.restype = _u64
    L.ljsim_cut.argtypes = [_p64, _u64, _u64, _u64]
    L.ljsim_gather.restype = _u64
    L.ljsim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, _cp, _u64, _cp, _u64, _p8, _u64, _p32, _p32, _p32,
                               _p64, _p64]
    return L


class Map:
    """a key map on the CPU: rows are tuples of nfields field texts, the first nkeys the key"""

    def __init__(self, jsim, rows, nfields, nkeys, fsep=0x09, delim=0x0A, final_delim=True, hash_bits=64):
        self.rows, self.nfields, self.k, self.v = rows, nfields, nkeys, nfields - nkeys
        texts = [bytes([fsep]).join(r) for r in rows]
        self.text = bytes([delim]).join(texts) + (bytes([delim]) if rows and final_delim else b"")
        ends, pos = [], 0
        for t in texts:
            ends.append(pos + len(t))
            pos += len(t) + 1
        n = len(rows)
        self.fstart, self.flen = (_u64 * max(n * self.k, 1))(), (_u64 * max(n * self.k, 1))()
        self.vstart, self.vlen = (_u64 * max(n * self.v, 1))(), (_u64 * max(n * self.v, 1))()
        self.bad = jsim.ljsim_fields(self.text, (_u64 * max(n, 1))(*ends), n, nfields, nkeys, fsep, self.fstart, self.flen,
                                     self.vstart, self.vlen) if n else NO_ROW
        self.hash_bits = hash_bits
        self.nslots = jsim.ljsim_nslots(n)
        self.tab = (_u64 * self.nslots)(*([NO_ROW] * self.nslots))
        if n and self.bad == NO_ROW:
            assert jsim.ljsim_insert(self.text, self.fstart, self.flen, n, nkeys, self.nslots, hash_bits, self.tab) == 0
        self.first = {}
        for r, row in enumerate(rows):
            self.first.setdefault(tuple(row[:nkeys]), r)


def join_table(jsim, m, lines, keys, cols, all_lines, delim=0x0A, keyid_n=None):
    """the join pass over the lines (keys[i]: the line's key tuple as (offset, length) spans inside the line, or None for a
    line without a match): (val, start, own key ids, caller's key ids, words), checked against the Python dict join"""
    LAST, UNSET, FIRST, LIT = jsim.ljsim_flag_last(), jsim.ljsim_flag_unset(), jsim.ljsim_flag_first(), jsim.ljsim_flag_literal()
    n, P, k = len(lines), 1 + len(cols), m.k
    buf = bytes([delim]).join(lines) + bytes([delim])
    ends, vval, vstart, pos = [], [], [], 0
    for ln, key in zip(lines, keys):
        for f in range(k):
            vval.append(0 if key is None else key[f][1] + 1)
            vstart.append(pos + (0 if key is None else key[f][0]) | (FIRST if f == 0 else 0) | (LAST if f == k - 1 else 0))
        ends.append(pos + len(ln))
        pos += len(ln) + 1
    kn = n if keyid_n is None else keyid_n
    val, start = (_u64 * (n * P))(*([7] * (n * P))), (_u64 * (n * P))(*([7] * (n * P)))
    own, kid, words = (_i64 * n)(), (_i64 * (kn + 1))(*([77] * (kn + 1))), (_u64 * 3)()
    jsim.ljsim_join(buf, (_u64 * (n * k))(*vval), (_u64 * (n * k))(*vstart), (_u64 * n)(*ends), n, k, m.text, m.fstart, m.flen,
                    m.vstart, m.vlen, m.v, m.tab, m.nslots, m.hash_bits, (_u32 * len(cols))(*cols), len(cols), int(all_lines),
                    val, start, own, kid, min(kn, n), words)
    # the Python join
    want_val, want_start, want_ids, rows, pos = [], [], [], [], 0
    for ln, key in zip(lines, keys):
        texts = None if key is None else tuple(ln[a:a + b] for a, b in key)
        rid = -2 if key is None else m.first.get(texts, -1)
        sel = all_lines or rid >= 0
        vals = [m.rows[rid][m.k + c] if rid >= 0 else b"" for c in cols]
        want_ids.append(rid)
        want_val += [len(ln) + 1 if sel else 0] + [len(v) + 1 if sel else 0 for v in vals]
        want_start.append(pos | FIRST)
        for x, c in enumerate(cols):
            last = LAST if x == len(cols) - 1 else 0
            if rid >= 0:
                w = m.vstart[rid * m.v + c]
                assert m.text[w:w + len(vals[x])] == vals[x]
                want_start.append(w | LIT | last)
            else:
                want_start.append(UNSET | last)
        if sel:
            rows.append((ln, vals))
        pos += len(ln) + 1
    assert list(val) == want_val
    assert list(start) == want_start
    assert list(own) == want_ids and list(kid)[:min(kn, n)] == want_ids[:kn] and kid[min(kn, n)] == 77
    assert list(words) == [sum(1 for v in want_ids if v != -2), sum(1 for v in want_ids if v >= 0), 0]
    return buf, list(val), list(start), rows, want_ids


def gather(jsim, m, buf, val, start, rows, src_off, dst_off, jsep=0x09, delim=0x0A, out_cap=None, P=None):
    """the gather over the table for one pair of heads; asserts the cut, what it writes and where it reads and writes;
    returns (windowed, global)"""
    nent = len(val)
    n = nent // P
    off = [0]
    for v in val:
        off.append(off[-1] + v)
    texts = [ln + b"".join(bytes([jsep]) + v for v in vals) + bytes([delim]) for ln, vals in rows]
    need = off[-1]
    assert sum(len(t) for t in texts) == need
    a_off, a_start = (_u64 * (nent + 1))(*off), (_u64 * max(nent, 1))(*start)
    cap = need if out_cap is None else out_cap
    cut = jsim.ljsim_cut(a_off, n, P, cap)
    out_bytes, want, nw = off[cut * P], b"", 0
    while nw < len(texts) and len(want) + len(texts[nw]) <= cap:
        want += texts[nw]
        nw += 1
    assert out_bytes == len(want)
    src_len = (src_off + len(buf) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
    lit = m.text + bytes([0xDD]) * 16           # the map's copy: its text and the 16 bytes allocated behind it
    dst_len = (dst_off + out_bytes + 15) // 16 * 16 + 16
    dst = (ctypes.c_uint8 * dst_len)(*([FILL] * dst_len))
    reads, lit_reads, writes = (_u32 * src_len)(), (_u32 * len(lit))(), (_u32 * dst_len)()
    win, glo = _u64(), _u64()
    bad = jsim.ljsim_gather(a_off, a_start, nent, out_bytes, src_off, dst_off, delim, jsep, src, src_len, lit, len(lit), dst, dst_len,
                            reads, lit_reads, writes, ctypes.byref(win), ctypes.byref(glo))
    assert bad == 0
    got = bytes(dst)
    assert got[dst_off:dst_off + out_bytes] == want
    assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + out_bytes:] == bytes([FILL]) * (dst_len - dst_off - out_bytes)
    w = list(writes)
    assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes and sum(w) == out_bytes         # every byte once, nothing else
    return win.value, glo.value


def keyed_lines(rng, nlines, keys, miss=0.2, nokey=0.2):
    """lines "<filler>k=<key>;<filler>" with the span of the key; some keys are foreign, some lines have no key"""
    lines, spans = [], []
    for _ in range(nlines):
        head = bytes(rng.choice(b"abcxyz ") for _ in range(rng.randrange(0, 20)))
        x = rng.random()
        if x < nokey:
            lines.append(head)
            spans.append(None)
            continue
        key = b"zz%d" % rng.randrange(100) if x < nokey + miss else rng.choice(keys)
        lines.append(head + b"k=" + key + b";" + bytes(rng.choice(b"pqr") for _ in range(rng.randrange(0, 9))))
        spans.append([(len(head) + 2, len(key))])
    return lines, spans


def aligned_map(jsim, final_delim=True):
    """a map of one key field and two value columns in which column 0 takes every length of VALUE_LENGTHS at every
    alignment in the dictionary (the key is padded to place it); without the final delimiter the last value is the
    dictionary's last bytes"""
    rows, pos, r = [], 0, 0
    for n in VALUE_LENGTHS:
        for a in range(16):
            key = b"key%d" % r
            key += b"_" * ((a - (pos + len(key) + 1)) % 16)
            v0 = bytes(0x41 + (r + j) % 26 for j in range(n))
            v1 = b"%d" % (r % 7)
            rows.append((key, v0, v1))
            assert (pos + len(key) + 1) % 16 == a
            pos += len(key) + 1 + len(v0) + 1 + len(v1) + 1
            r += 1
    # and a last row whose column 1 is 40 bytes: the end of the text
    rows.append((b"last", b"x", bytes(0x61 + j % 26 for j in range(40))))
    return Map(jsim, rows, 3, 1, final_delim=final_delim)


# ------------------------------------------------------------------ the map's fields

def test_fields_part_into_keys_and_values(jsim):
    rows = [(b"a", b"b", b"v0", b"", b"v2"), (b"", b"", b"", b"", b""), (b"a", b"b", b"other", b"x", b"y")]
    m = Map(jsim, rows, 5, 2)
    assert m.bad == NO_ROW and m.first == {(b"a", b"b"): 0, (b"", b""): 1}
    for r, row in enumerate(rows):
        for f in range(2):
            s, n = m.fstart[r * 2 + f], m.flen[r * 2 + f]
            assert m.text[s:s + n] == row[f]
        for c in range(3):
            s, n = m.vstart[r * 3 + c], m.vlen[r * 3 + c]
            assert m.text[s:s + n] == row[2 + c]


def test_the_lowest_bad_row_is_named(jsim):
    m = Map(jsim, [(b"a", b"1"), (b"b",), (b"c", b"2", b"3"), (b"d", b"4")], 2, 1)
    assert m.bad == 1
    assert Map(jsim, [(b"a", b"1"), (b"c", b"2", b"3")], 2, 1).bad == 1


# ------------------------------------------------------------------ the entry rule

@pytest.mark.parametrize("all_lines", [False, True], ids=["inner", "all"])
@pytest.mark.parametrize("hash_bits", [64, 2, 0])
def test_entry_rule_against_a_dict_join(jsim, all_lines, hash_bits):
    rng = random.Random(hash_bits * 2 + all_lines)
    keys = [b"key%d" % i for i in range(40)] + [b""]
    rows = [(k, b"v%d" % i, b"w" * (i % 5), b"") for i, k in enumerate(keys)]
    rows += [(rng.choice(keys), b"dup", b"dup", b"dup") for _ in range(15)]          # later rows of a key are ignored
    rng.shuffle(rows)
    m = Map(jsim, rows, 4, 1, final_delim=bool(hash_bits), hash_bits=hash_bits)
    lines, spans = keyed_lines(rng, 300, keys)
    for cols in ([0], [2, 0, 0, 1], [1] * 31):
        _, _, _, out, ids = join_table(jsim, m, lines, spans, cols, all_lines, keyid_n=rng.choice([0, 1, 300, 17]))
        assert len(out) == (300 if all_lines else sum(1 for v in ids if v >= 0)) and -1 in ids and -2 in ids


def test_two_key_fields_and_an_empty_map(jsim):
    rows = [(b"ab", b"c", b"one"), (b"a", b"bc", b"two"), (b"ab", b"c", b"never")]
    m = Map(jsim, rows, 3, 2)
    lines = [b"ab|c", b"a|bc", b"abc|", b"none"]
    spans = [[(0, 2), (3, 1)], [(0, 1), (2, 2)], [(0, 3), (4, 0)], None]
    for all_lines in (False, True):
        _, _, _, out, ids = join_table(jsim, m, lines, spans, [0], all_lines)
        assert ids == [0, 1, -1, -2] and [v for _, v in out][:2] == [[b"one"], [b"two"]]
    empty = Map(jsim, [], 3, 2)
    _, val, _, out, ids = join_table(jsim, empty, lines, spans, [0, 0], False)
    assert ids == [-1, -1, -1, -2] and out == [] and not any(val)
    _, val, _, out, ids = join_table(jsim, empty, lines, spans, [0, 0], True)
    assert [v for _, v in out] == [[b"", b""]] * 4


# ------------------------------------------------------------------ the gather

@pytest.mark.parametrize("final_delim", [True, False], ids=["delim", "no_final_delim"])
def test_gather_every_head_and_every_value_alignment(jsim, final_delim):
    m = aligned_map(jsim, final_delim)
    assert m.bad == NO_ROW
    seen = {(m.vlen[r * 2], m.vstart[r * 2] % 16) for r in range(len(m.rows) - 1)}
    assert seen == {(n, a) for n in VALUE_LENGTHS for a in range(16)}
    last = len(m.rows) - 1
    assert m.vlen[last * 2 + 1] == 40 and (m.vstart[last * 2 + 1] + 40 == len(m.text)) == (not final_delim)
    rng = random.Random(5)
    lines, spans = [], []
    for r, row in enumerate(m.rows):           # every row is joined, in an order of its own, with lines of many lengths
        head = b"." * ((r * 7) % 23)
        lines.append(head + row[0])
        spans.append([(len(head), len(row[0]))])
    lines += [b"", b"no key here", b"missing"]
    spans += [None, None, [(0, 7)]]
    order = list(range(len(lines)))
    rng.shuffle(order)
    lines, spans = [lines[i] for i in order], [spans[i] for i in order]
    for all_lines in (False, True):
        for cols in ([0, 1], [1, 0, 0]):
            buf, val, start, rows, _ = join_table(jsim, m, lines, spans, cols, all_lines)
            for src_off in range(16):
                for dst_off in range(16):
                    win, glo = gather(jsim, m, buf, val, start, rows, src_off, dst_off, P=1 + len(cols))
                    assert win >= 1 and glo == 0
    # truncation: whole rows only, at every row boundary of the first rows and one byte on either side
    buf, val, start, rows, _ = join_table(jsim, m, lines, spans, [0, 1], True)
    edge = 0
    for ln, vals in rows[:6]:
        edge += len(ln) + 1 + sum(len(v) + 1 for v in vals)
        for cap in (edge - 1, edge, edge + 1):
            gather(jsim, m, buf, val, start, rows, 3, 9, out_cap=cap, P=3)
    gather(jsim, m, buf, val, start, rows, 3, 9, out_cap=0, P=3)


@pytest.mark.parametrize("heads", [(0, 0), (5, 11), (15, 1)])
def test_gather_takes_the_global_table_for_short_rows(jsim, heads):
    """rows of 3 bytes (an empty line, two empty values): a 16 KiB tile spans more entries than the window holds; rows with
    values in between"""
    m = Map(jsim, [(b"k", b"value-0", b"v1")], 3, 1, final_delim=False)
    lines = [b""] * 6000 + [b"k"] * 40 + [b""] * 3000 + [b"k"] * 3000
    spans = [None if not ln else [(0, 1)] for ln in lines]
    buf, val, start, rows, _ = join_table(jsim, m, lines, spans, [1, 0], True)
    win, glo = gather(jsim, m, buf, val, start, rows, heads[0], heads[1], P=3)
    assert glo >= 1 and win >= 1 and jsim.ljsim_window() == 1024
    buf, val, start, rows, _ = join_table(jsim, m, lines, spans, [1, 0], False)
    assert len(rows) == 3040
    win, glo = gather(jsim, m, buf, val, start, rows, heads[0], heads[1], P=3)
    assert glo >= 1             # the unselected lines' entries lie inside the slices of the first tiles
