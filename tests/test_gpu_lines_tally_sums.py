"""The line tally with sums (sre_hip_tally_sums_lines): the tally's rows, counts, key ids and index, and per key and value
column the sum (modulo 2^64), minimum, maximum and count of the numbers in a capture group of the key's lines.

Expected values are pure Python: the extract test's `expected` over groups + vgroups, the number rule as a regular
expression, and a dict in first-occurrence order.  Every successful call goes through the tally test's run_tally, so its
output, counts, key ids, index and info are checked against the plain tally's expectations for the same arguments.  The
sums buffer is an Out too: 64 guard bytes in front and behind, 0xA5 throughout, and every check asserts that nothing
beyond the rows the call may write has changed.
"""
import ctypes
import random
import re
import struct

import pytest

import sregex_amd as S
from test_gpu_lines import upload_at
from test_gpu_lines_filter import Out
from test_gpu_lines_extract import DOTTED, Program, expected, run_extract
from test_gpu_lines_tally import KV, run_tally

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
KVW = [rb"k=([a-z]*);v=([^;]*);w=([^;]*);"]        # the value groups hold arbitrary text
KNUM = [rb"k=([0-9]*);v=([^;]*);"]                  # a key that is a number
OCTETS = [rb"(\d{1,3})\.\d{1,3}\.\d{1,3}\.(\d{1,3})"]
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
IDENTITY = (0, INT64_MAX, INT64_MIN, 0)
NINES = b"9" * 18
# the table of tests/test_tally_sums_abi.py
NUMBERS = [(b"0", 0), (b"-0", 0), (b"007", 7), (NINES, 10 ** 18 - 1), (b"-" + NINES, -(10 ** 18 - 1))]
NOT_NUMBERS = [b"", b"-", b"--1", b"+1", b"1 ", b" 1", b"12a", b"1-", b"1" * 19, b"-" + b"1" * 19, NINES + b"\0"]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def number(text):
    return int(text) if re.fullmatch(rb"-?[0-9]{1,18}", text, re.DOTALL) else None


def wrap(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def aggregates(exp, data, delim, groups, vgroups, all_lines):
    """{key: [count, (sum, min, max, n) per value column]} in first-occurrence order"""
    K = len(groups)
    d = {}
    for _, _, _, fields in expected(exp, data, delim, list(groups) + list(vgroups), all_lines):
        key = tuple(data[f[0]:f[0] + f[1]] if f else b"" for f in fields[:K])
        row = d.setdefault(key, [0] + [IDENTITY] * len(vgroups))
        row[0] += 1
        for c, f in enumerate(fields[K:]):
            x = number(data[f[0]:f[0] + f[1]]) if f else None
            if x is not None:
                s, lo, hi, n = row[1 + c]
                row[1 + c] = (wrap(s + x), min(lo, x), max(hi, x), n + 1)
    return d


class SumsCall:
    """a scanner whose tally_lines is tally_sums_lines with this test's value groups and sums array: what run_tally of
    the tally's test calls, so that everything the two calls share is checked by the tally's own expectations"""

    def __init__(self, sc, vgroups, sums_ptr, sums_cap):
        self.sc, self.lib, self.vgroups, self.sums_ptr, self.sums_cap = sc, sc.lib, vgroups, sums_ptr, sums_cap

    def tally_lines(self, ptr, length, out_ptr, out_cap, groups, max_keys, delim, fsep, flags, counts_ptr, counts_cap, keyid_ptr,
                    keyid_cap, index_ptr, index_cap):
        return self.sc.tally_sums_lines(ptr, length, out_ptr, out_cap, groups, self.vgroups, max_keys, delim, fsep, flags,
                                        counts_ptr, counts_cap, self.sums_ptr, self.sums_cap, keyid_ptr, keyid_cap, index_ptr,
                                        index_cap)


def run_sums(sc, exp, data, groups, vgroups, sums_cap=None, spare=3, **kw):
    """one call, checked in full; returns (info, [[count, aggregates ..]] per key)"""
    want = aggregates(exp, data, kw.get("delim", 0x0A), groups, vgroups, kw.get("all_lines", False))
    V, nkeys = len(vgroups), len(want)
    scap = nkeys + spare if sums_cap is None else sums_cap
    sums = Out(sc.lib, scap * V * 32, 0)
    try:
        info, _, counts = run_tally(SumsCall(sc, vgroups, sums.ptr if scap else None, scap), exp, data, groups, **kw)
        if kw.get("overflow"):
            sums.check(b"")
            return info, []
        assert info.nkeys == nkeys and counts == [row[0] for row in want.values()]
        rows = list(want.values())[:min(scap, nkeys)]
        sums.check(b"".join(struct.pack("<qqqQ", *a) for row in rows for a in row[1:]))
        for c in range(V):
            assert sum(row[1 + c][3] for row in want.values()) <= info.nselected
            assert all(row[1 + c][3] <= row[0] for row in want.values())
    finally:
        sums.free()
    return info, list(want.values())


VALUES = [b"", b"x1", NINES, b"1" * 19, b"-" + NINES, b"-", b"0"]


def base6(j):
    return (bytes([b"abcxyz"[j % 6]]) + base6(j // 6)) if j else b""


def kvw_lines(seed, nlines, nkeys, miss=0.15, odd=0.3, span=1000):
    """lines around k=KEY;v=TEXT;w=TEXT; with TEXT mostly small integers; some lines have no match"""
    rng = random.Random(seed)
    keys = [base6(j) for j in range(nkeys)]         # (key 0 is the empty text)
    pads = [b"", b" ", b"-- ", b"at 12 "]
    out = []
    for i in range(nlines):
        if rng.random() < miss:
            out.append(b"no key here;v=1;")
            continue
        v, w = (rng.choice(VALUES) if rng.random() < odd else b"%d" % rng.randrange(-span, span) for _ in range(2))
        out.append(pads[i % 4] + b"k=" + rng.choice(keys) + b";v=" + v + b";w=" + w + b";" + pads[(i // 4) % 4])
    return b"\n".join(out) + (b"\n" if nlines % 2 else b"")


# ------------------------------------------------------------------ 1. the table-driven scanner

@pytest.mark.parametrize("groups", [[1], [1, 2]], ids=["K1", "K2"])
@pytest.mark.parametrize("vgroups", [[2], [2, 3]], ids=["V1", "V2"])
@pytest.mark.parametrize("all_lines", [False, True])
def test_table_driven(gpu, groups, vgroups, all_lines):
    data = kvw_lines(3, 400, 90, span=3)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        assert p.sc.engine == S.ENGINE_SCAN
        info, rows = run_sums(p.sc, p.exp, data, groups, vgroups, all_lines=all_lines)
        assert p.sc.last_lines_device == 1
        assert info.nlines == 400 and 60 < info.nkeys < info.nselected and (info.nselected == 400) == all_lines
        ns = [row[1][3] for row in rows]
        assert any(n < row[0] for n, row in zip(ns, rows)), "lines without a number"
        assert max(ns) > 1 or len(groups) == 2, "keys with several numbers"
        # an empty buffer, and one without any match
        assert run_sums(p.sc, p.exp, b"", groups, vgroups, all_lines=all_lines)[0] == S.TallyInfo(0, 0, 0, 0, 0, 0)
        info, rows = run_sums(p.sc, p.exp, b"nothing\nat all\n", groups, vgroups, all_lines=all_lines)
        assert info.nkeys == (1 if all_lines else 0)
        assert all(a == IDENTITY for row in rows for a in row[1:])


def test_an_unset_value_group(gpu):
    """group 3 of k=..(;v=(..))? is unset without ";v=" and empty behind a bare ";v=": neither is a number"""
    lines = [b"k=a;v=5", b"k=a", b"k=a;v=", b"k=b", b"k=a;v=7", b"k=b;v="]
    with S.Pool() as pool:
        p = Program(pool, KV)
        _, rows = run_sums(p.sc, p.exp, b"\n".join(lines), [1], [3, 2])
        assert rows == [[4, (12, 5, 7, 2), IDENTITY], [2, IDENTITY, IDENTITY]]


# ------------------------------------------------------------------ 2. contention, size, wrapping, the number rule

def test_one_key_in_many_workgroups(gpu):
    data = b"\n".join(b"%sk=same;v=%d;w=;" % (b" " * (i % 3), i - 2500) for i in range(5000))
    with S.Pool() as pool:
        p = Program(pool, KVW)
        _, rows = run_sums(p.sc, p.exp, data, [1], [2])
        assert rows == [[5000, (-2500, -2500, 2499, 5000)]]


def test_every_line_its_own_key(gpu):
    rng = random.Random(8)
    order = list(range(5000))
    rng.shuffle(order)
    data = b"\n".join(b"k=" + bytes(b"abcdefghij"[int(c)] for c in str(i)) + b";v=%d;w=x;" % (i * 3 - 7000) for i in order)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        info, rows = run_sums(p.sc, p.exp, data, [1], [2])
        assert info.nkeys == 5000
        assert rows == [[1, (i * 3 - 7000, i * 3 - 7000, i * 3 - 7000, 1)] for i in order]


def test_a_wrapping_sum(gpu):
    lines = [b"k=p;v=" + NINES + b";w=;"] * 12 + [b"k=m;v=-" + NINES + b";w=;"] * 12
    random.Random(5).shuffle(lines)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        _, rows = run_sums(p.sc, p.exp, b"\n".join(lines), [1], [2])
        big = 10 ** 18 - 1
        assert 12 * big > INT64_MAX
        got = {row[1] for row in rows}
        assert got == {(12 * big - (1 << 64), big, big, 12), ((1 << 64) - 12 * big, -big, -big, 12)}


def test_the_number_rule_on_the_device(gpu):
    texts = [t for t, _ in NUMBERS] + NOT_NUMBERS
    lines = [b"k=t;v=" + t + b";w=" + texts[-1 - j] + b";" for j, t in enumerate(texts)]
    with S.Pool() as pool:
        p = Program(pool, KVW)
        _, rows = run_sums(p.sc, p.exp, b"\n".join(lines), [1], [2, 3])
        big = 10 ** 18 - 1
        assert rows == [[len(texts), (7, -big, big, len(NUMBERS)), (7, -big, big, len(NUMBERS))]]


def test_a_column_without_any_number(gpu):
    lines = [b"k=a;v=1;w=x;", b"k=b;v=;w=2;", b"k=a;v=2;w=-;", b"k=b;v=y;w=3;", b"k=c;v=+1;w=1 ;"]
    with S.Pool() as pool:
        p = Program(pool, KVW)
        _, rows = run_sums(p.sc, p.exp, b"\n".join(lines), [1], [2, 3])
        assert rows == [[2, (3, 1, 2, 2), IDENTITY], [2, IDENTITY, (5, 2, 3, 2)], [1, IDENTITY, IDENTITY]]


# ------------------------------------------------------------------ 3. batches, probe chains, overflow

def test_a_keys_lines_fall_into_different_batches(gpu, monkeypatch):
    data = kvw_lines(11, 100, 12)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        _, one = run_sums(p.sc, p.exp, data, [1], [2, 3], src_off=1, dst_off=2)
        assert p.sc.last_line_batches == 1
        assert max(row[0] for row in one) > 7, "a key with more lines than a batch of 7 holds"
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "7")
        _, two = run_sums(p.sc, p.exp, data, [1], [2, 3], src_off=1, dst_off=2)
        assert p.sc.last_line_batches == 15 and one == two


def test_key_numbers_reach_their_rows_through_one_probe_chain(gpu, monkeypatch):
    monkeypatch.setenv("SRE_HIP_TALLY_HASH_BITS", "0")
    data = kvw_lines(20, 1500, 300, miss=0.05)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        info, _ = run_sums(p.sc, p.exp, data, [1], [2, 3])
        assert info.nkeys >= 290


@pytest.mark.parametrize("copies", ["1", "3"])
def test_the_copies_do_not_show(gpu, monkeypatch, copies):
    """the waves send to copies of the rows that a last kernel merges (64 of them for so few keys); SRE_HIP_TALLY_SUM_COPIES
    caps them: 1 sends to the caller's rows themselves, as a call with very many keys does"""
    data = kvw_lines(21, 1500, 9, miss=0.05)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        _, many = run_sums(p.sc, p.exp, data, [1], [2, 3])
        monkeypatch.setenv("SRE_HIP_TALLY_SUM_COPIES", copies)
        _, few = run_sums(p.sc, p.exp, data, [1], [2, 3])
        _, capped = run_sums(p.sc, p.exp, data, [1], [2, 3], sums_cap=4)
        assert many == few == capped and len(many) == 9


def test_overflow_writes_no_sums(gpu):
    data = kvw_lines(4, 700, 60)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        info, _ = run_sums(p.sc, p.exp, data, [1], [2, 3])
        nkeys = info.nkeys
        assert nkeys > 40
        run_sums(p.sc, p.exp, data, [1], [2, 3], max_keys=nkeys - 1, overflow=True)
        run_sums(p.sc, p.exp, data, [1], [2, 3], max_keys=nkeys)
        run_sums(p.sc, p.exp, data, [1], [2, 3], max_keys=1, overflow=True)


# ------------------------------------------------------------------ 4. capacities, arguments, alignment

def test_capacities(gpu):
    data = kvw_lines(6, 300, 40)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        info, _ = run_sums(p.sc, p.exp, data, [1], [2, 3])
        nkeys, need = info.nkeys, info.need_bytes
        assert nkeys > 30
        for scap in (nkeys + 3, nkeys, 5, 1, 0):
            for ccap, kcap, icap in ((None, None, None), (5, 17, 3), (0, 0, 0), (0, 300, 0), (nkeys, 0, 2)):
                run_sums(p.sc, p.exp, data, [1], [2, 3], sums_cap=scap, counts_cap=ccap, keyid_cap=kcap, index_cap=icap)
        row = len(data[data.index(b"k=") + 2:].split(b";")[0]) + 1
        for cap in (need, need - 1, row, 0):
            got, _ = run_sums(p.sc, p.exp, data, [1], [2, 3], out_cap=cap, dst_off=3)
            assert got.nkeys == nkeys and got.nwritten == {need: nkeys, need - 1: nkeys - 1, row: 1, 0: 0}[cap]
        # a sizing call still delivers the sums in full
        got, _ = run_sums(p.sc, p.exp, data, [1], [2, 3], out_cap=0, null_out=True, counts_cap=0, keyid_cap=0, index_cap=0)
        assert got.need_bytes == need and got.nwritten == 0


def test_bad_arguments(gpu):
    data = b"k=a;v=1;w=2;\nk=b;v=3;w=4;\n"
    src = upload_at(data, 0)
    out, sums = Out(gpu, 256, 0), Out(gpu, 16 * 2 * 32, 0)
    info = S.TallyInfoStruct()

    def call(sc, groups=(1,), vgroups=(2,), nv=None, flags=0, max_keys=16, fsep=0x09, out_ptr=None, cap=256, counts=(None, 0),
             keyid=(None, 0), sum_args=None):
        arr = (ctypes.c_int * len(groups))(*groups)
        varr = None if vgroups is None else (ctypes.c_int * max(len(vgroups), 1))(*vgroups)
        nv = (0 if vgroups is None else len(vgroups)) if nv is None else nv
        sp, scap = (sums.ptr, 16) if sum_args is None else sum_args
        return gpu.sre_hip_tally_sums_lines(sc.h, src.ptr, len(data), 0x0A, arr, len(groups), varr, nv, fsep, flags, max_keys,
                                            out.ptr if out_ptr is None else out_ptr, cap, counts[0], counts[1], sp, scap,
                                            keyid[0], keyid[1], None, 0, ctypes.byref(info), None)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, KVW))
            # Thompson and COUNT scanners have no first-match captures
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                assert call(S.Scanner(pool, prog, mode)) == -1
            sc = S.Scanner(pool, prog, FIRST)
            # the value columns
            assert call(sc, vgroups=()) == -1 and call(sc, vgroups=(2,) * 9) == -1
            assert call(sc, vgroups=None, nv=1) == -1
            assert call(sc, vgroups=(4,)) == -1 and call(sc, vgroups=(2, -1)) == -1
            assert call(sc, sum_args=(None, 3)) == -1
            assert call(sc, sum_args=(sums.ptr + 4, 3)) == -1
            # everything the tally refuses
            for mk in (0, S.HIP_TALLY_MAX_KEYS + 1):
                assert call(sc, max_keys=mk) == -1
            for flags in (S.HIP_LINES_INVERT, 4, 4 | S.HIP_LINES_ALL):
                assert call(sc, flags=flags) == -1
            assert call(sc, groups=(4,)) == -1 and call(sc, fsep=256) == -1
            assert call(sc, counts=(None, 3)) == -1 and call(sc, keyid=(None, 3)) == -1
            assert call(sc, out_ptr=src.ptr + 2, cap=4) == -1
            out.check(b"")
            sums.check(b"")
            assert call(sc, vgroups=(2, 3)) == 0 and info.nkeys == 2 and info.nselected == 2
            out.check(b"a\nb\n")
            sums.check(struct.pack("<" + "qqqQ" * 4, 1, 1, 1, 1, 2, 2, 2, 1, 3, 3, 3, 1, 4, 4, 4, 1))
            assert call(sc, vgroups=(2,) * 8) == 0
            sums.check(struct.pack("<qqqQ", 1, 1, 1, 1) * 8 + struct.pack("<qqqQ", 3, 3, 3, 1) * 8)
    finally:
        for b in (src, out, sums):
            b.free()


def test_a_value_group_that_is_a_key_group_and_one_named_twice(gpu):
    rng = random.Random(12)
    lines = [b"k=%d;v=%d;" % (rng.randrange(25), rng.randrange(-99, 99)) for _ in range(300)] + [b"k=;v=4;", b"k=007;v=x;"]
    with S.Pool() as pool:
        p = Program(pool, KNUM)
        _, rows = run_sums(p.sc, p.exp, b"\n".join(lines), [1], [1, 2, 2])
        assert len(rows) == 27
        for count, key, a, b in rows:
            assert a == b
            assert key == IDENTITY or key == (wrap(key[1] * count), key[1], key[1], count)
        assert rows[-2][1] == IDENTITY and rows[-1][1] == (7, 7, 7, 1) and rows[-1][2] == IDENTITY


@pytest.mark.parametrize("src_off", [1, 7, 13, 15])
def test_odd_alignments(gpu, src_off):
    data = kvw_lines(src_off, 260, 50).rstrip(b"\n -")
    data = data[:data.rindex(b"\n") + 1] + b"k=last;v=-12;w=345"        # the last value field ends the buffer
    with S.Pool() as pool:
        p = Program(pool, [rb"k=([a-z]*);v=([^;]*);w=([0-9]*)"])
        _, rows = run_sums(p.sc, p.exp, data, [1], [2, 3], src_off=src_off, dst_off=16 - src_off)
        assert rows[-1] == [1, (-12, -12, -12, 1), (345, 345, 345, 1)]


# ------------------------------------------------------------------ 5. the other routes

def dotted_lines(seed, nlines=600):
    rng = random.Random(seed)
    addrs = [b"%d.%d.%d.%d" % (rng.randrange(4), rng.randrange(256), rng.randrange(256), rng.randrange(256)) for _ in range(60)]
    return b"\n".join(rng.choice([b"GET / from ", b"", b"x "]) + rng.choice(addrs + [b"1.2.3", b"none"]) + b" ok" for _ in range(nlines))


@pytest.mark.parametrize("pats,groups,vgroups", [(DOTTED, [0], [1, 0]), (OCTETS, [1], [2, 1])], ids=["dotted", "octets"])
def test_the_nfa_tier_and_its_host_route(gpu, monkeypatch, pats, groups, vgroups):
    data = dotted_lines(2)
    with S.Pool() as pool:
        p = Program(pool, pats, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        info, one = run_sums(p.sc, p.exp, data, groups, vgroups, src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 1 and info.nselected < info.nlines
        monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
        _, two = run_sums(p.sc, p.exp, data, groups, vgroups, src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 0 and one == two
        if pats is OCTETS:
            assert len(one) == 4 and all(row[1][3] == row[0] and row[1][1] < row[1][2] for row in one)
        else:
            assert all(row[1] == IDENTITY and row[2] == IDENTITY for row in one), "'.7' and '1.2.3.4' are no numbers"


# ------------------------------------------------------------------ 6. the scanner's other calls

def test_the_scanners_other_calls_behave_as_on_a_fresh_scanner(gpu):
    data = kvw_lines(9, 500, 30)
    with S.Pool() as pool:
        p, fresh = Program(pool, KVW), Program(pool, KVW)
        _, want_rows, _ = run_extract(fresh.sc, fresh.exp, data, [1, 2], src_off=2, dst_off=9)
        _, want_keys, want_counts = run_tally(fresh.sc, fresh.exp, data, [1], src_off=2, dst_off=9)
        run_sums(p.sc, p.exp, data, [1], [2, 3], src_off=2, dst_off=9)
        run_sums(p.sc, p.exp, data, [1, 2], [3], max_keys=3, overflow=True)
        _, got_keys, got_counts = run_tally(p.sc, p.exp, data, [1], src_off=2, dst_off=9)
        _, got_rows, _ = run_extract(p.sc, p.exp, data, [1, 2], src_off=2, dst_off=9)
        assert (got_keys, got_counts) == (want_keys, want_counts) and got_rows == want_rows and len(want_rows) > 1000
        run_sums(p.sc, p.exp, data, [1], [3, 2], src_off=2, dst_off=9)
