"""The line route by key (sre_hip_route_lines_by_key): the lines of a device buffer grouped by the dictionary row of their
captured key, bucket-major in ONE output buffer, with the key id of every line, index rows and a device table of the
non-empty buckets.

Expected values are pure Python: the lookup test's key sets and keys (make_set, keys_of: the split rule of line mode and the
oracle's first-match record of every line), then a stable sort by (id, line) with the ids -1 and -2 behind the dictionary's.
Output, key-id, index and bucket buffers have 64 guard bytes in front and behind and are pre-filled with 0xA5 (the filter
test's Out); every call asserts that the guards and everything beyond what the call may write still hold 0xA5.

run_route_key asserts a condition on its INPUT as well: unless the case says otherwise, a buffer of four or more selected
lines holds at least two non-empty buckets and at least one bucket with two lines that are not adjacent in the buffer, so
that an output in line order, or one grouped by runs, cannot pass.
"""
import ctypes
import itertools
import random

import pytest

import sregex_amd as S
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import Out, run_filter
from test_gpu_lines_extract import DOTTED, Program
from test_gpu_lines_tally import KV, kv_lines, words, dotted_lines
from test_gpu_lines_lookup import make_set, keys_of, run_lookup, half_and_foreign, letters
from test_gpu_lines_join import make_map, run_join
from test_gpu_lines_route import setup as route_setup, run_route

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
SIZES = (1, 63, 64, 65, 257, 1024 + 17, 2 * 1024 + 1)


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def sort_key(i, nrows):
    return i if i >= 0 else nrows if i == -1 else nrows + 1


def expect(exp, data, groups, ids, nrows, all_lines, delim=0x0A):
    """(key id per line, keyed lines, [(line, start, len, id)] in output order)"""
    lines = split_lines(data, delim)
    want_ids = [-2] * len(lines)
    keyed = keys_of(exp, data, groups, delim)
    for i, _, _, key in keyed:
        want_ids[i] = ids.get(key, -1)
    sel = [(i, st, n, want_ids[i]) for i, (st, n) in enumerate(lines) if all_lines or want_ids[i] >= 0]
    sel.sort(key=lambda r: sort_key(r[3], nrows))           # stable: line order inside a bucket
    return want_ids, keyed, sel


def shape_holds(sel):
    """at least two buckets, and one bucket with two lines that are not adjacent in the buffer"""
    groups = [[r[0] for r in g] for _, g in itertools.groupby(sel, key=lambda r: r[3])]
    return len(groups) >= 2 and any(b - a > 1 for g in groups for a, b in zip(g, g[1:]))


def run_route_key(sc, exp, data, groups, ks, ids, all_lines=False, delim=0x0A, src_off=0, dst_off=0, out_cap=None,
                  keyid_cap=None, index_cap=None, buckets_cap=None, null_out=False, shape=True):
    """one call, checked in full; returns (info, output bytes, key ids of all lines, bucket rows)"""
    lib = sc.lib
    d = bytes([delim])
    nrows = ks.rows
    nlines = len(split_lines(data, delim))
    want_ids, keyed, sel = expect(exp, data, groups, ids, nrows, all_lines, delim)
    if shape and len(sel) >= 4:
        assert shape_holds(sel), "the case's input does not exercise the grouping"
    nmembers = sum(1 for v in want_ids if v >= 0)
    need = sum(n + 1 for _, _, n, _ in sel)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for _, _, n, _ in sel:
        if out_bytes + n + 1 > cap:
            break
        out_bytes += n + 1
        nwritten += 1
    want = b"".join(data[st:st + n] + d for _, st, n, _ in sel[:nwritten])
    want_buckets, rank, at = [], 0, 0
    for kid_, g in itertools.groupby(sel, key=lambda r: r[3]):
        g = list(g)
        by = sum(r[2] + 1 for r in g)
        want_buckets.append((kid_, rank, len(g), at, by))
        rank += len(g)
        at += by
    assert [b[0] for b in want_buckets] == sorted({r[3] for r in sel}, key=lambda i: sort_key(i, nrows))
    kcap = nlines + 3 if keyid_cap is None else keyid_cap
    icap = len(sel) + 3 if index_cap is None else index_cap
    bcap = len(want_buckets) + 3 if buckets_cap is None else buckets_cap
    src = upload_at(data, src_off)
    out, kid, idx, bkt = Out(lib, cap, dst_off), Out(lib, kcap * 8, 0), Out(lib, icap * 40, 0), Out(lib, bcap * 40, 0)
    try:
        info = sc.route_lines_by_key(src.ptr + src_off, len(data), None if null_out else out.ptr, cap, groups, ks, delim, all_lines,
                                     kid.ptr if kcap else None, kcap, idx.ptr if icap else None, icap, bkt.ptr if bcap else None, bcap)
        assert info == S.RouteKeyInfo(nlines, len(keyed), nmembers, len(sel), len(want_buckets), need, nwritten, out_bytes), \
            (info, len(keyed), nmembers, len(sel), len(want_buckets), need, nwritten, out_bytes)
        out.check(want)
        got_ids = words(lib, kid, min(kcap, nlines))
        assert got_ids == want_ids[:kcap], [(i, g, w) for i, (g, w) in enumerate(zip(got_ids, want_ids)) if g != w][:3]
        nidx = min(icap, nwritten)
        rows, o = [], 0
        for i, st, n, kid_ in sel[:nidx]:
            rows.append((i, st, n, o, kid_))
            o += n + 1
        raw = words(lib, idx, 5 * nidx)
        got = [tuple(raw[5 * r:5 * r + 5]) for r in range(nidx)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
        nb = min(bcap, len(want_buckets))
        raw = words(lib, bkt, 5 * nb)
        got = [tuple(raw[5 * r:5 * r + 5]) for r in range(nb)]
        assert got == want_buckets[:nb], [(g, w) for g, w in zip(got, want_buckets) if g != w][:3]
    finally:
        for b in (src, out, kid, idx, bkt):
            b.free()
    return info, want, want_ids, want_buckets


def keyed_text(seed, nlines, keys, miss=0.1, foreign=0.1, final_delim=None):
    """lines around k=KEY from `keys` (byte strings of a-z), some with a key the pool does not hold, some without one"""
    rng = random.Random(seed)
    pads = [b"", b" ", b"-- ", b"at 12 "]
    out = []
    for i in range(nlines):
        r = rng.random()
        if r < miss:
            out.append(b"no key here")
        elif r < miss + foreign:
            out.append(pads[i % 4] + b"k=qq" + rng.choice(keys)[:3] + b" ")
        else:
            out.append(pads[i % 4] + b"k=" + rng.choice(keys) + pads[(i // 4) % 4])
    final = nlines % 2 == 1 if final_delim is None else final_delim
    return b"\n".join(out) + (b"\n" if final else b"")


# ------------------------------------------------------------------ 1. the table-driven scanner

@pytest.mark.parametrize("groups", [[1], [1, 3]], ids=["K1", "K2"])
@pytest.mark.parametrize("n", SIZES)
def test_table_driven(gpu, groups, n):
    rng = random.Random(n * 2 + len(groups))
    data = kv_lines(n + len(groups), n, 30, longest=12)
    with S.Pool() as pool:
        p = Program(pool, KV)
        assert p.sc.engine == S.ENGINE_SCAN
        keyed = keys_of(p.exp, data, groups)
        if n == 1 and not keyed:
            data = b"x k=only;v=7 y"
            keyed = keys_of(p.exp, data, groups)
        ks, ids = make_set(half_and_foreign(rng, keyed, len(groups)), len(groups), off=rng.randrange(1, 16), final_delim=n % 2 == 0)
        try:
            for all_lines in (False, True):
                # (source and destination at odd alignments)
                so, do = rng.randrange(1, 16) | 1, rng.randrange(1, 16) | 1
                info, out, _, _ = run_route_key(p.sc, p.exp, data, groups, ks, ids, all_lines, src_off=so, dst_off=do)
                assert p.sc.last_lines_device == 1 and info.nkeyed == len(keyed)
                if n >= 63:
                    assert 0 < info.nmembers < info.nkeyed < info.nlines and info.nbuckets >= 3
                assert info.nselected == (info.nlines if all_lines else info.nmembers)
        finally:
            ks.close()


def test_all_lines_is_a_permutation_of_the_input(gpu):
    data = kv_lines(77, 500, 25)            # (even: the final line has no delimiter)
    assert not data.endswith(b"\n")
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(half_and_foreign(random.Random(7), keys_of(p.exp, data, [1]), 1), 1)
        try:
            info, out, kid, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids, True, src_off=5, dst_off=3)
            assert sorted(out[:-1].split(b"\n")) == sorted(data.split(b"\n")) and info.nselected == info.nlines == 500
            assert [b[0] for b in buckets[-2:]] == [-1, -2]
            # the final line got its delimiter wherever its bucket put it
            assert out.count(b"\n") == 500 and len(out) == len(data) + 1
        finally:
            ks.close()


# ------------------------------------------------------------------ 2. digit passes

def boundary_case(nrows, seed, nlines=300):
    """a set of nrows rows and lines whose members come from both ends of the id range"""
    rows = [(letters(i),) for i in range(nrows)]
    ends = [letters(i) for i in list(range(0, 6)) + list(range(max(nrows - 6, 0), nrows)) + [nrows // 2, nrows // 3]]
    return rows, keyed_text(seed, nlines, sorted(set(ends)))


@pytest.mark.parametrize("nrows", (254, 255, 256, 257))
def test_pass_boundaries(gpu, nrows):
    """with ALL the largest sort key is nrows + 1: 255 takes one pass of 8 bits, 256 / 257 / 258 two"""
    rows, data = boundary_case(nrows, nrows)
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(rows, 1)
        try:
            info, _, _, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids, True, src_off=1, dst_off=7)
            got = [b[0] for b in buckets]
            assert got[0] == 0 and nrows - 1 in got and got[-2:] == [-1, -2] and info.nbuckets == len(got) >= 12
            run_route_key(p.sc, p.exp, data, [1], ks, ids, False, src_off=1, dst_off=7)
        finally:
            ks.close()


@pytest.fixture(scope="module")
def big_set(gpu):
    """65 535 rows, a few hundred KB of dictionary text, built once"""
    ks, ids = make_set([(letters(i),) for i in range(65535)], 1)
    yield ks, ids
    ks.close()


@pytest.mark.parametrize("all_lines", (False, True))
def test_65535_rows(gpu, big_set, all_lines):
    """the largest sort key is 65534 (two passes), with ALL 65536 (three)"""
    ks, ids = big_set
    assert ks.rows == 65535
    ends = [letters(i) for i in (0, 1, 2, 255, 256, 257, 4095, 4096, 32767, 32768, 65279, 65280, 65532, 65533, 65534)]
    data = keyed_text(9, 1500, ends)
    with S.Pool() as pool:
        p = Program(pool, KV)
        info, _, _, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids, all_lines, src_off=3, dst_off=9)
        got = [b[0] for b in buckets]
        assert got[:3] == [0, 1, 2] and 65534 in got and 32768 in got and info.nbuckets == (17 if all_lines else 15)


@pytest.mark.parametrize("bits,passes", (("1", 9), ("2", 5), ("5", 2)))
def test_narrow_digits_take_many_passes(gpu, monkeypatch, bits, passes):
    """300 rows: 9 bits of sort key, so 9, 5 and 2 passes; the results are those of the default width"""
    rows = [(letters(i),) for i in range(300)]
    data = keyed_text(11, 1024 + 300, [letters(i) for i in range(0, 300, 7)] + [letters(299), letters(256), letters(255)])
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(rows, 1)
        try:
            one = [run_route_key(p.sc, p.exp, data, [1], ks, ids, a, src_off=2, dst_off=5) for a in (False, True)]
            monkeypatch.setenv("SRE_HIP_ROUTE_KEY_DIGIT_BITS", bits)
            two = [run_route_key(p.sc, p.exp, data, [1], ks, ids, a, src_off=2, dst_off=5) for a in (False, True)]
            assert one == two and one[0][0].nbuckets > 40
            for junk in ("0", "9", "x"):
                monkeypatch.setenv("SRE_HIP_ROUTE_KEY_DIGIT_BITS", junk)           # anything else means 8
                assert run_route_key(p.sc, p.exp, data, [1], ks, ids, True, src_off=2, dst_off=5) == one[1]
        finally:
            ks.close()


def test_both_rank_rules_give_the_same_output(gpu, monkeypatch):
    rows = [(letters(i),) for i in range(300)]
    data = keyed_text(12, 1024 + 100, [letters(i) for i in range(300)])          # up to 64 distinct digits in a slot
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(rows, 1)
        try:
            one = run_route_key(p.sc, p.exp, data, [1], ks, ids, True, src_off=2, dst_off=5)
            monkeypatch.setenv("SRE_HIP_ROUTE_KEY_RANK", "turns")
            assert run_route_key(p.sc, p.exp, data, [1], ks, ids, True, src_off=2, dst_off=5) == one
            monkeypatch.setenv("SRE_HIP_ROUTE_KEY_DIGIT_BITS", "3")
            assert run_route_key(p.sc, p.exp, data, [1], ks, ids, True, src_off=2, dst_off=5) == one
        finally:
            ks.close()


# ------------------------------------------------------------------ 3. keys and sets

def test_all_lines_one_key(gpu):
    data = b"\n".join(b"%d k=same %d" % (i, i * 7) for i in range(1100)) + b"\n"
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set([(b"other",), (b"same",), (b"more",)], 1)
        try:
            for all_lines in (False, True):
                info, out, _, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids, all_lines, shape=False)
                assert out == data and buckets == [(1, 0, 1100, 0, len(data))] and info.nbuckets == 1
        finally:
            ks.close()


def test_every_line_its_own_key_and_descending_ids(gpu):
    n = 1024 + 50
    lines = [b"k=" + letters(i) for i in range(n)]
    data = b"\n".join(lines)
    with S.Pool() as pool:
        p = Program(pool, KV)
        # row r holds the key of line n - 1 - r: the ids descend with the line number, the output is the input reversed
        ks, ids = make_set([(letters(n - 1 - r),) for r in range(n)], 1)
        try:
            info, out, kid, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids, shape=False, dst_off=1)
            assert kid == list(range(n - 1, -1, -1)) and out == b"".join(ln + b"\n" for ln in reversed(lines))
            assert info.nbuckets == n and all(b[2] == 1 for b in buckets)
        finally:
            ks.close()


def test_ids_descend_with_the_line_number(gpu):
    """blocks of lines: the later the block, the lower its dictionary row"""
    n, nkeys = 1200, 40
    lines = [b"k=" + letters(i * nkeys // n) + b" #%d" % i for i in range(n)]
    for i in range(0, n, 97):
        lines[i] = b"k=" + letters(0) + b" early"          # (a bucket whose lines are far apart)
    data = b"\n".join(lines) + b"\n"
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set([(letters(nkeys - 1 - r),) for r in range(nkeys)], 1)
        try:
            info, out, _, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids, src_off=9)
            assert [b[0] for b in buckets] == list(range(nkeys)) and out.startswith(b"k=" + letters(nkeys - 1))
        finally:
            ks.close()


def test_duplicate_rows_and_keys_no_line_carries(gpu):
    """the lowest row of a key is its id, so the ids have gaps; a key no line carries has no bucket row"""
    rows = [(b"b",), (b"a",), (b"b",), (b"unused",), (b"c",), (b"a",), (b"",), (b"",), (b"c",), (b"never",)]
    data = b"k=c 1\nk=a 2\nk= 3\nk=b 4\nk=d 5\nnone 6\nk=c 7\nk=b 8\nk=a 9\nk= 10\nk=c 11\n"
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(rows, 1, final_delim=False)
        try:
            assert ks.rows == 10 and ks.distinct == 6
            info, out, kid, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids)
            assert kid == [4, 1, 6, 0, -1, -2, 4, 0, 1, 6, 4]
            assert out == b"k=b 4\nk=b 8\nk=a 2\nk=a 9\nk=c 1\nk=c 7\nk=c 11\nk= 3\nk= 10\n"
            assert [b[:3] for b in buckets] == [(0, 0, 2), (1, 2, 2), (4, 4, 3), (6, 7, 2)]
            info, out, _, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids, True)
            assert out.endswith(b"k= 10\nk=d 5\nnone 6\n") and [b[0] for b in buckets] == [0, 1, 4, 6, -1, -2]
        finally:
            ks.close()


def test_an_empty_set_and_an_empty_buffer(gpu):
    data = kv_lines(5, 300, 20)
    with S.Pool() as pool:
        p = Program(pool, KV)
        empty, none = make_set([], 1)
        ks, ids = make_set([(b"a",)], 1)
        try:
            info, out, _, buckets = run_route_key(p.sc, p.exp, data, [1], empty, none)
            assert (info.nselected, info.nbuckets, out, buckets) == (0, 0, b"", []) and info.nkeyed > 0
            info, out, _, buckets = run_route_key(p.sc, p.exp, data, [1], empty, none, True, dst_off=3)
            assert info.nselected == info.nlines == 300 and [b[0] for b in buckets] == [-1, -2]
            assert buckets[0][2] == info.nkeyed and buckets[1][2] == 300 - info.nkeyed
            # no keyed line at all: one rest bucket, the input as it is
            plain = b"nothing\nhere\nat all\n"
            info, out, _, buckets = run_route_key(p.sc, p.exp, plain, [1], empty, none, True)
            assert out == plain and buckets == [(-2, 0, 3, 0, len(plain))]
            for target in (ks, empty):
                for all_lines in (False, True):
                    info, out, _, buckets = run_route_key(p.sc, p.exp, b"", [1], target, ids if target is ks else none, all_lines)
                    assert info == S.RouteKeyInfo(0, 0, 0, 0, 0, 0, 0, 0) and out == b"" and buckets == []
        finally:
            empty.close()
            ks.close()


@pytest.mark.parametrize("final_delim", (False, True))
def test_a_final_line_without_a_delimiter(gpu, final_delim):
    keys = [letters(i) for i in range(9)]
    data = keyed_text(21, 200, keys, final_delim=final_delim)
    if not final_delim:
        data += b"\nk=" + keys[0]           # the final line belongs to the FIRST bucket
    assert data.endswith(b"\n") == final_delim
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set([(k,) for k in keys], 1)
        try:
            info, out, _, _ = run_route_key(p.sc, p.exp, data, [1], ks, ids, True, src_off=11, dst_off=13)
            assert out.endswith(b"\n") and info.need_bytes == len(data) + (0 if final_delim else 1)
        finally:
            ks.close()


# ------------------------------------------------------------------ 4. capacities

def test_truncation_the_sizing_call_and_the_side_arrays(gpu):
    data = kv_lines(6, 300, 40)
    rng = random.Random(6)
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(half_and_foreign(rng, keys_of(p.exp, data, [1, 3]), 2), 2)
        try:
            for all_lines in (False, True):
                info, out, _, buckets = run_route_key(p.sc, p.exp, data, [1, 3], ks, ids, all_lines)
                need, row = info.need_bytes, out.index(b"\n") + 1
                assert info.out_bytes == need > row and info.nselected > 3 and info.nbuckets > 3
                for cap in (need, need - 1, row, 0):
                    got, _, _, same = run_route_key(p.sc, p.exp, data, [1, 3], ks, ids, all_lines, out_cap=cap, dst_off=3)
                    assert (got.nkeyed, got.nmembers, got.need_bytes, got.nbuckets) == (info.nkeyed, info.nmembers, need, info.nbuckets)
                    assert got.nwritten == {need: info.nselected, need - 1: info.nselected - 1, row: 1, 0: 0}[cap]
                    assert same == buckets          # the bucket table does not depend on out_cap
                got, _, _, same = run_route_key(p.sc, p.exp, data, [1, 3], ks, ids, all_lines, out_cap=0, null_out=True)
                assert got.need_bytes == need and got.nwritten == 0 and same == buckets         # a sizing call
                for kcap, icap, bcap in ((17, 3, 2), (1, 1, 1), (0, 0, 0), (300, 0, 1), (0, 2, 0), (5, 0, info.nbuckets - 1)):
                    run_route_key(p.sc, p.exp, data, [1, 3], ks, ids, all_lines, keyid_cap=kcap, index_cap=icap, buckets_cap=bcap)
        finally:
            ks.close()


# ------------------------------------------------------------------ 5. beside the other calls

def test_a_set_of_one_row_is_the_lookup(gpu):
    data = kv_lines(8, 400, 12)
    with S.Pool() as pool:
        p = Program(pool, KV)
        keyed = keys_of(p.exp, data, [1])
        key = max({k for _, _, _, k in keyed}, key=lambda k: sum(1 for x in keyed if x[3] == k))
        ks, ids = make_set([key], 1)
        try:
            linfo, lout, lkid = run_lookup(p.sc, p.exp, data, [1], ks, ids, src_off=3, dst_off=5)
            info, out, kid, buckets = run_route_key(p.sc, p.exp, data, [1], ks, ids, src_off=3, dst_off=5, shape=False)
            assert out == lout and kid == lkid and len(out) > 0
            assert (info.nlines, info.nkeyed, info.nmembers, info.nselected, info.need_bytes, info.nwritten, info.out_bytes) == tuple(linfo)
            # index words 0 .. 3 are the lookup's rows
            n = info.nselected
            src = upload_at(data, 3)
            a, b, o = S.DeviceBuffer(32 * n), S.DeviceBuffer(40 * n), S.DeviceBuffer(len(out))
            try:
                p.sc.lookup_lines(src.ptr + 3, len(data), o.ptr, len(out), [1], ks, index_ptr=a.ptr, index_cap=n)
                p.sc.route_lines_by_key(src.ptr + 3, len(data), o.ptr, len(out), [1], ks, index_ptr=b.ptr, index_cap=n)
                wa = list((ctypes.c_int64 * (4 * n)).from_buffer_copy(a.to_bytes(32 * n)))
                wb = list((ctypes.c_int64 * (5 * n)).from_buffer_copy(b.to_bytes(40 * n)))
                assert [wb[5 * r:5 * r + 4] for r in range(n)] == [wa[4 * r:4 * r + 4] for r in range(n)]
                assert {wb[5 * r + 4] for r in range(n)} == {0}
            finally:
                for x in (src, a, b, o):
                    x.free()
        finally:
            ks.close()


@pytest.mark.parametrize("groups", [[1], [1, 3]], ids=["K1", "K2"])
def test_round_trip_through_the_tally(gpu, groups):
    """the tally's rows as the dictionary: the buckets are the tally's keys in the tally's order, with the tally's counts"""
    data = kv_lines(21, 700, 80)
    K = len(groups)
    nlines = len(split_lines(data, 0x0A))
    with S.Pool() as pool:
        p = Program(pool, KV)
        src = upload_at(data, 3)
        rows, cnts, bkt = S.DeviceBuffer(1 << 16), S.DeviceBuffer(8 * 1000), S.DeviceBuffer(40 * 1000)
        try:
            t = p.sc.tally_lines(src.ptr + 3, len(data), rows.ptr, 1 << 16, groups, 1000, counts_ptr=cnts.ptr, counts_cap=1000)
            assert t.nwritten == t.nkeys > 50
            with S.KeySet(rows.ptr, t.out_bytes, K) as ks:
                assert ks.rows == ks.distinct == t.nkeys
                info = p.sc.route_lines_by_key(src.ptr + 3, len(data), None, 0, groups, ks, buckets_ptr=bkt.ptr, buckets_cap=1000)
                assert info.nkeyed == info.nmembers == info.nselected == t.nselected and info.nbuckets == t.nkeys
                counts = list((ctypes.c_uint64 * t.nkeys).from_buffer_copy(cnts.to_bytes(8 * t.nkeys)))
                b = list((ctypes.c_int64 * (5 * t.nkeys)).from_buffer_copy(bkt.to_bytes(40 * t.nkeys)))
                assert [b[5 * r] for r in range(t.nkeys)] == list(range(t.nkeys))
                assert [b[5 * r + 2] for r in range(t.nkeys)] == counts and sum(counts) == t.nselected
                # ... and checked in full against Python with the same dictionary
                text = rows.to_bytes(t.out_bytes)
                ids = {tuple(r.split(b"\t")): i for i, r in enumerate(text[:-1].split(b"\n"))}
                run_route_key(p.sc, p.exp, data, groups, ks, ids, True, src_off=1, dst_off=1)
        finally:
            for x in (src, rows, cnts, bkt):
                x.free()
    assert nlines == 700


def test_a_key_map_is_a_set_whose_values_are_ignored(gpu):
    data = kv_lines(31, 400, 25)
    rng = random.Random(31)
    with S.Pool() as pool:
        p = Program(pool, KV)
        keys = sorted({k for _, _, _, k in keys_of(p.exp, data, [1])})
        half = [k for k in keys if rng.random() < 0.6]
        km, mids = make_map([k + (b"V%d" % i, b"") for i, k in enumerate(half)], 3, 1)
        ks, ids = make_set([k for k in half], 1)
        try:
            assert mids == ids
            for all_lines in (False, True):
                assert run_route_key(p.sc, p.exp, data, [1], km, mids, all_lines, dst_off=7) == \
                    run_route_key(p.sc, p.exp, data, [1], ks, ids, all_lines, dst_off=7)
        finally:
            km.close()
            ks.close()


def test_the_nfa_tier_and_the_host_route(gpu, monkeypatch):
    data = dotted_lines(5, 300)
    with S.Pool() as pool:
        p = Program(pool, DOTTED, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        ks, ids = make_set(half_and_foreign(random.Random(2), keys_of(p.exp, data, [0, 1]), 2), 2)
        try:
            res = {}
            for all_lines in (False, True):
                res[all_lines] = run_route_key(p.sc, p.exp, data, [0, 1], ks, ids, all_lines, src_off=3, dst_off=5)
                assert p.sc.last_lines_device == 1 and 0 < res[all_lines][0].nmembers < res[all_lines][0].nkeyed
            monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
            for all_lines in (False, True):
                got = run_route_key(p.sc, p.exp, data, [0, 1], ks, ids, all_lines, src_off=3, dst_off=5)
                assert p.sc.last_lines_device == 0 and got == res[all_lines]
        finally:
            ks.close()


def test_forced_batch_cuts(gpu, monkeypatch):
    data = kv_lines(41, 257, 30)
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(half_and_foreign(random.Random(3), keys_of(p.exp, data, [1, 3]), 2), 2)
        try:
            one = [run_route_key(p.sc, p.exp, data, [1, 3], ks, ids, a, src_off=1, dst_off=2) for a in (False, True)]
            assert p.sc.last_line_batches == 1
            monkeypatch.setenv("SRE_HIP_LINES_BATCH", "100")
            two = [run_route_key(p.sc, p.exp, data, [1, 3], ks, ids, a, src_off=1, dst_off=2) for a in (False, True)]
            assert p.sc.last_line_batches == 3 and two == one
            # a bucket spans the batches: lines of one key in each of the three
            _, _, kid, buckets = one[1]
            assert any(len({i // 100 for i, v in enumerate(kid) if v == b[0]}) == 3 for b in buckets)
        finally:
            ks.close()


def test_other_calls_are_unchanged_by_a_route_by_key(gpu):
    """filter, route, lookup and join on the same scanner before and after: they share grow-only arrays"""
    data = kv_lines(51, 1300, 30)
    with S.Pool() as pool:
        p = Program(pool, KV)
        rng = random.Random(4)
        keys = sorted({k for _, _, _, k in keys_of(p.exp, data, [1])})
        half = [k for k in keys if rng.random() < 0.5]
        ks, ids = make_set(half, 1)
        km, mids = make_map([k + (b"V%d" % i,) for i, k in enumerate(half)], 2, 1)
        exp2, sc2, R = route_setup(pool, [rb"k=a", rb"k=[b-z]", rb"v=\d"])
        try:
            def others():
                return (run_filter(p.sc, p.exp, data, 0x0A, FIRST, src_off=2, dst_off=9),
                        run_lookup(p.sc, p.exp, data, [1], ks, ids, src_off=2, dst_off=9),
                        run_join(p.sc, p.exp, data, [1], km, mids, [0], src_off=2, dst_off=9),
                        run_route(sc2, exp2, data, R, [0, 1, 2, 3], 4, src_off=2, dst_off=9))
            before = others()
            for all_lines in (False, True):
                run_route_key(p.sc, p.exp, data, [1], ks, ids, all_lines, src_off=2, dst_off=9)
                run_route_key(sc2, exp2, data, [0], ks, ids, all_lines, src_off=2, dst_off=9, shape=False)
            assert others() == before
            run_route_key(p.sc, p.exp, data[:4000], [1], ks, ids, True)
            assert others() == before
        finally:
            ks.close()
            km.close()


# ------------------------------------------------------------------ 6. refusals

def test_refusals(gpu, capfd):
    data = b"k=a\nk=b\nk=a\n"
    src = upload_at(data, 0)
    out = Out(gpu, 256, 0)
    info = (ctypes.c_size_t * 8)()
    one, _ = make_set([(b"a",)], 1)
    two, _ = make_set([(b"a", b"")], 2)
    side = S.DeviceBuffer(512)

    def call(sc, groups=(1,), ks=one, flags=0, out_ptr=None, cap=256, keyid=(None, 0), index=(None, 0), buckets=(None, 0), delim=0x0A):
        arr = (ctypes.c_int * max(len(groups), 1))(*groups) if groups is not None else None
        return gpu.sre_hip_route_lines_by_key(sc.h, src.ptr, len(data), delim, arr, len(groups) if groups is not None else 1,
                                              ks.h if ks else None, flags, out.ptr if out_ptr is None else out_ptr, cap, keyid[0],
                                              keyid[1], index[0], index[1], buckets[0], buckets[1], info, None)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, KV))
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                capfd.readouterr()
                assert call(S.Scanner(pool, prog, mode)) == -1
                assert "line route by key" in capfd.readouterr().err        # by name
            sc = S.Scanner(pool, prog, FIRST)
            for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_ALL | S.HIP_LINES_INVERT, 4, 4 | S.HIP_LINES_ALL):
                assert call(sc, flags=flags) == -1
            assert call(sc, groups=(1, 3)) == -1 and call(sc, ks=two) == -1         # ngroups != the set's fields
            assert call(sc, ks=None) == -1 and call(sc, groups=(4,)) == -1 and call(sc, groups=(-1,)) == -1
            assert call(sc, groups=None) == -1 and call(sc, groups=()) == -1
            assert call(sc, keyid=(None, 3)) == -1 and call(sc, index=(None, 3)) == -1 and call(sc, buckets=(None, 3)) == -1
            assert call(sc, out_ptr=0, cap=4) == -1 and call(sc, delim=256) == -1 and call(sc, delim=-1) == -1
            assert call(sc, out_ptr=src.ptr + 2, cap=4) == -1                       # the output overlaps the buffer
            out.check(b"")
            assert call(sc, buckets=(side.ptr, 4)) == 0 and list(info) == [3, 3, 2, 2, 1, 8, 2, 8]
            out.check(b"k=a\nk=a\n")
            assert list((ctypes.c_int64 * 5).from_buffer_copy(side.to_bytes(40))) == [0, 0, 2, 0, 8]
            assert call(sc, groups=(1, 3), ks=two, flags=S.HIP_LINES_ALL) == 0 and list(info) == [3, 3, 2, 3, 2, 12, 3, 12]
            out.check(b"k=a\nk=a\nk=b\n")
    finally:
        src.free()
        out.free()
        side.free()
        one.close()
        two.close()
