"""The key set and the line lookup (sre_hip_keyset_create, sre_hip_lookup_lines): the lines whose captured key is in a set
of keys that lives on the device (with invert: the keyed lines whose key is not), written as the filter writes lines,
with the id of every line's key.

Expected values are pure Python: the split rule of line mode, the oracle's first-match record of every line (the extract
test's `expected`), and a dict {key tuple: lowest row}.  Output, key-id and index buffers have 64 guard bytes in front and
behind and are pre-filled with 0xA5 (the filter test's Out); every check asserts that the guards and everything beyond
what the call may write still hold 0xA5.
"""
import ctypes
import random

import pytest

import sregex_amd as S
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import Out, run_filter
from test_gpu_lines_extract import DOTTED, Program, expected
from test_gpu_lines_tally import KV, PAIR, kv_lines, run_tally, words, dotted_lines

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
SIZES = (1, 63, 64, 65, 257, 1024 + 17)


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def dict_bytes(rows, fsep=0x09, delim=0x0A, final_delim=True):
    """the rows as text; (an empty final row is a row only with its delimiter)"""
    texts = [bytes([fsep]).join(r) for r in rows]
    return bytes([delim]).join(texts) + (bytes([delim]) if rows and (final_delim or not texts[-1]) else b"")


def make_set(rows, K, fsep=0x09, delim=0x0A, off=0, final_delim=True):
    """a KeySet of the rows (tuples of K field texts); the caller's buffer is overwritten and freed before it is used"""
    text = dict_bytes(rows, fsep, delim, final_delim)
    buf = upload_at(text, off)
    try:
        ks = S.KeySet(buf.ptr + off, len(text), K, fsep, delim)
        if text:
            assert buf.lib.sre_hip_upload(buf.ptr + off, b"\xEE" * len(text), len(text)) == 0
    finally:
        buf.free()
    ids = {}
    for r, row in enumerate(rows):
        ids.setdefault(tuple(row), r)
    assert (ks.rows, ks.distinct, ks.fields) == (len(rows), len(ids), K)
    slots = ks.slots
    assert slots >= 1024 and slots >= 2 * len(rows) and slots & (slots - 1) == 0 and (slots == 1024 or slots < 4 * len(rows))
    assert ks.device_bytes >= 8 * slots + len(text)
    return ks, ids


def keys_of(exp, data, groups, delim=0x0A):
    """[(line, start, len, key tuple)] of the keyed lines"""
    return [(i, st, n, tuple(data[f[0]:f[0] + f[1]] if f else b"" for f in fields))
            for i, st, n, fields in expected(exp, data, delim, groups, False)]


def run_lookup(sc, exp, data, groups, ks, ids, invert=False, delim=0x0A, src_off=0, dst_off=0, out_cap=None, keyid_cap=None,
               index_cap=None, null_out=False):
    """one call, checked in full; returns (info, output bytes, key ids of all lines)"""
    lib = sc.lib
    d = bytes([delim])
    nlines = len(split_lines(data, delim))
    keyed = keys_of(exp, data, groups, delim)
    want_ids = [-2] * nlines
    for i, _, _, key in keyed:
        want_ids[i] = ids.get(key, -1)
    nmembers = sum(1 for v in want_ids if v >= 0)
    sel = [(i, st, n) for i, st, n, _ in keyed if (want_ids[i] >= 0) != invert]
    need = sum(n + 1 for _, _, n in sel)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for _, _, n in sel:
        if out_bytes + n + 1 > cap:
            break
        out_bytes += n + 1
        nwritten += 1
    want = b"".join(data[st:st + n] + d for _, st, n in sel[:nwritten])
    kcap = nlines + 3 if keyid_cap is None else keyid_cap
    icap = len(sel) + 3 if index_cap is None else index_cap
    src = upload_at(data, src_off)
    out, kid, idx = Out(lib, cap, dst_off), Out(lib, kcap * 8, 0), Out(lib, icap * 32, 0)
    try:
        info = sc.lookup_lines(src.ptr + src_off, len(data), None if null_out else out.ptr, cap, groups, ks, delim, invert,
                               kid.ptr if kcap else None, kcap, idx.ptr if icap else None, icap)
        assert info == S.LookupInfo(nlines, len(keyed), nmembers, len(sel), need, nwritten, out_bytes), \
            (info, len(keyed), nmembers, len(sel), need)
        out.check(want)
        got_ids = words(lib, kid, min(kcap, nlines))
        assert got_ids == want_ids[:kcap], [(i, g, w) for i, (g, w) in enumerate(zip(got_ids, want_ids)) if g != w][:3]
        nrows = min(icap, nwritten)
        rows, o = [], 0
        for i, st, n in sel[:nrows]:
            rows.append((i, st, n, o))
            o += n + 1
        raw = words(lib, idx, 4 * nrows)
        got = [tuple(raw[4 * r:4 * r + 4]) for r in range(nrows)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
    finally:
        for b in (src, out, kid, idx):
            b.free()
    return info, want, want_ids


def half_and_foreign(rng, keyed, K, nforeign=20):
    """set rows: a random half of the buffer's distinct keys, some twice, and keys the buffer does not hold"""
    distinct = sorted({key for _, _, _, key in keyed})
    rows = [k for k in distinct if rng.random() < 0.5]
    rows += [rng.choice(rows) for _ in range(len(rows) // 4)] if rows else []
    rows += [tuple(b"zz%d" % rng.randrange(1000) for _ in range(K)) for _ in range(nforeign)]
    rng.shuffle(rows)
    return rows


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
        rows = half_and_foreign(rng, keyed, len(groups))
        ks, ids = make_set(rows, len(groups), off=rng.randrange(1, 16), final_delim=n % 2 == 0)
        empty, none = make_set([], len(groups))
        try:
            for invert in (False, True):
                so, do = rng.randrange(1, 16), rng.randrange(1, 16)
                info, _, _ = run_lookup(p.sc, p.exp, data, groups, ks, ids, invert, src_off=so, dst_off=do)
                assert p.sc.last_lines_device == 1 and info.nkeyed == len(keyed)
                if n >= 63:
                    assert 0 < info.nmembers < info.nkeyed < info.nlines
                # an empty set makes no line a member; an empty buffer gives zeros
                info, _, _ = run_lookup(p.sc, p.exp, data, groups, empty, none, invert, src_off=so, dst_off=do)
                assert info.nmembers == 0 and info.nselected == (info.nkeyed if invert else 0)
                assert run_lookup(p.sc, p.exp, b"", groups, ks, ids, invert)[0] == S.LookupInfo(0, 0, 0, 0, 0, 0, 0)
        finally:
            ks.close()
            empty.close()


def test_fields_are_compared_one_by_one(gpu):
    """("ab", "c") is in the set, ("a", "bc") is not; an unset group equals an empty dictionary field"""
    lines = [b"<ab><c>", b"<a><bc>", b"<abc><>", b"<><abc>", b"<><>", b"nothing", b"<ab><c>"]
    with S.Pool() as pool:
        p = Program(pool, PAIR)
        ks, ids = make_set([(b"ab", b"c"), (b"", b"abc"), (b"", b"")], 2, fsep=ord("|"))
        q = Program(pool, KV)
        kv, kvids = make_set([(b"a", b""), (b"b", b"1")], 2)
        try:
            info, out, kid = run_lookup(p.sc, p.exp, b"\n".join(lines), [1, 2], ks, ids)
            assert kid == [0, -1, -1, 1, 2, -2, 0] and out == b"<ab><c>\n<><abc>\n<><>\n<ab><c>\n"
            info, out, kid = run_lookup(p.sc, p.exp, b"\n".join(lines), [1, 2], ks, ids, invert=True)
            assert out == b"<a><bc>\n<abc><>\n" and info.nkeyed == 6 and info.nmembers == 4
            # group 3 unset ("k=a") and empty ("k=a;v=") both equal the row whose second field is empty
            info, out, kid = run_lookup(q.sc, q.exp, b"k=a\nk=a;v=\nk=a;v=1\nk=b;v=1\n", [1, 3], kv, kvids)
            assert kid == [0, 0, -1, 1]
        finally:
            ks.close()
            kv.close()


# ------------------------------------------------------------------ 2. capacities

def test_truncation_and_side_arrays(gpu):
    data = kv_lines(6, 300, 40)
    rng = random.Random(6)
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(half_and_foreign(rng, keys_of(p.exp, data, [1, 3]), 2), 2)
        try:
            for invert in (False, True):
                info, out, _ = run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, invert)
                need, row = info.need_bytes, out.index(b"\n") + 1
                assert info.out_bytes == need > row and info.nselected > 3
                for cap in (need, need - 1, row, 0):
                    got, _, _ = run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, invert, out_cap=cap, dst_off=3)
                    assert (got.nkeyed, got.nmembers, got.need_bytes) == (info.nkeyed, info.nmembers, need)
                    assert got.nwritten == {need: info.nselected, need - 1: info.nselected - 1, row: 1, 0: 0}[cap]
                got, _, _ = run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, invert, out_cap=0, null_out=True)    # a sizing call
                assert got.need_bytes == need and got.nwritten == 0
                for kcap, icap in ((17, 3), (1, 1), (0, 0), (300, 0), (0, 2)):
                    run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, invert, keyid_cap=kcap, index_cap=icap)
        finally:
            ks.close()


# ------------------------------------------------------------------ 3. sets

def test_duplicate_rows_have_the_lowest_id(gpu):
    rows = [(b"b",), (b"a",), (b"b",), (b"c",), (b"a",), (b"",), (b"",), (b"c",)]
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(rows, 1, final_delim=False)
        try:
            assert ks.rows == 8 and ks.distinct == 4
            _, _, kid = run_lookup(p.sc, p.exp, b"k=c\nk=a\nk=\nk=b\nk=d\nnone\n", [1], ks, ids)
            assert kid == [3, 1, 5, 0, -1, -2]
        finally:
            ks.close()


def letters(i):
    return bytes(b"abcdefghij"[int(c)] for c in str(i))


def test_600_keys_take_a_larger_table(gpu):
    rows = [(letters(i),) for i in range(600)]
    data = b"\n".join(b"k=" + letters(i) for i in range(0, 900, 3))
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(rows, 1)
        try:
            assert ks.slots == 2048
            info, _, _ = run_lookup(p.sc, p.exp, data, [1], ks, ids)
            assert info.nmembers == 200 and info.nkeyed == 300
        finally:
            ks.close()


@pytest.mark.parametrize("bits", ["0", "2"])
def test_long_probe_chains(gpu, monkeypatch, bits):
    monkeypatch.setenv("SRE_HIP_KEYSET_HASH_BITS", bits)
    rows = [(letters(i), b"%d" % (i % 7)) for i in range(200)]
    data = b"\n".join(b"k=%s;v=%d" % (letters(i), i % 7) for i in range(0, 400, 2)) + b"\nk=zzz;v=\n"
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(rows, 2)
        monkeypatch.delenv("SRE_HIP_KEYSET_HASH_BITS")          # the lookup takes the mask from the set
        try:
            for invert in (False, True):
                info, _, _ = run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, invert)
                assert info.nmembers == 100 and info.nkeyed == 201
        finally:
            ks.close()


def test_a_chain_across_the_end_of_the_table(gpu):
    """keys whose home slot is one of the table's last two: their chain goes on at word 0"""
    tail, i = [], 0
    while len(tail) < 12:
        key = letters(i)
        if S.keyset_hash(key) & 1023 >= 1022:
            tail.append(key)
        i += 1
    rows = [(k,) for k in tail[:8]]
    data = b"\n".join(b"k=" + k for k in tail + tail[::-1])
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(rows, 1)
        try:
            assert ks.slots == 1024
            info, _, kid = run_lookup(p.sc, p.exp, data, [1], ks, ids)
            assert info.nmembers == 16 and info.nkeyed == 24 and kid[:12] == list(range(8)) + [-1] * 4
        finally:
            ks.close()


def test_a_bad_row_gives_no_set(gpu, capfd):
    text = b"a\tb\nc\td\ne\nf\tg\th\nx\ty\n"
    buf = upload_at(text, 5)
    try:
        with pytest.raises(ValueError):
            S.KeySet(buf.ptr + 5, len(text), 2)
        assert "row 2 " in capfd.readouterr().err            # the lowest of the two bad rows
        with pytest.raises(ValueError):
            S.KeySet(buf.ptr + 5, len(text), 3)
        assert "row 0 " in capfd.readouterr().err
        with S.KeySet(buf.ptr + 5, len(text), 1) as ks:         # K = 1: nothing is split
            assert ks.rows == 5 and ks.distinct == 5
    finally:
        buf.free()


# ------------------------------------------------------------------ 4. the tally's rows as the dictionary

@pytest.mark.parametrize("groups", [[1], [1, 3]], ids=["K1", "K2"])
def test_round_trip_through_the_tally(gpu, groups):
    data = kv_lines(21, 700, 80)
    K = len(groups)
    nlines = len(split_lines(data, 0x0A))
    with S.Pool() as pool:
        p = Program(pool, KV)
        src = upload_at(data, 3)
        rows, tid, lid = S.DeviceBuffer(1 << 16), S.DeviceBuffer(8 * nlines), S.DeviceBuffer(8 * nlines)
        try:
            t = p.sc.tally_lines(src.ptr + 3, len(data), rows.ptr, 1 << 16, groups, 1000, keyid_ptr=tid.ptr, keyid_cap=nlines)
            assert t.nwritten == t.nkeys > 50
            with S.KeySet(rows.ptr, t.out_bytes, K) as ks:
                assert ks.rows == ks.distinct == t.nkeys
                info = p.sc.lookup_lines(src.ptr + 3, len(data), None, 0, groups, ks, keyid_ptr=lid.ptr, keyid_cap=nlines)
                assert info.nkeyed == info.nmembers == info.nselected == t.nselected
                a = list((ctypes.c_int64 * nlines).from_buffer_copy(tid.to_bytes(8 * nlines)))
                b = list((ctypes.c_int64 * nlines).from_buffer_copy(lid.to_bytes(8 * nlines)))
                # (the tally says -1 for a line without a key, the lookup -2)
                assert [v if v >= 0 else -2 for v in a] == b and min(b) == -2 and max(b) == t.nkeys - 1
        finally:
            for x in (src, rows, tid, lid):
                x.free()


# ------------------------------------------------------------------ 5. scanners and routes

def test_one_set_two_scanners(gpu):
    data = kv_lines(31, 200, 25)
    with S.Pool() as pool:
        p, q = Program(pool, KV), Program(pool, [rb"k=([a-z]*)"])
        ks, ids = make_set(half_and_foreign(random.Random(1), keys_of(p.exp, data, [1]), 1), 1)
        try:
            _, one, k1 = run_lookup(p.sc, p.exp, data, [1], ks, ids)
            _, two, k2 = run_lookup(q.sc, q.exp, data, [1], ks, ids)
            _, again, _ = run_lookup(p.sc, p.exp, data, [1], ks, ids)
            assert one == two == again and k1 == k2 and len(one) > 100
        finally:
            ks.close()


def test_the_nfa_tier_and_the_host_route(gpu, monkeypatch):
    data = dotted_lines(5, 300)
    with S.Pool() as pool:
        p = Program(pool, DOTTED, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        ks, ids = make_set(half_and_foreign(random.Random(2), keys_of(p.exp, data, [0, 1]), 2), 2)
        try:
            res = {}
            for invert in (False, True):
                res[invert] = run_lookup(p.sc, p.exp, data, [0, 1], ks, ids, invert, src_off=3, dst_off=5)
                assert p.sc.last_lines_device == 1 and 0 < res[invert][0].nmembers < res[invert][0].nkeyed
            monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
            for invert in (False, True):
                got = run_lookup(p.sc, p.exp, data, [0, 1], ks, ids, invert, src_off=3, dst_off=5)
                assert p.sc.last_lines_device == 0 and got == res[invert]
        finally:
            ks.close()


def test_forced_batch_cuts(gpu, monkeypatch):
    data = kv_lines(41, 257, 30)
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(half_and_foreign(random.Random(3), keys_of(p.exp, data, [1, 3]), 2), 2)
        try:
            one = run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, src_off=1, dst_off=2)
            assert p.sc.last_line_batches == 1
            monkeypatch.setenv("SRE_HIP_LINES_BATCH", "100")
            for invert in (False, True):
                two = run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, invert, src_off=1, dst_off=2)
                assert p.sc.last_line_batches == 3
                assert invert or two == one
        finally:
            ks.close()


def test_filter_and_tally_are_unchanged_by_a_lookup(gpu):
    data = kv_lines(51, 400, 30)
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_set(half_and_foreign(random.Random(4), keys_of(p.exp, data, [1]), 1), 1)
        try:
            f0 = run_filter(p.sc, p.exp, data, 0x0A, FIRST, src_off=2, dst_off=9)
            t0 = run_tally(p.sc, p.exp, data, [1, 3], src_off=2, dst_off=9)
            run_lookup(p.sc, p.exp, data, [1], ks, ids, src_off=2, dst_off=9)
            assert run_filter(p.sc, p.exp, data, 0x0A, FIRST, src_off=2, dst_off=9) == f0
            run_lookup(p.sc, p.exp, data, [1], ks, ids, invert=True)
            assert run_tally(p.sc, p.exp, data, [1, 3], src_off=2, dst_off=9) == t0
            assert run_filter(p.sc, p.exp, data, 0x0A, FIRST, invert=True)[0].nselected > 0
        finally:
            ks.close()


# ------------------------------------------------------------------ 6. refusals

def test_refusals(gpu, capfd):
    data = b"k=a\nk=b\n"
    src = upload_at(data, 0)
    out = Out(gpu, 256, 0)
    info = (ctypes.c_size_t * 7)()
    one, _ = make_set([(b"a",)], 1)
    two, _ = make_set([(b"a", b"")], 2)

    def call(sc, groups=(1,), ks=one, flags=0, out_ptr=None, cap=256, keyid=(None, 0)):
        arr = (ctypes.c_int * len(groups))(*groups)
        return gpu.sre_hip_lookup_lines(sc.h, src.ptr, len(data), 0x0A, arr, len(groups), ks.h if ks else None, flags,
                                        out.ptr if out_ptr is None else out_ptr, cap, keyid[0], keyid[1], None, 0, info, None)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, KV))
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                capfd.readouterr()
                assert call(S.Scanner(pool, prog, mode)) == -1
                assert "line lookup" in capfd.readouterr().err          # by name
            sc = S.Scanner(pool, prog, FIRST)
            for flags in (S.HIP_LINES_ALL, S.HIP_LINES_ALL | S.HIP_LINES_INVERT, 4):
                assert call(sc, flags=flags) == -1
            assert call(sc, groups=(1, 3)) == -1 and call(sc, ks=two) == -1         # ngroups != the set's fields
            assert call(sc, ks=None) == -1 and call(sc, groups=(4,)) == -1
            assert call(sc, keyid=(None, 3)) == -1 and call(sc, out_ptr=src.ptr + 2, cap=4) == -1
            out.check(b"")
            assert call(sc) == 0 and list(info) == [2, 2, 1, 1, 4, 1, 4]
            out.check(b"k=a\n")
            assert call(sc, groups=(1, 3), ks=two, flags=S.HIP_LINES_INVERT) == 0 and list(info) == [2, 2, 1, 1, 4, 1, 4]
    finally:
        src.free()
        out.free()
        one.close()
        two.close()
