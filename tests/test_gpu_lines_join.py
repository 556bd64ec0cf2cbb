"""Key maps and the line join (sre_hip_keyset_create_map, sre_hip_join_lines): every line whose captured key is in a key map
that lives on the device, with the chosen value columns of the key's dictionary row behind it (with all_lines: every
line, empty values without a row), the id of every line's key, and index rows that say where each value landed.

Expected values are pure Python: the split rule of line mode, the oracle's first-match record of every line (the extract
test's `expected`), and a dict {key tuple: lowest row}.  Output, key-id and index buffers have 64 guard bytes in front and
behind and are pre-filled with 0xA5 (the filter test's Out); every check asserts that the guards and everything beyond
what the call may write still hold 0xA5.
"""
import collections
import ctypes
import random

import pytest

import sregex_amd as S
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import Out
from test_gpu_lines_extract import DOTTED, Program
from test_gpu_lines_tally import KV, kv_lines, words, dotted_lines
from test_gpu_lines_lookup import dict_bytes, keys_of, make_set, run_lookup

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
SIZES = (1, 63, 64, 65, 257, 1024 + 17)
TAB = 0x09


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def make_map(rows, nfields, nkeys, fsep=TAB, delim=0x0A, off=0, final_delim=True):
    """a key map of the rows (tuples of nfields field texts); the caller's buffer is overwritten and freed before the map
    is used.  Returns (map, {key: lowest row})"""
    text = dict_bytes(rows, fsep, delim, final_delim)
    buf = upload_at(text, off)
    try:
        ks = S.KeySet(buf.ptr + off, len(text), nfields, fsep, delim, nkeys=nkeys)
        if text:
            assert buf.lib.sre_hip_upload(buf.ptr + off, b"\xEE" * len(text), len(text)) == 0
    finally:
        buf.free()
    ids = {}
    for r, row in enumerate(rows):
        ids.setdefault(tuple(row[:nkeys]), r)
    assert (ks.rows, ks.distinct, ks.fields, ks.values) == (len(rows), len(ids), nkeys, nfields - nkeys)
    assert ks.device_bytes >= 8 * ks.slots + len(text) + 16 * nfields * len(rows)
    ks.py_rows = rows
    return ks, ids


def value_rows(rng, keys, nvalues, dups=True, nforeign=10):
    """map rows: every key with nvalues values of 0 .. 20 bytes (capitals and digits), a quarter of the keys a second
    time with other values further down, and keys the buffer does not hold"""
    def values():
        return tuple(bytes(rng.choice(b"ABCDEFG0123") for _ in range(rng.choice((0, 1, 2, 3, 5, 8, 15, 16, 17, 20))))
                     for _ in range(nvalues))
    rows = [tuple(k) + values() for k in keys]
    nk = len(keys[0]) if keys else 1
    rows += [tuple(b"zz%d" % rng.randrange(1000) for _ in range(nk)) + values() for _ in range(nforeign)]
    rng.shuffle(rows)
    if dups and keys:
        rows += [tuple(rng.choice(keys)) + values() for _ in range(max(len(keys) // 4, 1))]
    return rows


def half_of(rng, keyed):
    distinct = sorted({key for _, _, _, key in keyed})
    return [k for k in distinct if rng.random() < 0.5] or distinct[:1]


def run_join(sc, exp, data, groups, ks, ids, vcols, all_lines=False, jsep=TAB, delim=0x0A, src_off=0, dst_off=0, out_cap=None,
             keyid_cap=None, index_cap=None, null_out=False):
    """one call, checked in full; returns (info, output bytes, key ids of all lines)"""
    lib = sc.lib
    d, js, nk = bytes([delim]), bytes([jsep]), len(groups)
    lines = split_lines(data, delim)
    nlines = len(lines)
    want_ids = [-2] * nlines
    keyed = keys_of(exp, data, groups, delim)
    for i, _, _, key in keyed:
        want_ids[i] = ids.get(key, -1)
    nmembers = sum(1 for v in want_ids if v >= 0)
    sel = [(i, st, n) for i, (st, n) in enumerate(lines) if all_lines or want_ids[i] >= 0]
    texts, vals = [], []
    for i, st, n in sel:
        v = [ks.py_rows[want_ids[i]][nk + c] if want_ids[i] >= 0 else None for c in vcols]
        vals.append(v)
        texts.append(data[st:st + n] + b"".join(js + (x or b"") for x in v) + d)
    need = sum(len(t) for t in texts)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for t in texts:
        if out_bytes + len(t) > cap:
            break
        out_bytes += len(t)
        nwritten += 1
    want = b"".join(texts[:nwritten])
    width = 5 + 2 * len(vcols)
    kcap = nlines + 3 if keyid_cap is None else keyid_cap
    icap = len(sel) + 3 if index_cap is None else index_cap
    src = upload_at(data, src_off)
    out, kid, idx = Out(lib, cap, dst_off), Out(lib, kcap * 8, 0), Out(lib, icap * 8 * width, 0)
    try:
        info = sc.join_lines(src.ptr + src_off, len(data), None if null_out else out.ptr, cap, groups, ks, vcols, jsep, delim,
                             all_lines, kid.ptr if kcap else None, kcap, idx.ptr if icap else None, icap)
        assert info == S.LookupInfo(nlines, len(keyed), nmembers, len(sel), need, nwritten, out_bytes), \
            (info, len(keyed), nmembers, len(sel), need, nwritten, out_bytes)
        out.check(want)
        got_ids = words(lib, kid, min(kcap, nlines))
        assert got_ids == want_ids[:kcap], [(i, g, w) for i, (g, w) in enumerate(zip(got_ids, want_ids)) if g != w][:3]
        nrows = min(icap, nwritten)
        rows, o = [], 0
        for (i, st, n), v, t in zip(sel[:nrows], vals, texts):
            row, at = [i, st, n, o, want_ids[i]], o + n + 1
            for x in v:
                row += [-1, -1] if x is None else [at, len(x)]
                at += len(x or b"") + 1
            rows.append(tuple(row))
            o += len(t)
        raw = words(lib, idx, width * nrows)
        got = [tuple(raw[width * r:width * r + width]) for r in range(nrows)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
    finally:
        for b in (src, out, kid, idx):
            b.free()
    return info, want, want_ids


# ------------------------------------------------------------------ 1. the table-driven scanner

@pytest.mark.parametrize("nv", [1, 2, 31])
@pytest.mark.parametrize("n", SIZES)
def test_table_driven(gpu, n, nv):
    rng = random.Random(n * 3 + nv)
    data = kv_lines(n + nv, n, 30, longest=12)
    with S.Pool() as pool:
        p = Program(pool, KV)
        assert p.sc.engine == S.ENGINE_SCAN
        keyed = keys_of(p.exp, data, [1])
        if n == 1 and not keyed:
            data = b"x k=only;v=7 y"
            keyed = keys_of(p.exp, data, [1])
        ks, ids = make_map(value_rows(rng, half_of(rng, keyed), nv), 1 + nv, 1, off=(0, 5)[n % 2], final_delim=n % 2 == 0)
        empty, none = make_map([], 1 + nv, 1)
        vcols = list(range(nv))
        try:
            for all_lines in (False, True):
                so, do = rng.choice((0, 1, 15)), rng.choice((0, 1, 15))
                info, _, _ = run_join(p.sc, p.exp, data, [1], ks, ids, vcols, all_lines, src_off=so, dst_off=do)
                assert p.sc.last_lines_device == 1 and info.nkeyed == len(keyed)
                if n >= 63:
                    assert 0 < info.nmembers < info.nkeyed < info.nlines
                # an empty map: nothing, or every line with empty values; an empty buffer gives zeros
                info, _, _ = run_join(p.sc, p.exp, data, [1], empty, none, vcols, all_lines, src_off=so, dst_off=do)
                assert info.nmembers == 0 and info.nselected == (info.nlines if all_lines else 0)
                assert run_join(p.sc, p.exp, b"", [1], ks, ids, vcols, all_lines)[0] == S.LookupInfo(0, 0, 0, 0, 0, 0, 0)
        finally:
            ks.close()
            empty.close()


def test_columns_in_any_order_and_repeated(gpu):
    data = kv_lines(7, 200, 25)
    rng = random.Random(7)
    with S.Pool() as pool:
        p = Program(pool, KV)
        keyed = keys_of(p.exp, data, [1, 3])
        ks, ids = make_map(value_rows(rng, half_of(rng, keyed), 4), 6, 2, fsep=ord("|"), off=5)
        try:
            for vcols in ([3, 0], [2, 2, 2], [0, 1, 2, 3, 3, 2, 1, 0], [1] * 31, [3]):
                for all_lines in (False, True):
                    info, _, _ = run_join(p.sc, p.exp, data, [1, 3], ks, ids, vcols, all_lines, jsep=ord(","), src_off=1, dst_off=15)
                    assert 0 < info.nmembers < info.nkeyed
        finally:
            ks.close()


# ------------------------------------------------------------------ 2. collisions and missing rows

def test_the_lowest_row_of_a_key_gives_the_values(gpu):
    rows = [(b"b", b"B0"), (b"a", b"A1"), (b"b", b"B2"), (b"c", b""), (b"a", b"A4"), (b"", b"E5"), (b"", b"E6"), (b"c", b"C7")]
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_map(rows, 2, 1, final_delim=False)
        try:
            assert ks.rows == 8 and ks.distinct == 4
            _, out, kid = run_join(p.sc, p.exp, b"k=c\nk=a\nk=\nk=b\nk=d\nnone\n", [1], ks, ids, [0])
            assert kid == [3, 1, 5, 0, -1, -2] and out == b"k=c\t\nk=a\tA1\nk=\tE5\nk=b\tB0\n"
            _, out, _ = run_join(p.sc, p.exp, b"k=c\nk=a\nk=\nk=b\nk=d\nnone\n", [1], ks, ids, [0], True)
            assert out == b"k=c\t\nk=a\tA1\nk=\tE5\nk=b\tB0\nk=d\t\nnone\t\n"
        finally:
            ks.close()


def letters(i):
    return bytes(b"abcdefghij"[int(c)] for c in str(i))


@pytest.mark.parametrize("bits", ["0", "2"])
def test_long_probe_chains(gpu, monkeypatch, bits):
    monkeypatch.setenv("SRE_HIP_KEYSET_HASH_BITS", bits)
    rows = [(letters(i), b"%d" % (i % 7), b"V%d" % i, b"W" * (i % 18)) for i in range(200)]
    data = b"\n".join(b"k=%s;v=%d" % (letters(i), i % 7) for i in range(0, 400, 2)) + b"\nk=zzz;v=\n"
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_map(rows, 4, 2)
        monkeypatch.delenv("SRE_HIP_KEYSET_HASH_BITS")          # the join takes the mask from the map
        try:
            for all_lines in (False, True):
                info, _, _ = run_join(p.sc, p.exp, data, [1, 3], ks, ids, [1, 0], all_lines)
                assert info.nmembers == 100 and info.nkeyed == 201
        finally:
            ks.close()


def test_lines_without_a_dictionary_row_under_all(gpu):
    data = b"k=a\nnothing\nk=q\n\nk=b;v=1\nk=a"
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_map([(b"a", b"AA", b""), (b"b", b"", b"BBB")], 3, 1)
        try:
            lib = p.sc.lib
            src, out, idx = upload_at(data, 0), Out(lib, 256, 0), Out(lib, 9 * 8 * 8, 0)
            try:
                info = p.sc.join_lines(src.ptr, len(data), out.ptr, 256, [1], ks, [0, 1], all_lines=True, index_ptr=idx.ptr,
                                       index_cap=8)
                want = b"k=a\tAA\t\nnothing\t\t\nk=q\t\t\n\t\t\nk=b;v=1\t\tBBB\nk=a\tAA\t\n"
                assert info == S.LookupInfo(6, 4, 3, 6, len(want), 6, len(want))
                out.check(want)
                raw = words(lib, idx, 9 * 6)
                rows = [tuple(raw[9 * r:9 * r + 9]) for r in range(6)]
                assert [r[4] for r in rows] == [0, -2, -1, -2, 1, 0]
                assert [r[5:] for r in rows] == [(4, 2, 7, 0), (-1,) * 4, (-1,) * 4, (-1,) * 4, (35, 0, 36, 3), (44, 2, 47, 0)]
                assert [r[:4] for r in rows] == [(0, 0, 3, 0), (1, 4, 7, 8), (2, 12, 3, 18), (3, 16, 0, 24), (4, 17, 7, 27), (5, 25, 3, 40)]
            finally:
                for b in (src, out, idx):
                    b.free()
            run_join(p.sc, p.exp, data, [1], ks, ids, [0, 1], True)
        finally:
            ks.close()


# ------------------------------------------------------------------ 3. alignments and capacities

@pytest.mark.parametrize("dict_off", [0, 5])
def test_alignments(gpu, dict_off):
    data = kv_lines(11, 120, 20)
    rng = random.Random(11)
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_map(value_rows(rng, half_of(rng, keys_of(p.exp, data, [1])), 2), 3, 1, off=dict_off, final_delim=False)
        try:
            outs = set()
            for so in (0, 1, 15):
                for do in (0, 1, 15):
                    outs.add(run_join(p.sc, p.exp, data, [1], ks, ids, [1, 0], so == 1, src_off=so, dst_off=do)[1])
            assert len(outs) == 2
        finally:
            ks.close()


def test_truncation_and_side_arrays(gpu):
    data = b"k=a\nzzz\nk=bb;v=1\nk=a;v=22\nk=\nk=nope\nk=ccc\n"
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_map([(b"a", b"1", b"ONE"), (b"bb", b"22", b""), (b"", b"", b"EMPTY"), (b"ccc", b"333", b"C")], 3, 1)
        try:
            info, out, kid = run_join(p.sc, p.exp, data, [1], ks, ids, [0, 1])
            assert info.nselected == 5 and kid == [0, -2, 1, 0, 2, -1, 3]
            need, edges, at = info.need_bytes, [], 0
            for row in out.split(b"\n")[:-1]:
                at += len(row) + 1
                edges.append(at)
            assert edges[-1] == need and len(edges) == 5
            for r, edge in enumerate(edges):
                for cap, nw in ((edge - 1, r), (edge, r + 1), (edge + 1, r + 1)):
                    got, _, _ = run_join(p.sc, p.exp, data, [1], ks, ids, [0, 1], out_cap=cap, dst_off=3)
                    assert (got.nwritten, got.need_bytes, got.nkeyed, got.nmembers) == (nw, need, 6, 5)
            assert run_join(p.sc, p.exp, data, [1], ks, ids, [0, 1], out_cap=0)[0].nwritten == 0
            # the sizing call still delivers every key id
            got, _, _ = run_join(p.sc, p.exp, data, [1], ks, ids, [0, 1], out_cap=0, null_out=True)
            assert got.need_bytes == need and got.nwritten == 0 and got.out_bytes == 0
            for all_lines in (False, True):
                for kcap in (0, 1, 7 + 3):
                    for icap in (0, 1, 7 + 3):
                        run_join(p.sc, p.exp, data, [1], ks, ids, [1], all_lines, keyid_cap=kcap, index_cap=icap)
        finally:
            ks.close()


def test_short_rows_take_the_global_table_of_the_gather(gpu):
    """6000 empty lines under all_lines with two columns and no member: every row is 3 bytes, so a 16 KiB tile of the output
    spans more entries than the gather's window holds"""
    data = b"\n" * 6000
    with S.Pool() as pool:
        p = Program(pool, KV)
        ks, ids = make_map([(b"a", b"x", b"y")], 3, 1)
        try:
            info, out, _ = run_join(p.sc, p.exp, data, [1], ks, ids, [0, 1], True, src_off=1, dst_off=15, index_cap=5)
            assert info == S.LookupInfo(6000, 0, 0, 6000, 18000, 6000, 18000) and out == b"\t\t\n" * 6000
            assert run_join(p.sc, p.exp, data, [1], ks, ids, [0, 1], False)[0].nselected == 0
        finally:
            ks.close()


# ------------------------------------------------------------------ 4. batches and routes

def test_forced_batch_cuts(gpu, monkeypatch):
    data = kv_lines(41, 257, 30)
    with S.Pool() as pool:
        p = Program(pool, KV)
        rng = random.Random(3)
        ks, ids = make_map(value_rows(rng, half_of(rng, keys_of(p.exp, data, [1, 3])), 2), 4, 2)
        try:
            one = {a: run_join(p.sc, p.exp, data, [1, 3], ks, ids, [0, 1], a, src_off=1, dst_off=2) for a in (False, True)}
            assert p.sc.last_line_batches == 1
            monkeypatch.setenv("SRE_HIP_LINES_BATCH", "100")
            for a in (False, True):
                two = run_join(p.sc, p.exp, data, [1, 3], ks, ids, [0, 1], a, src_off=1, dst_off=2)
                assert p.sc.last_line_batches == 3 and two == one[a]
        finally:
            ks.close()


def test_the_nfa_tier_and_the_host_route(gpu, monkeypatch):
    data = dotted_lines(5, 300)
    with S.Pool() as pool:
        p = Program(pool, DOTTED, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        rng = random.Random(2)
        ks, ids = make_map(value_rows(rng, half_of(rng, keys_of(p.exp, data, [0, 1])), 2), 4, 2, off=5)
        try:
            res = {}
            for a in (False, True):
                res[a] = run_join(p.sc, p.exp, data, [0, 1], ks, ids, [1, 0], a, src_off=3, dst_off=5)
                assert p.sc.last_lines_device == 1 and 0 < res[a][0].nmembers < res[a][0].nkeyed
            monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
            for a in (False, True):
                got = run_join(p.sc, p.exp, data, [0, 1], ks, ids, [1, 0], a, src_off=3, dst_off=5)
                assert p.sc.last_lines_device == 0 and got == res[a]
        finally:
            ks.close()


# ------------------------------------------------------------------ 5. closure

def test_a_lookup_on_a_map_is_the_lookup_on_its_keys(gpu):
    data = kv_lines(51, 400, 30)
    rng = random.Random(4)
    with S.Pool() as pool:
        p = Program(pool, KV)
        rows = value_rows(rng, half_of(rng, keys_of(p.exp, data, [1, 3])), 3)
        ks, ids = make_map(rows, 5, 2, off=5)
        plain, pids = make_set([r[:2] for r in rows], 2)
        try:
            assert ids == pids and (ks.slots, ks.distinct, ks.rows, ks.fields) == (plain.slots, plain.distinct, plain.rows, plain.fields)
            assert plain.values == 0 and ks.device_bytes > plain.device_bytes
            for invert in (False, True):
                a = run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, invert, src_off=2, dst_off=9)
                b = run_lookup(p.sc, p.exp, data, [1, 3], plain, pids, invert, src_off=2, dst_off=9)
                assert a == b and a[0].nselected > 0
            # and a join in between changes neither
            run_join(p.sc, p.exp, data, [1, 3], ks, ids, [2, 0], True)
            assert run_lookup(p.sc, p.exp, data, [1, 3], ks, ids, False, src_off=2, dst_off=9) == \
                run_lookup(p.sc, p.exp, data, [1, 3], plain, pids, False, src_off=2, dst_off=9)
        finally:
            ks.close()
            plain.close()


def test_the_joined_column_feeds_a_tally(gpu):
    """the output is a line buffer again: a second scanner tallies the appended column with no host round trip"""
    data = kv_lines(61, 500, 40)
    rng = random.Random(6)
    with S.Pool() as pool:
        p, q = Program(pool, KV), Program(pool, [rb"\t([A-Z]*)"], key=False)
        keys = half_of(rng, keys_of(p.exp, data, [1]))
        classes = [b"ALPHA", b"BETA", b"", b"GAMMA"]
        rows = [k + (classes[j % 4], b"%d" % j) for j, k in enumerate(keys)]
        ks, ids = make_map(rows, 3, 1)
        lib = p.sc.lib
        src, out = upload_at(data, 3), S.DeviceBuffer(1 << 16)
        trows, counts = S.DeviceBuffer(4096), S.DeviceBuffer(8 * 16)
        try:
            for all_lines in (False, True):
                info = p.sc.join_lines(src.ptr + 3, len(data), out.ptr, 1 << 16, [1], ks, [0, 1], all_lines=all_lines)
                assert info.nwritten == info.nselected > 50
                key_of = {i: key for i, _, _, key in keys_of(p.exp, data, [1])}
                want = collections.Counter()
                for i in range(info.nlines):
                    r = ids.get(key_of.get(i), -1)
                    if all_lines or r >= 0:
                        want[rows[r][1] if r >= 0 else b""] += 1
                t = q.sc.tally_lines(out.ptr, info.out_bytes, trows.ptr, 4096, [1], 16, counts_ptr=counts.ptr, counts_cap=16)
                assert t.nselected == info.nwritten and t.nkeys == len(want)
                names = trows.to_bytes(t.out_bytes).split(b"\n")[:-1]
                got = dict(zip(names, (ctypes.c_uint64 * t.nkeys).from_buffer_copy(counts.to_bytes(8 * t.nkeys))))
                assert got == dict(want) and set(got) <= set(classes)
        finally:
            for x in (src, out, trows, counts):
                x.free()
            ks.close()


# ------------------------------------------------------------------ 6. refusals

def test_refusals(gpu, capfd):
    data = b"k=a\nk=b\n"
    src = upload_at(data, 0)
    out = Out(gpu, 256, 0)
    info = (ctypes.c_size_t * 7)()
    one, _ = make_map([(b"a", b"1", b"2")], 3, 1)
    two, _ = make_map([(b"a", b"", b"1")], 3, 2)
    semi, _ = make_map([(b"a", b"1")], 2, 1, delim=ord(";"))
    plain, _ = make_set([(b"a",)], 1)

    def call(sc, groups=(1,), ks=one, vcols=(0,), nvcols=None, jsep=TAB, flags=0, delim=0x0A, out_ptr=None, cap=256, keyid=(None, 0)):
        arr = (ctypes.c_int * len(groups))(*groups)
        cols = (ctypes.c_int * max(len(vcols), 1))(*vcols) if vcols is not None else None
        return gpu.sre_hip_join_lines(sc.h, src.ptr, len(data), delim, arr, len(groups), ks.h if ks else None, cols,
                                      len(vcols) if nvcols is None else nvcols, jsep, flags, out.ptr if out_ptr is None else out_ptr,
                                      cap, keyid[0], keyid[1], None, 0, info, None)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, KV))
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                capfd.readouterr()
                assert call(S.Scanner(pool, prog, mode)) == -1
                assert "line join" in capfd.readouterr().err            # by name
            sc = S.Scanner(pool, prog, FIRST)
            assert call(sc, ks=None) == -1 and call(sc, ks=plain) == -1             # no set, no value columns
            assert call(sc, vcols=(), nvcols=0) == -1 and call(sc, vcols=(0,) * 32) == -1 and call(sc, vcols=None, nvcols=1) == -1
            assert call(sc, vcols=(2,)) == -1 and call(sc, vcols=(0, -1)) == -1 and call(sc, ks=two, groups=(1, 3), vcols=(1,)) == -1
            assert call(sc, jsep=-1) == -1 and call(sc, jsep=256) == -1 and call(sc, jsep=0x0A) == -1
            assert call(sc, ks=semi) == -1 and call(sc, delim=ord(";")) == -1       # not the map's delimiter
            for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_ALL | S.HIP_LINES_INVERT, 4):
                assert call(sc, flags=flags) == -1
            assert call(sc, groups=(1, 3)) == -1 and call(sc, ks=two) == -1         # ngroups != the map's key fields
            assert call(sc, groups=(4,)) == -1
            assert call(sc, keyid=(None, 3)) == -1 and call(sc, out_ptr=src.ptr + 2, cap=4) == -1
            out.check(b"")
            assert call(sc, vcols=(1, 0)) == 0 and list(info) == [2, 2, 1, 1, 8, 1, 8]
            out.check(b"k=a\t2\t1\n")
            assert call(sc, ks=semi, delim=ord(";")) == 0 and list(info) == [1, 1, 1, 1, 11, 1, 11]
            assert call(sc, ks=two, groups=(1, 3), vcols=(0,), flags=S.HIP_LINES_ALL) == 0 and list(info) == [2, 2, 1, 2, 11, 2, 11]
    finally:
        src.free()
        out.free()
        for ks in (one, two, semi, plain):
            ks.close()
