"""The line tally (sre_hip_tally_lines): one row per distinct tuple of capture-group texts, in the order of the first
line that carries each, with the number of lines per key and the key number of every line.

Expected values are pure Python: the split rule of line mode, the oracle's first-match record of every line (the
extract test's `expected`), and a dict in first-occurrence order.  Output, counts, key-id and index buffers have 64 guard
bytes in front and behind and are pre-filled with 0xA5 (the filter test's Out); every check asserts that the guards and
everything beyond what the call may write still hold 0xA5.  Every successful call is also checked for
sum(counts) == nselected and keyid[first line of key k] == k.
"""
import ctypes
import random

import pytest

import sregex_amd as S
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import Out, download
from test_gpu_lines_extract import DOTTED, Program, expected, row_text, run_extract

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
KV = [rb"k=([a-z]*)(;v=([0-9]*))?"]         # group 1 may be empty, group 3 empty (";v=") or unset (no ";v=")
PAIR = [rb"<([a-z|]*)><([a-z|]*)>"]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def tally(data, sel):
    """({key: [first entry of sel, count]} in first-occurrence order, key number per line of the buffer or -1)"""
    keys, ids = {}, {}
    for s in sel:
        key = tuple(data[f[0]:f[0] + f[1]] if f else b"" for f in s[3])
        k = keys.setdefault(key, [s, 0, len(keys)])
        k[1] += 1
        ids[s[0]] = k[2]
    return keys, ids


def words(lib, out, n, ctype=ctypes.c_int64):
    """the first n 8-byte words of an Out, after asserting that nothing else of it was touched"""
    raw = download(lib, out.ptr, 8 * n)
    out.check(raw)
    return list((ctype * n).from_buffer_copy(raw)) if n else []


def run_tally(sc, exp, data, groups, max_keys=None, delim=0x0A, fsep=0x09, all_lines=False, src_off=0, dst_off=0, out_cap=None,
              counts_cap=None, keyid_cap=None, index_cap=None, null_out=False, overflow=False):
    """one call, checked in full; returns (info, output bytes, counts)"""
    lib = sc.lib
    K = len(groups)
    nlines = len(split_lines(data, delim))
    sel = expected(exp, data, delim, groups, all_lines)
    keys, ids = tally(data, sel)
    firsts = [v[0] for v in keys.values()]
    texts = [row_text(data, s[3], fsep, delim) for s in firsts]
    need = sum(len(t) for t in texts)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for t in texts:
        if out_bytes + len(t) > cap:
            break
        out_bytes += len(t)
        nwritten += 1
    want = b"".join(texts[:nwritten])
    mk = max(len(keys), 1) if max_keys is None else max_keys
    ccap = len(keys) + 3 if counts_cap is None else counts_cap
    kcap = nlines + 3 if keyid_cap is None else keyid_cap
    icap = len(keys) + 3 if index_cap is None else index_cap
    width = 4 + 2 * K
    src = upload_at(data, src_off)
    out, cnt, kid, idx = Out(lib, cap, dst_off), Out(lib, ccap * 8, 0), Out(lib, kcap * 8, 0), Out(lib, icap * width * 8, 0)
    flags = S.HIP_LINES_ALL if all_lines else 0
    try:
        args = (src.ptr + src_off, len(data), None if null_out else out.ptr, cap, groups, mk, delim, fsep, flags,
                cnt.ptr if ccap else None, ccap, kid.ptr if kcap else None, kcap, idx.ptr if icap else None, icap)
        if overflow:
            with pytest.raises(S.TallyOverflow) as e:
                sc.tally_lines(*args)
            assert e.value.info == S.TallyInfo(nlines, len(sel), 0, 0, 0, 0), e.value.info
            for o in (out, cnt, kid, idx):
                o.check(b"")            # 0xA5 throughout
            return e.value.info, b"", []
        info = sc.tally_lines(*args)
        assert info == S.TallyInfo(nlines, len(sel), len(keys), need, nwritten, out_bytes), (info, len(sel), len(keys), need)
        out.check(want)
        # counts and key ids are complete whatever out_cap is
        want_counts = [v[1] for v in keys.values()]
        got_counts = words(lib, cnt, min(ccap, len(keys)), ctypes.c_uint64)
        assert got_counts == want_counts[:ccap], [(k, g, w) for k, (g, w) in enumerate(zip(got_counts, want_counts)) if g != w][:3]
        want_ids = [ids.get(i, -1) for i in range(nlines)]
        got_ids = words(lib, kid, min(kcap, nlines))
        assert got_ids == want_ids[:kcap], [(i, g, w) for i, (g, w) in enumerate(zip(got_ids, want_ids)) if g != w][:3]
        if ccap >= len(keys):
            assert sum(got_counts) == info.nselected
        for k, s in enumerate(firsts):
            if s[0] < len(got_ids):
                assert got_ids[s[0]] == k
        # the extract's index rows of the keys' first lines
        nrows = min(icap, nwritten)
        rows, o = [], 0
        for (i, st, n, fields), t in zip(firsts[:nrows], texts):
            row = [i, st, n, o]
            for f in fields:
                row += list(f) if f else [-1, -1]
            rows.append(tuple(row))
            o += len(t)
        raw = words(lib, idx, width * nrows)
        got = [tuple(raw[width * r:width * (r + 1)]) for r in range(nrows)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
    finally:
        for b in (src, out, cnt, kid, idx):
            b.free()
    return info, want, want_counts


def kv_lines(seed, nlines, nkeys, longest=40, miss=0.15):
    """lines around k=KEY or k=KEY;v=DIGITS; KEY 0 .. longest letters, DIGITS may be empty; some lines have no match"""
    rng = random.Random(seed)
    pool = []
    for j in range(nkeys):
        key = bytes(rng.choice(b"abcxyz") for _ in range(j % (longest + 1)))
        tail = rng.choice([b"", b";v=", b";v=%d" % rng.randrange(30)])
        pool.append(b"k=" + key + tail)
    pads = [b"", b" ", b"-- ", b"at 12 "]
    out = []
    for i in range(nlines):
        out.append(b"no key here" if rng.random() < miss else pads[i % 4] + rng.choice(pool) + pads[(i // 4) % 4])
    return b"\n".join(out) + (b"\n" if nlines % 2 else b"")


# ------------------------------------------------------------------ 1. the table-driven scanner

@pytest.mark.parametrize("groups", [[1], [1, 3]], ids=["K1", "K2"])
@pytest.mark.parametrize("all_lines", [False, True])
def test_table_driven(gpu, groups, all_lines):
    data = kv_lines(3, 400, 90)
    with S.Pool() as pool:
        p = Program(pool, KV)
        assert p.sc.engine == S.ENGINE_SCAN
        info, _, counts = run_tally(p.sc, p.exp, data, groups, all_lines=all_lines)
        assert p.sc.last_lines_device == 1
        assert info.nlines == 400 and 40 < info.nkeys < info.nselected and max(counts) > 1
        assert (info.nselected == 400) == all_lines
        # an empty buffer, and one without any key
        assert run_tally(p.sc, p.exp, b"", groups, all_lines=all_lines)[0] == S.TallyInfo(0, 0, 0, 0, 0, 0)
        info, _, _ = run_tally(p.sc, p.exp, b"nothing\nat all\n", groups, all_lines=all_lines)
        assert info.nkeys == (1 if all_lines else 0)


def test_fields_are_compared_one_by_one(gpu):
    """("ab", "c") and ("a", "bc") are two keys, and so are ("a|b", "c") and ("a", "b|c") whose rows are the same text"""
    lines = [b"<ab><c>", b"<a><bc>", b"<a|b><c>", b"<a><b|c>", b"<ab><c>", b"<a><b|c>", b"<abc><>", b"<><abc>", b"<a><bc>"]
    with S.Pool() as pool:
        p = Program(pool, PAIR)
        info, out, counts = run_tally(p.sc, p.exp, b"\n".join(lines), [1, 2], fsep=ord("|"))
        assert info.nkeys == 6 and counts == [2, 2, 1, 2, 1, 1]
        assert out == b"ab|c\na|bc\na|b|c\na|b|c\nabc|\n|abc\n"


# ------------------------------------------------------------------ 2. contention and size

def test_one_key_in_many_workgroups(gpu):
    data = b"\n".join(b"%sk=same;v=1 %d" % (b" " * (i % 3), i % 50) for i in range(5000))
    with S.Pool() as pool:
        p = Program(pool, KV)
        info, out, counts = run_tally(p.sc, p.exp, data, [1, 3])
        assert info.nkeys == 1 and counts == [5000] and out == b"same\t1\n"


def test_every_line_its_own_key(gpu):
    rng = random.Random(8)
    order = list(range(5000))
    rng.shuffle(order)
    data = b"\n".join(b"k=" + bytes(b"abcdefghij"[int(c)] for c in str(i)) for i in order)
    with S.Pool() as pool:
        p = Program(pool, KV)
        info, _, counts = run_tally(p.sc, p.exp, data, [1])
        assert info.nkeys == 5000 and counts == [1] * 5000


def test_a_key_of_40_kib(gpu):
    big = bytes(b"abcdefg"[i % 7] for i in range(40 * 1024))
    lines = [b"k=tiny", b"k=" + big, b"k=" + big[:-1] + b"z", b"x k=" + big + b" tail", b"k=tiny", b"k=" + big[:-1]]
    with S.Pool() as pool:
        p = Program(pool, KV)
        info, _, counts = run_tally(p.sc, p.exp, b"\n".join(lines), [1])
        assert info.nkeys == 4 and counts == [2, 2, 1, 1]


def test_keys_recur_across_batches(gpu, monkeypatch):
    data = kv_lines(11, 100, 12)
    with S.Pool() as pool:
        p = Program(pool, KV)
        _, one, c1 = run_tally(p.sc, p.exp, data, [1, 3], src_off=1, dst_off=2)
        assert p.sc.last_line_batches == 1
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "7")
        _, two, c2 = run_tally(p.sc, p.exp, data, [1, 3], src_off=1, dst_off=2)
        assert p.sc.last_line_batches == 15 and one == two and c1 == c2


@pytest.mark.parametrize("bits", ["2", "0"])
def test_long_probe_chains(gpu, monkeypatch, bits):
    monkeypatch.setenv("SRE_HIP_TALLY_HASH_BITS", bits)
    data = kv_lines(int(bits) + 20, 1500, 360, miss=0.05)
    with S.Pool() as pool:
        p = Program(pool, KV)
        info, _, _ = run_tally(p.sc, p.exp, data, [1, 3])
        assert info.nkeys >= 300


# ------------------------------------------------------------------ 3. max_keys

def test_max_keys_and_overflow(gpu):
    data = kv_lines(4, 700, 60)
    with S.Pool() as pool:
        p = Program(pool, KV)
        info, _, _ = run_tally(p.sc, p.exp, data, [1, 3])
        nkeys = info.nkeys
        assert nkeys > 40
        run_tally(p.sc, p.exp, data, [1, 3], max_keys=nkeys)                        # exactly full: fine
        run_tally(p.sc, p.exp, data, [1, 3], max_keys=nkeys - 1, overflow=True)
        run_tally(p.sc, p.exp, data, [1, 3], max_keys=1, overflow=True)
        run_tally(p.sc, p.exp, data, [1, 3], max_keys=100000)                       # a larger table, then the small one again
        run_tally(p.sc, p.exp, data, [1, 3], max_keys=nkeys)


def test_bad_arguments(gpu):
    data = b"k=a\nk=b\n"
    src = upload_at(data, 0)
    out = Out(gpu, 256, 0)
    info = S.TallyInfoStruct()

    def call(sc, groups=(1,), flags=0, max_keys=16, fsep=0x09, out_ptr=None, cap=256, counts=(None, 0), keyid=(None, 0)):
        arr = (ctypes.c_int * len(groups))(*groups)
        return gpu.sre_hip_tally_lines(sc.h, src.ptr, len(data), 0x0A, arr, len(groups), fsep, flags, max_keys,
                                       out.ptr if out_ptr is None else out_ptr, cap, counts[0], counts[1], keyid[0], keyid[1],
                                       None, 0, ctypes.byref(info), None)
    try:
        with S.Pool() as pool:
            re = S.parse(pool, KV)
            prog = S.compile(pool, re)
            # Thompson and COUNT scanners have no first-match captures
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                assert call(S.Scanner(pool, prog, mode)) == -1
            sc = S.Scanner(pool, prog, FIRST)
            for mk in (0, S.HIP_TALLY_MAX_KEYS + 1):
                assert call(sc, max_keys=mk) == -1
            for flags in (S.HIP_LINES_INVERT, 4, 4 | S.HIP_LINES_ALL):
                assert call(sc, flags=flags) == -1
            assert call(sc, groups=(4,)) == -1 and call(sc, fsep=256) == -1
            assert call(sc, counts=(None, 3)) == -1 and call(sc, keyid=(None, 3)) == -1
            assert call(sc, out_ptr=src.ptr + 2, cap=4) == -1
            out.check(b"")
            assert call(sc) == 0 and info.nkeys == 2 and info.nselected == 2
            out.check(b"a\nb\n")
    finally:
        src.free()
        out.free()


# ------------------------------------------------------------------ 4. capacities and alignment

def test_out_cap(gpu):
    data = kv_lines(6, 300, 40)
    with S.Pool() as pool:
        p = Program(pool, KV)
        info, out, _ = run_tally(p.sc, p.exp, data, [1, 3])
        need, row = info.need_bytes, out.index(b"\n") + 1
        assert info.out_bytes == need > row
        for cap in (need, need - 1, row, 0):
            got, _, _ = run_tally(p.sc, p.exp, data, [1, 3], out_cap=cap, dst_off=3)
            assert got.nkeys == info.nkeys and got.need_bytes == need
            assert got.nwritten == {need: info.nkeys, need - 1: info.nkeys - 1, row: 1, 0: 0}[cap]
        got, _, _ = run_tally(p.sc, p.exp, data, [1, 3], out_cap=0, null_out=True)          # a sizing call
        assert got.need_bytes == need and got.nwritten == 0


def test_small_and_absent_side_arrays(gpu):
    data = kv_lines(7, 300, 40)
    with S.Pool() as pool:
        p = Program(pool, KV)
        for ccap, kcap, icap in ((5, 17, 3), (1, 1, 1), (0, 0, 0), (0, 300, 0), (40, 0, 2)):
            run_tally(p.sc, p.exp, data, [1, 3], counts_cap=ccap, keyid_cap=kcap, index_cap=icap)


@pytest.mark.parametrize("src_off,dst_off", [(1, 15), (7, 7), (15, 1), (13, 0)])
def test_odd_alignments(gpu, src_off, dst_off):
    data = kv_lines(src_off, 260, 50)
    with S.Pool() as pool:
        p = Program(pool, KV)
        run_tally(p.sc, p.exp, data, [1, 3], src_off=src_off, dst_off=dst_off)


# ------------------------------------------------------------------ 5. the other routes

def dotted_lines(seed, nlines=600):
    rng = random.Random(seed)
    addrs = [b"%d.%d.%d.%d" % tuple(rng.randrange(256) for _ in range(4)) for _ in range(37)]
    return b"\n".join(rng.choice([b"GET / from ", b"", b"x "]) + rng.choice(addrs + [b"1.2.3", b"none"]) + b" ok" for _ in range(nlines))


def test_first_match_on_the_nfa_tier(gpu):
    data = dotted_lines(2)
    with S.Pool() as pool:
        p = Program(pool, DOTTED, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        info, _, _ = run_tally(p.sc, p.exp, data, [0], src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 1 and info.nkeys == 37 and info.nselected < info.nlines


def test_the_host_route(gpu, monkeypatch):
    data = dotted_lines(3)
    with S.Pool() as pool:
        p = Program(pool, DOTTED, S.ENGINE_NFA)
        _, one, c1 = run_tally(p.sc, p.exp, data, [0, 1], src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 1
        monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
        _, two, c2 = run_tally(p.sc, p.exp, data, [0, 1], src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 0 and one == two and c1 == c2


# ------------------------------------------------------------------ 6. the scanner's other calls

def test_extract_after_tally_is_the_extract_of_a_fresh_scanner(gpu):
    data = kv_lines(9, 500, 30)
    with S.Pool() as pool:
        p, fresh = Program(pool, KV), Program(pool, KV)
        _, want, _ = run_extract(fresh.sc, fresh.exp, data, [1, 3], src_off=2, dst_off=9)
        run_tally(p.sc, p.exp, data, [1, 3], src_off=2, dst_off=9)
        run_tally(p.sc, p.exp, data, [1], max_keys=3, overflow=True)
        _, got, _ = run_extract(p.sc, p.exp, data, [1, 3], src_off=2, dst_off=9)
        assert got == want and len(want) > 1000
