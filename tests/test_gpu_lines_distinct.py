"""The line distinct (sre_hip_distinct_lines): the lines of a device buffer deduplicated by their captured key, the first
or the last line of every key or every line of the keys whose count lies in a range (with invert: the keyed lines the rule
does not pick), written as the filter writes lines, with the count and the first line of every line's key.

Expected values are pure Python: the split rule of line mode, the oracle's first-match record of every line (the lookup
test's keys_of), and a dict {key tuple: [first line, last line, count]}.  Output, per-line and index buffers have 64 guard
bytes in front and behind and are pre-filled with 0xA5 (the filter test's Out); every check asserts that the guards and
everything beyond what the call may write still hold 0xA5.
"""
import ctypes
import random

import pytest

import sregex_amd as S
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import COUNTED, Out, download, run_filter
from test_gpu_lines_extract import DOTTED, Program
from test_gpu_lines_tally import KV, PAIR, kv_lines, run_tally, words, dotted_lines
from test_gpu_lines_lookup import keys_of, letters

pytestmark = pytest.mark.gpu

FIRST, LAST, EVERY = S.HIP_DISTINCT_FIRST, S.HIP_DISTINCT_LAST, S.HIP_DISTINCT_EVERY
WHICH = (FIRST, LAST, EVERY)
SIZES = (1, 63, 64, 65, 257, 1024 + 17)


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def per_key(keyed):
    """{key: [first line, last line, count]} in first-occurrence order"""
    d = {}
    for i, _, _, key in keyed:
        e = d.setdefault(key, [i, i, 0])
        e[1] = i
        e[2] += 1
    return d


def qualifies(lo, hi, count):
    return lo <= count and (hi == 0 or count <= hi)


def select(keyed, which, lo, hi, invert):
    """[(line, start, len)] of the selected lines, and the qualifying keys"""
    keys = per_key(keyed)
    sel = []
    for i, st, n, key in keyed:
        first, last, count = keys[key]
        named = i == first if which == FIRST else i == last if which == LAST else True
        if (named and qualifies(lo, hi, count)) != invert:
            sel.append((i, st, n))
    return sel, sum(1 for e in keys.values() if qualifies(lo, hi, e[2]))


def run_distinct(sc, exp, data, groups, which=FIRST, lo=1, hi=0, invert=False, max_keys=None, delim=0x0A, src_off=0, dst_off=0,
                 out_cap=None, keycount_cap=None, keyline_cap=None, index_cap=None, null_out=False, overflow=False):
    """one call, checked in full; returns (info, output bytes, key counts of all lines, key lines of all lines)"""
    lib = sc.lib
    d = bytes([delim])
    nlines = len(split_lines(data, delim))
    keyed = keys_of(exp, data, groups, delim)
    keys = per_key(keyed)
    sel, kept = select(keyed, which, lo, hi, invert)
    want_count, want_line = [0] * nlines, [-1] * nlines
    for i, _, _, key in keyed:
        want_line[i], _, want_count[i] = keys[key]
    need = sum(n + 1 for _, _, n in sel)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for _, _, n in sel:
        if out_bytes + n + 1 > cap:
            break
        out_bytes += n + 1
        nwritten += 1
    want = b"".join(data[st:st + n] + d for _, st, n in sel[:nwritten])
    mk = max(len(keys), 1) if max_keys is None else max_keys
    ccap = nlines + 3 if keycount_cap is None else keycount_cap
    lcap = nlines + 3 if keyline_cap is None else keyline_cap
    icap = len(sel) + 3 if index_cap is None else index_cap
    src = upload_at(data, src_off)
    out, kc, kl, idx = Out(lib, cap, dst_off), Out(lib, ccap * 8, 0), Out(lib, lcap * 8, 0), Out(lib, icap * 32, 0)
    try:
        args = (src.ptr + src_off, len(data), None if null_out else out.ptr, cap, groups, mk, which, lo, hi, delim, invert,
                kc.ptr if ccap else None, ccap, kl.ptr if lcap else None, lcap, idx.ptr if icap else None, icap)
        if overflow:
            with pytest.raises(S.TallyOverflow) as e:
                sc.distinct_lines(*args)
            assert e.value.info == S.DistinctInfo(nlines, len(keyed), 0, 0, 0, 0, 0, 0), e.value.info
            for o in (out, kc, kl, idx):
                o.check(b"")            # 0xA5 throughout
            return e.value.info, b"", [], []
        info = sc.distinct_lines(*args)
        assert info == S.DistinctInfo(nlines, len(keyed), len(keys), kept, len(sel), need, nwritten, out_bytes), \
            (info, len(keyed), len(keys), kept, len(sel), need)
        if which != EVERY and not invert:
            assert info.nselected == info.nkeys_kept
        out.check(want)
        # the per-line arrays are complete whatever which, the range, the flags and out_cap are
        got_count = words(lib, kc, min(ccap, nlines), ctypes.c_uint64)
        assert got_count == want_count[:ccap], [(i, g, w) for i, (g, w) in enumerate(zip(got_count, want_count)) if g != w][:3]
        got_line = words(lib, kl, min(lcap, nlines))
        assert got_line == want_line[:lcap], [(i, g, w) for i, (g, w) in enumerate(zip(got_line, want_line)) if g != w][:3]
        nrows = min(icap, nwritten)
        rows, o = [], 0
        for i, st, n in sel[:nrows]:
            rows.append((i, st, n, o))
            o += n + 1
        raw = words(lib, idx, 4 * nrows)
        got = [tuple(raw[4 * r:4 * r + 4]) for r in range(nrows)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
    finally:
        for b in (src, out, kc, kl, idx):
            b.free()
    return info, want, want_count, want_line


def ranges(keyed):
    most = max([e[2] for e in per_key(keyed).values()] or [0])
    return [(1, 0), (1, 1), (2, 0), (2, 3), (most, 0), (most + 1, 0)]


def keyed_lines(seed, n, nkeys, miss=0.15):
    """n lines k=KEY over nkeys distinct keys (every key used when n allows); some lines have no match"""
    rng = random.Random(seed)
    pads = [b"", b" ", b"-- ", b"at 12 "]
    out = []
    for i in range(n):
        if n > 1 and rng.random() < miss:
            out.append(b"no key here")
        else:
            j = i if nkeys >= n else rng.randrange(nkeys)
            out.append(pads[i % 4] + b"k=" + letters(j) + b";" + pads[(i // 4) % 4])
    return b"\n".join(out) + (b"\n" if n % 2 else b"")


# ------------------------------------------------------------------ 1. sizes, cardinalities, which x invert, ranges

@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_key_cardinalities(gpu, n):
    with S.Pool() as pool:
        p = Program(pool, KV)
        assert p.sc.engine == S.ENGINE_SCAN
        for nkeys in sorted({1, 3, max(n // 2, 1), n}):
            data = keyed_lines(n * 7 + nkeys, n, nkeys)
            rng = random.Random(n + nkeys)
            for which in WHICH:
                for invert in (False, True):
                    info, _, _, _ = run_distinct(p.sc, p.exp, data, [1], which, 1, 0, invert, src_off=rng.randrange(1, 16),
                                                 dst_off=rng.randrange(1, 16))
                    assert p.sc.last_lines_device == 1
                    if n >= 63:
                        assert 0 < info.nkeyed < info.nlines and (info.nkeys <= nkeys if nkeys < n else info.nkeys == info.nkeyed)
        assert run_distinct(p.sc, p.exp, b"", [1])[0] == S.DistinctInfo(0, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("which", WHICH)
def test_ranges(gpu, which):
    data = kv_lines(13, 400, 60)
    with S.Pool() as pool:
        p = Program(pool, KV)
        keyed = keys_of(p.exp, data, [1, 3])
        rs = ranges(keyed)
        assert rs[-2][0] >= 4
        for invert in (False, True):
            got = {}
            for lo, hi in rs:
                got[lo, hi] = run_distinct(p.sc, p.exp, data, [1, 3], which, lo, hi, invert)[0]
            assert got[rs[-1]].nkeys_kept == 0 and got[rs[-1]].nselected == (got[rs[-1]].nkeyed if invert else 0)
            assert got[rs[-2]].nkeys_kept >= 1 and got[1, 0].nkeys_kept == got[1, 0].nkeys
            assert got[1, 1].nkeys_kept + got[2, 0].nkeys_kept == got[1, 0].nkeys


def test_invert_and_plain_interleave_to_the_keyed_lines(gpu):
    data = kv_lines(17, 500, 70)
    with S.Pool() as pool:
        p = Program(pool, KV)
        keyed = [(i, st, n) for i, st, n, _ in keys_of(p.exp, data, [1])]
        src = upload_at(data, 0)
        cap, icap = len(data) + 8, len(keyed)
        try:
            for which in WHICH:
                for lo, hi in ((1, 0), (2, 3)):
                    rows = []
                    for invert in (False, True):
                        out, idx = Out(gpu, cap, 0), Out(gpu, icap * 32, 0)
                        try:
                            info = p.sc.distinct_lines(src.ptr, len(data), out.ptr, cap, [1], 1000, which, lo, hi, invert=invert,
                                                       index_ptr=idx.ptr, index_cap=icap)
                            raw = words(gpu, idx, 4 * info.nwritten)
                            text = download(gpu, out.ptr, info.out_bytes)
                            rows += [(raw[4 * r], raw[4 * r + 1], raw[4 * r + 2], text[raw[4 * r + 3]:raw[4 * r + 3] + raw[4 * r + 2]])
                                     for r in range(info.nwritten)]
                        finally:
                            out.free()
                            idx.free()
                    rows.sort()
                    assert [r[:3] for r in rows] == keyed
                    assert all(t == data[st:st + n] for _, st, n, t in rows)
        finally:
            src.free()


# ------------------------------------------------------------------ 2. field rules

def test_fields_are_compared_one_by_one(gpu):
    """("ab", "c") and ("a", "bc") stay apart; a group named twice works"""
    lines = [b"<ab><c>", b"<a><bc>", b"<abc><>", b"<><abc>", b"nothing", b"<ab><c>", b"<a><bc>", b"<a><bc>"]
    data = b"\n".join(lines)
    with S.Pool() as pool:
        p = Program(pool, PAIR)
        info, out, cnt, line = run_distinct(p.sc, p.exp, data, [1, 2])
        assert out == b"<ab><c>\n<a><bc>\n<abc><>\n<><abc>\n" and cnt == [2, 3, 1, 1, 0, 2, 3, 3] and line == [0, 1, 2, 3, -1, 0, 1, 1]
        info, out, _, _ = run_distinct(p.sc, p.exp, data, [1, 2], LAST)
        assert out == b"<abc><>\n<><abc>\n<ab><c>\n<a><bc>\n"
        info, out, _, _ = run_distinct(p.sc, p.exp, data, [1, 2], FIRST, 1, 1)             # uniq -u
        assert out == b"<abc><>\n<><abc>\n"
        info, out, _, _ = run_distinct(p.sc, p.exp, data, [1, 2], FIRST, 2, 0)             # uniq -d
        assert out == b"<ab><c>\n<a><bc>\n"
        info, out, _, _ = run_distinct(p.sc, p.exp, data, [1, 2], EVERY, 3, 0)             # uniq -D, at least 3
        assert out == b"<a><bc>\n" * 3
        info, out, _, _ = run_distinct(p.sc, p.exp, data, [1, 2], FIRST, invert=True)       # the duplicates
        assert out == b"<ab><c>\n<a><bc>\n<a><bc>\n"
        # group 1 alone: "<a><bc>" lines; group 1 named twice gives the same keys
        a = run_distinct(p.sc, p.exp, data, [1])
        b = run_distinct(p.sc, p.exp, data, [1, 1])
        assert a[1:] == b[1:] and a[0] == b[0]


def test_an_unset_group_equals_an_empty_one(gpu):
    """group 3 unset ("k=a") and empty ("k=a;v=") are one key"""
    data = b"k=a\nk=a;v=\nk=a;v=1\nk=b;v=1\nk=a;v=\n"
    with S.Pool() as pool:
        p = Program(pool, KV)
        info, out, cnt, line = run_distinct(p.sc, p.exp, data, [1, 3])
        assert out == b"k=a\nk=a;v=1\nk=b;v=1\n" and cnt == [3, 3, 1, 1, 3] and line == [0, 0, 2, 3, 0]
        info, out, _, _ = run_distinct(p.sc, p.exp, data, [1, 3], LAST)
        assert out == b"k=a;v=1\nk=b;v=1\nk=a;v=\n"


def test_empty_lines_are_keyed_by_a_program_that_matches_the_empty_text(gpu):
    data = b"\n\nab\n\nab\nc\n\n"
    with S.Pool() as pool:
        p = Program(pool, [rb"([a-z]*)"])
        info, out, cnt, line = run_distinct(p.sc, p.exp, data, [1])
        assert out == b"\nab\nc\n" and cnt == [4, 4, 2, 4, 2, 1, 4] and line == [0, 0, 2, 0, 2, 5, 0]
        info, out, _, _ = run_distinct(p.sc, p.exp, data, [1], LAST)
        assert out == b"ab\nc\n\n" and info.nkeyed == info.nlines == 7
        info, out, _, _ = run_distinct(p.sc, p.exp, data, [0], EVERY, 2, 0, invert=True)
        assert out == b"c\n"


# ------------------------------------------------------------------ 3. batches, chains, overflow

def test_a_keys_first_and_last_lines_in_different_batches(gpu, monkeypatch):
    data = keyed_lines(5, 1024 + 17, 40)
    with S.Pool() as pool:
        p = Program(pool, KV)
        one = {(w, inv): run_distinct(p.sc, p.exp, data, [1], w, 1, 0, inv, src_off=1, dst_off=2) for w in WHICH for inv in (False, True)}
        assert p.sc.last_line_batches == 1
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "100")
        keys = per_key(keys_of(p.exp, data, [1]))
        assert all(e[0] // 100 != e[1] // 100 for e in keys.values())
        for (w, inv), want in one.items():
            assert run_distinct(p.sc, p.exp, data, [1], w, 1, 0, inv, src_off=1, dst_off=2) == want
            assert p.sc.last_line_batches == 11


def test_long_probe_chains(gpu, monkeypatch):
    data = b"\n".join(b"k=" + letters(i % 300) for i in range(700)) + b"\nnone\n"
    with S.Pool() as pool:
        p = Program(pool, KV)
        whole = {(w, inv): run_distinct(p.sc, p.exp, data, [1], w, 2, 0, inv) for w in WHICH for inv in (False, True)}
        assert whole[FIRST, False][0].nkeys == 300 and whole[FIRST, False][0].nkeys_kept == 300
        for bits in ("0", "1"):
            monkeypatch.setenv("SRE_HIP_TALLY_HASH_BITS", bits)
            for (w, inv), want in whole.items():
                assert run_distinct(p.sc, p.exp, data, [1], w, 2, 0, inv) == want


def test_max_keys_and_overflow(gpu):
    data = kv_lines(4, 700, 60)
    with S.Pool() as pool:
        p = Program(pool, KV)
        distinct = len(per_key(keys_of(p.exp, data, [1, 3])))
        assert distinct > 20
        for which in WHICH:
            run_distinct(p.sc, p.exp, data, [1, 3], which, max_keys=distinct - 1, overflow=True)
            assert run_distinct(p.sc, p.exp, data, [1, 3], which, max_keys=distinct)[0].nkeys == distinct
        run_distinct(p.sc, p.exp, data, [1, 3], FIRST, max_keys=1, overflow=True, invert=True)


# ------------------------------------------------------------------ 4. truncation, capacities, alignment

def test_truncation_and_side_arrays(gpu):
    data = kv_lines(6, 300, 40)
    with S.Pool() as pool:
        p = Program(pool, KV)
        for which, invert in ((FIRST, False), (LAST, False), (EVERY, False), (FIRST, True)):
            lo = 2 if which == EVERY else 1
            info, out, _, _ = run_distinct(p.sc, p.exp, data, [1, 3], which, lo, 0, invert)
            need, row = info.need_bytes, out.index(b"\n") + 1
            assert info.out_bytes == need > row and info.nselected > 3
            for cap in (need, need - 1, row, 0):
                got = run_distinct(p.sc, p.exp, data, [1, 3], which, lo, 0, invert, out_cap=cap, dst_off=3)[0]
                assert (got.nkeyed, got.nkeys, got.nkeys_kept, got.need_bytes) == (info.nkeyed, info.nkeys, info.nkeys_kept, need)
                assert got.nwritten == {need: info.nselected, need - 1: info.nselected - 1, row: 1, 0: 0}[cap]
            # a sizing call still delivers both per-line arrays in full (run_distinct checks them)
            got = run_distinct(p.sc, p.exp, data, [1, 3], which, lo, 0, invert, out_cap=0, null_out=True)[0]
            assert got.need_bytes == need and got.nwritten == 0
            for ccap, lcap, icap in ((17, 3, 3), (1, 1, 1), (0, 0, 0), (300, 0, 0), (0, 300, 2), (0, 5, 0)):
                run_distinct(p.sc, p.exp, data, [1, 3], which, lo, 0, invert, keycount_cap=ccap, keyline_cap=lcap, index_cap=icap)


@pytest.mark.parametrize("src_off,dst_off", [(1, 15), (7, 1), (15, 7)])
def test_odd_alignments_and_a_final_line_without_a_delimiter(gpu, src_off, dst_off):
    data = kv_lines(src_off, 260, 50)
    assert not data.endswith(b"\n")
    with S.Pool() as pool:
        p = Program(pool, KV)
        for which in WHICH:
            run_distinct(p.sc, p.exp, data, [1], which, 1, 0, False, src_off=src_off, dst_off=dst_off)
        # the final line is the last of its key, and a key of its own
        tail = data + b"\nk=" + letters(src_off) + b"\nk=onlyhere"
        info, out, _, _ = run_distinct(p.sc, p.exp, tail, [1], LAST, src_off=src_off, dst_off=dst_off)
        assert out.endswith(b"k=" + letters(src_off) + b"\nk=onlyhere\n")


# ------------------------------------------------------------------ 5. routes and scanner modes

def test_the_nfa_tier_and_the_host_route(gpu, monkeypatch):
    data = dotted_lines(5, 300)
    with S.Pool() as pool:
        p = Program(pool, DOTTED, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        res = {}
        for which in WHICH:
            for invert in (False, True):
                res[which, invert] = run_distinct(p.sc, p.exp, data, [0, 1], which, 2, 0, invert, src_off=3, dst_off=5)
                assert p.sc.last_lines_device == 1 and 0 < res[which, invert][0].nkeys_kept <= res[which, invert][0].nkeys
        monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
        for (which, invert), want in res.items():
            assert run_distinct(p.sc, p.exp, data, [0, 1], which, 2, 0, invert, src_off=3, dst_off=5) == want
            assert p.sc.last_lines_device == 0


def test_a_counted_repeat_on_the_nfa_tier(gpu):
    rng = random.Random(9)
    heads = [bytes(rng.choice(b"ab") for _ in range(rng.randrange(8, 14))) for _ in range(9)]
    data = b"\n".join(rng.choice([b"", b"x "]) + rng.choice(heads) + rng.choice([b"@z", b"", b"@"]) for _ in range(200))
    with S.Pool() as pool:
        p = Program(pool, COUNTED, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        for which in WHICH:
            info = run_distinct(p.sc, p.exp, data, [0], which, 1, 0, False)[0]
            assert p.sc.last_lines_device == 1 and 1 < info.nkeys < info.nkeyed < info.nlines


def test_thompson_and_count_scanners_are_refused(gpu, capfd):
    data = b"k=a\nk=b\nk=a\n"
    src = upload_at(data, 0)
    out = Out(gpu, 256, 0)
    info = (ctypes.c_size_t * 8)(*([77] * 8))
    arr = (ctypes.c_int * 1)(1)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, KV))
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                capfd.readouterr()
                sc = S.Scanner(pool, prog, mode)
                assert gpu.sre_hip_distinct_lines(sc.h, src.ptr, len(data), 0x0A, arr, 1, FIRST, 1, 0, 0, 16, out.ptr, 256, None, 0,
                                                  None, 0, None, 0, info, None) == -1
                assert "line distinct" in capfd.readouterr().err            # by name
            sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
            arr[0] = 4          # not a group of the program
            assert gpu.sre_hip_distinct_lines(sc.h, src.ptr, len(data), 0x0A, arr, 1, FIRST, 1, 0, 0, 16, out.ptr, 256, None, 0,
                                              None, 0, None, 0, info, None) == -1
            assert list(info) == [77] * 8
            out.check(b"")
            arr[0] = 1
            assert gpu.sre_hip_distinct_lines(sc.h, src.ptr, len(data), 0x0A, arr, 1, FIRST, 1, 0, 0, 16, out.ptr, 256, None, 0,
                                              None, 0, None, 0, info, None) == 0
            assert list(info) == [3, 3, 2, 2, 2, 8, 2, 8]
            out.check(b"k=a\nk=b\n")
    finally:
        src.free()
        out.free()


# ------------------------------------------------------------------ 6. equivalences with existing calls

def test_every_1_0_is_the_filter(gpu):
    data = kv_lines(23, 500, 45)
    with S.Pool() as pool:
        p = Program(pool, KV)
        f, ftext = run_filter(p.sc, p.exp, data, 0x0A, S.HIP_PIKE_FIRST, src_off=2, dst_off=9)[:2]
        d, dtext, _, _ = run_distinct(p.sc, p.exp, data, [1], EVERY, 1, 0, src_off=2, dst_off=9)
        assert dtext == ftext and (d.nselected, d.need_bytes, d.nwritten, d.out_bytes) == (f.nselected, f.need_bytes, f.nwritten, f.out_bytes)
        # (both helpers checked the same four-word index rows against the same expected lines)
        assert run_filter(p.sc, p.exp, data, 0x0A, S.HIP_PIKE_FIRST, src_off=2, dst_off=9)[:2] == (f, ftext)


@pytest.mark.parametrize("groups", [[1], [1, 3]], ids=["K1", "K2"])
def test_first_writes_the_lines_the_tally_names(gpu, groups):
    data = kv_lines(21, 700, 80)
    nlines = len(split_lines(data, 0x0A))
    width = 4 + 2 * len(groups)
    with S.Pool() as pool:
        p = Program(pool, KV)
        src = upload_at(data, 3)
        bufs = [S.DeviceBuffer(1 << 16) for _ in range(3)] + [S.DeviceBuffer(8 * nlines) for _ in range(4)]
        rows, tidx, didx, tcnt, tid, dcnt, dline = bufs
        try:
            t = p.sc.tally_lines(src.ptr + 3, len(data), rows.ptr, 1 << 16, groups, 1000, counts_ptr=tcnt.ptr, counts_cap=nlines,
                                 keyid_ptr=tid.ptr, keyid_cap=nlines, index_ptr=tidx.ptr, index_cap=(1 << 16) // (8 * width))
            d = p.sc.distinct_lines(src.ptr + 3, len(data), None, 0, groups, 1000, keycount_ptr=dcnt.ptr, keycount_cap=nlines,
                                    keyline_ptr=dline.ptr, keyline_cap=nlines, index_ptr=didx.ptr, index_cap=(1 << 16) // 32)
            assert (d.nkeyed, d.nkeys, d.nkeys_kept, d.nselected) == (t.nselected, t.nkeys, t.nkeys, t.nkeys) and t.nkeys > 50
            d = p.sc.distinct_lines(src.ptr + 3, len(data), rows.ptr, 1 << 16, groups, 1000, index_ptr=didx.ptr,
                                    index_cap=(1 << 16) // 32)
            assert d.nwritten == t.nkeys

            def i64(buf, n):
                return list((ctypes.c_int64 * n).from_buffer_copy(buf.to_bytes(8 * n)))
            ti, di = i64(tidx, width * t.nkeys), i64(didx, 4 * t.nkeys)
            firsts = [ti[width * k] for k in range(t.nkeys)]
            assert firsts == [di[4 * k] for k in range(t.nkeys)]
            counts, keyid, kcount, kline = i64(tcnt, t.nkeys), i64(tid, nlines), i64(dcnt, nlines), i64(dline, nlines)
            assert [kcount[f] for f in firsts] == counts
            assert [(-1 if kline[i] < 0 else keyid[kline[i]]) for i in range(nlines)] == keyid
            assert [(0 if keyid[i] < 0 else counts[keyid[i]]) for i in range(nlines)] == kcount
        finally:
            for x in [src] + bufs:
                x.free()


def test_sort_then_first_is_sort_u(gpu):
    rng = random.Random(31)
    lines = [letters(rng.randrange(150)) for _ in range(600)]
    data = b"\n".join(lines) + b"\n"
    with S.Pool() as pool:
        p = Program(pool, [rb"[a-z]+"])
        src = upload_at(data, 0)
        mid, out = S.DeviceBuffer(len(data) + 16), Out(gpu, len(data), 0)
        try:
            s = p.sc.sort_lines_text(src.ptr, len(data), mid.ptr, len(data), 0)
            assert s.out_bytes == len(data)
            d = p.sc.distinct_lines(mid.ptr, s.out_bytes, out.ptr, len(data), [0], 1000)
            want = b"".join(t + b"\n" for t in sorted(set(lines)))
            assert d.nselected == d.nkeys == len(set(lines)) and d.out_bytes == len(want)
            out.check(want)
        finally:
            for x in (src, mid, out):
                x.free()


def test_first_on_its_own_output_reproduces_it_and_two_calls_agree(gpu):
    data = kv_lines(29, 600, 70)
    with S.Pool() as pool:
        p = Program(pool, KV)
        for which in (FIRST, LAST):
            a = run_distinct(p.sc, p.exp, data, [1, 3], which, src_off=5, dst_off=3)
            b = run_distinct(p.sc, p.exp, data, [1, 3], which, src_off=5, dst_off=3)
            assert a == b and a[0].nselected > 30
            again = run_distinct(p.sc, p.exp, a[1], [1, 3], FIRST)
            assert again[1] == a[1] and again[0].nkeys == again[0].nselected == a[0].nselected
        t0 = run_tally(p.sc, p.exp, data, [1, 3], src_off=2, dst_off=9)
        run_distinct(p.sc, p.exp, data, [1], LAST)
        assert run_tally(p.sc, p.exp, data, [1, 3], src_off=2, dst_off=9) == t0
