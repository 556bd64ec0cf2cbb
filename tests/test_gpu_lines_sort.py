"""The line sort (sre_hip_sort_lines) on the device against pure Python: the oracle's first-match text of the sort group per
line (keys_of), its value under the tally's number rule (S.tally_number), and sorted(key=(v or -v, line)) for the order; the
lines that are not numbered follow in line order under ALL; limit is a slice.  Output and index buffers carry guard bytes and
a fill.  Unless a case opts out, the runner asserts of its INPUT that an unsorted or unstable output could not pass: at least
two distinct values, not already in output order, and two equal values with a different one between them in the buffer."""
import ctypes
import random

import pytest

import sregex_amd as S
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import Out, run_filter
from test_gpu_lines_extract import Program
from test_gpu_lines_tally import words
from test_gpu_lines_lookup import keys_of

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
SIZES = (1, 63, 64, 65, 257, 1024 + 17, 2 * 1024 + 1)
BIG = 10 ** 18 - 1
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
# group 1: the text between "v=" and ";", empty for "v=;", unset for a line that only has "u="
VAL = [rb"(?:v=([^;]*);|u=)"]
# two columns
AB = [rb"a=(-?[0-9]*) b=(-?[0-9]*)"]
# a counted repeat, for the NFA tier
COUNTED = [rb"t=[0-9]{1,3}ms n=(-?[0-9]*)"]
NOT_NUMBERS = (b"+1", b"1 ", b"-", b"1234567890123456789", b"", b"12a")


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def host_passes(max_key):
    return (max(max_key.bit_length(), 1) + 7) // 8


def expect(exp, data, group, desc, all_lines, delim=0x0A):
    """(classes, values, [(line, start, len)] of the candidates in output order)"""
    lines = split_lines(data, delim)
    cls, val = [-2] * len(lines), [0] * len(lines)
    for i, _, _, key in keys_of(exp, data, [group], delim):
        v = S.tally_number(key[0])
        cls[i], val[i] = (1, v) if v is not None else (-1, 0)
    numbered = sorted((i for i in range(len(lines)) if cls[i] == 1), key=lambda i: (-val[i] if desc else val[i], i))
    rest = [i for i in range(len(lines)) if cls[i] != 1] if all_lines else []
    return cls, val, [(i,) + lines[i] for i in numbered + rest]


def shape_holds(cls, val, cand):
    nums = [val[i] for i in range(len(cls)) if cls[i] == 1]         # in line order
    order = [r[0] for r in cand]
    last, between = {}, False
    for at, v in enumerate(nums):
        if v in last and any(w != v for w in nums[last[v] + 1:at]):
            between = True
        last[v] = at
    return len(set(nums)) >= 2 and order != sorted(order) and between


def run_sort(sc, exp, data, group, desc=False, all_lines=False, limit=0, delim=0x0A, src_off=0, dst_off=0, out_cap=None,
             index_cap=None, null_out=False, shape=True):
    """one call, checked in full; returns (info, output bytes, index rows)"""
    lib = sc.lib
    d = bytes([delim])
    cls, val, cand = expect(exp, data, group, desc, all_lines, delim)
    nlines = len(cls)
    if shape and len(cand) >= 4:
        assert shape_holds(cls, val, cand), "the case's input does not exercise the sort"
    nums = [v for c, v in zip(cls, val) if c == 1]
    vmin, vmax = min(nums, default=I64_MAX), max(nums, default=I64_MIN)
    rng_ = vmax - vmin if nums else 0
    passes = host_passes(rng_ + 1 if all_lines and len(nums) < nlines else rng_) if cand else 0
    sel = cand[:limit] if limit else cand
    need = sum(n + 1 for _, _, n in sel)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for _, _, n in sel:
        if out_bytes + n + 1 > cap:
            break
        out_bytes += n + 1
        nwritten += 1
    want = b"".join(data[st:st + n] + d for _, st, n in sel[:nwritten])
    icap = len(sel) + 3 if index_cap is None else index_cap
    src = upload_at(data, src_off)
    out, idx = Out(lib, cap, dst_off), Out(lib, icap * 48, 0)
    try:
        info = sc.sort_lines(src.ptr + src_off, len(data), None if null_out else out.ptr, cap, group, delim, desc, all_lines, limit,
                             idx.ptr if icap else None, icap)
        want_info = S.SortInfo(nlines, sum(1 for c in cls if c != -2), len(nums), len(sel), need, nwritten, out_bytes, passes, vmin, vmax)
        print("sort_lines", nlines, "lines:", info)
        assert info == want_info, (info, want_info)
        out.check(want)
        nidx = min(icap, nwritten)
        rows, o = [], 0
        for i, st, n in sel[:nidx]:
            rows.append((i, st, n, o, val[i], cls[i]))
            o += n + 1
        raw = words(lib, idx, 6 * nidx)
        got = [tuple(raw[6 * r:6 * r + 6]) for r in range(nidx)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
    finally:
        for b in (src, out, idx):
            b.free()
    return info, want, rows


def value_lines(seed, nlines, lo, hi, pick=None, junk=0.25, final_delim=None, extra=()):
    """lines around v=TEXT; with TEXT drawn from a pool of about nlines / 3 values of [lo, hi] (so values repeat); the first
    three numbered lines carry lo, hi, lo, which makes the runner's condition on its input hold.  `junk` of the lines is
    split between no match, an unset group and texts that are not numbers."""
    rng = random.Random(seed)
    pick = pick or (lambda r: r.randrange(lo, hi + 1))
    pool = [lo, hi] + [pick(rng) for _ in range(max(nlines // 3, 1))]
    pads = [b"", b" ", b"-- ", b"at 12 "]
    out, forced = [], [lo, hi, lo]
    for i in range(nlines):
        r = rng.random()
        if r < junk / 3:
            out.append(b"no value here")
        elif r < 2 * junk / 3:
            out.append(pads[i % 4] + b"u= x")
        elif r < junk:
            out.append(pads[i % 4] + b"v=" + rng.choice(NOT_NUMBERS) + b";")
        else:
            v = forced.pop(0) if forced else rng.choice(pool)
            text = rng.choice((b"%d", b"%d", b"00%d")) % v if v >= 0 and hi < 10 ** 15 else b"%d" % v
            out.append(pads[i % 4] + b"v=" + text + b";" + pads[(i // 4) % 4])
    out += list(extra)
    final = nlines % 2 == 1 if final_delim is None else final_delim
    return b"\n".join(out) + (b"\n" if final else b"")


MIXES = {
    # name: (lo, hi, pick or None, passes without ALL)
    "one_digit": (100, 355, None, 1),
    "status_codes": (200, 599, None, 2),
    "sixteen_bits": (0, 65535, None, 2),
    "below_2_24": (0, (1 << 24) - 1, None, 3),
    "below_2_32": (-5, (1 << 32) - 6, None, 4),
    # values that differ ONLY in bits 32 .. 39: a 32-bit digit shift sorts nothing
    "bits_32_to_39": (777, 777 + (255 << 32), lambda r: 777 + (r.randrange(256) << 32), 5),
    # values that differ only in the top digit of an 8-pass range: a dropped last pass sorts nothing
    "top_digit": (0, 7 << 56, lambda r: r.randrange(8) << 56, 8),
    "full_range": (-BIG, BIG, None, 8),
}


# ------------------------------------------------------------------ 1. sizes, directions, ALL

@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    rng = random.Random(n)
    data = value_lines(n, n, 200, 599) if n > 1 else b"x v=42; y"
    with S.Pool() as pool:
        p = Program(pool, VAL)
        assert p.sc.engine == S.ENGINE_SCAN
        for desc in (False, True):
            for all_lines in (False, True):
                # (source and destination at odd alignments)
                so, do = rng.randrange(1, 16) | 1, rng.randrange(1, 16) | 1
                info, out, _ = run_sort(p.sc, p.exp, data, 1, desc, all_lines, src_off=so, dst_off=do)
                assert p.sc.last_lines_device == 1
                if n >= 63:
                    assert 0 < info.nnumbered < info.nkeyed < info.nlines
                assert info.nselected == (info.nlines if all_lines else info.nnumbered)
                if all_lines:
                    assert sorted(out.split(b"\n")[:-1]) == sorted(l for l in data.split(b"\n")[:n])


@pytest.mark.parametrize("mix", sorted(MIXES))
def test_value_mixes_and_their_passes(gpu, mix):
    lo, hi, pick, passes = MIXES[mix]
    data = value_lines(len(mix), 1024 + 17, lo, hi, pick)
    with S.Pool() as pool:
        p = Program(pool, VAL)
        for desc in (False, True):
            info, _, _ = run_sort(p.sc, p.exp, data, 1, desc, False, src_off=3, dst_off=7)
            assert info.passes == passes and (info.vmin, info.vmax) == (lo, hi)
            info, _, _ = run_sort(p.sc, p.exp, data, 1, desc, True, src_off=3, dst_off=7)
            assert info.passes == host_passes(hi - lo + 1)


def test_all_equal_values(gpu):
    data = value_lines(9, 300, -42, -42)
    with S.Pool() as pool:
        p = Program(pool, VAL)
        for desc in (False, True):
            info, out, rows = run_sort(p.sc, p.exp, data, 1, desc, False, shape=False)
            assert info.passes == 1 and info.vmin == info.vmax == -42 and [r[0] for r in rows] == sorted(r[0] for r in rows)
            assert run_sort(p.sc, p.exp, data, 1, desc, True, shape=False)[0].passes == 1


def test_descending_input_and_minus_zero(gpu):
    lines = [b"v=%d;" % (300 - i) for i in range(300)] + [b"v=-0;", b"v=007;", b"v=0;", b"v=7;"]
    data = b"\n".join(lines) + b"\n"
    with S.Pool() as pool:
        p = Program(pool, VAL)
        _, out, rows = run_sort(p.sc, p.exp, data, 1, shape=False)
        assert out.startswith(b"v=-0;\nv=0;\nv=1;\n") and b"v=007;\nv=7;\nv=8;" in out
        assert [r[4] for r in rows[:3]] == [0, 0, 1]
        _, out, _ = run_sort(p.sc, p.exp, data, 1, desc=True, shape=False)
        assert out.startswith(b"v=300;\nv=299;") and out.endswith(b"v=1;\nv=-0;\nv=0;\n")


# ------------------------------------------------------------------ 2. limit, capacities, the index

def test_limits(gpu):
    data = value_lines(21, 700, 200, 209)           # long runs of equal values
    with S.Pool() as pool:
        p = Program(pool, VAL)
        for desc, all_lines in ((False, False), (True, False), (False, True), (True, True)):
            cls, val, cand = expect(p.exp, data, 1, desc, all_lines)
            mid = next(r for r in range(2, len(cand)) if cls[cand[r][0]] == 1 and val[cand[r][0]] == val[cand[r - 1][0]] == val[cand[r + 1][0]])
            full = run_sort(p.sc, p.exp, data, 1, desc, all_lines, src_off=5, dst_off=3)
            for limit in (1, mid, len(cand), len(cand) + 1, 1 << 40):
                info, out, rows = run_sort(p.sc, p.exp, data, 1, desc, all_lines, limit, src_off=5, dst_off=3)
                assert info.nselected == min(limit, len(cand)) and full[1].startswith(out) and rows == full[2][:len(rows)]
                assert (info.nkeyed, info.nnumbered, info.vmin, info.vmax, info.passes) == \
                    (full[0].nkeyed, full[0].nnumbered, full[0].vmin, full[0].vmax, full[0].passes)


def test_truncation_the_sizing_call_and_the_index(gpu):
    data = value_lines(22, 500, 0, 65535)
    with S.Pool() as pool:
        p = Program(pool, VAL)
        for all_lines, limit in ((False, 0), (True, 0), (False, 100)):
            info, out, _ = run_sort(p.sc, p.exp, data, 1, True, all_lines, limit)
            need = info.need_bytes
            assert need == len(out)
            sizing, nothing, _ = run_sort(p.sc, p.exp, data, 1, True, all_lines, limit, out_cap=0, null_out=True)
            assert sizing.need_bytes == need and sizing.nwritten == 0 and nothing == b""
            boundary = len(b"\n".join(out.split(b"\n")[:41])) + 1           # the end of row 41
            short, _, _ = run_sort(p.sc, p.exp, data, 1, True, all_lines, limit, out_cap=boundary - 1, dst_off=9)
            assert short.nwritten == 40 and short.need_bytes == need
            assert run_sort(p.sc, p.exp, data, 1, True, all_lines, limit, out_cap=boundary, dst_off=9)[0].nwritten == 41
            assert run_sort(p.sc, p.exp, data, 1, True, all_lines, limit, out_cap=need)[0].nwritten == info.nselected
            for icap in (0, 7, info.nselected, info.nselected + 50):
                run_sort(p.sc, p.exp, data, 1, True, all_lines, limit, index_cap=icap, src_off=1)
            run_sort(p.sc, p.exp, data, 1, True, all_lines, limit, out_cap=boundary - 1, index_cap=1000)


# ------------------------------------------------------------------ 3. what is not a number, and what has none

def test_not_numbers(gpu):
    junk = [b"v=+1;", b"v=1 ;", b"v=-;", b"v=1234567890123456789;", b"v=;", b"u= only", b"nothing", b"v=--1;", b"v=1.5;"]
    rng = random.Random(6)
    lines = [b"v=%d;" % rng.choice((5, -5, 123456789012345678)) for _ in range(40)]
    for k, j in enumerate(junk):
        lines.insert(3 + 4 * k, j)
    data = b"\n".join(lines)
    with S.Pool() as pool:
        p = Program(pool, VAL)
        info, out, _ = run_sort(p.sc, p.exp, data, 1)
        assert info.nnumbered == 40 and info.nkeyed == 48 and info.nlines == 49 and not any(j in out for j in junk)
        for desc in (False, True):
            info, out, rows = run_sort(p.sc, p.exp, data, 1, desc, True)
            assert out.split(b"\n")[40:49] == junk, "all of them in the rest, in line order, in both directions"
            assert [r[5] for r in rows[40:49]] == [-1, -1, -1, -1, -1, -1, -2, -1, -1] and all(r[4] == 0 for r in rows[40:49])


def test_no_numbered_line_and_the_empty_buffer(gpu):
    data = b"v=x;\nnothing\nu=\nv=;\nv=+5;\n"
    with S.Pool() as pool:
        p = Program(pool, VAL)
        for desc in (False, True):
            info, out, _ = run_sort(p.sc, p.exp, data, 1, desc, False, shape=False)
            assert info == S.SortInfo(5, 4, 0, 0, 0, 0, 0, 0, I64_MAX, I64_MIN) and out == b""
            info, out, _ = run_sort(p.sc, p.exp, data, 1, desc, True, shape=False)
            assert info == S.SortInfo(5, 4, 0, 5, len(data), 5, len(data), 1, I64_MAX, I64_MIN) and out == data
            info, out, _ = run_sort(p.sc, p.exp, b"", 1, desc, True, shape=False)
            assert info == S.SortInfo(0, 0, 0, 0, 0, 0, 0, 0, I64_MAX, I64_MIN)
        assert run_sort(p.sc, p.exp, b"\n" * 3000, 1, False, True, shape=False)[0].nselected == 3000


@pytest.mark.parametrize("final_delim", (False, True))
def test_a_final_line_without_a_delimiter_and_delim_0(gpu, final_delim):
    data = value_lines(31, 130, 0, 50, final_delim=final_delim, junk=0.1)
    with S.Pool() as pool:
        p = Program(pool, VAL)
        for all_lines in (False, True):
            _, out, _ = run_sort(p.sc, p.exp, data, 1, True, all_lines, src_off=7, dst_off=1)
            assert out.endswith(b"\n")
            zero = data.replace(b"\n", b"\0")
            _, out0, _ = run_sort(p.sc, p.exp, zero, 1, True, all_lines, delim=0, src_off=7, dst_off=1)
            assert out0 == out.replace(b"\n", b"\0")


# ------------------------------------------------------------------ 4. engines and batches

def counted_lines(seed, nlines, long_at=None):
    rng = random.Random(seed)
    out = []
    for i in range(nlines):
        v = (50, 900000, 50)[i] if i < 3 else rng.choice((50, 7, -3, 900000, 12))
        line = rng.choice([b"GET / ", b"", b"x "]) + b"t=%dms n=%d" % (rng.randrange(1000), v) if rng.random() < 0.8 or i < 3 else b"t=ms n=1"
        if i == long_at:
            line = bytes(rng.choice(b"xyw ") for _ in range(700)) + b" " + line
        out.append(line)
    return b"\n".join(out)


def test_the_nfa_tier_a_long_line_and_the_host_route(gpu, monkeypatch):
    data = counted_lines(5, 300, long_at=150)
    assert max(n for _, n in split_lines(data, 0x0A)) >= 512
    with S.Pool() as pool:
        p = Program(pool, COUNTED, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        res = {}
        for all_lines in (False, True):
            res[all_lines] = run_sort(p.sc, p.exp, data, 1, True, all_lines, src_off=3, dst_off=5)
            assert p.sc.last_lines_device == 1 and 0 < res[all_lines][0].nnumbered < res[all_lines][0].nlines
        monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
        for all_lines in (False, True):
            got = run_sort(p.sc, p.exp, data, 1, True, all_lines, src_off=3, dst_off=5)
            assert p.sc.last_lines_device == 0 and got == res[all_lines]


def test_a_long_line_on_the_table_driven_scanner(gpu):
    data = value_lines(8, 200, 200, 599, extra=[b"z" * 600 + b" v=300;", b"v=201;" + b"q" * 5000])
    with S.Pool() as pool:
        p = Program(pool, VAL)
        assert p.sc.engine == S.ENGINE_SCAN
        for all_lines in (False, True):
            run_sort(p.sc, p.exp, data, 1, False, all_lines, src_off=9, dst_off=2)


def test_forced_batch_cuts(gpu, monkeypatch):
    data = value_lines(41, 257, 200, 599)
    with S.Pool() as pool:
        p = Program(pool, VAL)
        one = [run_sort(p.sc, p.exp, data, 1, d, a, src_off=1, dst_off=2) for d in (False, True) for a in (False, True)]
        assert p.sc.last_line_batches == 1
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "100")
        two = [run_sort(p.sc, p.exp, data, 1, d, a, src_off=1, dst_off=2) for d in (False, True) for a in (False, True)]
        assert p.sc.last_line_batches == 3 and two == one
        # a run of equal values spans the batches
        rows = one[0][2]
        assert any(len({r[0] // 100 for r in rows if r[4] == v}) == 3 for v in {r[4] for r in rows})


# ------------------------------------------------------------------ 5. composition, neighbours, refusals

def test_two_columns_by_two_calls(gpu):
    """sort by column B, then sort the output by column A: sorted(key=(A, B, line))"""
    rng = random.Random(12)
    rows = [(rng.randrange(-3, 4), rng.randrange(-2, 3)) for _ in range(1500)]
    data = b"\n".join(b"%d: a=%d b=%d" % (i, a, b) for i, (a, b) in enumerate(rows)) + b"\n"
    with S.Pool() as pool:
        p = Program(pool, AB)
        _, by_b, _ = run_sort(p.sc, p.exp, data, 2, src_off=1, dst_off=3)
        _, by_ab, _ = run_sort(p.sc, p.exp, by_b, 1, src_off=5, dst_off=1)
        want = sorted(range(len(rows)), key=lambda i: (rows[i][0], rows[i][1], i))
        assert by_ab == b"".join(b"%d: a=%d b=%d\n" % ((i,) + rows[i]) for i in want)
        _, by_b, _ = run_sort(p.sc, p.exp, data, 2, desc=True)
        _, by_ab, _ = run_sort(p.sc, p.exp, by_b, 1, desc=True)
        want = sorted(range(len(rows)), key=lambda i: (-rows[i][0], -rows[i][1], i))
        assert by_ab == b"".join(b"%d: a=%d b=%d\n" % ((i,) + rows[i]) for i in want)


def test_the_filter_is_unchanged_by_a_sort(gpu):
    """they share grow-only arrays"""
    data = value_lines(51, 1300, 0, 65535)
    with S.Pool() as pool:
        p = Program(pool, VAL)
        before = run_filter(p.sc, p.exp, data, 0x0A, FIRST, src_off=2, dst_off=9)
        for all_lines in (False, True):
            run_sort(p.sc, p.exp, data, 1, True, all_lines, src_off=2, dst_off=9)
        assert run_filter(p.sc, p.exp, data, 0x0A, FIRST, src_off=2, dst_off=9) == before
        run_sort(p.sc, p.exp, data[:4000], 1, False, True, shape=False)
        assert run_filter(p.sc, p.exp, data, 0x0A, FIRST, src_off=2, dst_off=9) == before


def test_refusals(gpu, capfd):
    data = b"v=3;\nv=1;\nv=2;\n"
    src = upload_at(data, 0)
    out = Out(gpu, 256, 0)
    info = S.SortInfoStruct()

    def call(sc, group=1, flags=0, limit=0, out_ptr=None, cap=256, index=(None, 0), delim=0x0A):
        return gpu.sre_hip_sort_lines(sc.h, src.ptr, len(data), delim, group, flags, limit, out.ptr if out_ptr is None else out_ptr, cap,
                                      index[0], index[1], ctypes.byref(info), None)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, VAL))
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                capfd.readouterr()
                assert call(S.Scanner(pool, prog, mode)) == -1
                assert "line sort" in capfd.readouterr().err        # by name
            sc = S.Scanner(pool, prog, FIRST)
            for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_ALL | S.HIP_LINES_INVERT, 8, S.HIP_SORT_DESC | 8, 1 << 30):
                assert call(sc, flags=flags) == -1
            assert call(sc, group=2) == -1 and call(sc, group=-1) == -1 and call(sc, group=70000) == -1
            assert call(sc, index=(None, 3)) == -1 and call(sc, out_ptr=0, cap=4) == -1
            assert call(sc, delim=256) == -1 and call(sc, delim=-1) == -1
            assert call(sc, out_ptr=src.ptr + 2, cap=4) == -1                       # the output overlaps the buffer
            out.check(b"")
            assert call(sc, flags=S.HIP_SORT_DESC, limit=2) == 0
            assert [getattr(info, f) for f in S.SortInfo._fields] == [3, 3, 3, 2, 10, 2, 10, 1, 1, 3]
            out.check(b"v=3;\nv=2;\n")
            assert call(sc, group=0, flags=S.HIP_LINES_ALL) == 0 and info.nnumbered == 0 and info.nselected == 3
    finally:
        src.free()
        out.free()
