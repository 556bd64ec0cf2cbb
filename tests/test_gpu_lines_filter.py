"""The line filter (sre_hip_filter_lines): the selected lines of a device buffer, each followed by one delimiter,
compacted in order into another device buffer, with an optional device-side index.

Expected output is pure Python: the split rule of line mode, the oracle's verdict on every line, joined with
delimiters.  Every output buffer has 64 guard bytes in front and behind and is pre-filled with 0xA5; every check
asserts that the guards and everything at or beyond out_bytes still hold 0xA5.
"""
import ctypes
import os
import random

import pytest

import sregex_amd as S
from test_gpu_lines import Expect, split_lines, upload_at
from test_gpu_nfa_wide import WIDE

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
HEADLINE = [rb"[a-z]+@[a-z]+\.[a-z]+"]
COUNTED = [rb"(?:a|b)*a(?:a|b){7}@"]
DOTTED = [rb"\d{1,3}(\.\d{1,3}){3}"]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def download(lib, ptr, n):
    out = ctypes.create_string_buffer(max(n, 1))
    if n and lib.sre_hip_download(out, ptr, n) != 0:
        raise RuntimeError("download failed")
    return out.raw[:n]


class Out:
    """GUARD bytes, `offset` more (the output's alignment), `cap` bytes of output, GUARD bytes; all FILL"""

    def __init__(self, lib, cap, offset):
        self.lib, self.cap, self.front = lib, cap, GUARD + offset
        self.total = self.front + cap + GUARD
        self.buf = S.DeviceBuffer(self.total)
        assert self.buf.ptr % 16 == 0
        if lib.sre_hip_upload(self.buf.ptr, bytes([FILL]) * self.total, self.total) != 0:
            raise RuntimeError("upload failed")
        self.ptr = self.buf.ptr + self.front

    def check(self, want):
        """the output is `want`, and nothing else was touched"""
        got = download(self.lib, self.buf.ptr, self.total)
        assert got[:self.front] == bytes([FILL]) * self.front, "written in front of the output"
        body = got[self.front:self.front + len(want)]
        assert body == want, first_difference(body, want)
        rest = got[self.front + len(want):]
        assert rest == bytes([FILL]) * len(rest), ("written at or beyond out_bytes", len(want))

    def free(self):
        self.buf.free()


def first_difference(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return ("first difference at", k, a[max(0, k - 8):k + 8], b[max(0, k - 8):k + 8])
    return ("lengths", len(a), len(b))


def expected(exp, data, delim, mode, invert=False, all_lines=False):
    """[(line, start, len)] of the selected lines"""
    out = []
    for i, (st, n) in enumerate(split_lines(data, delim)):
        hit = exp.record(data[st:st + n], mode)[0] != S.SRE_DECLINED
        if all_lines or hit != invert:
            out.append((i, st, n))
    return out


def cut(sel, cap):
    """the selected lines that fit cap whole, and their bytes"""
    k, total = 0, 0
    for _, _, n in sel:
        if total + n + 1 > cap:
            break
        total += n + 1
        k += 1
    return k, total


def run_filter(sc, exp, data, delim, mode, src_off=0, dst_off=0, invert=False, all_lines=False, out_cap=None,
               index_cap=None, null_out=False):
    """one call, checked in full; returns (info, output bytes)"""
    lib = sc.lib
    d = bytes([delim])
    sel = expected(exp, data, delim, mode, invert, all_lines)
    need = sum(n + 1 for _, _, n in sel)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = cut(sel, cap)
    want = b"".join(data[st:st + n] + d for _, st, n in sel[:nwritten])
    assert len(want) == out_bytes
    icap = len(sel) + 3 if index_cap is None else index_cap
    src = upload_at(data, src_off)
    out = Out(lib, cap, dst_off)
    idx = Out(lib, icap * 32, 0)
    try:
        info = sc.filter_lines(src.ptr + src_off, len(data), None if null_out else out.ptr, cap, delim, invert, all_lines,
                               idx.ptr if icap else None, icap)
        assert info == S.FilterInfo(len(split_lines(data, delim)), len(sel), need, nwritten, out_bytes), (info, len(sel), need)
        out.check(want)
        nrows = min(icap, nwritten)
        rows, o = [], 0
        for i, st, n in sel[:nrows]:
            rows.append((i, st, n, o))
            o += n + 1
        raw = (ctypes.c_int64 * (4 * nrows)).from_buffer_copy(download(lib, idx.ptr, 32 * nrows)) if nrows else []
        got = [tuple(raw[4 * r:4 * r + 4]) for r in range(nrows)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
        idx.check(download(lib, idx.ptr, 32 * nrows))          # nothing behind the rows, nothing around the index
    finally:
        src.free()
        out.free()
        idx.free()
    return info, want


# ------------------------------------------------------------------ 1. the split

def test_split_edges(gpu):
    with S.Pool() as pool:
        for pats in ([rb"a"], [rb"^$|b"]):          # the second matches the empty line
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            exp = Expect(prog, re.ncaps)
            sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
            for delim in (0x0A, 0, 255):
                d = bytes([delim])
                for data in [b"", d, b"a" + d + d + b"b", b"a", d * 5, d * 40 + b"a", b"a" + d, b"b" + d + b"a" + d + d]:
                    for invert in (False, True):
                        info, _ = run_filter(sc, exp, data, delim, S.HIP_PIKE_FIRST, invert=invert)
                    if data == b"":
                        assert info == S.FilterInfo(0, 0, 0, 0, 0)
            # empty lines are selected by the second program: a buffer of delimiters comes back whole
            if pats == [rb"^$|b"]:
                info, want = run_filter(sc, exp, b"\n" * 300, 0x0A, S.HIP_PIKE_FIRST)
                assert info.nselected == 300 and want == b"\n" * 300


# ------------------------------------------------------------------ 2. alignment and lengths

LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
PATTERNS = ["every", "second", "first", "last", "none"]


def marked_buffer(rng, mark, pattern, final_delim):
    """lines of LENGTHS and one of 200 KiB; `mark` is put into the lines the pattern picks"""
    lens = LENGTHS[:7] + [200 * 1024] + LENGTHS[7:]
    lines = []
    for i, n in enumerate(lens):
        pick = {"every": True, "second": i % 2 == 1, "first": i == 1, "last": i == len(lens) - 1, "none": False}[pattern]
        line = bytearray(rng.choice(b"xyw ") for _ in range(n))
        if pick and n:
            line[rng.randrange(n)] = mark
        lines.append(bytes(line))
    return b"\n".join(lines) + (b"\n" if final_delim else b"")


@pytest.mark.parametrize("pats,mark", [([rb"K"], ord("K")), ([rb"^[^Z]*$"], ord("Z"))])
def test_alignment_and_lengths(gpu, pats, mark):
    """K: a line is selected when it holds a K (the empty line never is); ^[^Z]*$: when it holds no Z (the empty line
    always is)"""
    rng = random.Random(31 + mark)
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps)
        sc = S.Scanner(pool, prog, S.HIP_THOMPSON)
        buffers = [(p, marked_buffer(rng, mark, p, k % 2 == 0)) for k, p in enumerate(PATTERNS)]
        offsets = [(s, d) for s in (0, 1, 7, 15) for d in (0, 1, 8, 15)]
        if mark == ord("Z"):
            offsets = [(0, 0), (1, 15), (7, 8), (15, 1)]
        seen = set()
        for src_off, dst_off in offsets:
            for pattern, data in buffers:
                info, _ = run_filter(sc, exp, data, 0x0A, S.HIP_THOMPSON, src_off, dst_off)
                seen.add((pattern, info.nselected))
        nl = len(LENGTHS) + 1
        if mark == ord("K"):
            assert seen == {("every", nl - 1), ("second", nl // 2), ("first", 1), ("last", 1), ("none", 0)}, seen
        else:
            assert seen == {("every", 1), ("second", nl - nl // 2), ("first", nl - 1), ("last", nl - 1), ("none", nl)}, seen


# ------------------------------------------------------------------ 3. every route

PLANTS = [b"ab@ab.ab", b"abaabaabab@", b"1.22.3.4", b"a" + b"ab" * 20 + b"c" + b"q" * 40 + b"@", b"q@q.q", b"10.0.0.255 "]


def random_lines(seed):
    rng = random.Random(seed)
    lines = []
    for k in range(2000):
        n = 5000 if k % 400 == 7 else rng.randrange(0, 301)
        line = bytes(rng.choice(b"ab@.1c x") for _ in range(n))
        if rng.random() < 0.3:
            p = rng.choice(PLANTS)
            at = rng.randrange(0, max(1, n - len(p)))
            line = line[:at] + p + line[at + len(p):]
        lines.append(line)
    return b"\n".join(lines)            # (no final delimiter)


ROUTES = [
    ("scan-first", HEADLINE, S.HIP_PIKE_FIRST, S.ENGINE_AUTO, S.ENGINE_SCAN, 1),
    ("scan-count", HEADLINE, S.HIP_PIKE_COUNT, S.ENGINE_AUTO, S.ENGINE_SCAN, 1),
    ("scan-thompson", HEADLINE, S.HIP_THOMPSON, S.ENGINE_AUTO, S.ENGINE_SCAN, 1),
    ("nfa-thompson", COUNTED, S.HIP_THOMPSON, S.ENGINE_NFA, S.ENGINE_NFA, 1),
    ("nfa-first", COUNTED, S.HIP_PIKE_FIRST, S.ENGINE_NFA, S.ENGINE_NFA, 1),
    ("nfa-thompson-dotted", DOTTED, S.HIP_THOMPSON, S.ENGINE_NFA, S.ENGINE_NFA, 1),
    ("nfa-first-dotted", DOTTED, S.HIP_PIKE_FIRST, S.ENGINE_NFA, S.ENGINE_NFA, 1),
    ("nfa-count-host", COUNTED, S.HIP_PIKE_COUNT, S.ENGINE_NFA, S.ENGINE_NFA, 0),
    ("vm-first", HEADLINE, S.HIP_PIKE_FIRST, S.ENGINE_VM, S.ENGINE_VM, 0),
    ("nfa-wide-thompson", WIDE[1][0], S.HIP_THOMPSON, S.ENGINE_NFA, S.ENGINE_NFA, 1),
    ("nfa-wide-first", WIDE[1][0], S.HIP_PIKE_FIRST, S.ENGINE_NFA, S.ENGINE_NFA, 1),
]


@pytest.mark.parametrize("name,pats,mode,engine,routed,device", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route(gpu, name, pats, mode, engine, routed, device):
    data = random_lines(5)
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps, key=("filter", tuple(pats)))
        sc = S.Scanner(pool, prog, mode, engine)
        assert sc.engine == routed
        if name.startswith("nfa-wide"):
            assert sc.nfa_bits == WIDE[1][1]
        src = upload_at(data, 3)
        try:
            nl, nr, rows = sc.scan_lines(src.ptr + 3, len(data), cap=2001)
            assert sc.last_lines_device == device
            sel = expected(exp, data, 0x0A, mode)
            # the index rows are [line, start, len] of the scan_lines rows (checked against the oracle in run_filter)
            assert [tuple(r[:3]) for r in rows] == sel and nr == len(sel)
        finally:
            src.free()
        assert 0 < len(sel) < nl == 2000, (len(sel), nl)
        for invert in (False, True):
            run_filter(sc, exp, data, 0x0A, mode, 3, 5, invert=invert)
            assert sc.last_lines_device == device
            assert sc.last_line_batches >= 1


# ------------------------------------------------------------------ 4. flags

def small_buffer(seed, nlines=120, final_delim=False):
    rng = random.Random(seed)
    words = [b"ab@ab.ab", b"x", b"", b"  ", b"q@q.q tail", b"nothing here", b"a@b", b"@", b"zz@zz.zz" * 9]
    lines = [b" ".join(rng.choice(words) for _ in range(rng.randrange(0, 6))) for _ in range(nlines)]
    return b"\n".join(lines) + (b"\n" if final_delim else b"")


def test_flags(gpu):
    with S.Pool() as pool:
        re = S.parse(pool, HEADLINE)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps, key=("filter", tuple(HEADLINE)))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for final in (False, True):
            data = small_buffer(9, final_delim=final)
            lines = split_lines(data, 0x0A)
            ia, a = run_filter(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST)
            ib, b = run_filter(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, invert=True)
            # the two outputs are a partition of the lines: interleaved by the verdicts they give the buffer back
            assert ia.nselected + ib.nselected == len(lines) and ia.nselected and ib.nselected
            la, lb, back = a.split(b"\n")[:-1], b.split(b"\n")[:-1], []
            for st, n in lines:
                hit = exp.record(data[st:st + n], S.HIP_PIKE_FIRST)[0] != S.SRE_DECLINED
                back.append((la if hit else lb).pop(0))
            assert not la and not lb
            assert b"\n".join(back) + b"\n" == (data if final else data + b"\n")
            # every line, and the final delimiter when it was missing
            iall, c = run_filter(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, all_lines=True)
            assert c == (data if final else data + b"\n") and iall.nselected == iall.nlines == len(lines)
        # ALL | INVERT and unknown bits
        src = upload_at(data, 0)
        out = Out(gpu, 4096, 0)
        try:
            info = (ctypes.c_size_t * 5)()
            for flags in (S.HIP_LINES_ALL | S.HIP_LINES_INVERT, 4, 8 | S.HIP_LINES_ALL, -1):
                assert gpu.sre_hip_filter_lines(sc.h, src.ptr, len(data), 0x0A, flags, out.ptr, 4096, None, 0, info, None) == -1
            with pytest.raises(RuntimeError):
                sc.filter_lines(src.ptr, len(data), out.ptr, 4096, invert=True, all_lines=True)
            out.check(b"")
        finally:
            src.free()
            out.free()


# ------------------------------------------------------------------ 5. truncation

def test_truncation(gpu):
    with S.Pool() as pool:
        re = S.parse(pool, HEADLINE)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps, key=("filter", tuple(HEADLINE)))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        data = small_buffer(10)
        sel = expected(exp, data, 0x0A, S.HIP_PIKE_FIRST)
        need = sum(n + 1 for _, _, n in sel)
        first = sel[0][2]
        assert len(sel) > 8 and first > 0
        for dst_off in (0, 5):
            for cap, nwritten in [(need, len(sel)), (need - 1, len(sel) - 1), (first, 0), (first + 1, 1), (need // 2, None)]:
                info, _ = run_filter(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, 1, dst_off, out_cap=cap)
                assert info.need_bytes == need and info.nselected == len(sel)
                assert nwritten is None or info.nwritten == nwritten
                assert info.out_bytes <= cap
        # a sizing call: no output buffer at all
        info, _ = run_filter(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, out_cap=0, null_out=True, index_cap=0)
        assert info == S.FilterInfo(len(split_lines(data, 0x0A)), len(sel), need, 0, 0)
        # fewer index rows than written lines, and no index at all
        for icap in (0, 1, 5, len(sel) - 1):
            info, _ = run_filter(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, index_cap=icap)
            assert info.nwritten == len(sel)
        info, _ = run_filter(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, out_cap=need // 2, index_cap=3)
        assert 3 < info.nwritten < len(sel)


# ------------------------------------------------------------------ 6. several batches

@pytest.mark.parametrize("engine,mode", [(S.ENGINE_AUTO, S.HIP_PIKE_FIRST), (S.ENGINE_NFA, S.HIP_THOMPSON),
                                         (S.ENGINE_NFA, S.HIP_PIKE_COUNT)])
def test_several_batches(gpu, monkeypatch, engine, mode):
    with S.Pool() as pool:
        re = S.parse(pool, HEADLINE)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps, key=("filter", tuple(HEADLINE)))
        sc = S.Scanner(pool, prog, mode, engine)
        data = small_buffer(12, nlines=100)
        assert len(split_lines(data, 0x0A)) == 100
        _, one = run_filter(sc, exp, data, 0x0A, mode, 2, 9)
        assert sc.last_line_batches == 1
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "7")
        for invert in (False, True):
            _, many = run_filter(sc, exp, data, 0x0A, mode, 2, 9, invert=invert)
            assert sc.last_line_batches == 15
            assert invert or many == one


# ------------------------------------------------------------------ 7. idempotence and coexistence

def test_filtering_the_output_again_reproduces_it(gpu):
    with S.Pool() as pool:
        for pats, mode, engine in [(HEADLINE, S.HIP_PIKE_FIRST, S.ENGINE_AUTO), (COUNTED, S.HIP_THOMPSON, S.ENGINE_NFA)]:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            exp = Expect(prog, re.ncaps, key=("filter", tuple(pats)))
            sc = S.Scanner(pool, prog, mode, engine)
            data = random_lines(6)[:60000]
            info, once = run_filter(sc, exp, data, 0x0A, mode, 7, 1)
            assert 0 < info.nselected < info.nlines
            info2, twice = run_filter(sc, exp, once, 0x0A, mode, 1, 7)
            assert twice == once and info2.nlines == info2.nselected == info.nselected
            assert info2.need_bytes == info.need_bytes == len(once)


def test_scan_lines_and_scan_are_unchanged_by_a_filter_call(gpu):
    with S.Pool() as pool:
        for pats, mode, engine in [(HEADLINE, S.HIP_PIKE_FIRST, S.ENGINE_AUTO), (COUNTED, S.HIP_PIKE_FIRST, S.ENGINE_NFA),
                                   (COUNTED, S.HIP_PIKE_COUNT, S.ENGINE_NFA)]:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            sc = S.Scanner(pool, prog, mode, engine)
            data = random_lines(7)[:40000]
            lines = split_lines(data, 0x0A)
            src = upload_at(data, 5)
            out = Out(gpu, len(data) + len(lines) + 1, 3)
            try:
                base = src.ptr + 5
                before = sc.scan_lines(base, len(data), cap=len(lines) + 1)
                diag = (sc.last_lines_device, sc.last_line_batches, sc.last_short_lines, sc.last_fixups)
                batched = sc.scan([base + st for st, _ in lines], [n for _, n in lines])
                info = sc.filter_lines(base, len(data), out.ptr, out.cap)
                assert info.nselected == before[1]
                assert (sc.last_lines_device, sc.last_line_batches, sc.last_short_lines, sc.last_fixups) == diag
                with pytest.raises(RuntimeError):
                    sc.results()            # the filter call replaced the scanner's last call, as scan_lines does
                assert sc.scan_lines(base, len(data), cap=len(lines) + 1) == before
                sc.filter_lines(base, len(data), out.ptr, out.cap, invert=True)
                assert sc.scan([base + st for st, _ in lines], [n for _, n in lines]) == batched
                assert sc.scan_lines(base, len(data), all_lines=True, cap=len(lines) + 1)[1] == len(lines)
            finally:
                src.free()
                out.free()
