"""Line mode on the bit-parallel NFA tier (sre_hip_scan_lines with a Thompson or first-match scanner of the tier):
every batch on the device — short lines one to a lane through sre_k_lines_nfa, the longer ones through the tier's
set pass, chain check and fix-up rounds — against the per-line oracle and sre_hip_scan_batch on the same
(pointer, length) pairs.
"""
import ctypes
import random
import statistics
import time

import pytest

import sregex_amd as S
import harness
from test_gpu_lines import Expect, check, split_lines, upload_at
from test_gpu_parity import NFA_ZOO
from test_gpu_nfa_wide import WIDE

pytestmark = pytest.mark.gpu

MODES = (S.HIP_THOMPSON, S.HIP_PIKE_FIRST)
COUNTED = [rb"(?:a|b)*a(?:a|b){7}@"]
NEVER_FORGETS = [rb"x[^y]*y(?:a|b){20}@"]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def scan_lines_checked(sc, exp, data, delim, mode, all_lines, cap=None):
    """scan_lines on a fresh upload; the rows against the oracle's"""
    buf = upload_at(data, 0)
    try:
        want = exp.rows(data, delim, mode, all_lines)
        got = sc.scan_lines(buf.ptr, len(data), delim, all_lines, cap=len(want) + 1 if cap is None else cap)
        assert got[0] == len(split_lines(data, delim)) and got[1] == len(want), (got[:2], len(want))
        assert got[2] == (want if cap is None else want[:cap]), [(g, w) for g, w in zip(got[2], want) if g != w][:3]
        return got
    finally:
        buf.free()


# ------------------------------------------------------------------ 1. the route

def test_route(gpu, monkeypatch):
    rng = random.Random(5)
    lines = [bytes(rng.choice(b"ab@ ") for _ in range(rng.randrange(0, 120))) for _ in range(300)]
    lines[17] = b"bb" + b"ab" * 6 + b"@b"
    data = b"\n".join(lines) + b"\n"
    with S.Pool() as pool:
        re = S.parse(pool, COUNTED)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps)
        for mode in MODES:
            sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
            assert sc.last_lines_device == 0            # before the first call
            monkeypatch.delenv("SRE_HIP_LINES_NFA_HOST", raising=False)
            dev = scan_lines_checked(sc, exp, data, 0x0A, mode, True)
            assert sc.last_lines_device == 1 and sc.last_short_lines == 300
            assert sc.last_kernel_ms > 0 and sc.last_line_batches == 1
            monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
            host = scan_lines_checked(sc, exp, data, 0x0A, mode, True)
            assert sc.last_lines_device == 0 and sc.last_short_lines == 0
            assert host == dev
            monkeypatch.delenv("SRE_HIP_LINES_NFA_HOST")
        # find-all counting on the tier and the exact VM keep the host route; the table-driven scanner is on the device
        for mode, engine, device in [(S.HIP_PIKE_COUNT, S.ENGINE_NFA, 0), (S.HIP_PIKE_FIRST, S.ENGINE_VM, 0),
                                     (S.HIP_THOMPSON, S.ENGINE_VM, 0)]:
            sc = S.Scanner(pool, prog, mode, engine)
            assert sc.engine == engine
            scan_lines_checked(sc, exp, data, 0x0A, mode, True)
            assert sc.last_lines_device == device and sc.last_short_lines == 0
        small = S.compile(pool, S.parse(pool, [rb"a@"]))
        sc = S.Scanner(pool, small, S.HIP_PIKE_FIRST)
        assert sc.engine == S.ENGINE_SCAN
        scan_lines_checked(sc, Expect(small, 0), data, 0x0A, S.HIP_PIKE_FIRST, False)
        assert sc.last_lines_device == 1 and sc.last_short_lines == 0


# ------------------------------------------------------------------ 2. the short-line kernel: shapes

SHAPE_PROGRAMS = [[rb"(?:a|b)*a(?:a|b){7}@"], [rb"[ab]{3,9}c{2}(x)?"], [rb"(a+)(b+)?"], [rb"a[^x]{20}x"], [rb"(\w+ ){3}(\w+)"], [rb"c$"], [rb"\bab\b"], [rb"^(.*)$"],
                  [rb"^a.{3}b", rb"\nc{2,4}"],
                  [b"a", b"ab", b"c", b"a(bc)", b"e(f)", b"gh", b"A", b"b", b"BLAH", rb"\s+", b"abcd", b"bc"]]
SHORT_LENGTHS = [0, 1, 15, 16, 17, 63, 64]      # at most SRE_HIP_LINES_SHORT_MAX=64: the short-line kernel
LONG_LENGTH = 65                                # the set pass
TAILS = [b"abaabaabab@", b"a" + b"q" * 20 + b"x", b"aa bb cc dd", b"abc", b" ab", b"ab", b"a...b", b"cc", b"BLAH ", b"e", b"abbbccx"]


def shape_of(kernel_name):
    """(shift-and, look-ahead, events from the consumed set) of a 64-bit kernel, from its name"""
    args = [a.strip() for a in kernel_name[kernel_name.index("<") + 1:-1].split(",")]
    if kernel_name.startswith("sre_k_nfa_sa<"):
        return (True, args[5] == "true", args[3] == "true")
    assert kernel_name.startswith("sre_k_nfa<"), kernel_name
    return (False, args[2] == "true", False)


def shape_buffer(rng, nlines, delim, final_delim):
    """nlines lines whose lengths walk SHORT_LENGTHS + [LONG_LENGTH]; bytes other than the delimiter, newlines among
    them when it is not the delimiter; some lines end in text the programs match"""
    alpha = bytes(b for b in b"abcx @.\nqe" if b != delim)
    lens = SHORT_LENGTHS + [LONG_LENGTH]
    lines = []
    for i in range(nlines):
        n = lens[(i + i // len(lens)) % len(lens)]
        body = bytes(rng.choice(alpha) for _ in range(n))
        t = rng.choice(TAILS)
        if rng.random() < 0.4 and len(t) <= n and delim not in t:
            body = body[:n - len(t)] + t
        lines.append(body)
    d = bytes([delim])
    return d.join(lines) + (d if final_delim else b""), lines


@pytest.mark.parametrize("sa", [0, 128])        # sre_nfa.h: 128 = the plain slices only
def test_short_line_kernel_shapes(gpu, monkeypatch, sa):
    assert all(p in NFA_ZOO for p in SHAPE_PROGRAMS)
    monkeypatch.setenv("SRE_HIP_NFA_SA", str(sa))
    monkeypatch.setenv("SRE_HIP_LINES_SHORT_MAX", "64")
    rng = random.Random(41 + sa)
    shapes = set()
    # (line count, offset past an aligned base, delimiter, final delimiter, every line reported)
    cases = []
    for k, nlines in enumerate([1, 63, 64, 65, 256, 257]):
        for j, off in enumerate([0, 1, 15]):
            cases.append((nlines, off, 0x0A if (k + j) % 3 else ord(";"), (k + j) % 2 == 0, (k + j) % 4 < 2))
    buffers = [(c, shape_buffer(rng, c[0], c[2], c[3])) for c in cases]
    for pats in SHAPE_PROGRAMS:
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            exp = Expect(prog, re.ncaps, key=("lines_nfa",) + tuple(pats))
            for mode in MODES:
                sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
                assert sc.nfa_bits == 64
                shapes.add(shape_of(sc.kernel_name))
                for (nlines, off, delim, final_delim, all_lines), (data, lines) in buffers:
                    check(sc, exp, data, delim, mode, all_lines, offset=off)
                    assert sc.last_lines_device == 1
                    # (a final empty line without a delimiter is no line)
                    counted = split_lines(data, delim)
                    assert sc.last_short_lines == sum(1 for _, n in counted if n <= 64), (pats, nlines, off)
                # delimiters only; the empty buffer
                for data in (b"\n" * 300, b"\n", b""):
                    check(sc, exp, data, 0x0A, mode, True, offset=1)
                    assert sc.last_short_lines == len(data) and sc.last_lines_device == 1
    if sa == 128:
        assert shapes == {(False, False, False), (False, True, False)}, shapes
    else:
        assert {(True, False, False), (True, True, False), (True, False, True)} <= shapes, shapes


# ------------------------------------------------------------------ 3. mixed batches and fix-up rounds

def mixed_buffer(rng):
    """some hundred short lines and a few 2-20 KiB lines whose `x` comes early with no `y` behind it (a thread that
    never dies: speculation cannot settle them), two of them with a match at the very end.  Lines 0-6 are short,
    7-13 long, 14-20 both, so that batches of 7 lines are of every kind."""
    def short():
        s = bytes(rng.choice(b"abx@ y") for _ in range(rng.randrange(0, 100)))
        return s if rng.random() < 0.8 else s[:40] + b"xqy" + b"ab" * 10 + b"@"
    def long(n, hit):
        body = b"ab x" + bytes(rng.choice(b"ab @q") for _ in range(n))
        return body + (b"y" + b"ba" * 10 + b"@" if hit else b"")
    lines = [short() for _ in range(7)] + [long(2048 + 100 * i, i == 3) for i in range(7)]
    lines += [short(), long(3000, False), short(), short(), long(20 << 10, True), short(), long(2500, False)]
    for i in range(140):
        lines.append(long(rng.randrange(2 << 10, 9 << 10), False) if i % 35 == 20 else short())
    return b"\n".join(lines), lines


@pytest.mark.parametrize("seg", [64, 256])
def test_mixed_batches_and_fixups(gpu, monkeypatch, seg):
    rng = random.Random(77)
    data, lines = mixed_buffer(rng)
    nshort = sum(1 for l in lines if len(l) <= 512)
    assert 0 < nshort < len(lines)
    with S.Pool() as pool:
        re = S.parse(pool, NEVER_FORGETS)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps, key=("lines_nfa_mixed",))
        for mode in MODES:
            sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
            assert sc.nfa_bits == 64
            sc.set_segment_bytes(seg)
            monkeypatch.delenv("SRE_HIP_LINES_BATCH", raising=False)
            for all_lines in (True, False):
                check(sc, exp, data, 0x0A, mode, all_lines, offset=3)
            assert sc.last_lines_device == 1 and sc.last_short_lines == nshort
            ref = scan_lines_checked(sc, exp, data, 0x0A, mode, True)
            assert sc.last_line_batches == 1 and sc.last_segment_bytes == seg
            assert sc.last_fixups > 0 and sc.last_exact_passes > 0, (sc.last_fixups, sc.last_exact_passes)
            assert sum(1 for r in ref[2] if r[3] != S.SRE_DECLINED) >= 3
            monkeypatch.setenv("SRE_HIP_LINES_BATCH", "7")
            for all_lines in (True, False):
                got = scan_lines_checked(sc, exp, data, 0x0A, mode, all_lines)
                assert sc.last_line_batches == (len(lines) + 6) // 7
                assert sc.last_lines_device == 1 and sc.last_short_lines == nshort
                assert sc.last_fixups > 0 and sc.last_exact_passes > 0
                # cap below the number of reported lines
                for cap in (0, 1, got[1] - 1):
                    assert scan_lines_checked(sc, exp, data, 0x0A, mode, all_lines, cap=cap)[:2] == got[:2]
            monkeypatch.delenv("SRE_HIP_LINES_BATCH")
            # the short-line kernel off: every line through the set pass
            monkeypatch.setenv("SRE_HIP_LINES_SHORT_MAX", "0")
            assert scan_lines_checked(sc, exp, data, 0x0A, mode, True) == ref
            assert sc.last_lines_device == 1 and sc.last_short_lines == 0
            monkeypatch.delenv("SRE_HIP_LINES_SHORT_MAX")


# ------------------------------------------------------------------ 4. the wide tier

def test_wide_tier(gpu):
    pats, bits = WIDE[1]
    assert bits == 128
    rng = random.Random(19)
    ab = lambda n: bytes(rng.choice(b"ab") for _ in range(n))
    lines = []
    for i in range(200):
        n = rng.choice([0, 1, 63, 64, 65, 100, 300, 2000])
        lines.append(ab(n) if i % 9 else ab(n) + b"a" + ab(40) + b"c" + b"y" * 40 + b"@" + ab(5))
    data = b"\n".join(lines) + b"\n"
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps, key=("lines_nfa_wide",))
        for mode in MODES:
            sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
            assert sc.nfa_bits == 128
            for all_lines in (True, False):
                rows = check(sc, exp, data, 0x0A, mode, all_lines, offset=5)
                assert sc.last_lines_device == 1 and sc.last_short_lines == 0
            assert len(rows) >= 20


# ------------------------------------------------------------------ 5. mixed calls

def test_mixed_calls_on_one_nfa_scanner(gpu):
    rng = random.Random(29)
    lines = [bytes(rng.choice(b"ab@ ") for _ in range(rng.choice([0, 5, 64, 90, 700]))) for _ in range(500)]
    for i in range(0, 500, 11):
        lines[i] = lines[i] + b"ab" * 5 + b"@"
    data = b"\n".join(lines) + b"\n"
    spans = split_lines(data, 0x0A)
    buf = S.DeviceBuffer.from_bytes(data)
    try:
        with S.Pool() as pool:
            re = S.parse(pool, COUNTED)
            prog = S.compile(pool, re)
            exp = Expect(prog, re.ncaps)
            for mode in MODES:
                sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
                want = [exp.record(data[st:st + k], mode) for st, k in spans]
                for _ in range(2):
                    nl, nr, rows = sc.scan_lines(buf.ptr, len(data), all_lines=True, cap=len(spans) + 1)
                    assert (nl, nr) == (len(spans), len(spans))
                    assert rows == [[i, st, k] + w for i, ((st, k), w) in enumerate(zip(spans, want))]
                    assert sc.last_lines_device == 1
                    out = (ctypes.c_ssize_t * sc.slots)()
                    assert gpu.sre_hip_scan_results(sc.h, out) == -1
                    half = spans[: len(spans) // 2]
                    assert sc.scan([buf.ptr + st for st, _ in half], [k for _, k in half]) == want[: len(half)]
    finally:
        buf.free()


# ------------------------------------------------------------------ 6. rate sanity

def test_device_route_is_not_slower_than_the_host_route(gpu, monkeypatch):
    """2^18 lines of 96 bytes, a match on about 1 % of them.  On the table-driven scanner leaving the per-line host
    loop was worth 4-15x, so a device route that loses to it is broken, not slow: the only timing assertion."""
    nlines, width = 1 << 18, 96
    rng = random.Random(3)
    data = bytearray(rng.randbytes(nlines * width).translate(bytes(97 + (b & 1) for b in range(256))))
    data[width - 1::width] = b"\n" * nlines
    hits = sorted(rng.sample(range(nlines), nlines // 100))
    for i in hits:
        data[i * width + 42] = ord("a")
        data[i * width + 50] = ord("@")
    data = bytes(data)
    buf = S.DeviceBuffer.from_bytes(data)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, COUNTED))
            sc = S.Scanner(pool, prog, S.HIP_THOMPSON, S.ENGINE_NFA)
            times, outs = {"device": [], "host": []}, {}
            for rep in range(6):        # (the first pair warms up)
                for route in ("device", "host"):
                    if route == "host":
                        monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
                    else:
                        monkeypatch.delenv("SRE_HIP_LINES_NFA_HOST", raising=False)
                    t0 = time.perf_counter()
                    outs[route] = sc.scan_lines(buf.ptr, len(data), cap=4096)
                    dt = time.perf_counter() - t0
                    assert sc.last_lines_device == (1 if route == "device" else 0)
                    if rep:
                        times[route].append(dt)
            monkeypatch.delenv("SRE_HIP_LINES_NFA_HOST", raising=False)
            assert outs["device"] == outs["host"]
            assert outs["device"][:2] == (nlines, len(hits)) and [r[0] for r in outs["device"][2]] == hits
            dev, host = statistics.median(times["device"]), statistics.median(times["host"])
            print("lines on the NFA tier, 2^18 x 96 B: device route %.3f ms, host route %.3f ms, ratio %.2f"
                  % (dev * 1e3, host * 1e3, host / dev))
            assert dev <= host, (dev, host)
    finally:
        buf.free()
