"""Line mode (sre_hip_scan_lines): one device buffer, every line its own stream.

Expected rows come from a pure-Python split rule (the rules of grep and wc -l) and the oracle run
on each line; where stated the rows are also compared with sre_hip_scan_batch on the same
(pointer, length) pairs.
"""
import ctypes
import random

import pytest

import sregex_amd as S
import harness

pytestmark = pytest.mark.gpu

# sre_hip_lines.h SRE_LINES_TILE_BYTES: workgroup w of the split owns the 64 KiB tile that starts
# at buffer offset w * TILE - (d_buf % 16); a wave covers 1 KiB of it per step, the workgroup 4 KiB
TILE = 65536
WAVE_STEP = 1024
WG_STEP = 4096


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def split_lines(data, delim):
    """(start, length) of every line: maximal runs between delimiters, no empty line behind a
    final delimiter, a final line without one."""
    out, start, d = [], 0, bytes([delim])
    while start < len(data):
        e = data.find(d, start)
        if e < 0:
            out.append((start, len(data) - start))
            break
        out.append((start, e - start))
        start = e + 1
    return out


def expect_records(ora, prog, ncaps, line):
    """{mode: record} the batched API returns for one stream, from the oracle's find-all."""
    nov = 2 * (ncaps + 1)
    allm = harness.findall(ora, prog, ncaps, line)
    final, matches = allm[-1][0], allm[:-1]
    if matches:
        first = [matches[0][0], 1] + matches[0][1:]
        cnt = [S.SRE_ERROR if final == S.SRE_ERROR else matches[-1][0], len(matches)] + matches[-1][1:]
        th = [0, 1] + [-1] * nov
    else:
        first = [S.SRE_DECLINED, 0] + [-1] * nov
        cnt = [final, 0] + [-1] * nov
        th = [S.SRE_DECLINED, 0] + [-1] * nov
    return {S.HIP_PIKE_FIRST: first, S.HIP_PIKE_COUNT: cnt, S.HIP_THOMPSON: th}


_CACHES = {}


class Expect:
    """oracle rows of a buffer, cached by line content (and across tests by the patterns)"""

    def __init__(self, prog, ncaps, key=None):
        self.ora = harness.OracleEngine()
        self.prog, self.ncaps = prog, ncaps
        self.cache = _CACHES.setdefault(key, {}) if key is not None else {}

    def record(self, line, mode):
        if line not in self.cache:
            self.cache[line] = expect_records(self.ora, self.prog, self.ncaps, line)
        return self.cache[line][mode]

    def rows(self, data, delim, mode, all_lines):
        out = []
        for i, (st, n) in enumerate(split_lines(data, delim)):
            rec = self.record(data[st:st + n], mode)
            if all_lines or rec[0] != S.SRE_DECLINED:
                out.append([i, st, n] + rec)
        return out


def batched_rows(sc, base, data, delim, all_lines):
    """the same lines through sre_hip_scan_batch"""
    lines = split_lines(data, delim)
    if not lines:
        return []
    recs = sc.scan([base + st for st, _ in lines], [n for _, n in lines])
    return [[i, st, n] + r for i, ((st, n), r) in enumerate(zip(lines, recs))
            if all_lines or r[0] != S.SRE_DECLINED]


def upload_at(data, offset):
    """a device buffer holding data at `offset` bytes past an aligned base"""
    buf = S.DeviceBuffer(max(len(data) + offset, 1))
    if data and buf.lib.sre_hip_upload(buf.ptr + offset, bytes(data), len(data)) != 0:
        raise RuntimeError("upload failed")
    return buf


def check(sc, exp, data, delim, mode, all_lines, offset=0, batched=True):
    buf = upload_at(data, offset)
    try:
        nl, nr, rows = sc.scan_lines(buf.ptr + offset, len(data), delim, all_lines,
                                     cap=len(split_lines(data, delim)) + 1)
        want = exp.rows(data, delim, mode, all_lines)
        assert nl == len(split_lines(data, delim))
        assert nr == len(want), (nr, len(want))
        assert rows == want, [(g, w) for g, w in zip(rows, want) if g != w][:3]
        if batched:
            assert rows == batched_rows(sc, buf.ptr + offset, data, delim, all_lines)
    finally:
        buf.free()
    return rows


# ------------------------------------------------------------------ 1. the split

def test_split_edge_cases(gpu):
    with S.Pool() as pool:
        re = S.parse(pool, [rb"^(\w+)", rb"(\w)$", rb"(a)b"])
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps)
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        assert sc.engine == S.ENGINE_SCAN
        for data in [b"", b"\n", b"a", b"a\n", b"\n\n", b"a\n\nb", b"\r\n\r", b"ab\rab\n\nxab"]:
            check(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, True)
        # one 10 MiB line, the match at its end
        big = b"xyz" * (10 * 1024 * 1024 // 3) + b"ab"
        rows = check(sc, exp, big, 0x0A, S.HIP_PIKE_FIRST, True, batched=False)
        assert len(rows) == 1 and rows[0][:3] == [0, 0, len(big)]
        # other delimiters: lines that hold newlines, so ^ and $ inside a line decide
        rng = random.Random(11)
        for delim in (0x00, 0xFF, ord("a"), 0x0A):
            words = [b"ab", b"b\n", b"\nc", b"dd", b"\x00", b"\xff", b" ", b"a", b"\n"]
            data = b"".join(rng.choice(words) for _ in range(3000))
            check(sc, exp, data, delim, S.HIP_PIKE_FIRST, True)
            check(sc, exp, data, delim, S.HIP_PIKE_FIRST, False)


def test_split_alignment_and_tile_boundaries(gpu):
    """d_buf at every offset 0..15 from an aligned base; delimiters at tile, workgroup-step and
    wave-step boundaries and one byte either side of them; buffers that end on and next to a
    tile boundary."""
    rng = random.Random(3)
    with S.Pool() as pool:
        re = S.parse(pool, [rb"(a)b", rb"x$"])
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps)
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        base = bytearray(rng.choice(b"xyab ") for _ in range(3 * TILE + 777))
        for off in range(16):
            data = bytearray(base)
            marks = set()
            for t in range(1, 4):
                marks.add(t * TILE - off)
            for j in range(1, 3 * TILE // WG_STEP, 5):
                marks.add(j * WG_STEP - off)
            for j in range(1, 40, 3):
                marks.add(j * WAVE_STEP - off)
            for p in sorted(marks):
                for q in (p - 1, p, p + 1):
                    if 0 <= q < len(data) and rng.random() < 0.7:
                        data[q] = 0x0A
            data = bytes(data)
            check(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, True, offset=off)
            # ends exactly on a tile boundary, one short of it, one past it; with and without a final delimiter
            for end in (TILE - off, TILE - off - 1, TILE - off + 1, 2 * TILE - off):
                piece = data[:end]
                check(sc, exp, piece, 0x0A, S.HIP_PIKE_FIRST, True, offset=off, batched=False)
                check(sc, exp, piece[:-1] + b"\n", 0x0A, S.HIP_PIKE_FIRST, True, offset=off, batched=False)


# ------------------------------------------------------------------ 2. random text

WORDS = [b"GET ", b"/index.html ", b"user ", b"a@abc.cc ", b"x@y.zz ", b"nobody ", b"@@ ", b"q@w ",
         b"[abc] ", b"\"quoted ", b"text\" ", b"42 ", b"7", b"\r", b"ab", b"word ", b"\t", b"zz@qq.rr"]


def random_text(seed, nlines=20000, nlong=8, long_bytes=(64 << 10, 1 << 20)):
    rng = random.Random(seed)
    lines = []
    for _ in range(nlines):
        n = rng.randrange(0, 300)
        s = b""
        while len(s) < n:
            s += rng.choice(WORDS)
        lines.append(s[:n])
    for i in range(nlong):
        n = long_bytes[1] if i == 0 else rng.randrange(long_bytes[0], long_bytes[1] // 4)
        # a long line of words; half of them open a quote at the start that closes only at the end
        body = b"".join(rng.choice(WORDS[:12]) for _ in range(n // 6)).replace(b"\"", b"'")
        body = b"\"" + body[:n - 20] + b"\" tail@end.cc" if i % 2 else body[:n]
        lines.insert(rng.randrange(len(lines)), body)
    return b"\n".join(lines) + b"\n"


TEXT_PROGRAMS = [
    ([rb"([a-z]+)@([a-z]+)\.[a-z]+"], (S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT, S.HIP_THOMPSON)),
    ([rb"([a-z]+)@([a-z]+)\.[a-z]+", rb"\[(\w+)\]"], (S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT)),
    ([rb"\bab\w*\b"], (S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT, S.HIP_THOMPSON)),
    ([rb"(\d+)$", rb"^GET (\S+)"], (S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT)),
    ([rb"[a-z]+"], (S.HIP_PIKE_COUNT,)),
    ([rb"\"([^\"]*)\""], (S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT, S.HIP_THOMPSON)),
]


@pytest.mark.parametrize("seg", [256, 0])
def test_random_text_vs_oracle_and_batched(gpu, seg):
    data = random_text(7)
    buf = S.DeviceBuffer.from_bytes(data)
    fixups = lineage = exact = 0
    on_scanner = []
    try:
        for pats, modes in TEXT_PROGRAMS:
            with S.Pool() as pool:
                re = S.parse(pool, pats)
                prog = S.compile(pool, re)
                exp = Expect(prog, re.ncaps, key=tuple(pats))
                for mode in modes:
                    sc = S.Scanner(pool, prog, mode)
                    if sc.engine != S.ENGINE_SCAN:
                        continue        # (the exact VM over megabyte lines: test_engines_agree covers the fallbacks)
                    on_scanner.append((pats, mode))
                    if seg:
                        sc.set_segment_bytes(seg)
                    for all_lines in (True, False):
                        nl, nr, rows = sc.scan_lines(buf.ptr, len(data), all_lines=all_lines, cap=20008)
                        fixups += sc.last_fixups
                        lineage += sc.last_lineage_passes
                        exact += sc.last_exact_passes
                        assert sc.last_line_batches == 1
                        assert sc.last_kernel_ms > 0
                        want = exp.rows(data, 0x0A, mode, all_lines)
                        assert nl == 20008 and nr == len(want)
                        bad = [(g, w) for g, w in zip(rows, want) if g != w]
                        assert rows == want, (pats, mode, all_lines, len(bad), bad[:2])
                        assert rows == batched_rows(sc, buf.ptr, data, 0x0A, all_lines), (pats, mode)
    finally:
        buf.free()
    assert len(on_scanner) >= 10, on_scanner
    if seg == 256:
        # long lines span many segments: fix-up rounds, exact entry states and lineage maps ran inside line mode
        assert fixups > 0 and exact > 0 and lineage > 0, (fixups, exact, lineage)


# ------------------------------------------------------------------ 3. engines agree

def test_engines_agree(gpu):
    from test_gpu_parity import NFA_ZOO
    rng = random.Random(17)
    alpha = b"abcxy@,. \r\nAB"
    lines = [bytes(rng.choice(alpha[:-3]) for _ in range(rng.randrange(0, 200))) for _ in range(1000)]
    data = b"\n".join(lines)
    buf = S.DeviceBuffer.from_bytes(data)
    ran = 0
    try:
        for pats in NFA_ZOO:
            with S.Pool() as pool:
                prog = S.compile(pool, S.parse(pool, pats))
                for mode in (S.HIP_PIKE_FIRST, S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                    try:
                        nfa = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
                    except RuntimeError:
                        continue
                    outs = []
                    for sc in (nfa, S.Scanner(pool, prog, mode, S.ENGINE_VM), S.Scanner(pool, prog, mode, S.ENGINE_AUTO)):
                        outs.append(sc.scan_lines(buf.ptr, len(data), all_lines=True, cap=1001))
                        assert sc.last_line_batches == 1
                    assert outs[0] == outs[1] == outs[2], (pats, mode)
                    ran += 1
    finally:
        buf.free()
    assert ran >= 10, ran


# ------------------------------------------------------------------ 4. batches

def test_forced_small_batches(gpu, monkeypatch):
    data = random_text(9, nlines=6000, nlong=2, long_bytes=(16 << 10, 128 << 10))
    buf = S.DeviceBuffer.from_bytes(data)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [rb"([a-z]+)@([a-z]+)\.[a-z]+", rb"\"([^\"]*)\""]))
            for mode in (S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT):
                for engine in (S.ENGINE_AUTO, S.ENGINE_VM):
                    sc = S.Scanner(pool, prog, mode, engine)
                    monkeypatch.delenv("SRE_HIP_LINES_BATCH", raising=False)
                    ref = sc.scan_lines(buf.ptr, len(data), all_lines=True, cap=6003)
                    assert sc.last_line_batches == 1
                    monkeypatch.setenv("SRE_HIP_LINES_BATCH", "1000")
                    for all_lines in (True, False):
                        got = sc.scan_lines(buf.ptr, len(data), all_lines=all_lines, cap=6003)
                        assert sc.last_line_batches == 7, sc.last_line_batches
                        want_rows = [r for r in ref[2] if all_lines or r[3] != S.SRE_DECLINED]
                        assert got == (ref[0], len(want_rows), want_rows), (mode, engine, all_lines)
                    monkeypatch.delenv("SRE_HIP_LINES_BATCH")
    finally:
        buf.free()


def test_64_mi_empty_lines(gpu):
    n = 64 << 20
    buf = S.DeviceBuffer(n)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [rb"a"]))
            block = b"\n" * (1 << 20)
            for o in range(0, n, len(block)):
                assert gpu.sre_hip_upload(buf.ptr + o, block, len(block)) == 0
            sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
            nl, nr = ctypes.c_size_t(), ctypes.c_size_t()
            assert gpu.sre_hip_scan_lines(sc.h, buf.ptr, n, 0x0A, 0, None, 0, ctypes.byref(nl), ctypes.byref(nr), None) == 0
            assert (nl.value, nr.value) == (n, 0)
            assert gpu.sre_hip_scan_lines(sc.h, buf.ptr, n, 0x0A, S.HIP_LINES_ALL, None, 0, ctypes.byref(nl),
                                          ctypes.byref(nr), None) == 0
            assert (nl.value, nr.value) == (n, n)
            assert sc.last_line_batches >= n // (1 << 20)
    finally:
        buf.free()


# ------------------------------------------------------------------ 5. cap

def test_cap(gpu):
    data = random_text(13, nlines=5000, nlong=0)
    cap = 5001
    buf = S.DeviceBuffer.from_bytes(data)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [rb"([a-z]+)@([a-z]+)\.[a-z]+"]))
            for engine in (S.ENGINE_AUTO, S.ENGINE_VM):
                sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST, engine)
                nl, nr, rows = sc.scan_lines(buf.ptr, len(data), cap=cap)
                assert 0 < nr < nl and len(rows) == nr
                for c in (1, 7, nr - 1):
                    assert sc.scan_lines(buf.ptr, len(data), cap=c) == (nl, nr, rows[:c])
                n1, n2 = ctypes.c_size_t(), ctypes.c_size_t()
                assert gpu.sre_hip_scan_lines(sc.h, buf.ptr, len(data), 0x0A, 0, None, 0, ctypes.byref(n1),
                                              ctypes.byref(n2), None) == 0
                assert (n1.value, n2.value) == (nl, nr)
                # bad arguments
                assert gpu.sre_hip_scan_lines(sc.h, buf.ptr, len(data), 256, 0, None, 0, None, None, None) == -1
                assert gpu.sre_hip_scan_lines(sc.h, buf.ptr, len(data), 0x0A, 2, None, 0, None, None, None) == -1
                assert gpu.sre_hip_scan_lines(sc.h, buf.ptr, len(data), 0x0A, 0, None, 5, None, None, None) == -1
    finally:
        buf.free()


# ------------------------------------------------------------------ 6. beyond 4 GiB

def test_beyond_4_gib(gpu):
    block_bytes, line_bytes, nblocks = 64 << 20, 4096, 96
    rng = random.Random(23)
    line = bytes(rng.choice(b"abcdefgh x") for _ in range(line_bytes - 1)) + b"\n"
    block = line * (block_bytes // line_bytes)
    last_line = line[:1000] + b"needle(1234)" + line[1012:]
    last_block = block[:-line_bytes] + last_line
    n = block_bytes * nblocks
    buf = S.DeviceBuffer(n)
    try:
        for b in range(nblocks):
            src = last_block if b == nblocks - 1 else block
            assert gpu.sre_hip_upload(buf.ptr + b * block_bytes, src, block_bytes) == 0
        nlines = nblocks * (block_bytes // line_bytes)
        with S.Pool() as pool:
            re = S.parse(pool, [rb"needle\((\d+)\)"])
            prog = S.compile(pool, re)
            sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
            nl, nr, rows = sc.scan_lines(buf.ptr, n, cap=4)
            assert (nl, nr) == (nlines, 1)
            start = n - line_bytes
            assert start > (1 << 32)
            want = expect_records(harness.OracleEngine(), prog, re.ncaps, last_line[:-1])[S.HIP_PIKE_FIRST]
            assert rows == [[nlines - 1, start, line_bytes - 1] + want], rows
            assert sc.last_line_batches > 1
            every = S.compile(pool, S.parse(pool, [rb"[a-h]+"]))
            sc = S.Scanner(pool, every, S.HIP_PIKE_COUNT)
            assert sc.scan_lines(buf.ptr, n, cap=0) == (nlines, nlines, [])
    finally:
        buf.free()


# ------------------------------------------------------------------ 7. mixed calls

def test_mixed_calls_on_one_scanner(gpu):
    data = random_text(29, nlines=3000, nlong=1)
    lines = split_lines(data, 0x0A)
    buf = S.DeviceBuffer.from_bytes(data)
    try:
        with S.Pool() as pool:
            re = S.parse(pool, [rb"([a-z]+)@([a-z]+)\.[a-z]+"])
            prog = S.compile(pool, re)
            exp = Expect(prog, re.ncaps)
            for mode in (S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT, S.HIP_THOMPSON):
                sc = S.Scanner(pool, prog, mode)
                want = [exp.record(data[st:st + k], mode) for st, k in lines]
                assert sc.scan([buf.ptr + st for st, _ in lines], [k for _, k in lines]) == want
                nl, nr, rows = sc.scan_lines(buf.ptr, len(data), all_lines=True, cap=len(lines) + 1)
                assert (nl, nr) == (len(lines), len(lines))
                assert rows == [[i, st, k] + w for i, ((st, k), w) in enumerate(zip(lines, want))]
                out = (ctypes.c_ssize_t * sc.slots)()
                assert gpu.sre_hip_scan_results(sc.h, out) == -1
                half = lines[: len(lines) // 2]
                assert sc.scan([buf.ptr + st for st, _ in half], [k for _, k in half]) == want[: len(half)]
    finally:
        buf.free()
